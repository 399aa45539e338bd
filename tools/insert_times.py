"""Insert kernel times (ef_map_insert; csrc/ef_insert.inc).

    python tools/insert_times.py               wall clock per call (host clock around a call that synchronises before and after, median of
                                               REPS), the box's copy rate (ef_dev_calibrate), the shapes of every launch ("SHAPE" lines), the
                                               nearest-surfel query at the same n and max_dist (the gate is that walk plus one normal load
                                               and two bytes), and the time of the path an insert replaces (downloadMap + numpy concatenate +
                                               uploadMap + restore) on the same map
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/insert_times.py
                                               the same run under the profiler: its kernel trace has the launches' own durations
    python tools/insert_times.py --summarise DIR/.../*_kernel_trace.csv LOG
                                               medians per kernel and map from that trace, the gate's ratio to k_query<16, 1>, and the scatter's
                                               algorithmic bytes (from the SHAPE lines of the run's output LOG) as a fraction of the box's copy rate

Maps: the steady bench map (140 replay steps of the bench sequence, 640x480) and the configs[2] map (bench.preseed with 1 M surfels, then
three 1280x960 frames).  Records: 100 000 at the default parameters (gate on, 0.01 m, every surfel can suppress, normal cosine 0.5) under a
motion of a few millimetres: half are map surfels moved by 3 mm (duplicates but for those whose nearest neighbour is another surfel with another
normal), half map surfels lifted 5 cm along their normals (new).  After every timed insert the inserted rows are erased again by their creation
time (untimed: k_select_flags / k_select_compact, so that every k_select_count of the trace is an insert's)."""
import csv
import ctypes as C
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from select_times import bench_map, big_map

REPS = 10
NI = 100000
MARK = 999999    # the creation time the timed inserts stamp, and the erase between them selects
KERNELS = ("k_insert_gate", "k_insert_scatter", "k_select_count", "k_query<16, 1>")


def records_for(S, accuracy, T):
    rng = np.random.default_rng(8)
    ok = np.nonzero(np.isfinite(S[:, :3]).all(1))[0]
    pick = rng.choice(ok, NI, replace=len(ok) < NI)
    R = S[pick].copy()
    off = rng.normal(size=(NI // 2, 3))
    R[:NI // 2, :3] += (off / np.linalg.norm(off, axis=1, keepdims=True) * 0.003).astype(np.float32)
    R[NI // 2:, :3] += R[NI // 2:, 8:11] * np.float32(0.05)
    return accuracy.move_surfels(R, np.linalg.inv(T))


def run(api, accuracy, ef, last, label):
    from elasticfusion_amd.api import SEL_INIT_TIME
    S = ef.downloadMap()
    n0 = len(S)
    w = 0.002
    T = np.array([[np.cos(w), -np.sin(w), 0, 0.003], [np.sin(w), np.cos(w), 0, -0.002], [0, 0, 1, 0.001], [0, 0, 0, 1]])
    R = records_for(S, accuracy, T)
    d_rec = api.DevBuf.from_array(R)
    d_new, d_match = api.DevBuf(NI * 4), api.DevBuf(NI * 4)
    prm = ef.insertParams(init_time=MARK)
    keep, pT = api._pose16(T)
    res = api.ef_insert_result()
    undo = ef.mapSelection(tests=SEL_INIT_TIME, init_time_min=MARK, init_time_max=MARK)
    print(f"{label}: {n0} surfels, {NI} records; wall clock per call in us (median of {REPS} after a warm-up)", flush=True)
    t = []
    for rep in range(1 + REPS):
        ef.queryNearestRaw(S[:4, :3], 0.01, -1.0)     # the index of the map as it stands: the insert reuses it, as it would after any query
        t0 = time.perf_counter()
        api._chk(api.lib().ef_map_insert_dev(ef.h, d_rec.p, C.c_uint32(NI), pT, C.byref(prm), C.byref(res), d_new.p, d_match.p), ef.h)
        t.append((time.perf_counter() - t0) * 1e6)
        assert ef.eraseSurfels(undo) == res.inserted and ef.lastCount() == n0
    print(f"  insert {NI} records (index already built) {float(np.median(t[1:])):9.1f}   inserted {res.inserted} duplicates {res.duplicates} "
          f"skipped {res.skipped}", flush=True)
    print("SHAPE " + json.dumps(dict(map=label, op="insert", n0=n0, n=NI, inserted=int(res.inserted), duplicates=int(res.duplicates))), flush=True)
    t = []
    for rep in range(3):
        t0 = time.perf_counter()
        api._chk(api.lib().ef_map_insert_dev(ef.h, d_rec.p, C.c_uint32(NI), pT, C.byref(prm), C.byref(res), d_new.p, d_match.p), ef.h)
        t.append((time.perf_counter() - t0) * 1e6)
        assert ef.eraseSurfels(undo) == res.inserted
    print(f"  insert {NI} records (index stale: rebuilt inside the call) {float(np.median(t)):9.1f}", flush=True)
    # the query at the same n and max_dist, on the same index
    Tf = T.astype(np.float32)
    p = np.stack([((Tf[a, 0] * R[:, 0] + Tf[a, 1] * R[:, 1]) + Tf[a, 2] * R[:, 2]) + Tf[a, 3] for a in range(3)], 1)
    d_p, d_row = api.DevBuf.from_array(np.ascontiguousarray(p, np.float32)), api.DevBuf(NI * 4)
    t = []
    for rep in range(1 + REPS):
        ef.synchronize()
        t0 = time.perf_counter()
        ef.queryNearestDevice(d_p.p, NI, 0.01, -1.0, row=d_row.p)
        ef.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    hits = int((d_row.to_array(np.uint32, NI) != 0xFFFFFFFF).sum())
    print(f"  queryNearest {NI} points at 0.01 m {float(np.median(t[1:])):9.1f}   hits {hits}", flush=True)
    # the path an insert replaces, on the same map: the whole map to the host and back, a full re-preprocess of the last frame
    new = accuracy.move_surfels(R[NI // 2:], T)
    t0 = time.perf_counter()
    m = ef.downloadMap()
    ck = dict(map=np.concatenate([m, new]), tick=ef.getTick(), qt=ef.getPoseQT(), rgb=last[0], depth=last[1])
    ef.restore(ck)
    ef.synchronize()
    legacy = (time.perf_counter() - t0) * 1e6
    print(f"  the replaced path (downloadMap + numpy concatenate + uploadMap + restore), {len(new)} rows added, no gate: {legacy:9.1f} us", flush=True)


def summarise(path, log):
    shapes = [json.loads(ln[6:]) for ln in open(log) if ln.startswith("SHAPE ")]
    copy_rate = None
    for ln in open(log):
        m = re.search(r"copy rate ([0-9.]+) GB/s", ln)
        if m:
            copy_rate = float(m.group(1)) * 1e9
    by = {}
    for r in csv.DictReader(open(path)):
        name = re.sub(r"\s+", " ", r["Kernel_Name"])
        for k in KERNELS:
            if k in name:
                by.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    # per map, in the order of the run: 1 + REPS + 3 inserts (gate, two counts, scatter each; before each of the first 1 + REPS a query of four
    # points that builds the index), then 1 + REPS queries of the records' moved positions: those are the last of the map
    per_map = {"k_insert_gate": 1 + REPS + 3, "k_insert_scatter": 1 + REPS + 3, "k_select_count": 2 * (1 + REPS + 3), "k_query<16, 1>": 2 * (1 + REPS)}
    print(f"copy rate of the box (16 MiB read + 16 MiB written per launch): {copy_rate / 1e9 if copy_rate else float('nan'):.0f} GB/s")
    print("kernel             map               launches  median us")
    med = {}
    for k, c in per_map.items():
        v = [d for _, d in sorted(by.get(k, []))]
        if len(v) != c * len(shapes):
            print(f"{k}: {len(v)} launches in the trace, {c * len(shapes)} expected: not summarised")
            continue
        for i, s in enumerate(shapes):
            d = v[i * c:(i + 1) * c]
            if k.startswith("k_query"):
                d = d[-REPS:]
            med[(k, s["map"])] = float(np.median(d)) / 1e3
            print(f"{k:18s} {s['map']:16s} {c:9d}  {med[(k, s['map'])]:9.1f}")
    for s in shapes:
        g, q, sc = (med.get((k, s["map"])) for k in ("k_insert_gate", "k_query<16, 1>", "k_insert_scatter"))
        if g and q:
            print(f"{s['map']}: k_insert_gate / k_query<16, 1> = {g / q:.2f}")
        if sc and copy_rate:
            b = 96 * s["inserted"] + 5 * s["n"]      # 48 B read + 48 B written per inserted record, a flag byte and a new_row word per record
            rate = b / (sc * 1e-6)
            print(f"{s['map']}: k_insert_scatter moves {b / 1e6:.2f} MB at {rate / 1e9:.0f} GB/s = {rate / copy_rate:.2f} of the copy rate")


if __name__ == "__main__":
    if "--summarise" in sys.argv:
        i = sys.argv.index("--summarise")
        summarise(sys.argv[i + 1], sys.argv[i + 2])
        sys.exit(0)
    import bench
    from elasticfusion_amd import accuracy, api
    e, s = C.c_float(0), C.c_float(0)
    api._chk(api.lib().ef_dev_calibrate(None, C.byref(e), C.byref(s)))
    print(f"ef_dev_calibrate: empty kernel {e.value:.2f} us, 16 MiB copy {s.value:.2f} us per launch: copy rate {2 * 16 * 1048576 / (s.value * 1e-6) / 1e9:.0f} GB/s "
          "(bytes read + bytes written)", flush=True)
    for make, label in ((bench_map, "bench map"), (big_map, "configs[2] map")):
        ef, last = make(api, bench)
        run(api, accuracy, ef, last, label)
        ef.close()
