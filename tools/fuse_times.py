"""Fuse kernel times (ef_map_fuse; csrc/ef_fuse.inc).

    python tools/fuse_times.py                 wall clock per call (host clock around a call that synchronises before and after, median of
                                               REPS) of ef_map_fuse_dev and of ef_map_insert_dev over the same records on the same map, the
                                               box's copy rate (ef_dev_calibrate) and the shapes of the calls ("SHAPE" lines)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fuse_times.py
                                               the same run under the profiler: its kernel trace has the launches' own durations
    python tools/fuse_times.py --summarise DIR/.../*_kernel_trace.csv LOG
                                               medians per kernel and map from that trace: k_fuse_pick, k_fuse_outcome, k_fuse_apply, the counts
                                               (k_select_count) and, as the yardstick, k_insert_gate and k_insert_scatter of the fuse's calls
                                               and of the insert's calls of the same run

Maps: the steady bench map (140 replay steps of the bench sequence, 640x480) and the configs[2] map (bench.preseed with 1 M surfels, then
three 1280x960 frames).  Records: 99 999 at the default parameters under a motion of a few millimetres: a third are map surfels moved by up to
3 mm, a third the same surfels moved again (so that most surfels with a competitor have two), a third map surfels lifted 5 cm along their
normals (new).  A fuse changes the map in place, so every timed call is preceded by an (untimed) uploadMap of the saved map and a query that
builds the index; neither launches a kernel this tool summarises."""
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
NI = 99999
KERNELS = ("k_fuse_pick", "k_fuse_outcome", "k_fuse_apply", "k_insert_gate", "k_insert_scatter", "k_select_count")


def records_for(S, accuracy, T):
    rng = np.random.default_rng(8)
    third = NI // 3
    ok = np.nonzero(np.isfinite(S[:, :3]).all(1))[0]
    pick = rng.choice(ok, third, replace=len(ok) < third)

    def moved(rows):
        r = S[rows].copy()
        off = rng.normal(size=(len(rows), 3))
        r[:, :3] += (off / np.linalg.norm(off, axis=1, keepdims=True) * rng.uniform(0, 0.003, (len(rows), 1))).astype(np.float32)
        r[:, 3] = rng.uniform(0.5, 12, len(rows))
        return r

    lifted = S[rng.choice(ok, third, replace=len(ok) < third)].copy()
    lifted[:, :3] += lifted[:, 8:11] * np.float32(0.05)
    R = np.concatenate([moved(pick), moved(pick), lifted])
    return accuracy.move_surfels(R[rng.permutation(len(R))], np.linalg.inv(T))


def run(api, accuracy, ef, label):
    S = ef.downloadMap()
    n0 = len(S)
    w = 0.002
    T = np.array([[np.cos(w), -np.sin(w), 0, 0.003], [np.sin(w), np.cos(w), 0, -0.002], [0, 0, 1, 0.001], [0, 0, 0, 1]])
    R = records_for(S, accuracy, T)
    d_rec = api.DevBuf.from_array(R)
    d_new, d_match, d_out = api.DevBuf(NI * 4), api.DevBuf(NI * 4), api.DevBuf(NI)
    keep, pT = api._pose16(T)
    print(f"{label}: {n0} surfels, {NI} records; wall clock per call in us (median of {REPS} after a warm-up; the index already built)", flush=True)

    def timed(call):
        t = []
        for rep in range(1 + REPS):
            ef.uploadMap(S)
            ef.queryNearestRaw(S[:4, :3], 0.01, -1.0)
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(t[1:]))

    fprm, fres = ef.fuseParams(), api.ef_fuse_result()
    us = timed(lambda: api._chk(api.lib().ef_map_fuse_dev(ef.h, d_rec.p, C.c_uint32(NI), pT, C.byref(fprm), C.byref(fres), d_new.p, d_match.p,
                                                            d_out.p), ef.h))
    print(f"  fuse   {NI} records {us:9.1f}   fused {fres.fused} absorbed {fres.absorbed} weightless {fres.weightless} novel {fres.novel} "
          f"skipped {fres.skipped}", flush=True)
    iprm, ires = ef.insertParams(), api.ef_insert_result()
    us = timed(lambda: api._chk(api.lib().ef_map_insert_dev(ef.h, d_rec.p, C.c_uint32(NI), pT, C.byref(iprm), C.byref(ires), d_new.p, d_match.p),
                                ef.h))
    print(f"  insert {NI} records {us:9.1f}   inserted {ires.inserted} duplicates {ires.duplicates} skipped {ires.skipped}", flush=True)
    print("SHAPE " + json.dumps(dict(map=label, n0=n0, n=NI, fused=int(fres.fused), absorbed=int(fres.absorbed), novel=int(fres.novel))), flush=True)


def summarise(path, log):
    shapes = [json.loads(ln[6:]) for ln in open(log) if ln.startswith("SHAPE ")]
    by = {}
    for r in csv.DictReader(open(path)):
        name = re.sub(r"\s+", " ", r["Kernel_Name"])
        for k in KERNELS:
            if k in name:
                by.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    # per map, in the order of the run: 1 + REPS fuses (gate, two counts, pick, outcome, two more counts, apply, scatter), then 1 + REPS inserts
    # (gate, two counts, scatter); the first call of each kind is the warm-up
    c = 1 + REPS
    per_map = {"k_fuse_pick": c, "k_fuse_outcome": c, "k_fuse_apply": c, "k_insert_gate": 2 * c, "k_insert_scatter": 2 * c, "k_select_count": 6 * c}
    print("kernel                        map               launches  median us")
    for k, per in per_map.items():
        v = [d for _, d in sorted(by.get(k, []))]
        if len(v) != per * len(shapes):
            print(f"{k}: {len(v)} launches in the trace, {per * len(shapes)} expected: median of all of them {float(np.median(v)) / 1e3 if v else float('nan'):.1f} us")
            continue
        for i, s in enumerate(shapes):
            d = v[i * per:(i + 1) * per]
            if k in ("k_insert_gate", "k_insert_scatter"):
                for who, part in (("fuse's", d[1:c]), ("insert's", d[c + 1:])):
                    print(f"{k + ' (' + who + ')':29s} {s['map']:16s} {len(part):9d}  {float(np.median(part)) / 1e3:9.1f}")
            elif k == "k_select_count":
                fuse_part = np.array(d[4:4 * c]).reshape(-1, 4)      # per fuse: flags, duplicates, not fused, not weightless
                print(f"{'k_select_count (one of 4)':29s} {s['map']:16s} {fuse_part.size:9d}  {float(np.median(fuse_part)) / 1e3:9.1f}")
            else:
                print(f"{k:29s} {s['map']:16s} {len(d) - 1:9d}  {float(np.median(d[1:])) / 1e3:9.1f}")
    for s in shapes:
        print(f"{s['map']}: n0 {s['n0']}, n {s['n']}, fused {s['fused']}, absorbed {s['absorbed']}, novel {s['novel']}")


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
        run(api, accuracy, ef, label)
        ef.close()
