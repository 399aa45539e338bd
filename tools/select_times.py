"""Select / gather / erase kernel times (ef_map_select, ef_map_gather, ef_map_erase; csrc/ef_select.inc).

    python tools/select_times.py               wall clock per call (host clock around work that ends in a synchronise, median of REPS), the
                                               box's copy rate (ef_dev_calibrate), the shapes of every launch ("SHAPE" lines), and the time of
                                               the path an erase replaces (downloadMap + numpy mask + uploadMap + restore) on the same map
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/select_times.py
                                               the same run under the profiler: its kernel trace has the launches' own durations
    python tools/select_times.py --summarise DIR/.../*_kernel_trace.csv LOG
                                               medians per kernel and map from that trace, the algorithmic bytes of each launch (from the SHAPE
                                               lines of the run's output LOG) and their rate as a fraction of the box's copy rate

Maps: the steady bench map (140 replay steps of the bench sequence, 640x480) and the configs[2] map (bench.preseed with 1 M surfels, then
three 1280x960 frames).  Selections: BOX only (the half-space below the median x), BOX + LAST_TIME, LABEL at C = 14; gather of 100 000 rows
drawn with replacement; three erases of a tenth of the map each (a slab of x), prediction renewal included in the wall clock."""
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

REPS = 10
NG = 100000
KERNELS = ("k_select_flags", "k_select_rows", "k_select_compact", "k_select_count", "k_select_mark_rows", "k_map_gather")


def bench_map(api, bench):
    frames = bench.replay_frames(0xEF0001, 140, 640, 480)
    dev = bench.upload_frames(api, frames)
    ef = api.ElasticFusion()
    for k, (r, d) in enumerate(dev):
        ef.processFrameDevice(r.p.value, d.p.value, k)
    ef.synchronize()
    return ef, frames[-1]


def big_map(api, bench):
    w, h = 1280, 960
    frames = bench.replay_frames(0xEF0001, 4, w, h)
    ef = api.ElasticFusion(width=w, height=h, fx=1056.0, fy=1056.0, cx=640.0, cy=480.0)
    bench.preseed(ef, 0xEF0001, w, h, 1 << 20, frames[0])
    dev = bench.upload_frames(api, frames)
    for k, (r, d) in enumerate(dev[1:]):
        ef.processFrameDevice(r.p.value, d.p.value, 2 + k)
    ef.synchronize()
    return ef, frames[-1]


def timed(ef, fn, reps=REPS):
    fn()
    ef.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ef.synchronize()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6


def run(api, ef, last, label):
    from elasticfusion_amd.api import SEL_BOX, SEL_LABEL, SEL_LAST_TIME
    S = ef.downloadMap()
    n = len(S)
    fin = np.isfinite(S[:, 0])
    xmed = float(np.median(S[fin, 0]))
    tick = ef.getTick()
    sels = {"box": ef.mapSelection(tests=SEL_BOX, box_max=[xmed, np.inf, np.inf]),
            "box_last": ef.mapSelection(tests=SEL_BOX | SEL_LAST_TIME, box_max=[xmed, np.inf, np.inf], last_time_min=tick - 10)}
    rows = api.DevBuf(n * 4)
    cnt = api.DevBuf(16)
    print(f"{label}: {n} surfels; wall clock per call in us (median of {REPS} after a warm-up)", flush=True)
    for name, sel in sels.items():
        us = timed(ef, lambda: ef.selectSurfelsDevice(sel, rows.p, n, cnt.p))
        k = int(cnt.to_array(np.uint32, 1)[0])
        print(f"  select {name:9s} {us:9.1f}   selected {k}", flush=True)
        print("SHAPE " + json.dumps(dict(map=label, op="select_" + name, n=n, selected=k)), flush=True)
    ef.enableLabels(14)
    sel = ef.mapSelection(tests=SEL_LABEL, label_class=0, label_min_prob=0.0)
    us = timed(ef, lambda: ef.selectSurfelsDevice(sel, rows.p, n, cnt.p))
    k = int(cnt.to_array(np.uint32, 1)[0])
    print(f"  select label C=14 {us:7.1f}   selected {k}   (each call re-aligns the table first: k_labels_align)", flush=True)
    print("SHAPE " + json.dumps(dict(map=label, op="select_label", n=n, selected=k, C=14)), flush=True)
    ef.enableLabels(0)
    ef.setSurfelIds(False)
    g = np.random.default_rng(3).integers(0, n, NG).astype(np.uint32)
    d_g, d_out = api.DevBuf.from_array(g), api.DevBuf(NG * 48)
    us = timed(ef, lambda: ef.gatherSurfelsDevice(d_g.p, NG, d_out.p))
    print(f"  gather {NG} rows {us:7.1f}", flush=True)
    print("SHAPE " + json.dumps(dict(map=label, op="gather", n=n, rows=NG)), flush=True)
    # the path an erase replaces, on the same map: the whole map to the host and back, a full re-preprocess of the last frame
    ck_rgb, ck_depth = last[0], last[1]
    t0 = time.perf_counter()
    m = ef.downloadMap()
    keep = ~(m[:, 0] <= np.float32(np.quantile(S[fin, 0], 0.1)))
    ck = dict(map=m[keep], tick=ef.getTick(), qt=ef.getPoseQT(), rgb=ck_rgb, depth=ck_depth)
    ef.restore(ck)
    ef.synchronize()
    legacy = (time.perf_counter() - t0) * 1e6
    print(f"  the replaced path (downloadMap + numpy mask + uploadMap + restore), a tenth of the map removed: {legacy:9.1f} us   kept {int(keep.sum())}", flush=True)
    for q in (0.2, 0.3, 0.4):
        before = ef.lastCount()
        sel = ef.mapSelection(tests=SEL_BOX, box_max=[float(np.quantile(S[fin, 0], q)), np.inf, np.inf])
        t0 = time.perf_counter()
        removed = ef.eraseSurfels(sel)
        us = (time.perf_counter() - t0) * 1e6
        print(f"  erase (x below the {q:.1f} quantile) {us:9.1f}   rows {before} removed {removed}", flush=True)
        print("SHAPE " + json.dumps(dict(map=label, op="erase", n=before, kept=before - removed)), flush=True)


def summarise(path, log):
    shapes = [json.loads(ln[6:]) for ln in open(log) if ln.startswith("SHAPE ")]
    copy_rate = None
    for ln in open(log):
        m = re.search(r"copy rate ([0-9.]+) GB/s", ln)
        if m:
            copy_rate = float(m.group(1)) * 1e9
    maps = []
    for s in shapes:
        if s["map"] not in maps:
            maps.append(s["map"])
    by = {}
    for r in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                by.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    # the launches of a kernel come in the order of the run: per map, per op, 1 + REPS launches of each select / gather, one per erase
    plan = {"k_select_flags": [("select_box", 1 + REPS), ("select_box_last", 1 + REPS), ("select_label", 1 + REPS), ("erase", 3)],
            "k_select_rows": [("select_box", 1 + REPS), ("select_box_last", 1 + REPS), ("select_label", 1 + REPS)],
            "k_map_gather": [("gather", 1 + REPS)], "k_select_compact": [("erase", 3)]}
    bytes_of = {("k_select_flags", "select_box"): lambda s: 17 * s["n"], ("k_select_flags", "select_box_last"): lambda s: 33 * s["n"],
                ("k_select_flags", "select_label"): lambda s: (4 * s["C"] + 1) * s["n"], ("k_select_flags", "erase"): lambda s: 17 * s["n"],
                ("k_select_rows", "select_box"): lambda s: s["n"] + 4 * s["selected"], ("k_select_rows", "select_box_last"): lambda s: s["n"] + 4 * s["selected"],
                ("k_select_rows", "select_label"): lambda s: s["n"] + 4 * s["selected"],
                ("k_map_gather", "gather"): lambda s: (4 + 96) * s["rows"], ("k_select_compact", "erase"): lambda s: s["n"] + 96 * s["kept"]}
    print(f"copy rate of the box (16 MiB read + 16 MiB written per launch): {copy_rate / 1e9 if copy_rate else float('nan'):.0f} GB/s")
    print("kernel             op               map               launches  median us   algorithmic MB   GB/s   of the copy rate")
    for k, ops in plan.items():
        v = [d for _, d in sorted(by.get(k, []))]
        per_map = sum(c for _, c in ops)
        if len(v) != per_map * len(maps):
            print(f"{k}: {len(v)} launches in the trace, {per_map * len(maps)} expected: not summarised")
            continue
        at = 0
        for mp in maps:
            for op, c in ops:
                d = v[at:at + c]
                at += c
                sh = [s for s in shapes if s["map"] == mp and s["op"] == op]
                med = float(np.median(d)) / 1e3
                b = float(np.median([bytes_of[(k, op)](s) for s in sh]))
                rate = b / (med * 1e-6)
                frac = f"{rate / copy_rate:.2f}" if copy_rate else "n/a"
                print(f"{k:18s} {op:16s} {mp:16s} {c:9d}  {med:9.1f}   {b / 1e6:14.2f}   {rate / 1e9:5.0f}   {frac}")


if __name__ == "__main__":
    if "--summarise" in sys.argv:
        i = sys.argv.index("--summarise")
        summarise(sys.argv[i + 1], sys.argv[i + 2])
        sys.exit(0)
    import bench
    from elasticfusion_amd import api
    e, s = C.c_float(0), C.c_float(0)
    api._chk(api.lib().ef_dev_calibrate(None, C.byref(e), C.byref(s)))
    print(f"ef_dev_calibrate: empty kernel {e.value:.2f} us, 16 MiB copy {s.value:.2f} us per launch: copy rate {2 * 16 * 1048576 / (s.value * 1e-6) / 1e9:.0f} GB/s "
          "(bytes read + bytes written)", flush=True)
    for make, label in ((bench_map, "bench map"), (big_map, "configs[2] map")):
        ef, last = make(api, bench)
        run(api, ef, last, label)
        ef.close()
