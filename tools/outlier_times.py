"""Outlier filter times (ef_map_outliers_select / ef_map_remove_outliers; csrc/ef_outlier.inc).

    python tools/outlier_times.py [--no-composed]
                                               wall clock per call (host clock around work that ends in a synchronise, median of REPS) on
                                               the bench map and the configs[2] map: the outlier list with default parameters at cell =
                                               radius / 2, radius and 2 radius (index already built at that cell), the neighbour statistics
                                               alone, the plain kNN query (k = 8, one lane per query) over the map's own positions in ROW
                                               order (the A/B of the join's index order), ef_map_remove_outliers itself, and the path it
                                               replaces: downloadMap + ef_query_knn on the map's own positions + numpy + ef_map_erase_rows
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/outlier_times.py --no-composed
                                               the same run under the profiler: its kernel trace has the launches' own durations
    python tools/outlier_times.py --summarise DIR/.../*_kernel_trace.csv
                                               median, minimum and maximum per kernel and map from that trace
    python tools/outlier_times.py --all OUT.txt
                                               the three steps above as child processes, each under its own `timeout`, the next one started
                                               only if the one before ended with status 0; writes OUT.txt (profiles/r27_outlier_times.txt)

Maps: the steady bench map (140 replay steps of the bench sequence, 640x480) and the configs[2] map (bench.preseed with 1 M surfels, then
three 1280x960 frames).  A removal changes the map, so every timed removal is preceded by an (untimed) uploadMap of the saved map."""
import csv
import ctypes as C
import glob
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from select_times import bench_map, big_map, timed

REPS = 5
REMOVALS = 3
KERNELS = ("k_outlier_join", "k_outlier_partials", "k_outlier_finish", "k_outlier_flags", "k_outlier_tally", "k_outlier_split", "k_select_count",
           "k_select_rows", "k_select_compact", "k_query_count", "k_query_scatter", "k_query<1, 8>", "k_queryILi1ELi8E")


def composed(ef, prm):
    """the path a user composes without the feature; returns (outlier rows, seconds of [download, query, numpy, erase])"""
    k = prm.k
    t0 = time.perf_counter()
    m = ef.downloadMap()
    t1 = time.perf_counter()
    rows, d2, count = ef.queryKnn(m[:, :3], k + 1, prm.radius, prm.min_conf)       # one more: the surfel finds itself
    t2 = time.perf_counter()
    n = len(m)
    own = rows == np.arange(n, dtype=np.uint32)[:, None]
    found = own.any(1)
    d2 = np.where(own, np.inf, d2)
    d2.sort(1)                                                                    # (d2 ascending: the self slot goes last)
    cnt = count - found
    mean = np.sqrt(d2[:, :k]).sum(1, dtype=np.float32) / np.float32(k)
    fin = np.isfinite(m[:, :3]).all(1)
    measured = fin & (cnt >= k)
    mu = mean[measured].astype(np.float64).mean() if measured.any() else 0.0
    sd = mean[measured].astype(np.float64).std() if measured.any() else 0.0
    thr = np.float32(mu + prm.std_ratio * sd) if measured.any() else np.float32(np.inf)
    out = np.nonzero((measured & (mean > thr)) | (fin & ~measured & (prm.flag_sparse != 0)))[0].astype(np.uint32)
    t3 = time.perf_counter()
    ef.eraseRows(out)
    t4 = time.perf_counter()
    return out, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)


def run(api, ef, label, with_composed):
    S = ef.downloadMap()
    n = len(S)
    rows, cnt, res = api.DevBuf(n * 4), api.DevBuf(16), api.DevBuf(C.sizeof(api.ef_outlier_result))
    print(f"{label}: {n} surfels; wall clock per call in us (median of {REPS} after a warm-up; removals and the composed path: median of {REMOVALS})",
          flush=True)
    radius = ef.outlierParams().radius
    for cell in (radius / 2, radius, 2 * radius):
        prm = ef.outlierParams(cell=cell)
        us = timed(ef, lambda: ef.outlierSelectDevice(prm, None, rows.p, n, cnt.p, res.p), REPS)
        k = int(cnt.to_array(np.uint32, 1)[0])
        us_stats = timed(ef, lambda: ef.neighborStatsDevice(prm, None, None, None, 0), REPS)
        print(f"  cell {cell:.3f} m: outlier list {us:10.1f}   the join alone {us_stats:10.1f}   outliers {k}", flush=True)
    prm = ef.outlierParams()
    # the A/B of the index order: the plain query kernel, one lane per query, over the map's own positions in row order at the same cell
    pts = api.DevBuf.from_array(np.ascontiguousarray(S[:, :3]))
    q_rows, q_d2, q_cnt = api.DevBuf(n * 8 * 4), api.DevBuf(n * 8 * 4), api.DevBuf(n * 4)
    ef.setQueryCell(prm.cell)
    us_q = timed(ef, lambda: ef.queryKnnDevice(pts.p, n, 8, prm.radius, prm.min_conf, q_rows.p, q_d2.p, q_cnt.p), REPS)
    print(f"  k_query<1, 8> over the map's positions in row order, cell {prm.cell:.3f}: {us_q:10.1f}", flush=True)
    t_fused = []
    for _ in range(REMOVALS):
        ef.uploadMap(S)
        ef.outlierSelectDevice(prm, None, None, 0, cnt.p)          # the index of the map as it stands, at this cell
        ef.synchronize()
        t0 = time.perf_counter()
        got = ef.removeOutliers(prm)
        t_fused.append((time.perf_counter() - t0) * 1e6)
    fused = float(np.median(t_fused))
    print(f"  ef_map_remove_outliers {fused:10.1f}   removed {got['outliers']} of {n}, threshold {got['threshold']:.6f}, measured {got['measured']}, "
          f"sparse {got['sparse']}", flush=True)
    if with_composed:
        parts = []
        for _ in range(REMOVALS):
            ef.uploadMap(S)
            ef.queryKnn(S[:8, :3], 2, prm.radius)                  # the index of the map as it stands, at this cell
            ef.synchronize()
            out, t = composed(ef, prm)
            parts.append(t)
        p = np.median(np.array(parts), 0) * 1e6
        print(f"  the composed path: downloadMap {p[0]:10.1f} + ef_query_knn {p[1]:10.1f} + numpy {p[2]:10.1f} + ef_map_erase_rows {p[3]:10.1f} = "
              f"{p.sum():10.1f} us; removed {len(out)}; fused / composed = {fused / p.sum():.4f}", flush=True)
    ef.uploadMap(S)


def summarise(path):
    by = {}
    for r in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                by.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    print("kernel               map              launches  median us    min us    max us   (the first half of a kernel's launches is the bench map's)")
    per_cell = 2 * (1 + REPS)             # the join's launches per cell: the lists and the statistics, a warm-up each
    for k in KERNELS:
        v = np.array([d for _, d in sorted(by.get(k, []))]) / 1e3
        if not len(v):
            continue
        half = len(v) // 2
        for name, d in (("bench map", v[:half]), ("configs[2] map", v[half:])):
            groups = [(name, d)]
            if k == "k_outlier_join" and len(d) == 3 * per_cell + 2 * REMOVALS:
                groups = [(f"{name}, cell {c}", d[i * per_cell:(i + 1) * per_cell]) for i, c in enumerate(("r/2", "r", "2r"))]
            for label, g in groups:
                if len(g):
                    print(f"{k:20s} {label:26s} {len(g):6d}  {float(np.median(g)):9.1f} {g.min():9.1f} {g.max():9.1f}")


def everything(out):
    d = out + ".d"
    os.makedirs(d, exist_ok=True)
    me = os.path.join(ROOT, "tools", "outlier_times.py")
    plain, traced = os.path.join(d, "plain.log"), os.path.join(d, "traced.log")
    steps = [(["timeout", "-k", "10", "420", sys.executable, me], plain),
             (["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "trace"), "--",
               sys.executable, me, "--no-composed"], traced)]
    for cmd, log in steps:
        with open(log, "w") as f:
            rc = subprocess.run(cmd, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT).returncode
        print(" ".join(cmd[:6]), "...", "exit", rc, flush=True)
        if rc != 0:                                   # nothing more is started after a step that failed or ran out of time
            print(open(log).read()[-3000:])
            sys.exit(rc)
    trace = sorted(glob.glob(os.path.join(d, "trace", "**", "*_kernel_trace.csv"), recursive=True))[-1]
    summary = subprocess.run([sys.executable, me, "--summarise", trace], stdout=subprocess.PIPE, text=True, check=True).stdout
    keep = lambda p: "".join(ln for ln in open(p) if re.match(r"^(ef_dev|bench|configs|  )", ln))
    with open(out, "w") as f:
        f.write("tools/outlier_times.py on one MI355X, one visit.  Plain run (profiler off): wall clocks and the box's copy rate.\n\n" + keep(plain))
        f.write("\nThe same run under rocprofv3 --kernel-trace --stats (wall clocks that carry the tracer's cost; without the composed path):\n\n" + keep(traced))
        f.write("\npython tools/outlier_times.py --summarise <kernel trace>: the launches' own durations\n\n" + summary)
    print(open(out).read())


if __name__ == "__main__":
    if "--summarise" in sys.argv:
        summarise(sys.argv[sys.argv.index("--summarise") + 1])
        sys.exit(0)
    if "--all" in sys.argv:
        everything(sys.argv[sys.argv.index("--all") + 1])
        sys.exit(0)
    import bench
    from elasticfusion_amd import api
    e, s = C.c_float(0), C.c_float(0)
    api._chk(api.lib().ef_dev_calibrate(None, C.byref(e), C.byref(s)))
    print(f"ef_dev_calibrate: empty kernel {e.value:.2f} us, 16 MiB copy {s.value:.2f} us per launch: copy rate {2 * 16 * 1048576 / (s.value * 1e-6) / 1e9:.0f} GB/s "
          "(bytes read + bytes written)", flush=True)
    for make, label in ((bench_map, "bench map"), (big_map, "configs[2] map")):
        ef, last = make(api, bench)
        run(api, ef, label, "--no-composed" not in sys.argv)
        ef.close()
