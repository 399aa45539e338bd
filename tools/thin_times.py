"""Thin kernel times (ef_map_thin / ef_map_thin_select; csrc/ef_thin.inc).

    python tools/thin_times.py [--no-legacy]   wall clock per call (host clock around work that ends in a synchronise, median of REPS) of one
                                               thin at cell 1 / 2 / 5 / 10 cm: the removed list (index already built at that cell), the same
                                               with the index rebuilt, ef_map_thin itself and ef_map_erase_rows_dev of the same rows; the
                                               shapes ("SHAPE" lines); and, as context only, the path a thin replaces on the same map
                                               (downloadMap + the numpy reference of tests/thinref.py + eraseRows)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/thin_times.py --no-legacy
                                               the same run under the profiler: its kernel trace has the launches' own durations
    python tools/thin_times.py --summarise DIR/.../*_kernel_trace.csv LOG
                                               medians per kernel, map and cell from that trace
    python tools/thin_times.py --all OUT.txt   the three steps above as child processes, each under its own `timeout`, the next one started
                                               only if the one before ended with status 0; writes OUT.txt (profiles/r19_thin_kernel_times.txt)

Maps: the steady bench map (140 replay steps of the bench sequence, 640x480) and the configs[2] map (bench.preseed with 1 M surfels, then
three 1280x960 frames).  A thin changes the map, so every timed ef_map_thin / erase is preceded by an (untimed) uploadMap of the saved map."""
import csv
import ctypes as C
import glob
import json
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

REPS = 10
THINS = 3
CELLS = (0.01, 0.02, 0.05, 0.10)
KERNELS = ("k_thin_flags", "k_query_count", "k_query_scatter", "k_select_count", "k_select_rows", "k_select_compact")


def run(api, ef, label, legacy):
    S = ef.downloadMap()
    n = len(S)
    rows = api.DevBuf(n * 4)
    cnt = api.DevBuf(16)
    print(f"{label}: {n} surfels; wall clock per call in us (median of {REPS} after a warm-up; thin and erase: median of {THINS})", flush=True)
    for cell in CELLS:
        ef.uploadMap(S)          # (the replaced path of the cell before left its thinned map)
        prm = ef.thinParams(cell=cell)
        us = timed(ef, lambda: ef.thinSelectDevice(prm, None, False, rows.p, n, cnt.p))
        k = int(cnt.to_array(np.uint32, 1)[0])
        removed = rows.to_array(np.uint32, n)[:k].copy()
        d_removed = api.DevBuf.from_array(removed) if k else None

        def stale():
            ef.uploadMap(S)
            ef.synchronize()
            t0 = time.perf_counter()
            ef.thinSelectDevice(prm, None, False, rows.p, n, cnt.p)
            ef.synchronize()
            return (time.perf_counter() - t0) * 1e6
        us_stale = float(np.median([stale() for _ in range(THINS)]))
        t_thin, t_erase = [], []
        for _ in range(THINS):
            ef.uploadMap(S)
            ef.thinSelectDevice(prm, None, False, None, 0, cnt.p)      # the index of the map as it stands, at this cell
            ef.synchronize()
            t0 = time.perf_counter()
            res = ef.thinSurfels(prm)
            t_thin.append((time.perf_counter() - t0) * 1e6)
            assert res["removed"] == k and res["count_after"] == n - k, (res, k)
            ef.uploadMap(S)
            ef.synchronize()
            t0 = time.perf_counter()
            gone = ef.eraseRowsDevice(d_removed.p if k else None, k)
            t_erase.append((time.perf_counter() - t0) * 1e6)
            assert gone == k
        print(f"  cell {cell:.2f} m: removed list {us:9.1f}   with the index rebuilt {us_stale:9.1f}   ef_map_thin {float(np.median(t_thin)):9.1f}   "
              f"ef_map_erase_rows_dev of the same rows {float(np.median(t_erase)):9.1f}   cells {res['cells']} removed {k}", flush=True)
        print("SHAPE " + json.dumps(dict(map=label, cell=cell, n=n, cells=res["cells"], removed=k)), flush=True)
        if legacy:
            import thinref
            ef.uploadMap(S)
            ef.synchronize()
            t0 = time.perf_counter()
            m = ef.downloadMap()
            t1 = time.perf_counter()
            t = thinref.thin(m, cell)
            t2 = time.perf_counter()
            ef.eraseRows(t["rows_removed"])
            t3 = time.perf_counter()
            assert np.array_equal(t["rows_removed"], removed)
            print(f"    the replaced path: downloadMap {(t1 - t0) * 1e6:9.1f} + numpy reference {(t2 - t1) * 1e6:11.1f} + eraseRows {(t3 - t2) * 1e6:9.1f} us",
                  flush=True)
    ef.uploadMap(S)


def summarise(path, log):
    shapes = [json.loads(ln[6:]) for ln in open(log) if ln.startswith("SHAPE ")]
    by = {}
    for r in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                by.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    # per map and cell, in the order of the run: 1 + REPS lists, THINS lists on a stale index, then THINS x (a count-only list, a thin); an index
    # build per stale list, per count-only list and one for the first list of the cell; a compaction per thin and per erase
    per = {"k_thin_flags": 1 + REPS + 3 * THINS, "k_query_count": 1 + 2 * THINS, "k_query_scatter": 1 + 2 * THINS, "k_select_rows": 1 + REPS + THINS,
           "k_select_compact": 2 * THINS}
    print("kernel             map               cell   launches  median us    min us    max us")
    for k, c in per.items():
        v = [d for _, d in sorted(by.get(k, []))]
        if k.startswith("k_query"):
            v = v[len(v) - c * len(shapes):]      # (the maps' own construction launches nothing of the index; anything earlier is dropped)
        if len(v) != c * len(shapes):
            print(f"{k}: {len(v)} launches in the trace, {c * len(shapes)} expected: not summarised")
            continue
        for i, s in enumerate(shapes):
            d = np.array(v[i * c:(i + 1) * c]) / 1e3
            print(f"{k:18s} {s['map']:16s} {s['cell']:5.2f} {c:9d}  {float(np.median(d)):9.1f} {d.min():9.1f} {d.max():9.1f}")


def everything(out):
    d = out + ".d"
    os.makedirs(d, exist_ok=True)
    me = os.path.join(ROOT, "tools", "thin_times.py")
    plain, traced = os.path.join(d, "plain.log"), os.path.join(d, "traced.log")
    steps = [(["timeout", "-k", "10", "420", sys.executable, me], plain),
             (["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "trace"), "--",
               sys.executable, me, "--no-legacy"], traced)]
    for cmd, log in steps:
        with open(log, "w") as f:
            rc = subprocess.run(cmd, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT).returncode
        print(" ".join(cmd[:6]), "...", "exit", rc, flush=True)
        if rc != 0:                                   # nothing more is started after a step that failed or ran out of time
            print(open(log).read()[-3000:])
            sys.exit(rc)
    trace = sorted(glob.glob(os.path.join(d, "trace", "**", "*_kernel_trace.csv"), recursive=True))[-1]
    summary = subprocess.run([sys.executable, me, "--summarise", trace, traced], stdout=subprocess.PIPE, text=True, check=True).stdout
    keep = lambda p: "".join(ln for ln in open(p) if not ln.startswith("SHAPE ") and re.match(r"^(ef_dev|bench|configs|  )", ln))
    with open(out, "w") as f:
        f.write("tools/thin_times.py on one MI355X, one visit.  Plain run (profiler off): wall clocks and the box's copy rate.\n\n" + keep(plain))
        f.write("\nThe same run under rocprofv3 --kernel-trace --stats (wall clocks that carry the tracer's cost; without the replaced path):\n\n" + keep(traced))
        f.write("\npython tools/thin_times.py --summarise <kernel trace> <log of the traced run>: the launches' own durations\n\n" + summary)
    print(open(out).read())


if __name__ == "__main__":
    if "--summarise" in sys.argv:
        i = sys.argv.index("--summarise")
        summarise(sys.argv[i + 1], sys.argv[i + 2])
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
        run(api, ef, label, "--no-legacy" not in sys.argv)
        ef.close()
