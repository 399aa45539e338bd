"""Carve kernel times (ef_map_carve_select_dev; csrc/ef_carve.inc) beside the box selection's (ef_map_select_dev with EF_SEL_BOX), which reads
the same map stream and writes the same flag bytes: the yardstick.

    python tools/carve_times.py               wall clock per call (host clock around work that ends in a synchronise, median of REPS) of the
                                              removed list for (K, window) = (1, 0), (1, 1), (8, 1), and of the box selection's list, on two
                                              maps; the shapes ("SHAPE" lines)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/carve_times.py
                                              the same run under the profiler: its kernel trace has the launches' own durations
    python tools/carve_times.py --summarise DIR/.../*_kernel_trace.csv LOG
                                              medians per kernel, map and case from that trace, and the ratio to the box selection's kernel
    python tools/carve_times.py --all OUT.txt the steps above as child processes, each under its own `timeout`, the next one started only if
                                              the one before ended with status 0; writes OUT.txt (profiles/r24_carve_kernel_times.txt)

Maps: the steady bench map (140 replay steps of the bench sequence, 640x480) and the configs[2] map (bench.preseed with 1 M surfels, then three
1280x960 frames).  Views: the last frame's depth image K times (K separate copies in memory) from the current pose moved sideways by k
centimetres, with the default parameters: most surfels are supported, few are free, as when a map is carved with the frames it was built from."""
import csv
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from select_times import REPS, bench_map, big_map, timed

CASES = ((1, 0), (1, 1), (8, 1))


def run(api, ef, last, label):
    n = ef.lastCount()
    depth = np.ascontiguousarray(last[1], np.uint16)
    T = ef.get_T_wc()
    rows, cnt, votes = api.DevBuf(max(n, 1) * 4), api.DevBuf(16), api.DevBuf(max(n, 1) * 2)
    print(f"{label}: {n} surfels, depth images {depth.shape[1]} x {depth.shape[0]}; wall clock per call in us (median of {REPS} after a warm-up)",
          flush=True)
    S = ef.downloadMap()
    xmed = float(np.median(S[np.isfinite(S[:, 0]), 0]))
    sel = ef.mapSelection(tests=api.SEL_BOX, box_max=[xmed, np.inf, np.inf])
    us_box = timed(ef, lambda: ef.selectSurfelsDevice(sel, rows.p, n, cnt.p))
    k_box = int(cnt.to_array(np.uint32, 1)[0])
    print(f"  box selection (half the map): list {us_box:9.1f}   selected {k_box}", flush=True)
    for K, w in CASES:
        poses = np.stack([T.copy() for _ in range(K)])
        poses[:, 0, 3] += 0.01 * np.arange(K)
        d_img = api.DevBuf.from_array(np.stack([depth] * K))
        prm = ef.carveParams(window=w)
        us = timed(ef, lambda: ef.carveSelectDevice(d_img.p, poses, prm, None, rows.p, n, cnt.p))
        k = int(cnt.to_array(np.uint32, 1)[0])
        us_votes = timed(ef, lambda: ef.carveSelectDevice(d_img.p, poses, prm, None, rows.p, n, cnt.p, votes.p))
        v = votes.to_array(np.uint8, (n, 2)).astype(np.int64)
        print(f"  K {K} window {w}: removed list {us:9.1f}   with the vote bytes {us_votes:9.1f}   box selection x {us / us_box:5.2f}   removed {k}   "
              f"FREE votes {int(v[:, 0].sum())}  SUPPORTED votes {int(v[:, 1].sum())}", flush=True)
        print("SHAPE " + json.dumps(dict(map=label, K=K, window=w, n=n, removed=k)), flush=True)


def summarise(path, log):
    shapes = [json.loads(ln[6:]) for ln in open(log) if ln.startswith("SHAPE ")]
    maps = list(dict.fromkeys(s["map"] for s in shapes))
    by = {}
    for r in csv.DictReader(open(path)):
        for k in ("k_carve_flags", "k_select_flags"):
            if k in r["Kernel_Name"]:
                by.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    carve = [d for _, d in sorted(by.get("k_carve_flags", []))]
    box = [d for _, d in sorted(by.get("k_select_flags", []))]
    per_case, per_map = 2 * (1 + REPS), 1 + REPS        # (each case is timed twice: without and with the vote bytes)
    box = box[len(box) - per_map * len(maps):] if len(box) >= per_map * len(maps) else []      # (anything a map's construction launched is dropped)
    if len(carve) != per_case * len(shapes) or not box:
        print(f"k_carve_flags: {len(carve)} launches in the trace, {per_case * len(shapes)} expected; k_select_flags: {len(box)}: not summarised")
        return
    print("kernel          map               K  window   launches  median us    min us    max us   x box selection")
    box_med = {}
    for i, m in enumerate(maps):
        d = np.array(box[i * per_map:(i + 1) * per_map]) / 1e3
        box_med[m] = float(np.median(d))
        print(f"k_select_flags  {m:16s}  -    -    {per_map:9d}  {box_med[m]:9.1f} {d.min():9.1f} {d.max():9.1f}        1.00")
    for i, s in enumerate(shapes):
        d = np.array(carve[i * per_case:i * per_case + 1 + REPS]) / 1e3      # (the launches without the vote bytes)
        dv = np.array(carve[i * per_case + 1 + REPS:(i + 1) * per_case]) / 1e3
        print(f"k_carve_flags   {s['map']:16s} {s['K']:2d}    {s['window']}    {1 + REPS:9d}  {float(np.median(d)):9.1f} {d.min():9.1f} {d.max():9.1f}   "
              f"{float(np.median(d)) / box_med[s['map']]:9.2f}")
        print(f"  + vote bytes  {s['map']:16s} {s['K']:2d}    {s['window']}    {1 + REPS:9d}  {float(np.median(dv)):9.1f} {dv.min():9.1f} {dv.max():9.1f}   "
              f"{float(np.median(dv)) / box_med[s['map']]:9.2f}")


def everything(out):
    d = out + ".d"
    os.makedirs(d, exist_ok=True)
    me = os.path.join(ROOT, "tools", "carve_times.py")
    plain, traced = os.path.join(d, "plain.log"), os.path.join(d, "traced.log")
    steps = [(["timeout", "-k", "10", "300", sys.executable, me], plain),
             (["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "trace"), "--",
               sys.executable, me], traced)]
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
        f.write("tools/carve_times.py on one MI355X, one visit.  Plain run (profiler off): wall clocks and the box's copy rate.\n\n" + keep(plain))
        f.write("\nThe same run under rocprofv3 --kernel-trace --stats (wall clocks that carry the tracer's cost):\n\n" + keep(traced))
        f.write("\npython tools/carve_times.py --summarise <kernel trace> <log of the traced run>: the launches' own durations\n\n" + summary)
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
        run(api, ef, last, label)
        ef.close()
