"""Normal-estimation times (ef_map_normals_dev / ef_map_reestimate_normals; csrc/ef_normals.inc).

    python tools/normal_times.py               wall clock per call (host clock around work that ends in a synchronise, median of REPS) on two
                                               synthetic maps of 100 k and 1 M surfels: the estimate for k = 8 and k = 16 at the default
                                               radius and cell (index already built), the outliers' neighbour statistics with the same
                                               radius, cell and k (the same walk without the gather and the fit), the list of the CURVED rows,
                                               and ef_map_reestimate_normals itself
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/normal_times.py
                                               the same run under the profiler: its kernel trace has the launches' own durations
    python tools/normal_times.py --summarise DIR/.../*_kernel_trace.csv
                                               median, minimum and maximum per kernel, map and k from that trace
    python tools/normal_times.py --all OUT.txt
                                               the three steps above as child processes, each under its own `timeout`, the next one started
                                               only if the one before ended with status 0; writes OUT.txt (profiles/r30_normal_times.txt)

Maps: a jittered 5 mm lattice on a wavy surface (about 110 surfels within the default 3 cm), stored normals +z: every row is a participant."""
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
import numpy as np

REPS = 5
WRITES = 3
SIZES = (100_000, 1_000_000)
KS = (8, 16)
KERNELS = ("k_normal_join", "k_outlier_join", "k_normal_split", "k_normal_flags", "k_normal_tally", "k_normal_apply", "k_select_count", "k_select_rows",
           "k_query_count", "k_query_scatter")


def surface(n, pitch=0.005, seed=1):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    x = (i % side + rng.uniform(-0.3, 0.3, n)) * pitch
    y = (i // side + rng.uniform(-0.3, 0.3, n)) * pitch
    S = np.zeros((n, 12), np.float32)
    S[:, 0], S[:, 1], S[:, 2] = x, y, 1.0 + 0.05 * np.sin(3.0 * x) * np.cos(2.0 * y) + rng.normal(0.0, 0.0005, n)
    S[:, 3], S[:, 4], S[:, 6], S[:, 7], S[:, 10], S[:, 11] = 20.0, float(0x808080), 1, 2, 1.0, 0.004
    return S[rng.permutation(n)]


def timed(ef, call, reps):
    call()
    ef.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ef.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t))


def run(api, n):
    S = surface(n)
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    out = {k: api.DevBuf(n * w) for k, w in (("normals", 12), ("curvature", 4), ("spacing", 4), ("count", 4), ("status", 1), ("rows", 4))}
    cnt, res = api.DevBuf(16), api.DevBuf(C.sizeof(api.ef_normal_result))
    print(f"map of {n} surfels; wall clock per call in us (median of {REPS} after a warm-up; the write-back: median of {WRITES})", flush=True)
    for k in KS:
        prm = ef.normalParams(k=k)
        oprm = ef.outlierParams(k=k, radius=prm.radius, cell=prm.cell)
        us = timed(ef, lambda: ef.estimateNormalsDevice(prm, None, out["normals"].p, out["curvature"].p, out["spacing"].p, out["count"].p, out["status"].p, n), REPS)
        us_join = timed(ef, lambda: ef.estimateNormalsDevice(prm, None, None, None, None, None, None, 0), REPS)
        us_out = timed(ef, lambda: ef.neighborStatsDevice(oprm, None, None, None, 0), REPS)
        us_sel = timed(ef, lambda: ef.normalSelectDevice(prm, None, api.NORMALS_CURVED, out["rows"].p, n, cnt.p, res.p), REPS)
        st = np.bincount(out["status"].to_array(np.uint8, n), minlength=4)
        print(f"  n {n} k {k:2d}: ef_map_normals_dev {us:10.1f}   its join alone {us_join:10.1f}   the outliers' join alone {us_out:10.1f}   "
              f"the CURVED list {us_sel:10.1f}   status counts {st.tolist()}   curved {int(cnt.to_array(np.uint32, 1)[0])}", flush=True)
    t = []
    for _ in range(WRITES):
        ef.uploadMap(S)
        ef.estimateNormalsDevice(prm, None, None, None, None, None, None, 0)       # the index of the map as it stands, at this cell
        ef.synchronize()
        t0 = time.perf_counter()
        got = ef.reestimateNormals(prm)
        t.append((time.perf_counter() - t0) * 1e6)
    print(f"  n {n} k {prm.k:2d}: ef_map_reestimate_normals {float(np.median(t)):10.1f}   {got}", flush=True)
    ef.close()


def summarise(path):
    by = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"\b(k_\w+(?:<[^>]*>)?)", r["Kernel_Name"])
        if m and m.group(1).split("<")[0] in KERNELS:
            by.setdefault(m.group(1), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    print("kernel                                   map        launches  median us    min us    max us   (the first half of a kernel's launches is the 100 k map's)")
    for name in sorted(by):
        v = np.array([d for _, d in sorted(by[name])]) / 1e3
        half = len(v) // 2
        for label, g in ((f"{SIZES[0]}", v[:half]), (f"{SIZES[1]}", v[half:])):
            if len(g):
                print(f"{name:40s} {label:10s} {len(g):6d}  {float(np.median(g)):9.1f} {g.min():9.1f} {g.max():9.1f}")


def everything(out):
    d = out + ".d"
    os.makedirs(d, exist_ok=True)
    me = os.path.join(ROOT, "tools", "normal_times.py")
    plain, traced = os.path.join(d, "plain.log"), os.path.join(d, "traced.log")
    steps = [(["timeout", "-k", "10", "240", sys.executable, me], plain),
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
    summary = subprocess.run([sys.executable, me, "--summarise", trace], stdout=subprocess.PIPE, text=True, check=True).stdout
    keep = lambda p: "".join(ln for ln in open(p) if re.match(r"^(ef_dev|map of|  )", ln))
    with open(out, "w") as f:
        f.write("tools/normal_times.py on one MI355X, one visit.  Plain run (profiler off): wall clocks and the box's copy rate.\n\n" + keep(plain))
        f.write("\nThe same run under rocprofv3 --kernel-trace --stats (wall clocks that carry the tracer's cost):\n\n" + keep(traced))
        f.write("\npython tools/normal_times.py --summarise <kernel trace>: the launches' own durations\n\n" + summary)
    print(open(out).read())


if __name__ == "__main__":
    if "--summarise" in sys.argv:
        summarise(sys.argv[sys.argv.index("--summarise") + 1])
        sys.exit(0)
    if "--all" in sys.argv:
        everything(sys.argv[sys.argv.index("--all") + 1])
        sys.exit(0)
    from elasticfusion_amd import api
    e, s = C.c_float(0), C.c_float(0)
    api._chk(api.lib().ef_dev_calibrate(None, C.byref(e), C.byref(s)))
    print(f"ef_dev_calibrate: empty kernel {e.value:.2f} us, 16 MiB copy {s.value:.2f} us per launch: copy rate {2 * 16 * 1048576 / (s.value * 1e-6) / 1e9:.0f} GB/s "
          "(bytes read + bytes written)", flush=True)
    for n in SIZES:
        run(api, n)
