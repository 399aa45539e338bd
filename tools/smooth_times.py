"""Smoothing times (ef_map_smooth_dev / ef_map_smooth_apply; csrc/ef_smooth.inc).

    python tools/smooth_times.py               wall clock per call (host clock around work that ends in a synchronise, median of REPS) on a
                                               synthetic map of 1 M surfels at the defaults (radius = cell = 0.03 m, k 12, compact weights):
                                               ef_map_smooth_dev for iterations 1 .. 4 with and without its output arrays, with the normal
                                               gate, ef_map_normals_dev at the same radius, cell and k (the same walk, one fit), and
                                               ef_map_smooth_apply itself
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/smooth_times.py --kernels
                                               REPS calls at iterations = 4 and REPS calls of ef_map_normals_dev under the profiler: its kernel
                                               trace has the launches' own durations
    python tools/smooth_times.py --summarise DIR/.../*_kernel_trace.csv
                                               median, minimum and maximum per kernel from that trace; the step's launches by iteration
    python tools/smooth_times.py --all OUT.txt
                                               the three steps above as child processes, each under its own `timeout`, the next one started
                                               only if the one before ended with status 0; writes OUT.txt

Map: tools/normal_times.py's, a jittered 5 mm lattice on a wavy surface with 0.5 mm noise (about 110 surfels within the default 3 cm), stored
normals +z, rows shuffled: every row is a participant and is fitted."""
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
N = 1_000_000
ITERATIONS = (1, 2, 3, 4)
KERNELS = ("k_smooth_neighbours", "k_smooth_step", "k_smooth_finish", "k_smooth_tally", "k_smooth_split", "k_smooth_flags", "k_smooth_apply",
           "k_normal_join", "k_normal_split")


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


def buffers(api, n):
    return {k: api.DevBuf(n * w) for k, w in (("position", 12), ("normal", 12), ("curvature", 4), ("shift", 4), ("count", 4), ("status", 1))}


def smooth_call(ef, prm, out, n, res):
    return lambda: ef.smoothMapDevice(prm, None, out["position"].p, out["normal"].p, out["curvature"].p, out["shift"].p, out["count"].p,
                                      out["status"].p, n, res.p)


def run(api, n):
    S = surface(n)
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    out = buffers(api, n)
    res = api.DevBuf(C.sizeof(api.ef_smooth_result))
    print(f"map of {n} surfels; wall clock per call in us (median of {REPS} after a warm-up; the write-back: median of {WRITES})", flush=True)
    nprm = ef.normalParams()
    us_n = timed(ef, lambda: ef.estimateNormalsDevice(nprm, None, None, None, None, None, None, 0), REPS)
    print(f"  ef_map_normals_dev without outputs, radius {nprm.radius:.3f} cell {nprm.cell:.3f} k {nprm.k}: {us_n:10.1f}", flush=True)
    last = None
    for it in ITERATIONS:
        prm = ef.smoothParams(iterations=it)
        us = timed(ef, smooth_call(ef, prm, out, n, res), REPS)
        us_bare = timed(ef, lambda: ef.smoothMapDevice(prm, None, None, None, None, None, None, None, 0, None), REPS)
        gprm = ef.smoothParams(iterations=it, normal_gate=1, min_normal_cos=0.9)
        us_gate = timed(ef, lambda: ef.smoothMapDevice(gprm, None, None, None, None, None, None, None, 0, None), REPS)
        r = ef._smoothResult(api.ef_smooth_result.from_buffer_copy(res.to_array(np.uint8, C.sizeof(api.ef_smooth_result)).tobytes()))
        step = "" if last is None else f"   one more iteration {us_bare - last:8.1f}"
        print(f"  iterations {it}: ef_map_smooth_dev {us:10.1f}   without outputs {us_bare:10.1f}   with the gate {us_gate:10.1f}{step}   {r}", flush=True)
        last = us_bare
    prm = ef.smoothParams()
    t = []
    for _ in range(WRITES):
        ef.uploadMap(S)
        ef.smoothMapDevice(prm, None, None, None, None, None, None, None, 0, None)       # the index of the map as it stands, at this cell
        ef.synchronize()
        t0 = time.perf_counter()
        got = ef.applySmooth(prm)
        t.append((time.perf_counter() - t0) * 1e6)
    print(f"  ef_map_smooth_apply, iterations 1: {float(np.median(t)):10.1f}   {got}", flush=True)
    ef.close()


def kernels(api, n):
    ef = api.ElasticFusion()
    ef.uploadMap(surface(n))
    out = buffers(api, n)
    res = api.DevBuf(C.sizeof(api.ef_smooth_result))
    prm, nprm = ef.smoothParams(iterations=ITERATIONS[-1]), ef.normalParams()
    call = smooth_call(ef, prm, out, n, res)
    for _ in range(REPS + 1):
        call()
        ef.synchronize()
    for _ in range(REPS + 1):
        ef.estimateNormalsDevice(nprm, None, out["normal"].p, out["curvature"].p, None, None, None, n)
        ef.synchronize()
    ef.close()


def summarise(path):
    by = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"\b(k_\w+(?:<[^>]*>)?)", r["Kernel_Name"])
        if m and m.group(1).split("<")[0] in KERNELS:
            by.setdefault(m.group(1), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    print("kernel                                   which              launches  median us    min us    max us")
    for name in sorted(by):
        v = np.array([d for _, d in sorted(by[name])]) / 1e3
        groups = [("all", v)]
        if name.startswith("k_smooth_step") and len(v) % ITERATIONS[-1] == 0:      # the calls run four iterations each: launch i of a call is iteration i + 1
            groups = [(f"iteration {i + 1}", v[i::ITERATIONS[-1]]) for i in range(ITERATIONS[-1])]
        for label, g in groups:
            print(f"{name:40s} {label:18s} {len(g):6d}  {float(np.median(g)):9.1f} {g.min():9.1f} {g.max():9.1f}")


def everything(out):
    d = out + ".d"
    os.makedirs(d, exist_ok=True)
    me = os.path.join(ROOT, "tools", "smooth_times.py")
    plain, traced = os.path.join(d, "plain.log"), os.path.join(d, "traced.log")
    steps = [(["timeout", "-k", "10", "240", sys.executable, me], plain),
             (["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "trace"), "--",
               sys.executable, me, "--kernels"], traced)]
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
        f.write("tools/smooth_times.py on one MI355X, one visit.  Plain run (profiler off): wall clocks and the box's copy rate.\n\n" + keep(plain))
        f.write("\npython tools/smooth_times.py --kernels under rocprofv3 --kernel-trace --stats, then --summarise <kernel trace>: the launches' own "
                "durations\n\n" + summary)
    print(open(out).read())


if __name__ == "__main__":
    if "--summarise" in sys.argv:
        summarise(sys.argv[sys.argv.index("--summarise") + 1])
        sys.exit(0)
    if "--all" in sys.argv:
        everything(sys.argv[sys.argv.index("--all") + 1])
        sys.exit(0)
    from elasticfusion_amd import api
    if "--kernels" in sys.argv:
        kernels(api, N)
        sys.exit(0)
    e, s = C.c_float(0), C.c_float(0)
    api._chk(api.lib().ef_dev_calibrate(None, C.byref(e), C.byref(s)))
    print(f"ef_dev_calibrate: empty kernel {e.value:.2f} us, 16 MiB copy {s.value:.2f} us per launch: copy rate {2 * 16 * 1048576 / (s.value * 1e-6) / 1e9:.0f} GB/s "
          "(bytes read + bytes written)", flush=True)
    run(api, N)
