"""Boundary-estimation times (ef_map_boundaries_dev / ef_map_boundaries_select_dev; csrc/ef_boundary.inc).

    python tools/boundary_times.py             wall clock per call (host clock around work that ends in a synchronise, median of REPS) on a
                                               synthetic map of 1 M surfels at the defaults (radius = cell = 3 cm, k 12): the whole
                                               ef_map_boundaries_dev with and without its output arrays, with stored and with estimated
                                               normals, the BOUNDARY list, and beside them ef_map_normals_dev without outputs (the normals'
                                               join alone, the same walk at the same radius, cell and k) and ef_map_components_dev of the
                                               whole map (the union-find the loops run on the BOUNDARY rows only)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/boundary_times.py
                                               the same run under the profiler: its kernel trace has the launches' own durations
    python tools/boundary_times.py --summarise DIR/.../*_kernel_trace.csv
                                               median, minimum and maximum per kernel from that trace
    python tools/boundary_times.py --all OUT.txt
                                               the three steps above as child processes, each under its own `timeout`, the next one started
                                               only if the one before ended with status 0; writes OUT.txt (profiles/r33_boundary_times.txt)

Map: a jittered 5 mm lattice on a wavy surface (about 110 surfels within the default 3 cm), stored normals +z, with a lattice of round holes of
10 cm diameter cut out: the sheet's rim and every hole are loops."""
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
N = 1_000_000
KERNELS = ("k_boundary_join", "k_boundary_flags", "k_boundary_tally", "k_boundary_result", "k_boundary_split", "k_normal_join", "k_comp_init",
           "k_comp_first", "k_comp_jump", "k_comp_hook", "k_comp_label", "k_comp_finish", "k_select_count", "k_select_rows")


def surface(n, pitch=0.005, seed=1):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    x = (i % side + rng.uniform(-0.3, 0.3, n)) * pitch
    y = (i // side + rng.uniform(-0.3, 0.3, n)) * pitch
    S = np.zeros((n, 12), np.float32)
    S[:, 0], S[:, 1], S[:, 2] = x, y, 1.0 + 0.05 * np.sin(3.0 * x) * np.cos(2.0 * y) + rng.normal(0.0, 0.0005, n)
    S[:, 3], S[:, 4], S[:, 6], S[:, 7], S[:, 10], S[:, 11] = 20.0, float(0x808080), 1, 2, 1.0, 0.004
    hole = np.hypot((x + 0.25) % 0.5 - 0.25, (y + 0.25) % 0.5 - 0.25) < 0.05      # a hole every half metre
    S = S[~hole]
    return S[rng.permutation(len(S))]


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
    n = len(S)
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    out = {k: api.DevBuf(n * w) for k, w in (("gap", 4), ("count", 4), ("status", 1), ("label", 4), ("size", 4), ("rows", 4))}
    cnt, res = api.DevBuf(16), api.DevBuf(C.sizeof(api.ef_boundary_result))
    print(f"map of {n} surfels; wall clock per call in us (median of {REPS} after a warm-up)", flush=True)
    for src, name in ((api.BOUNDARY_STORED, "stored normals"), (api.BOUNDARY_ESTIMATED, "estimated normals")):
        prm = ef.boundaryParams(normal_source=src)
        us = timed(ef, lambda: ef.boundariesDevice(prm, None, out["gap"].p, out["count"].p, out["status"].p, out["label"].p, out["size"].p, n, res.p), REPS)
        us_bare = timed(ef, lambda: ef.boundariesDevice(prm, None, None, None, None, None, None, 0, res.p), REPS)
        us_sel = timed(ef, lambda: ef.boundarySelectDevice(prm, None, api.BOUNDARY_BOUNDARY, out["rows"].p, n, cnt.p, res.p), REPS)
        r = ef._boundaryResult(api.ef_boundary_result.from_buffer_copy(res.to_array(np.uint8, C.sizeof(api.ef_boundary_result)).tobytes()))
        print(f"  {name:17s}: ef_map_boundaries_dev {us:10.1f}   without outputs {us_bare:10.1f}   the BOUNDARY list {us_sel:10.1f}   {r}", flush=True)
    nprm = ef.normalParams(radius=prm.radius, cell=prm.cell, k=prm.k, min_neighbors=prm.min_neighbors)
    us_nrm = timed(ef, lambda: ef.estimateNormalsDevice(nprm, None, None, None, None, None, None, 0), REPS)
    cprm = ef.componentParams(radius=prm.radius, cell=prm.cell, min_size=1)
    us_comp = timed(ef, lambda: ef.componentsDevice(cprm, None, None, None, 0), REPS)
    print(f"  beside them      : ef_map_normals_dev without outputs (its join alone) {us_nrm:10.1f}   ef_map_components_dev of the whole map {us_comp:10.1f}", flush=True)
    ef.close()


def summarise(path):
    by = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"\b(k_\w+(?:<[^>]*>)?)", r["Kernel_Name"])
        if m and m.group(1).split("<")[0] in KERNELS:
            by.setdefault(m.group(1), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    print("kernel                                   launches  median us    min us    max us   sum ms")
    for name in sorted(by):
        v = np.array(by[name]) / 1e3
        print(f"{name:40s} {len(v):6d}  {float(np.median(v)):9.1f} {v.min():9.1f} {v.max():9.1f} {v.sum() / 1e3:8.2f}")


def everything(out):
    d = out + ".d"
    os.makedirs(d, exist_ok=True)
    me = os.path.join(ROOT, "tools", "boundary_times.py")
    plain, traced = os.path.join(d, "plain.log"), os.path.join(d, "traced.log")
    steps = [(["timeout", "-k", "10", "180", sys.executable, me], plain),
             (["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "trace"), "--",
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
        f.write("tools/boundary_times.py on one MI355X, one visit.  Plain run (profiler off): wall clocks and the box's copy rate.\n\n" + keep(plain))
        f.write("\nThe same run under rocprofv3 --kernel-trace --stats (wall clocks that carry the tracer's cost):\n\n" + keep(traced))
        f.write("\npython tools/boundary_times.py --summarise <kernel trace>: the launches' own durations over that whole run\n\n" + summary)
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
    run(api, N)
