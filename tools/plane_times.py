"""Plane-segmentation times (ef_map_planes_dev / ef_map_planes_select_dev; csrc/ef_planes.inc).

    python tools/plane_times.py [--rows 100000,1000000]
                                               wall clock per call (host clock around work that ends in a synchronise, median of REPS) on
                                               synthetic rooms of 100 k and 1 M surfels (uploadMap): the whole extraction (max_planes 4)
                                               at H = 256 / 1024, refine on / off, normal_cos on / off, and the ON list of all planes
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/plane_times.py --single
                                               ONE round per call (max_planes 1, refine 1) for every (rows, H, normal_cos) under the
                                               profiler, 1 + REPS calls each, in a fixed order: every launch of the scoring kernel in the
                                               trace then scores exactly rows x H pairs
    python tools/plane_times.py --summarise DIR/.../*_kernel_trace.csv
                                               median, minimum and maximum per kernel and configuration from that trace, and the scoring
                                               kernel's pairs per second; an unexpected number of launches is an error
    python tools/plane_times.py --all OUT.txt
                                               the steps above as child processes, each under its own `timeout`, the next one started only
                                               if the one before ended with status 0; writes OUT.txt

The room: 40 % of the rows on a floor, 25 % and 15 % on two walls, 20 % clutter in the volume; 2 mm of noise on the surfaces; rows shuffled."""
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
ROWS = (100_000, 1_000_000)
HS = (256, 1024)
COS = (0.0, 0.9)
KERNELS = ("k_plane_init", "k_plane_part", "k_scan_chunks", "k_plane_compact", "k_plane_hyp", "k_plane_score", "k_plane_pick", "k_plane_moments",
           "k_plane_fit", "k_plane_mark", "k_plane_flags", "k_plane_tally", "k_plane_split", "k_select_count", "k_select_rows")


def room(n, seed=1):
    rng = np.random.default_rng(seed)
    k = [int(0.40 * n), int(0.25 * n), int(0.15 * n)]
    k.append(n - sum(k))
    noise = lambda m: np.clip(rng.normal(0.0, 0.002, m), -0.004, 0.004)
    floor = np.stack([rng.uniform(0, 4, k[0]), rng.uniform(0, 4, k[0]), noise(k[0])], 1)
    wall_a = np.stack([noise(k[1]), rng.uniform(0, 4, k[1]), rng.uniform(0, 2.5, k[1])], 1)
    wall_b = np.stack([rng.uniform(0, 4, k[2]), noise(k[2]), rng.uniform(0, 2.5, k[2])], 1)
    clutter = rng.uniform([0.1, 0.1, 0.05], [4, 4, 2.5], (k[3], 3))
    nrm = np.concatenate([np.tile([0, 0, 1.0], (k[0], 1)), np.tile([1.0, 0, 0], (k[1], 1)), np.tile([0, 1.0, 0], (k[2], 1)), rng.normal(size=(k[3], 3))])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    S = np.zeros((n, 12), np.float32)
    S[:, :3] = np.concatenate([floor, wall_a, wall_b, clutter])
    S[:, 3], S[:, 4], S[:, 6], S[:, 7], S[:, 11] = 20.0, 0x808080, 1, 2, 0.004
    S[:, 8:11] = nrm
    return S[rng.permutation(n)]


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


def run(api, rows, single):
    for n in rows:
        ef = api.ElasticFusion()
        ef.uploadMap(room(n))
        nres, nmod = C.sizeof(api.ef_plane_result), C.sizeof(api.ef_plane_model) * api.PLANE_MAX_PLANES
        d_rows, d_cnt, d_res, d_mod = api.DevBuf(n * 4), api.DevBuf(16), api.DevBuf(nres), api.DevBuf(nmod)
        result = lambda: ef._planeResult(api.ef_plane_result.from_buffer_copy(d_res.to_array(np.uint8, nres).tobytes()))
        print(f"room of {n} surfels; wall clock per call in us (median of {REPS} after a warm-up)", flush=True)
        for H in HS:
            for cos in COS:
                if single:
                    prm = ef.planeParams(hypotheses=H, normal_cos=cos, max_planes=1, refine=1, min_inliers=n // 50, seed=7)
                    us = timed(ef, lambda: ef.planesDevice(prm, None, None, 0, d_mod.p, d_res.p))
                    print(f"  H {H:4d} normal_cos {cos:.1f} one round: {us:10.1f}   {result()}", flush=True)
                    continue
                for refine in (1, 0):
                    prm = ef.planeParams(hypotheses=H, normal_cos=cos, max_planes=4, refine=refine, min_inliers=n // 50, seed=7)
                    us = timed(ef, lambda: ef.planesDevice(prm, None, None, 0, d_mod.p, d_res.p))
                    got = result()
                    us_list = timed(ef, lambda: ef.planeSelectDevice(prm, None, api.PLANES_ON, -1, d_rows.p, n, d_cnt.p, d_mod.p, d_res.p))
                    print(f"  H {H:4d} normal_cos {cos:.1f} refine {refine}: the extraction {us:10.1f}   the ON list {us_list:10.1f}   {got}", flush=True)
        ef.close()


def summarise(path):
    """the trace of a --single run: per configuration 1 + REPS calls, so 1 + REPS launches of every per-round kernel, in the order of run()"""
    by = {}
    for r in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                by.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    configs = [(n, H, cos) for n in ROWS for H in HS for cos in COS]
    per = 1 + REPS
    for k in ("k_plane_score", "k_plane_hyp", "k_plane_pick", "k_plane_moments", "k_plane_fit", "k_plane_mark", "k_plane_part", "k_plane_compact"):
        if len(by.get(k, [])) != per * len(configs):
            sys.exit(f"{path}: {len(by.get(k, []))} launches of {k}, expected {per * len(configs)}: the run is not the one this summary was written for")
    print("kernel             rows      H  cos  launches  median us    min us    max us")
    for k in KERNELS:
        v = np.array([d for _, d in sorted(by.get(k, []))]) / 1e3
        if len(v) != per * len(configs):
            if len(v):
                print(f"{k:18s} (all configurations)  {len(v):6d}  {float(np.median(v)):9.1f} {v.min():9.1f} {v.max():9.1f}")
            continue
        for i, (n, H, cos) in enumerate(configs):
            g = v[i * per:(i + 1) * per]
            extra = f"   {n * H / (float(np.median(g)) * 1e-6):.3e} pairs/s" if k == "k_plane_score" else ""
            print(f"{k:18s} {n:8d} {H:5d} {cos:4.1f}  {len(g):6d}  {float(np.median(g)):9.1f} {g.min():9.1f} {g.max():9.1f}{extra}")


def everything(out):
    d = out + ".d"
    os.makedirs(d, exist_ok=True)
    me = os.path.join(ROOT, "tools", "plane_times.py")
    plain, traced = os.path.join(d, "plain.log"), os.path.join(d, "traced.log")
    steps = [(["timeout", "-k", "10", "240", sys.executable, me], plain),
             (["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "trace"), "--",
               sys.executable, me, "--single"], traced)]
    for cmd, log in steps:
        with open(log, "w") as f:
            rc = subprocess.run(cmd, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT).returncode
        print(" ".join(cmd[:6]), "...", "exit", rc, flush=True)
        if rc != 0:                                   # nothing more is started after a step that failed or ran out of time
            print(open(log).read()[-3000:])
            sys.exit(rc)
    keep = lambda p: "".join(ln for ln in open(p) if re.match(r"^(ef_dev|room|  )", ln))
    trace = sorted(glob.glob(os.path.join(d, "trace", "**", "*_kernel_trace.csv"), recursive=True))[-1]
    summary = subprocess.run([sys.executable, me, "--summarise", trace], stdout=subprocess.PIPE, text=True, check=True).stdout
    with open(out, "w") as f:
        f.write("tools/plane_times.py on one MI355X, one visit.  Plain run (profiler off): wall clocks and the box's copy rate.\n\n" + keep(plain))
        f.write("\nOne round per call under rocprofv3 --kernel-trace --stats (wall clocks that carry the tracer's cost):\n\n" + keep(traced))
        f.write("\npython tools/plane_times.py --summarise <kernel trace>: the launches' own durations\n\n" + summary)
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
    rows = tuple(int(v) for v in sys.argv[sys.argv.index("--rows") + 1].split(",")) if "--rows" in sys.argv else ROWS
    run(api, rows, "--single" in sys.argv)
