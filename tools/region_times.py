"""Smooth-region times (ef_map_regions_dev / ef_map_regions_select_dev / ef_map_remove_regions; csrc/ef_regions.inc).

    python tools/region_times.py [--size N]    wall clock per call (host clock around work that ends in a synchronise, median of REPS) on the
                                               two synthetic maps of tools/normal_times.py (100 k and 1 M surfels; --size: one of them) at
                                               the default radius, cell and k (index already built): the labels, the BORDERS list, and beside
                                               them on the same map, radius, cell and k the normals' estimate alone (ef_map_normals_dev, no
                                               outputs), the components' labels (ef_map_components_dev) and ef_map_remove_regions itself
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/region_times.py --size N
                                               the same calls on ONE map under the profiler: its kernel trace has the launches' own durations
    python tools/region_times.py --summarise DIR/.../*_kernel_trace.csv N
                                               median, minimum and maximum per kernel from that trace
    python tools/region_times.py --all OUT.txt
                                               the steps above (the traced one once per map) as child processes, each under its own `timeout`,
                                               the next one started only if the one before ended with status 0; writes OUT.txt

Maps: normal_times.surface: a jittered 5 mm lattice on a wavy surface (about 110 surfels within the default 3 cm), stored normals +z, rows
shuffled: every row is a node.  A removal changes the map, so every timed removal is preceded by an (untimed) uploadMap."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from normal_times import SIZES, surface, timed

REPS = 5
REMOVALS = 3
KERNELS = ("k_region_init", "k_region_first", "k_region_hook", "k_region_attach", "k_region_label", "k_region_finish", "k_region_tally", "k_region_split",
           "k_comp_jump", "k_comp_init", "k_comp_first", "k_comp_hook", "k_comp_label", "k_comp_finish", "k_normal_join", "k_select_count", "k_select_rows",
           "k_select_compact", "k_query_count", "k_query_scatter")


def run(api, n):
    S = surface(n)
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    nres = C.sizeof(api.ef_region_result)
    label, size, kind, rows = api.DevBuf(n * 4), api.DevBuf(n * 4), api.DevBuf(n), api.DevBuf(n * 4)
    cnt, res = api.DevBuf(16), api.DevBuf(nres)
    print(f"map of {n} surfels; wall clock per call in us (median of {REPS} after a warm-up; the removal: median of {REMOVALS})", flush=True)
    prm = ef.regionParams()
    nprm = ef.normalParams(radius=prm.radius, cell=prm.cell, k=prm.k, min_neighbors=prm.min_neighbors)
    cprm = ef.componentParams(radius=prm.radius, cell=prm.cell)
    for source, name in ((api.REGIONS_ESTIMATED, "estimated"), (api.REGIONS_STORED, "stored")):
        prm.normal_source = source
        us = timed(ef, lambda: ef.regionsDevice(prm, None, label.p, size.p, kind.p, n, res.p), REPS)
        got = ef._regionResult(api.ef_region_result.from_buffer_copy(res.to_array(np.uint8, nres).tobytes()))
        us_none = timed(ef, lambda: ef.regionsDevice(prm, None, None, None, None, 0), REPS)
        us_sel = timed(ef, lambda: ef.regionSelectDevice(prm, None, api.REGIONS_BORDERS, rows.p, n, cnt.p, res.p), REPS)
        print(f"  n {n} {name:9s} normals: ef_map_regions_dev {us:10.1f}   without outputs {us_none:10.1f}   the BORDERS list {us_sel:10.1f}   {got}", flush=True)
    prm.normal_source = api.REGIONS_ESTIMATED
    us_nrm = timed(ef, lambda: ef.estimateNormalsDevice(nprm, None, None, None, None, None, None, 0), REPS)
    us_cmp = timed(ef, lambda: ef.componentsDevice(cprm, None, None, None, 0), REPS)
    print(f"  n {n} beside them: ef_map_normals_dev (k {nprm.k}, no outputs) {us_nrm:10.1f}   ef_map_components_dev (no outputs) {us_cmp:10.1f}   "
          f"their sum {us_nrm + us_cmp:10.1f}", flush=True)
    t = []
    for _ in range(REMOVALS):
        ef.uploadMap(S)
        ef.regionsDevice(prm, None, None, None, None, 0)                 # the index of the map as it stands, at this cell
        ef.synchronize()
        t0 = time.perf_counter()
        got = ef.removeRegions(prm, what=api.REGIONS_BORDERS)
        t.append((time.perf_counter() - t0) * 1e6)
    print(f"  n {n} ef_map_remove_regions (BORDERS) {float(np.median(t)):10.1f}   {got}", flush=True)
    ef.close()


def summarise(path, name):
    by = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"\b(k_\w+(?:<[^>]*>)?)", r["Kernel_Name"])
        if m and m.group(1).split("<")[0] in KERNELS:
            by.setdefault(m.group(1), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    for k in sorted(by):
        v = np.array([d for _, d in sorted(by[k])]) / 1e3
        print(f"{k:28s} {name:10s} {len(v):6d}  {float(np.median(v)):9.1f} {v.min():9.1f} {v.max():9.1f}")


def everything(out):
    d = out + ".d"
    os.makedirs(d, exist_ok=True)
    me = os.path.join(ROOT, "tools", "region_times.py")
    plain = os.path.join(d, "plain.log")
    steps = [(["timeout", "-k", "10", "300", sys.executable, me], plain)]
    for n in SIZES:                                    # one trace per map: every launch of a trace belongs to that map
        steps.append((["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, f"trace_{n}"),
                       "--", sys.executable, me, "--size", str(n)], os.path.join(d, f"traced_{n}.log")))
    for cmd, log in steps:
        with open(log, "w") as f:
            rc = subprocess.run(cmd, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT).returncode
        print(" ".join(cmd[:6]), "...", "exit", rc, flush=True)
        if rc != 0:                                   # nothing more is started after a step that failed or ran out of time
            print(open(log).read()[-3000:])
            sys.exit(rc)
    keep = lambda p: "".join(ln for ln in open(p) if re.match(r"^(ef_dev|map of|  )", ln))
    summary = "kernel                       map        launches  median us    min us    max us\n"
    for n in SIZES:
        trace = sorted(glob.glob(os.path.join(d, f"trace_{n}", "**", "*_kernel_trace.csv"), recursive=True))[-1]
        summary += subprocess.run([sys.executable, me, "--summarise", trace, str(n)], stdout=subprocess.PIPE, text=True, check=True).stdout
    with open(out, "w") as f:
        f.write("tools/region_times.py on one MI355X, one visit.  Plain run (profiler off): wall clocks and the box's copy rate.\n\n" + keep(plain))
        f.write("\nThe same calls under rocprofv3 --kernel-trace --stats, one run per map (wall clocks that carry the tracer's cost):\n\n"
                + "".join(keep(os.path.join(d, f"traced_{n}.log")) for n in SIZES))
        f.write("\npython tools/region_times.py --summarise <kernel trace> <map>: the launches' own durations\n\n" + summary)
    print(open(out).read())


if __name__ == "__main__":
    if "--summarise" in sys.argv:
        i = sys.argv.index("--summarise")
        summarise(sys.argv[i + 1], sys.argv[i + 2])
        sys.exit(0)
    if "--all" in sys.argv:
        everything(sys.argv[sys.argv.index("--all") + 1])
        sys.exit(0)
    from elasticfusion_amd import api
    e, s = C.c_float(0), C.c_float(0)
    api._chk(api.lib().ef_dev_calibrate(None, C.byref(e), C.byref(s)))
    print(f"ef_dev_calibrate: empty kernel {e.value:.2f} us, 16 MiB copy {s.value:.2f} us per launch: copy rate {2 * 16 * 1048576 / (s.value * 1e-6) / 1e9:.0f} GB/s "
          "(bytes read + bytes written)", flush=True)
    only = int(sys.argv[sys.argv.index("--size") + 1]) if "--size" in sys.argv else None
    for n in SIZES:
        if only in (None, n):
            run(api, n)
