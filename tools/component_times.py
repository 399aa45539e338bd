"""Connected-component times (ef_map_components_select / ef_map_remove_components; csrc/ef_components.inc).

    python tools/component_times.py [--no-composed] [--map bench|big]
                                               wall clock per call (host clock around work that ends in a synchronise, median of REPS) on
                                               the bench map and the configs[2] map: the rejected list with default parameters at cell =
                                               radius / 2, radius and 2 radius (index already built at that cell), the labels alone, the
                                               outliers' join (k = 8) at cell = radius beside them, ef_map_remove_components itself, and the
                                               path it replaces: downloadMap + ef_query_knn (k = 16) on the map's own positions + a host
                                               union-find + ef_map_erase_rows
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/component_times.py --no-composed --map bench
                                               the same calls on ONE map under the profiler: its kernel trace has the launches' own
                                               durations, and every launch in it belongs to that map
    python tools/component_times.py --summarise DIR/.../*_kernel_trace.csv "bench map"
                                               median, minimum and maximum per kernel from that trace; an unexpected number of launches
                                               of the hook or of the outliers' join is an error
    python tools/component_times.py --all OUT.txt
                                               the steps above (the traced one once per map) as child processes, each under its own `timeout`, the next one started
                                               only if the one before ended with status 0; writes OUT.txt (profiles/r28_component_times.txt)

Maps: the steady bench map (140 replay steps of the bench sequence, 640x480) and the configs[2] map (bench.preseed with 1 M surfels, then
three 1280x960 frames).  A removal changes the map, so every timed removal is preceded by an (untimed) uploadMap of the saved map.  min_size
is MIN_SIZE for every call, so that something is removed on both maps."""
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
MIN_SIZE = 50
KERNELS = ("k_comp_init", "k_comp_first", "k_comp_jump", "k_comp_hook", "k_comp_label", "k_comp_finish", "k_comp_tally", "k_comp_split", "k_outlier_join", "k_select_count",
           "k_select_rows", "k_select_compact", "k_query_count", "k_query_scatter")


def host_components(n, s, t):
    """label per row (the smallest row of its set) of the graph with the edges (s[i], t[i]): scipy's connected components where it is
    installed, else minimum propagation with pointer jumping in numpy"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        _, comp = connected_components(coo_matrix((np.ones(len(s), np.int8), (s, t)), shape=(n, n)), directed=False)
        low = np.full(comp.max() + 1 if n else 0, n, np.int64)
        np.minimum.at(low, comp, np.arange(n))
        return low[comp]
    except ImportError:
        label = np.arange(n)
        while True:
            new = label.copy()
            np.minimum.at(new, s, label[t])
            np.minimum.at(new, t, label[s])
            new = new[new]
            if np.array_equal(new, label):
                return label
            label = new


def composed(ef, prm):
    """the path a user composes without the feature; returns (rejected rows, seconds of [download, query, union-find, erase]).  k = 16 is the
    query's limit: a surfel with more than 15 neighbours within the radius loses edges, so this can split what the device call joins"""
    t0 = time.perf_counter()
    m = ef.downloadMap()
    t1 = time.perf_counter()
    rows, d2, count = ef.queryKnn(m[:, :3], 16, prm.radius, prm.min_conf)
    t2 = time.perf_counter()
    n = len(m)
    s = np.repeat(np.arange(n), 16)
    t = rows.reshape(-1).astype(np.int64)
    keep = (t != 0xFFFFFFFF) & (t != s)
    node = np.isfinite(m[:, :3]).all(1) & (m[:, 3] > prm.min_conf)
    keep &= node[s]
    label = host_components(n, s[keep], t[keep])
    size = np.bincount(label[node], minlength=n)[label]
    out = np.nonzero(node & ((size < prm.min_size) | ((prm.max_size != 0) & (size > prm.max_size))))[0].astype(np.uint32)
    t3 = time.perf_counter()
    ef.eraseRows(out)
    t4 = time.perf_counter()
    return out, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)


def run(api, ef, label, with_composed):
    S = ef.downloadMap()
    n = len(S)
    nres = C.sizeof(api.ef_component_result)
    rows, cnt, res = api.DevBuf(n * 4), api.DevBuf(16), api.DevBuf(nres)
    print(f"{label}: {n} surfels; wall clock per call in us (median of {REPS} after a warm-up; removals and the composed path: median of {REMOVALS})",
          flush=True)
    radius = ef.componentParams().radius
    for cell in (radius / 2, radius, 2 * radius):
        prm = ef.componentParams(cell=cell, min_size=MIN_SIZE)
        us = timed(ef, lambda: ef.componentSelectDevice(prm, None, api.COMPONENTS_REJECTED, rows.p, n, cnt.p, res.p), REPS)
        k = int(cnt.to_array(np.uint32, 1)[0])
        got = ef._componentResult(api.ef_component_result.from_buffer_copy(res.to_array(np.uint8, nres).tobytes()))
        us_lab = timed(ef, lambda: ef.componentsDevice(prm, None, None, None, 0), REPS)
        print(f"  cell {cell:.3f} m: rejected list {us:10.1f}   the labels alone {us_lab:10.1f}   rejected {k}   {got}", flush=True)
    prm = ef.componentParams(min_size=MIN_SIZE)
    oprm = ef.outlierParams(radius=prm.radius, cell=prm.cell, k=8)
    us_join = timed(ef, lambda: ef.neighborStatsDevice(oprm, None, None, None, 0), REPS)
    print(f"  the outliers' join (k_outlier_join<8>) at cell {prm.cell:.3f}, the same radius: {us_join:10.1f}", flush=True)
    t_fused = []
    for _ in range(REMOVALS):
        ef.uploadMap(S)
        ef.componentSelectDevice(prm, None, api.COMPONENTS_REJECTED, None, 0, cnt.p)          # the index of the map as it stands, at this cell
        ef.synchronize()
        t0 = time.perf_counter()
        got = ef.removeComponents(prm)
        t_fused.append((time.perf_counter() - t0) * 1e6)
    fused = float(np.median(t_fused))
    print(f"  ef_map_remove_components {fused:10.1f}   removed {got['rejected_rows']} of {n} in {got['rejected_components']} of {got['components']} "
          f"components, largest {got['largest']}", flush=True)
    if with_composed:
        parts = []
        for _ in range(REMOVALS):
            ef.uploadMap(S)
            ef.queryKnn(S[:8, :3], 2, prm.radius)                  # the index of the map as it stands, at this cell
            ef.synchronize()
            out, t = composed(ef, prm)
            parts.append(t)
        p = np.median(np.array(parts), 0) * 1e6
        print(f"  the composed path: downloadMap {p[0]:10.1f} + ef_query_knn k=16 {p[1]:10.1f} + host union-find {p[2]:10.1f} + ef_map_erase_rows "
              f"{p[3]:10.1f} = {p.sum():10.1f} us; removed {len(out)}; fused / composed = {fused / p.sum():.4f}", flush=True)
    ef.uploadMap(S)


def summarise(path, name):
    """path: the kernel trace of a run over ONE map (--map), so that no launch can be attributed to the other; the hook's launches are cut
    into the three cells by their count, and a count that is not the expected one is an error, not a guess"""
    by = {}
    for r in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                by.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    per_cell = 2 * (1 + REPS)             # the hook's launches per cell: the lists and the labels, a warm-up each
    want = {"k_comp_hook": 3 * per_cell + 2 * REMOVALS, "k_outlier_join": 1 + REPS}
    for k, w in want.items():
        if len(by.get(k, [])) != w:
            sys.exit(f"{path}: {len(by.get(k, []))} launches of {k}, expected {w}: the run is not the one this summary was written for")
    for k in KERNELS:
        v = np.array([d for _, d in sorted(by.get(k, []))]) / 1e3
        if not len(v):
            continue
        groups = [(name, v)]
        if k == "k_comp_hook":
            groups = [(f"{name}, cell {c}", v[i * per_cell:(i + 1) * per_cell]) for i, c in enumerate(("r/2", "r", "2r"))]
            groups.append((f"{name}, removals (cell r)", v[3 * per_cell:]))
        for label, g in groups:
            print(f"{k:20s} {label:36s} {len(g):6d}  {float(np.median(g)):9.1f} {g.min():9.1f} {g.max():9.1f}")


MAPS = (("bench", "bench map"), ("big", "configs[2] map"))


def everything(out):
    d = out + ".d"
    os.makedirs(d, exist_ok=True)
    me = os.path.join(ROOT, "tools", "component_times.py")
    plain = os.path.join(d, "plain.log")
    steps = [(["timeout", "-k", "10", "420", sys.executable, me], plain)]
    for key, _ in MAPS:                                # one trace per map: every launch of a trace belongs to that map
        steps.append((["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "trace_" + key),
                       "--", sys.executable, me, "--no-composed", "--map", key], os.path.join(d, f"traced_{key}.log")))
    for cmd, log in steps:
        with open(log, "w") as f:
            rc = subprocess.run(cmd, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT).returncode
        print(" ".join(cmd[:6]), "...", "exit", rc, flush=True)
        if rc != 0:                                   # nothing more is started after a step that failed or ran out of time
            print(open(log).read()[-3000:])
            sys.exit(rc)
    keep = lambda p: "".join(ln for ln in open(p) if re.match(r"^(ef_dev|bench|configs|  )", ln))
    summary = "kernel               map                                  launches  median us    min us    max us\n"
    for key, name in MAPS:
        trace = sorted(glob.glob(os.path.join(d, "trace_" + key, "**", "*_kernel_trace.csv"), recursive=True))[-1]
        summary += subprocess.run([sys.executable, me, "--summarise", trace, name], stdout=subprocess.PIPE, text=True, check=True).stdout
    with open(out, "w") as f:
        f.write("tools/component_times.py on one MI355X, one visit.  Plain run (profiler off): wall clocks and the box's copy rate.\n\n" + keep(plain))
        f.write("\nThe same calls under rocprofv3 --kernel-trace --stats, one run per map (wall clocks that carry the tracer's cost; without the composed path):\n\n"
                + "".join(keep(os.path.join(d, f"traced_{key}.log")) for key, _ in MAPS))
        f.write("\npython tools/component_times.py --summarise <kernel trace> <map>: the launches' own durations\n\n" + summary)
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
    only = sys.argv[sys.argv.index("--map") + 1] if "--map" in sys.argv else None
    for make, (key, label) in zip((bench_map, big_map), MAPS):
        if only not in (None, key):
            continue
        ef, last = make(api, bench)
        run(api, ef, label, "--no-composed" not in sys.argv)
        ef.close()
