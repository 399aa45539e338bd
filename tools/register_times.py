"""Registration kernel times (ef_register_step / ef_register_cloud; csrc/ef_register.inc) beside the nearest-surfel query on the same points.

    python tools/register_times.py             wall clock (host clock around calls that end in a synchronise), profiler off: one step at 100 k
                                               and 1 M points on both maps beside ef_query_nearest_dev on the transformed points, and a
                                               whole registration (iterations, wall time)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/register_times.py --trace
                                               REPS + 1 queries and REPS + 1 steps per size and map
    python tools/register_times.py --summarise DIR/.../*_kernel_trace.csv
                                               medians per kernel, size and map from that trace

Maps: those of tools/query_times.py (the steady bench map, the configs[2] map).  Cloud: map positions (drawn with replacement) jittered by
N(0, 2 mm) and moved by the inverse of a 2.7 cm / 1.3 degree motion, so that a registration has something to recover; max_dist 0.05, every
surfel, no normals.  The query is the floor of a step: the step does the query's work plus the transform and the sums."""
import csv
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

REPS = 10
SIZES = (100000, 1000000)
MAX_DIST = 0.05
TWIST = np.array([0.02, -0.015, 0.01, 0.017, -0.01, 0.012])


def motion():
    """exp of TWIST (Rodrigues), float64"""
    v, w = TWIST[:3], TWIST[3:]
    th = float(np.linalg.norm(w))
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W
    V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = R, V @ v
    return G


class Setup:
    def __init__(self, api, ef, label):
        self.ef, self.label = ef, label
        S = ef.downloadMap()
        self.n = len(S)
        rng = np.random.default_rng(1)
        nq = max(SIZES)
        world = S[rng.integers(0, len(S), nq), :3].astype(np.float64) + rng.normal(0, 0.002, (nq, 3))
        self.G = motion()
        Gi = np.linalg.inv(self.G)
        self.world = api.DevBuf.from_array(world.astype(np.float32))                            # what the query is asked
        self.cloud = api.DevBuf.from_array((world @ Gi[:3, :3].T + Gi[:3, 3]).astype(np.float32))   # what the step is given, with T = G
        self.row, self.plane = api.DevBuf(nq * 4), api.DevBuf(nq * 4)
        self.params = ef.registerParams(max_dist=MAX_DIST, min_conf=-1.0)

    def query(self, n):
        self.ef.queryNearestDevice(self.world.p, n, MAX_DIST, -1.0, row=self.row.p, plane=self.plane.p)

    def step(self, n, outputs=False):
        return self.ef.registerStepDevice(self.cloud.p, n, T=self.G, params=self.params, row=self.row.p if outputs else None,
                                          plane=self.plane.p if outputs else None)

    def cloud_run(self, n):
        return self.ef.registerCloudDevice(self.cloud.p, n, params=self.params)


def med_us(fn, sync):
    fn()
    sync()
    v = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        sync()
        v.append(time.perf_counter() - t0)
    return float(np.median(v)) * 1e6


def wall(setups):
    for s in setups:
        print(f"{s.label}: {s.n} surfels, max_dist {MAX_DIST}; wall clock per call in us (median of {REPS}), each call ends in a synchronise", flush=True)
        print("   points      query       step  step+row,plane   pairs", flush=True)
        for n in SIZES:
            q = med_us(lambda: s.query(n), s.ef.synchronize)
            st = med_us(lambda: s.step(n), s.ef.synchronize)
            so = med_us(lambda: s.step(n, True), s.ef.synchronize)
            print(f"  {n:8d}  {q:9.1f}  {st:9.1f}  {so:14.1f}  {s.step(n)['pairs']:7d}", flush=True)
        for n in SIZES:
            s.cloud_run(n)
            v = []
            for _ in range(5):
                t0 = time.perf_counter()
                T, res = s.cloud_run(n)
                v.append(time.perf_counter() - t0)
            d = T @ np.linalg.inv(s.G)
            print(f"  registration of {n} points from the identity: {res['status_name']} after {res['iterations']} updates "
                  f"({res['iterations'] + 1} steps), {res['pairs']} pairs, rms {res['rms_first'] * 1e3:.3f} -> {res['rms_last'] * 1e3:.3f} mm, "
                  f"pose off by {np.linalg.norm(d[:3, 3]) * 1e3:.4f} mm; wall {float(np.median(v)) * 1e3:.3f} ms", flush=True)


def trace(setups):
    for s in setups:
        for n in SIZES:
            for _ in range(REPS + 1):
                s.query(n)
            s.ef.synchronize()
            for _ in range(REPS + 1):
                s.step(n)
        print(f"{s.label}: {s.n} surfels, {REPS + 1} queries and steps at each of {SIZES}", flush=True)


def summarise(path):
    rows = list(csv.DictReader(open(path)))
    by = {}
    for r in rows:
        m = re.search(r"(k_register_reduce|k_register(?:<[^>]*>)?|k_query<[^>]*>)", r["Kernel_Name"])
        if m:
            by.setdefault(m.group(1), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    per = REPS + 1
    print(f"kernel times in us, medians of {per} launches; columns: bench map 100 k, 1 M points, configs[2] map 100 k, 1 M points")
    for name in sorted(by):
        v = [d for _, d in sorted(by[name])]
        groups = [v[i * per:(i + 1) * per] for i in range(len(v) // per)]
        print(f"{name:24s} launches {len(v):5d}   " + "   ".join(f"{float(np.median(g)) / 1e3:9.1f}" for g in groups))


if __name__ == "__main__":
    if "--summarise" in sys.argv:
        summarise(sys.argv[sys.argv.index("--summarise") + 1])
        sys.exit(0)
    import bench
    import query_times
    from elasticfusion_amd import api
    setups = [Setup(api, make(api, bench), label) for make, label in ((query_times.bench_map, "bench map"), (query_times.big_map, "configs[2] map"))]
    (trace if "--trace" in sys.argv else wall)(setups)
    for s in setups:
        s.ef.close()
