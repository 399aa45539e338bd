"""Spatial-query kernel times (ef_query_nearest / ef_query_knn; csrc/ef_query.inc).

    python tools/query_times.py --sweep        wall clock (host clock around work that ends in a synchronise), profiler off: build + 1 M nearest
                                               queries per cell size (1, 2, 4, 8 cm) and lanes per query (1, 8, 16, 64), on both maps
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/query_times.py
                                               the default configuration only: REPS builds, REPS nearest and REPS kNN (k = 8) launches per map
    python tools/query_times.py --summarise DIR/.../*_kernel_trace.csv
                                               medians per kernel and map from that trace (each kernel runs equally often on both maps: the
                                               first half of its launches is the bench map's) and the build's share of the HBM peak

Maps: the steady bench map (140 replay steps of the bench sequence, 640x480) and the configs[2] map (bench.preseed with 1 M surfels, then
three 1280x960 frames).  Queries: 1 M points = map positions (drawn with replacement) jittered by N(0, 5 mm), max_dist 0.02, every surfel."""
import csv
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

REPS = 10
NQ = 1 << 20
MAX_DIST = 0.02
PEAK = 8e12


def bench_map(api, bench):
    frames = bench.replay_frames(0xEF0001, 140, 640, 480)
    dev = bench.upload_frames(api, frames)
    ef = api.ElasticFusion()
    for k, (r, d) in enumerate(dev):
        ef.processFrameDevice(r.p.value, d.p.value, k)
    ef.synchronize()
    return ef


def big_map(api, bench):
    w, h = 1280, 960
    frames = bench.replay_frames(0xEF0001, 4, w, h)
    ef = api.ElasticFusion(width=w, height=h, fx=1056.0, fy=1056.0, cx=640.0, cy=480.0)
    bench.preseed(ef, 0xEF0001, w, h, 1 << 20, frames[0])
    dev = bench.upload_frames(api, frames)
    for k, (r, d) in enumerate(dev[1:]):
        ef.processFrameDevice(r.p.value, d.p.value, 2 + k)
    ef.synchronize()
    return ef


class Setup:
    def __init__(self, api, ef, label):
        self.ef, self.label = ef, label
        S = ef.downloadMap()
        self.n = len(S)
        rng = np.random.default_rng(1)
        pts = (S[rng.integers(0, len(S), NQ), :3].astype(np.float64) + rng.normal(0, 0.005, (NQ, 3))).astype(np.float32)
        self.pts = api.DevBuf.from_array(pts)
        self.row, self.d2, self.plane = api.DevBuf(NQ * 4), api.DevBuf(NQ * 4), api.DevBuf(NQ * 4)
        self.krow, self.kd2, self.kcnt = api.DevBuf(NQ * 8 * 4), api.DevBuf(NQ * 8 * 4), api.DevBuf(NQ * 4)

    def nearest(self):
        self.ef.queryNearestDevice(self.pts.p, NQ, MAX_DIST, -1.0, row=self.row.p, dist2=self.d2.p, plane=self.plane.p)

    def knn(self):
        self.ef.queryKnnDevice(self.pts.p, NQ, 8, MAX_DIST, -1.0, rows=self.krow.p, dist2=self.kd2.p, count=self.kcnt.p)

    def rebuild(self, cell, i):
        self.ef.setQueryCell(cell * (1.0 + 1e-6 * (i & 1)))   # another cell size: the next query rebuilds the index

    def hits(self):
        return int((self.row.to_array(np.uint32, NQ) != 0xFFFFFFFF).sum())


def sweep(setups):
    for s in setups:
        print(f"{s.label}: {s.n} surfels, {NQ} queries, max_dist {MAX_DIST}; wall clock per call in us (median of {REPS}; build+nearest includes "
              f"one read of the map count)", flush=True)
        print("  cell_m  lanes  build+nearest    nearest  knn(k=8)  hits", flush=True)
        for cell in (0.01, 0.02, 0.04, 0.08):
            for lanes in (1, 8, 16, 64):
                s.ef.debugQueryLanes(lanes)
                s.rebuild(cell, 1)
                s.nearest()
                s.ef.synchronize()   # warm-up of this shape
                tb, tq, tk = [], [], []
                for i in range(REPS):
                    s.rebuild(cell, i)
                    t0 = time.perf_counter()
                    s.nearest()
                    s.ef.synchronize()
                    tb.append(time.perf_counter() - t0)
                for i in range(REPS):
                    t0 = time.perf_counter()
                    s.nearest()
                    s.ef.synchronize()
                    tq.append(time.perf_counter() - t0)
                if lanes in (1, 8):
                    s.knn()
                    s.ef.synchronize()
                    for i in range(REPS):
                        t0 = time.perf_counter()
                        s.knn()
                        s.ef.synchronize()
                        tk.append(time.perf_counter() - t0)
                med = lambda v: float(np.median(v)) * 1e6 if v else float("nan")
                print(f"  {cell:6.3f}  {lanes:5d}  {med(tb):13.1f}  {med(tq):9.1f}  {med(tk):8.1f}  {s.hits()}", flush=True)
        s.ef.debugQueryLanes(0)


def trace(setups):
    from elasticfusion_amd import api
    cell = api.ElasticFusion.QUERY_DEFAULT_CELL
    for s in setups:
        s.rebuild(cell, 1)
        s.nearest()
        s.knn()
        s.ef.synchronize()
        for i in range(REPS):
            s.rebuild(cell, i)
            s.nearest()
            s.knn()
        s.ef.synchronize()
        print(f"{s.label}: {s.n} surfels, cell {cell}, {REPS + 1} builds / nearest / kNN launches, hits {s.hits()}", flush=True)


def summarise(path):
    rows = list(csv.DictReader(open(path)))
    by = {}
    for r in rows:
        name = r["Kernel_Name"]
        if "k_query" not in name and "k_scan_chunks" not in name:
            continue
        short = re.search(r"(k_query(?:_[a-z]+)?(?:<[^>]*>)?|k_scan_chunks)", name).group(1)
        by.setdefault(short, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    print("kernel                      launches   bench map (us)   configs[2] map (us)   (medians)")
    out = {}
    for name in sorted(by):
        v = [d for _, d in sorted(by[name])]
        if name == "k_scan_chunks":   # also a frame kernel: the query's launches are the last ones of each map (one per build)
            v = v[-2 * (REPS + 1):] if len(v) >= 2 * (REPS + 1) else v
        h = len(v) // 2
        a, b = float(np.median(v[:h])) / 1e3, float(np.median(v[h:])) / 1e3
        out[name] = (a, b)
        print(f"{name:26s}  {len(v):8d}   {a:14.1f}   {b:19.1f}")
    return out


if __name__ == "__main__":
    if "--summarise" in sys.argv:
        summarise(sys.argv[sys.argv.index("--summarise") + 1])
        sys.exit(0)
    import bench
    from elasticfusion_amd import api
    setups = []
    for make, label in ((bench_map, "bench map"), (big_map, "configs[2] map")):
        ef = make(api, bench)
        setups.append(Setup(api, ef, label))
    (sweep if "--sweep" in sys.argv else trace)(setups)
    for s in setups:
        s.ef.close()
