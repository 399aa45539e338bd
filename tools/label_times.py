"""Label kernel times: python tools/label_times.py under rocprofv3 --kernel-trace --stats --output-format csv.  640x480 with C = 14 on the
steady bench map (140 replay steps of the bench sequence), 1280x960 with C = 40 on the configs[2] map preseeded with 1 M surfels.  Every
label call runs k_ids_assign and k_labels_align (a full re-alignment of the table); a fuse adds the render pair (index only) and
k_labels_fuse, a label image the render pair and k_labels_gather."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from elasticfusion_amd import api

REPS = 20


def labels(ef, w, h, C, label):
    ef.enableLabels(C)
    n = ef.lastCount()
    p = ef.renderParams(drawUnstable=True)
    probs = api.DevBuf.from_array(np.random.RandomState(1).uniform(0, 1, (C, h, w)).astype(np.float32))
    lab, prob = api.DevBuf(w * h * 4), api.DevBuf(w * h * 4)
    ef.fuseLabelsDevice(probs.p, p)
    ef.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        ef.fuseLabelsDevice(probs.p, p)
    ef.synchronize()
    t1 = time.perf_counter()
    for _ in range(REPS):
        ef.renderLabelsDevice(p, lab.p, prob.p)
    ef.synchronize()
    t2 = time.perf_counter()
    ids, P = ef.labels()
    obs = int((np.abs(P - np.float32(1.0 / C)) > 0).any(1).sum())
    table = n * C * 4
    print(f"{label}: {w}x{h} C={C} surfels {n} rows changed by the fuses {obs} table {table / 1e6:.1f} MB "
          f"(align moves {2 * table / 1e6:.1f} MB + IDs {12 * n / 1e6:.1f} MB) wall/fuse {(t1 - t0) / REPS * 1e6:.1f} us "
          f"wall/label image {(t2 - t1) / REPS * 1e6:.1f} us", flush=True)
    ef.enableLabels(0)


def bench_map():
    seed = 0xEF0001
    frames = bench.replay_frames(seed, 140, 640, 480)
    dev = bench.upload_frames(api, frames)
    ef = api.ElasticFusion()
    for k, (r, d) in enumerate(dev):
        ef.processFrameDevice(r.p.value, d.p.value, k)
    ef.synchronize()
    labels(ef, 640, 480, 14, "bench map")
    ef.close()


def big_map():
    seed = 0xEF0001
    w, h = 1280, 960
    frames = bench.replay_frames(seed, 4, w, h)
    ef = api.ElasticFusion(width=w, height=h, fx=1056.0, fy=1056.0, cx=640.0, cy=480.0)
    n = bench.preseed(ef, seed, w, h, 1 << 20, frames[0])
    dev = bench.upload_frames(api, frames)
    for k, (r, d) in enumerate(dev[1:]):
        ef.processFrameDevice(r.p.value, d.p.value, 2 + k)
    ef.synchronize()
    print("preseeded", n, flush=True)
    labels(ef, w, h, 40, "configs[2] map")
    ef.close()


if __name__ == "__main__":
    bench_map()
    big_map()
