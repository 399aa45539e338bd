"""Render kernel times: python tools/render_times.py under rocprofv3 --kernel-trace --stats --output-format csv.  640x480 and 1920x1080
on the steady bench map (140 replay steps of the bench sequence), 1280x960 on the configs[2] map preseeded with 1 M surfels."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from elasticfusion_amd import api

REPS = 20


def renders(ef, w, h, fx, fy, cx, cy, label):
    p = ef.renderParams(width=w, height=h, fx=fx, fy=fy, cx=cx, cy=cy)
    P = w * h
    outs = dict(rgba=api.DevBuf(P * 4), depth=api.DevBuf(P * 4), vertex=api.DevBuf(P * 16), normal=api.DevBuf(P * 16), index=api.DevBuf(P * 4))
    ef.renderPointCloudDevice(p, **{n: b.p for n, b in outs.items()})
    ef.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        ef.renderPointCloudDevice(p, **{n: b.p for n, b in outs.items()})
    ef.synchronize()
    dt = (time.perf_counter() - t0) / REPS
    idx = outs["index"].to_array(np.uint32, (h, w))
    print(f"{label}: {w}x{h} surfels {ef.lastCount()} drawn px {(idx != 0xFFFFFFFF).mean():.3f} wall/render {dt * 1e6:.1f} us", flush=True)


def bench_map():
    seed = 0xEF0001
    frames = bench.replay_frames(seed, 140, 640, 480)
    dev = bench.upload_frames(api, frames)
    ef = api.ElasticFusion()
    for k, (r, d) in enumerate(dev):
        ef.processFrameDevice(r.p.value, d.p.value, k)
    ef.synchronize()
    renders(ef, 640, 480, 528.0, 528.0, 320.0, 240.0, "bench map")
    renders(ef, 1920, 1080, 1584.0, 1584.0, 960.0, 540.0, "bench map")
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
    renders(ef, w, h, 1056.0, 1056.0, 640.0, 480.0, "configs[2] map")
    ef.close()


if __name__ == "__main__":
    bench_map()
    big_map()
