"""Surface accuracy and completeness of a reconstructed map against the synthetic scene's ground-truth surfels (elasticfusion_amd/accuracy.py):

    python tools/map_accuracy.py [--frames 60] [--width 640 --height 480] [--max-dist 0.05] [--gt 1048576] [--seed 0xEF0001]

runs the box sequence through the engine, samples the scene's surfaces (synth.sample_surfels) and prints, for accuracy (each stable map surfel ->
the nearest ground-truth surfel) and completeness (each ground-truth surfel -> the nearest stable map surfel): mean, median and RMS of the
distance and of the point-to-plane distance, and the share of points without a partner within max_dist.  Every nearest-neighbour search runs on
the device (ef_query_nearest)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--max-dist", type=float, default=0.05)
    ap.add_argument("--gt", type=int, default=1 << 20, help="ground-truth surfels to sample on the scene's surfaces")
    ap.add_argument("--seed", type=lambda v: int(v, 0), default=0xEF0001)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    from elasticfusion_amd import accuracy, api, synth
    seq = synth.Sequence(a.seed, width=a.width, height=a.height)
    ef = api.ElasticFusion(width=a.width, height=a.height, fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)
    for k in range(a.frames):
        rgb, depth, _ = seq.frame(k)
        ef.processFrame(rgb, depth, k)
    rep = accuracy.map_accuracy(ef, synth.sample_surfels(seq, n=a.gt), max_dist=a.max_dist)
    ef.close()
    print(f"{a.frames} frames at {a.width}x{a.height}, {a.gt} ground-truth surfels asked for")
    print(accuracy.format_report(rep))
    if a.json:
        print(json.dumps(rep))


if __name__ == "__main__":
    main()
