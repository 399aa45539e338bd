"""Surface accuracy and completeness of a reconstructed map against the synthetic scene's ground-truth surfels (elasticfusion_amd/accuracy.py):

    python tools/map_accuracy.py [--frames 60] [--width 640 --height 480] [--max-dist 0.05] [--gt 1048576] [--seed 0xEF0001]
                                 [--align [--perturb TX,TY,TZ,RX,RY,RZ]]

runs the box sequence through the engine, samples the scene's surfaces (synth.sample_surfels) and prints, for accuracy (each stable map surfel ->
the nearest ground-truth surfel) and completeness (each ground-truth surfel -> the nearest stable map surfel): mean, median and RMS of the
distance and of the point-to-plane distance, and the share of points without a partner within max_dist.  Every nearest-neighbour search runs on
the device (ef_query_nearest).

--align first registers the ground truth to the map (point-to-plane ICP on the device, ef_register_cloud through accuracy.register_to_map), as
one does with a model that is not in the map's frame; --perturb moves the ground truth by the inverse of a known twist (metres, radians) before
that, and the motion that was recovered is printed beside it."""
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
    ap.add_argument("--align", action="store_true", help="register the ground truth to the map before the figures are taken")
    ap.add_argument("--perturb", type=lambda v: [float(x) for x in v.split(",")], default=None,
                    help="TX,TY,TZ,RX,RY,RZ: move the ground truth by the inverse of this twist first (needs --align to be undone)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    from elasticfusion_amd import accuracy, api, synth
    seq = synth.Sequence(a.seed, width=a.width, height=a.height)
    ef = api.ElasticFusion(width=a.width, height=a.height, fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)
    for k in range(a.frames):
        rgb, depth, _ = seq.frame(k)
        ef.processFrame(rgb, depth, k)
    gt = synth.sample_surfels(seq, n=a.gt)
    G = None
    if a.perturb is not None:
        import numpy as np
        from scipy.linalg import expm
        assert len(a.perturb) == 6, "--perturb takes six numbers"
        v, w = a.perturb[:3], a.perturb[3:]
        M = np.zeros((4, 4))
        M[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
        M[:3, 3] = v
        G = expm(M)
        gt = accuracy.move_surfels(gt, np.linalg.inv(G))
    rep = accuracy.map_accuracy(ef, gt, max_dist=a.max_dist, align=a.align)
    ef.close()
    print(f"{a.frames} frames at {a.width}x{a.height}, {a.gt} ground-truth surfels asked for")
    print(accuracy.format_report(rep))
    if G is not None and a.align:
        d = np.asarray(rep["align"]["T"]) @ np.linalg.inv(G)
        k = (d[:3, :3] - d[:3, :3].T) / 2
        print(f"perturbed by the inverse of the twist {a.perturb}; the recovered motion differs from it by {np.linalg.norm(d[:3, 3]) * 1e3:.3f} mm, "
              f"{np.degrees(np.arcsin(min(1.0, np.sqrt(k[2, 1] ** 2 + k[0, 2] ** 2 + k[1, 0] ** 2)))):.4f} deg (it also absorbs the map's own drift)")
    if a.json:
        print(json.dumps(rep))


if __name__ == "__main__":
    main()
