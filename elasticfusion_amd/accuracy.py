"""Surface accuracy and completeness of a map against ground-truth surfels (the ElasticFusion paper's second figure beside the trajectory
error), on the device: the nearest-surfel query (ef_query_nearest) finds each point's partner, the figures are then taken in float64 on the
host from the two rows' own floats.

    accuracy      each stable map surfel (confidence > the context's threshold)  ->  the nearest ground-truth surfel
    completeness  each ground-truth surfel                                        ->  the nearest stable map surfel

Each side reports, over the points that found a partner within max_dist: mean, median and RMS of the distance and of the absolute distance
along the partner's normal (point to plane), and the share of points that found none.  The ground truth lives in a second context
(ef_map_upload); neither the oracle nor any reference checkout is read."""
from __future__ import annotations

import numpy as np

from . import api

MISS = 0xFFFFFFFF


def _figures(points: np.ndarray, rows: np.ndarray, target: np.ndarray) -> dict:
    hit = rows != MISS
    out = {"points": int(len(points)), "hits": int(hit.sum()), "miss_share": float(1.0 - hit.mean()) if len(points) else 0.0}
    q = points[hit].astype(np.float64)
    t = target[rows[hit].astype(np.int64)].astype(np.float64)
    d = q - t[:, :3]
    dist = np.sqrt((d * d).sum(1))
    plane = np.abs((d * t[:, 8:11]).sum(1))
    for name, v in (("dist", dist), ("plane", plane)):
        some = len(v) > 0
        out[name + "_mean"] = float(v.mean()) if some else float("nan")
        out[name + "_median"] = float(np.median(v)) if some else float("nan")
        out[name + "_rms"] = float(np.sqrt((v * v).mean())) if some else float("nan")
    return out


def map_accuracy(ef: "api.ElasticFusion", gt_surfels: np.ndarray, max_dist: float = 0.05, map_rows=None, gt_rows=None, device: int = 0) -> dict:
    """ef: a context with a map; gt_surfels: [m, 12] float32 in the map's world frame, laid out as downloadMap() gives them (synth.sample_surfels).
    map_rows / gt_rows: optional row subsets to ask from (map rows that are not stable are dropped); partners are always sought in the whole
    other side.  Returns {"accuracy": {...}, "completeness": {...}, "max_dist", "stable", "map_count"}."""
    gt = np.ascontiguousarray(gt_surfels, np.float32).reshape(-1, 12)
    surfels = ef.downloadMap()
    thresh = float(ef.cfg.confidence)
    rows = np.arange(len(surfels)) if map_rows is None else np.asarray(map_rows, np.int64)
    rows = rows[surfels[rows, 3] > np.float32(thresh)]
    truth = api.ElasticFusion(maxSurfels=max(len(gt), 1 << 20), device=device)
    try:
        truth.uploadMap(gt)
        map_pts = np.ascontiguousarray(surfels[rows, :3])
        acc_rows = truth.queryNearest(map_pts, max_dist, -1.0)[0]
    finally:
        truth.close()
    gt_pts = np.ascontiguousarray(gt[:, :3] if gt_rows is None else gt[np.asarray(gt_rows, np.int64), :3])
    com_rows = ef.queryNearest(gt_pts, max_dist, thresh)[0]
    return {"accuracy": _figures(map_pts, acc_rows, gt), "completeness": _figures(gt_pts, com_rows, surfels), "max_dist": float(max_dist),
            "stable": int((surfels[:, 3] > np.float32(thresh)).sum()), "map_count": int(len(surfels))}


def format_report(r: dict) -> str:
    lines = [f"map {r['map_count']} surfels, {r['stable']} stable; max_dist {r['max_dist']:.3f} m"]
    for side in ("accuracy", "completeness"):
        f = r[side]
        lines.append(f"{side:12s} points {f['points']} hits {f['hits']} miss share {f['miss_share']:.4f}  "
                     f"dist mean {f['dist_mean'] * 1e3:.3f} median {f['dist_median'] * 1e3:.3f} rms {f['dist_rms'] * 1e3:.3f} mm  "
                     f"|plane| mean {f['plane_mean'] * 1e3:.3f} median {f['plane_median'] * 1e3:.3f} rms {f['plane_rms'] * 1e3:.3f} mm")
    return "\n".join(lines)
