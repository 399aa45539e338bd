"""Surface accuracy and completeness of a map against ground-truth surfels (the ElasticFusion paper's second figure beside the trajectory
error), on the device: the nearest-surfel query (ef_query_nearest) finds each point's partner, the figures are then taken in float64 on the
host from the two rows' own floats.

    accuracy      each stable map surfel (confidence > the context's threshold)  ->  the nearest ground-truth surfel
    completeness  each ground-truth surfel                                        ->  the nearest stable map surfel

Each side reports, over the points that found a partner within max_dist: mean, median and RMS of the distance and of the absolute distance
along the partner's normal (point to plane), and the share of points that found none.  The ground truth lives in a second context
(ef_map_upload); neither the oracle nor any reference checkout is read.

A ground truth that is not in the map's world frame (another dataset's model, a second session, a scan) is first placed there by
point-to-plane ICP against the map (register_to_map over ef_register_cloud; map_accuracy(align=True))."""
from __future__ import annotations

import ctypes as C

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


REGISTER_SCHEDULE = (0.10, 0.05, 0.025)   # max_dist per stage, coarse to fine; each at most EF_QUERY_MAX_RATIO cells of the index


def move_surfels(surfels: np.ndarray, T: np.ndarray) -> np.ndarray:
    """[m, 12] surfels moved by the rigid 4 x 4 T: positions by T, normals by its rotation block (float64, rounded to float32 once)"""
    out = np.array(surfels, np.float32).reshape(-1, 12)
    T = np.asarray(T, np.float64)
    out[:, :3] = out[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    out[:, 8:11] = out[:, 8:11].astype(np.float64) @ T[:3, :3].T
    return out


def register_to_map(ef: "api.ElasticFusion", surfels_or_points: np.ndarray, T_init=None, schedule=REGISTER_SCHEDULE, min_conf: float | None = None,
                    use_normals: bool = True, **params) -> tuple:
    """Point-to-plane ICP (ef_register_cloud) of a cloud against ef's map on a coarse-to-fine schedule of max_dist, each stage starting from
    the last stage's pose.  surfels_or_points: [m, 12] surfels (positions, and normals unless use_normals is off) or [m, 3] points, in their
    own frame.  min_conf None = the context's confidence threshold (stable surfels only); other keywords are ef_register_params fields.
    Returns (T 4 x 4 float64 cloud -> map, [per-stage result dicts with "max_dist" added]).  A stage that ends TOO_FEW_PAIRS or DEGENERATE
    leaves the pose where it was and the later, finer stages are not run."""
    a = np.asarray(surfels_or_points, np.float32)
    assert a.ndim == 2 and a.shape[1] in (3, 12), a.shape
    pts = np.ascontiguousarray(a[:, :3])
    nrm = np.ascontiguousarray(a[:, 8:11]) if a.shape[1] == 12 and use_normals else None
    T = np.eye(4) if T_init is None else np.array(T_init, np.float64).reshape(4, 4)
    if min_conf is None:
        min_conf = float(ef.cfg.confidence)
    stages = []
    for md in schedule:
        T, res = ef.registerCloud(pts, nrm, T_init=T, max_dist=float(md), min_conf=float(min_conf), **params)
        res["max_dist"] = float(md)
        stages.append(res)
        if res["status"] in (api.REG_TOO_FEW_PAIRS, api.REG_DEGENERATE):
            break
    return T, stages


def merge_session(ef: "api.ElasticFusion", surfels: np.ndarray, T_init=None, register: dict | None = None, rows: bool = False, fuse: bool = False,
                  **insert) -> tuple:
    """Continues ef's map with the surfels of another session ([m, 12] as downloadMap() gives them, in their own frame): register_to_map on
    their positions and normals from T_init (keywords in `register`), then insertSurfels with the pose found (ef_map_insert: the records
    the map does not already hold within min_separation are appended; other keywords are ef_insert_params fields).  A registration whose last
    stage ended TOO_FEW_PAIRS or DEGENERATE inserts nothing.  Returns (T 4 x 4 float64, [per-stage registration results], the insert
    result or None) — with rows=True the insert result is insertSurfels' (result, new_row, match_row).  fuse=True: fuseSurfels(append=1) in
    insertSurfels' place (ef_map_fuse: the records the map does hold are merged into the surfels they match instead of being thrown away, so
    confidences rise where both sessions saw the surface; keywords are ef_fuse_params fields, the result is fuseSurfels')."""
    rec = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
    T, stages = register_to_map(ef, rec, T_init=T_init, **(register or {}))
    if not stages or stages[-1]["status"] in (api.REG_TOO_FEW_PAIRS, api.REG_DEGENERATE):
        return T, stages, None
    if fuse:
        return T, stages, ef.fuseSurfels(rec, T=T, rows=rows, **dict(insert, append=1))
    return T, stages, ef.insertSurfels(rec, T=T, rows=rows, **insert)


def thinned_map(ef: "api.ElasticFusion", cell: float, keep: int = api.THIN_KEEP_MAX_CONF, among=None) -> np.ndarray:
    """One surfel per `cell`-sized voxel of ef's map, [k, 12] float32 as downloadMap() gives them, without a download of the map and without
    changing it: thinSelect(representatives=True) + gatherSurfels (ef_map_thin_select + ef_map_gather).  keep: which surfel stands for its
    voxel (api.THIN_KEEP_*); among: as thinSelect takes it, only the surfels it selects (and only their representatives) come out."""
    return ef.gatherSurfels(ef.thinSelect(cell=float(cell), keep=int(keep), among=among, representatives=True))


def carved_map(ef: "api.ElasticFusion", depths, poses=None, **kw) -> np.ndarray:
    """ef's map without the surfels that the depth views see through, [k, 12] float32 as downloadMap() gives them, without a download of the
    whole map and without changing it: carveSelect + gatherSurfels of the other rows (ef_map_carve_select + ef_map_gather), which is what
    carveSurfels with the same arguments would leave.  depths, poses and the keywords (params, among, ef_carve_params fields) as carveSelect
    takes them."""
    removed = ef.carveSelect(depths, poses, **kw)
    kept = np.ones(ef.lastCount(), bool)
    kept[removed] = False
    return ef.gatherSurfels(np.nonzero(kept)[0].astype(np.uint32))


def without_outliers(ef: "api.ElasticFusion", **params) -> np.ndarray:
    """ef's map without its outlier surfels, [k, 12] float32 as downloadMap() gives them, without a download of the whole map and without
    changing it: outlierSelect + gatherSurfels of the other rows (ef_map_outliers_select + ef_map_gather), which is what removeOutliers with
    the same arguments would leave.  The keywords (params, among, ef_outlier_params fields) as outlierSelect takes them."""
    removed = ef.outlierSelect(**params)
    kept = np.ones(ef.lastCount(), bool)
    kept[removed] = False
    return ef.gatherSurfels(np.nonzero(kept)[0].astype(np.uint32))


def segments(ef: "api.ElasticFusion", min_size: int = 50, max_segments: int | None = None, **params) -> list:
    """ef's map cut into its connected components under "closer than radius": a list of [k, 12] float32 arrays as downloadMap() gives them,
    one per component of at least min_size nodes, LARGEST FIRST with ties by label (the component's smallest row), at most max_segments of
    them; the map does not change and is not downloaded: components + one gatherSurfels per segment (ef_map_components + ef_map_gather).
    The keywords (params, among, ef_component_params fields) as components takes them."""
    label, size = ef.components(**params)
    roots = np.nonzero((label == np.arange(len(label), dtype=np.uint32)) & (size >= max(int(min_size), 1)))[0]
    roots = roots[np.lexsort((roots, -size[roots].astype(np.int64)))]
    if max_segments is not None:
        roots = roots[:max_segments]
    order = np.argsort(label, kind="stable")                # one pass: the rows of every label, ascending within it
    first = np.searchsorted(label[order], roots)
    return [ef.gatherSurfels(order[a:a + int(size[r])].astype(np.uint32)) for r, a in zip(roots, first)]


def largest_component(ef: "api.ElasticFusion", **params) -> np.ndarray:
    """the surfels of ef's largest connected component (ties: the lowest label), [k, 12] float32, [0, 12] for a map without nodes; the map
    does not change.  The keywords as segments takes them."""
    got = segments(ef, min_size=1, max_segments=1, **params)
    return got[0] if got else np.zeros((0, 12), np.float32)


def plane_segments(ef: "api.ElasticFusion", **params) -> list:
    """ef's map cut into its planes: a list of (model dict, [k, 12] float32 surfels as downloadMap() gives them), one per plane found, in
    the order they were found; the map does not change and is not downloaded: planes + one gatherSurfels per plane (ef_map_planes +
    ef_map_gather).  The keywords (params, among, ef_plane_params fields) as planes takes them."""
    plane, models = ef.planes(**params)
    order = np.argsort(plane, kind="stable")                # one pass: the rows of every plane, ascending within it
    first = np.searchsorted(plane[order], np.arange(len(models), dtype=np.uint32))
    return [(m, ef.gatherSurfels(order[a:a + m["inliers"]].astype(np.uint32))) for m, a in zip(models, first)]


def smooth_regions(ef: "api.ElasticFusion", min_size: int = 50, max_regions: int | None = None, **params) -> list:
    """ef's map cut along its creases into smooth regions: a list of [k, 12] float32 arrays as downloadMap() gives them, one per region of at
    least min_size rows (cores and attached borders; with max_size among the keywords, of at most that many), LARGEST FIRST with ties by
    label (the region's smallest core row), at most max_regions of them, each in ascending row order; the map does not change and is not
    downloaded: regions + one gatherSurfels per region (ef_map_regions + ef_map_gather).  The keywords (params, among, ef_region_params
    fields) as regions takes them."""
    label, size, _ = ef.regions(**params)
    p = params.get("params")
    max_size = int(p.max_size if p is not None else params.get("max_size", 0))
    roots = np.nonzero((label == np.arange(len(label), dtype=np.uint32)) & (size >= max(int(min_size), 1)) & ((max_size == 0) | (size <= max_size)))[0]
    roots = roots[np.lexsort((roots, -size[roots].astype(np.int64)))]
    if max_regions is not None:
        roots = roots[:max_regions]
    order = np.argsort(label, kind="stable")                # one pass: the rows of every label, ascending within it
    first = np.searchsorted(label[order], roots)
    return [ef.gatherSurfels(order[a:a + int(size[r])].astype(np.uint32)) for r, a in zip(roots, first)]


def without_planes(ef: "api.ElasticFusion", **params) -> np.ndarray:
    """a gathered copy of the participants that lie on no found plane (the PLANES_OFF rows: what removePlanes leaves of them), [k, 12] float32;
    the map does not change and is not downloaded.  The keywords as plane_segments takes them."""
    return ef.gatherSurfels(ef.planeSelect(what=api.PLANES_OFF, **params))


def estimated_normals(ef: "api.ElasticFusion", **params) -> np.ndarray:
    """a gathered copy of the surfels whose normal the map's own geometry determines (the ESTIMATED rows, ascending), [k, 12] float32 as
    downloadMap() gives them with floats 8 .. 10 replaced by the estimate and, with set_radius, float 11 by radius_scale * spacing: what
    reestimateNormals with the same arguments would leave of those rows.  The map does not change and is not downloaded: estimateNormals +
    gatherSurfels (ef_map_normals + ef_map_gather).  The keywords (params, among, ef_normal_params fields) as estimateNormals takes them."""
    est = ef.estimateNormals(**params)
    rows = np.nonzero(est["status"] == api.NORMAL_ESTIMATED)[0].astype(np.uint32)
    out = ef.gatherSurfels(rows)
    out[:, 8:11] = est["normals"][rows]
    p = params.get("params")
    set_radius, scale = (p.set_radius, p.radius_scale) if p is not None else (params.get("set_radius", 0), params.get("radius_scale", 1.0))
    if set_radius:
        out[:, 11] = np.float32(scale) * est["spacing"][rows]
    return out


def smoothed_map(ef: "api.ElasticFusion", **params) -> np.ndarray:
    """a smoothed copy of the map's records, [n, 12] float32 as downloadMap() gives them with floats 0 .. 2 of every participant replaced by
    its moving-least-squares position and, with set_normal, floats 8 .. 10 of the SMOOTHED rows by the last fit's normal: what applySmooth
    with the same arguments would leave.  The map does not change: smoothMap + gatherSurfels (ef_map_smooth + ef_map_gather).  The keywords
    (params, among, ef_smooth_params fields) as smoothMap takes them."""
    sm = ef.smoothMap(**params)
    out = ef.gatherSurfels(np.arange(len(sm["status"]), dtype=np.uint32))
    part = sm["status"] != api.SMOOTH_NONE
    out[part, 0:3] = sm["position"][part]
    p = params.get("params")
    if p.set_normal if p is not None else params.get("set_normal", 0):
        done = sm["status"] == api.SMOOTH_SMOOTHED
        out[done, 8:11] = sm["normal"][done]
    return out


def map_boundaries(ef: "api.ElasticFusion", max_loops: int | None = None, **params) -> list:
    """where ef's map ends: the loops of its boundary surfels (the rim of the scanned surface and the rims of the holes in it), what a
    next-view planner consumes.  A list of dicts, one per ACCEPTED loop (min_size / max_size among the keywords), LARGEST FIRST with ties by
    label, at most max_loops of them:
        label      the loop's smallest row
        rows       its rows, ascending (uint32): what gatherSurfels and eraseRows take
        size       their number
        surfels    [size, 12] float32 as downloadMap() gives them
        centroid   the mean position (float64 [3])
        axes       [3, 3] float64: the principal axes of the positions as rows, longest first (the last is the normal of the loop's plane)
        extent     float64 [3]: max - min of the positions along each axis (a round hole: two equal extents and a small third)
    The map does not change and is not downloaded.  Which rows belong to an accepted loop is the device's verdict (boundarySelect with
    BOUNDARY_LOOPS_ACCEPTED: ef_map_boundaries_select); the select lists carry no labels, so a second call brings the label word of every
    row (ef_map_boundaries with every other array NULL: 4 bytes per row; the device work runs twice) and is looked at in the listed rows only; then one gatherSurfels
    per loop (ef_map_gather), the moments in double on the host.  The keywords (params, among, ef_boundary_params fields) as boundaries
    takes them."""
    prm, among, pa = ef._boundaryArgs(params.pop("params", None), params.pop("among", None), params)
    listed = ef.boundarySelect(prm, among, what=api.BOUNDARY_LOOPS_ACCEPTED)
    n = ef.lastCount()
    label = np.zeros(max(n, 1), np.uint32)
    api._chk(api.lib().ef_map_boundaries(ef.h, C.byref(prm), pa, None, None, None, api._ptr(label), None, n, None), ef.h)
    mine = label[listed]                                    # (ascending rows, so every loop's rows stay ascending below)
    roots, size = np.unique(mine, return_counts=True)
    keep = np.lexsort((roots, -size.astype(np.int64)))
    roots, size = roots[keep], dict(zip(roots.tolist(), size.tolist()))
    if max_loops is not None:
        roots = roots[:max_loops]
    order = np.argsort(mine, kind="stable")                 # one pass: the listed rows of every label, ascending within it
    first = np.searchsorted(mine[order], roots)
    listed = listed[order]
    out = []
    for r, a in zip(roots, first):
        rows = listed[a:a + size[int(r)]]
        S = ef.gatherSurfels(rows)
        P = S[:, :3].astype(np.float64)
        centroid = P.mean(0)
        Q = P - centroid
        w, v = np.linalg.eigh(Q.T @ Q)
        axes = v[:, ::-1].T.copy()
        proj = Q @ axes.T
        out.append(dict(label=int(r), rows=rows, size=size[int(r)], surfels=S, centroid=centroid, axes=axes, extent=proj.max(0) - proj.min(0)))
    return out


CLOUD_RADIUS = 2.0 ** -20     # insert_cloud's placeholder radius: a value no frame and no spacing produces, so that it marks the inserted rows


def insert_cloud(ef: "api.ElasticFusion", points: np.ndarray, colours=None, viewpoint=(0.0, 0.0, 0.0), T=None, confidence: float | None = None,
                 min_separation: float = 0.01, side: int = -1, **normal) -> tuple:
    """Adds a cloud that has no normals (a LiDAR sweep, a photogrammetry cloud, a mesh's vertices) to ef's map: [m, 3] points in their own
    frame, moved by T (4 x 4, cloud -> map; None: as they are), optional colours [m, 3] uint8.  The records are built with a ZERO normal and
    the placeholder radius CLOUD_RADIUS and inserted with min_normal_cos = -1 (insertSurfels: the points the map already holds within
    min_separation are dropped); then the normals AND radii of the inserted rows alone are estimated from the map's geometry, old rows
    counting as neighbours (reestimateNormals among the inserted rows, set_radius = 1, VIEWPOINT orientation: `viewpoint` is the sensor's
    position in the MAP frame, side = -1 the map's convention).  The inserted rows are selected by their ID range where surfel IDs are on,
    otherwise by the creation time the insert gave them (the context's tick) together with the placeholder radius.  confidence None: just
    above the context's threshold, so that the rows are stable.  Other keywords are ef_normal_params fields (radius, k, radius_scale, ...).
    An inserted row whose neighbourhood is SPARSE or DEGENERATE keeps the zero normal and the placeholder radius: normalSelect lists them.
    Returns (the insert's result, the re-estimate's result)."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    rec = np.zeros((len(pts), 12), np.float32)
    rec[:, :3] = pts
    rec[:, 3] = float(ef.cfg.confidence) + 1.0 if confidence is None else float(confidence)
    if colours is None:
        rec[:, 4] = float(0x808080)
    else:
        c = np.ascontiguousarray(colours, np.uint8).reshape(-1, 3).astype(np.int64)
        rec[:, 4] = ((c[:, 0] << 16) + (c[:, 1] << 8) + c[:, 2]).astype(np.float32)
    rec[:, 11] = CLOUD_RADIUS
    tick = ef.insertParams().init_time
    ins = ef.insertSurfels(rec, T=T, min_separation=float(min_separation), min_normal_cos=-1.0, init_time=tick, last_time=tick)
    n1 = ins["count_after"]
    n0 = n1 - ins["inserted"]
    ends = ef.gatherSurfels(np.array([n0, n1 - 1], np.uint32))[:, 5].view(np.uint32) if n1 > n0 else np.zeros(2, np.uint32)
    if ends[0] and ends[1]:      # surfel IDs are on (the ID lane is zero otherwise); the gather has numbered the new rows, ascending by row
        among = dict(tests=api.SEL_ID, id_min=int(ends[0]), id_max=int(ends[1]))
    else:
        among = dict(tests=api.SEL_INIT_TIME | api.SEL_RADIUS, init_time_min=tick, init_time_max=tick, radius_min=CLOUD_RADIUS,
                     radius_max=CLOUD_RADIUS)
    kw = dict(dict(set_radius=1), **normal)
    return ins, ef.reestimateNormals(among=among, orientation=api.NORMALS_VIEWPOINT, side=int(side), viewpoint=tuple(float(v) for v in viewpoint), **kw)


def map_accuracy(ef: "api.ElasticFusion", gt_surfels: np.ndarray, max_dist: float = 0.05, map_rows=None, gt_rows=None, device: int = 0,
                 align: bool = False, align_schedule=REGISTER_SCHEDULE) -> dict:
    """ef: a context with a map; gt_surfels: [m, 12] float32, laid out as downloadMap() gives them (synth.sample_surfels), in the map's world
    frame unless align is set.  map_rows / gt_rows: optional row subsets to ask from (map rows that are not stable are dropped); partners are
    always sought in the whole other side.  align: the ground truth is first registered to the map's stable surfels (register_to_map with its
    positions and normals, the established protocol for a model made elsewhere) and moved by the result; the figures are then taken as
    without it.  Returns {"accuracy": {...}, "completeness": {...}, "max_dist", "stable", "map_count"[, "align": {"T", "stages"}]}."""
    gt = np.ascontiguousarray(gt_surfels, np.float32).reshape(-1, 12)
    aligned = None
    if align:
        T, stages = register_to_map(ef, gt, schedule=align_schedule)
        gt = move_surfels(gt, T)
        aligned = {"T": T.tolist(), "stages": [{k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in st.items()} for st in stages]}
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
    rep = {"accuracy": _figures(map_pts, acc_rows, gt), "completeness": _figures(gt_pts, com_rows, surfels), "max_dist": float(max_dist),
           "stable": int((surfels[:, 3] > np.float32(thresh)).sum()), "map_count": int(len(surfels))}
    if aligned is not None:
        rep["align"] = aligned
    return rep


def format_report(r: dict) -> str:
    lines = [f"map {r['map_count']} surfels, {r['stable']} stable; max_dist {r['max_dist']:.3f} m"]
    for side in ("accuracy", "completeness"):
        f = r[side]
        lines.append(f"{side:12s} points {f['points']} hits {f['hits']} miss share {f['miss_share']:.4f}  "
                     f"dist mean {f['dist_mean'] * 1e3:.3f} median {f['dist_median'] * 1e3:.3f} rms {f['dist_rms'] * 1e3:.3f} mm  "
                     f"|plane| mean {f['plane_mean'] * 1e3:.3f} median {f['plane_median'] * 1e3:.3f} rms {f['plane_rms'] * 1e3:.3f} mm")
    if "align" in r:
        T = np.asarray(r["align"]["T"], np.float64)
        ang = float(np.arccos(np.clip((np.trace(T[:3, :3]) - 1) / 2, -1, 1)))
        lines.append(f"aligned first: translation {np.linalg.norm(T[:3, 3]) * 1e3:.3f} mm, rotation {np.degrees(ang):.4f} deg; stages " +
                     ", ".join(f"{st['max_dist']:.3f} m: {st['status_name']} after {st['iterations']} ({st['pairs']} pairs, rms "
                               f"{st['rms_first'] * 1e3:.3f} -> {st['rms_last'] * 1e3:.3f} mm)" for st in r["align"]["stages"]))
    return "\n".join(lines)
