"""The smooth regions of include/ef_hip.h ("Segment the map into smooth regions") restated in numpy from the header alone: the estimates of
tests/normalref.py (orientation KEEP_SIDE), the node, core and border rules, an exhaustive f32 d2 matrix and the f32 dot with the header's
bracketing, componentref's sequential union-find over the core edges, the borders' attachment by (d2, row), sizes, verdicts, the four lists and
the result.  No grid, no index.  Every output is an integer or a byte: the device must equal it exactly."""
import numpy as np

import componentref as cref
import normalref as nref

F = np.float32
NONE = 0xFFFFFFFF
KIND_NONE, KIND_CORE, KIND_BORDER = 0, 1, 2
ESTIMATED, STORED = 0, 1
REJECTED, ACCEPTED, UNASSIGNED, BORDERS = 0, 1, 2, 3
LISTS = ((REJECTED, "rejected"), (ACCEPTED, "accepted"), (UNASSIGNED, "unassigned"), (BORDERS, "borders"))
DEFAULTS = dict(radius=0.03, min_conf=-1.0, k=12, min_neighbors=5, line_ratio=1e-4, normal_source=ESTIMATED, two_sided=0,
                min_normal_cos=F(0.9659258), max_curvature=0.05, attach_borders=1, min_size=50, max_size=0)
ESTIMATE_KEYS = ("radius", "min_conf", "k", "min_neighbors", "line_ratio")


def estimate(S, among=None, **kw):
    """the ESTIMATE of the header: normalref's, with this call's radius, min_conf, k, min_neighbors and line_ratio and KEEP_SIDE"""
    p = dict(DEFAULTS, **kw)
    return nref.estimate(S, among=among, orientation=nref.KEEP_SIDE, **{k: p[k] for k in ESTIMATE_KEYS})


def dots(N, q):
    """[len(q), n] f32: dot = (n_s.x * n_t.x + n_s.y * n_t.y) + n_s.z * n_t.z of the rows q against every row"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (N[q, None, 0] * N[None, :, 0] + N[q, None, 1] * N[None, :, 1]) + N[q, None, 2] * N[None, :, 2]
    assert d.dtype == F
    return d


def smooth(dot, p):
    with np.errstate(invalid="ignore"):
        return (np.abs(dot) if p["two_sided"] else dot) >= F(p["min_normal_cos"])


def regions(S, among=None, est=None, **kw):
    """everything the header defines for one call.  among: a bool mask of the selected rows, or None; est: estimate(S, among, ...) when the
    caller has it already"""
    p = dict(DEFAULTS, **kw)
    S = np.ascontiguousarray(S, F).reshape(-1, 12)
    n = len(S)
    if est is None:
        est = estimate(S, among, **kw)
    with np.errstate(invalid="ignore"):
        node = est["part"] & (S[:, 3] > F(p["min_conf"])) & (est["status"] == nref.ESTIMATED)
        core = node & (est["curvature"] <= F(p["max_curvature"]))
    border = node & ~core
    N = np.ascontiguousarray(est["normals"] if p["normal_source"] == ESTIMATED else S[:, 8:11], F)
    r = F(p["radius"])
    r2 = F(r * r)
    px, py, pz = S[:, 0], S[:, 1], S[:, 2]
    rows = np.arange(n)
    pairs = []
    attach = np.full(n, -1, np.int64)
    chunk = 512
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, n, chunk):
            q = np.arange(a, min(a + chunk, n))
            if not node[q].any():
                continue
            dx = px[q, None] - px[None, :]
            dy = py[q, None] - py[None, :]
            dz = pz[q, None] - pz[None, :]
            d2 = ((dx * dx + dy * dy) + dz * dz)
            assert d2.dtype == F
            hit = (d2 <= r2) & smooth(dots(N, q), p) & core[None, :] & (rows[q, None] != rows[None, :])
            s, t = np.nonzero(hit & core[q, None] & (rows[q, None] > rows[None, :]))
            pairs.append(np.stack([s + a, t], 1))
            if p["attach_borders"]:
                for i in np.nonzero(border[q])[0]:
                    t = np.nonzero(hit[i])[0]
                    if len(t):
                        attach[q[i]] = t[np.lexsort((t, d2[i, t]))[0]]           # the first by (d2, row)
    pairs = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)
    core_label, _ = cref.labels_of(n, core, pairs)                                # the smallest core row of every core's region
    label = core_label.copy()
    got = attach >= 0
    label[got] = core_label[attach[got]]
    has = label != NONE
    members = np.bincount(label[has].astype(np.int64), minlength=max(n, 1))
    size = np.where(has, members[np.where(has, label, 0).astype(np.int64)], 0).astype(np.uint32) if n else np.zeros(0, np.uint32)
    kind = np.where(core, KIND_CORE, np.where(border, KIND_BORDER, KIND_NONE)).astype(np.uint8)
    lo, hi = np.uint32(p["min_size"]), np.uint32(p["max_size"])
    rejected = has & ((size < lo) | ((hi != 0) & (size > hi)))
    masks = {REJECTED: rejected, ACCEPTED: has & ~rejected, UNASSIGNED: node & ~has, BORDERS: border}
    is_root = core & (label == np.arange(n, dtype=np.uint32))
    res = dict(nodes=int(node.sum()), cores=int(core.sum()), borders=int(border.sum()), attached=int((border & has).sum()),
               unassigned=int((node & ~has).sum()), regions=int(is_root.sum()), largest=int(size.max()) if n else 0,
               rejected_rows=int(rejected.sum()), rejected_regions=int((is_root & rejected).sum()), status=0)
    out = dict(label=label, size=size, kind=kind, attach=attach, pairs=pairs, est=est, normal=N, result=res, params=p)
    for what, key in LISTS:
        out[key] = np.nonzero(masks[what])[0].astype(np.uint32)
    return out


def result_for(ref, what, n):
    """the ef_region_result of a call with `what` (ef_map_regions: REJECTED)"""
    listed = len(ref[dict(LISTS)[what]])
    return dict(ref["result"], listed=listed, count_after=n - listed)


def region_rows(ref):
    """{label: ascending rows} of every region"""
    lab = ref["label"]
    return {int(l): np.nonzero(lab == l)[0] for l in np.unique(lab[lab != NONE])}
