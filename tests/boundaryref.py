"""The boundary estimation of include/ef_hip.h ("Find the map's boundaries") restated in numpy and Python floats from the header alone: the
normals' exhaustive neighbour lists and (for ESTIMATED normals) their estimate, the frame, the projections, TURN, the gap, the verdicts, the
loops (componentref's union-find on the BOUNDARY nodes), the lists and the result.  No grid, no index.

A Python float is an IEEE double whose +, -, *, / round once per operation, math.sqrt is correctly rounded and abs is exact."""
import math

import numpy as np

import componentref as cr
import normalref as nr

F = np.float32
STORED, ESTIMATED = 0, 1
NONE, INTERIOR, BOUNDARY, SPARSE, DEGENERATE, LOOPS_ACCEPTED, LOOPS_REJECTED = 0, 1, 2, 3, 4, 5, 6
LOOP_NONE = 0xFFFFFFFF
DEFAULTS = dict(radius=0.03, min_conf=-1.0, k=12, min_neighbors=5, normal_source=STORED, line_ratio=1e-4, max_gap=1.0, min_size=1, max_size=0)


def finite(x):
    return x - x == 0.0


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def frame(m):
    """(e1, e2, i0) for the f32 normal m, or None where the row is DEGENERATE"""
    a = [float(F(x)) for x in m]
    nn = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    if not (finite(nn) and nn > 0.0):
        return None
    ln = math.sqrt(nn)
    h = (a[0] / ln, a[1] / ln, a[2] / ln)
    i0, low = 0, abs(h[0])
    if abs(h[1]) < low:
        i0, low = 1, abs(h[1])
    if abs(h[2]) < low:
        i0 = 2
    e = tuple(1.0 if i == i0 else 0.0 for i in range(3))
    e1 = cross(e, h)
    e2 = cross(h, e1)
    return e1, e2, i0


def project(e1, e2, p, t):
    """(x, y, is a direction) of the neighbour at t (f32 [3]) seen from the row at p (f32 [3])"""
    q = [float(F(t[i])) - float(F(p[i])) for i in range(3)]
    x = (q[0] * e1[0] + q[1] * e1[1]) + q[2] * e1[2]
    y = (q[0] * e2[0] + q[1] * e2[1]) + q[2] * e2[2]
    return x, y, bool(finite(x) and finite(y) and abs(x) + abs(y) > 0.0)


def turn(xj, yj, xi, yi, i_below_j):
    d = xj * xi + yj * yi
    c = xj * yi - yj * xi
    s = abs(d) + abs(c)
    if s == 0.0 or not finite(s):
        t = 0.0
    elif d >= 0.0 and c >= 0.0:
        t = c / s
    elif d < 0.0:
        t = 2.0 - c / s
    else:
        t = 4.0 + c / s
    if t == 0.0 and i_below_j:
        t = 4.0
    return t


def widest(xy):
    """G over the slots of xy = [(x, y, is a direction)]"""
    G = 0.0
    for j, (xj, yj, dj) in enumerate(xy):
        if not dj:
            continue
        g = 4.0
        for i, (xi, yi, di) in enumerate(xy):
            if i == j or not di:
                continue
            t = turn(xj, yj, xi, yi, i < j)
            if t < g:
                g = t
        if g > G:
            G = g
    return G


def gap(m, p, nbrs):
    """G (a Python float) of the row at p with the normal m and the used neighbours' positions nbrs in neighbour order; None: DEGENERATE"""
    fr = frame(m)
    if fr is None:
        return None
    xy = [project(fr[0], fr[1], p, t) for t in nbrs]
    if not any(d for _, _, d in xy):
        return None
    return widest(xy)


def boundaries(S, among=None, nl=None, **kw):
    """everything the header defines per row and for the call.  among: a bool mask of the selected rows, or None; nl:
    normalref.neighbour_lists(S, radius, min_conf, part) when the caller has it already"""
    p = dict(DEFAULTS, **kw)
    S = np.ascontiguousarray(S, F).reshape(-1, 12)
    n = len(S)
    part = nr.participants(S, among)
    count, D, R = nr.neighbour_lists(S, p["radius"], p["min_conf"], part) if nl is None else nl
    k = int(p["k"])
    normals, nstatus = S[:, 8:11], None
    if p["normal_source"] == ESTIMATED:
        est = nr.estimate(S, among=among, nl=(count, D, R), radius=p["radius"], min_conf=p["min_conf"], k=k, min_neighbors=p["min_neighbors"],
                          line_ratio=p["line_ratio"], orientation=nr.KEEP_SIDE)
        normals, nstatus = est["normals"], est["status"]
    status = np.zeros(n, np.uint8)
    gaps = np.zeros(n, F)
    mg = float(F(p["max_gap"]))
    for s in np.nonzero(part)[0]:
        if count[s] < np.uint32(p["min_neighbors"]) or (nstatus is not None and nstatus[s] == nr.SPARSE):
            status[s] = SPARSE
            continue
        if nstatus is not None and nstatus[s] == nr.DEGENERATE:
            status[s] = DEGENERATE
            continue
        c = int(min(int(count[s]), k))
        G = gap(normals[s], S[s, :3], [S[int(R[s, j]), :3] for j in range(c)])
        if G is None:
            status[s] = DEGENERATE
            continue
        gaps[s] = F(G)
        status[s] = BOUNDARY if G > mg else INTERIOR
    node = (status == BOUNDARY) & cr.nodes(S, None, p["min_conf"])
    label, size = cr.labels_of(n, node, cr.edges(S, node, p["radius"]))
    lo, hi = np.uint32(p["min_size"]), np.uint32(p["max_size"])
    rejected = node & ((size < lo) | ((hi != 0) & (size > hi)))
    accepted = node & ~rejected
    is_root = node & (label == np.arange(n, dtype=np.uint32))
    result = dict(participants=int(part.sum()), interior=int((status == INTERIOR).sum()), boundary=int((status == BOUNDARY).sum()),
                  sparse=int((status == SPARSE).sum()), degenerate=int((status == DEGENERATE).sum()), loops=int(is_root.sum()),
                  accepted=int((is_root & accepted).sum()), largest=int(size.max()) if n else 0, status=0)
    return dict(gap=gaps, count=np.where(part, count, 0).astype(np.uint32), status=status, label=label, size=size, part=part,
                accepted=accepted, rejected=rejected, result=result, params=p)


def listed(ref, what):
    """the ascending rows `what` names in boundaries()'s return value"""
    if what == LOOPS_ACCEPTED:
        mask = ref["accepted"]
    elif what == LOOPS_REJECTED:
        mask = ref["rejected"]
    else:
        mask = ref["status"] == what
    return np.nonzero(mask)[0].astype(np.uint32)


def gap_from_angle(radians):
    """TURN from (1, 0) to (cos a, sin a) with math's cos and sin: what ef_boundary_gap_from_angle agrees with to rounding"""
    return turn(1.0, 0.0, math.cos(radians), math.sin(radians), False)
