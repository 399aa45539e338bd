"""The normal estimation of include/ef_hip.h ("Estimate normals, curvature and spacing from the map's neighbourhoods") restated in numpy and Python
floats from the header alone: an exhaustive neighbour scan in f32 with the header's bracketing, the spacing, the nine double sums in neighbour
order, the eigen-decomposition (planeref's Jacobi rotation), the orientation, the curvature, the verdicts, the lists and the write-back.  No
grid, no index.

numpy's float32 and float64 arithmetic rounds once per operation, and its sqrt and division are the correctly rounded IEEE operations; a Python
float is an IEEE double with the same properties, and math.sqrt is correctly rounded."""
import math

import numpy as np

from outlierref import neighbours, participants
from planeref import SWEEPS, finite, rotate

F = np.float32
KEEP_SIDE, VIEWPOINT = 0, 1
NONE, ESTIMATED, SPARSE, DEGENERATE, CURVED, FLAT = 0, 1, 2, 3, 4, 5
DEFAULTS = dict(radius=0.03, min_conf=-1.0, k=12, min_neighbors=5, orientation=KEEP_SIDE, side=-1, viewpoint=(0.0, 0.0, 0.0), line_ratio=1e-4,
                max_curvature=0.05, set_radius=0, radius_scale=1.0)


def neighbour_lists(S, radius, min_conf=-1.0, part=None, chunk=512):
    """(count uint32 [n], d2 float32 [n, 16], row int64 [n, 16]): per participant the number of ALL neighbours and the first 16 of them in
    (d2, row) order, d2 = +inf and row = -1 where there are fewer; count 0 for a row that does not participate.  count and d2 are what
    outlierref.neighbours returns (tests/test_normals_host.py compares them)"""
    S = np.ascontiguousarray(S, F)
    n = len(S)
    part = participants(S) if part is None else part
    r = F(radius)
    r2 = F(r * r)
    mc = F(min_conf)
    count = np.zeros(n, np.uint32)
    D = np.full((n, 16), np.inf, F)
    R = np.full((n, 16), -1, np.int64)
    px, py, pz, conf = S[:, 0], S[:, 1], S[:, 2], S[:, 3]
    rows = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        good = conf > mc
        for a in range(0, n, chunk):
            q = slice(a, min(a + chunk, n))
            dx = px[q, None] - px[None, :]
            dy = py[q, None] - py[None, :]
            dz = pz[q, None] - pz[None, :]
            d2 = ((dx * dx + dy * dy) + dz * dz)
            assert d2.dtype == F
            elig = good[None, :] & (d2 <= r2) & (rows[q, None] != rows[None, :]) & part[q, None]
            qi, tj = np.nonzero(elig)
            dd = d2[qi, tj]
            order = np.lexsort((tj, dd, qi))               # by query, then d2, then row
            qi, tj, dd = qi[order], tj[order], dd[order]
            cnt = np.bincount(qi, minlength=q.stop - q.start)
            count[q] = cnt
            start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
            rank = np.arange(len(qi)) - start[qi]
            keep = rank < 16
            D[a + qi[keep], rank[keep]] = dd[keep]
            R[a + qi[keep], rank[keep]] = tj[keep]
    return count, D, R


def spacing(count, D, k):
    """(((sqrt(d2_1) + sqrt(d2_2)) + ...) + sqrt(d2_c)) / (float)c with c = min(count, k); +inf for c = 0"""
    c = np.minimum(count, np.uint32(k)).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.sqrt(D[:, 0])
        for j in range(1, int(k)):
            s = np.where(j < c, s + np.sqrt(D[:, j]), s)
        assert s.dtype == F
        m = s / c.astype(F)
    assert m.dtype == F
    return np.where(c > 0, m, F(np.inf)).astype(F)


def moments(S, count, R, k):
    """[n, 9] float64: the sums over the first c = min(count, k) neighbours of q and of the six products, j ascending from +0.0, with
    q = (double)p_j - (double)p_s"""
    P = S[:, :3].astype(np.float64)
    c = np.minimum(count, np.uint32(k)).astype(np.int64)
    M = np.zeros((len(S), 9), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int(k)):
            use = j < c
            q = np.where(use[:, None], P[np.where(use, R[:, j], 0)] - P, 0.0)
            x, y, z = q[:, 0], q[:, 1], q[:, 2]
            terms = (x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)
            for i, t in enumerate(terms):
                M[:, i] = np.where(use, M[:, i] + t, M[:, i])
    return M


def eigen(S, m):
    """the header's EIGEN-DECOMPOSITION up to the choice: (unit eigenvector of the smallest diagonal entry as three Python floats, the three
    diagonal entries, the chosen one), or None where the fit gives up"""
    if m < 3:
        return None
    S = [float(x) for x in S]
    md = float(m)
    mx, my, mz = S[0] / md, S[1] / md, S[2] / md
    A = [[0.0] * 3 for _ in range(3)]
    A[0][0] = S[3] / md - mx * mx
    A[0][1] = S[4] / md - mx * my
    A[0][2] = S[5] / md - mx * mz
    A[1][1] = S[6] / md - my * my
    A[1][2] = S[7] / md - my * mz
    A[2][2] = S[8] / md - mz * mz
    A[1][0], A[2][0], A[2][1] = A[0][1], A[0][2], A[1][2]
    if not all(finite(A[i][j]) for i in range(3) for j in range(3)):
        return None
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(SWEEPS):
        rotate(A, V, 0, 1, 2)
        rotate(A, V, 0, 2, 1)
        rotate(A, V, 1, 2, 0)
    l = (A[0][0], A[1][1], A[2][2])
    lam, nx, ny, nz = l[0], V[0][0], V[1][0], V[2][0]
    if l[1] < lam:
        lam, nx, ny, nz = l[1], V[0][1], V[1][1], V[2][1]
    if l[2] < lam:
        lam, nx, ny, nz = l[2], V[0][2], V[1][2], V[2][2]
    if not finite(lam):
        return None
    l2 = (nx * nx + ny * ny) + nz * nz
    ln = math.sqrt(l2) if finite(l2) and l2 >= 0.0 else math.nan
    if not (ln > 0.0) or not finite(ln):
        return None
    n = (nx / ln, ny / ln, nz / ln)
    if not all(finite(x) for x in l + n):
        return None
    return n, l, lam


def normal_fit(S, m, hn, line_ratio):
    """(status, normal f32 [3], curvature f32, flipped, l): ESTIMATED or DEGENERATE for a neighbourhood of m members with the sums S and the
    orientation hint hn (3 f32); l = the three diagonal entries, None where the fit gave up"""
    zero = np.zeros(3, F)
    e = eigen(S, m)
    if e is None:
        return DEGENERATE, zero, F(0), False, None
    (nx, ny, nz), l, lam = e
    hn = [float(F(x)) for x in hn]
    flipped = (nx * hn[0] + ny * hn[1]) + nz * hn[2] < 0.0
    if flipped:
        nx, ny, nz = -nx, -ny, -nz
    e0, e1, e2 = (x if x > 0.0 else 0.0 for x in l)
    emin = lam if lam > 0.0 else 0.0
    lo, hi = (e1, e0) if e1 < e0 else (e0, e1)
    emax = e2 if e2 > hi else hi
    emid = hi if e2 > hi else (lo if e2 < lo else e2)
    if not (emid > float(F(line_ratio)) * emax):
        return DEGENERATE, zero, F(0), False, l
    tot = (e0 + e1) + e2
    curv = F(emin / tot) if tot > 0.0 else F(0)
    return ESTIMATED, np.array([nx, ny, nz], np.float64).astype(F), curv, flipped, l


def hints(S, p):
    """[n, 3] f32: the orientation hint of every row"""
    S = np.ascontiguousarray(S, F)
    if p["orientation"] == VIEWPOINT:
        v = np.asarray(p["viewpoint"], F)
        with np.errstate(invalid="ignore", over="ignore"):
            h = F(p["side"]) * (v[None, :] - S[:, :3])
        assert h.dtype == F
        return h
    return S[:, 8:11].copy()


def estimate(S, among=None, nl=None, **kw):
    """everything the header defines per row.  among: a bool mask of the selected rows, or None; nl: neighbour_lists(S, radius, min_conf, part)
    when the caller has it already"""
    p = dict(DEFAULTS, **kw)
    S = np.ascontiguousarray(S, F).reshape(-1, 12)
    n = len(S)
    part = participants(S, among)
    count, D, R = neighbour_lists(S, p["radius"], p["min_conf"], part) if nl is None else nl
    k = int(p["k"])
    sp = spacing(count, D, k)
    sp[~part] = F(np.inf)
    M = moments(S, count, R, k)
    H = hints(S, p)
    c = np.minimum(count, np.uint32(k))
    status = np.zeros(n, np.uint8)
    normals = np.zeros((n, 3), F)
    curv = np.zeros(n, F)
    flipped = np.zeros(n, bool)
    for s in np.nonzero(part)[0]:
        if count[s] < np.uint32(p["min_neighbors"]):
            status[s] = SPARSE
            continue
        status[s], normals[s], curv[s], flipped[s], _ = normal_fit(M[s], int(c[s]) + 1, H[s], p["line_ratio"])
    est = status == ESTIMATED
    result = dict(participants=int(part.sum()), estimated=int(est.sum()), sparse=int((status == SPARSE).sum()),
                  degenerate=int((status == DEGENERATE).sum()), flipped=int(flipped.sum()))
    return dict(normals=normals, curvature=curv, spacing=sp, count=np.where(part, count, 0).astype(np.uint32), status=status, flipped=flipped,
                part=part, result=result, params=p)


def listed(ref, what):
    """the ascending rows `what` names in estimate()'s return value"""
    st, cv = ref["status"], ref["curvature"]
    if what in (CURVED, FLAT):
        with np.errstate(invalid="ignore"):
            curved = (st == ESTIMATED) & (cv > F(ref["params"]["max_curvature"]))
        mask = curved if what == CURVED else (st == ESTIMATED) & ~curved
    else:
        mask = st == what
    return np.nonzero(mask)[0].astype(np.uint32)


def written(S, ref):
    """the map ef_map_reestimate_normals leaves: floats 8 .. 10 of the ESTIMATED rows, and float 11 = radius_scale * spacing with set_radius"""
    out = np.ascontiguousarray(S, F).reshape(-1, 12).copy()
    est = ref["status"] == ESTIMATED
    out[est, 8:11] = ref["normals"][est]
    if ref["params"]["set_radius"]:
        with np.errstate(invalid="ignore", over="ignore"):
            out[est, 11] = (F(ref["params"]["radius_scale"]) * ref["spacing"])[est]
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
