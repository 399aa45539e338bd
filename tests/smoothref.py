"""The smoothing of include/ef_hip.h ("Smooth the map's positions") restated in numpy from the header alone: the normals' exhaustive neighbour
scan in f32 (normalref.neighbour_lists: no grid, no index), taken once; per iteration the f32 d2, the double weights, the ten double sums in
neighbour order, the weighted eigen-decomposition (the header's text, here over all rows at once), the orientation, the curvature, the
verdicts, the projection with its clamp; then the shift, the lists, the result and the write-back.

numpy's float32 and float64 arithmetic rounds once per operation, and its sqrt and division are the correctly rounded IEEE operations, element
by element: an expression over arrays gives each row the bits the same expression gives it alone.  A branch of the header is a numpy.where
between both sides' values.  tests/test_smooth_host.py compares fit() with smooth_fit of csrc/ef_plane_fit.hpp compiled for the host, bit for bit,
and with normalref's scalar normal_fit where the weights are 1."""
import numpy as np

from normalref import neighbour_lists
from outlierref import participants
from planeref import SWEEPS

F = np.float32
D = np.float64
UNIFORM, COMPACT = 0, 1
NONE, SMOOTHED, SPARSE, DEGENERATE, CLAMPED, SHIFTED = 0, 1, 2, 3, 4, 5
GAVE_UP, FIT_ESTIMATED, FIT_DEGENERATE = 0, 1, 2          # fit()'s verdicts (smooth_fit's return values)
DEFAULTS = dict(radius=0.03, min_conf=-1.0, k=12, min_neighbors=5, iterations=1, weighting=COMPACT, normal_gate=0, min_normal_cos=0.9, strength=1.0,
                max_shift=None, line_ratio=1e-4, set_normal=0, shift_threshold=0.0)       # max_shift None: = radius


def finite(x):
    return (x - x) == 0.0


def rotate(A, V, p, q, r):
    """one Jacobi rotation of the header's EIGEN-DECOMPOSITION in the plane (p, q), every row at once: a row whose a_pq is 0 or NaN keeps everything"""
    apq = A[p][q]
    do = (apq < 0.0) | (apq > 0.0)
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    root = np.sqrt(theta * theta + 1.0)
    t = np.where(theta < 0.0, -1.0 / (root - theta), 1.0 / (root + theta))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    app, aqq = A[p][p] - t * apq, A[q][q] + t * apq
    arp, arq = A[r][p], A[r][q]
    nrp, nrq = c * arp - s * arq, s * arp + c * arq
    A[p][p], A[q][q] = np.where(do, app, A[p][p]), np.where(do, aqq, A[q][q])
    A[p][q] = A[q][p] = np.where(do, 0.0, apq)
    A[r][p] = A[p][r] = np.where(do, nrp, arp)
    A[r][q] = A[q][r] = np.where(do, nrq, arq)
    for k in range(3):
        vkp, vkq = V[k][p], V[k][q]
        V[k][p], V[k][q] = np.where(do, c * vkp - s * vkq, vkp), np.where(do, s * vkp + c * vkq, vkq)


def fit(S, W, m, hn, line_ratio):
    """the header's FIT for every row: S [n, 9] and W [n] float64, m [n] = c + 1, hn [n, 3] float32 the stored normals.  Returns (verdict [n]:
    GAVE_UP / FIT_ESTIMATED / FIT_DEGENERATE, n [n, 3] float64, mean [n, 3] float64, curvature [n] float32), zeros unless FIT_ESTIMATED"""
    S, W = np.asarray(S, D).reshape(-1, 9), np.asarray(W, D).reshape(-1)
    m, hn = np.asarray(m).reshape(-1), np.asarray(hn, F).reshape(-1, 3).astype(D)
    with np.errstate(all="ignore"):
        ok = m >= 3
        mx, my, mz = S[:, 0] / W, S[:, 1] / W, S[:, 2] / W
        A = [[None] * 3 for _ in range(3)]
        A[0][0] = S[:, 3] / W - mx * mx
        A[0][1] = S[:, 4] / W - mx * my
        A[0][2] = S[:, 5] / W - mx * mz
        A[1][1] = S[:, 6] / W - my * my
        A[1][2] = S[:, 7] / W - my * mz
        A[2][2] = S[:, 8] / W - mz * mz
        A[1][0], A[2][0], A[2][1] = A[0][1], A[0][2], A[1][2]
        for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
            ok = ok & finite(A[i][j])
        one, zero = np.ones(len(S)), np.zeros(len(S))
        V = [[one if i == j else zero for j in range(3)] for i in range(3)]
        for _ in range(SWEEPS):
            rotate(A, V, 0, 1, 2)
            rotate(A, V, 0, 2, 1)
            rotate(A, V, 1, 2, 0)
        l0, l1, l2 = A[0][0], A[1][1], A[2][2]
        lam, nx, ny, nz = l0, V[0][0], V[1][0], V[2][0]
        pick = l1 < lam
        lam, nx, ny, nz = np.where(pick, l1, lam), np.where(pick, V[0][1], nx), np.where(pick, V[1][1], ny), np.where(pick, V[2][1], nz)
        pick = l2 < lam
        lam, nx, ny, nz = np.where(pick, l2, lam), np.where(pick, V[0][2], nx), np.where(pick, V[1][2], ny), np.where(pick, V[2][2], nz)
        ok = ok & finite(lam)
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok = ok & (ln > 0.0) & finite(ln)
        nx, ny, nz = nx / ln, ny / ln, nz / ln
        flip = (nx * hn[:, 0] + ny * hn[:, 1]) + nz * hn[:, 2] < 0.0
        nx, ny, nz = np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)
        for x in (l0, l1, l2, nx, ny, nz):
            ok = ok & finite(x)
        e0, e1, e2 = np.where(l0 > 0.0, l0, 0.0), np.where(l1 > 0.0, l1, 0.0), np.where(l2 > 0.0, l2, 0.0)
        emin = np.where(lam > 0.0, lam, 0.0)
        lo, hi = np.where(e1 < e0, e1, e0), np.where(e1 < e0, e0, e1)
        emax = np.where(e2 > hi, e2, hi)
        emid = np.where(e2 > hi, hi, np.where(e2 < lo, lo, e2))
        plane = emid > D(F(line_ratio)) * emax
        tot = (e0 + e1) + e2
        curv = np.where(tot > 0.0, (emin / tot).astype(F), F(0)).astype(F)
    est = ok & plane
    verdict = np.where(est, FIT_ESTIMATED, np.where(ok, FIT_DEGENERATE, GAVE_UP))
    n = np.where(est[:, None], np.stack([nx, ny, nz], 1), 0.0)
    mean = np.where(est[:, None], np.stack([mx, my, mz], 1), 0.0)
    return verdict, n, mean, np.where(est, curv, F(0)).astype(F)


def d2_f32(a, b):
    """the queries' d2(q, p) of the rows of two [n, 3] f32 arrays"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1], a[:, 2] - b[:, 2]
        d2 = ((dx * dx + dy * dy) + dz * dz)
    assert d2.dtype == F
    return d2


def sums(P, N, fitted, c, R, p, seen=None):
    """the header's SUMS of one iteration from the positions P [n, 3] f32: (S [n, 9], W [n]) float64; rows outside `fitted` keep zeros and 1.
    seen (a dict) collects what the scenes are asked to contain: (row, slot) pairs past the radius and gated out"""
    n = len(P)
    Pd = P.astype(D)
    r = F(p["radius"])
    r2 = D(F(r * r))
    mnc = F(p["min_normal_cos"])
    S, W = np.zeros((n, 9), D), np.ones(n, D)
    own = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int(p["k"])):
            use = fitted & (j < c)
            t = np.where(use, R[:, j], own)
            d2 = d2_f32(P, P[t])
            if p["weighting"] == COMPACT:
                u = 1.0 - d2.astype(D) / r2
                w = np.where(u > 0.0, u * u, 0.0)
            else:
                w = np.ones(n, D)
            if seen is not None:
                seen["past_radius"] = seen.get("past_radius", 0) + int((use & (d2 > F(r2))).sum())
            if p["normal_gate"]:
                dot = (N[:, 0] * N[t, 0] + N[:, 1] * N[t, 1]) + N[:, 2] * N[t, 2]
                assert dot.dtype == F
                smooth = dot >= mnc
                if seen is not None:
                    seen["gated_out"] = seen.get("gated_out", 0) + int((use & ~smooth).sum())
                w = np.where(smooth, w, 0.0)
            q = Pd[t] - Pd
            x, y, z = q[:, 0], q[:, 1], q[:, 2]
            a, b, g = w * x, w * y, w * z
            for i, term in enumerate((a, b, g, a * x, a * y, a * z, b * y, b * z, g * z)):
                S[:, i] = np.where(use, S[:, i] + term, S[:, i])
            W = np.where(use, W + w, W)
    return S, W


def smooth_runs(S, among=None, nl=None, seen=None, **kw):
    """everything the header defines per row, after every iteration: a list of `iterations` dicts, the i-th what a call with iterations = i
    gives.  among: a bool mask of the selected rows, or None; nl: normalref.neighbour_lists(S, radius, min_conf, part) when the caller has it;
    seen: see sums() (per iteration: seen[i] for iteration i + 1)"""
    p = dict(DEFAULTS, **kw)
    if p["max_shift"] is None:
        p["max_shift"] = p["radius"]
    S = np.ascontiguousarray(S, F).reshape(-1, 12)
    n = len(S)
    part = participants(S, among)
    count, _, R = neighbour_lists(S, p["radius"], p["min_conf"], part) if nl is None else nl
    k = int(p["k"])
    c = np.minimum(count, np.uint32(k)).astype(np.int64)
    sparse = part & (count < np.uint32(p["min_neighbors"]))
    fitted = part & ~sparse
    P0 = S[:, :3].copy()
    N = S[:, 8:11].copy()
    P = P0.copy()
    clamped = np.zeros(n, bool)
    strength, ms = D(F(p["strength"])), D(F(p["max_shift"]))
    runs = []
    for it in range(int(p["iterations"])):
        here = None if seen is None else seen.setdefault(it, {})
        Sm, W = sums(P, N, fitted, c, R, p, here)
        verdict, nrm, mean, curv = fit(Sm, W, c + 1, N, p["line_ratio"])
        est = fitted & (verdict == FIT_ESTIMATED)
        with np.errstate(invalid="ignore", over="ignore"):
            t = (nrm[:, 0] * mean[:, 0] + nrm[:, 1] * mean[:, 1]) + nrm[:, 2] * mean[:, 2]
            s = strength * t
            above = s > ms
            below = ~above & (s < -ms)
            s = np.where(above, ms, np.where(below, -ms, s))
            clamped = clamped | (est & (above | below))
            new = (P.astype(D) + s[:, None] * nrm).astype(F)
        done = est & np.isfinite(new).all(1)
        P = np.where(done[:, None], new, P).astype(F)
        status = np.where(done, SMOOTHED, DEGENERATE).astype(np.uint8)
        status[sparse] = SPARSE
        status[~part] = NONE
        with np.errstate(invalid="ignore", over="ignore"):
            shift = np.where(fitted, np.sqrt(d2_f32(P, P0)), F(0)).astype(F)
        result = dict(participants=int(part.sum()), smoothed=int(done.sum()), sparse=int(sparse.sum()), degenerate=int((fitted & ~done).sum()),
                      clamped=int(clamped.sum()), moved=int((shift > 0).sum()), largest_shift=float(shift.max()) if n else 0.0)
        runs.append(dict(position=P.copy(), normal=np.where(done[:, None], nrm.astype(F), F(0)).astype(F), curvature=np.where(done, curv, F(0)).astype(F),
                         shift=shift, count=np.where(part, count, 0).astype(np.uint32), status=status, clamped=clamped.copy(), part=part,
                         result=result, params=p))
    return runs


def smooth(S, among=None, nl=None, **kw):
    return smooth_runs(S, among, nl, **kw)[-1]


def listed(ref, what):
    """the ascending rows `what` names in smooth()'s return value"""
    if what == CLAMPED:
        mask = ref["clamped"]
    elif what == SHIFTED:
        mask = ref["shift"] > F(ref["params"]["shift_threshold"])
    else:
        mask = ref["status"] == what
    return np.nonzero(mask)[0].astype(np.uint32)


def written(S, ref):
    """the map ef_map_smooth_apply leaves: floats 0 .. 2 of the participants, and floats 8 .. 10 of the SMOOTHED rows with set_normal"""
    out = np.ascontiguousarray(S, F).reshape(-1, 12).copy()
    part = ref["status"] != NONE
    out[part, 0:3] = ref["position"][part]
    if ref["params"]["set_normal"]:
        done = ref["status"] == SMOOTHED
        out[done, 8:11] = ref["normal"][done]
    return out
