"""The plane segmentation of include/ef_hip.h ("Segment the map into planes") restated in numpy from the header alone: the hashed samples,
the hypotheses in f32 with the header's bracketing, the exhaustive M x H score, the pick, the nine double sums in the outliers' order
(outlierref.lane_sum), the least-squares fit and the labels.  plane_fit() restates elasticfusion_amd/csrc/ef_plane_fit.hpp line by line.

numpy's float32 arithmetic rounds once per operation, and its sqrt and division are the correctly rounded IEEE operations; a Python float is
an IEEE double with the same properties, and math.sqrt is correctly rounded."""
import math

import numpy as np

from outlierref import lane_sum

F = np.float32
U32 = 0xFFFFFFFF
NONE = 0xFFFFFFFF
AXIS_OFF, AXIS_NORMAL, AXIS_INPLANE = 0, 1, 2
ON, OFF = 0, 1
SWEEPS = 8
DEFAULTS = dict(distance=0.01, normal_cos=0.0, min_conf=-1.0, hypotheses=1024, seed=0, max_planes=4, min_inliers=500, refine=1,
                axis_mode=AXIS_OFF, axis=(0.0, 0.0, 1.0), axis_bound=0.95)


def h32(x):
    """on uint32, scalar or array (uint64 arithmetic masked to 32 bits)"""
    x = np.asarray(x, np.uint64) & U32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & U32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & U32
    x ^= x >> np.uint64(16)
    return x


def samples(seed, k, H, M):
    """[H, 3] participant indices of round k"""
    base = h32((int(seed) + 0x9E3779B9 * (k + 1)) & U32)
    hj = (3 * np.arange(H, dtype=np.uint64)[:, None] + np.arange(3, dtype=np.uint64)[None, :]) & U32
    return ((h32(base ^ hj) * np.uint64(M)) >> np.uint64(32)).astype(np.int64)


def nodes(S, among=None, min_conf=-1.0):
    S = np.asarray(S, F)
    with np.errstate(invalid="ignore"):
        node = (np.abs(S[:, :3]) <= np.finfo(F).max).all(1) & (S[:, 3] > F(min_conf))
    return node if among is None else node & np.asarray(among, bool)


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def hypotheses(P, idx, axis_mode=AXIS_OFF, axis=(0, 0, 1), axis_bound=0.95):
    """P: [M, 3] f32 participants, idx: [H, 3].  (planes f32 [H, 4] with NaN rows for the invalid ones, valid bool [H])"""
    with np.errstate(all="ignore"):
        a, b, c = P[idx[:, 0]], P[idx[:, 1]], P[idx[:, 2]]
        u, v = b - a, c - a
        cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        l2 = (cx * cx + cy * cy) + cz * cz
        assert l2.dtype == F
        valid = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2]) & (l2 > 0) & (l2 <= np.finfo(F).max)
        ln = np.sqrt(l2)
        nx, ny, nz = cx / ln, cy / ln, cz / ln
        d = -dot3(nx, ny, nz, a[:, 0], a[:, 1], a[:, 2])
        if axis_mode != AXIS_OFF:
            ax = np.asarray(axis, F)
            t = dot3(nx, ny, nz, ax[0], ax[1], ax[2])
            neg = t < 0
            nx, ny, nz, d = (np.where(neg, -q, q) for q in (nx, ny, nz, d))
            valid &= (np.abs(t) >= F(axis_bound)) if axis_mode == AXIS_NORMAL else (np.abs(t) <= F(axis_bound))
        pl = np.stack([nx, ny, nz, d], 1).astype(F)
        assert pl.dtype == F
        pl[~valid] = np.nan
    return pl, valid


def inliers(pl, P, N, distance, normal_cos):
    """pl: [..., 4] planes, P / N: [M, 3] positions / normals.  bool [..., M]"""
    pl = np.asarray(pl, F)
    with np.errstate(all="ignore"):
        n = pl[..., None, :]
        e = dot3(n[..., 0], n[..., 1], n[..., 2], P[:, 0], P[:, 1], P[:, 2]) + n[..., 3]
        assert e.dtype == F
        ok = np.abs(e) <= F(distance)
        if F(normal_cos) > 0:
            ok &= np.abs(dot3(n[..., 0], n[..., 1], n[..., 2], N[:, 0], N[:, 1], N[:, 2])) >= F(normal_cos)
    return ok


def finite(x):
    return x - x == 0.0


def rotate(A, V, p, q, r):
    apq = A[p][q]
    if not (apq < 0.0 or apq > 0.0):
        return
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    root = math.sqrt(theta * theta + 1.0) if finite(theta * theta) else math.inf
    t = -1.0 / (root - theta) if theta < 0.0 else 1.0 / (root + theta)
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    A[p][p] = A[p][p] - t * apq
    A[q][q] = A[q][q] + t * apq
    A[p][q] = 0.0
    A[q][p] = 0.0
    arp, arq = A[r][p], A[r][q]
    A[r][p] = c * arp - s * arq
    A[p][r] = A[r][p]
    A[r][q] = s * arp + c * arq
    A[q][r] = A[r][q]
    for k in range(3):
        vkp, vkq = V[k][p], V[k][q]
        V[k][p] = c * vkp - s * vkq
        V[k][q] = s * vkp + c * vkq


def plane_fit(S, m, a, hn):
    """S: nine doubles, m: the inliers, a: the anchor (3 f32), hn: the hypothesis's normal (3 f32).  (n f32 [3], d f32, thickness f32) or None.
    Python floats overflow to inf silently in + - *, raise only in / by zero (never reached: every divisor is tested or >= 1)"""
    if m < 3:
        return None
    S = [float(x) for x in S]
    a = [float(F(x)) for x in a]
    hn = [float(F(x)) for x in hn]
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
    lam, nx, ny, nz = A[0][0], V[0][0], V[1][0], V[2][0]
    if A[1][1] < lam:
        lam, nx, ny, nz = A[1][1], V[0][1], V[1][1], V[2][1]
    if A[2][2] < lam:
        lam, nx, ny, nz = A[2][2], V[0][2], V[1][2], V[2][2]
    if not finite(lam):
        return None
    l2 = (nx * nx + ny * ny) + nz * nz
    ln = math.sqrt(l2) if finite(l2) and l2 >= 0.0 else math.nan
    if not (ln > 0.0) or not finite(ln):
        return None
    nx, ny, nz = nx / ln, ny / ln, nz / ln
    if (nx * hn[0] + ny * hn[1]) + nz * hn[2] < 0.0:
        nx, ny, nz = -nx, -ny, -nz
    d = -((nx * (a[0] + mx) + ny * (a[1] + my)) + nz * (a[2] + mz))
    th = math.sqrt(lam if lam > 0.0 else 0.0)
    if not all(finite(x) for x in (nx, ny, nz, d, th)):
        return None
    with np.errstate(over="ignore"):
        n32, d32, t32 = np.array([nx, ny, nz], np.float64).astype(F), F(d), F(th)
    if not finite(float(d32)) or not finite(float(t32)):
        return None
    return n32, d32, t32


def moments(S, inl, a):
    """the nine sums by map row over the rows of the bool mask inl, q = (double)p - (double)a"""
    q = S[:, :3].astype(np.float64) - np.asarray(a, F).astype(np.float64)[None, :]
    q = np.where(inl[:, None], q, 0.0)
    terms = [q[:, 0], q[:, 1], q[:, 2], q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2], q[:, 1] * q[:, 1], q[:, 1] * q[:, 2],
             q[:, 2] * q[:, 2]]
    return [lane_sum(np.where(inl, t, 0.0)) for t in terms]


def planes(S, among=None, **kw):
    """everything the header defines for one extraction: label uint32 [n], models (list of dicts), result (without count_after's `which`:
    lists() gives it), node bool [n], and per round the debug record rounds[k] = dict(M, counts, planes, valid, idx, rows)"""
    p = dict(DEFAULTS, **kw)
    S = np.ascontiguousarray(S, F).reshape(-1, 12)
    n = len(S)
    node = nodes(S, among, p["min_conf"])
    label = np.full(n, NONE, np.uint32)
    models, rounds = [], []
    H = int(p["hypotheses"])
    for k in range(int(p["max_planes"])):
        rows = np.nonzero(node & (label == NONE))[0]
        M = len(rows)
        if M == 0:
            rounds.append(dict(M=0, best=0))
            break
        P, N = S[rows, 0:3], S[rows, 8:11]
        idx = samples(p["seed"], k, H, M)
        pl, valid = hypotheses(P, idx, p["axis_mode"], p["axis"], p["axis_bound"])
        counts = np.zeros(H, np.int64)
        for a in range(0, H, 64):
            counts[a:a + 64] = inliers(pl[a:a + 64], P, N, p["distance"], p["normal_cos"]).sum(-1)
        assert (counts[~valid] == 0).all()
        h = int(np.argmax(counts))                       # (the first of the greatest)
        best = int(counts[h])
        rounds.append(dict(M=M, counts=counts, planes=pl, valid=valid, idx=idx, rows=rows, best=best, h=h))
        if best == 0 or best < int(p["min_inliers"]):
            break
        final, thickness = pl[h].copy(), F(0)
        if p["refine"] and best >= 3:
            inl = np.zeros(n, bool)
            inl[rows] = inliers(pl[h], P, N, p["distance"], p["normal_cos"])
            anchor = P[idx[h, 0]]
            fit = plane_fit(moments(S, inl, anchor), best, anchor, pl[h, :3])
            if fit is not None:
                final = np.array([fit[0][0], fit[0][1], fit[0][2], fit[1]], F)
                thickness = fit[2]
        on = inliers(final, P, N, p["distance"], p["normal_cos"])
        label[rows[on]] = k
        models.append(dict(normal=final[:3].copy(), d=F(final[3]), inliers=int(on.sum()), sampled_inliers=best, hypothesis=h,
                           valid_hypotheses=int(valid.sum()), participants=M, thickness=F(thickness)))
    on_rows = int((label != NONE).sum())
    result = dict(nodes=int(node.sum()), planes=len(models), on_rows=on_rows, off_rows=int(node.sum()) - on_rows)
    return dict(label=label, models=models, result=result, node=node, rounds=rounds, n=n)


def lists(ref, which=-1):
    """(ON rows, OFF rows, count_after) of planes()'s return value for `which`"""
    label, node = ref["label"], ref["node"]
    on = (label != NONE) & ((which < 0) | (label == np.uint32(which & U32)))
    return (np.nonzero(on)[0].astype(np.uint32), np.nonzero(node & ~on)[0].astype(np.uint32), ref["n"] - int(on.sum()))


def same_model(got, want):
    """every integer equal and the bits of normal, d and thickness"""
    for k in ("inliers", "sampled_inliers", "hypothesis", "valid_hypotheses", "participants"):
        if int(got[k]) != int(want[k]):
            return False
    bits = lambda v: np.asarray(v, F).reshape(-1).view(np.uint32)
    return all(np.array_equal(bits(got[k]), bits(want[k])) for k in ("normal", "d", "thickness"))
