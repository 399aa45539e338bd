"""The outlier filters of include/ef_hip.h ("Remove outlier surfels") restated in numpy from the header alone: an exhaustive neighbour scan in
f32 with the header's bracketing, the P-lane sums and the twelve-round tree in double, the threshold and the flags.  No grid, no index.

numpy's float32 arithmetic rounds once per operation, and its sqrt and division are the correctly rounded IEEE operations."""
import numpy as np

F = np.float32
RADIUS, STATISTICAL = 0, 1
P = 4096
DEFAULTS = dict(mode=STATISTICAL, radius=0.03, min_conf=-1.0, min_neighbors=4, k=8, std_ratio=2.0, max_mean_dist=0.0, flag_sparse=1)


def participants(S, among=None):
    """among: a bool mask of the selected rows, or None"""
    with np.errstate(invalid="ignore"):
        fin = (np.abs(S[:, :3].astype(F)) <= np.finfo(F).max).all(1)
    return fin if among is None else fin & np.asarray(among, bool)


def neighbours(S, radius, min_conf=-1.0, part=None, chunk=512):
    """(count uint32 [n], d2 float32 [n, 16]): per participant the number of ALL neighbours and the d2 of the first 16 in (d2, row) order, +inf
    where there are fewer; count 0 and +inf for a row that does not participate"""
    S = np.ascontiguousarray(S, F)
    n = len(S)
    part = participants(S) if part is None else part
    r = F(radius)
    r2 = F(r * r)
    mc = F(min_conf)
    count = np.zeros(n, np.uint32)
    D = np.full((n, 16), np.inf, F)
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
            qi, tj = np.nonzero(elig)                       # (row-major: tj ascends within a query)
            dd = d2[qi, tj]
            order = np.lexsort((tj, dd, qi))               # by query, then d2, then row
            qi, dd = qi[order], dd[order]
            cnt = np.bincount(qi, minlength=q.stop - q.start)
            count[q] = cnt
            start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
            rank = np.arange(len(qi)) - start[qi]
            keep = rank < 16
            D[a + qi[keep], rank[keep]] = dd[keep]
    return count, D


def mean_dist(count, D, k):
    """mean_s = (((sqrt(d2_1) + sqrt(d2_2)) + ...) + sqrt(d2_k)) / (float)k where count >= k, else +inf"""
    k = int(k)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.sqrt(D[:, 0])
        for j in range(1, k):
            s = s + np.sqrt(D[:, j])
        m = s / F(k)
    assert m.dtype == F
    return np.where(count >= k, m, F(np.inf)).astype(F)


def lane_sum(term):
    """term: float64 per row.  partial[j] = ((term(j) + term(j+P)) + term(j+2P)) + ... from +0.0, then twelve rounds of a[i] = a[2i] + a[2i+1]"""
    term = np.asarray(term, np.float64)
    m = max(1, -(-len(term) // P))
    padded = np.zeros(m * P, np.float64)
    padded[:len(term)] = term
    a = np.zeros(P, np.float64)
    for row in padded.reshape(m, P):
        a = a + row
    for _ in range(12):
        a = a[0::2] + a[1::2]
    assert a.shape == (1,)
    return float(a[0])


def threshold(S1, S2, N, std_ratio, max_mean_dist):
    if F(max_mean_dist) > 0:
        return F(max_mean_dist)
    if N == 0:
        return F(np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        S1, S2, Nd = np.float64(S1), np.float64(S2), np.float64(N)
        mu = S1 / Nd
        var = S2 / Nd - mu * mu
        if var < 0.0:
            var = np.float64(0.0)
        return F(mu + np.float64(F(std_ratio)) * np.sqrt(var))


def outliers(S, among=None, nb=None, **kw):
    """everything the header defines for one call.  nb: neighbours(S, radius, min_conf, part) when the caller has it already"""
    p = dict(DEFAULTS, **kw)
    S = np.ascontiguousarray(S, F)
    part = participants(S, among)
    count, D = neighbours(S, p["radius"], p["min_conf"], part) if nb is None else nb
    k = p["k"] if p["mode"] == STATISTICAL else 1
    mean = mean_dist(count, D, k)
    measured = part & (count >= k)
    sparse = part & ~measured
    if p["mode"] == STATISTICAL:
        m64 = np.where(measured, mean, F(0)).astype(np.float64)
        S1, S2 = lane_sum(m64), lane_sum(m64 * m64)
        thr = threshold(S1, S2, int(measured.sum()), p["std_ratio"], p["max_mean_dist"])
        with np.errstate(invalid="ignore"):
            out = (measured & (mean > thr)) | (sparse & (p["flag_sparse"] != 0))
    else:
        S1 = S2 = 0.0
        thr = F(np.inf)
        out = part & (count < np.uint32(p["min_neighbors"]))
    rows = np.nonzero(out)[0].astype(np.uint32)
    return dict(mean=mean, count=count, part=part, rows=rows,
                result=dict(sum=S1, sum_sq=S2, participants=int(part.sum()), measured=int(measured.sum()), sparse=int(sparse.sum()),
                            outliers=len(rows), count_after=len(S) - len(rows), threshold=thr))
