"""ef_map_insert restated in numpy from include/ef_hip.h alone (the section "Insert surfels"), shared by test_insert_host.py and
test_gpu_insert.py: the transform, the novelty gate (on queryref.brute, the exhaustive scan of ef_query_nearest), the outcome per record and the
map an insert leaves.  All per-record arithmetic is float32 with one rounding per operation, in the written order; comparisons with NaN are
false; records never gate one another."""
import numpy as np

from queryref import MISS, brute

F = np.float32
KEEP = -1   # EF_INSERT_KEEP


def default_params(tick, **kw):
    """ef_default_insert_params as a dict"""
    p = dict(gate=1, min_separation=0.01, min_conf=-1.0, min_normal_cos=0.5, init_time=int(tick), last_time=int(tick))
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


def move(records, T):
    """(p' n x 3, m' n x 3): T None copies bit for bit; else Rf, tf = T rounded to float32 once,
    p' = ((R0*x + R1*y) + R2*z) + t and m' = (R0*mx + R1*my) + R2*mz per axis"""
    R = np.ascontiguousarray(records, F).reshape(-1, 12)
    p, m = R[:, 0:3].copy(), R[:, 8:11].copy()
    if T is None:
        return p, m
    Tf = np.asarray(T, np.float64).reshape(4, 4).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        pp = np.stack([((Tf[a, 0] * p[:, 0] + Tf[a, 1] * p[:, 1]) + Tf[a, 2] * p[:, 2]) + Tf[a, 3] for a in range(3)], 1)
        mm = np.stack([(Tf[a, 0] * m[:, 0] + Tf[a, 1] * m[:, 1]) + Tf[a, 2] * m[:, 2] for a in range(3)], 1)
    assert pp.dtype == F and mm.dtype == F
    return pp, mm


def normal_cos(m, ns):
    with np.errstate(invalid="ignore", over="ignore"):
        return (m[:, 0] * ns[:, 0] + m[:, 1] * ns[:, 1]) + m[:, 2] * ns[:, 2]


def outcome(old, records, T, params):
    """per record: (skipped, duplicate, nearest) — nearest = the row ef_query_nearest gives for p' on the OLD map (MISS without the gate)"""
    old = np.ascontiguousarray(old, F).reshape(-1, 12)
    p, m = move(records, T)
    n = len(p)
    skipped = ~np.isfinite(p).all(1)
    dup = np.zeros(n, bool)
    nearest = np.full(n, MISS, np.uint32)
    if int(params["gate"]) and n:
        nearest = brute(p, old, params["min_separation"], params["min_conf"])[0][:, 0]
        hit = nearest != MISS
        dup = hit.copy()
        if F(params["min_normal_cos"]) > F(-1):
            c = normal_cos(m[hit], old[nearest[hit].astype(np.int64), 8:11])
            with np.errstate(invalid="ignore"):
                dup[hit] = c >= F(params["min_normal_cos"])
    assert not (dup & skipped).any()   # a non-finite position never matches
    return skipped, dup, nearest


def stored_rows(records, T, params):
    """the rows the records would be stored as: moved position and normal, zero ID bits, the two times as the params say"""
    R = np.ascontiguousarray(records, F).reshape(-1, 12)
    out = R.copy()
    p, m = move(R, T)
    out[:, 0:3], out[:, 8:11] = p, m
    out[:, 5] = 0
    if int(params["init_time"]) != KEEP:
        out[:, 6] = F(int(params["init_time"]))
    if int(params["last_time"]) != KEEP:
        out[:, 7] = F(int(params["last_time"]))
    return out


def insert(old, records, T, params, capacity=None, known=None):
    """dict(result, new_row, match_row, map): what ef_map_insert returns and leaves.  capacity given and exceeded: map = old, count_after =
    the old count, new_row None (the header leaves it unwritten).  known: outcome() of these records when the caller has it already (the
    outcome of a record depends on the old map alone, so that of a repeated record is that of its first copy)"""
    old = np.ascontiguousarray(old, F).reshape(-1, 12)
    R = np.ascontiguousarray(records, F).reshape(-1, 12)
    skipped, dup, nearest = outcome(old, R, T, params) if known is None else known
    ins = ~skipped & ~dup
    n0 = len(old)
    match_row = np.where(dup, nearest, MISS).astype(np.uint32)
    new_row = np.full(len(R), MISS, np.uint32)
    new_row[ins] = n0 + np.arange(int(ins.sum()), dtype=np.uint32)
    result = dict(inserted=int(ins.sum()), duplicates=int(dup.sum()), skipped=int(skipped.sum()), count_after=n0 + int(ins.sum()))
    if capacity is not None and n0 + int(ins.sum()) > capacity:
        result["count_after"] = n0
        return dict(result=result, new_row=None, match_row=match_row, map=old.copy(), refused=True)
    return dict(result=result, new_row=new_row, match_row=match_row, map=np.concatenate([old, stored_rows(R, T, params)[ins]]), refused=False)
