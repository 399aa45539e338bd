"""ef_map_fuse restated in numpy from include/ef_hip.h alone (the section "Fuse surfels"), shared by test_fuse_host.py and test_gpu_fuse.py.
It stands on insertref (the transform, the match = the insert's gate, the rows an append stores) and on queryref.brute.  All per-record
arithmetic is float32 with one rounding per operation, in the written order; comparisons with NaN are false; records never match one another;
a map surfel takes at most one record per call."""
import numpy as np

import insertref as ir
from queryref import MISS

F = np.float32
KEEP = ir.KEEP
SKIPPED, NOVEL, WEIGHTLESS, ABSORBED, FUSED, INSERTED = 0, 1, 2, 3, 4, 5   # EF_FUSE_*


def default_params(tick, **kw):
    """ef_default_fuse_params as a dict"""
    p = dict(min_separation=0.01, min_conf=-1.0, min_normal_cos=0.5, append=1, init_time=int(tick), last_time=int(tick))
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


def as_insert(params):
    """the ef_insert_params whose gate is the fuse's match and whose append is the fuse's"""
    return dict(gate=1, min_separation=params["min_separation"], min_conf=params["min_conf"], min_normal_cos=params["min_normal_cos"],
                init_time=params["init_time"], last_time=params["last_time"])


def d2_of(p, ps):
    """point 2: the query's expression between p' and the stored positions, row by row"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (p[:, j] - ps[:, j] for j in range(3))
        return (dx * dx + dy * dy) + dz * dz


def decode(c):
    """a colour float -> three float32 channels: (int)c toward zero (saturated outside int, NaN -> 0), byte / 255.0f"""
    c = np.asarray(c, F).astype(np.float64)
    ic = np.clip(np.trunc(np.where(np.isnan(c), 0.0, c)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
    return [((ic >> s) & 0xFF).astype(F) / F(255) for s in (16, 8, 0)]


def int_or_indefinite(v):
    """roundf (half away from zero) of float32 values, then (unsigned)(int) inside int's range and 0x80000000 outside it or for NaN"""
    v = np.asarray(v, F).astype(np.float64)
    with np.errstate(invalid="ignore"):
        q = np.where(np.abs(v) < 2.0 ** 23, np.trunc(v + np.copysign(0.5, v)), v)     # (exact in float64; from 2^23 on a float32 is whole)
        ok = (q >= -2.0 ** 31) & (q < 2.0 ** 31)
    return np.where(ok, np.where(ok, q, 0).astype(np.int64) & 0xFFFFFFFF, 0x80000000).astype(np.int64)


def encode_merged(ch):
    with np.errstate(invalid="ignore", over="ignore"):
        u = [int_or_indefinite(c * F(255)) for c in ch]
    rgb = ((((u[0] << 8) + u[1]) & 0xFFFFFFFF) << 8) + u[2] & 0xFFFFFFFF
    return rgb.astype(np.uint32).view(np.int32).astype(F)


def merge(rows, p, m, rec, last_time):
    """point 3 for k (row, winner) pairs: rows k x 12 stored, p / m k x 3 the moved position and normal, rec k x 12 the records; the rows after"""
    rows = np.ascontiguousarray(rows, F).reshape(-1, 12).copy()
    rec = np.ascontiguousarray(rec, F).reshape(-1, 12)
    ck, a = rows[:, 3].copy(), rec[:, 3]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        def avg(old, new):
            return ((ck * old) + (a * new)) / (ck + a)
        full = rec[:, 11] < (F(1.0) + F(0.5)) * rows[:, 11]
        out = rows.copy()
        for j in range(3):
            out[:, j] = avg(rows[:, j], p[:, j])
        v = [avg(rows[:, 8 + j], m[:, j]) for j in range(3)]
        dot = (v[2] * v[2]) + ((v[1] * v[1]) + (v[0] * v[0]))
        rn = F(1.0) / np.sqrt(dot)
        for j in range(3):
            out[:, 8 + j] = v[j] * rn
        out[:, 11] = avg(rows[:, 11], rec[:, 11])
        old, new = decode(rows[:, 4]), decode(rec[:, 4])
        out[:, 4] = encode_merged([avg(o, n) for o, n in zip(old, new)])
        assert out.dtype == F and dot.dtype == F and rn.dtype == F
        rows[full] = out[full]
        rows[:, 3] = ck + a
    rows[:, 7] = rec[:, 7] if int(last_time) == KEEP else F(int(last_time))
    return rows


def fuse(old, records, T, params, capacity=None, known=None):
    """dict(result, new_row, match_row, outcome, map, refused): what ef_map_fuse returns and leaves.  known: insertref.outcome() of these
    records when the caller has it already"""
    old = np.ascontiguousarray(old, F).reshape(-1, 12)
    R = np.ascontiguousarray(records, F).reshape(-1, 12)
    n, n0 = len(R), len(old)
    append = int(params["append"])
    assert append in (0, 1)
    skipped, matched, nearest = ir.outcome(old, R, T, as_insert(params)) if known is None else known
    novel = ~skipped & ~matched
    p, m = ir.move(R, T)
    a = R[:, 3]
    with np.errstate(invalid="ignore"):
        competes = matched & (a > 0) & (a < np.inf)
    outcome = np.full(n, SKIPPED, np.uint8)
    outcome[novel] = INSERTED if append else NOVEL
    outcome[matched & ~competes] = WEIGHTLESS
    outcome[competes] = ABSORBED
    idx = np.nonzero(competes)[0]
    row = nearest[idx].astype(np.int64)
    d2 = d2_of(p[idx], old[row, :3])
    assert np.isfinite(d2).all() and (d2 >= 0).all()
    order = np.lexsort((idx, d2.view(np.uint32), row))          # by row, then d2 (its bits: monotone for finite d2 >= 0), then record index
    first = np.ones(len(order), bool)
    first[1:] = row[order][1:] != row[order][:-1]
    win, win_row = idx[order][first], row[order][first]
    outcome[win] = FUSED
    match_row = np.where(matched, nearest, MISS).astype(np.uint32)
    new_row = np.full(n, MISS, np.uint32)
    app = int(novel.sum()) if append else 0
    if append:
        new_row[novel] = n0 + np.arange(app, dtype=np.uint32)
    result = dict(fused=len(win), absorbed=int(competes.sum()) - len(win), weightless=int((matched & ~competes).sum()), novel=int(novel.sum()),
                  skipped=int(skipped.sum()), inserted=app, count_after=n0 + app)
    if capacity is not None and n0 + app > capacity:
        result["count_after"] = n0
        return dict(result=result, new_row=None, match_row=match_row, outcome=outcome, map=old.copy(), refused=True)
    out = old.copy()
    out[win_row] = merge(old[win_row], p[win], m[win], R[win], params["last_time"])
    if append:
        out = np.concatenate([out, ir.stored_rows(R, T, as_insert(params))[novel]])
    return dict(result=result, new_row=new_row, match_row=match_row, outcome=outcome, map=out, refused=False)
