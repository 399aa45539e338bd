"""Fuse surfels into the map on the device (ef_map_fuse, include/ef_hip.h; kernels in elasticfusion_amd/csrc/ef_fuse.inc).

The fuse is restated in numpy from the header alone (tests/fuseref.py, on insertref and the exhaustive scan of queryref): the match, the election
of one record per map surfel, the weighted merge in float32 in the written order, the append.  The device must give the same result, the same
new_row / match_row / outcome and the same map, bit for bit; and a context that fuses and keeps mapping must compute what a fresh context
computes after uploadMap(the reference's map) + restore, bit for bit.  There are no tolerances here.
"""
import ctypes as C

import numpy as np
import pytest

import fuseref as fr
import insertref as ir
from queryref import MISS, assert_bits_equal, brute, default_cell
from test_gpu_insert import cos_of, d2_of, normal_at_cos, point_at_d2, record_at, surfel_at, unit
from test_gpu_select import scene_T, state_of, step, u32

pytestmark = pytest.mark.gpu

F = np.float32
SEP = F(0.01)
R2 = SEP * SEP
MIN_CONF = F(-1.0)       # a surfel is eligible iff its confidence is ABOVE it: one at exactly -1 is not, one at 0 is
COS = F(0.5)
RADIUS_S = F(0.005)
BOUND = (F(1.0) + F(0.5)) * RADIUS_S
SENTINEL = 0xABABABAB
RESULT_KEYS = ("fused", "absorbed", "weightless", "novel", "skipped", "inserted", "count_after")


def params_of(append=1, cos=COS, init_time=ir.KEEP, last_time=ir.KEEP, sep=SEP, min_conf=MIN_CONF):
    return fr.default_params(0, min_separation=sep, min_conf=min_conf, min_normal_cos=cos, append=append, init_time=init_time, last_time=last_time)


def to_api(ef, p):
    return ef.fuseParams(min_separation=float(p["min_separation"]), min_conf=float(p["min_conf"]), min_normal_cos=float(p["min_normal_cos"]),
                         append=int(p["append"]), init_time=int(p["init_time"]), last_time=int(p["last_time"]))


def check_fuse(got, exp, ef, what):
    res, new, match, outcome = got
    assert res == exp["result"], (what, res, exp["result"])
    assert new.dtype == np.uint32 and np.array_equal(new, exp["new_row"]), (what, np.nonzero(new != exp["new_row"])[0][:8])
    assert np.array_equal(match, exp["match_row"]), (what, np.nonzero(match != exp["match_row"])[0][:8])
    assert outcome.dtype == np.uint8 and np.array_equal(outcome, exp["outcome"]), (what, np.nonzero(outcome != exp["outcome"])[0][:8],
                                                                                     outcome[outcome != exp["outcome"]][:8])
    assert ef.lastCount() == exp["result"]["count_after"], what
    assert_bits_equal(ef.downloadMap(), exp["map"], what + ": the map")


def local_outcome(old, R, T, prm):
    """insertref.outcome for records that lie in a small part of a large map: the exhaustive scan over the map rows inside the records' bounding
    box widened by twice the separation (a superset of every row within the separation of a record; ascending, so ties still go to the lower
    row), with the rows translated back"""
    p = ir.move(R, T)[0]
    fin = np.isfinite(p).all(1)
    lo, hi = p[fin].min(0) - 2 * SEP, p[fin].max(0) + 2 * SEP
    sub = np.nonzero(((old[:, :3] >= lo) & (old[:, :3] <= hi)).all(1))[0]
    skipped, matched, near = ir.outcome(old[sub], R, T, fr.as_insert(prm))
    hit = near != MISS
    near[hit] = sub[near[hit].astype(np.int64)]
    return skipped, matched, near


def patch_rows(m, half, rng, count):
    """`count` rows of m within `half` metres (per axis) of the surfel in the middle of the map"""
    c = m[len(m) // 2, :3]
    rows = np.nonzero((np.abs(m[:, :3] - c) < F(half)).all(1))[0]
    assert len(rows) >= count, (len(rows), count)
    return np.sort(rng.choice(rows, count, replace=False))


def fuse_dev(ef, rec, T, params, pad=16):
    """ef_map_fuse_dev with sentinels behind the three arrays: (result dict, new_row, match_row, outcome)"""
    from elasticfusion_amd import api
    n = len(rec)
    d_rec = api.DevBuf.from_array(rec) if n else None
    d_new = api.DevBuf.from_array(np.full(n + pad, SENTINEL, np.uint32))
    d_match = api.DevBuf.from_array(np.full(n + pad, SENTINEL, np.uint32))
    d_out = api.DevBuf.from_array(np.full(n + pad, 0xAB, np.uint8))
    keep, pT = api._pose16(T)
    res = api.ef_fuse_result()
    rc = api.lib().ef_map_fuse_dev(ef.h, d_rec.p if n else None, C.c_uint32(n), pT, C.byref(params), C.byref(res), d_new.p, d_match.p, d_out.p)
    assert rc == 0, (rc, api.lib().ef_last_error(ef.h))
    new, match, out = d_new.to_array(np.uint32, n + pad), d_match.to_array(np.uint32, n + pad), d_out.to_array(np.uint8, n + pad)
    assert (new[n:] == SENTINEL).all() and (match[n:] == SENTINEL).all() and (out[n:] == 0xAB).all(), "the device variant wrote beyond its outputs"
    return {k: int(getattr(res, k)) for k in RESULT_KEYS}, new[:n], match[:n], out[:n]


@pytest.fixture(scope="module")
def ctx():
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    yield ef
    ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the edge scene (pure numpy: what it contains is asserted on the reference before the device is asked anything)
# ---------------------------------------------------------------------------------------------------------------------------------------
def edge_scene():
    """(map S, records R, T, names): one isolated cluster per case, 0.25 m apart, then a small random background; `names` maps a case to its
    record(s) and map row(s)"""
    rng = np.random.default_rng(91)
    T = scene_T()
    Ti = np.linalg.inv(T)
    S, R, names = [], [], {}
    direction = (0.58, 0.71, 0.40)
    k = [0]

    def centre():
        c = np.array([-3.0 + 0.25 * k[0], 0.1 * (k[0] % 3), 0.3])
        k[0] += 1
        return c

    def new_record(c, normal=(0.0, 0.0, 1.0), offset=(0.0, 0.0, 0.0), **kw):
        R.append(record_at(Ti, c + np.asarray(offset), unit(normal), **kw))
        p, m = ir.move(R[-1], T)
        return len(R) - 1, p[0], m[0]

    def surfel(pos, normal, conf=5.0, colour=0x0A0B0C, radius=RADIUS_S):
        s = surfel_at(pos, normal, conf=conf)
        s[4], s[11] = colour, radius
        S.append(s)
        return len(S) - 1

    def beside(p, mm):
        return (p.astype(np.float64) + unit(direction) * mm * 1e-3).astype(F)

    for name, target in (("d2_below", step(R2, False)), ("d2_at", R2), ("d2_above", step(R2, True))):
        i, p, m = new_record(centre(), (0.2, -0.3, 0.9))
        names[name] = (i, surfel(point_at_d2(p, direction, target), m))
    for name, target in (("cos_below", step(COS, False)), ("cos_at", COS)):
        i, p, m = new_record(centre(), (-0.4, 0.5, 0.7))
        names[name] = (i, surfel(beside(p, 3), normal_at_cos(m, target)))
    # the nearest surfel is not eligible (its confidence is not above min_conf): the farther one takes the record
    i, p, m = new_record(centre())
    names["conf"] = (i, surfel(beside(p, 2), m, conf=float(MIN_CONF)), surfel(beside(p, -6), m))
    for name, a in (("a_zero", 0.0), ("a_negative", -1.0), ("a_inf", np.inf), ("a_nan", np.nan)):
        i, p, m = new_record(centre(), conf=a)
        names[name] = (i, surfel(beside(p, 2), m))
    i, p, m = new_record(centre())
    R[i][1] = np.nan
    names["nan_pos"] = (i,)
    for name, radius in (("radius_below", np.nextafter(BOUND, F(0))), ("radius_at", BOUND), ("radius_above", np.nextafter(BOUND, F(1)))):
        i, p, m = new_record(centre(), (0.1, 0.2, 0.95), radius=float(radius), colour=0x654321)
        names[name] = (i, surfel(beside(p, 2), unit((0.0, 0.1, 1.0)).astype(F)))
    # two records at the same position (bit-identical d2) beside one surfel, a third farther away before them
    c = centre()
    i0, p, m = new_record(c, offset=(0.004, 0, 0), conf=9.0)
    i1, p, m = new_record(c, conf=2.0, colour=0x111111)
    i2, _, _ = new_record(c, conf=3.0, colour=0xEEEEEE)
    names["tie"] = (i0, i1, i2, surfel(beside(p, 2), m))
    # the later record is the nearer one
    c = centre()
    i0, p0, m = new_record(c, offset=(0.003, 0, 0), conf=4.0)
    i1, p1, m = new_record(c, conf=1.5)
    names["later_nearer"] = (i0, i1, surfel(beside(p1, 1), m))
    # a surfel with no confidence yet takes the record whole
    i, p, m = new_record(centre(), (0.3, 0.1, 0.9), conf=2.0, colour=0x102030)
    names["ck_zero"] = (i, surfel(beside(p, 2), unit((0.0, 0.0, 1.0)).astype(F), conf=0.0))
    # a stored colour with 255 in two channels
    i, p, m = new_record(centre(), conf=1.0, colour=0x00FF01)
    names["colour_255"] = (i, surfel(beside(p, 2), m, colour=0xFF80FF))
    assert k[0] <= 24
    # the background: surfels in [2, 3]^3, records beside half of them (up to 15 mm away) and a few anywhere
    nb = 400 - len(S)
    B = np.zeros((nb, 12), F)
    B[:, :3] = rng.uniform(2, 3, (nb, 3))
    B[:, 3] = rng.uniform(0, 8, nb)
    nrm = rng.normal(size=(nb, 3))
    B[:, 8:11] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    B[:, 4], B[:, 6], B[:, 7], B[:, 11] = rng.integers(0, 1 << 24, nb), rng.integers(1, 9, nb), 9, rng.uniform(0.003, 0.008, nb)
    S = np.concatenate([np.array(S, F), B])
    for j in range(260):
        if j < 200:
            off = rng.normal(size=3)
            off *= rng.uniform(0, 0.015) / np.linalg.norm(off)
            b = B[j % 60]                                           # (several records per surfel)
            target = b[:3].astype(np.float64) + off
            normal = b[8:11].astype(np.float64) if j % 3 else unit(rng.normal(size=3))
        else:
            target, normal = rng.uniform(2, 3, 3), unit(rng.normal(size=3))
        R.append(record_at(Ti, target, normal, conf=float(rng.uniform(0.01, 12)), colour=int(rng.integers(0, 1 << 24)), idbits=1000 + j,
                           t0=float(rng.integers(1, 9)), t1=float(10 + j % 7), radius=float(rng.uniform(0.002, 0.012))))
    return S, np.array(R, F), T, names


def plain_records(R, T):
    """the records for T = None: the moved position and normal stored as the record's own, so that every edge stays where it is"""
    P = R.copy()
    P[:, :3], P[:, 8:11] = ir.move(R, T)
    return P


def test_the_scene_contains_every_edge_the_header_names():
    """CPU only in effect (no device call): the reference alone shows that the edges are exercised"""
    S, R, T, names = edge_scene()
    assert len(S) == 400 and len(R) > 256
    for Rx, Tx in ((R, T), (plain_records(R, T), None)):
        p, m = ir.move(Rx, Tx)
        exp = fr.fuse(S, Rx, Tx, params_of(append=1, last_time=31))
        out, match, M = exp["outcome"], exp["match_row"], exp["map"]
        near_all = brute(p, S, SEP, -np.inf)[0][:, 0]
        for name, want in (("d2_below", fr.FUSED), ("d2_at", fr.FUSED), ("d2_above", fr.INSERTED)):
            i, s = names[name]
            d2 = d2_of(p[i], S[s, :3])[0]
            assert d2 == {"d2_below": step(R2, False), "d2_at": R2, "d2_above": step(R2, True)}[name] and out[i] == want, name
            assert match[i] == (s if want == fr.FUSED else MISS)
        for name, want in (("cos_below", fr.INSERTED), ("cos_at", fr.FUSED)):
            i, s = names[name]
            assert cos_of(m[i], S[s, 8:11])[0] == (COS if name == "cos_at" else step(COS, False)) and out[i] == want, name
        i, a, b = names["conf"]
        assert near_all[i] == a and match[i] == b and out[i] == fr.FUSED and u32(M[a]).tolist() == u32(S[a]).tolist()
        for name in ("a_zero", "a_negative", "a_inf", "a_nan"):
            i, s = names[name]
            assert out[i] == fr.WEIGHTLESS and match[i] == s and u32(M[s]).tolist() == u32(S[s]).tolist(), name
        i, = names["nan_pos"]
        assert out[i] == fr.SKIPPED and match[i] == MISS
        for name, full in (("radius_below", True), ("radius_at", False), ("radius_above", False)):
            i, s = names[name]
            assert out[i] == fr.FUSED and M[s, 3] == S[s, 3] + Rx[i, 3] and M[s, 7] == 31, name
            assert (M[s, 0] != S[s, 0]) == full and (M[s, 4] != S[s, 4]) == full and (M[s, 11] != S[s, 11]) == full and (M[s, 8] != S[s, 8]) == full
        i0, i1, i2, s = names["tie"]
        assert (match[[i0, i1, i2]] == s).all() and out[[i0, i1, i2]].tolist() == [fr.ABSORBED, fr.FUSED, fr.ABSORBED]
        assert d2_of(p[i1], S[s, :3])[0] == d2_of(p[i2], S[s, :3])[0] < d2_of(p[i0], S[s, :3])[0]
        assert M[s, 3] == S[s, 3] + Rx[i1, 3]
        i0, i1, s = names["later_nearer"]
        assert out[[i0, i1]].tolist() == [fr.ABSORBED, fr.FUSED] and M[s, 3] == S[s, 3] + Rx[i1, 3]
        i, s = names["ck_zero"]
        assert out[i] == fr.FUSED and S[s, 3] == 0 and M[s, 3] == Rx[i, 3] and int(M[s, 4]) == 0x102030
        assert u32(M[s, :3]).tolist() == u32(p[i]).tolist(), "(0 * old + a * new) / (0 + a) is the record's position"
        i, s = names["colour_255"]
        assert out[i] == fr.FUSED and int(S[s, 4]) == 0xFF80FF and (int(M[s, 4]) >> 16) & 0xFF not in (0, 255)
        # the background has every outcome in number
        res = exp["result"]
        assert res["fused"] > 40 and res["absorbed"] > 15 and res["weightless"] == 4 and res["inserted"] > 60 and res["skipped"] == 1, res
        # the ID lane and the creation time of every old row are untouched
        assert_bits_equal(np.ascontiguousarray(M[:400, 5:7]), np.ascontiguousarray(S[:, 5:7]), "ID lane and creation time")


@pytest.mark.parametrize("moved", (True, False))
def test_edge_scene_equals_the_reference_exactly(ctx, moved):
    ef = ctx
    S, R, T, names = edge_scene()
    if not moved:
        R, T = plain_records(R, T), None
    for append in (1, 0):
        for last_time in (31, ir.KEEP):
            prm = params_of(append=append, init_time=4 if last_time != ir.KEEP else ir.KEEP, last_time=last_time)
            exp = fr.fuse(S, R, T, prm)
            for device in (False, True):
                what = f"T {moved} append {append} last_time {last_time} device {device}"
                ef.uploadMap(S)
                got = fuse_dev(ef, R, T, to_api(ef, prm)) if device else ef.fuseSurfels(R, T=T, params=to_api(ef, prm), rows=True)
                check_fuse(got, exp, ef, what)
            print(f"T {moved} append {append} last_time {last_time}:", exp["result"])
    # without the normal test the record below the cosine is fused too; and without the row arrays
    prm = params_of(cos=F(-1), last_time=7)
    exp = fr.fuse(S, R, T, prm)
    assert exp["outcome"][names["cos_below"][0]] == fr.FUSED
    ef.uploadMap(S)
    assert ef.fuseSurfels(R, T=T, params=to_api(ef, prm)) == exp["result"]
    assert_bits_equal(ef.downloadMap(), exp["map"], "no normal test, no row arrays")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. contention and chunk edges
# ---------------------------------------------------------------------------------------------------------------------------------------
def plain_surfels(pos, conf=5.0):
    pos = np.asarray(pos, F).reshape(-1, 3)
    S = np.zeros((len(pos), 12), F)
    S[:, :3] = pos
    S[:, 3], S[:, 4], S[:, 6], S[:, 7], S[:, 10], S[:, 11] = conf, 0x406080, 1, 2, 1, 0.005
    return S


def test_six_hundred_records_contend_for_one_surfel(ctx):
    ef = ctx
    S = plain_surfels([(0.0, 0.0, 0.5), (1.0, 0.0, 0.5), (0.0, 1.0, 0.5)])
    j = (np.arange(600) - 417) % 600                                    # 0 at index 417
    R = plain_surfels(np.stack([0.001 + 0.00001 * j, 0 * j, 0.5 + 0 * j], 1), conf=1.0)
    R[:, 3] = 0.5 + np.arange(600) % 7
    R[:, 4] = np.arange(600) * 1000
    prm = params_of()
    exp = fr.fuse(S, R, None, prm)
    d2 = fr.d2_of(R[:, :3], np.repeat(S[:1, :3], 600, 0))
    assert len(np.unique(d2)) == 600 and np.argmin(d2) == 417
    assert exp["result"] == dict(fused=1, absorbed=599, weightless=0, novel=0, skipped=0, inserted=0, count_after=3)
    assert exp["outcome"][417] == fr.FUSED and (np.delete(exp["outcome"], 417) == fr.ABSORBED).all()
    for device in (False, True):
        ef.uploadMap(S)
        got = fuse_dev(ef, R, None, to_api(ef, prm)) if device else ef.fuseSurfels(R, params=to_api(ef, prm), rows=True)
        check_fuse(got, exp, ef, f"contention, device {device}")


@pytest.mark.parametrize("n", (1, 255, 256, 257, 513))
def test_a_chunk_boundary_between_every_pair_of_outcomes(ctx, n):
    ef = ctx
    i = np.arange(n)
    S = plain_surfels(np.stack([0.1 * (i % 32), 0.1 * (i // 32), 0.5 + 0 * i], 1))
    R = np.repeat(S, 3, 0)                                              # {novel, match, weightless} per surfel
    R[0::3, 2] += F(1.0)
    R[1::3, 0] += F(0.001)
    R[2::3, 0] += F(0.002)
    R[:, 3] = 2.0
    R[2::3, 3] = 0.0
    R[:, 4] = np.arange(3 * n)
    prm = params_of(init_time=3, last_time=4)
    exp = fr.fuse(S, R, None, prm)
    assert exp["outcome"].tolist() == [fr.INSERTED, fr.FUSED, fr.WEIGHTLESS] * n
    ef.uploadMap(S)
    check_fuse(ef.fuseSurfels(R, params=to_api(ef, prm), rows=True), exp, ef, f"pattern x {n}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. a random scene that cannot pass vacuously, and the composition with the insert
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_scene():
    rng = np.random.default_rng(2024)
    n0, third = 4096, 2000
    S = plain_surfels(np.stack([rng.uniform(0, 2, n0), rng.uniform(0, 2, n0), np.full(n0, 0.5)], 1))
    S[:, 3] = rng.uniform(0, 12, n0)
    S[:, 4] = rng.integers(0, 1 << 24, n0)
    S[:, 11] = rng.uniform(0.003, 0.008, n0)
    pick = rng.choice(n0, third, replace=False)

    def jittered(rows, lift=0.0):
        r = S[rows].copy()
        off = rng.normal(size=(len(rows), 3))
        off *= (rng.uniform(0, 0.003, len(rows)) / np.linalg.norm(off, axis=1))[:, None]
        r[:, :3] = (r[:, :3].astype(np.float64) + off + (0, 0, lift)).astype(F)
        r[:, 3] = 20.0 - rng.uniform(0, 20, len(rows))               # (0, 20]
        r[:, 4] = rng.integers(0, 1 << 24, len(rows))
        r[:, 7] = rng.integers(3, 30, len(rows))
        r[:, 11] = rng.uniform(0.003, 0.012, len(rows))
        return r

    R = np.concatenate([jittered(pick), jittered(pick), jittered(rng.choice(n0, third, replace=False), lift=0.05)])
    R = R[rng.permutation(len(R))]
    w = 0.3
    T = np.array([[np.cos(w), -np.sin(w), 0, 0.25], [np.sin(w), np.cos(w), 0, -0.5], [0, 0, 1, 0.125], [0, 0, 0, 1]])
    from elasticfusion_amd import accuracy
    R = accuracy.move_surfels(R, np.linalg.inv(T))
    prm = params_of(init_time=5, last_time=40)
    exp = fr.fuse(S, R, T, prm)
    res, n = exp["result"], len(R)
    # on the reference's output, before the device is asked anything: every kind of work is there in number
    assert res["fused"] >= n // 5 and res["absorbed"] >= n // 5 and res["inserted"] >= n // 5, res
    return dict(S=S, R=R, T=T, prm=prm, exp=exp)


def test_random_scene_equals_the_reference_exactly(ctx, random_scene):
    ef, sc = ctx, random_scene
    print("random scene:", sc["exp"]["result"])
    for device in (False, True):
        ef.uploadMap(sc["S"])
        got = fuse_dev(ef, sc["R"], sc["T"], to_api(ef, sc["prm"])) if device else \
            ef.fuseSurfels(sc["R"], T=sc["T"], params=to_api(ef, sc["prm"]), rows=True)
        check_fuse(got, sc["exp"], ef, f"random scene, device {device}")


def test_the_append_composes_with_the_insert(ctx, random_scene):
    ef, sc = ctx, random_scene
    S, R, T, prm = sc["S"], sc["R"], sc["T"], sc["prm"]
    n0 = len(S)
    ef.uploadMap(S)
    res, new, match, outcome = ef.fuseSurfels(R, T=T, params=to_api(ef, prm), rows=True)
    fused_map = ef.downloadMap()
    ef.uploadMap(S)
    ires, inew, imatch = ef.insertSurfels(R, T=T, rows=True, gate=1, min_separation=float(SEP), min_conf=float(MIN_CONF),
                                          min_normal_cos=float(COS), init_time=5, last_time=40)
    inserted_map = ef.downloadMap()
    assert res["inserted"] == ires["inserted"] > 0 and res["count_after"] == ires["count_after"] and np.array_equal(new, inew)
    assert np.array_equal(match, imatch) and res["fused"] + res["absorbed"] + res["weightless"] == ires["duplicates"]
    assert_bits_equal(fused_map[n0:], inserted_map[n0:], "the appended rows are the insert's")
    assert_bits_equal(inserted_map[:n0], S, "the insert leaves the old rows")
    # append = 0: the count stays, rows that are nobody's match keep their bits, the matched ones are the fuse's
    ef.uploadMap(S)
    res0, new0, match0, outcome0 = ef.fuseSurfels(R, T=T, params=to_api(ef, dict(prm, append=0)), rows=True)
    m0 = ef.downloadMap()
    assert res0 == dict(res, inserted=0, count_after=n0) and len(m0) == n0 and (new0 == MISS).all() and np.array_equal(match0, match)
    assert np.array_equal(np.where(outcome0 == fr.NOVEL, fr.INSERTED, outcome0), outcome) and (outcome0 != fr.INSERTED).all()
    quiet = np.setdiff1d(np.arange(n0), match[outcome == fr.FUSED])
    assert len(quiet) > 1000 and len(quiet) == n0 - res["fused"]
    assert_bits_equal(m0[quiet], S[quiet], "rows that took no record")
    assert_bits_equal(m0, fused_map[:n0], "the fused rows do not depend on append")
    changed = (u32(m0) != u32(S)).any(1)
    assert changed.sum() == res["fused"], "every fused row changed (its confidence rose)"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. IDs and labels
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_ids_and_labels_follow_a_fuse(frames):
    from elasticfusion_amd import api
    NC = 3
    ef = api.ElasticFusion()
    try:
        ef.setSurfelIds(True)
        ef.enableLabels(NC)
        for k in range(3):
            ef.processFrame(frames[k][0], frames[k][1], k)
        ef.surfelIds()                                                  # an ID-consuming call: every row is numbered
        before = ef.downloadMap()
        n0 = len(before)
        ids = u32(before[:, 5]).astype(np.int64)
        assert ids.min() >= 1 and (np.diff(ids) > 0).all()
        rng = np.random.default_rng(6)
        P = rng.dirichlet(np.ones(NC), n0).astype(F)
        ef.setLabels(P)
        rows = patch_rows(before, 0.25, rng, 600)
        near = before[rows].copy()
        near[:, :3] += rng.uniform(-0.0005, 0.0005, (600, 3)).astype(F)
        near[:, 3] = 3.0
        far = before[rows[:200]].copy()
        far[:, 2] += F(30.0)
        R = np.concatenate([near, far])
        R[:, 5] = (90000 + np.arange(len(R))).astype(np.uint32).view(F)      # IDs of another session: never kept
        prm = params_of(min_conf=F(-1.0), cos=F(-1), init_time=2, last_time=2)
        exp = fr.fuse(before, R, None, prm, known=local_outcome(before, R, None, prm))
        assert exp["result"]["fused"] > 300 and exp["result"]["inserted"] == 200, exp["result"]
        res, new, match, outcome = ef.fuseSurfels(R, params=to_api(ef, prm), rows=True)
        assert res == exp["result"] and np.array_equal(outcome, exp["outcome"]) and np.array_equal(match, exp["match_row"])
        after = ef.downloadMap()
        assert_bits_equal(after[:n0], exp["map"][:n0], "the fused old rows, ID lane included")
        assert_bits_equal(np.ascontiguousarray(after[:n0, 5]), np.ascontiguousarray(before[:, 5]), "fused rows keep their IDs")
        cols = [c for c in range(12) if c != 5]
        assert_bits_equal(np.ascontiguousarray(after[n0:, cols]), np.ascontiguousarray(exp["map"][n0:, cols]), "the appended rows")
        ids2 = u32(after[:, 5]).astype(np.int64)
        assert (np.diff(ids2) > 0).all() and ids2[n0:].min() > ids.max(), "appended rows are numbered above every earlier ID"
        lid, probs = ef.labels()
        assert np.array_equal(lid.astype(np.int64), ids2)
        assert_bits_equal(probs[:n0], P, "the old rows' labels, fused ones included")
        assert (probs[n0:] == F(1) / F(NC)).all(), "appended rows start at the prior"
        ef.processFrame(frames[3][0], frames[3][1], 3)                  # and a frame on top still numbers above everything
        ids3 = ef.surfelIds().astype(np.int64)
        assert (np.diff(ids3) > 0).all() and ids3.max() >= ids2.max()
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. capacity
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_fuse_beyond_the_capacity_changes_nothing():
    from elasticfusion_amd import api
    rng = np.random.default_rng(8)
    n0 = 7000
    S = plain_surfels(np.stack([rng.uniform(0, 3, n0), rng.uniform(0, 3, n0), np.full(n0, 0.5)], 1))
    R = S[rng.choice(n0, 1500, replace=False)].copy()
    R[:, :3] += rng.uniform(-0.001, 0.001, (1500, 3)).astype(F)
    R[800:, 2] += F(0.5)                                                # 700 novel records
    R[:, 3] = 2.0
    prm = params_of(init_time=1, last_time=1)
    free = fr.fuse(S, R, None, prm)
    novel = free["result"]["novel"]
    assert novel == 700 and free["result"]["fused"] > 500
    CAP = n0 + novel - 1                                                # the append overflows by one
    exp = fr.fuse(S, R, None, prm, capacity=CAP)
    assert exp["refused"] and exp["result"] == dict(free["result"], count_after=n0)
    ef = api.ElasticFusion(width=100, height=76, fx=100.0, fy=100.0, cx=50.0, cy=38.0, maxSurfels=CAP)
    try:
        ef.uploadMap(S)
        q = R[:64, :3]
        rows_before = ef.queryNearestRaw(q, 0.01, -1.0)
        for rec in (R, api.DevBuf.from_array(R)):
            with pytest.raises(api.EFError) as e:
                ef.fuseSurfels(rec, params=to_api(ef, prm), rows=True)
            assert e.value.rc == -5 and "max_surfels" in str(e.value), str(e.value)      # EF_ECAPACITY
            assert e.value.result == exp["result"], (e.value.result, exp["result"])
            assert ef.lastCount() == n0
            assert_bits_equal(ef.downloadMap(), S, "the map after the refused fuse, the rows it would have fused included")
        rows_after = ef.queryNearestRaw(q, 0.01, -1.0)
        for a, b in zip(rows_before, rows_after):
            assert_bits_equal(a, b, "the query after the refused fuse")
        # with append = 0 the same records fit, and one record fewer fits with append = 1
        got = ef.fuseSurfels(R, params=to_api(ef, dict(prm, append=0)), rows=True)
        check_fuse(got, fr.fuse(S, R, None, dict(prm, append=0)), ef, "append 0 at the capacity")
        ef.uploadMap(S)
        got = ef.fuseSurfels(R[:-1], params=to_api(ef, prm), rows=True)
        fits = fr.fuse(S, R[:-1], None, prm)
        assert fits["result"]["count_after"] == CAP
        check_fuse(got, fits, ef, "exactly as many as fit")
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. fuse, then keep mapping = upload + restore
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fourteen(seq):
    return [seq.frame(k) for k in range(14)]


@pytest.mark.parametrize("keys_pending", (True, False))
def test_fuse_then_mapping_equals_upload_and_restore(fourteen, keys_pending):
    """keys_pending: the fuse comes right after a frame whose index maps are still z-buffer keys (the default); False: they were resolved
    first (an index image was fetched).  Either way the in-place edit must leave what upload + restore leaves."""
    from elasticfusion_amd import api
    fr_ = fourteen

    def feed(ef, k):
        ef.processFrame(fr_[k][0], fr_[k][1], k * 33333)

    a, b, plain = api.ElasticFusion(), api.ElasticFusion(), api.ElasticFusion()
    try:
        for k in range(12):
            feed(a, k)
            feed(plain, k)
        if not keys_pending:
            assert a.image("vertConf").any()
        thr = a.getConfidenceThreshold()
        m12 = a.downloadMap()
        ck = a.checkpoint(fr_[11][0], fr_[11][1])
        rng = np.random.default_rng(5)
        rows = patch_rows(m12, 0.3, rng, 1500)
        R = m12[rows].copy()
        R[:, :3] += rng.uniform(-0.0008, 0.0008, (1500, 3)).astype(F)
        R[:, 3] = F(thr) + F(2)                                         # whatever they are fused into becomes stable
        R[1000:, 2] += F(0.3)                                           # and 500 of them are new surface
        prm = params_of(min_conf=F(-1.0), cos=F(0.5), init_time=a.getTick(), last_time=a.getTick())
        exp = fr.fuse(m12, R, None, prm, known=local_outcome(m12, R, None, prm))
        assert exp["result"]["fused"] > 500 and exp["result"]["inserted"] > 300, exp["result"]
        res = a.fuseSurfels(R, params=to_api(a, prm))
        print("frame 12: surfels", len(m12), res)
        assert res == exp["result"]
        assert_bits_equal(a.downloadMap(), exp["map"], "the edited map")
        assert a.getTick() == ck["tick"] and np.array_equal(a.getPoseQT(), ck["qt"])
        ck["map"] = exp["map"]
        b.restore(ck)
        for k in range(12, 14):
            feed(a, k)
            feed(b, k)
            feed(plain, k)
            (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
            assert np.array_equal(qa.view(np.uint64), qb.view(np.uint64)), (k, qa, qb)
            assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), (k, sa, sb)
            assert_bits_equal(ma, mb, f"the map after frame {k}")
        mp = plain.downloadMap()
        assert mp.shape != ma.shape or not np.array_equal(u32(mp), u32(ma)), "the fuse mattered"
    finally:
        for ef in (a, b, plain):
            ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 8. refusals with a context
# ---------------------------------------------------------------------------------------------------------------------------------------
def refused(fn, code):
    from elasticfusion_amd import api
    with pytest.raises(api.EFError) as e:
        fn()
    assert f"error {code}:" in str(e.value), str(e.value)
    return str(e.value)


def test_refusals_with_a_context(random_scene):
    from elasticfusion_amd import api
    S, R = random_scene["S"], random_scene["R"][:64]
    dR = api.DevBuf.from_array(R)
    ef = api.ElasticFusion(closeLoops=True)
    try:
        ef.uploadMap(S)
        assert "close_loops" in refused(lambda: ef.fuseSurfels(R), -4)              # EF_ESTATE
        assert "close_loops" in refused(lambda: ef.fuseSurfels(dR, append=0), -4)
        assert ef.lastCount() == len(S)
        assert_bits_equal(ef.downloadMap(), S, "a refused fuse leaves the map")
    finally:
        ef.close()
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        # a min_separation beyond the query's ratio to the cell: refused as the insert refuses it
        wide = 20.0 * default_cell()
        msg_f = refused(lambda: ef.fuseSurfels(R, min_separation=wide), -1)           # EF_EINVAL
        msg_i = refused(lambda: ef.insertSurfels(R, min_separation=wide), -1)
        assert msg_f.replace("ef_map_fuse", "ef_map_insert") == msg_i, (msg_f, msg_i)
        refused(lambda: ef.fuseSurfels(R, append=2), -1)
        # misaligned device records
        res = api.ef_fuse_result()
        prm = ef.fuseParams()
        rc = api.lib().ef_map_fuse_dev(ef.h, C.c_void_p(dR.p.value + 4), C.c_uint32(8), None, C.byref(prm), C.byref(res), None, None, None)
        assert rc == -1 and b"16-byte aligned" in api.lib().ef_last_error(ef.h)
        assert_bits_equal(ef.downloadMap(), S, "refused calls leave the map")
        # n = 0 and the empty map are valid calls
        zero = dict(fused=0, absorbed=0, weightless=0, novel=0, skipped=0, inserted=0)
        res, new, match, outcome = ef.fuseSurfels(np.zeros((0, 12), F), rows=True)
        assert res == dict(zero, count_after=len(S)) and len(new) == len(match) == len(outcome) == 0
        assert ef.fuseSurfels(api.DevBuf(48), n=0) == dict(zero, count_after=len(S))
        assert_bits_equal(ef.downloadMap(), S, "n = 0")
        ef.uploadMap(np.zeros((0, 12), F))
        assert ef.fuseSurfels(np.zeros((0, 12), F)) == dict(zero, count_after=0)
        prm0 = params_of(append=0)
        check_fuse(ef.fuseSurfels(R, params=to_api(ef, prm0), rows=True), fr.fuse(np.zeros((0, 12), F), R, None, prm0), ef, "empty map, append 0")
        assert ef.lastCount() == 0
        prm1 = params_of(append=1)
        exp = fr.fuse(np.zeros((0, 12), F), R, None, prm1)
        assert exp["result"]["inserted"] == 64
        check_fuse(ef.fuseSurfels(R, params=to_api(ef, prm1), rows=True), exp, ef, "empty map, append 1")
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 9. merge_session(fuse=True)
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_merge_session_with_fuse_raises_confidences():
    from scipy.linalg import expm
    from elasticfusion_amd import accuracy, api, synth
    from test_gpu_register import TWIST, twist_matrix
    S = synth.sample_surfels(synth.Sequence(0xEF0001), n=10000, conf=6.0)       # a first session that saw everything once: nothing is stable
    Gi = np.linalg.inv(expm(twist_matrix(TWIST)))
    pick = np.sort(np.random.default_rng(0xC10D).choice(len(S), 3000, replace=False))
    gy, gz = np.meshgrid(np.arange(20) * 0.02, np.arange(20) * 0.02, indexing="ij")
    patch = np.zeros((400, 12), F)
    patch[:, 0] = S[:, 0].max() + 1.0
    patch[:, 1], patch[:, 2] = gy.reshape(-1), gz.reshape(-1)
    patch[:, 3], patch[:, 4], patch[:, 6], patch[:, 7], patch[:, 8], patch[:, 11] = 20, 0x808080, 1, 2, -1, 0.005
    cloud = accuracy.move_surfels(np.concatenate([S[pick], patch]), Gi)   # a second session: part of the same surface, and a patch beyond it
    kw = dict(register=dict(schedule=(0.05,), min_conf=-1.0, max_iterations=6), min_normal_cos=-1.0, init_time=ir.KEEP, last_time=ir.KEEP)
    plain, fused = api.ElasticFusion(), api.ElasticFusion()
    try:
        thr = F(plain.getConfidenceThreshold())
        plain.uploadMap(S)
        fused.uploadMap(S)
        T0, st0, res0 = accuracy.merge_session(plain, cloud, **kw)
        T1, st1, (res1, new, match, outcome) = accuracy.merge_session(fused, cloud, fuse=True, rows=True, **kw)
        assert st0[-1]["status"] == api.REG_CONVERGED and np.array_equal(T0.view(np.uint64), T1.view(np.uint64))
        m0 = plain.downloadMap()
        # on the reference first: the fuse makes surfels stable that the insert leaves unstable
        prm = fr.default_params(0, min_normal_cos=-1.0, init_time=ir.KEEP, last_time=ir.KEEP)
        exp = fr.fuse(S, cloud, T1, prm)
        stable0, stable_ref = int((m0[:, 3] > thr).sum()), int((exp["map"][:, 3] > thr).sum())
        print("merge_session: insert", res0, "fuse", res1, "stable", stable0, "->", stable_ref)
        assert stable_ref > stable0 == 400 and exp["result"]["fused"] > 2900
        assert res1 == exp["result"] and res1["count_after"] == res0["count_after"] and res1["inserted"] == res0["inserted"] == 400
        m1 = fused.downloadMap()
        assert_bits_equal(m1, exp["map"], "the merged map")
        assert int((m1[:, 3] > thr).sum()) == stable_ref > stable0
        assert np.array_equal(outcome, exp["outcome"]) and np.array_equal(match, exp["match_row"])
    finally:
        plain.close()
        fused.close()
