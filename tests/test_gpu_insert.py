"""Insert surfels into the map on the device (ef_map_insert, include/ef_hip.h; kernels in elasticfusion_amd/csrc/ef_insert.inc).

The insert is restated in numpy from the header alone (tests/insertref.py, on the exhaustive scan of tests/queryref.py): the float32 transform
in the written order, the novelty gate against the map as it stood before the call, the outcome per record and the stable append.  The device
must give the same result, the same new_row / match_row and the same map, bit for bit; and a context that inserts and keeps mapping must compute
what a fresh context computes after uploadMap(old rows ++ inserted rows) + restore, bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest

import insertref as ir
from queryref import MISS, assert_bits_equal, brute
from test_gpu_select import scene_T, state_of, step, u32

pytestmark = pytest.mark.gpu

F = np.float32
SEP = F(0.01)            # min_separation of the edge scene
R2 = SEP * SEP           # r2 as the host computes it
MIN_CONF = F(2.5)
COS = F(0.5)
SENTINEL = 0xABABABAB


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def d2_of(q, s):
    """the header's d2 of one query point against rows of positions, float32 in the written order"""
    s = np.ascontiguousarray(s, F).reshape(-1, 3)
    dx, dy, dz = (F(q[j]) - s[:, j] for j in range(3))
    return (dx * dx + dy * dy) + dz * dz


def cos_of(m, ns):
    ns = np.ascontiguousarray(ns, F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (F(m[0]) * ns[:, 0] + F(m[1]) * ns[:, 1]) + F(m[2]) * ns[:, 2]


def lattice(c, k=16):
    """the float32 points within k floats per coordinate of c"""
    c = np.asarray(c, F)
    s = np.arange(-k, k + 1)
    i, j, l = (g.reshape(-1) for g in np.meshgrid(s, s, s, indexing="ij"))
    return np.stack([c[0] + i * np.float64(np.spacing(c[0])), c[1] + j * np.float64(np.spacing(c[1])), c[2] + l * np.float64(np.spacing(c[2]))],
                    1).astype(F)


def point_at_d2(q, direction, target):
    """a float32 point near q + 0.01 direction whose d2 from q is exactly target"""
    cand = lattice((np.asarray(q, np.float64) + unit(direction) * float(SEP)).astype(F))
    hit = np.nonzero(d2_of(q, cand) == target)[0]
    assert len(hit), ("no float32 point at d2", float(target))
    return cand[hit[0]]


def normal_at_cos(m, target):
    """a float32 vector whose header cosine with m is exactly target"""
    m64 = np.asarray(m, np.float64)
    cand = lattice((float(target) * m64 / (m64 @ m64)).astype(F))
    hit = np.nonzero(cos_of(m, cand) == target)[0]
    assert len(hit), ("no float32 normal at cosine", float(target))
    return cand[hit[0]]


def record_at(Ti, target, normal_world, conf=5.0, colour=0x123456, idbits=77, t0=3.0, t1=8.0, radius=0.004):
    """a record whose moved position lies at about `target` and whose moved normal is about normal_world"""
    r = np.zeros(12, F)
    r[:3] = (Ti[:3, :3] @ np.asarray(target, np.float64) + Ti[:3, 3]).astype(F)
    r[8:11] = (Ti[:3, :3] @ np.asarray(normal_world, np.float64)).astype(F)
    r[3], r[4], r[6], r[7], r[11] = conf, colour, t0, t1, radius
    r[5:6].view(np.uint32)[0] = idbits
    return r


def surfel_at(pos, normal, conf=5.0):
    s = np.zeros(12, F)
    s[:3], s[8:11] = pos, normal
    s[3], s[4], s[6], s[7], s[11] = conf, 0x0A0B0C, 1.0, 2.0, 0.005
    return s


def edge_scene():
    """(map S n x 12, records R m x 12, T, names): hand-built clusters around the moved positions of single records — each far from every other
    cluster and from the background — followed by a random background; `names` maps a case to its record (and map rows)"""
    rng = np.random.default_rng(77)
    T = scene_T()
    Ti = np.linalg.inv(T)
    S, R, names = [], [], {}
    direction = (0.58, 0.71, 0.40)

    def centre(k):
        return np.array([-1.5 + 0.25 * k, 0.1 * (k % 3), 0.3])

    def new_record(k, normal=(0.0, 0.0, 1.0), **kw):
        R.append(record_at(Ti, centre(k), unit(normal), **kw))
        p, m = ir.move(R[-1], T)
        return len(R) - 1, p[0], m[0]

    k = 0
    for name, target in (("d2_below", step(R2, False)), ("d2_at", R2), ("d2_above", step(R2, True))):
        i, p, m = new_record(k, (0.2, -0.3, 0.9))
        S.append(surfel_at(point_at_d2(p, direction, target), m))
        names[name] = (i, len(S) - 1)
        k += 1
    for name, target in (("cos_below", step(COS, False)), ("cos_at", COS), ("cos_above", step(COS, True))):
        i, p, m = new_record(k, (-0.4, 0.5, 0.7))
        S.append(surfel_at((p.astype(np.float64) + unit(direction) * 0.003).astype(F), normal_at_cos(m, target)))
        names[name] = (i, len(S) - 1)
        k += 1
    # two surfels at the same d2: the moved position +- 2^-8 along x (both sums exact)
    i, p, m = new_record(k)
    S.append(surfel_at(p + np.array([2.0 ** -8, 0, 0], F), m))
    S.append(surfel_at(p - np.array([2.0 ** -8, 0, 0], F), m))
    names["tie"] = (i, len(S) - 2, len(S) - 1)
    k += 1
    # the nearest is not eligible (conf == min_conf is not above it), an eligible one lies farther inside the radius
    i, p, m = new_record(k)
    S.append(surfel_at((p.astype(np.float64) + unit(direction) * 0.002).astype(F), m, conf=float(MIN_CONF)))
    S.append(surfel_at((p.astype(np.float64) - unit(direction) * 0.006).astype(F), m))
    names["conf"] = (i, len(S) - 2, len(S) - 1)
    k += 1
    # the nearest eligible one fails the normal test (a back face), a passing one lies farther inside the radius: INSERTED
    i, p, m = new_record(k)
    S.append(surfel_at((p.astype(np.float64) + unit(direction) * 0.002).astype(F), -m))
    S.append(surfel_at((p.astype(np.float64) - unit(direction) * 0.006).astype(F), m))
    names["back_face"] = (i, len(S) - 2, len(S) - 1)
    k += 1
    # a NaN normal beside a surfel
    i, p, m = new_record(k)
    R[i][9] = np.nan
    S.append(surfel_at((p.astype(np.float64) + unit(direction) * 0.002).astype(F), m))
    names["nan_normal"] = (i, len(S) - 1)
    k += 1
    for name, bad in (("nan_pos", (1, np.nan)), ("inf_pos", (0, np.inf)), ("neg_inf_pos", (2, -np.inf))):
        i, p, m = new_record(k)
        R[i][bad[0]] = bad[1]
        names[name] = (i,)
        k += 1
    assert k <= 14
    # the background: surfels in [2, 4]^3, records beside two hundred of them (up to 15 mm away, half with the surfel's normal) and a hundred anywhere
    nb = 3000 - len(S)
    B = np.zeros((nb, 12), F)
    B[:, :3] = rng.uniform(2, 4, (nb, 3))
    B[:, 3] = rng.uniform(0, 8, nb)
    nrm = rng.normal(size=(nb, 3))
    B[:, 8:11] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    B[:, 4], B[:, 6], B[:, 7], B[:, 11] = rng.integers(0, 1 << 24, nb), rng.integers(1, 9, nb), 9, 0.005
    S = np.concatenate([np.array(S, F), B])
    for j in range(300):
        if j < 200:
            off = rng.normal(size=3)
            off *= rng.uniform(0, 0.015) / np.linalg.norm(off)
            target = B[j * 7, :3].astype(np.float64) + off
            normal = B[j * 7, 8:11].astype(np.float64) if j % 2 == 0 else unit(rng.normal(size=3))
        else:
            target, normal = rng.uniform(2, 4, 3), unit(rng.normal(size=3))
        R.append(record_at(Ti, target, normal, conf=float(rng.uniform(0, 12)), colour=int(rng.integers(0, 1 << 24)), idbits=1000 + j,
                           t0=float(rng.integers(1, 9)), t1=9.0, radius=float(rng.uniform(0.002, 0.01))))
    return S, np.array(R, F), T, names


def plain_scene(S):
    """records for T = None on the edge scene's map: bit copies of map rows, -0.0 coordinates, NaN payloads in a normal, and some beside the map"""
    rng = np.random.default_rng(78)
    rows = np.nonzero(S[:, 3] > F(4))[0][[40, 600, 1400]]
    R = [S[r].copy() for r in rows]
    R.append(surfel_at((-0.0, 7.25, -0.0), (-0.0, 0.0, 1.0)))
    R.append(surfel_at((7.5, -0.0, 0.125), np.array([0x7FC01234, 0x80000000, 0xFFC00001], np.uint32).view(F)))
    for j in range(60):
        r = S[100 + 31 * j].copy()
        r[:3] += rng.normal(size=3).astype(F) * F(0.006)
        r[5:6].view(np.uint32)[0] = 5000 + j
        R.append(r)
    return np.array(R, F), rows


def params_of(gate=1, cos=COS, init_time=ir.KEEP, last_time=ir.KEEP):
    return ir.default_params(0, gate=gate, min_separation=SEP, min_conf=MIN_CONF, min_normal_cos=cos, init_time=init_time, last_time=last_time)


def to_api(ef, p):
    return ef.insertParams(gate=int(p["gate"]), min_separation=float(p["min_separation"]), min_conf=float(p["min_conf"]),
                           min_normal_cos=float(p["min_normal_cos"]), init_time=int(p["init_time"]), last_time=int(p["last_time"]))


def test_the_scene_contains_every_edge_the_header_names():
    """CPU only in effect (no device call): the reference alone shows that the edges are exercised"""
    S, R, T, names = edge_scene()
    assert len(S) == 3000 and len(S) % 256 and len(R) > 300
    p, m = ir.move(R, T)
    near_all = brute(p, S, SEP, -1.0)[0][:, 0]
    near, d2, _, count = brute(p, S, SEP, MIN_CONF)
    near, d2 = near[:, 0], d2[:, 0]
    sk, dup, _ = ir.outcome(S, R, T, params_of())
    sk1, dup1, _ = ir.outcome(S, R, T, params_of(cos=F(-1)))
    ins = ~sk & ~dup
    # d2 == r2 exactly, and one float to either side
    i, s = names["d2_at"]
    assert d2[i] == R2 and near[i] == s and dup[i]
    i, s = names["d2_below"]
    assert d2[i] == step(R2, False) and near[i] == s and dup[i]
    i, s = names["d2_above"]
    assert d2_of(p[i], S[s, :3])[0] == step(R2, True) and near[i] == MISS and count[i] == 0 and ins[i]
    # the cosine exactly at min_normal_cos, and one float to either side
    for name, want, is_dup in (("cos_below", step(COS, False), False), ("cos_at", COS, True), ("cos_above", step(COS, True), True)):
        i, s = names[name]
        assert near[i] == s and cos_of(m[i], S[s, 8:11])[0] == want and dup[i] == is_dup and dup1[i], name
    # a tie: the lower row
    i, a, b = names["tie"]
    assert a < b and d2_of(p[i], S[a, :3])[0] == d2_of(p[i], S[b, :3])[0] == d2[i] and near[i] == a and count[i] == 2 and dup[i]
    # min_conf: the nearest is not eligible, the farther one is the match
    i, a, b = names["conf"]
    assert near_all[i] == a and near[i] == b and count[i] == 1 and dup[i]
    assert d2_of(p[i], S[a, :3])[0] < d2_of(p[i], S[b, :3])[0] <= R2
    # the back face: only the nearest is asked
    i, a, b = names["back_face"]
    assert near[i] == a and count[i] == 2 and cos_of(m[i], S[a, 8:11])[0] < COS <= cos_of(m[i], S[b, 8:11])[0]
    assert ins[i] and dup1[i]
    i, s = names["nan_normal"]
    assert np.isnan(m[i]).any() and np.isfinite(p[i]).all() and near[i] == s and ins[i] and dup1[i]
    for name in ("nan_pos", "inf_pos", "neg_inf_pos"):
        i, = names[name]
        assert sk[i] and not np.isfinite(p[i]).all() and near[i] == MISS
    assert np.isnan(p[names["nan_pos"][0]]).any() and np.isinf(R[names["inf_pos"][0], :3]).any()
    # the background has all three outcomes in number, and duplicates that exist only without the normal test
    assert dup.sum() > 40 and ins.sum() > 100 and sk.sum() == 3 and (dup1 & ~dup).sum() > 20
    # T = None: bit copies of map rows (duplicates of their own row), -0.0 coordinates, NaN payloads
    R0, rows = plain_scene(S)
    sk0, dup0, near0 = ir.outcome(S, R0, None, params_of())
    for k, r in enumerate(rows):
        assert (u32(R0[k]) == u32(S[r])).all() and dup0[k] and near0[k] == r
    assert u32(R0[3, :3]).tolist() == [0x80000000, u32(F(7.25)), 0x80000000] and not dup0[3] and not sk0[3]
    assert u32(R0[4, 8:11]).tolist() == [0x7FC01234, 0x80000000, 0xFFC00001] and not dup0[4] and not sk0[4]
    exp = ir.insert(S, R0, None, params_of())
    k = int(exp["new_row"][3])
    assert u32(exp["map"][k, :3]).tolist() == [0x80000000, u32(F(7.25)), 0x80000000]
    assert 10 < dup0.sum() < len(R0) - 10


def insert_dev(ef, rec, T, params, pad=16):
    """ef_map_insert_dev with sentinels behind both row arrays: (result dict, new_row, match_row)"""
    from elasticfusion_amd import api
    n = len(rec)
    d_rec = api.DevBuf.from_array(rec) if n else None
    d_new = api.DevBuf.from_array(np.full(n + pad, SENTINEL, np.uint32))
    d_match = api.DevBuf.from_array(np.full(n + pad, SENTINEL, np.uint32))
    keep, pT = api._pose16(T)
    res = api.ef_insert_result()
    rc = api.lib().ef_map_insert_dev(ef.h, d_rec.p if n else None, C.c_uint32(n), pT, C.byref(params), C.byref(res), d_new.p, d_match.p)
    assert rc == 0, (rc, api.lib().ef_last_error(ef.h))
    new, match = d_new.to_array(np.uint32, n + pad), d_match.to_array(np.uint32, n + pad)
    assert (new[n:] == SENTINEL).all() and (match[n:] == SENTINEL).all(), "the device variant wrote beyond its outputs"
    return dict(inserted=res.inserted, duplicates=res.duplicates, skipped=res.skipped, count_after=res.count_after), new[:n], match[:n]


def check_insert(got, exp, ef, what):
    res, new, match = got
    assert res == exp["result"], (what, res, exp["result"])
    assert new.dtype == np.uint32 and np.array_equal(new, exp["new_row"]), (what, np.nonzero(new != exp["new_row"])[0][:8])
    assert np.array_equal(match, exp["match_row"]), (what, np.nonzero(match != exp["match_row"])[0][:8])
    assert ef.lastCount() == exp["result"]["count_after"], what
    assert_bits_equal(ef.downloadMap(), exp["map"], what + ": the map")


@pytest.fixture(scope="module")
def ctx():
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    yield ef
    ef.close()


@pytest.mark.parametrize("moved", (True, False))
def test_edge_scene_equals_the_reference_exactly(ctx, moved):
    ef = ctx
    S, R, T, names = edge_scene()
    if not moved:
        R, T = plain_scene(S)[0], None
    p = ir.move(R, T)[0]
    for gate in (1, 0):
        for cos in (COS, F(-1)):
            for times in ((ir.KEEP, ir.KEEP), (21, ir.KEEP), (0, 34)):
                prm = params_of(gate, cos, *times)
                exp = ir.insert(S, R, T, prm)
                for device in (False, True):
                    what = f"T {moved} gate {gate} cos {float(cos)} times {times} device {device}"
                    ef.uploadMap(S)
                    qrow = ef.queryNearestRaw(p, float(SEP), float(MIN_CONF))[0]     # (also: an index built before the insert)
                    got = insert_dev(ef, R, T, to_api(ef, prm)) if device else ef.insertSurfels(R, T=T, params=to_api(ef, prm), rows=True)
                    check_insert(got, exp, ef, what)
                    if gate:
                        dup = got[2] != MISS
                        assert np.array_equal(got[2][dup], qrow[dup]), what
                        if cos <= -1:
                            assert np.array_equal(got[2], qrow), what + ": match_row is the query's row"
                print(f"T {moved} gate {gate} cos {float(cos)} times {times}:", exp["result"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------------------------------------------------------------------
# 16 records fill one workgroup of the gate (16 lanes each), 256 are one chunk of the counts and of the scatter, and 262144 + 257 records are
# 1026 chunks: the one-workgroup scan of the chunk counts (1024 per trip) takes a second trip with a carry
SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 262144 + 257)
BASE = 4097


@pytest.fixture(scope="module")
def sized():
    """a 5000-surfel map (not a multiple of 256) and 4097 base records under a non-trivial T, about half of them duplicates, every 97th skipped;
    the reference outcome of the base records is computed once: a longer input repeats them, and records never gate one another"""
    T = scene_T()
    Ti = np.linalg.inv(T)
    i = np.arange(5000)
    S = np.zeros((5000, 12), F)
    S[:, 0], S[:, 1], S[:, 2] = 0.05 * (i % 50), 0.05 * ((i // 50) % 50), 0.05 * (i // 2500)
    S[:, 3], S[:, 4], S[:, 6], S[:, 7], S[:, 10], S[:, 11] = 5, i, 1, 2, 1, 0.004
    j = np.arange(BASE)
    target = np.where((j % 2 == 0)[:, None], S[(j * 7) % 5000, :3].astype(np.float64) + (0.002, 0.001, 0.0),
                      np.stack([10 + 0.02 * j, 0.0 * j, 0.5 + 0.0 * j], 1))
    B = np.zeros((BASE, 12), F)
    B[:, :3] = (target @ Ti[:3, :3].T + Ti[:3, 3]).astype(F)
    B[:, 8:11] = (Ti[:3, :3] @ np.array([0.0, 0.0, 1.0])).astype(F)
    B[:, 3], B[:, 4], B[:, 6], B[:, 7], B[:, 11] = 3, j, 4, 6, 0.003
    B[:, 5] = (j + 1).astype(np.uint32).view(F)
    B[::97, 1] = np.nan
    prm = ir.default_params(7)
    known = ir.outcome(S, B, T, prm)
    assert 1900 < known[1].sum() < 2100 and known[0].sum() == 43
    return dict(S=S, B=B, T=T, prm=prm, known=known)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, sized, n):
    ef = ctx
    S, T, prm = sized["S"], sized["T"], sized["prm"]
    idx = np.arange(n) % BASE
    R = sized["B"][idx]
    exp = ir.insert(S, R, T, prm, known=tuple(a[idx] for a in sized["known"]))
    ef.uploadMap(S)
    check_insert(ef.insertSurfels(R, T=T, params=to_api(ef, prm), rows=True), exp, ef, f"n {n}")
    if n in (0, 257):      # without the row arrays, and the gate off
        ef.uploadMap(S)
        assert ef.insertSurfels(R, T=T, params=to_api(ef, prm)) == exp["result"]
        assert_bits_equal(ef.downloadMap(), exp["map"], f"n {n} without row arrays")
        off = dict(prm, gate=0)
        ef.uploadMap(S)
        check_insert(ef.insertSurfels(R, T=T, params=to_api(ef, off), rows=True), ir.insert(S, R, T, off), ef, f"n {n}, gate off")


def test_an_empty_map_takes_every_finite_record(ctx, sized):
    ef = ctx
    R, T = sized["B"][:300], sized["T"]
    empty = np.zeros((0, 12), F)
    for gate in (1, 0):
        prm = dict(sized["prm"], gate=gate)
        exp = ir.insert(empty, R, T, prm)
        assert exp["result"]["inserted"] == 300 - 4 and exp["result"]["duplicates"] == 0
        ef.uploadMap(empty)
        check_insert(ef.insertSurfels(R, T=T, params=to_api(ef, prm), rows=True), exp, ef, f"empty map, gate {gate}")
    # and a second insert of the same records on top: every finite one is now a duplicate of its own first copy
    res, new, match = ef.insertSurfels(R, T=T, params=to_api(ef, dict(sized["prm"], gate=1)), rows=True)
    assert res == dict(inserted=0, duplicates=296, skipped=4, count_after=296) and (new == MISS).all()
    assert np.array_equal(match[match != MISS], np.arange(296, dtype=np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# round trip: gather, erase, insert back
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_gather_erase_insert_round_trip(ctx, sized):
    ef = ctx
    S = sized["S"].copy()
    S[:, 5] = (3 * np.arange(5000) + 9).astype(np.uint32).view(F)      # something in the ID lane (IDs are off: plain data)
    ef.uploadMap(S)
    rows = np.arange(1, 5000, 3, dtype=np.uint32)
    ef.queryNearestRaw(S[:8, :3], 0.01, -1.0)                          # an index of the unedited map
    G = ef.gatherSurfels(rows)
    assert_bits_equal(G, S[rows], "gather")
    assert ef.eraseRows(rows) == len(rows)
    mask = np.zeros(5000, bool)
    mask[rows] = True
    res, new, match = ef.insertSurfels(G, T=None, rows=True, gate=0, init_time=ir.KEEP, last_time=ir.KEEP)
    kept = int((~mask).sum())
    assert res == dict(inserted=len(rows), duplicates=0, skipped=0, count_after=5000)
    assert np.array_equal(new, kept + np.arange(len(rows), dtype=np.uint32)) and (match == MISS).all()
    back = G.copy()
    back[:, 5] = 0
    assert_bits_equal(ef.downloadMap(), np.concatenate([S[~mask], back]), "kept ++ gathered")
    # the index went stale: a query at an inserted surfel's position finds its new row
    k = np.array([0, 1, len(rows) // 2, len(rows) - 1])
    row, d2, _ = ef.queryNearestRaw(G[k, :3], 0.001, -1.0)
    assert np.array_equal(row, (kept + k).astype(np.uint32)) and (d2 == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# IDs and labels
# ---------------------------------------------------------------------------------------------------------------------------------------
def far_records(n, x0, seed):
    rng = np.random.default_rng(seed)
    R = np.zeros((n, 12), F)
    R[:, 0], R[:, 1], R[:, 2] = x0 + 0.02 * np.arange(n), rng.uniform(0, 1, n), 0.5
    R[:, 3], R[:, 4], R[:, 6], R[:, 7], R[:, 10], R[:, 11] = 12, 77, 1, 2, 1, 0.004
    R[:, 5] = (90000 + np.arange(n)).astype(np.uint32).view(F)          # IDs of another session: never kept
    return R


def test_ids_and_labels_follow_an_insert(frames):
    from elasticfusion_amd import api
    NC = 4
    ef = api.ElasticFusion()
    try:
        ef.setSurfelIds(True)
        ef.enableLabels(NC)
        for k in range(3):
            ef.processFrame(frames[k][0], frames[k][1], k)
        # the rows the last frame created are not numbered yet: the insert numbers them BEFORE it appends
        res = ef.insertSurfels(far_records(500, 50.0, 1), gate=0)
        n = res["count_after"] - 500
        before = ef.downloadMap()
        ids = u32(before[:, 5]).astype(np.int64)
        assert res["inserted"] == 500 and len(before) == n + 500
        assert ids.min() >= 1 and (np.diff(ids) > 0).all(), "old rows first, then the inserted ones, strictly increasing"
        rng = np.random.default_rng(4)
        P = rng.dirichlet(np.ones(NC), len(before)).astype(F)
        ef.setLabels(P)
        largest = int(ids.max())
        # a second insert: old rows keep IDs and label floats bit for bit, the new rows continue the IDs and start at the prior
        R2 = far_records(300, 80.0, 2)
        res2, new2, _ = ef.insertSurfels(R2, gate=1, rows=True)
        assert res2["inserted"] == 300 and np.array_equal(new2, len(before) + np.arange(300, dtype=np.uint32))
        after = ef.downloadMap()
        assert_bits_equal(after[:len(before)], before, "the old rows, ID lane included")
        ids2 = u32(after[:, 5]).astype(np.int64)
        assert (np.diff(ids2) > 0).all() and ids2[len(before):].min() > largest
        lid, probs = ef.labels()
        assert np.array_equal(lid.astype(np.int64), ids2)
        assert_bits_equal(probs[:len(before)], P, "the old rows' labels")
        assert (probs[len(before):] == F(1) / F(NC)).all(), "inserted rows start at the prior"
        # the newest rows (the holders of the largest IDs) are erased in between: IDs are still never reused
        largest2 = int(ids2.max())
        assert ef.eraseRows(np.arange(len(after) - 200, len(after), dtype=np.uint32)) == 200
        assert int(ef.surfelIds().max()) < largest2
        res3 = ef.insertSurfels(far_records(100, 120.0, 3), gate=0)
        ids3 = ef.surfelIds().astype(np.int64)
        assert res3["inserted"] == 100 and len(ids3) == len(after) - 200 + 100
        assert (np.diff(ids3) > 0).all() and ids3[-100:].min() > largest2
        lid3, probs3 = ef.labels()
        assert np.array_equal(lid3.astype(np.int64), ids3)
        assert_bits_equal(probs3[:len(before)], P, "the old rows' labels after erase and insert")
        assert (probs3[len(before):] == F(1) / F(NC)).all()
        # and a frame on top still numbers above everything
        ef.processFrame(frames[3][0], frames[3][1], 3)
        ids4 = ef.surfelIds().astype(np.int64)
        assert (np.diff(ids4) > 0).all() and ids4.max() >= ids3.max()
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# insert, then keep mapping = upload + restore
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sixteen(seq):
    return [seq.frame(k) for k in range(16)]


@pytest.mark.parametrize("persistent", (True, False))
def test_insert_then_mapping_equals_upload_and_restore(sixteen, persistent):
    from elasticfusion_amd import api
    fr = sixteen

    def context():
        ef = api.ElasticFusion()
        if not persistent:
            ef.setPersistentTracker(0)
        return ef

    def feed(ef, k):
        ef.processFrame(fr[k][0], fr[k][1], k * 33333)

    a, b, plain = context(), context(), context()
    try:
        for k in range(12):
            feed(a, k)
            feed(plain, k)
        thr = a.getConfidenceThreshold()
        m12 = a.downloadMap()
        # the surfels of the world half-space x <= 0 are taken out and put back a few millimetres away as STABLE surfels (twelve frames make
        # none stable yet): the prediction the next frames are tracked against shows them
        mask = m12[:, 0] <= 0
        rows = np.nonzero(mask)[0].astype(np.uint32)
        ck = a.checkpoint(fr[11][0], fr[11][1])
        G = a.gatherSurfels(rows)
        assert_bits_equal(G, m12[rows], "gather")
        G[:, 3] = F(thr) + F(2)
        assert a.eraseRows(rows) == len(rows) > 1000 and (~mask).sum() > 1000
        w = 0.001
        T = np.array([[np.cos(w), -np.sin(w), 0, 0.002], [np.sin(w), np.cos(w), 0, -0.001], [0, 0, 1, 0.0015], [0, 0, 0, 1]])
        prm = ir.default_params(a.getTick(), gate=0, init_time=ir.KEEP, last_time=ir.KEEP)
        exp = ir.insert(m12[~mask], G, T, prm)
        res = a.insertSurfels(G, T=T, params=to_api(a, prm))
        print("frame 12: surfels", len(m12), "taken out and put back", len(rows), res)
        assert res == exp["result"] and res["inserted"] == len(rows)
        assert_bits_equal(a.downloadMap(), exp["map"], "the edited map")
        assert a.getTick() == ck["tick"] and np.array_equal(a.getPoseQT(), ck["qt"])
        ck["map"] = exp["map"]
        b.restore(ck)
        for k in range(12, 16):
            feed(a, k)
            feed(b, k)
            feed(plain, k)
            (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
            assert np.array_equal(qa.view(np.uint64), qb.view(np.uint64)), (k, qa, qb)
            assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), (k, sa, sb)
            assert_bits_equal(ma, mb, f"the map after frame {k}")
        mp = plain.downloadMap()
        assert mp.shape != ma.shape or not np.array_equal(u32(mp), u32(ma)), "the insert mattered"
    finally:
        for ef in (a, b, plain):
            ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# capacity
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_an_insert_beyond_the_capacity_changes_nothing(frames):
    from elasticfusion_amd import api
    CAP = 400000
    a, twin = api.ElasticFusion(maxSurfels=CAP), api.ElasticFusion(maxSurfels=CAP)
    try:
        for ef in (a, twin):
            for k in range(2):
                ef.processFrame(frames[k][0], frames[k][1], k)
        n0 = a.lastCount()
        assert n0 == twin.lastCount() and 1000 < n0 < CAP
        a.queryNearestRaw(np.zeros((4, 3), F), 0.01, -1.0)
        R = far_records(CAP - n0 + 1, 50.0, 5)           # one more than fits
        for gate in (1, 0):
            with pytest.raises(api.EFError) as e:
                a.insertSurfels(R, gate=gate)
            assert "error -5:" in str(e.value) and "max_surfels" in str(e.value), str(e.value)     # EF_ECAPACITY
            assert e.value.result == dict(inserted=len(R), duplicates=0, skipped=0, count_after=n0), e.value.result
            assert a.lastCount() == n0
        assert_bits_equal(a.downloadMap(), twin.downloadMap(), "the map after the refused inserts")
        for ef in (a, twin):
            ef.processFrame(frames[2][0], frames[2][1], 2)
        (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(twin)
        assert np.array_equal(qa.view(np.uint64), qb.view(np.uint64)) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
        assert_bits_equal(ma, mb, "the map after the next frame")
        # exactly as many as fit are taken
        n1 = a.lastCount()
        if n1 < CAP:
            res = a.insertSurfels(far_records(CAP - n1, 50.0, 6), gate=0)
            assert res == dict(inserted=CAP - n1, duplicates=0, skipped=0, count_after=CAP) and a.lastCount() == CAP
    finally:
        a.close()
        twin.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals on the device path
# ---------------------------------------------------------------------------------------------------------------------------------------
def refused(fn, code):
    from elasticfusion_amd import api
    with pytest.raises(api.EFError) as e:
        fn()
    assert f"error {code}:" in str(e.value), str(e.value)
    return str(e.value)


def test_state_refusals(sized):
    import ctypes.util
    from elasticfusion_amd import api
    S, R = sized["S"], sized["B"][:64]
    dR = api.DevBuf.from_array(R)
    ef = api.ElasticFusion(closeLoops=True)
    try:
        ef.uploadMap(S)
        assert "close_loops" in refused(lambda: ef.insertSurfels(R), -4)          # EF_ESTATE
        assert "close_loops" in refused(lambda: ef.insertSurfels(dR, gate=0), -4)
        assert ef.lastCount() == 5000
    finally:
        ef.close()
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        name = ctypes.util.find_library("amdhip64") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")
        hip = C.CDLL(name)
        s = C.c_void_p(ef.stream())
        ef.synchronize()
        assert hip.hipStreamBeginCapture(s, C.c_int(2)) == 0   # relaxed
        try:
            assert "captured" in refused(lambda: ef.insertSurfels(R), -4)
            assert "captured" in refused(lambda: ef.insertSurfels(dR), -4)
            assert "captured" in refused(lambda: ef.insertSurfels(np.zeros((0, 12), F)), -4)
        finally:
            g = C.c_void_p()
            assert hip.hipStreamEndCapture(s, C.byref(g)) == 0
            if g.value:
                hip.hipGraphDestroy(g)
        ef.synchronize()
        assert ef.lastCount() == 5000
        # an ID-consuming call on a context whose uploaded lane was refused
        ef.setSurfelIds(True)
        bad = S.copy()
        bad[:, 5] = (6000 - np.arange(5000)).astype(np.uint32).view(F)      # decreasing
        ef.uploadMap(bad)
        assert "ID lane" in refused(lambda: ef.insertSurfels(R), -4)
        assert ef.lastCount() == 5000
        ef.uploadMap(S)                                                      # an all-zero lane is valid again
        assert ef.insertSurfels(R, gate=0)["inserted"] == 64 - 1
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# merge_session end to end
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_merge_session_registers_then_inserts_what_is_new():
    from scipy.linalg import expm
    from elasticfusion_amd import accuracy, api, synth
    from test_gpu_register import ALLOW_C, TWIST, icp_float64, pose_error, twist_matrix
    S = synth.sample_surfels(synth.Sequence(0xEF0001), n=40000)
    G = expm(twist_matrix(TWIST))
    Gi = np.linalg.inv(G)
    pick = np.sort(np.random.default_rng(0xC10D).choice(len(S), 12000, replace=False))
    # a second session: part of the map's own surfels seen from a frame moved by the twist, and a patch beyond everything the map covers
    gy, gz = np.meshgrid(np.arange(40) * 0.02, np.arange(25) * 0.02, indexing="ij")
    patch = np.zeros((1000, 12), F)
    patch[:, 0] = S[:, 0].max() + 1.0
    patch[:, 1], patch[:, 2] = gy.reshape(-1), gz.reshape(-1)
    patch[:, 3], patch[:, 4], patch[:, 6], patch[:, 7], patch[:, 8], patch[:, 11] = 20, 0x808080, 1, 2, -1, 0.005
    cloud = accuracy.move_surfels(np.concatenate([S[pick], patch]), Gi)
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        T, stages, (res, new, match) = accuracy.merge_session(ef, cloud, register=dict(schedule=(0.05,), min_conf=-1.0, max_iterations=6),
                                                              rows=True, min_normal_cos=-1.0, init_time=ir.KEEP, last_time=ir.KEEP)
        st = stages[-1]
        T64, log = icp_float64(S, cloud[:, :3], cloud[:, 8:11], st["iterations"], 0.05, 0.5)
        et, er = pose_error(T, G)
        et64, er64 = pose_error(T64, G)
        big = float(np.abs(S[:, :3]).max())
        extent = float(np.linalg.norm(S[:, :3].max(0) - S[:, :3].min(0)))
        unit_t, unit_r = 2.0 ** -24 * big, 2.0 ** -24 * big / extent
        print(f"registration {st['status_name']} after {st['iterations']}, pairs {st['pairs']}; pose error device {et:.3e} m {er:.3e} rad, "
              f"float64 {et64:.3e} m {er64:.3e} rad; in 2^-24 units {(et - et64) / unit_t:.2f} {(er - er64) / unit_r:.2f}; insert {res}")
        assert len(stages) == 1 and st["status"] == api.REG_CONVERGED and st["pairs"] > 11000
        assert et <= et64 + ALLOW_C * unit_t, (et, et64, unit_t)
        assert er <= er64 + ALLOW_C * unit_r, (er, er64, unit_r)
        # by brute force on the old map, at the moved positions the header defines
        p = ir.move(cloud, T)[0]
        near = brute(p, S, 0.01, -1.0)[0][:, 0]
        ins, dup = new != MISS, match != MISS
        assert not (ins & dup).any() and (ins | dup).all() and res["skipped"] == 0
        assert (near[ins] == MISS).all(), "an inserted record has no map surfel within min_separation"
        assert np.array_equal(match[dup], near[dup]), "a duplicate has one: the nearest"
        assert ins[12000:].all(), "the patch is inserted in full"
        assert dup[:12000].sum() > 11000, "the map's own surfels are recognised"
        assert res == dict(inserted=int(ins.sum()), duplicates=int(dup.sum()), skipped=0, count_after=len(S) + int(ins.sum()))
        prm = ir.default_params(0, min_normal_cos=-1.0, init_time=ir.KEEP, last_time=ir.KEEP)
        exp = ir.insert(S, cloud, T, prm, known=(np.zeros(len(cloud), bool), near != MISS, near))
        assert_bits_equal(ef.downloadMap(), exp["map"], "the merged map")
    finally:
        ef.close()
