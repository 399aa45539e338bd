"""Thin the map to one surfel per voxel on the device (ef_map_thin / ef_map_thin_select, include/ef_hip.h; kernels in
elasticfusion_amd/csrc/ef_thin.inc).

The operation is restated in numpy from the header alone (tests/thinref.py).  Its outcome is a pure function of the map (no sums, no order
dependence), so everything is compared BIT FOR BIT: the two row lists, the counts, the gathered representatives and the map a thin leaves.
The scenes are hand-built; a CPU-side test first shows that they contain every edge the header names.
"""
import ctypes as C
import os

import numpy as np
import pytest

import selectref as sr
import thinref as tr
from queryref import assert_bits_equal, cells_of, hash_of
from test_gpu_select import refused, sixteen, state_of, step, to_api, u32   # noqa: F401  (sixteen is a fixture)

pytestmark = pytest.mark.gpu

F = np.float32
KEEPS = (tr.KEEP_MAX_CONF, tr.KEEP_NEWEST, tr.KEEP_FIRST)
EDGE_CELLS = (0.02, 2.0 ** -6, 0.05)
CLAMP_CELL = 2.0 ** -20


def rows_of(n):
    S = np.zeros((n, 12), F)
    S[:, 3] = 5
    S[:, 4] = 0x808080
    S[:, 6] = 1
    S[:, 7] = 2
    S[:, 10] = 1
    S[:, 11] = 0.004
    return S


def interleave(groups, rng=None):
    """the rows of the groups dealt round-robin (group 0's first row, group 1's first row, ...), so that a cell's rows lie far apart"""
    order = []
    for k in range(max(len(g) for g in groups)):
        for gi, g in enumerate(groups):
            if k < len(g):
                order.append((gi, k))
    return np.stack([groups[gi][k] for gi, k in order]), np.array([gi for gi, _ in order])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the scenes (pure numpy)
# ---------------------------------------------------------------------------------------------------------------------------------------
def edge_scene():
    """cell edges: on every axis, coordinates at exact multiples of each cell and one float to either side, negative ones, -0.0 beside +0.0,
    and one pair beyond the +-2^20 clamp of cell 2^-20.  Each cluster lies metres from every other."""
    rng = np.random.default_rng(31)
    pts = []
    for ci, cell in enumerate(EDGE_CELLS):
        for axis in range(3):
            centre = np.array([7.0 * (ci + 1), 3.0 * (axis + 1), -5.0], np.float64)
            centre = (np.floor(centre / cell) + 0.5) * cell            # the middle of a cell on the two other axes
            for k in (-9, -1, 0, 1, 14):
                v = F(F(k) * F(cell))
                for x in (step(v, False), v, step(v, True)):
                    for _ in range(3):                                 # three surfels per coordinate: they compete
                        p = centre.copy()
                        p[axis] = x
                        pts.append(p)
            for z in (-0.0, 0.0):
                p = centre.copy()
                p[axis] = z
                pts.append(p)
    pts = np.array(pts).astype(F)
    S = rows_of(len(pts) + 2)
    S[:len(pts), :3] = pts
    S[len(pts), :3] = (3.0, 0.25, 0.25)        # both beyond the clamp of cell 2^-20 on x, 997 m apart
    S[len(pts) + 1, :3] = (1000.0, 0.25, 0.25)
    S[:, 3] = rng.integers(0, 4, len(S))
    S[:, 7] = rng.integers(0, 4, len(S))
    perm = rng.permutation(len(S) - 2)
    S[:len(S) - 2] = S[perm]
    return S


ORDER_CASES = dict(
    equal_far_apart=[(3.0, 9.0), (3.0, 9.0), (1.0, 1.0)],
    zero_signs=[(-0.0, 0.0), (0.0, -0.0), (-1.0, -2.0)],
    zero_signs_swapped=[(0.0, -0.0), (-0.0, 0.0)],
    plus_inf=[(1e30, 5.0), (np.inf, 1.0), (np.inf, 7.0), (2.0, np.inf)],
    nan_among_numbers=[(np.nan, 1.0), (-4.0, np.nan), (np.nan, 3.0), (-7.0, 2.0)],
    cycle_under_raw_compare=[(1.0, 2.0), (np.nan, np.nan), (2.0, 1.0)],
    all_nan=[(np.nan, np.nan), (np.nan, np.nan), (np.nan, np.nan)],
    nan_and_minus_inf=[(np.nan, -np.inf), (-np.inf, np.nan)],
    disagree=[(1.0, 30.0), (9.0, 10.0), (5.0, 20.0)],
)
# the representative's position in each case's list, per keep (MAX_CONF, NEWEST, FIRST), worked out by hand from the header
ORDER_WANT = dict(equal_far_apart=(0, 0, 0), zero_signs=(0, 0, 0), zero_signs_swapped=(0, 0, 0), plus_inf=(1, 3, 0), nan_among_numbers=(1, 2, 0),
                  cycle_under_raw_compare=(2, 0, 0), all_nan=(0, 0, 0), nan_and_minus_inf=(0, 0, 0), disagree=(1, 0, 0))


def order_scene():
    """(surfels, group of each row, the cases' names): one cell per case, the rows of a case dealt out more than 256 rows apart"""
    names = list(ORDER_CASES)
    groups = []
    for gi, name in enumerate(names):
        g = rows_of(len(ORDER_CASES[name]))
        g[:, :3] = (1.0 + gi, 0.011, 0.011)
        for k, (conf, last) in enumerate(ORDER_CASES[name]):
            g[k, 3], g[k, 7] = conf, last
        groups.append(g)
    for k in range(300 - len(names)):                       # lone surfels in cells of their own: a round of the deal is 300 rows long
        g = rows_of(4)
        g[:, 0], g[:, 1], g[:, 2] = -1.0 - 0.1 * k, 0.011 + np.arange(4), 0.011
        groups.append(g)
    S, gid = interleave(groups)
    return S, gid, names


LONG = (63, 64, 65, 129, 1000)
LONG_AT = ("lowest", "highest", "middle")


def long_scene(at):
    """one cell each with 63 / 64 / 65 / 129 / 1000 participants (whole strides of 64, one over, one under, many), the one strongest surfel at the
    cell's lowest row, at its highest row, or in the middle; all others tie"""
    groups = []
    rng = np.random.default_rng(7)
    for gi, L in enumerate(LONG):
        g = rows_of(L)
        g[:, :3] = np.array([2.0 * gi, 0.5, 0.5]) + rng.uniform(0.001, 0.019, (L, 3))     # inside the cell [2 gi, 2 gi + 0.02) x [0.5, 0.52)^2
        g[:, 3] = 4
        g[:, 7] = 4
        k = dict(lowest=0, highest=L - 1, middle=L // 2)[at]
        g[k, 3], g[k, 7] = 6, 8
        groups.append(g)
    S, gid = interleave(groups)
    return S.astype(F), gid


def shared_bucket_scene():
    """5 distinct cells of the block [0, 12)^3 (cell 0.05) that share one of the 1024 buckets of a map of at most 1024 rows, 70 participants each,
    rows interleaved: one stride of 64 records holds records of several cells"""
    g = np.arange(12)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    h = hash_of(block, 1023)
    b, cnt = np.unique(h, return_counts=True)
    crowded = b[cnt >= 5]
    cells = block[h == crowded[0]][:5]
    rng = np.random.default_rng(17)
    groups = []
    for c in cells:
        q = rows_of(70)
        q[:, :3] = (c + rng.uniform(0.1, 0.9, (70, 3))) * 0.05
        q[:, 3] = rng.integers(0, 3, 70)
        q[:, 7] = rng.integers(0, 3, 70)
        groups.append(q)
    S, gid = interleave(groups)
    return S.astype(F), cells, len(crowded)


def participation_scene():
    rng = np.random.default_rng(23)
    n = 2100
    S = rows_of(n)
    S[:, :3] = rng.uniform(-0.25, 0.25, (n, 3))
    S[:, 3] = rng.integers(0, 10, n)
    S[:, 7] = rng.integers(0, 30, n)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]], F)
    S[50:50 + 4 * 300:300, :3] = bad
    return S


AMONG = dict(
    conf_excludes_the_strongest=sr.default_selection(tests=sr.CONF, conf_min=0.0, conf_max=8.0),
    box_cuts_cells=sr.default_selection(tests=sr.BOX, box_min=[-np.inf, -0.113, -np.inf], box_max=[0.0123, np.inf, 0.2]),
    inverted=sr.default_selection(tests=sr.CONF | sr.INVERT, conf_min=3.0, conf_max=5.0),
    nothing=sr.default_selection(tests=sr.INVERT),
)


def test_the_scenes_contain_every_edge_the_header_names():
    """CPU only in effect (no device call): the reference alone shows that the edges are exercised"""
    S = edge_scene()
    for cell in EDGE_CELLS:
        split = same = 0
        for axis in range(3):
            v = S[:, axis]
            for k in (-9, -1, 0, 1, 14):
                at = F(F(k) * F(cell))
                lo, hi = step(at, False), step(at, True)
                assert (v == at).any() and (v == lo).any() and (v == hi).any(), (cell, axis, k)
                c = cells_of(np.array([[lo, 0, 0], [at, 0, 0], [hi, 0, 0]], F), cell)[:, 0]
                assert c[0] <= c[1] <= c[2] and c[2] - c[0] <= 1
                split += int(c[0] != c[2])
                same += int(c[0] == c[2])
        assert split >= 9, (cell, split, same)      # adjacent floats fall into different cells: the edge is really there
        t = tr.thin(S, cell)
        assert 0 < t["result"]["removed"] < len(S) - 2
    assert (S[:, :3] < 0).any() and (u32(S[:, :3]) == 0x80000000).any() and (u32(S[:, :3]) == 0).any()
    c = cells_of(S[-2:, :3], CLAMP_CELL)
    assert (c[0] == c[1]).all() and c[0, 0] == 1 << 20 and S[-1, 0] - S[-2, 0] > 900            # beyond the clamp: one cell, metres apart
    t = tr.thin(S, CLAMP_CELL)
    assert t["part"][-2:].all() and t["rep"][-2:].sum() == 1 and t["removed"][-2:].sum() == 1
    # ordering: the representatives worked out by hand
    S, gid, names = order_scene()
    for ki, keep in enumerate(KEEPS):
        t = tr.thin(S, 0.02, keep)
        for gi, name in enumerate(names):
            rows = np.nonzero(gid == gi)[0]
            assert np.diff(rows).min() >= 256, name
            assert t["rep"][rows].sum() == 1 and t["removed"][rows].sum() == len(rows) - 1, name
            assert np.nonzero(t["rep"][rows])[0][0] == ORDER_WANT[name][ki], (name, keep)
    assert np.isnan(S[:, 3]).any() and np.isposinf(S[:, 3]).any() and (u32(S[:, 3]) == 0x80000000).any()
    # long cells: the lengths around the stride of 64, the winner where it was put
    for at in LONG_AT:
        S, gid = long_scene(at)
        t = tr.thin(S, 0.02)
        assert t["result"] == dict(participants=sum(LONG), cells=len(LONG), removed=sum(LONG) - len(LONG), count_after=len(LONG))
        for gi, L in enumerate(LONG):
            rows = np.nonzero(gid == gi)[0]
            assert len(rows) == L and len(np.unique(cells_of(S[rows, :3], 0.02), axis=0)) == 1
            assert t["rows_rep"][gi] == rows[dict(lowest=0, highest=L - 1, middle=L // 2)[at]]
    # shared buckets
    S, cells, crowded = shared_bucket_scene()
    print("buckets of the 12^3 block that hold >= 5 cells:", crowded)
    assert crowded >= 1 and len(S) == 350 and len(S) <= 1024
    got = cells_of(S[:, :3], 0.05)
    assert len(np.unique(got, axis=0)) == 5 and len(np.unique(hash_of(got, 1023))) == 1
    assert len(np.unique(got[:64], axis=0)) == 5, "one stride holds records of several cells"
    # participation
    S = participation_scene()
    fin = np.isfinite(S[:, :3]).all(1)
    assert (~fin).sum() == 4
    t0 = tr.thin(S, 0.05)
    t = tr.thin(S, 0.05, among=AMONG["conf_excludes_the_strongest"])
    strongest = S[:, 3] == 9
    assert (t0["rep"] & strongest).sum() > 100 and not t["part"][strongest].any() and t["kept"][strongest].all()
    t = tr.thin(S, 0.05, among=AMONG["box_cuts_cells"])
    c = cells_of(np.nan_to_num(S[:, :3], posinf=0, neginf=0), 0.05)
    cut = np.unique(c[t["part"]], axis=0)
    outside = np.unique(c[~t["part"] & fin], axis=0)
    assert len(set(map(tuple, cut)) & set(map(tuple, outside))) > 20, "cells with surfels on both sides of the box"
    for name, a in AMONG.items():
        t = tr.thin(S, 0.05, among=a)
        assert t["kept"][~fin].all() and not t["part"][~fin].any(), name
        assert (name == "nothing") == (t["result"]["participants"] == 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the device against the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    yield ef
    ef.close()


def check_lists(ef, S, cell, keep, among=None, what=""):
    """both lists and their counts against the reference; returns the reference"""
    t = tr.thin(S, cell, keep, among)
    a = None if among is None else to_api(ef, among)
    rem, n_rem = ef.thinSelect(cell=float(cell), keep=keep, among=a, count=True)
    rep, n_rep = ef.thinSelect(cell=float(cell), keep=keep, among=a, representatives=True, count=True)
    print(what, "cell", cell, "keep", keep, "rows", len(S), t["result"])
    assert n_rem == t["result"]["removed"] and n_rep == t["result"]["cells"], (what, cell, keep, n_rem, n_rep, t["result"])
    assert rem.dtype == np.uint32 and np.array_equal(rem, t["rows_removed"]), (what, cell, keep, np.setxor1d(rem, t["rows_removed"])[:8])
    assert np.array_equal(rep, t["rows_rep"]), (what, cell, keep, np.setxor1d(rep, t["rows_rep"])[:8])
    return t


def test_cell_edges(ctx):
    S = edge_scene()
    ctx.uploadMap(S)
    for cell in EDGE_CELLS + (CLAMP_CELL,):
        check_lists(ctx, S, cell, tr.KEEP_MAX_CONF, what="edges")
    check_lists(ctx, S, 0.02, tr.KEEP_NEWEST, what="edges")


@pytest.mark.parametrize("keep", KEEPS)
def test_ordering(ctx, keep):
    S, gid, names = order_scene()
    ctx.uploadMap(S)
    check_lists(ctx, S, 0.02, keep, what="ordering")


@pytest.mark.parametrize("at", LONG_AT)
def test_long_cells(ctx, at):
    S, gid = long_scene(at)
    ctx.uploadMap(S)
    for keep in (tr.KEEP_MAX_CONF, tr.KEEP_NEWEST):
        t = check_lists(ctx, S, 0.02, keep, what="long " + at)
        assert t["result"]["cells"] == len(LONG)
    # all primaries tie: the lowest row of every cell
    t = check_lists(ctx, S, 0.02, tr.KEEP_FIRST, what="long, first")
    assert [int(r) for r in t["rows_rep"]] == [int(np.nonzero(gid == gi)[0][0]) for gi in range(len(LONG))]


def test_shared_buckets(ctx):
    S, cells, _ = shared_bucket_scene()
    ctx.uploadMap(S)
    for keep in KEEPS:
        t = check_lists(ctx, S, 0.05, keep, what="shared bucket")
        assert t["result"]["cells"] == 5 and t["result"]["removed"] == 345


def test_participation():
    from elasticfusion_amd import api
    S = participation_scene()
    ef = api.ElasticFusion()
    try:
        ef.setSurfelIds(True)
        ef.uploadMap(S)                                       # a zero ID lane: the rows are numbered by the first ID-consuming call
        idsel = ef.mapSelection(tests=sr.ID, id_min=400, id_max=1800)
        rem = ef.thinSelect(cell=0.05, among=idsel)           # ... which is this one (ids_prepare inside the thin)
        M = ef.downloadMap()
        ids = u32(M[:, 5])
        assert (ids > 0).all() and (np.diff(ids.astype(np.int64)) > 0).all()
        assert_bits_equal(np.delete(M, 5, 1), np.delete(S, 5, 1), "the uploaded scene")
        t = tr.thin(M, 0.05, among=sr.default_selection(tests=sr.ID, id_min=400, id_max=1800))
        assert 0 < t["result"]["participants"] < len(S) and np.array_equal(rem, t["rows_removed"])
        for name, a in AMONG.items():
            for keep in (tr.KEEP_MAX_CONF, tr.KEEP_NEWEST):
                t = check_lists(ef, M, 0.05, keep, among=a, what=name)
                assert not t["part"][~np.isfinite(S[:, :3]).all(1)].any()
        t = check_lists(ef, M, 0.05, tr.KEEP_MAX_CONF, among=sr.default_selection(tests=sr.ID | sr.CONF, id_min=400, id_max=1800, conf_min=2.0,
                                                                                 conf_max=7.0), what="id and conf")
        # a dict of mapSelection keywords is accepted as well
        assert np.array_equal(ef.thinSelect(cell=0.05, among=dict(tests=sr.ID | sr.CONF, id_min=400, id_max=1800, conf_min=2.0, conf_max=7.0)),
                              t["rows_removed"])
        # the thin itself, among a selection: non-participants stay, the IDs of the kept rows stay
        res = ef.thinSurfels(cell=0.05, among=to_api(ef, AMONG["conf_excludes_the_strongest"]))
        t = tr.thin(M, 0.05, among=AMONG["conf_excludes_the_strongest"])
        assert res == t["result"], (res, t["result"])
        assert_bits_equal(ef.downloadMap(), M[t["kept"]], "the thinned map")
        assert np.array_equal(ef.surfelIds(), ids[t["kept"]])
    finally:
        ef.close()


def line_map(n):
    S = rows_of(n)
    i = np.arange(n)
    S[:, 0] = (i // 3) * F(0.02) + F(0.003) * (i % 3)        # three surfels per 2 cm
    S[:, 1:3] = 0.005
    S[:, 3] = (i * 7) % 5
    S[:, 7] = (i * 3) % 4
    return S


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257, 1024, 1025))
def test_sizes(ctx, n):
    S = line_map(n)
    ctx.uploadMap(S)
    assert ctx.lastCount() == n
    for keep in KEEPS:
        t = check_lists(ctx, S, 0.02, keep, what="sizes")
    total = t["result"]["removed"]
    for cap in sorted({0, 1, max(total - 1, 0), total, total + 1}):
        rows, got = ctx.thinSelect(cell=0.02, keep=tr.KEEP_FIRST, max_rows=cap, count=True)
        assert got == total and np.array_equal(rows, t["rows_removed"][:cap]), (n, cap, got, total)   # the count is the total, however short the list
    res = ctx.thinSurfels(cell=0.02, keep=tr.KEEP_FIRST)
    assert res == t["result"], (res, t["result"])
    assert_bits_equal(ctx.downloadMap(), S[t["kept"]], "the thinned map")


def test_the_whole_map_in_one_cell(ctx):
    """the linear-work case: 65 536 surfels of the octant [0, 1)^3 at cell 1e6 are one cell (negative coordinates would make eight)"""
    rng = np.random.default_rng(41)
    n = 65536
    S = rows_of(n)
    P = rng.uniform(0, 1, (n, 3)).astype(F)
    P[P >= 1] = 0.5                                # (a double just below 1 may round up)
    S[:, :3] = P
    S[:, 3] = rng.integers(0, 8, n)
    S[:, 7] = rng.integers(0, 100, n)
    ctx.uploadMap(S)
    for keep in KEEPS:
        t = check_lists(ctx, S, 1e6, keep, what="one cell")
        assert t["result"] == dict(participants=n, cells=1, removed=n - 1, count_after=1)
    res = ctx.thinSurfels(cell=1e6)
    assert res == dict(participants=n, cells=1, removed=n - 1, count_after=1), res
    assert_bits_equal(ctx.downloadMap(), S[tr.thin(S, 1e6)["kept"]], "the one surfel left")


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(43)
    n = 200000
    S = rows_of(n)
    S[:, :3] = rng.uniform(-1, 1, (n, 3))
    S[:, 3] = rng.integers(0, 8, n)                # ties are the rule
    S[:, 7] = rng.integers(0, 16, n)
    return S, {keep: tr.thin(S, 0.05, keep) for keep in KEEPS}


def test_random_scene_with_ties_everywhere(ctx, big):
    S, want = big
    ctx.uploadMap(S)
    for keep in KEEPS:
        t = want[keep]
        rem, n_rem = ctx.thinSelect(cell=0.05, keep=keep, count=True)
        rep, n_rep = ctx.thinSelect(cell=0.05, keep=keep, representatives=True, count=True)
        print("200 000 rows, keep", keep, t["result"])
        assert (n_rem, n_rep) == (t["result"]["removed"], t["result"]["cells"])
        assert np.array_equal(rem, t["rows_removed"]) and np.array_equal(rep, t["rows_rep"])
    assert t["result"]["cells"] > 50000


def test_device_variant_lists_gather_and_thinned_map(ctx, big):
    from elasticfusion_amd import accuracy, api
    S, want = big
    ctx.uploadMap(S)
    t = want[tr.KEEP_MAX_CONF]
    prm = ctx.thinParams(cell=0.05)
    assert prm.keep == api.THIN_KEEP_MAX_CONF
    for representatives, rows_want in ((False, t["rows_removed"]), (True, t["rows_rep"])):
        cap = len(rows_want) - 7
        rows = api.DevBuf.from_array(np.full(cap + 16, 0xABABABAB, np.uint32))
        cnt = api.DevBuf.from_array(np.zeros(1, np.uint32))
        ctx.thinSelectDevice(prm, None, representatives, rows.p, cap, cnt.p)
        ctx.synchronize()
        got = rows.to_array(np.uint32, cap + 16)
        assert cnt.to_array(np.uint32, 1)[0] == len(rows_want)
        assert np.array_equal(got[:cap], rows_want[:cap]) and (got[cap:] == 0xABABABAB).all()      # nothing is written past max_rows
        ctx.thinSelectDevice(prm, None, representatives, None, 0, cnt.p)                               # a count only
        ctx.synchronize()
        assert cnt.to_array(np.uint32, 1)[0] == len(rows_want)
    M = ctx.downloadMap()
    assert_bits_equal(M, S, "thinSelect changes nothing")
    assert_bits_equal(ctx.gatherSurfels(ctx.thinSelect(prm, representatives=True)), M[t["rows_rep"]], "gather(representatives)")
    assert_bits_equal(accuracy.thinned_map(ctx, 0.05, keep=api.THIN_KEEP_NEWEST), M[want[tr.KEEP_NEWEST]["rows_rep"]], "thinned_map")
    a = sr.default_selection(tests=sr.CONF, conf_min=2.0, conf_max=6.0)
    assert_bits_equal(accuracy.thinned_map(ctx, 0.05, among=to_api(ctx, a)), M[tr.thin(S, 0.05, among=a)["rows_rep"]], "thinned_map among")
    assert ctx.lastCount() == len(S)
    # the removed list is what eraseRows takes: the same map as the thin leaves, and a second identical thin removes nothing
    assert ctx.eraseRows(t["rows_removed"]) == t["result"]["removed"]
    assert_bits_equal(ctx.downloadMap(), S[t["kept"]], "eraseRows(thinSelect)")
    ctx.uploadMap(S)
    res = ctx.thinSurfels(prm)
    assert res == t["result"], (res, t["result"])
    assert_bits_equal(ctx.downloadMap(), S[t["kept"]], "thinSurfels")
    again = ctx.thinSurfels(prm)
    assert again == dict(participants=res["cells"], cells=res["cells"], removed=0, count_after=res["count_after"]), again
    assert_bits_equal(ctx.downloadMap(), S[t["kept"]], "a second identical thin")


def test_queries_are_not_disturbed_by_a_thin_at_another_cell(ctx):
    S = participation_scene()
    ctx.uploadMap(S)
    pts = S[np.isfinite(S[:, :3]).all(1)][:500, :3] + F(0.002)
    before = ctx.queryNearestRaw(pts, 0.03, -1.0)
    t = check_lists(ctx, S, 0.11, tr.KEEP_MAX_CONF, what="between two queries")      # the index is rebuilt at 0.11 ...
    after = ctx.queryNearestRaw(pts, 0.03, -1.0)                                    # ... and again at the query's own cell
    for b, a, what in zip(before, after, ("row", "dist2", "plane")):
        assert_bits_equal(a, b, "queryNearest " + what)
    assert (before[0] != 0xFFFFFFFF).sum() > 400
    assert np.array_equal(ctx.thinSelect(cell=0.11), t["rows_removed"])              # and back


def test_ids_are_kept_and_never_reused(frames):
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    try:
        ef.setSurfelIds(True)
        for k in range(3):
            ef.processFrame(frames[k][0], frames[k][1], k)
        before = ef.downloadMap()               # (numbers the rows the last frame created)
        ids = u32(before[:, 5])
        largest = int(ids.max())
        t = tr.thin(before, 0.01, tr.KEEP_NEWEST)
        res = ef.thinSurfels(cell=0.01, keep=api.THIN_KEEP_NEWEST)
        print("surfels", len(before), res)
        assert res == t["result"] and res["removed"] > 1000 and res["cells"] > 1000
        assert_bits_equal(ef.downloadMap(), before[t["kept"]], "thin after frames")
        assert np.array_equal(ef.surfelIds(), ids[t["kept"]])
        ef.processFrame(frames[3][0], frames[3][1], 3)
        after = ef.surfelIds()
        new = ~np.isin(after, ids)
        assert new.sum() > 0 and int(after[new].min()) > largest and (np.diff(after.astype(np.int64)) > 0).all()
    finally:
        ef.close()


def test_thin_then_mapping_equals_upload_and_restore(sixteen):
    from elasticfusion_amd import api
    fr = sixteen

    def feed(ef, k):
        ef.processFrame(fr[k][0], fr[k][1], k * 33333)

    a, b, plain = api.ElasticFusion(), api.ElasticFusion(), api.ElasticFusion()
    try:
        for k in range(8):
            feed(a, k)
            feed(plain, k)
        m8 = a.downloadMap()
        t = tr.thin(m8, 0.01)
        ck = a.checkpoint(fr[7][0], fr[7][1])
        res = a.thinSurfels(cell=0.01)
        print("frame 8: surfels", len(m8), res)
        assert res == t["result"] and res["removed"] > 1000 and res["cells"] > 1000
        assert_bits_equal(a.downloadMap(), m8[t["kept"]], "the thinned map")
        assert a.getTick() == ck["tick"] and np.array_equal(a.getPoseQT(), ck["qt"])
        ck["map"] = m8[t["kept"]]
        b.restore(ck)
        for k in range(8, 16):
            feed(a, k)
            feed(b, k)
            feed(plain, k)
            (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
            assert np.array_equal(qa.view(np.uint64), qb.view(np.uint64)), (k, qa, qb)
            assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), (k, sa, sb)
            assert_bits_equal(ma, mb, f"the map after frame {k}")
        mp = plain.downloadMap()
        assert mp.shape != ma.shape or not np.array_equal(u32(mp), u32(ma)), "the thin mattered"
    finally:
        for ef in (a, b, plain):
            ef.close()


def test_state_refusals():
    import ctypes.util
    from elasticfusion_amd import api
    S = line_map(1000)
    t = tr.thin(S, 0.02)
    ef = api.ElasticFusion(closeLoops=True)
    try:
        ef.uploadMap(S)
        assert "close_loops" in refused(lambda: ef.thinSurfels(cell=0.02), -4)          # EF_ESTATE
        assert ef.lastCount() == 1000
        assert_bits_equal(ef.downloadMap(), S, "a refused thin leaves the map")
        assert np.array_equal(ef.thinSelect(cell=0.02), t["rows_removed"])                # the lists work there
        assert np.array_equal(ef.thinSelect(cell=0.02, representatives=True), t["rows_rep"])
    finally:
        ef.close()
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        assert "IDs are off" in refused(lambda: ef.thinSelect(cell=0.02, among=dict(tests=sr.ID)), -4)
        assert "IDs are off" in refused(lambda: ef.thinSurfels(cell=0.02, among=dict(tests=sr.ID)), -4)
        refused(lambda: ef.thinSelect(cell=0.0), -1)                                      # EF_EINVAL
        refused(lambda: ef.thinSurfels(keep=3), -1)
        name = ctypes.util.find_library("amdhip64") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")
        hip = C.CDLL(name)
        s = C.c_void_p(ef.stream())
        d = api.DevBuf(64)
        ef_params = ef.thinParams(cell=0.02)
        ef.synchronize()
        assert hip.hipStreamBeginCapture(s, C.c_int(2)) == 0   # relaxed
        try:
            assert "captured" in refused(lambda: ef.thinSelect(cell=0.02, max_rows=8), -4)
            assert "captured" in refused(lambda: ef.thinSelectDevice(ef_params, None, False, d.p, 8, d.p), -4)
            assert "captured" in refused(lambda: ef.thinSurfels(ef_params), -4)
        finally:
            g = C.c_void_p()
            assert hip.hipStreamEndCapture(s, C.byref(g)) == 0
            if g.value:
                hip.hipGraphDestroy(g)
        ef.synchronize()
        assert ef.lastCount() == 1000
        assert ef.thinSurfels(cell=0.02) == t["result"]
    finally:
        ef.close()
