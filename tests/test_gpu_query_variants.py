"""Every instantiation of k_query<L, K>, the intermediate k, k_register's own butterfly and the index's size edges, pinned to the exhaustive
scan (ef_query_nearest / ef_query_knn / ef_debug_query_lanes, include/ef_hip.h; kernels in elasticfusion_amd/csrc/ef_query.inc and
ef_register.inc).

test_gpu_query.py compares the default dispatch (<16,1>, <1,4>, <1,8>, <1,16>) with the scan.  Here ef_debug_query_lanes selects the others, on
scenes (queryscenes.py) built so that a wrong group merge, a double count through a shared bucket, a box that stops at the cell clamp or a broken
second trip of the tile scan moves an answer.  Every comparison is bit equality with queryref.brute (f32, the header's written order) on rows,
dist2, plane (nearest) and count (kNN).  What a scene is for is asserted on the scan before the device is asked, so no test can pass with
nothing to find.

Which test launches which instantiation against the scan (lanes 16 and 64 with K > 1 dispatch to 8 lanes):

    lanes \\ K   1                             4 (k = 2, 3, 4)             8 (k = 5, 7, 8)             16 (k = 9, 15, 16)
    1           merge[1] box[1] large[1]      merge[1] sizes              merge[1] clamp large[1]     merge[1] box[1]
    8           merge[8] clamp                merge[8, 16, 64]            merge[8] clamp large[8]     merge[8, 16, 64] box[8]
    16          merge[16] box[16] sizes       -                           -                           -
                clamp large[16]
    64          merge[64] box[64]             -                           -                           -

    merge[L] = test_merge_scene_every_k[L], box[L] = test_largest_box_on_fewest_buckets[L], clamp = test_both_sides_of_the_cell_clamp,
    sizes = test_bucket_count_steps, large[L] = test_large_map_second_scan_trip[L]; k_register<16>: test_register_pairs_equal_the_scan.
"""
import contextlib

import numpy as np
import pytest

import queryscenes as qs
from queryref import MISS, assert_bits_equal, brute, buckets_of, cells_of, default_cell, hash_of

pytestmark = pytest.mark.gpu

KS = (2, 3, 4, 5, 7, 8, 9, 15, 16)


@contextlib.contextmanager
def variant(ef, lanes, cell=None):
    """the lane count and cell size for the block; the defaults come back whatever happens inside"""
    try:
        ef.setQueryCell(default_cell() if cell is None else cell)
        ef.debugQueryLanes(lanes)
        yield ef
    finally:
        ef.debugQueryLanes(0)
        ef.setQueryCell(default_cell())


def nearest_equals(ef, Q, max_dist, min_conf, scan, what):
    er, ed, ep, _ = scan
    row, d2, plane = ef.queryNearestRaw(Q, max_dist, min_conf)
    assert_bits_equal(row, np.ascontiguousarray(er[:len(Q), 0]), what + " rows")
    assert_bits_equal(d2, np.ascontiguousarray(ed[:len(Q), 0]), what + " dist2")
    assert_bits_equal(plane, ep[:len(Q)], what + " plane")


def knn_equals(ef, Q, k, max_dist, min_conf, scan, what):
    er, ed, _, ec = scan
    rows, d2, cnt = ef.queryKnn(Q, k, max_dist, min_conf)
    assert_bits_equal(cnt, ec[:len(Q)], what + " count")
    assert_bits_equal(rows, np.ascontiguousarray(er[:len(Q), :k]), what + " rows")
    assert_bits_equal(d2, np.ascontiguousarray(ed[:len(Q), :k]), what + " dist2")
    return rows, d2, cnt


def merge_scans(S, Q):
    """brute(k = 17) per setting of the merge scene, after asserting on it what the scene was built for"""
    scans = {}
    cells = cells_of(S[:, :3], qs.MERGE_CELL)
    for md, mc in qs.MERGE_SETTINGS:
        scan = scans[(md, mc)] = brute(Q, S, md, mc, k=17)
        er, ed, _, ec = scan
        groups = [int((ec == 0).sum()), int(((ec >= 1) & (ec <= 3)).sum()), int(((ec >= 4) & (ec <= 15)).sum()), int((ec > 16).sum())]
        print("max_dist", md, "min_conf", mc, "eligible zero / 1..3 / 4..15 / > 16:", groups)
        assert min(groups) > 0, (md, mc, groups)   # empty lists, lists that run dry inside every K, and more than the largest K
        if mc > 0:   # the nearest surfel of some query is ineligible: it must not take a list slot
            allr = brute(Q, S, md, -1.0)[0][:, 0]
            assert (allr != er[:, 0]).sum() > 100
        if (md, mc) != (0.05, -1.0):
            continue
        ties = {k: int(((ec > k) & (ed[:, k - 1] == ed[:, k])).sum()) for k in (1,) + KS}
        print("queries with a tie exactly at the cut, per k:", ties)
        assert min(ties.values()) > 0, ties   # the row order alone decides what the cut keeps
        full = np.nonzero(ec >= 16)[0]
        ncell = np.array([len({tuple(cells[r]) for r in er[i, :16]}) for i in full])
        print("cells of the top 16: median", float(np.median(ncell)), "max", int(ncell.max()), "all from one cell:", int((ncell == 1).sum()))
        assert (ncell >= 8).any() and (ncell == 1).any()   # winners spread over the group's lanes, and 16 winners on one lane
    return scans


@pytest.fixture(scope="module")
def merge():
    from elasticfusion_amd import api
    S, Q, _ = qs.merge_scene()
    scans = merge_scans(S, Q)
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    yield dict(ef=ef, S=S, Q=Q, scans=scans)
    ef.close()


@pytest.fixture(scope="module")
def ctx():
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    yield ef
    ef.close()


@pytest.mark.parametrize("lanes", [1, 8, 16, 64])
def test_merge_scene_every_k(merge, lanes):
    ef, Q = merge["ef"], merge["Q"]
    with variant(ef, lanes, qs.MERGE_CELL):
        for (md, mc), scan in merge["scans"].items():
            what = f"lanes {lanes} max_dist {md} min_conf {mc}"
            nearest_equals(ef, Q, md, mc, scan, what + " nearest")
            knn_equals(ef, Q, 1, md, mc, scan, what + " k 1")
            for k in KS if lanes in (1, 8) else (4, 16):
                got = knn_equals(ef, Q, k, md, mc, scan, what + f" k {k}")
                if lanes in (16, 64):   # the dispatch maps both to 8 lanes
                    ef.debugQueryLanes(8)
                    ref = ef.queryKnn(Q, k, md, mc)
                    ef.debugQueryLanes(lanes)
                    for a, b, name in zip(got, ref, ("rows", "dist2", "count")):
                        assert_bits_equal(a, b, what + f" k {k} {name} against 8 lanes")
            for n in (1, 3, 17):   # fewer queries than one group, one wave, one workgroup hold
                nearest_equals(ef, Q[:n], md, mc, scan, what + f" nearest, {n} queries")
                knn_equals(ef, Q[:n], 16, md, mc, scan, what + f" k 16, {n} queries")


def test_register_pairs_equal_the_scan(merge):
    """k_register carries its own copy of the 16-lane butterfly: with the identity the f32 transform returns the points unchanged, so its pairs
    are the scan's nearest rows.  The sums are bounded by test_gpu_register.py."""
    ef, Q = merge["ef"], merge["Q"]
    assert np.isfinite(Q).all()   # ((1 * x + 0 * y) + 0 * z) + 0 == x then (a -0 would become +0, which no difference q - p can tell)
    with variant(ef, 0, qs.MERGE_CELL):
        for (md, mc), (er, _, ep, _) in merge["scans"].items():
            out = ef.registerStep(Q, None, T=None, pairs=True, max_dist=md, min_conf=mc)
            assert_bits_equal(out["row"], np.ascontiguousarray(er[:, 0]), f"max_dist {md} min_conf {mc} rows")
            assert_bits_equal(out["plane"], ep, f"max_dist {md} min_conf {mc} plane")
            assert out["pairs"] == int((er[:, 0] != MISS).sum()) > 0 and out["points"] == len(Q)


@pytest.fixture(scope="module")
def box():
    S, Q = qs.box_scene()
    cell, md = 0.0625, 1.0
    assert md / cell == 16 and buckets_of(len(S)) == 1024
    scan = brute(Q, S, md, -1.0, k=16)
    ec = scan[3]
    print("eligible min / median / max", int(ec.min()), float(np.median(ec)), int(ec.max()))
    assert ec.min() >= 40 and ec.max() <= len(S)
    cells = cells_of(S[:, :3], cell)
    h = hash_of(cells, 1023)
    shared = sum(len({tuple(c) for c in cells[h == b]}) > 1 for b in np.unique(h))
    print("buckets used", len(np.unique(h)), "holding surfels of more than one cell", shared)
    assert shared >= 100   # a surfel is seen in the visits of other cells of the box: only the own-cell test keeps it from being counted again
    return dict(S=S, Q=Q, cell=cell, md=md, scan=scan)


@pytest.mark.parametrize("lanes", [1, 8, 16, 64])
def test_largest_box_on_fewest_buckets(ctx, box, lanes):
    ef, Q, md, scan = ctx, box["Q"], box["md"], box["scan"]
    ef.uploadMap(box["S"])
    with variant(ef, lanes, box["cell"]):
        if lanes in (1, 8):
            knn_equals(ef, Q, 16, md, -1.0, scan, f"lanes {lanes} k 16")
        if lanes in (1, 16, 64):
            nearest_equals(ef, Q, md, -1.0, scan, f"lanes {lanes} nearest")


def test_both_sides_of_the_cell_clamp(ctx):
    """surfels and queries within max_dist of each other on both sides of the +-2^20 cell clamp: the box of a query below the clamp has to reach
    the boundary cell that everything beyond shares, and a query beyond it has to reach back"""
    ef = ctx
    S, Q = qs.clamp_scene()
    cells = cells_of(S[:, :3], qs.CLAMP_CELL)
    beyond = cells[:, 0] == 1048576
    print("x cells below the clamp", int((~beyond).sum()), "at it", int(beyond.sum()), "; y cells at the lower clamp", int((cells[:, 1] == -1048576).sum()))
    assert (~beyond).sum() >= 400 and beyond.sum() >= 400 and cells[:, 0].max() == 1048576
    assert (cells[:, 1] == -1048576).any() and (cells[:, 1] > -1048576).any()
    ef.uploadMap(S)
    with variant(ef, 0, qs.CLAMP_CELL):
        for md in (8 * 2.0 ** -20, 16 * 2.0 ** -20):
            scan = brute(Q, S, md, -1.0, k=8)
            er, _, _, ec = scan
            across = int((beyond[er[:, 1].astype(np.int64)] != beyond).sum())
            print("max_dist", md, "second nearest across the clamp", across, "eligible min / median", int(ec.min()), float(np.median(ec)))
            assert across > 0 and ec.min() > 8
            for lanes in (0, 8):
                ef.debugQueryLanes(lanes)
                nearest_equals(ef, Q, md, -1.0, scan, f"max_dist {md} lanes {lanes} nearest")
                knn_equals(ef, Q, 8, md, -1.0, scan, f"max_dist {md} lanes {lanes} k 8")


def test_bucket_count_steps(ctx):
    """maps of 1023 .. 2049 surfels cross 1024 -> 2048 -> 4096 buckets (one, two and four scan tiles)"""
    ef = ctx
    S, Q, _ = qs.merge_scene()
    Q = Q[:200]
    sizes = (1023, 1024, 1025, 2048, 2049)
    assert [buckets_of(n) for n in sizes] == [1024, 1024, 2048, 2048, 4096]
    with variant(ef, 0, qs.MERGE_CELL):
        for n in sizes:
            scan = brute(Q, S[:n], 0.05, -1.0, k=4)
            assert (scan[3] > 4).any() and (scan[3] < 4).any()   # lists cut at k and lists padded with misses
            ef.uploadMap(S[:n])
            nearest_equals(ef, Q, 0.05, -1.0, scan, f"{n} surfels nearest")
            knn_equals(ef, Q, 4, 0.05, -1.0, scan, f"{n} surfels k 4")


@pytest.fixture(scope="module")
def large():
    S, Q = qs.large_scene()
    nb = buckets_of(len(S))
    assert nb == 1 << 21   # 2048 scan tiles: k_scan_chunks scans 1024 a trip
    scan = brute(Q, S, 0.02, -1.0, k=8, chunk=16)
    hit = scan[0][:, 0] != MISS
    b = hash_of(cells_of(S[scan[0][hit, 0].astype(np.int64), :3], default_cell()), nb - 1)
    lo, hi = int((b < (1 << 20)).sum()), int((b >= (1 << 20)).sum())
    print("hits", int(hit.sum()), "misses", int((~hit).sum()), "; winners in buckets below 2^20", lo, "and from 2^20", hi)
    assert lo >= 50 and hi >= 50 and (~hit).any()   # a broken second trip of the tile scan moves real answers
    return dict(S=S, Q=Q, scan=scan)


@pytest.mark.parametrize("lanes", [16, 1, 8])
def test_large_map_second_scan_trip(ctx, large, lanes):
    ef, Q, scan = ctx, large["Q"], large["scan"]
    ef.uploadMap(large["S"])
    with variant(ef, lanes):
        if lanes in (16, 1):
            nearest_equals(ef, Q, 0.02, -1.0, scan, f"lanes {lanes} nearest")
        if lanes in (1, 8):
            knn_equals(ef, Q, 8, 0.02, -1.0, scan, f"lanes {lanes} k 8")
