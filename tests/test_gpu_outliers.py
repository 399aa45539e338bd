"""Remove outlier surfels on the device (ef_map_neighbor_stats / ef_map_outliers_select / ef_map_remove_outliers, include/ef_hip.h; kernels in
elasticfusion_amd/csrc/ef_outlier.inc).

The operation is restated in numpy from the header alone (tests/outlierref.py).  The header fixes every rounding and the order of both sums, so
everything is compared BIT FOR BIT: mean distances, counts, the two sums, the threshold, the row lists and the map a removal leaves.  The scenes
(tests/outlierscenes.py) are hand-built; tests/test_outlier_host.py shows on the CPU that they contain every edge they claim.
"""
import ctypes as C

import numpy as np
import pytest

import outlierref as oref
import outlierscenes as sc
from queryref import assert_bits_equal
from test_gpu_select import refused, sixteen, state_of   # noqa: F401  (sixteen is a fixture)

pytestmark = pytest.mark.gpu

F = np.float32


def check_result(got, want, what):
    for key in ("participants", "measured", "sparse", "outliers", "count_after"):
        assert got[key] == want[key], (what, key, got, want)
    for key in ("sum", "sum_sq"):
        assert np.float64(got[key]).view(np.uint64) == np.float64(want[key]).view(np.uint64), (what, key, got[key].hex(), float(want[key]).hex())
    assert F(got["threshold"]).view(np.uint32) == F(want["threshold"]).view(np.uint32), (what, got["threshold"], want["threshold"])


def check_select(ef, S, nb, what, among=None, among_mask=None, **kw):
    want = oref.outliers(S, among=among_mask, nb=nb, **{k: v for k, v in kw.items() if k != "cell"})
    rows, total, res = ef.outlierSelect(among=among, count=True, result=True, **kw)
    assert total == len(want["rows"]) and np.array_equal(rows, want["rows"]), (what, total, len(want["rows"]))
    check_result(res, want["result"], what)
    return want


# ---------------------------------------------------------------------------------------------------------------------------------------
# per-row statistics
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stats():
    from elasticfusion_amd import api
    S, marks = sc.stats_scene()
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    thr = float(ef.getConfidenceThreshold())
    assert sc.CONF_LOW < thr < sc.CONF_HIGH
    nb = {mc: oref.neighbours(S, sc.R_STATS, mc) for mc in (-1.0, thr)}
    yield dict(ef=ef, S=S, marks=marks, thr=thr, nb=nb)
    ef.close()


@pytest.mark.parametrize("stable_only", (False, True))
@pytest.mark.parametrize("cell", (sc.R_STATS, sc.R_STATS / 16))
def test_stats_equal_the_scan_exactly(stats, cell, stable_only):
    ef, S = stats["ef"], stats["S"]
    mc = stats["thr"] if stable_only else -1.0
    count, D = stats["nb"][mc]
    for k in sc.STATS_KS:
        mean, cnt = ef.neighborStats(radius=sc.R_STATS, cell=cell, k=k, min_conf=mc)
        assert np.array_equal(cnt, count), (k, np.nonzero(cnt != count)[0][:10])
        assert_bits_equal(mean, oref.mean_dist(count, D, k), f"mean_dist k={k} cell={cell} min_conf={mc}")
    mean, cnt = ef.neighborStats(mode=oref.RADIUS, radius=sc.R_STATS, cell=cell, k=12, min_conf=mc)      # RADIUS: k is ignored, the mean is that of k = 1
    assert np.array_equal(cnt, count)
    assert_bits_equal(mean, oref.mean_dist(count, D, 1), "mean_dist in RADIUS mode")
    assert ef.lastCount() == len(S)
    assert_bits_equal(ef.downloadMap(), S, "the stats change nothing")


@pytest.mark.parametrize("n", (2048, 2049))
def test_bucket_steps(n):
    from elasticfusion_amd import api
    S = sc.plain_scene(n, seed=n)
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        nb = oref.neighbours(S, sc.R_SUMS)
        for k in (1, 8):
            mean, cnt = ef.neighborStats(radius=sc.R_SUMS, cell=sc.R_SUMS, k=k)
            assert np.array_equal(cnt, nb[0]), k
            assert_bits_equal(mean, oref.mean_dist(*nb, k), f"mean_dist at {n} rows, k={k}")
        want = check_select(ef, S, nb, f"{n} rows", radius=sc.R_SUMS, cell=sc.R_SUMS)
        assert 0 < len(want["rows"]) < n
    finally:
        ef.close()


def test_among_a_box_and_its_inversion(stats):
    from elasticfusion_amd import api
    ef, S = stats["ef"], stats["S"]
    nb = stats["nb"][-1.0]
    box = dict(box_min=[0.05, 0.0, -1.0], box_max=[0.2, 0.15, 50.0])                 # cuts through the random cloud
    for tests in (api.SEL_BOX, api.SEL_BOX | api.SEL_INVERT):
        sel = ef.mapSelection(tests=tests, **box)
        mask = np.zeros(len(S), bool)
        mask[ef.selectSurfels(sel)] = True
        assert 100 < mask.sum() < len(S) - 100
        part = oref.participants(S, mask)
        count, D = oref.neighbours(S, sc.R_STATS, -1.0, part)
        # a row that takes no part still counts as a neighbour: the participants' counts are those of the whole map
        assert np.array_equal(count[part], nb[0][part]) and (count[~part] == 0).all() and (nb[0][~part] > 0).any()
        for k in (1, 5):
            mean, cnt = ef.neighborStats(among=sel, radius=sc.R_STATS, cell=sc.R_STATS, k=k)
            assert np.array_equal(cnt, count)
            assert_bits_equal(mean, oref.mean_dist(count, D, k), f"mean_dist among tests={tests:#x} k={k}")
            assert np.isinf(mean[~part]).all()
        want = check_select(ef, S, (count, D), f"among tests={tests:#x}", among=sel, among_mask=mask, radius=sc.R_STATS, cell=sc.R_STATS, k=5)
        assert 0 < len(want["rows"]) and mask[want["rows"]].all()
        check_select(ef, S, (count, D), "among, RADIUS", among=dict(tests=tests, **box), among_mask=mask, mode=oref.RADIUS, radius=sc.R_STATS,
                     cell=sc.R_STATS, min_neighbors=3)


# ---------------------------------------------------------------------------------------------------------------------------------------
# sums, threshold, flags
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sums():
    from elasticfusion_amd import api
    S = sc.sums_scene()
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    yield dict(ef=ef, S=S, nb=oref.neighbours(S, sc.R_SUMS))
    ef.close()


def test_sums_threshold_and_list_equal_the_reference(sums):
    ef, S, nb = sums["ef"], sums["S"], sums["nb"]
    assert len(S) == 2 * oref.P + 5
    seen = []
    for cell in (sc.R_SUMS, sc.R_SUMS / 2, sc.R_SUMS):          # two cells (another order inside the buckets), and the first one again
        want = check_select(ef, S, nb, f"cell {cell}", radius=sc.R_SUMS, cell=cell)
        seen.append((ef.outlierSelect(radius=sc.R_SUMS, cell=cell, count=True, result=True), want))
    (r0, t0, res0) = seen[0][0]
    for (rows, total, res), _ in seen[1:]:
        assert np.array_equal(rows, r0) and total == t0 and res == res0
    print("sums scene:", res0)
    assert res0["measured"] > 7000 and res0["sparse"] > 40 and res0["outliers"] > res0["sparse"]


@pytest.mark.parametrize("kw", (dict(std_ratio=0.0), dict(max_mean_dist=0.0125), dict(k=16, std_ratio=1.0), dict(flag_sparse=0),
                                dict(mode=oref.RADIUS, min_neighbors=0), dict(mode=oref.RADIUS, min_neighbors=1),
                                dict(mode=oref.RADIUS, min_neighbors=20), dict(mode=oref.RADIUS, min_neighbors=40)),
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_threshold_and_radius_cases(sums, kw):
    ef, S, nb = sums["ef"], sums["S"], sums["nb"]
    want = check_select(ef, S, nb, str(kw), radius=sc.R_SUMS, cell=sc.R_SUMS, **kw)
    n_out = len(want["rows"])
    if kw.get("min_neighbors") == 0:
        assert n_out == 0
    elif "max_mean_dist" in kw:
        assert want["result"]["threshold"] == F(0.0125) and want["result"]["sum"] > 0 and 0 < n_out < len(S)
    else:
        assert 0 < n_out < len(S)


@pytest.mark.parametrize("flag_sparse", (0, 1))
def test_nothing_measured(flag_sparse):
    from elasticfusion_amd import api
    S = sc.sparse_scene()
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        want = check_select(ef, S, None, "N = 0", radius=sc.R_SUMS, cell=sc.R_SUMS, flag_sparse=flag_sparse)
        assert want["result"]["measured"] == 0 and np.isinf(want["result"]["threshold"]) and len(want["rows"]) == (len(S) if flag_sparse else 0)
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# lists, device variants
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_list_conventions(sums):
    from elasticfusion_amd import api
    ef, S = sums["ef"], sums["S"]
    full, total = ef.outlierSelect(radius=sc.R_SUMS, count=True)
    assert total == len(full) > 10
    none, t0 = ef.outlierSelect(radius=sc.R_SUMS, max_rows=0, count=True)              # NULL rows with max_rows 0
    assert len(none) == 0 and t0 == total
    prm = ef.outlierParams(radius=sc.R_SUMS)
    rows = np.full(16, 0xABCD1234, np.uint32)
    cnt = C.c_uint32(0)
    api._chk(api.lib().ef_map_outliers_select(ef.h, C.byref(prm), None, api._ptr(rows), 7, C.byref(cnt), None), ef.h)
    assert cnt.value == total and np.array_equal(rows[:7], full[:7]) and (rows[7:] == 0xABCD1234).all()
    rows[:] = 0xABCD1234
    api._chk(api.lib().ef_map_outliers_select(ef.h, C.byref(prm), None, api._ptr(rows), 16, C.byref(cnt), None), ef.h)
    assert np.array_equal(rows, full[:16])
    mean = np.full(len(S) + 3, -7.0, F)                                               # the stats write min(max_rows, map count) entries
    api._chk(api.lib().ef_map_neighbor_stats(ef.h, C.byref(prm), None, api._ptr(mean), None, 100), ef.h)
    assert (mean[100:] == -7.0).all() and (mean[:100] != -7.0).all()
    api._chk(api.lib().ef_map_neighbor_stats(ef.h, C.byref(prm), None, api._ptr(mean), None, len(mean)), ef.h)
    assert (mean[len(S):] == -7.0).all() and (mean[:len(S)] != -7.0).all()


def test_device_variants_equal_the_host_variants(sums):
    from elasticfusion_amd import api
    ef, S = sums["ef"], sums["S"]
    n = len(S)
    for kw in (dict(radius=sc.R_SUMS), dict(radius=sc.R_SUMS, mode=oref.RADIUS, min_neighbors=30, cell=sc.R_SUMS / 2)):
        prm = ef.outlierParams(**kw)
        rows, total, res = ef.outlierSelect(prm, count=True, result=True)
        mean, cnt = ef.neighborStats(prm)
        d_rows, d_cnt, d_res = api.DevBuf(n * 4, fill=0xEE), api.DevBuf(16), api.DevBuf(C.sizeof(api.ef_outlier_result))
        d_mean, d_count = api.DevBuf((n + 2) * 4, fill=0xEE), api.DevBuf((n + 2) * 4, fill=0xEE)
        ef.outlierSelectDevice(prm, None, d_rows.p, n, d_cnt.p, d_res.p)
        ef.neighborStatsDevice(prm, None, d_mean.p, d_count.p, n + 2)
        ef.synchronize()
        assert int(d_cnt.to_array(np.uint32, 1)[0]) == total
        got = d_rows.to_array(np.uint32, n)
        assert np.array_equal(got[:total], rows) and (got[total:] == 0xEEEEEEEE).all()
        raw = d_res.to_array(np.uint8, C.sizeof(api.ef_outlier_result)).tobytes()
        assert ef._outlierResult(api.ef_outlier_result.from_buffer_copy(raw)) == res
        gm, gc = d_mean.to_array(np.uint32, n + 2), d_count.to_array(np.uint32, n + 2)
        assert np.array_equal(gm[:n], mean.view(np.uint32)) and np.array_equal(gc[:n], cnt)
        assert (gm[n:] == 0xEEEEEEEE).all() and (gc[n:] == 0xEEEEEEEE).all()
        ef.outlierSelectDevice(prm, None, None, 0, d_cnt.p)                                # no list, no result
        ef.synchronize()
        assert int(d_cnt.to_array(np.uint32, 1)[0]) == total


# ---------------------------------------------------------------------------------------------------------------------------------------
# removal
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_removal_equals_erasing_the_list(frames):
    from elasticfusion_amd import api
    a, b = api.ElasticFusion(), api.ElasticFusion()
    try:
        for ef in (a, b):
            ef.setSurfelIds(True)
            ef.enableLabels(3)
            for k in range(3):
                ef.processFrame(frames[k][0], frames[k][1], k)
        n = a.lastCount()
        kw = dict(radius=0.01, cell=0.01, k=8, std_ratio=1.0)
        rows, total, res = a.outlierSelect(count=True, result=True, **kw)
        assert 0 < total < n // 2, (total, n)
        got = a.removeOutliers(**kw)
        assert b.eraseRows(rows) == total
        want = dict(res, count_after=n - total)
        assert got == want and a.lastCount() == b.lastCount() == n - total, (got, want)
        (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
        assert_bits_equal(ma, mb, "the map after the removal")
        assert np.array_equal(a.surfelIds(), b.surfelIds())
        (ia, pa), (ib, pb) = a.labels(), b.labels()
        assert np.array_equal(ia, ib)
        assert_bits_equal(pa, pb, "the labels after the removal")
        # not idempotent: what is left has another mean and deviation
        again = a.outlierSelect(count=True, **kw)[1]
        print("surfels", n, "removed", total, "a second call would remove", again)
        for ef in (a, b):
            ef.processFrame(frames[3][0], frames[3][1], 3)
        (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
        assert np.array_equal(qa.view(np.uint64), qb.view(np.uint64)) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
        assert_bits_equal(ma, mb, "the map after the following frame")
        assert len(ma) > n - total
    finally:
        a.close()
        b.close()


def test_a_loop_closing_context_refuses_the_removal_only():
    from elasticfusion_amd import api
    S, _ = sc.stats_scene()
    ef = api.ElasticFusion(closeLoops=True)
    try:
        ef.uploadMap(S)
        assert "close_loops" in refused(lambda: ef.removeOutliers(radius=sc.R_STATS, cell=sc.R_STATS), -4)      # EF_ESTATE
        assert ef.lastCount() == len(S)
        assert_bits_equal(ef.downloadMap(), S, "a refused removal")
        nb = oref.neighbours(S, sc.R_STATS)
        check_select(ef, S, nb, "select on a loop-closing context", radius=sc.R_STATS, cell=sc.R_STATS)
        mean, cnt = ef.neighborStats(radius=sc.R_STATS, cell=sc.R_STATS)
        assert np.array_equal(cnt, nb[0])
        refused(lambda: ef.outlierSelect(k=0), -1)                                                                # EF_EINVAL
        refused(lambda: ef.outlierSelect(radius=1.0, cell=0.01), -1)
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_injected_specks_go_and_the_surface_stays(sixteen):
    from elasticfusion_amd import accuracy, api
    ef = api.ElasticFusion(confidence=2.0)                         # a threshold that sixteen frames reach: most of the map is stable
    try:
        for k in range(16):
            ef.processFrame(sixteen[k][0], sixteen[k][1], k * 33333)
        M = ef.downloadMap()
        n = len(M)
        thr = ef.getConfidenceThreshold()
        rng = np.random.default_rng(3)
        cand = M[rng.choice(n, 600, replace=False)].copy()
        cand[:, :3] += F(0.05) * cand[:, 8:11]                      # 5 cm off the surface along the normal
        miss = ef.queryNearestRaw(cand[:, :3], 0.03, -1.0)[0] == 0xFFFFFFFF          # nothing of the map within the filter's radius
        specks = cand[miss][:200]
        assert len(specks) == 200, int(miss.sum())
        specks[:, 3] = 2 * thr                                       # specks that became stable
        both = np.concatenate([M, specks])
        ef.uploadMap(both)
        stable = both[:, 3] > thr
        stable[n:] = False
        assert stable.sum() > 1000
        rows, total, res = ef.outlierSelect(count=True, result=True)
        flagged = np.zeros(len(both), bool)
        flagged[rows] = True
        share = flagged[stable].mean()
        print(f"map {n} + 200 specks: {total} outliers, {int(flagged[:n].sum())} of the map, share of the original stable surfels {share:.4f}; {res}")
        assert flagged[n:].all(), "an injected speck stays"
        assert share < 0.5
        kept = accuracy.without_outliers(ef)
        assert_bits_equal(kept, both[~flagged], "without_outliers gathers what a removal leaves")
        assert ef.lastCount() == len(both)
        got = ef.removeOutliers()
        assert got["outliers"] == total and got["count_after"] == len(both) - total
        assert_bits_equal(ef.downloadMap(), both[~flagged], "the default removal")
    finally:
        ef.close()
