"""CPU-only checks around the outlier filters (include/ef_hip.h, "Remove outlier surfels"): the numpy restatement (tests/outlierref.py) on cases
whose answers are worked out by hand, the summation order, every EF_EINVAL with a NULL context, the binding of the two new structs and the
constants, and that the scenes of tests/test_gpu_outliers.py contain the edges they claim."""
import ctypes as C
import os

import numpy as np
import pytest

import outlierref as oref
import outlierscenes as sc
from test_api_binding_host import defines, header_structs

F = np.float32
INF = F(np.inf)


def surfels(points, conf=None):
    S = sc.rows_of(len(points))
    S[:, :3] = np.asarray(points, F)
    if conf is not None:
        S[:, 3] = conf
    return S


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference on hand-worked cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_mean_and_count_by_hand():
    # row 0 at the origin; neighbours at 0.25, 0.5, 0.5 (a tie at the second place) and one at 2 (outside radius 1)
    S = surfels([(0, 0, 0), (0.25, 0, 0), (0, 0.5, 0), (0, 0, -0.5), (2, 0, 0)])
    count, D = oref.neighbours(S, 1.0)
    assert count.tolist() == [3, 3, 3, 3, 0]
    assert D[0, :4].tolist() == [0.0625, 0.25, 0.25, np.inf]
    assert oref.mean_dist(count, D, 1)[0] == F(0.25)
    assert oref.mean_dist(count, D, 2)[0] == F(0.375)                          # (0.25 + 0.5) / 2: the tie's second member is not taken
    assert oref.mean_dist(count, D, 3)[0] == F(F(1.25) / F(3))                 # ((0.25 + 0.5) + 0.5) / 3
    assert oref.mean_dist(count, D, 4)[0] == INF                               # sparse: three neighbours
    # row 1 sees the origin at 0.25 and the two others at sqrt(0.0625 + 0.25)
    assert D[1, :3].tolist() == [0.0625, 0.3125, 0.3125]
    assert oref.mean_dist(count, D, 2)[1] == F((F(0.25) + np.sqrt(F(0.3125))) / F(2))
    assert oref.mean_dist(count, D, 1)[4] == INF and count[4] == 0             # the lone row


def test_a_coincident_pair_are_neighbours_at_zero_and_self_is_excluded_by_row():
    S = surfels([(1, 2, 3), (1, 2, 3), (9, 9, 9)])
    count, D = oref.neighbours(S, 0.5)
    assert count.tolist() == [1, 1, 0] and D[0, 0] == 0 and D[1, 0] == 0
    assert oref.mean_dist(count, D, 1).tolist() == [0.0, 0.0, np.inf]


def test_exactly_k_minus_one_k_and_k_plus_one_neighbours():
    k = 3
    pts = []
    for g, m in enumerate((k - 1, k, k + 1)):                  # a query at x = 10 g with m neighbours at 2^-4 .. : all within radius 1 of it
        pts.append((10.0 * g, 0, 0))
        pts += [(10.0 * g + 2.0 ** -(4 + j), 0, 0) for j in range(m)]
    S = surfels(pts)
    r = oref.outliers(S, radius=0.1, k=k, flag_sparse=1, max_mean_dist=1.0)
    q = [0, k, 2 * k + 1]
    assert r["count"][q].tolist() == [k - 1, k, k + 1]
    assert r["mean"][q[0]] == INF
    want = F(F(F(2.0 ** -6 + 2.0 ** -5) + F(2.0 ** -4)) / F(3))               # the three nearest of the query, nearest first
    assert r["mean"][q[1]] == want
    assert r["mean"][q[2]] == F(F(F(2.0 ** -7 + 2.0 ** -6) + F(2.0 ** -5)) / F(3))
    assert r["result"]["sparse"] == k and r["result"]["measured"] == len(S) - k     # the first group's rows have k - 1 neighbours each
    assert r["rows"].tolist() == [0, 1, 2]                                        # sparse rows are flagged, no mean exceeds 1
    assert oref.outliers(S, radius=0.1, k=k, flag_sparse=0, max_mean_dist=1.0)["rows"].tolist() == []


def test_a_neighbour_at_exactly_the_radius_and_one_float_to_either_side():
    r = F(0.03)
    for x, want in ((sc.step(r, False), 1), (r, 1), (sc.step(r, True), 0)):
        S = surfels([(0, 0, 0), (float(x), 0, 0)])
        assert F(x) * F(x) == np.square(F(x))
        count, _ = oref.neighbours(S, r)
        assert count.tolist() == [want, want], (x, count)


def test_confidence_gates_neighbours_not_the_judged_row():
    S = surfels([(0, 0, 0), (0.01, 0, 0)], conf=[sc.CONF_LOW, sc.CONF_HIGH])
    count, _ = oref.neighbours(S, 0.03, min_conf=10.0)
    assert count.tolist() == [1, 0]                            # the weak row is judged and has the strong one; the strong row has nobody
    assert oref.neighbours(S, 0.03, min_conf=-1.0)[0].tolist() == [1, 1]


def test_radius_mode_and_non_participants():
    S = surfels([(0, 0, 0), (0.01, 0, 0), (0.02, 0, 0), (np.nan, 0, 0), (5, 5, 5)])
    r = oref.outliers(S, mode=oref.RADIUS, radius=0.015, min_neighbors=2)
    assert r["count"].tolist() == [1, 2, 1, 0, 0] and r["rows"].tolist() == [0, 2, 4]
    assert r["result"] == dict(sum=0.0, sum_sq=0.0, participants=4, measured=3, sparse=1, outliers=3, count_after=2, threshold=INF)
    assert oref.outliers(S, mode=oref.RADIUS, radius=0.015, min_neighbors=0)["rows"].tolist() == []
    among = np.array([0, 1, 0, 1, 1], bool)                    # rows 0 and 2 are not selected: not judged, but still neighbours of row 1
    r = oref.outliers(S, among=among, mode=oref.RADIUS, radius=0.015, min_neighbors=3)
    assert r["count"].tolist() == [0, 2, 0, 0, 0] and r["rows"].tolist() == [1, 4] and r["mean"][0] == INF


def test_threshold_by_hand():
    assert oref.threshold(6.0, 14.0, 3, 2.0, 0.0) == F(2.0 + 2.0 * np.sqrt(14.0 / 3 - 4.0))     # means 1, 2, 3
    assert oref.threshold(6.0, 14.0, 3, 0.0, 0.0) == F(2.0)
    assert oref.threshold(6.0, 11.9, 3, 5.0, 0.0) == F(2.0)                                     # a negative variance counts as 0
    assert oref.threshold(0.0, 0.0, 0, 2.0, 0.0) == INF and oref.threshold(6.0, 14.0, 3, 2.0, 0.25) == F(0.25)


def test_the_summation_order_is_the_specified_one():
    P = oref.P
    t = np.zeros(P + 2)
    t[0], t[1], t[P + 1] = 1.0, 2.0 ** -53, 2.0 ** -53
    # lane 1 adds its two terms first (2^-52), the tree's first round adds lanes 0 and 1; a running sum rounds each 2^-53 away
    assert oref.lane_sum(t) == 1.0 + 2.0 ** -52
    run = 0.0
    for v in t:
        run = run + v
    assert run == 1.0
    # the tree pairs neighbours: lanes 0 | 1 and 2 | 3 first
    t = np.zeros(P)
    t[0], t[2], t[3] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert oref.lane_sum(t) == 1.0 + 2.0 ** -52
    assert oref.lane_sum(np.zeros(0)) == 0.0 and oref.lane_sum([3.0]) == 3.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# the scenes of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_stats_scene_contains_every_edge_it_claims():
    S, m = sc.stats_scene()
    r = sc.R_STATS
    assert len(S) == 1025 and len(S) % 64 == 1
    count, D = oref.neighbours(S, r)
    cells = np.floor(S[:, :3] * F(1 / r))
    for rows in m["clump"]:
        assert len(rows) > 16 and (cells[rows] == cells[rows[0]]).all() and (count[rows] >= len(rows) - 1).all()
    assert (D[m["pairs"][:, 0], 0] == 0).all() and (D[m["pairs"][:, 1], 0] == 0).all()
    assert (S[m["pairs"][:, 0], :3] == S[m["pairs"][:, 1], :3]).all() and (m["pairs"][:, 0] != m["pairs"][:, 1]).all()
    lat = S[m["lattice"], :3]
    assert (lat * F(16 / r) == np.round(lat * F(16 / r))).all()               # on exact multiples of radius / 16
    inner = m["lattice"][count[m["lattice"]] >= 16]
    assert len(inner) and (D[inner, 0] == D[inner, 2]).all() and (D[inner, 15] == D[inner, 14]).any()   # ties, also at the 16th place
    assert len(np.unique(np.floor(lat * F(1 / r)), axis=0)) > 1                # across cells
    assert not np.isfinite(S[m["bad"], :3]).all(1).any() and (count[m["bad"]] == 0).all()
    assert count[m["specks"]].tolist() == m["speck_neighbours"].tolist() == list(range(18))
    assert S[m["specks"][3], 3] == sc.CONF_LOW
    assert [count[q] for q, _ in m["rim"]] == [1, 1, 0]
    assert len(m["low"]) > 100
    c10, _ = oref.neighbours(S, r, min_conf=10.0)
    assert (c10 <= count).all() and (c10[m["low"]] > 0).any() and (c10 < count).sum() > 100
    cloud = np.setdiff1d(np.arange(len(S)), np.concatenate([m["bad"], m["lattice"], *m["clump"]]))
    for k in sc.STATS_KS:                                      # measured and sparse rows for every k
        assert 10 < (count[cloud] >= k).sum() < len(cloud) - 10 or k == 1, k


def test_the_sums_scene_makes_every_lane_add_more_than_one_term():
    S = sc.sums_scene()
    assert len(S) == 2 * oref.P + 5
    r = oref.outliers(S, radius=sc.R_SUMS)
    res = r["result"]
    measured = r["part"] & (r["count"] >= 8)
    per_lane = np.array([measured[j::oref.P].sum() for j in range(oref.P)])
    assert (per_lane >= 2).sum() > 3500 and (per_lane[:5] == 3).sum() >= 3 and (per_lane == 0).sum() < 20
    assert res["measured"] > 7000 and 40 <= res["sparse"] < 600 and 50 < res["outliers"] < 2000
    assert 0 < (r["mean"][measured] > res["threshold"]).sum() < res["outliers"]          # both kinds of outlier
    m64 = np.where(measured, r["mean"], 0).astype(np.float64)
    run1 = run2 = 0.0
    for v in m64:
        run1 += v
        run2 += v * v
    assert (run1, run2) != (res["sum"], res["sum_sq"]), "a running sum by row gives the same bits: the order would go unseen"
    # a sparse scene: nothing is measured
    r = oref.outliers(sc.sparse_scene(), radius=sc.R_SUMS)
    assert r["result"]["measured"] == 0 and r["result"]["threshold"] == INF and r["result"]["outliers"] == len(sc.sparse_scene())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C ABI without a context
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    return api.lib()


def good_params(**kw):
    from elasticfusion_amd import api
    p = api.ef_outlier_params(mode=api.OUTLIER_STATISTICAL, radius=0.03, cell=0.03, min_conf=-1.0, min_neighbors=4, k=8, std_ratio=2.0,
                              max_mean_dist=0.0, flag_sparse=1)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD = [(dict(mode=2), "mode"), (dict(mode=-1), "mode"), (dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"),
       (dict(radius=float("nan")), "radius"), (dict(radius=float("inf")), "radius"), (dict(cell=0.0), "cell"), (dict(cell=float("nan")), "cell"),
       (dict(cell=float("inf")), "cell"), (dict(cell=1e-45), "cell"), (dict(radius=0.5, cell=0.03), "radius / cell"), (dict(k=0), "k must"),
       (dict(k=17), "k must"), (dict(min_neighbors=-1), "min_neighbors"), (dict(min_conf=float("nan")), "min_conf"),
       (dict(std_ratio=float("nan")), "std_ratio"), (dict(std_ratio=-0.5), "std_ratio"), (dict(max_mean_dist=-1.0), "max_mean_dist"),
       (dict(max_mean_dist=float("nan")), "max_mean_dist")]


def test_every_refusal_names_its_argument_with_a_null_context(lib):
    from elasticfusion_amd import api
    EINVAL = -1
    res, cnt, rows = api.ef_outlier_result(), C.c_uint32(0), (C.c_uint32 * 4)()
    calls = {
        "ef_map_neighbor_stats": lambda p, a: lib.ef_map_neighbor_stats(None, p, a, None, None, 0),
        "ef_map_neighbor_stats_dev": lambda p, a: lib.ef_map_neighbor_stats_dev(None, p, a, None, None, 0),
        "ef_map_outliers_select": lambda p, a: lib.ef_map_outliers_select(None, p, a, rows, 4, C.byref(cnt), None),
        "ef_map_outliers_select_dev": lambda p, a: lib.ef_map_outliers_select_dev(None, p, a, rows, 4, C.byref(cnt), None),
        "ef_map_remove_outliers": lambda p, a: lib.ef_map_remove_outliers(None, p, a, C.byref(res)),
    }

    def refused(rc, fn, word):
        msg = lib.ef_last_error(None).decode()
        assert rc == EINVAL and msg.startswith(fn + ":") and word in msg, (fn, word, rc, msg)

    for fn, call in calls.items():
        refused(call(None, None), fn, "null params")
        for change, word in BAD:
            refused(call(C.byref(good_params(**change)), None), fn, word)
        refused(call(C.byref(good_params(mode=api.OUTLIER_RADIUS, k=0)), None), fn, "null context")        # k is ignored in RADIUS mode
        refused(call(C.byref(good_params()), None), fn, "null context")                                    # all is well but the context
        sel = api.ef_map_selection()
        lib.ef_default_map_selection(C.byref(sel))
        sel.tests = 0x8000
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "unknown bits")                            # what ef_map_select refuses
        sel.tests, sel.conf_min = api.SEL_CONF, float("nan")
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "NaN")
    p = C.byref(good_params())
    refused(lib.ef_map_outliers_select(None, p, None, None, 4, C.byref(cnt), None), "ef_map_outliers_select", "null rows")
    refused(lib.ef_map_outliers_select_dev(None, p, None, None, 4, C.byref(cnt), None), "ef_map_outliers_select_dev", "null rows")
    refused(lib.ef_map_outliers_select(None, p, None, rows, 4, None, None), "ef_map_outliers_select", "null count")
    refused(lib.ef_map_outliers_select_dev(None, p, None, rows, 4, None, None), "ef_map_outliers_select_dev", "null count")
    refused(lib.ef_map_remove_outliers(None, p, None, None), "ef_map_remove_outliers", "null result")
    refused(lib.ef_map_outliers_select(None, p, None, None, 0, C.byref(cnt), None), "ef_map_outliers_select", "null context")   # NULL rows with max_rows 0 is fine
    assert lib.ef_default_outlier_params(None, C.byref(good_params())) == EINVAL and b"null context" in lib.ef_last_error(None)


def test_the_new_structs_and_constants_are_the_headers():
    from elasticfusion_amd import api
    structs = header_structs()
    assert structs["ef_outlier_params"] == [f for f, _ in api.ef_outlier_params._fields_]
    assert structs["ef_outlier_result"] == [f for f, _ in api.ef_outlier_result._fields_]
    assert C.sizeof(api.ef_outlier_params) == 36 and C.sizeof(api.ef_outlier_result) == 40          # nine 4-byte fields; 2 x 8 + 6 x 4, no padding
    assert api.ef_outlier_result.participants.offset == 16 and api.ef_outlier_result.threshold.offset == 36
    want = defines("OUTLIER_")
    mine = {k: v for k, v in vars(api).items() if k.startswith("OUTLIER_") and isinstance(v, int)}
    assert want == dict(OUTLIER_RADIUS=0, OUTLIER_STATISTICAL=1, OUTLIER_SUM_LANES=4096) and mine == want, (mine, want)
    assert (oref.RADIUS, oref.STATISTICAL, oref.P) == (api.OUTLIER_RADIUS, api.OUTLIER_STATISTICAL, api.OUTLIER_SUM_LANES)
    for name in ("outlierParams", "neighborStats", "outlierSelect", "outlierSelectDevice", "removeOutliers"):
        assert callable(getattr(api.ElasticFusion, name))
    from elasticfusion_amd import accuracy
    assert callable(accuracy.without_outliers)
