"""Plane segmentation of the map on the device (ef_map_planes / ef_map_planes_select / ef_map_remove_planes, include/ef_hip.h; kernels in
elasticfusion_amd/csrc/ef_planes.inc).

The operation is restated in numpy from the header alone (tests/planeref.py).  Every comparison with it is EXACT: the labels, every integer
of the models and the result, the row lists, the maps a removal leaves, and the BITS of normal, d and thickness.  The scenes
(tests/planescenes.py) are hand-built; tests/test_plane_host.py shows on the CPU that they contain every edge they claim.
"""
import ctypes as C

import numpy as np
import pytest

import planeref as pr
import planescenes as sc
from queryref import assert_bits_equal
from test_gpu_select import refused, state_of

pytestmark = pytest.mark.gpu

F = np.float32
NONE = pr.NONE


def check(ef, S, what, among=None, among_mask=None, lists=True, **kw):
    """labels, models, the result and (lists) both lists for every `which` of one parameter set against the reference; returns the reference"""
    want = pr.planes(S, among=among_mask, **kw)
    label, models, res = ef.planes(among=among, result=True, **kw)
    bad = np.nonzero(label != want["label"])[0]
    assert len(bad) == 0, (what, "label", bad[:10], label[bad[:10]], want["label"][bad[:10]])
    assert len(models) == len(want["models"]), (what, len(models), len(want["models"]))
    for k, (g, w) in enumerate(zip(models, want["models"])):
        assert pr.same_model(g, w), (what, "model", k, g, w)
    assert res == dict(want["result"], count_after=pr.lists(want, -1)[2]), (what, res, want["result"])
    if lists:
        max_planes = kw.get("max_planes", pr.DEFAULTS["max_planes"])
        for which in range(-1, max_planes):
            on, off, after = pr.lists(want, which)
            for w, rows_want in ((pr.ON, on), (pr.OFF, off)):
                rows, total, mods, r = ef.planeSelect(among=among, what=w, which=which, count=True, models=True, result=True, **kw)
                assert total == len(rows_want) and np.array_equal(rows, rows_want), (what, which, w, total, len(rows_want))
                assert r == dict(want["result"], count_after=after), (what, which, w, r)
                assert len(mods) == len(models) and all(pr.same_model(g, m) for g, m in zip(mods, models))
    return want


def context_with(S):
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    if len(S):
        ef.uploadMap(S)
    return ef


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1: the base scene
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    S, part = sc.base()
    ef = context_with(S)
    yield dict(ef=ef, S=S, part=part)
    ef.close()


@pytest.mark.parametrize("H", (1, 65, 256, 300))
@pytest.mark.parametrize("refine", (0, 1))
@pytest.mark.parametrize("normal_cos", (0.0, 0.9))
def test_the_base_scene_equals_the_reference_exactly(base, H, refine, normal_cos):
    ef, S = base["ef"], base["S"]
    kw = dict(sc.BASE, hypotheses=H, refine=refine, normal_cos=normal_cos)
    if H == 1:
        kw["min_inliers"] = 1          # a single hypothesis finds a few dozen rows (none with the normal test): a "plane" per round, or none
    want = check(ef, S, f"base H={H} refine={refine} cos={normal_cos}", lists=(H == 256), **kw)
    assert want["result"]["planes"] == (3 if H > 1 else 0 if normal_cos else 5)
    assert ef.lastCount() == len(S)
    assert_bits_equal(ef.downloadMap(), S, "the calls change nothing")


def test_max_planes_stops_early_and_min_inliers_ends(base):
    ef, S = base["ef"], base["S"]
    two = check(ef, S, "max_planes 2", **dict(sc.BASE, max_planes=2))
    five = check(ef, S, "max_planes 5", **sc.BASE)
    assert two["result"]["planes"] == 2 and five["result"]["planes"] == 3 and five["rounds"][3]["best"] < sc.BASE["min_inliers"]
    one = check(ef, S, "max_planes 1, min_inliers above the floor", **dict(sc.BASE, max_planes=1, min_inliers=1501))
    assert one["result"] == dict(nodes=len(S), planes=0, on_rows=0, off_rows=len(S))


def test_axis_modes(base):
    from elasticfusion_amd import api
    ef, S = base["ef"], base["S"]
    floor = check(ef, S, "floor only", **dict(sc.BASE, axis_mode=api.PLANE_AXIS_NORMAL, axis=(0.0, 0.0, 1.0), axis_bound=0.95))
    assert floor["result"]["planes"] == 1 and floor["models"][0]["normal"][2] > 0.99                     # oriented along +z: t >= 0
    down = check(ef, S, "floor only, the axis down", **dict(sc.BASE, axis_mode=api.PLANE_AXIS_NORMAL, axis=(0.0, 0.0, -1.0), axis_bound=0.95))
    assert down["models"][0]["normal"][2] < -0.99 and np.array_equal(down["label"], floor["label"])
    walls = check(ef, S, "walls only", **dict(sc.BASE, refine=0, axis_mode=api.PLANE_AXIS_INPLANE, axis=(0.0, 0.0, 1.0), axis_bound=0.1))
    assert walls["result"]["planes"] == 1 and abs(walls["models"][0]["normal"][0]) > 0.99 and walls["models"][0]["normal"][2] >= 0
    skew = check(ef, S, "an axis that is not exactly unit", **dict(sc.BASE, axis_mode=api.PLANE_AXIS_NORMAL, axis=(0.6, 0.0, 0.8), axis_bound=0.7))
    assert skew["result"]["planes"] >= 1


def test_a_second_run_on_a_fresh_context_is_bit_identical(base):
    S = base["S"]
    first = base["ef"].planes(result=True, **sc.BASE)
    ef = context_with(S)
    try:
        second = ef.planes(result=True, **sc.BASE)
        third = ef.planes(result=True, **sc.BASE)
    finally:
        ef.close()
    for other in (second, third):
        assert np.array_equal(first[0], other[0]) and first[2] == other[2] and len(first[1]) == len(other[1]) == 3
        assert all(pr.same_model(a, b) for a, b in zip(first[1], other[1]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2: sizes, degenerate and empty inputs, ties, thresholds
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_m_on_the_scoring_chunk_edges():
    S, part = sc.chunks()
    ef = context_with(S)
    try:
        want = check(ef, S, "chunk scene", seed=1, hypotheses=128, min_inliers=500, max_planes=4)
        assert [x["M"] for x in want["rounds"]] == [2 * sc.CHUNK + 1, sc.CHUNK, 1024] and want["result"]["planes"] == 2
        check(ef, S, "chunk scene, normals", lists=False, seed=1, hypotheses=128, min_inliers=500, max_planes=4, normal_cos=0.9)
    finally:
        ef.close()


@pytest.mark.parametrize("m", (0, 1, 2, 3))
def test_fewer_participants_than_a_plane_needs(m):
    S = sc.few(m)
    ef = context_with(S)
    try:
        want = check(ef, S, f"M = {m}", seed=1, hypotheses=32, min_inliers=1, max_planes=2)
        assert want["result"]["nodes"] == m and want["result"]["planes"] == (1 if m == 3 else 0)
    finally:
        ef.close()


@pytest.mark.parametrize("scene", ("coincident", "collinear", "empty"))
def test_no_valid_hypothesis_yields_no_plane(scene):
    S = sc.of(np.zeros((0, 3))) if scene == "empty" else getattr(sc, scene)()
    ef = context_with(S)
    try:
        want = check(ef, S, scene, seed=1, hypotheses=64, min_inliers=1, max_planes=2)
        assert want["result"] == dict(nodes=len(S), planes=0, on_rows=0, off_rows=len(S))
        if len(S):
            assert ef.removePlanes(seed=1, hypotheses=64, min_inliers=1, max_planes=2) == dict(want["result"], count_after=len(S))
    finally:
        ef.close()


def test_ties_go_to_the_lowest_hypothesis():
    S = sc.twins()
    ef = context_with(S)
    try:
        want = check(ef, S, "twins", seed=2, hypotheses=64, min_inliers=100, max_planes=2, refine=0)
        c = want["rounds"][0]["counts"]
        top = np.nonzero(c == c.max())[0]
        assert len(top) > 2 and want["models"][0]["hypothesis"] == top[0] > 0
        check(ef, S, "twins, refined", seed=2, hypotheses=64, min_inliers=100, max_planes=2, refine=1)
    finally:
        ef.close()


def test_threshold_edges():
    S, m = sc.thresholds()
    ef = context_with(S)
    try:
        for nc in (0.0, sc.NORMAL_COS):
            kw = dict(seed=2, hypotheses=64, min_inliers=100, max_planes=1, refine=0, normal_cos=nc)
            check(ef, S, f"thresholds cos={nc}", **kw)
            lab = ef.planes(**kw)[0]
            assert lab[m["at"]] == lab[m["below_at"]] == 0 and lab[m["beyond"]] == lab[m["below_beyond"]] == NONE
            assert lab[m["cos_at"]] == 0 and lab[m["cos_below"]] == (NONE if nc else 0)
    finally:
        ef.close()


def test_rows_that_are_no_participants_change_nothing():
    from elasticfusion_amd import api
    S, m = sc.outsiders()
    ef = context_with(S)
    try:
        thr = float(ef.getConfidenceThreshold())
        assert sc.CONF_LOW < thr < sc.CONF_HIGH
        kw = dict(seed=2, hypotheses=64, min_inliers=100, max_planes=2)
        every = check(ef, S, "every finite row", **kw)
        conf = check(ef, S, "min_conf", min_conf=thr, **kw)
        assert every["result"]["nodes"] == len(S) - len(m["bad"]) and conf["result"]["nodes"] == every["result"]["nodes"] - len(m["low"])
        assert (conf["label"][np.concatenate([m["bad"], m["low"]])] == NONE).all() and (every["label"][m["bad"]] == NONE).all()
        box = dict(box_min=m["box_min"], box_max=m["box_max"])
        inside = ((S[:, :3] >= F(box["box_min"])) & (S[:, :3] <= F(box["box_max"]))).all(1)
        out = check(ef, S, "among the inverted box", among=dict(tests=api.SEL_BOX | api.SEL_INVERT, **box), among_mask=~inside, min_conf=thr, **kw)
        assert (out["label"][m["boxed"]] == NONE).all() and out["result"]["nodes"] == conf["result"]["nodes"] - len(m["boxed"])
        # the rows outside take no part: without them the rest gives the same models and, row for row, the same labels
        keep = np.nonzero(out["node"])[0]
        alone = pr.planes(S[keep], **kw)
        assert np.array_equal(alone["label"], out["label"][keep]) and all(pr.same_model(a, b) for a, b in zip(alone["models"], out["models"]))
        only = check(ef, S, "among the box", among=dict(tests=api.SEL_BOX, **box), among_mask=inside, seed=2, hypotheses=64, min_inliers=10, max_planes=1)
        assert only["result"]["nodes"] == len(m["boxed"]) and set(np.nonzero(only["label"] == 0)[0]) <= set(m["boxed"])
        assert_bits_equal(ef.downloadMap(), S, "the calls change nothing")
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3: lists, device variants, removal
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_list_conventions(base):
    from elasticfusion_amd import api
    ef = base["ef"]
    full, total = ef.planeSelect(count=True, **sc.BASE)
    assert total == len(full) > 2000 and (np.diff(full.astype(np.int64)) > 0).all()
    none, t0 = ef.planeSelect(max_rows=0, count=True, **sc.BASE)                       # NULL rows with max_rows 0
    assert len(none) == 0 and t0 == total
    some, t1 = ef.planeSelect(max_rows=100, count=True, **sc.BASE)
    assert t1 == total and np.array_equal(some, full[:100])
    prm = ef.planeParams(**sc.BASE)
    rows = np.full(16, 0xABCD1234, np.uint32)
    cnt = C.c_uint32(0)
    api._chk(api.lib().ef_map_planes_select(ef.h, C.byref(prm), None, pr.ON, -1, api._ptr(rows), 7, C.byref(cnt), None, None), ef.h)
    assert cnt.value == total and np.array_equal(rows[:7], full[:7]) and (rows[7:] == 0xABCD1234).all()
    n = ef.lastCount()
    lab = np.full(n + 3, 0x5A5A5A5A, np.uint32)                                      # the labels: min(max_rows, map count) entries
    api._chk(api.lib().ef_map_planes(ef.h, C.byref(prm), None, api._ptr(lab), 100, None, None), ef.h)
    assert (lab[100:] == 0x5A5A5A5A).all() and (lab[:100] != 0x5A5A5A5A).all()
    api._chk(api.lib().ef_map_planes(ef.h, C.byref(prm), None, api._ptr(lab), len(lab), None, None), ef.h)
    assert (lab[n:] == 0x5A5A5A5A).all() and np.array_equal(lab[:n], ef.planes(prm)[0])
    api._chk(api.lib().ef_map_planes(ef.h, C.byref(prm), None, None, 0, None, None), ef.h)                # nothing asked for
    # the models: max_planes entries, zero bytes from result.planes on; the entries past max_planes are left as they were
    mods = (api.ef_plane_model * api.PLANE_MAX_PLANES)()
    C.memset(mods, 0x5A, C.sizeof(mods))
    res = api.ef_plane_result()
    api._chk(api.lib().ef_map_planes(ef.h, C.byref(prm), None, None, 0, mods, C.byref(res)), ef.h)
    raw = np.frombuffer(bytes(mods), np.uint8).reshape(api.PLANE_MAX_PLANES, -1)
    assert res.planes == 3 and prm.max_planes == 5 and (raw[3:5] == 0).all() and (raw[5:] == 0x5A).all() and mods[0].inliers == 1500


def test_device_variants_equal_the_host_variants(base):
    from elasticfusion_amd import api
    ef = base["ef"]
    n = ef.lastCount()
    nres, nmod = C.sizeof(api.ef_plane_result), C.sizeof(api.ef_plane_model)
    for kw in (sc.BASE, dict(sc.BASE, refine=0, normal_cos=0.9, max_planes=2)):
        prm = ef.planeParams(**kw)
        label, models, res = ef.planes(prm, result=True)

        def models_of(buf):
            arr = (api.ef_plane_model * api.PLANE_MAX_PLANES).from_buffer_copy(buf.to_array(np.uint8, nmod * api.PLANE_MAX_PLANES).tobytes())
            return arr

        for what in (pr.ON, pr.OFF):
            for which in (-1, 1):
                rows, total, r = ef.planeSelect(prm, what=what, which=which, count=True, result=True)
                d_rows, d_cnt, d_res, d_mod = api.DevBuf(n * 4, fill=0xEE), api.DevBuf(16), api.DevBuf(nres), api.DevBuf(nmod * api.PLANE_MAX_PLANES, fill=0xEE)
                ef.planeSelectDevice(prm, None, what, which, d_rows.p, n, d_cnt.p, d_mod.p, d_res.p)
                ef.synchronize()
                assert int(d_cnt.to_array(np.uint32, 1)[0]) == total
                got = d_rows.to_array(np.uint32, n)
                assert np.array_equal(got[:total], rows) and (got[total:] == 0xEEEEEEEE).all()
                assert ef._planeResult(api.ef_plane_result.from_buffer_copy(d_res.to_array(np.uint8, nres).tobytes())) == r
                arr = models_of(d_mod)
                assert all(pr.same_model(g, m) for g, m in zip(ef._planeModels(arr, len(models)), models))
                raw = np.frombuffer(bytes(arr), np.uint8).reshape(api.PLANE_MAX_PLANES, -1)
                assert (raw[len(models):prm.max_planes] == 0).all() and (raw[prm.max_planes:] == 0xEE).all()
                ef.planeSelectDevice(prm, None, what, which, None, 0, d_cnt.p)                # no list, no models, no result
                ef.synchronize()
                assert int(d_cnt.to_array(np.uint32, 1)[0]) == total
        d_label, d_res, d_mod = api.DevBuf((n + 2) * 4, fill=0xEE), api.DevBuf(nres), api.DevBuf(nmod * api.PLANE_MAX_PLANES)
        ef.planesDevice(prm, None, d_label.p, n + 2, d_mod.p, d_res.p)
        ef.synchronize()
        gl = d_label.to_array(np.uint32, n + 2)
        assert np.array_equal(gl[:n], label) and (gl[n:] == 0xEEEEEEEE).all()
        assert ef._planeResult(api.ef_plane_result.from_buffer_copy(d_res.to_array(np.uint8, nres).tobytes())) == res
        assert all(pr.same_model(g, m) for g, m in zip(ef._planeModels(models_of(d_mod), len(models)), models))


@pytest.mark.parametrize("which", (-1, 0, 1, 4))
def test_removal_equals_erasing_the_list_on_the_base_scene(base, which):
    S = base["S"]
    a, b = context_with(S), context_with(S)
    try:
        want = pr.planes(S, **sc.BASE)
        on, off, after = pr.lists(want, which)
        rows, res = a.planeSelect(which=which, result=True, **sc.BASE)
        assert np.array_equal(rows, on) and res["count_after"] == after
        got, models = a.removePlanes(which=which, models=True, **sc.BASE)
        assert b.eraseRows(rows) == len(on)
        assert got == res and all(pr.same_model(g, m) for g, m in zip(models, want["models"])) and len(models) == 3
        assert a.lastCount() == b.lastCount() == after
        keep = np.ones(len(S), bool)
        keep[on] = False
        assert_bits_equal(a.downloadMap(), S[keep], "the removal leaves the other rows in their order")
        assert_bits_equal(a.downloadMap(), b.downloadMap(), "the removal equals the erase of the list")
    finally:
        a.close()
        b.close()


def test_removal_equals_erasing_the_list_in_a_running_context(frames):
    from elasticfusion_amd import api
    a, b = api.ElasticFusion(), api.ElasticFusion()
    try:
        for ef in (a, b):
            ef.setSurfelIds(True)
            ef.enableLabels(3)
            for k in range(3):
                ef.processFrame(frames[k][0], frames[k][1], k)
        n = a.lastCount()
        kw = dict(distance=0.02, hypotheses=128, min_inliers=1000, max_planes=2, seed=1)
        rows, total, res = a.planeSelect(count=True, result=True, **kw)
        print("surfels", n, "on planes", total, res)
        assert 0 < total < n and res["planes"] >= 1, (total, n, res)
        before = a.downloadMap()
        want = pr.planes(before, **kw)                      # 150 scoring chunks per round: the reference once more, on a real map
        assert np.array_equal(rows, pr.lists(want, -1)[0]) and res == dict(want["result"], count_after=n - total)
        got = a.removePlanes(**kw)
        assert b.eraseRows(rows) == total
        assert got == dict(res, count_after=n - total) and a.lastCount() == b.lastCount() == n - total, (got, res)
        (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
        assert_bits_equal(ma, mb, "the map after the removal")
        assert len(before) == n and a.getTick() == b.getTick()
        assert np.array_equal(a.surfelIds(), b.surfelIds())
        (ia, pa), (ib, pb) = a.labels(), b.labels()
        assert np.array_equal(ia, ib)
        assert_bits_equal(pa, pb, "the labels after the removal")
        for ef in (a, b):
            ef.processFrame(frames[3][0], frames[3][1], 3)
        (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
        assert np.array_equal(qa.view(np.uint64), qb.view(np.uint64)) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
        assert_bits_equal(ma, mb, "the map after the following frame")
    finally:
        a.close()
        b.close()


def test_a_loop_closing_context_refuses_the_removal_only(base):
    from elasticfusion_amd import api
    S = base["S"]
    ef = api.ElasticFusion(closeLoops=True)
    try:
        ef.uploadMap(S)
        assert "close_loops" in refused(lambda: ef.removePlanes(**sc.BASE), -4)                                  # EF_ESTATE
        assert ef.lastCount() == len(S)
        assert_bits_equal(ef.downloadMap(), S, "a refused removal")
        check(ef, S, "on a loop-closing context", lists=False, **sc.BASE)
        refused(lambda: ef.planeSelect(what=2), -1)                                                              # EF_EINVAL
        refused(lambda: ef.planeSelect(which=4), -1)                                                             # the default max_planes is 4
        refused(lambda: ef.planes(distance=float("nan")), -1)
        refused(lambda: ef.planes(axis_mode=api.PLANE_AXIS_NORMAL, axis=(0.0, 0.0, 2.0)), -1)
    finally:
        ef.close()


def test_plane_segments_and_without_planes(base):
    from elasticfusion_amd import accuracy
    ef, S = base["ef"], base["S"]
    want = pr.planes(S, **sc.BASE)
    segs = accuracy.plane_segments(ef, **sc.BASE)
    assert len(segs) == 3
    for k, (model, surfels) in enumerate(segs):
        assert pr.same_model(model, want["models"][k])
        assert_bits_equal(surfels, S[want["label"] == k], f"the surfels of plane {k}")
    assert_bits_equal(accuracy.without_planes(ef, **sc.BASE), S[want["node"] & (want["label"] == NONE)], "the rows on no plane")
    assert ef.lastCount() == len(S)
    assert_bits_equal(ef.downloadMap(), S, "the calls change nothing")
