"""Smooth regions of the map on the device (ef_map_regions / ef_map_regions_select / ef_map_remove_regions, include/ef_hip.h; kernels in
elasticfusion_amd/csrc/ef_regions.inc).

The operation is restated in numpy from the header alone (tests/regionref.py over tests/normalref.py: brute-force f32 distances and dots and a
sequential union-find).  Every output is an integer or a byte and is compared EXACTLY: labels, sizes, kinds, every field of the result, the four
row lists and the map a removal leaves.  The scenes (tests/regionscenes.py) are hand-built; tests/test_regions_host.py shows on the CPU that
they contain what they claim.  result["status"] == 0 (no loop reached its cap) is part of every comparison of a result.
"""
import ctypes as C

import numpy as np
import pytest

import componentscenes as csc
import regionref as rref
import regionscenes as sc
from queryref import assert_bits_equal
from test_gpu_select import refused

pytestmark = pytest.mark.gpu

F = np.float32
NONE = rref.NONE


def check(ef, name, what, among=None, among_mask=None, among_key=None, **kw):
    """labels, sizes, kinds, the result and all four lists of one parameter set of a scene against the reference; returns the reference's dict"""
    want = sc.ref_of(name, among=among_mask, among_key=among_key, **kw)
    n = len(want["label"])
    label, size, kind, res = ef.regions(among=among, result=True, **kw)
    bad = np.nonzero(label != want["label"])[0]
    assert len(bad) == 0, (what, "label", len(bad), bad[:10], label[bad[:10]], want["label"][bad[:10]])
    assert np.array_equal(kind, want["kind"]), (what, "kind", np.nonzero(kind != want["kind"])[0][:10])
    assert np.array_equal(size, want["size"]), (what, "size", np.nonzero(size != want["size"])[0][:10])
    assert res == rref.result_for(want, rref.REJECTED, n), (what, res, rref.result_for(want, rref.REJECTED, n))
    for which, key in rref.LISTS:
        rows, total, res = ef.regionSelect(among=among, what=which, count=True, result=True, **kw)
        assert total == len(want[key]) and np.array_equal(rows, want[key]), (what, key, total, len(want[key]))
        assert res == rref.result_for(want, which, n), (what, key, res, rref.result_for(want, which, n))
    return want


def context_with(S):
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    return ef


@pytest.fixture(scope="module")
def box():
    S, m = sc.scene("box")
    ef = context_with(S)
    yield dict(ef=ef, S=S, m=m)
    ef.close()


@pytest.fixture(scope="module")
def thresholds():
    S, m = sc.scene("thresholds")
    ef = context_with(S)
    yield dict(ef=ef, S=S, m=m)
    ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_defaults_are_the_headers(box):
    p = box["ef"].regionParams()
    d = rref.DEFAULTS
    for k, _ in type(p)._fields_:
        assert F(getattr(p, k)) == F(d[k] if k != "cell" else d["radius"]), k


def test_the_box_corner_is_three_regions_every_time(box):
    ef, S, m = box["ef"], box["S"], box["m"]
    seen = [ef.regions(result=True) for _ in range(2)]
    other = context_with(S)
    try:
        seen.append(other.regions(result=True))
    finally:
        other.close()
    want = sc.ref_of("box")
    for label, size, kind, res in seen:
        assert np.array_equal(label, want["label"]) and np.array_equal(size, want["size"]) and np.array_equal(kind, want["kind"])
        assert res == rref.result_for(want, rref.REJECTED, len(S)) and res["regions"] == 3 and res["rejected_regions"] == 0 and res["status"] == 0
    check(ef, "box", "box, defaults")
    check(ef, "box", "box, stored normals", normal_source=rref.STORED)
    check(ef, "box", "box, cell = r / 2, bounds", cell=sc.R / 2, min_size=851, max_size=855)
    check(ef, "box", "box, min_conf", min_conf=10.0)
    assert ef.lastCount() == len(S)
    assert_bits_equal(ef.downloadMap(), S, "the calls change nothing")


def test_among_plain_and_inverted(box):
    from elasticfusion_amd import api
    ef, S = box["ef"], box["S"]
    band = sc.box_band(S)
    for tests, key in ((api.SEL_BOX | api.SEL_INVERT, "band out"), (api.SEL_BOX, "band in")):
        sel = ef.mapSelection(tests=tests, **band)
        mask = np.zeros(len(S), bool)
        mask[ef.selectSurfels(sel)] = True
        want = check(ef, "box", f"among {key}", among=sel, among_mask=mask, among_key=key, normal_source=rref.STORED, min_size=20)
        assert want["result"]["regions"] == (4 if key == "band out" else 1) and (want["kind"][~mask] == 0).all()
    check(ef, "box", "among as keywords, estimated", among=dict(tests=api.SEL_BOX | api.SEL_INVERT, **band),
          among_mask=~((S[:, :3] >= F(band["box_min"])) & (S[:, :3] <= F(band["box_max"]))).all(1), among_key="band out")


def test_the_cylinder_and_its_plane():
    S, _ = sc.scene("cylinder")
    ef = context_with(S)
    try:
        want = check(ef, "cylinder", "cylinder")
        assert want["result"]["regions"] == 2
        check(ef, "cylinder", "cylinder, k = 8, cell = 2 r", k=8, cell=2 * sc.R, min_normal_cos=0.9)
    finally:
        ef.close()


@pytest.mark.parametrize("source", (rref.ESTIMATED, rref.STORED), ids=("estimated", "stored"))
def test_the_thin_wall(source):
    S, _ = sc.scene("wall")
    ef = context_with(S)
    try:
        assert check(ef, "wall", "wall, signed", normal_source=source)["result"]["regions"] == 2
        assert check(ef, "wall", "wall, two-sided", normal_source=source, two_sided=1)["result"]["regions"] == 1
    finally:
        ef.close()


@pytest.mark.parametrize("order", ("ascending", "descending", "shuffled"))
def test_a_core_chain_is_labelled_by_its_smallest_core_row(order):
    S, m = sc.scene("chain_" + order)
    ef = context_with(S)
    try:
        label, size, kind, res = ef.regions(result=True)
        assert (label[m["ribbon"]] == sc.N_SPECKS).all() and (label[m["specks"]] == NONE).all() and (size[m["ribbon"]] == len(m["ribbon"])).all()
        assert res["regions"] == 1 and res["status"] == 0
        check(ef, "chain_" + order, f"chain {order}")
    finally:
        ef.close()


def test_patches_that_touch_only_through_borders():
    S, _ = sc.scene("strip")
    ef = context_with(S)
    try:
        want = check(ef, "strip", "strip, stored", normal_source=rref.STORED)
        assert want["result"]["regions"] == 2 and want["result"]["attached"] > 0 and want["result"]["unassigned"] > 0
        off = check(ef, "strip", "strip, stored, no attachment", normal_source=rref.STORED, attach_borders=0)
        assert off["result"]["attached"] == 0 and off["result"]["unassigned"] == want["result"]["borders"]
        check(ef, "strip", "strip, estimated")
        check(ef, "strip", "strip, estimated, a loose cosine", min_normal_cos=0.5)
    finally:
        ef.close()


def test_threshold_edges(thresholds):
    ef, S, m = thresholds["ef"], thresholds["S"], thresholds["m"]
    kw = sc.THRESHOLD_KW
    s, t = m["dot_pair"]
    c = float((S[s, 8] * S[t, 8] + S[s, 9] * S[t, 9]) + S[s, 10] * S[t, 10])       # (a Python float that is the f32 value)
    at = check(ef, "thresholds", "min_normal_cos = the pair's dot", min_normal_cos=c, **kw)
    up = check(ef, "thresholds", "one float above", min_normal_cos=float(sc.step(c, True)), **kw)
    assert at["label"][s] == at["label"][t] and up["label"][s] != up["label"][t]
    check(ef, "thresholds", "min_normal_cos 0: a zero normal joins, a NaN never", min_normal_cos=0.0, **kw)
    check(ef, "thresholds", "two-sided, cell = r / 16", **dict(kw, cell=sc.R_EXACT / 16, two_sided=1, min_normal_cos=c))
    check(ef, "thresholds", "estimated normals", **dict(kw, normal_source=rref.ESTIMATED))
    assert_bits_equal(ef.downloadMap(), S, "the calls change nothing")


def test_max_curvature_at_a_rows_own_curvature(box):
    ef = box["ef"]
    ref = sc.ref_of("box")
    cv = ref["est"]["curvature"]
    x = int(np.nonzero((ref["kind"] == rref.KIND_CORE) & (cv > 0.01))[0][0])
    assert check(ef, "box", "max_curvature = the row's", max_curvature=float(cv[x]))["kind"][x] == rref.KIND_CORE
    assert check(ef, "box", "one float below", max_curvature=float(sc.step(cv[x], False)))["kind"][x] == rref.KIND_BORDER


@pytest.mark.parametrize("cell", (csc.R_EDGE, csc.R_EDGE / 16), ids=("cell=r", "cell=r/16"))
def test_the_components_edge_scene(cell):
    S, m = sc.scene("edge")
    ef = context_with(S)
    try:
        thr = float(ef.getConfidenceThreshold())
        assert sc.CONF_LOW < thr < sc.CONF_HIGH
        want = check(ef, "edge", f"edge scene, cell {cell}", radius=csc.R_EDGE, cell=cell, **sc.EDGE_KW)
        assert (want["kind"][m["bad"]] == 0).all() and want["result"]["regions"] > 10
        check(ef, "edge", "edge scene, min_conf", radius=csc.R_EDGE, cell=cell, min_conf=thr, **sc.EDGE_KW)
        check(ef, "edge", "edge scene, a tight cosine and curvature", radius=csc.R_EDGE, cell=cell, **dict(sc.EDGE_KW, max_curvature=0.1, min_normal_cos=0.8, two_sided=0))
        assert_bits_equal(ef.downloadMap(), S, "the calls change nothing")
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# lists, the device tier
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_list_conventions(box):
    from elasticfusion_amd import api
    ef = box["ef"]
    full, total = ef.regionSelect(what=rref.BORDERS, count=True)
    assert total == len(full) > 20 and (np.diff(full.astype(np.int64)) > 0).all()
    none, t0 = ef.regionSelect(what=rref.BORDERS, max_rows=0, count=True)                   # NULL rows with max_rows 0
    assert len(none) == 0 and t0 == total
    prm = ef.regionParams()
    rows = np.full(16, 0xABCD1234, np.uint32)
    cnt = C.c_uint32(0)
    api._chk(api.lib().ef_map_regions_select(ef.h, C.byref(prm), None, rref.BORDERS, api._ptr(rows), 7, C.byref(cnt), None), ef.h)
    assert cnt.value == total and np.array_equal(rows[:7], full[:7]) and (rows[7:] == 0xABCD1234).all()
    n = ef.lastCount()
    lab = np.full(n + 3, 0x5A5A5A5A, np.uint32)                                           # min(max_rows, map count) entries
    knd = np.full(n + 3, 0x5A, np.uint8)
    api._chk(api.lib().ef_map_regions(ef.h, C.byref(prm), None, api._ptr(lab), None, api._ptr(knd), 100, None), ef.h)
    assert (lab[100:] == 0x5A5A5A5A).all() and (lab[:100] != 0x5A5A5A5A).all() and (knd[100:] == 0x5A).all() and (knd[:100] <= 2).all()
    api._chk(api.lib().ef_map_regions(ef.h, C.byref(prm), None, api._ptr(lab), None, None, len(lab), None), ef.h)
    assert (lab[n:] == 0x5A5A5A5A).all() and np.array_equal(lab[:n], ef.regions(prm)[0])
    api._chk(api.lib().ef_map_regions(ef.h, C.byref(prm), None, None, None, None, 0, None), ef.h)      # nothing asked for


def test_device_variants_equal_the_host_variants(box):
    from elasticfusion_amd import api
    ef = box["ef"]
    n = ef.lastCount()
    nres = C.sizeof(api.ef_region_result)
    for kw in (dict(), dict(normal_source=rref.STORED, cell=sc.R / 2, min_size=851, max_size=855)):
        prm = ef.regionParams(**kw)
        label, size, kind, res = ef.regions(prm, result=True)
        for what, _ in rref.LISTS:
            rows, total, rres = ef.regionSelect(prm, what=what, count=True, result=True)
            d_rows, d_cnt, d_res = api.DevBuf(n * 4, fill=0xEE), api.DevBuf(16), api.DevBuf(nres)
            ef.regionSelectDevice(prm, None, what, d_rows.p, n, d_cnt.p, d_res.p)
            ef.synchronize()
            assert int(d_cnt.to_array(np.uint32, 1)[0]) == total
            got = d_rows.to_array(np.uint32, n)
            assert np.array_equal(got[:total], rows) and (got[total:] == 0xEEEEEEEE).all()
            raw = d_res.to_array(np.uint8, nres).tobytes()
            assert ef._regionResult(api.ef_region_result.from_buffer_copy(raw)) == rres and rres["listed"] == total and rres["status"] == 0
            ef.regionSelectDevice(prm, None, what, None, 0, d_cnt.p)                        # no list, no result
            ef.synchronize()
            assert int(d_cnt.to_array(np.uint32, 1)[0]) == total
        d_label, d_size, d_kind, d_res = api.DevBuf((n + 2) * 4, fill=0xEE), api.DevBuf((n + 2) * 4, fill=0xEE), api.DevBuf(n + 2, fill=0xEE), api.DevBuf(nres)
        ef.regionsDevice(prm, None, d_label.p, d_size.p, d_kind.p, n + 2, d_res.p)
        ef.synchronize()
        gl, gs, gk = d_label.to_array(np.uint32, n + 2), d_size.to_array(np.uint32, n + 2), d_kind.to_array(np.uint8, n + 2)
        assert np.array_equal(gl[:n], label) and np.array_equal(gs[:n], size) and np.array_equal(gk[:n], kind)
        assert (gl[n:] == 0xEEEEEEEE).all() and (gs[n:] == 0xEEEEEEEE).all() and (gk[n:] == 0xEE).all()
        raw = d_res.to_array(np.uint8, nres).tobytes()
        assert ef._regionResult(api.ef_region_result.from_buffer_copy(raw)) == res and res["status"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# removal, refusals, end to end
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,kw", ((rref.REJECTED, dict(min_size=851, max_size=855)), (rref.BORDERS, dict())), ids=("rejected", "borders"))
def test_removal_equals_erasing_the_list(what, kw):
    S, _ = sc.scene("box")
    a, b = context_with(S), context_with(S)
    try:
        n = len(S)
        rows, total, res = a.regionSelect(what=what, count=True, result=True, **kw)
        want = sc.ref_of("box", **kw)
        assert np.array_equal(rows, want[dict(rref.LISTS)[what]]) and 0 < total < n and res["status"] == 0
        got = a.removeRegions(what=what, **kw)
        assert b.eraseRows(rows) == total
        assert got == dict(res, listed=total, count_after=n - total) and a.lastCount() == b.lastCount() == n - total, (got, res)
        assert_bits_equal(a.downloadMap(), b.downloadMap(), "the map after the removal")
        keep = np.ones(n, bool)
        keep[rows] = False
        assert_bits_equal(a.downloadMap(), S[keep], "the rows that stay, in order")
        assert a.getTick() == b.getTick()
        # the next call sees the map that is left (the index is rebuilt): what the reference makes of it
        after = rref.regions(S[keep], **kw)
        label, size, kind = a.regions(**kw)
        assert np.array_equal(label, after["label"]) and np.array_equal(size, after["size"]) and np.array_equal(kind, after["kind"])
    finally:
        a.close()
        b.close()


def test_a_loop_closing_context_refuses_the_removal_only():
    from elasticfusion_amd import api
    S, _ = sc.scene("wall")
    ef = api.ElasticFusion(closeLoops=True)
    try:
        ef.uploadMap(S)
        assert "close_loops" in refused(lambda: ef.removeRegions(what=rref.ACCEPTED), -4)                      # EF_ESTATE
        assert ef.lastCount() == len(S)
        assert_bits_equal(ef.downloadMap(), S, "a refused removal")
        check(ef, "wall", "on a loop-closing context")
        refused(lambda: ef.regionSelect(what=4), -1)                                                         # EF_EINVAL
        refused(lambda: ef.removeRegions(what=-1), -1)
        refused(lambda: ef.regions(normal_source=2), -1)
        refused(lambda: ef.regions(min_normal_cos=float("nan")), -1)
        refused(lambda: ef.regions(radius=1.0, cell=0.01), -1)
    finally:
        ef.close()


def test_smooth_regions_gathers_the_three_faces(box):
    from elasticfusion_amd import accuracy
    ef, S = box["ef"], box["S"]
    want = sc.ref_of("box")
    regs = sorted(rref.region_rows(want).items(), key=lambda kv: (-len(kv[1]), kv[0]))
    got = accuracy.smooth_regions(ef)
    assert len(got) == len(regs) == 3
    for g, (_, rows) in zip(got, regs):
        assert_bits_equal(g, S[rows], "a region's rows, ascending")
    assert len(accuracy.smooth_regions(ef, max_regions=1)) == 1 and len(accuracy.smooth_regions(ef, min_size=len(regs[0][1]) + 1)) == 0
    assert ef.lastCount() == len(S)
