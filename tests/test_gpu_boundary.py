"""Find the map's boundaries on the device (ef_map_boundaries / ef_map_boundaries_select, include/ef_hip.h; kernels in
elasticfusion_amd/csrc/ef_boundary.inc).

The operation is restated in numpy and Python floats from the header alone (tests/boundaryref.py).  The header fixes every rounding and every
order, so everything is compared BIT FOR BIT: gaps, counts, status, loop labels and sizes, the row lists and the results.  The scenes
(tests/boundaryscenes.py) are hand-built; tests/test_boundary_host.py shows on the CPU that they contain every edge they claim, and that the
plate's verdicts follow from geometry alone (plate_expectation), which the device is held to as well.
"""
import ctypes as C
import ctypes.util
import os

import numpy as np
import pytest

import boundaryref as br
import boundaryscenes as bs
import normalref as nr
from queryref import assert_bits_equal
from test_boundary_host import plate_expectation
from test_gpu_select import refused

pytestmark = pytest.mark.gpu

F = np.float32
WHATS = (br.INTERIOR, br.BOUNDARY, br.SPARSE, br.DEGENERATE, br.LOOPS_ACCEPTED, br.LOOPS_REJECTED)


def check_rows(got, want, what):
    for key in ("status", "count", "label", "size"):
        assert np.array_equal(got[key], want[key]), (what, key, np.nonzero(got[key] != want[key])[0][:10])
    assert_bits_equal(got["gap"], want["gap"], f"gap: {what}")


def check_result(got, want, listed, what):
    assert got == dict(want, listed=listed), (what, got, want, listed)


def unchanged(ef, S, probe):
    """the map, its count and a later query are what they were"""
    assert ef.lastCount() == len(S)
    assert_bits_equal(ef.downloadMap(), S, "the call changes nothing")
    pts, want = probe
    got = ef.queryNearestRaw(pts, 0.05)
    for a, b in zip(got, want):
        assert_bits_equal(a, b, "a later queryNearest")


@pytest.fixture(scope="module")
def edge():
    from elasticfusion_amd import api
    S, marks = bs.edge_scene()
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    thr = float(ef.getConfidenceThreshold())
    assert bs.CONF_LOW < thr < bs.CONF_HIGH
    nl = {mc: nr.neighbour_lists(S, bs.R_EDGE, mc) for mc in (-1.0, thr)}
    pts = S[::7, :3] + F(0.001)
    pts = pts[np.isfinite(pts).all(1)]
    probe = (pts, ef.queryNearestRaw(pts, 0.05))
    yield dict(ef=ef, S=S, marks=marks, thr=thr, nl=nl, probe=probe)
    ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# per-row verdicts and loops
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable_only", (False, True))
@pytest.mark.parametrize("cell", (bs.R_EDGE, bs.R_EDGE / 16))
def test_the_edge_scene_equals_the_reference_exactly(edge, cell, stable_only):
    ef, S, m = edge["ef"], edge["S"], edge["marks"]
    mc = edge["thr"] if stable_only else -1.0
    seen = set()
    for k in bs.KS:
        for src in (br.STORED, br.ESTIMATED):
            kw = dict(radius=bs.R_EDGE, min_conf=mc, k=k, min_neighbors=bs.MIN_NEIGHBORS, normal_source=src)
            want = br.boundaries(S, nl=edge["nl"][mc], **kw)
            got, res = ef.boundaries(cell=cell, result=True, **kw)
            check_rows(got, want, f"k={k} cell={cell} min_conf={mc} source={src}")
            check_result(res, want["result"], 0, f"k={k} cell={cell} min_conf={mc} source={src}")
            assert res["status"] == 0
            seen |= set(np.unique(want["status"]).tolist())
    assert seen == {br.NONE, br.INTERIOR, br.BOUNDARY, br.SPARSE, br.DEGENERATE}
    unchanged(ef, S, edge["probe"])


def test_the_marked_rows_on_the_device(edge):
    ef, m = edge["ef"], edge["marks"]
    got = ef.boundaries(radius=bs.R_EDGE, cell=bs.R_EDGE, k=8, min_neighbors=bs.MIN_NEIGHBORS)
    st, gap = got["status"], got["gap"]
    assert st[m["nan_pos"]] == br.NONE and st[m["sparse"]] == br.SPARSE
    assert [int(st[m[g]]) for g in ("zero_normal", "nan_normal", "along")] == [br.DEGENERATE] * 3
    assert [float(gap[m[g]]) for g in ("one_dir", "opposite", "coincident", "cross", "long_normal", "low_boundary", "low_neighbour")] == [4, 2, 3, 1, 1, 4, 1]
    two = ef.boundaries(radius=bs.R_EDGE, cell=bs.R_EDGE, k=8, min_neighbors=bs.MIN_NEIGHBORS, max_gap=2.0)
    assert two["status"][m["opposite"]] == br.INTERIOR and two["status"][m["one_dir"]] == br.BOUNDARY          # the test is >
    low = ef.boundaries(radius=bs.R_EDGE, cell=bs.R_EDGE, k=8, min_neighbors=bs.MIN_NEIGHBORS, min_conf=edge["thr"])
    assert low["status"][m["low_boundary"]] == br.BOUNDARY and low["label"][m["low_boundary"]] == br.LOOP_NONE and low["gap"][m["low_neighbour"]] == 2


@pytest.mark.parametrize("jitter", (0.0, 0.1), ids=("plain", "jittered"))
def test_the_plate_with_a_hole(jitter):
    from elasticfusion_amd import accuracy, api
    S, m = bs.plate_scene(jitter=jitter)
    n = len(S)
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        for max_gap in (1.0, 0.75):
            for sizes in (dict(), dict(min_size=20), dict(max_size=20)):
                kw = dict(max_gap=max_gap, **bs.PLATE_KW, **sizes)
                want = br.boundaries(S, **kw)
                got, res = ef.boundaries(cell=bs.R_PLATE, result=True, **kw)
                check_rows(got, want, f"plate jitter={jitter} {kw}")
                check_result(res, want["result"], 0, f"plate jitter={jitter} {kw}")
                for what in WHATS:
                    rows, total, res = ef.boundarySelect(what=what, count=True, result=True, cell=bs.R_PLATE, **kw)
                    exp = br.listed(want, what)
                    assert total == len(exp) and np.array_equal(rows, exp), (jitter, kw, what)
                    check_result(res, want["result"], total, f"plate jitter={jitter} {kw} what={what}")
                if not jitter:                                               # the device against geometry alone
                    gap, status, loops = plate_expectation(m, n, max_gap)
                    assert_bits_equal(got["gap"], gap, "the plate's analytic gaps")
                    assert np.array_equal(got["status"], status)
                    for rows in loops:
                        assert (got["label"][rows] == rows.min()).all() and (got["size"][rows] == len(rows)).all()
                    assert (got["label"][status != br.BOUNDARY] == br.LOOP_NONE).all() and res["loops"] == 2 and res["largest"] == 40
                    if "min_size" in sizes or "max_size" in sizes:
                        acc = 0 if "min_size" in sizes else 1
                        assert np.array_equal(ef.boundarySelect(what=br.LOOPS_ACCEPTED, cell=bs.R_PLATE, **kw), loops[acc])
                        assert np.array_equal(ef.boundarySelect(what=br.LOOPS_REJECTED, cell=bs.R_PLATE, **kw), loops[1 - acc])
        if not jitter:
            # what a planner consumes: the two loops, the larger first, each with its frame
            found = accuracy.map_boundaries(ef, cell=bs.R_PLATE, **bs.PLATE_KW)
            _, _, loops = plate_expectation(m, n, 1.0)
            assert [l["size"] for l in found] == [40, 14] and [l["label"] for l in found] == [int(r.min()) for r in loops]
            M = ef.downloadMap()
            for l, rows in zip(found, loops):
                assert np.array_equal(l["rows"], rows) and np.array_equal(l["surfels"].view(np.uint32), M[rows].view(np.uint32))
                assert np.allclose(l["centroid"], M[rows, :3].astype(np.float64).mean(0)) and abs(l["axes"][2, 2]) > 0.999 and l["extent"][2] < 1e-9
            assert np.allclose(found[0]["extent"][:2], [11 * bs.SPACING, 9 * bs.SPACING]) and np.allclose(found[1]["extent"][:2], [5 * bs.SPACING, 4 * bs.SPACING])
            assert [l["size"] for l in accuracy.map_boundaries(ef, cell=bs.R_PLATE, max_size=20, **bs.PLATE_KW)] == [14]
        assert_bits_equal(ef.downloadMap(), S, "the calls change nothing")
    finally:
        ef.close()


@pytest.mark.parametrize("which", ("sphere", "hemisphere"))
def test_the_closed_sphere_and_the_hemisphere(which):
    from elasticfusion_amd import api
    S, radial = bs.sphere_scene() if which == "sphere" else bs.hemisphere_scene()
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        want = br.boundaries(S, **bs.SPHERE)
        got, res = ef.boundaries(cell=bs.R_SPHERE, result=True, **bs.SPHERE)
        check_rows(got, want, which)
        check_result(res, want["result"], 0, which)
        if which == "sphere":
            assert res["boundary"] == 0 and res["loops"] == 0 and (got["label"] == br.LOOP_NONE).all()
        else:
            assert res["loops"] == 1 and res["largest"] == res["boundary"] >= 20
        rows, total = ef.boundarySelect(what=br.BOUNDARY, count=True, cell=bs.R_SPHERE, **bs.SPHERE)
        assert total == res["boundary"] and np.array_equal(rows, br.listed(want, br.BOUNDARY))
    finally:
        ef.close()


@pytest.mark.parametrize("n", (2048, 2049, 2, 1, 0))
def test_size_steps(n):
    from elasticfusion_amd import api
    S = bs.patch_scene(n, seed=n + 1)
    ef = api.ElasticFusion()
    try:
        if n:
            ef.uploadMap(S)                                                  # (n = 0: the map of a fresh context)
        assert ef.lastCount() == n
        nl = nr.neighbour_lists(S, 0.06)
        for k, src in ((8, br.STORED), (16, br.ESTIMATED)):
            kw = dict(radius=0.06, k=k, normal_source=src, max_gap=1.5, min_size=3)
            want = br.boundaries(S, nl=nl, **kw)
            got, res = ef.boundaries(cell=0.06, result=True, **kw)
            check_rows(got, want, f"{n} rows, k={k}")
            check_result(res, want["result"], 0, f"{n} rows, k={k}")
            for what in WHATS:
                rows, total, res = ef.boundarySelect(what=what, count=True, result=True, cell=0.06, **kw)
                exp = br.listed(want, what)
                assert total == len(exp) and np.array_equal(rows, exp), (n, k, what)
                check_result(res, want["result"], total, f"{n} rows, k={k}, what={what}")
        if n >= 2048:
            r = want["result"]
            assert r["interior"] > 500 and r["boundary"] > 50 and r["sparse"] >= 1 and r["loops"] > r["accepted"] >= 1
        # max_rows smaller than the map: the arrays are written up to it and no further
        gap, cnt, st = np.full(n + 3, -7.0, F), np.full(n + 3, 0xABCD1234, np.uint32), np.full(n + 3, 0xEE, np.uint8)
        lab, size = np.full(n + 3, 0xABCD1234, np.uint32), np.full(n + 3, 0xABCD1234, np.uint32)
        prm = ef.boundaryParams(cell=0.06, **kw)
        cap = n // 2
        api._chk(api.lib().ef_map_boundaries(ef.h, C.byref(prm), None, api._ptr(gap), None, api._ptr(st), api._ptr(lab), None, cap, None), ef.h)
        assert (gap[cap:] == -7.0).all() and (st[cap:] == 0xEE).all() and (lab[cap:] == 0xABCD1234).all() and (cnt == 0xABCD1234).all()
        assert_bits_equal(gap[:cap], want["gap"][:cap], "max_rows below the map")
        assert np.array_equal(st[:cap], want["status"][:cap]) and np.array_equal(lab[:cap], want["label"][:cap])
        api._chk(api.lib().ef_map_boundaries(ef.h, C.byref(prm), None, None, api._ptr(cnt), None, None, api._ptr(size), n + 3, None), ef.h)
        assert (cnt[n:] == 0xABCD1234).all() and (size[n:] == 0xABCD1234).all() and np.array_equal(cnt[:n], want["count"]) and np.array_equal(size[:n], want["size"])
        assert (gap[cap:] == -7.0).all()
        assert_bits_equal(ef.downloadMap() if n else np.zeros((0, 12), F), S, "the calls change nothing")
    finally:
        ef.close()


def test_among_a_mask_a_box_and_its_inversion(edge):
    from elasticfusion_amd import api
    ef, S, m = edge["ef"], edge["S"], edge["marks"]
    full = edge["nl"][-1.0]
    box = dict(box_min=[39.95, -1.0, -1.0], box_max=[40.05, 1.0, 50.0])                  # cuts through the cloud
    for tests in (api.SEL_BOX, api.SEL_BOX | api.SEL_INVERT):
        sel = ef.mapSelection(tests=tests, **box)
        mask = np.zeros(len(S), bool)
        mask[ef.selectSurfels(sel)] = True
        assert 50 < mask.sum() < len(S) - 50
        part = nr.participants(S, mask)
        nl = nr.neighbour_lists(S, bs.R_EDGE, -1.0, part)
        # a row that takes no part still counts as a neighbour: the participants' counts are those of the whole map
        assert np.array_equal(nl[0][part], full[0][part]) and (nl[0][~part] == 0).all() and (full[0][~part] > 0).any()
        for src in (br.STORED, br.ESTIMATED):
            kw = dict(radius=bs.R_EDGE, k=8, min_neighbors=bs.MIN_NEIGHBORS, normal_source=src)
            want = br.boundaries(S, among=mask, nl=nl, **kw)
            got, res = ef.boundaries(among=sel, cell=bs.R_EDGE, result=True, **kw)
            check_rows(got, want, f"among tests={tests:#x} source={src}")
            check_result(res, want["result"], 0, f"among tests={tests:#x} source={src}")
            assert (got["status"][~part] == br.NONE).all() and (got["count"][~part] == 0).all() and (got["label"][~part] == br.LOOP_NONE).all()
            rows, total, res = ef.boundarySelect(among=dict(tests=tests, **box), what=br.LOOPS_ACCEPTED, count=True, result=True, cell=bs.R_EDGE, **kw)
            assert np.array_equal(rows, br.listed(want, br.LOOPS_ACCEPTED)) and mask[rows].all() and total > 10
            check_result(res, want["result"], total, f"among tests={tests:#x} source={src}")
    unchanged(ef, S, edge["probe"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# lists, device variants, refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_list_and_its_conventions(edge):
    from elasticfusion_amd import api
    ef, S = edge["ef"], edge["S"]
    kw = dict(radius=bs.R_EDGE, k=8, min_neighbors=bs.MIN_NEIGHBORS, min_size=4)
    want = br.boundaries(S, nl=edge["nl"][-1.0], **kw)
    M = ef.downloadMap()
    for what in WHATS:
        exp = br.listed(want, what)
        rows, total, res = ef.boundarySelect(what=what, count=True, result=True, cell=bs.R_EDGE, **kw)
        assert total == len(exp) >= 2 and np.array_equal(rows, exp), what
        check_result(res, want["result"], total, f"what={what}")
        none, t0 = ef.boundarySelect(what=what, max_rows=0, count=True, cell=bs.R_EDGE, **kw)          # NULL rows with max_rows 0
        assert len(none) == 0 and t0 == total
        assert_bits_equal(ef.gatherSurfels(rows), M[exp], f"the list of what={what} is what gatherSurfels takes")
    prm = ef.boundaryParams(cell=bs.R_EDGE, **kw)
    full = br.listed(want, br.BOUNDARY)
    rows = np.full(16, 0xABCD1234, np.uint32)
    cnt = C.c_uint32(0)
    api._chk(api.lib().ef_map_boundaries_select(ef.h, C.byref(prm), None, br.BOUNDARY, api._ptr(rows), 7, C.byref(cnt), None), ef.h)
    assert cnt.value == len(full) and np.array_equal(rows[:7], full[:7]) and (rows[7:] == 0xABCD1234).all()
    unchanged(ef, S, edge["probe"])


def test_device_variants_equal_the_host_variants(edge):
    from elasticfusion_amd import api
    ef, S = edge["ef"], edge["S"]
    n = len(S)
    size_of = C.sizeof(api.ef_boundary_result)
    for kw in (dict(radius=bs.R_EDGE, cell=bs.R_EDGE, k=8, min_neighbors=2, min_size=4),
               dict(radius=bs.R_EDGE, cell=bs.R_EDGE / 2, k=16, min_neighbors=3, normal_source=br.ESTIMATED, max_gap=1.5)):
        prm = ef.boundaryParams(**kw)
        host, hres = ef.boundaries(prm, result=True)
        d = {key: api.DevBuf((n + 2) * 4, fill=0xEE) for key in ("gap", "count", "label", "size")}
        d["status"] = api.DevBuf(n + 2, fill=0xEE)
        d_res = api.DevBuf(size_of)
        ef.boundariesDevice(prm, None, d["gap"].p, d["count"].p, d["status"].p, d["label"].p, d["size"].p, n + 2, d_res.p)
        ef.synchronize()
        for key in ("gap", "count", "label", "size"):
            got = d[key].to_array(np.uint32, n + 2)
            assert np.array_equal(got[:n], host[key].view(np.uint32)) and (got[n:] == 0xEEEEEEEE).all(), key
        got = d["status"].to_array(np.uint8, n + 2)
        assert np.array_equal(got[:n], host["status"]) and (got[n:] == 0xEE).all()
        raw = d_res.to_array(np.uint8, size_of).tobytes()
        assert ef._boundaryResult(api.ef_boundary_result.from_buffer_copy(raw)) == hres
        ef.boundariesDevice(prm, None, None, None, None, d["label"].p, None, 5)                        # any array may be missing
        ef.synchronize()
        for what in (br.BOUNDARY, br.LOOPS_REJECTED):
            rows, total, res = ef.boundarySelect(prm, what=what, count=True, result=True)
            d_rows, d_cnt, d_res = api.DevBuf(n * 4, fill=0xEE), api.DevBuf(16), api.DevBuf(size_of)
            ef.boundarySelectDevice(prm, None, what, d_rows.p, n, d_cnt.p, d_res.p)
            ef.synchronize()
            assert int(d_cnt.to_array(np.uint32, 1)[0]) == total
            got = d_rows.to_array(np.uint32, n)
            assert np.array_equal(got[:total], rows) and (got[total:] == 0xEEEEEEEE).all()
            raw = d_res.to_array(np.uint8, size_of).tobytes()
            assert ef._boundaryResult(api.ef_boundary_result.from_buffer_copy(raw)) == res
            ef.boundarySelectDevice(prm, None, what, None, 0, d_cnt.p)                                   # no list, no result
            ef.synchronize()
            assert int(d_cnt.to_array(np.uint32, 1)[0]) == total
    unchanged(ef, S, edge["probe"])


def test_refusals_with_a_context_and_during_capture():
    from elasticfusion_amd import api
    S, _ = bs.plate_scene()
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        refusals(api, ef, S)
    finally:
        ef.close()


def refusals(api, ef, S):
    refused(lambda: ef.boundaries(k=2), -1)                                                              # EF_EINVAL
    refused(lambda: ef.boundaries(max_gap=4.0), -1)
    refused(lambda: ef.boundarySelect(what=0), -1)
    refused(lambda: ef.boundarySelect(what=7), -1)
    refused(lambda: ef.boundaries(radius=1.0, cell=0.01), -1)
    assert "IDs are off" in refused(lambda: ef.boundaries(among=dict(tests=api.SEL_ID)), -4)
    name = ctypes.util.find_library("amdhip64") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")
    hip = C.CDLL(name)
    s = C.c_void_p(ef.stream())
    d = api.DevBuf(64)
    prm = ef.boundaryParams(cell=bs.R_PLATE, **bs.PLATE_KW)
    ef.synchronize()
    assert hip.hipStreamBeginCapture(s, C.c_int(2)) == 0   # relaxed
    try:
        # (the C call itself: boundaries asks for the map's count first, which waits for the stream and would end the capture)
        assert "captured" in refused(lambda: api._chk(api.lib().ef_map_boundaries(ef.h, C.byref(prm), None, None, None, None, None, None, 0, None), ef.h), -4)
        assert "captured" in refused(lambda: ef.boundariesDevice(prm, None, None, d.p, None, None, None, 8), -4)
        assert "captured" in refused(lambda: ef.boundarySelect(prm, max_rows=8), -4)
        assert "captured" in refused(lambda: ef.boundarySelectDevice(prm, None, br.BOUNDARY, d.p, 8, d.p), -4)
    finally:
        g = C.c_void_p()
        assert hip.hipStreamEndCapture(s, C.byref(g)) == 0
        if g.value:
            hip.hipGraphDestroy(g)
    ef.synchronize()
    assert ef.lastCount() == len(S)
    assert_bits_equal(ef.downloadMap(), S, "the refused calls changed nothing")
    check_rows(ef.boundaries(prm), br.boundaries(S, **bs.PLATE_KW), "after the capture")


def test_a_loop_closing_context_finds_its_boundaries_too():
    from elasticfusion_amd import api
    S, m = bs.plate_scene()
    ef = api.ElasticFusion(closeLoops=True)
    try:
        ef.uploadMap(S)
        want = br.boundaries(S, **bs.PLATE_KW)
        check_rows(ef.boundaries(cell=bs.R_PLATE, **bs.PLATE_KW), want, "a loop-closing context")
        assert np.array_equal(ef.boundarySelect(what=br.BOUNDARY, cell=bs.R_PLATE, **bs.PLATE_KW), br.listed(want, br.BOUNDARY))
    finally:
        ef.close()
