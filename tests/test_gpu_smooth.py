"""Smooth the map's positions on the device (ef_map_smooth / ef_map_smooth_select / ef_map_smooth_apply, include/ef_hip.h; kernels in
elasticfusion_amd/csrc/ef_smooth.inc).

The operation is restated in numpy from the header alone (tests/smoothref.py).  The header fixes every rounding and every order, so everything
is compared BIT FOR BIT: positions, normals, curvature, shift, counts, status, the row lists, the results and the map a write-back leaves.  The
scenes (tests/normalscenes.py, tests/regionscenes.py, tests/smoothscenes.py) are hand-built; tests/test_smooth_host.py shows on the CPU that
they contain what they claim.  A reference is computed once per set of parameters and shared (ref_runs)."""
import ctypes as C
import ctypes.util
import os

import numpy as np
import pytest

import normalref as nr
import normalscenes as ns
import regionscenes as rs
import smoothref as sr
import smoothscenes as ss
from queryref import assert_bits_equal
from test_gpu_select import refused, state_of, u32

pytestmark = pytest.mark.gpu

F = np.float32
WHATS = (sr.SMOOTHED, sr.SPARSE, sr.DEGENERATE, sr.CLAMPED, sr.SHIFTED)
DRIFT = dict(radius=ss.R_DRIFT, k=16)
_scenes, _lists, _runs = {}, {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = {"edge": lambda: ns.edge_scene()[0], "drift": ss.drift_scene, "box": lambda: ss.noisy_box_corner()[0]}[name]()
    return _scenes[name]


def ref_runs(name, S=None, among=None, among_key=None, **kw):
    """smoothref.smooth_runs of a scene, once per set of parameters; the neighbour lists once per (scene, radius, min_conf, selection)"""
    S = scene(name) if S is None else S
    p = dict(sr.DEFAULTS, **kw)
    lk = (name, float(p["radius"]), float(p["min_conf"]), among_key)
    if lk not in _lists:
        _lists[lk] = nr.neighbour_lists(S, p["radius"], p["min_conf"], nr.participants(S, among))
    rk = lk + tuple(sorted(kw.items()))
    if rk not in _runs:
        _runs[rk] = sr.smooth_runs(S, among=among, nl=_lists[lk], **kw)
    return _runs[rk]


def check_rows(got, want, what):
    assert np.array_equal(got["status"], want["status"]), (what, np.nonzero(got["status"] != want["status"])[0][:10])
    assert np.array_equal(got["count"], want["count"]), (what, np.nonzero(got["count"] != want["count"])[0][:10])
    for key in ("position", "normal", "curvature", "shift"):
        assert_bits_equal(got[key], want[key], f"{key}: {what}")


def check_result(got, want, listed, what):
    assert got == dict(want, listed=listed), (what, got, want, listed)


@pytest.fixture(scope="module")
def edge():
    from elasticfusion_amd import api
    S = scene("edge")
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    thr = float(ef.getConfidenceThreshold())
    assert ns.CONF_LOW < thr < ns.CONF_HIGH
    yield dict(ef=ef, S=S, thr=thr)
    ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# per-row outputs
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable_only", (False, True))
@pytest.mark.parametrize("cell", (ns.R_EDGE, ns.R_EDGE / 16))
def test_the_edge_scene_equals_the_reference_exactly(edge, cell, stable_only):
    ef, S = edge["ef"], edge["S"]
    mc = edge["thr"] if stable_only else -1.0
    seen = set()
    for k in ns.KS:
        for w in (sr.UNIFORM, sr.COMPACT):
            for gate in (0, 1):
                kw = dict(radius=ns.R_EDGE, min_conf=mc, k=k, min_neighbors=ns.MIN_NEIGHBORS[k], weighting=w, normal_gate=gate, min_normal_cos=0.0)
                runs = ref_runs("edge", iterations=3, **kw)
                for it in (1, 2, 3):                                         # both ping-pong parities are the last buffer
                    got, res = ef.smoothMap(cell=cell, iterations=it, result=True, **kw)
                    what = f"k={k} cell={cell} min_conf={mc} weighting={w} gate={gate} iterations={it}"
                    check_rows(got, runs[it - 1], what)
                    check_result(res, runs[it - 1]["result"], 0, what)
                    seen |= set(np.unique(got["status"]).tolist())
    assert seen == {sr.NONE, sr.SMOOTHED, sr.SPARSE, sr.DEGENERATE}
    assert ef.lastCount() == len(S)
    assert_bits_equal(ef.downloadMap(), S, "smoothMap changes nothing")


def test_unit_weights_give_the_normals_of_estimate_normals(edge):
    ef = edge["ef"]
    for k in ns.KS:
        for cell in (ns.R_EDGE, ns.R_EDGE / 16):
            kw = dict(radius=ns.R_EDGE, cell=cell, k=k, min_neighbors=ns.MIN_NEIGHBORS[k])
            sm = ef.smoothMap(weighting=sr.UNIFORM, normal_gate=0, iterations=1, **kw)
            est = ef.estimateNormals(orientation=nr.KEEP_SIDE, **kw)
            assert_bits_equal(sm["normal"], est["normals"], f"normal k={k}")
            assert_bits_equal(sm["curvature"], est["curvature"], f"curvature k={k}")
            assert np.array_equal(sm["count"], est["count"])
            for mine, theirs in ((sr.NONE, nr.NONE), (sr.SMOOTHED, nr.ESTIMATED), (sr.SPARSE, nr.SPARSE), (sr.DEGENERATE, nr.DEGENERATE)):
                assert np.array_equal(sm["status"] == mine, est["status"] == theirs), (k, mine)


@pytest.mark.parametrize("shift", ((0.0, 0.0, 0.0), ns.SHIFT), ids=("origin", "shifted"))
def test_the_noisy_sphere_and_its_shifted_copy(shift):
    from elasticfusion_amd import api
    S, radial = ns.sphere_scene(noise=0.001, shift=shift)
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        nl = nr.neighbour_lists(S, ns.R_SPHERE)
        for kw in (dict(iterations=2), dict(iterations=3, weighting=sr.UNIFORM, normal_gate=1, min_normal_cos=0.95)):
            kw = dict(kw, radius=ns.R_SPHERE, k=12)
            want = sr.smooth(S, nl=nl, **kw)
            got, res = ef.smoothMap(cell=ns.R_SPHERE, result=True, **kw)
            check_rows(got, want, f"sphere at {shift} {kw}")
            check_result(res, want["result"], 0, f"sphere at {shift}")
            assert (got["status"] == sr.SMOOTHED).all() and res["moved"] > 2000
        centre = np.asarray(shift, np.float64)
        before = np.abs(np.linalg.norm(S[:, :3].astype(np.float64) - centre, axis=1) - 0.3)
        after = np.abs(np.linalg.norm(got["position"].astype(np.float64) - centre, axis=1) - 0.3)
        print("sphere at", shift, "RMS radial error in mm: %.3f -> %.3f" % (1e3 * np.sqrt((before ** 2).mean()), 1e3 * np.sqrt((after ** 2).mean())))
    finally:
        ef.close()


@pytest.mark.parametrize("n", (2048, 2049, 1, 0))
def test_size_steps(n):
    from elasticfusion_amd import api
    S = ns.patch_scene(n, seed=n + 1)
    ef = api.ElasticFusion()
    try:
        if n:
            ef.uploadMap(S)                                                  # (n = 0: the map of a fresh context)
        assert ef.lastCount() == n
        nl = nr.neighbour_lists(S, ns.R_SPHERE)
        for k in (8, 16):
            kw = dict(radius=ns.R_SPHERE, k=k, iterations=2, max_shift=2e-4, shift_threshold=1e-4)
            want = sr.smooth(S, nl=nl, **kw)
            got, res = ef.smoothMap(cell=ns.R_SPHERE, result=True, **kw)
            check_rows(got, want, f"{n} rows, k={k}")
            check_result(res, want["result"], 0, f"{n} rows, k={k}")
            for what in WHATS:
                rows, total, res = ef.smoothSelect(what=what, count=True, result=True, cell=ns.R_SPHERE, **kw)
                exp = sr.listed(want, what)
                assert total == len(exp) and np.array_equal(rows, exp), (n, k, what)
                check_result(res, want["result"], total, f"{n} rows, k={k}, what={what}")
        if n >= 2048:
            r = want["result"]
            assert r["smoothed"] > 1900 and r["sparse"] >= 5 and r["clamped"] > 20 and 20 < len(sr.listed(want, sr.SHIFTED)) < r["moved"]
        # max_rows smaller than the map: the arrays are written up to it and no further
        pos, cnt, st, sh = np.full((n + 3, 3), -7.0, F), np.full(n + 3, 0xABCD1234, np.uint32), np.full(n + 3, 0xEE, np.uint8), np.full(n + 3, -7.0, F)
        prm = ef.smoothParams(cell=ns.R_SPHERE, **kw)
        cap = n // 2
        api._chk(api.lib().ef_map_smooth(ef.h, C.byref(prm), None, api._ptr(pos), None, None, api._ptr(sh), api._ptr(cnt), api._ptr(st), cap, None), ef.h)
        assert (pos[cap:] == -7.0).all() and (cnt[cap:] == 0xABCD1234).all() and (st[cap:] == 0xEE).all() and (sh[cap:] == -7.0).all()
        assert_bits_equal(pos[:cap], want["position"][:cap], "max_rows below the map")
        assert np.array_equal(st[:cap], want["status"][:cap])
        api._chk(api.lib().ef_map_smooth(ef.h, C.byref(prm), None, api._ptr(pos), None, None, api._ptr(sh), api._ptr(cnt), api._ptr(st), n + 3, None), ef.h)
        assert (pos[n:] == -7.0).all() and (cnt[n:] == 0xABCD1234).all() and (st[n:] == 0xEE).all() and np.array_equal(cnt[:n], want["count"])
        assert_bits_equal(sh[:n], want["shift"], "max_rows above the map")
        if n:
            assert_bits_equal(ef.downloadMap(), S, "the map is unchanged")
    finally:
        ef.close()


def test_among_a_box_that_cuts_a_face():
    from elasticfusion_amd import api
    S = scene("box")
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        full = ref_runs("box", iterations=2)[-1]
        for tests in (api.SEL_BOX, api.SEL_BOX | api.SEL_INVERT):
            sel = ef.mapSelection(tests=tests, **rs.box_band(S))
            mask = np.zeros(len(S), bool)
            mask[ef.selectSurfels(sel)] = True
            assert 100 < mask.sum() < len(S) - 100
            want = ref_runs("box", among=mask, among_key=tests, iterations=2)[-1]
            got, res = ef.smoothMap(among=sel, iterations=2, result=True)
            check_rows(got, want, f"among tests={tests:#x}")
            check_result(res, want["result"], 0, f"among tests={tests:#x}")
            part = want["part"]
            assert (got["status"][~part] == sr.NONE).all() and (got["shift"][~part] == 0).all()
            assert_bits_equal(got["position"][~part], S[~part, :3], "rows outside keep their bits")
            # ... and still act as neighbours: the participants' counts are those of the whole map, and the first iteration moves them as it
            # does without the selection (from the second on the rows outside stand still, and the two runs part)
            assert np.array_equal(got["count"][part], full["count"][part])
            first = ref_runs("box", among=mask, among_key=tests, iterations=2)[0]
            assert_bits_equal(first["position"][part], ref_runs("box", iterations=2)[0]["position"][part], "iteration 1 of the participants")
            assert not np.array_equal(u32(want["position"][part]), u32(full["position"][part]))
            rows, total, res = ef.smoothSelect(among=dict(tests=tests, **rs.box_band(S)), what=sr.SMOOTHED, iterations=2, count=True, result=True)
            assert np.array_equal(rows, sr.listed(want, sr.SMOOTHED)) and mask[rows].all()
            check_result(res, want["result"], total, f"among tests={tests:#x}")
    finally:
        ef.close()


def test_the_gate_on_the_box_corner():
    from elasticfusion_amd import api
    S, marks, near = ss.noisy_box_corner()
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        rms = {}
        for gate in (0, 1):
            kw = dict(normal_gate=gate, min_normal_cos=0.9)
            want = ref_runs("box", S=S, **kw)[-1]
            got = ef.smoothMap(**kw)
            check_rows(got, want, f"box corner gate={gate}")
            rms[gate] = ss.crease_rms(got["position"], marks, near)
        print("RMS distance to the own face near a crease in mm: gated %.3f, ungated %.3f" % (1e3 * rms[1], 1e3 * rms[0]))
        assert rms[1] < rms[0]
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the clamp, the strength, the lists, the device variants
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drift():
    from elasticfusion_amd import api
    S = scene("drift")
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    yield dict(ef=ef, S=S)
    ef.close()


def test_the_clamp_the_strength_and_neighbours_past_the_radius(drift):
    ef = drift["ef"]
    for kw in (dict(max_shift=ss.R_DRIFT / 16, strength=0.5), dict(strength=0.5), dict(max_shift=ss.R_DRIFT / 16, weighting=sr.UNIFORM),
               dict(normal_gate=1, min_normal_cos=0.5), dict(max_shift=float("inf"))):
        runs = ref_runs("drift", iterations=3, **DRIFT, **kw)
        for it in (1, 2, 3):
            got, res = ef.smoothMap(cell=ss.R_DRIFT, iterations=it, result=True, **DRIFT, **kw)
            check_rows(got, runs[it - 1], f"drift {kw} iterations={it}")
            check_result(res, runs[it - 1]["result"], 0, f"drift {kw} iterations={it}")
        if "max_shift" in kw and kw["max_shift"] < 1:
            assert 20 < runs[0]["result"]["clamped"] < runs[2]["result"]["clamped"]
            rows = ef.smoothSelect(what=sr.CLAMPED, cell=ss.R_DRIFT, iterations=3, **DRIFT, **kw)
            assert np.array_equal(rows, sr.listed(runs[2], sr.CLAMPED))


def test_every_list_and_its_conventions(drift):
    from elasticfusion_amd import api
    ef, S = drift["ef"], drift["S"]
    kw = dict(iterations=3, max_shift=ss.R_DRIFT / 16, shift_threshold=0.001, normal_gate=1, min_normal_cos=0.5, **DRIFT)
    want = ref_runs("drift", **kw)[-1]
    for what in WHATS:
        exp = sr.listed(want, what)
        rows, total, res = ef.smoothSelect(what=what, count=True, result=True, cell=ss.R_DRIFT, **kw)
        assert total == len(exp) > 5 and np.array_equal(rows, exp), what
        check_result(res, want["result"], total, f"what={what}")
        none, t0 = ef.smoothSelect(what=what, max_rows=0, count=True, cell=ss.R_DRIFT, **kw)            # NULL rows with max_rows 0
        assert len(none) == 0 and t0 == total
        assert_bits_equal(ef.gatherSurfels(rows), S[exp], f"the list of what={what} is what gatherSurfels takes")
    prm = ef.smoothParams(cell=ss.R_DRIFT, **kw)
    full = sr.listed(want, sr.SHIFTED)
    rows = np.full(16, 0xABCD1234, np.uint32)
    cnt = C.c_uint32(0)
    api._chk(api.lib().ef_map_smooth_select(ef.h, C.byref(prm), None, sr.SHIFTED, api._ptr(rows), 7, C.byref(cnt), None), ef.h)
    assert cnt.value == len(full) and np.array_equal(rows[:7], full[:7]) and (rows[7:] == 0xABCD1234).all()


def test_device_variants_equal_the_host_variants(drift):
    from elasticfusion_amd import api
    ef, S = drift["ef"], drift["S"]
    n = len(S)
    for kw in (dict(cell=ss.R_DRIFT, iterations=2), dict(cell=ss.R_DRIFT / 2, iterations=3, k=8, normal_gate=1, min_normal_cos=0.5, max_shift=0.002)):
        prm = ef.smoothParams(**dict(DRIFT, **kw))
        host, hres = ef.smoothMap(prm, result=True)
        d = dict(position=api.DevBuf((n + 2) * 12, fill=0xEE), normal=api.DevBuf((n + 2) * 12, fill=0xEE), curvature=api.DevBuf((n + 2) * 4, fill=0xEE),
                 shift=api.DevBuf((n + 2) * 4, fill=0xEE), count=api.DevBuf((n + 2) * 4, fill=0xEE), status=api.DevBuf(n + 2, fill=0xEE))
        d_res = api.DevBuf(C.sizeof(api.ef_smooth_result))
        ef.smoothMapDevice(prm, None, d["position"].p, d["normal"].p, d["curvature"].p, d["shift"].p, d["count"].p, d["status"].p, n + 2, d_res.p)
        ef.synchronize()
        for key, words in (("position", 3), ("normal", 3), ("curvature", 1), ("shift", 1), ("count", 1)):
            got = d[key].to_array(np.uint32, (n + 2) * words)
            assert np.array_equal(got[:n * words], host[key].reshape(-1).view(np.uint32)) and (got[n * words:] == 0xEEEEEEEE).all(), key
        got = d["status"].to_array(np.uint8, n + 2)
        assert np.array_equal(got[:n], host["status"]) and (got[n:] == 0xEE).all()
        raw = d_res.to_array(np.uint8, C.sizeof(api.ef_smooth_result)).tobytes()
        assert ef._smoothResult(api.ef_smooth_result.from_buffer_copy(raw)) == hres
        ef.smoothMapDevice(prm, None, None, None, None, d["shift"].p, None, None, 5)                      # any array may be missing
        ef.synchronize()
        for what in (sr.SMOOTHED, sr.SHIFTED):
            rows, total, res = ef.smoothSelect(prm, what=what, count=True, result=True)
            d_rows, d_cnt = api.DevBuf(n * 4, fill=0xEE), api.DevBuf(16)
            ef.smoothSelectDevice(prm, None, what, d_rows.p, n, d_cnt.p, d_res.p)
            ef.synchronize()
            assert int(d_cnt.to_array(np.uint32, 1)[0]) == total
            got = d_rows.to_array(np.uint32, n)
            assert np.array_equal(got[:total], rows) and (got[total:] == 0xEEEEEEEE).all()
            raw = d_res.to_array(np.uint8, C.sizeof(api.ef_smooth_result)).tobytes()
            assert ef._smoothResult(api.ef_smooth_result.from_buffer_copy(raw)) == res
            ef.smoothSelectDevice(prm, None, what, None, 0, d_cnt.p)                                     # no list, no result
            ef.synchronize()
            assert int(d_cnt.to_array(np.uint32, 1)[0]) == total


# ---------------------------------------------------------------------------------------------------------------------------------------
# the write-back
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", (dict(), dict(set_normal=1, iterations=3), dict(set_normal=1, normal_gate=1, min_normal_cos=0.5, max_shift=0.002)),
                         ids=("positions", "normals-too", "gated-clamped"))
def test_the_write_back_changes_positions_and_nothing_else(kw):
    from elasticfusion_amd import accuracy, api
    S = scene("drift").copy()
    S[:, 5] = np.arange(1, len(S) + 1, dtype=np.uint32).view(F)              # bits in the ID lane, both times and the colour differ by row
    S[:, 6], S[:, 7], S[:, 4] = np.arange(len(S)) % 7, 7 + np.arange(len(S)) % 5, np.arange(len(S)) * 31.0
    S[3, 0], S[4, 3] = np.nan, ns.CONF_LOW
    kw = dict(kw, **DRIFT)
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        want = sr.smooth(S, **kw)
        W = sr.written(S, want)
        assert_bits_equal(accuracy.smoothed_map(ef, cell=ss.R_DRIFT, **kw), W, "smoothed_map is gather + the reference")
        q0, s0, m0 = state_of(ef)
        assert_bits_equal(m0, S, "smoothed_map changes nothing")
        res = ef.applySmooth(cell=ss.R_DRIFT, **kw)
        check_result(res, want["result"], want["result"]["moved"], str(kw))
        q1, s1, got = state_of(ef)
        assert np.array_equal(q0.view(np.uint64), q1.view(np.uint64)) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
        assert ef.lastCount() == len(S)
        assert np.array_equal(u32(got), u32(W)), np.nonzero(u32(got) != u32(W))
        changed = u32(got) != u32(S)
        moved = want["shift"] > 0
        done = want["status"] == sr.SMOOTHED
        assert not changed[:, 3:8].any() and not changed[:, 11].any() and not changed[~moved, :3].any() and changed[moved, :3].any(1).all()
        assert moved.sum() > 400 and not changed[3].any() and not changed[want["status"] == sr.SPARSE].any()
        assert (changed[done, 8:11].any(1).sum() > 400 and not changed[~done, 8:11].any()) if kw.get("set_normal") else not changed[:, 8:11].any()
        # the index was rebuilt: a query at a moved position finds a row that lies there, and nothing lies where a far-moved row was
        far = np.nonzero(want["shift"] > 1e-3)[0]
        rows = ef.queryNearest(W[far, :3], 1e-6)[0]
        assert (rows != api.ROW_NONE).all()
        assert_bits_equal(W[rows, :3], W[far, :3], "the query sees the moved positions")
        old = ef.queryNearest(S[far, :3], 1e-6)[0]
        assert (old == api.ROW_NONE).sum() > 0.9 * len(far)
        again = ef.applySmooth(cell=ss.R_DRIFT, **kw)                          # not idempotent: it fits the moved positions
        want2 = sr.smooth(W, **kw)
        check_result(again, want2["result"], want2["result"]["moved"], "a second write-back")
        assert np.array_equal(u32(ef.downloadMap()), u32(sr.written(W, want2)))
    finally:
        ef.close()


def test_a_write_back_that_moves_nothing_is_valid():
    from elasticfusion_amd import api
    S = ns.patch_scene(300, seed=5)
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        kw = dict(radius=1e-4, cell=1e-4)                                    # nobody has a neighbour: every row is SPARSE
        res = ef.applySmooth(**kw)
        assert res == dict(participants=300, smoothed=0, sparse=300, degenerate=0, clamped=0, moved=0, listed=0, largest_shift=0.0)
        assert_bits_equal(ef.downloadMap(), S, "nothing moved")
        sel = ef.mapSelection(tests=api.SEL_CONF, conf_min=1e6, conf_max=2e6)                              # nobody participates
        assert ef.applySmooth(among=sel)["participants"] == 0
        assert_bits_equal(ef.downloadMap(), S, "nothing took part")
        assert ef.queryNearest(S[:4, :3], 1e-6)[0].tolist() == [0, 1, 2, 3]
    finally:
        ef.close()
    ef = api.ElasticFusion()
    try:
        res = ef.applySmooth()                                               # the empty map of a fresh context
        assert res["participants"] == 0 and ef.lastCount() == 0
    finally:
        ef.close()


def test_write_back_then_mapping_equals_upload_and_restore(seq):
    from elasticfusion_amd import api
    fr = [seq.frame(k) for k in range(8)]

    def feed(ef, k):
        ef.processFrame(fr[k][0], fr[k][1], k * 33333)

    a, b = api.ElasticFusion(), api.ElasticFusion()
    try:
        for k in range(6):
            feed(a, k)
        m6 = a.downloadMap()
        ck = a.checkpoint(fr[5][0], fr[5][1])
        kw = dict(radius=0.01, cell=0.01, k=8, set_normal=1)
        sm = a.smoothMap(**kw)                                               # (the device's own result: the reference is quadratic in the map)
        res = a.applySmooth(**kw)
        print("frame 6: surfels", len(m6), res)
        part, done = sm["status"] != sr.NONE, sm["status"] == sr.SMOOTHED
        assert res["smoothed"] == int(done.sum()) > len(m6) // 2 and res["listed"] == res["moved"] > len(m6) // 4
        W = m6.copy()
        W[part, :3] = sm["position"][part]
        W[done, 8:11] = sm["normal"][done]
        assert np.array_equal(u32(a.downloadMap()), u32(W))
        assert a.getTick() == ck["tick"] and np.array_equal(a.getPoseQT(), ck["qt"])
        ck["map"] = W
        b.restore(ck)
        for k in range(6, 8):
            feed(a, k)
            feed(b, k)
            (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
            assert np.array_equal(qa.view(np.uint64), qb.view(np.uint64)), (k, qa, qb)
            assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), (k, sa, sb)
            assert_bits_equal(ma, mb, f"the map after frame {k}")
    finally:
        for ef in (a, b):
            ef.close()


def test_refusals_on_a_loop_closing_context_and_during_capture():
    from elasticfusion_amd import api
    S = scene("drift")
    ef = api.ElasticFusion(closeLoops=True)
    try:
        ef.uploadMap(S)
        assert "close_loops" in refused(lambda: ef.applySmooth(cell=ss.R_DRIFT, **DRIFT), -4)           # EF_ESTATE
        assert ef.lastCount() == len(S)
        assert_bits_equal(ef.downloadMap(), S, "a refused write-back")
        want = ref_runs("drift", iterations=3, **DRIFT)[0]
        check_rows(ef.smoothMap(cell=ss.R_DRIFT, **DRIFT), want, "smoothMap on a loop-closing context")
        assert np.array_equal(ef.smoothSelect(what=sr.SPARSE, cell=ss.R_DRIFT, **DRIFT), sr.listed(want, sr.SPARSE))
        refused(lambda: ef.smoothMap(k=2), -1)                                                           # EF_EINVAL
        refused(lambda: ef.smoothSelect(what=0), -1)
        refused(lambda: ef.smoothMap(iterations=17), -1)
        refused(lambda: ef.applySmooth(strength=0.0), -1)
    finally:
        ef.close()
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        assert "IDs are off" in refused(lambda: ef.smoothMap(among=dict(tests=api.SEL_ID)), -4)
        name = ctypes.util.find_library("amdhip64") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")
        hip = C.CDLL(name)
        s = C.c_void_p(ef.stream())
        d = api.DevBuf(64)
        prm = ef.smoothParams(cell=ss.R_DRIFT, **DRIFT)
        ef.synchronize()
        assert hip.hipStreamBeginCapture(s, C.c_int(2)) == 0   # relaxed
        try:
            # (the C call itself: smoothMap asks for the map's count first, which waits for the stream and would end the capture)
            assert "captured" in refused(lambda: api._chk(api.lib().ef_map_smooth(ef.h, C.byref(prm), None, None, None, None, None, None, None, 0, None),
                                                          ef.h), -4)
            assert "captured" in refused(lambda: ef.smoothMapDevice(prm, None, None, None, None, d.p, None, None, 8), -4)
            assert "captured" in refused(lambda: ef.smoothSelect(prm, max_rows=8), -4)
            assert "captured" in refused(lambda: ef.smoothSelectDevice(prm, None, sr.SHIFTED, d.p, 8, d.p), -4)
            assert "captured" in refused(lambda: ef.applySmooth(prm), -4)
        finally:
            g = C.c_void_p()
            assert hip.hipStreamEndCapture(s, C.byref(g)) == 0
            if g.value:
                hip.hipGraphDestroy(g)
        ef.synchronize()
        assert_bits_equal(ef.downloadMap(), S, "the refused calls changed nothing")
        want = ref_runs("drift", iterations=3, **DRIFT)[0]
        check_result(ef.applySmooth(prm), want["result"], want["result"]["moved"], "after the capture")
    finally:
        ef.close()
