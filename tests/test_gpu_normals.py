"""Estimate normals, curvature and spacing on the device (ef_map_normals / ef_map_normals_select / ef_map_reestimate_normals,
include/ef_hip.h; kernels in elasticfusion_amd/csrc/ef_normals.inc).

The operation is restated in numpy and Python floats from the header alone (tests/normalref.py).  The header fixes every rounding and every
order, so everything is compared BIT FOR BIT: normals, curvature, spacing, counts, status, the row lists, the results and the map a write-back
leaves.  The scenes (tests/normalscenes.py) are hand-built; tests/test_normals_host.py shows on the CPU that they contain every edge they claim.
"""
import ctypes as C

import numpy as np
import pytest

import insertref as ir
import normalref as nr
import normalscenes as sc
from queryref import assert_bits_equal
from test_gpu_select import refused, sixteen, state_of, u32   # noqa: F401  (sixteen is a fixture)

pytestmark = pytest.mark.gpu

F = np.float32
WHATS = (nr.ESTIMATED, nr.SPARSE, nr.DEGENERATE, nr.CURVED, nr.FLAT)


def check_rows(got, want, what):
    assert np.array_equal(got["status"], want["status"]), (what, np.nonzero(got["status"] != want["status"])[0][:10])
    assert np.array_equal(got["count"], want["count"]), (what, np.nonzero(got["count"] != want["count"])[0][:10])
    for key in ("spacing", "curvature", "normals"):
        assert_bits_equal(got[key], want[key], f"{key}: {what}")


def check_result(got, want, listed, what):
    assert got == dict(want, listed=listed), (what, got, want, listed)


@pytest.fixture(scope="module")
def edge():
    from elasticfusion_amd import api
    S, marks = sc.edge_scene()
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    thr = float(ef.getConfidenceThreshold())
    assert sc.CONF_LOW < thr < sc.CONF_HIGH
    nl = {mc: nr.neighbour_lists(S, sc.R_EDGE, mc) for mc in (-1.0, thr)}
    yield dict(ef=ef, S=S, marks=marks, thr=thr, nl=nl)
    ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# per-row estimates
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stable_only", (False, True))
@pytest.mark.parametrize("cell", (sc.R_EDGE, sc.R_EDGE / 16))
def test_the_edge_scene_equals_the_reference_exactly(edge, cell, stable_only):
    ef, S, m = edge["ef"], edge["S"], edge["marks"]
    mc = edge["thr"] if stable_only else -1.0
    v = [float(x) for x in S[m["at_view"], :3]]
    seen = set()
    for k in sc.KS:
        base = dict(radius=sc.R_EDGE, min_conf=mc, k=k, min_neighbors=sc.MIN_NEIGHBORS[k])
        for orient in (dict(orientation=nr.KEEP_SIDE), dict(orientation=nr.VIEWPOINT, side=1, viewpoint=v), dict(orientation=nr.VIEWPOINT, side=-1, viewpoint=v)):
            want = nr.estimate(S, nl=edge["nl"][mc], **base, **orient)
            got = ef.estimateNormals(cell=cell, **base, **orient)
            check_rows(got, want, f"k={k} cell={cell} min_conf={mc} {orient}")
            seen |= set(np.unique(want["status"]).tolist())
    assert seen == {nr.NONE, nr.ESTIMATED, nr.SPARSE, nr.DEGENERATE}
    assert ef.lastCount() == len(S)
    assert_bits_equal(ef.downloadMap(), S, "the estimate changes nothing")


@pytest.mark.parametrize("shift", ((0.0, 0.0, 0.0), sc.SHIFT), ids=("origin", "shifted"))
def test_the_sphere_and_its_shifted_copy(shift):
    from elasticfusion_amd import api
    S, radial = sc.sphere_scene(shift=shift)
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        want = nr.estimate(S, radius=sc.R_SPHERE, k=12)
        got = ef.estimateNormals(radius=sc.R_SPHERE, cell=sc.R_SPHERE, k=12)
        check_rows(got, want, f"sphere at {shift}")
        assert (got["status"] == nr.ESTIMATED).all()
        ang = np.degrees(np.arcsin(np.clip(np.linalg.norm(np.cross(got["normals"].astype(np.float64), radial), axis=1), 0, 1)))
        print("sphere at", shift, "angle to the radial direction: median %.3f max %.3f degrees" % (np.median(ang), ang.max()))
        assert ang.max() <= 1.5 * 6.155                   # the CPU test's bar: the reference's own maximum times 1.5
    finally:
        ef.close()


@pytest.mark.parametrize("n", (2048, 2049, 1, 0))
def test_size_steps(n):
    from elasticfusion_amd import api
    S = sc.patch_scene(n, seed=n + 1)
    ef = api.ElasticFusion()
    try:
        if n:
            ef.uploadMap(S)                                                  # (n = 0: the map of a fresh context)
        assert ef.lastCount() == n
        for k in (8, 16):
            kw = dict(radius=sc.R_SPHERE, k=k, max_curvature=2e-4)
            want = nr.estimate(S, **kw)
            got = ef.estimateNormals(cell=sc.R_SPHERE, **kw)
            check_rows(got, want, f"{n} rows, k={k}")
            for what in WHATS:
                rows, total, res = ef.normalSelect(what=what, count=True, result=True, cell=sc.R_SPHERE, **kw)
                exp = nr.listed(want, what)
                assert total == len(exp) and np.array_equal(rows, exp), (n, k, what)
                check_result(res, want["result"], total, f"{n} rows, k={k}, what={what}")
        if n >= 2048:
            assert want["result"]["estimated"] > 1900 and want["result"]["sparse"] >= 5 and len(nr.listed(want, nr.CURVED)) > 20
        # max_rows smaller than the map: the arrays are written up to it and no further
        nrm, cnt, st = np.full((n + 3, 3), -7.0, F), np.full(n + 3, 0xABCD1234, np.uint32), np.full(n + 3, 0xEE, np.uint8)
        prm = ef.normalParams(cell=sc.R_SPHERE, **kw)
        cap = n // 2
        api._chk(api.lib().ef_map_normals(ef.h, C.byref(prm), None, api._ptr(nrm), None, None, api._ptr(cnt), api._ptr(st), cap), ef.h)
        assert (nrm[cap:] == -7.0).all() and (cnt[cap:] == 0xABCD1234).all() and (st[cap:] == 0xEE).all()
        assert_bits_equal(nrm[:cap], want["normals"][:cap], "max_rows below the map")
        assert np.array_equal(st[:cap], want["status"][:cap])
        api._chk(api.lib().ef_map_normals(ef.h, C.byref(prm), None, api._ptr(nrm), None, None, api._ptr(cnt), api._ptr(st), n + 3), ef.h)
        assert (nrm[n:] == -7.0).all() and (cnt[n:] == 0xABCD1234).all() and np.array_equal(cnt[:n], want["count"])
    finally:
        ef.close()


def test_among_a_box_and_its_inversion(edge):
    from elasticfusion_amd import api
    ef, S = edge["ef"], edge["S"]
    full = edge["nl"][-1.0]
    box = dict(box_min=[-0.05, -1.0, -1.0], box_max=[0.05, 1.0, 50.0])                  # cuts through the cloud
    for tests in (api.SEL_BOX, api.SEL_BOX | api.SEL_INVERT):
        sel = ef.mapSelection(tests=tests, **box)
        mask = np.zeros(len(S), bool)
        mask[ef.selectSurfels(sel)] = True
        assert 50 < mask.sum() < len(S) - 50
        part = nr.participants(S, mask)
        nl = nr.neighbour_lists(S, sc.R_EDGE, -1.0, part)
        # a row that takes no part still counts as a neighbour: the participants' counts are those of the whole map
        assert np.array_equal(nl[0][part], full[0][part]) and (nl[0][~part] == 0).all() and (full[0][~part] > 0).any()
        kw = dict(radius=sc.R_EDGE, k=8)
        want = nr.estimate(S, among=mask, nl=nl, **kw)
        got = ef.estimateNormals(among=sel, cell=sc.R_EDGE, **kw)
        check_rows(got, want, f"among tests={tests:#x}")
        assert (got["status"][~part] == nr.NONE).all() and np.isposinf(got["spacing"][~part]).all()
        rows, total, res = ef.normalSelect(among=dict(tests=tests, **box), what=nr.ESTIMATED, count=True, result=True, cell=sc.R_EDGE, **kw)
        assert np.array_equal(rows, nr.listed(want, nr.ESTIMATED)) and mask[rows].all()
        check_result(res, want["result"], total, f"among tests={tests:#x}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# lists, device variants
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_list_and_its_conventions(edge):
    from elasticfusion_amd import api
    ef, S = edge["ef"], edge["S"]
    kw = dict(radius=sc.R_EDGE, k=8, max_curvature=0.01)
    want = nr.estimate(S, nl=edge["nl"][-1.0], **kw)
    M = ef.downloadMap()
    for what in WHATS:
        exp = nr.listed(want, what)
        rows, total, res = ef.normalSelect(what=what, count=True, result=True, cell=sc.R_EDGE, **kw)
        assert total == len(exp) > 5 and np.array_equal(rows, exp), what
        check_result(res, want["result"], total, f"what={what}")
        none, t0 = ef.normalSelect(what=what, max_rows=0, count=True, cell=sc.R_EDGE, **kw)            # NULL rows with max_rows 0
        assert len(none) == 0 and t0 == total
        assert_bits_equal(ef.gatherSurfels(rows), M[exp], f"the list of what={what} is what gatherSurfels takes")
    prm = ef.normalParams(cell=sc.R_EDGE, **kw)
    full = nr.listed(want, nr.ESTIMATED)
    rows = np.full(16, 0xABCD1234, np.uint32)
    cnt = C.c_uint32(0)
    api._chk(api.lib().ef_map_normals_select(ef.h, C.byref(prm), None, nr.ESTIMATED, api._ptr(rows), 7, C.byref(cnt), None), ef.h)
    assert cnt.value == len(full) and np.array_equal(rows[:7], full[:7]) and (rows[7:] == 0xABCD1234).all()


def test_device_variants_equal_the_host_variants(edge):
    from elasticfusion_amd import api
    ef, S = edge["ef"], edge["S"]
    n = len(S)
    v = [float(x) for x in S[edge["marks"]["at_view"], :3]]
    for kw in (dict(radius=sc.R_EDGE, cell=sc.R_EDGE, k=8), dict(radius=sc.R_EDGE, cell=sc.R_EDGE / 2, k=16, orientation=nr.VIEWPOINT, viewpoint=v)):
        prm = ef.normalParams(**kw)
        host = ef.estimateNormals(prm)
        d = dict(normals=api.DevBuf((n + 2) * 12, fill=0xEE), curvature=api.DevBuf((n + 2) * 4, fill=0xEE), spacing=api.DevBuf((n + 2) * 4, fill=0xEE),
                 count=api.DevBuf((n + 2) * 4, fill=0xEE), status=api.DevBuf(n + 2, fill=0xEE))
        ef.estimateNormalsDevice(prm, None, d["normals"].p, d["curvature"].p, d["spacing"].p, d["count"].p, d["status"].p, n + 2)
        ef.synchronize()
        for key, words in (("normals", 3), ("curvature", 1), ("spacing", 1), ("count", 1)):
            got = d[key].to_array(np.uint32, (n + 2) * words)
            assert np.array_equal(got[:n * words], host[key].reshape(-1).view(np.uint32)) and (got[n * words:] == 0xEEEEEEEE).all(), key
        got = d["status"].to_array(np.uint8, n + 2)
        assert np.array_equal(got[:n], host["status"]) and (got[n:] == 0xEE).all()
        ef.estimateNormalsDevice(prm, None, None, d["curvature"].p, None, None, None, 5)               # any array may be missing
        ef.synchronize()
        for what in (nr.ESTIMATED, nr.FLAT):
            rows, total, res = ef.normalSelect(prm, what=what, count=True, result=True)
            d_rows, d_cnt, d_res = api.DevBuf(n * 4, fill=0xEE), api.DevBuf(16), api.DevBuf(C.sizeof(api.ef_normal_result))
            ef.normalSelectDevice(prm, None, what, d_rows.p, n, d_cnt.p, d_res.p)
            ef.synchronize()
            assert int(d_cnt.to_array(np.uint32, 1)[0]) == total
            got = d_rows.to_array(np.uint32, n)
            assert np.array_equal(got[:total], rows) and (got[total:] == 0xEEEEEEEE).all()
            raw = d_res.to_array(np.uint8, C.sizeof(api.ef_normal_result)).tobytes()
            assert ef._normalResult(api.ef_normal_result.from_buffer_copy(raw)) == res
            ef.normalSelectDevice(prm, None, what, None, 0, d_cnt.p)                                     # no list, no result
            ef.synchronize()
            assert int(d_cnt.to_array(np.uint32, 1)[0]) == total


# ---------------------------------------------------------------------------------------------------------------------------------------
# the write-back
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", (dict(), dict(set_radius=1, radius_scale=0.75), dict(orientation=nr.VIEWPOINT, side=-1, set_radius=1)),
                         ids=("keep-side", "radius", "viewpoint"))
def test_the_write_back_changes_the_estimated_normals_and_nothing_else(kw):
    from elasticfusion_amd import accuracy, api
    S, m = sc.edge_scene()
    S[:, 5] = np.arange(1, len(S) + 1, dtype=np.uint32).view(F)              # bits in the ID lane, both times and the colour differ by row
    S[:, 6], S[:, 7], S[:, 4] = np.arange(len(S)) % 7, 7 + np.arange(len(S)) % 5, np.arange(len(S)) * 31.0
    if "orientation" in kw:
        kw = dict(kw, viewpoint=[float(x) for x in S[m["at_view"], :3]])
    kw = dict(kw, radius=sc.R_EDGE, k=8)
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        want = nr.estimate(S, **kw)
        W = nr.written(S, want)
        est = want["status"] == nr.ESTIMATED
        assert_bits_equal(accuracy.estimated_normals(ef, cell=sc.R_EDGE, **kw), W[est], "estimated_normals gathers what the write-back leaves")
        assert_bits_equal(ef.downloadMap(), S, "estimated_normals changes nothing")
        res = ef.reestimateNormals(cell=sc.R_EDGE, **kw)
        check_result(res, want["result"], want["result"]["estimated"], str(kw))
        got = ef.downloadMap()
        assert ef.lastCount() == len(S)
        assert np.array_equal(u32(got), u32(W)), np.nonzero(u32(got) != u32(W))
        changed = u32(got) != u32(S)
        assert not changed[~est].any() and not changed[:, :8].any() and changed[est, 8:11].any(1).sum() > 300
        assert changed[est, 11].all() if kw.get("set_radius") else not changed[:, 11].any()
        if kw.get("orientation", nr.KEEP_SIDE) == nr.KEEP_SIDE:              # idempotent bit for bit
            again = ef.reestimateNormals(cell=sc.R_EDGE, **kw)
            assert again == res and np.array_equal(u32(ef.downloadMap()), u32(W))        # (the same rows are turned again: the stored side is theirs)
            assert again == dict(nr.estimate(W, **kw)["result"], listed=res["listed"])
    finally:
        ef.close()


def test_write_back_then_mapping_equals_upload_and_restore(sixteen):
    from elasticfusion_amd import api
    fr = sixteen

    def feed(ef, k):
        ef.processFrame(fr[k][0], fr[k][1], k * 33333)

    a, b, plain = api.ElasticFusion(), api.ElasticFusion(), api.ElasticFusion()
    try:
        for k in range(12):
            feed(a, k)
            feed(plain, k)
        m12 = a.downloadMap()
        ck = a.checkpoint(fr[11][0], fr[11][1])
        kw = dict(radius=0.01, cell=0.01, k=8)
        est = a.estimateNormals(**kw)                                        # (the device's own estimate: the reference is quadratic in the map)
        done = est["status"] == nr.ESTIMATED
        res = a.reestimateNormals(**kw)
        print("frame 12: surfels", len(m12), res)
        assert res["estimated"] == int(done.sum()) > len(m12) // 2 and res["listed"] == res["estimated"]
        W = m12.copy()
        W[done, 8:11] = est["normals"][done]
        got = a.downloadMap()
        assert np.array_equal(u32(got), u32(W)) and (u32(got) != u32(m12)).any(1).sum() > len(m12) // 4
        assert a.getTick() == ck["tick"] and np.array_equal(a.getPoseQT(), ck["qt"])
        ck["map"] = W
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
        assert mp.shape != ma.shape or not np.array_equal(u32(mp), u32(ma)), "the write-back mattered"
    finally:
        for ef in (a, b, plain):
            ef.close()


def test_a_loop_closing_context_refuses_the_write_back_only():
    from elasticfusion_amd import api
    S, _ = sc.edge_scene()
    ef = api.ElasticFusion(closeLoops=True)
    try:
        ef.uploadMap(S)
        assert "close_loops" in refused(lambda: ef.reestimateNormals(radius=sc.R_EDGE, cell=sc.R_EDGE), -4)        # EF_ESTATE
        assert ef.lastCount() == len(S)
        assert_bits_equal(ef.downloadMap(), S, "a refused write-back")
        kw = dict(radius=sc.R_EDGE, k=8)
        want = nr.estimate(S, **kw)
        check_rows(ef.estimateNormals(cell=sc.R_EDGE, **kw), want, "estimate on a loop-closing context")
        assert np.array_equal(ef.normalSelect(what=nr.DEGENERATE, cell=sc.R_EDGE, **kw), nr.listed(want, nr.DEGENERATE))
        refused(lambda: ef.estimateNormals(k=2), -1)                                                                 # EF_EINVAL
        refused(lambda: ef.normalSelect(what=0), -1)
        refused(lambda: ef.estimateNormals(radius=1.0, cell=0.01), -1)
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# end to end: a cloud without normals
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", (False, True), ids=("by-time", "by-id"))
def test_insert_cloud_gives_a_position_only_patch_its_normals_and_radii(ids):
    from elasticfusion_amd import accuracy, api
    S, radial = sc.sphere_scene()
    patch = radial[:, 2] > 0.8                                               # a cap of the sphere comes as bare points; the map holds the rest
    assert 150 < patch.sum() < 400
    old, pts = S[~patch], S[patch, :3]
    centre = np.zeros(3)
    ef = api.ElasticFusion()
    try:
        if ids:
            ef.setSurfelIds(True)
        ef.uploadMap(old)
        kw = dict(radius=sc.R_SPHERE, cell=sc.R_SPHERE, k=12, radius_scale=0.5)
        sep = 0.0005                                                         # (random points: a few lie within the default centimetre of an old row)
        ins, res = accuracy.insert_cloud(ef, pts, viewpoint=centre, side=-1, min_separation=sep, **kw)       # away from the centre: outward
        tick = ef.getTick()
        rec = np.zeros((len(pts), 12), F)
        rec[:, :3], rec[:, 3], rec[:, 4], rec[:, 11] = pts, F(ef.getConfidenceThreshold()) + F(1), F(0x808080), F(accuracy.CLOUD_RADIUS)
        prm = ir.default_params(tick, min_normal_cos=-1.0, min_separation=sep)
        exp = ir.insert(old, rec, None, prm)
        assert ins == exp["result"] and ins["inserted"] == len(pts)
        mid = exp["map"]
        new = np.arange(len(mid)) >= len(old)
        del kw["cell"]
        want = nr.estimate(mid, among=new, orientation=nr.VIEWPOINT, side=-1, viewpoint=centre, set_radius=1, **kw)
        check_result(res, want["result"], want["result"]["estimated"], "insert_cloud")
        W = nr.written(mid, want)
        got = ef.downloadMap()
        if ids:
            assert (u32(got)[:, 5] != 0).all()
            got[:, 5] = 0                                                    # (the IDs are the numbering's, not the insert's or the estimate's)
        assert np.array_equal(u32(got[:len(old)]), u32(old)), "the old rows keep every bit"
        assert np.array_equal(u32(got), u32(W))
        assert res["estimated"] == len(pts) and res["participants"] == len(pts)
        n = got[new, 8:11].astype(np.float64)
        ang = np.degrees(np.arccos(np.clip((n * radial[patch]).sum(1), -1, 1)))           # the full angle: the side counts too
        print("inserted", len(pts), "angle to the radial direction: median %.3f max %.3f degrees" % (np.median(ang), ang.max()))
        assert ang.max() <= 1.5 * 6.145                                      # the CPU test's bar
        assert (got[new, 11] > 0.002).all() and (got[new, 11] < 0.03).all()
    finally:
        ef.close()
