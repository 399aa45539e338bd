"""Carve free space on the device (ef_map_carve / ef_map_carve_select, include/ef_hip.h; the kernel in elasticfusion_amd/csrc/ef_carve.inc;
DESIGN.md §8h).

The operation is restated in numpy from the header alone (tests/carveref.py).  A row's outcome is a pure function of the row, the views and
the parameters (no sums, no order dependence), so everything is compared BIT FOR BIT: the removed rows, the vote bytes, the counts, the result
and the map a carve leaves.  There is no tolerance anywhere.  The hand-built scenes use a 33 x 17 image (odd width: an image row is only
2-byte aligned) with power-of-two intrinsics and the identity pose, so that the projection of a chosen point is exact and the expected votes
can be written down by hand beside the reference's."""
import ctypes as C
import os

import numpy as np
import pytest

import carveref as cr
import selectref as sr
from queryref import assert_bits_equal
from test_carve_host import OWN_ROWS_REMOVED_CAP, POSES, pose, surfels_at
from test_gpu_select import refused, state_of, step, to_api, u32

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 33, 17
CAM = dict(width=W, height=H, fx=16.0, fy=16.0, cx=16.0, cy=8.0)
EYE = np.eye(4)
NC = 4


@pytest.fixture(scope="module")
def ctx():
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    yield ef
    ef.close()


def api_params(ef, p):
    return ef.carveParams(**{k: (int(p[k]) if k in ("width", "height", "window", "min_views", "protect") else float(p[k])) for k in cr.FIELDS})


def check(ef, S, depths, poses, p, among=None, probs=None, what=""):
    """the removed rows, their count and the vote bytes of the host tier against the reference; returns the reference"""
    c = cr.carve(S, depths, poses, p, among, probs)
    a = None if among is None else to_api(ef, among)
    rows, total, votes = ef.carveSelect(np.asarray(depths, np.uint16), np.asarray(poses, np.float64), api_params(ef, p), a, count=True, votes=True)
    assert total == c["result"]["removed"], (what, total, c["result"])
    assert rows.dtype == np.uint32 and np.array_equal(rows, c["rows"]), (what, np.setxor1d(rows, c["rows"])[:8])
    bad = np.nonzero((votes != c["votes"]).any(1))[0]
    assert votes.shape == c["votes"].shape and not len(bad), (what, bad[:8], votes[bad[:8]].tolist(), c["votes"][bad[:8]].tolist())
    return c


def at_texel(u, v, z, p=CAM):
    """the point whose projection is exactly (u, v) (floats) at depth z, for the identity pose: fx, fy, cx, cy are small powers of two or
    integers and the u, v, z used here have short mantissas, so that every operation of the projection is exact"""
    z = F(z)
    return [(F(u) - F(p["cx"])) / F(p["fx"]) * z, (F(v) - F(p["cy"])) / F(p["fy"]) * z, z]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. hand-built rows
# ---------------------------------------------------------------------------------------------------------------------------------------
PROJECTION = [  # (name, point, the votes {free, support} worked out by hand: the image is a wall at 2 m, the points lie at 1 m)
    ("uf exactly 0", at_texel(0.0, 8.5, 1.0), (1, 0)),
    ("uf just below 0", [step(-1.0, False), F(0.03125), F(1.0)], (0, 0)),
    ("uf = -0.5: no truncation to 0", at_texel(-0.5, 8.5, 1.0), (0, 0)),
    ("u = W - 1", at_texel(32.0, 8.5, 1.0), (1, 0)),
    ("uf = W - 0.5", at_texel(32.5, 8.5, 1.0), (1, 0)),
    ("uf = W exactly", at_texel(33.0, 8.5, 1.0), (0, 0)),
    ("vf exactly 0", at_texel(16.5, 0.0, 1.0), (1, 0)),
    ("vf just below 0", [F(0.03125), step(-0.5, False), F(1.0)], (0, 0)),
    ("v = H - 1", at_texel(16.5, 16.0, 1.0), (1, 0)),
    ("vf = H exactly", at_texel(16.5, 17.0, 1.0), (0, 0)),
    ("z = 0", [0.0, 0.0, 0.0], (0, 0)),
    ("z = -0", [0.0, 0.0, -0.0], (0, 0)),
    ("z < 0", [0.25, 0.25, -1.0], (0, 0)),
    ("z = 1e-38, off axis: uf is inf", [0.5, 0.0, 1e-38], (0, 0)),
    ("z = 1e-38, on the axis: the centre texel", [0.0, 0.0, 1e-38], (1, 0)),
    ("x NaN", [np.nan, 0.0, 1.0], (0, 0)),
    ("y +inf", [0.0, np.inf, 1.0], (0, 0)),
    ("z -inf", [0.0, 0.0, -np.inf], (0, 0)),
    ("z +inf", [0.0, 0.0, np.inf], (0, 0)),
    ("1e12 m off axis: uf beyond int", [1e12, 0.0, 1.0], (0, 0)),
    ("-1e12 m off axis", [-1e12, -1e12, 1.0], (0, 0)),
    ("1e12 m away, inside the image: occluded by the wall", [1e12, 0.0, 1e12], (0, 0)),
    ("on the wall", at_texel(16.5, 8.5, 2.0), (0, 1)),
    ("behind the wall", at_texel(16.5, 8.5, 2.5), (0, 0)),
]


def test_projection_edges(ctx):
    S = surfels_at(np.array([pt for _, pt, _ in PROJECTION], F))
    ctx.uploadMap(S)
    depth = np.full((H, W), 2000, np.uint16)
    for w in (0, 1, 2):
        p = cr.default_params(**CAM, window=w)
        c = check(ctx, S, [depth], [EYE], p, what=f"projection, window {w}")
        for k, (name, _, want) in enumerate(PROJECTION):
            assert tuple(c["votes"][k]) == want, (name, w, c["votes"][k])
    # the same rows seen from a camera that is not at the origin: T_cw is formed from T_wc on the host, in double
    for T in POSES[1:]:
        check(ctx, S, [depth], [T], cr.default_params(**CAM), what="projection, moved camera")


def test_depth_texel_edges(ctx):
    """one texel per case along image row 8, the surfels at 0.125 m (window 0: the centre texel alone decides)"""
    texels = [(0, "no data", (0, 0)), (65535, "beyond max_depth", (0, 0)), (299, "just inside min_depth's outside", (0, 0)),
              (300, "min_depth itself", (1, 0)), (3000, "max_depth itself", (1, 0)), (3001, "just outside max_depth", (0, 0)), (1, "1 mm", (0, 0))]
    depth = np.full((H, W), 2000, np.uint16)
    for k, (d, _, _) in enumerate(texels):
        depth[8, 2 + 3 * k] = d
    S = surfels_at(np.array([at_texel(2.5 + 3 * k, 8.5, 0.125) for k in range(len(texels))], F))
    ctx.uploadMap(S)
    p = cr.default_params(**CAM, window=0, min_depth=0.3, max_depth=3.0)
    assert F(300) / F(1000) == F(0.3) and F(3000) / F(1000) == F(3.0)
    c = check(ctx, S, [depth], [EYE], p, what="texels")
    for k, (d, name, want) in enumerate(texels):
        assert tuple(c["votes"][k]) == want, (name, c["votes"][k])
    # with a window of 1 the neighbours (the wall) have data: a centre without data still says nothing, a hole beside a centre is ignored
    S2 = surfels_at(np.array([at_texel(2.5 + 3 * k + 1, 8.5, 0.125) for k in range(len(texels))], F))
    ctx.uploadMap(S2)
    c = check(ctx, S2, [depth], [EYE], dict(p, window=1), what="beside the texels")
    assert [tuple(v) for v in c["votes"]] == [(1, 0)] * len(texels)     # (0.3 m and 1 mm texels beside them: no data or behind ... all FREE)
    # 65535 mm is data under a far cut-off
    ctx.uploadMap(S)
    c = check(ctx, S, [depth], [EYE], dict(p, max_depth=100.0), what="far cut-off")
    assert tuple(c["votes"][1]) == (1, 0) and tuple(c["votes"][5]) == (1, 0)


def test_threshold_equalities(ctx):
    """(z + tol) == zo exactly: not FREE, SUPPORTED.  (zo + tol) == z exactly: SUPPORTED, and one float further it is occluded.  The depths come
    from the reference's own f32 values; the identity pose makes z the stored coordinate."""
    p = cr.default_params(**CAM, window=0)
    pts, want = [], []
    for d in (700, 1000, 1234, 2000, 2999):
        zo = F(d) / F(1000)
        tol = cr.tol(zo, p)
        near = [z for z in (F(zo - tol) + F(k) * np.spacing(F(zo - tol)) for k in range(-3, 4)) if F(F(z) + tol) == zo]
        assert near, d                                   # some float z has fl(z + tol) == zo
        z_eq = F(min(near))
        z_free = step(z_eq, False)
        assert F(z_free + tol) < zo
        z_far = F(zo + tol)                              # fl(zo + tol) == z: not in front
        pts += [(d, z_free), (d, z_eq), (d, z_far), (d, step(z_far, True))]
        want += [(1, 0), (0, 1), (0, 1), (0, 0)]
    depth = np.full((H, W), 0, np.uint16)
    S = np.zeros((len(pts), 3), F)
    for k, (d, z) in enumerate(pts):
        u, v = 1 + k % 31, 1 + 2 * (k // 31)
        depth[v, u] = d
        S[k] = [(F(u + 0.5) - F(16)) / F(16) * z, (F(v + 0.5) - F(8)) / F(16) * z, z]      # (anywhere inside its texel will do)
    S = surfels_at(S)
    ok, z, u, v, _, _ = cr.project(S[:, :3], EYE, p)
    assert ok.all() and np.array_equal(z, S[:, 2]) and np.array_equal(depth[v, u], [d for d, _ in pts])
    ctx.uploadMap(S)
    c = check(ctx, S, [depth], [EYE], p, what="thresholds")
    assert [tuple(x) for x in c["votes"]] == want, c["votes"].tolist()


def window_scene():
    """a wall at 2 m; one nearer texel at (10, 8), a hole at (20, 8), a nearer texel diagonal to the corner (0, 0) and one two texels from the
    corner (32, 16); surfels at 1 m on the texels around them and in all four corners"""
    depth = np.full((H, W), 2000, np.uint16)
    depth[8, 10] = 900
    depth[8, 20] = 0
    depth[1, 1] = 900
    depth[16, 30] = 900
    at = [(9, 8), (11, 8), (10, 7), (10, 10), (12, 8), (10, 8), (19, 8), (20, 8), (0, 0), (32, 0), (0, 16), (32, 16), (31, 15)]
    S = surfels_at(np.array([at_texel(u + 0.5, v + 0.5, 1.0) for u, v in at], F))
    # FREE per window 0, 1, 2, by hand: a nearer texel inside the window silences the view, a hole is ignored, (10, 8) itself is in FRONT of
    # its texel (0.9 m: occluded), (20, 8) has no data
    free = {(9, 8): (1, 0, 0), (11, 8): (1, 0, 0), (10, 7): (1, 0, 0), (10, 10): (1, 1, 0), (12, 8): (1, 1, 0), (10, 8): (0, 0, 0), (19, 8): (1, 1, 1),
            (20, 8): (0, 0, 0), (0, 0): (1, 0, 0), (32, 0): (1, 1, 1), (0, 16): (1, 1, 1), (32, 16): (1, 1, 0), (31, 15): (1, 0, 0)}
    return S, depth, [free[a] for a in at]


def test_windows_holes_and_corners(ctx):
    S, depth, free = window_scene()
    ctx.uploadMap(S)
    for w in (0, 1, 2):
        c = check(ctx, S, [depth], [EYE], cr.default_params(**CAM, window=w), what=f"window {w}")
        assert c["free"].tolist() == [f[w] for f in free], (w, c["free"].tolist())
        assert not c["support"].any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. sizes
# ---------------------------------------------------------------------------------------------------------------------------------------
def random_case(n, w, h, K, seed):
    """n surfels 0.5 .. 3 m in front of K cameras that look along z from nearby, images of a mix of holes, near, far and matching depths"""
    rng = np.random.default_rng(seed)
    p = cr.default_params(width=w, height=h, fx=0.8 * w, fy=0.8 * w, cx=w / 2, cy=h / 2, window=int(rng.integers(0, 3)))
    z = rng.uniform(0.5, 3.0, n)
    S = surfels_at(np.stack([rng.uniform(-0.7, 0.7, n) * z, rng.uniform(-0.7, 0.7, n) * z * h / w, z], 1))
    poses = np.stack([pose(*rng.uniform(-0.05, 0.05, 3), yaw=rng.uniform(-0.05, 0.05)) for _ in range(K)])
    D = rng.choice(np.array([0, 400, 1000, 1500, 2000, 2500, 3000, 3100], np.uint16), (K, h, w))
    return S, D, poses, p


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 257, 1000))
def test_sizes(ctx, n):
    seen = np.zeros(2, int)
    for (w, h) in ((1, 1), (5, 3), (64, 48)):
        for K in (1, 3, 32):
            S, D, poses, p = random_case(n, w, h, K, seed=n * 100 + w + K)
            ctx.uploadMap(S)
            assert ctx.lastCount() == n
            for kw in (dict(), dict(min_views=(K + 1) // 2, protect=0)):
                c = check(ctx, S, D, poses, dict(p, **kw), what=f"n {n}, {w} x {h}, K {K} {kw}")
                seen += (int(c["free"].sum()), int(c["support"].sum()))
    assert n < 63 or (seen > 0).all(), seen


def test_thirty_two_views_one_short_and_the_veto(ctx):
    depth = np.full((32, H, W), 2000, np.uint16)
    depth[7, 8, 4] = 0                      # row 0's texel is a hole in view 7: 31 FREE views
    depth[11, 8, 12] = 1000                 # row 2 is measured where it is by view 11: 31 FREE, 1 SUPPORTED
    S = surfels_at(np.array([at_texel(4.5, 8.5, 1.0), at_texel(8.5, 8.5, 1.0), at_texel(12.5, 8.5, 1.0)], F))
    ctx.uploadMap(S)
    poses = [EYE] * 32
    p = cr.default_params(**CAM, window=0, min_views=32)
    c = check(ctx, S, depth, poses, p, what="min_views 32")
    assert c["votes"].tolist() == [[31, 0], [32, 0], [31, 1]] and c["rows"].tolist() == [1]
    c = check(ctx, S, depth, poses, dict(p, min_views=31), what="min_views 31, protect")
    assert c["rows"].tolist() == [0, 1] and c["result"]["protected_"] == 1
    c = check(ctx, S, depth, poses, dict(p, min_views=31, protect=0), what="min_views 31, no protection")
    assert c["rows"].tolist() == [0, 1, 2]


def raw_select(ef, D, poses, prm, rows, max_rows, among=None):
    """ef_map_carve_select on a caller's rows array (or None): the return code and the count"""
    from elasticfusion_amd import api
    T = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
    D = np.ascontiguousarray(D, np.uint16)
    views = api.ef_carve_views(len(T), T.ctypes.data, D.ctypes.data)
    total = C.c_uint32(0xFFFFFFFF)
    rc = api.lib().ef_map_carve_select(ef.h, C.byref(prm), C.byref(views), among, None if rows is None else rows.ctypes.data_as(C.c_void_p),
                                       C.c_uint32(max_rows), C.byref(total), None)
    return rc, total.value


def test_max_rows_smaller_than_the_total(ctx):
    S, D, poses, p = random_case(1000, 64, 48, 3, seed=77)
    ctx.uploadMap(S)
    c = cr.carve(S, D, poses, p)
    total = c["result"]["removed"]
    assert total > 20
    prm = api_params(ctx, p)
    for cap in (0, 1, total - 1, total, total + 5):
        rows = np.full(total + 8, 0xDEADBEEF, np.uint32)
        rc, got = raw_select(ctx, D, poses, prm, rows, cap)
        assert rc == 0 and got == total, (cap, rc, got)
        k = min(cap, total)
        assert np.array_equal(rows[:k], c["rows"][:k]) and (rows[k:] == 0xDEADBEEF).all(), cap      # the prefix; the rest as it was
    rc, got = raw_select(ctx, D, poses, prm, None, 0)                                               # a count only
    assert rc == 0 and got == total
    assert np.array_equal(ctx.carveSelect(D, poses, prm, max_rows=7), c["rows"][:7])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. among
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_among_limits_the_participants():
    from elasticfusion_amd import api
    S, D, poses, p = random_case(2100, 64, 48, 3, seed=5)
    p = dict(p, window=0)               # (the images are noise: a wider window leaves few FREE rows to tell the selections apart)
    rng = np.random.default_rng(6)
    S[:, 3] = rng.integers(0, 10, len(S))
    S[50:50 + 4 * 300:300, :3] = np.array([[np.nan, 0, 1], [0, np.inf, 1], [0, 0, -np.inf], [np.nan, np.nan, np.nan]], F)
    P = rng.dirichlet(np.ones(NC), len(S)).astype(F)
    ef = api.ElasticFusion()
    try:
        ef.setSurfelIds(True)
        ef.enableLabels(NC)
        ef.uploadMap(S)
        ef.setLabels(P)
        M = ef.downloadMap()            # (the rows are numbered)
        assert (u32(M[:, 5]) > 0).all()
        among = dict(
            conf=sr.default_selection(tests=sr.CONF, conf_min=0.0, conf_max=6.0),
            box=sr.default_selection(tests=sr.BOX, T_bw=pose(0.01, -0.02, 0.03, yaw=0.3), box_min=[-np.inf, -0.4, -np.inf], box_max=[0.3, np.inf, 2.0]),
            inverted=sr.default_selection(tests=sr.CONF | sr.INVERT, conf_min=3.0, conf_max=5.0),
            nothing=sr.default_selection(tests=sr.INVERT),
            ids=sr.default_selection(tests=sr.ID, id_min=400, id_max=1800),
            label=sr.default_selection(tests=sr.LABEL, label_class=2, label_min_prob=0.3),
            id_conf_label=sr.default_selection(tests=sr.ID | sr.CONF | sr.LABEL, id_min=100, conf_min=2.0, label_class=1),
        )
        free_of_all = cr.carve(M, D, poses, dict(p, protect=0))
        for name, a in among.items():
            c = check(ef, M, D, poses, dict(p, protect=0), a, P, what=name)
            out = ~sr.select_mask(M, a, P)
            print(name, c["result"])
            assert (c["votes"][out] == 0).all() and c["kept"][out].all()                  # non-participants are untouched
            assert np.array_equal(c["votes"][~out], free_of_all["votes"][~out])             # participants vote as without among
            assert name == "nothing" or 0 < c["result"]["removed"] < free_of_all["result"]["removed"]
        assert not free_of_all["part"][50:50 + 4 * 300:300].any()
        # a dict of mapSelection keywords is accepted as well
        a = among["conf"]
        rows = ef.carveSelect(D, poses, api_params(ef, dict(p, protect=0)), among=dict(tests=sr.CONF, conf_min=0.0, conf_max=6.0))
        assert np.array_equal(rows, cr.carve(M, D, poses, dict(p, protect=0), a)["rows"])
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. tiers
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_host_and_device_tiers_agree_and_views_add_up(ctx):
    from elasticfusion_amd import accuracy, api
    S, D, poses, p = random_case(5000, 64, 48, 5, seed=31)
    n = len(S)
    ctx.uploadMap(S)
    prm = api_params(ctx, dict(p, min_views=2))
    c = cr.carve(S, D, poses, dict(p, min_views=2))
    rows, total, votes = ctx.carveSelect(D, poses, prm, count=True, votes=True)
    assert total == len(c["rows"]) > 10 and np.array_equal(rows, c["rows"]) and np.array_equal(votes, c["votes"])
    # the _dev tier only enqueues: two calls back to back into two sets of buffers (the second with other views), one synchronise
    d_img, d_img2 = api.DevBuf.from_array(D), api.DevBuf.from_array(D[::-1].copy())
    out = [(api.DevBuf(n * 4), api.DevBuf(16), api.DevBuf(n * 2)) for _ in range(2)]
    ctx.carveSelectDevice(d_img.p, poses, prm, None, out[0][0].p, n, out[0][1].p, out[0][2].p)
    ctx.carveSelectDevice(d_img2.p, poses[::-1].copy(), prm, None, out[1][0].p, n, out[1][1].p, out[1][2].p)
    ctx.synchronize()
    for r, cnt, v in out:          # (the reversed views are the same views: the same votes)
        assert int(cnt.to_array(np.uint32, (4,))[0]) == total
        assert np.array_equal(r.to_array(np.uint32, (n,))[:total], rows) and np.array_equal(v.to_array(np.uint8, (n, 2)), votes)
    # K images in one call = the K calls' votes summed
    summed = np.zeros((n, 2), int)
    for k in range(len(D)):
        _, v = ctx.carveSelect(D[k], poses[k:k + 1], api_params(ctx, p), votes=True)
        summed += v
    assert np.array_equal(summed, votes)
    # carved_map: the map without the carved rows, the context unchanged; the device-image tier of the carve itself
    assert_bits_equal(accuracy.carved_map(ctx, D, poses, params=prm), S[c["kept"]], "carved_map")
    assert ctx.lastCount() == n
    res = ctx.carveSurfels(d_img, poses, prm)
    assert res == c["result"], (res, c["result"])
    assert_bits_equal(ctx.downloadMap(), S[c["kept"]], "ef_map_carve_dev")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the erase, 7. the workload's size
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def six(seq):
    return [seq.frame(k) for k in range(7)]


def phantom_blob(T, n=500, seed=12):
    """n surfels 0.5 m in front of the camera at T: where something stood that the camera now looks through"""
    rng = np.random.default_rng(seed)
    cam = np.stack([rng.uniform(-0.25, 0.25, n), rng.uniform(-0.2, 0.2, n), np.full(n, 0.5)], 1)
    S = surfels_at((T[:3, :3] @ cam.T).T + T[:3, 3])
    S[:, 4] = 0x808080
    return S


def test_carve_equals_erase_rows_of_the_selection(six):
    from elasticfusion_amd import api
    fr = six
    a, b = api.ElasticFusion(), api.ElasticFusion()
    try:
        for ef in (a, b):
            ef.setSurfelIds(True)
            ef.enableLabels(NC)
            for k in range(6):
                ef.processFrame(fr[k][0], fr[k][1], k * 33333)
            ins = ef.insertSurfels(phantom_blob(ef.get_T_wc()), gate=0)
            assert ins["inserted"] == 500
        M = a.downloadMap()
        assert_bits_equal(b.downloadMap(), M, "the twins before the carve")
        T = a.get_T_wc()
        depth = fr[5][1]
        p = cr.default_params()
        c = cr.carve(M, [depth], [T], p)
        res = a.carveSurfels(depth)                         # the current pose, the defaults
        print("surfels", len(M), res)
        assert res == c["result"], (res, c["result"])
        assert res["removed"] >= 400 and c["removed"][len(M) - 500:].sum() >= 400           # the phantoms go
        rows = b.carveSelect(depth)
        assert np.array_equal(rows, c["rows"])
        assert b.eraseRows(rows) == res["removed"]
        (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
        assert_bits_equal(ma, mb, "the map after the carve")
        assert_bits_equal(ma, M[c["kept"]], "the map after the carve against the reference")
        assert np.array_equal(a.surfelIds(), b.surfelIds()) and np.array_equal(a.surfelIds(), u32(M[c["kept"], 5]))
        assert_bits_equal(a.labels()[1], b.labels()[1], "labels")
        assert np.array_equal(qa.view(np.uint64), qb.view(np.uint64)) and a.getTick() == b.getTick()
        assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
        # removing nothing is valid: the phantoms are gone, the same view finds nothing more (a row's outcome depends on no other row)
        again = a.carveSurfels(depth)
        assert again["removed"] == 0 and again["count_after"] == res["count_after"], again
        assert b.eraseRows(b.carveSelect(depth)) == 0
        assert_bits_equal(a.downloadMap(), ma, "a carve that removes nothing")
        for ef in (a, b):
            ef.processFrame(fr[6][0], fr[6][1], 6 * 33333)
        (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
        assert np.array_equal(qa.view(np.uint64), qb.view(np.uint64)), (qa, qb)
        assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
        assert_bits_equal(ma, mb, "the map one frame later")
        assert np.array_equal(a.surfelIds(), b.surfelIds())
    finally:
        a.close()
        b.close()


def test_three_views_at_the_workloads_size(six):
    """640 x 480, K = 3 on the 6-frame map with the phantom blob: the one test at the workload's size.  The map's own rows that go are capped
    by what test_carve_host measured on the oracle's map (a condition on the outcome, not a tolerance of the comparison)."""
    from elasticfusion_amd import api
    fr = six
    ef = api.ElasticFusion()
    try:
        poses = []
        for k in range(6):
            ef.processFrame(fr[k][0], fr[k][1], k * 33333)
            poses.append(ef.get_T_wc())
        ef.insertSurfels(phantom_blob(poses[5]), gate=0)
        M = ef.downloadMap()
        D = np.stack([fr[k][1] for k in (3, 4, 5)])
        T = np.stack(poses[3:6])
        p = cr.default_params()
        c = cr.carve(M, D, T, p)
        rows, total, votes = ef.carveSelect(D, T, count=True, votes=True)
        own = int(c["removed"][:len(M) - 500].sum())
        print("surfels", len(M), c["result"], "own rows removed", own)
        assert total == c["result"]["removed"] and np.array_equal(rows, c["rows"]) and np.array_equal(votes, c["votes"])
        assert c["removed"][len(M) - 500:].sum() >= 400
        assert own <= OWN_ROWS_REMOVED_CAP, own
        assert ef.carveSurfels(D, T) == c["result"]
        assert_bits_equal(ef.downloadMap(), M[c["kept"]], "the carved map")
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. state refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_state_refusals():
    import ctypes.util
    from elasticfusion_amd import api
    S, D, poses, p = random_case(1000, 64, 48, 3, seed=77)
    c = cr.carve(S, D, poses, p)
    ef = api.ElasticFusion(closeLoops=True)
    try:
        ef.uploadMap(S)
        prm = api_params(ef, p)
        assert "close_loops" in refused(lambda: ef.carveSurfels(D, poses, prm), -4)          # EF_ESTATE
        assert "close_loops" in refused(lambda: ef.carveSurfels(api.DevBuf.from_array(D), poses, prm), -4)
        assert ef.lastCount() == 1000
        assert_bits_equal(ef.downloadMap(), S, "a refused carve leaves the map")
        assert np.array_equal(ef.carveSelect(D, poses, prm), c["rows"])                      # the select works there
    finally:
        ef.close()
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        prm = api_params(ef, p)
        assert "min_views" in refused(lambda: ef.carveSelect(D, poses, api_params(ef, dict(p, min_views=4))), -1)      # EF_EINVAL: above n
        assert "min_views" in refused(lambda: ef.carveSurfels(D, poses, api_params(ef, dict(p, min_views=4))), -1)
        assert "labels are off" in refused(lambda: ef.carveSelect(D, poses, prm, among=dict(tests=sr.LABEL)), -4)
        assert "labels are off" in refused(lambda: ef.carveSurfels(D, poses, prm, among=dict(tests=sr.LABEL)), -4)
        assert "IDs are off" in refused(lambda: ef.carveSurfels(D, poses, prm, among=dict(tests=sr.ID)), -4)
        refused(lambda: ef.carveSelect(D, poses, api_params(ef, dict(p, window=3))), -1)
        dflt = ef.carveParams()
        assert (dflt.width, dflt.height, dflt.fx, dflt.cy) == (640, 480, 528.0, 240.0)
        assert (dflt.min_depth, dflt.max_depth, dflt.margin, dflt.margin_quad) == tuple(float(F(v)) for v in (0.3, 3.0, 0.02, 0.0025))
        assert (dflt.window, dflt.min_views, dflt.protect) == (1, 1, 1)
        name = ctypes.util.find_library("amdhip64") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")
        hip = C.CDLL(name)
        s = C.c_void_p(ef.stream())
        d = api.DevBuf(64)
        d_img = api.DevBuf.from_array(D)
        ef.synchronize()
        assert hip.hipStreamBeginCapture(s, C.c_int(2)) == 0   # relaxed
        try:
            assert "captured" in refused(lambda: ef.carveSelect(D, poses, prm, max_rows=8), -4)
            assert "captured" in refused(lambda: ef.carveSelectDevice(d_img.p, poses, prm, None, d.p, 8, d.p), -4)
            assert "captured" in refused(lambda: ef.carveSurfels(D, poses, prm), -4)
        finally:
            g = C.c_void_p()
            assert hip.hipStreamEndCapture(s, C.byref(g)) == 0
            if g.value:
                hip.hipGraphDestroy(g)
        ef.synchronize()
        assert ef.lastCount() == 1000
        assert ef.carveSurfels(D, poses, prm) == c["result"]
    finally:
        ef.close()
