"""Hand-built edge scenes for the map prediction passes (k_index_splat / k_index_resolve, k_surface_splat / k_surface_resolve /
k_depth_resolve, k_fill_in, k_dense_count, k_seed_flags / k_seed_scatter), importable without a GPU.

A scene is a few surfel rows (N x 12 float32: position + confidence, packed colour / 0 / init time / last time, normal + radius), a pose,
the gate parameters and ONE image size, plus check(outputs): assertions on the ORACLE's result alone that the scene does what it was
written for (which id owns which pixel, how many pixels are drawn, which stay empty).  A scene is compared with the device only after its
check has passed (tests/test_gpu_predict_edges.py); tests/test_splat_scenes_host.py runs every check without a GPU.

fx = fy = 40, cx = W / 2, cy = H / 2 and the identity pose unless a scene says otherwise, so a point's camera-space position IS its row
and ((fx * x) / z) + cx is evaluated below exactly as the passes evaluate it (float32, one rounding per operation).

Surface scenes carry the surfel id in the confidence (conf = TAG + id, confThreshold far below): the vertex map's w channel names the
winner of every pixel.  TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import numpy as np

F = np.float32
FX = FY = 40.0
MAXD = 20.0
TD_OPEN = 2147483647 // 2
TAG = 10.0                       # surface scenes: confidence of surfel id = TAG + id
SIZES = ((36, 28), (52, 36), (12, 44))
GREY = float(0x808080)
INDEX_STRIDE = 1024 * 256        # lanes of the index splat's grid-stride loop
SURFACE_STRIDE = 1024 * 256      # surfels per trip of the surface splat (4096 workgroups x 256 lanes / 4 lanes per surfel)


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


def proj(x, z, f, c):
    """((f * x) / z) + c in float32, as index_map.vert / splat.vert evaluate it"""
    return F(F(F(F(f) * F(x)) / F(z)) + F(c))


def solve(target, z, f, c):
    """the float x whose projection is exactly `target`"""
    x = F((float(target) - c) / f * float(z))
    for _ in range(4096):
        u = proj(x, z, f, c)
        if u == F(target):
            return x
        x = up(x) if u < F(target) else down(x)
    raise AssertionError(f"no float projects onto {target}")


def step_until_changed(x, z, f, c, direction):
    """the float next to x (towards +/-inf) whose projection differs from x's"""
    u0, step = proj(x, z, f, c), (up if direction > 0 else down)
    for _ in range(4096):
        x = step(x)
        if proj(x, z, f, c) != u0:
            return x
    raise AssertionError("projection does not move")


def window_pixel(u, n):
    """N1: the pixel of window coordinate u on an axis of n pixels after index_map.vert's round trip through NDC (None: culled)"""
    half = F(F(n) * F(0.5))
    ndc = F(F(F(u) - half) / half)
    w = (float(ndc) + 1.0) * 0.5 * float(n)
    return int(np.floor(w)) if 0 <= w < n else None


def row(p, conf=TAG, colour=GREY, t_init=1, t_last=1, n=(0, 0, -1), rad=0.01):
    return np.array([p[0], p[1], p[2], conf, colour, 0, t_init, t_last, n[0], n[1], n[2], rad], F)


def culled_row():
    """a surfel beyond every maxDepth used here: keeps id 0 (== the index map's background) out of a scene"""
    return row((0, 0, 1000.0), t_last=1)


class SplatScene:
    """kind 'index': predict_indices -> (index, vertConf, colorTime, normRad)
    kind 'surface': combined_predict + synthesize_depth -> (image, vertex, normal, time, depth)"""

    def __init__(self, name, kind, W, H, rows, check, time=2, maxDepth=MAXD, conf=1.0, maxTime=None, timeDelta=TD_OPEN, cam=None, T=None):
        self.name, self.kind, self.W, self.H, self.check = name, kind, W, H, check
        self.surf = np.ascontiguousarray(np.asarray(rows, F).reshape(-1, 12))
        self.time, self.maxDepth, self.conf, self.timeDelta = time, maxDepth, conf, timeDelta
        self.maxTime = time if maxTime is None else maxTime
        self.cam = (W, H, FX, FY, W / 2.0, H / 2.0) if cam is None else cam
        self.T = np.eye(4) if T is None else T

    def run(self, be, cam):
        """be: the oracle module (tests/efo.py) or api.ops; cam: that backend's camera struct of self.cam"""
        if self.kind == "index":
            return be.predict_indices(cam, self.T, self.time, self.surf, self.maxDepth, self.timeDelta)
        out = be.combined_predict(cam, self.T, self.surf, self.maxDepth, self.conf, self.time, self.maxTime, self.timeDelta)
        d = be.synthesize_depth(cam, self.T, self.surf, self.maxDepth, self.conf, self.time, self.maxTime, self.timeDelta)
        return tuple(out) + (d,)

    def __repr__(self):
        return f"{self.name}@{self.W}x{self.H}"


def owners(out):
    """surface scenes: surfel id per pixel from the vertex map's confidence, -1 where nothing was drawn"""
    img, vt = out[0], out[1]
    drawn = img[..., 3] == 255
    own = np.where(drawn, vt[..., 3] - TAG, -1).astype(np.int64)
    assert np.array_equal(out[4].view(np.uint32), vt[..., 2].view(np.uint32)), "synthesized depth == the vertex map's z"
    return own


def centre(W, H, i, j, z, du=0.0, dv=0.0):
    """the point at depth z that projects onto pixel (i, j)'s centre plus (du, dv) pixels"""
    return ((i + 0.5 + du - W / 2.0) / FX * z, (j + 0.5 + dv - H / 2.0) / FY * z, z)


# ------------------------------------------------------------------------------------------------------------------------------------
# predict_indices
# ------------------------------------------------------------------------------------------------------------------------------------
def index_pixel_edges(W, H):
    """points whose window position falls on a pixel edge and one float to either side of it, in x and in y (N1)"""
    rows, want = [culled_row()], {}
    cx, cy = W / 2.0, H / 2.0
    lanes_y = iter(range(10, 19))            # x-edge points: one image row each
    lanes_x = iter(range(0, 9))              # y-edge points: one image column each
    straddles = 0
    for axis, n, c, edges in (("x", W, cx, (1, 7, W - 1)), ("y", H, cy, (1, 21, H - 1))):
        for k in edges:
            on = solve(k, 1.0, FX, c)
            trio = (step_until_changed(on, 1.0, FX, c, -1), on, step_until_changed(on, 1.0, FX, c, +1))
            us = [proj(x, 1.0, FX, c) for x in trio]
            assert us[0] < us[1] == F(k) < us[2] and us[2] - us[0] < 1e-5, us      # the nearest window positions a float x reaches
            pix = [window_pixel(u, n) for u in us]
            straddles += pix[0] == k - 1 and pix[2] == k
            for x, px in zip(trio, pix):
                lane = next(lanes_y if axis == "x" else lanes_x)
                other = (lane + 0.5 - (cy if axis == "x" else cx)) / FX
                rows.append(row((x, other, 1.0) if axis == "x" else (other, x, 1.0)))
                want[len(rows) - 1] = (lane, px) if axis == "x" else (px, lane)     # (row, column)
    assert straddles == 6, "every edge has a point in the pixel on either side of it"

    def check(out):
        idx = out[0]
        assert (idx > 0).sum() == len(want)
        for sid, (r, c) in want.items():
            assert idx[r, c] == sid, (sid, r, c)
    return SplatScene("index_pixel_edges", "index", W, H, rows, check)


def index_viewport_edges(W, H):
    """points on the four edges of the viewport: window coordinate 0 is kept, cols (rows) is culled, one float inside / outside"""
    rows, want, gone = [culled_row()], {}, []
    cx, cy = W / 2.0, H / 2.0
    # x-edge points on image rows 2, 4, 6, 8; y-edge points on image columns 10 .. 16, or 3 .. 9 where the image has only 12 columns
    for axis, n, c, lanes in (("x", W, cx, (2, 4, 6, 8)), ("y", H, cy, (10, 12, 14, 16) if W > 16 else (3, 5, 7, 9))):
        lo, hi = solve(0, 1.0, FX, c), solve(n, 1.0, FX, c)
        for lane, x in zip(lanes, (lo, step_until_changed(lo, 1.0, FX, c, -1), step_until_changed(hi, 1.0, FX, c, -1), hi)):
            px = window_pixel(proj(x, 1.0, FX, c), n)
            other = (lane + 0.5 - (cy if axis == "x" else cx)) / FX
            rows.append(row((x, other, 1.0) if axis == "x" else (other, x, 1.0)))
            if px is None:
                gone.append(len(rows) - 1)
            else:
                want[len(rows) - 1] = (lane, px) if axis == "x" else (px, lane)
    assert sorted(want) == [1, 3, 5, 7] and sorted(gone) == [2, 4, 6, 8], (want, gone)
    assert want[1][1] == 0 and want[3][1] == W - 1 and want[5][0] == 0 and want[7][0] == H - 1

    def check(out):
        idx = out[0]
        assert (idx > 0).sum() == len(want) and not np.isin(idx, gone).any()
        for sid, (r, c) in want.items():
            assert idx[r, c] == sid, (sid, r, c)
    return SplatScene("index_viewport_edges", "index", W, H, rows, check)


def index_gates(W, H):
    """p.z == maxDepth, +0, -0, slightly negative; time - t == timeDelta and one tick more"""
    time, td = 10, 3
    cases = [("z_at_max", F(MAXD), 9, True), ("z_past_max", up(MAXD), 9, False), ("z_plus_zero", F(0.0), 9, False),
             ("z_minus_zero", F(-0.0), 9, False), ("z_negative", F(-1e-30), 9, False), ("z_tiny", F(1e-30), 9, True),
             ("t_at_delta", F(1.0), time - td, True), ("t_past_delta", F(1.0), time - td - 1, False), ("plain", F(1.0), time, True)]
    rows, want, gone = [culled_row()], {}, []
    for k, (_, z, t, kept) in enumerate(cases):
        i, j = 1 + 2 * (k % 5), 3 + 4 * (k // 5)
        p = centre(W, H, i, j, float(z)) if z != 0 else (0.0 if k % 2 else 0.01, 0.0, z)    # z = 0: u is 0 / 0 or +/-inf, culled either way
        rows.append(row((p[0], p[1], z), t_last=t))
        (want.__setitem__(len(rows) - 1, (j, i)) if kept else gone.append(len(rows) - 1))

    def check(out):
        idx, vc = out[0], out[1]
        assert (idx > 0).sum() == len(want) and not np.isin(idx, gone).any()
        for sid, (r, c) in want.items():
            assert idx[r, c] == sid, (sid, r, c)
        assert vc[3, 1, 2] == F(MAXD)
    return SplatScene("index_gates", "index", W, H, rows, check, time=time, timeDelta=td)


def index_ties(W, H):
    """identical depths on one pixel (lowest id wins), a later id nearer by one ulp (it wins), surfel 0 winning a pixel"""
    z = F(1.25)
    rows = [row(centre(W, H, 2, 2, 1.0), conf=3)]                                   # 0: owns (2, 2): index 0 on a populated texel
    rows += [row(centre(W, H, 5, 3, z, du=d), conf=c) for d, c in ((0.2, 4), (-0.2, 5))]            # 1, 2: tie -> 1
    rows += [row(centre(W, H, 8, 5, z, dv=d), conf=c) for d, c in ((0.3, 6), (0.0, 7), (-0.3, 8))]  # 3, 4, 5: tie -> 3
    rows += [row(centre(W, H, 3, 9, z), conf=9), row(centre(W, H, 3, 9, down(z), du=0.1), conf=10)]  # 6, 7: 7 nearer by one ulp
    rows += [row(centre(W, H, 9, 9, down(z)), conf=11), row(centre(W, H, 9, 9, z, du=0.1), conf=12)]  # 8, 9: 8 nearer and earlier

    def check(out):
        idx, vc = out[0], out[1]
        assert idx[2, 2] == 0 and vc[2, 2, 2] == 1 and vc[2, 2, 3] == 3
        assert idx[3, 5] == 1 and idx[5, 8] == 3 and idx[9, 3] == 7 and idx[9, 9] == 8
        assert (vc[..., 2] != 0).sum() == 5 and (idx > 0).sum() == 4
    return SplatScene("index_ties", "index", W, H, rows, check)


def index_stride(W, H):
    """262 144 + 3 surfels: the last three are the second trip of the splat's grid-stride loop; all but a few dozen of the bulk fail
    the time gate (they lie NEARER than everything else on pixels all over the image: a gate that lets them through is seen)"""
    n, time, td = INDEX_STRIDE, 10, 3
    rng = np.random.RandomState(5)
    bulk = np.zeros((n + 3, 12), F)
    ii, jj = rng.randint(0, W, n), rng.randint(0, H, n)
    bulk[:n, 2] = 0.5
    bulk[:n, 0] = (ii + 0.5 - W / 2.0) / FX * 0.5
    bulk[:n, 1] = (jj + 0.5 - H / 2.0) / FY * 0.5
    bulk[:, 3], bulk[:, 4], bulk[:, 6], bulk[:, 7] = 5, GREY, 1, 1          # last time 1: 10 - 1 > 3
    bulk[:, 10], bulk[:, 11] = -1, 0.01
    live = [1, 63, 64, 255, 256, 1023, 65535, 65536, n // 2, n - 257, n - 256, n - 65, n - 64, n - 2, n - 1] + list(range(3000, 3020))
    spots = [(i, j) for j in range(1, H, 3) for i in range(1, W, 2)][:len(live) + 3]
    want = {}
    for sid, (i, j) in zip(live, spots):
        bulk[sid, :3] = centre(W, H, i, j, 2.0)
        bulk[sid, 7] = time
        want[sid] = (j, i)
    shared = spots[0]                                  # the pixel of surfel 1, the first live one
    for k, (i, j) in enumerate(spots[len(live):]):
        sid = n + k
        bulk[sid, :3] = centre(W, H, i, j, 2.0)
        bulk[sid, 7] = time
        want[sid] = (j, i)
    # ... and the last three also beat earlier ids on a shared pixel: n (z 1.5) loses to n + 1 (z 1.0); n + 2 takes surfel 63's pixel
    extra = np.zeros((2, 12), F)
    extra[:] = bulk[n]
    extra[0, :3], extra[1, :3] = centre(W, H, shared[0], shared[1], 1.0), centre(W, H, spots[1][0], spots[1][1], 1.5)
    surf = np.concatenate([bulk, extra])               # ids n + 3, n + 4
    want[n + 3] = (shared[1], shared[0])
    want[n + 4] = (spots[1][1], spots[1][0])
    del want[1], want[63]

    def check(out):
        idx = out[0]
        assert (idx > 0).sum() == len(want) == len(live) + 3
        for sid, (r, c) in want.items():
            assert idx[r, c] == sid, (sid, r, c)
    return SplatScene("index_stride", "index", W, H, surf, check, time=time, timeDelta=td)


INDEX_BUILDERS = (index_pixel_edges, index_viewport_edges, index_gates, index_ties, index_stride)


# ------------------------------------------------------------------------------------------------------------------------------------
# combined_predict / synthesize_depth
# ------------------------------------------------------------------------------------------------------------------------------------
def disc(W, H, u, v, sid, z=1.0, rpx=1.0, n=(0, 0, -1), x=None, y=None, **kw):
    """a disc facing the camera whose centre projects onto window position (u, v), rpx pixels in radius; x / y: exact coordinates instead"""
    px = (u - W / 2.0) / FX * z if x is None else x
    py = (v - H / 2.0) / FY * z if y is None else y
    return row((px, py, z), conf=TAG + sid, n=n, rad=rpx * z / FX, **kw)


def surface_edge_centres(W, H, axis):
    """sprite centres on the image edge (u = 0, u just below cols: kept and clamped) and just outside (culled by the centre)"""
    n, c = (W, W / 2.0) if axis == "x" else (H, H / 2.0)
    lo, hi = solve(0, 1.0, FX, c), solve(n, 1.0, FX, c)
    xs = (lo, step_until_changed(lo, 1.0, FX, c, -1), step_until_changed(hi, 1.0, FX, c, -1), hi)
    assert proj(xs[0], 1.0, FX, c) == 0 and proj(xs[1], 1.0, FX, c) < 0 and n - 1e-5 < proj(xs[2], 1.0, FX, c) < n and proj(xs[3], 1.0, FX, c) == n
    rows = []
    for k, e in enumerate(xs):
        lane = 1.5 + 3 * k
        rows.append(disc(W, H, lane, lane, k, rpx=1.2, **({"x": e} if axis == "x" else {"y": e})))     # size 3.4: bounding boxes of 2 x 3 after the clamp, 3 pixels drawn

    def check(out):
        own = owners(out)
        if axis == "y":
            own = own.T
        assert set(np.unique(own)) == {-1, 0, 2}
        assert (own[0:3, 0] == 0).all() and (own == 0).sum() == 3
        assert (own[6:9, n - 1] == 2).all() and (own == 2).sum() == 3
        box = (2, 3) if axis == "x" else (3, 2)
        assert [sprite_box(r, (W, H, FX, FY, W / 2.0, H / 2.0)) for r in rows] == [box, None, box, None]
    return SplatScene(f"surface_edge_centres_{axis}", "surface", W, H, rows, check)


def surface_corners(W, H):
    """a sprite clamped at each corner"""
    x0, x1 = solve(0, 1.0, FX, W / 2.0), step_until_changed(solve(W, 1.0, FX, W / 2.0), 1.0, FX, W / 2.0, -1)
    y0, y1 = solve(0, 1.0, FY, H / 2.0), step_until_changed(solve(H, 1.0, FY, H / 2.0), 1.0, FY, H / 2.0, -1)
    rows = [disc(W, H, 0, 0, k, rpx=1.8, x=x, y=y) for k, (x, y) in enumerate(((x0, y0), (x1, y0), (x0, y1), (x1, y1)))]   # size 5.09

    def check(out):
        own = owners(out)
        assert own[0, 0] == 0 and own[0, W - 1] == 1 and own[H - 1, 0] == 2 and own[H - 1, W - 1] == 3
        # centre on the corner, radius 1.8 px: the 2 x 2 block less its far pixel (2.12 px away) ... and 3 x 3 bounding boxes, clamped
        assert [(own == k).sum() for k in range(4)] == [3, 3, 3, 3]
        assert [sprite_box(r, (W, H, FX, FY, W / 2.0, H / 2.0)) for r in rows] == [(3, 3)] * 4
    return SplatScene("surface_corners", "surface", W, H, rows, check)


def _glmin(x, y):
    return y if y < x else x


def _glmax(x, y):
    return y if x < y else x


def sprite_box(r, cam):
    """(columns, rows) of the bounding box k_surface_splat deals to its SPLAT_LANES lanes for surfel row r under the identity pose:
    splat.vert:70-85 and the point rasterisation N3 in float32, as make_sprite evaluates them (None: culled by its centre)"""
    W, H, fx, fy, cx, cy = cam
    p, rad = [F(v) for v in r[0:3]], F(r[11])
    rn = F(1.0) / np.sqrt(F(F(F(r[8] * r[8]) + F(r[9] * r[9])) + F(r[10] * r[10])))
    n = [F(v * rn) for v in r[8:11]]
    x1 = sprite_axis(r[8:11], rad)
    y1 = [F(F(n[1] * x1[2]) - F(n[2] * x1[1])), F(F(n[2] * x1[0]) - F(n[0] * x1[2])), F(F(n[0] * x1[1]) - F(n[1] * x1[0]))]
    with np.errstate(all="ignore"):
        q = [[F(p[c] + sg * ax[c]) for c in range(3)] for ax, sg in ((x1, F(1)), (y1, F(1)), (y1, F(-1)), (x1, F(-1)))]
        qx, qy = [proj(c[0], c[2], fx, cx) for c in q], [proj(c[1], c[2], fy, cy) for c in q]
        ext = []
        for v in (qx, qy):
            lo = _glmin(v[0], _glmin(v[1], _glmin(v[2], v[3])))
            hi = _glmax(v[0], _glmax(v[1], _glmax(v[2], v[3])))
            ext.append(F(abs(F(hi - lo))))
        size = _glmax(F(0), _glmax(ext[0], ext[1]))
        size = F(min(max(size, F(1.0)), F(2047.0)))
        u, v = proj(p[0], p[2], fx, cx), proj(p[1], p[2], fy, cy)
    if not (0 <= u < F(W) and 0 <= v < F(H)):
        return None
    hs = F(size * F(0.5))
    px0, px1 = max(0, int(np.ceil(F(F(u - hs) - F(0.5))))), min(W - 1, int(np.ceil(F(F(u + hs) - F(0.5)))) - 1)
    py0, py1 = max(0, int(np.ceil(F(F(v - hs) - F(0.5))))), min(H - 1, int(np.ceil(F(F(v + hs) - F(0.5)))) - 1)
    return px1 - px0 + 1, py1 - py0 + 1


# window position of the disc's centre (pixel (i, j)'s centre plus an offset, or on a border), radius in pixels -> pixels drawn, and the
# bounding box (columns, rows) whose columns x rows fragments the splat deals to the SPLAT_LANES = 4 lanes of the surfel
FRAGMENT_SHAPES = (((3.5, 4.5), 0.3, 1, (1, 1)), ((9.5, 5.0), 0.6, 2, (1, 2)), ((3.9, 10.9), 0.78, 3, (2, 2)), ((10.0, 11.0), 0.75, 4, (2, 2)),
                   ((3.5, 16.5), 1.1, 5, (3, 3)), ((9.7, 16.5), 1.3, 7, (4, 3)),
                   ((0.2, 22.5), 0.884, 1, (1, 3)),     # clamped at the left border: one column of three fragments
                   ((6.5, 0.2), 0.884, 1, (3, 1)))      # clamped at the top border: three columns of one fragment


def surface_fragment_counts(W, H):
    """sprites that draw 1, 2, 3, 4, 5 and 7 pixels, and bounding boxes — what k_surface_splat deals to its SPLAT_LANES lanes, column by
    column — of 1, 2, 3 (1 x 3 and 3 x 1, clamped at a border), 4, 9 and 12 fragments: nfrag % SPLAT_LANES of 1, 2, 3, 0, 1 and 0.
    (A BOX of 5 or 7 fragments cannot occur: it needs a side of one pixel, and a clamped side of one pixel bounds the point size by 3.)"""
    rows = [disc(W, H, u, v, k, rpx=rpx) for k, ((u, v), rpx, _, _) in enumerate(FRAGMENT_SHAPES)]
    cam = (W, H, FX, FY, W / 2.0, H / 2.0)

    def check(out):
        own = owners(out)
        assert [(own == k).sum() for k in range(len(FRAGMENT_SHAPES))] == [s[2] for s in FRAGMENT_SHAPES]
        boxes = [sprite_box(r, cam) for r in rows]
        assert boxes == [s[3] for s in FRAGMENT_SHAPES], boxes
        assert {(c * r) % 4 for c, r in boxes} == {0, 1, 2, 3}
        for k, (c, r) in enumerate(boxes):          # what is drawn lies inside the box
            rr, cc = np.nonzero(own == k)
            assert rr.max() - rr.min() < r and cc.max() - cc.min() < c, k
    return SplatScene("surface_fragment_counts", "surface", W, H, rows, check)


def surface_tall_clamped(W, H):
    """one sprite taller than wide after clamping at the left border (2 x 5 fragments, walked column by column)"""
    rows = [disc(W, H, 0.2, 8.5, 0, rpx=1.6)]       # size 4.5: a box of 2 x 5 fragments, of which 3 + 1 pass the radius test

    def check(out):
        own = owners(out)
        rr, cc = np.nonzero(own == 0)
        assert sorted(zip(rr.tolist(), cc.tolist())) == [(7, 0), (8, 0), (8, 1), (9, 0)]
        assert sprite_box(rows[0], (W, H, FX, FY, W / 2.0, H / 2.0)) == (2, 5)
    return SplatScene("surface_tall_clamped", "surface", W, H, rows, check)


def surface_size_small(W, H):
    """point size clamped to 1 from below: a sprite a quarter of a pixel wide still draws the pixel it lies in"""
    rows = [disc(W, H, 5.5, 5.5, 0, rpx=0.08), disc(W, H, 8.7, 7.3, 1, rpx=0.33)]

    def check(out):
        own = owners(out)
        assert own[5, 5] == 0 and (own == 0).sum() == 1 and own[7, 8] == 1 and (own == 1).sum() == 1
    return SplatScene("surface_size_small", "surface", W, H, rows, check)


def surface_size_2047(W, H):
    """a near surfel whose sprite (11 000 px, clamped to 2047) covers the whole image"""
    rows = [row((0.0001, 0.0002, 0.001), conf=TAG, rad=0.1)]

    def check(out):
        own = owners(out)
        assert (own == 0).all()
    return SplatScene("surface_size_2047", "surface", W, H, rows, check)


def sprite_axis(n, rad):
    """splat.vert:70 in float32: x1 = normalize((n.y - n.z, -n.x, n.x)) * rad * 1.41421356 for a unit normal n"""
    n = [F(v) for v in n]
    rn = F(1.0) / np.sqrt(F(F(F(n[0] * n[0]) + F(n[1] * n[1])) + F(n[2] * n[2])))
    n = [F(v * rn) for v in n]
    t = [F(n[1] - n[2]), F(-n[0]), n[0]]
    tn = F(1.0) / np.sqrt(F(F(F(t[0] * t[0]) + F(t[1] * t[1])) + F(t[2] * t[2])))
    return [F(F(F(v * tn) * F(rad)) * F(1.41421356)) for v in t]


def surface_size_infinite(W, H):
    """an infinite point size: the corner p - x1 has z = 0 and x != 0"""
    nrm, rad = (0.6, 0.0, -0.8), 0.05
    x1 = sprite_axis(nrm, rad)
    p = (F(0.005), F(0.005), x1[2])
    assert F(p[2] - x1[2]) == 0 and F(p[0] - x1[0]) != 0 and p[2] > 0
    rows = [row(p, conf=TAG, n=nrm, rad=rad)]

    def check(out):
        own = owners(out)
        assert (own == 0).sum() >= min(W * H, 36 * 28)  # the box is the whole image, and the disc lies close enough to fill it
    return SplatScene("surface_size_infinite", "surface", W, H, rows, check)


def surface_gates(W, H):
    """conf == confThreshold, t == maxTime, time - t == timeDelta, p.z == maxDepth: kept; one past each: culled"""
    time, max_time, td, thr = 10, 8, 3, TAG + 2
    cases = [dict(conf=F(thr)), dict(conf=down(thr)), dict(t_last=max_time), dict(t_last=max_time + 1), dict(t_last=time - td),
             dict(t_last=time - td - 1), dict(z=F(MAXD)), dict(z=up(MAXD))]
    rows, kept = [], []
    for k, c in enumerate(cases):
        i, j = 2 + 4 * (k % 2), 2 + 3 * (k // 2)
        r = disc(W, H, i + 0.5, j + 0.5, k, z=float(c.get("z", 1.0)), rpx=0.3, t_last=c.get("t_last", max_time))
        r[2] = c.get("z", r[2])
        r[3] = c.get("conf", F(thr + 1 + k))
        rows.append(r)
        if k % 2 == 0:
            kept.append((j, i, r[3]))

    def check(out):
        img, vt = out[0], out[1]
        assert (img[..., 3] == 255).sum() == 4
        for j, i, conf in kept:
            assert vt[j, i, 3] == conf and vt[j, i, 2] > 0, (j, i)
        assert vt[kept[0][0], kept[0][1], 3] == thr and vt[kept[3][0], kept[3][1], 2] >= F(MAXD) - F(1e-4)
    return SplatScene("surface_gates", "surface", W, H, rows, check, time=time, maxTime=max_time, timeDelta=td, conf=thr)


def surface_ties(W, H):
    """coplanar surfels of identical geometry under different ids on a block of pixels (lowest id wins); a later id nearer by one ulp"""
    z = F(1.5)
    rows = [disc(W, H, 4.0, 5.0, 0, z=float(z), rpx=1.6, colour=float(0x102030)), disc(W, H, 4.0, 5.0, 1, z=float(z), rpx=1.6, colour=float(0x405060)),
            disc(W, H, 4.0, 5.0, 2, z=float(z), rpx=1.6),
            disc(W, H, 7.0, 13.0, 3, z=float(z), rpx=1.6), disc(W, H, 7.0, 13.0, 4, z=float(z), rpx=1.6)]
    rows[4][2] = down(z)
    rows[4][0], rows[4][1] = rows[3][0], rows[3][1]

    def check(out):
        own, img = owners(out), out[0]
        assert (own == 0).sum() == 12 and (own == 1).sum() == 0 and (own == 2).sum() == 0      # 4 x 4 less its corners
        assert (img[own == 0][:, :3] == (0x10, 0x20, 0x30)).all()
        assert (own == 4).sum() > 0 and (own == 3).sum() + (own == 4).sum() == 12
    return SplatScene("surface_ties", "surface", W, H, rows, check)


def _ray(W, H, i, j):
    """pixel_ray in float32: normalize(((i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, 1))"""
    x, y = F(F(F(i) + F(0.5) - F(W / 2.0)) / F(FX)), F(F(F(j) + F(0.5) - F(H / 2.0)) / F(FY))
    rn = F(1.0) / np.sqrt(F(F(F(x * x) + F(y * y)) + F(1.0)))
    return F(x * rn), F(y * rn), F(rn)


def _sqr_dist(W, H, i, j, p):
    """combo_splat.frag:37-46 for a disc at p facing the camera (n = (0, 0, -1)): dot(diff, diff) of pixel (i, j)'s fragment, float32"""
    l = _ray(W, H, i, j)
    pn = F(F(F(p[0] * F(0)) + F(p[1] * F(0))) + F(p[2] * F(-1)))
    ln = F(F(F(l[0] * F(0)) + F(l[1] * F(0))) + F(l[2] * F(-1)))
    k = F(pn / ln)
    d = [F(F(k * l[c]) - p[c]) for c in range(3)]
    return F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))


def surface_radius(W, H):
    """a fragment exactly on the radius — dot(diff, diff) == rad * rad — is kept; with the radius one float smaller it is discarded"""
    i, j = 5, 6
    found = None
    for step in range(2000):                        # depths around 1.2 m until some float radius squares to the fragment's squared distance
        z = F(1.2) + F(step) * F(1e-4)
        p = tuple(F(v) for v in centre(W, H, i, j, float(z)))
        d2 = _sqr_dist(W, H, i + 1, j, p)
        r = F(np.sqrt(d2))
        for cand in (down(r), r, up(r)):
            if F(cand * cand) == d2:
                found = (p, cand, d2)
        if found:
            break
    assert found, "no depth gives an exactly representable radius"
    p, rad, d2 = found
    assert F(down(rad) * down(rad)) < d2
    q = (p[0], F(p[1] + F(6.0 / FY) * p[2]), p[2])  # the same disc six pixels further down (its squared distances are its own: checked below)
    rows = [row(p, conf=TAG, rad=rad), row(p, conf=TAG + 1, rad=down(rad))]
    rows[1][1] = q[1]

    def check(out):
        own = owners(out)
        assert own[j, i] == 0 and own[j, i + 1] == 0, "the fragment on the radius is kept"
        assert own[j + 6, i] == 1
        got0 = {(int(r) - j, int(c) - i) for r, c in zip(*np.nonzero(own == 0))}
        got1 = {(int(r) - j - 6, int(c) - i) for r, c in zip(*np.nonzero(own == 1))}
        assert (0, 1) in got0 and got1 < got0, (got0, got1)
    return SplatScene("surface_radius", "surface", W, H, rows, check)


def surface_negative_depths(W, H):
    """a disc straddling the camera plane (k < 0 on some rays: negative intersection depths) against a positive one on the same pixels"""
    rows = [row((0.0, 0.0, 1.0), conf=TAG, rad=5.0),                                   # 0: a wall at 1 m over the whole image
            row((0.0, 0.0, 0.02), conf=TAG + 1, n=(0.995, 0.0, -0.1), rad=0.5)]        # 1: steeply tilted: rays right of x / z = 0.1005 meet it behind the camera

    def check(out):
        own, vt = owners(out), out[1]
        neg = vt[..., 2] < 0
        assert neg.sum() > 0 and (own[neg] == 1).all(), "negative depths beat the wall, although their id is the higher one"
        assert (own >= 0).all() and (vt[..., 2][:, :W // 2] > 0).all() and neg[:, W - 1].all()
    return SplatScene("surface_negative_depths", "surface", W, H, rows, check)


def surface_signed_zeros(W, H, order):
    """both planes pass through the camera centre: every fragment has z = +0 or -0, of opposite sign for the two surfels; they tie, the
    lower id keeps every pixel, and ITS zero — sign included — comes out in vertex.z and in the synthesized depth"""
    a, b = (1.0, -1.0) if order == 0 else (-1.0, 1.0)
    rows = [row((0, 0, 0.05), conf=TAG, n=(a, 0, 0), rad=0.1), row((0, 0, 0.05), conf=TAG + 1, n=(b, 0, 0), rad=0.1)]

    def check(out):
        own, vt = owners(out), out[1]
        z = vt[..., 2]
        assert (own >= 0).sum() >= min(W * H, 36 * 28) // 2 and (own[own >= 0] == 0).all(), "the lower id keeps every pixel"
        drawn = own >= 0
        minus = np.signbit(z) & drawn
        assert (z[drawn] == 0).all() and minus.sum() > 0 and (drawn & ~minus).sum() > 0
        # the sign goes with the side of the image, mirrored between the two orders
        left = np.zeros_like(drawn)
        left[:, :W // 2] = True
        assert (minus[drawn] == left[drawn]).all() or (minus[drawn] == ~left[drawn]).all()
    return SplatScene(f"surface_signed_zeros_{order}", "surface", W, H, rows, check)


def surface_nan_axis(W, H):
    """n.x = 0 and n.y = n.z make the sprite axis 0 / 0 and every corner NaN.  splat.vert's max(0, NaN) is 0 by GLSL's definition
    of max, so the sprite is a point of size 0, clamped to 1 (N6): its centre pixel is drawn.  A zero normal makes the fragment's own
    intersection NaN: nothing is drawn.  A plain neighbour draws its five pixels."""
    rows = [disc(W, H, 4.5, 4.5, 0, rpx=1.1, n=(0.0, 0.70710678, 0.70710678)), disc(W, H, 4.5, 10.5, 1, rpx=1.1, n=(0, 0, 0)),
            disc(W, H, 4.5, 16.5, 2, rpx=1.1)]

    def check(out):
        own = owners(out)
        assert own[4, 4] == 0 and (own == 0).sum() == 1 and (own == 1).sum() == 0 and (own == 2).sum() == 5
    return SplatScene("surface_nan_axis", "surface", W, H, rows, check)


def surface_nan_corner(W, H, which):
    """exactly ONE NaN corner: (0, ., 0) projects its x as 0 / 0 (and its y as inf).  GLSL's min(x, y) = y < x ? y : x keeps a NaN that
    stands FIRST in splat.vert's nest min(p1, min(p2, min(p3, p4))) and drops one that stands last (N6):
      'last'       p - x1 is the NaN corner: dropped, the sprite keeps the infinite extent of the others and is drawn over the whole image
      'neighbour'  the same with p.z one float up: no corner is NaN, the same pixels are drawn
      'first'      p + x1 is the NaN corner: the extent is NaN, max(0, NaN) = 0, the sprite is a point of size 1"""
    nrm, rad = ((-0.6, 0.55, 0.58) if which == "first" else (0.6, 0.55, 0.58)), 0.05
    x1 = sprite_axis(nrm, rad)
    sgn = F(-1.0) if which == "first" else F(1.0)
    p = [F(sgn * x1[0]), F(0.005), F(sgn * x1[2])]
    assert F(p[0] - sgn * x1[0]) == 0 and F(p[2] - sgn * x1[2]) == 0 and F(p[0] + sgn * x1[0]) != 0 and p[2] > 0
    if which == "neighbour":
        p[2] = up(p[2])
    rows = [row(p, conf=TAG, n=nrm, rad=rad)]

    def check(out):
        own = owners(out)
        if which == "first":
            assert (own == 0).sum() == 1
        else:
            assert (own == 0).sum() >= 200
            if (W, H) == (36, 28):
                assert (own == 0).sum() == 887
    return SplatScene(f"surface_nan_corner_{which}", "surface", W, H, rows, check)


def surface_parallel_ray(W, H, through_origin):
    """a ray parallel to the plane: cx = W / 2 + 0.5 puts column W / 2 on x = 0, and n = (1, 0, 0) gives dot(l, n) == 0 there: k = +/-inf
    for a plane beside the camera centre, 0 / 0 for one through it (whose other fragments all lie AT the camera centre, z = +/-0)"""
    cam = (W, H, FX, FY, W / 2.0 + 0.5, H / 2.0)
    rows = [row((0.0 if through_origin else 0.01, 0.0, 1.0), conf=TAG, n=(1, 0, 0), rad=1.0)]

    def check(out):
        own, vt = owners(out), out[1]
        assert (own[:, W // 2] == -1).all() and (own[:, W // 2 + 1] == 0).all()
        if through_origin:
            assert (own[:, W // 2 - 1] == 0).all() and (vt[..., 2] == 0).all()
        else:
            assert (own[:, :W // 2] == -1).all() and (np.abs(vt[:, W // 2 + 1, 2] - 0.4) < 1e-6).all()
    return SplatScene(f"surface_parallel_ray_{'k_nan' if through_origin else 'k_inf'}", "surface", W, H, rows, check, cam=cam)


def surface_colour_time(W, H):
    """packed colours over all channel values (decoded c / 255, written back as round(. * 255)) and init times around and above 65 535"""
    times = [0, 1, 65534, 65535, 65536, 65537, 70000, 131071, 16777216.0]
    rows, want = [], []
    for k in range(256):
        i, j = k % 12, 1 + k // 12
        rgb = (k, 255 - k, (k * 7 + 3) % 256)
        t = times[k % len(times)]
        rows.append(disc(W, H, i + 0.5, j + 0.5, k, rpx=0.3, colour=float((rgb[0] << 16) | (rgb[1] << 8) | rgb[2]), t_init=t))
        want.append((j, i, rgb, int(t) % 65536))

    def check(out):
        img, tm = out[0], out[3]
        assert (img[..., 3] == 255).sum() == 256
        for j, i, rgb, t in want:
            assert tuple(int(v) for v in img[j, i, :3]) == rgb and tm[j, i] == t, (j, i)
    return SplatScene("surface_colour_time", "surface", W, H, rows, check, time=2, maxTime=2)


def surface_stride(W, H):
    """65 536 + 3 stable surfels ... times four: the surface splat takes 262 144 surfels per trip (4 lanes each), so the three surfels past
    262 144 are its second trip; 65 536 + 3 alone stays inside the first.  The bulk fails the time gate and lies nearer than the rest."""
    n, time, td = SURFACE_STRIDE, 10, 3
    rng = np.random.RandomState(6)
    surf = np.zeros((n + 3, 12), F)
    ii, jj = rng.randint(0, W, n + 3), rng.randint(0, H, n + 3)
    surf[:, 2] = 0.5
    surf[:, 0] = (ii + 0.5 - W / 2.0) / FX * 0.5
    surf[:, 1] = (jj + 0.5 - H / 2.0) / FY * 0.5
    surf[:, 3], surf[:, 4], surf[:, 6], surf[:, 7] = TAG, GREY, 1, 1
    surf[:, 10], surf[:, 11] = -1, 0.3 * 0.5 / FX
    live = [1, 63, 64, 65535, 65536, 65537, 65538, n // 2, n - 64, n - 1] + list(range(5000, 5012))
    spots = [(i, j) for j in range(1, H - 1, 3) for i in range(1, W - 1, 3)]
    want = {}
    for k, sid in enumerate(live + [n, n + 1, n + 2]):
        i, j = spots[k]
        surf[sid] = disc(W, H, i + 0.5, j + 0.5, 0, z=2.0, rpx=0.3, t_last=time)
        surf[sid, 3] = TAG + 1 + k
        want[(j, i)] = TAG + 1 + k
    # the last three also win pixels of earlier live surfels: nearer, on the pixels of surfels 1, 63 and 64
    extra = np.zeros((3, 12), F)
    for k in range(3):
        i, j = spots[k]
        extra[k] = disc(W, H, i + 0.5, j + 0.5, 0, z=1.0, rpx=0.3, t_last=time)
        extra[k, 3] = TAG + 100 + k
        want[(j, i)] = TAG + 100 + k
    surf = np.concatenate([surf, extra])

    def check(out):
        img, vt = out[0], out[1]
        assert (img[..., 3] == 255).sum() == len(want)
        for (j, i), conf in want.items():
            assert vt[j, i, 3] == conf, (j, i)
    return SplatScene("surface_stride", "surface", W, H, surf, check, time=time, maxTime=time, timeDelta=td)


def surface_nothing(W, H, empty):
    """a map in which every surfel fails a gate — and count = 0 itself: every output is zero"""
    rows = np.zeros((0, 12), F) if empty else [disc(W, H, 5.5, 5.5, 0, rpx=2.0, t_last=9), disc(W, H, 5.5, 9.5, -5, rpx=2.0),
                                               disc(W, H, 5.5, 13.5, 2, rpx=2.0, z=MAXD * 2), disc(W, H, 5.5, 17.5, 3, rpx=2.0, z=-1.0)]

    def check(out):
        for a in out:
            assert not a.view(np.uint8).any()
    return SplatScene(f"surface_nothing_{'count0' if empty else 'gated'}", "surface", W, H, rows, check, time=10, maxTime=8, timeDelta=3, conf=TAG)


def index_nothing(W, H):
    """count = 0 through predict_indices"""
    def check(out):
        for a in out:
            assert not a.view(np.uint8).any()
    return SplatScene("index_nothing_count0", "index", W, H, np.zeros((0, 12), F), check)


SURFACE_BUILDERS = (
    lambda W, H: surface_edge_centres(W, H, "x"), lambda W, H: surface_edge_centres(W, H, "y"), surface_corners, surface_fragment_counts,
    surface_tall_clamped, surface_size_small, surface_size_2047, surface_size_infinite, surface_gates, surface_ties, surface_radius,
    surface_negative_depths, lambda W, H: surface_signed_zeros(W, H, 0), lambda W, H: surface_signed_zeros(W, H, 1), surface_nan_axis,
    lambda W, H: surface_nan_corner(W, H, "last"), lambda W, H: surface_nan_corner(W, H, "neighbour"),
    lambda W, H: surface_nan_corner(W, H, "first"), lambda W, H: surface_parallel_ray(W, H, False),
    lambda W, H: surface_parallel_ray(W, H, True), surface_colour_time,
    surface_stride, lambda W, H: surface_nothing(W, H, False), lambda W, H: surface_nothing(W, H, True))


SPLAT_SCENE_NAMES = (
    "index_pixel_edges", "index_viewport_edges", "index_gates", "index_ties", "index_stride", "index_nothing_count0",
    "surface_edge_centres_x", "surface_edge_centres_y", "surface_corners", "surface_fragment_counts", "surface_tall_clamped",
    "surface_size_small", "surface_size_2047", "surface_size_infinite", "surface_gates", "surface_ties", "surface_radius",
    "surface_negative_depths", "surface_signed_zeros_0", "surface_signed_zeros_1", "surface_nan_axis", "surface_nan_corner_last",
    "surface_nan_corner_neighbour", "surface_nan_corner_first", "surface_parallel_ray_k_inf", "surface_parallel_ray_k_nan",
    "surface_colour_time", "surface_stride", "surface_nothing_gated", "surface_nothing_count0")


def splat_scene(W, H, k):
    """scene k (of SPLAT_SCENE_NAMES) at one image size; nothing else is built"""
    sc = (INDEX_BUILDERS + (index_nothing,) + SURFACE_BUILDERS)[k](W, H)
    assert sc.name == SPLAT_SCENE_NAMES[k], (sc.name, k)
    return sc


def splat_scenes(W, H):
    """every predict_indices and combined_predict / synthesize_depth scene at one image size"""
    return [b(W, H) for b in INDEX_BUILDERS + (index_nothing,) + SURFACE_BUILDERS]


# ------------------------------------------------------------------------------------------------------------------------------------
# fill_in, dense_enough, seed_map
# ------------------------------------------------------------------------------------------------------------------------------------
def fill_scene(W, H):
    """random prediction images with fill_in's three selectors hit independently of one another (vertex.z == 0; normal.z == 0 beside a
    non-zero x, y; image (0, 0, 0) with alpha 255, while (0, 0, 1) is kept), selected pixels on the right and bottom border (the forward
    differences clamp their taps there) and one whose filtered depths are 0 (the 0 / 0 normal).  Returns the inputs and
    check(plain, passthrough) for the oracle's two results."""
    rng = np.random.RandomState(W * 1000 + H)
    image = rng.randint(1, 256, size=(H, W, 4)).astype(np.uint8)
    image[..., 3] = 255
    vertex = rng.uniform(0.5, 2.0, size=(H, W, 4)).astype(F)
    normal = rng.uniform(0.1, 1.0, size=(H, W, 4)).astype(F) * np.where(rng.rand(H, W, 4) < 0.5, -1, 1).astype(F)
    depth = rng.randint(300, 3000, size=(H, W)).astype(np.uint16)
    rgb = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    sel_v = [(2, 3), (5, W - 1), (H - 1, 4), (H - 1, W - 1), (9, 9)]
    sel_n = [(3, 6), (6, W - 1), (H - 1, 7), (H - 1, W - 1), (12, 5), (15, 8)]
    sel_i = [(4, 1), (7, W - 1), (H - 1, 2), (H - 1, W - 1)]
    kept_i = [(4, 3), (8, 8)]
    for k, (r, c) in enumerate(sel_v):
        vertex[r, c, 2] = -0.0 if k % 2 else 0.0
    for k, (r, c) in enumerate(sel_n):
        normal[r, c, 2] = -0.0 if k % 2 else 0.0
    for r, c in sel_i:
        image[r, c, :3] = 0
    for r, c in kept_i:
        image[r, c, :3] = (0, 0, 1)
    depth[15, 8] = depth[15, 9] = depth[16, 8] = 0          # sel_n's last pixel: all three taps 0 -> normalize(0) = 0 / 0
    depth[12, 5] = 0                                        # ... and one with only its own tap 0

    def check(plain, passthrough):
        fi, fv, fn = plain
        mv, mn, mi = np.zeros((H, W), bool), np.zeros((H, W), bool), np.zeros((H, W), bool)
        for m, sel in ((mv, sel_v), (mn, sel_n), (mi, sel_i)):
            for r, c in sel:
                m[r, c] = True
        z = depth.astype(F) / F(1000.0)
        assert np.array_equal(fv[~mv].view(np.uint32), vertex[~mv].view(np.uint32)) and (fv[mv][:, 3] == 1).all() and np.array_equal(fv[mv][:, 2], z[mv])
        assert np.array_equal(fn[~mn].view(np.uint32), normal[~mn].view(np.uint32)) and (fn[mn][:, 3] == 1).all()
        assert np.isnan(fn[15, 8, :3]).all() and np.isfinite(fn[12, 5, :3]).all() and np.isfinite(fn[H - 1, W - 1, :3]).all()
        assert np.array_equal(fi[~mi], image[~mi]) and np.array_equal(fi[mi][:, :3], rgb[mi]) and (fi[mi][:, 3] == 255).all()
        pi, pv, pn = passthrough
        assert np.array_equal(pi[..., :3], rgb) and (pv[..., 3] == 1).all() and np.array_equal(pv[..., 2], z) and (pn[..., 3] == 1).all()
    return dict(image=image, vertex=vertex, normal=normal, depth=depth, rgb=rgb), check


def dense_cases():
    """(name, W, H, image, expected): denseEnough's sample grids — 1 x 1 at 20 x 20 and 36 x 28, 2 x 1 at 52 x 36, 3 x 2 at 60 x 40 with
    4 and 5 of 6 samples non-zero (either side of 0.75); a sample with one zero channel counts as empty.  Every pixel that is NOT a sample
    holds the opposite of what the samples hold, so a pass that looks at the wrong texel answers wrongly."""
    cases = []

    def image(W, H, filled, half=()):
        pts = [(20 * b + 10, 20 * a + 10) for b in range(H // 20) for a in range(W // 20)]
        img = np.zeros((H, W, 4), np.uint8)
        img[..., 3] = 255
        if len(filled) * 2 < len(pts) or not filled:
            img[..., :3] = 200                      # samples mostly empty: everything else is full
        for k, (r, c) in enumerate(pts):
            img[r, c, :3] = (9, 1, 255) if k in filled else 0
            if k in half:
                img[r, c, :3] = [(0, 7, 7), (7, 0, 7), (7, 7, 0)][k % 3]
        return img
    for W, H in ((20, 20), (36, 28)):
        cases += [(f"{W}x{H}_full", W, H, image(W, H, {0}), True), (f"{W}x{H}_empty", W, H, image(W, H, set()), False),
                  (f"{W}x{H}_one_zero_channel", W, H, image(W, H, {0}, half={0}), False)]
    cases += [("52x36_both", 52, 36, image(52, 36, {0, 1}), True), ("52x36_one_of_two", 52, 36, image(52, 36, {1}), False),
              ("60x40_4_of_6", 60, 40, image(60, 40, {0, 2, 3, 5}), False), ("60x40_5_of_6", 60, 40, image(60, 40, {0, 1, 2, 4, 5}), True),
              ("60x40_5_of_6_one_zero_channel", 60, 40, image(60, 40, {0, 1, 2, 4, 5}, half={4}), False),
              ("60x40_6_of_6", 60, 40, image(60, 40, {0, 1, 2, 3, 4, 5}), True)]
    return cases


def seed_scene(W, H):
    """first-frame seeding at 52 x 36 (1 872 pixels: one full compaction chunk of 1 024 and a partial one, whose last thread's four
    elements are cut short by e >= P) and 36 x 28 (one partial chunk): holes, depths on the maxDepth gate and one float past it, zero and
    negative depths, and a filtered stream shorter than the raw one (the normals past its end are the stale zeros).  The seeding pass
    has no near gate of its own — 0.3 m is cut where the depth is made metric — so 0.3 and its two neighbouring floats are ordinary
    depths here, and all three must come out.
    Returns the inputs and check(surfels) for the oracle's result."""
    rng = np.random.RandomState(W + H)
    max_depth = 2.5
    dm = rng.uniform(0.4, 2.4, size=(H, W)).astype(F)
    dm[rng.rand(H, W) < 0.1] = 0
    dm[3, 4], dm[3, 5], dm[3, 6], dm[3, 7] = F(max_depth), up(max_depth), F(-0.0), F(-1.0)
    dm[3, 8], dm[3, 9], dm[3, 10] = down(0.3), F(0.3), up(0.3)
    dm[H - 1, W - 1], dm[0, 0], dm[H - 1, 0], dm[0, W - 1] = 1.0, 1.25, 1.5, 1.75          # the first and last elements of the column-major walk
    dmf = dm.copy()
    dmf[rng.rand(H, W) < 0.2] = 0                                                              # the filter's own holes
    dmf[5, 4], dmf[5, 5] = F(max_depth), up(max_depth)
    rgb = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    n_raw = int(((dm > 0) & (dm <= F(max_depth))).sum())
    n_filt = int(((dmf > 0) & (dmf <= F(max_depth))).sum())
    assert 0 < n_filt < n_raw

    def check(s):
        assert s.shape == (n_raw, 12)
        assert not s[n_filt:, 8:12].view(np.uint32).any(), "normals past the end of the filtered stream: stale zeros"
        assert (s[:n_filt, 11] != 0).all()
        # column-major order: the first surfel is pixel (0, 0), the last one pixel (W - 1, H - 1)
        assert s[0, 2] == F(1.25) and s[-1, 2] == F(1.0) and (s[:, 2] == F(max_depth)).sum() == 1 and (s[:, 2] <= F(max_depth)).all() and (s[:, 2] > 0).all()
        assert (s[:, 5] == 0).all() and (s[:, 6] == 1).all() and (s[:, 7] == 1).all()
        assert all((s[:, 2] == z).sum() == 1 for z in (down(0.3), F(0.3), up(0.3))), "no near gate in the seeding pass"
    return dict(rgb=rgb, dm=dm, dmf=dmf, time=1, maxDepth=max_depth), check


SEED_SIZES = ((52, 36), (36, 28))
FILL_SIZES = SIZES
