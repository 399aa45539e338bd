"""Hand-built scenes for the launches that build the tracker's per-frame inputs (k_model_maps / k_frame_inputs, k_pyr_down_multi,
k_vn_sobel_levels / k_sobel_levels), the oracle's composition each launch stands for, and a numpy restatement of the frame-invariant
photometric gates (rgbMask).  Shared by test_input_scenes_host.py (the scenes provoke what they claim, on the oracle alone) and
test_gpu_tracker_inputs.py (HIP against the oracle, bit for bit).

Sizes (W != H, multiples of 4):
    36 x 28    narrower than one 64-lane model-map workgroup and than one 128-pixel filter tile; 7 bands of 4 rows: the second workgroup
               row is 3/4 live; one tally sample
    80 x 60    4 x 3 = 12 tally samples: 9 / 12 is exactly 0.75; the second model-map column has 16 live lanes
    132 x 36   the second filter tile has 4 live columns, the third model-map column exactly one live quad; level 2 is 33 x 9

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import efo

F = np.float32
SIZES = [(36, 28), (80, 60), (132, 36)]
MAX_DEPTH_RGB = 6.0                       # RGBDOdometry.cpp:42
MIN_SCALE = (1600.0, 576.0, 64.0)         # (minimumGradientMagnitudes / sobelScale)^2 = (5 * 8)^2, (3 * 8)^2, (1 * 8)^2, RGBDOdometry.cpp:112-114,425
DEPTH_CUT = 3.0
PLANES = ("vmap0", "nmap0", "vmap1", "nmap1", "vmap2", "nmap2")


def intr(W, H):
    return 0.82 * W, 0.82 * W, W / 2.0, H / 2.0


def size_id(s):
    return "%dx%d" % s


def rot_axis(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


# a turn of 135 degrees and a translation no output can hide: a missed `+ t` moves every vertex by metres
POSE_R = rot_axis((1.0, 2.0, 3.0), np.deg2rad(135.0)).astype(F)
POSE_T = np.array([3.5, -2.25, 4.75], F)


def init_pattern(name, shape, dtype):
    """what every output holds before either side runs: finite, non-zero, different in every element (a write that should not happen, or
    a stale plane read as a result, shows)"""
    n = int(np.prod(shape))
    seed = sum(ord(c) for c in name)
    if np.dtype(dtype).kind == "f":
        return (F(1000.0 + seed) + np.arange(n, dtype=F) * F(0.25)).reshape(shape)
    return ((np.arange(n, dtype=np.int64) * 7 + seed) % 251 + 1).astype(dtype).reshape(shape)


def mask_planes(m):
    """planar map -> copy with the y / z planes blanked where the x plane is NaN (quirk Q3: they hold stale data)"""
    m = m.copy()
    h = m.shape[0] // 3
    bad = np.isnan(m[:h])
    m[h:2 * h][bad] = 0
    m[2 * h:][bad] = 0
    return m


# ------------------------------------------------------------------------------------------------
# model-map scenes: inputs of ef_op_model_maps
# ------------------------------------------------------------------------------------------------
def _surface(W, H, dz, tilt):
    """camera-frame float4 vertex and normal maps of a slanted surface, valid everywhere"""
    fx, fy, cx, cy = intr(W, H)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    z = 1.5 + dz + 0.3 * (x / W - 0.5) + 0.2 * (y / H - 0.5) + 0.01 * np.sin(x * 0.7 + tilt) * np.cos(y * 0.9)
    v = np.stack([(x - cx) * z / fx, (y - cy) * z / fy, z, np.full_like(z, 7.0 + tilt)], axis=-1).astype(F)
    n = np.stack([0.2 + 0.05 * np.sin(x * 0.31 + tilt), -0.1 + 0.05 * np.cos(y * 0.43 + tilt), -0.95 + 0.0 * x], axis=-1)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    n4 = np.concatenate([n, np.full(n.shape[:2] + (1,), 0.01)], axis=-1).astype(F)
    return np.ascontiguousarray(v), np.ascontiguousarray(n4)


def _images(W, H):
    rng = np.random.RandomState(W * 131 + H)
    pred = rng.randint(1, 256, size=(H, W, 4)).astype(np.uint8)
    # a gray whose intensity is 90 or 110 away from the prediction's in every texel (checked by the host test)
    g = ((intensity_np(pred[..., :3]).astype(np.int32) + 90) % 200 + 20).astype(np.uint8)
    fill = np.stack([g, g, g, 255 - pred[..., 3] // 2], axis=-1).astype(np.uint8)
    return pred, np.ascontiguousarray(fill)


def sample_texels(W, H):
    """Resize::image's sample texels (x, y) = (20 a + 10, 20 b + 10), row-major over (b, a)"""
    return [(20 * a + 10, 20 * b + 10) for b in range(H // 20) for a in range(W // 20)]


def chosen_blocks(W, H):
    """the 4 x 4 blocks (bx, by) that receive a planted texel: a checkerboard, so that every chosen block has untouched neighbours"""
    return [(bx, by) for by in range(H // 4) for bx in range(W // 4) if (bx + by) % 2 == 0]


def verdict(dense_count, dense_samples):
    """the oracle's denseEnough() for a count of dense_count non-zero samples out of dense_samples: asked of efo.dense_enough on an image
    of dense_samples x 1 sample texels"""
    W, H = 20 * dense_samples, 20
    img = np.zeros((H, W, 4), np.uint8)
    for a in range(dense_count):
        img[10, 20 * a + 10] = (9, 9, 9, 255)
    return efo.dense_enough(efo.make_cam(W, H, *intr(W, H)), img)


class MapScene:
    def __init__(self, name, W, H):
        self.name, self.W, self.H = name, W, H
        self.pred_vertex, self.pred_normal = _surface(W, H, 0.0, 0.0)
        self.fill_vertex, self.fill_normal = _surface(W, H, 0.25, 1.0)
        self.pred_image, self.fill_image = _images(W, H)
        self.R, self.t = POSE_R, POSE_T
        self.camera_frame = self.force_fill_image = self.tally = False
        self.dense_samples = max(1, (W // 20) * (H // 20))
        self.dense_count = self.dense_samples        # the prediction, unless the scene says otherwise
        self.exact_planes = True                     # False: quirk Q3's stale planes differ by construction (compare with mask_planes)
        self.planted = []                            # (x, y) texels
        self.expect_fill = None
        self.checks = []

    def __str__(self):
        return f"{self.name}@{self.W}x{self.H}"

    # ---- the composition k_model_maps' comment names, on the oracle ----
    def oracle(self):
        W, H = self.W, self.H
        cam = efo.make_cam(W, H, *intr(W, H))
        if self.tally:
            dense = efo.dense_enough(cam, self.pred_image)
            left = sum(1 for (x, y) in sample_texels(W, H) if (self.pred_image[y, x, :3] > 0).all())
        else:
            dense = verdict(self.dense_count, self.dense_samples)
            left = self.dense_count
        fill = not dense
        v4, n4 = (self.fill_vertex, self.fill_normal) if fill else (self.pred_vertex, self.pred_normal)
        tmp, v0, n0 = efo.copy_maps(v4, n4)
        cam_maps = {"vmap0": v0, "nmap0": n0}
        for l in (1, 2):
            for k, norm in (("vmap", False), ("nmap", True)):
                cam_maps[f"{k}{l}"] = efo.resize_map(cam_maps[f"{k}{l - 1}"], norm, out=init_pattern(f"{k}{l}", (3 * (H >> l), W >> l), F).copy())
        out = {}
        for l in range(3):
            if self.camera_frame:
                out[f"vmap{l}"], out[f"nmap{l}"] = cam_maps[f"vmap{l}"], cam_maps[f"nmap{l}"]
            else:
                out[f"vmap{l}"], out[f"nmap{l}"] = efo.transform_maps(cam_maps[f"vmap{l}"], cam_maps[f"nmap{l}"], self.R, self.t)
        out["depth0"] = efo.vertices_to_depth(tmp, MAX_DEPTH_RGB)
        out["last0"] = efo.bgr_to_intensity(self.fill_image if (fill or self.force_fill_image) else self.pred_image)
        out["dense_count"] = left
        out["_fill"], out["_cam"] = fill, cam_maps
        return out

    def oracle_frame(self, frame):
        """what the pre-processing half of the joint launch leaves"""
        raw, rgb = frame["depth"], frame["rgb"]
        filtered = efo.filter_depth(raw, DEPTH_CUT)
        rgba = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
        rgba[..., :3] = rgb
        return dict(filtered=filtered, metric=efo.metricise_depth(raw, DEPTH_CUT), metric_filtered=efo.metricise_depth(filtered, DEPTH_CUT),
                    next0=efo.bgr_to_intensity(rgba))

    def run_device(self, ops, joint=False, frame=None):
        W, H = self.W, self.H
        init = {k: init_pattern(k, (3 * (H >> int(k[-1])), W >> int(k[-1])), F) for k in PLANES}
        kw = dict(joint=True, raw=frame["depth"], rgb=frame["rgb"], depth_cut=DEPTH_CUT) if joint else {}
        return ops.model_maps(self.pred_vertex, self.pred_normal, self.fill_vertex, self.fill_normal, self.R, self.t, MAX_DEPTH_RGB,
                              pred_image=self.pred_image, fill_image=self.fill_image, camera_frame=self.camera_frame,
                              force_fill_image=self.force_fill_image, tally=self.tally, dense_count=self.dense_count,
                              dense_samples=self.dense_samples, init=init, **kw)

    def check(self, ref):
        """the scene provokes what it claims, on the oracle's result"""
        if self.expect_fill is not None:
            assert ref["_fill"] == self.expect_fill, (str(self), ref["_fill"])
            src = self.fill_vertex if self.expect_fill else self.pred_vertex
            z, d = src[..., 2], ref["depth0"]
            ok = ~np.isnan(d)
            assert ok.any() and np.array_equal(d[ok], z[ok]), (str(self), "depth0 comes from the expected source")
            img = self.fill_image if (self.expect_fill or self.force_fill_image) else self.pred_image
            assert np.array_equal(ref["last0"], efo.bgr_to_intensity(img)), (str(self), "last0 comes from the expected image")
        for c in self.checks:
            c(ref)


def _plant(sc, kind):
    """one bad texel per chosen block, at each of the 16 positions in turn"""
    for k, (bx, by) in enumerate(chosen_blocks(sc.W, sc.H)):
        px, py = (k % 16) % 4, (k % 16) // 4
        x, y = 4 * bx + px, 4 * by + py
        sc.planted.append((x, y))
        for v4, n4 in ((sc.pred_vertex, sc.pred_normal), (sc.fill_vertex, sc.fill_normal)):
            if kind == "z0":
                v4[y, x, 2] = 0.0             # (x and y stay finite)
            elif kind == "xnan":
                v4[y, x, 0] = np.nan          # (z != 0)
            else:
                n4[y, x, 0] = np.nan          # (vertex valid)
    assert len(sc.planted) >= 16, "every position of a block is visited"
    # (a texel whose x alone is NaN keeps its camera-frame y / z on the oracle, tranformMaps writing x only, where the launch writes NaN: Q3)
    sc.exact_planes = kind == "z0"

    def check(ref):
        W, H = sc.W, sc.H
        bad = [np.zeros((H >> l, W >> l), bool) for l in range(3)]
        for (x, y) in sc.planted:
            for l in range(3):
                bad[l][y >> l, x >> l] = True
        for l in range(3):
            vbad, nbad = np.isnan(ref[f"vmap{l}"][:H >> l]), np.isnan(ref[f"nmap{l}"][:H >> l])
            if kind == "nnan":      # vertex and normal validity differ
                assert not vbad.any() and np.array_equal(nbad, bad[l]), (str(sc), l)
            elif kind == "xnan":    # the normal's x stays a number: the texel, its box and its block are invalid for vertices only
                assert np.array_equal(vbad, bad[l]) and not nbad.any(), (str(sc), l)
            else:
                assert np.array_equal(vbad, bad[l]) and np.array_equal(nbad, bad[l]), (str(sc), l)
    sc.checks.append(check)


def _plant_inf(sc):
    """blocks whose texels are all valid but hold +inf and -inf in x: in one 2 x 2 box (the level-1 average is NaN under a set valid flag), or
    in two boxes of the block (level 1 holds +inf and -inf, the level-2 average is NaN under a set valid flag); vertices and normals in turn"""
    sc.exact_planes = False
    sc.inf_blocks = []
    for k, (bx, by) in enumerate(chosen_blocks(sc.W, sc.H)):
        if k % 2:
            continue
        same_box, normals = (k // 2) % 2 == 0, (k // 4) % 2 == 1
        x, y = 4 * bx, 4 * by
        for v4, n4 in ((sc.pred_vertex, sc.pred_normal), (sc.fill_vertex, sc.fill_normal)):
            m = n4 if normals else v4
            m[y, x + 1, 0] = np.inf
            if same_box:
                m[y + 1, x, 0] = -np.inf
            else:
                m[y + 3, x + 2, 0] = -np.inf
        sc.inf_blocks.append((bx, by, same_box, normals))
    kinds = {(s, n) for (_, _, s, n) in sc.inf_blocks}
    assert len(kinds) == 4, kinds

    def check(ref):
        cam = ref["_cam"]
        for (bx, by, same_box, normals) in sc.inf_blocks:
            key = "nmap" if normals else "vmap"
            h0 = sc.H
            assert not np.isnan(cam[f"{key}0"][:h0][4 * by:4 * by + 4, 4 * bx:4 * bx + 4]).any(), "all sixteen sources are numbers"
            l1 = cam[f"{key}1"][:sc.H // 2][2 * by:2 * by + 2, 2 * bx:2 * bx + 2]
            if same_box:     # the level-1 box average (+inf + -inf) is NaN under a set valid flag, vertices and normals alike
                assert np.isnan(l1[0, 0]) and not np.isnan(l1[0, 1]) and not np.isnan(l1[1, 0]) and not np.isnan(l1[1, 1]), (str(sc), bx, by, l1)
            elif not normals:
                assert l1[0, 0] == np.inf and l1[1, 1] == -np.inf, (str(sc), bx, by, l1)    # level 1 valid, level 2 NaN under the flag
            else:            # a normal's average of +-inf is normalised: inf / inf, NaN under a set valid flag at level 1 already, in both boxes
                assert np.isnan(l1[0, 0]) and np.isnan(l1[1, 1]) and not np.isnan(l1[0, 1]) and not np.isnan(l1[1, 0]), (str(sc), bx, by, l1)
            assert np.isnan(ref[f"{key}2"][:sc.H // 4][by, bx]), (str(sc), bx, by)
            other = "vmap" if normals else "nmap"
            assert not np.isnan(ref[f"{other}2"][:sc.H // 4][by, bx]), (str(sc), bx, by, "the other map stays valid")
    sc.checks.append(check)


DEPTH_GATES = (F(MAX_DEPTH_RGB), np.nextafter(F(MAX_DEPTH_RGB), F(np.inf)), F(-0.0), F(-1.5), F(0.0))


def _plant_depth_gates(sc):
    sc.exact_planes = True
    sc.gated = []
    W, H = sc.W, sc.H
    for i in range(3, W * H, 7):
        x, y, g = i % W, i // W, DEPTH_GATES[(i // 7) % 5]
        sc.pred_vertex[y, x, 2] = sc.fill_vertex[y, x, 2] = g
        sc.gated.append((x, y, g))

    def check(ref):
        d, v0 = ref["depth0"], ref["vmap0"][:sc.H]
        seen = set()
        for (x, y, g) in sc.gated:
            k = DEPTH_GATES.index(g) if not (g == 0) else (2 if np.signbit(g) else 4)
            seen.add(k)
            if k == 0:
                assert d[y, x] == F(MAX_DEPTH_RGB) and not np.isnan(v0[y, x])      # z == maxDepthRGB passes
            elif k == 1:
                assert np.isnan(d[y, x]) and not np.isnan(v0[y, x])                 # one float above it does not; the vertex is valid
            elif k == 3:
                assert np.isnan(d[y, x]) and not np.isnan(v0[y, x])                 # a negative z is a valid vertex without a depth
            else:
                assert np.isnan(d[y, x]) and np.isnan(v0[y, x])                     # +0 and -0: no vertex, no depth
        assert seen == {0, 1, 2, 3, 4}, seen
    sc.checks.append(check)


def _threshold_counts(S):
    """(largest count that reads the fill-in, smallest count that reads the prediction) out of S samples, by the rule
    float(count) / float(S) > 0.75 evaluated in float32"""
    above = min(k for k in range(S + 1) if F(k) / F(S) > F(0.75))
    return above - 1, above


def _tally_image(sc, nonzero):
    """pred_image with `nonzero` non-zero sample texels; of the others the first has a single zero channel, the rest are zero in all three;
    every other texel is non-zero"""
    samples = sample_texels(sc.W, sc.H)
    assert 0 <= nonzero <= len(samples)
    for k, (x, y) in enumerate(samples[nonzero:]):
        sc.pred_image[y, x, :3] = (200, 0, 100) if k == 0 else (0, 0, 0)
    mask = np.ones((sc.H, sc.W), bool)
    for (x, y) in samples[nonzero:]:
        mask[y, x] = False
    assert (sc.pred_image[mask][:, :3] > 0).all()
    sc.tally, sc.dense_count = True, 77      # (a count the tally must overwrite)


MAP_SCENE_NAMES = ("bad_z0", "bad_xnan", "bad_nnan", "inf_averages", "depth0_gates", "source_below", "source_at", "source_above",
                   "tally_fill", "tally_pred", "tally_pred_force_fill_image", "camera_frame_z0", "camera_frame_xnan", "camera_frame_inf")


@functools.lru_cache(maxsize=None)
def map_scene(W, H, name):
    sc = MapScene(name, W, H)
    S = sc.dense_samples
    if name.startswith("bad_"):
        _plant(sc, name[4:])
    elif name == "inf_averages":
        _plant_inf(sc)
    elif name == "depth0_gates":
        _plant_depth_gates(sc)
    elif name.startswith("source_"):
        # tally off: the launch reads dense_count / dense_samples as it finds them.  9 / 12 is exactly 0.75 at every size (the samples
        # are the caller's here)
        sc.dense_samples = 12
        sc.dense_count = dict(below=8, at=9, above=10)[name[7:]]
        sc.expect_fill = name != "source_above"
    elif name.startswith("tally_"):
        below, above = _threshold_counts(S)
        if (W, H) == (80, 60):
            assert (below, above) == (9, 10)
        _tally_image(sc, below if name == "tally_fill" else above)
        sc.expect_fill = name == "tally_fill"
        sc.force_fill_image = name.endswith("force_fill_image")
        sc.checks.append(lambda ref, n=(below if name == "tally_fill" else above): _eq(ref["dense_count"], n))
    elif name.startswith("camera_frame_"):
        sc.camera_frame = True
        if name.endswith("inf"):
            _plant_inf(sc)
            sc.exact_planes = True      # resizeMapKernel alone writes the three averages as they come: nothing stale
        else:
            _plant(sc, name[13:])
            sc.exact_planes = True      # copyMaps + resize alone: an invalid texel of level 0 has all planes NaN, one of levels 1-2 keeps its y / z
    else:
        raise KeyError(name)
    return sc


def _eq(a, b):
    assert a == b, (a, b)


@functools.lru_cache(maxsize=None)
def map_oracle(W, H, name):
    """the oracle's result on a scene, computed once and read-only for every test that shares it"""
    return map_scene(W, H, name).oracle()


# ------------------------------------------------------------------------------------------------
# frame-side scenes: rgb + raw depth
# ------------------------------------------------------------------------------------------------
def intensity_np(rgb):
    """bgr2IntensityKernel on packed rgb (cudafuncs.cu:593), restated"""
    c = rgb.astype(F)
    return ((c[..., 0] * F(0.114) + c[..., 1] * F(0.299)) + c[..., 2] * F(0.587)).astype(np.int32).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _gray_for():
    """gray level g with intensity_np((g, g, g)) == v, for every v"""
    lut = {}
    for g in range(256):
        lut.setdefault(int(intensity_np(np.array([[[g, g, g]]], np.uint8))[0, 0]), g)
    assert all(v in lut for v in range(8, 251)), sorted(set(range(8, 251)) - set(lut))
    return np.array([lut.get(v, v) for v in range(256)], np.uint8)


def stripe_rows(H):
    """rows of the exact-gate stripes: the lower half of the image, short of the last two rows"""
    return H // 2 + 2, H - 3


def _near_gate(mt, elig, minScale):
    """Sobel units between the gate and the nearest eligible gradient magnitude (at or above it, below it)"""
    d = np.sqrt(mt[elig].astype(np.float64)) - np.sqrt(minScale)
    return (d[d >= 0].min() if (d >= 0).any() else np.inf), (-d[d < 0].max() if (d < 0).any() else np.inf)


def gates_reached(W, H, k, params):
    """the oracle's derivative images of levels 1 and 2 hold a gradient magnitude within one Sobel unit of the level's gate on EACH side of
    it, among the pixels the border and window gates let through"""
    img = efo.bgr_to_intensity(rgba_of(_frame_scene(W, H, k, *params)["rgb"]))
    for l in (1, 2):
        img = efo.pyr_down_uchar_gauss(img)
        dx, dy = efo.derivative_images(img)
        g = mask_gates(img, dx, dy, np.zeros(img.shape, F), MIN_SCALE[l])
        up, down = _near_gate(dx.astype(np.int64) ** 2 + dy.astype(np.int64) ** 2, g["border"] & g["window"], MIN_SCALE[l])
        if up > 1.0 or down > 1.0:
            return False
    return True


def search_texture(W, H, ks):
    """(amplitude of the first wave at the first row, its phase, amplitude and phase of the second wave): the first point of a fixed grid
    with gates_reached for every frame of ks.  A level of 9 x 7 pixels does not offer that by chance; TEXTURE holds what this search found
    (`python tests/inputscenes.py` prints the table), check_frame_oracle asserts the property itself."""
    grid = itertools.product(np.linspace(0.0, 2 * np.pi, 8, endpoint=False), (30.0, 20.0, 10.0), np.linspace(0.0, 0.6, 25),
                             np.linspace(0.0, 2 * np.pi, 32, endpoint=False))
    for q, amp2, amp0, ph in grid:
        params = (round(float(amp0), 6), round(float(ph), 6), amp2, round(float(q), 6))
        if all(gates_reached(W, H, k, params) for k in ks):
            return params
    return None


# One texture for the three frames of a size where the grid holds one (the frame tier's sizes: the frames are views of one surface); 36 x 28,
# whose level 2 has 24 pixels inside the border rule, gets one per frame and is not a frame-tier size (FRAME_SIZES below).
TEXTURE = {
    (36, 28, 0): (0.0, 0.785398, 20.0, 1.570796),
    (36, 28, 1): (0.325, 4.908739, 10.0, 0.785398),
    (36, 28, 2): (0.025, 1.963495, 10.0, 0.785398),
    (80, 60, 0): (0.025, 0.392699, 30.0, 0.0),
    (80, 60, 1): (0.025, 0.392699, 30.0, 0.0),
    (80, 60, 2): (0.025, 0.392699, 30.0, 0.0),
    (132, 36, 0): (0.075, 3.926991, 30.0, 0.0),
    (132, 36, 1): (0.075, 3.926991, 30.0, 0.0),
    (132, 36, 2): (0.075, 3.926991, 30.0, 0.0),
}


PATCH_FRAME = 3     # frame_scene's k of the patch variant
PATCH = 13          # level-0 pixels under one pixel of level 2 through two 5-tap steps: 4 X - 6 .. 4 X + 6


def _patched(W, H, Xi, Yi, Xd, Yd):
    """frame 0 with a square of zero intensity under level-2 pixel (Xi, Yi) and a square of zero depth under (Xd, Yd): what a single zero
    pixel or hole cannot do, both survive the two pyramid steps, so the window and the depth gate decide at levels 1 and 2 as well"""
    fr = _frame_scene(W, H, 0, *TEXTURE[(W, H, 0)])
    fr["rgb"][max(4 * Yi - 6, 0):4 * Yi + 7, max(4 * Xi - 6, 0):4 * Xi + 7] = 0
    fr["depth"][max(4 * Yd - 6, 0):4 * Yd + 7, max(4 * Xd - 6, 0):4 * Xd + 7] = 0
    return fr


def search_patches(W, H):
    """the first pair of level-2 pixels, row-major inside the border rule, for which check_patch_oracle holds (PATCHES keeps it)"""
    inside = [(X, Y) for Y in range((H >> 2) - 1) for X in range((W >> 2) - 5)]
    for (Xi, Yi), (Xd, Yd) in itertools.product(inside, inside):
        try:
            check_patch_oracle(_oracle_of(_patched(W, H, Xi, Yi, Xd, Yd), W, H), W, H)
            return Xi, Yi, Xd, Yd
        except AssertionError:
            continue
    return None


PATCHES = {(36, 28): (0, 0, 3, 0), (80, 60): (0, 0, 3, 0), (132, 36): (0, 0, 3, 0)}     # (Xi, Yi, Xd, Yd): what search_patches found


def frame_scene(W, H, k=0):
    """frame k (1, 2: slightly shifted views of the surface of frame 0; PATCH_FRAME: frame 0 with the two patches) of the frame-side scene:
    dict(rgb, depth, zeros, holes, gates)"""
    if k == PATCH_FRAME:
        return _patched(W, H, *PATCHES[(W, H)])
    return _frame_scene(W, H, k, *TEXTURE[(W, H, k)])


def _frame_scene(W, H, k, amp0, ph, amp2, q):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    xs, ys = x + 0.4 * k, y - 0.3 * k
    # texture: steep in x with a slope that grows along y (gradient magnitudes on both sides of every level's gate), reaching every border
    t = 128.0 + 70.0 * np.sin(2 * np.pi * xs / 13.0 + ph) * (amp0 + (1.0 - amp0) * (ys / H)) + amp2 * np.sin(2 * np.pi * ys / 11.0 + xs / 9.0 + q)
    inten = np.clip(np.rint(t), 8, 250).astype(np.uint8)
    # exact gates at level 0: vertical stripes a | b with b - a = 22 (Sobel 40: 40^2 = minScale) and 21 (Sobel 38: 1444, the nearest attainable
    # value below 1600 for a vertical edge: int(d * 1.83853) skips 39)
    r0, r1 = stripe_rows(H)
    inten[r0:r1, 4:8] = 60
    inten[r0:r1, 8:12] = 82
    inten[r0:r1, 12:16] = 103
    inten[r0:r1, 16:20] = 103
    zeros = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2 + 3, H - 1), (0, H // 2 - 3), (W - 1, H // 2 - 4),
             (W // 3, H // 3), (W - 9, H // 4 + 1)]
    rgb = np.repeat(_gray_for()[inten][..., None], 3, axis=2)
    for (zx, zy) in zeros:
        rgb[zy, zx] = (0, 0, 0)
    zx, zy = zeros[-1]
    rgb[zy, zx] = (1, 1, 0)        # a non-zero triple whose intensity is 0
    z = 1500.0 + 200.0 * (xs / W - 0.5) + 150.0 * (ys / H - 0.5) + 5.0 * np.sin(2 * np.pi * xs / 19.0) * np.cos(2 * np.pi * ys / 15.0)
    depth = np.rint(z).astype(np.uint16)
    holes = []
    blocks = [(bx, by) for by in range(1, H // 4 - 1) for bx in range(1, W // 4 - 1) if (bx + by) % 2 == 0]
    for i, (bx, by) in enumerate(blocks[:16]):     # one hole at each of the 16 positions of a 4 x 4 block
        holes.append((4 * bx + i % 4, 4 * by + i // 4))
    assert len(holes) == 16, (W, H, len(holes))
    holes += [(W - 1, 5), (W - 1, H // 2 + 1), (7, H - 1), (W // 2 + 5, H - 1)]     # the last column and the last row
    for (hx, hy) in holes:
        depth[hy, hx] = 0
    # the depth cut (3000 passes, 3001 does not) and the 300 mm gate (299 does not pass, 300 and 301 do), in the first rows
    gates = (3000, 3001, 299, 300, 301)
    for i, g in enumerate(gates):
        depth[1 + i // 3, 3 + 4 * (i % 3)] = g
    return dict(rgb=np.ascontiguousarray(rgb), depth=np.ascontiguousarray(depth), zeros=zeros, holes=holes,
                gates=[(3 + 4 * (i % 3), 1 + i // 3, g) for i, g in enumerate(gates)])


def rgba_of(rgb):
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = rgb
    return out


@functools.lru_cache(maxsize=None)
def frame_oracle(W, H, k=0):
    """the frame's side of the tracker inputs as the oracle's operators leave them (initICP(filteredDepth) + initRGB's image half), and a
    depth pyramid for the photometric gate made from the frame's own filtered depth"""
    return _oracle_of(frame_scene(W, H, k), W, H)


def _oracle_of(fr, W, H):
    fx, fy, cx, cy = intr(W, H)
    filtered = efo.filter_depth(fr["depth"], DEPTH_CUT)
    o = dict(frame=fr, filtered=filtered, depth_tmp=[filtered], nextImage=[efo.bgr_to_intensity(rgba_of(fr["rgb"]))])
    dmf = efo.metricise_depth(filtered, DEPTH_CUT)
    nd = dmf.copy()
    nd[dmf == 0] = np.nan
    o["nextDepth"] = [nd]
    for l in (1, 2):
        o["depth_tmp"].append(efo.pyr_down_u16(o["depth_tmp"][-1]))
        o["nextImage"].append(efo.pyr_down_uchar_gauss(o["nextImage"][-1]))
        o["nextDepth"].append(efo.pyr_down_gauss_f(o["nextDepth"][-1]))
    o["vmap_curr"], o["nmap_curr"], o["dIdx"], o["dIdy"], o["mask"] = [], [], [], [], []
    for l in range(3):
        d = 1 << l
        v = efo.create_vmap(o["depth_tmp"][l], fx / d, fy / d, cx / d, cy / d, DEPTH_CUT)
        o["vmap_curr"].append(v)
        o["nmap_curr"].append(efo.create_nmap(v))
        dx, dy = efo.derivative_images(o["nextImage"][l])
        o["dIdx"].append(dx)
        o["dIdy"].append(dy)
        o["mask"].append(rgb_mask(o["nextImage"][l], dx, dy, o["nextDepth"][l], MIN_SCALE[l]))
    return o


# ------------------------------------------------------------------------------------------------
# rgbMask: residualKernel's frame-invariant gates (reduce.cu:631-667, as sobel_mask_px cites), restated
# ------------------------------------------------------------------------------------------------
def mask_gates(nextImage, dIdx, dIdy, nextDepth, minScale):
    """the four gates, each as a boolean image: border (x < cols - 5 and y < rows - 1), window (no zero pixel of nextImage in rows
    y - 2 .. y + 1, columns x - 2 .. x + 1, clipped to the image: quirk Q10), gradient ((float)(dx^2 + dy^2) >= minScale), depth
    (nextDepth is a number)"""
    rows, cols = nextImage.shape
    y, x = np.mgrid[0:rows, 0:cols]
    border = (x < cols - 5) & (y < rows - 1)
    pos = np.ones((rows + 3, cols + 3), bool)          # padded: outside the image nothing is tested
    pos[2:rows + 2, 2:cols + 2] = nextImage > 0
    window = np.ones((rows, cols), bool)
    for a in range(4):
        for b in range(4):
            window &= pos[a:a + rows, b:b + cols]      # pos[y + a, x + b] is pixel (y - 2 + a, x - 2 + b)
    vx, vy = dIdx.astype(np.int32), dIdy.astype(np.int32)
    grad = (vx * vx + vy * vy).astype(F) >= F(minScale)
    depth = ~np.isnan(nextDepth)
    return dict(border=border, window=window, grad=grad, depth=depth)


def rgb_mask(nextImage, dIdx, dIdy, nextDepth, minScale):
    g = mask_gates(nextImage, dIdx, dIdy, nextDepth, minScale)
    return (g["border"] & g["window"] & g["grad"] & g["depth"]).astype(np.uint8)


def check_frame_oracle(o, W, H):
    """what every frame-side scene provokes, on the oracle's result alone"""
    fr = o["frame"]
    # depth: the normal map is NaN in the last column and row, and beside every hole (createNMap reads x + 1 and y + 1)
    n0 = o["nmap_curr"][0][:H]
    assert np.isnan(n0[:, W - 1]).all() and np.isnan(n0[H - 1, :]).all()
    v0 = o["vmap_curr"][0][:H]
    for (hx, hy) in fr["holes"]:
        assert o["filtered"][hy, hx] == 0 and np.isnan(v0[hy, hx]), (hx, hy)
        for (ax, ay) in ((hx, hy), (hx - 1, hy), (hx, hy - 1)):
            if ax >= 0 and ay >= 0:
                assert np.isnan(n0[ay, ax]), (hx, hy, ax, ay)
    got = {g: int(o["filtered"][y, x]) for (x, y, g) in fr["gates"]}
    assert got[3000] > 0 and got[3001] == 0 and got[299] == 0 and got[300] > 0 and got[301] > 0, got
    # intensity: the planted zeros are zeros of nextImage[0], the non-zero triple among them
    for (zx, zy) in fr["zeros"]:
        assert o["nextImage"][0][zy, zx] == 0, (zx, zy)
    zx, zy = fr["zeros"][-1]
    assert fr["rgb"][zy, zx].any()
    for l in range(3):
        rows, cols = H >> l, W >> l
        g = mask_gates(o["nextImage"][l], o["dIdx"][l], o["dIdy"][l], o["nextDepth"][l], MIN_SCALE[l])
        m = o["mask"][l].astype(bool)
        frac = m.mean()
        assert 0.10 <= frac <= 0.90, ("both values of the mask on at least a tenth of the pixels", l, frac)
        # each gate decides alone somewhere, and passes somewhere (single zero pixels and single holes do not survive the pyramids: here the
        # window and the depth gate decide at level 0; at levels 1 and 2 they do in the patch variant, check_patch_oracle)
        for name in ("border", "grad") + (("window", "depth") if l == 0 else ()):
            others = np.ones_like(m)
            for k, v in g.items():
                if k != name:
                    others &= v
            assert (others & ~g[name]).any() and (others & g[name]).any(), ("gate hit on each side", l, name)
        # the border rule alone masks columns cols - 5 .. cols - 1 and row rows - 1: the texture reaches them
        inner = g["window"] & g["grad"] & g["depth"]
        for c in range(cols - 5, cols):
            assert inner[:rows - 1, c].any() and not m[:, c].any(), (l, c)
        assert inner[rows - 1, :cols - 5].any() and not m[rows - 1].any(), l
        assert inner[:, cols - 6].any() and m[:, cols - 6].any() and m[rows - 2].any(), l
        # the gradient gate at its exact value
        mt = (o["dIdx"][l].astype(np.int64) ** 2 + o["dIdy"][l].astype(np.int64) ** 2)
        elig = g["border"] & g["window"] & g["depth"]
        if l == 0:
            assert (mt[elig] == 1600).any() and (mt[elig] == 1444).any(), "Sobel 40 and 38 on the stripes"
            assert m[elig & (mt == 1600)].all() and not m[elig & (mt == 1444)].any()
        else:   # the nearest attainable pairs around the gate: within one Sobel unit on each side
            mag, gate = np.sqrt(mt[elig].astype(np.float64)), np.sqrt(MIN_SCALE[l])
            assert ((mag >= gate) & (mag <= gate + 1)).any() and ((mag < gate) & (mag >= gate - 1)).any(), (l, np.sort(np.abs(mag - gate))[:4])
    # the window's reach (quirk Q10): a zero pixel two columns to the left or two rows above decides, outside the 3 x 3 Sobel taps
    g0 = mask_gates(o["nextImage"][0], o["dIdx"][0], o["dIdy"][0], o["nextDepth"][0], MIN_SCALE[0])
    img = o["nextImage"][0]
    far = np.zeros_like(g0["window"])
    for (zy, zx) in zip(*np.nonzero(img == 0)):
        for (px, py) in ((zx + 2, zy), (zx + 2, zy + 1), (zx, zy + 2), (zx + 1, zy + 2), (zx + 2, zy + 2)):
            if px < W and py < H:
                far[py, px] = True
    assert (far & g0["border"] & g0["grad"] & g0["depth"] & ~g0["window"]).any(), "a pixel masked by the window's far row / column alone"


def check_patch_oracle(o, W, H):
    """the patch variant: at EVERY level the window gate and the depth gate each decide alone somewhere and pass somewhere, and the mask
    keeps both values"""
    for l in range(3):
        g = mask_gates(o["nextImage"][l], o["dIdx"][l], o["dIdy"][l], o["nextDepth"][l], MIN_SCALE[l])
        m = o["mask"][l].astype(bool)
        assert m.any() and not m.all(), l
        for name in ("window", "depth"):
            others = np.ones_like(m)
            for k, v in g.items():
                if k != name:
                    others &= v
            assert (others & ~g[name]).any() and (others & g[name]).any(), ("gate hit on each side", l, name)


def identity_residual(o, l, lastImage=None):
    """efo.rgb_residual of level l under identity motion (kt = 0, krkinv = I), nextDepth on both sides"""
    li = o["nextImage"][l] if lastImage is None else lastImage
    return efo.rgb_residual(MIN_SCALE[l], o["dIdx"][l], o["dIdy"][l], o["nextDepth"][l], o["nextDepth"][l], li, o["nextImage"][l], 0.07,
                            np.zeros(3, F), np.eye(3, dtype=F))


# ------------------------------------------------------------------------------------------------
# frame tier: a checkpoint whose map is a trackable slanted textured surface with planted holes and an uncovered region
# ------------------------------------------------------------------------------------------------
# The sizes at which the oracle tracks both frames (ICP and RGB counts above a fifth of the pixels).  At 36 x 28 it does not: level 2 is
# 9 x 7 pixels, the second frame's normal equations come out singular (statistics NaN, counts 0) and the first frame's RGB count is 151 of
# 1008 — the size stays an operator-tier size.
FRAME_SIZES = [(80, 60), (132, 36)]


def fusion_kw(W, H, **kw):
    fx, fy, cx, cy = intr(W, H)
    d = dict(width=W, height=H, fx=fx, fy=fy, cx=cx, cy=cy, confidence=0.05, maxSurfels=1 << 16)
    d.update(kw)
    return d


@functools.lru_cache(maxsize=None)
def checkpoint(W, H, covered=0.5):
    """The map the oracle seeds from frame 0, every surfel confident, minus the surfels of the left-hand part of the view (uncovered, with
    the only sample texel of 36 x 28 in it, for the cases that run at that size: the restore's prediction is not dense enough, the first tracked frame reads the fill-in) and of
    a few planted holes."""
    fr = frame_scene(W, H, 0)
    o = efo.Fusion(**fusion_kw(W, H))
    o.process_frame(fr["rgb"], fr["depth"], 0)
    m = o.map().copy()
    fx, fy, cx, cy = intr(W, H)
    u = m[:, 0] / m[:, 2] * fx + cx
    v = m[:, 1] / m[:, 2] * fy + cy
    keep = u >= (1.0 - covered) * W
    for (hx, hy) in ((W - W // 5, H // 3), (W - W // 4 - 2, H // 2 + 3), (W - 5, H - 6)):
        keep &= ~((np.abs(u - hx) < 1.5) & (np.abs(v - hy) < 1.5))
    m = np.ascontiguousarray(m[keep])
    m[:, 3] = 20.0
    return dict(map=m, tick=o.tick(), qt=o.pose_qt(), rgb=fr["rgb"], depth=fr["depth"])


if __name__ == "__main__":
    print("TEXTURE = {")
    for (W, H) in SIZES:
        joint = search_texture(W, H, (0, 1, 2))
        for k in (0, 1, 2):
            print(f"    ({W}, {H}, {k}): {joint or search_texture(W, H, (k,))},")
    print("}")
