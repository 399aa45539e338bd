"""The map prediction passes on hand-built edge scenes (tests/splatscenes.py), operator tier and frame tier, bit for bit against the oracle.

Operator tier: every scene at 36 x 28, 52 x 36 (ragged 16 x 16 resolve tiles in both axes) and 12 x 44 (narrower than one tile: the second
wavefront column of every tile lies outside the image); W != H everywhere, so a row-major / column-major mix-up cannot cancel.  A scene's
check() runs on the oracle's result BEFORE the device is asked.  Runs k_index_splat<false>, k_index_resolve, k_surface_splat<false>,
k_surface_resolve<false>, k_depth_resolve, k_fill_in, k_dense_count, k_seed_flags / k_seed_scatter.

Frame tier: a checkpoint whose map is a surface scene, restored into the engine and into the oracle: the restore's own prediction runs
k_surface_splat<true> (ray table) and k_surface_resolve<true> (fused fill-in), the frame after it k_index_splat<true> (merge while
splatting) on a map with edge surfels.

Two findings of these scenes were fixed with them ("Ties at zero and NaN corners"): fragments at +0 and -0 tie in the
z-buffer key (surface_signed_zeros_*), and the sprite's point size follows GLSL's min / max to the letter (surface_nan_corner_*,
surface_nan_axis).
"""
import functools

import numpy as np
import pytest

import efo
import splatscenes as S
from test_gpu_ops_tracking import bits_equal

pytestmark = pytest.mark.gpu

NAMES = list(S.SPLAT_SCENE_NAMES)      # (static: collecting this module builds no scene)
OUTPUTS = dict(index=("index", "vertConf", "colorTime", "normRad"), surface=("image", "vertex", "normal", "time", "depth"))


@pytest.fixture(scope="module")
def api():
    from elasticfusion_amd import api
    return api


@functools.lru_cache(maxsize=None)
def scene(W, H, k):
    return S.splat_scene(W, H, k)


def differing(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return int((a.view(np.uint8) != b.view(np.uint8)).reshape(a.shape[0] * a.shape[1], -1).any(axis=1).sum())


@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
def test_splat_scene(api, size, k):
    sc = scene(*size, k)
    ref = sc.run(efo, efo.make_cam(*sc.cam))
    sc.check(ref)                                   # the scene does its job on the oracle ...
    got = sc.run(api.ops, api.ef_cam(*sc.cam))      # ... before the device is asked
    for name, a, b in zip(OUTPUTS[sc.kind], got, ref):
        print(f"{sc} {name}: {differing(a, b)} of {a.shape[0] * a.shape[1]} pixels differ")
    for name, a, b in zip(OUTPUTS[sc.kind], got, ref):
        assert bits_equal(a, b), (str(sc), name, differing(a, b))


@pytest.mark.parametrize("size", S.FILL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fill_in_selectors_borders_and_modes(api, size):
    W, H = size
    inp, check = S.fill_scene(W, H)
    args = (inp["image"], inp["vertex"], inp["normal"], inp["depth"], inp["rgb"])
    ocam, cam = efo.make_cam(W, H, S.FX, S.FY, W / 2.0, H / 2.0), api.ef_cam(W, H, S.FX, S.FY, W / 2.0, H / 2.0)
    ref = {m: efo.fill_in(ocam, *args, *m) for m in ((0, 0), (1, 1), (1, 0), (0, 1))}
    check(ref[(0, 0)], ref[(1, 1)])
    for m, r in ref.items():
        got = api.ops.fill_in(cam, *args, *m)
        for name, a, b in zip(("fill_image", "fill_vertex", "fill_normal"), got, r):
            assert bits_equal(a, b), (m, name, differing(a, b))


@pytest.mark.parametrize("case", S.dense_cases(), ids=lambda c: c[0])
def test_dense_enough_sample_grids(api, case):
    name, W, H, image, expected = case
    assert efo.dense_enough(efo.make_cam(W, H, S.FX, S.FY, W / 2.0, H / 2.0), image) == expected
    assert api.ops.dense_enough(api.ef_cam(W, H, S.FX, S.FY, W / 2.0, H / 2.0), image) == expected


@pytest.mark.parametrize("size", S.SEED_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_seed_map_partial_chunks(api, size):
    W, H = size
    inp, check = S.seed_scene(W, H)
    ref = efo.seed_map(efo.make_cam(W, H, S.FX, S.FY, W / 2.0, H / 2.0), inp["rgb"], inp["dm"], inp["dmf"], inp["time"], inp["maxDepth"])
    check(ref)
    got = api.ops.seed_map(api.ef_cam(W, H, S.FX, S.FY, W / 2.0, H / 2.0), inp["rgb"], inp["dm"], inp["dmf"], inp["time"], inp["maxDepth"])
    assert got.shape == ref.shape and bits_equal(got, ref)


# ---- frame tier ----
FRAME_SCENES = ("surface_ties", "surface_fragment_counts", "surface_edge_centres_x", "surface_corners", "surface_signed_zeros_1",
                "surface_nan_corner_last", "surface_nan_corner_first", "surface_negative_depths")


@pytest.mark.parametrize("size", [(36, 28), (52, 36)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", FRAME_SCENES)
def test_restored_surface_scene_and_the_frame_after_it(api, size, name):
    """tick 2, identity pose, a flat depth frame.  restore() predicts from the uploaded map (ray table, fused fill-in); the frame after it,
    its pose injected, merges while it splats the index map.  The oracle keeps every buffer compared here."""
    W, H = size
    sc = scene(W, H, NAMES.index(name))
    assert sc.time == 2 and sc.conf == 1.0 and sc.timeDelta == S.TD_OPEN and sc.maxDepth == S.MAXD and sc.cam == (W, H, S.FX, S.FY, W / 2.0, H / 2.0)
    sc.check(sc.run(efo, efo.make_cam(*sc.cam)))
    rng = np.random.RandomState(3)
    rgb = rng.randint(1, 256, size=(H, W, 3)).astype(np.uint8)
    depth = np.full((H, W), 1500, np.uint16)
    ck = dict(map=sc.surf, tick=2, qt=np.array([0, 0, 0, 1, 0, 0, 0], np.float64), rgb=rgb, depth=depth)
    kw = dict(width=W, height=H, fx=S.FX, fy=S.FY, cx=W / 2.0, cy=H / 2.0, confidence=1.0, maxSurfels=1 << 16)
    ef, o = api.ElasticFusion(**kw), efo.Fusion(**kw)
    try:
        ef.restore(ck)
        o.restore(ck)
        ref = {n: o.buffer(n) for n in ("image", "vertex", "normal", "time", "fill_image", "fill_vertex", "fill_normal")}
        assert bits_equal(ref["vertex"], sc.run(efo, efo.make_cam(*sc.cam))[1]), "the restored prediction is the scene's"
        for n, r in ref.items():
            assert bits_equal(ef.image(n), r), (n, differing(ef.image(n), r))
        ef.processFrame(rgb, depth, 1, in_T_wc=np.eye(4))
        o.process_frame(rgb, depth, 1, T_wc=np.eye(4))
        for n in ("index", "vertConf", "colorTime", "normRad"):
            assert bits_equal(ef.image(n), o.buffer(n)), (n, differing(ef.image(n), o.buffer(n)))
        assert ef.lastCount() == o.map_count() > len(sc.surf)
        assert bits_equal(ef.downloadMap(), o.map())
    finally:
        ef.close()
