"""tests/inputscenes.py on the oracle alone (no GPU): every scene provokes what it claims, the numpy restatement of the frame-invariant
photometric gates (rgbMask) is residualKernel's under identity motion, and the frame-tier checkpoint gives the oracle a frame it tracks.
"""
import numpy as np
import pytest

import efo
import inputscenes as S

SIZE_IDS = dict(ids=S.size_id)


@pytest.mark.parametrize("size", S.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("name", S.MAP_SCENE_NAMES)
def test_model_map_scene_provokes_what_it_claims(size, name):
    sc = S.map_scene(*size, name)
    ref = S.map_oracle(*size, name)
    sc.check(ref)
    W, H = size
    for l in range(3):
        assert ref[f"vmap{l}"].shape == (3 * (H >> l), W >> l)
    # the surface is valid and posed: untouched texels are numbers, and far from where a missed `+ t` or R would leave them
    v0 = ref["vmap0"][:H]
    assert (~np.isnan(v0)).mean() > 0.5
    if not sc.camera_frame:
        src = (sc.fill_vertex if ref["_fill"] else sc.pred_vertex)
        world = np.stack([ref["vmap0"][p * H:(p + 1) * H] for p in range(3)], axis=-1)
        ok = ~np.isnan(v0) & np.isfinite(src[..., 0])
        assert np.linalg.norm(world[ok] - src[..., :3][ok], axis=-1).min() > 1.0, "the pose moves every vertex by more than a metre"
        assert np.abs(np.linalg.norm(world[ok] - S.POSE_T, axis=-1) - np.linalg.norm(src[..., :3][ok], axis=-1)).max() < 1e-3, "by R, then t"


@pytest.mark.parametrize("size", S.SIZES, **SIZE_IDS)
def test_prediction_and_fill_in_differ_in_every_texel(size):
    sc = S.map_scene(*size, "source_at")
    assert (sc.pred_vertex[..., 2] != sc.fill_vertex[..., 2]).all() and (sc.pred_normal[..., :3] != sc.fill_normal[..., :3]).any(axis=-1).all()
    assert (efo.bgr_to_intensity(sc.pred_image) != efo.bgr_to_intensity(sc.fill_image)).all()


def test_verdicts_around_three_quarters():
    assert [S.verdict(k, 12) for k in (8, 9, 10)] == [False, False, True]
    assert S._threshold_counts(12) == (9, 10) and S._threshold_counts(1) == (0, 1) and S._threshold_counts(6) == (4, 5)
    sc9, sc10 = S.map_scene(80, 60, "tally_fill"), S.map_scene(80, 60, "tally_pred")
    assert S.map_oracle(80, 60, "tally_fill")["dense_count"] == 9 and S.map_oracle(80, 60, "tally_pred")["dense_count"] == 10
    for sc in (sc9, sc10):   # one sample texel with a single zero channel
        px = [sc.pred_image[y, x, :3] for (x, y) in S.sample_texels(80, 60)]
        assert sum(1 for p in px if (p == 0).sum() == 1) == 1


@pytest.mark.parametrize("size", S.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("k", (0, 1, 2))
def test_frame_scene_provokes_what_it_claims(size, k):
    W, H = size
    o = S.frame_oracle(W, H, k)
    assert np.array_equal(o["nextImage"][0], S.intensity_np(o["frame"]["rgb"])), "the intensity restatement is the oracle's"
    S.check_frame_oracle(o, W, H)


@pytest.mark.parametrize("size", S.SIZES, **SIZE_IDS)
def test_patch_variant_reaches_the_window_and_depth_gates_at_every_level(size):
    W, H = size
    assert S.search_patches(W, H) == S.PATCHES[size], "the table is what the search finds"
    S.check_patch_oracle(S.frame_oracle(W, H, S.PATCH_FRAME), W, H)


@pytest.mark.parametrize("size", S.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("k", (0, 1, 2, S.PATCH_FRAME))
@pytest.mark.parametrize("level", (0, 1, 2))
def test_rgb_mask_restatement_is_the_residual_kernels(size, level, k):
    """Under identity motion every pixel looks itself up: what residualKernel accepts is the frame-invariant mask and the three tests on the
    other image.  lastImage: the frame's own with planted zeros, so that the `lastImage != 0` half decides somewhere."""
    W, H = size
    o = S.frame_oracle(W, H, k)
    last = o["nextImage"][level].copy()
    last[::3, 1::4] = 0
    corres, sigma, count = S.identity_residual(o, level, last)
    valid = corres["valid"].astype(bool)
    mask = o["mask"][level].astype(bool)
    nd = o["nextDepth"][level]
    assert valid.any() and not (valid & ~mask).any(), "valid is a subset of the mask"
    with np.errstate(invalid="ignore"):
        expect = mask & (nd > 0) & (last != 0)      # (in bounds: every pixel projects onto itself)
    assert np.array_equal(valid, expect), int((valid != expect).sum())
    assert (mask & ~valid).any(), "the other image's tests decide somewhere"
    assert count == int(valid.sum())
    ys, xs = np.nonzero(valid)
    assert np.array_equal(corres["zero"][valid], np.stack([xs, ys], axis=1)) and np.array_equal(corres["one"][valid], np.stack([xs, ys], axis=1))


@pytest.mark.parametrize("size", S.FRAME_SIZES, **SIZE_IDS)
def test_checkpoint_gives_the_oracle_two_frames_it_tracks(size):
    """first tracked frame from the fill-in (the uncovered region), the second from the prediction; both really track"""
    W, H = size
    o = efo.Fusion(**S.fusion_kw(W, H))
    o.restore(S.checkpoint(W, H))
    cam = efo.make_cam(W, H, *S.intr(W, H))
    verdicts = []
    for k in (1, 2):
        verdicts.append(efo.dense_enough(cam, o.buffer("image")))
        fr = S.frame_scene(W, H, k)
        o.process_frame(fr["rgb"], fr["depth"], k)
        st = o.stats()
        assert st[1] > W * H / 5 and st[3] > W * H / 5, (k, st, W * H)
    assert verdicts == [False, True], verdicts
