"""The hand-built edge scenes of tests/splatscenes.py, on the CPU.

1. Every scene's check() against the oracle: a scene that stops doing what it was written for (a tie that is no tie any more, a sprite
   that misses the border) fails here, without a GPU.
2. The predict_indices and combined_predict / synthesize_depth scenes through the REFERENCE's own shaders compiled for the CPU
   (oracle/_ref/libefr_glsl.so, the bridge's fixed-function rules N1-N3): the oracle has to equal them bit for bit on every scene.  This
   is what decides who is right where the device and the oracle disagree: +0 against -0 in the z-buffer (they tie, the lower id wins,
   the winner's own zero comes out) and a sprite with NaN corners (GLSL's min / max to the letter, N6).
"""
import numpy as np
import pytest

import efo
import splatscenes as S
import trackops


def cam_of(W, H):
    return efo.make_cam(W, H, S.FX, S.FY, W / 2.0, H / 2.0)


def test_every_scene_does_its_job_on_the_oracle():
    n = 0
    for W, H in S.SIZES:
        for sc in S.splat_scenes(W, H):
            sc.check(sc.run(efo, efo.make_cam(*sc.cam)))
            n += 1
    assert n == 90, n
    for W, H in S.FILL_SIZES:
        inp, check = S.fill_scene(W, H)
        args = (cam_of(W, H), inp["image"], inp["vertex"], inp["normal"], inp["depth"], inp["rgb"])
        check(efo.fill_in(*args), efo.fill_in(*args, 1, 1))
    for name, W, H, image, expected in S.dense_cases():
        assert efo.dense_enough(cam_of(W, H), image) == expected, name
    for W, H in S.SEED_SIZES:
        inp, check = S.seed_scene(W, H)
        check(efo.seed_map(cam_of(W, H), inp["rgb"], inp["dm"], inp["dmf"], inp["time"], inp["maxDepth"]))


@pytest.mark.skipif(not efo.have_reference_glsl(), reason="oracle/_ref/libefr_glsl.so absent and /root/reference not present to build it")
def test_oracle_equals_the_compiled_shaders_on_every_splat_scene():
    so = efo.reference_glsl_lib()
    so.efg_use_specified_exp(1)
    so.efg_set_depth_compare(1)     # N2 as specified: depth test on the camera-space z
    for W, H in S.SIZES:
        for sc in S.splat_scenes(W, H):
            cam = efo.make_cam(*sc.cam)
            with efo.backend("reference_glsl"):
                ref = sc.run(efo, cam)
            with efo.backend("nofma"):
                got = sc.run(efo, cam)
            sc.check(got)
            for k, (a, b) in enumerate(zip(got, ref)):
                assert a.shape == b.shape and trackops.bits_differ(a, b) == 0, (sc, k)
