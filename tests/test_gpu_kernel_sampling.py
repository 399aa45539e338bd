"""HIP-event sampling of the dominant kernels (ef_kernel_timing, ef_get_kernel_timing, ef_get_tracker_timing, ef_get_splat_timing;
include/ef_hip.h; host code in elasticfusion_amd/csrc/ef_host_inspect.inc).  bench.py's roofline leg is their only other user.

Six synthetic frames at 100 x 76 (the smallest size test_gpu_frame.py tracks and fuses at), sampling every frame, under the persistent
tracker launch and under the launch-per-step script.  What is sampled follows from the frame script:
  * frame 0 seeds the map: it neither tracks nor fuses; frames 1..5 track and fuse (no relocalisation: every tracked frame fuses);
  * launch-per-step script: the level-0 normal-equation launch of every level-0 iteration is sampled: 10 iterations (fastOdom off)
    per tracked frame; the persistent launch is not run, so ef_get_tracker_timing reports 0 launches;
  * persistent launch: the one launch of a tracked frame is sampled; no level-0 launch of its own exists, so ef_get_kernel_timing reports 0;
  * the point splat of a fusing frame's first predictIndices is sampled once per fusing frame.
The byte figures are the formulas in the comments of the three getters, for the default ICP + RGB configuration."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, FRAMES = 100, 76, 6
TRACKED = FUSED = FRAMES - 1
LEVEL0_ITERATIONS = 10          # RGBDOdometry.cpp:371-373, fastOdom off


@pytest.fixture(scope="module")
def hip():
    from elasticfusion_amd import api
    return api


@pytest.fixture(scope="module")
def scene():
    from elasticfusion_amd import synth
    sq = synth.Sequence(seed=0xEF0003, width=W, height=H)
    return dict(width=W, height=H, fx=sq.fx, fy=sq.fy, cx=sq.cx, cy=sq.cy), [sq.frame(k)[:2] for k in range(FRAMES + 1)]


def start(hip, scene, persistent, every):
    ef = hip.ElasticFusion(maxSurfels=1 << 19, **scene[0])
    ef.setPersistentTracker(persistent)
    if every:
        hip._chk(hip.lib().ef_kernel_timing(ef.h, every), ef.h)
    for k in range(FRAMES):
        ef.processFrame(*scene[1][k], k * 33333)
    return ef


def sampled(hip, ef):
    out = {}
    for key, fn in (("step", "ef_get_kernel_timing"), ("tracker", "ef_get_tracker_timing"), ("splat", "ef_get_splat_timing")):
        t = hip.ef_kernel_time()
        hip._chk(getattr(hip.lib(), fn)(ef.h, C.byref(t)), ef.h)
        assert t.name
        print(key, t.launches, t.avg_us, t.bytes_per_launch, t.bytes_per_launch_survey)
        out[key] = t
    return out


@pytest.mark.parametrize("persistent", [1, 0])
def test_sample_counts_bytes_restart_and_unchanged_results(hip, scene, persistent):
    plain = start(hip, scene, persistent, 0)
    poses, count, surfels = plain.trajectory()[0], plain.lastCount(), plain.downloadMap()
    plain.close()
    ef = start(hip, scene, persistent, 1)
    t = sampled(hip, ef)
    assert t["step"].launches == (0 if persistent else LEVEL0_ITERATIONS * TRACKED)
    assert t["tracker"].launches == (TRACKED if persistent else 0)
    assert t["splat"].launches == FUSED
    for k in t.values():
        assert (k.avg_us > 0) == (k.launches > 0), (k.name, k.launches, k.avg_us)
    # 48 B per pixel-visit of icpStep + the 4-byte packed correspondence of rgbStep; the survey's numerator is the ICP reduction alone
    visits = sum(it * (W >> l) * (H >> l) for l, it in enumerate((LEVEL0_ITERATIONS, 5, 4)))
    assert (t["step"].bytes_per_launch, t["step"].bytes_per_launch_survey) == (52.0 * W * H, 48.0 * W * H)
    assert (t["tracker"].bytes_per_launch, t["tracker"].bytes_per_launch_survey) == (52.0 * visits, 48.0 * visits)
    assert ef.lastCount() == count and count > 0
    assert (t["splat"].bytes_per_launch, t["splat"].bytes_per_launch_survey) == (40.0 * count, 48.0 * count)
    # sampling changes no result: the sampled launches are the same kernels with a start and a stop event
    assert np.array_equal(ef.trajectory()[0].view(np.uint64), poses.view(np.uint64))
    assert np.array_equal(ef.downloadMap().view(np.uint32), surfels.view(np.uint32))
    # off and on again: the counts start from 0, and one more frame adds one frame's samples
    hip._chk(hip.lib().ef_kernel_timing(ef.h, 0), ef.h)
    hip._chk(hip.lib().ef_kernel_timing(ef.h, 1), ef.h)
    assert [k.launches for k in sampled(hip, ef).values()] == [0, 0, 0]
    ef.processFrame(*scene[1][FRAMES], FRAMES * 33333)
    assert [k.launches for k in sampled(hip, ef).values()] == ([0, 1, 1] if persistent else [LEVEL0_ITERATIONS, 0, 1])
    ef.close()
