"""Which script eft::track() runs (elasticfusion_amd/csrc/ef_track_host_track.inc: the script plan) never changes what it computes.  Synthetic frames
on device pointers; every case must leave the same trajectory, map count and map as its plain run, bit for bit, with no persistent launch fallen back
to one workgroup and a synchronize() that succeeds (no barrier timed out, no sticky abort word lost or invented at a switch).
  (a) ONE context at 640 x 480 whose ef_set_persistent_tracker is switched between frames through 1, 0, 2, 1, 2, 0: every switch clears the exchange
      areas and carries their sticky words over on the host.  Full size because mode 2's split exists only above PT_MAX_PIXELS = 131072 pixels:
      there level 0 runs one launch per step behind the launch of the small levels;
  (b) 100 x 76 with graph replay on, persistent 1 and 0: a captured tracker runs the per-step script whatever the option says;
  (c) 100 x 76 rgbOnly, persistent 1 against 0: rgbOnly keeps the per-step script;
  (d) 100 x 76 without the pyramid, persistent 1 against 0: one level, first_level = 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = 8
SWITCHES = (1, 0, 2, 1, 2, 0)   # set before frames 1..6 (frame 0 tracks nothing); frame 7 keeps the last


@pytest.fixture(scope="module")
def hip():
    from elasticfusion_amd import api
    return api


def make_scene(hip, w, h):
    from elasticfusion_amd import synth
    sq = synth.Sequence(seed=0xEF0003, width=w, height=h)
    dev = []
    for k in range(FRAMES):
        rgb, depth, _ = sq.frame(k)
        dev.append((hip.DevBuf.from_array(rgb), hip.DevBuf.from_array(depth)))
    return dict(width=w, height=h, fx=sq.fx, fy=sq.fy, cx=sq.cx, cy=sq.cy), dev


@pytest.fixture(scope="module")
def small(hip):
    return make_scene(hip, 100, 76)


def run(hip, scene, setup=None, before_frame=None):
    """-> (trajectory, map count, map) after FRAMES frames; setup(ef) before the first frame, before_frame(ef, k) before frame k"""
    kw, dev = scene
    ef = hip.ElasticFusion(maxSurfels=1 << 19, **kw)
    if setup:
        setup(ef)
    for k in range(FRAMES):
        if before_frame:
            before_frame(ef, k)
        ef.processFrameDevice(dev[k][0].p.value, dev[k][1].p.value, k * 33333)
    ef.synchronize()
    assert ef.trackerFallbacks() == 0
    out = ef.trajectory()[0], ef.lastCount(), ef.downloadMap()
    ef.close()
    return out


def assert_same(got, want):
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)), np.abs(got[0] - want[0]).max()
    assert got[1] == want[1] and want[1] > 0
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


def test_script_switched_between_frames_of_one_context(hip):
    scene = make_scene(hip, 640, 480)
    want = run(hip, scene)

    def before_frame(ef, k):
        if 1 <= k <= len(SWITCHES):
            ef.setPersistentTracker(SWITCHES[k - 1])
    assert_same(run(hip, scene, before_frame=before_frame), want)


@pytest.fixture(scope="module")
def small_plain(hip, small):
    return run(hip, small)


@pytest.mark.parametrize("persistent", (1, 0))
def test_graph_replay_runs_the_per_step_script(hip, small, small_plain, persistent):
    def setup(ef):
        ef.setGraphReplay(True)
        ef.setPersistentTracker(persistent)
    assert_same(run(hip, small, setup), small_plain)


def with_option(option, persistent):
    def setup(ef):
        option(ef)
        ef.setPersistentTracker(persistent)
    return setup


def test_rgb_only_keeps_the_per_step_script(hip, small):
    want = run(hip, small, with_option(lambda ef: ef.setRgbOnly(True), 0))
    assert_same(run(hip, small, with_option(lambda ef: ef.setRgbOnly(True), 1)), want)


def test_one_level_without_the_pyramid(hip, small):
    want = run(hip, small, with_option(lambda ef: ef.setPyramid(False), 0))
    assert_same(run(hip, small, with_option(lambda ef: ef.setPyramid(False), 1)), want)
