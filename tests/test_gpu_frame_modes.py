"""Pairs of frame modes that the other GPU tests switch on one at a time (elasticfusion_amd/csrc/ef_host_frame.inc: plan_frame and the stages of
process_frame).  Eight synthetic frames at 100 x 76; a plain single-stream run on device-pointer frames is the baseline, and every mode pair
must leave the same trajectory, map count and map, bit for bit: the modes change where and when work is enqueued, never what is computed.
  (a) stage timers on in every frame (no overlap, no joint input launch, resolved index maps, the update pass a launch of its own);
  (b) kernel sampling every 2nd frame with graph replay on: sampled frames leave the replay, the others use it;
  (c) host-pointer frames with input overlap 1;
  (d) input overlap 2 on a quarter of the CUs with the persistent tracker on (mode 2 is demoted to mode 1);
  (e) a pose handed in for one middle frame, single-stream against overlapped;
  (f) loop closure with the built-in solver, single-stream against overlapped."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, FRAMES = 100, 76, 8


@pytest.fixture(scope="module")
def hip():
    from elasticfusion_amd import api
    return api


@pytest.fixture(scope="module")
def scene(hip):
    from elasticfusion_amd import synth
    sq = synth.Sequence(seed=0xEF0003, width=W, height=H)
    frames = [sq.frame(k) for k in range(FRAMES)]
    dev = [(hip.DevBuf.from_array(rgb), hip.DevBuf.from_array(depth)) for rgb, depth, _ in frames]
    return dict(width=W, height=H, fx=sq.fx, fy=sq.fy, cx=sq.cx, cy=sq.cy), frames, dev


def run(hip, scene, setup=None, host=False, pose_at=None, **ctor):
    """-> (trajectory, map count, map, per-frame local-loop flags) after FRAMES frames; setup(ef) switches the modes on before the first frame"""
    kw, frames, dev = scene
    ef = hip.ElasticFusion(maxSurfels=1 << 19, **kw, **ctor)
    if setup:
        setup(ef)
    loops = []
    for k, (rgb, depth, T) in enumerate(frames):
        T_in = T if k == pose_at else None
        if host:
            ef.processFrame(rgb, depth, k * 33333, in_T_wc=T_in)
        else:
            ef.processFrameDevice(dev[k][0].p.value, dev[k][1].p.value, k * 33333, in_T_wc=T_in)
        if ctor.get("closeLoops"):
            a, _ = ef.localLoop()
            loops.append((a.attempted, a.gates_ok, a.n_constraints, a.applied, a.graph_nodes))
    ef.synchronize()
    out = ef.trajectory()[0], ef.lastCount(), ef.downloadMap(), loops
    ef.close()
    return out


def assert_same(got, want):
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)), np.abs(got[0] - want[0]).max()
    assert got[1] == want[1] and want[1] > 0
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    assert got[3] == want[3]


@pytest.fixture(scope="module")
def baseline(hip, scene):
    return run(hip, scene)


def test_stage_timers_every_frame(hip, scene, baseline):
    assert_same(run(hip, scene, lambda ef: ef.enableTiming(True)), baseline)


def test_sampled_frames_leave_the_graph_replay(hip, scene, baseline):
    def setup(ef):
        ef.setGraphReplay(True)
        hip._chk(hip.lib().ef_kernel_timing(ef.h, 2), ef.h)
    assert_same(run(hip, scene, setup), baseline)


def test_host_pointer_frames_with_overlap(hip, scene, baseline):
    assert_same(run(hip, scene, lambda ef: ef.setInputOverlap(1), host=True), baseline)


def test_overlap_two_is_demoted_under_the_persistent_tracker(hip, scene, baseline):
    def setup(ef):
        ef.setPersistentTracker(1)
        ef.setInputCuMask(4)
        ef.setInputOverlap(2)
    assert_same(run(hip, scene, setup), baseline)


def test_pose_handed_in_for_a_middle_frame(hip, scene):
    want = run(hip, scene, pose_at=4)
    assert_same(run(hip, scene, lambda ef: ef.setInputOverlap(1), pose_at=4), want)


def test_loop_closure_with_builtin_solver_and_overlap(hip, scene):
    # A time window of one frame and a confidence threshold every surfel passes after a frame or two: in the middle of a frame every surfel
    # was last seen at or before tick - 1, so the INACTIVE view is the whole map and the model-to-model tracker registers it against the ACTIVE
    # view of the same surfaces: thousands of correspondences at almost no error.  With the gates' thresholds far below that, constraints are
    # sampled and the built-in solver runs, at this size and length.
    ctor = dict(closeLoops=True, timeDelta=1, confidence=0.5, countThresh=100, errThresh=1.0, covThresh=1.0)
    want = run(hip, scene, lambda ef: ef.useBuiltinLoopSolver(True), **ctor)
    print("local loops (attempted, gates_ok, n_constraints, applied, graph_nodes):", want[3])
    assert all(a[0] for a in want[3][1:])   # every tracked frame attempts the local closure
    assert any(a[1] and a[2] > 0 for a in want[3])   # and the gates open: the solver's path is live

    def setup(ef):
        ef.useBuiltinLoopSolver(True)
        ef.setInputOverlap(1)
    assert_same(run(hip, scene, setup, **ctor), want)
