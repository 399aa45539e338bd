"""GPU parity, frame tier: a camera that has turned round.  The synthetic sequences never rotate the camera more than 0.3 rad away from the
world frame, so every pose of every other frame test has a positive trace; here the same frames are tracked in worlds turned by 130 degrees
and more, where the end of every tracking call takes one of the three non-positive-trace branches of matrix -> quaternion and the pose
algebra behind it (inverse, product, log, the float matrices of the map passes) works on such quaternions.

How the world is turned: the first frame of a run seeds the map at the identity and does not look at a caller-supplied pose
(ElasticFusion.cpp:290-296), so a pose G T_0 cannot be injected there.  Instead the checkpoint after frame 0 (map, tick, pose, last frame) is
turned by G — surfel positions and normals by the float G, the pose set to G T_0 — and restored into a fresh product context and a fresh
oracle, which then track frames 1-3.  Both receive the same bits."""
import numpy as np
import pytest

import efo
import gn_cases
import tracksizes

pytestmark = pytest.mark.gpu

ROW = min((r for r in tracksizes.FRAME_LADDER), key=lambda r: r["cols"] * r["rows"])     # the smallest frame size the size ladder has
W, H = ROW["cols"], ROW["rows"]
WORLDS = [("y_180deg", [0, 1, 0], np.pi), ("x_130deg", [1, 0, 0], np.radians(130.0)), ("diagonal_2.6rad", [1, 1, 1], 2.6)]


def test_tracking_in_worlds_turned_by_more_than_120_degrees():
    from elasticfusion_amd import api, synth
    assert (W, H) == (512, 256)
    sq = synth.Sequence(seed=0xEF0003, width=W, height=H)
    frames = [sq.frame(k)[:2] for k in range(4)]
    kw = dict(width=W, height=H, fx=sq.fx, fy=sq.fy, cx=sq.cx, cy=sq.cy, maxSurfels=1 << 19)
    seed = efo.Fusion(**kw)
    seed.process_frame(frames[0][0], frames[0][1], 0)
    ck0 = seed.checkpoint(frames[0][0], frames[0][1])
    assert np.array_equal(ck0["qt"], [0, 0, 0, 1, 0, 0, 0]) and len(ck0["map"]) > 100000
    branches = set()
    for name, axis, angle in WORLDS:
        G = np.eye(4)
        G[:3, :3] = gn_cases.rot(axis, angle)
        Gf = G[:3, :3].astype(np.float32)
        m = ck0["map"].copy()
        m[:, 0:3] = m[:, 0:3] @ Gf.T                                   # positions and normals into the turned world
        m[:, 8:11] = m[:, 8:11] @ Gf.T
        q8 = np.zeros(8)
        efo.lib().efo_mat_to_quat(efo.ptr(np.ascontiguousarray(G[:3, :3])), efo.ptr(q8))
        ck = dict(ck0, map=m, qt=np.concatenate([q8[4:], (G @ sq.pose(0))[:3, 3]]))
        o = efo.Fusion(**kw)
        o.restore(ck)
        ef = api.ElasticFusion(**kw)
        ef.restore(ck)
        for k in range(1, 4):
            o.process_frame(frames[k][0], frames[k][1], k * 33333)
            ef.processFrame(frames[k][0], frames[k][1], k * 33333)
            # the oracle alone: it tracks (the criterion of ElasticFusion.cpp:326), stays with the ground truth, and its pose is one of the
            # non-positive-trace kind
            qt_o, T_o, st_o, want = o.pose_qt(), o.pose(), o.stats(), G @ sq.pose(k)
            assert o.reloc_state()["trackingOk"] and st_o[0] < 1e-4 and st_o[1] > 1000 and st_o[3] > 1000, (name, k, st_o)
            assert np.linalg.norm(T_o[:3, 3] - want[:3, 3]) < 0.02 and np.abs(T_o[:3, :3] - want[:3, :3]).max() < 0.02, (name, k)
            assert np.trace(T_o[:3, :3]) <= 0.0, (name, k, T_o)
            branches.add(gn_cases.quat_branch(T_o[:3, :3]))
            # the product against it
            st = np.asarray(ef.trackingStats()[0], np.float32)
            assert np.array_equal(st.view(np.uint32), np.asarray(st_o, np.float32).view(np.uint32)), (name, k, st, st_o)
            assert np.array_equal(ef.getPoseQT().astype(np.float32), qt_o.astype(np.float32)), (name, k, ef.getPoseQT(), qt_o)
            assert np.array_equal(ef.get_T_wc().astype(np.float32), T_o.astype(np.float32)), (name, k)
            assert ef.lastCount() == o.map_count(), (name, k)
            assert np.array_equal(ef.downloadMap().view(np.uint32), o.map().view(np.uint32)), (name, k)
        assert ef.trackerFallbacks() == 0
        # one more frame with its pose handed in by the caller (no tracking: the device builds its pose matrices from the caller's 4x4, whose
        # quaternion again comes from a non-positive-trace branch), fused into the same map
        rgb4, depth4 = sq.frame(4)[:2]
        T4 = np.ascontiguousarray(G @ sq.pose(4))
        assert np.trace(T4[:3, :3]) <= 0.0, name
        o.process_frame(rgb4, depth4, 4 * 33333, T_wc=T4)
        ef.processFrame(rgb4, depth4, 4 * 33333, in_T_wc=T4)
        assert np.array_equal(ef.getPoseQT().astype(np.float32), o.pose_qt().astype(np.float32)), (name, ef.getPoseQT(), o.pose_qt())
        assert np.array_equal(ef.get_T_wc().astype(np.float32), o.pose().astype(np.float32)), name
        assert ef.lastCount() == o.map_count(), name
        assert np.array_equal(ef.downloadMap().view(np.uint32), o.map().view(np.uint32)), name
        ef.close()
    assert branches == {0, 1, 2}, branches
