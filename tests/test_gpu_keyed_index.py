"""Round 9: a frame that fuses no longer resolves its two predictIndices into the four index maps — the association (k_associate<true>) and
the keep-test of clean() (clean_test<true>) tap the z-buffer keys the splats leave (efm::KeyedIndex), and the maps are resolved on demand
when ef_get_image asks for one.  The build variant "resolve" (-DEF_KEEP_INDEX_RESOLVE, elasticfusion_amd/build.py) keeps rounds 1-8's script:
two resolve launches per frame, consumers on the maps.  Everything here compares the two scripts of the same sources byte for byte
(tolerance zero, as everywhere in this suite), or the frame tier with the operator tier, which keeps the resolve launch.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INDEX_MAPS = ("index", "vertConf", "colorTime", "normRad")


@pytest.fixture(scope="module")
def resolve_lib():
    """libefusion_hip_resolve.so, (re)built when it is missing or older than the kernel sources"""
    from elasticfusion_amd import build
    path = os.path.join(os.path.dirname(build.LIB), "libefusion_hip_resolve.so")
    deps = [os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith((".hip", ".inc", ".hpp", ".h"))] + [build.__file__]
    if not os.path.exists(path) or any(os.path.getmtime(d) > os.path.getmtime(path) for d in deps):
        build.build_variant("resolve", [])
    return path


class library:
    """api bound to another build of the library for the length of a with block"""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        from elasticfusion_amd import api
        api.use_library(self.path)
        return api

    def __exit__(self, *exc):
        from elasticfusion_amd import api
        api.use_library(None)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def replay(api, frames, every=10, **kw):
    ef = api.ElasticFusion(**kw)
    rec = dict(pose=[], count=[], maps={})
    for k, (rgb, depth, _) in enumerate(frames):
        ef.processFrame(rgb, depth, k * 33333)
        rec["count"].append(ef.lastCount())
        if (k + 1) % every == 0:
            rec["maps"][k] = ef.downloadMap()
    Ts, _ = ef.trajectory()                      # the device-resident pose log: one 4x4 double matrix per frame
    rec["pose"] = np.asarray(Ts)
    ef.close()
    return rec


@pytest.mark.parametrize("size,confidence", [((640, 480), 10.0), ((324, 244), 2.0)])
def test_replay_equals_the_resolved_script(resolve_lib, size, confidence):
    """>= 60 free-running frames twice — consumers on the keys (default) and on the resolved maps (variant): logged poses, surfel counts and the
    downloaded map after every 10th frame, byte for byte.  324 x 244 (ef_create takes multiples of 4 only: the nearest size to an odd 322 x 242):
    neither the pixels (79 056) nor the fused quarter (162 x 122) fill whole workgroups, so every launch that clears a z-buffer on the side
    ends in a partial one; confidence 2 there so that stable surfels (what the keep-test counts) exist from the first frames on."""
    from elasticfusion_amd import api, synth
    W, H = size
    n = 64
    sq = synth.Sequence(seed=0xEF0004, width=W, height=H)
    frames = [sq.frame(k) for k in range(n)]
    kw = dict(width=W, height=H, fx=sq.fx, fy=sq.fy, cx=sq.cx, cy=sq.cy, confidence=confidence, maxSurfels=1 << 21)
    a = replay(api, frames, **kw)
    with library(resolve_lib) as v:
        b = replay(v, frames, **kw)
    assert len(a["pose"]) == n and same(a["pose"], b["pose"])
    assert a["count"] == b["count"] and min(a["count"]) > 1000 and len(set(a["count"])) > n // 2
    assert sorted(a["maps"]) == [9, 19, 29, 39, 49, 59]
    for k in a["maps"]:
        assert same(a["maps"][k], b["maps"][k]), k
    stable = int((a["maps"][59][:, 3] > confidence).sum())
    assert stable > 1000, stable                  # the keep-test had stable texels to count


def index_maps(ef):
    return {name: ef.image(name) for name in INDEX_MAPS}


def fetch_scenarios(api, frames):
    """what ef_get_image hands out for the four index maps in every situation the on-demand resolve has to cover"""
    out = {}
    ef = api.ElasticFusion(confidence=1.0)
    feed = lambda k: ef.processFrame(frames[k][0], frames[k][1], k * 33333)   # noqa: E731
    for k in range(5):
        feed(k)
    out["first"] = index_maps(ef)                 # resolved now
    out["second"] = index_maps(ef)                # already resolved
    out["vertConf_alone"] = ef.image("vertConf")
    feed(5)                                       # a fusing frame behind a fetch: its association clears the keys the fetch read
    out["map_after_fetch_and_frame"] = ef.downloadMap()
    out["after_next_frame"] = index_maps(ef)
    feed(6)
    feed(7)                                       # two fusing frames with no fetch in between
    ef.setTrackOnly(True)
    feed(8)                                       # a frame that does not fuse moves the pose: the maps are still frame 7's
    out["after_track_only"] = index_maps(ef)
    ef.setTrackOnly(False)
    feed(9)
    ck = ef.checkpoint(frames[9][0], frames[9][1])
    ef.restore(ck)                                # ef_map_upload + ef_restore_state on the live context: pose rewritten, maps untouched
    out["after_restore"] = index_maps(ef)
    out["after_restore_again"] = index_maps(ef)
    feed(10)
    ef.enableTiming(True)                         # stage timers: the resolve launches are back for this frame
    feed(11)
    ef.enableTiming(False)
    out["after_timed_frame"] = index_maps(ef)
    feed(12)
    out["after_untimed_frame"] = index_maps(ef)
    out["map_end"] = ef.downloadMap()
    ef.close()
    return out


def test_index_maps_on_demand_equal_the_resolved_ones(resolve_lib, seq):
    from elasticfusion_amd import api
    frames = [seq.frame(k) for k in range(13)]
    a = fetch_scenarios(api, frames)
    with library(resolve_lib) as v:
        b = fetch_scenarios(v, frames)
    assert sorted(a) == sorted(b)
    for key in a:
        if isinstance(a[key], dict):
            for name in INDEX_MAPS:
                assert same(a[key][name], b[key][name]), (key, name)
        else:
            assert same(a[key], b[key]), key
    # the scenarios are not vacuous: the maps are populated, change from frame to frame, and a second fetch returns the first one's bytes
    assert (a["first"]["index"] > 0).mean() > 0.5 and np.abs(a["first"]["normRad"]).sum() > 0
    assert not same(a["first"]["vertConf"], a["after_next_frame"]["vertConf"])
    for name in INDEX_MAPS:
        assert same(a["first"][name], a["second"][name]) and same(a["after_restore"][name], a["after_restore_again"][name]), name
    assert same(a["first"]["vertConf"], a["vertConf_alone"])


def test_texel_won_by_surfel_zero_frame_tier_against_operator_tier(seq):
    """The index maps' quirk: a texel won by surfel id 0 has index 0, and both consumers skip it (`current > 0U`, `idx > 0U`) although the
    texel's other maps are populated.  The keyed consumers must skip it the same way.  Surfel 0 is made to win a texel in the middle of the
    image that a fused pixel taps (its own centre tap) and that the pixel's new unstable candidate then taps in clean(); the frame tier (keys)
    is compared with ef_op_predict_indices / ef_op_fuse / ef_op_clean (resolved maps) on the same inputs.  Identity pose: exact in every
    representation, and with the previous pose also the identity the velocity weighting is exactly 1."""
    from elasticfusion_amd import api
    ops = api.ops
    rgb, depth, _ = seq.frame(0)
    I = np.eye(4)
    conf = 1.0
    a = api.ElasticFusion(confidence=conf)
    for k in range(4):
        a.processFrame(rgb, depth, k * 33333, in_T_wc=None if k == 0 else I)
    M, tick = a.downloadMap(), a.getTick()
    maxD, TD, cut = a.getMaxDepthProcessed(), a.getTimeDelta(), 3.0
    a.close()
    cam = api.ef_cam(640, 480, 528.0, 528.0, 320.0, 240.0)
    idx, vc, _, _ = ops.predict_indices(cam, I, tick, M, maxD, TD)
    dm = ops.metricise_depth(depth, cut)
    dmf = ops.metricise_depth(ops.filter_depth(depth, cut), cut)
    # a fused pixel (both coordinates of the frame's parity) in the middle of the image whose own texel is won by a surfel at its depth
    par = tick % 2
    ys, xs = np.mgrid[200:280, 280:360]
    ok = (xs % 2 == par) & (ys % 2 == par) & (idx[ys, xs] > 0) & (dm[ys, xs] > 0) & (np.abs(vc[ys, xs, 2] - dm[ys, xs]) < 0.005)
    assert ok.any()
    y0, x0 = int(ys[ok][0]), int(xs[ok][0])
    j = int(idx[y0, x0])
    M2 = M.copy()
    M2[[0, j]] = M[[j, 0]]                        # the winner's record moves to row 0: same depth, lowest id
    # operator tier
    idx, vc, ct, nr = ops.predict_indices(cam, I, tick, M2, maxD, TD)
    assert idx[y0, x0] == 0 and vc[y0, x0, 2] > 0 and np.abs(nr[y0, x0, :3]).sum() > 0      # won by surfel 0: index 0, maps populated
    s2, nu = ops.fuse(cam, I, tick, rgb, dm, dmf, idx, vc, ct, nr, maxD, 1.0, M2)
    u = np.floor(528.0 * nu[:, 0] / nu[:, 2] + 320.0 + 1e-3).astype(int)
    v = np.floor(528.0 * nu[:, 1] / nu[:, 2] + 240.0 + 1e-3).astype(int)
    assert ((u == x0) & (v == y0)).any()          # the pixel found no surfel (its texel reads index 0): it became a new unstable surfel
    idx2, vc2, ct2, nr2 = ops.predict_indices(cam, I, tick, s2, maxD, TD)
    assert idx2[y0, x0] == 0 and vc2[y0, x0, 2] > 0
    want = ops.clean(cam, I, tick, idx2, vc2, ct2, nr2, conf, TD, maxD, s2, nu)
    # frame tier
    b = api.ElasticFusion(confidence=conf)
    b.uploadMap(M2)
    b.setTick(tick)
    b.processFrame(rgb, depth, tick * 33333, in_T_wc=I)
    got = b.downloadMap()
    got_idx = b.image("index")
    b.close()
    assert len(got) == len(want) > len(M2)
    assert same(got, want)
    assert same(got_idx, idx2)
