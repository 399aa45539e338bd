"""The launches that build the tracker's inputs each frame, bit for bit against the oracle's pyramids (scenes: tests/inputscenes.py).

Operator tier: ef_op_model_maps runs the shipped k_model_maps and — joint — the model-map half of k_frame_inputs (whose grid also carries
the depth pre-processing tiles) on every model-map scene, ef_op_sobel_mask runs k_sobel_levels on every frame-side scene, at 36 x 28, 80 x 60
and 132 x 36.  The oracle is the composition k_model_maps' comment names (copy_maps -> resize_map x2 -> transform_maps x3,
vertices_to_depth, bgr_to_intensity, dense_enough); a scene's check() passes on the oracle's result before the device is asked.  Both sides
start every output from the same contents (inputscenes.init_pattern), so that maps are compared plane for plane; scenes whose y / z planes
differ under a NaN x by construction (quirk Q3: exact_planes False) are compared through mask_planes.

Frame tier: a checkpoint restored into api.ElasticFusion and efo.Fusion, two frames tracked without a pose (the first reads the fill-in,
the second the prediction), every trackerBuffer name compared with the oracle's RGBDOdometry after each frame, under every setting that
changes the input launches.  What the names hold AFTER a frame: getIncrementalTransformation ends by swapping nextImage and lastNextImage
at every level when so3 is on (RGBDOdometry.cpp:552-553, the default: every frame-to-model case here), so `lastNextImage` is the frame's
intensity pyramid — the image the derivative images and rgbMask were made from — and `nextImage` the previous frame's; nothing else is
exchanged.  nextDepth is lastDepth on tracker 0 (quirk Q1: both come from the model's vertices; one set of buffers on the device).
The model-to-model tracker (tracker 1, so3 off: no swap) keeps a nextDepth of its own.

Sizes of the frame tier: the two-frame cases with the condition "ICP and RGB counts above a fifth of the pixels" run at 80 x 60 and
132 x 36.  At 36 x 28 the oracle's frame-to-model tracker does not meet it (inputscenes.FRAME_SIZES: RGB count 151 of 1008 on the first
frame, singular on the second); test_first_frame_at_the_narrowest_size compares the buffers of the first frame there all the same (ICP count
258, which is above a fifth), without the RGB half of the condition.  The model-to-model case runs at 36 x 28, the smallest of the three
sizes — the oracle runs modelToModel.track there on both frames, with ICP counts 526 and 863 of 1008 on a non-empty inactive view — and at
80 x 60.
"""
import ctypes as C

import numpy as np
import pytest

import efo
import inputscenes as S
from test_gpu_ops_tracking import bits_equal

pytestmark = pytest.mark.gpu
SIZE_IDS = dict(ids=S.size_id)


@pytest.fixture(scope="module")
def api():
    from elasticfusion_amd import api
    return api


def differing(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return f"shapes {a.shape} {b.shape}"
    d = a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,))
    idx = np.argwhere(d.any(axis=-1))
    return f"{len(idx)} elements, first {idx[:4].tolist()}"


# ---- operator tier ----
@pytest.mark.parametrize("joint", (False, True), ids=("k_model_maps", "k_frame_inputs"))
@pytest.mark.parametrize("size", S.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("name", S.MAP_SCENE_NAMES)
def test_model_maps_scene(api, name, size, joint):
    W, H = size
    sc = S.map_scene(W, H, name)
    ref = S.map_oracle(W, H, name)
    sc.check(ref)                                                   # the scene does its job on the oracle ...
    frame = S.frame_scene(W, H, 1) if joint else None
    got = sc.run_device(api.ops, joint=joint, frame=frame)          # ... before the device is asked
    bad = []
    for k in S.PLANES:
        a, b = (got[k], ref[k]) if sc.exact_planes else (S.mask_planes(got[k]), S.mask_planes(ref[k]))
        if not bits_equal(a, b):
            bad.append((k, differing(a, b)))
    for k in ("depth0", "last0"):
        if not bits_equal(got[k], ref[k]):
            bad.append((k, differing(got[k], ref[k])))
    if got["dense_count"] != ref["dense_count"]:
        bad.append(("dense_count", got["dense_count"], ref["dense_count"]))
    if joint:   # the other half of the grid: the frame's pre-processing
        for k, r in sc.oracle_frame(frame).items():
            if not bits_equal(got[k], r):
                bad.append((k, differing(got[k], r)))
    assert not bad, (str(sc), bad)


@pytest.mark.parametrize("k", (0, 1, 2, S.PATCH_FRAME), ids=("0", "1", "2", "patches"))
@pytest.mark.parametrize("size", S.SIZES, **SIZE_IDS)
def test_sobel_mask_scene(api, size, k):
    W, H = size
    o = S.frame_oracle(W, H, k)
    if k == S.PATCH_FRAME:     # the window and the depth gate deciding at levels 1 and 2 as well
        S.check_patch_oracle(o, W, H)
    else:
        S.check_frame_oracle(o, W, H)
    dIdx, dIdy, mask, corres = api.ops.sobel_mask(o["nextImage"], o["nextDepth"])
    for l in range(3):
        assert bits_equal(dIdx[l], o["dIdx"][l]), (l, differing(dIdx[l], o["dIdx"][l]))
        assert bits_equal(dIdy[l], o["dIdy"][l]), (l, differing(dIdy[l], o["dIdy"][l]))
        assert bits_equal(mask[l], o["mask"][l]), (l, differing(mask[l], o["mask"][l]))
        assert not corres[l].any(), l


# ---- frame tier ----
ORACLE_NAMES = ("vmap_curr", "nmap_curr", "vmap_g_prev", "nmap_g_prev", "lastDepth", "nextDepth", "lastImage", "nextImage", "lastNextImage",
                "dIdx", "dIdy", "depth_tmp")
SOBEL_NAMES = ("dIdx", "dIdy")


def compare_tracker(ef, od, W, H, tracker=0, sobel=True, skip=()):
    """every trackerBuffer name at levels 0-2 against the oracle's RGBDOdometry `od`; -> list of mismatches"""
    bad = []
    for l in range(3):
        for name in ORACLE_NAMES:
            if name in skip or (not sobel and name in SOBEL_NAMES):
                continue
            a, b = ef.trackerBuffer(name, l, tracker), od.buffer(name, l)
            if not bits_equal(a, b):
                bad.append((name, l, differing(a, b)))
        if not sobel:
            continue
        # rgbMask against the restatement, on the oracle's buffers: the image the derivative images were made from is nextImage before the
        # swap (tracker 0: lastNextImage now), the depth is nextDepth
        img = od.buffer("lastNextImage" if tracker == 0 else "nextImage", l)
        want = S.rgb_mask(img, od.buffer("dIdx", l), od.buffer("dIdy", l), od.buffer("nextDepth", l), S.MIN_SCALE[l])
        mask, corres = ef.trackerBuffer("rgbMask", l, tracker), ef.trackerBuffer("corres", l, tracker)
        if not bits_equal(mask, want):
            bad.append(("rgbMask", l, differing(mask, want)))
        if corres[mask == 0].any():
            bad.append(("corres", l, "non-zero where rgbMask is 0"))
    return bad


def same_stats(ef, o):
    a, b = np.asarray(ef.trackingStats()[0], np.float32), np.asarray(o.stats(), np.float32)
    return bits_equal(a, b), a, b


CONFIGS = ("default", "timing", "overlap", "graph_replay", "device_frames", "icp_only", "frame_to_frame_rgb")


@pytest.mark.parametrize("size", S.FRAME_SIZES, **SIZE_IDS)
@pytest.mark.parametrize("config", CONFIGS)
def test_tracker_buffers_after_each_frame(api, config, size):
    W, H = size
    ck = S.checkpoint(W, H)
    ctor = dict(frameToFrameRGB=True) if config == "frame_to_frame_rgb" else {}
    okw = dict(frameToFrameRGB=1) if config == "frame_to_frame_rgb" else {}
    if config == "icp_only":
        okw["icpWeight"] = 100.0
    kw = S.fusion_kw(W, H)
    ef, o = api.ElasticFusion(**kw, **ctor), efo.Fusion(**kw, **okw)
    keep = []
    try:
        if config == "timing":
            ef.enableTiming(True)
        elif config == "overlap":
            ef.setInputOverlap(True)
        elif config == "graph_replay":
            ef.setGraphReplay(True)
        elif config == "icp_only":
            ef.setIcpWeight(100)
        ef.restore(ck)
        o.restore(ck)
        cam = efo.make_cam(W, H, *S.intr(W, H))
        verdicts = []
        for k in (1, 2):
            fr = S.frame_scene(W, H, k)
            verdicts.append(efo.dense_enough(cam, o.buffer("image")))
            if config == "device_frames":
                keep.append((api.DevBuf.from_array(fr["rgb"]), api.DevBuf.from_array(fr["depth"])))
                ef.processFrameDevice(keep[-1][0].p.value, keep[-1][1].p.value, k)
            else:
                ef.processFrame(fr["rgb"], fr["depth"], k)
            o.process_frame(fr["rgb"], fr["depth"], k)
            ef.synchronize()
            st = o.stats()
            assert st[1] > W * H / 5, ("the oracle's ICP count: the frame really tracked", k, st)
            if config != "icp_only":
                assert st[3] > W * H / 5, ("the oracle's RGB count", k, st)
            bad = compare_tracker(ef, o.odometry(), W, H, sobel=config != "icp_only")
            assert not bad, (config, k, bad)
            ok, a, b = same_stats(ef, o)
            assert ok, (config, k, a, b)
        assert verdicts == [False, True], "the first frame reads the fill-in, the second the prediction"
        assert ef.lastCount() == o.map_count() and bits_equal(ef.downloadMap(), o.map())
    finally:
        ef.close()


def test_first_frame_at_the_narrowest_size(api):
    """36 x 28: narrower than one model-map workgroup and than one filter tile.  The oracle's frame-to-model tracker finds 258 ICP
    correspondences on the first frame there (above a fifth of the 1008 pixels) but only 151 photometric ones, and its second frame is
    singular: the two-frame condition of the cases above cannot hold, so this case stands beside them, with the ICP half of the condition,
    for what runs at this size only here: k_frame_inputs, k_pyr_down_multi with its u16 job and k_vn_sobel_levels inside a frame."""
    W, H = 36, 28
    ck = S.checkpoint(W, H)
    kw = S.fusion_kw(W, H)
    ef, o = api.ElasticFusion(**kw), efo.Fusion(**kw)
    try:
        ef.restore(ck)
        o.restore(ck)
        fr = S.frame_scene(W, H, 1)
        ef.processFrame(fr["rgb"], fr["depth"], 1)
        o.process_frame(fr["rgb"], fr["depth"], 1)
        ef.synchronize()
        st = o.stats()
        print("oracle statistics at 36 x 28, frame 1:", st)
        assert st[1] > W * H / 5 and st[3] > 0, st
        bad = compare_tracker(ef, o.odometry(), W, H)
        assert not bad, bad
        ok, a, b = same_stats(ef, o)
        assert ok, (a, b)
        assert ef.lastCount() == o.map_count() and bits_equal(ef.downloadMap(), o.map())
    finally:
        ef.close()


@pytest.mark.parametrize("size", [(36, 28), (80, 60)], **SIZE_IDS)
def test_model_to_model_tracker_buffers(api, size):
    """closeLoops on a time window of one frame: in the middle of a frame every surfel was last seen at or before tick - 1, so the INACTIVE
    view is the checkpoint's map and modelToModel registers it against the ACTIVE view (init_model_pair: two k_model_maps, k_rgba_intensity_pair,
    k_pyr_down_multi over four jobs of two types, k_sobel_levels).  tracker 1 against odometry(1); its depth_tmp is never written.
    36 x 28 is the smallest of the three sizes and the oracle runs the tracker there (its transcript says so, ICP counts 526 and 863);
    tracker 0 is compared as well at both sizes, whatever it found."""
    W, H = size
    ck = S.checkpoint(W, H)
    kw = S.fusion_kw(W, H, timeDelta=1)
    ef, o = api.ElasticFusion(closeLoops=True, **kw), efo.Fusion(**kw)
    o.set_close_loops(True)
    take = efo.lib().efo_fusion_take_trace
    take.restype = C.c_char_p
    try:
        ef.restore(ck)
        o.restore(ck)
        for k in (1, 2):
            fr = S.frame_scene(W, H, k)
            efo.lib().efo_fusion_trace(o.h_, 1)
            ef.processFrame(fr["rgb"], fr["depth"], k)
            o.process_frame(fr["rgb"], fr["depth"], k)
            ef.synchronize()
            trace = take(o.h_).decode().splitlines()
            assert any(line.startswith("modelToModel.track") for line in trace), trace
            assert (o.old_buffer("vertex")[..., 2] > 0).mean() > 0.3, "the inactive view is not empty"
            b, _ = o.local_loop()
            a, _ = ef.localLoop()
            assert b.attempted and a.attempted and b.stats[1] > W * H / 5, list(b.stats)
            assert bits_equal(np.array(a.stats, np.float32), np.array(b.stats, np.float32)), (list(a.stats), list(b.stats))
            bad = compare_tracker(ef, o.odometry(1), W, H, tracker=1, skip=("depth_tmp",))
            assert not bad, (k, bad)
            bad = compare_tracker(ef, o.odometry(0), W, H)
            assert not bad, (k, bad)
    finally:
        ef.close()
