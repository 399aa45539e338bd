"""GlobalModel::renderPointCloud without OpenGL (ef_render_model / ef_render_model_dev, include/ef_hip.h; kernels in
elasticfusion_amd/csrc/ef_render.inc): the live map drawn on the device from any pinhole camera and pose.

The geometry is the model prediction's splat with another camera, so a render of stable surfels is pinned bit for bit to the CPU
oracle's combinedPredict; the selection, the unstable surfels' depth offset and the shading are pinned to numpy restatements of
draw_global_surface.{vert,geom,frag} as DESIGN.md §8 states them.  A render must change nothing a frame computes.
"""
import os
import subprocess

import numpy as np
import pytest

import efo

pytestmark = pytest.mark.gpu

INT_MAX = 2147483647
EMPTY = 0xFFFFFFFF
ALL = ("rgba", "depth", "vertex", "normal", "index")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bits_equal(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    d = bits(a) != bits(b)
    assert not d.any(), (what, int(d.sum()), np.argwhere(d)[:5])


def depth_key(z):
    """the z-buffer's order-preserving float -> uint (ef_map_kernels.hip depth_key)"""
    b = np.ascontiguousarray(z, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(4)
    R[i, i] = R[j, j] = c
    R[i, j], R[j, i] = -s, s
    return R


@pytest.fixture(scope="module")
def mature():
    import mapops
    return mapops.make_inputs()


@pytest.fixture(scope="module")
def ctx(mature):
    from elasticfusion_amd import api
    w, h, fx, fy, cx, cy = mature["cam"]
    ef = api.ElasticFusion(width=int(w), height=int(h), fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy))
    yield ef
    ef.close()


def tick_of(mature):
    return int(np.asarray(mature["tick"]).reshape(-1)[0])


def cameras(mature):
    w, h, fx, fy, cx, cy = [float(v) for v in mature["cam"]]
    T = mature["T"]
    moved = T @ rot(1, 30.0)
    moved[:3, 3] += moved[:3, :3] @ np.array([0.5, 0.0, 0.0])
    return [("frame", (int(w), int(h), fx, fy, cx, cy), T),
            ("800x600", (800, 600, 610.0, 590.0, 395.5, 304.25), T),
            ("rotated", (int(w), int(h), fx, fy, cx, cy), moved)]


def render(ef, cam, T, **kw):
    w, h, fx, fy, cx, cy = cam
    kw.setdefault("outputs", ALL)
    return ef.renderPointCloud(T_wc=T, width=w, height=h, fx=fx, fy=fy, cx=cx, cy=cy, **kw)


def oracle(cam, T, surf, tick):
    w, h, fx, fy, cx, cy = cam
    return efo.combined_predict(efo.make_cam(w, h, fx, fy, cx, cy), T, surf, 20.0, 0.0, tick, INT_MAX, INT_MAX // 2)


def test_stable_render_equals_the_oracle_prediction_bit_for_bit(ctx, mature):
    surf, tick = mature["surf"], tick_of(mature)
    assert surf[:, 3].min() > 0.0
    ctx.uploadMap(surf)
    for name, cam, T in cameras(mature):
        r = render(ctx, cam, T, threshold=0.0, drawColors=True, maxDepth=20.0, time=tick)
        img, vt, nm, _ = oracle(cam, T, surf, tick)
        drawn = r["index"] != EMPTY
        assert drawn.sum() > 1000, name
        assert_bits_equal(r["vertex"], vt, name + " vertex")
        assert_bits_equal(r["normal"], nm, name + " normal")
        assert_bits_equal(r["depth"], vt[..., 2], name + " depth")
        assert_bits_equal(r["rgba"][..., :3], img[..., :3], name + " rgb")
        assert (r["rgba"][..., 3] == np.where(drawn, 255, 0)).all(), name
        # the index names the surfel whose camera-frame normal / radius / confidence the pixel carries
        idx = r["index"][drawn]
        assert idx.max() < len(surf)
        assert_bits_equal(r["normal"][drawn][:, 3], surf[idx, 11], name + " radius")
        assert_bits_equal(r["vertex"][drawn][:, 3], surf[idx, 3], name + " confidence")
        R_cw = np.linalg.inv(T)[:3, :3]
        n = surf[idx, 8:11].astype(np.float64) @ R_cw.T
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        assert np.abs(n - r["normal"][drawn][:, :3]).max() < 1e-5, name
        assert (r["depth"][~drawn] == 0).all() and (r["vertex"][~drawn] == 0).all() and (r["normal"][~drawn] == 0).all()


def test_threshold_selects_the_rows_above_it(ctx, mature):
    surf, tick = mature["surf"].copy(), tick_of(mature)
    surf[:, 3] *= 8.0   # confidences on both sides of 10
    rows = np.nonzero(surf[:, 3] > 10.0)[0]
    assert 1000 < len(rows) < len(surf)
    sub = np.ascontiguousarray(surf[rows])
    for name, cam, T in cameras(mature):
        ctx.uploadMap(surf)
        r = render(ctx, cam, T, threshold=10.0, drawColors=True, maxDepth=20.0, time=tick)
        img, vt, nm, _ = oracle(cam, T, sub, tick)
        assert_bits_equal(r["vertex"], vt, name + " vertex")
        assert_bits_equal(r["normal"], nm, name + " normal")
        assert_bits_equal(r["rgba"][..., :3], img[..., :3], name + " rgb")
        ctx.uploadMap(sub)
        r2 = render(ctx, cam, T, threshold=0.0, drawColors=True, maxDepth=20.0, time=tick, outputs=("index",))
        drawn = r2["index"] != EMPTY
        assert (drawn == (r["index"] != EMPTY)).all(), name
        assert (rows[r2["index"][drawn]] == r["index"][drawn]).all(), name


def test_unstable_surfels_compete_behind_their_radius(ctx, mature):
    surf, tick = mature["surf"].copy(), tick_of(mature)
    surf[:, 3] *= 8.0
    unstable = np.nonzero(~(surf[:, 3] > 10.0))[0]
    name, cam, T = cameras(mature)[0]
    kw = dict(threshold=10.0, maxDepth=20.0, time=tick, outputs=("depth", "index"))
    ctx.uploadMap(surf)
    union = render(ctx, cam, T, drawUnstable=True, **kw)
    stable = render(ctx, cam, T, drawUnstable=False, **kw)
    ctx.uploadMap(np.ascontiguousarray(surf[unstable]))
    only = render(ctx, cam, T, drawUnstable=True, **kw)
    u_drawn = only["index"] != EMPTY
    u_id = np.where(u_drawn, unstable[np.where(u_drawn, only["index"], 0)], EMPTY).astype(np.uint64)
    u_depth = np.where(u_drawn, only["depth"], 0).astype(np.float32)
    u_key = np.where(u_drawn, depth_key(u_depth + surf[u_id.clip(0, len(surf) - 1).astype(np.int64), 11]), 2**32)
    s_drawn = stable["index"] != EMPTY
    s_key = np.where(s_drawn, depth_key(stable["depth"]), 2**32)
    s_id = stable["index"].astype(np.uint64)
    take_u = (u_key < s_key) | ((u_key == s_key) & (u_id < s_id))
    assert u_drawn.sum() > 1000 and s_drawn.sum() > 1000 and (take_u & u_drawn & s_drawn).any()
    assert (union["index"] == np.where(take_u, u_id, s_id)).all()
    assert_bits_equal(union["depth"], np.where(take_u, u_depth, stable["depth"]).astype(np.float32), "depth")

    # two overlapping discs facing the camera: the unstable one 3 cm in front of the stable one, within its 5 cm radius
    def disc(z, conf, rad):
        return [0.0, 0.0, z, conf, float(0x204060), 0.0, 1.0, 1.0, 0.0, 0.0, -1.0, rad]
    two = np.array([disc(0.97, 1.0, 0.05), disc(1.0, 20.0, 0.05)], np.float32)
    small = (64, 48, 50.0, 50.0, 32.0, 24.0)
    ctx.uploadMap(two)
    r = render(ctx, small, np.eye(4), threshold=10.0, drawUnstable=True, maxDepth=20.0, time=2)
    assert r["index"][24, 32] == 1 and abs(r["depth"][24, 32] - 1.0) < 1e-3
    ctx.uploadMap(two[:1])
    r = render(ctx, small, np.eye(4), threshold=10.0, drawUnstable=True, maxDepth=20.0, time=2)
    assert r["index"][24, 32] == 0 and abs(r["depth"][24, 32] - 0.97) < 1e-3 and abs(r["vertex"][24, 32, 2] - 0.97) < 1e-3
    r = render(ctx, small, np.eye(4), threshold=10.0, drawUnstable=False, maxDepth=20.0, time=2)
    assert (r["index"] == EMPTY).all()


def shade(surf, idx, color_type, draw_window, time, time_delta):
    """draw_global_surface.geom:49-79 in float32, the order DESIGN.md §8 states (fmax: the operand that is not NaN)"""
    f = np.float32
    s = surf[idx]
    n, ct = s[:, 8:11], s[:, 4:8]
    with np.errstate(all="ignore"):
        sm = np.abs((n[:, 0] + n[:, 1]) + n[:, 2])
        if color_type == 1:
            c = n.copy()
        elif color_type == 2:
            ic = ct[:, 0].astype(np.int32)
            c = np.stack([((ic >> 16) & 255), ((ic >> 8) & 255), (ic & 255)], 1).astype(f) / f(255)
        elif color_type == 3:
            ratio = f(2) * (ct[:, 2] - f(1)) / (f(time) - f(1))
            r = np.fmax(f(0), f(1) - ratio)
            g = np.fmax(f(0), ratio - f(1))
            m = sm + f(0.1)
            c = np.stack([r * m, g * m, ((f(1) - r) - g) * m], 1)
        else:
            c = np.repeat((f(0.5) * sm + f(0.1))[:, None], 3, 1)
        if draw_window:
            c = np.where(((f(time) - ct[:, 3]) > f(time_delta))[:, None], c * f(0.25), c)
        c = np.where(c >= 0, np.minimum(c, f(1)), f(0)).astype(f) * f(255)   # NaN -> 0
        r = np.trunc(c)
        r = r + (c - r >= f(0.5))   # roundf: half away from zero (np.round is half to even)
    return r.astype(np.uint8)


def test_shading_follows_the_geometry_shader(ctx, mature):
    surf, tick = mature["surf"], tick_of(mature)
    ctx.uploadMap(surf)
    name, cam, T = cameras(mature)[0]
    assert (surf[:, 7] < tick - 2).any() and (surf[:, 7] >= tick - 2).any()   # the window dims some surfels and not others
    cases = [(ct, win, tick) for ct in range(4) for win in (False, True)] + [(3, False, 1), (3, True, 1)]
    for color_type, win, time in cases:
        flags = dict(drawNormals=color_type == 1, drawColors=color_type == 2, drawTimes=color_type == 3)
        r = render(ctx, cam, T, threshold=0.0, drawWindow=win, time=time, timeDelta=2, maxDepth=20.0, outputs=("rgba", "index"), **flags)
        drawn = r["index"] != EMPTY
        assert drawn.sum() > 1000
        want = shade(surf, r["index"][drawn].astype(np.int64), color_type, win, time, 2)
        got = r["rgba"][drawn]
        assert (got[:, :3] == want).all(), (color_type, win, time, int((got[:, :3] != want).any(1).sum()))
        assert (got[:, 3] == 255).all() and (r["rgba"][~drawn] == 0).all()


def test_small_cases(ctx, mature):
    from elasticfusion_amd import api
    small = (64, 48, 50.0, 50.0, 32.0, 24.0)

    def empty(r):
        return (r["index"] == EMPTY).all() and not r["rgba"].any() and not r["depth"].any() and not r["vertex"].any() and not r["normal"].any()

    def one(x, z, rad=0.2):
        return np.array([[x, 0.0, z, 5.0, float(0x808080), 0.0, 1.0, 1.0, 0.0, 0.0, -1.0, rad]], np.float32)

    ctx.uploadMap(np.zeros((0, 12), np.float32))
    assert empty(render(ctx, small, np.eye(4), threshold=0.0, drawUnstable=True))
    ctx.uploadMap(one(0.0, 2.0))
    assert not empty(render(ctx, small, np.eye(4), threshold=0.0))
    assert empty(render(ctx, small, rot(1, 180.0), threshold=0.0))                       # camera looking away
    assert empty(render(ctx, small, np.eye(4), threshold=0.0, maxDepth=1.5))               # beyond max_depth
    assert not empty(render(ctx, small, np.eye(4), threshold=0.0, maxDepth=2.5))
    # centre at u = -1 (outside the image), footprint reaching well into it: not drawn, as in the prediction
    ctx.uploadMap(one((-1.0 - 32.0) / 50.0 * 2.0, 2.0))
    assert empty(render(ctx, small, np.eye(4), threshold=0.0))
    ctx.uploadMap(one((1.0 - 32.0) / 50.0 * 2.0, 2.0))
    assert not empty(render(ctx, small, np.eye(4), threshold=0.0))
    # sizes 1 x 1 and 4096 x 4096
    ctx.uploadMap(one(0.0, 2.0))
    r = render(ctx, (1, 1, 50.0, 50.0, 0.5, 0.5), np.eye(4), threshold=0.0)
    assert r["index"].shape == (1, 1) and r["index"][0, 0] == 0 and r["rgba"][0, 0, 3] == 255
    ctx.uploadMap(mature["surf"])
    r = render(ctx, (4096, 4096, 3400.0, 3400.0, 2048.0, 2048.0), mature["T"], threshold=0.0, maxDepth=20.0, outputs=("rgba", "index"))
    assert r["rgba"].shape == (4096, 4096, 4) and (r["index"] != EMPTY).sum() > 100000
    for w, h in ((0, 48), (64, 0), (4097, 48), (64, 4097), (-1, 48)):
        with pytest.raises(api.EFError, match="error -1"):
            render(ctx, (w, h, 50.0, 50.0, 32.0, 24.0), np.eye(4), threshold=0.0, outputs=("index",))
    # a refused call leaves the context usable
    ctx.uploadMap(one(0.0, 2.0))
    assert render(ctx, small, np.eye(4), threshold=0.0, outputs=("index",))["index"][24, 32] == 0


def _run_sequence(frames, dev, with_renders):
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    bufs = []
    T_other = np.eye(4)
    T_other[:3, 3] = [0.2, -0.1, -0.3]
    T_other = T_other @ rot(0, 10.0)
    cam = dict(width=320, height=256, fx=300.0, fy=310.0, cx=160.0, cy=128.0)
    outs = {}
    if with_renders and dev:
        p = ef.renderParams(T_wc=T_other, drawUnstable=True, drawColors=True, **cam)
        P = 320 * 256
        outs = dict(rgba=api.DevBuf(P * 4), depth=api.DevBuf(P * 4), vertex=api.DevBuf(P * 16), normal=api.DevBuf(P * 16),
                    index=api.DevBuf(P * 4))
    for k, (rgb, depth, _) in enumerate(frames):
        if dev:
            bufs.append((api.DevBuf.from_array(rgb), api.DevBuf.from_array(depth)))
            ef.processFrameDevice(bufs[-1][0].p.value, bufs[-1][1].p.value, k)
        else:
            ef.processFrame(rgb, depth, k)
        if with_renders and k + 1 < len(frames):
            if dev:   # enqueued behind the frame, nothing synchronises
                ef.renderPointCloudDevice(p, **{n: b.p for n, b in outs.items()})
            else:
                ef.renderPointCloud(T_wc=T_other, drawUnstable=True, drawColors=True, outputs=ALL, **cam)
    ef.synchronize()
    res = dict(traj=ef.trajectory()[0], pose=ef.get_T_wc(), map=ef.downloadMap(), count=ef.lastCount())
    if with_renders:
        host = ef.renderPointCloud(T_wc=T_other, drawUnstable=True, drawColors=True, outputs=ALL, **cam)
        if dev:   # the device variant's last render saw the map before the last frame: render the final map once more
            ef.renderPointCloudDevice(p, **{n: b.p for n, b in outs.items()})
            ef.synchronize()
            for n, (dt, ch) in ef.RENDER_OUTPUTS.items():
                got = outs[n].to_array(dt, host[n].shape)
                assert_bits_equal(got, host[n], "device variant " + n)
        res["render"] = host
    ef.close()
    return res


@pytest.mark.parametrize("dev", [True, False], ids=["device_frames", "host_frames"])
def test_renders_change_nothing(seq, dev):
    frames = [seq.frame(k) for k in range(30)]
    a = _run_sequence(frames, dev, False)
    b = _run_sequence(frames, dev, True)
    assert a["count"] == b["count"] > 0
    assert_bits_equal(a["traj"].astype(np.float64).view(np.uint64), b["traj"].astype(np.float64).view(np.uint64), "trajectory")
    assert_bits_equal(a["pose"].view(np.uint64), b["pose"].view(np.uint64), "pose")
    assert_bits_equal(a["map"], b["map"], "downloadMap")
    assert (b["render"]["index"] != EMPTY).sum() > 1000


def test_replay_front_end_writes_snapshots(tmp_path, seq):
    from elasticfusion_amd import api, synth
    replay = os.path.join(os.path.dirname(api.LIB_PATH), "efusion_replay")
    frames = [seq.frame(k) for k in range(8)]
    a, b = str(tmp_path / "a.klg"), str(tmp_path / "b.klg")
    synth.write_klg(a, frames)
    synth.write_klg(b, frames)
    out = tmp_path / "snaps"
    out.mkdir()
    for cmd in ([replay, "-l", a, "-q"],
                [replay, "-l", b, "-q", "-render", str(out), "-render-every", "3", "-render-cam", "320", "240", "210", "210", "160", "120",
                 "-render-mode", "colors", "-render-unstable"]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
        assert r.returncode == 0, (cmd, r.stdout[-1000:], r.stderr[-1000:])
    assert open(a + ".freiburg", "rb").read() == open(b + ".freiburg", "rb").read()
    assert sorted(os.listdir(out)) == ["render_000000.ppm", "render_000003.ppm", "render_000006.ppm"]   # 7 frames: the last is not delivered
    for f in sorted(os.listdir(out)):
        data = open(out / f, "rb").read()
        head = b"P6\n320 240\n255\n"
        assert data.startswith(head) and len(data) == len(head) + 320 * 240 * 3
        img = np.frombuffer(data[len(head):], np.uint8).reshape(240, 320, 3)
        assert (img.max(2) > 0).mean() > 0.2, f
