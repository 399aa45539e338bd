"""The tracker's size-dependent kernel paths, restated in Python, the two ladders of sizes that visit every one of them, and a deterministic
scene for any (cols, rows).  Shared by test_track_sizes_host.py (the tables are what they claim; the scene gives the oracle something to find)
and test_gpu_track_sizes.py (HIP against the oracle at every row).

Everything the tracker chooses by a level's pixel count N hangs on two numbers (elasticfusion_amd/csrc/ef_track.hpp: VTHREADS = 16384):

    K = ceil(N / 16384)     passes of the 16384 virtual threads
    S = (K + 3) >> 2        steps of four passes

  accumulation variant  launch_accum (ef_track_host_ops.inc) picks k_se3_accum<CH> from S: S <= 2 -> CH 2; S % 6 in {0, 5} or S % 4 not in
                        {0, 3} -> CH 6; else CH 4.  The unpacked RGB-only operator (rgb_step): CH 5 when N > 8 * 16384, else CH 2.
  rounds                a round is CH steps; rounds behind the first reload inside the kernel's loop.  Steps past S and passes past K are
                        visits that do not exist: they read pixel N - 1 and must contribute nothing.
  search launch         k_track_step<PPT>: PPT 2 from N >= 256 * 1024 (ef_track_host_track.inc)
  residency mode        k_track_ref keeps a level's pixel data in LDS (ef_track_ref_persistent.inc, rt_res_mode): 2 = both terms
                        (S * 14336 bytes), 1 = the ICP side (S * 6144), 0 = streamed; the resident loops run in chunks of RT_CH = 5 steps
  script 2              k_track_small takes a level only with N <= PT_MAX_PIXELS = 131072 and at most 16 iterations so far (plan_script)

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import functools

import numpy as np

import efo
from trackops import rot

VTHREADS = 16384
PT_MAX_PIXELS = 8 * VTHREADS
PT_MAX_ITER = 16
FT_MAX_ITER = 24
RT_ICP_STEP_BYTES = 4 * 6 * 64 * 4
RT_RGB_STEP_BYTES = 4 * 8 * 64 * 4
RT_CH = 5
PPT2_FROM = 256 * 1024

# What rt_res_budget() gives on the MI355X: 160 KB of LDS per workgroup - k_track_ref<true, true>'s static LDS (41792 bytes in the code
# object's metadata, .group_segment_fixed_size) - 1 KB of margin, rounded down to a whole KB = 118 KB.  The frame ladder's residency classes
# (rows "664x496" to "1360x1020") are picked for THIS budget: mode 2 up to S 8, mode 1 up to S 19.
RES_BUDGET = 118 * 1024


# ------------------------------------------------------------------------------------------------
# the selection rules
# ------------------------------------------------------------------------------------------------
def passes(n):
    """(K, S) of a level of n pixels"""
    k = (n + VTHREADS - 1) // VTHREADS
    return k, (k + 3) >> 2


def accum_ch(s):
    """CH of k_se3_accum for the ICP operator and for every packed (frame-tier) launch"""
    if s <= 2:
        return 2
    if s % 6 in (0, 5) or s % 4 not in (0, 3):
        return 6
    return 4


def rgb_op_ch(n):
    """CH of k_se3_accum for the unpacked RGB-only operator (rgb_step)"""
    return 5 if n > 8 * VTHREADS else 2


def rounds(s, ch):
    """(rounds, empty steps of the last round)"""
    r = (s + ch - 1) // ch
    return r, r * ch - s


def search_ppt(n):
    return 2 if n >= PPT2_FROM else 1


def res_need(s, budget, icp=True, rgb=True):
    """bytes of LDS a level of S steps asks of a persistent launch under `budget` (launch_persistent)"""
    n2 = s * ((RT_ICP_STEP_BYTES if icp else 0) + (RT_RGB_STEP_BYTES if rgb else 0))
    n1 = s * RT_ICP_STEP_BYTES if icp else 0
    return n2 if n2 <= budget else (n1 if n1 <= budget else 0)


def res_mode(s, res_bytes, icp=True, rgb=True):
    """rt_res_mode: what a level of S steps keeps resident in a launch with res_bytes of dynamic LDS"""
    ni = s * RT_ICP_STEP_BYTES if icp else 0
    nr = s * RT_RGB_STEP_BYTES if rgb else 0
    if ni + nr <= res_bytes:
        return 2
    return 1 if icp and ni <= res_bytes else 0


def res_chunks(s):
    """steps of each chunk of a resident loop"""
    return [min(RT_CH, s - s0) for s0 in range(0, s, RT_CH)]


def size_class(cols, rows):
    """every size-dependent choice for one level of cols x rows pixels"""
    n = cols * rows
    k, s = passes(n)
    ch, ch_rgb = accum_ch(s), rgb_op_ch(n)
    r, e = rounds(s, ch)
    r_rgb, e_rgb = rounds(s, ch_rgb)
    return dict(N=n, K=k, S=s, CH=ch, rounds=r, empty=e, CH_rgb=ch_rgb, rounds_rgb=r_rgb, empty_rgb=e_rgb, PPT=search_ppt(n))


def level_iterations(fast_odom=False, pyramid=True):
    """Gauss-Newton iterations of levels 0, 1, 2 (plan_script)"""
    return [3 if fast_odom else 10, 5 if pyramid else 0, 4 if pyramid else 0]


def plan_script(cols, rows, asked, fast_odom=False, pyramid=True, so3=True):
    """(script, n_small, n_iter, levels) of one call, as plan_script / launch_persistent decide them (reference-order build, no capture, not
    rgbOnly); levels = the level of each iteration inside the one launch"""
    it = level_iterations(fast_odom, pyramid)
    total = sum(it)
    order = [lv for lv in (2, 1, 0) for _ in range(it[lv])]
    if asked == 1 and total <= FT_MAX_ITER:
        return 1, 0, total, order
    if asked == 2:
        n_small, fits = 0, True
        for lv in (2, 1, 0):
            if it[lv] == 0 or not fits:
                continue
            fits = (cols >> lv) * (rows >> lv) <= PT_MAX_PIXELS and n_small + it[lv] <= PT_MAX_ITER
            if fits:
                n_small += it[lv]
        if n_small > 0 or so3:
            return 2, n_small, total, order[:n_small]
    return 0, 0, total, []


def launch_res_bytes(cols, rows, budget, fast_odom=False, pyramid=True):
    """dynamic LDS of the persistent launch: the largest need of a level that iterates (launch_persistent)"""
    it = level_iterations(fast_odom, pyramid)
    return max(res_need(passes((cols >> lv) * (rows >> lv))[1], budget) if it[lv] else 0 for lv in range(3))


# ------------------------------------------------------------------------------------------------
# the ladders
# ------------------------------------------------------------------------------------------------
def _row(cols, rows, what, **kw):
    return dict(cols=cols, rows=rows, what=what, **kw)


# Operator tier: the smallest pixel counts at which each branch of k_se3_accum exists.  K, S: passes and steps; CH / rounds / empty: the ICP
# operator's variant, its rounds and the steps of the last round that do not exist; CH_rgb / rounds_rgb / empty_rgb: the unpacked RGB operator's.
OP_LADDER = [
    _row(16, 3, "48 pixels: most of one wavefront idle", K=1, S=1, CH=2, rounds=1, empty=1, CH_rgb=2, rounds_rgb=1, empty_rgb=1),
    _row(128, 128, "exactly one pass", K=1, S=1, CH=2, rounds=1, empty=1, CH_rgb=2, rounds_rgb=1, empty_rgb=1),
    _row(145, 113, "one pixel in the second pass", K=2, S=1, CH=2, rounds=1, empty=1, CH_rgb=2, rounds_rgb=1, empty_rgb=1),
    _row(257, 256, "CH 2, second step ragged", K=5, S=2, CH=2, rounds=1, empty=0, CH_rgb=2, rounds_rgb=1, empty_rgb=0),
    _row(512, 256, "CH 2 full; N = 8 * VTHREADS: unpacked RGB stays on CH 2", K=8, S=2, CH=2, rounds=1, empty=0, CH_rgb=2, rounds_rgb=1, empty_rgb=0),
    _row(516, 256, "CH 4, one empty step; unpacked RGB moves to CH 5", K=9, S=3, CH=4, rounds=1, empty=1, CH_rgb=5, rounds_rgb=1, empty_rgb=2),
    _row(512, 512, "CH 4, exactly full", K=16, S=4, CH=4, rounds=1, empty=0, CH_rgb=5, rounds_rgb=1, empty_rgb=1),
    _row(523, 512, "CH 6 and CH 5, one round", K=17, S=5, CH=6, rounds=1, empty=1, CH_rgb=5, rounds_rgb=1, empty_rgb=0),
    _row(768, 512, "CH 6 exactly full; CH 5 second round", K=24, S=6, CH=6, rounds=1, empty=0, CH_rgb=5, rounds_rgb=2, empty_rgb=4),
    _row(771, 512, "CH 4, two rounds, one empty step", K=25, S=7, CH=4, rounds=2, empty=1, CH_rgb=5, rounds_rgb=2, empty_rgb=3),
    _row(1024, 512, "CH 4, two full rounds", K=32, S=8, CH=4, rounds=2, empty=0, CH_rgb=5, rounds_rgb=2, empty_rgb=2),
    _row(1027, 512, "CH 6, two rounds, three empty steps", K=33, S=9, CH=6, rounds=2, empty=3, CH_rgb=5, rounds_rgb=2, empty_rgb=1),
    _row(1409, 512, "CH 6, two full rounds", K=45, S=12, CH=6, rounds=2, empty=0, CH_rgb=5, rounds_rgb=3, empty_rgb=3),
    _row(1537, 512, "CH 6, three rounds, five empty steps", K=49, S=13, CH=6, rounds=3, empty=5, CH_rgb=5, rounds_rgb=3, empty_rgb=2),
    _row(1793, 512, "CH 4, four rounds", K=57, S=15, CH=4, rounds=4, empty=1, CH_rgb=5, rounds_rgb=3, empty_rgb=0),
    _row(1360, 1020, "CH 6, four rounds; the mode-0 size of the frame tier", K=85, S=22, CH=6, rounds=4, empty=2, CH_rgb=5, rounds_rgb=5, empty_rgb=3),
]

# Frame tier.  K, S, CH, PPT: level 0.  mode: level 0's residency in the persistent launch at RES_BUDGET; n_small: iterations script 2 runs
# inside k_track_small; n_iter: iterations of the call.  reference: "oracle", or "steps" = the launch-per-step run of the same frames (sizes
# at which the CPU oracle takes tens of seconds).  Widths and heights are multiples of 4 (three pyramid levels); each size is the smallest
# 4:3-ish one of its class.  As ef_get_tracker_plan reported them on an MI355X (res_budget 120832): res_bytes 43008, 57344, 86016 and 114688 for
# the four mode-2 sizes, 55296 and 61440 (the ICP side of level 0) for 840x628 and 888x668, 86016 (level 1's) for 1360x1020.
FRAME_LADDER = [
    _row(480, 360, "CH 4 with an empty step; level 0 above PT_MAX_PIXELS", K=11, S=3, CH=4, PPT=1, mode=2, n_small=9, n_iter=19, reference="oracle"),
    _row(512, 512, "every pass full; PPT 2 at its lower edge", K=16, S=4, CH=4, PPT=2, mode=2, n_small=9, n_iter=19, reference="oracle"),
    _row(664, 496, "mode 2, second resident chunk of one step; CH 6 full", K=21, S=6, CH=6, PPT=2, mode=2, n_small=9, n_iter=19, reference="oracle"),
    _row(784, 588, "largest mode 2 at the 118 KB budget (chunks 5 + 3)", K=29, S=8, CH=4, PPT=2, mode=2, n_small=9, n_iter=19, reference="oracle"),
    _row(840, 628, "first mode-1 size (chunks 5 + 4); level 1 (420x314) just above PT_MAX_PIXELS", K=33, S=9, CH=6, PPT=2, mode=1, n_small=4,
         n_iter=19, reference="oracle"),
    _row(888, 668, "mode 1, two full resident chunks", K=37, S=10, CH=6, PPT=2, mode=1, n_small=4, n_iter=19, reference="steps"),
    _row(1360, 1020, "mode 0 without forcing", K=85, S=22, CH=6, PPT=2, mode=0, n_small=4, n_iter=19, reference="steps"),
    _row(512, 256, "script 2 carries all 12 iterations; N = PT_MAX_PIXELS", fast_odom=True, K=8, S=2, CH=2, PPT=1, mode=2, n_small=12, n_iter=12,
         reference="oracle"),
    _row(512, 256, "script 2, level 0 only, 10 iterations", pyramid=False, K=8, S=2, CH=2, PPT=1, mode=2, n_small=10, n_iter=10, reference="oracle"),
    _row(516, 256, "level 0 leaves k_track_small", fast_odom=True, K=9, S=3, CH=4, PPT=1, mode=2, n_small=9, n_iter=12, reference="oracle"),
]


def row_id(r):
    return "%dx%d" % (r["cols"], r["rows"]) + ("-fastOdom" if r.get("fast_odom") else "") + ("-nopyramid" if r.get("pyramid") is False else "")


# ------------------------------------------------------------------------------------------------
# the scene
# ------------------------------------------------------------------------------------------------
DIST_THRES = 0.10
ANGLE_THRES = float(np.sin(20 * 3.14159254 / 180))
MIN_SCALE = float(5 * 5 * 64)     # level 0's gradient gate (RGBDOdometry.cpp:112,425)
MAX_DEPTH_DELTA = 0.07
SOBEL_SCALE = 0.125


def _texture(x, y):
    """band-limited: the shortest period is 11 pixels; values 28 .. 228 (never 0: intensity 0 is "no data" to the search)"""
    t = (44.0 * np.sin(2 * np.pi * x / 23.0 + 0.7) + 30.0 * np.sin(2 * np.pi * y / 17.0 + 1.9) + 16.0 * np.sin(2 * np.pi * (x + y) / 11.0) +
         10.0 * np.sin(2 * np.pi * (x - 2 * y) / 41.0 + 0.3))
    return np.rint(128.0 + t).astype(np.uint8)


def scene(cols, rows):
    """inputs of icp_step, rgb_residual + rgb_step and so3_step at cols x rows: a slanted, gently rippled surface seen twice under a small motion"""
    fx = fy = 0.82 * cols
    cx, cy = cols / 2.0, rows / 2.0
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    z = 1500.0 + 260.0 * (x / cols - 0.5) + 180.0 * (y / rows - 0.5) + 6.0 * np.sin(2 * np.pi * x / 53.0) * np.cos(2 * np.pi * y / 47.0)
    depth = np.rint(z).astype(np.uint16)
    rng = np.random.RandomState((cols * 4099 + rows) & 0x7FFFFFFF)
    depth[rng.rand(rows, cols) < 0.03] = 0
    depth_f = depth.astype(np.float32) / np.float32(1000.0)
    depth_f[depth == 0] = np.nan
    last_image, next_image = _texture(x, y), _texture(x + 0.3, y - 0.2)
    vmap = efo.create_vmap(depth, fx, fy, cx, cy, 20.0)
    nmap = efo.create_nmap(vmap)
    dIdx, dIdy = efo.derivative_images(next_image)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    Kinv = np.linalg.inv(K)
    R2 = rot(0.003, -0.004, 0.002).astype(np.float64)
    s = dict(
        cols=cols, rows=rows, intr=(fx, fy, cx, cy),
        vmap_curr=vmap, nmap_curr=nmap, vmap_g_prev=vmap, nmap_g_prev=nmap,
        Rprev_inv=np.eye(3, dtype=np.float32), tprev=np.zeros(3, np.float32),
        Rcurr=rot(0.004, -0.003, 0.002), tcurr=np.array([0.003, -0.002, 0.004], np.float32),
        dIdx=dIdx, dIdy=dIdy, lastDepth=depth_f, nextDepth=depth_f, lastImage=last_image, nextImage=next_image,
        kt=np.array([0.4, -0.3, 0.002], np.float32) * np.float32(cols / 640.0),
        krkinv=(K @ rot(0.002, -0.001, 0.001).astype(np.float64) @ Kinv).astype(np.float32),
        so3_basis=(K @ R2 @ Kinv).astype(np.float32), so3_kinv=Kinv.astype(np.float32), so3_krlr=(K @ R2).astype(np.float32),
    )
    return {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in s.items()}


def run_ops(be, s):
    """the four size-dependent operators on backend `be` (efo, or api.ops): dict of their results"""
    fx, fy, cx, cy = s["intr"]
    out = {}
    out["icp_A"], out["icp_b"], out["icp_res"] = be.icp_step(s["Rcurr"], s["tcurr"], s["vmap_curr"], s["nmap_curr"], s["Rprev_inv"], s["tprev"],
                                                             s["intr"], s["vmap_g_prev"], s["nmap_g_prev"], DIST_THRES, ANGLE_THRES)
    c, sig, cnt = be.rgb_residual(MIN_SCALE, s["dIdx"], s["dIdy"], s["lastDepth"], s["nextDepth"], s["lastImage"], s["nextImage"],
                                  MAX_DEPTH_DELTA, s["kt"], s["krkinv"])
    out["corres"], out["sigma"], out["count"] = c, sig, cnt
    return out


@functools.lru_cache(maxsize=1)
def oracle_case(cols, rows):
    """(scene, the oracle's results on it), the last shape asked for kept: read-only for every test that shares it"""
    s = scene(cols, rows)
    fx, fy, cx, cy = s["intr"]
    o = run_ops(efo, s)
    o["cloud"] = efo.project_to_point_cloud(s["lastDepth"], fx, fy, cx, cy)
    o["rgb_sigma"] = float(np.sqrt(o["count"]))
    o["rgb_A"], o["rgb_b"] = efo.rgb_step(o["corres"], o["rgb_sigma"], o["cloud"], fx, fy, s["dIdx"], s["dIdy"], SOBEL_SCALE)
    o["so3_A"], o["so3_b"], o["so3_res"] = efo.so3_step(s["lastImage"], s["nextImage"], s["so3_basis"], s["so3_kinv"], s["so3_krlr"])
    return s, o


def assert_oracle_finds_enough(cols, rows, o):
    """the condition every operator-ladder shape meets on the oracle: a shape at which it finds next to nothing would pass vacuously"""
    n = cols * rows
    assert o["icp_res"][1] >= n / 5, ("ICP inliers", cols, rows, o["icp_res"], n)
    assert o["count"] >= n / 5, ("RGB correspondences", cols, rows, o["count"], n)
    assert o["so3_res"][1] >= n / 5, ("SO(3) pixels", cols, rows, o["so3_res"], n)
    for k in ("icp_A", "icp_b", "rgb_A", "rgb_b", "so3_A", "so3_b"):
        assert np.isfinite(o[k]).all(), (k, cols, rows)
