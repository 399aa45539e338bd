"""The tracker's size-dependent kernel paths against the oracle, at the sizes of tests/tracksizes.py (which states the selection rules and what
each row exercises; test_track_sizes_host.py proves the tables on the CPU).

Operator tier: icp_step, rgb_residual + rgb_step and so3_step on the generated scene at every row of OP_LADDER — every k_se3_accum<CH> variant
with one round and with several, with a full last round and with steps that do not exist.  The bar is test_gpu_ops_tracking.py's: A, b and res
bit-identical, sigma and the count exact, `valid` identical and zero / one / diff identical where valid, A symmetric.  The condition of the host
test (the oracle finds at least N / 5 of everything) is asserted again on the very result that is compared.

Frame tier: two frames of synth.Sequence(0xEF0003) (seed, then one tracked frame: every iteration of every level) at every row of FRAME_LADDER,
under each script setting; ef_get_tracker_plan must report the script, the iterations inside k_track_small and the residency mode the row names
(the mode is derived from the reported res_bytes, not assumed), no launch may have fallen back, synchronize() must succeed.  The bar is
test_small_and_odd_resolutions_match_oracle's: statistics bit for bit, float32 pose equal, map count equal, whole map bit for bit.

888x668 and 1360x1020 compare every setting with the LAUNCH-PER-STEP run of the same frames, not with the oracle: the CPU oracle takes about
8 us per pixel and frame (2 frames of 1360x1020: 22 s), far beyond what a test of this suite may cost.  What that leaves unpinned is little: the
single-term accumulation kernels of the launch-per-step script are pinned to the oracle at the same N by the operator tier (1360x1020 is a row
of OP_LADDER; S 10's CH 6 over two rounds is 1027x512's class), and residency mode 1 itself is pinned to the oracle at 840x628 here and at
1280x960 by test_gpu_frame.py.

The residency classes are those of a 118 KB budget (tracksizes.RES_BUDGET): 160 KB - k_track_ref's 41792 bytes of static LDS - 1 KB, whole KB.
On a device or build that answers otherwise the assertion on res_budget says what to re-pick."""
import numpy as np
import pytest

import efo
import tracksizes as ts
from test_gpu_ops_tracking import bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from elasticfusion_amd import api
    return api


# ------------------------------------------------------------------------------------------------
# operator tier
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=ts.OP_LADDER, ids=ts.row_id)
def case(request):
    row = request.param
    s, o = ts.oracle_case(row["cols"], row["rows"])
    ts.assert_oracle_finds_enough(row["cols"], row["rows"], o)
    return row, s, o


def test_icp_step(hip, case):
    row, s, o = case
    A, b, res = hip.ops.icp_step(s["Rcurr"], s["tcurr"], s["vmap_curr"], s["nmap_curr"], s["Rprev_inv"], s["tprev"], s["intr"], s["vmap_g_prev"],
                                 s["nmap_g_prev"], ts.DIST_THRES, ts.ANGLE_THRES)
    print(ts.row_id(row), "icp: CH", row["CH"], "rounds", row["rounds"], "empty", row["empty"], "res", res, "oracle", o["icp_res"],
          "max |dA|", np.abs(A - o["icp_A"]).max())
    assert o["icp_res"][1] >= row["cols"] * row["rows"] / 5
    assert bits_equal(res, o["icp_res"]), (row["what"], res, o["icp_res"])
    assert bits_equal(A, o["icp_A"]) and bits_equal(b, o["icp_b"]), (row["what"], np.abs(A - o["icp_A"]).max(), np.abs(b - o["icp_b"]).max())
    assert np.array_equal(A, A.T)


def test_rgb_residual_and_step(hip, case):
    row, s, o = case
    fx, fy, _, _ = s["intr"]
    c, sig, cnt = hip.ops.rgb_residual(ts.MIN_SCALE, s["dIdx"], s["dIdy"], s["lastDepth"], s["nextDepth"], s["lastImage"], s["nextImage"],
                                       ts.MAX_DEPTH_DELTA, s["kt"], s["krkinv"])
    print(ts.row_id(row), "rgb: CH", row["CH_rgb"], "rounds", row["rounds_rgb"], "empty", row["empty_rgb"], "sigma, count", (sig, cnt),
          "oracle", (o["sigma"], o["count"]))
    assert o["count"] >= row["cols"] * row["rows"] / 5
    assert (sig, cnt) == (o["sigma"], o["count"])
    cr = o["corres"]
    assert np.array_equal(c["valid"], cr["valid"])
    v = cr["valid"] != 0
    for f in ("zero", "one", "diff"):
        assert np.array_equal(c[f][v], cr[f][v]), f
    A, b = hip.ops.rgb_step(c, o["rgb_sigma"], o["cloud"], fx, fy, s["dIdx"], s["dIdy"], ts.SOBEL_SCALE)
    print(ts.row_id(row), "rgb_step max |dA|", np.abs(A - o["rgb_A"]).max(), "max |db|", np.abs(b - o["rgb_b"]).max())
    assert bits_equal(A, o["rgb_A"]) and bits_equal(b, o["rgb_b"]), (row["what"], np.abs(A - o["rgb_A"]).max(), np.abs(b - o["rgb_b"]).max())
    assert np.array_equal(A, A.T)


def test_so3_step(hip, case):
    row, s, o = case
    A, b, res = hip.ops.so3_step(s["lastImage"], s["nextImage"], s["so3_basis"], s["so3_kinv"], s["so3_krlr"])
    print(ts.row_id(row), "so3: res", res, "oracle", o["so3_res"])
    assert o["so3_res"][1] >= row["cols"] * row["rows"] / 5
    assert bits_equal(res, o["so3_res"]), (res, o["so3_res"])
    assert bits_equal(A, o["so3_A"]) and bits_equal(b, o["so3_b"]), (np.abs(A - o["so3_A"]).max(), np.abs(b - o["so3_b"]).max())
    assert np.array_equal(A, A.T)


# ------------------------------------------------------------------------------------------------
# frame tier
# ------------------------------------------------------------------------------------------------
FRAMES = 2
# (name, ef_set_persistent_tracker, resident levels, fused step)
SETTINGS = [("persistent", 1, True, False), ("persistent-streamed", 1, False, False), ("steps", 0, True, False), ("steps-fused", 0, True, True),
            ("small-levels", 2, True, False)]


def options_of(row):
    return bool(row.get("fast_odom")), row.get("pyramid", True)


def run_hip(hip, row, frames, kw, setting):
    """-> (statistics, float32 pose, map count, map, plan) after FRAMES frames under one script setting"""
    _, persistent, resident, fused = setting
    fast, pyr = options_of(row)
    ef = hip.ElasticFusion(**kw)
    ef.setFastOdom(fast)
    ef.setPyramid(pyr)
    ef.setPersistentTracker(persistent)
    ef.setResidentLevels(resident)
    ef.setFusedStep(fused)
    assert ef.trackerPlan() == dict(script=0, n_small=0, n_iter=0, levels=[], res_bytes=0, res_budget=0)   # nothing tracked yet
    for k in range(FRAMES):
        ef.processFrame(frames[k][0], frames[k][1], k * 33333)
    plan = ef.trackerPlan()
    ef.synchronize()
    assert ef.trackerFallbacks() == 0
    st, _, _ = ef.trackingStats()
    out = np.asarray(st, np.float32), ef.get_T_wc().astype(np.float32), ef.lastCount(), ef.downloadMap(), plan
    ef.close()
    return out


def check_plan(row, setting, plan):
    name, persistent, resident, _ = setting
    cols, rows = row["cols"], row["rows"]
    fast, pyr = options_of(row)
    script, n_small, n_iter, levels = ts.plan_script(cols, rows, persistent, fast, pyr)
    assert (plan["script"], plan["n_small"], plan["n_iter"], plan["levels"]) == (script, n_small, n_iter, levels), (name, plan)
    assert plan["n_iter"] == row["n_iter"]
    if persistent == 2:
        assert plan["script"] == 2 and plan["n_small"] == row["n_small"], (name, plan)
    if persistent == 1:
        assert plan["script"] == 1
        if resident:
            assert plan["res_budget"] == ts.RES_BUDGET, (
                "the residency rows of tracksizes.FRAME_LADDER are picked for a budget of %d bytes, this device gives %d: keep the classes (mode 2 "
                "with a second chunk, the largest mode 2, the first mode 1, mode 0) and re-pick those sizes — width and height multiples of 4, "
                "the smallest N of the class" % (ts.RES_BUDGET, plan["res_budget"]))
            assert plan["res_bytes"] == ts.launch_res_bytes(cols, rows, plan["res_budget"], fast, pyr), plan
            assert ts.res_mode(row["S"], plan["res_bytes"]) == row["mode"], (name, plan)
        else:
            assert plan["res_bytes"] == 0 and ts.res_mode(row["S"], plan["res_bytes"]) == 0, (name, plan)
    else:
        assert plan["res_bytes"] == 0, (name, plan)


@pytest.fixture(scope="module", params=ts.FRAME_LADDER, ids=ts.row_id)
def frame_case(request, hip):
    """the row, its frames, the context arguments and the reference: the oracle's (statistics, pose, count, map), or the launch-per-step run's"""
    from elasticfusion_amd import synth
    row = request.param
    W, H = row["cols"], row["rows"]
    sq = synth.Sequence(seed=0xEF0003, width=W, height=H)
    frames = [sq.frame(k)[:2] for k in range(FRAMES)]
    kw = dict(width=W, height=H, fx=sq.fx, fy=sq.fy, cx=sq.cx, cy=sq.cy, maxSurfels=max(1 << 19, 1 << int(np.ceil(np.log2(3 * W * H)))))
    if row["reference"] == "oracle":
        fast, pyr = options_of(row)
        o = efo.Fusion(fastOdom=int(fast), pyramid=int(pyr), **kw)
        for k in range(FRAMES):
            o.process_frame(frames[k][0], frames[k][1], k * 33333)
        want = np.asarray(o.stats(), np.float32), o.pose().astype(np.float32), o.map_count(), o.map()
    else:
        want = run_hip(hip, row, frames, kw, SETTINGS[2])[:4]
    return row, frames, kw, want


@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_frames_under_every_script(hip, frame_case, setting):
    row, frames, kw, want = frame_case
    st, pose, count, surfels, plan = run_hip(hip, row, frames, kw, setting)
    mode = ts.res_mode(row["S"], plan["res_bytes"]) if plan["script"] == 1 else None
    print(ts.row_id(row), setting[0], "K", row["K"], "S", row["S"], "CH", row["CH"], "PPT", row["PPT"], "script", plan["script"], "n_small",
          plan["n_small"], "of", plan["n_iter"], "res_bytes", plan["res_bytes"], "budget", plan["res_budget"], "mode", mode, "vs", row["reference"])
    check_plan(row, setting, plan)
    assert np.isfinite(want[0]).all() and want[0][1] > 1000 and want[0][3] > 1000 and want[2] > 0   # ICP and RGB both found something to add up
    assert np.array_equal(st.view(np.uint32), want[0].view(np.uint32)), (st, want[0])
    assert np.array_equal(pose, want[1])
    assert count == want[2]
    assert np.array_equal(surfels.view(np.uint32), want[3].view(np.uint32))
