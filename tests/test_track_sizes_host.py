"""The size ladders of tests/tracksizes.py are what they claim, on the CPU alone: every row's class recomputed from (cols, rows) by the Python
restatement of the tracker's selection rules, the classes the rows must cover between them, and the condition that keeps the GPU comparison of
test_gpu_track_sizes.py from passing vacuously — at every operator-ladder shape the oracle finds at least N / 5 ICP inliers, N / 5 RGB
correspondences and N / 5 SO(3) pixels on the generated scene."""
import numpy as np
import pytest

import tracksizes as ts


@pytest.mark.parametrize("row", ts.OP_LADDER, ids=ts.row_id)
def test_operator_ladder_rows_state_their_class(row):
    c = ts.size_class(row["cols"], row["rows"])
    for k in ("K", "S", "CH", "rounds", "empty", "CH_rgb", "rounds_rgb", "empty_rgb"):
        assert row[k] == c[k], (ts.row_id(row), k, row[k], c[k])


def test_selection_rules_at_their_edges():
    assert ts.passes(1) == (1, 1) and ts.passes(16384) == (1, 1) and ts.passes(16385) == (2, 1) and ts.passes(4 * 16384 + 1) == (5, 2)
    assert [ts.accum_ch(s) for s in range(1, 25)] == [2, 2, 4, 4, 6, 6, 4, 4, 6, 6, 6, 6, 6, 6, 4, 4, 6, 6, 4, 4, 6, 6, 6, 6]
    assert ts.accum_ch(5) == 6 and ts.accum_ch(19) == 4    # 640 x 480 and 1280 x 960, as the launcher's comment has them
    assert ts.rgb_op_ch(8 * 16384) == 2 and ts.rgb_op_ch(8 * 16384 + 1) == 5
    assert ts.search_ppt(256 * 1024 - 1) == 1 and ts.search_ppt(256 * 1024) == 2
    assert ts.rounds(5, 6) == (1, 1) and ts.rounds(19, 4) == (5, 1) and ts.rounds(8, 4) == (2, 0)
    b = ts.RES_BUDGET
    assert b == 120832
    assert ts.res_mode(8, ts.res_need(8, b)) == 2 and ts.res_mode(9, ts.res_need(9, b)) == 1      # the boundary between modes 2 and 1
    assert ts.res_mode(19, ts.res_need(19, b)) == 1 and ts.res_mode(20, ts.res_need(20, b)) == 0  # ... and between 1 and 0
    assert ts.res_mode(5, 0) == 0 and ts.res_chunks(9) == [5, 4] and ts.res_chunks(5) == [5] and ts.res_chunks(6) == [5, 1]


def test_operator_ladder_covers_every_class():
    rows = [ts.size_class(r["cols"], r["rows"]) for r in ts.OP_LADDER]
    seen = {(c["CH"], c["rounds"] > 1, c["empty"] == 0) for c in rows}
    for ch in (4, 6):
        for several in (False, True):
            for full in (False, True):
                assert (ch, several, full) in seen, (ch, several, full)
    assert {(2, False, False), (2, False, True)} <= seen                      # CH 2: S 1 (one empty step) and S 2 (full)
    seen5 = {(c["rounds_rgb"] > 1) for c in rows if c["CH_rgb"] == 5}
    assert seen5 == {False, True}                                             # CH 5 with one round and with several
    assert any(c["CH_rgb"] == 5 and c["empty_rgb"] == 0 for c in rows) and any(c["CH_rgb"] == 5 and c["empty_rgb"] > 0 for c in rows)
    assert any(c["N"] == c["K"] * ts.VTHREADS for c in rows)                  # every pass full
    assert any(c["N"] == (c["K"] - 1) * ts.VTHREADS + 1 for c in rows)        # one pixel in the last pass
    assert any(c["N"] < 64 for c in rows)                                     # less than a wavefront
    assert any(c["N"] == 8 * ts.VTHREADS for c in rows) and any(8 * ts.VTHREADS < c["N"] <= 9 * ts.VTHREADS for c in rows)   # CH 2 | CH 5
    assert any(c["K"] % 4 for c in rows) and any(c["K"] % 4 == 0 for c in rows)   # a last step with passes that do not exist, and without
    assert max(r["cols"] for r in ts.OP_LADDER) < 2048 and max(r["rows"] for r in ts.OP_LADDER) < 2048   # (packed correspondences: 11 bits)


@pytest.mark.parametrize("row", ts.FRAME_LADDER, ids=ts.row_id)
def test_frame_ladder_rows_state_their_class(row):
    cols, rows = row["cols"], row["rows"]
    assert cols % 4 == 0 and rows % 4 == 0
    fast, pyr = bool(row.get("fast_odom")), row.get("pyramid", True)
    c = ts.size_class(cols, rows)
    for k in ("K", "S", "CH", "PPT"):
        assert row[k] == c[k], (ts.row_id(row), k, row[k], c[k])
    res = ts.launch_res_bytes(cols, rows, ts.RES_BUDGET, fast, pyr)
    assert ts.res_mode(c["S"], res) == row["mode"], (ts.row_id(row), res)
    assert ts.res_mode(c["S"], 0) == 0
    script, n_small, n_iter, levels = ts.plan_script(cols, rows, 2, fast, pyr)
    assert (script, n_small, n_iter) == (2, row["n_small"], row["n_iter"]) and len(levels) == n_small
    assert ts.plan_script(cols, rows, 1, fast, pyr)[:3] == (1, 0, row["n_iter"])
    assert ts.plan_script(cols, rows, 0, fast, pyr)[:3] == (0, 0, row["n_iter"])


def test_frame_ladder_covers_every_class():
    by = {ts.row_id(r): r for r in ts.FRAME_LADDER}
    full = [r for r in ts.FRAME_LADDER if not r.get("fast_odom") and r.get("pyramid", True)]
    assert {r["mode"] for r in full} == {0, 1, 2}
    # the boundary between mode 2 and mode 1: S 8 and S 9 at this budget, both present; mode 2 with a second resident chunk
    assert {r["S"] for r in full if r["mode"] == 2} >= {6, 8} and min(r["S"] for r in full if r["mode"] == 1) == 9
    assert ts.res_need(8, ts.RES_BUDGET) == 8 * 14336 and ts.res_need(9, ts.RES_BUDGET) == 9 * 6144
    assert any(r["cols"] * r["rows"] == ts.PPT2_FROM for r in full)                                  # PPT 2 at its lower edge
    assert any(r["PPT"] == 1 and r["cols"] * r["rows"] > ts.PT_MAX_PIXELS for r in full)
    assert by["512x256-fastOdom"]["n_small"] == by["512x256-fastOdom"]["n_iter"] == 12               # k_track_small carries the whole call
    assert by["512x256-fastOdom"]["cols"] * by["512x256-fastOdom"]["rows"] == ts.PT_MAX_PIXELS       # a level of exactly PT_MAX_PIXELS
    assert by["516x256-fastOdom"]["n_small"] == 9 and by["512x256-nopyramid"]["n_small"] == 10
    r = by["840x628"]
    assert (r["cols"] >> 1) * (r["rows"] >> 1) > ts.PT_MAX_PIXELS and r["n_small"] == 4              # level 1 leaves k_track_small
    assert {r["reference"] for r in ts.FRAME_LADDER} == {"oracle", "steps"}
    assert all(r["reference"] == "oracle" for r in ts.FRAME_LADDER if r["cols"] * r["rows"] <= 840 * 628)


@pytest.mark.parametrize("row", ts.OP_LADDER, ids=ts.row_id)
def test_oracle_finds_enough_on_the_generated_scene(row):
    cols, rows = row["cols"], row["rows"]
    s, o = ts.oracle_case(cols, rows)
    n = cols * rows
    print("%dx%d: ICP inliers %.3f N, RGB correspondences %.3f N, SO(3) pixels %.3f N" %
          (cols, rows, o["icp_res"][1] / n, o["count"] / n, o["so3_res"][1] / n))
    ts.assert_oracle_finds_enough(cols, rows, o)
    holes = float((s["lastDepth"] != s["lastDepth"]).mean())
    assert n < 1000 or 0.02 < holes < 0.04, holes
    assert s["lastImage"].min() > 0 and s["nextImage"].min() > 0
    assert np.array_equal(np.isnan(s["lastDepth"]), s["vmap_curr"][:rows] != s["vmap_curr"][:rows])   # the holes are the vertex map's holes
