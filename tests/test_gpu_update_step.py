"""GPU parity, operator tier: what the tracker does between two reductions, and at the end of a call, as its kernels run it.

The update step (ef_op_gn_update): one workgroup runs the head of k_track_step — solve_prefetch, the 58 sums in LDS, solve_step_wave with
gauss_newton_update_wave behind it (A and b from the sums, the 6x6 LDL^T, computeUpdateSE3, upd * resultRt, the float pose, K R K^-1 / K t),
with a flag in the SPLIT_TAIL form whose two tails run on two wavefronts side by side — on caller-supplied state, no image.  The reference is
efo_gn_update: the function the oracle's driver loop itself runs (tests/test_oracle_vs_reference_driver.py pins that loop to the compiled
RGBDOdometry.cpp).  sin and cos of the increment's angle come from two libms, so the test takes the angle from the oracle's own solution,
asks the device for its sin and cos (the `scalar` probe) and hands them to the oracle: EVERY output is then compared bit for bit.  The
device code evaluates one sincos() where the oracle has sin() and cos(); it claims the three agree bit for bit, and this comparison holds
it to that.  tests/test_wave_emulation.py runs the same cases through the same device code on 64 emulated lanes without a GPU.

The end of tracking (ef_op_track_end_tail): track_end_tail on one lane — the 0.3 m guard, polar3, matrix -> quaternion, the float pose
matrices, the velocity weighting, the logged pose — against efo_track_end, the oracle's own statements."""
import numpy as np
import pytest

import efo
import gn_cases

pytestmark = pytest.mark.gpu

GN_ARGS = ("sums", "prev", "Rprev", "tprev", "count", "sigma", "icp", "rgb", "rgbOnly", "icpWeight", "knext", "level_changes")
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def ops():
    from elasticfusion_amd import api
    return api.ops


def ulps(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), 5e-324)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b, equal_nan=False):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b, a.dtype)
    if equal_nan and a.dtype.kind == "f":   # a NaN is a NaN (0 / 0 has the sign bit set on one machine and clear on the other)
        n = np.isnan(a)
        return np.array_equal(n, np.isnan(b)) and np.array_equal(bits(a)[~n], bits(b)[~n])
    return np.array_equal(bits(a), bits(b))


def canaries():
    return np.full(36, gn_cases.CANARY), np.full(6, gn_cases.CANARY), np.full(4, gn_cases.CANARY, np.float32)


@pytest.fixture(scope="module")
def references(ops):
    """per case: the oracle's update step with the DEVICE's sin and cos of its own angle (computed once, shared, never modified)"""
    out = {}
    for c in gn_cases.cases():
        args = [c[k] for k in GN_ARGS]
        x = efo.gn_update(*args, *canaries())[4]
        sincos = None
        if np.all(np.isfinite(x)):
            theta = np.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5])
            sincos = ops.linalg("scalar", [theta, 1.0], 5)[2:4]
            assert ulps(sincos, [np.sin(theta), np.cos(theta)]).max() <= 1, (c["name"], theta, sincos)
        else:
            assert gn_cases.takes_the_break(c), c["name"]
        ref = efo.gn_update(*args, *canaries(), sincos=sincos)
        for a in ref[1:]:
            a.flags.writeable = False
        out[c["name"]] = ref
    return out


def test_the_cases_reach_the_edges(references):
    """asserted on the CPU, from the oracle's results: which cases rotate, which take the identity arm of the DBL_EPSILON test, which
    break, where K R K^-1 is re-evaluated and where it is copied"""
    cs = {c["name"]: c for c in gn_cases.cases()}
    theta = {n: float(np.sqrt(np.sum(r[4][3:] ** 2))) for n, r in references.items()}
    assert theta["all_zero_sums"] == 0.0 and 0 < theta["theta_below_epsilon"] < EPS < theta["theta_above_epsilon"] and theta["theta_equals_epsilon"] == EPS
    eye = np.eye(4).reshape(16)
    assert np.array_equal(references["theta_below_epsilon"][0]["resultRt"][[0, 5, 10]], [1, 1, 1]) and references["theta_below_epsilon"][0]["resultRt"][9] == 0
    assert references["theta_equals_epsilon"][0]["resultRt"][9] == EPS         # >= : the bound itself rotates (about x)
    assert np.array_equal(references["all_zero_sums"][0]["resultRt"], eye)
    assert 2.3 < theta["rotation_2p5"] < 2.7
    broke = sorted(n for n, c in cs.items() if gn_cases.takes_the_break(c))
    assert broke == sorted(n for n in cs if "error_above" in n or "already_broken" in n), broke
    for n in broke:
        nxt, A, b, st, _ = references[n]
        lc = cs[n]["level_changes"]
        assert np.all(A == gn_cases.CANARY) and np.all(b == gn_cases.CANARY) and np.all(st == gn_cases.CANARY)
        assert nxt["rgb_broken"] == (0 if lc else 1) and np.array_equal(nxt["resultRt"], cs[n]["prev"]["resultRt"])
        assert np.array_equal(nxt["krkinv"], cs[n]["prev"]["krkinv"]) == (not lc), n   # copied / re-evaluated for the new level
    assert np.isnan(references["icp_off"][3][0]) and references["icp_off"][3][1] == 0
    assert np.isinf(references["icp_count_zero"][3][0])
    assert references["rgbonly_count_zero"][3][3] == 0 and references["rgbonly_count_zero"][3][2] == np.float32(np.sqrt(90001.0))


@pytest.mark.parametrize("name", [c["name"] for c in gn_cases.cases()])
def test_update_step_equals_the_oracle_bit_for_bit(ops, references, name):
    c = next(c for c in gn_cases.cases() if c["name"] == name)
    want, A_w, b_w, st_w, _ = references[name]
    runs = []
    for split in (0, 1):
        got, A, b, st = ops.gn_update(*[c[k] for k in GN_ARGS], split, *canaries())
        for k in ("resultRt", "Rcurr", "tcurr", "krkinv", "kt", "lastRGBErrorLevel"):
            assert same_bits(got[k], want[k]), (name, split, k, got[k], want[k])
        assert got["rgb_broken"] == want["rgb_broken"], (name, split)
        assert same_bits(A, A_w) and same_bits(b, b_w), (name, split, A, A_w, b, b_w)
        assert same_bits(st, st_w, equal_nan=True), (name, split, st, st_w)
        runs.append((got, A, b, st))
    (g0, A0, b0, s0), (g1, A1, b1, s1) = runs                                   # ... and the two forms of the tail agree with each other
    assert all(same_bits(g0[k], g1[k]) for k in g0 if k != "rgb_broken") and g0["rgb_broken"] == g1["rgb_broken"]
    assert same_bits(A0, A1) and same_bits(b0, b1) and same_bits(s0, s1)


# ------------------------------------------------------------------------------------------------
# the end of tracking
# ------------------------------------------------------------------------------------------------
END_KEYS = ("q", "t", "T_cw", "pose_f", "R_wc_f", "t_wc_f", "logged")
IDENT_Q = np.array([0.0, 0.0, 0.0, 1.0])


def check_track_end(ops, tag, *args):
    want = efo.track_end(*args)
    got = ops.track_end_tail(*args)
    for k in END_KEYS:
        assert same_bits(got[k], want[k]), (tag, k, got[k], want[k])
    # the weighting passes through atan2 / sin / cos of two libms: the oracle's float or a neighbour of it
    d = abs(int(np.float32(got["weighting"]).view(np.int32)) - int(np.float32(want["weighting"]).view(np.int32)))
    assert d <= 1, (tag, got["weighting"], want["weighting"])
    return want


def test_track_end_quaternion_branches(ops):
    """Rcurr = the float cast of rotations of 119 ... 180 degrees, as they are and with 1e-6 of float noise (polar3 has work to do): a camera
    that has turned round takes the non-positive-trace branches of matrix -> quaternion in every frame"""
    rng = np.random.RandomState(21)
    taken, w_negative = [], 0
    for name, R in gn_cases.big_rotations():
        for noise in (0.0, 1e-6):
            Rc = (R.astype(np.float32) + (rng.randn(3, 3) * noise).astype(np.float32)).reshape(9)
            tc = rng.randn(3).astype(np.float32) * np.float32(0.05)
            want = check_track_end(ops, (name, noise), Rc, tc, np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32), IDENT_Q, np.zeros(3), 1, 1.0)
            Rp = np.zeros(9)
            efo.lib().efo_polar3(efo.ptr(np.ascontiguousarray(Rc, np.float64)), efo.ptr(Rp))
            taken.append(gn_cases.quat_branch(Rp))
            w_negative += want["q"][3] < 0
    assert all(taken.count(k) >= 3 for k in range(4)), taken
    assert w_negative >= 3


def test_track_end_displacement_guard(ops):
    """the photometric term's 0.3 m guard compares a float norm with the DOUBLE 0.3: a displacement of exactly 0.3f (0.30000001...) is
    over it, the float below is not; 0.29 and 0.31 along an oblique direction; each with the term on and off.  Where the guard applies the
    pose falls back to Rprev | tprev — here a rotation of another quaternion branch, so a wrong fall-back shows in q"""
    rots = dict(gn_cases.big_rotations())
    Rprev, Rcurr = rots["oblique_4"].astype(np.float32).reshape(9), rots["y_121.0000"].astype(np.float32).reshape(9)
    f03 = np.float32(0.3)
    d = np.array([0.48, -0.6, 0.64])
    tp = np.array([0.5, -1.25, 2.0], np.float32)
    cases = [("exactly_0.3f", np.zeros(3, np.float32), np.array([0, f03, 0], np.float32), True),
             ("float_below_0.3f", np.zeros(3, np.float32), np.array([0, np.nextafter(f03, np.float32(0)), 0], np.float32), False),
             ("oblique_0.29", tp, (tp + (d * 0.29).astype(np.float32)).astype(np.float32), False),
             ("oblique_0.31", tp, (tp + (d * 0.31).astype(np.float32)).astype(np.float32), True)]
    for tag, tprev, tcurr, over in cases:
        for rgb in (1, 0):
            want = check_track_end(ops, (tag, rgb), Rcurr, tcurr, Rprev, tprev, IDENT_Q, np.zeros(3), rgb, 1.0)
            fell_back = same_bits(want["t"], tprev.astype(np.float64))
            assert fell_back == bool(over and rgb), (tag, rgb, want["t"])
            assert (gn_cases.quat_branch(want["logged"].reshape(4, 4)[:3, :3]) == 2) == fell_back, (tag, rgb)


def _quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def test_track_end_velocity_weighting(ops):
    """the previous pose identical to the new one, 1e-12 away, 0.002 / 0.005 / 0.02 m away, 0.004 / 0.02 rad away — the weighting's 0.01
    clamp and its 0.5 floor from both sides — and the same previous pose with its quaternion negated (the same rotation; the relative pose
    then has w < 0), for a pose of the positive-trace branch and for one whose own quaternion has w < 0, with weightMultiplier 1 and 0.25"""
    rots = dict(gn_cases.big_rotations())
    seen = set()
    for name in ("x_119.0000", "oblique_1"):
        Rc, tc = rots[name].astype(np.float32).reshape(9), np.array([0.2, -0.1, 0.4], np.float32)
        eye, zero = np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32)
        pose = efo.track_end(Rc, tc, eye, zero, IDENT_Q, np.zeros(3), 0, 1.0)
        q, t = pose["q"], pose["t"]
        assert (q[3] < 0) == (name == "oblique_1")
        small = lambda a: np.array([0.6 * np.sin(a / 2), 0.0, -0.8 * np.sin(a / 2), np.cos(a / 2)])
        prevs = [("identical", q, t, 1.0), ("1e-12", q, t + 1e-12, 1.0), ("2mm", q, t + np.array([0.0012, 0.0, -0.0016]), 0.8),
                 ("5mm", q, t + np.array([0.003, -0.004, 0.0]), 0.5), ("2cm", q, t + np.array([0.0, 0.012, 0.016]), 0.5),
                 ("4mrad", _quat_mul(q, small(0.004)), t, 0.6), ("20mrad", _quat_mul(q, small(0.02)), t, 0.5), ("negated_previous", -q, t + np.array([0.001, 0.0, 0.0]), 0.9),
                 ("negated_4mrad", -_quat_mul(q, small(0.004)), t, 0.6)]   # the relative rotation has w < 0: SE3::log's atan2(-n, -w) arm
        for tag, qp, tp, expect in prevs:
            for wm in (1.0, 0.25):
                want = check_track_end(ops, (name, tag, wm), Rc, tc, eye, zero, qp, tp, 0, wm)
                assert abs(float(want["weighting"]) - expect * wm) < 2e-3 * wm, (name, tag, wm, want["weighting"])
                seen.add("floor" if float(want["weighting"]) == 0.5 * wm else "slope")
    assert seen == {"floor", "slope"}
