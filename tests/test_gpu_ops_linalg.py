"""GPU parity, operator tier: the tracking driver's small linear algebra (Eigen / Sophus restatement) as the DEVICE
evaluates it (elasticfusion_amd/csrc/ef_linalg_dev.hpp and the wavefront factorisations of ef_solve_dev.hpp, through ef_op_linalg)
against the oracle's efo_linalg.h.
Everything built from IEEE +,-,*,/,sqrt must agree bit for bit; sin/cos/atan2 come from two different libms
(glibc on the host, ocml on the device), so results that pass through them get a 2-ulp bar."""
import ctypes as C

import numpy as np
import pytest

import efo
import gn_cases

pytestmark = pytest.mark.gpu

LDLT6 = ("ldlt6", "ldlt6_wave", "ldlt6_every_lane")   # the scalar restatement, the earlier one-element-per-lane wavefront version (kept for tests), the one the update step runs
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def ops():
    from elasticfusion_amd import api
    return api.ops


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ulps(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), 5e-324)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(np.ascontiguousarray(b, np.asarray(a).dtype)))


def oracle(name, *inputs, n_out):
    out = np.zeros(n_out)
    getattr(efo.lib(), name)(*[_p(np.ascontiguousarray(a, np.float64)) for a in inputs], _p(out))
    return out


def pose(R, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[:3, :3] = np.asarray(R).reshape(3, 3)
    T[:3, 3] = t
    return np.ascontiguousarray(T)


def test_fp64_scalar_ops_are_ieee(ops):
    rng = np.random.RandomState(3)
    for _ in range(200):
        a, b = float(rng.uniform(1e-6, 50.0)), float(rng.uniform(-30.0, 30.0)) or 1.0
        out = ops.linalg("scalar", [a, b], 5)
        assert out[0] == np.sqrt(a), (a, out[0], np.sqrt(a))
        assert out[1] == a / b
        assert ulps(out[2:5], [np.sin(a), np.cos(a), np.arctan2(a, b)]).max() <= 1


def check_ldlt6(ops, A, b, tag):
    """all three device versions of the 6x6 solve against the oracle's, bit for bit; returns the oracle's solution"""
    A, b = np.ascontiguousarray(A, np.float64), np.ascontiguousarray(b, np.float64)
    x_r = oracle("efo_ldlt6", A, b, n_out=6)
    for which in LDLT6:
        x = ops.linalg(which, np.concatenate([A.reshape(-1), b]), 6)
        assert same_bits(x, x_r), (which, tag, x, x_r)
    return x_r


def test_ldlt6_bit_exact(ops):
    rng = np.random.RandomState(0)
    for t in range(20):
        J = rng.randn(40, 6) * np.array([100, 100, 100, 1, 1, 1.0])
        A = np.ascontiguousarray(J.T @ J)
        if t % 5 == 4:
            A[2, :] = 0; A[:, 2] = 0   # a singular direction (Eigen leaves the component at 0)
        check_ldlt6(ops, A, rng.randn(6), t)


def test_ldlt6_degenerate_systems(ops):
    """what a frame without correspondences hands the solver (a covered lens: A = 0, b = 0), a rank-one system, and a system with a zero
    block: Eigen::LDLT's zero-pivot branch leaves the factorisation where it stands and the solve sets those components to 0"""
    rng = np.random.RandomState(5)
    cases = []
    cases.append((np.zeros((6, 6)), np.zeros(6)))
    cases.append((np.zeros((6, 6)), rng.randn(6)))
    v = rng.randn(6)
    cases.append((np.outer(v, v), rng.randn(6)))
    J = rng.randn(30, 3)
    A = np.zeros((6, 6))
    A[3:, 3:] = J.T @ J                                            # rotation constrained, translation not at all
    cases.append((A, rng.randn(6)))
    for t, (A, b) in enumerate(cases):
        x_r = check_ldlt6(ops, A, b, t)
    assert not np.any(x_r[:3]) and np.all(np.isfinite(x_r))


def pivoting_systems():
    rng = np.random.RandomState(7)
    J = rng.randn(40, 6) * np.array([100, 100, 100, 1, 1, 1.0])
    A, b = J.T @ J, rng.randn(6)
    out = [("largest_pivots_last", A[::-1, ::-1].copy(), b)]                       # every step swaps
    T = A.copy()
    T[np.arange(6), np.arange(6)] = np.array([3.0, 3.0, 5.0, 5.0, 5.0, 3.0]) * 1e4   # exact ties on the diagonal: the first one wins
    out.append(("diagonal_ties", T, b))
    out.append(("identity_all_ties", np.eye(6), b))
    N = A.copy()
    N[4, 4] = -2.0 * A[0, 0]                                                        # indefinite: the largest |diagonal| is negative
    out.append(("negative_pivot", N, b))
    out.append(("negative_definite", -A, b))
    D = np.diag([4.0, 1e-300, 2.0, 8.0, 0.5, 1.0])
    out.append(("diagonal_with_1e-300", D, b))
    out.append(("scaled_up_1e150", A * 1e150, b * 1e150))
    out.append(("scaled_down_1e-150", A * 1e-150, b * 1e-150))
    return out


def test_ldlt6_pivoting_edges(ops):
    """every step swaps, ties (first wins), a negative pivot, a pivot of 1e-300 (above DBL_MIN: divided by, not zeroed), 1e+-150 scalings:
    the static-index swap chains of the three device versions against the oracle; and the pivots ldlt_pivots reports for the same
    matrices against the ones the oracle's solve divides by"""
    pivots = {}
    for tag, A, b in pivoting_systems():
        check_ldlt6(ops, A, b, tag)
        A = np.ascontiguousarray(A, np.float64)
        pivots[tag] = d_r = oracle("efo_ldlt_pivots", A, n_out=6)
        assert same_bits(ops.linalg("ldlt_pivots", A.reshape(-1), 6), d_r), (tag, d_r)
    # the cases are what their names say: the first step of the reversed system takes its pivot from the far end and the small diagonal
    # entries come last, the identity's pivots are its diagonal in order, the indefinite system's first pivot is the negative entry
    A_rev = pivoting_systems()[0][1]
    assert np.argmax(np.abs(np.diag(A_rev))) >= 3 and pivots["largest_pivots_last"][0] == np.abs(np.diag(A_rev)).max()
    assert np.all(np.abs(pivots["largest_pivots_last"][:3]) > 100 * np.abs(pivots["largest_pivots_last"][3:]))
    assert np.array_equal(pivots["identity_all_ties"], np.ones(6)) and pivots["diagonal_ties"][0] == 5e4
    assert pivots["negative_pivot"][0] < 0 and np.all(pivots["negative_definite"] < 0)
    assert np.array_equal(pivots["diagonal_with_1e-300"], [8.0, 4.0, 2.0, 1.0, 0.5, 1e-300])
    rng = np.random.RandomState(8)
    for t in range(5):                                                               # ... and on the everyday systems
        J = rng.randn(40, 6) * np.array([100, 100, 100, 1, 1, 1.0])
        A = np.ascontiguousarray(J.T @ J)
        assert same_bits(ops.linalg("ldlt_pivots", A.reshape(-1), 6), oracle("efo_ldlt_pivots", A, n_out=6)), t


def test_lu_inverse6_bit_exact(ops):
    """getCovariance's PartialPivLU inverse: normal matrices, the same with the largest entries last, and general matrices whose first
    column has its largest entry anywhere (row pivoting at every step)"""
    rng = np.random.RandomState(9)
    mats = []
    for t in range(4):
        J = rng.randn(40, 6) * np.array([100, 100, 100, 1, 1, 1.0])
        mats += [J.T @ J, (J.T @ J)[::-1, ::-1].copy()]
    for t in range(4):
        M = rng.randn(6, 6)
        M[0, 0] = 1e-9
        mats.append(M)
    for t, M in enumerate(mats):
        M = np.ascontiguousarray(M, np.float64)
        inv = ops.linalg("lu_inverse6", M.reshape(-1), 36)
        assert same_bits(inv, efo.covariance(M).reshape(-1)), t
    assert np.abs(mats[-1] @ efo.covariance(mats[-1]) - np.eye(6)).max() < 1e-6


def test_ldlt3f_bit_exact(ops):
    rng = np.random.RandomState(1)
    for _ in range(20):
        J = rng.randn(30, 3).astype(np.float32)
        A = np.ascontiguousarray(J.T @ J)
        b = rng.randn(3).astype(np.float32)
        x_r = np.zeros(3, np.float32)
        efo.lib().efo_ldlt3f(_p(A), _p(b), _p(x_r))
        x = ops.linalg("ldlt3f", np.concatenate([A.reshape(-1), b]).astype(np.float64), 3).astype(np.float32)
        assert np.array_equal(x.view(np.uint32), x_r.view(np.uint32))


def _small_rot(rng, s=0.05):
    v = rng.randn(3) * s
    R = np.zeros(9)
    efo.lib().efo_rodrigues(_p(np.ascontiguousarray(v)), _p(R))
    return R.reshape(3, 3)


def test_polar3_bit_exact(ops):
    rng = np.random.RandomState(2)
    for _ in range(20):
        A = np.ascontiguousarray((_small_rot(rng).astype(np.float32) + rng.randn(3, 3).astype(np.float32) * 1e-6).astype(np.float64))
        R_r = np.zeros(9)
        efo.lib().efo_polar3(_p(A), _p(R_r))
        R = ops.linalg("polar3", A, 9)
        assert np.array_equal(R.view(np.uint64), R_r.view(np.uint64)), np.abs(R - R_r).max()


def test_polar3_away_from_a_rotation(ops):
    """inputs the Jacobi sweeps have to work on: a rotation plus 0.3 randn, a rotation with one column scaled by 1e-3, a reflection
    (rotation times diag(1, 1, -1): the answer has determinant -1, and the device must return the same bits), float-rounded rotations of up
    to 3 rad.  No rank-deficient input: there the oracle's answer is arbitrary."""
    rng = np.random.RandomState(12)
    mats = []
    for k in range(5):
        R = gn_cases.rot(rng.randn(3), rng.uniform(0.2, 3.0))
        mats.append(("noisy", R + 0.3 * rng.randn(3, 3)))
        S = R.copy()
        S[:, k % 3] *= 1e-3
        mats.append(("scaled_column", S))
        mats.append(("reflected", R @ np.diag([1.0, 1.0, -1.0])))
        mats.append(("float_rounded", gn_cases.rot(rng.randn(3), (k + 1) * 0.6).astype(np.float32).astype(np.float64)))
    dets = []
    for tag, A in mats:
        assert np.linalg.svd(A, compute_uv=False).min() > 5e-4, tag
        A = np.ascontiguousarray(A)
        R_r = oracle("efo_polar3", A, n_out=9)
        R = ops.linalg("polar3", A, 9)
        assert same_bits(R, R_r), (tag, np.abs(R - R_r).max())
        assert np.abs(R_r.reshape(3, 3) @ R_r.reshape(3, 3).T - np.eye(3)).max() < 1e-12, tag
        dets.append((tag, np.linalg.det(R_r.reshape(3, 3))))
    assert all((d < -0.99) == (tag == "reflected") for tag, d in dets), dets


def test_rodrigues_and_se3(ops):
    rng = np.random.RandomState(4)
    for _ in range(20):
        v = np.ascontiguousarray(rng.randn(3) * 0.02)
        R_r = np.zeros(9)
        efo.lib().efo_rodrigues(_p(v), _p(R_r))
        R = ops.linalg("rodrigues", v, 9)
        assert ulps(R, R_r).max() <= 2 or np.abs(R - R_r).max() < 1e-18      # sin / cos from two libms
        T = np.eye(4)
        T[:3, :3] = R_r.reshape(3, 3)
        T[:3, 3] = rng.randn(3) * 0.01
        T = np.ascontiguousarray(T)
        Ti_r = np.zeros(16)
        efo.lib().efo_se3_inverse(_p(T), _p(Ti_r))
        Ti = ops.linalg("se3_inverse", T, 16)
        assert np.array_equal(Ti.view(np.uint64), Ti_r.view(np.uint64))       # +,-,*,/,sqrt only
        efo.lib().efo_se3_log_norm.restype = C.c_double
        ln_r = efo.lib().efo_se3_log_norm(_p(T), None)
        ln = ops.linalg("se3_log_norm", T, 1)[0]
        assert abs(ln - ln_r) <= 1e-12 * max(ln_r, 1e-6)                      # atan2 / sin / cos inside


RODRIGUES_NORMS = (0.0, 1e-17, 2.0e-16, EPS, 2.5e-16, 1e-8, 1.0, np.pi)   # zero, far below / just below / on / just above DBL_EPSILON, small, large, pi


def test_rodrigues_edges(ops):
    """theta = 0, either side of the DBL_EPSILON test and on it (>= : the bound rotates), 1e-8, 1 and pi.
    Against the oracle with glibc's sin / cos the file's 2-ulp bar applies, along a coordinate axis: there every entry is cos, +-sin, a sum
    that is 1 to the last bit or 0, so the bar measures the two libms and nothing else (along an oblique axis entries such as
    cos + (1 - cos) r_x^2 cancel near pi, and one ulp of cos becomes many of the entry).  Oblique axes are compared bit for bit instead, with
    the device's own sin and cos of the same theta handed to the oracle; those two stay within 1 ulp of numpy's."""
    d = np.array([0.48, -0.6, 0.64])                                       # |d| = 1 up to rounding
    for n in RODRIGUES_NORMS:
        for k in range(3):
            v = np.zeros(3)
            v[k] = n                                                       # |v| = n exactly
            R_r = oracle("efo_rodrigues", v, n_out=9)
            R = ops.linalg("rodrigues", v, 9)
            assert ulps(R, R_r).max() <= 2 or np.abs(R - R_r).max() < 1e-18, (n, k, R, R_r)
            assert (n >= EPS) == bool(np.any(R_r != np.eye(3).reshape(9))), (n, k)
        v = np.ascontiguousarray(d * n)
        theta = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        sc = ops.linalg("scalar", [theta, 1.0], 5)[2:4]
        assert ulps(sc, [np.sin(theta), np.cos(theta)]).max() <= 1, (n, sc)
        R_r = oracle("efo_rodrigues_sc", v, sc, n_out=9)
        R = ops.linalg("rodrigues", v, 9)
        assert same_bits(R, R_r), (n, R, R_r)


def test_quaternion_branches(ops):
    """rotations of 119 (positive trace), 121, 179.9999 and 180 degrees about x, y, z and ten oblique ones of 2.1 rad and more: all four
    branches of Eigen's matrix -> quaternion (the three diagonal ones are templates over the index so that nothing is indexed at run time),
    results with w < 0, and what the pose algebra makes of such quaternions: inverse, product with its renormalisation, the two float matrices"""
    rots = gn_cases.big_rotations()
    branch = [gn_cases.quat_branch(R) for _, R in rots]
    assert all(branch.count(k) >= 3 for k in range(4)), branch
    rng = np.random.RandomState(13)
    w_negative = 0
    for k, (name, R) in enumerate(rots):
        R = np.ascontiguousarray(R)
        q_r = oracle("efo_mat_to_quat", R, n_out=8)
        q = ops.linalg("mat_to_quat", R, 8)
        assert same_bits(q, q_r), (name, q, q_r)
        assert int(np.argmax(np.abs(q_r[:4]) * [1, 1, 1, 0])) == branch[k] or branch[k] == 3, (name, q_r)
        w_negative += q_r[7] < 0
        T, T2 = pose(R, rng.randn(3)), pose(rots[(k + 7) % len(rots)][1], rng.randn(3))
        assert same_bits(ops.linalg("se3_inverse", T, 16), oracle("efo_se3_inverse", T, n_out=16)), name
        assert same_bits(ops.linalg("se3_mul", np.concatenate([T.reshape(-1), T2.reshape(-1)]), 7), oracle("efo_se3_mul", T, T2, n_out=7)), name
        T_cw, pose_f = np.zeros(16, np.float32), np.zeros(16, np.float32)
        efo.lib().efo_pose_matrices(_p(T), _p(T_cw), _p(pose_f))
        assert same_bits(ops.linalg("se3_castf", T, 16).astype(np.float32), pose_f), name
        assert same_bits(ops.linalg("se3_inverse_f", T, 16).astype(np.float32), T_cw), name
    assert w_negative >= 3, w_negative


def test_se3_mul_renormalises(ops):
    """Sophus' product rescales the quaternion by 2 / (1 + |q|^2) unless |q|^2 is 1 to the last bit: both arms, on everyday poses"""
    rng = np.random.RandomState(14)
    for _ in range(12):
        Ta, Tb = pose(gn_cases.rot(rng.randn(3), rng.uniform(0, 3)), rng.randn(3)), pose(gn_cases.rot(rng.randn(3), rng.uniform(0, 0.1)), rng.randn(3) * 0.01)
        qt_r = oracle("efo_se3_mul", Ta, Tb, n_out=7)
        assert same_bits(ops.linalg("se3_mul", np.concatenate([Ta.reshape(-1), Tb.reshape(-1)]), 7), qt_r)
    I = pose(np.eye(3))
    assert same_bits(ops.linalg("se3_mul", np.concatenate([I.reshape(-1), I.reshape(-1)]), 7), oracle("efo_se3_mul", I, I, n_out=7))   # |q|^2 == 1: no rescale


def test_m4_affine_inverse_bit_exact(ops):
    """resultRt.inverse() (RGBDOdometry.cpp:407): a 4x4 with a general 3x3 block — rotations of up to 3 rad, the same perturbed, a sheared one"""
    rng = np.random.RandomState(15)
    for k in range(8):
        M = pose(gn_cases.rot(rng.randn(3), 0.4 * k + 0.1) + (0.1 * rng.randn(3, 3) if k % 2 else 0.0), rng.randn(3))
        assert same_bits(ops.linalg("m4_affine_inverse", M, 16), oracle("efo_m4_affine_inverse", M, n_out=16)), k


def log_norm_cases():
    t = np.array([0.3, -0.2, 0.5])
    rv = lambda v: oracle("efo_rodrigues", np.asarray(v, np.float64), n_out=9)
    negative = next(R for _, R in gn_cases.big_rotations() if oracle("efo_mat_to_quat", np.ascontiguousarray(R), n_out=8)[7] < 0)
    series = rv([6e-12, -8e-12, 0.0])
    return [("identity", pose(np.eye(3))), ("translation", pose(np.eye(3), t)),
            ("series", pose(series)),                                     # no translation: the norm IS |omega| = two_atan |q.xyz|
            ("series_small_t", pose(series, 1e-11 * t)),                  # translation of the rotation's own size: both halves carry weight
            ("series_t", pose(series, t)),
            ("angle_1e-6", pose(rv([6e-7, 0.0, 8e-7]))), ("angle_1e-3_t", pose(rv([6e-4, 0.0, 8e-4]), t)),
            ("angle_1_t", pose(rv([0.48, -0.6, 0.64]), t)), ("angle_3", pose(rv([1.8, -2.4, 0.0]))), ("angle_3_t", pose(rv([1.8, -2.4, 0.0]), t)),
            ("w_negative", pose(negative)), ("w_negative_t", pose(negative, t))]


def test_se3_log_norm_edges(ops):
    """the identity and a pure translation (series arm with sqn = 0), a rotation vector of 1e-11 (series arm, sqn > 0) without translation,
    with one of its own size and with one of order one, angles of 1e-6, 1e-3, 1 and 3.0, and a quaternion with w < 0 (the atan2(-n, -w) arm),
    the large ones with and without translation.
    Without translation the norm is |omega| = two_atan |q.xyz| and nothing else, so an error in two_atan shows at full size; with a
    translation of order one and an angle of 1e-3 and more, coef |omega|^2 is 1e-7 of the result and more, so the coef formula shows too.
    The series arm and coef = 1/12 use no libm, so there the comparison is bit for bit; elsewhere 1e-12 relative (atan2, sin, cos).
    What no input can show, in the norm or in the six components: the VALUE 1/12.  That arm is taken only when |omega| <= 2e-10, where
    coef Omega^2 t = -coef |omega|^2 t_perp is at most 4e-21 of the translation it is added to, far below half an ulp; any coef below 1e3
    gives the same bits."""
    efo.lib().efo_se3_log_norm.restype = C.c_double
    seen = set()
    for tag, T in log_norm_cases():
        q = oracle("efo_mat_to_quat", np.ascontiguousarray(T[:3, :3]), n_out=8)[4:]
        sqn = float(q[:3] @ q[:3])
        arm = "series" if sqn < 1e-20 else ("w<0" if q[3] < 0 else "atan2")
        seen.add(arm)
        assert (sqn > 0) == (tag not in ("identity", "translation")), (tag, sqn)
        ln_r = efo.lib().efo_se3_log_norm(_p(T), None)
        ln = ops.linalg("se3_log_norm", T, 1)[0]
        if arm == "series":
            assert same_bits(np.float64(ln), np.float64(ln_r)), (tag, ln, ln_r)
        else:
            assert abs(ln - ln_r) <= 1e-12 * ln_r, (tag, ln, ln_r)
    assert seen == {"series", "w<0", "atan2"}, seen
