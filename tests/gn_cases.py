"""Inputs of one Gauss-Newton update step (the 58 sums two reductions leave, the state of the previous iteration, the call's constants)
at the edges of the step, shared by the GPU operator test (tests/test_gpu_update_step.py) and the host emulation of the same device
code (tests/test_wave_emulation.py).  Plain data, no GPU, no oracle."""
import numpy as np

FLT_MAX = np.float32(3.402823466e+38)
K640 = (528.0, 528.0, 320.0, 240.0)          # level 0 of a 640x480 camera
K160 = tuple(v / 4 for v in K640)            # its level 2
CANARY = -7.0                                # lastA / lastb / statistics before the step: a step that breaks must leave them


def pack29(A, b, r0=0.0, r1=0.0):
    """A [6, 6] symmetric, b [6], the two residual members -> the 29 floats of JtJJtrSE3 (types.cuh:98-143, reduce.cu:385-400)"""
    out = []
    for i in range(6):
        for j in range(i, 7):
            out.append(b[i] if j == 6 else A[i, j])
    return np.array(out + [r0, r1], np.float32)


def normal_equations(seed, x=None):
    """J^T J and J^T r of 40 rows with the tracker's usual scaling (translations in metres, rotations in radians); x given: b = A x"""
    rng = np.random.RandomState(seed)
    J = rng.randn(40, 6) * np.array([100, 100, 100, 1, 1, 1.0])
    r = rng.randn(40) * 0.01
    A = J.T @ J
    b = J.T @ r if x is None else A @ np.asarray(x, np.float64)
    return A, b, float(r @ r)


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _case(name, **kw):
    A1, b1, r1 = normal_equations(1)
    A2, b2, _ = normal_equations(2)
    c = dict(name=name, sums=np.concatenate([pack29(A1, b1, r1, 40.0), pack29(A2, b2)]),
             prev=dict(Rcurr=np.eye(3, dtype=np.float32).reshape(9), tcurr=np.zeros(3, np.float32), resultRt=np.eye(4).reshape(16),
                       krkinv=np.linspace(-2, 3, 9).astype(np.float32), kt=np.array([7.5, -3.25, 0.125], np.float32),
                       lastRGBErrorLevel=FLT_MAX, rgb_broken=0),
             Rprev=np.eye(3, dtype=np.float32).reshape(9), tprev=np.zeros(3, np.float32), count=30011, sigma=700001,
             icp=1, rgb=1, rgbOnly=0, icpWeight=10.0, knext=K640, level_changes=0)
    prev = kw.pop("prev", {})
    c.update(kw)
    c["prev"] = dict(c["prev"], **prev)
    return c


def _rgb_error(sigma, count):
    return np.float32(np.sqrt(np.float64(sigma)) / (count if count else 1))


def cases():
    out = [_case("icp_rgb_w10"), _case("icp_only", rgb=0, icpWeight=100.0), _case("icp_off", icp=0, icpWeight=0.0)]
    A1, b1, r1 = normal_equations(1)
    A2, b2, _ = normal_equations(2)
    # largest pivots last: every step of the factorisation swaps
    out.append(_case("reversed", sums=np.concatenate([pack29(A1[::-1, ::-1], b1[::-1], r1, 40.0), pack29(A2[::-1, ::-1], b2[::-1])])))
    Z1, Z2 = A1.copy(), A2.copy()
    Z1[2, :] = 0; Z1[:, 2] = 0; Z2[2, :] = 0; Z2[:, 2] = 0
    out.append(_case("zero_row_and_column", sums=np.concatenate([pack29(Z1, b1, r1, 40.0), pack29(Z2, b2)])))
    out.append(_case("all_zero_sums", sums=np.zeros(58, np.float32)))                       # theta = 0: the update is the identity
    # the two sides of DBL_EPSILON, and the bound itself (2^-52 is a float; theta = sqrt(2^-104) = 2^-52 exactly: >= rotates, > would not)
    for tag, v in (("below", 1e-16), ("above", 3e-16), ("equals", 2.0 ** -52)):
        b = np.zeros(6); b[3] = v
        out.append(_case("theta_%s_epsilon" % tag, rgb=0, icpWeight=100.0, sums=np.concatenate([pack29(np.eye(6), b, 1.0, 40.0), np.zeros(29, np.float32)])))
    A, b, r = normal_equations(3, x=[0.01, 0.02, -0.01, 1.5, -1.2, 1.6])                      # |rotation| ~ 2.5
    out.append(_case("rotation_2p5", rgb=0, icpWeight=100.0, sums=np.concatenate([pack29(A, b, r, 40.0), np.zeros(29, np.float32)])))
    T = np.eye(4)
    T[:3, :3] = rot([0.3, -1.0, 0.5], 2.0)
    T[:3, 3] = [0.1, -0.15, 0.09]                                                             # 0.2 m
    out.append(_case("prev_2rad_0p2m", prev=dict(resultRt=T.reshape(16))))
    out.append(_case("Rprev_170deg", Rprev=rot([1, 2, -1], np.radians(170)).astype(np.float32).reshape(9), tprev=np.array([0.5, -1.25, 2.0], np.float32)))
    out.append(_case("k640_level_changes", level_changes=1))
    out.append(_case("k160", knext=K160))
    out.append(_case("k160_level_changes", knext=K160, level_changes=1, prev=dict(resultRt=T.reshape(16))))
    # rgbOnly: the break on either side of lastRGBErrorLevel (and on it: not greater, no break), with and without a level change — which
    # selects between re-evaluating K R K^-1 / K t for the new level and copying them
    count, sigma = 10000, 40001
    e = _rgb_error(sigma, count)
    ro = dict(icp=0, rgbOnly=1, icpWeight=0.0, count=count, sigma=sigma)
    for lc in (0, 1):
        out.append(_case("rgbonly_error_above_last_lc%d" % lc, level_changes=lc, knext=K160 if lc else K640, prev=dict(lastRGBErrorLevel=np.nextafter(e, np.float32(0)), resultRt=T.reshape(16)), **ro))
        out.append(_case("rgbonly_error_equals_last_lc%d" % lc, level_changes=lc, prev=dict(lastRGBErrorLevel=e), **ro))
        out.append(_case("rgbonly_error_below_last_lc%d" % lc, level_changes=lc, prev=dict(lastRGBErrorLevel=np.nextafter(e, np.float32(1))), **ro))
        out.append(_case("rgbonly_already_broken_lc%d" % lc, level_changes=lc, knext=K160 if lc else K640, prev=dict(rgb_broken=1, lastRGBErrorLevel=np.float32(0.5), resultRt=T.reshape(16)), **ro))
    out.append(_case("rgbonly_count_zero", **dict(ro, count=0, sigma=90001)))                # the error divides by 1
    s = _case("x")["sums"].copy()
    s[28] = 0
    out.append(_case("icp_count_zero", sums=s))                                               # lastICPError = sqrt(.) / 0
    return out


def takes_the_break(c):
    """whether the step leaves everything as it is (the oracle's loop has left the level)"""
    return bool(c["prev"]["rgb_broken"]) or bool(c["rgbOnly"] and _rgb_error(c["sigma"], c["count"]) > c["prev"]["lastRGBErrorLevel"])


# ---- rotations of 120 degrees and more: the three non-positive-trace branches of Eigen's matrix -> quaternion ----
def big_rotations():
    """[(name, R [3, 3] float64)]: 119 (the trace > 0 side), 121, 179.9999 and 180 degrees about x, y, z, and ten oblique axes of either
    sign with angles in [2.1, pi]"""
    out = []
    for deg in (119.0, 121.0, 179.9999, 180.0):
        for k, n in enumerate("xyz"):
            out.append(("%s_%.4f" % (n, deg), rot(np.eye(3)[k], np.radians(deg))))
    rng = np.random.RandomState(11)
    for i in range(10):
        out.append(("oblique_%d" % i, rot(rng.randn(3), rng.uniform(2.1, np.pi))))
    return out


def quat_branch(R):
    """the branch Eigen::Quaternion(Matrix3) takes for R: 3 = positive trace, otherwise the index of the largest diagonal entry (first wins)"""
    R = np.asarray(R).reshape(3, 3)
    if R[0, 0] + R[1, 1] + R[2, 2] > 0.0:
        return 3
    i = 1 if R[1, 1] > R[0, 0] else 0
    return 2 if R[2, 2] > R[i, i] else i
