"""Rigid registration of a point set against the map (ef_register_step / ef_register_update / ef_register_cloud, include/ef_hip.h; kernels in
elasticfusion_amd/csrc/ef_register.inc).

One step is restated here in numpy from the header's own words: the f32 transform in the written order, the pair ef_query_nearest gives for
the transformed point (pinned bit for bit against an exhaustive scan by test_gpu_query.py), the normal gate, the f32 row J and residual,
and the sums of exact double products taken with math.fsum.  The loop is restated from registerStep + register_update, and the answer it
converges to is judged against an independent float64 ICP (scipy cKDTree, numpy.linalg.solve, scipy expm), never against the library.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = 0xFFFFFFFF
F = np.float32
U = 2.0 ** -53
TWIST = np.array([0.02, -0.015, 0.01, 0.017, -0.01, 0.012])   # the generating motion: about 2.7 cm and 1.3 degrees


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def assert_bits_equal(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    d = bits(a) != bits(b)
    assert not d.any(), (what, int(d.sum()), np.argwhere(d)[:5], a[d][:5], b[d][:5])


def twist_matrix(xi):
    v, w = xi[:3], xi[3:]
    M = np.zeros((4, 4))
    M[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    M[:3, 3] = v
    return M


def pose_error(T, G):
    """translation (m) and rotation (rad) of T G^-1; the angle from the skew part (sin), which resolves angles far below the 1e-8 of arccos"""
    d = np.asarray(T, np.float64) @ np.linalg.inv(G)
    k = (d[:3, :3] - d[:3, :3].T) / 2
    return float(np.linalg.norm(d[:3, 3])), float(np.arcsin(min(1.0, math.sqrt(k[2, 1] ** 2 + k[0, 2] ** 2 + k[1, 0] ** 2))))


def transform_f32(T, pts, with_translation=True):
    """p' = ((Rf00*x + Rf01*y) + Rf02*z) + tfx ..., every operation rounded to f32 once, in the header's order"""
    T = np.eye(4) if T is None else np.asarray(T, np.float64)
    Rf, tf = T[:3, :3].astype(F), T[:3, 3].astype(F)
    x, y, z = (np.ascontiguousarray(pts[:, j], F) for j in range(3))
    out = np.empty((len(pts), 3), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(3):
            v = (Rf[i, 0] * x + Rf[i, 1] * y) + Rf[i, 2] * z
            out[:, i] = v + tf[i] if with_translation else v
    return out


def restate_step(ef, S, pts, nrm, T, max_dist, min_conf, min_normal_cos):
    """the header's step: (sums dict with "abs" = the sum of |term| per entry, row, plane)"""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    n = len(pts)
    q = transform_f32(T, pts)
    row, _, plane = ef.queryNearestRaw(q, max_dist, min_conf)
    row, plane = row.copy(), plane.copy()
    hit = row != MISS
    w = np.where(hit, row, 0).astype(np.int64)
    Ns = S[w, 8:11] if len(S) else np.zeros((n, 3), F)
    with np.errstate(invalid="ignore", over="ignore"):
        if nrm is not None and min_normal_cos > -1:
            m = transform_f32(T, np.ascontiguousarray(nrm, F).reshape(-1, 3), with_translation=False)
            cos = (m[:, 0] * Ns[:, 0] + m[:, 1] * Ns[:, 1]) + m[:, 2] * Ns[:, 2]
            hit = hit & (cos >= F(min_normal_cos))
        row[~hit] = MISS
        plane[~hit] = 0
        qh, nh = q[hit], Ns[hit]
        J = np.empty((len(qh), 6), F)
        J[:, :3] = nh
        J[:, 3] = qh[:, 1] * nh[:, 2] - qh[:, 2] * nh[:, 1]
        J[:, 4] = qh[:, 2] * nh[:, 0] - qh[:, 0] * nh[:, 2]
        J[:, 5] = qh[:, 0] * nh[:, 1] - qh[:, 1] * nh[:, 0]
    Jd, rd = J.astype(np.float64), plane[hit].astype(np.float64)
    A, Aabs = np.zeros((6, 6)), np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            t = Jd[:, i] * Jd[:, j]   # exact: two 24-bit significands
            A[i, j] = A[j, i] = math.fsum(t)
            Aabs[i, j] = Aabs[j, i] = math.fsum(np.abs(t))
    b, babs = np.zeros(6), np.zeros(6)
    for i in range(6):
        t = -(Jd[:, i] * rd)
        b[i], babs[i] = math.fsum(t), math.fsum(np.abs(t))
    e = math.fsum(rd * rd)
    return {"A": A, "b": b, "e": e, "pairs": int(hit.sum()), "points": n, "Aabs": Aabs, "babs": babs}, row, plane


def check_step(ef, S, pts, nrm, T, what, max_dist=0.05, min_conf=-1.0, min_normal_cos=-1.0):
    want, row, plane = restate_step(ef, S, pts, nrm, T, max_dist, min_conf, min_normal_cos)
    got = ef.registerStep(pts, nrm, T=T, pairs=True, max_dist=max_dist, min_conf=min_conf, min_normal_cos=min_normal_cos)
    bare = ef.registerStep(pts, nrm, T=T, max_dist=max_dist, min_conf=min_conf, min_normal_cos=min_normal_cos)
    print(what, "pairs", got["pairs"], "of", got["points"], "e", got["e"])
    assert got["pairs"] == want["pairs"] and got["points"] == want["points"] == len(np.asarray(pts).reshape(-1, 3)), (what, got["pairs"], want["pairs"])
    assert_bits_equal(got["row"], row, what + " rows")
    assert_bits_equal(got["plane"], plane, what + " plane")
    m = max(got["pairs"] - 1, 0)
    gamma = m * U / (1 - m * U)   # any order of adding `pairs` exact terms in double (Higham, Accuracy and Stability, eq. 4.4)
    worst = 0.0
    for key, mag in (("A", want["Aabs"]), ("b", want["babs"]), ("e", want["e"])):
        err = np.abs(np.asarray(got[key]) - np.asarray(want[key]))
        bound = gamma * np.asarray(mag)
        assert (err <= bound).all(), (what, key, err, bound)
        if np.any(np.asarray(mag) > 0):
            worst = max(worst, float(np.max(err[np.asarray(mag) > 0] / np.asarray(mag)[np.asarray(mag) > 0])))
    print(what, "largest error / sum of |terms|", worst, "gamma", gamma)
    assert_bits_equal(got["A"], got["A"].T.copy(), what + " symmetry")
    for key in ("A", "b"):
        assert_bits_equal(bare[key], got[key], what + " with and without the per-point outputs: " + key)
    assert bare["e"] == got["e"] and bare["pairs"] == got["pairs"]
    return got


@pytest.fixture(scope="module")
def world():
    from scipy.linalg import expm
    from elasticfusion_amd import api, synth
    S = synth.sample_surfels(synth.Sequence(0xEF0001), n=200000)
    assert len(S) == 199579
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    G = expm(twist_matrix(TWIST))
    Gi = np.linalg.inv(G)
    pick = np.sort(np.random.default_rng(0xC10D).choice(len(S), 50000, replace=False))
    pts = (S[pick, :3].astype(np.float64) @ Gi[:3, :3].T + Gi[:3, 3]).astype(F)
    nrm = (S[pick, 8:11].astype(np.float64) @ Gi[:3, :3].T).astype(F)
    yield dict(ef=ef, S=S, G=G, pts=pts, nrm=nrm, pick=pick)
    ef.close()


def test_step_equals_its_specification(world):
    ef, S, pts, nrm, G = (world[k] for k in ("ef", "S", "pts", "nrm", "G"))
    first = check_step(ef, S, pts, None, None, "identity, no normals")
    assert 40000 < first["pairs"] < 50000
    gated = check_step(ef, S, pts, nrm, None, "identity, normals, gate 0.5", min_normal_cos=0.5)
    assert 0 < gated["pairs"] < first["pairs"]            # the gate drops pairs across the room's edges
    tight = check_step(ef, S, pts, nrm, np.eye(4), "identity, normals, gate 0.999", min_normal_cos=0.999)   # the motion turns by 1.3 degrees: cos 0.99973
    assert 0 < tight["pairs"] <= gated["pairs"]
    off = check_step(ef, S, pts, nrm, None, "identity, normals, gate off", min_normal_cos=-1.0)
    for key in ("A", "b"):
        assert_bits_equal(off[key], first[key], "gate off equals no normals: " + key)
    at = check_step(ef, S, pts, nrm, G, "generating motion, normals", min_normal_cos=0.5)
    assert at["pairs"] > 49000 and math.sqrt(at["e"] / at["pairs"]) < 1e-5
    check_step(ef, S, pts[:777], None, G, "generating motion, 777 points, 2 cm", max_dist=0.02)


def test_step_edge_cases(world):
    from elasticfusion_amd import api
    ef, S, pts = world["ef"], world["S"], world["pts"]
    # NaN / inf points are misses; the finite ones beside them pair as before
    bad = pts[:64].copy()
    bad[3, 0], bad[7, 1], bad[11, 2], bad[20] = np.nan, np.inf, -np.inf, np.nan
    got = check_step(ef, S, bad, None, None, "non-finite points")
    assert (got["row"][[3, 7, 11, 20]] == MISS).all() and (got["plane"][[3, 7, 11, 20]] == 0).all() and got["pairs"] > 0
    assert np.isfinite(got["A"]).all() and np.isfinite(got["b"]).all()
    # n = 0
    none = ef.registerStep(np.zeros((0, 3), F), pairs=True, min_conf=-1.0)
    assert none["pairs"] == 0 and none["points"] == 0 and not none["A"].any() and not none["b"].any() and none["e"] == 0 and len(none["row"]) == 0
    T, res = ef.registerCloud(np.zeros((0, 3), F), min_conf=-1.0)
    assert res["status"] == api.REG_TOO_FEW_PAIRS and res["iterations"] == 0 and res["pairs"] == 0
    assert_bits_equal(T, np.eye(4), "n = 0 leaves the pose")
    # an empty map
    empty = api.ElasticFusion()
    try:
        got = check_step(empty, np.zeros((0, 12), F), pts[:100], None, None, "empty map")
        assert got["pairs"] == 0 and (got["row"] == MISS).all() and not got["A"].any()
        T0 = np.linalg.inv(world["G"])
        T, res = empty.registerCloud(pts[:100], T_init=T0, min_conf=-1.0)
        assert res["status"] == api.REG_TOO_FEW_PAIRS and res["rms_first"] == 0 and res["rms_last"] == 0
        assert_bits_equal(T, T0, "empty map leaves the pose")
        # min_conf at the context's threshold on a map with unstable surfels
        thr = float(empty.cfg.confidence)
        part = S[::8].copy()
        part[::3, 3] = thr          # not stable: eligible iff conf > min_conf
        part[1::3, 3] = thr / 2
        empty.uploadMap(part)
        every = check_step(empty, part, pts[:4096], None, None, "every surfel", max_dist=0.05, min_conf=-1.0)
        stable = check_step(empty, part, pts[:4096], None, None, "stable surfels", max_dist=0.05, min_conf=thr)
        assert 0 < stable["pairs"] < every["pairs"]
        assert (part[stable["row"][stable["row"] != MISS], 3] > F(thr)).all()
    finally:
        empty.close()


def test_step_is_reproducible_for_any_cell_size(world):
    ef, pts, nrm = world["ef"], world["pts"], world["nrm"]
    ref = None
    try:
        for cell in (0.02, 0.02, 0.01, 0.05):
            ef.setQueryCell(cell)
            for normals, cos in ((None, -1.0), (nrm, 0.5)):
                s = ef.registerStep(pts, normals, pairs=True, max_dist=0.05, min_conf=-1.0, min_normal_cos=cos)
                key = normals is None
                if ref is None:
                    ref = {}
                if key not in ref:
                    ref[key] = s
                    continue
                for name in ("A", "b", "row", "plane"):
                    assert_bits_equal(s[name], ref[key][name], f"cell {cell} {name}")
                assert s["e"] == ref[key]["e"] and s["pairs"] == ref[key]["pairs"]
    finally:
        ef.setQueryCell(ef.QUERY_DEFAULT_CELL)


def drive_loop(ef, api, pts, nrm, T0, params):
    """the header's loop from registerStep + register_update"""
    T = np.eye(4) if T0 is None else np.array(T0, np.float64)
    out = dict(iterations=0)
    closing = None
    first = True
    while True:
        s = ef.registerStep(pts, nrm, T=T, params=params)
        rms = math.sqrt(s["e"] / s["pairs"]) if s["pairs"] else 0.0
        if first:
            out["rms_first"] = rms
            first = False
        out["rms_last"], out["pairs"], out["A"] = rms, s["pairs"], s["A"]
        if closing is not None:
            out["status"] = closing
            break
        if s["pairs"] < params.min_pairs:
            out["status"] = api.REG_TOO_FEW_PAIRS
            break
        Tn, xi, degenerate = api.register_update(s, T)
        if degenerate:
            out["status"] = api.REG_DEGENERATE
            break
        T = Tn
        out["iterations"] += 1
        if math.sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]) < params.stop_translation and \
                math.sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]) < params.stop_rotation:
            closing = api.REG_CONVERGED
        elif out["iterations"] >= params.max_iterations:
            closing = api.REG_MAX_ITERATIONS
    return T, out


@pytest.mark.parametrize("normals", [False, True])
def test_loop_equals_its_parts(world, normals):
    from elasticfusion_amd import api
    ef, pts = world["ef"], world["pts"]
    nrm = world["nrm"] if normals else None
    seen = set()
    for k in range(1, 7):
        params = ef.registerParams(max_iterations=k, min_conf=-1.0)
        T, res = ef.registerCloud(pts, nrm, params=params)
        Tw, want = drive_loop(ef, api, pts, nrm, None, params)
        print("k", k, res["status_name"], res["iterations"], res["pairs"], res["rms_first"], res["rms_last"])
        assert_bits_equal(T, Tw, f"k = {k}: pose")
        for key in ("status", "iterations", "pairs", "rms_first", "rms_last"):
            assert res[key] == want[key], (k, key, res[key], want[key])
        assert_bits_equal(res["A"], want["A"], f"k = {k}: A")
        assert res["iterations"] <= k
        seen.add(res["status"])
    assert api.REG_MAX_ITERATIONS in seen and api.REG_CONVERGED in seen, seen
    # from another start, and a start nothing is near
    T0 = np.eye(4)
    T0[:3, 3] = (0.004, -0.003, 0.002)
    params = ef.registerParams(max_iterations=3, min_conf=-1.0, max_dist=0.03)
    T, res = ef.registerCloud(pts, nrm, T_init=T0, params=params)
    Tw, want = drive_loop(ef, api, pts, nrm, T0, params)
    assert_bits_equal(T, Tw, "other start: pose")
    assert res["status"] == want["status"] and res["iterations"] == want["iterations"] and res["pairs"] == want["pairs"]


def icp_float64(S, pts, nrm, iterations, max_dist, min_normal_cos):
    """an independent float64 point-to-plane ICP from the identity: scipy's KD-tree on the float64 surfel positions, the same gates, LAPACK, expm"""
    from scipy.linalg import expm
    from scipy.spatial import cKDTree
    P, N = S[:, :3].astype(np.float64), S[:, 8:11].astype(np.float64)
    tree = cKDTree(P)
    q0 = pts.astype(np.float64)
    T = np.eye(4)
    log = []
    for _ in range(iterations):
        q = q0 @ T[:3, :3].T + T[:3, 3]
        d, w = tree.query(q, k=1, distance_upper_bound=max_dist)
        ok = np.isfinite(d)
        if nrm is not None and min_normal_cos > -1:
            m = nrm.astype(np.float64) @ T[:3, :3].T
            ok &= (m * N[np.where(ok, w, 0)]).sum(1) >= min_normal_cos
        q, n = q[ok], N[w[ok]]
        r = ((q - P[w[ok]]) * n).sum(1)
        J = np.concatenate([n, np.cross(q, n)], 1)
        xi = np.linalg.solve(J.T @ J, -(J.T @ r))
        T = expm(twist_matrix(xi)) @ T
        log.append((int(ok.sum()), float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:]))))
    return T, log


# The allowance for the f32 transform of the points, on top of the float64 restatement's own error: ALLOW_C * 2^-24 * max |coordinate| metres
# (per radian: divided by the scene's extent).  The device sees the pose only through its f32 rounding (Rf, tf) and rounds p' four times per
# coordinate, each by at most 2^-24 of a coordinate: one unit is the error a single such rounding can cause, and the 50 000 points average
# most of it out.  Measured on the MI355X (profiles/r13_register_accuracy.txt): 0.21 / 0.20 units in translation, 0.14 / 0.20 in rotation
# (without / with normals).  One unit keeps the bar within an order of magnitude of that and still an order below a defect of one f32 ulp
# per point that does not average out.
ALLOW_C = 1.0


@pytest.mark.parametrize("normals", [False, True])
def test_it_recovers_the_motion(world, normals):
    from elasticfusion_amd import api
    ef, S, pts, G = world["ef"], world["S"], world["pts"], world["G"]
    nrm = world["nrm"] if normals else None
    cos = 0.5 if normals else -1.0
    T, res = ef.registerCloud(pts, nrm, max_dist=0.05, min_conf=-1.0, min_normal_cos=cos, max_iterations=6)
    T64, log = icp_float64(S, pts, nrm, res["iterations"], 0.05, cos)
    et, er = pose_error(T, G)
    et64, er64 = pose_error(T64, G)
    big = float(np.abs(S[:, :3]).max())
    extent = float(np.linalg.norm(S[:, :3].max(0) - S[:, :3].min(0)))
    unit_t, unit_r = 2.0 ** -24 * big, 2.0 ** -24 * big / extent
    print(f"normals {normals}: status {res['status_name']} iterations {res['iterations']} pairs {res['pairs']} rms {res['rms_first']:.3e} -> {res['rms_last']:.3e}")
    print(f"  float64 restatement: per iteration (pairs, |xi_t|, |xi_w|) {log}")
    print(f"  pose error  device {et:.3e} m {er:.3e} rad   float64 restatement {et64:.3e} m {er64:.3e} rad")
    print(f"  max |coordinate| {big:.3f} m, extent {extent:.3f} m: 2^-24 units {unit_t:.3e} m {unit_r:.3e} rad; "
          f"device error in units {(et - et64) / unit_t:.2f} {(er - er64) / unit_r:.2f}; allowance c = {ALLOW_C}")
    assert res["status"] == api.REG_CONVERGED
    assert res["rms_last"] < res["rms_first"]
    assert res["pairs"] > 49000
    assert et <= et64 + ALLOW_C * unit_t, (et, et64, unit_t)
    assert er <= er64 + ALLOW_C * unit_r, (er, er64, unit_r)


def test_a_cloud_out_of_reach_is_too_few_pairs(world):
    from elasticfusion_amd import api
    ef, pts = world["ef"], world["pts"]
    T0 = np.eye(4)
    T0[:3, 3] = (40.0, -30.0, 25.0)   # further than max_dist from every surfel
    T, res = ef.registerCloud(pts, world["nrm"], T_init=T0, max_dist=0.05, min_conf=-1.0)
    assert res["status"] == api.REG_TOO_FEW_PAIRS and res["iterations"] == 0 and res["pairs"] == 0
    assert_bits_equal(T, T0, "pose")


# What aligning may cost on a reconstructed map, relative to the unmoved ground truth without alignment (profiles/r13_register_accuracy.txt has
# both sets of figures and the reasoning): ICP moves the ground truth onto the map's own drift, so the plane figures do not get worse; the
# margins cover the change of partners at max_dist's edge.
ALIGN_MISS_MARGIN = 0.005    # absolute, on a share
ALIGN_PLANE_MARGIN = 1.10    # factor on plane_rms


def test_alignment_on_a_reconstructed_map(seq):
    from scipy.linalg import expm
    from elasticfusion_amd import accuracy, api, synth
    ef = api.ElasticFusion()
    try:
        for k in range(60):
            rgb, depth, _ = seq.frame(k)
            ef.processFrame(rgb, depth, k)
        gt = synth.sample_surfels(seq, n=1 << 18)
        base = accuracy.map_accuracy(ef, gt, max_dist=0.05)
        G = expm(twist_matrix(TWIST))
        moved = accuracy.move_surfels(gt, np.linalg.inv(G))
        rep = accuracy.map_accuracy(ef, moved, max_dist=0.05, align=True)
        same = accuracy.map_accuracy(ef, gt, max_dist=0.05, align=False)
    finally:
        ef.close()
    print("unmoved ground truth, no alignment:\n" + accuracy.format_report(base))
    print("ground truth moved by the inverse of the twist", TWIST.tolist(), "then aligned:\n" + accuracy.format_report(rep))
    T = np.asarray(rep["align"]["T"])
    et, er = pose_error(T, G)
    print(f"recovered motion against the generating one: {et:.3e} m, {er:.3e} rad (no bar: it lawfully absorbs the map's drift)")
    for st in rep["align"]["stages"]:
        print("  stage", st["max_dist"], st["status_name"], st["iterations"], st["pairs"], st["rms_first"], st["rms_last"])
    assert "align" not in base and json.dumps(base) == json.dumps(same)
    assert rep["align"]["stages"][-1]["status"] in (api.REG_CONVERGED, api.REG_MAX_ITERATIONS) and len(rep["align"]["stages"]) == 3
    for side in ("accuracy", "completeness"):
        a, b = rep[side], base[side]
        print(side, "miss share", b["miss_share"], "->", a["miss_share"], " plane rms", b["plane_rms"], "->", a["plane_rms"])
        assert a["points"] == b["points"]
        assert a["miss_share"] <= b["miss_share"] + ALIGN_MISS_MARGIN, (side, a["miss_share"], b["miss_share"])
        assert a["plane_rms"] <= b["plane_rms"] * ALIGN_PLANE_MARGIN, (side, a["plane_rms"], b["plane_rms"])


def _run_sequence(frames, with_registration):
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(-2, 2, (1024, 3)), [[np.nan, 0, 0]]]).astype(F)
    nrm = rng.normal(0, 1, pts.shape).astype(F)
    n = len(pts)
    dpts, dnrm = api.DevBuf.from_array(pts), api.DevBuf.from_array(nrm)
    drow, dpl = api.DevBuf(n * 4), api.DevBuf(n * 4)
    pairs = 0
    for k, (rgb, depth, _) in enumerate(frames):
        ef.processFrame(rgb, depth, k)
        if with_registration and k + 1 < len(frames):
            if k % 2 == 0:
                s = ef.registerStepDevice(dpts.p, n, normals_dev=dnrm.p, row=drow.p, plane=dpl.p, max_dist=0.1, min_conf=-1.0, min_normal_cos=0.0)
                pairs += s["pairs"]
                ef.registerCloudDevice(dpts.p, n, max_dist=0.1, min_conf=-1.0, max_iterations=3, row=drow.p)
            else:
                pairs += ef.registerStep(pts, nrm, max_dist=0.1, min_conf=-1.0)["pairs"]
                ef.registerCloud(pts, None, max_dist=0.1, min_conf=float(ef.cfg.confidence), max_iterations=2, pairs=True)
    ef.synchronize()
    res = dict(traj=ef.trajectory()[0], pose=ef.get_T_wc(), map=ef.downloadMap(), count=ef.lastCount(), pairs=pairs)
    ef.close()
    return res


def test_registration_changes_nothing(seq):
    frames = [seq.frame(k) for k in range(40)]
    a = _run_sequence(frames, False)
    b = _run_sequence(frames, True)
    assert a["count"] == b["count"] > 0
    assert_bits_equal(a["traj"].astype(np.float64), b["traj"].astype(np.float64), "trajectory")
    assert_bits_equal(a["pose"], b["pose"], "pose")
    assert_bits_equal(a["map"], b["map"], "downloadMap")
    assert b["pairs"] > 0


def test_device_variants_equal_host_and_capture_is_refused(world):
    from elasticfusion_amd import api
    ef, pts, nrm = world["ef"], world["pts"][:8192], world["nrm"][:8192]
    n = len(pts)
    dpts, dnrm = api.DevBuf.from_array(pts), api.DevBuf.from_array(nrm)
    drow, dpl = api.DevBuf(n * 4, fill=0x55), api.DevBuf(n * 4, fill=0x55)
    for normals, dn, cos in ((None, None, -1.0), (nrm, dnrm.p, 0.5)):
        host = ef.registerStep(pts, normals, pairs=True, max_dist=0.05, min_conf=-1.0, min_normal_cos=cos)
        dev = ef.registerStepDevice(dpts.p, n, normals_dev=dn, row=drow.p, plane=dpl.p, max_dist=0.05, min_conf=-1.0, min_normal_cos=cos)
        for key in ("A", "b"):
            assert_bits_equal(dev[key], host[key], "step " + key)
        assert dev["e"] == host["e"] and dev["pairs"] == host["pairs"] > 0 and dev["points"] == n
        assert_bits_equal(drow.to_array(np.uint32, n), host["row"], "step rows")
        assert_bits_equal(dpl.to_array(np.float32, n), host["plane"], "step plane")
        T, res = ef.registerCloud(pts, normals, pairs=True, max_dist=0.05, min_conf=-1.0, min_normal_cos=cos, max_iterations=4)
        Td, resd = ef.registerCloudDevice(dpts.p, n, normals_dev=dn, row=drow.p, plane=dpl.p, max_dist=0.05, min_conf=-1.0, min_normal_cos=cos,
                                          max_iterations=4)
        assert_bits_equal(Td, T, "cloud pose")
        for key in ("status", "iterations", "pairs", "rms_first", "rms_last"):
            assert resd[key] == res[key], (key, resd[key], res[key])
        assert_bits_equal(resd["A"], res["A"], "cloud A")
        assert_bits_equal(drow.to_array(np.uint32, n), res["row"], "cloud rows")
        assert_bits_equal(dpl.to_array(np.float32, n), res["plane"], "cloud plane")
    # NULL optional outputs
    ef.registerStepDevice(dpts.p, n, max_dist=0.05, min_conf=-1.0)
    ef.registerCloudDevice(dpts.p, n, max_dist=0.05, min_conf=-1.0, max_iterations=1)
    import ctypes.util
    name = ctypes.util.find_library("amdhip64") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")
    hip = C.CDLL(name)
    s = C.c_void_p(ef.stream())
    ef.synchronize()
    assert hip.hipStreamBeginCapture(s, C.c_int(2)) == 0   # relaxed
    try:
        with pytest.raises(api.EFError, match="error -4"):
            ef.registerStepDevice(dpts.p, n, max_dist=0.05, min_conf=-1.0)
        with pytest.raises(api.EFError, match="error -4"):
            ef.registerCloudDevice(dpts.p, n, max_dist=0.05, min_conf=-1.0)
        with pytest.raises(api.EFError, match="error -4"):
            ef.registerStep(pts, max_dist=0.05, min_conf=-1.0)
        with pytest.raises(api.EFError, match="error -4"):
            ef.registerCloud(pts, max_dist=0.05, min_conf=-1.0)
        with pytest.raises(api.EFError, match="error -4"):
            ef.registerCloud(np.zeros((0, 3), F), max_dist=0.05, min_conf=-1.0)
    finally:
        g = C.c_void_p()
        assert hip.hipStreamEndCapture(s, C.byref(g)) == 0
        if g.value:
            hip.hipGraphDestroy(g)
    ef.synchronize()
    again = ef.registerStep(pts, None, max_dist=0.05, min_conf=-1.0)
    assert_bits_equal(again["A"], ef.registerStep(pts, nrm, max_dist=0.05, min_conf=-1.0, min_normal_cos=-1.0)["A"], "usable afterwards")
