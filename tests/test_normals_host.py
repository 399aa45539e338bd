"""CPU-only checks of the normal estimation (ef_map_normals / ef_map_normals_select / ef_map_reestimate_normals, include/ef_hip.h; DESIGN.md
§8l): the hand-built scenes contain the edges they claim, shown on the numpy reference (tests/normalref.py, written from the header alone); the
definition estimates normals (against numpy.linalg.eigh and the true normals of a sphere); normal_fit of csrc/ef_plane_fit.hpp compiled by the
host compiler into a stand-alone program (tests/normal_fit_main.cpp; once more with the address and undefined-behaviour sanitizers) equals the
reference bit for bit; every EF_EINVAL of the header through the C ABI without a device; the binding."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import normalref as nr
import normalscenes as sc
import outlierref as oref
from test_api_binding_host import defines, header_structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
THR = 10.0           # a context's default confidence threshold (the GPU tests read it from the context and assert the scenes straddle it)


@pytest.fixture(scope="module")
def edge():
    S, marks = sc.edge_scene()
    nl = {mc: nr.neighbour_lists(S, sc.R_EDGE, mc) for mc in (-1.0, THR)}
    refs = {(k, mc): nr.estimate(S, nl=nl[mc], radius=sc.R_EDGE, min_conf=mc, k=k, min_neighbors=sc.MIN_NEIGHBORS[k]) for k in sc.KS for mc in nl}
    return dict(S=S, marks=marks, nl=nl, refs=refs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the scenes contain the edges they claim
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_neighbour_lists_are_the_outlier_references(edge):
    for mc, (count, D, R) in edge["nl"].items():
        c0, D0 = oref.neighbours(edge["S"], sc.R_EDGE, mc)
        assert np.array_equal(count, c0) and nr.same_bits(D, D0)
        have = np.arange(16)[None, :] < np.minimum(count, 16)[:, None]
        assert ((R >= 0) == have).all() and (R[have] != np.nonzero(have)[0]).all()          # self is excluded by row


def test_counts_at_and_below_min_neighbors(edge):
    m, (count, D, R) = edge["marks"], edge["nl"][-1.0]
    assert (count[m["exact"]] == 5).all() and (count[m["fewer"]] == 4).all()
    ref = edge["refs"][(5, -1.0)]
    assert (ref["status"][m["exact"]] == nr.ESTIMATED).all() and (ref["status"][m["fewer"]] == nr.SPARSE).all()
    assert np.isfinite(ref["spacing"][m["fewer"]]).all() and (ref["normals"][m["fewer"]] == 0).all()       # a sparse row still has its spacing
    assert (edge["refs"][(4, -1.0)]["status"][m["fewer"]] == nr.ESTIMATED).all()                           # min_neighbors 3: the same rows fit


def test_ties_at_rank_k_are_decided_by_the_row(edge):
    m, (count, D, R) = edge["marks"], edge["nl"][-1.0]
    c = m["centre"]
    assert count[c] == 48
    for k in sc.TIE_KS:
        j = min(k, 15)                                           # (k = 16: ranks 13 .. 20 tie; the list holds the first sixteen)
        assert D[c, j - 1] == D[c, j] and R[c, j - 1] < R[c, j], k
    # ... and who is used matters: swapping the last used neighbour for its tied twin changes the estimate
    k = 5
    ref = edge["refs"][(k, -1.0)]
    R2 = R.copy()
    R2[c, k - 1] = R[c, k]
    other = nr.normal_fit(nr.moments(edge["S"], count, R2, k)[c], k + 1, edge["S"][c, 8:11], 1e-4)
    assert ref["status"][c] == nr.ESTIMATED and other[0] == nr.ESTIMATED and not nr.same_bits(other[1], ref["normals"][c])
    for k in (4, 8):
        assert D[c, k - 1] < D[c, k]


def test_duplicates_lines_points_and_triangles(edge):
    m, (count, D, R) = edge["marks"], edge["nl"][-1.0]
    a, b = m["pair"]
    assert D[a, 0] == 0 and R[a, 0] == b and D[b, 0] == 0 and R[b, 0] == a                  # coincident rows are neighbours at d2 = 0
    for k in sc.KS:
        ref = edge["refs"][(k, -1.0)]
        assert (ref["status"][m["pair"]] == nr.ESTIMATED).all()
        for g in ("line", "slant", "point"):
            assert (count[m[g]] >= 5).all() and (ref["status"][m[g]] == nr.DEGENERATE).all(), (k, g)
            assert (ref["normals"][m[g]] == 0).all() and (ref["curvature"][m[g]] == 0).all()
        assert (ref["spacing"][m["point"]] == 0).all()
    tri = edge["refs"][(3, -1.0)]                                                           # min_neighbors 2: three points are a plane
    assert (count[m["triangle"]] == 2).all() and (tri["status"][m["triangle"]] == nr.ESTIMATED).all()
    assert (tri["curvature"][m["triangle"]] <= 1e-12).all(), tri["curvature"][m["triangle"]]           # thickness 0
    assert (edge["refs"][(4, -1.0)]["status"][m["triangle"]] == nr.SPARSE).all()


def test_non_finite_rows_take_no_part(edge):
    m = edge["marks"]
    for ref in edge["refs"].values():
        bad = m["bad"]
        assert (ref["status"][bad] == nr.NONE).all() and (ref["count"][bad] == 0).all() and np.isposinf(ref["spacing"][bad]).all()
        assert (ref["normals"][bad] == 0).all() and ref["result"]["participants"] == len(edge["S"]) - len(bad)


def test_keep_side_flips_nothing_on_a_perpendicular_zero_or_nan_normal(edge):
    m, ref = edge["marks"], edge["refs"][(8, -1.0)]
    for g in ("perp", "zero", "nan"):
        assert (ref["status"][m[g]] == nr.ESTIMATED).all() and not ref["flipped"][m[g]].any(), g
        assert nr.same_bits(ref["normals"][m[g]], np.tile(np.array([0, 0, 1], F), (3, 1))), g      # the plane z = 1: exactly +z, unturned
    assert ref["flipped"][m["down"]].all() and nr.same_bits(ref["normals"][m["down"]], np.tile(np.array([-0.0, -0.0, -1], F), (3, 1)))
    assert (ref["curvature"][m["plane"]] == 0).all()
    est = ref["status"] == nr.ESTIMATED
    assert 100 < ref["flipped"][est].sum() < est.sum() - 100                                       # random stored normals: both sides occur


def test_viewpoint_orientation_and_a_surfel_at_the_viewpoint(edge):
    S, m = edge["S"], edge["marks"]
    v = S[m["at_view"], :3]
    keep = edge["refs"][(8, -1.0)]
    refs = {side: nr.estimate(S, nl=edge["nl"][-1.0], radius=sc.R_EDGE, k=8, orientation=nr.VIEWPOINT, side=side, viewpoint=v) for side in (1, -1)}
    assert keep["status"][m["at_view"]] == nr.ESTIMATED
    for side, ref in refs.items():
        assert np.array_equal(ref["status"], keep["status"]) and nr.same_bits(ref["curvature"], keep["curvature"])
        assert not ref["flipped"][m["at_view"]]                                                    # hn = 0 there: nothing is turned
        est = (ref["status"] == nr.ESTIMATED) & (np.arange(len(S)) != m["at_view"])
        d = ((v[None, :] - S[est, :3]).astype(np.float64) * ref["normals"][est]).sum(1)
        assert (side * d >= 0).all()
    a, b = refs[1]["normals"], refs[-1]["normals"]
    assert nr.same_bits(a[est], -b[est]) and nr.same_bits(a[m["at_view"]], b[m["at_view"]])           # the two sides are each other's negation
    assert refs[1]["result"]["flipped"] + refs[-1]["result"]["flipped"] == est.sum()


def test_min_conf_excludes_low_rows_as_neighbours_only(edge):
    S, m = edge["S"], edge["marks"]
    low = m["low"]
    assert 40 < len(low) < 120 and (S[low, 3] < THR).all() and (np.delete(S[:, 3], low) > THR).all()
    all_, stable = edge["nl"][-1.0], edge["nl"][THR]
    assert (stable[0] <= all_[0]).all() and (stable[0][m["cloud"]] < all_[0][m["cloud"]]).any()
    assert not np.isin(stable[2][stable[2] >= 0], low).any() and np.isin(all_[2], low).any()
    ref = edge["refs"][(8, THR)]
    assert (ref["status"][low] != nr.NONE).all() and (ref["status"][low] == nr.ESTIMATED).any()       # a low row is still judged
    assert not nr.same_bits(ref["normals"], edge["refs"][(8, -1.0)]["normals"])


def test_every_k_uses_its_own_neighbourhood(edge):
    seen = [edge["refs"][(k, -1.0)]["normals"][edge["marks"]["cloud"]] for k in sc.KS]
    for a, b in zip(seen, seen[1:]):
        assert not nr.same_bits(a, b)
    count, D, R = edge["nl"][-1.0]
    for k in sc.KS:
        ref = edge["refs"][(k, -1.0)]
        full = count >= k
        assert full.sum() > 200 and nr.same_bits(ref["spacing"][full], oref.mean_dist(count, D, k)[full])    # spacing = the outliers' mean there
        short = ref["part"] & (count < k) & (count > 0)
        assert short.any() and np.isfinite(ref["spacing"][short]).all()


def test_lists_and_the_write_back_of_the_reference(edge):
    S = edge["S"]
    ref = nr.estimate(S, nl=edge["nl"][-1.0], radius=sc.R_EDGE, k=8, max_curvature=0.01, set_radius=1, radius_scale=0.75)
    rows = {w: nr.listed(ref, w) for w in (nr.ESTIMATED, nr.SPARSE, nr.DEGENERATE, nr.CURVED, nr.FLAT)}
    assert all(len(r) > 5 for r in rows.values())
    assert np.array_equal(np.sort(np.concatenate([rows[nr.CURVED], rows[nr.FLAT]])), rows[nr.ESTIMATED])
    assert len(rows[nr.ESTIMATED]) + len(rows[nr.SPARSE]) + len(rows[nr.DEGENERATE]) == ref["result"]["participants"]
    W = nr.written(S, ref)
    est = ref["status"] == nr.ESTIMATED
    assert nr.same_bits(W[~est], S[~est]) and nr.same_bits(W[:, :8], S[:, :8])
    assert nr.same_bits(W[est, 11], (F(0.75) * ref["spacing"][est]).astype(F)) and not nr.same_bits(W[est, 8:11], S[est, 8:11])
    # KEEP_SIDE is idempotent: the estimate agrees with its own sign
    again = nr.estimate(W, nl=edge["nl"][-1.0], radius=sc.R_EDGE, k=8, set_radius=1, radius_scale=0.75)
    assert nr.same_bits(nr.written(W, again), W) and not again["flipped"][est & ~ref["flipped"]].any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the definition estimates normals
# ---------------------------------------------------------------------------------------------------------------------------------------
# (noise, shift) -> the reference's own (median, 99th percentile, maximum) angle in degrees to the true radial direction on the committed seed
SPHERE_MEASURED = {(0.0, (0.0, 0.0, 0.0)): (1.117, 3.822, 6.145), (0.001, (0.0, 0.0, 0.0)): (1.442, 4.524, 6.162), (0.0, sc.SHIFT): (1.116, 3.833, 6.155)}


@pytest.mark.parametrize("noise, shift", list(SPHERE_MEASURED), ids=("sphere", "noise-1mm", "shifted"))
def test_the_definition_estimates_the_normals_of_a_sphere(noise, shift):
    S, radial = sc.sphere_scene(noise=noise, shift=shift)
    nl = nr.neighbour_lists(S, sc.R_SPHERE)
    ref = nr.estimate(S, nl=nl, radius=sc.R_SPHERE, k=12)
    assert (ref["status"] == nr.ESTIMATED).all() and ref["result"]["estimated"] == 2048
    assert not ref["flipped"].any() or (ref["normals"].astype(np.float64) * radial).sum(1).min() > 0      # KEEP_SIDE: the stored side, outward
    M = nr.moments(S, nl[0], nl[2], 12)
    m = (np.minimum(nl[0], 12) + 1).astype(np.float64)
    mean = M[:, :3] / m[:, None]
    Cm = np.empty((len(S), 3, 3))
    for (i, j), col in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(3, 9)):
        Cm[:, i, j] = Cm[:, j, i] = M[:, col] / m - mean[:, i] * mean[:, j]
    w, v = np.linalg.eigh(Cm)
    gap = (w[:, 1] - w[:, 0]) >= 1e-3 * w[:, 2]
    n = ref["normals"].astype(np.float64)
    sin = np.linalg.norm(np.cross(n, v[:, :, 0]), axis=1)
    print(f"gap condition on {gap.mean():.4f} of the rows; worst |sin| against eigh {sin[gap].max():.3g}")
    assert gap.mean() >= 0.99
    # the f32 rounding of the output: at most sqrt(3) * 2^-24 = 1.03e-7
    assert sin[gap].max() <= 2e-7
    with np.errstate(invalid="ignore"):
        assert (np.abs(np.linalg.norm(n, axis=1) - 1.0) <= 2e-7).all() and ((ref["curvature"] >= 0) & (ref["curvature"] <= F(1 / 3))).all()
    ang = np.degrees(np.arcsin(np.clip(np.linalg.norm(np.cross(n, radial), axis=1), 0, 1)))
    got = (float(np.median(ang)), float(np.percentile(ang, 99)), float(ang.max()))
    print("angle to the radial direction: median %.3f, 99th percentile %.3f, max %.3f degrees" % got)
    # the bars: the reference's own figures on this seed (SPHERE_MEASURED) times 1.5
    for g, measured in zip(got, SPHERE_MEASURED[(noise, shift)]):
        assert g <= 1.5 * measured, (got, SPHERE_MEASURED[(noise, shift)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# normal_fit of ef_plane_fit.hpp on the host
# ---------------------------------------------------------------------------------------------------------------------------------------
def fit_cases(edge):
    """(m, hn, line_ratio, S): the moments of every fitted row of the edge scene at two k, random blobs at several scales, degenerate sets"""
    cases = []
    S, (count, D, R) = edge["S"], edge["nl"][-1.0]
    for k in (5, 16):
        M = nr.moments(S, count, R, k)
        for s in np.nonzero(nr.participants(S) & (count >= 2))[0]:
            cases.append((int(min(count[s], k)) + 1, S[s, 8:11], 1e-4, M[s]))
    rng = np.random.default_rng(3)
    for i in range(40):
        q = rng.normal(size=(int(rng.integers(2, 17)), 3)) * 10.0 ** rng.uniform(-4, 2) * rng.uniform(0.01, 1.0, 3)
        x, y, z = q.T
        Sm = [t.sum() for t in (x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)]
        cases.append((len(q) + 1, rng.normal(size=3).astype(F), [0.0, 1e-4, 0.5, 1.0][i % 4], Sm))
    hn, z = np.array([0, 0, 1], F), [0.0] * 9
    cases += [(5, hn, 1e-4, z),                                                       # a repeated point: C = 0
              (4, hn, 1e-4, [2.0, 0.0, 0.0, 2.0, 0, 0, 0, 0, 0]),                     # collinear along x
              (4, hn, 0.0, [0.0, 0, 0, 4.0, 0, 0, 4.0, 0, 0.0]),                      # a plane at line_ratio 0: emid > 0
              (4, hn, 0.0, [0.0, 0, 0, 4.0, 0, 0, 0.0, 0, 0.0]),                      # a line at line_ratio 0: !(0 > 0)
              (4, hn, 1e-4, [0.0, 0, 0, 4.0, 0, 0, 4.0, 0, 4.0]),                     # isotropic: curvature 1 / 3, ties to the lowest index
              (4, -hn, 1e-4, [0.0, 0, 0, 4.0, 0, 0, 4.0, 0, 1.0]),                    # already diagonal, turned
              (4, np.array([1, 1, 0], F), 1e-4, [0.0, 0, 0, 4.0, 0, 0, 4.0, 0, 1.0]), # a perpendicular hint
              (4, np.array([np.nan, 0, 0], F), 1e-4, [0.0, 0, 0, 4.0, 0, 0, 4.0, 0, 1.0]),
              (4, hn, 1e-4, [0.0, 0, 0, 1e300, 1e300, 0, 1e300, 0, 1e300]),           # huge but finite
              (4, hn, 1e-4, [0.0, 0, 0, 1e-300, 1e-301, 0, 1e-300, 0, 1e-300]),       # tiny
              (4, hn, 1e-4, [1e200, 0, 0, 1.0, 0, 0, 1.0, 0, 1.0]),                   # mean^2 overflows: gives up
              (4, hn, 1e-4, [np.nan, 0, 0, 1.0, 0, 0, 1.0, 0, 1.0]), (4, hn, 1e-4, [0.0, 0, 0, np.inf, 0, 0, 1.0, 0, 1.0]),
              (2, hn, 1e-4, [0.0, 0, 0, 4.0, 0, 0, 4.0, 0, 1.0]),                     # fewer than three members
              (4, hn, 1e-4, [0.0, 0, 0, -1.0, 0, 0, 4.0, 0, 1.0])]                    # a negative "variance": clamped to 0
    return cases


@pytest.mark.parametrize("sanitized", (False, True), ids=("plain", "asan+ubsan"))
def test_the_fit_compiled_for_the_host_equals_the_reference_bit_for_bit(tmp_path, edge, sanitized):
    src = os.path.join(ROOT, "tests", "normal_fit_main.cpp")
    cmd = ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "elasticfusion_amd", "csrc")]
    if sanitized:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        trial = tmp_path / "trial.cpp"
        trial.write_text("int main() { return 0; }\n")
        ok = subprocess.run(cmd + [str(trial), "-o", str(tmp_path / "trial")], capture_output=True).returncode == 0
        if not (ok and subprocess.run([str(tmp_path / "trial")], capture_output=True).returncode == 0):
            cmd = cmd[:-2]
            print("sanitizers: not available, plain build")
    exe = tmp_path / "normal_fit"
    subprocess.run(cmd + [src, "-o", str(exe)], check=True)
    cases = fit_cases(edge)
    bits32 = lambda v: "%08x" % struct.unpack("<I", struct.pack("<f", float(v)))[0]
    bits64 = lambda v: "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    text = "".join(" ".join([str(m)] + [bits32(v) for v in hn] + [bits32(lr)] + [bits64(v) for v in S]) + "\n" for m, hn, lr, S in cases)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases) > 900
    seen = {nr.ESTIMATED: 0, nr.DEGENERATE: 0, "gave up": 0, "flipped": 0}
    for i, ((m, hn, lr, S), line) in enumerate(zip(cases, lines)):
        w = line.split()
        status, normal, curv, flipped, l = nr.normal_fit(S, m, hn, lr)
        # the program's status: 0 gave up, 1 estimated, 2 degenerate; the header's verdict for the first and the last is DEGENERATE
        assert int(w[0]) == (1 if status == nr.ESTIMATED else 0 if l is None else 2), (i, line, status, l)
        want = [bits32(v) for v in normal] + [bits32(curv), str(int(flipped))] + [bits64(v) for v in (l or (0.0, 0.0, 0.0))]
        assert w[1:] == want, (i, line, want)
        seen["gave up" if l is None else status] += 1
        seen["flipped"] += int(flipped)
    print(seen)
    assert seen[nr.ESTIMATED] > 800 and seen[nr.DEGENERATE] > 40 and seen["gave up"] == 4 and seen["flipped"] > 200


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C ABI's refusals and the binding
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    return api.lib()


def good_params(**kw):
    from elasticfusion_amd import api
    p = api.ef_normal_params(radius=0.03, cell=0.03, min_conf=-1.0, k=12, min_neighbors=5, orientation=0, side=-1, viewpoint=(C.c_float * 3)(0, 0, 0),
                             line_ratio=1e-4, max_curvature=0.05, set_radius=0, radius_scale=1.0)
    for k, v in kw.items():
        setattr(p, k, (C.c_float * 3)(*v) if k == "viewpoint" else v)
    return p


NAN, INF = float("nan"), float("inf")
BAD = [(dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=NAN), "radius"), (dict(radius=INF), "radius"),
       (dict(cell=0.0), "cell"), (dict(cell=NAN), "cell"), (dict(cell=INF), "cell"), (dict(cell=1e-45), "cell"),
       (dict(radius=1.0, cell=0.01), "radius / cell"), (dict(min_conf=NAN), "min_conf"),
       (dict(k=2, min_neighbors=2), "k must"), (dict(k=17), "k must"), (dict(k=0), "k must"),
       (dict(min_neighbors=1), "min_neighbors"), (dict(min_neighbors=13), "min_neighbors"), (dict(k=3, min_neighbors=4), "min_neighbors"),
       (dict(orientation=2), "orientation"), (dict(orientation=-1), "orientation"), (dict(side=0), "side"), (dict(side=2), "side"),
       (dict(orientation=1, viewpoint=(NAN, 0, 0)), "viewpoint"), (dict(orientation=1, viewpoint=(0, INF, 0)), "viewpoint"),
       (dict(line_ratio=NAN), "line_ratio"), (dict(line_ratio=-1e-6), "line_ratio"), (dict(max_curvature=NAN), "max_curvature"),
       (dict(max_curvature=-0.1), "max_curvature"), (dict(radius_scale=NAN), "radius_scale"), (dict(radius_scale=-1.0), "radius_scale")]


def test_every_refusal_names_its_argument_with_a_null_context(lib):
    from elasticfusion_amd import api
    EINVAL = -1
    res, cnt, rows = api.ef_normal_result(), C.c_uint32(0), (C.c_uint32 * 4)()
    calls = {
        "ef_map_normals": lambda p, a: lib.ef_map_normals(None, p, a, None, None, None, None, None, 0),
        "ef_map_normals_dev": lambda p, a: lib.ef_map_normals_dev(None, p, a, None, None, None, None, None, 0),
        "ef_map_normals_select": lambda p, a: lib.ef_map_normals_select(None, p, a, api.NORMAL_ESTIMATED, rows, 4, C.byref(cnt), None),
        "ef_map_normals_select_dev": lambda p, a: lib.ef_map_normals_select_dev(None, p, a, api.NORMALS_FLAT, rows, 4, C.byref(cnt), None),
        "ef_map_reestimate_normals": lambda p, a: lib.ef_map_reestimate_normals(None, p, a, C.byref(res)),
    }

    def refused(rc, fn, word):
        msg = lib.ef_last_error(None).decode()
        assert rc == EINVAL and msg.startswith(fn + ":") and word in msg, (fn, word, rc, msg)

    for fn, call in calls.items():
        refused(call(None, None), fn, "null params")
        for change, word in BAD:
            refused(call(C.byref(good_params(**change)), None), fn, word)
        refused(call(C.byref(good_params(viewpoint=(NAN, 0, 0))), None), fn, "null context")           # the viewpoint is not looked at in KEEP_SIDE mode
        refused(call(C.byref(good_params(k=3, min_neighbors=2, line_ratio=0.0, max_curvature=0.0, radius_scale=0.0)), None), fn, "null context")
        refused(call(C.byref(good_params(k=16, min_neighbors=16, orientation=1, side=1, radius=0.16, cell=0.01)), None), fn, "null context")   # the limits themselves
        sel = api.ef_map_selection()
        lib.ef_default_map_selection(C.byref(sel))
        sel.tests = 0x8000
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "unknown bits")                        # what ef_map_select refuses
        sel.tests, sel.conf_min = api.SEL_CONF, NAN
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "NaN")
    p = C.byref(good_params())
    for fn in ("ef_map_normals_select", "ef_map_normals_select_dev"):
        call = getattr(lib, fn)
        for what in (0, 6, -1, -5):
            refused(call(None, p, None, what, rows, 4, C.byref(cnt), None), fn, "what")
        for what in (1, 2, 3, 4, 5):
            refused(call(None, p, None, what, rows, 4, C.byref(cnt), None), fn, "null context")
        refused(call(None, p, None, 1, None, 4, C.byref(cnt), None), fn, "null rows")
        refused(call(None, p, None, 1, rows, 4, None, None), fn, "null count")
        refused(call(None, p, None, 1, None, 0, C.byref(cnt), None), fn, "null context")               # NULL rows with max_rows 0 is fine
    refused(lib.ef_map_reestimate_normals(None, p, None, None), "ef_map_reestimate_normals", "null result")
    assert lib.ef_default_normal_params(None, C.byref(good_params())) == EINVAL and b"null context" in lib.ef_last_error(None)


def test_the_new_structs_and_constants_are_the_headers():
    from elasticfusion_amd import accuracy, api
    structs = header_structs()
    for name in ("ef_normal_params", "ef_normal_result"):
        assert structs[name] == [f for f, _ in getattr(api, name)._fields_]
    assert C.sizeof(api.ef_normal_params) == 56 and C.sizeof(api.ef_normal_result) == 24 and api.ef_normal_params.viewpoint.offset == 28
    want = defines("NORMAL")
    mine = {k: v for k, v in vars(api).items() if k.startswith("NORMAL") and isinstance(v, int)}
    assert want == dict(NORMALS_KEEP_SIDE=0, NORMALS_VIEWPOINT=1, NORMAL_NONE=0, NORMAL_ESTIMATED=1, NORMAL_SPARSE=2, NORMAL_DEGENERATE=3,
                        NORMALS_CURVED=4, NORMALS_FLAT=5) and mine == want, (mine, want)
    assert (nr.KEEP_SIDE, nr.VIEWPOINT, nr.NONE, nr.ESTIMATED, nr.SPARSE, nr.DEGENERATE, nr.CURVED, nr.FLAT) == (
        api.NORMALS_KEEP_SIDE, api.NORMALS_VIEWPOINT, api.NORMAL_NONE, api.NORMAL_ESTIMATED, api.NORMAL_SPARSE, api.NORMAL_DEGENERATE,
        api.NORMALS_CURVED, api.NORMALS_FLAT)
    for name in ("normalParams", "estimateNormals", "estimateNormalsDevice", "normalSelect", "normalSelectDevice", "reestimateNormals"):
        assert callable(getattr(api.ElasticFusion, name))
    assert callable(accuracy.estimated_normals) and callable(accuracy.insert_cloud)
    src = open(os.path.join(ROOT, "elasticfusion_amd", "csrc", "ef_plane_fit.hpp")).read()
    assert "EF_PLANE_FIT_SWEEPS = %d;" % nr.SWEEPS in src and "normal_fit(" in src
