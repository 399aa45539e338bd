"""CPU-only checks around the map's plane segmentation (include/ef_hip.h, "Segment the map into planes"): the numpy restatement
(tests/planeref.py) on cases whose answers are worked out by hand, that the scenes of tests/test_gpu_planes.py contain the edges they claim,
csrc/ef_plane_fit.hpp compiled by the host compiler into a stand-alone program (tests/plane_fit_main.cpp; once more with the address and
undefined-behaviour sanitizers where the compiler has their runtimes) against planeref bit for bit, its eigenvector against numpy.linalg.eigh,
every EF_EINVAL with a NULL context, and the binding of the three new structs and the constants."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import planeref as pr
import planescenes as sc
from test_api_binding_host import defines, header_structs

F = np.float32
NONE = pr.NONE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference by hand
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_hash_and_the_samples_by_hand():
    def h32(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        x ^= x >> 16
        return x
    assert int(pr.h32(0)) == 0 and all(int(pr.h32(v)) == h32(v) for v in (1, 0x9E3779B9, 0xFFFFFFFF, 12345))
    for seed, k, M in ((0, 0, 1), (12345, 0, 3100), (0xFFFFFFFF, 15, 0xFFFFFFFF), (7, 3, 2)):
        base = h32(seed + 0x9E3779B9 * (k + 1))
        want = [[(h32(base ^ (3 * h + j)) * M) >> 32 for j in range(3)] for h in range(5)]
        got = pr.samples(seed, k, 5, M)
        assert got.tolist() == want and (got < M).all()


def test_one_hypothesis_by_hand():
    P = np.array([[0, 0, 1], [2, 0, 1], [0, 3, 1], [0, 0, 5]], F)
    pl, valid = pr.hypotheses(P, np.array([[0, 1, 2], [0, 2, 1], [0, 0, 1], [0, 1, 3]]))
    assert valid.tolist() == [True, True, False, True]
    assert pl[0].tolist() == [0, 0, 1, -1] and pl[1].tolist() == [0, 0, -1, 1] and np.isnan(pl[2]).all()      # (2,0,0) x (0,3,0) = (0,0,6)
    assert pl[3].tolist() == [0, -1, 0, 0]                                                                    # (2,0,0) x (0,0,4) = (0,-8,0)
    for mode, bound, want in ((pr.AXIS_NORMAL, 0.9, [True, True, False, False]), (pr.AXIS_INPLANE, 0.1, [False, False, False, True])):
        pl, valid = pr.hypotheses(P, np.array([[0, 1, 2], [0, 2, 1], [0, 0, 1], [0, 1, 3]]), mode, (0, 0, 1), bound)
        assert valid.tolist() == want
        if mode == pr.AXIS_NORMAL:
            assert pl[0].tolist() == pl[1].tolist() == [0, 0, 1, -1]                                         # oriented along the axis: t >= 0
    # collinear and coincident samples are invalid; so is a triangle whose cross product overflows
    pl, valid = pr.hypotheses(np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [1e30, 0, 0], [0, 1e30, 0]], F), np.array([[0, 1, 2], [0, 3, 4]]))
    assert valid.tolist() == [False, False]


def test_the_score_and_the_labels_by_hand():
    # five rows on z = 0, two on z = 1, one at z = 0.5: one plane of five with min_inliers 3, then nothing (the rest is 2 + 1)
    pts = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0.5, 0.5, 0), (0.5, 0.5, 0.5)]
    r = pr.planes(sc.of(pts), seed=1, hypotheses=64, distance=0.01, min_inliers=4, max_planes=3, refine=0)
    assert r["label"].tolist() == [0, 0, 0, NONE, 0, NONE, 0, NONE]
    assert r["result"] == dict(nodes=8, planes=1, on_rows=5, off_rows=3) and r["rounds"][1]["best"] < 4
    m = r["models"][0]
    assert abs(m["normal"]).tolist() == [0, 0, 1] and m["d"] == 0 and m["inliers"] == m["sampled_inliers"] == 5 and m["participants"] == 8
    on, off, after = pr.lists(r, -1)
    assert on.tolist() == [0, 1, 2, 4, 6] and off.tolist() == [3, 5, 7] and after == 3
    on, off, after = pr.lists(r, 1)
    assert len(on) == 0 and len(off) == 8 and after == 8


def test_the_refinement_by_hand():
    # the sums of four points around the anchor: mean (0.5, 0.5, 0), covariance diag(0.25, 0.25, 0): normal +-z, through the mean
    S = sc.of([(1, 1, 2), (2, 1, 2), (1, 2, 2), (2, 2, 2)])
    sums = pr.moments(S, np.ones(4, bool), S[0, :3])
    assert sums == [2.0, 2.0, 0.0, 2.0, 1.0, 0.0, 2.0, 0.0, 0.0]
    n, d, th = pr.plane_fit(sums, 4, S[0, :3], (0, 0, -1))
    assert n.tolist() == [0, 0, -1] and d == 2 and th == 0
    n, d, th = pr.plane_fit(sums, 4, S[0, :3], (0, 0, 1))
    assert n.tolist() == [0, 0, 1] and d == -2
    assert pr.plane_fit(sums, 2, S[0, :3], (0, 0, 1)) is None and pr.plane_fit([np.inf] + sums[1:], 4, S[0, :3], (0, 0, 1)) is None
    assert pr.plane_fit([np.nan] * 9, 4, S[0, :3], (0, 0, 1)) is None


# ---------------------------------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_base_scene_has_three_planes_and_ends_by_min_inliers():
    S, part = sc.base()
    assert len(S) == 3100 and len(S) % 64 and len(S) % 256
    r = pr.planes(S, **sc.BASE)
    assert r["result"]["planes"] == 3 and len(r["rounds"]) == 4 and 0 < r["rounds"][3]["best"] < sc.BASE["min_inliers"]
    assert [m["participants"] for m in r["models"]] == [3100, 1600, 700]        # M crosses the chunk edge at 2048 after round 0
    for k, m in enumerate(r["models"]):
        assert (part[r["label"] == k] == k).mean() > 0.95 and m["inliers"] >= (sc.N_FLOOR, sc.N_WALL, sc.N_PATCH)[k]
        assert 0.001 < m["thickness"] < 0.003                                   # the surfaces' 2 mm of noise
    assert pr.planes(S, **dict(sc.BASE, max_planes=2))["result"]["planes"] == 2
    flat = pr.planes(S, **dict(sc.BASE, refine=0))
    assert flat["result"]["planes"] == 3 and not np.array_equal(flat["models"][0]["normal"], r["models"][0]["normal"])
    assert all(m["thickness"] == 0 for m in flat["models"])
    gated = pr.planes(S, **dict(sc.BASE, normal_cos=0.9))
    assert gated["result"]["planes"] == 3 and gated["models"][2]["inliers"] < r["models"][2]["inliers"]      # the clutter on the patch fails it
    floor = pr.planes(S, **dict(sc.BASE, axis_mode=pr.AXIS_NORMAL, axis_bound=0.95))
    assert floor["result"]["planes"] == 1 and floor["models"][0]["normal"][2] > 0.99 and floor["models"][0]["valid_hypotheses"] < 256
    walls = pr.planes(S, **dict(sc.BASE, axis_mode=pr.AXIS_INPLANE, axis_bound=0.1))
    assert walls["result"]["planes"] == 1 and abs(walls["models"][0]["normal"][0]) > 0.99


def test_the_chunk_scene_puts_m_on_the_chunk_edges():
    S, part = sc.chunks()
    r = pr.planes(S, seed=1, hypotheses=128, min_inliers=500, max_planes=4)
    assert [x["M"] for x in r["rounds"]] == [2 * sc.CHUNK + 1, sc.CHUNK, 1024]
    assert [m["inliers"] for m in r["models"]] == [sc.CHUNK + 1, 1024]
    src = open(os.path.join(ROOT, "elasticfusion_amd", "csrc", "ef_map.hpp")).read()
    assert "PLANE_CHUNK = %d;" % sc.CHUNK in src


def test_the_twins_tie_across_the_two_planes():
    S = sc.twins()
    r = pr.planes(S, seed=2, hypotheses=64, min_inliers=100, max_planes=2, refine=0)
    c, pl = r["rounds"][0]["counts"], r["rounds"][0]["planes"]
    top = np.nonzero(c == c.max())[0]
    assert c.max() == 400 and len(top) > 2 and len({float(abs(d)) for d in pl[top, 3]}) == 2        # both planes among the best
    assert r["models"][0]["hypothesis"] == top[0] > 0                                                # the lowest h wins, and it is not h = 0
    assert r["result"]["planes"] == 2 and (r["label"][0::2] != r["label"][1::2]).all()


def test_the_threshold_scene_has_rows_at_and_one_step_beyond():
    S, m = sc.thresholds()
    for nc in (0.0, sc.NORMAL_COS):
        r = pr.planes(S, seed=2, hypotheses=64, min_inliers=100, max_planes=1, refine=0, normal_cos=nc)
        mod, lab = r["models"][0], r["label"]
        assert abs(mod["normal"]).tolist() == [0, 0, 1] and mod["d"] == 0
        assert lab[m["at"]] == lab[m["below_at"]] == lab[m["good"]] == 0 and lab[m["beyond"]] == lab[m["below_beyond"]] == NONE
        assert lab[m["cos_at"]] == 0 and lab[m["cos_below"]] == (NONE if nc else 0)


def test_the_outsiders_and_the_degenerate_scenes():
    S, m = sc.outsiders()
    r = pr.planes(S, seed=2, hypotheses=64, min_inliers=100, max_planes=2, min_conf=10.0)
    assert r["result"] == dict(nodes=1230, planes=1, on_rows=1230, off_rows=0)
    assert (r["label"][np.concatenate([m["bad"], m["low"]])] == NONE).all() and (r["label"][m["boxed"]] == 0).all()
    for k in range(4):
        r = pr.planes(sc.few(k), seed=1, hypotheses=32, min_inliers=1, max_planes=2)
        assert r["result"]["nodes"] == k and r["result"]["planes"] == (1 if k == 3 else 0)
        assert k == 0 or r["rounds"][0]["valid"].sum() == (3 if k == 3 else 0)
    for S in (sc.coincident(), sc.collinear()):
        r = pr.planes(S, seed=1, hypotheses=64, min_inliers=1, max_planes=2)
        assert r["result"] == dict(nodes=50, planes=0, on_rows=0, off_rows=50) and not r["rounds"][0]["valid"].any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# ef_plane_fit.hpp on the host
# ---------------------------------------------------------------------------------------------------------------------------------------
def fit_cases():
    """(m, a, hn, S): sums of random planar patches at several scales and offsets, and degenerate covariances"""
    rng = np.random.default_rng(11)
    cases = []
    for i in range(60):
        n = sc.unit(rng.normal(size=3))
        e1 = sc.unit(np.cross(n, rng.normal(size=3)))
        e2 = np.cross(n, e1)
        k = int(rng.integers(3, 400))
        scale = 10.0 ** rng.uniform(-2, 1)
        pts = rng.normal(size=3) * 5 + scale * (rng.uniform(-1, 1, (k, 1)) * e1 + rng.uniform(-1, 1, (k, 1)) * e2) + rng.normal(0, 0.002, (k, 1)) * n
        S = sc.of(pts)
        hn = sc.unit(n + rng.normal(0, 0.05, 3)).astype(F) * (1 if i % 2 else -1)
        cases.append((k, S[0, :3].copy(), hn, pr.moments(S, np.ones(k, bool), S[0, :3])))
    a, hn = np.zeros(3, F), np.array([0, 0, 1], F)
    z = [0.0] * 9
    cases += [(5, a, hn, z),                                                     # every inlier at the anchor: C = 0, the first eigenvector
              (4, a, hn, [2.0, 0.0, 0.0, 2.0, 0, 0, 0, 0, 0]),                   # collinear along x: two zero eigenvalues, ties to the lowest index
              (4, a, hn, [0.0, 0, 0, 4.0, 0, 0, 4.0, 0, 4.0]),                   # isotropic: three equal eigenvalues
              (4, a, hn, [0.0, 0, 0, 4.0, 0, 0, 4.0, 0, 1.0]),                   # already diagonal
              (4, a, hn, [0.0, 0, 0, 1e300, 1e300, 0, 1e300, 0, 0]),             # huge but finite
              (4, a, hn, [0.0, 0, 0, 1e-300, 1e-300, 0, 1e-300, 0, 0]),          # tiny
              (4, a, hn, [1e200, 0, 0, 1.0, 0, 0, 1.0, 0, 1.0]),                 # mean^2 overflows: refused
              (4, a, hn, [np.nan, 0, 0, 1.0, 0, 0, 1.0, 0, 1.0]), (4, a, hn, [0.0, 0, 0, np.inf, 0, 0, 1.0, 0, 1.0]),
              (2, a, hn, [0.0, 0, 0, 4.0, 0, 0, 4.0, 0, 1.0]),                   # fewer than three
              # the normal (1, 1, 0) / sqrt 2 at an anchor of (3e38, 3e38, 0): d = -4.2e38 leaves f32's range: refused
              (4, np.array([3e38, 3e38, 0], F), np.array([0.7, 0.7, 0], F), [0.0, 0, 0, 4.0, -4.0, 0, 4.0, 0, 4.0])]
    return cases


def run_fit_program(exe, cases):
    bits32 = lambda v: "%08x" % struct.unpack("<I", struct.pack("<f", float(v)))[0]
    bits64 = lambda v: "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    text = "".join(" ".join([str(m)] + [bits32(v) for v in a] + [bits32(v) for v in hn] + [bits64(v) for v in S]) + "\n" for m, a, hn, S in cases)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    return [None if ln == "0" else [int(w, 16) for w in ln.split()[1:]] for ln in lines]


@pytest.mark.parametrize("sanitized", (False, True), ids=("plain", "asan+ubsan"))
def test_the_fit_compiled_for_the_host_equals_the_reference_bit_for_bit(tmp_path, sanitized):
    src = os.path.join(ROOT, "tests", "plane_fit_main.cpp")
    cmd = ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "elasticfusion_amd", "csrc")]
    if sanitized:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        trial = tmp_path / "trial.cpp"
        trial.write_text("int main() { return 0; }\n")
        ok = subprocess.run(cmd + [str(trial), "-o", str(tmp_path / "trial")], capture_output=True).returncode == 0
        if not (ok and subprocess.run([str(tmp_path / "trial")], capture_output=True).returncode == 0):
            cmd = cmd[:-2]
            print("sanitizers: not available, plain build")
    exe = tmp_path / "plane_fit"
    subprocess.run(cmd + [src, "-o", str(exe)], check=True)
    cases = fit_cases()
    got = run_fit_program(exe, cases)
    refused = 0
    for i, ((m, a, hn, S), g) in enumerate(zip(cases, got)):
        want = pr.plane_fit(S, m, a, hn)
        if want is None:
            assert g is None, (i, g)
            refused += 1
            continue
        bits = np.concatenate([want[0], [want[1], want[2]]]).astype(F).view(np.uint32).tolist()
        assert g == bits, (i, g, bits)
    assert refused == 5


def test_the_eigenvector_agrees_with_eigh():
    worst, seen = 0.0, 0
    for m, a, hn, S in fit_cases()[:60]:
        mean = np.array(S[:3]) / m
        Cm = np.array([[S[3], S[4], S[5]], [S[4], S[6], S[7]], [S[5], S[7], S[8]]]) / m - np.outer(mean, mean)
        w, v = np.linalg.eigh(Cm)
        if w[1] - w[0] < 1e-3 * w[2]:
            continue
        # the double normal before its rounding to f32: plane_fit's own steps, stopped there
        A = [[float(Cm[i][j]) for j in range(3)] for i in range(3)]
        V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
        for _ in range(pr.SWEEPS):
            pr.rotate(A, V, 0, 1, 2)
            pr.rotate(A, V, 0, 2, 1)
            pr.rotate(A, V, 1, 2, 0)
        best = int(np.argmin([A[0][0], A[1][1], A[2][2]]))
        n = np.array([V[0][best], V[1][best], V[2][best]])
        assert max(abs(A[0][1]), abs(A[0][2]), abs(A[1][2])) <= 1e-30 * w[2] + 1e-300, "the sweeps have converged"
        worst = max(worst, float(np.linalg.norm(np.cross(n / np.linalg.norm(n), v[:, 0]))))
        seen += 1
        got = pr.plane_fit(S, m, a, hn)
        assert got is not None and np.dot(got[0].astype(np.float64), np.asarray(hn, np.float64)) >= 0
        assert abs(float(got[2]) - np.sqrt(max(w[0], 0))) <= 1e-6 * np.sqrt(w[2])
    print("eigenvector against eigh: worst |sin angle| %.3g over %d cases" % (worst, seen))
    assert seen >= 50 and worst <= 1e-9


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
    p = api.ef_plane_params(distance=0.01, normal_cos=0.0, min_conf=-1.0, hypotheses=256, seed=1, max_planes=4, min_inliers=100, refine=1,
                            axis_mode=0, axis=(C.c_float * 3)(0, 0, 1), axis_bound=0.95)
    for k, v in kw.items():
        setattr(p, k, (C.c_float * 3)(*v) if k == "axis" else v)
    return p


NAN, INF = float("nan"), float("inf")
BAD = [(dict(distance=0.0), "distance"), (dict(distance=-1.0), "distance"), (dict(distance=NAN), "distance"), (dict(distance=INF), "distance"),
       (dict(normal_cos=-0.1), "normal_cos"), (dict(normal_cos=1.5), "normal_cos"), (dict(normal_cos=NAN), "normal_cos"),
       (dict(axis_bound=-0.1), "axis_bound"), (dict(axis_bound=1.01), "axis_bound"), (dict(axis_bound=NAN), "axis_bound"),
       (dict(min_conf=NAN), "min_conf"), (dict(hypotheses=0), "hypotheses"), (dict(hypotheses=4097), "hypotheses"),
       (dict(max_planes=0), "max_planes"), (dict(max_planes=17), "max_planes"), (dict(refine=2), "refine"), (dict(axis_mode=3), "axis_mode"),
       (dict(axis_mode=1, axis=(0, 0, 0.9)), "axis"), (dict(axis_mode=2, axis=(0, 0.8, 0.8)), "axis"), (dict(axis_mode=1, axis=(NAN, 0, 1)), "axis")]


def test_every_refusal_names_its_argument_with_a_null_context(lib):
    from elasticfusion_amd import api
    EINVAL = -1
    res, cnt, rows = api.ef_plane_result(), C.c_uint32(0), (C.c_uint32 * 4)()
    calls = {
        "ef_map_planes": lambda p, a: lib.ef_map_planes(None, p, a, None, 0, None, None),
        "ef_map_planes_dev": lambda p, a: lib.ef_map_planes_dev(None, p, a, None, 0, None, None),
        "ef_map_planes_select": lambda p, a: lib.ef_map_planes_select(None, p, a, api.PLANES_OFF, -1, rows, 4, C.byref(cnt), None, None),
        "ef_map_planes_select_dev": lambda p, a: lib.ef_map_planes_select_dev(None, p, a, api.PLANES_ON, 3, rows, 4, C.byref(cnt), None, None),
        "ef_map_remove_planes": lambda p, a: lib.ef_map_remove_planes(None, p, a, 0, None, C.byref(res)),
    }

    def refused(rc, fn, word):
        msg = lib.ef_last_error(None).decode()
        assert rc == EINVAL and msg.startswith(fn + ":") and word in msg, (fn, word, rc, msg)

    for fn, call in calls.items():
        refused(call(None, None), fn, "null params")
        for change, word in BAD:
            refused(call(C.byref(good_params(**change)), None), fn, word)
        refused(call(C.byref(good_params(axis=(0, 0, 5))), None), fn, "null context")                      # the axis is not looked at with the mode off
        refused(call(C.byref(good_params(axis_mode=1, axis=(0, 0.6, 0.8), normal_cos=1.0, axis_bound=0.0)), None), fn, "null context")
        refused(call(C.byref(good_params(hypotheses=4096, max_planes=16)), None), fn, "null context")      # the limits themselves are allowed
        sel = api.ef_map_selection()
        lib.ef_default_map_selection(C.byref(sel))
        sel.tests = 0x8000
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "unknown bits")                            # what ef_map_select refuses
        sel.tests, sel.conf_min = api.SEL_CONF, NAN
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "NaN")
    p = C.byref(good_params())
    for fn in ("ef_map_planes_select", "ef_map_planes_select_dev"):
        call = getattr(lib, fn)
        for what in (2, -1):
            refused(call(None, p, None, what, 0, rows, 4, C.byref(cnt), None, None), fn, "what")
        for which in (-2, 4, 16):
            refused(call(None, p, None, 0, which, rows, 4, C.byref(cnt), None, None), fn, "which")
        refused(call(None, p, None, 0, 0, None, 4, C.byref(cnt), None, None), fn, "null rows")
        refused(call(None, p, None, 0, 0, rows, 4, None, None, None), fn, "null count")
        refused(call(None, p, None, 1, 3, None, 0, C.byref(cnt), None, None), fn, "null context")          # NULL rows with max_rows 0 is fine
    refused(lib.ef_map_remove_planes(None, p, None, 0, None, None), "ef_map_remove_planes", "null result")
    refused(lib.ef_map_remove_planes(None, p, None, 4, None, C.byref(res)), "ef_map_remove_planes", "which")
    assert lib.ef_default_plane_params(None, C.byref(good_params())) == EINVAL and b"null context" in lib.ef_last_error(None)


def test_the_new_structs_and_constants_are_the_headers():
    from elasticfusion_amd import accuracy, api
    structs = header_structs()
    for name in ("ef_plane_params", "ef_plane_model", "ef_plane_result"):
        assert structs[name] == [f for f, _ in getattr(api, name)._fields_]
    assert C.sizeof(api.ef_plane_params) == 52 and C.sizeof(api.ef_plane_model) == 40 and C.sizeof(api.ef_plane_result) == 20
    assert api.ef_plane_params.axis.offset == 36 and api.ef_plane_model.thickness.offset == 36
    want = defines("PLANE")
    mine = {k: v for k, v in vars(api).items() if k.startswith("PLANE") and isinstance(v, int)}
    assert want == dict(PLANE_NONE=0xFFFFFFFF, PLANE_MAX_PLANES=16, PLANE_MAX_HYPOTHESES=4096, PLANE_AXIS_OFF=0, PLANE_AXIS_NORMAL=1,
                        PLANE_AXIS_INPLANE=2, PLANES_ON=0, PLANES_OFF=1) and mine == want, (mine, want)
    assert (pr.NONE, pr.AXIS_OFF, pr.AXIS_NORMAL, pr.AXIS_INPLANE, pr.ON, pr.OFF) == (api.PLANE_NONE, api.PLANE_AXIS_OFF, api.PLANE_AXIS_NORMAL,
                                                                                    api.PLANE_AXIS_INPLANE, api.PLANES_ON, api.PLANES_OFF)
    for name in ("planeParams", "planes", "planeSelect", "planeSelectDevice", "planesDevice", "removePlanes"):
        assert callable(getattr(api.ElasticFusion, name))
    assert callable(accuracy.plane_segments) and callable(accuracy.without_planes)
    # the reference's sweeps and summation lanes are the kernels'
    src = open(os.path.join(ROOT, "elasticfusion_amd", "csrc", "ef_plane_fit.hpp")).read()
    assert "EF_PLANE_FIT_SWEEPS = %d;" % pr.SWEEPS in src
