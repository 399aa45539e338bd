"""CPU-only checks of the smoothing (ef_map_smooth / ef_map_smooth_select / ef_map_smooth_apply, include/ef_hip.h): the scenes
contain what they claim, shown on the numpy reference (tests/smoothref.py, written from the header alone); the definition smooths (the orderings
DESIGN.md §8n records); with unit weights it is the normal estimation bit for bit; smooth_fit of csrc/ef_plane_fit.hpp compiled by the host
compiler into a stand-alone program (tests/smooth_fit_main.cpp; once more with the address and undefined-behaviour sanitizers) equals the
reference bit for bit; every EF_EINVAL of the header through the C ABI without a device; the binding."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import normalref as nr
import normalscenes as ns
import smoothref as sr
import smoothscenes as ss
from test_api_binding_host import defines, header_structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DRIFT = dict(radius=ss.R_DRIFT, k=16, iterations=3)


@pytest.fixture(scope="module")
def edge():
    S, marks = ns.edge_scene()
    nl = nr.neighbour_lists(S, ns.R_EDGE, -1.0)
    return dict(S=S, marks=marks, nl=nl)


def edge_kw(k, **kw):
    return dict(dict(radius=ns.R_EDGE, k=k, min_neighbors=ns.MIN_NEIGHBORS[k]), **kw)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the scenes contain what they claim
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_edge_scene_has_every_status_short_neighbourhoods_and_ties(edge):
    S, m, (count, D, R) = edge["S"], edge["marks"], edge["nl"]
    for k in ns.KS:
        for w in (sr.UNIFORM, sr.COMPACT):
            runs = sr.smooth_runs(S, nl=edge["nl"], iterations=3, weighting=w, **edge_kw(k))
            for ref in runs:
                assert set(np.unique(ref["status"]).tolist()) == {sr.NONE, sr.SMOOTHED, sr.SPARSE, sr.DEGENERATE}, (k, w)
                res = ref["result"]
                assert res["smoothed"] + res["sparse"] + res["degenerate"] == res["participants"] == len(S) - len(m["bad"])
                assert (ref["status"][m["bad"]] == sr.NONE).all() and (ref["shift"][m["bad"]] == 0).all() and (ref["count"][m["bad"]] == 0).all()
                still = ref["shift"] == 0
                assert nr.same_bits(ref["position"][still], S[still, :3])                       # a row that never moved keeps the map's bits
                never = (ref["status"] == sr.SPARSE) | (ref["status"] == sr.NONE)
                assert still[never].all() and (ref["normal"][ref["status"] != sr.SMOOTHED] == 0).all()
                for g in ("line", "slant", "point"):
                    assert (ref["status"][m[g]] == sr.DEGENERATE).all() and still[m[g]].all(), (k, g)
            assert (runs[0]["status"][m["fewer"]] == (sr.SPARSE if k >= 5 else sr.SMOOTHED)).all()
            assert not nr.same_bits(runs[0]["position"], runs[1]["position"]) and not nr.same_bits(runs[1]["position"], runs[2]["position"])
    short = sr.smooth(S, nl=edge["nl"], **edge_kw(16))
    fitted = (short["status"] == sr.SMOOTHED) | (short["status"] == sr.DEGENERATE)
    assert (fitted & (count < 16)).sum() > 50                                                    # participants with c < k
    c = m["centre"]
    for k in ns.TIE_KS:                                                                          # a tie in d2 at rank k, decided by the row
        j = min(k, 15)
        assert D[c, j - 1] == D[c, j] and R[c, j - 1] < R[c, j], k
    assert sr.smooth(S, nl=edge["nl"], **edge_kw(5))["status"][c] == sr.SMOOTHED


def test_the_drift_scene_has_neighbours_past_the_radius_gated_neighbours_and_clamped_rows():
    S = ss.drift_scene()
    for w in (sr.UNIFORM, sr.COMPACT):
        seen = {}
        runs = sr.smooth_runs(S, weighting=w, normal_gate=1, min_normal_cos=0.5, seen=seen, **DRIFT)
        assert seen[0]["past_radius"] == 0 and seen[1]["past_radius"] > 10 and seen[2]["past_radius"] > 10, seen      # the weight's clamp at 0
        assert seen[0]["gated_out"] > 100
        assert runs[-1]["result"]["sparse"] > 20 and runs[-1]["result"]["degenerate"] > 5 and runs[-1]["result"]["clamped"] == 0
    open_, gated = sr.smooth(S, **DRIFT), sr.smooth(S, normal_gate=1, min_normal_cos=0.5, **DRIFT)
    assert not nr.same_bits(open_["position"], gated["position"])
    cl = sr.smooth_runs(S, max_shift=ss.R_DRIFT / 16, strength=0.5, **DRIFT)
    n_cl = [r["result"]["clamped"] for r in cl]
    assert n_cl[0] > 20 and n_cl[0] <= n_cl[1] <= n_cl[2] and n_cl[2] > n_cl[0], n_cl                # the bit is sticky
    assert abs(cl[0]["result"]["largest_shift"] - ss.R_DRIFT / 16) < 1e-6                            # a clamped step is max_shift long
    assert len(sr.listed(cl[2], sr.CLAMPED)) == n_cl[2] and cl[2]["clamped"][cl[0]["clamped"]].all()
    half, full = sr.smooth(S, radius=ss.R_DRIFT, k=16, strength=0.5), sr.smooth(S, radius=ss.R_DRIFT, k=16)
    mv = full["shift"] > 1e-3                                # (positions near z = 2 are rounded to 2.4e-7: a shift of a millimetre is known to 5e-4 of itself)
    ratio = half["shift"][mv].astype(np.float64) / full["shift"][mv]
    assert mv.sum() > 200 and np.abs(ratio - 0.5).max() < 2e-3


def test_lists_and_the_write_back_of_the_reference():
    S = ss.drift_scene()
    S[5, 0] = np.nan
    ref = sr.smooth(S, max_shift=ss.R_DRIFT / 16, shift_threshold=0.001, set_normal=1, normal_gate=1, min_normal_cos=0.5, **DRIFT)
    rows = {w: sr.listed(ref, w) for w in (sr.SMOOTHED, sr.SPARSE, sr.DEGENERATE, sr.CLAMPED, sr.SHIFTED)}
    assert all(len(r) > 5 for r in rows.values()), {w: len(r) for w, r in rows.items()}
    assert len(rows[sr.SMOOTHED]) + len(rows[sr.SPARSE]) + len(rows[sr.DEGENERATE]) == ref["result"]["participants"] == len(S) - 1
    assert len(rows[sr.SHIFTED]) < ref["result"]["moved"]
    W = sr.written(S, ref)
    done = ref["status"] == sr.SMOOTHED
    assert nr.same_bits(W[:, 3:8], S[:, 3:8]) and nr.same_bits(W[:, 11], S[:, 11]) and nr.same_bits(W[~done, 8:11], S[~done, 8:11])
    assert nr.same_bits(W[5], S[5]) and not nr.same_bits(W[done, :3], S[done, :3]) and not nr.same_bits(W[done, 8:11], S[done, 8:11])
    keep = sr.written(S, dict(ref, params=dict(ref["params"], set_normal=0)))
    assert nr.same_bits(keep[:, 3:], S[:, 3:]) and nr.same_bits(keep[:, :3], W[:, :3])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the definition smooths: the orderings DESIGN.md §8n records with their values
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_noisy_plane_gets_flatter_with_every_iteration():
    S = ss.plane_lattice()
    for w in (sr.COMPACT, sr.UNIFORM):
        runs = sr.smooth_runs(S, iterations=3, weighting=w)
        rms = [ss.plane_rms(S[:, :3])] + [ss.plane_rms(r["position"]) for r in runs]
        print("weighting", w, "RMS distance to the true plane in mm: input %.3f, iterations 1 .. 3: %.3f %.3f %.3f" % tuple(1e3 * v for v in rms))
        assert rms[0] > rms[1] > rms[2] > rms[3], rms
        assert runs[-1]["result"]["smoothed"] == len(S)
        d = (runs[-1]["position"] - S[:, :3]).astype(np.float64)
        assert np.sqrt((d[:, :2] ** 2).sum(1).mean()) < 0.2 * np.sqrt((d[:, 2] ** 2).mean())           # the motion is along the normal


def test_the_normal_gate_keeps_a_crease_sharp():
    S, marks, near = ss.noisy_box_corner()
    nl = nr.neighbour_lists(S, 0.03)
    before = ss.crease_rms(S[:, :3], marks, near)
    seen = {}
    gated = sr.smooth_runs(S, nl=nl, normal_gate=1, min_normal_cos=0.9, seen=seen)[-1]
    plain = sr.smooth(S, nl=nl)
    a, b = ss.crease_rms(gated["position"], marks, near), ss.crease_rms(plain["position"], marks, near)
    print("RMS distance to the own face within 2 pitches of a crease in mm: input %.3f, gated %.3f, ungated %.3f" % (1e3 * before, 1e3 * a, 1e3 * b))
    assert a < b and seen[0]["gated_out"] > 1000 and sum(len(r) for r in near) > 300


# ---------------------------------------------------------------------------------------------------------------------------------------
# with unit weights it is the normal estimation
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_uniform_weights_without_the_gate_give_the_normals_estimate(edge):
    S = edge["S"]
    for k in ns.KS:
        a = sr.smooth(S, nl=edge["nl"], weighting=sr.UNIFORM, **edge_kw(k))
        b = nr.estimate(S, nl=edge["nl"], **edge_kw(k))
        assert nr.same_bits(a["normal"], b["normals"]) and nr.same_bits(a["curvature"], b["curvature"]) and np.array_equal(a["count"], b["count"])
        assert np.array_equal(a["status"] == sr.SMOOTHED, b["status"] == nr.ESTIMATED) and np.array_equal(a["status"] == sr.SPARSE, b["status"] == nr.SPARSE)
        assert np.array_equal(a["status"] == sr.DEGENERATE, b["status"] == nr.DEGENERATE)
        c = sr.smooth(S, nl=edge["nl"], **edge_kw(k))
        assert not nr.same_bits(a["normal"], c["normal"])                                        # the compact weights matter


# ---------------------------------------------------------------------------------------------------------------------------------------
# smooth_fit of ef_plane_fit.hpp on the host
# ---------------------------------------------------------------------------------------------------------------------------------------
def scene_sums(S, **kw):
    """(m, hn, line_ratio, W, S) of every fitted row and every iteration of a run on S"""
    p = dict(sr.DEFAULTS, **kw)
    p["max_shift"] = p["radius"] if p["max_shift"] is None else p["max_shift"]
    part = nr.participants(S)
    nl = nr.neighbour_lists(S, p["radius"], p["min_conf"], part)
    count, R = nl[0], nl[2]
    c = np.minimum(count, np.uint32(p["k"])).astype(np.int64)
    fitted = part & (count >= np.uint32(p["min_neighbors"]))
    runs = sr.smooth_runs(S, nl=nl, **kw)
    P, N, out = S[:, :3].copy(), S[:, 8:11].copy(), []
    for run in runs:
        Sm, W = sr.sums(P, N, fitted, c, R, p)
        out += [(int(c[s]) + 1, N[s], p["line_ratio"], W[s], Sm[s]) for s in np.nonzero(fitted)[0]]
        P = run["position"]
    return out


def fit_cases(edge):
    cases = scene_sums(edge["S"], iterations=2, **edge_kw(5)) + scene_sums(edge["S"], weighting=sr.UNIFORM, **edge_kw(16))
    cases += scene_sums(ss.drift_scene(), normal_gate=1, min_normal_cos=0.5, **DRIFT)
    hn, z = np.array([0, 0, 1], F), [0.0] * 9
    plane = [0.0, 0, 0, 4.0, 0, 0, 4.0, 0, 1.0]
    tiny = float(np.nextafter(1.0, 2.0))
    cases += [(5, hn, 1e-4, 1.0, z),                                                          # all weights 0: W stays 1, C = 0
              (5, hn, 1e-4, tiny, [1e-17, 2e-17, 0, 1e-17, 0, 0, 2e-17, 0, 0]),                # W barely above 1
              (5, hn, 1e-4, tiny, plane), (4, hn, 1e-4, 2.5, plane), (4, -hn, 1e-4, 3.75, plane),
              (4, np.array([np.nan, 0, 0], F), 1e-4, 2.5, plane), (4, np.array([1, 1, 0], F), 1e-4, 2.5, plane),
              (4, hn, 1e-4, np.nan, plane), (4, hn, 1e-4, np.inf, plane), (4, hn, 1e-4, 0.0, plane), (4, hn, 1e-4, -2.0, plane),
              (4, hn, 1e-4, 2.5, [np.nan, 0, 0, 1.0, 0, 0, 1.0, 0, 1.0]), (4, hn, 1e-4, 2.5, [0.0, 0, 0, np.inf, 0, 0, 1.0, 0, 1.0]),
              (4, hn, 1e-4, 2.5, [0.0, 0, 0, -1.0, 0, 0, 4.0, 0, 1.0]),                          # a negative "variance": clamped to 0
              (4, hn, 1e-4, 2.5, [0.0, 0, 0, 1e300, 1e300, 0, 1e300, 0, 1e300]),                 # huge but finite
              (4, hn, 1e-4, 2.5, [0.0, 0, 0, 1e-300, 1e-301, 0, 1e-300, 0, 1e-300]),             # tiny
              (4, hn, 1e-4, 2.5, [1e200, 0, 0, 1.0, 0, 0, 1.0, 0, 1.0]),                         # mean^2 overflows: gives up
              (4, hn, 1e-4, 1e-300, plane),                                                      # a tiny divisor: overflows
              (2, hn, 1e-4, 2.0, plane),                                                         # fewer than three members
              (4, hn, 0.0, 2.5, [0.0, 0, 0, 4.0, 0, 0, 0.0, 0, 0.0]),                            # a line at line_ratio 0
              (4, hn, 1e-4, 2.5, [0.5, 0.25, 0.125, 4.0, 1.0, 0.5, 3.0, 0.25, 1.0])]
    return cases


def test_the_vectorised_fit_is_the_scalar_normal_fit_for_unit_weights(edge):
    cases = scene_sums(edge["S"], weighting=sr.UNIFORM, **edge_kw(8))
    m, hn, lr, W, S = (np.array([c[i] for c in cases]) for i in range(5))
    assert (W == m).all()                                                                        # W == (double)(c + 1)
    verdict, n, mean, curv = sr.fit(S, W, m, hn, 1e-4)
    for i, (mi, h, _, _, Si) in enumerate(cases):
        status, normal, cv, flipped, l = nr.normal_fit(Si, mi, h, 1e-4)
        assert (verdict[i] == sr.FIT_ESTIMATED) == (status == nr.ESTIMATED)
        assert nr.same_bits(n[i].astype(F), normal) and nr.same_bits(curv[i], cv), i
    assert (verdict == sr.FIT_ESTIMATED).sum() > 400 and (verdict != sr.FIT_ESTIMATED).sum() > 10


@pytest.mark.parametrize("sanitized", (False, True), ids=("plain", "asan+ubsan"))
def test_the_fit_compiled_for_the_host_equals_the_reference_bit_for_bit(tmp_path, edge, sanitized):
    src = os.path.join(ROOT, "tests", "smooth_fit_main.cpp")
    cmd = ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "elasticfusion_amd", "csrc")]
    if sanitized:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        trial = tmp_path / "trial.cpp"
        trial.write_text("int main() { return 0; }\n")
        ok = subprocess.run(cmd + [str(trial), "-o", str(tmp_path / "trial")], capture_output=True).returncode == 0
        if not (ok and subprocess.run([str(tmp_path / "trial")], capture_output=True).returncode == 0):
            cmd = cmd[:-2]
            print("sanitizers: not available, plain build")
    exe = tmp_path / "smooth_fit"
    subprocess.run(cmd + [src, "-o", str(exe)], check=True)
    cases = fit_cases(edge)
    bits32 = lambda v: "%08x" % struct.unpack("<I", struct.pack("<f", float(v)))[0]
    bits64 = lambda v: "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    text = "".join(" ".join([str(m)] + [bits32(v) for v in hn] + [bits32(lr), bits64(W)] + [bits64(v) for v in S]) + "\n" for m, hn, lr, W, S in cases)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases) > 2500
    seen = {sr.GAVE_UP: 0, sr.FIT_ESTIMATED: 0, sr.FIT_DEGENERATE: 0}
    lrs = sorted({float(c[2]) for c in cases})
    want = {}
    for lr in lrs:                                                                               # the reference once per line_ratio, every row at once
        idx = [i for i, c in enumerate(cases) if float(c[2]) == lr]
        v, n, mean, curv = sr.fit([cases[i][4] for i in idx], [cases[i][3] for i in idx], [cases[i][0] for i in idx], [cases[i][1] for i in idx], lr)
        for j, i in enumerate(idx):
            want[i] = (int(v[j]), n[j], mean[j], curv[j])
    for i, line in enumerate(lines):
        v, n, mean, curv = want[i]
        exp = [str(v)] + [bits64(x) for x in n] + [bits64(x) for x in mean] + [bits32(curv)]
        assert line.split() == exp, (i, cases[i], line, exp)
        seen[v] += 1
    print(seen)
    assert seen[sr.FIT_ESTIMATED] > 2000 and seen[sr.FIT_DEGENERATE] > 40 and seen[sr.GAVE_UP] >= 5


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
    p = api.ef_smooth_params(radius=0.03, cell=0.03, min_conf=-1.0, k=12, min_neighbors=5, iterations=1, weighting=1, normal_gate=0, min_normal_cos=0.9,
                             strength=1.0, max_shift=0.03, line_ratio=1e-4, set_normal=0, shift_threshold=0.0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


NAN, INF = float("nan"), float("inf")
BAD = [(dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=NAN), "radius"), (dict(radius=INF), "radius"),
       (dict(cell=0.0), "cell"), (dict(cell=NAN), "cell"), (dict(cell=INF), "cell"), (dict(cell=1e-45), "cell"),
       (dict(radius=1.0, cell=0.01), "radius / cell"), (dict(min_conf=NAN), "min_conf"),
       (dict(k=2, min_neighbors=2), "k must"), (dict(k=17), "k must"), (dict(k=0), "k must"),
       (dict(min_neighbors=1), "min_neighbors"), (dict(min_neighbors=13), "min_neighbors"), (dict(k=3, min_neighbors=4), "min_neighbors"),
       (dict(iterations=0), "iterations"), (dict(iterations=17), "iterations"), (dict(iterations=-1), "iterations"),
       (dict(weighting=2), "weighting"), (dict(weighting=-1), "weighting"), (dict(normal_gate=2), "normal_gate"), (dict(normal_gate=-1), "normal_gate"),
       (dict(min_normal_cos=NAN), "min_normal_cos"), (dict(strength=0.0), "strength"), (dict(strength=-0.5), "strength"),
       (dict(strength=1.5), "strength"), (dict(strength=NAN), "strength"), (dict(max_shift=0.0), "max_shift"), (dict(max_shift=-1.0), "max_shift"),
       (dict(max_shift=NAN), "max_shift"), (dict(line_ratio=NAN), "line_ratio"), (dict(line_ratio=-1e-6), "line_ratio"),
       (dict(shift_threshold=NAN), "shift_threshold"), (dict(shift_threshold=-1e-6), "shift_threshold")]


def test_every_refusal_names_its_argument_with_a_null_context(lib):
    from elasticfusion_amd import api
    EINVAL = -1
    res, cnt, rows = api.ef_smooth_result(), C.c_uint32(0), (C.c_uint32 * 4)()
    calls = {
        "ef_map_smooth": lambda p, a: lib.ef_map_smooth(None, p, a, None, None, None, None, None, None, 0, None),
        "ef_map_smooth_dev": lambda p, a: lib.ef_map_smooth_dev(None, p, a, None, None, None, None, None, None, 0, None),
        "ef_map_smooth_select": lambda p, a: lib.ef_map_smooth_select(None, p, a, api.SMOOTH_SMOOTHED, rows, 4, C.byref(cnt), None),
        "ef_map_smooth_select_dev": lambda p, a: lib.ef_map_smooth_select_dev(None, p, a, api.SMOOTH_SHIFTED, rows, 4, C.byref(cnt), None),
        "ef_map_smooth_apply": lambda p, a: lib.ef_map_smooth_apply(None, p, a, C.byref(res)),
    }

    def refused(rc, fn, word):
        msg = lib.ef_last_error(None).decode()
        assert rc == EINVAL and msg.startswith(fn + ":") and word in msg, (fn, word, rc, msg)

    for fn, call in calls.items():
        refused(call(None, None), fn, "null params")
        for change, word in BAD:
            refused(call(C.byref(good_params(**change)), None), fn, word)
        refused(call(C.byref(good_params(k=3, min_neighbors=2, iterations=16, weighting=0, normal_gate=1, min_normal_cos=-INF, strength=1e-6,
                                         max_shift=INF, line_ratio=0.0, shift_threshold=INF, set_normal=7)), None), fn, "null context")   # the limits themselves
        refused(call(C.byref(good_params(k=16, min_neighbors=16, radius=0.16, cell=0.01, max_shift=1e-30)), None), fn, "null context")
        sel = api.ef_map_selection()
        lib.ef_default_map_selection(C.byref(sel))
        sel.tests = 0x8000
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "unknown bits")                        # what ef_map_select refuses
        sel.tests, sel.conf_min = api.SEL_CONF, NAN
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "NaN")
    p = C.byref(good_params())
    for fn in ("ef_map_smooth_select", "ef_map_smooth_select_dev"):
        call = getattr(lib, fn)
        for what in (0, 6, -1, -5):
            refused(call(None, p, None, what, rows, 4, C.byref(cnt), None), fn, "what")
        for what in (1, 2, 3, 4, 5):
            refused(call(None, p, None, what, rows, 4, C.byref(cnt), None), fn, "null context")
        refused(call(None, p, None, 1, None, 4, C.byref(cnt), None), fn, "null rows")
        refused(call(None, p, None, 1, rows, 4, None, None), fn, "null count")
        refused(call(None, p, None, 1, None, 0, C.byref(cnt), None), fn, "null context")               # NULL rows with max_rows 0 is fine
    refused(lib.ef_map_smooth_apply(None, p, None, None), "ef_map_smooth_apply", "null result")
    assert lib.ef_default_smooth_params(None, C.byref(good_params())) == EINVAL and b"null context" in lib.ef_last_error(None)


def test_the_new_structs_and_constants_are_the_headers():
    from elasticfusion_amd import accuracy, api
    structs = header_structs()
    for name in ("ef_smooth_params", "ef_smooth_result"):
        assert structs[name] == [f for f, _ in getattr(api, name)._fields_]
    assert C.sizeof(api.ef_smooth_params) == 56 and C.sizeof(api.ef_smooth_result) == 32 and api.ef_smooth_result.largest_shift.offset == 28
    want = defines("SMOOTH")
    mine = {k: v for k, v in vars(api).items() if k.startswith("SMOOTH") and isinstance(v, int)}
    assert want == dict(SMOOTH_UNIFORM=0, SMOOTH_COMPACT=1, SMOOTH_NONE=0, SMOOTH_SMOOTHED=1, SMOOTH_SPARSE=2, SMOOTH_DEGENERATE=3, SMOOTH_CLAMPED=4,
                        SMOOTH_SHIFTED=5) and mine == want, (mine, want)
    assert (sr.UNIFORM, sr.COMPACT, sr.NONE, sr.SMOOTHED, sr.SPARSE, sr.DEGENERATE, sr.CLAMPED, sr.SHIFTED) == (
        api.SMOOTH_UNIFORM, api.SMOOTH_COMPACT, api.SMOOTH_NONE, api.SMOOTH_SMOOTHED, api.SMOOTH_SPARSE, api.SMOOTH_DEGENERATE, api.SMOOTH_CLAMPED,
        api.SMOOTH_SHIFTED)
    assert (sr.SMOOTHED, sr.SPARSE, sr.DEGENERATE) == (api.NORMAL_ESTIMATED, api.NORMAL_SPARSE, api.NORMAL_DEGENERATE)
    for name in ("smoothParams", "smoothMap", "smoothMapDevice", "smoothSelect", "smoothSelectDevice", "applySmooth"):
        assert callable(getattr(api.ElasticFusion, name))
    assert callable(accuracy.smoothed_map)
    src = open(os.path.join(ROOT, "elasticfusion_amd", "csrc", "ef_plane_fit.hpp")).read()
    assert "EF_PLANE_FIT_SWEEPS = %d;" % sr.SWEEPS in src and "smooth_fit(" in src
    hdr = open(os.path.join(ROOT, "include", "ef_hip.h")).read()
    assert "Not provided: smoothing of positions" not in hdr and "Smooth the map's positions" in hdr
