"""CPU-only checks of the boundary estimation (ef_map_boundaries / ef_map_boundaries_select, include/ef_hip.h): the hand-built
scenes contain the edges they claim, shown on the numpy reference (tests/boundaryref.py, written from the header alone); the plate's analytic
verdicts and loops equal the reference's; boundary_gap of csrc/ef_boundary_gap.hpp compiled by the host compiler into a stand-alone program
(tests/boundary_gap_main.cpp; once more with the address and undefined-behaviour sanitizers) equals the reference bit for bit;
ef_boundary_gap_from_angle; every EF_EINVAL of the header through the C ABI without a device; the binding."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import boundaryref as br
import boundaryscenes as bs
import componentref as cr
import normalref as nr
from test_api_binding_host import defines, header_structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
THR = 10.0           # a context's default confidence threshold (the GPU tests read it from the context and assert the scenes straddle it)


@pytest.fixture(scope="module")
def edge():
    S, marks = bs.edge_scene()
    nl = {mc: nr.neighbour_lists(S, bs.R_EDGE, mc) for mc in (-1.0, THR)}
    refs = {(k, mc): br.boundaries(S, nl=nl[mc], radius=bs.R_EDGE, min_conf=mc, k=k, min_neighbors=bs.MIN_NEIGHBORS) for k in bs.KS for mc in nl}
    return dict(S=S, marks=marks, nl=nl, refs=refs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the scenes contain the edges they claim
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_rows_that_take_no_part_and_sparse_rows(edge):
    S, m = edge["S"], edge["marks"]
    for ref in edge["refs"].values():
        r = m["nan_pos"]
        assert ref["status"][r] == br.NONE and ref["count"][r] == 0 and ref["gap"][r] == 0 and ref["label"][r] == br.LOOP_NONE
        assert ref["status"][m["sparse"]] == br.SPARSE and ref["count"][m["sparse"]] == 1 and ref["gap"][m["sparse"]] == 0
        assert ref["status"][m["excluded"]] in (br.INTERIOR, br.BOUNDARY)    # judged without the mask ...
    nl = nr.neighbour_lists(S, bs.R_EDGE, -1.0, nr.participants(S, m["among"]))
    ref = br.boundaries(S, among=m["among"], nl=nl, radius=bs.R_EDGE, k=8, min_neighbors=bs.MIN_NEIGHBORS)
    full = edge["refs"][(8, -1.0)]
    assert ref["status"][m["excluded"]] == br.NONE and ref["result"]["participants"] == full["result"]["participants"] - 1      # ... NONE with it
    keep = np.arange(len(S)) != m["excluded"]
    assert np.array_equal(ref["status"][keep], full["status"][keep]) and nr.same_bits(ref["gap"][keep], full["gap"][keep])      # it stays a neighbour


def test_degenerate_rows(edge):
    m = edge["marks"]
    for ref in edge["refs"].values():
        for g in ("zero_normal", "nan_normal", "along"):
            assert ref["status"][m[g]] == br.DEGENERATE and ref["gap"][m[g]] == 0 and ref["count"][m[g]] >= 2, g
    S = edge["S"]
    assert br.frame(S[m["zero_normal"], 8:11]) is None and br.frame(S[m["nan_normal"], 8:11]) is None
    count, D, R = edge["nl"][-1.0]
    a = m["along"]
    e1, e2, _ = br.frame(S[a, 8:11])
    assert count[a] == 2 and not any(br.project(e1, e2, S[a, :3], S[R[a, j], :3])[2] for j in range(2))     # m_s == 0


def test_exact_gaps(edge):
    m = edge["marks"]
    for (k, mc), ref in edge["refs"].items():
        gap, st = ref["gap"], ref["status"]
        assert gap[m["one_dir"]] == 4 and st[m["one_dir"]] == br.BOUNDARY                    # exactly one direction
        assert gap[m["opposite"]] == 2 and st[m["opposite"]] == br.BOUNDARY
        assert gap[m["low_boundary"]] == 4 and st[m["low_boundary"]] == br.BOUNDARY
        if k >= 4:                                                                           # (k = 3 uses three of the four arms)
            assert gap[m["cross"]] == 1 and st[m["cross"]] == br.INTERIOR                    # a gap of exactly 1: the test is >
            assert gap[m["coincident"]] == 3, (k, gap[m["coincident"]])
            assert nr.same_bits(gap[m["long_normal"]], gap[m["cross"]]) and nr.same_bits(gap[m["axis0"]], gap[m["cross"]])
            assert gap[m["low_neighbour"]] == (1 if mc < 0 else 2)                           # the low arm is no neighbour at the threshold
    S, nl = edge["S"], edge["nl"][-1.0]
    two = br.boundaries(S, nl=nl, radius=bs.R_EDGE, k=8, min_neighbors=bs.MIN_NEIGHBORS, max_gap=2.0)
    assert two["status"][m["opposite"]] == br.INTERIOR and two["status"][m["one_dir"]] == br.BOUNDARY
    low = br.boundaries(S, nl=nl, radius=bs.R_EDGE, k=8, min_neighbors=bs.MIN_NEIGHBORS, max_gap=0.75)
    assert low["status"][m["cross"]] == br.BOUNDARY


def test_coincident_directions_and_every_branch_of_turn(edge):
    S, m = edge["S"], edge["marks"]
    count, D, R = edge["nl"][-1.0]
    c = m["coincident"]
    e1, e2, _ = br.frame(S[c, 8:11])
    xy = [br.project(e1, e2, S[c, :3], S[R[c, j], :3]) for j in range(4)]
    assert count[c] == 4 and D[c, 0] == D[c, 1] and R[c, 0] < R[c, 1] and all(d for _, _, d in xy)
    same = [j for j in range(4) if br.turn(*xy[0][:2], *xy[j][:2], False) == 0.0]
    assert same == [0, 1, 3]                                                                 # slots 1, 2 and 4 are one direction
    g = []
    for j in range(4):
        g.append(min(br.turn(*xy[j][:2], *xy[i][:2], i < j) for i in range(4) if i != j))
    assert g == [0.0, 0.0, 3.0, 1.0]                                                         # only the highest slot of the group looks past it
    q = m["quadrants"]
    e1, e2, _ = br.frame(S[q, 8:11])
    xy = [br.project(e1, e2, S[q, :3], S[R[q, j], :3]) for j in range(4)]
    seen = set()
    for j in range(4):
        for i in range(4):
            if i != j:
                d = xy[j][0] * xy[i][0] + xy[j][1] * xy[i][1]
                cc = xy[j][0] * xy[i][1] - xy[j][1] * xy[i][0]
                ci = xy[i][0] * xy[j][1] - xy[i][1] * xy[j][0]
                assert cc == -ci                                                             # exactly antisymmetric
                seen.add("first" if d >= 0 and cc >= 0 else "second" if d < 0 and cc >= 0 else "third" if d < 0 else "fourth")
    assert seen == {"first", "second", "third", "fourth"}
    # the two branches no f32 position reaches (|x| and |y| of a direction lie in [2^-150, 2^130]: no product under- or overflows)
    assert br.turn(1e-200, 0.0, 0.0, 1e-200, False) == 0.0 and br.turn(1e-200, 0.0, 0.0, 1e-200, True) == 4.0
    assert br.turn(1e200, 0.0, 1e200, 1e200, False) == 0.0 and br.turn(float("nan"), 0.0, 1.0, 1.0, False) == 0.0
    # the measure is monotone in the angle and hits the quarter turns exactly
    ang = np.linspace(0.01, 2 * math.pi - 0.01, 721)
    t = [br.turn(1.0, 0.0, math.cos(a), math.sin(a), False) for a in ang]
    assert all(a < b for a, b in zip(t, t[1:])) and 0 < t[0] and t[-1] < 4
    assert [br.turn(1.0, 0.0, x, y, False) for x, y in ((0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), (1.0, 1.0))] == [1.0, 2.0, 3.0, 0.5]


def test_every_axis_of_the_frame_and_its_ties(edge):
    S, m = edge["S"], edge["marks"]
    assert [br.frame(S[m[g], 8:11])[2] for g in ("axis0", "axis1", "axis2", "tie", "long_normal")] == [0, 1, 2, 0, 0]
    for g in ("axis0", "axis1", "axis2", "tie"):
        e1, e2, _ = br.frame(S[m[g], 8:11])
        h = S[m[g], 8:11].astype(np.float64)
        h /= np.linalg.norm(h)
        assert abs(np.dot(e1, h)) < 1e-15 and abs(np.dot(e2, h)) < 1e-15 and abs(np.dot(e1, e2)) < 1e-15
        assert np.allclose(np.cross(e1, e2) / np.dot(e1, e1), h, atol=1e-15)                  # right-handed about the normal: TURN is counter-clockwise seen along it
        ref = edge["refs"][(8, -1.0)]
        assert ref["status"][m[g]] in (br.INTERIOR, br.BOUNDARY) and 0 < ref["gap"][m[g]] < 4


def test_loops_leave_out_rows_below_min_conf(edge):
    m = edge["marks"]
    low = m["low_boundary"]
    ref = edge["refs"][(8, -1.0)]
    assert ref["label"][low] != br.LOOP_NONE and ref["size"][low] >= 1
    ref = edge["refs"][(8, THR)]
    assert ref["status"][low] == br.BOUNDARY and ref["label"][low] == br.LOOP_NONE and ref["size"][low] == 0
    b = ref["status"] == br.BOUNDARY
    assert np.array_equal(ref["label"] != br.LOOP_NONE, b & (edge["S"][:, 3] > F(THR))) and (ref["size"][ref["label"] == br.LOOP_NONE] == 0).all()
    # the loops are the components of the BOUNDARY nodes
    node = b & cr.nodes(edge["S"], None, THR)
    label, size = cr.labels_of(len(b), node, cr.edges(edge["S"], node, bs.R_EDGE))
    assert np.array_equal(label, ref["label"]) and np.array_equal(size, ref["size"])
    assert ref["result"]["loops"] == len(np.unique(label[node])) > 5 and ref["result"]["largest"] == size.max()


def test_every_k_sees_its_own_neighbourhood_and_every_status_occurs(edge):
    cloud = edge["marks"]["cloud"]
    seen = [edge["refs"][(k, -1.0)]["gap"][cloud] for k in bs.KS]
    for a, b in zip(seen, seen[1:]):
        assert not nr.same_bits(a, b)
    count = edge["nl"][-1.0][0]
    assert (count[cloud] < 8).any() and (count[cloud] > 16).any()
    for (k, mc), ref in edge["refs"].items():
        assert set(np.unique(ref["status"]).tolist()) == {br.NONE, br.INTERIOR, br.BOUNDARY, br.SPARSE, br.DEGENERATE} or k == 3     # (three neighbours leave more than a right angle)
        r = ref["result"]
        assert r["interior"] + r["boundary"] + r["sparse"] + r["degenerate"] == r["participants"] == len(edge["S"]) - 1
        st = ref["status"][cloud]
        print(k, mc, "cloud: interior", (st == br.INTERIOR).sum(), "boundary", (st == br.BOUNDARY).sum())
        assert (st == br.BOUNDARY).sum() > 10 and ((st == br.INTERIOR).sum() > 10 or k < 8)
    S = edge["S"]
    low = S[:, 3] < F(THR)
    assert 40 < low.sum() < 120
    assert not nr.same_bits(edge["refs"][(8, THR)]["gap"], edge["refs"][(8, -1.0)]["gap"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the plate: analytic verdicts, independent of any reference
# ---------------------------------------------------------------------------------------------------------------------------------------
def plate_expectation(marks, n, max_gap):
    """(gap, status, loops as a list of row arrays) of the plain plate by geometry alone"""
    gap = np.zeros(n, F)
    for kind, g in bs.PLATE_GAPS.items():
        gap[marks[kind]] = g
    status = np.where(gap > F(max_gap), br.BOUNDARY, br.INTERIOR).astype(np.uint8)
    b = status == br.BOUNDARY
    return gap, status, [marks["outer_rim"][b[marks["outer_rim"]]], marks["hole_rim"][b[marks["hole_rim"]]]]


@pytest.mark.parametrize("max_gap", (1.0, 0.75))
def test_the_plates_analytic_verdicts_and_loops_are_the_references(max_gap):
    S, m = bs.plate_scene()
    n = len(S)
    assert [len(m[k]) for k in ("inner", "edge", "convex", "concave", "beside")] == [50, 42, 4, 4, 8] and n == 108
    gap, status, loops = plate_expectation(m, n, max_gap)
    ref = br.boundaries(S, max_gap=max_gap, **bs.PLATE_KW)
    assert nr.same_bits(ref["gap"], gap) and np.array_equal(ref["status"], status)
    assert (ref["count"] == [dict(inner=8, edge=5, convex=3, concave=7, beside=6)[k] for r in range(n) for k in bs.PLATE_GAPS if r in m[k]]).all()
    # BOUNDARY is exactly the two rims at max_gap 1 without the hole's concave corners (G = 1, and the test is >), with them at 0.75
    rims = np.sort(np.concatenate([m["outer_rim"], m["hole_rim"]]))
    want = rims if max_gap < 1 else np.setdiff1d(rims, m["concave"])
    assert np.array_equal(br.listed(ref, br.BOUNDARY), want)
    assert [len(l) for l in loops] == ([40, 18] if max_gap < 1 else [40, 14])
    for rows in loops:
        assert (ref["label"][rows] == rows.min()).all() and (ref["size"][rows] == len(rows)).all()
    assert ref["result"]["loops"] == 2 and ref["result"]["largest"] == 40 and (ref["label"][status != br.BOUNDARY] == br.LOOP_NONE).all()
    # one min_size / max_size setting separates the two loops
    for kw, acc in ((dict(min_size=20), 0), (dict(max_size=20), 1)):
        r = br.boundaries(S, max_gap=max_gap, **bs.PLATE_KW, **kw)
        assert np.array_equal(br.listed(r, br.LOOPS_ACCEPTED), loops[acc]) and np.array_equal(br.listed(r, br.LOOPS_REJECTED), loops[1 - acc])
        assert r["result"]["accepted"] == 1 and r["result"]["loops"] == 2


def test_the_jittered_plate_keeps_its_rims():
    S, m = bs.plate_scene(jitter=0.1)
    ref = br.boundaries(S, **bs.PLATE_KW)
    b = ref["status"] == br.BOUNDARY
    # every straight edge is still found, most inner rows are still inner, a corner that lost one of its three neighbours is SPARSE, and no
    # two gaps are the same double any more
    assert b[m["edge"]].all() and b[m["beside"]].all() and b[m["inner"]].mean() < 0.25 and len(np.unique(ref["gap"])) > 100
    assert set(np.unique(ref["status"][m["convex"]]).tolist()) == {br.BOUNDARY, br.SPARSE}


def test_the_closed_sphere_has_no_boundary_and_the_hemisphere_one_loop():
    """conditions on the inputs, shown on the reference alone: the parameters of boundaryscenes.SPHERE were chosen for them"""
    S, _ = bs.sphere_scene()
    ref = br.boundaries(S, **bs.SPHERE)
    assert ref["result"]["boundary"] == 0 and ref["result"]["interior"] == len(S) == 2048 and ref["result"]["loops"] == 0
    H, radial = bs.hemisphere_scene()
    ref = br.boundaries(H, **bs.SPHERE)
    b = ref["status"] == br.BOUNDARY
    assert ref["result"]["loops"] == 1 and ref["result"]["largest"] == b.sum() >= 20 and ref["result"]["sparse"] == 0
    assert radial[b, 2].max() < 0.06 and radial[~b, 2].max() > 0.99                          # the loop is the rim: within 3.5 degrees of the equator
    assert len(np.unique(np.floor(np.degrees(np.arctan2(radial[b, 1], radial[b, 0])) / 90.0))) == 4       # ... all the way round


# ---------------------------------------------------------------------------------------------------------------------------------------
# ef_boundary_gap.hpp on the host
# ---------------------------------------------------------------------------------------------------------------------------------------
def gap_cases(edge):
    """(m, p, neighbours): every judged row of the edge scene at two k, the plates, and seeded random neighbourhoods at several scales"""
    cases = []
    S, (count, D, R) = edge["S"], edge["nl"][-1.0]
    for k in (5, 16):
        for s in np.nonzero(nr.participants(S) & (count >= 1))[0]:
            cases.append((S[s, 8:11], S[s, :3], [S[int(R[s, j]), :3] for j in range(int(min(count[s], k)))]))
    for jitter in (0.0, 0.1):
        P, _ = bs.plate_scene(jitter=jitter)
        c, _, Rp = nr.neighbour_lists(P, bs.R_PLATE)
        for s in range(len(P)):
            cases.append((P[s, 8:11], P[s, :3], [P[int(Rp[s, j]), :3] for j in range(int(min(c[s], 8)))]))
    rng = np.random.default_rng(5)
    for i in range(3000):
        c = int(rng.integers(0, 17))
        scale = 10.0 ** rng.uniform(-6, 3)
        p = (rng.normal(size=3) * scale * 10).astype(F)
        nb = (p + rng.normal(size=(c, 3)) * scale * rng.uniform(0.01, 1.0, 3)).astype(F)
        if i % 7 == 0 and c > 2:
            nb[1] = nb[0]                                                    # coincident neighbours
        if i % 11 == 0 and c > 0:
            nb[c - 1] = p                                                    # a neighbour on the row itself: no direction
        m = rng.normal(size=3) * 10.0 ** rng.uniform(-20, 10)
        if i % 13 == 0:
            m[rng.integers(0, 3)] = 0.0
        if i % 17 == 0:
            m[:] = np.round(m / np.abs(m).max())                            # ties among the |h_i|
        cases.append((m.astype(F), p, list(nb)))
    z = np.zeros(3, F)
    one = np.array([1, 0, 0], F)
    cases += [(z, z, [one]), (np.array([np.nan, 0, 1], F), z, [one]), (np.array([np.inf, 0, 1], F), z, [one]), (np.array([1e-30, 0, 0], F), z, [np.array([0, 1, 0], F)]),
              (np.array([0, 0, 1], F), z, []), (np.array([0, 0, 1], F), z, [np.array([np.inf, 0, 0], F), one]),
              (np.array([3e38, 3e38, 3e38], F), z, [one, -one]), (np.array([0, 0, 1], F), z, [np.array([1e-45, 0, 0], F), np.array([0, 3e38, 0], F)])]
    return cases


@pytest.mark.parametrize("sanitized", (False, True), ids=("plain", "asan+ubsan"))
def test_the_gap_compiled_for_the_host_equals_the_reference_bit_for_bit(tmp_path, edge, sanitized):
    src = os.path.join(ROOT, "tests", "boundary_gap_main.cpp")
    cmd = ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "elasticfusion_amd", "csrc")]
    if sanitized:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        trial = tmp_path / "trial.cpp"
        trial.write_text("int main() { return 0; }\n")
        ok = subprocess.run(cmd + [str(trial), "-o", str(tmp_path / "trial")], capture_output=True).returncode == 0
        if not (ok and subprocess.run([str(tmp_path / "trial")], capture_output=True).returncode == 0):
            pytest.skip("this toolchain cannot build or run a program with -fsanitize=address,undefined: the plain case has run")
    exe = tmp_path / "boundary_gap"
    subprocess.run(cmd + [src, "-o", str(exe)], check=True)
    cases = gap_cases(edge)
    bits32 = lambda v: "%08x" % struct.unpack("<I", struct.pack("<f", float(v)))[0]
    bits64 = lambda v: "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    with np.errstate(all="ignore"):
        text = "".join(" ".join(["G", str(len(nb))] + [bits32(v) for v in list(m) + list(p) + [x for t in nb for x in t]]) + "\n" for m, p, nb in cases)
    rng = np.random.default_rng(9)
    turns = [tuple(rng.normal(size=4) * 10.0 ** rng.uniform(-3, 3)) + (int(i % 2),) for i in range(500)]
    turns += [(1.0, 0.0, 1.0, 0.0, 0), (1.0, 0.0, 2.0, 0.0, 1), (1.0, 0.0, -1.0, 0.0, 0), (-1.0, 0.0, 1.0, -0.0, 0), (0.0, -1.0, 0.0, 1.0, 1),
              (1e-200, 0.0, 0.0, 1e-200, 0), (1e-200, 0.0, 0.0, 1e-200, 1), (1e200, 0.0, 1e200, 1e200, 0), (float("nan"), 0.0, 1.0, 1.0, 0),
              (float("inf"), 0.0, 1.0, 1.0, 1)]
    text += "".join("T " + " ".join(bits64(v) for v in t[:4]) + " %d\n" % t[4] for t in turns)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases) + len(turns) and len(cases) > 3500
    seen = {"gap": 0, "degenerate": 0, "four": 0, "zero": 0}
    for i, ((m, p, nb), line) in enumerate(zip(cases, lines)):
        G = br.gap(m, p, nb)
        want = "1 %016x" % 0 if G is None else "0 " + bits64(G)
        assert line == want, (i, line, want, m, p, nb)
        seen["degenerate" if G is None else "gap"] += 1
        seen["four"] += G == 4.0
        seen["zero"] += G == 0.0
    for t, line in zip(turns, lines[len(cases):]):
        assert line == bits64(br.turn(t[0], t[1], t[2], t[3], bool(t[4]))), (t, line)
    print(seen)
    assert seen["gap"] > 3000 and seen["degenerate"] > 150 and seen["four"] > 100


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C ABI's refusals, the angle conversion and the binding
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    return api.lib()


def test_gap_from_angle_agrees_with_math_and_is_exact_at_the_quarter_turns(lib):
    from elasticfusion_amd import api
    assert api.boundary_gap(math.pi / 2) == 1.0 and api.boundary_gap(math.pi) == 2.0 and api.boundary_gap(1.5 * math.pi) == 3.0
    assert api.boundary_gap(math.pi / 4) == pytest.approx(0.5, abs=1e-15)
    for a in np.linspace(1e-6, 2 * math.pi - 1e-6, 2001):
        g = api.boundary_gap(float(a))
        assert abs(g - br.gap_from_angle(float(a))) <= 1e-12, a
        assert abs(api.boundary_angle(g) - a) <= 1e-12, a
    g = C.c_double(-7.0)
    for bad in (0.0, -1.0, 2 * math.pi, 7.0, float("nan"), float("inf")):
        assert lib.ef_boundary_gap_from_angle(bad, C.byref(g)) == -1 and b"angle" in lib.ef_last_error(None) and g.value == -7.0
    assert lib.ef_boundary_gap_from_angle(1.0, None) == -1 and b"null gap" in lib.ef_last_error(None)
    for bad in (0.0, 4.0, -1.0):
        with pytest.raises(ValueError):
            api.boundary_angle(bad)


def good_params(**kw):
    from elasticfusion_amd import api
    p = api.ef_boundary_params(radius=0.03, cell=0.03, min_conf=-1.0, k=12, min_neighbors=5, normal_source=0, line_ratio=1e-4, max_gap=1.0,
                               min_size=1, max_size=0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


NAN, INF = float("nan"), float("inf")
BAD = [(dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=NAN), "radius"), (dict(radius=INF), "radius"),
       (dict(cell=0.0), "cell"), (dict(cell=NAN), "cell"), (dict(cell=INF), "cell"), (dict(cell=1e-45), "cell"),
       (dict(radius=1.0, cell=0.01), "radius / cell"), (dict(min_conf=NAN), "min_conf"),
       (dict(k=2, min_neighbors=2), "k must"), (dict(k=17), "k must"), (dict(k=0), "k must"),
       (dict(min_neighbors=1), "min_neighbors"), (dict(min_neighbors=13), "min_neighbors"), (dict(k=3, min_neighbors=4), "min_neighbors"),
       (dict(normal_source=2), "normal_source"), (dict(normal_source=-1), "normal_source"),
       (dict(line_ratio=NAN), "line_ratio"), (dict(line_ratio=-1e-6), "line_ratio"),
       (dict(max_gap=0.0), "max_gap"), (dict(max_gap=4.0), "max_gap"), (dict(max_gap=-1.0), "max_gap"), (dict(max_gap=NAN), "max_gap"),
       (dict(max_gap=INF), "max_gap")]


def test_every_refusal_names_its_argument_with_a_null_context(lib):
    from elasticfusion_amd import api
    EINVAL = -1
    cnt, rows = C.c_uint32(0), (C.c_uint32 * 4)()
    calls = {
        "ef_map_boundaries": lambda p, a: lib.ef_map_boundaries(None, p, a, None, None, None, None, None, 0, None),
        "ef_map_boundaries_dev": lambda p, a: lib.ef_map_boundaries_dev(None, p, a, None, None, None, None, None, 0, None),
        "ef_map_boundaries_select": lambda p, a: lib.ef_map_boundaries_select(None, p, a, api.BOUNDARY_BOUNDARY, rows, 4, C.byref(cnt), None),
        "ef_map_boundaries_select_dev": lambda p, a: lib.ef_map_boundaries_select_dev(None, p, a, api.BOUNDARY_LOOPS_REJECTED, rows, 4, C.byref(cnt), None),
    }

    def refused(rc, fn, word):
        msg = lib.ef_last_error(None).decode()
        assert rc == EINVAL and msg.startswith(fn + ":") and word in msg, (fn, word, rc, msg)

    for fn, call in calls.items():
        refused(call(None, None), fn, "null params")
        for change, word in BAD:
            refused(call(C.byref(good_params(**change)), None), fn, word)
        refused(call(C.byref(good_params(k=3, min_neighbors=2, line_ratio=0.0, max_gap=1e-30, normal_source=1)), None), fn, "null context")
        refused(call(C.byref(good_params(k=16, min_neighbors=16, radius=0.16, cell=0.01, max_gap=3.9999998, min_size=0, max_size=1)), None), fn, "null context")   # the limits themselves
        sel = api.ef_map_selection()
        lib.ef_default_map_selection(C.byref(sel))
        sel.tests = 0x8000
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "unknown bits")                        # what ef_map_select refuses
        sel.tests, sel.conf_min = api.SEL_CONF, NAN
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "NaN")
    p = C.byref(good_params())
    for fn in ("ef_map_boundaries_select", "ef_map_boundaries_select_dev"):
        call = getattr(lib, fn)
        for what in (0, 7, -1, -5):
            refused(call(None, p, None, what, rows, 4, C.byref(cnt), None), fn, "what")
        for what in (1, 2, 3, 4, 5, 6):
            refused(call(None, p, None, what, rows, 4, C.byref(cnt), None), fn, "null context")
        refused(call(None, p, None, 2, None, 4, C.byref(cnt), None), fn, "null rows")
        refused(call(None, p, None, 2, rows, 4, None, None), fn, "null count")
        refused(call(None, p, None, 2, None, 0, C.byref(cnt), None), fn, "null context")               # NULL rows with max_rows 0 is fine
    assert lib.ef_default_boundary_params(None, C.byref(good_params())) == EINVAL and b"null context" in lib.ef_last_error(None)


def test_the_new_structs_and_constants_are_the_headers():
    from elasticfusion_amd import accuracy, api
    structs = header_structs()
    for name in ("ef_boundary_params", "ef_boundary_result"):
        assert structs[name] == [f for f, _ in getattr(api, name)._fields_]
    assert C.sizeof(api.ef_boundary_params) == 40 and C.sizeof(api.ef_boundary_result) == 40
    assert api.ef_boundary_params.normal_source.offset == 20 and api.ef_boundary_params.max_gap.offset == 28 and api.ef_boundary_result.status.offset == 36
    want = defines("BOUNDARY")
    mine = {k: v for k, v in vars(api).items() if k.startswith("BOUNDARY") and isinstance(v, int)}
    assert want == dict(BOUNDARY_STORED=0, BOUNDARY_ESTIMATED=1, BOUNDARY_NONE=0, BOUNDARY_INTERIOR=1, BOUNDARY_BOUNDARY=2, BOUNDARY_SPARSE=3,
                        BOUNDARY_DEGENERATE=4, BOUNDARY_LOOPS_ACCEPTED=5, BOUNDARY_LOOPS_REJECTED=6) and mine == want, (mine, want)
    assert (br.STORED, br.ESTIMATED, br.NONE, br.INTERIOR, br.BOUNDARY, br.SPARSE, br.DEGENERATE, br.LOOPS_ACCEPTED, br.LOOPS_REJECTED) == (
        api.BOUNDARY_STORED, api.BOUNDARY_ESTIMATED, api.BOUNDARY_NONE, api.BOUNDARY_INTERIOR, api.BOUNDARY_BOUNDARY, api.BOUNDARY_SPARSE,
        api.BOUNDARY_DEGENERATE, api.BOUNDARY_LOOPS_ACCEPTED, api.BOUNDARY_LOOPS_REJECTED)
    assert br.LOOP_NONE == api.COMPONENT_NONE
    for name in ("boundaryParams", "boundaries", "boundariesDevice", "boundarySelect", "boundarySelectDevice"):
        assert callable(getattr(api.ElasticFusion, name))
    assert callable(accuracy.map_boundaries) and callable(api.boundary_angle) and callable(api.boundary_gap)
    assert api.signatures()["ef_boundary_gap_from_angle"] == (C.c_int, [C.c_double, C.c_void_p])
    assert br.DEFAULTS == dict(radius=0.03, min_conf=-1.0, k=12, min_neighbors=5, normal_source=0, line_ratio=1e-4, max_gap=1.0, min_size=1, max_size=0)
    src = open(os.path.join(ROOT, "elasticfusion_amd", "csrc", "ef_boundary_gap.hpp")).read()
    assert "boundary_gap(" in src and "boundary_turn(" in src
