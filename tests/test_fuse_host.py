"""CPU-only checks of the fuse entry points (include/ef_hip.h, "Fuse surfels"): the section is C99, the library and the Python mirror carry it
with structs of the same size, every EF_EINVAL case that needs no context is refused before any GPU work (in a child process, so that a crash
would be a failed test and not a dead session), and the numpy restatement of tests/fuseref.py agrees with cases merged by hand and has the
properties the header states."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np

import fuseref as fr
import insertref as ir
from queryref import MISS, assert_bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("ef_default_fuse_params", "ef_map_fuse", "ef_map_fuse_dev")
F = np.float32


def test_header_declares_the_fuse_section_as_c99(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(r'''
#include <stdio.h>
#include "ef_hip.h"
int main(void) {
  int (*a)(ef_ctx*, ef_fuse_params*) = ef_default_fuse_params;
  int (*b)(ef_ctx*, const float*, uint32_t, const double*, const ef_fuse_params*, ef_fuse_result*, uint32_t*, uint32_t*, uint8_t*) = ef_map_fuse;
  int (*c)(ef_ctx*, const float*, uint32_t, const double*, const ef_fuse_params*, ef_fuse_result*, uint32_t*, uint32_t*, uint8_t*) = ef_map_fuse_dev;
  ef_fuse_params p;
  ef_fuse_result r;
  p.min_separation = 0.01f; p.min_conf = -1.f; p.min_normal_cos = 0.5f; p.append = 1; p.init_time = EF_INSERT_KEEP; p.last_time = 0;
  r.fused = r.absorbed = r.weightless = r.novel = r.skipped = r.inserted = r.count_after = 0u;
  printf("%d %u %u %d %u %d\n", a != 0 && b != 0 && c != 0, (unsigned)sizeof(p), (unsigned)sizeof(r), p.init_time, r.fused,
         EF_FUSE_SKIPPED + EF_FUSE_NOVEL + EF_FUSE_WEIGHTLESS + EF_FUSE_ABSORBED + EF_FUSE_FUSED + EF_FUSE_INSERTED);
  return 0;
}
''')
    exe = str(tmp_path / "decl")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe + ".o"],
                   check=True)
    hdr = open(os.path.join(ROOT, "include", "ef_hip.h")).read()
    for name, v in (("SKIPPED", fr.SKIPPED), ("NOVEL", fr.NOVEL), ("WEIGHTLESS", fr.WEIGHTLESS), ("ABSORBED", fr.ABSORBED), ("FUSED", fr.FUSED),
                    ("INSERTED", fr.INSERTED)):
        assert f"#define EF_FUSE_{name:<10} {v}\n" in hdr, name


def test_library_and_python_mirror_carry_the_entry_points():
    import ctypes as C
    import inspect
    from elasticfusion_amd import accuracy, api, build
    build.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in ENTRY:
        assert f" {name}\n" in syms, name
    for m in ("fuseParams", "fuseSurfels"):
        assert callable(getattr(api.ElasticFusion, m, None)), m
    assert inspect.signature(accuracy.merge_session).parameters["fuse"].default is False
    assert (api.FUSE_SKIPPED, api.FUSE_NOVEL, api.FUSE_WEIGHTLESS, api.FUSE_ABSORBED, api.FUSE_FUSED, api.FUSE_INSERTED) == \
        (fr.SKIPPED, fr.NOVEL, fr.WEIGHTLESS, fr.ABSORBED, fr.FUSED, fr.INSERTED)
    # the C layouts: six and seven 4-byte fields, no padding
    assert C.sizeof(api.ef_fuse_params) == 24 and C.sizeof(api.ef_fuse_result) == 28
    assert [f for f, _ in api.ef_fuse_params._fields_] == ["min_separation", "min_conf", "min_normal_cos", "append", "init_time", "last_time"]
    assert [f for f, _ in api.ef_fuse_result._fields_] == ["fused", "absorbed", "weightless", "novel", "skipped", "inserted", "count_after"]


def test_every_einval_case_is_refused_without_a_gpu():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    code = r'''
import ctypes as C
from elasticfusion_amd import api
L = api.lib()
u, p = C.c_uint32, C.c_void_p
PP, RP = C.POINTER(api.ef_fuse_params), C.POINTER(api.ef_fuse_result)
L.ef_map_fuse.argtypes = L.ef_map_fuse_dev.argtypes = [p, p, u, p, PP, RP, p, p, p]
L.ef_default_fuse_params.argtypes = [p, PP]
z = None
rec = (C.c_float * 48)()
rows = (C.c_uint32 * 8)()
out = (C.c_uint8 * 8)()
res = api.ef_fuse_result()
inf, nan = float("inf"), float("nan")
def show(name, case, rc):
    print(name, case, rc, (L.ef_last_error(None) or b"").decode().replace(" ", "_"), flush=True)
def par(**kw):
    q = api.ef_fuse_params(0.01, -1.0, 0.5, 1, 3, 3)
    for k, v in kw.items():
        setattr(q, k, v)
    return q
def T16(i, v):
    a = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    a[i] = v
    return (C.c_double * 16)(*a)
bad = [
    ("append_2", par(append=2)), ("append_negative", par(append=-1)),
    ("min_separation_zero", par(min_separation=0.0)), ("min_separation_negative", par(min_separation=-0.01)),
    ("min_separation_nan", par(min_separation=nan)), ("min_separation_inf", par(min_separation=inf)),
    ("min_conf_nan", par(min_conf=nan)), ("min_normal_cos_nan", par(min_normal_cos=nan)),
    ("init_time_below_keep", par(init_time=-2)), ("last_time_below_keep", par(last_time=-7)),
]
for name in ("ef_map_fuse", "ef_map_fuse_dev"):
    fn = getattr(L, name)
    for case, q in bad:
        show(name, case, fn(z, rec, 4, z, C.byref(q), C.byref(res), rows, rows, out))
    show(name, "null_params", fn(z, rec, 4, z, None, C.byref(res), rows, rows, out))
    show(name, "null_result", fn(z, rec, 4, z, C.byref(par()), None, rows, rows, out))
    show(name, "null_records", fn(z, z, 4, z, C.byref(par()), C.byref(res), rows, rows, out))
    show(name, "too_many_records", fn(z, rec, 1 << 28, z, C.byref(par()), C.byref(res), z, z, z))
    show(name, "T_nan", fn(z, rec, 4, T16(11, nan), C.byref(par()), C.byref(res), rows, rows, out))
    show(name, "T_inf", fn(z, rec, 4, T16(5, inf), C.byref(par(append=0)), C.byref(res), rows, rows, out))
    show(name, "null_context", fn(z, rec, 4, z, C.byref(par()), C.byref(res), z, z, z))
    show(name, "null_context_empty", fn(z, z, 0, z, C.byref(par(append=0)), C.byref(res), z, z, z))
show("ef_default_fuse_params", "null_context", L.ef_default_fuse_params(z, C.byref(par())))
'''
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 2 * (10 + 8) + 1, rows
    assert all(int(rc) == -1 for _, _, rc, _ in rows), rows   # EF_EINVAL, never a crash
    assert all(m.startswith(name + ":") for name, _, _, m in rows), rows
    expect = dict(append_2="append_must_be", append_negative="append_must_be", min_separation_zero="max_dist_must_be",
                  min_separation_negative="max_dist_must_be", min_separation_nan="max_dist_must_be", min_separation_inf="max_dist_must_be",
                  min_conf_nan="min_conf_is_NaN", min_normal_cos_nan="min_normal_cos_is_NaN", init_time_below_keep="EF_INSERT_KEEP",
                  last_time_below_keep="EF_INSERT_KEEP", null_params="null_params", null_result="null_result", null_records="null_surfels12",
                  too_many_records="EF_INSERT_MAX_RECORDS", T_nan="T_has_a_non-finite", T_inf="T_has_a_non-finite", null_context="null_context",
                  null_context_empty="null_context")
    for name, case, _, m in rows:
        assert expect[case] in m, (name, case, m)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference against cases merged by hand
# ---------------------------------------------------------------------------------------------------------------------------------------
def f32(x):
    """one rounding to float32 of an exactly known value (a Fraction of float32 operands: product, sum or quotient)"""
    if isinstance(x, Fraction):
        lo = F(x.numerator / x.denominator)                       # within a float of the answer: pick the nearest of it and its neighbours
        best = min((lo, np.nextafter(lo, F(np.inf)), np.nextafter(lo, F(-np.inf))),
                   key=lambda c: (abs(Fraction(float(c)) - x), int(c.view(np.uint32)) & 1))
        return F(best)
    return F(x)


def fr_(x):
    return Fraction(float(F(x)))


def avg_by_hand(ck, a, old, new):
    """((c_k*old) + (a*new)) / (c_k + a), every operation exact then rounded once"""
    num = f32(fr_(f32(fr_(ck) * fr_(old))) + fr_(f32(fr_(a) * fr_(new))))
    return f32(fr_(num) / fr_(f32(fr_(ck) + fr_(a))))


def row(pos, conf, colour, normal, radius, t0=1.0, t1=2.0, idbits=0):
    s = np.zeros(12, F)
    s[:3], s[3], s[4], s[6], s[7], s[8:11], s[11] = pos, conf, colour, t0, t1, normal, radius
    s[5:6].view(np.uint32)[0] = idbits
    return s


def one_pair(colour_s=0x204060, colour_r=0x406181, radius_r=0.004, last_time=9, ck=3.0, a=1.25):
    S = np.array([row((0.125, -0.25, 0.5), ck, colour_s, (0.0, 0.6, 0.8), 0.005, idbits=41)], F)
    R = np.array([row((0.126, -0.2495, 0.5012), a, colour_r, (0.1, 0.5, 0.85), radius_r, t0=5.0, t1=7.0, idbits=99)], F)
    prm = fr.default_params(0, min_normal_cos=-1.0, append=0, last_time=last_time)
    return S, R, prm


def test_one_pair_merged_by_hand():
    S, R, prm = one_pair()
    got = fr.fuse(S, R, None, prm)
    assert got["result"] == dict(fused=1, absorbed=0, weightless=0, novel=0, skipped=0, inserted=0, count_after=1)
    assert got["outcome"].tolist() == [fr.FUSED] and got["match_row"].tolist() == [0] and got["new_row"].tolist() == [MISS]
    s, r, ck, a = S[0], R[0], S[0, 3], R[0, 3]
    want = s.copy()
    for j in range(3):
        want[j] = avg_by_hand(ck, a, s[j], r[j])
    v = [avg_by_hand(ck, a, s[8 + j], r[8 + j]) for j in range(3)]
    dot = f32(fr_(f32(fr_(v[2]) * fr_(v[2]))) + fr_(f32(fr_(f32(fr_(v[1]) * fr_(v[1]))) + fr_(f32(fr_(v[0]) * fr_(v[0]))))))
    rn = F(1.0) / np.sqrt(dot)                                     # (float32 sqrt and divide are correctly rounded)
    for j in range(3):
        want[8 + j] = f32(fr_(v[j]) * fr_(rn))
    want[11] = avg_by_hand(ck, a, s[11], r[11])
    want[3] = f32(fr_(ck) + fr_(a))
    rgb = 0
    for sh in (16, 8, 0):
        co, cn = f32(Fraction((0x204060 >> sh) & 0xFF, 255)), f32(Fraction((0x406181 >> sh) & 0xFF, 255))
        mean = f32(fr_(avg_by_hand(ck, a, co, cn)) * 255)
        q = int(abs(fr_(mean)) + Fraction(1, 2))                   # half away from zero (the mean is positive)
        rgb = (rgb << 8) + q
    want[4] = F(rgb)
    want[7] = F(9)
    assert_bits_equal(got["map"][0], want, "the merged row")
    assert got["map"][0, 5:6].view(np.uint32)[0] == 41 and got["map"][0, 6] == 1.0, "the ID lane and the creation time are untouched"


def test_the_radius_gate_at_its_edge():
    bound = (F(1.0) + F(0.5)) * F(0.005)
    for radius_r, full in ((np.nextafter(bound, F(0)), True), (bound, False), (np.nextafter(bound, F(1)), False)):
        S, R, prm = one_pair(radius_r=radius_r)
        m = fr.fuse(S, R, None, prm)["map"][0]
        assert m[3] == S[0, 3] + R[0, 3] and m[7] == 9, "confidence and time change on both sides"
        rest = [0, 1, 2, 4, 5, 6, 8, 9, 10, 11]
        same = (m[rest].view(np.uint32) == S[0, rest].view(np.uint32)).all()
        assert same == (not full), (float(radius_r), full)
        if full:
            assert m[0] != S[0, 0] and m[11] != S[0, 11] and m[4] != S[0, 4]


def test_colour_rounds_half_away_from_zero():
    # equal weights, channels 0 and 1: the mean is 0.5 / 255, times 255 exactly 0.5 in float32 -> 1 (numpy's rint gives 0); 0 and 5 -> 2.5 -> 3 (rint: 2)
    S, R, prm = one_pair(colour_s=0x000000, colour_r=0x010005, ck=2.0, a=2.0)
    for ch, (o, n) in enumerate(((0, 1), (0, 0), (0, 5))):
        mean = avg_by_hand(2.0, 2.0, f32(Fraction(o, 255)), f32(Fraction(n, 255)))
        assert fr_(f32(fr_(mean) * 255)) == Fraction(o + n, 2), ch
    m = fr.fuse(S, R, None, prm)["map"][0]
    assert int(m[4]) == 0x010003, hex(int(m[4]))
    assert int(np.rint(F(0.5))) == 0 and int(np.rint(F(2.5))) == 2 and fr.int_or_indefinite(F([0.5, 2.5, -0.5, -2.5])).tolist() == \
        [1, 3, 0xFFFFFFFF, 0xFFFFFFFD]
    # a mean outside int (c_k + a == 0: 0 / 0) gives INT_MIN per channel, and the shifts wrap
    assert fr.int_or_indefinite(F([np.nan, 2.0 ** 31, -2.0 ** 31, np.inf])).tolist() == [0x80000000, 0x80000000, 0x80000000, 0x80000000]
    S, R, prm = one_pair(ck=-1.25)
    prm["min_conf"] = -2.0                                       # (a surfel is eligible iff its confidence is ABOVE min_conf)
    m = fr.fuse(S, R, None, prm)["map"][0]
    assert m[4] == F(-2147483648.0) and m[3] == 0 and not np.isfinite(m[0])
    # a stored 255 decodes to exactly 1
    assert [float(c[0]) for c in fr.decode(F([0xFF00FF]))] == [1.0, 0.0, 1.0]


def test_last_time_under_keep_is_the_records_own():
    S, R, prm = one_pair(last_time=fr.KEEP)
    assert fr.fuse(S, R, None, prm)["map"][0, 7] == 7.0
    S, R, prm = one_pair(last_time=fr.KEEP, radius_r=0.01)       # the short branch too
    m = fr.fuse(S, R, None, prm)["map"][0]
    assert m[7] == 7.0 and m[0] == S[0, 0]
    S, R, prm = one_pair(last_time=0)
    assert fr.fuse(S, R, None, prm)["map"][0, 7] == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# the election
# ---------------------------------------------------------------------------------------------------------------------------------------
def election_scene():
    """60 surfels on a grid; 400 records within 4 mm of them (so several per surfel), some at bit-identical positions (equal d2), a few
    weightless, a few far away, one non-finite"""
    rng = np.random.default_rng(11)
    i = np.arange(60)
    S = np.zeros((60, 12), F)
    S[:, 0], S[:, 1], S[:, 2] = 0.1 * (i % 10), 0.1 * (i // 10), 0.5
    S[:, 3], S[:, 4], S[:, 6], S[:, 7], S[:, 10], S[:, 11] = rng.uniform(0, 9, 60), rng.integers(0, 1 << 24, 60), 1, 2, 1, 0.005
    R = np.zeros((400, 12), F)
    who = rng.integers(0, 60, 400)
    R[:, :3] = S[who, :3] + rng.uniform(-0.004, 0.004, (400, 3)).astype(F)
    R[200:260, :3] = R[100:160, :3]                                # the same position twice: equal d2 on the same row
    R[:, 3], R[:, 4], R[:, 6], R[:, 7], R[:, 10] = rng.uniform(0.1, 12, 400), rng.integers(0, 1 << 24, 400), 3, 4 + np.arange(400) % 5, 1
    R[:, 11] = rng.uniform(0.003, 0.009, 400)
    R[300:310, 3] = (0, -1, np.inf, np.nan, -0.0, 0, -np.inf, np.nan, 0, -2)
    R[310:330, 2] += 1.0
    R[330, 1] = np.nan
    return S, R


def test_the_election_is_a_total_order():
    S, R = election_scene()
    prm = fr.default_params(6, append=1)
    base = fr.fuse(S, R, None, prm)
    res = base["result"]
    assert res["fused"] > 40 and res["absorbed"] > 200 and res["weightless"] == 10 and res["novel"] == 20 and res["skipped"] == 1
    assert res["fused"] + res["absorbed"] + res["weightless"] + res["novel"] + res["skipped"] == 400
    p = ir.move(R, None)[0]
    comp = np.isin(base["outcome"], (fr.FUSED, fr.ABSORBED))
    d2 = np.full(400, np.inf, F)
    d2[comp] = fr.d2_of(p[comp], S[base["match_row"][comp].astype(np.int64), :3])
    # exactly one winner per row that has a competitor, and it is the minimum of (d2, index)
    for s in np.unique(base["match_row"][comp]):
        c = np.nonzero(comp & (base["match_row"] == s))[0]
        w = c[np.lexsort((c, d2[c]))][0]
        assert base["outcome"][w] == fr.FUSED and (base["outcome"][c[c != w]] == fr.ABSORBED).all()
    tied = [s for s in np.unique(base["match_row"][comp])
            if (lambda c: (d2[c] == d2[c].min()).sum() > 1)(np.nonzero(comp & (base["match_row"] == s))[0])]
    assert len(tied) > 5, "the scene has rows whose two nearest records are at equal d2"
    rng = np.random.default_rng(12)
    # any permutation: match_row, and every outcome but FUSED / ABSORBED among records at the winner's d2, go with their records
    perm = rng.permutation(400)
    q = fr.fuse(S, R[perm], None, prm)
    assert np.array_equal(q["match_row"], base["match_row"][perm])
    differ = q["outcome"] != base["outcome"][perm]
    assert differ.any(), "reversing a tie changes who is fused"
    for k in np.nonzero(differ)[0]:
        assert base["match_row"][perm[k]] in tied and {int(q["outcome"][k]), int(base["outcome"][perm[k]])} == {fr.FUSED, fr.ABSORBED}
    assert q["result"] == base["result"]
    # a permutation that keeps the relative order of records with equal d2 on the same row leaves the fused map as it is: sort by a random key
    # with the (row, d2) groups' members keeping their order
    key = rng.permutation(400)
    groups = {}
    for k in range(400):
        groups.setdefault((int(base["match_row"][k]), int(d2[k].view(np.uint32))) if comp[k] else ("alone", k), []).append(k)
    for g in groups.values():                                      # within a group the random keys are handed out in ascending order
        key[g] = np.sort(key[g])
    perm = np.argsort(key)
    assert not np.array_equal(perm, np.arange(400))
    q = fr.fuse(S, R[perm], None, prm)
    assert np.array_equal(q["outcome"], base["outcome"][perm])
    assert_bits_equal(q["map"][:60], base["map"][:60], "the fused rows")
    # (the appended tail follows the input order: the same rows, permuted)
    assert_bits_equal(q["map"][q["new_row"][q["new_row"] != MISS]], base["map"][base["new_row"][perm][q["new_row"] != MISS]], "the appended rows")


def test_the_append_is_the_inserts():
    S, R = election_scene()
    w = 0.01
    T = np.array([[np.cos(w), -np.sin(w), 0, 0.001], [np.sin(w), np.cos(w), 0, -0.002], [0, 0, 1, 0.0005], [0, 0, 0, 1]])
    for times in ((fr.KEEP, fr.KEEP), (5, 8)):
        prm = fr.default_params(0, append=1, init_time=times[0], last_time=times[1])
        f = fr.fuse(S, R, T, prm)
        i = ir.insert(S, R, T, fr.as_insert(prm))
        assert np.array_equal(f["new_row"], i["new_row"]) and np.array_equal(f["match_row"], i["match_row"])
        assert_bits_equal(f["map"][60:], i["map"][60:], "the appended tail")
        assert f["result"]["inserted"] == i["result"]["inserted"] == f["result"]["novel"] and f["result"]["skipped"] == i["result"]["skipped"]
        assert f["result"]["fused"] + f["result"]["absorbed"] + f["result"]["weightless"] == i["result"]["duplicates"]
        assert (f["outcome"][i["new_row"] != MISS] == fr.INSERTED).all()
        # append = 0: the same fused rows, nothing appended, NOVEL in INSERTED's place
        g = fr.fuse(S, R, T, dict(prm, append=0))
        assert len(g["map"]) == 60 and (g["new_row"] == MISS).all() and g["result"]["inserted"] == 0 and g["result"]["count_after"] == 60
        assert_bits_equal(g["map"], f["map"][:60], "the fused rows")
        assert np.array_equal(np.where(g["outcome"] == fr.NOVEL, fr.INSERTED, g["outcome"]), f["outcome"])
        # rows that are nobody's match keep their bits
        quiet = np.setdiff1d(np.arange(60), f["match_row"][f["match_row"] != MISS])
        assert_bits_equal(f["map"][quiet], S[quiet], "unmatched rows")
    # capacity: refused as a whole, every count still reported
    c = fr.fuse(S, R, T, prm, capacity=60 + f["result"]["novel"] - 1)
    assert c["refused"] and c["result"] == dict(f["result"], count_after=60) and c["new_row"] is None
    assert_bits_equal(c["map"], S, "a refused fuse leaves the map")
