"""CPU-only checks of the insert entry points (include/ef_hip.h, "Insert surfels"): the section is C99, the library and the Python mirror carry
it with structs of the same size, every EF_EINVAL case is refused before any GPU work (in a child process, so that a crash would be a failed
test and not a dead session), and the numpy restatement of tests/insertref.py has the properties the header states."""
import os
import subprocess
import sys

import numpy as np

import insertref as ir
from queryref import MISS, assert_bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("ef_default_insert_params", "ef_map_insert", "ef_map_insert_dev")
F = np.float32


def test_header_declares_the_insert_section_as_c99(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(r'''
#include <stdio.h>
#include "ef_hip.h"
int main(void) {
  int (*a)(ef_ctx*, ef_insert_params*) = ef_default_insert_params;
  int (*b)(ef_ctx*, const float*, uint32_t, const double*, const ef_insert_params*, ef_insert_result*, uint32_t*, uint32_t*) = ef_map_insert;
  int (*c)(ef_ctx*, const float*, uint32_t, const double*, const ef_insert_params*, ef_insert_result*, uint32_t*, uint32_t*) = ef_map_insert_dev;
  ef_insert_params p;
  ef_insert_result r;
  p.gate = 1; p.min_separation = 0.01f; p.min_conf = -1.f; p.min_normal_cos = 0.5f; p.init_time = EF_INSERT_KEEP; p.last_time = 0;
  r.inserted = r.duplicates = r.skipped = r.count_after = 0u;
  printf("%d %u %u %d %u\n", a != 0 && b != 0 && c != 0, (unsigned)sizeof(p), (unsigned)sizeof(r), p.init_time, r.inserted);
  return 0;
}
''')
    exe = str(tmp_path / "decl")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe + ".o"],
                   check=True)
    hdr = open(os.path.join(ROOT, "include", "ef_hip.h")).read()
    assert "#define EF_INSERT_KEEP (-1)" in hdr and ir.KEEP == -1


def test_library_and_python_mirror_carry_the_entry_points():
    import ctypes as C
    from elasticfusion_amd import accuracy, api, build
    build.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in ENTRY:
        assert f" {name}\n" in syms, name
    for m in ("insertParams", "insertSurfels"):
        assert callable(getattr(api.ElasticFusion, m, None)), m
    assert callable(accuracy.merge_session)
    assert api.INSERT_KEEP == ir.KEEP and api.ROW_NONE == MISS
    # the C layouts: six and four 4-byte fields, no padding
    assert C.sizeof(api.ef_insert_params) == 24 and C.sizeof(api.ef_insert_result) == 16
    assert [f for f, _ in api.ef_insert_params._fields_] == ["gate", "min_separation", "min_conf", "min_normal_cos", "init_time", "last_time"]
    assert [f for f, _ in api.ef_insert_result._fields_] == ["inserted", "duplicates", "skipped", "count_after"]


def test_every_einval_case_is_refused_without_a_gpu():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    code = r'''
import ctypes as C
from elasticfusion_amd import api
L = api.lib()
u, p = C.c_uint32, C.c_void_p
PP, RP = C.POINTER(api.ef_insert_params), C.POINTER(api.ef_insert_result)
L.ef_map_insert.argtypes = L.ef_map_insert_dev.argtypes = [p, p, u, p, PP, RP, p, p]
L.ef_default_insert_params.argtypes = [p, PP]
z = None
rec = (C.c_float * 48)()
rows = (C.c_uint32 * 8)()
res = api.ef_insert_result()
inf, nan = float("inf"), float("nan")
def show(name, case, rc):
    print(name, case, rc, (L.ef_last_error(None) or b"").decode().replace(" ", "_"), flush=True)
def par(**kw):
    q = api.ef_insert_params(1, 0.01, -1.0, 0.5, 3, 3)
    for k, v in kw.items():
        setattr(q, k, v)
    return q
def T16(i, v):
    a = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    a[i] = v
    return (C.c_double * 16)(*a)
bad = [
    ("gate_2", par(gate=2)), ("gate_negative", par(gate=-1)),
    ("min_separation_zero", par(min_separation=0.0)), ("min_separation_negative", par(min_separation=-0.01)),
    ("min_separation_nan", par(min_separation=nan)), ("min_separation_inf", par(min_separation=inf)),
    ("min_conf_nan", par(min_conf=nan)), ("min_normal_cos_nan", par(min_normal_cos=nan)),
    ("init_time_below_keep", par(init_time=-2)), ("last_time_below_keep", par(last_time=-7)),
    ("init_time_below_keep_gate_off", par(gate=0, init_time=-2)),
]
for name in ("ef_map_insert", "ef_map_insert_dev"):
    fn = getattr(L, name)
    for case, q in bad:
        show(name, case, fn(z, rec, 4, z, C.byref(q), C.byref(res), rows, rows))
    show(name, "null_params", fn(z, rec, 4, z, None, C.byref(res), rows, rows))
    show(name, "null_result", fn(z, rec, 4, z, C.byref(par()), None, rows, rows))
    show(name, "null_records", fn(z, z, 4, z, C.byref(par()), C.byref(res), rows, rows))
    show(name, "too_many_records", fn(z, rec, 1 << 28, z, C.byref(par(gate=0)), C.byref(res), z, z))
    show(name, "T_nan", fn(z, rec, 4, T16(11, nan), C.byref(par()), C.byref(res), rows, rows))
    show(name, "T_inf", fn(z, rec, 4, T16(5, inf), C.byref(par(gate=0)), C.byref(res), rows, rows))
    show(name, "null_context", fn(z, rec, 4, z, C.byref(par()), C.byref(res), z, z))
    show(name, "null_context_gate_off", fn(z, rec, 4, T16(3, 0.5), C.byref(par(gate=0)), C.byref(res), z, z))
    show(name, "null_context_empty", fn(z, z, 0, z, C.byref(par()), C.byref(res), z, z))
    # with the gate off its three fields are neither read nor checked: NaN in them reaches the context check
    show(name, "gate_off_fields_unchecked", fn(z, rec, 4, z, C.byref(par(gate=0, min_separation=nan, min_conf=nan, min_normal_cos=nan)),
                                                C.byref(res), z, z))
show("ef_default_insert_params", "null_context", L.ef_default_insert_params(z, C.byref(par())))
'''
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 2 * (11 + 10) + 1, rows
    assert all(int(rc) == -1 for _, _, rc, _ in rows), rows   # EF_EINVAL, never a crash
    assert all(m.startswith(name + ":") for name, _, _, m in rows), rows
    expect = dict(gate_2="gate_must_be", gate_negative="gate_must_be", min_separation_zero="max_dist_must_be", min_separation_negative="max_dist_must_be",
                  min_separation_nan="max_dist_must_be", min_separation_inf="max_dist_must_be", min_conf_nan="min_conf_is_NaN",
                  min_normal_cos_nan="min_normal_cos_is_NaN", init_time_below_keep="EF_INSERT_KEEP", last_time_below_keep="EF_INSERT_KEEP",
                  init_time_below_keep_gate_off="EF_INSERT_KEEP", null_params="null_params", null_result="null_result",
                  null_records="null_surfels12", too_many_records="EF_INSERT_MAX_RECORDS", T_nan="T_has_a_non-finite", T_inf="T_has_a_non-finite", null_context="null_context",
                  null_context_gate_off="null_context", null_context_empty="null_context", gate_off_fields_unchecked="null_context")
    for name, case, _, m in rows:
        assert expect[case] in m, (name, case, m)


def small_scene():
    rng = np.random.default_rng(3)
    old = np.zeros((400, 12), F)
    old[:, :3] = rng.uniform(-1, 1, (400, 3))
    old[:, 3] = rng.uniform(0, 12, 400)
    old[:, 8:11] = (0, 0, 1)
    old[:, 11] = 0.005
    rec = np.zeros((300, 12), F)
    rec[:, :3] = rng.uniform(-1, 1, (300, 3))
    rec[:100, :3] = old[:100, :3] + F(0.001)              # near a map surfel, the same normal
    rec[100:150, :3] = old[100:150, :3] + F(0.001)        # near one, the opposite normal
    rec[:, 8:11] = (0, 0, 1)
    rec[100:150, 10] = -1
    rec[:, 3] = rng.uniform(0, 12, 300)
    rec[:, 4] = rng.integers(0, 1 << 24, 300)
    rec[:, 5] = np.arange(7, 307, dtype=np.uint32).view(F)     # old IDs: never stored
    rec[:, 6], rec[:, 7], rec[:, 11] = 4, 9, 0.004
    rec[200, 0], rec[201, 1], rec[202, 2] = np.nan, np.inf, -np.inf
    rec[203, :3] = (-0.0, 0.25, -0.0)
    rec[204, 8:11] = np.array([0x7FC01234, 0x80000000, 0xFFC00001], np.uint32).view(F)   # NaN payloads and -0 in a normal
    return old, rec


def test_the_reference_has_the_properties_the_header_states():
    old, rec = small_scene()
    # without T and without the gate: the stored rows are the records but for float 5 and the two times, bit for bit
    r = ir.insert(old, rec, None, ir.default_params(12, gate=0, init_time=ir.KEEP, last_time=ir.KEEP))
    fin = np.isfinite(rec[:, :3]).all(1)
    assert r["result"] == dict(inserted=int(fin.sum()), duplicates=0, skipped=3, count_after=400 + int(fin.sum()))
    assert_bits_equal(r["map"][:400], old, "the old rows")
    new = r["map"][400:]
    cols = [c for c in range(12) if c != 5]
    assert_bits_equal(np.ascontiguousarray(new[:, cols]), np.ascontiguousarray(rec[fin][:, cols]), "the records, all but the ID lane")
    assert (new[:, 5].view(np.uint32) == 0).all()
    assert (r["match_row"] == MISS).all() and (r["new_row"][~fin] == MISS).all()
    assert np.array_equal(r["new_row"][fin], 400 + np.arange(fin.sum(), dtype=np.uint32))
    # the times overridden: floats 6 and 7 alone differ from the above
    r2 = ir.insert(old, rec, None, ir.default_params(12, gate=0))
    assert (r2["map"][400:, 6] == 12).all() and (r2["map"][400:, 7] == 12).all()
    rest = [c for c in range(12) if c not in (6, 7)]
    assert_bits_equal(np.ascontiguousarray(r2["map"][:, rest]), np.ascontiguousarray(r["map"][:, rest]), "all but the times")
    # the gate: the 100 records beside a map surfel with its normal are duplicates; the 50 with the opposite normal only without the normal test
    g = ir.insert(old, rec, None, ir.default_params(12))
    assert g["result"]["duplicates"] >= 100 and (g["match_row"][:100] != MISS).all() and (g["match_row"][100:150] == MISS).all()
    g2 = ir.insert(old, rec, None, ir.default_params(12, min_normal_cos=-1.0))
    assert (g2["match_row"][:150] != MISS).all() and g2["result"]["duplicates"] >= g["result"]["duplicates"] + 50
    # records never gate one another: the outcome of a subset is the subset of the outcomes
    half = ir.insert(old, rec[::2], None, ir.default_params(12))
    assert np.array_equal(half["match_row"], g["match_row"][::2])
    # an identity T computes (-0 + 0 = +0) where no T copies
    p, m = ir.move(rec[203:205], np.eye(4))
    assert p[0].view(np.uint32).tolist() == [0, F(0.25).view(np.uint32), 0] and rec[203, 0].view(np.uint32) == 0x80000000
    # capacity: refused as a whole, the counts still reported
    c = ir.insert(old, rec, None, ir.default_params(12, gate=0), capacity=500)
    assert c["refused"] and c["result"]["count_after"] == 400 and c["result"]["inserted"] == int(fin.sum()) and len(c["map"]) == 400
