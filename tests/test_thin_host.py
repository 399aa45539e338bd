"""CPU-only checks of the thin entry points (include/ef_hip.h, "Thin the map"): the section is C99, the library and the Python mirror carry it
with structs of the same size, every EF_EINVAL case is refused before any GPU work (in a child process, so that a crash would be a failed
test and not a dead session), and the numpy restatement of tests/thinref.py has the properties the header states."""
import os
import subprocess
import sys

import numpy as np

import selectref as sr
import thinref as tr
from queryref import cells_of, default_cell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("ef_default_thin_params", "ef_map_thin_select", "ef_map_thin_select_dev", "ef_map_thin")
F = np.float32


def test_header_declares_the_thin_section_as_c99(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(r'''
#include <stdio.h>
#include "ef_hip.h"
int main(void) {
  int (*a)(ef_ctx*, ef_thin_params*) = ef_default_thin_params;
  int (*b)(ef_ctx*, const ef_thin_params*, const ef_map_selection*, int, uint32_t*, uint32_t, uint32_t*) = ef_map_thin_select;
  int (*c)(ef_ctx*, const ef_thin_params*, const ef_map_selection*, int, uint32_t*, uint32_t, uint32_t*) = ef_map_thin_select_dev;
  int (*d)(ef_ctx*, const ef_thin_params*, const ef_map_selection*, ef_thin_result*) = ef_map_thin;
  ef_thin_params p;
  ef_thin_result r;
  p.cell = EF_QUERY_DEFAULT_CELL; p.keep = EF_THIN_KEEP_NEWEST;
  r.participants = r.cells = r.removed = r.count_after = 0u;
  printf("%d %u %u %d %u %d %d\n", a != 0 && b != 0 && c != 0 && d != 0, (unsigned)sizeof(p), (unsigned)sizeof(r), p.keep, r.cells,
         EF_THIN_ROWS_REMOVED, EF_THIN_ROWS_REPRESENTATIVES);
  return 0;
}
''')
    exe = str(tmp_path / "decl")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe + ".o"],
                   check=True)
    hdr = open(os.path.join(ROOT, "include", "ef_hip.h")).read()
    for name, v in (("EF_THIN_KEEP_MAX_CONF", tr.KEEP_MAX_CONF), ("EF_THIN_KEEP_NEWEST", tr.KEEP_NEWEST), ("EF_THIN_KEEP_FIRST", tr.KEEP_FIRST),
                    ("EF_THIN_ROWS_REMOVED", tr.ROWS_REMOVED), ("EF_THIN_ROWS_REPRESENTATIVES", tr.ROWS_REPRESENTATIVES)):
        assert f"#define {name}" in hdr and int(hdr.split(f"#define {name}")[1].split()[0]) == v, name


def test_library_and_python_mirror_carry_the_entry_points():
    import ctypes as C
    from elasticfusion_amd import accuracy, api, build
    build.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in ENTRY:
        assert f" {name}\n" in syms, name
    for m in ("thinParams", "thinSelect", "thinSelectDevice", "thinSurfels"):
        assert callable(getattr(api.ElasticFusion, m, None)), m
    assert callable(accuracy.thinned_map)
    assert (api.THIN_KEEP_MAX_CONF, api.THIN_KEEP_NEWEST, api.THIN_KEEP_FIRST) == (tr.KEEP_MAX_CONF, tr.KEEP_NEWEST, tr.KEEP_FIRST)
    assert (api.THIN_ROWS_REMOVED, api.THIN_ROWS_REPRESENTATIVES) == (tr.ROWS_REMOVED, tr.ROWS_REPRESENTATIVES)
    # the C layouts: two and four 4-byte fields, no padding
    assert C.sizeof(api.ef_thin_params) == 8 and C.sizeof(api.ef_thin_result) == 16
    assert [f for f, _ in api.ef_thin_params._fields_] == ["cell", "keep"]
    assert [f for f, _ in api.ef_thin_result._fields_] == ["participants", "cells", "removed", "count_after"]


def test_every_einval_case_is_refused_without_a_gpu():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    code = r'''
import ctypes as C
from elasticfusion_amd import api
L = api.lib()
u, p, i = C.c_uint32, C.c_void_p, C.c_int
PP, RP, SP = C.POINTER(api.ef_thin_params), C.POINTER(api.ef_thin_result), C.POINTER(api.ef_map_selection)
L.ef_map_thin_select.argtypes = L.ef_map_thin_select_dev.argtypes = [p, PP, SP, i, p, u, p]
L.ef_map_thin.argtypes = [p, PP, SP, RP]
L.ef_default_thin_params.argtypes = [p, PP]
z = None
rows = (C.c_uint32 * 8)()
cnt = C.c_uint32(0)
res = api.ef_thin_result()
inf, nan = float("inf"), float("nan")
def show(name, case, rc):
    print(name, case, rc, (L.ef_last_error(None) or b"").decode().replace(" ", "_"), flush=True)
def par(**kw):
    q = api.ef_thin_params(0.02, 0)
    for k, v in kw.items():
        setattr(q, k, v)
    return q
def sel(**kw):
    s = api.ElasticFusion.mapSelection(**kw)
    return C.byref(s)
bad = [("cell_zero", par(cell=0.0)), ("cell_negative", par(cell=-0.02)), ("cell_nan", par(cell=nan)), ("cell_inf", par(cell=inf)),
       ("cell_inverse_overflows", par(cell=1e-39)), ("keep_3", par(keep=3)), ("keep_negative", par(keep=-1))]
bad_among = [("among_unknown_bits", sel(tests=0x200)), ("among_conf_nan", sel(tests=api.SEL_CONF, conf_min=nan)),
             ("among_box_nan", sel(tests=api.SEL_BOX, box_min=[nan, 0, 0])), ("among_radius_nan", sel(tests=api.SEL_RADIUS, radius_max=nan)),
             ("among_label_class", sel(tests=api.SEL_LABEL, label_class=-1))]
Tbad = api.ElasticFusion.mapSelection(tests=api.SEL_BOX)
Tbad.T_bw[7] = inf
bad_among.append(("among_T_inf", C.byref(Tbad)))
for name in ("ef_map_thin_select", "ef_map_thin_select_dev"):
    fn = getattr(L, name)
    for case, q in bad:
        show(name, case, fn(z, C.byref(q), None, 0, rows, 8, C.byref(cnt)))
    for case, a in bad_among:
        show(name, case, fn(z, C.byref(par()), a, 0, rows, 8, C.byref(cnt)))
    show(name, "null_params", fn(z, None, None, 0, rows, 8, C.byref(cnt)))
    show(name, "null_count", fn(z, C.byref(par()), None, 0, rows, 8, None))
    show(name, "what_2", fn(z, C.byref(par()), None, 2, rows, 8, C.byref(cnt)))
    show(name, "what_negative", fn(z, C.byref(par()), None, -1, rows, 8, C.byref(cnt)))
    show(name, "null_rows", fn(z, C.byref(par()), None, 1, None, 8, C.byref(cnt)))
    show(name, "null_context", fn(z, C.byref(par()), None, 1, rows, 8, C.byref(cnt)))
    show(name, "null_context_count_only", fn(z, C.byref(par(keep=2)), sel(tests=api.SEL_INVERT), 0, None, 0, C.byref(cnt)))
for case, q in bad:
    show("ef_map_thin", case, L.ef_map_thin(z, C.byref(q), None, C.byref(res)))
for case, a in bad_among:
    show("ef_map_thin", case, L.ef_map_thin(z, C.byref(par()), a, C.byref(res)))
show("ef_map_thin", "null_params", L.ef_map_thin(z, None, None, C.byref(res)))
show("ef_map_thin", "null_result", L.ef_map_thin(z, C.byref(par()), None, None))
show("ef_map_thin", "null_context", L.ef_map_thin(z, C.byref(par()), None, C.byref(res)))
show("ef_default_thin_params", "null_context", L.ef_default_thin_params(z, C.byref(par())))
'''
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 2 * (7 + 6 + 7) + (7 + 6 + 3) + 1, rows
    assert all(int(rc) == -1 for _, _, rc, _ in rows), rows   # EF_EINVAL, never a crash
    assert all(m.startswith(name + ":") for name, _, _, m in rows), rows
    expect = dict(cell_zero="cell_must_be", cell_negative="cell_must_be", cell_nan="cell_must_be", cell_inf="cell_must_be",
                  cell_inverse_overflows="cell_must_be", keep_3="keep_must_be", keep_negative="keep_must_be", among_unknown_bits="unknown_bits",
                  among_conf_nan="confidence_bound_is_NaN", among_box_nan="box_bound_is_NaN", among_radius_nan="radius_bound_is_NaN",
                  among_label_class="label_class_outside", among_T_inf="T_bw_has_a_non-finite", null_params="null_params", null_count="null_count",
                  null_result="null_result", what_2="what_must_be", what_negative="what_must_be", null_rows="null_rows",
                  null_context="null_context", null_context_count_only="null_context")
    for name, case, _, m in rows:
        assert expect[case] in m, (name, case, m)


def small_scene():
    rng = np.random.default_rng(11)
    n = 3000
    S = np.zeros((n, 12), F)
    S[:, :3] = rng.uniform(-0.5, 0.5, (n, 3))
    S[:, 3] = rng.integers(0, 6, n)                  # ties are the rule
    S[:, 7] = rng.integers(0, 40, n)
    S[::97, 3] = np.nan
    S[5::131, 3] = -0.0
    S[7, 0], S[8, 1], S[9, 2] = np.nan, np.inf, -np.inf
    S[:, 11] = 0.004
    return S


def test_the_reference_has_the_properties_the_header_states():
    S = small_scene()
    cell = 0.05
    for keep in (tr.KEEP_MAX_CONF, tr.KEEP_NEWEST, tr.KEEP_FIRST):
        t = tr.thin(S, cell, keep)
        res = t["result"]
        assert res["participants"] == len(S) - 3 and res["removed"] == res["participants"] - res["cells"] and 0 < res["cells"] < res["participants"]
        assert not t["part"][7:10].any() and t["kept"][7:10].all()                      # a non-finite position is kept and counted nowhere
        cells = cells_of(np.nan_to_num(S[:, :3], posinf=0, neginf=0), cell)
        assert len(np.unique(cells[t["rep"]], axis=0)) == res["cells"]                  # one representative per cell that holds a participant
        assert len(np.unique(cells[t["part"]], axis=0)) == res["cells"]
        # idempotence: the representatives are alone in their cells
        again = tr.thin(S[t["kept"]], cell, keep)
        assert again["result"]["removed"] == 0 and again["result"]["cells"] == res["cells"]
        # the outcome of a row depends on its own cell only: a subset made of whole cells gives the subset of the outcomes
        whole = cells[:, 0] < 0
        sub = tr.thin(S[whole], cell, keep)
        assert np.array_equal(sub["rep"], t["rep"][whole]) and np.array_equal(sub["removed"], t["removed"][whole])
    # KEEP_FIRST: the lowest row of every cell
    t = tr.thin(S, cell, tr.KEEP_FIRST)
    fin = np.isfinite(S[:, :3]).all(1)
    _, first = np.unique(cells_of(S[fin, :3], cell), axis=0, return_index=True)
    assert np.array_equal(t["rows_rep"], np.sort(np.nonzero(fin)[0][first]).astype(np.uint32))
    # non-participants are untouched: they are kept, win nothing and beat nobody
    among = sr.default_selection(tests=sr.CONF, conf_min=0.0, conf_max=3.0)            # (NaN fails the range: not a participant)
    t = tr.thin(S, cell, tr.KEEP_MAX_CONF, among)
    out = ~sr.select_mask(S, among)
    assert out.sum() > 500 and t["kept"][out].all() and not t["rep"][out].any() and not t["part"][out].any()
    inner = tr.thin(S[~out], cell, tr.KEEP_MAX_CONF)
    assert np.array_equal(inner["rep"], t["rep"][~out]) and np.array_equal(inner["removed"], t["removed"][~out])
    assert tr.thin(S, default_cell())["result"]["cells"] > tr.thin(S, cell)["result"]["cells"]


def test_the_order_of_the_primaries_is_total():
    def one_cell(conf):
        S = np.zeros((len(conf), 12), F)
        S[:, :3] = (0.001, 0.002, 0.003)
        S[:, 3] = np.asarray(conf, F)
        return S
    nan, inf = np.nan, np.inf
    # +0 equals -0: the lower row wins whichever sign it carries
    assert tr.thin(one_cell([-0.0, 0.0]), 0.02)["rows_rep"].tolist() == [0]
    assert tr.thin(one_cell([0.0, -0.0]), 0.02)["rows_rep"].tolist() == [0]
    assert tr.thin(one_cell([-1.0, -0.0, 0.0]), 0.02)["rows_rep"].tolist() == [1]
    # a NaN counts as -inf: it loses to every number, ties with -inf and with other NaNs by row
    assert tr.thin(one_cell([nan, -5.0, nan]), 0.02)["rows_rep"].tolist() == [1]
    assert tr.thin(one_cell([nan, -inf]), 0.02)["rows_rep"].tolist() == [0]
    assert tr.thin(one_cell([-inf, nan]), 0.02)["rows_rep"].tolist() == [0]
    assert tr.thin(one_cell([nan, nan, nan]), 0.02)["rows_rep"].tolist() == [0]
    assert tr.thin(one_cell([1.0, inf, inf]), 0.02)["rows_rep"].tolist() == [1]
    # the cycle of raw `>`: with "b beats a iff conf_b > conf_a, or neither is greater and row_b < row_a" and NaN left raw, the confidences
    # (1, NaN, 2) beat each other in a circle (row 0 beats row 1 and row 1 beats row 2 by their lower rows, since no comparison with NaN is
    # true; row 2 beats row 0 by its confidence): every surfel is beaten and the cell would empty itself
    conf = np.array([1.0, nan, 2.0], F)

    def beats(b, a):
        with np.errstate(invalid="ignore"):
            return bool(conf[b] > conf[a]) or (not bool(conf[a] > conf[b]) and b < a)
    assert beats(0, 1) and beats(1, 2) and beats(2, 0), "raw comparisons: every one of the three is beaten by another"
    t = tr.thin(one_cell(conf), 0.02)
    assert t["rows_rep"].tolist() == [2] and t["result"] == dict(participants=3, cells=1, removed=2, count_after=1)


def test_the_reference_is_quick_enough_for_the_gpu_suite():
    import time
    rng = np.random.default_rng(1)
    S = np.zeros((200000, 12), F)
    S[:, :3] = rng.uniform(0, 2, (200000, 3))
    S[:, 3] = rng.integers(0, 8, 200000)
    t0 = time.perf_counter()
    t = tr.thin(S, 0.05)
    dt = time.perf_counter() - t0
    print("200 000 rows:", t["result"], f"{dt:.2f} s")
    assert t["result"]["cells"] <= 41 ** 3 and dt < 10
