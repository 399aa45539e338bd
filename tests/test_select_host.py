"""CPU-only checks of the select / gather / erase entry points (include/ef_hip.h, "Select, extract and erase surfels"): the section is C99,
the library and the Python mirror carry it, every EF_EINVAL case is refused before any GPU work (in a child process, so that a crash would be
a failed test and not a dead session), and the float32 box test of tests/selectref.py agrees with a float64 evaluation away from the faces."""
import os
import subprocess
import sys

import numpy as np

import selectref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("ef_default_map_selection", "ef_map_select", "ef_map_select_dev", "ef_map_gather", "ef_map_gather_dev", "ef_map_erase",
         "ef_map_erase_rows", "ef_map_erase_rows_dev")


def test_header_declares_the_selection_section_as_c99(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(r'''
#include <stdio.h>
#include "ef_hip.h"
int main(void) {
  void (*a)(ef_map_selection*) = ef_default_map_selection;
  int (*b)(ef_ctx*, const ef_map_selection*, uint32_t*, uint32_t, uint32_t*) = ef_map_select;
  int (*c)(ef_ctx*, const ef_map_selection*, uint32_t*, uint32_t, uint32_t*) = ef_map_select_dev;
  int (*d)(ef_ctx*, const uint32_t*, uint32_t, float*) = ef_map_gather;
  int (*e)(ef_ctx*, const uint32_t*, uint32_t, float*) = ef_map_gather_dev;
  int (*f)(ef_ctx*, const ef_map_selection*, uint32_t*) = ef_map_erase;
  int (*g)(ef_ctx*, const uint32_t*, uint32_t, uint32_t*) = ef_map_erase_rows;
  int (*h)(ef_ctx*, const uint32_t*, uint32_t, uint32_t*) = ef_map_erase_rows_dev;
  ef_map_selection s;
  unsigned all = EF_SEL_BOX | EF_SEL_CONF | EF_SEL_INIT_TIME | EF_SEL_LAST_TIME | EF_SEL_RADIUS | EF_SEL_ID | EF_SEL_LABEL | EF_SEL_INVERT;
  s.tests = all; s.T_bw[15] = 1.0; s.box_min[2] = 0.f; s.box_max[2] = 1.f; s.conf_min = s.conf_max = 0.f;
  s.init_time_min = s.init_time_max = s.last_time_min = s.last_time_max = 0; s.radius_min = s.radius_max = 0.f;
  s.id_min = s.id_max = 0u; s.label_class = 0; s.label_min_prob = 0.f;
  printf("%d %u %u\n", a != 0 && b != 0 && c != 0 && d != 0 && e != 0 && f != 0 && g != 0 && h != 0, all, (unsigned)sizeof(s));
  return 0;
}
''')
    exe = str(tmp_path / "decl")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe + ".o"],
                   check=True)
    assert sr.BOX | sr.CONF | sr.INIT_TIME | sr.LAST_TIME | sr.RADIUS | sr.ID | sr.LABEL | sr.INVERT == 0x17F


def test_library_and_python_mirror_carry_the_entry_points():
    import ctypes as C
    from elasticfusion_amd import api, build
    build.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in ENTRY:
        assert f" {name}\n" in syms, name
    for m in ("mapSelection", "selectSurfels", "countSurfels", "gatherSurfels", "eraseSurfels", "eraseRows", "selectSurfelsDevice",
              "gatherSurfelsDevice", "eraseRowsDevice"):
        assert callable(getattr(api.ElasticFusion, m, None)), m
    assert (api.SEL_BOX, api.SEL_CONF, api.SEL_INIT_TIME, api.SEL_LAST_TIME, api.SEL_RADIUS, api.SEL_ID, api.SEL_LABEL, api.SEL_INVERT) == \
        (sr.BOX, sr.CONF, sr.INIT_TIME, sr.LAST_TIME, sr.RADIUS, sr.ID, sr.LABEL, sr.INVERT)
    # the default selection needs neither a context nor a GPU, and is what selectref restates
    s = api.ElasticFusion.mapSelection()
    d = sr.default_selection()
    assert s.tests == 0 and np.array_equal(np.array(s.T_bw).reshape(4, 4), np.eye(4))
    assert list(s.box_min) == d["box_min"] and list(s.box_max) == d["box_max"]
    for k in ("conf_min", "conf_max", "init_time_min", "init_time_max", "last_time_min", "last_time_max", "radius_min", "radius_max", "id_min",
              "id_max", "label_class", "label_min_prob"):
        assert getattr(s, k) == d[k], k
    assert C.sizeof(api.ef_map_selection) == 8 + 128 + 24 + 8 + 16 + 8 + 8 + 8   # the C layout: no padding but the 4 bytes after `tests`


def test_every_einval_case_is_refused_without_a_gpu():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    code = r'''
import ctypes as C
from elasticfusion_amd import api
L = api.lib()
u, p = C.c_uint32, C.c_void_p
S = C.POINTER(api.ef_map_selection)
L.ef_map_select.argtypes = L.ef_map_select_dev.argtypes = [p, S, p, u, p]
L.ef_map_gather.argtypes = L.ef_map_gather_dev.argtypes = [p, p, u, p]
L.ef_map_erase.argtypes = [p, S, p]
L.ef_map_erase_rows.argtypes = L.ef_map_erase_rows_dev.argtypes = [p, p, u, p]
z = None
buf = (C.c_uint32 * 64)()
out = (C.c_float * 64)()
inf, nan = float("inf"), float("nan")
def show(name, case, rc):
    print(name, case, rc, (L.ef_last_error(None) or b"").decode().replace(" ", "_"), flush=True)
def sel(**kw):
    return api.ElasticFusion.mapSelection(**kw)
T_nan = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, nan, 0, 0, 0, 1]
T_inf = [1, 0, 0, 0, 0, inf, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
bad = [
    ("unknown_bit", sel(tests=0x80)),
    ("unknown_high_bit", sel(tests=0x200 | api.SEL_BOX)),
    ("T_nan", sel(tests=api.SEL_BOX, T_bw=T_nan)),
    ("T_inf", sel(tests=api.SEL_BOX, T_bw=T_inf)),
    ("box_min_nan", sel(tests=api.SEL_BOX, box_min=[0, nan, 0])),
    ("box_max_nan", sel(tests=api.SEL_BOX | api.SEL_INVERT, box_max=[0, 0, nan])),
    ("conf_min_nan", sel(tests=api.SEL_CONF, conf_min=nan)),
    ("conf_max_nan", sel(tests=api.SEL_CONF, conf_max=nan)),
    ("radius_min_nan", sel(tests=api.SEL_RADIUS, radius_min=nan)),
    ("radius_max_nan", sel(tests=api.SEL_RADIUS, radius_max=nan)),
    ("label_class_negative", sel(tests=api.SEL_LABEL, label_class=-1)),
    ("label_min_prob_nan", sel(tests=api.SEL_LABEL, label_min_prob=nan)),
]
for name in ("ef_map_select", "ef_map_select_dev"):
    fn = getattr(L, name)
    for case, s in bad:
        show(name, case, fn(z, C.byref(s), buf, 8, buf))
    show(name, "null_selection", fn(z, None, buf, 8, buf))
    show(name, "null_rows", fn(z, C.byref(sel()), z, 8, buf))
    show(name, "null_count", fn(z, C.byref(sel()), buf, 8, z))
    show(name, "null_context", fn(z, C.byref(sel()), buf, 8, buf))
    show(name, "null_context_count_only", fn(z, C.byref(sel(tests=api.SEL_BOX, box_max=[inf, inf, 0])), z, 0, buf))
for case, s in bad:
    show("ef_map_erase", case, L.ef_map_erase(z, C.byref(s), buf))
show("ef_map_erase", "null_selection", L.ef_map_erase(z, None, buf))
show("ef_map_erase", "null_context", L.ef_map_erase(z, C.byref(sel()), z))
for name in ("ef_map_gather", "ef_map_gather_dev"):
    fn = getattr(L, name)
    show(name, "null_rows", fn(z, z, 4, out))
    show(name, "null_surfels12", fn(z, buf, 4, z))
    show(name, "null_context", fn(z, buf, 4, out))
    show(name, "null_context_empty", fn(z, z, 0, z))
for name in ("ef_map_erase_rows", "ef_map_erase_rows_dev"):
    fn = getattr(L, name)
    show(name, "null_rows", fn(z, z, 4, buf))
    show(name, "null_context", fn(z, buf, 4, z))
    show(name, "null_context_empty", fn(z, z, 0, z))
# a test that is not enabled is not checked: NaN in the fields of a disabled test reaches the context check
s = sel(tests=api.SEL_CONF, box_min=[nan, nan, nan], radius_min=nan, label_min_prob=nan, label_class=-5, T_bw=T_nan)
show("ef_map_select", "disabled_fields_unchecked", L.ef_map_select(z, C.byref(s), buf, 8, buf))
'''
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 2 * 17 + 14 + 2 * 4 + 2 * 3 + 1, rows
    assert all(int(rc) == -1 for _, _, rc, _ in rows), rows   # EF_EINVAL, never a crash
    assert all(m.startswith(name + ":") for name, _, _, m in rows), rows
    expect = dict(unknown_bit="unknown_bits", unknown_high_bit="unknown_bits", T_nan="T_bw", T_inf="T_bw", box_min_nan="box_bound_is_NaN",
                  box_max_nan="box_bound_is_NaN", conf_min_nan="confidence_bound_is_NaN", conf_max_nan="confidence_bound_is_NaN",
                  radius_min_nan="radius_bound_is_NaN", radius_max_nan="radius_bound_is_NaN", label_class_negative="label_class",
                  label_min_prob_nan="label_min_prob_is_NaN", null_selection="null_selection", null_rows="null_rows", null_count="null_count",
                  null_surfels12="null_surfels12", null_context="null_context", null_context_count_only="null_context",
                  null_context_empty="null_context", disabled_fields_unchecked="null_context")
    for name, case, _, m in rows:
        assert expect[case] in m, (name, case, m)


def test_f32_box_test_agrees_with_float64_away_from_the_faces():
    """The float32 evaluation of b = ((R0 x + R1 y) + R2 z) + t carries at most three roundings of partial sums no larger than
    |R0 x| + |R1 y| + |R2 z| + |t| <= sqrt(3) |p| + |t| < 16 here, each below 2^-24 of that: under 4e-6, well inside the 1e-4 of the box size
    (2e-4 for the smallest edge, 2) that the points compared keep from every face."""
    rng = np.random.default_rng(11)
    a = 0.7
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(0.4), -np.sin(0.4)], [0, np.sin(0.4), np.cos(0.4)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Rx
    T[:3, 3] = (0.3, -1.1, 2.0)
    lo, hi = np.array([-1.0, -2.0, 0.5], np.float32), np.array([1.0, 1.5, 3.0], np.float32)
    xyz = rng.uniform(-4, 4, (200000, 3)).astype(np.float32)
    b32, b64 = sr.box_coords(xyz, T), sr.box_coords(xyz, T, np.float64)
    assert b32.dtype == np.float32 and b64.dtype == np.float64
    size = float((hi - lo).min())
    margin = np.minimum(np.abs(b64 - lo.astype(np.float64)), np.abs(b64 - hi.astype(np.float64))).min(1)
    far = margin > 1e-4 * size
    in32, in64 = sr.in_box(b32, lo, hi), sr.in_box(b64, lo, hi)
    print("points", len(xyz), "far from every face", int(far.sum()), "inside", int(in64.sum()), "largest |b32 - b64|", float(np.abs(b32 - b64).max()))
    assert far.sum() > 0.99 * len(xyz) and in64.sum() > 1000 and (~in64).sum() > 1000
    assert np.abs(b32 - b64).max() < 4e-6
    assert np.array_equal(in32[far], in64[far])
