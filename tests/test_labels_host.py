"""CPU-only checks of the surfel-ID / label entry points (include/ef_hip.h): the header declares them as C99, the library and the Python
mirror carry them, and bad arguments or a NULL context are refused with EF_EINVAL before any GPU work (in a child process, so that a crash
would be a failed test and not a dead session)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("ef_set_surfel_ids", "ef_get_surfel_ids", "ef_enable_labels", "ef_set_labels", "ef_get_labels", "ef_fuse_labels",
         "ef_fuse_labels_dev", "ef_render_labels", "ef_render_labels_dev")


def test_header_declares_the_label_entry_points_as_c99(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(r'''
#include <stdio.h>
#include "ef_hip.h"
int main(void) {
  int (*a)(ef_ctx*, int) = ef_set_surfel_ids;
  int (*b)(ef_ctx*, uint32_t*, uint32_t, uint32_t*) = ef_get_surfel_ids;
  int (*c)(ef_ctx*, int) = ef_enable_labels;
  int (*d)(ef_ctx*, const float*, uint32_t) = ef_set_labels;
  int (*e)(ef_ctx*, uint32_t*, float*, uint32_t, uint32_t*) = ef_get_labels;
  int (*f)(ef_ctx*, const ef_render_params*, const float*) = ef_fuse_labels;
  int (*g)(ef_ctx*, const ef_render_params*, const float*) = ef_fuse_labels_dev;
  int (*h)(ef_ctx*, const ef_render_params*, int32_t*, float*) = ef_render_labels;
  int (*i)(ef_ctx*, const ef_render_params*, int32_t*, float*) = ef_render_labels_dev;
  printf("%d\n", a != 0 && b != 0 && c != 0 && d != 0 && e != 0 && f != 0 && g != 0 && h != 0 && i != 0);
  return 0;
}
''')
    obj = str(tmp_path / "decl.o")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", obj],
                   check=True)


def test_library_and_python_mirror_carry_the_entry_points():
    from elasticfusion_amd import api, build
    build.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in ENTRY:
        assert f" {name}\n" in syms, name
    for m in ("setSurfelIds", "surfelIds", "enableLabels", "fuseLabels", "fuseLabelsDevice", "labels", "setLabels", "renderLabels",
              "renderLabelsDevice"):
        assert callable(getattr(api.ElasticFusion, m, None)), m


def test_label_entry_points_refuse_bad_arguments_without_a_gpu():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    code = r'''
import ctypes as C
from elasticfusion_amd import api
L = C.CDLL(%r)
L.ef_last_error.restype = C.c_char_p
L.ef_last_error.argtypes = [C.c_void_p]
z = C.c_void_p(None)
img = (C.c_float * 16)()
n = C.c_uint32(0)
def show(name, rc):
    print(name, rc, (L.ef_last_error(None) or b"").decode().replace(" ", "_"), flush=True)
good = api.ef_render_params(width=64, height=48, fx=50.0, fy=50.0, cx=32.0, cy=24.0, max_depth=1000.0)
show("ef_set_surfel_ids", L.ef_set_surfel_ids(z, 1))
show("ef_get_surfel_ids", L.ef_get_surfel_ids(z, z, 0, C.byref(n)))
for k in (-1, 257, 1 << 20):
    show("ef_enable_labels", L.ef_enable_labels(z, k))
show("ef_enable_labels", L.ef_enable_labels(z, 4))
show("ef_set_labels", L.ef_set_labels(z, img, 1))
show("ef_get_labels", L.ef_get_labels(z, z, z, 0, C.byref(n)))
for name in ("ef_fuse_labels", "ef_fuse_labels_dev"):
    show(name, getattr(L, name)(z, C.byref(good), z))
    show(name, getattr(L, name)(z, z, z))
    for w, h in ((0, 48), (4097, 48)):
        show(name, getattr(L, name)(z, C.byref(api.ef_render_params(width=w, height=h, fx=50.0, fy=50.0, cx=32.0, cy=24.0)), img))
    show(name, getattr(L, name)(z, C.byref(api.ef_render_params(width=64, height=48, fx=0.0, fy=50.0, cx=32.0, cy=24.0)), img))
    show(name, getattr(L, name)(z, C.byref(good), img))
    show(name, getattr(L, name)(z, z, img))
for name in ("ef_render_labels", "ef_render_labels_dev"):
    show(name, getattr(L, name)(z, z, z, z))
    show(name, getattr(L, name)(z, C.byref(api.ef_render_params(width=64, height=0, fx=50.0, fy=50.0, cx=32.0, cy=24.0)), z, z))
    show(name, getattr(L, name)(z, C.byref(good), z, z))
''' % api.LIB_PATH
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 2 + 4 + 2 + 2 * 7 + 2 * 3, rows
    assert all(int(rc) == -1 for _, rc, _ in rows), rows   # EF_EINVAL, never a crash
    assert all(m.startswith(name + ":") for name, _, m in rows), rows
    by = {}
    for name, _, m in rows:
        by.setdefault(name, []).append(m)
    assert all("0_.._256" in m for m in by["ef_enable_labels"][:3])
    assert all(m.endswith("null_context") for m in ([by["ef_enable_labels"][3], by["ef_set_surfel_ids"][0], by["ef_get_surfel_ids"][0],
                                                     by["ef_set_labels"][0], by["ef_get_labels"][0]]))
    for name in ("ef_fuse_labels", "ef_fuse_labels_dev"):
        m = by[name]
        assert "null_probability_image" in m[0] and "null_probability_image" in m[1], m
        assert "1_.._4096" in m[2] and "1_.._4096" in m[3] and "intrinsics" in m[4], m
        assert m[5].endswith("null_context") and m[6].endswith("null_context"), m
    for name in ("ef_render_labels", "ef_render_labels_dev"):
        m = by[name]
        assert "null_params" in m[0] and "1_.._4096" in m[1] and m[2].endswith("null_context"), m
