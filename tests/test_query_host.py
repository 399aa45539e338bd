"""CPU-only checks of the spatial-query entry points (include/ef_hip.h): the header declares them as C99, the library and the Python mirror
carry them, and bad arguments or a NULL context are refused with EF_EINVAL before any GPU work (in a child process, so that a crash would be
a failed test and not a dead session)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("ef_set_query_cell", "ef_query_nearest", "ef_query_knn", "ef_query_nearest_dev", "ef_query_knn_dev")


def test_header_declares_the_query_entry_points_as_c99(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(r'''
#include <stdio.h>
#include "ef_hip.h"
int main(void) {
  int (*a)(ef_ctx*, float) = ef_set_query_cell;
  int (*b)(ef_ctx*, const float*, uint32_t, float, float, uint32_t*, uint32_t*, float*, float*) = ef_query_nearest;
  int (*c)(ef_ctx*, const float*, uint32_t, int, float, float, uint32_t*, float*, uint32_t*) = ef_query_knn;
  int (*d)(ef_ctx*, const float*, uint32_t, float, float, uint32_t*, uint32_t*, float*, float*) = ef_query_nearest_dev;
  int (*e)(ef_ctx*, const float*, uint32_t, int, float, float, uint32_t*, float*, uint32_t*) = ef_query_knn_dev;
  float cell = EF_QUERY_DEFAULT_CELL;
  printf("%d %d %f\n", a != 0 && b != 0 && c != 0 && d != 0 && e != 0, EF_QUERY_MAX_RATIO >= 8, cell);
  return 0;
}
''')
    obj = str(tmp_path / "decl.o")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", obj],
                   check=True)


def test_library_and_python_mirror_carry_the_entry_points():
    from elasticfusion_amd import accuracy, api, build
    build.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in ENTRY:
        assert f" {name}\n" in syms, name
    for m in ("setQueryCell", "queryNearest", "queryKnn", "queryNearestDevice", "queryKnnDevice"):
        assert callable(getattr(api.ElasticFusion, m, None)), m
    assert callable(accuracy.map_accuracy)


def test_the_ratio_limit_is_at_least_eight():
    import re
    hdr = open(os.path.join(ROOT, "include", "ef_hip.h")).read()
    assert int(re.search(r"#define EF_QUERY_MAX_RATIO (\d+)", hdr).group(1)) >= 8
    from elasticfusion_amd import api
    assert float(re.search(r"#define EF_QUERY_DEFAULT_CELL ([0-9.]+)f", hdr).group(1)) == api.ElasticFusion.QUERY_DEFAULT_CELL


def test_query_entry_points_refuse_bad_arguments_without_a_gpu():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    code = r'''
import ctypes as C
L = C.CDLL(%r)
L.ef_last_error.restype = C.c_char_p
L.ef_last_error.argtypes = [C.c_void_p]
f, u, i, p = C.c_float, C.c_uint32, C.c_int, C.c_void_p
near = [p, p, u, f, f, p, p, p, p]
knn = [p, p, u, i, f, f, p, p, p]
L.ef_set_query_cell.argtypes = [p, f]
L.ef_query_nearest.argtypes = L.ef_query_nearest_dev.argtypes = near
L.ef_query_knn.argtypes = L.ef_query_knn_dev.argtypes = knn
z = None
pts = (C.c_float * 12)()
out = (C.c_uint32 * 64)()
inf, nan = float("inf"), float("nan")
def show(name, rc):
    print(name, rc, (L.ef_last_error(None) or b"").decode().replace(" ", "_"), flush=True)
for cell in (0.0, -0.01, inf, nan):
    show("ef_set_query_cell", L.ef_set_query_cell(z, cell))
show("ef_set_query_cell", L.ef_set_query_cell(z, 0.02))
for name in ("ef_query_nearest", "ef_query_nearest_dev"):
    fn = getattr(L, name)
    for md in (0.0, -1.0, inf, nan):
        show(name, fn(z, pts, 4, md, -1.0, out, z, z, z))
    show(name, fn(z, pts, 4, 0.02, nan, out, z, z, z))
    show(name, fn(z, z, 4, 0.02, -1.0, out, z, z, z))
    show(name, fn(z, pts, 4, 0.02, -1.0, z, z, z, z))
    show(name, fn(z, pts, 4, 0.02, -1.0, out, z, z, z))
    show(name, fn(z, z, 0, 0.02, -1.0, out, z, z, z))
for name in ("ef_query_knn", "ef_query_knn_dev"):
    fn = getattr(L, name)
    for k in (0, -1, 17, 1 << 20):
        show(name, fn(z, pts, 4, k, 0.02, -1.0, out, z, z))
    for md in (0.0, -1.0, inf, nan):
        show(name, fn(z, pts, 4, 4, md, -1.0, out, z, z))
    show(name, fn(z, pts, 4, 4, 0.02, nan, out, z, z))
    show(name, fn(z, z, 4, 4, 0.02, -1.0, out, z, z))
    show(name, fn(z, pts, 4, 4, 0.02, -1.0, z, z, z))
    show(name, fn(z, pts, 4, 4, 0.02, -1.0, out, z, z))
''' % api.LIB_PATH
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 5 + 2 * 9 + 2 * 12, rows
    assert all(int(rc) == -1 for _, rc, _ in rows), rows   # EF_EINVAL, never a crash
    assert all(m.startswith(name + ":") for name, _, m in rows), rows
    by = {}
    for name, _, m in rows:
        by.setdefault(name, []).append(m)
    m = by["ef_set_query_cell"]
    assert all("finite_and_positive" in x for x in m[:4]) and m[4].endswith("null_context"), m
    for name in ("ef_query_nearest", "ef_query_nearest_dev"):
        m = by[name]
        assert all("max_dist" in x for x in m[:4]) and "NaN" in m[4] and "null_points" in m[5] and "null_row" in m[6], m
        assert m[7].endswith("null_context") and m[8].endswith("null_context"), m
    for name in ("ef_query_knn", "ef_query_knn_dev"):
        m = by[name]
        assert all("1_.._16" in x for x in m[:4]) and all("max_dist" in x for x in m[4:8]) and "NaN" in m[8], m
        assert "null_points" in m[9] and "null_row" in m[10] and m[11].endswith("null_context"), m
