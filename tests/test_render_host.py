"""CPU-only checks of the render entry points (ef_default_render_params / ef_render_model / ef_render_model_dev, include/ef_hip.h):
the Python mirror of ef_render_params has the C layout, and bad parameters or a NULL context are refused with EF_EINVAL before anything
is read or a GPU touched (in a child process, so that a crash would be a failed test and not a dead session)."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_params_layout_matches_the_header(tmp_path):
    from elasticfusion_amd import api
    src = tmp_path / "layout.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "ef_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(ef_render_params), offsetof(ef_render_params, T_wc), offsetof(ef_render_params, max_depth),
         offsetof(ef_render_params, color_type), offsetof(ef_render_params, time_delta));
  return 0;
}
''')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    P = api.ef_render_params
    assert got == [C.sizeof(P), P.T_wc.offset, P.max_depth.offset, P.color_type.offset, P.time_delta.offset]


def test_render_entry_points_refuse_bad_parameters_without_a_gpu():
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
def call(name, p):
    rc = getattr(L, name)(z, p, z, z, z, z, z)
    print(name, rc, (L.ef_last_error(None) or b"").decode().replace(" ", "_"), flush=True)
good = api.ef_render_params(width=64, height=48, fx=50.0, fy=50.0, cx=32.0, cy=24.0, max_depth=1000.0)
for name in ("ef_render_model", "ef_render_model_dev"):
    call(name, None)
    for w, h in ((0, 48), (64, 0), (4097, 48), (64, 4097), (-5, 48)):
        call(name, C.byref(api.ef_render_params(width=w, height=h, fx=50.0, fy=50.0, cx=32.0, cy=24.0)))
    call(name, C.byref(api.ef_render_params(width=64, height=48, fx=50.0, fy=50.0, cx=32.0, cy=24.0, color_type=4)))
    call(name, C.byref(api.ef_render_params(width=64, height=48, fx=0.0, fy=50.0, cx=32.0, cy=24.0)))
    call(name, C.byref(api.ef_render_params(width=64, height=48, fx=float("nan"), fy=50.0, cx=32.0, cy=24.0)))
    call(name, C.byref(good))
print("ef_default_render_params", L.ef_default_render_params(z, C.byref(good)), "-", flush=True)
print("ef_default_render_params", L.ef_default_render_params(z, z), "-", flush=True)
''' % api.LIB_PATH
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 2 * 10 + 2
    assert all(int(rc) == -1 for _, rc, _ in rows), rows   # EF_EINVAL, never a crash
    msgs = [m for name, _, m in rows if name != "ef_default_render_params"]
    for k, prefix in enumerate(("ef_render_model:", "ef_render_model_dev:")):
        m = msgs[k * 10:(k + 1) * 10]
        assert all(x.startswith(prefix) for x in m), m
        assert "null_params" in m[0]
        assert all("1_.._4096" in x for x in m[1:6]), m
        assert "color_type" in m[6] and "intrinsics" in m[7] and "intrinsics" in m[8]
        assert m[9].endswith("null_context")


def test_shim_exports_the_headless_render():
    from elasticfusion_amd import api, build
    build.build()
    shim = os.path.join(os.path.dirname(api.LIB_PATH), "libefusion.so")
    syms = subprocess.run(["nm", "-DC", "--defined-only", shim], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "efusion::GlobalModelView::renderPointCloudImage(" in syms
