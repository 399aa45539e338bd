"""CPU-only checks of the registration entry points (ef_register_step / ef_register_update / ef_register_cloud, include/ef_hip.h): the header
declares them and their structs as C99, the library and the Python mirror carry them, every EF_EINVAL case is refused before any GPU work
(in a child process, so that a crash would be a failed test and not a dead session), and ef_register_update, which needs no GPU, is compared
with a float64 numpy / scipy restatement."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("ef_default_register_params", "ef_register_step", "ef_register_update", "ef_register_cloud", "ef_register_step_dev",
         "ef_register_cloud_dev")


def test_header_declares_the_register_entry_points_as_c99(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(r'''
#include <stdio.h>
#include "ef_hip.h"
int main(void) {
  ef_register_params p;
  ef_register_sums s;
  ef_register_result r;
  int (*a)(ef_ctx*, ef_register_params*) = ef_default_register_params;
  int (*b)(ef_ctx*, const float*, const float*, uint32_t, const ef_register_params*, const double*, ef_register_sums*, uint32_t*, float*) =
      ef_register_step;
  int (*c)(const ef_register_sums*, const double*, double*, double*) = ef_register_update;
  int (*d)(ef_ctx*, const float*, const float*, uint32_t, const ef_register_params*, const double*, double*, ef_register_result*, uint32_t*,
           float*) = ef_register_cloud;
  int (*e)(ef_ctx*, const float*, const float*, uint32_t, const ef_register_params*, const double*, ef_register_sums*, uint32_t*, float*) =
      ef_register_step_dev;
  int (*f)(ef_ctx*, const float*, const float*, uint32_t, const ef_register_params*, const double*, double*, ef_register_result*, uint32_t*,
           float*) = ef_register_cloud_dev;
  p.max_dist = 0.05f; p.min_conf = -1.0f; p.min_normal_cos = -1.0f; p.max_iterations = EF_REGISTER_MAX_ITERATIONS; p.min_pairs = 6;
  p.stop_translation = 1e-6; p.stop_rotation = 1e-6;
  s.A[35] = 0.0; s.b[5] = 0.0; s.e = 0.0; s.pairs = 0u; s.points = 0u;
  r.status = EF_REG_CONVERGED; r.iterations = 0; r.pairs = 0u; r.rms_first = r.rms_last = 0.0; r.A[35] = EF_REGISTER_SMALL_ANGLE;
  printf("%d %d %d %d %d %f %f %f\n", a != 0 && b != 0 && c != 0 && d != 0 && e != 0 && f != 0, EF_REG_MAX_ITERATIONS, EF_REG_TOO_FEW_PAIRS,
         EF_REG_DEGENERATE, p.max_iterations, s.A[35], r.A[35], (double)p.max_dist);
  return 0;
}
''')
    obj = str(tmp_path / "decl.o")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", obj],
                   check=True)


def test_library_and_python_mirror_carry_the_entry_points():
    import ctypes as C
    import re
    from elasticfusion_amd import accuracy, api, build
    build.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in ENTRY:
        assert f" {name}\n" in syms, name
    for m in ("registerParams", "registerStep", "registerCloud", "registerStepDevice", "registerCloudDevice"):
        assert callable(getattr(api.ElasticFusion, m, None)), m
    assert callable(api.register_update) and callable(accuracy.register_to_map)
    # the mirrors are as large as the C structs (C99 layout: 4-byte members, then 8-byte ones on 8-byte boundaries)
    assert C.sizeof(api.ef_register_params) == 40 and C.sizeof(api.ef_register_sums) == 43 * 8 + 8 and C.sizeof(api.ef_register_result) == 16 + 38 * 8
    hdr = open(os.path.join(ROOT, "include", "ef_hip.h")).read()
    for name, val in (("CONVERGED", api.REG_CONVERGED), ("MAX_ITERATIONS", api.REG_MAX_ITERATIONS), ("TOO_FEW_PAIRS", api.REG_TOO_FEW_PAIRS),
                      ("DEGENERATE", api.REG_DEGENERATE)):
        assert int(re.search(r"#define EF_REG_%s (\d+)" % name, hdr).group(1)) == val


def test_struct_sizes_match_the_compiler(tmp_path):
    import ctypes as C
    from elasticfusion_amd import api
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ef_hip.h"\nint main(void) { printf("%d %d %d %d %d %d\\n", '
                   '(int)sizeof(ef_register_params), (int)sizeof(ef_register_sums), (int)sizeof(ef_register_result), '
                   '(int)offsetof(ef_register_params, stop_translation), (int)offsetof(ef_register_sums, pairs), '
                   '(int)offsetof(ef_register_result, rms_first)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(api.ef_register_params), C.sizeof(api.ef_register_sums), C.sizeof(api.ef_register_result),
                   api.ef_register_params.stop_translation.offset, api.ef_register_sums.pairs.offset, api.ef_register_result.rms_first.offset], got


def test_register_entry_points_refuse_bad_arguments_without_a_gpu():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    code = r'''
import ctypes as C
import sys
sys.path.insert(0, %r)
from elasticfusion_amd import api
L = C.CDLL(%r)
L.ef_last_error.restype = C.c_char_p
L.ef_last_error.argtypes = [C.c_void_p]
u, p = C.c_uint32, C.c_void_p
L.ef_default_register_params.argtypes = [p, p]
L.ef_register_step.argtypes = L.ef_register_step_dev.argtypes = [p, p, p, u, p, p, p, p, p]
L.ef_register_cloud.argtypes = L.ef_register_cloud_dev.argtypes = [p, p, p, u, p, p, p, p, p, p]
L.ef_register_update.argtypes = [p, p, p, p]
z = None
pts = (C.c_float * 12)()
inf, nan = float("inf"), float("nan")
def params(**kw):
    q = api.ef_register_params(0.05, -1.0, 0.5, 10, 6, 1e-6, 1e-6)
    for k, v in kw.items():
        setattr(q, k, v)
    return q
def pose(bad=None):
    T = (C.c_double * 16)(*[1.0 if i %% 5 == 0 else 0.0 for i in range(16)])
    if bad is not None:
        T[7] = bad
    return T
def show(name, rc):
    print(name, rc, (L.ef_last_error(None) or b"").decode().replace(" ", "_"), flush=True)
good = params()
sums, res, Tout = api.ef_register_sums(), api.ef_register_result(), (C.c_double * 16)()
show("ef_default_register_params", L.ef_default_register_params(z, C.byref(good)))
def call(name, q, T, pp=pts, n=4, out=True):
    fn = getattr(L, name)
    qq = C.byref(q) if q is not None else z
    if "step" in name:
        return fn(z, pp, z, n, qq, T, C.byref(sums) if out else z, z, z)
    return fn(z, pp, z, n, qq, T, Tout if out else z, C.byref(res), z, z)
for name in ("ef_register_step", "ef_register_step_dev", "ef_register_cloud", "ef_register_cloud_dev"):
    for md in (0.0, -1.0, inf, nan):
        show(name, call(name, params(max_dist=md), z))
    show(name, call(name, params(min_conf=nan), z))
    show(name, call(name, params(min_normal_cos=nan), z))
    for it in (0, -3, 101):
        show(name, call(name, params(max_iterations=it), z))
    for mp in (5, 0, -1):
        show(name, call(name, params(min_pairs=mp), z))
    for sb in (-1e-9, inf, nan):
        show(name, call(name, params(stop_translation=sb), z))
        show(name, call(name, params(stop_rotation=sb), z))
    for bad in (inf, -inf, nan):
        show(name, call(name, good, pose(bad)))
    show(name, call(name, None, z))
    show(name, call(name, good, z, out=False))
    show(name, call(name, good, z, pp=z))
    show(name, call(name, good, pose()))          # all well but the context
    show(name, call(name, good, z, pp=z, n=0))    # likewise
for T in (pose(inf), pose(nan)):
    show("ef_register_update", L.ef_register_update(C.byref(sums), T, Tout, z))
show("ef_register_update", L.ef_register_update(z, pose(), Tout, z))
show("ef_register_update", L.ef_register_update(C.byref(sums), pose(), z, z))
''' % (ROOT, api.LIB_PATH)
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 1 + 4 * 26 + 4, rows
    assert all(int(rc) == -1 for _, rc, _ in rows), rows   # EF_EINVAL, never a crash
    assert all(m.startswith(name + ":") for name, _, m in rows), rows
    by = {}
    for name, _, m in rows:
        by.setdefault(name, []).append(m)
    assert by["ef_default_register_params"][0].endswith("null_context")
    for name in ENTRY[1:]:
        if name == "ef_register_update":
            continue
        m = by[name]
        assert all("max_dist" in x for x in m[:4]) and "min_conf_is_NaN" in m[4] and "min_normal_cos" in m[5], m
        assert all("max_iterations" in x for x in m[6:9]) and all("min_pairs" in x for x in m[9:12]) and all("stop_bounds" in x for x in m[12:18]), m
        assert all("non-finite" in x for x in m[18:21]) and "null_params" in m[21] and ("null_out" in m[22] or "null_T_out" in m[22]), m
        assert "null_points" in m[23] and m[24].endswith("null_context") and m[25].endswith("null_context"), m
    m = by["ef_register_update"]
    assert "non-finite" in m[0] and "non-finite" in m[1] and "null" in m[2] and "null" in m[3], m


def _twist_matrix(xi):
    v, w = xi[:3], xi[3:]
    M = np.zeros((4, 4))
    M[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    M[:3, 3] = v
    return M


def _random_pose(rng):
    from scipy.linalg import expm
    T = expm(_twist_matrix(rng.normal(0, 0.7, 6)))
    T[:3, 3] = rng.uniform(-3, 3, 3)
    return T


def test_update_against_float64_numpy():
    """A = M^T M + I is well conditioned; both solvers (the library's pivoted LDL^T, LAPACK's LU behind numpy.linalg.solve) are backward
    stable, so each returns xi with a relative error of at most about n^2 cond(A) u (n = 6, u = 2^-53; Higham, Accuracy and Stability of
    Numerical Algorithms, theorems 9.4 / 10.4 with a growth factor of order one), and the two differ by at most twice that.  exp is Lipschitz
    with constant (1 + |xi|) on the entries of the 4 x 4 matrix for the |xi| used here, the product with T scales by |T|; forming exp and the
    product adds a few dozen roundings on entries of size |exp| |T|."""
    from scipy.linalg import expm
    from elasticfusion_amd import api
    u = 2.0 ** -53
    rng = np.random.default_rng(0xE6)
    worst = 0.0
    for case in range(60):
        M = rng.normal(0, 1, (6, 6))
        A = M.T @ M + np.eye(6)
        A = (A + A.T) / 2
        scale = (1.0, 0.05, 1e-6, 1e-3)[case % 4]   # rotations above and below EF_REGISTER_SMALL_ANGLE
        b = A @ (rng.normal(0, 1, 6) * scale)
        T = _random_pose(rng) if case % 3 else np.eye(4)
        T_lib, xi_lib, degenerate = api.register_update({"A": A, "b": b}, None if case % 3 == 0 else T)
        assert not degenerate
        xi = np.linalg.solve(A, b)
        T_ref = expm(_twist_matrix(xi)) @ T
        cond = np.linalg.cond(A)
        nx, nT = np.linalg.norm(xi), np.linalg.norm(T)
        bound_xi = 2 * 36 * cond * u * nx
        bound_T = bound_xi * (1 + nx) * nT + 64 * u * (1 + nx) * nT
        err_xi, err_T = np.abs(xi_lib - xi).max(), np.abs(T_lib - T_ref).max()
        worst = max(worst, err_T / bound_T)
        assert err_xi <= bound_xi, (case, err_xi, bound_xi, cond)
        assert err_T <= bound_T, (case, err_T, bound_T, cond)
        assert (T_lib[3] == [0, 0, 0, 1]).all()
    print("largest error / bound", worst)


def test_update_zero_b_returns_T_bit_for_bit_and_bad_A_is_degenerate():
    from elasticfusion_amd import api
    rng = np.random.default_rng(5)
    M = rng.normal(0, 1, (6, 6))
    A = M.T @ M + np.eye(6)
    A = (A + A.T) / 2
    T = _random_pose(rng)
    T[0, 1] = -0.0   # a product with the identity would lose the sign
    T_lib, xi, degenerate = api.register_update({"A": A, "b": np.zeros(6)}, T)
    assert not degenerate and (xi == 0).all()
    assert (T_lib.view(np.uint64) == T.view(np.uint64)).all()
    I_lib, _, degenerate = api.register_update({"A": A, "b": np.zeros(6)}, None)
    assert not degenerate and (I_lib.view(np.uint64) == np.eye(4).view(np.uint64)).all()
    b = rng.normal(0, 1, 6)
    indefinite = A - 2 * np.linalg.eigvalsh(A)[2] * np.eye(6)
    nan_A = A.copy()
    nan_A[2, 2] = np.nan
    for name, bad in (("zero", np.zeros((6, 6))), ("indefinite", indefinite), ("negative definite", -A), ("NaN", nan_A),
                      ("rank three", np.diag([1.0, 1, 1, 0, 0, 0]))):
        T_lib, xi, degenerate = api.register_update({"A": bad, "b": b}, T)
        assert degenerate, name
        assert (T_lib.view(np.uint64) == T.view(np.uint64)).all() and (xi == 0).all(), name
    # a NaN right-hand side has no finite solution either
    assert api.register_update({"A": A, "b": np.full(6, np.nan)}, T)[2]
