"""CPU-only checks of the carve entry points (include/ef_hip.h, "Carve free space"): the section is C99, the library and the Python mirror carry
it with structs of the same size, every EF_EINVAL case is refused before any GPU work (in a child process, so that a crash would be a failed
test and not a dead session), and the numpy restatement of tests/carveref.py has properties that do not depend on any implementation: a map is
never carved by depth images of itself, a moved object goes, the outcome is monotone in min_views / margin / protect and independent per row."""
import os
import subprocess
import sys
import time

import numpy as np

import carveref as cr
import selectref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("ef_default_carve_params", "ef_map_carve_select", "ef_map_carve_select_dev", "ef_map_carve", "ef_map_carve_dev")
F = np.float32
# The oracle's map after frames 0 .. 2 of synthetic sequence 1, carved with frame 2's depth at the oracle's pose and the default parameters:
# the number of the map's OWN rows that are removed.  Measured 0 is the claim; test_gpu_carve asserts the same cap at the workload's size.
OWN_ROWS_REMOVED_CAP = 0


def test_header_declares_the_carve_section_as_c99(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(r'''
#include <stdio.h>
#include "ef_hip.h"
int main(void) {
  int (*a)(ef_ctx*, ef_carve_params*) = ef_default_carve_params;
  int (*b)(ef_ctx*, const ef_carve_params*, const ef_carve_views*, const ef_map_selection*, uint32_t*, uint32_t, uint32_t*, uint8_t*) = ef_map_carve_select;
  int (*c)(ef_ctx*, const ef_carve_params*, const ef_carve_views*, const ef_map_selection*, uint32_t*, uint32_t, uint32_t*, uint8_t*) = ef_map_carve_select_dev;
  int (*d)(ef_ctx*, const ef_carve_params*, const ef_carve_views*, const ef_map_selection*, ef_carve_result*) = ef_map_carve;
  int (*e)(ef_ctx*, const ef_carve_params*, const ef_carve_views*, const ef_map_selection*, ef_carve_result*) = ef_map_carve_dev;
  ef_carve_params p;
  ef_carve_views v;
  ef_carve_result r;
  p.width = 640; p.height = 480; p.fx = p.fy = 528.f; p.cx = 320.f; p.cy = 240.f; p.min_depth = 0.3f; p.max_depth = 3.f;
  p.margin = 0.02f; p.margin_quad = 0.0025f; p.window = 1; p.min_views = 1; p.protect = 1;
  v.n = EF_CARVE_MAX_VIEWS; v.T_wc16 = 0; v.depth = 0;
  r.participants = r.observed = r.free_space = r.protected_ = r.removed = r.count_after = 0u;
  printf("%d %u %u %u %d %u\n", a != 0 && b != 0 && c != 0 && d != 0 && e != 0, (unsigned)sizeof(p), (unsigned)sizeof(v), (unsigned)sizeof(r),
         v.n + p.window, r.removed);
  return 0;
}
/* 13 and 6 four-byte fields without padding: a negative array size fails the compilation */
typedef char params_are_52_bytes[sizeof(ef_carve_params) == 52 ? 1 : -1];
typedef char result_is_24_bytes[sizeof(ef_carve_result) == 24 ? 1 : -1];
''')
    exe = str(tmp_path / "decl")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe + ".o"],
                   check=True)
    hdr = open(os.path.join(ROOT, "include", "ef_hip.h")).read()
    assert int(hdr.split("#define EF_CARVE_MAX_VIEWS")[1].split()[0]) == cr.MAX_VIEWS


def test_library_and_python_mirror_carry_the_entry_points():
    import ctypes as C
    from elasticfusion_amd import accuracy, api, build
    build.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in ENTRY:
        assert f" {name}\n" in syms, name
    for m in ("carveParams", "carveSelect", "carveSelectDevice", "carveSurfels"):
        assert callable(getattr(api.ElasticFusion, m, None)), m
    assert callable(accuracy.carved_map)
    assert api.CARVE_MAX_VIEWS == cr.MAX_VIEWS
    # the C layouts: thirteen and six 4-byte fields, no padding; {int, pointer, pointer}
    assert C.sizeof(api.ef_carve_params) == 52 and C.sizeof(api.ef_carve_result) == 24 and C.sizeof(api.ef_carve_views) == 24
    assert tuple(f for f, _ in api.ef_carve_params._fields_) == cr.FIELDS
    assert [f for f, _ in api.ef_carve_result._fields_] == ["participants", "observed", "free_space", "protected_", "removed", "count_after"]
    assert [f for f, _ in api.ef_carve_views._fields_] == ["n", "T_wc16", "depth"]
    assert sorted(cr.default_params()) == sorted(cr.FIELDS)


BAD_PARAMS = dict(width_zero="width_and_height", height_4097="width_and_height", fx_nan="intrinsics", cy_inf="intrinsics", margin_nan="margin",
                  margin_negative="margin", margin_quad_negative="margin", margin_quad_nan="margin", min_depth_nan="min_depth",
                  max_depth_nan="min_depth", min_above_max="min_depth", window_negative="window", window_3="window", min_views_zero="min_views",
                  min_views_above_n="min_views")
BAD_VIEWS = dict(n_zero="views.n", n_33="views.n", null_T="null_views.T_wc16", null_depth="null_views.depth", T_nan="non-finite",
                 T_inf_in_the_last_view="non-finite")
BAD_AMONG = dict(among_unknown_bits="unknown_bits", among_conf_nan="confidence_bound_is_NaN", among_box_nan="box_bound_is_NaN",
                 among_radius_nan="radius_bound_is_NaN", among_label_class="label_class_outside", among_T_inf="T_bw_has_a_non-finite")


def test_every_einval_case_is_refused_without_a_gpu():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    code = r'''
import ctypes as C
import numpy as np
from elasticfusion_amd import api
L = api.lib()
u, p, i = C.c_uint32, C.c_void_p, C.c_int
PP, VP, RP, SP = C.POINTER(api.ef_carve_params), C.POINTER(api.ef_carve_views), C.POINTER(api.ef_carve_result), C.POINTER(api.ef_map_selection)
L.ef_map_carve_select.argtypes = L.ef_map_carve_select_dev.argtypes = [p, PP, VP, SP, p, u, p, p]
L.ef_map_carve.argtypes = L.ef_map_carve_dev.argtypes = [p, PP, VP, SP, RP]
L.ef_default_carve_params.argtypes = [p, PP]
z = None
rows = (C.c_uint32 * 8)()
cnt = C.c_uint32(0)
res = api.ef_carve_result()
inf, nan = float("inf"), float("nan")
T = np.tile(np.eye(4).reshape(16), 3)
D = np.full((3, 4, 6), 1000, np.uint16)
def show(name, case, rc):
    print(name, case, rc, (L.ef_last_error(None) or b"").decode().replace(" ", "_"), flush=True)
def par(**kw):
    q = api.ef_carve_params(6, 4, 5.0, 5.0, 3.0, 2.0, 0.3, 3.0, 0.02, 0.0025, 1, 1, 1)
    for k, v in kw.items():
        setattr(q, k, v)
    return q
def views(n=3, T=T, D=D):
    return api.ef_carve_views(n, None if T is None else T.ctypes.data, None if D is None else D.ctypes.data)
def sel(**kw):
    return C.byref(api.ElasticFusion.mapSelection(**kw))
Tnan, Tinf = T.copy(), T.copy()
Tnan[5] = nan
Tinf[2 * 16 + 3] = inf
bad = [("width_zero", par(width=0)), ("height_4097", par(height=4097)), ("fx_nan", par(fx=nan)), ("cy_inf", par(cy=inf)),
       ("margin_nan", par(margin=nan)), ("margin_negative", par(margin=-0.01)), ("margin_quad_negative", par(margin_quad=-1.0)),
       ("margin_quad_nan", par(margin_quad=nan)), ("min_depth_nan", par(min_depth=nan)), ("max_depth_nan", par(max_depth=nan)),
       ("min_above_max", par(min_depth=3.5)), ("window_negative", par(window=-1)), ("window_3", par(window=3)),
       ("min_views_zero", par(min_views=0)), ("min_views_above_n", par(min_views=4))]
bad_views = [("n_zero", views(0)), ("n_33", views(33)), ("null_T", views(T=None)), ("null_depth", views(D=None)), ("T_nan", views(T=Tnan)),
             ("T_inf_in_the_last_view", views(T=Tinf))]
bad_among = [("among_unknown_bits", sel(tests=0x200)), ("among_conf_nan", sel(tests=api.SEL_CONF, conf_min=nan)),
             ("among_box_nan", sel(tests=api.SEL_BOX, box_min=[nan, 0, 0])), ("among_radius_nan", sel(tests=api.SEL_RADIUS, radius_max=nan)),
             ("among_label_class", sel(tests=api.SEL_LABEL, label_class=-1))]
Tbad = api.ElasticFusion.mapSelection(tests=api.SEL_BOX)
Tbad.T_bw[7] = inf
bad_among.append(("among_T_inf", C.byref(Tbad)))
ok, okv = par(), views()
for name in ("ef_map_carve_select", "ef_map_carve_select_dev", "ef_map_carve", "ef_map_carve_dev"):
    fn = getattr(L, name)
    tail = (rows, 8, C.byref(cnt), None) if "select" in name else (C.byref(res),)
    for case, q in bad:
        show(name, case, fn(z, C.byref(q), C.byref(okv), None, *tail))
    for case, v in bad_views:
        show(name, case, fn(z, C.byref(ok), C.byref(v), None, *tail))
    for case, a in bad_among:
        show(name, case, fn(z, C.byref(ok), C.byref(okv), a, *tail))
    show(name, "null_params", fn(z, None, C.byref(okv), None, *tail))
    show(name, "null_views", fn(z, C.byref(ok), None, None, *tail))
    show(name, "null_context", fn(z, C.byref(ok), C.byref(okv), None, *tail))
    if "select" in name:
        show(name, "null_count", fn(z, C.byref(ok), C.byref(okv), None, rows, 8, None, None))
        show(name, "null_rows", fn(z, C.byref(ok), C.byref(okv), None, None, 8, C.byref(cnt), None))
        show(name, "null_context_count_only", fn(z, C.byref(par(window=0, protect=0)), C.byref(okv), sel(tests=api.SEL_INVERT), None, 0, C.byref(cnt), None))
    else:
        show(name, "null_result", fn(z, C.byref(ok), C.byref(okv), None, None))
show("ef_default_carve_params", "null_context", L.ef_default_carve_params(z, C.byref(par())))
'''
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    common = len(BAD_PARAMS) + len(BAD_VIEWS) + len(BAD_AMONG) + 3
    assert len(rows) == 2 * (common + 3) + 2 * (common + 1) + 1, rows
    assert all(int(rc) == -1 for _, _, rc, _ in rows), rows   # EF_EINVAL, never a crash
    assert all(m.startswith(name + ":") for name, _, _, m in rows), rows
    expect = dict(BAD_PARAMS, **BAD_VIEWS, **BAD_AMONG, null_params="null_params", null_views="null_views", null_count="null_count",
                  null_result="null_result", null_rows="null_rows", null_context="null_context", null_context_count_only="null_context")
    seen = {}
    for name, case, _, m in rows:
        assert expect[case] in m, (name, case, m)
        seen.setdefault(name, set()).add(case)
    assert all(set(BAD_PARAMS) | set(BAD_VIEWS) | set(BAD_AMONG) <= seen[n] for n in ENTRY[1:]), seen


# ---- properties of the reference ----
CAM = dict(width=96, height=72, fx=80.0, fy=80.0, cx=48.0, cy=36.0)


def pose(tx=0.0, ty=0.0, tz=0.0, yaw=0.0, pitch=0.0):
    cy_, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    T = np.eye(4)
    T[:3, :3] = Ry @ Rx
    T[:3, 3] = (tx, ty, tz)
    return T


def surfels_at(xyz):
    S = np.zeros((len(xyz), 12), F)
    S[:, :3] = xyz
    S[:, 3] = 12.0
    S[:, 10] = -1.0
    S[:, 11] = 0.005
    return S


def two_planes(n=3000, seed=5):
    rng = np.random.default_rng(seed)
    xyz = np.zeros((n, 3))
    xyz[:, 0] = rng.uniform(-1.2, 1.2, n)
    xyz[:, 1] = rng.uniform(-0.9, 0.9, n)
    xyz[:, 2] = np.where(np.arange(n) % 2 == 0, 2.0, 1.2 + 0.25 * xyz[:, 0])      # a wall, and a slanted plane in front of part of it
    return surfels_at(xyz)


def self_depth(S, T_wc, p):
    """the depth image a camera at T_wc would see if the surfels' centres were all there is: per pixel the minimum of round(1000 z) over the
    centres that project into it (the specification's projection); also the row that wins each pixel"""
    ok, z, u, v, _, _ = cr.project(S[:, :3], T_wc, p)
    mm = np.rint(z.astype(np.float64) * 1000.0)
    ok &= (mm >= 1) & (mm <= 65535)
    img = np.full((p["height"], p["width"]), 1 << 30, np.int64)
    idx = np.nonzero(ok)[0]
    np.minimum.at(img, (v[idx], u[idx]), mm[idx].astype(np.int64))
    wins = np.zeros(len(S), bool)
    wins[idx] = img[v[idx], u[idx]] == mm[idx]
    img[img == 1 << 30] = 0
    return img.astype(np.uint16), wins


POSES = [pose(), pose(tx=0.3, yaw=-0.12), pose(tx=-0.25, ty=0.1, tz=0.2, yaw=0.1, pitch=0.05)]


def test_a_map_is_never_carved_by_depth_images_of_itself():
    S = two_planes()
    for w in (0, 1, 2):
        p = cr.default_params(**CAM, window=w)
        imgs = [self_depth(S, T, p) for T in POSES]
        c = cr.carve(S, [d for d, _ in imgs], POSES, p)
        assert (c["free"] == 0).all() and c["result"]["removed"] == 0, (w, int((c["free"] > 0).sum()))
        won = np.zeros(len(S), bool)
        for k, (d, wins) in enumerate(imgs):
            f, s = cr.view_votes(S[:, :3], POSES[k], d, p)
            assert s[wins].all(), (w, k)            # the row that wins its pixel is what the pixel measured
            won |= wins
        assert won.sum() > len(S) // 2 and (c["support"][won] >= 1).all()


def wall_and_blob(p, n_blob=200, seed=9):
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.linspace(-1.1, 1.1, 70), np.linspace(-0.85, 0.85, 54))
    wall = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 2.0)], 1)
    blob = np.array([0.05, -0.02, 1.0]) + rng.normal(scale=0.06, size=(n_blob, 3))
    S = surfels_at(np.concatenate([wall, blob]))
    depth = np.full((p["height"], p["width"]), 2000, np.uint16)      # rendered from the wall alone: it fills the view
    return S, depth, len(wall)


def test_a_moved_object_goes_and_the_wall_stays():
    p = cr.default_params(**CAM)
    S, depth, n_wall = wall_and_blob(p)
    c = cr.carve(S, [depth], [np.eye(4)], p)
    ok, z, u, v, _, _ = cr.project(S[:, :3], np.eye(4), p)
    blob = np.arange(len(S)) >= n_wall
    assert ok[blob].all() and c["removed"][blob].all() and c["result"]["removed"] == blob.sum() == 200
    assert not c["removed"][~blob].any() and (c["support"][~blob & ok] == 1).all()
    assert c["result"]["protected_"] == 0 and c["result"]["free_space"] == 200 and c["result"]["observed"] == int(ok.sum())
    # a hole in the depth image where the blob's centre falls: nothing is said about those rows
    holed = depth.copy()
    holed[v[blob][0], u[blob][0]] = 0
    c2 = cr.carve(S, [holed], [np.eye(4)], p)
    at_hole = blob & (u == u[blob][0]) & (v == v[blob][0])
    assert at_hole.any() and not c2["removed"][at_hole].any() and (c2["votes"][at_hole] == 0).all()
    assert c2["removed"][blob & ~at_hole].all()      # (a hole inside a window is ignored: the neighbours still go)


def test_monotone_in_min_views_margin_and_protect():
    rng = np.random.default_rng(3)
    S = two_planes(2000, seed=6)
    p0 = cr.default_params(**CAM, protect=0)
    imgs = []
    for T in POSES:
        d, _ = self_depth(S, T, p0)
        imgs.append((d.astype(np.int64) + rng.integers(-60, 400, d.shape) * (d > 0)).clip(0, 65535).astype(np.uint16))   # the scene moved back, unevenly
    base = cr.carve(S, imgs, POSES, p0)["removed"]
    assert 100 < base.sum() < len(S)
    for kw in (dict(min_views=2), dict(min_views=3), dict(margin=0.1), dict(margin_quad=0.05), dict(protect=1)):
        sub = cr.carve(S, imgs, POSES, dict(p0, **kw))["removed"]
        assert (sub <= base).all() and sub.sum() < base.sum(), kw
    assert (cr.carve(S, imgs, POSES, dict(p0, min_views=3))["removed"] <= cr.carve(S, imgs, POSES, dict(p0, min_views=2))["removed"]).all()


def test_rows_are_independent_and_non_participants_are_untouched():
    rng = np.random.default_rng(4)
    p = cr.default_params(**CAM, window=2, protect=0)
    S, depth, n_wall = wall_and_blob(p)
    S[::7, 3] = 2.0
    S[n_wall + 3, 0], S[n_wall + 4, 1], S[n_wall + 5, 2] = np.nan, np.inf, -np.inf
    views = ([depth, depth], [np.eye(4), pose(tx=0.02)])
    full = cr.carve(S, *views, p)
    pick = rng.random(len(S)) < 0.3
    sub = cr.carve(S[pick], *views, p)
    assert np.array_equal(sub["votes"], full["votes"][pick]) and np.array_equal(sub["removed"], full["removed"][pick])
    # a non-finite position: votes {0, 0}, kept, counted nowhere
    bad = np.arange(n_wall + 3, n_wall + 6)
    assert not full["part"][bad].any() and (full["votes"][bad] == 0).all() and full["kept"][bad].all()
    assert full["result"]["participants"] == len(S) - 3 and full["result"]["removed"] == 200 - 3
    # among: the rows it does not select are kept whatever the views say
    among = sr.default_selection(tests=sr.CONF, conf_min=5.0)
    a = cr.carve(S, *views, p, among)
    out = ~sr.select_mask(S, among)
    assert out.sum() > 100 and (a["votes"][out] == 0).all() and a["kept"][out].all() and not a["part"][out].any()
    assert np.array_equal(a["votes"][~out], full["votes"][~out]) and np.array_equal(a["removed"][~out], full["removed"][~out])
    assert a["result"]["participants"] == int((~out).sum()) - 3
    # the window at the image's border is the part of it inside the image: a surfel in the corner texel, the wall behind it, still goes
    z = F(1.0)
    corner = np.array([[(F(0.5) - F(p["cx"])) / F(p["fx"]) * z, (F(0.5) - F(p["cy"])) / F(p["fy"]) * z, z]])
    cc = cr.carve(surfels_at(corner), [depth], [np.eye(4)], p)
    assert cc["votes"].tolist() == [[1, 0]] and cc["rows"].tolist() == [0]


def test_the_oracle_map_survives_its_own_frame_and_phantoms_go(oracle_state, frames):
    """the claim on a real map: with the defaults, frame 2's depth at the oracle's pose removes every phantom placed 0.5 m in front of the
    camera whose centre texel has data, and at most OWN_ROWS_REMOVED_CAP of the map's own rows"""
    M = oracle_state.map()
    T = oracle_state.pose()
    depth = frames[2][1]
    rng = np.random.default_rng(12)
    p = cr.default_params()
    cam = np.stack([rng.uniform(-0.25, 0.25, 500), rng.uniform(-0.2, 0.2, 500), np.full(500, 0.5)], 1)
    phantoms = surfels_at((T[:3, :3] @ cam.T).T + T[:3, 3])
    S = np.concatenate([M, phantoms])
    c = cr.carve(S, [depth], [T], p)
    ph = np.arange(len(S)) >= len(M)
    ok, z, u, v, _, _ = cr.project(S[:, :3], T, p)
    data, zo = cr.has_data(depth[v, u], p)
    seen = ph & ok & data
    own = int(c["removed"][~ph].sum())
    print("map rows", len(M), "own rows removed", own, "phantoms with data", int(seen.sum()), "removed", int(c["removed"][ph].sum()), c["result"])
    assert seen.sum() > 400 and (zo[seen] > 0.6).all()
    assert c["removed"][seen].all() and not c["removed"][ph & ~seen].any()
    assert own <= OWN_ROWS_REMOVED_CAP, own


def test_the_reference_is_quick_enough_for_the_gpu_suite():
    rng = np.random.default_rng(1)
    n = 200000
    p = cr.default_params()
    z = rng.uniform(0.5, 3.0, n)
    S = surfels_at(np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.45, 0.45, n) * z, z], 1))
    D = rng.integers(400, 3500, (3, 480, 640)).astype(np.uint16)
    t0 = time.perf_counter()
    c = cr.carve(S, D, POSES, p)
    dt = time.perf_counter() - t0
    print("200 000 rows x 3 views:", c["result"], f"{dt:.2f} s")
    assert c["result"]["observed"] > 0 and dt < 10
