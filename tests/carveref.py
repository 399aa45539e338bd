"""ef_map_carve / ef_map_carve_select restated in numpy from include/ef_hip.h alone (the section "Carve free space"), shared by
test_carve_host.py and test_gpu_carve.py.  T_cw is formed in double (the transpose and its product with t, in the written order) and rounded to
float32 once; everything per row is float32 with one rounding per operation, in the written order; comparisons with NaN are false.  One pass
over the rows per view and window texel: no loop over rows."""
import numpy as np

import selectref as sr

F = np.float32
MAX_VIEWS = 32
FIELDS = ("width", "height", "fx", "fy", "cx", "cy", "min_depth", "max_depth", "margin", "margin_quad", "window", "min_views", "protect")


def default_params(width=640, height=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, depth_cut=3.0, **kw):
    """ef_default_carve_params as a dict (the camera and the depth cut-off are the context's: the defaults here are ef_default_config's)"""
    p = dict(width=width, height=height, fx=fx, fy=fy, cx=cx, cy=cy, min_depth=0.3, max_depth=depth_cut, margin=0.02, margin_quad=0.0025,
             window=1, min_views=1, protect=1)
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


def tcw(T_wc):
    """the twelve floats of T_cw as [3, 4] float32: Rc[i][j] = T_wc[j][i], tc[i] = -((T_wc[0][i]*t0 + T_wc[1][i]*t1) + T_wc[2][i]*t2)"""
    T = np.asarray(T_wc, np.float64).reshape(4, 4)
    t = [np.float64(T[0, 3]), np.float64(T[1, 3]), np.float64(T[2, 3])]
    out = np.zeros((3, 4), np.float64)
    for i in range(3):
        for j in range(3):
            out[i, j] = T[j, i]
        out[i, 3] = -((T[0, i] * t[0] + T[1, i] * t[1]) + T[2, i] * t[2])
    return out.astype(F)


def camera_point(xyz, Tc):
    p = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return [((Tc[a, 0] * X + Tc[a, 1] * Y) + Tc[a, 2] * Z) + Tc[a, 3] for a in range(3)]


def project(xyz, T_wc, p):
    """(ok, z, u, v, uf, vf): ok = the row has a texel in this view; u, v are 0 where it has none"""
    x, y, z = camera_point(xyz, tcw(T_wc))
    with np.errstate(all="ignore"):
        uf = (F(p["fx"]) * x) / z + F(p["cx"])
        vf = (F(p["fy"]) * y) / z + F(p["cy"])
        ok = (z > 0) & (uf >= 0) & (uf < F(p["width"])) & (vf >= 0) & (vf < F(p["height"]))
    u = np.where(ok, uf, 0).astype(np.int64)
    v = np.where(ok, vf, 0).astype(np.int64)
    return ok, z, u, v, uf, vf


def has_data(d, p):
    zo = d.astype(F) / F(1000.0)
    return (d != 0) & (F(p["min_depth"]) <= zo) & (zo <= F(p["max_depth"])), zo


def tol(zo, p):
    return F(p["margin"]) + (F(p["margin_quad"]) * zo) * zo


def view_votes(xyz, T_wc, depth, p):
    """(free, support): boolean per row, what this one view says"""
    depth = np.ascontiguousarray(depth, np.uint16).reshape(p["height"], p["width"])
    W, H, w = int(p["width"]), int(p["height"]), int(p["window"])
    ok, z, u, v, _, _ = project(xyz, T_wc, p)
    data, zo = has_data(depth[v, u], p)
    centre = ok & data
    with np.errstate(all="ignore"):
        t = tol(zo, p)
        behind, front = (z + t) < zo, (zo + t) < z
        support = centre & ~behind & ~front
        free = centre & behind
        for b in range(-w, w + 1):
            for a in range(-w, w + 1):
                uu, vv = u + a, v + b
                inside = (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
                dat, zq = has_data(depth[np.clip(vv, 0, H - 1), np.clip(uu, 0, W - 1)], p)
                free &= ~(inside & dat) | ((z + tol(zq, p)) < zq)
    return free, support


def participants(surfels, among=None, probs=None):
    S = np.ascontiguousarray(surfels, F).reshape(-1, 12)
    part = np.isfinite(S[:, :3]).all(1)
    if among is not None:
        part &= sr.select_mask(S, among, probs)
    return part


def carve(surfels, depths, poses, params, among=None, probs=None):
    """dict: part / removed / kept (boolean per row), free / support (uint8 per row), votes ([n, 2] uint8), rows (the removed rows, ascending
    uint32), result (ef_carve_result as a dict)"""
    p = params
    S = np.ascontiguousarray(surfels, F).reshape(-1, 12)
    n = len(S)
    T = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    D = np.ascontiguousarray(depths, np.uint16).reshape(-1, p["height"], p["width"])
    assert 1 <= len(T) <= MAX_VIEWS and len(T) == len(D), (T.shape, D.shape)
    part = participants(S, among, probs)
    free, support = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    idx = np.nonzero(part)[0]
    for k in range(len(T)):
        f, s = view_votes(S[idx, :3], T[k], D[k], p)
        free[idx] += f
        support[idx] += s
    free_space = part & (free >= int(p["min_views"]))
    removed = free_space & ~((int(p["protect"]) != 0) & (support > 0))
    res = dict(participants=int(part.sum()), observed=int((part & (free.astype(int) + support > 0)).sum()), free_space=int(free_space.sum()),
               protected_=int((free_space & ~removed).sum()), removed=int(removed.sum()), count_after=n - int(removed.sum()))
    return dict(part=part, free=free, support=support, votes=np.stack([free, support], 1), removed=removed, kept=~removed,
                rows=np.nonzero(removed)[0].astype(np.uint32), result=res)
