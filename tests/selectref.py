"""The selection of ef_map_select / ef_map_erase restated in numpy from include/ef_hip.h alone (the section "Select, extract and erase
surfels"), shared by test_select_host.py and test_gpu_select.py.  All per-row arithmetic is float32 with one rounding per operation, in the
written order; comparisons with NaN are false; a row is selected iff every enabled test passes, XOR EF_SEL_INVERT."""
import numpy as np

F = np.float32
BOX, CONF, INIT_TIME, LAST_TIME, RADIUS, ID, LABEL, INVERT = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x100
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def default_selection(**kw):
    """ef_default_map_selection as a dict: tests 0, identity, box +-inf, every range covering everything"""
    s = dict(tests=0, T_bw=np.eye(4), box_min=[-np.inf] * 3, box_max=[np.inf] * 3, conf_min=-np.inf, conf_max=np.inf, init_time_min=INT_MIN,
             init_time_max=INT_MAX, last_time_min=INT_MIN, last_time_max=INT_MAX, radius_min=-np.inf, radius_max=np.inf, id_min=0,
             id_max=0xFFFFFFFF, label_class=0, label_min_prob=-np.inf)
    for k, v in kw.items():
        assert k in s, k
        s[k] = v
    return s


def box_coords(xyz, T_bw, dtype=np.float32):
    """b = ((R0*x + R1*y) + R2*z) + t per axis, R and t rounded to float32 once; dtype float64 evaluates the same rounded inputs exactly enough
    to serve as the yardstick of the float32 evaluation"""
    T = np.asarray(T_bw, np.float64).reshape(4, 4).astype(np.float32)
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3).astype(dtype)
    R, t = T[:3, :3].astype(dtype), T[:3, 3].astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1]) + R[a, 2] * p[:, 2]) + t[a] for a in range(3)], 1)


def in_box(b, box_min, box_max):
    lo, hi = np.asarray(box_min, np.float32).astype(b.dtype), np.asarray(box_max, np.float32).astype(b.dtype)
    with np.errstate(invalid="ignore"):
        return ((lo[None, :] <= b) & (b <= hi[None, :])).all(1)


def label_argmax(probs):
    """best = 0, m = p[0]; a later class replaces it only when strictly greater (ties to the lowest class; a NaN never wins)"""
    probs = np.ascontiguousarray(probs, np.float32)
    best = np.zeros(len(probs), np.int64)
    m = probs[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for c in range(1, probs.shape[1]):
            w = probs[:, c] > m
            best[w] = c
            m[w] = probs[w, c]
    return best, m


def rng_ok(lo, v, hi):
    with np.errstate(invalid="ignore"):
        return (lo <= v) & (v <= hi)


def passes(surfels, sel, probs=None):
    """per enabled test bit, the boolean vector of the rows that pass it"""
    S = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
    t = int(sel["tests"])
    out = {}
    if t & BOX:
        out[BOX] = in_box(box_coords(S[:, :3], sel["T_bw"]), sel["box_min"], sel["box_max"])
    if t & CONF:
        out[CONF] = rng_ok(F(sel["conf_min"]), S[:, 3], F(sel["conf_max"]))
    if t & INIT_TIME:
        out[INIT_TIME] = rng_ok(F(sel["init_time_min"]), S[:, 6], F(sel["init_time_max"]))
    if t & LAST_TIME:
        out[LAST_TIME] = rng_ok(F(sel["last_time_min"]), S[:, 7], F(sel["last_time_max"]))
    if t & RADIUS:
        out[RADIUS] = rng_ok(F(sel["radius_min"]), S[:, 11], F(sel["radius_max"]))
    if t & ID:
        ids = np.ascontiguousarray(S[:, 5]).view(np.uint32).astype(np.int64)
        out[ID] = (int(sel["id_min"]) <= ids) & (ids <= int(sel["id_max"]))
    if t & LABEL:
        best, m = label_argmax(probs)
        with np.errstate(invalid="ignore"):
            out[LABEL] = (best == int(sel["label_class"])) & (m >= F(sel["label_min_prob"]))
    return out


def select_mask(surfels, sel, probs=None):
    S = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
    ok = np.ones(len(S), bool)
    for v in passes(S, sel, probs).values():
        ok &= v
    return ok ^ bool(int(sel["tests"]) & INVERT)


def select_rows(surfels, sel, probs=None):
    return np.nonzero(select_mask(surfels, sel, probs))[0].astype(np.uint32)
