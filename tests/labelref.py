"""Surfel IDs and label fusion restated in numpy from include/ef_hip.h alone (the section "Stable surfel IDs and per-surfel label fusion"),
shared by test_gpu_label_edges.py.  No project code.  Where the device computes in float32 this does too: one rounding per operation, in the
written order, no fused multiply-add; comparisons with NaN are false.  Every function is a plain sequential statement of its rule: a dict
for the alignment, a loop per row for the fusion, a loop per pixel for the gather, none of the kernels' tiling.

Also the hand-built scenes of that suite (gate_scene, turned_scene, corner_scene) and the value recipes of its fusion and gather tests."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
FLT_MAX = np.finfo(np.float32).max
DENORM = np.float32(1e-40)
TINY = np.frombuffer(np.uint32(1).tobytes(), np.float32)[0]   # the smallest denormal


# ---- IDs --------------------------------------------------------------------------------------
def lane_ok(lane, counter=None):
    """the upload rule: a strictly increasing non-zero prefix followed by a zero suffix of z rows, and (counter given: one past every ID the
    context has handed out) room to number that suffix: b + z <= 0xFFFFFFFF for b = max(counter, largest ID + 1)"""
    lane = np.asarray(lane, np.uint32).astype(np.int64)
    nz = np.flatnonzero(lane)
    s = len(nz)
    if s and nz[-1] != s - 1:
        return False            # a zero before a non-zero
    if (np.diff(lane[:s]) <= 0).any():
        return False
    if counter is None:
        return True
    base = max(int(counter), int(lane[s - 1]) + 1) if s else int(counter)
    return base + (len(lane) - s) <= 0xFFFFFFFF


def assign(lane, counter):
    """(lane', counter'): the zero suffix numbered from max(counter, last non-zero + 1), the counter one past the last ID handed out"""
    lane = np.asarray(lane, np.uint32).astype(np.int64)
    assert lane_ok(lane)
    s = int(np.count_nonzero(lane))
    base = int(counter)
    if s:
        base = max(base, int(lane[s - 1]) + 1)
    out = lane.copy()
    out[s:] = base + np.arange(len(lane) - s, dtype=np.int64)
    counter = base + (len(lane) - s)
    assert counter <= 0xFFFFFFFF, "the counter left uint32"
    return out.astype(np.uint32), counter


def spaced_ids(s, first):
    """s increasing IDs from `first` with gaps of 1, 2, 3, 1, 2, 3, ..."""
    return (int(first) + np.concatenate([[0], np.cumsum(1 + np.arange(max(s - 1, 0)) % 3)])[:s]).astype(np.int64)


# ---- alignment --------------------------------------------------------------------------------
def id_rows(ids, C):
    """a distribution derived from each ID (float32), as in test_gpu_labels.py"""
    v = ((np.asarray(ids).astype(np.uint64)[:, None] * 2654435761 + np.arange(C, dtype=np.uint64)[None, :] * 40503) % 997 + 1).astype(np.float32)
    return v / v.sum(1, keepdims=True, dtype=np.float32)


def align(ids_prev, tab_prev, ids_now, C):
    """the table of the current rows: a row whose ID was present at the previous alignment keeps its C floats bit for bit, any other gets 1 / C"""
    ids_prev, ids_now = np.asarray(ids_prev, np.int64), np.asarray(ids_now, np.int64)
    assert (np.diff(ids_prev) > 0).all() and (np.diff(ids_now) > 0).all()
    tab = np.full((len(ids_now), C), F(1) / F(C), np.float32)
    if len(ids_prev):
        k = np.minimum(np.searchsorted(ids_prev, ids_now), len(ids_prev) - 1)
        seen = ids_prev[k] == ids_now
        tab[seen] = np.asarray(tab_prev, np.float32).reshape(-1, C)[k[seen]]
    return tab


def table_rows(ids, C):
    """what the alignment tests store per ID: id_rows, and for C = 1 (where a normalised row is 1, the prior itself) an unnormalised value"""
    if C > 1:
        return id_rows(ids, C)
    return ((np.asarray(ids).astype(np.uint64) * 2654435761 % 997) + 2).astype(np.float32)[:, None]


def filler_map(n):
    """n distinct finite surfels with a zero ID lane"""
    m = np.zeros((n, 12), np.float32)
    k = np.arange(n)
    m[:, 0], m[:, 1], m[:, 2] = (k % 97) * 0.01, (k // 97 % 89) * 0.01, 1.0 + (k // 8633) * 0.01
    m[:, 3], m[:, 6], m[:, 7], m[:, 10], m[:, 11] = 20.0, 1.0, 1.0, -1.0, 0.004
    return m


def with_lane(m, lane):
    m = np.array(m, np.float32, copy=True)
    m[:, 5] = np.asarray(lane, np.uint32).view(np.float32)
    return m


def lane_of(m):
    return np.ascontiguousarray(m[:, 5]).view(np.uint32)


# ---- fusion -----------------------------------------------------------------------------------
def t_cw(T_wc):
    """float T_cw of a rigid T_wc: the inverse in double, every entry rounded once"""
    T = np.asarray(T_wc, np.float64).reshape(4, 4)
    M = np.eye(4)
    M[:3, :3] = T[:3, :3].T
    M[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return M.astype(np.float32)


def project(surfels, T_wc, cam, dtype=np.float32):
    """(p, u, v) per row: p = R x + t with each row of R as (R0 x + R1 y) + R2 z, u = (fx x) / z + cx, v likewise; dtype float64 evaluates the
    same rounded inputs exactly enough to be the yardstick of the float32 evaluation"""
    W, H, fx, fy, cx, cy = cam
    M = t_cw(T_wc).astype(dtype)
    S = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
    x, y, z = (S[:, k].astype(dtype) for k in range(3))
    with np.errstate(all="ignore"):
        p = [((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3] for a in range(3)]
        u = (dtype(F(fx)) * p[0]) / p[2] + dtype(F(cx))
        v = (dtype(F(fy)) * p[1]) / p[2] + dtype(F(cy))
    return np.stack(p, 1), u, v


def pixel_of(surfels, T_wc, cam, dtype=np.float32):
    """(inside, u, v): z > 0 and the floors of the projection inside the image; u, v integers (-1 where not inside)"""
    W, H = cam[0], cam[1]
    p, u, v = project(surfels, T_wc, cam, dtype)
    with np.errstate(invalid="ignore"):
        uf, vf = np.floor(u), np.floor(v)
        inside = (p[:, 2] > 0) & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
    return inside, np.where(inside, uf, -1).astype(np.int64), np.where(inside, vf, -1).astype(np.int64)


def observed(surfels, T_wc, cam, index_image):
    """(obs, u, v): the rows whose own pixel shows them in the view's index image"""
    inside, u, v = pixel_of(surfels, T_wc, cam)
    I = np.asarray(index_image).reshape(cam[1], cam[0])
    obs = np.zeros(len(inside), bool)
    for s in np.flatnonzero(inside):
        obs[s] = int(I[v[s], u[s]]) == s
    return obs, u, v


def fuse(surfels, T_wc, cam, index_image, probs, tab):
    """(tab', obs, updated): for every observed row q_c = p_c o_c, Z = sum of q_c in ascending c from 0, p_c <- q_c / Z iff 0 < Z <= FLT_MAX"""
    obs, u, v = observed(surfels, T_wc, cam, index_image)
    probs = np.asarray(probs, np.float32)
    out = np.array(tab, np.float32, copy=True)
    updated = np.zeros(len(out), bool)
    C = out.shape[1]
    with np.errstate(all="ignore"):
        for s in np.flatnonzero(obs):
            o = probs[:, v[s], u[s]]
            Z = F(0)
            for c in range(C):
                Z = F(Z + F(out[s, c] * o[c]))
            if not (Z > F(0) and Z <= FLT_MAX):
                continue
            for c in range(C):
                out[s, c] = F(F(out[s, c] * o[c]) / Z)
            updated[s] = True
    return out, obs, updated


# ---- gather -----------------------------------------------------------------------------------
def gather(index_image, tab):
    """(label int32, prob float32) per pixel: best = 0, m = row[0]; a later class replaces it only when strictly greater (the first strict
    maximum: ties to the lowest class, a NaN never replaces anything and a NaN at class 0 is never replaced); -1 / 0 where nothing is drawn"""
    I = np.asarray(index_image)
    label = np.full(I.shape, -1, np.int32)
    prob = np.zeros(I.shape, np.float32)
    for pix in np.ndindex(*I.shape):
        s = int(I[pix])
        if s == NONE:
            continue
        row = tab[s]
        best, m = 0, row[0]
        for c in range(1, len(row)):
            if row[c] > m:
                best, m = c, row[c]
        label[pix], prob[pix] = best, m
    return label, prob


# ---- scenes -----------------------------------------------------------------------------------
W, H = 52, 36
GATE_CAM = (W, H, 64.0, 64.0, 26.0, 18.0)       # every x, y a multiple of z / 64: every projection exact in float32 and float64
GATE_VIEW = dict(T_wc=np.eye(4), width=W, height=H, fx=64.0, fy=64.0, cx=26.0, cy=18.0, maxDepth=3.0, drawUnstable=True)


def surfel(x, y, z, radius, conf=20.0):
    r = np.zeros(12, np.float32)
    r[:4] = x, y, z, conf
    r[6:8] = 1.0
    r[8:11] = 0.0, 0.0, -1.0
    r[11] = radius
    return r


def at_pixel(u, v, z):
    """the surfel of GATE_CAM whose centre projects to (u, v) (multiples of z / 64) at depth z, its disc 1.28 pixels wide"""
    x, y = (u - 26.0) * z / 64.0, (v - 18.0) * z / 64.0
    assert x * 64 == round(x * 64) and y * 64 == round(y * 64), (u, v, z)
    return surfel(x, y, z, 0.02 * z)


def gate_scene():
    """(surfels, claims): rows that sit on the gates of the observation test seen from GATE_VIEW, then a grid of plain rows.  claims[name] =
    (row, observed?)"""
    rows, claims = [], {}

    def add(name, rec, seen):
        claims[name] = (len(rows), seen)
        rows.append(rec)

    add("u=0", at_pixel(0, 5, 1), True)
    add("u=cols-1", at_pixel(W - 1, 9, 1), True)
    add("u=cols", at_pixel(W, 13, 1), False)
    add("v=0", at_pixel(8, 0, 1), True)
    add("v=rows-1", at_pixel(12, H - 1, 1), True)
    add("v=rows", at_pixel(7, H, 1), False)
    add("u=-1/2", at_pixel(-0.5, 17, 2), False)
    add("v=-1/2", at_pixel(17, -0.5, 2), False)
    add("corner 0,0", at_pixel(0, 0, 2), True)
    add("corner cols-1,rows-1", at_pixel(W - 1, H - 1, 2), True)
    add("z=0", surfel(0.0, 0.0, 0.0, 0.02), False)
    add("z<0", surfel(0.0, 0.0, -1.0, 0.02), False)
    add("z=nan", surfel(0.0, 0.0, np.nan, 0.02), False)
    add("x=inf", surfel(np.inf, 0.0, 1.0, 0.02), False)
    add("front", at_pixel(20, 10, 1), True)
    add("hidden", at_pixel(20, 10, 2), False)            # the same pixels, farther
    add("winner", at_pixel(30, 20, 1), True)
    add("loser", at_pixel(30.5, 20.5, 2), False)         # the same pixel, farther, another sub-pixel position
    add("twin low", at_pixel(40, 25, 1), True)
    add("twin high", at_pixel(40, 25, 1), False)         # equal depth: the lower row wins
    add("past max_depth", at_pixel(44, 8, 4), False)     # GATE_VIEW's maxDepth is 3
    taken = [(r[0] * 64 / r[2] + 26, r[1] * 64 / r[2] + 18) for r in rows if np.isfinite(r[:3]).all() and r[2] > 0]
    k = 0
    for v in range(2, H, 4):
        for u in range(3, W, 4):
            if all(max(abs(u - a), abs(v - b)) >= 3 for a, b in taken):
                add(f"grid {u},{v}", at_pixel(u, v, 1 + k % 2), True)
                k += 1
    return np.stack(rows), claims


TURN = np.array([[np.cos(np.deg2rad(30.0)), 0, np.sin(np.deg2rad(30.0)), 0], [0, 1, 0, 0],
                 [-np.sin(np.deg2rad(30.0)), 0, np.cos(np.deg2rad(30.0)), 0], [0, 0, 0, 1]])
TURN[:3, 3] = 0.05, -0.02, 0.1
TURNED_CAM = (W, H, 61.7, 63.1, 25.3, 17.6)
TURNED_VIEW = dict(T_wc=TURN, width=W, height=H, fx=61.7, fy=63.1, cx=25.3, cy=17.6, maxDepth=3.0, drawUnstable=True)


def turned_scene():
    """the gate scene's rows and 200 scattered ones, for the view turned by 30 degrees: the general path"""
    rng = np.random.RandomState(77)
    base, _ = gate_scene()
    extra = []
    for _ in range(200):
        z = rng.uniform(0.7, 2.6)
        extra.append(surfel(rng.uniform(-0.2, 1.6) * z, rng.uniform(-0.35, 0.35) * z, z, rng.uniform(0.01, 0.03) * z, conf=rng.choice([5.0, 20.0])))
    return np.concatenate([base, np.stack(extra)])


CORNER_CAM = (W, H, 0.5, 0.5, -0.0, -0.0)
CORNER_VIEW = dict(T_wc=np.eye(4), width=W, height=H, fx=0.5, fy=0.5, cx=-0.0, cy=-0.0, maxDepth=3.0, drawUnstable=True)


def corner_scene():
    """a principal point of -0 at the image corner: 0.5 times the smallest negative denormal rounds to -0, and -0 + -0 = -0, so row 0 projects
    to (-0, -0), which is inside (pixel 0, 0); row 1, one pixel to the left of it, is not"""
    return np.stack([surfel(-TINY, -TINY, 1.0, 2.0), surfel(-2.0, 3.0, 1.0, 2.0), surfel(7.0, 5.0, 1.0, 2.0)])


# ---- value recipes ----------------------------------------------------------------------------
def fusion_recipes(C):
    """[(name, row, observation, updated?)]: C-vectors whose products give the sum named"""
    def vec(first, rest=0.0, second=None):
        a = np.full(C, rest, np.float32)
        a[0] = first
        if second is not None and C > 1:
            a[1] = second
        return a

    rec = [("normal", np.linspace(0.25, 1.0, C).astype(np.float32), np.linspace(1.0, 0.5, C).astype(np.float32), True),
           ("Z=0", vec(0.5, 0.25), vec(0.0, 0.0), False),
           ("Z<0", vec(0.5, 0.25), vec(-1.0, 0.0), False),
           ("Z=nan", vec(0.5, 0.25), vec(np.nan, 1.0), False),
           ("Z=inf by overflow", vec(FLT_MAX, 0.25), vec(2.0, 0.0), False),
           ("Z=inf by an inf", vec(0.5, 0.25), vec(np.inf, 1.0), False),
           ("Z=FLT_MAX", vec(FLT_MAX, 0.25), vec(1.0, 0.0), True),
           ("Z denormal", vec(DENORM, 0.25), vec(1.0, 0.0), True),
           ("Z smallest denormal", vec(TINY, 0.25), vec(1.0, 0.0), True)]
    if C > 1:
        rec += [("negative entry, Z>0", vec(0.5, 0.0, 0.5), vec(-1.0, 0.0, 3.0), True),
                ("inf - inf", vec(0.5, 0.0, 0.5), vec(np.inf, 0.0, -np.inf), False),
                ("overflow in the sum", vec(FLT_MAX, 0.0, FLT_MAX), vec(1.0, 0.0, 1.0), False),
                ("FLT_MAX after cancellation", vec(FLT_MAX, 0.0, 1.0), vec(1.0, 0.0, 1.0), True)]
    return rec


def gather_recipes(C):
    """[(name, row, label)]: rows on the rules of the first strict maximum"""
    nan = np.float32(np.nan)
    base = np.linspace(0.1, 0.2, C).astype(np.float32)

    def put(a, **kv):
        a = np.array(a, np.float32)
        for k, x in kv.items():
            a[int(k[1:]) % C] = x
        return a

    rec = [("all equal", np.full(C, 0.5, np.float32), 0),
           ("negative only", -np.linspace(2.0, 1.0, C).astype(np.float32), C - 1),
           ("negative only, first largest", -np.linspace(1.0, 2.0, C).astype(np.float32), 0),
           ("all nan", np.full(C, nan), 0),
           ("nan at class 0", put(base, _0=nan), 0),
           ("-0 then +0", put(np.zeros(C), _0=-0.0), 0)]
    if C > 2:
        rec += [("tie at 0, 1", put(base, _0=0.9, _1=0.9), 0),
                ("tie at C-2, C-1", put(base, **{f"_{C - 2}": 0.9, f"_{C - 1}": 0.9}), C - 2),
                ("nan at a later class", put(base, _1=nan), C - 1),
                ("nan after the maximum", put(base, _1=0.9, _2=nan), 1),
                ("last class", put(base, **{f"_{C - 1}": 0.9}), C - 1)]
    return rec
