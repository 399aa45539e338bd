"""Hand-built maps for the plane tests (pure numpy): tests/test_plane_host.py shows with tests/planeref.py that they contain the edges they
claim, tests/test_gpu_planes.py runs them on the device."""
import numpy as np

from outlierscenes import CONF_HIGH, CONF_LOW, rows_of, step  # noqa: F401

F = np.float32
DIST = 0.01
BASE = dict(seed=12345, hypotheses=256, distance=DIST, min_inliers=200, max_planes=5)   # the base scene's parameters
N_FLOOR, N_WALL, N_PATCH, N_CLUTTER = 1500, 900, 400, 300                              # 3100 rows: no multiple of 64 or of 256
PATCH_N = np.array([np.sqrt(0.75), 0.0, 0.5])                                          # the tilted patch's normal: 30 degrees off horizontal
CHUNK = 2048                                                                           # csrc/ef_map.hpp: PLANE_CHUNK
NORMAL_COS = 0.5                                                                       # exact in f32


def of(pts, normals=None, conf=None):
    S = rows_of(len(pts))
    if len(pts):
        S[:, :3] = np.asarray(pts, np.float64).astype(F)
    if normals is not None:
        S[:, 8:11] = np.asarray(normals, np.float64).astype(F)
    if conf is not None:
        S[:, 3] = conf
    return S


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def base(seed=3):
    """a floor (z = 0), a wall (x = 0), a tilted patch and clutter, each surface with 2 mm of noise, rows shuffled.  (S, part) with
    part[r] in {0: floor, 1: wall, 2: patch, 3: clutter}"""
    rng = np.random.default_rng(seed)
    noise = lambda k: np.clip(rng.normal(0.0, 0.002, k), -0.004, 0.004)
    floor = np.stack([rng.uniform(0.0, 2.0, N_FLOOR), rng.uniform(0.0, 2.0, N_FLOOR), noise(N_FLOOR)], 1)
    wall = np.stack([noise(N_WALL), rng.uniform(0.0, 2.0, N_WALL), rng.uniform(0.05, 1.5, N_WALL)], 1)
    e1, e2 = np.array([0.0, 1.0, 0.0]), np.cross(PATCH_N, [0.0, 1.0, 0.0])
    uv = rng.uniform(-0.25, 0.25, (N_PATCH, 2))
    patch = np.array([1.2, 1.0, 0.6]) + uv[:, :1] * e1 + uv[:, 1:] * e2 + noise(N_PATCH)[:, None] * PATCH_N
    clutter = rng.uniform([0.2, 0.0, 0.1], [2.0, 2.0, 1.5], (N_CLUTTER, 3))
    pts = np.concatenate([floor, wall, patch, clutter])
    nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (N_FLOOR, 1)), np.tile([1.0, 0.0, 0.0], (N_WALL, 1)), np.tile(PATCH_N, (N_PATCH, 1)),
                          unit(rng.normal(size=(N_CLUTTER, 3)))])
    part = np.repeat(np.arange(4), [N_FLOOR, N_WALL, N_PATCH, N_CLUTTER])
    order = rng.permutation(len(pts))
    return of(pts[order], nrm[order]), part[order]


def grid(k, origin, e1, e2, pitch=2.0 ** -6):
    """the first k points of a square grid with an exact f32 pitch spanned by two axis vectors"""
    side = int(np.ceil(np.sqrt(k)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:k]
    return np.asarray(origin, np.float64) + pitch * (ij[:, :1] * np.asarray(e1, np.float64) + ij[:, 1:] * np.asarray(e2, np.float64))


def chunks(seed=5):
    """exact planes whose sizes put the rounds' M on the scoring kernel's chunk edges: 2049 floor rows (z = 0), 1024 wall rows (x = -1) and
    1024 clutter rows well off both: M = 4097 (two chunks and one row), then 2048 (exactly one chunk), then 1024.  Rows shuffled.  (S, part)"""
    rng = np.random.default_rng(seed)
    floor = grid(CHUNK + 1, (0.0, 0.0, 0.0), (1, 0, 0), (0, 1, 0))
    wall = grid(1024, (-1.0, 0.0, 0.25), (0, 1, 0), (0, 0, 1))
    clutter = rng.uniform([-0.75, 0.0, 0.25], [0.9, 0.9, 1.0], (1024, 3))
    pts = np.concatenate([floor, wall, clutter])
    nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (len(floor), 1)), np.tile([1.0, 0.0, 0.0], (1024, 1)), unit(rng.normal(size=(1024, 3)))])
    part = np.repeat(np.arange(3), [len(floor), 1024, 1024])
    order = rng.permutation(len(pts))
    return of(pts[order], nrm[order]), part[order]


def twins(k=400):
    """two disjoint exact planes of k rows each, z = 0 (even rows) and z = 1 (odd rows): every valid hypothesis inside one plane counts
    exactly k, so the round's best count is shared by hypotheses of BOTH planes"""
    a = grid(k, (0.0, 0.0, 0.0), (1, 0, 0), (0, 1, 0))
    b = grid(k, (0.5, 0.25, 1.0), (1, 0, 0), (0, 1, 0))
    pts = np.empty((2 * k, 3))
    pts[0::2], pts[1::2] = a, b
    return of(pts)


def thresholds(k=600):
    """the exact floor z = 0 (normal (0, 0, 1)) and, in its own rows at the end, probes: marks = dict(at, beyond, below_at, below_beyond: rows at
    z = +-distance exactly and one f32 step further; cos_at, cos_below: rows ON the floor whose normal's z is NORMAL_COS exactly and one
    step less; good: a floor row with a full normal).  Every hypothesis inside the floor is (0, 0, +-1, -+0): e = +-z exactly."""
    floor = grid(k, (0.0, 0.0, 0.0), (1, 0, 0), (0, 1, 0))
    d = F(DIST)
    probes = np.array([[0.3, 0.3, 0.0]] * 6, np.float64)
    S = of(np.concatenate([floor, probes]))
    m = dict(at=k, beyond=k + 1, below_at=k + 2, below_beyond=k + 3, cos_at=k + 4, cos_below=k + 5, good=0)
    S[m["at"], 2], S[m["beyond"], 2] = d, step(d, True)
    S[m["below_at"], 2], S[m["below_beyond"], 2] = -d, -step(d, True)
    S[m["cos_at"], 8:11] = (0.0, 0.75, NORMAL_COS)
    S[m["cos_below"], 8:11] = (0.0, 0.75, step(NORMAL_COS, False))
    return S, m


def outsiders(seed=8):
    """the base scene's floor alone (exact, 1200 rows) with rows ON it that must take no part: bad (non-finite positions), low (conf =
    CONF_LOW), boxed (inside the box x >= 4): marks = dict(bad, low, boxed, box_min, box_max)"""
    rng = np.random.default_rng(seed)
    floor = grid(1200, (0.0, 0.0, 0.0), (1, 0, 0), (0, 1, 0))
    extra = np.stack([rng.uniform(0.0, 0.5, 90), rng.uniform(0.0, 0.5, 90), np.zeros(90)], 1)
    extra[60:, 0] += 4.0
    S = of(np.concatenate([floor, extra]))
    bad, low, boxed = np.arange(1200, 1230), np.arange(1230, 1260), np.arange(1260, 1290)
    S[bad[0::3], 0], S[bad[1::3], 1], S[bad[2::3], 2] = np.nan, np.inf, -np.inf
    S[low, 3] = CONF_LOW
    order = rng.permutation(len(S))
    inv = np.argsort(order)
    return S[order], dict(bad=np.sort(inv[bad]), low=np.sort(inv[low]), boxed=np.sort(inv[boxed]), box_min=(3.5, -1.0, -1.0), box_max=(5.0, 1.0, 1.0))


def few(m):
    """m nodes in general position (m <= 3: at most one valid hypothesis exists) behind two rows that are no nodes"""
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])[:m]
    S = of(np.concatenate([[[np.nan, 0.0, 0.0], [0.5, 0.5, 0.0]], pts]))
    S[1, 3] = -2.0            # below the default min_conf of -1
    return S


def coincident(k=50):
    return of(np.tile([[0.25, -0.5, 1.0]], (k, 1)))


def collinear(k=50):
    """k points at an exact pitch on the x axis: every cross product is exactly zero"""
    pts = np.zeros((k, 3))
    pts[:, 0] = np.arange(k) * 0.125
    return of(pts)
