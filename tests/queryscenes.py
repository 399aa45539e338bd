"""The scenes of test_gpu_query_variants.py: small maps built so that a wrong group merge, a double count or a broken scan trip moves an
answer.  Every scene is a pure function of its seed; the order of the random draws is part of the scene."""
import numpy as np

F = np.float32
MERGE_CELL = 0.02
MERGE_SETTINGS = ((0.05, -1.0), (0.05, 1.0), (0.02, -1.0))   # (max_dist, min_conf)


def surfels_of(pos, conf=12.0, normals=None):
    """map rows {x y z conf | colour, 0, initTime, lastTime | nx ny nz radius} around the given positions"""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    S = np.zeros((len(pos), 12), F)
    S[:, :3] = pos
    S[:, 3] = conf
    S[:, 6] = S[:, 7] = 1
    S[:, 8:11] = (0.6, 0.0, 0.8) if normals is None else normals
    S[:, 11] = 0.004
    return S


def merge_scene():
    """(surfels 4785 x 12, queries 1021 x 3, first row of the lattice block) at cell 0.02: more than 16 surfels in one cell (clumps), exact ties
    across cells (a lattice of cell corners, queried from the corners and from the cell centres), equal d2 on rows far apart (repeated rows),
    surfels that are nearest but ineligible (confidence 0.5 under min_conf 1), and a query count that leaves the last group of every lane count partial"""
    rng = np.random.default_rng(0x9E7)
    U = rng.uniform(-0.2, 0.2, (3000, 3)).astype(F)
    centres = rng.uniform(-0.2, 0.2, (24, 3)).astype(F)
    clumps = (centres[:, None, :].astype(np.float64) + rng.normal(0, 0.0015, (24, 40, 3))).astype(F).reshape(-1, 3)
    g = np.arange(-4, 5).astype(F) * F(MERGE_CELL)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    repeats = np.repeat(U[rng.choice(3000, 32, replace=False)], 3, 0)
    P = np.concatenate([U, clumps, lattice, repeats]).astype(F)
    n = len(P)
    conf = rng.choice([0.5, 12.0], n, p=[0.3, 0.7])
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    near = (P[rng.integers(0, n, 600)].astype(np.float64) + rng.normal(0, 0.01, (600, 3))).astype(F)
    wide = rng.uniform(-0.3, 0.3, (200, 3)).astype(F)
    corners = lattice[rng.integers(0, len(lattice), 100)]
    c = (np.arange(-4, 4).astype(F) + F(0.5)) * F(MERGE_CELL)
    mids = c[rng.integers(0, 8, (100, 3))]
    Q = np.concatenate([near, wide, corners, mids, centres[:21]]).astype(F)
    assert P.shape == (4785, 3) and Q.shape == (1021, 3)
    return surfels_of(P, conf, nrm.astype(F)), Q, 3000 + 960


def box_scene():
    """(surfels 700 x 12, queries 257 x 3): with cell 0.0625 and max_dist 1.0 (ratio 16, the largest served) a query walks up to 35^3 cells that
    fold onto 1024 buckets, so every bucket is visited about 40 times and only the own-cell test keeps a surfel from being counted 40 times"""
    rng = np.random.default_rng(0xB0C)
    P = rng.uniform(-1.2, 1.2, (700, 3)).astype(F)
    Q = rng.uniform(-1.2, 1.2, (257, 3)).astype(F)
    return surfels_of(P), Q


CLAMP_CELL = 2.0 ** -20   # its inverse is exact, so the cell coordinate reaches the clamp (+-2^20) at |x| = 1


def clamp_scene():
    """891 points (surfels = queries) half a cell apart around (1, -1, 1): x on both sides of the upper clamp, y on both sides of the lower"""
    xs = 1 + np.arange(-64, 65, 4) * 2.0 ** -21
    ys = -1 + np.arange(-16, 17, 4) * 2.0 ** -21
    zs = 1 + np.arange(-4, 5, 4) * 2.0 ** -21
    P64 = np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3)
    P = P64.astype(F)
    assert P.shape == (891, 3) and (P.astype(np.float64) == P64).all()   # exactly representable
    return surfels_of(P), P.copy()


LARGE_N = (1 << 20) + 4097   # 2^21 buckets = 2048 scan tiles: k_scan_chunks takes a second trip


def large_scene():
    """(surfels LARGE_N x 12, queries 320 x 3)"""
    rng = np.random.default_rng(0xC0DE)
    lo, hi = np.array([-2.0, -1.25, 0.0]), np.array([2.0, 1.25, 4.0])
    P = rng.uniform(lo, hi, (LARGE_N, 3)).astype(F)
    near = (P[rng.integers(0, LARGE_N, 256)].astype(np.float64) + rng.normal(0, 0.004, (256, 3))).astype(F)
    wide = rng.uniform(lo - 0.2, hi + 0.2, (64, 3)).astype(F)
    return surfels_of(P), np.concatenate([near, wide]).astype(F)
