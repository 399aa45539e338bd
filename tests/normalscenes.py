"""Hand-built maps for the normal-estimation tests (pure numpy): tests/test_normals_host.py shows on the reference that they contain the edges
they claim, tests/test_gpu_normals.py runs them on the device."""
import numpy as np

from outlierscenes import CONF_HIGH, CONF_LOW, rows_of

F = np.float32
R_EDGE = 2.0 ** -5           # the edge scene's radius: a power of two, so that radius, radius / 16 and the grid's pitch are exact in f32
PITCH = 2.0 ** -8            # the pitch of the bump's grid: radius / 8
KS = (3, 4, 5, 8, 9, 16)     # both sides of every K cut of the join (4 / 8 / 16)
MIN_NEIGHBORS = {3: 2, 4: 3, 5: 5, 8: 5, 9: 5, 16: 5}       # min_neighbors lies in 2 .. k
TIE_KS = (3, 5, 9, 16)       # the k at whose rank the bump's centre has two neighbours of equal d2
R_SPHERE = 0.06
SHIFT = (1000.0, -500.0, 250.0)


def edge_scene(seed=7):
    """(S, marks): a few hundred rows, groups metres apart, shuffled.  marks names the rows of each edge:
    exact / fewer   groups whose rows have exactly 5 and exactly 4 neighbours
    bump, centre    a 7 x 7 grid of pitch PITCH on z = 4 (x^2 + y^2) about `centre`: mirror pairs at equal d2 from the centre
    pair            two rows at one position
    line, slant     collinear rows along x and along (1, 1, 0)
    point           six rows at one position
    triangle        three rows
    bad             rows with a non-finite position
    plane           a patch at z = 1 exactly; perp, zero, nan, down: rows of it whose stored normal is (1, 0, 0), zero, NaN and (0, 0, -1)
    cloud, low      a random surface patch, a quarter of it below the confidence threshold (`low`)
    at_view         a row of the cloud: the viewpoint of the VIEWPOINT runs is its position"""
    rng = np.random.default_rng(seed)
    r = R_EDGE
    parts, marks = [], {}

    def add(name, pts):
        a = sum(len(p) for p in parts)
        parts.append(np.asarray(pts, np.float64).reshape(-1, 3))
        marks[name] = np.arange(a, a + len(parts[-1]))

    add("exact", np.array([3.0, 0.0, 0.0]) + rng.uniform(-0.2, 0.2, (6, 3)) * r)
    add("fewer", np.array([6.0, 0.0, 0.0]) + rng.uniform(-0.2, 0.2, (5, 3)) * r)
    g = (np.arange(7) - 3) * PITCH
    gx, gy = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    add("bump", np.stack([gx + 9.0, gy + 1.0, 4.0 * (gx * gx + gy * gy) + 2.0], 1))      # (every term is exact in f32)
    add("pair", np.array([[12.0, 0.0, 0.0], [12.0, 0.0, 0.0]]) + np.array([0.25, 0.5, 0.125]) * r)
    add("pair_near", np.array([12.0, 0.0, 0.0]) + rng.uniform(0.1, 0.6, (7, 3)) * r)
    add("line", np.array([15.0, 0.0, 0.0]) + np.arange(8)[:, None] * np.array([PITCH, 0.0, 0.0]))
    add("slant", np.array([18.0, 0.0, 0.0]) + np.arange(8)[:, None] * np.array([PITCH, PITCH, 0.0]))
    add("point", np.tile([21.0, 0.5, 0.25], (6, 1)))
    add("triangle", np.array([24.0, 0.0, 0.0]) + np.array([[0.0, 0.0, 0.0], [0.3, 0.1, 0.0], [0.1, 0.4, 0.2]]) * r)
    bad = np.tile([0.1, 0.1, 0.1], (5, 1))
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, :], bad[4, 1] = np.nan, np.inf, -np.inf, np.nan, np.inf
    add("bad", bad)
    pl = rng.uniform(0.0, 3.0 * r, (120, 3)) + np.array([27.0, 0.0, 0.0])
    pl[:, 2] = 1.0
    add("plane", pl)
    xy = rng.uniform(-0.12, 0.12, (300, 2))
    add("cloud", np.stack([xy[:, 0], xy[:, 1], 0.5 + 1.5 * xy[:, 0] ** 2 - xy[:, 1] ** 2 + rng.normal(0.0, 0.0005, 300)], 1))
    n = sum(len(p) for p in parts)
    S = rows_of(n)
    S[:, :3] = np.concatenate(parts).astype(F)
    nrm = rng.normal(size=(n, 3))
    S[:, 8:11] = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F)                    # stored normals on either side of any estimate
    S[marks["plane"], 8:11] = (0.0, 0.0, 1.0)
    perp, zero, nan, down = (marks["plane"][i::30][:3] for i in range(4))
    S[perp, 8:11] = (1.0, 0.0, 0.0)
    S[zero, 8:11] = 0.0
    S[nan, 8:11] = np.nan
    S[down, 8:11] = (0.0, 0.0, -1.0)
    low = marks["cloud"][rng.random(300) < 0.25]
    S[low, 3] = CONF_LOW
    assert CONF_LOW < CONF_HIGH
    perm = rng.permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    S = S[perm]
    out = {k: inv[v] for k, v in marks.items()}
    out.update(centre=int(inv[marks["bump"][24]]), perp=inv[perp], zero=inv[zero], nan=inv[nan], down=inv[down], low=np.sort(inv[low]),
               at_view=int(inv[marks["cloud"][7]]))
    return np.ascontiguousarray(S, F), out


def sphere_scene(n=2048, radius=0.3, noise=0.0, shift=(0.0, 0.0, 0.0), seed=1):
    """(S, radial): n rows on a sphere about `shift` (the same points for every shift, moved in double and rounded once), stored normal = the
    true outward direction; radial = that direction in double"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    rad = radius + (rng.normal(0.0, noise, n) if noise else np.zeros(n))
    S = rows_of(n)
    S[:, :3] = (d * rad[:, None] + np.asarray(shift, np.float64)).astype(F)
    S[:, 8:11] = d.astype(F)
    return S, d


def patch_scene(n, seed):
    """n rows of a random surface patch of the sphere scene's density, a fifth below the confidence threshold, and a few rows alone far away
    (the size steps: 2048 and 2049 rows)"""
    rng = np.random.default_rng(seed)
    S = rows_of(n)
    side = 0.6 * (n / 2048.0) ** 0.5
    xy = rng.uniform(0.0, side, (n, 2))
    S[:, :3] = np.stack([xy[:, 0], xy[:, 1], 1.0 + 0.3 * np.sin(4.0 * xy[:, 0]) * np.cos(3.0 * xy[:, 1])], 1).astype(F)
    m = min(5, n)
    S[:m, :3] += F(5.0) + np.arange(m, dtype=F)[:, None]
    S[rng.random(n) < 0.2, 3] = CONF_LOW
    S[:, 8:11] = (0.0, 0.0, -1.0)
    return S
