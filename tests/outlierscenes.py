"""Hand-built maps for the outlier tests (pure numpy): tests/test_outlier_host.py shows that they contain the edges they claim,
tests/test_gpu_outliers.py runs them on the device."""
import numpy as np

F = np.float32
R_STATS = 2.0 ** -5          # the stats scene's radius: a power of two, so that radius, radius / 16 and the lattice's pitch are exact in f32
R_SUMS = 0.03                # the sums scene's radius: the default
CONF_LOW, CONF_HIGH = 5.0, 20.0      # either side of a context's default confidence threshold (10)
STATS_KS = (1, 4, 5, 8, 16)


def rows_of(n):
    S = np.zeros((n, 12), F)
    S[:, 3] = CONF_HIGH
    S[:, 4] = 0x808080
    S[:, 6] = 1
    S[:, 7] = 2
    S[:, 10] = 1
    S[:, 11] = 0.004
    return S


def step(v, up):
    return np.nextafter(F(v), F(np.inf if up else -np.inf))


def speck_groups(rng, r, most, origin):
    """for m = 0 .. most a speck with exactly m neighbours, each group metres from every other: (points, the specks' positions in them, m)"""
    pts, at, want = [], [], []
    for m in range(most + 1):
        c = np.array(origin, np.float64) + (3.0 * m, 0, 0)
        at.append(len(pts))
        want.append(m)
        pts.append(c)
        for _ in range(m):
            d = rng.normal(size=3)
            pts.append(c + d / np.linalg.norm(d) * rng.uniform(0.2, 0.8) * r)
    return np.array(pts), np.array(at), np.array(want)


def stats_scene(n=1025, seed=5):
    """(S, marks): n rows, shuffled.  marks names the rows of each edge: clump (two lists), pairs [m, 2], lattice, bad, low, specks (rows) with
    speck_neighbours (their wanted counts), rim [3, 2] = (query row, neighbour row) at radius - one float, radius, radius + one float"""
    rng = np.random.default_rng(seed)
    r = R_STATS
    parts, marks = [], {}

    def add(name, pts, conf=None):
        a = sum(len(p) for p, _ in parts)
        parts.append((np.asarray(pts, np.float64), conf))
        marks[name] = np.arange(a, a + len(pts))

    # two clumps of 20 and 24 surfels inside one cell of the grid at cell = radius
    add("clump0", (np.array([16.0, 16.0, 16.0]) + rng.uniform(0.1, 0.3, (20, 3))) * r)
    add("clump1", (np.array([-9.0, 3.0, 40.0]) + rng.uniform(0.6, 0.9, (24, 3))) * r)
    # a 4 x 4 x 4 lattice of pitch radius / 2 on exact multiples of radius / 16 (and of radius): equal distances across cells
    g = np.arange(4) * (r / 2)
    add("lattice", np.stack(np.meshgrid(g + 2.0, g - 1.0, g + 0.5, indexing="ij"), -1).reshape(-1, 3))
    # rows with a non-finite position
    bad = np.tile([0.1, 0.1, 0.1], (6, 1))
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, :], bad[5, 1] = np.nan, np.inf, -np.inf, np.nan, np.nan, np.inf
    add("bad", bad)
    # specks with exactly 0 .. 17 neighbours
    sp, at, want = speck_groups(rng, r, 17, (10.0, -20.0, 3.0))
    add("speckgroups", sp)
    # a neighbour at radius - one float, at radius, at radius + one float: x = 0 on the query, so the difference is the neighbour's x itself
    rim = []
    for i, x in enumerate((step(r, False), F(r), step(r, True))):
        rim += [(0.0, 30.0 + i, 7.0), (float(x), 30.0 + i, 7.0)]
    add("rimpts", rim)
    # the random cloud, a quarter of it below the confidence threshold; coincident pairs: copies of ten of its points
    n_rand = n - sum(len(p) for p, _ in parts) - 10
    assert n_rand >= 650, n_rand
    cloud = rng.uniform(0.0, 0.25, (n_rand, 3))
    add("cloud", cloud)
    add("copies", cloud[:10])
    S = rows_of(n)
    S[:, :3] = np.concatenate([p for p, _ in parts]).astype(F)
    low = marks["cloud"][rng.random(n_rand) < 0.25]
    S[low, 3] = CONF_LOW
    S[marks["speckgroups"][at[3]], 3] = CONF_LOW          # a low-confidence speck is judged all the same
    perm = rng.permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    S = S[perm]
    out = dict(clump=[inv[marks["clump0"]], inv[marks["clump1"]]], lattice=inv[marks["lattice"]], bad=inv[marks["bad"]],
               low=np.sort(inv[low]), specks=inv[marks["speckgroups"][at]], speck_neighbours=want,
               rim=inv[marks["rimpts"]].reshape(3, 2), pairs=np.stack([inv[marks["cloud"][:10]], inv[marks["copies"]]], 1))
    return S, out


def plain_scene(n, seed):
    """n rows of a random cloud of the stats scene's density with a few specks far away (the bucket steps: 2048 and 2049 rows)"""
    rng = np.random.default_rng(seed)
    S = rows_of(n)
    side = 0.25 * (n / 700.0) ** (1 / 3)
    S[:, :3] = rng.uniform(0.0, side, (n, 3)).astype(F)
    S[:7, :3] += F(5.0) + np.arange(7, dtype=F)[:, None]
    S[rng.random(n) < 0.2, 3] = CONF_LOW
    return S


def sums_scene(n=2 * 4096 + 5, seed=11):
    """n rows: a slab dense enough that nearly every row has 8 neighbours within 0.03 m, 60 specks with a few neighbours, 40 lone rows, and
    three rows with a non-finite position, shuffled"""
    rng = np.random.default_rng(seed)
    S = rows_of(n)
    S[:, :3] = rng.uniform(0.0, 1.0, (n, 3)) * (0.5, 0.5, 0.03)
    k = n - 400
    for i in range(60):                       # specks of 1 + (i % 5) rows, 1 cm apart
        c = np.array([3.0 + 0.5 * i, 1.0, 1.0])
        m = 1 + i % 5
        S[k:k + m, :3] = c + rng.uniform(-0.005, 0.005, (m, 3))
        k += m
    S[k:k + 40, :3] = np.array([0.0, -3.0, 0.0]) + np.arange(40)[:, None] * (0.5, 0.0, 0.0)
    k += 40
    S[k, 0], S[k + 1, 1], S[k + 2, 2] = np.nan, np.inf, -np.inf
    S[rng.random(n) < 0.1, 3] = CONF_LOW
    return S[rng.permutation(n)].astype(F)


def sparse_scene(n=600):
    """every row alone: N = 0"""
    S = rows_of(n)
    S[:, :3] = (np.arange(n, dtype=F) * F(0.5))[:, None] * np.array([1.0, 0.0, 0.0], F) + F(0.25)
    return S
