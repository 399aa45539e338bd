"""Hand-built maps for the component tests (pure numpy): tests/test_components_host.py shows that they contain the edges they claim,
tests/test_gpu_components.py runs them on the device."""
import numpy as np

from outlierscenes import CONF_HIGH, CONF_LOW, rows_of, step  # noqa: F401

F = np.float32
R = 0.03                     # the chains', the sheet's and the clouds' radius: the default
R_EDGE = 0.25                # the edge scene's radius: a power of two, so that radius, radius / 16 and 0.25 apart on an axis are exact in f32
N_CHAIN = 3000
SHEET = 96
N_CLOUD = 20000
R_CLOUD = 0.0335             # 20 000 uniform points in the unit cube: a mean of 3.1 neighbours, just above the percolation threshold (2.7)
SIZES = (0, 1, 64, 65, 256, 257, 2048, 2049)


def of_points(pts, conf=None):
    S = rows_of(len(pts))
    if len(pts):
        S[:, :3] = np.asarray(pts, np.float64).astype(F)
    if conf is not None:
        S[:, 3] = conf
    return S


def chain(order, n=N_CHAIN, seed=7):
    """n surfels on a line along x at spacing 0.9 R, from x = -40 R on (negative and positive cells, a bucket per surfel at cell = R).
    order: "ascending" (row i at the i-th place), "descending" (row 0 at the far end) or "shuffled".  (S, place of every row)"""
    place = np.arange(n)
    if order == "descending":
        place = place[::-1].copy()
    elif order == "shuffled":
        place = np.random.default_rng(seed).permutation(n)
    else:
        assert order == "ascending"
    pts = np.zeros((n, 3))
    pts[:, 0] = (place - 40 / 0.9) * (0.9 * R)
    pts[:, 1], pts[:, 2] = 0.5 * R, -0.25 * R
    return of_points(pts), place


def sheet(m=SHEET, seed=9):
    """an m x m grid at spacing 0.7 R in the plane z = 1, rows shuffled"""
    g = np.arange(m) * (0.7 * R)
    pts = np.stack(np.meshgrid(g - 1.0, g + 0.5, [1.0], indexing="ij"), -1).reshape(-1, 3)
    return of_points(pts[np.random.default_rng(seed).permutation(len(pts))])


def cloud(n, seed, r=R_CLOUD, n_ref=N_CLOUD):
    """n uniform points of the density of n_ref points in the unit cube (a mean of 3.1 neighbours within r), a fifth of them below the
    confidence threshold"""
    rng = np.random.default_rng(seed)
    side = (n / n_ref) ** (1 / 3) if n else 1.0
    S = of_points(rng.uniform(0.0, side, (n, 3)))
    S[rng.random(n) < 0.2, 3] = CONF_LOW
    return S


def query_buckets(n):
    """csrc/ef_query.inc: the index's number of buckets for n rows"""
    nb = 1024
    while nb < n and nb < (1 << 22):
        nb <<= 1
    return nb


def query_hash(c, mask):
    """csrc/ef_query.inc: the bucket of the integer cell c = (x, y, z)"""
    x, y, z = (int(v) & 0xFFFFFFFF for v in c)
    return (((x * 73856093) & 0xFFFFFFFF) ^ ((y * 19349663) & 0xFFFFFFFF) ^ ((z * 83492791) & 0xFFFFFFFF)) & mask


def colliding_cell(cell_a, mask):
    """a cell more than a hundred cells from cell_a along x whose bucket is cell_a's"""
    want = query_hash(cell_a, mask)
    for x in range(cell_a[0] + 100, cell_a[0] + 100000):
        if query_hash((x, cell_a[1], cell_a[2]), mask) == want:
            return (x, cell_a[1], cell_a[2])
    raise AssertionError("no colliding cell")


CELL_A = (40, 3, -7)


def edge_scene(seed=13):
    """(S, marks): fewer than 1024 rows (1024 buckets), shuffled, every piece metres from every other.  marks names the rows of each piece:
    at_r [2], beyond_r [2], coincident [2], lone [1]; bad (non-finite positions); bridge_among = (left [2], bridge [1], right [2]) and
    bridge_conf likewise (its bridge has CONF_LOW); negative [3] (one component across the cells -1 and -2); far = (joined [2], apart [1])
    beyond the cell clamp; collide = (group in CELL_A, group in the colliding cell); clumps = {size: rows} of isolated clumps"""
    rng = np.random.default_rng(seed)
    r = R_EDGE
    parts, marks, confs = [], {}, []

    def add(name, pts, conf=CONF_HIGH):
        a = sum(len(p) for p in parts)
        parts.append(np.asarray(pts, np.float64).reshape(-1, 3))
        confs.append(np.full(len(parts[-1]), conf))
        marks[name] = np.arange(a, a + len(parts[-1]))

    add("at_r", [(0, 0, 0), (r, 0, 0)])                                         # d2 == r2 exactly: joined
    add("beyond_r", [(0, 10, 0), (float(step(r, True)), 10, 0)])               # one float beyond: not joined
    add("coincident", [(1.5, 20, 2.5), (1.5, 20, 2.5)])
    add("lone", [(0, 30, 0)])
    bad = np.tile([0.1, 40.0, 0.1], (5, 1))
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, :], bad[4, 0] = np.nan, np.inf, -np.inf, np.nan, -np.inf
    add("bad", bad)
    for name, y, conf in (("among", 50.0, CONF_HIGH), ("conf", 60.0, CONF_LOW)):   # two pairs joined only through the surfel between them
        add(f"{name}_left", [(0.0, y, 0), (0.8 * r, y, 0)])
        add(f"{name}_bridge", [(1.6 * r, y, 0)], conf)
        add(f"{name}_right", [(2.4 * r, y, 0), (3.2 * r, y, 0)])
    add("negative", [(-0.1, -70.0, -0.2), (-0.3, -70.0, -0.2), (-0.45, -70.1, -0.3)])
    add("far_joined", [(300000.0, 0, 0), (300000.125, 0, 0)])                   # cells beyond +2^20 at cell = radius and below: the clamp's cell
    add("far_apart", [(300000.5, 0, 0)])
    add("far_negative", [(-300000.0, -300000.0, 5.0), (-300000.0, -300000.125, 5.0)])
    n_guess = 700                                                               # (< 1024 rows: 1024 buckets; the host test checks the collision)
    cell_b = colliding_cell(CELL_A, query_buckets(n_guess) - 1)
    for name, c in (("collide_a", CELL_A), ("collide_b", cell_b)):
        add(name, (np.array(c) + rng.uniform(0.3, 0.6, (6, 3))) * r)
    for i, m in enumerate((3, 5, 6, 7)):                                        # isolated clumps of exactly m surfels
        add(f"clump{m}", np.array([5.0 * i, 90.0, 3.0]) + rng.uniform(0.0, 0.2, (m, 3)) * r)
    rest = n_guess - sum(len(p) for p in parts)
    add("cloud", rng.uniform(0.0, 2.2, (rest, 3)) + (0, 120.0, 0))              # a random cloud around its own percolation threshold
    n = sum(len(p) for p in parts)
    assert n == n_guess
    S = of_points(np.concatenate(parts), np.concatenate(confs))
    lowc = marks["cloud"][rng.random(rest) < 0.2]
    S[lowc, 3] = CONF_LOW
    perm = rng.permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    S = S[perm]
    m = {k: inv[v] for k, v in marks.items()}
    out = dict(at_r=m["at_r"], beyond_r=m["beyond_r"], coincident=m["coincident"], lone=m["lone"], bad=m["bad"], negative=m["negative"],
               bridge_among=(m["among_left"], m["among_bridge"], m["among_right"]), bridge_conf=(m["conf_left"], m["conf_bridge"], m["conf_right"]),
               far=(m["far_joined"], m["far_apart"]), far_negative=m["far_negative"], collide=(m["collide_a"], m["collide_b"]), cell_b=cell_b,
               clumps={k: m[f"clump{k}"] for k in (3, 5, 6, 7)}, cloud=m["cloud"])
    return S, out


def bridge_box(S, marks):
    """mapSelection keywords of a box that holds the bridge of bridge_among and no other row"""
    p = S[marks["bridge_among"][1][0], :3].astype(np.float64)
    return dict(box_min=list(p - 0.01), box_max=list(p + 0.01))


def blob(centre, n, seed, spread=0.012):
    """n surfels around a point, dense enough to be one component at the default radius"""
    rng = np.random.default_rng(seed)
    side = spread * max(1.0, (n / 30.0) ** (1 / 3))
    return np.asarray(centre, np.float64) + rng.uniform(-side, side, (n, 3))
