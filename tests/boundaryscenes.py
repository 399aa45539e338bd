"""Hand-built maps for the boundary tests (pure numpy) beside those of normalscenes: tests/test_boundary_host.py shows on the reference that
they contain what they claim, tests/test_gpu_boundary.py runs them on the device."""
import numpy as np

from normalscenes import sphere_scene
from outlierscenes import CONF_HIGH, CONF_LOW, rows_of

F = np.float32
R_EDGE = 2.0 ** -5           # the edge scene's radius: a power of two, so that radius and radius / 16 are exact in f32
U = 2.0 ** -8                # the unit of the edge scene's offsets: radius / 8
KS = (3, 4, 5, 8, 9, 16)     # both sides of every K cut of the join (4 / 8 / 16)
MIN_NEIGHBORS = 2            # of the edge scene, at every k: a row with two neighbours is judged
SPACING = 2.0 ** -6          # the plate's pitch
R_PLATE = 1.5 * SPACING      # exact in f32: the eight surrounding surfels and nothing else (the next ring is at 2 pitches)
PLATE = (12, 10)             # the plate's columns and rows
HOLE = (4, 3, 4, 3)          # the hole: its first column and row, its columns and rows (never at the rim)
R_SPHERE = 0.2               # the radius of the sphere runs: every row of normalscenes' sphere has its 16 nearest inside it, and the rim's rows reach each other
# chosen on the CPU (tests/test_boundary_host.py asserts it of the reference alone): with the sixteen nearest neighbours and a half turn as the
# gap, the closed sphere has no BOUNDARY row and the hemisphere's BOUNDARY rows are one loop along its rim.  (At radius 0.06 seven rows of
# the closed sphere have fewer than sixteen neighbours and a gap above a half turn.)
SPHERE = dict(radius=R_SPHERE, k=16, min_neighbors=5, normal_source=1, max_gap=2.0)


def edge_scene(seed=11):
    """(S, marks): groups metres apart, shuffled; every offset is a small multiple of U, so every double of the definition is exact.  marks
    names ONE row for each edge (the group's centre; its normal is +z unless said) and the bool mask `among`:
    nan_pos         a NaN position: NONE
    excluded        a row `among` leaves out: NONE with the mask, judged without
    sparse          one neighbour: SPARSE at min_neighbors 2
    zero_normal, nan_normal      three neighbours: DEGENERATE
    along           two neighbours, both along the normal: no direction, DEGENERATE
    one_dir         one neighbour along the normal, one in the plane: exactly one direction, G = 4
    opposite        two opposite directions: G = 2 (INTERIOR at max_gap 2: the test is >)
    coincident      two neighbours at one position and a third further along the same ray (three coincident directions, in slots 1, 2 and 4) and one
                    at a right angle: G = 3, found by the highest slot of the group alone
    cross           four neighbours at right angles: a gap of exactly 1
    quadrants       four neighbours whose pairs take every reachable branch of TURN (both signs of d and of c)
    axis0, axis1, axis2, tie     normals +z (|h_0| = |h_1| = 0: the tie goes to axis 0), +x (axis 1), (1, 1, 0) (axis 2), (1, 1, 1) (a three-way tie)
    long_normal     the cross with the normal (0, 0, 2): the gap of `cross`, bit for bit
    low_boundary    one_dir's shape with a confidence below the threshold: BOUNDARY, and in no loop once min_conf is the threshold
    low_neighbour   the cross with one arm below the threshold: G = 1 with every surfel eligible, G = 2 with min_conf at the threshold
    cloud           (many rows) a random surface patch with random normals about +z, a quarter of it below the threshold: counts on both
                    sides of every k"""
    rng = np.random.default_rng(seed)
    pos, nrm, conf, marks = [], [], [], {}
    origin = [0.0]

    def group(name, offsets, normal=(0.0, 0.0, 1.0), centre_conf=CONF_HIGH, low=()):
        o = np.array([origin[0], 0.25, -0.5])
        origin[0] += 1.0
        marks[name] = len(pos)
        pos.append(o)
        nrm.append(normal)
        conf.append(centre_conf)
        for i, d in enumerate(offsets):
            pos.append(o + np.asarray(d, np.float64) * U)
            nrm.append((0.0, 0.0, 1.0))
            conf.append(CONF_LOW if i in low else CONF_HIGH)

    cross = [(2, 0, 0), (0, 2, 0), (-2, 0, 0), (0, -2, 0)]
    group("nan_pos", cross)
    group("excluded", cross)
    group("sparse", [(2, 0, 0)])
    group("zero_normal", cross[:3], normal=(0.0, 0.0, 0.0))
    group("nan_normal", cross[:3], normal=(np.nan, 0.0, 1.0))
    group("along", [(0, 0, 2), (0, 0, -3)])
    group("one_dir", [(0, 0, 2), (3, 0, 0)])
    group("opposite", [(2, 0, 0), (-3, 0, 0)])
    group("coincident", [(1, 0, 0), (1, 0, 0), (3, 0, 0), (0, 2, 0)])
    group("cross", cross)
    group("quadrants", [(4, 2, 0), (-1, 4, 1), (-4, -2, 0), (2, -4, -1)])
    group("axis0", cross)
    group("axis1", [(0, 2, 0), (0, 0, 2), (0, -2, 0), (1, 0, -2)], normal=(1.0, 0.0, 0.0))
    group("axis2", [(2, -2, 0), (0, 0, 2), (-2, 2, 1), (0, 0, -2)], normal=(1.0, 1.0, 0.0))
    group("tie", [(2, -2, 0), (0, 2, -2), (-2, 0, 2), (1, 1, -2)], normal=(1.0, 1.0, 1.0))
    group("long_normal", cross, normal=(0.0, 0.0, 2.0))
    group("low_boundary", [(0, 0, 2), (3, 0, 0)], centre_conf=CONF_LOW)
    group("low_neighbour", cross, low=(3,))
    pos[marks["nan_pos"]] = np.array([np.nan, 0.25, -0.5])
    a = len(pos)
    xy = rng.uniform(-0.12, 0.12, (300, 2))
    cl = np.stack([xy[:, 0] + 40.0, xy[:, 1], 0.5 + 1.5 * xy[:, 0] ** 2 - xy[:, 1] ** 2 + rng.normal(0.0, 0.0005, 300)], 1)
    cn = rng.normal(0.0, 0.3, (300, 3)) + np.array([0.0, 0.0, 1.0])
    pos += list(cl)
    nrm += list(cn)
    conf += list(np.where(rng.random(300) < 0.25, CONF_LOW, CONF_HIGH))
    n = len(pos)
    S = rows_of(n)
    S[:, :3] = np.array(pos).astype(F)
    S[:, 8:11] = np.array(nrm).astype(F)
    S[:, 3] = np.array(conf).astype(F)
    perm = rng.permutation(n)
    # the coincident group relies on its slots: its two twins keep their order (equal d2: the lower row comes first either way) and the third
    # coincident direction is further away, so any permutation leaves "the highest slot of the group" the far one
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    S = np.ascontiguousarray(S[perm], F)
    out = {k: int(inv[v]) for k, v in marks.items()}
    out["cloud"] = np.sort(inv[np.arange(a, n)])
    among = np.ones(n, bool)
    among[out["excluded"]] = False
    out["among"] = among
    return S, out


# the plain plate's analytic G by kind: an inner row sees eight directions 45 degrees apart, a row on a straight edge five over a half turn, a
# convex corner three over a quarter turn, the concave corner of the hole seven (one diagonal missing) and the rows BESIDE a concave corner
# six (the hole takes one straight and one diagonal neighbour: 135 degrees)
PLATE_GAPS = dict(inner=0.5, edge=2.0, convex=3.0, concave=1.0, beside=1.5)
PLATE_KW = dict(radius=R_PLATE, k=8, min_neighbors=3)


def plate_scene(jitter=0.0, seed=3):
    """(S, marks): a regular grid of PLATE surfels of pitch SPACING on the plane z = 1 with the rectangular HOLE cut out, normal +z, in a
    shuffled row order; jitter: a uniform in-plane displacement of at most jitter * SPACING per axis, from a fixed seed.  marks (row arrays):
    inner, edge, convex, concave, beside (by the plain grid's analytic gap, PLATE_GAPS), outer_rim and hole_rim (rim = the rows with at least
    one of the eight surrounding grid positions empty: every row that is not inner; the hole's rim includes its four concave corners)"""
    rng = np.random.default_rng(seed)
    W, H = PLATE
    hx, hy, hw, hh = HOLE
    have = np.ones((W, H), bool)
    have[hx:hx + hw, hy:hy + hh] = False
    pad = np.zeros((W + 2, H + 2), bool)
    pad[1:-1, 1:-1] = have
    cells = [(i, j) for i in range(W) for j in range(H) if have[i, j]]
    kind, ring = [], []
    for i, j in cells:
        nb = [pad[i + 1 + di, j + 1 + dj] for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di, dj) != (0, 0)]
        m = sum(nb)
        kind.append({8: "inner", 5: "edge", 3: "convex", 7: "concave", 6: "beside"}[m])
        ring.append("outer" if i in (0, W - 1) or j in (0, H - 1) else "hole" if m < 8 else "")
    n = len(cells)
    S = rows_of(n)
    P = np.array([(i * SPACING, j * SPACING, 1.0) for i, j in cells])
    if jitter:
        P[:, :2] += rng.uniform(-jitter, jitter, (n, 2)) * SPACING
    S[:, :3] = P.astype(F)
    S[:, 8:11] = (0.0, 0.0, 1.0)
    perm = rng.permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    S = np.ascontiguousarray(S[perm], F)
    kind, ring = np.array(kind), np.array(ring)
    marks = {k: np.sort(inv[np.nonzero(kind == k)[0]]) for k in PLATE_GAPS}
    marks["outer_rim"] = np.sort(inv[np.nonzero(ring == "outer")[0]])
    marks["hole_rim"] = np.sort(inv[np.nonzero(ring == "hole")[0]])
    return S, marks


def hemisphere_scene():
    """(S, radial): the rows of normalscenes' sphere with z >= 0, in their order"""
    S, radial = sphere_scene()
    keep = radial[:, 2] >= 0.0
    return np.ascontiguousarray(S[keep]), radial[keep]


def patch_scene(n, seed):
    """n rows of a random surface patch of the sphere scene's density with the normal (0, 0, -1) stored, a fifth below the confidence
    threshold, and a few rows alone far away (the size steps: 0, 1, 2, 2048 and 2049 rows)"""
    rng = np.random.default_rng(seed)
    S = rows_of(n)
    side = 0.6 * (max(n, 1) / 2048.0) ** 0.5
    xy = rng.uniform(0.0, side, (n, 2))
    S[:, :3] = np.stack([xy[:, 0], xy[:, 1], 1.0 + 0.05 * np.sin(4.0 * xy[:, 0]) * np.cos(3.0 * xy[:, 1])], 1).astype(F)
    m = min(5, n)
    S[:m, :3] += F(5.0) + np.arange(m, dtype=F)[:, None]
    S[rng.random(n) < 0.2, 3] = CONF_LOW
    S[:, 8:11] = (0.0, 0.0, -1.0)
    return S
