"""Hand-built maps for the region tests (pure numpy): tests/test_regions_host.py shows under the reference that they contain what they claim,
tests/test_gpu_regions.py runs them on the device.  Every scene is small enough for the brute-force reference and spans several workgroups.
The references are computed once per process and shared (ref_of)."""
import functools

import numpy as np

import regionref as rref
from componentscenes import of_points
from outlierscenes import CONF_HIGH, CONF_LOW, step  # noqa: F401

F = np.float32
R = 0.03                      # the default radius
PITCH = 0.01                  # the lattices' pitch: about 28 surfels within R on a face
R_EXACT = 2.0 ** -5           # the threshold scene's radius: a power of two, so that radius, the pitch radius / 4 and their products are exact
H = R_EXACT / 4


def with_normals(pts, nrm, conf=None):
    S = of_points(pts, conf)
    S[:, 8:11] = np.asarray(nrm, np.float64).astype(F)
    return S


def shuffled(S, marks, seed):
    """rows shuffled; marks (name -> rows, arrays or tuples of arrays) renumbered"""
    n = len(S)
    perm = np.random.default_rng(seed).permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    ren = lambda v: tuple(ren(x) for x in v) if isinstance(v, tuple) else inv[np.asarray(v, np.int64)]
    return S[perm], {k: ren(v) for k, v in marks.items()}


def face(m, origin, u, v, jitter, rng):
    """m x m jittered lattice points origin + (i + 0.5) PITCH u + (j + 0.5) PITCH v"""
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    a = (i.reshape(-1) + 0.5 + rng.uniform(-jitter, jitter, m * m)) * PITCH
    b = (j.reshape(-1) + 0.5 + rng.uniform(-jitter, jitter, m * m)) * PITCH
    return np.asarray(origin, np.float64) + a[:, None] * np.asarray(u, np.float64) + b[:, None] * np.asarray(v, np.float64)


def box_corner(m=30, seed=3):
    """(S, marks): three perpendicular m x m faces meeting in three edges and a corner at the origin, normals pointing into the positive octant,
    and six rows that are no nodes inside the faces (non-finite positions, a NaN and a low confidence).  marks: faces = (rows of z = 0, x = 0,
    y = 0), bad"""
    rng = np.random.default_rng(seed)
    fz = face(m, (0, 0, 0), (1, 0, 0), (0, 1, 0), 0.3, rng)
    fx = face(m, (0, 0, 0), (0, 1, 0), (0, 0, 1), 0.3, rng)
    fy = face(m, (0, 0, 0), (1, 0, 0), (0, 0, 1), 0.3, rng)
    bad = np.array([[0.1, 0.1, 0.0], [0.0, 0.1, 0.1], [0.1, 0.0, 0.1], [0.2, 0.2, 0.0], [0.0, 0.2, 0.2], [0.15, 0.15, 0.0]])
    pts = np.concatenate([fz, fx, fy, bad])
    nrm = np.concatenate([np.tile([0, 0, 1.0], (m * m, 1)), np.tile([1.0, 0, 0], (m * m, 1)), np.tile([0, 1.0, 0], (m * m, 1)),
                          [[0, 0, 1.0], [1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, 0, 0], [0, 0, 1.0]]])   # (each bad row has its face's normal)
    S = with_normals(pts, nrm)
    b0 = 3 * m * m
    S[b0, 0], S[b0 + 1, 1], S[b0 + 2, :3] = np.nan, np.inf, -np.inf
    S[b0 + 3, 3], S[b0 + 4, 3], S[b0 + 5, 3] = np.nan, CONF_LOW, CONF_LOW
    marks = dict(faces=(np.arange(m * m), np.arange(m * m, 2 * m * m), np.arange(2 * m * m, b0)), bad=np.arange(b0, b0 + 6))
    return shuffled(S, marks, seed)


def box_band(S):
    """mapSelection keywords of a box that cuts a band 2 R wide out of the face z = 0 (with EF_SEL_INVERT: the face falls into two regions)"""
    return dict(box_min=[0.12, -1.0, -0.001], box_max=[0.12 + 2 * R, 1.0, 0.001])


def cylinder_on_plane(seed=4):
    """(S, marks): the side of a cylinder of radius 0.08 and height 0.2 standing on the plane z = 0, which has a hole where the cylinder
    stands.  marks: side, plane"""
    rng = np.random.default_rng(seed)
    rad, around, up = 0.08, 50, 20
    a, k = np.meshgrid(np.arange(around), np.arange(up), indexing="ij")
    ang = (a.reshape(-1) + rng.uniform(-0.2, 0.2, around * up)) * (2 * np.pi / around)
    z = (k.reshape(-1) + 0.5 + rng.uniform(-0.2, 0.2, around * up)) * PITCH
    side = np.stack([rad * np.cos(ang), rad * np.sin(ang), z], 1)
    side_n = np.stack([np.cos(ang), np.sin(ang), np.zeros_like(ang)], 1)
    plane = face(44, (-0.22, -0.22, 0), (1, 0, 0), (0, 1, 0), 0.2, rng)
    plane = plane[np.hypot(plane[:, 0], plane[:, 1]) > rad + 0.004]
    S = with_normals(np.concatenate([side, plane]), np.concatenate([side_n, np.tile([0, 0, 1.0], (len(plane), 1))]))
    return shuffled(S, dict(side=np.arange(len(side)), plane=np.arange(len(side), len(S))), seed)


def thin_wall(m=26, seed=5):
    """(S, marks): two m x m sheets 4 mm apart with opposite stored normals.  marks: sheets = (rows of the lower, of the upper)"""
    rng = np.random.default_rng(seed)
    lo = face(m, (0, 0, 0), (1, 0, 0), (0, 1, 0), 0.2, rng)
    hi = face(m, (0.003, 0.004, 0.004), (1, 0, 0), (0, 1, 0), 0.2, rng)
    S = with_normals(np.concatenate([lo, hi]), np.concatenate([np.tile([0, 0, -1.0], (m * m, 1)), np.tile([0, 0, 1.0], (m * m, 1))]))
    return shuffled(S, dict(sheets=(np.arange(m * m), np.arange(m * m, 2 * m * m))), seed)


N_SPECKS = 5
RIBBON = (4, 600)


def core_chain(order, seed=6):
    """(S, marks): a flat ribbon 4 surfels wide and 600 long, every surfel a core, its cross-sections numbered along it in the given order
    ("ascending", "descending", "shuffled"), behind five isolated specks in rows 0 .. 4 that are no nodes.  marks: ribbon, specks"""
    w, n = RIBBON
    place = np.arange(n)
    if order == "descending":
        place = place[::-1].copy()
    elif order == "shuffled":
        place = np.random.default_rng(seed).permutation(n)
    else:
        assert order == "ascending"
    j = np.tile(np.arange(w), n)
    pts = np.stack([(np.repeat(place, w) - 40.0) * PITCH, j * PITCH, np.full(w * n, -0.25)], 1)
    specks = np.array([[5.0 + i, 7.0, 3.0] for i in range(N_SPECKS)])
    S = with_normals(np.concatenate([specks, pts]), np.tile([0, 0, 1.0], (N_SPECKS + w * n, 1)))
    return S, dict(specks=np.arange(N_SPECKS), ribbon=np.arange(N_SPECKS, len(S)))


def rough_strip(m=28, seed=8):
    """(S, marks): two coplanar flat m x m patches either side of a strip 8 surfels wide whose heights are rough (+-12 mm): the strip's surfels
    and the patches' rims are borders, and every core of one patch is farther than R from every core of the other.  All stored normals are
    +z.  marks: patches = (left, right), strip"""
    rng = np.random.default_rng(seed)
    left = face(m, (0, 0, 0), (1, 0, 0), (0, 1, 0), 0.2, rng)
    right = face(m, ((m + 8) * PITCH, 0, 0), (1, 0, 0), (0, 1, 0), 0.2, rng)
    i, j = np.meshgrid(np.arange(8), np.arange(m), indexing="ij")
    strip = np.stack([(m + i.reshape(-1) + 0.5) * PITCH, (j.reshape(-1) + 0.5) * PITCH, rng.uniform(-0.012, 0.012, 8 * m)], 1)
    S = with_normals(np.concatenate([left, right, strip]), np.tile([0, 0, 1.0], (2 * m * m + 8 * m, 1)))
    return shuffled(S, dict(patches=(np.arange(m * m), np.arange(m * m, 2 * m * m)), strip=np.arange(2 * m * m, len(S))), seed)


def patch_exact(nx, ny, x0, y0, z=1.0):
    """an nx x ny lattice of pitch H = R_EXACT / 4 from (x0, y0) on: every coordinate a multiple of H (exact in f32)"""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return np.stack([x0 + i.reshape(-1) * H, y0 + j.reshape(-1) * H, np.full(nx * ny, z)], 1)


def thresholds(seed=9):
    """(S, marks): pieces metres apart, all flat (every estimated curvature is 0 but the tie's), for EF_REGIONS_STORED at radius R_EXACT:
      dot     two 12 x 12 patches that meet corner to corner: the corners (marks dot_pair) are the only pair within the radius; the second
              patch's stored normal is tilted by 10 degrees
      at_r    two 12 x 12 patches whose facing columns are exactly R_EXACT apart (d2 == r2 in f32: marks at_r = a facing pair)
      beyond  the same, one float farther apart (marks beyond = a facing pair)
      tie     two 12 x 12 patches 6 H apart, mirror images of each other, and between them the row `tie_b` with six rows above and below it
              that make it a border: its nearest cores (marks tie_cores) are one in each patch, at equal d2 bits
      nan, zero   a core in the middle of the dot scene's first patch with a NaN, and one with a zero stored normal"""
    parts, normals, marks = [], [], {}

    def add(name, pts, nrm=(0, 0, 1.0)):
        a = sum(len(p) for p in parts)
        parts.append(np.asarray(pts, np.float64).reshape(-1, 3))
        normals.append(np.tile(np.asarray(nrm, np.float64), (len(parts[-1]), 1)))
        marks[name] = np.arange(a, a + len(parts[-1]))

    tilt = (np.sin(np.radians(10.0)), 0.0, np.cos(np.radians(10.0)))
    add("dot_a", patch_exact(12, 12, -11 * H, -11 * H))                       # its corner (0, 0)
    add("dot_b", patch_exact(12, 12, 2 * H, 3 * H), tilt)                     # its corner (2 H, 3 H): 3.6 H from (0, 0), every other pair > 4 H apart
    add("at_r_a", patch_exact(12, 12, -11 * H, 10.0))
    add("at_r_b", patch_exact(12, 12, 4 * H, 10.0))                           # columns x = 0 and x = 4 H = R_EXACT
    add("beyond_a", patch_exact(12, 12, -11 * H, 20.0))
    far = patch_exact(12, 12, 0.0, 20.0)
    far[:, 0] = far[:, 0] + float(step(R_EXACT, True))                        # x = nextafter(R_EXACT) + i H: the first column one float beyond
    add("beyond_b", far)
    add("tie_a", patch_exact(12, 12, -14 * H, 30.0 - 6 * H))                  # x = -14 H .. -3 H
    add("tie_c", patch_exact(12, 12, 3 * H, 30.0 - 6 * H))                    # x = 3 H .. 14 H
    add("tie_b", [(0.0, 30.0, 1.0)])
    add("tie_e", [(0.0, 30.0 + dy * H, 1.0 + dz * 2 * H) for dy in (-1, 0, 1) for dz in (-1, 1)])
    S = with_normals(np.concatenate(parts), np.concatenate(normals))
    at = lambda name, x, y: marks[name][np.nonzero((np.abs(parts_of[name][:, 0] - x) < 1e-9) & (np.abs(parts_of[name][:, 1] - y) < 1e-9))[0]]
    parts_of = dict(zip(marks, parts))
    out = dict(marks)
    out["dot_pair"] = np.concatenate([at("dot_a", 0.0, 0.0), at("dot_b", 2 * H, 3 * H)])
    out["at_r"] = np.concatenate([at("at_r_a", 0.0, 10.0 + 5 * H), at("at_r_b", 4 * H, 10.0 + 5 * H)])
    out["beyond"] = np.concatenate([at("beyond_a", 0.0, 20.0 + 5 * H), marks["beyond_b"][[5]]])
    out["tie_cores"] = np.concatenate([at("tie_a", -3 * H, 30.0), at("tie_c", 3 * H, 30.0)])
    out["nan"] = at("dot_a", -6 * H, -6 * H)
    out["zero"] = at("dot_a", -5 * H, -3 * H)
    S[out["nan"], 8:11] = np.nan
    S[out["zero"], 8:11] = 0.0
    assert all(len(out[k]) == n for k, n in (("dot_pair", 2), ("at_r", 2), ("beyond", 2), ("tie_cores", 2), ("nan", 1), ("zero", 1)))
    return shuffled(S, out, seed)


THRESHOLD_KW = dict(radius=R_EXACT, cell=R_EXACT, normal_source=rref.STORED, min_size=1)
# the components' edge scene (componentscenes.edge_scene) under the regions: most of its pieces are too small for an estimate, its cloud and
# its colliding groups give a few rough nodes, which these parameters make cores that are smooth with each other
EDGE_KW = dict(k=5, min_neighbors=2, max_curvature=0.3, min_normal_cos=0.0, two_sided=1, min_size=3)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(S, marks) of a scene by name, built once"""
    if name.startswith("chain_"):
        return core_chain(name[len("chain_"):])
    if name == "edge":
        from componentscenes import edge_scene
        return edge_scene()
    return dict(box=box_corner, cylinder=cylinder_on_plane, wall=thin_wall, strip=rough_strip, thresholds=thresholds)[name]()


_estimates, _refs = {}, {}


def ref_of(name, among=None, among_key=None, **kw):
    """the reference's regions of a scene with these parameters (cell is no parameter of the reference), computed once per process; the
    estimate is shared among the parameter sets that have its five fields in common.  among: a bool mask, named by among_key"""
    kw = {k: v for k, v in kw.items() if k != "cell"}
    S, _ = scene(name)
    p = dict(rref.DEFAULTS, **kw)
    ekey = (name, among_key) + tuple(float(p[k]) for k in rref.ESTIMATE_KEYS)
    if ekey not in _estimates:
        _estimates[ekey] = rref.estimate(S, among, **kw)
    key = (name, among_key) + tuple(sorted((k, float(v)) for k, v in p.items()))
    if key not in _refs:
        _refs[key] = rref.regions(S, among, est=_estimates[ekey], **kw)
    return _refs[key]
