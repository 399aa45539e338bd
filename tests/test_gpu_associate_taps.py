"""Round 10: k_associate evaluates each of the 9 distinct texels of a fused pixel's 16 taps once and deals them to the lanes of a group
(ASSOC_LANES, ef_map_kernels.hip); the groups' partial selections are combined in rank order.  The cases here are the ones a
de-duplication or a lane split can get wrong, on the smallest images that show them; the bar is the suite's: bit for bit.

Operator tier (k_associate<false>): hand-written index maps against the oracle's efo_fuse.  Every scene sits on its own ANCHOR pixel: the
raw depth of an anchor is a value no other pixel has, and the texels of its scene hold that depth, so only the anchor passes the depth
test on them and the number of tag -1 / -2 candidates is known in advance.  Rank of a texel = a3 * 3 + b3 (texel (i + a3 - 1, j + b3 - 1)),
the order in which the reference's 16 taps first touch it.

Frame tier (k_associate<true>): a 64 x 48 replay through the shipped library and through the `resolve` variant, the map after every frame.
"""
import os

import numpy as np
import pytest

import efo
from test_gpu_ops_tracking import bits_equal

pytestmark = pytest.mark.gpu

FX = FY = 40.0
MAXD = 20.0
WEIGHT = 0.8
FAR = 2000.0          # lateral offset of a texel that passes the depth test at a distance >= 1000 from the ray


def changed_rows(a, b):
    return set(np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[0].tolist())


class Scene:
    """index maps, depth images and surfel rows for one image size and one frame parity"""

    def __init__(self, W, H, tick, n0):
        self.W, self.H, self.tick, self.par = W, H, tick, tick % 2
        self.qc, self.qr = W // 2, H // 2
        self.n0 = np.asarray(n0, np.float32)          # the normal every pixel of the flat filtered depth gets
        self.idx = np.zeros((H, W), np.uint32)
        self.vc = np.zeros((H, W, 4), np.float32)
        self.nr = np.zeros((H, W, 4), np.float32)
        self.dm = np.full((H, W), 1.0, np.float32)    # raw depth: 1 m, an anchor's own value where a scene sits
        self.dmf = np.full((H, W), 1.0, np.float32)   # filtered depth: flat
        self.rows = [np.zeros(12, np.float32)]        # surfel 0: never associated
        self.tags = {}                                # candidate slot r -> expected tag
        self.winners = set()                          # surfel ids the update pass must touch
        self.losers = set()                           # ... and ids on qualifying texels it must leave alone
        self.n_anchor = 0
        free = [(qx, qy) for qx in range(2, self.qc - 2, 2) for qy in range(2, self.qr - 2, 2)]
        self.free = free[::-1]

    # -- building blocks
    def anchor(self, q=None):
        qx, qy = self.free.pop() if q is None else q
        i, j = 2 * qx + self.par, 2 * qy + self.par
        z = np.float32(1.5 + 0.25 * self.n_anchor)
        self.n_anchor += 1
        self.dm[j, i] = z
        return dict(i=i, j=j, z=z, r=qx * self.qr + qy)

    def texel(self, a, rank, dx=0.01, normal=None, sid=None, z=None, at=None):
        """puts a new surfel (or surfel `sid`) on the texel of `rank` of anchor a (or on texel `at`), on a's ray at a's depth, dx to the side"""
        tx, ty = at if at is not None else (a["i"] + rank // 3 - 1, a["j"] + rank % 3 - 1)
        assert 0 <= tx < self.W and 0 <= ty < self.H and self.vc[ty, tx, 2] == 0, (tx, ty)
        z = a["z"] if z is None else z
        xl, yl = (a["i"] + 0.5 - self.W / 2) / FX, (a["j"] + 0.5 - self.H / 2) / FY
        vc = np.array([xl * z + dx, yl * z, z, 1.0], np.float32)
        nr = np.array([*(self.n0 if normal is None else normal), 0.05], np.float32)
        if sid is None:
            sid = len(self.rows)
            self.rows.append(np.concatenate([vc, np.array([float(0x808080), 0, 1, 1], np.float32), np.array([*self.n0, 0.05], np.float32)]))
        self.idx[ty, tx], self.vc[ty, tx], self.nr[ty, tx] = sid, vc, nr
        return sid

    def expect(self, a, tag, winner=None, losers=()):
        self.tags[a["r"]] = tag
        if winner is not None:
            self.winners.add(winner)
        self.losers.update(losers)

    # -- the scenes of the issue
    def build(self):
        # 1. two ids with identical rows on two texels: the earlier RANK wins, although its id is the higher one
        #    (4, 5) and (0, 8): different segments for 2, 4 and 8 lanes; (2, 3): for 4 and 8; (3, 4): for 8 only; (0, 1), (7, 8): one segment
        for lo, hi in ((4, 5), (0, 8), (2, 3), (3, 4), (0, 1), (7, 8)):
            a = self.anchor()
            later = self.texel(a, hi)
            first = self.texel(a, lo)
            assert first > later
            self.rows[first][:] = self.rows[later]
            self.expect(a, -1, winner=first, losers=[later])
        #    ... and a strictly nearer texel of a later rank replaces an earlier one
        a = self.anchor()
        early, late = self.texel(a, 1, dx=0.02), self.texel(a, 6, dx=0.005)
        self.expect(a, -1, winner=late, losers=[early])
        # 2. a texel that passes the depth test at dist >= 1000: alone it is no match, and it does not stand in a nearer one's way
        a = self.anchor()
        self.expect(a, -2, losers=[self.texel(a, 4, dx=FAR)])
        a = self.anchor()
        far, near = self.texel(a, 0, dx=FAR), self.texel(a, 7)
        self.expect(a, -1, winner=near, losers=[far])
        # 3. cang NaN: a zero normal qualifies by |nr.z| < 0.75; a normal whose length overflows (|nr.z| >= 0.75) as the only candidate does not;
        #    nor does an ordinary normal under a pixel whose own normal is 0 / 0 (its filtered depths are all 0)
        a = self.anchor()
        self.expect(a, -1, winner=self.texel(a, 4, normal=(0, 0, 0)))
        a = self.anchor()
        self.expect(a, -2, losers=[self.texel(a, 4, normal=(0, 0, np.inf))])
        a = self.anchor()
        for di, dj in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
            self.dmf[a["j"] + dj, a["i"] + di] = 0
        self.expect(a, -2, losers=[self.texel(a, 4)])
        # 4. the only qualifying texel has the last rank; the first rank
        a = self.anchor()
        self.expect(a, -1, winner=self.texel(a, 8))
        a = self.anchor()
        self.expect(a, -1, winner=self.texel(a, 0))
        # 5. a texel won by surfel 0 (populated maps, index 0) among empty ones
        a = self.anchor()
        self.texel(a, 4, sid=0)
        self.expect(a, -2)
        # 6. two fused pixels pick the same surfel: the first in draw order owns the update
        a, b = self.anchor(), self.anchor()
        s = self.texel(a, 2)
        self.texel(b, 6, sid=s)
        self.expect(a, -1, winner=s)
        self.expect(b, -1)
        # 7. a corner pixel: its clamped taps repeat the border texels.  Identical rows on its own texel and on its inward neighbour in x:
        #    even frames (corner 0, 0) the own texel has ranks {0, 1, 3, 4} and wins; odd frames (corner W-1, H-1) the neighbour has ranks {1, 2}
        a = self.anchor((0, 0) if self.par == 0 else (self.qc - 1, self.qr - 1))
        own = self.texel(a, 4)
        nb = self.texel(a, 4, at=(a["i"] + (1 if self.par == 0 else -1), a["j"]))
        self.rows[nb][:] = self.rows[own]
        self.expect(a, -1, winner=own if self.par == 0 else nb, losers=[nb if self.par == 0 else own])
        self.surf = np.stack(self.rows).astype(np.float32)
        return self


def flat_normal(ocam, W, H, tick):
    """the normal of a pixel of the flat filtered depth image, from the oracle itself (identity pose: world == camera)"""
    z = np.zeros((H, W, 4), np.float32)
    one = np.full((H, W), 1.0, np.float32)
    _, nu = efo.fuse(ocam, np.eye(4), tick, np.zeros((H, W, 3), np.uint8), one, one, np.zeros((H, W), np.uint32), z, z, z, MAXD, WEIGHT,
                     np.zeros((1, 12), np.float32))
    n0 = nu[len(nu) // 2, 8:11]
    assert abs(n0[2]) == 1.0 and n0[0] == 0 and n0[1] == 0, n0
    return n0


@pytest.mark.parametrize("tick", [6, 7])
@pytest.mark.parametrize("size", [(32, 24), (36, 28)])
def test_hand_built_neighbourhoods(size, tick):
    """36 x 28: 18 x 14 = 252 fused pixels — the last wavefront and, for every lane count, the last workgroup are partial."""
    from elasticfusion_amd import api
    W, H = size
    cam, ocam = api.ef_cam(W, H, FX, FY, W / 2, H / 2), efo.make_cam(W, H, FX, FY, W / 2, H / 2)
    sc = Scene(W, H, tick, flat_normal(ocam, W, H, tick)).build()
    rgb = np.random.RandomState(W * 100 + tick).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    ct = np.zeros((H, W, 4), np.float32)
    T = np.eye(4)
    s_ref, nu_ref = efo.fuse(ocam, T, tick, rgb, sc.dm, sc.dmf, sc.idx, sc.vc, ct, sc.nr, MAXD, WEIGHT, sc.surf)
    # the scenes do what they were written for, on the oracle's output, before the device is asked
    assert len(nu_ref) == sc.qc * sc.qr                               # every fused pixel emits: candidate slot == row of nu
    tags = nu_ref[:, 7]
    for r, tag in sc.tags.items():
        assert tags[r] == tag, (r, tag, tags[r])
    n_match = sum(1 for t in sc.tags.values() if t == -1)
    assert n_match == 14 and len(sc.tags) == 18
    assert int((tags == -1).sum()) == n_match and int((tags == -2).sum()) == len(tags) - n_match
    touched = changed_rows(s_ref, sc.surf)
    assert touched == sc.winners and not (touched & sc.losers) and len(sc.winners) == 13   # `best` of every matched pixel, the tied ones included
    assert (sc.idx[sc.vc[..., 2] > 0] == 0).sum() == 1                # the texel won by surfel 0
    # the device
    s_got, nu_got = api.ops.fuse(cam, T, tick, rgb, sc.dm, sc.dmf, sc.idx, sc.vc, ct, sc.nr, MAXD, WEIGHT, sc.surf)
    assert len(nu_got) == len(nu_ref) and bits_equal(nu_got, nu_ref)
    assert bits_equal(s_got, s_ref)


# ---------------------------------------------------------------------------------------------------------------------------------------
# frame tier: the keyed association (and the z-buffer keys its launch clears) against the resolved script
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resolve_lib():
    """libefusion_hip_resolve.so, (re)built when it is missing or older than the kernel sources"""
    from elasticfusion_amd import build
    path = os.path.join(os.path.dirname(build.LIB), "libefusion_hip_resolve.so")
    deps = [os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith((".hip", ".inc", ".hpp", ".h"))] + [build.__file__]
    if not os.path.exists(path) or any(os.path.getmtime(d) > os.path.getmtime(path) for d in deps):
        build.build_variant("resolve", [])
    return path


def replay_maps(api, frames, **kw):
    ef = api.ElasticFusion(**kw)
    maps = []
    for k, (rgb, depth, _) in enumerate(frames):
        ef.processFrame(rgb, depth, k * 33333)
        maps.append(ef.downloadMap())
    ef.close()
    return maps


def test_small_replay_equals_the_resolved_script(resolve_lib):
    """8 free-running 64 x 48 frames: 32 x 24 = 768 fused pixels x ASSOC_LANES lanes clear 3 072 keys of the previous frame's second z-buffer — a
    key left behind shows as a surfel the keep-test counts (or an association) one frame later, so the map after EVERY frame is compared."""
    from elasticfusion_amd import api, synth
    W, H, n = 64, 48, 8
    sq = synth.Sequence(seed=0xEF0004, width=W, height=H)
    frames = [sq.frame(k) for k in range(n)]
    kw = dict(width=W, height=H, fx=sq.fx, fy=sq.fy, cx=sq.cx, cy=sq.cy, confidence=2.0, maxSurfels=1 << 16)
    a = replay_maps(api, frames, **kw)
    api.use_library(resolve_lib)
    try:
        b = replay_maps(api, frames, **kw)
    finally:
        api.use_library(None)
    assert len(a) == len(b) == n
    for k in range(n):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert min(len(m) for m in a) > 500                                # a populated map ...
    assert int((a[-1][:, 3] > 1.5).sum()) > 100                        # ... whose surfels were matched and merged again and again
    assert len({m.tobytes() for m in a}) == n                          # ... and which changes with every frame
