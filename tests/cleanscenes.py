"""Hand-built edge scenes for the stages behind association: the update pass (merge_surfel: k_merge, or inside k_index_splat<true>), the
keep-test and compaction of GlobalModel::clean (clean_test / dedupe_taps, k_clean_flags, k_clean_scatter) and the deformation-graph
application (deform_vertex, k_clean_deform).  Importable without a GPU; the companion of tests/splatscenes.py.

A scene carries the inputs of ONE operator call (hand-written index images, surfel rows, candidate rows, a graph) and check(out):
assertions on the ORACLE's result alone that the scene does what it was written for (this element kept, that one removed, this surfel
rewritten, that one untouched).  tests/test_clean_scenes_host.py runs every check without a GPU and compares the oracle with the
reference's compiled shaders; tests/test_gpu_merge_clean_edges.py compares the device with the oracle after the check has passed.

Geometry: fx = fy = 40, identity pose, and elements at z = 1.25, so that z / fx = 1 / 32: a window position u that is a multiple of a
quarter pixel has the camera-space coordinate (u - cx) / 32 exactly, and ((fx * x) / z) + cx gives u back without a rounding.  A scene
that needs an element ON the optical axis (dx = vc.x exactly) moves cx, cy by half a pixel instead of the element.

The keep-test's 16 taps (pixel offsets {-1, -.5, 0, +.5} per axis, texel floor(x + off), clamped) are restated here by tap_weights();
the kernels count 9 texels x multiplicity, so every weight pattern is placed and filled to the count on either side of each rule.
copy_unstable.vert's own float loop over the taps is restated by shader_trips(): evaluated in float32 it runs a fifth time at many
positions, which the specification (4 taps per axis) does not follow, so elements sit where it runs 4 times (whole(), edge(), spots()).

One case of the issue cannot exist: an element that the taps remove and the window rule force-keeps.  The gate in front of the taps asks
for ftime - lastTime < timeDelta and the window rule for ftime - lastTime > timeDelta on the same two floats (a new point's tag -2 opens
the gate with its raw value and is `time` for the rule, so it never reaches the window either).  The window scenes therefore hold the
nearest things that do exist: an element the age rule removes and the window rule keeps, and filled neighbourhoods behind a closed gate.

Frame tier (FrameScene): the map itself is the scene, see there.  TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import itertools

import numpy as np

from splatscenes import F, FX, FY, MAXD, TD_OPEN, down, proj, solve, step_until_changed, up

SIZES = ((36, 28), (52, 36))
Z = F(1.25)
TIME = 30
CONF = F(10.0)
GREY = float(0x808080)
EYE = np.eye(4)
CLEAN_ROW = 256                  # elements per compaction row (one workgroup trip)
BIG = 4096 * 256 + 300           # more rows than the clean kernels have workgroups: the second trip of their row loop


def row(p, conf=20.0, colour=GREY, t_init=5, t_last=TIME, n=(0, 0, -1), rad=0.01):
    return np.array([p[0], p[1], p[2], conf, colour, 0, t_init, t_last, n[0], n[1], n[2], rad], F)


def sentinel(k=0):
    """an element behind the camera, seen this frame: no rule touches it"""
    return row((k, 0, -5.0), t_last=TIME)


def at(u, v, cam, z=Z):
    """the camera-space point at depth z whose window position is exactly (u, v)"""
    return (solve(u, z, FX, cam[4]), solve(v, z, FY, cam[5]), F(z))


def tap_weights(x, y, W, H):
    """{(tx, ty): how many of the 16 taps of an element at window position (x, y) land on that texel}"""
    def axis(c, n):
        w = {}
        for off in (-1.0, -0.5, 0.0, 0.5):
            t = int(np.clip(np.floor(F(F(c) + F(off))), 0, n - 1))
            w[t] = w.get(t, 0) + 1
        return w
    ax, ay = axis(x, W), axis(y, H)
    return {(tx, ty): wx * wy for tx, wx in ax.items() for ty, wy in ay.items()}


def shader_trips(x, n):
    """how often copy_unstable.vert's own tap loop `for(i = x / n - 2 s; i < x / n + 2 s; i += s)`, s = 1 / n * 0.5, runs when every operation is
    rounded to float32 as the compiled shaders round it: 4 by its arithmetic, 5 where the rounding of the running sum leaves the fifth value
    just below the bound.  The specification is 4 taps per axis; scenes whose elements take a fifth trip are compared with
    the oracle and the device only (four_taps)."""
    step = F(F(F(1.0) / F(n)) * F(0.5))
    w = F(step * F(2.0))
    c = F(F(x) / F(n))
    i, end, k = F(c - w), F(c + w), 0
    while i < end:
        i, k = F(i + step), k + 1
    return k


def four_trips(rows, cam):
    """every in-view row's window position makes the shader's loop run 4 times per axis"""
    for r in np.asarray(rows, F).reshape(-1, 12):
        if r[2] > 0:
            u, v = proj(r[0], r[2], FX, cam[4]), proj(r[1], r[2], FY, cam[5])
            if 0 < u < cam[0] and 0 < v < cam[1] and (shader_trips(u, cam[0]) != 4 or shader_trips(v, cam[1]) != 4):
                return False
    return True


def whole(n, frac, start):
    """the integer i nearest to start (3 <= i < n - 3) for which the shader's loop runs 4 times at i + frac on an axis of n pixels"""
    return next(i for i in sorted(range(3, n - 3), key=lambda i: (abs(i - start), i)) if shader_trips(i + frac, n) == 4)


def edge(n, hi):
    """a window coordinate in (0, .5) (hi: in (n - .5, n)) at which the shader's loop runs 4 times, if one of these has it"""
    fr = (0.25, 0.125, 0.375, 0.0625, 0.4375, 0.1875, 0.3125)
    c = [n - f if hi else f for f in fr]
    return next((x for x in c if shader_trips(x, n) == 4), c[0])


def subset_with_sum(weights, target):
    """texels whose weights add up to `target` (None: unreachable)"""
    keys = sorted(weights)
    for n in range(len(keys) + 1):
        for sub in itertools.combinations(keys, n):
            if sum(weights[k] for k in sub) == target:
                return list(sub)
    return None


def reachable(weights):
    keys = sorted(weights)
    return sorted({sum(weights[k] for k in sub) for n in range(len(keys) + 1) for sub in itertools.combinations(keys, n)})


def bits_same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------------
# the keep-test and the compaction (clean)
# ------------------------------------------------------------------------------------------------------------------------------------
class KeepScene:
    """elements = surfel rows then candidate rows, each with the verdict the scene was written for"""
    kind = "clean"

    def __init__(self, name, W, H, time=TIME, conf=CONF, timeDelta=TD_OPEN, cam=None, sentinels=True):
        self.name, self.W, self.H, self.time, self.conf, self.timeDelta = name, W, H, time, F(conf), timeDelta
        self.cam = (W, H, FX, FY, W / 2.0, H / 2.0) if cam is None else cam
        self.idx = np.zeros((H, W), np.uint32)
        self.vc, self.ct, self.nr = (np.zeros((H, W, 4), F) for _ in range(3))
        self.rows, self.cands, self.keep_rows, self.keep_cands = [], [], [], []
        self.sentinels = sentinels
        if sentinels:
            self.element(sentinel(0), True)

    def element(self, r, kept, cand=False):
        (self.cands if cand else self.rows).append(np.asarray(r, F))
        (self.keep_cands if cand else self.keep_rows).append(bool(kept))
        return r

    def fill(self, t, el, rule="cnt", **over):
        """a texel that counts for `rule` against element el (a row), unless `over` says otherwise"""
        tx, ty = t
        assert 0 <= tx < self.W and 0 <= ty < self.H and self.idx[ty, tx] == 0, t
        if rule == "cnt":    # younger surfel just behind the element, within its radius
            f = dict(idx=7, x=el[0], y=el[1], z=F(el[2] + F(0.005)), w=F(11.0), init=F(el[6] - 1), last=F(self.time - 1))
        else:                # a surfel seen THIS frame, more than a centimetre behind the element
            f = dict(idx=7, x=el[0], y=el[1], z=F(el[2] + F(0.02)), w=F(11.0), init=F(el[6]), last=F(self.time))
        f.update(over)
        f["z"] = f.pop("vz", f["z"])
        self.idx[ty, tx] = f["idx"]
        self.vc[ty, tx] = (f["x"], f["y"], f["z"], f["w"])
        self.ct[ty, tx] = (GREY, 0, f["init"], f["last"])
        self.nr[ty, tx] = (0, 0, -1, 0.01)

    def fill_block(self, x0, x1, y0, y1, el, rule="cnt", **over):
        for tx in range(max(x0, 0), min(x1, self.W - 1) + 1):
            for ty in range(max(y0, 0), min(y1, self.H - 1) + 1):
                if self.idx[ty, tx] == 0:
                    self.fill((tx, ty), el, rule, **over)

    def done(self):
        if self.sentinels:
            self.element(sentinel(1), True)
        self.surf = np.stack(self.rows).astype(F) if self.rows else np.zeros((0, 12), F)
        self.nu = np.stack(self.cands).astype(F) if self.cands else np.zeros((0, 12), F)
        self.mask = np.array(self.keep_rows + self.keep_cands, bool)
        self.four_taps = four_trips(np.concatenate([self.surf, self.nu]), self.cam)
        return self

    def expected(self):
        e = np.concatenate([self.surf, self.nu])[self.mask].copy()
        e[e[:, 7] == -2, 7] = self.time                 # a new point's tag is resolved on the way out
        return e

    def run(self, be, cam):
        return be.clean(cam, EYE, self.time, self.idx, self.vc, self.ct, self.nr, float(self.conf), self.timeDelta, MAXD, self.surf, self.nu)

    def check(self, out):
        e = self.expected()
        assert len(out) == len(e), (self.name, len(out), len(e))
        assert bits_same(out, e), (self.name, np.nonzero((out.view(np.uint32) != e.view(np.uint32)).any(axis=1))[0][:8])

    def __repr__(self):
        return f"{self.name}@{self.W}x{self.H}"


def _cam(W, H, shift=0.0):
    """shift: the optical axis at the centre of a pixel near the image's, where the shader's tap loop runs 4 times"""
    if shift:
        return (W, H, FX, FY, whole(W, 0.5, W // 2) + 0.5, whole(H, 0.5, H // 2) + 0.5)
    return (W, H, FX, FY, W / 2.0, H / 2.0)


# -- 1. tap multiplicities -----------------------------------------------------------------------------------------------------------
def placements(W, H):
    """(name, u, v): every pair of fractional parts in the interior, then the borders where the clamp folds taps together"""
    i0, j0 = whole(W, 0.5, 7), whole(H, 0.5, 9)
    fr = (0.0, 0.25, 0.5, 0.75)
    out = [(f"in_{int(a * 100):02d}_{int(b * 100):02d}", whole(W, a, 7) + a, whole(H, b, 9) + b) for a in fr for b in fr]
    xl, xh, yl, yh = edge(W, False), edge(W, True), edge(H, False), edge(H, True)
    out += [("left_50", xl, j0 + 0.5), ("left_00", xl, whole(H, 0.0, 9) + 0.0), ("right_50", xh, j0 + 0.5), ("right_75", xh, whole(H, 0.75, 9) + 0.75),
            ("top_50", i0 + 0.5, yl), ("bottom_50", i0 + 0.5, yh), ("bottom_25", whole(W, 0.25, 7) + 0.25, yh),
            ("corner_00", xl, yl), ("corner_w0", xh, yl), ("corner_0h", xl, yh), ("corner_wh", xh, yh)]
    return out


def tap_scenes(W, H):
    """per placement and per counting rule: the largest fill the rule keeps (8 / 4 where reachable) and the smallest it removes
    (9 / 5 where reachable), weight-0 neighbours filled as well"""
    scenes = []
    exact = {"cnt": 0, "z": 0}
    for pname, u, v in placements(W, H):
        cam = _cam(W, H)
        wts = tap_weights(u, v, W, H)
        assert sum(wts.values()) == 16 and len(wts) <= 9
        sums = reachable(wts)
        for rule, limit in (("cnt", 8), ("z", 4)):
            keep_sum, drop_sum = max(s for s in sums if s <= limit), min(s for s in sums if s > limit)
            if pname.startswith("in_") and pname[3:5] in ("50", "75") and pname[6:8] in ("50", "75"):
                assert (keep_sum, drop_sum) == (limit, limit + 1), (pname, rule)      # (1, 2, 1) x (1, 2, 1): every count is reachable
            exact[rule] += (keep_sum, drop_sum) == (limit, limit + 1)
            for total, kept in ((keep_sum, True), (drop_sum, False)):
                sc = KeepScene(f"taps_{pname}_{rule}{total}", W, H, cam=cam)
                el = sc.element(row(at(u, v, cam)), kept)
                assert proj(el[0], Z, FX, cam[4]) == F(u) and proj(el[1], Z, FY, cam[5]) == F(v)
                for t in subset_with_sum(wts, total):
                    sc.fill(t, el, rule)
                if kept:      # texels next to the neighbourhood that no tap reaches: filled, and they must not count
                    xs, ys = [t[0] for t in wts], [t[1] for t in wts]
                    for tx in range(min(xs) - 1, max(xs) + 2):
                        for ty in range(min(ys) - 1, max(ys) + 2):
                            if (tx, ty) not in wts and 0 <= tx < W and 0 <= ty < H:
                                sc.fill((tx, ty), el, rule)
                sc.weights, sc.total = wts, total
                scenes.append(sc.done())
    assert exact["cnt"] >= 4 and exact["z"] >= 4
    return scenes


# -- 2. every comparison of both counting rules ----------------------------------------------------------------------------------------
def _nine(sc, el, u, v, rule):
    """fills 8 (cnt) or 4 (zCount) of the taps of an element at a (.5, .5) placement and returns the corner texel (weight 1) left for a probe"""
    i, j = int(np.floor(u)), int(np.floor(v))
    wts = tap_weights(u, v, sc.W, sc.H)
    assert wts[(i, j)] == 4 and wts[(i - 1, j)] == 2 and wts[(i, j + 1)] == 2 and wts[(i + 1, j + 1)] == 1
    sc.fill((i, j), el, rule)
    if rule == "cnt":
        sc.fill((i - 1, j), el, rule)
        sc.fill((i, j + 1), el, rule)
    return (i + 1, j + 1)


def steep_normals():
    """normals (a, 0, b) whose normalised z is one float below 0.85f, 0.85f itself and one float above"""
    a = F(np.sqrt(1 - 0.85 ** 2))
    want = {down(0.85): None, F(0.85): None, up(0.85): None}
    b = F(0.85)
    for _ in range(200):
        b = down(b)
    for _ in range(400):
        rn = F(F(1.0) / np.sqrt(F(F(F(a * a) + F(0.0)) + F(b * b))))
        z = F(b * rn)
        if z in want and want[z] is None:
            want[z] = (a, F(0.0), b)
        b = up(b)
    assert all(v is not None for v in want.values()), want
    return [want[down(0.85)], want[F(0.85)], want[up(0.85)]]


def comparison_scenes(W, H):
    scenes = []
    u, v = whole(W, 0.5, 11) + 0.5, whole(H, 0.5, 13) + 0.5

    def one(name, rule, counts, el_kw=None, centre=False, z=Z, **probe):
        """8 (cnt) or 4 (zCount) plain taps and the probe on a texel of weight 1: removed if and only if the probe counts"""
        cam = _cam(W, H, 0.5 if centre else 0.0)
        sc = KeepScene(f"cmp_{name}", W, H, cam=cam)
        uu, vv = (cam[4], cam[5]) if centre else (u, v)
        p = (F(0.0), F(0.0), Z) if centre else at(uu, vv, cam, z)
        el = sc.element(row(p, **(el_kw or {})), not counts)
        sc.fill(_nine(sc, el, uu, vv, rule), el, rule, **probe)
        scenes.append(sc.done())

    t_init = F(5)
    for tag, val, counts in (("below", down(t_init), True), ("at", t_init, False), ("above", up(t_init), False)):
        one(f"cnt_init_time_{tag}", "cnt", counts, init=val)
    for rule in ("cnt", "z"):
        for tag, val, counts in (("below", down(CONF), False), ("at", CONF, False), ("above", up(CONF), True)):
            one(f"{rule}_conf_{tag}", rule, counts, w=val)
        one(f"{rule}_index_zero", rule, False, idx=0)
    for tag, val, counts in (("below", down(Z), False), ("at", Z, False), ("above", up(Z), True)):
        one(f"cnt_behind_{tag}", "cnt", counts, vz=val)
    # vc.z - localPos.z against 0.01f: z = 0.01f and vc.z = 2 z make the difference exactly 0.01f (and its neighbours exact as well)
    z01 = F(0.01)
    assert F(F(2) * z01 - z01) == z01 and F(up(F(2) * z01) - z01) > z01 and F(down(F(2) * z01) - z01) < z01
    for tag, val, c_cnt, c_z in (("below", down(F(2) * z01), True, False), ("at", F(2) * z01, False, False), ("above", up(F(2) * z01), False, True)):
        for rule, counts in (("cnt", c_cnt), ("z", c_z)):
            one(f"{rule}_centimetre_{tag}", rule, counts, z=z01, vz=val)
    # sqrt(dx^2 + dy^2) < radius * 1.4f: the element on the optical axis, so that dx = vc.x
    thr = F(F(0.01) * F(1.4))
    assert F(np.sqrt(F(thr * thr))) == thr
    for axis in ("x", "y", "-x"):
        for tag, val, counts in (("below", down(thr), True), ("at", thr, False), ("above", up(thr), False)):
            val = F(-val) if axis == "-x" else val
            one(f"cnt_radius_{axis}_{tag}", "cnt", counts, centre=True, **({"y": val} if axis == "y" else {"x": val}))
    ft = F(TIME)
    for tag, val, counts in (("below", down(ft), False), ("at", ft, True), ("above", up(ft), False)):
        one(f"z_seen_now_{tag}", "z", counts, last=val)
    for (tag, counts), n in zip((("below", False), ("at", False), ("above", True)), steep_normals()):
        one(f"z_steep_{tag}", "z", counts, el_kw=dict(n=n))
        one(f"z_steep_neg_{tag}", "z", counts, el_kw=dict(n=(n[0], n[1], -n[2])))
    one("z_zero_normal", "z", False, el_kw=dict(n=(0, 0, 0)))
    one("z_plain", "z", True)
    one("cnt_plain", "cnt", True)
    return scenes


# -- 3. the gate in front of the taps -----------------------------------------------------------------------------------------------
def gate_scenes(W, H):
    scenes = []
    cam = _cam(W, H)
    j0, i0 = whole(H, 0.5, 9), whole(W, 0.5, 7)

    def full(name, p, kept, x0, x1, y0, y1, cam_=cam, **kw):
        sc = KeepScene(f"gate_{name}", W, H, cam=cam_, **{k: kw.pop(k) for k in ("timeDelta",) if k in kw})
        cand = kw.pop("cand", False)
        el = sc.element(row(p, **kw), kept, cand=cand)
        sc.fill_block(x0, x1, y0, y1, el, "cnt", **({"z": F(0.005), "x": F(0), "y": F(0)} if p[2] <= F(1e-20) else {}))
        scenes.append(sc.done())

    # x > 0, x < cols, y > 0, y < rows at equality and one float inside
    y_mid = solve(j0 + 0.5, Z, FY, cam[5])
    x_mid = solve(i0 + 0.5, Z, FX, cam[4])
    x_lo, x_hi = solve(0, Z, FX, cam[4]), solve(W, Z, FX, cam[4])
    y_lo, y_hi = solve(0, Z, FY, cam[5]), solve(H, Z, FY, cam[5])
    x_in_lo, x_in_hi = step_until_changed(x_lo, Z, FX, cam[4], +1), step_until_changed(x_hi, Z, FX, cam[4], -1)
    y_in_lo, y_in_hi = step_until_changed(y_lo, Z, FY, cam[5], +1), step_until_changed(y_hi, Z, FY, cam[5], -1)
    assert proj(x_lo, Z, FX, cam[4]) == 0 < proj(x_in_lo, Z, FX, cam[4]) < 1e-4 and W - 1e-4 < proj(x_in_hi, Z, FX, cam[4]) < W == proj(x_hi, Z, FX, cam[4])
    assert proj(y_lo, Z, FY, cam[5]) == 0 < proj(y_in_lo, Z, FY, cam[5]) < 1e-4 and H - 1e-4 < proj(y_in_hi, Z, FY, cam[5]) < H == proj(y_hi, Z, FY, cam[5])
    full("x_at_zero", (x_lo, y_mid, Z), True, 0, 2, j0 - 2, j0 + 2)
    full("x_past_zero", (x_in_lo, y_mid, Z), False, 0, 2, j0 - 2, j0 + 2)
    full("x_at_cols", (x_hi, y_mid, Z), True, W - 3, W - 1, j0 - 2, j0 + 2)
    full("x_before_cols", (x_in_hi, y_mid, Z), False, W - 3, W - 1, j0 - 2, j0 + 2)
    full("y_at_zero", (x_mid, y_lo, Z), True, i0 - 2, i0 + 2, 0, 2)
    full("y_past_zero", (x_mid, y_in_lo, Z), False, i0 - 2, i0 + 2, 0, 2)
    full("y_at_rows", (x_mid, y_hi, Z), True, i0 - 2, i0 + 2, H - 3, H - 1)
    full("y_before_rows", (x_mid, y_in_hi, Z), False, i0 - 2, i0 + 2, H - 3, H - 1)
    # localPos.z at 0 and below; a tiny positive depth passes (the element on the optical axis: x = 0 / z + cx)
    camc = _cam(W, H, 0.5)
    ci, cj = int(camc[4]), int(camc[5])
    for name, z, kept in (("z_plus_zero", F(0.0), True), ("z_minus_zero", F(-0.0), True), ("z_negative", F(-1e-30), True), ("z_tiny", F(1e-30), False)):
        full(name, (F(0), F(0), z), kept, ci - 2, ci + 2, cj - 2, cj + 2, cam_=camc)
    # ftime - ct.w < timeDelta
    p = (x_mid, y_mid, Z)
    for name, last, kept in (("time_inside", TIME - 6, False), ("time_at_delta", TIME - 7, True), ("time_past_delta", TIME - 8, True)):
        full(name, p, kept, i0 - 2, i0 + 2, j0 - 2, j0 + 2, timeDelta=7, t_last=last)
    # a new point's tag enters the gate raw: 30 - (-2) = 32
    full("tag_new_at_delta", p, True, i0 - 2, i0 + 2, j0 - 2, j0 + 2, timeDelta=TIME + 2, t_last=-2, t_init=TIME, cand=True)
    full("tag_new_inside", p, False, i0 - 2, i0 + 2, j0 - 2, j0 + 2, timeDelta=TIME + 3, t_last=-2, t_init=TIME, cand=True)
    return scenes


# -- 4. the time rules, with and without the taps saying "remove" -----------------------------------------------------------------
def spots(W, H):
    return [(3 + 4 * a + 0.5, 3 + 4 * b + 0.5) for b in range((H - 6) // 4 + 1) for a in range((W - 6) // 4 + 1)
            if shader_trips(3 + 4 * a + 0.5, W) == 4 and shader_trips(3 + 4 * b + 0.5, H) == 4]


def time_cases():
    """(name, row keywords, candidate?, kept with silent taps, kept with the taps saying remove) at time 30, timeDelta open"""
    cases = []
    for age, old in ((20, False), (21, True)):
        for tag, c in (("below", down(CONF)), ("at", CONF), ("above", up(CONF))):
            cases.append((f"age{age}_conf_{tag}", dict(t_last=TIME - age, conf=c), False, not (old and c < CONF), False))
    cases.append(("matched", dict(t_last=-1, t_init=TIME), True, False, False))
    cases.append(("new", dict(t_last=-2, t_init=TIME), True, True, False))
    cases.append(("new_low_conf", dict(t_last=-2, t_init=TIME, conf=0.5), True, True, False))
    cases.append(("fresh_low_conf", dict(t_last=TIME, conf=0.5), False, True, False))
    cases.append(("matched_surfel", dict(t_last=-1), False, False, False))
    return cases


def time_rule_scenes(W, H):
    scenes = []
    cam = _cam(W, H)
    for taps in (False, True):
        sc = KeepScene(f"time_rules_{'taps' if taps else 'silent'}", W, H, cam=cam)
        sp = iter(spots(W, H))
        for name, kw, cand, keep_silent, keep_taps in time_cases():
            u, v = next(sp)
            el = sc.element(row(at(u, v, cam), **kw), keep_taps if taps else keep_silent, cand=cand)
            if taps:
                sc.fill_block(int(u) - 1, int(u) + 1, int(v) - 1, int(v) + 1, el, "cnt")
        scenes.append(sc.done())
    # the window rule: lastTime > 0 && ftime - lastTime > timeDelta (25), which also closes the gate: filled neighbourhoods are never asked
    for fills in (False, True):
        sc = KeepScene(f"window_{'filled' if fills else 'empty'}", W, H, cam=cam, timeDelta=25)
        sp = iter(spots(W, H))
        for last, c, kept in ((5, 0.5, False), (4, 0.5, True), (5, 20.0, True), (4, 20.0, True), (0, 0.5, False), (0, 20.0, True), (6, 20.0, not fills),
                              (-1, 20.0, False), (-1, 0.5, False)):
            u, v = next(sp)
            el = sc.element(row(at(u, v, cam), t_last=last, conf=c), kept)
            if fills:
                sc.fill_block(int(u) - 1, int(u) + 1, int(v) - 1, int(v) + 1, el, "cnt")
        scenes.append(sc.done())
    return scenes


# -- 5. compaction ---------------------------------------------------------------------------------------------------------------------
def pattern(name, n, seed=0):
    i = np.arange(n)
    if name == "wave37":
        return (i // 37) % 2 == 0                # changes inside every wavefront and across every row edge
    if name == "edge":
        return ((i + 3) // CLEAN_ROW) % 2 == 0   # changes three elements in front of every 256-element row edge
    if name == "all":
        return np.ones(n, bool)
    if name == "none":
        return np.zeros(n, bool)
    return np.random.RandomState(seed + n).rand(n) < 0.6


def compaction_scene(W, H, n_surf, n_cand, pat, seed=0):
    """out-of-view elements decided by the time rules alone; position = (element number, pattern, -1): the order is visible in the output"""
    n = n_surf + n_cand
    keep = pattern(pat, n, seed)
    rows = np.zeros((n, 12), F)
    rows[:, 0] = np.arange(n) % 65536
    rows[:, 1] = np.arange(n) // 65536
    rows[:, 2] = -1.0
    rows[:, 3] = 0.5
    rows[:, 4] = GREY
    rows[:, 6] = 5
    rows[:, 7] = np.where(keep, TIME - 20, TIME - 21)     # one tick decides
    rows[n_surf:, 6] = TIME
    rows[n_surf:, 7] = np.where(keep[n_surf:], -2, -1)
    rows[:, 10] = -1
    rows[:, 11] = 0.01
    sc = KeepScene(f"compact_{n_surf}_{n_cand}_{pat}", W, H, sentinels=False)
    sc.four_taps = True
    sc.surf, sc.nu, sc.mask = np.ascontiguousarray(rows[:n_surf]), np.ascontiguousarray(rows[n_surf:]), keep
    return sc


def compaction_scenes(W, H):
    scenes = []
    for n in (1, 255, 256, 257, 8192 + 300):
        for pat in ("wave37", "edge", "rand") + (("all", "none") if n <= 257 else ()):
            scenes.append(compaction_scene(W, H, n, 0, pat))
        scenes.append(compaction_scene(W, H, n, 41, "wave37"))
        scenes.append(compaction_scene(W, H, n, 300, "rand"))
    scenes.append(compaction_scene(W, H, 0, 300, "rand"))
    scenes.append(compaction_scene(W, H, 0, 1, "all"))
    scenes.append(compaction_scene(W, H, 0, 257, "wave37"))
    return scenes


def big_compaction_scene(W, H):
    return compaction_scene(W, H, BIG, 0, "rand", seed=5)


def keep_scenes(W, H):
    return tap_scenes(W, H) + comparison_scenes(W, H) + gate_scenes(W, H) + time_rule_scenes(W, H) + compaction_scenes(W, H)


# ------------------------------------------------------------------------------------------------------------------------------------
# the update pass (fuse: association taken for granted, one surfel on the ray of its pixel)
# ------------------------------------------------------------------------------------------------------------------------------------
WEIGHT = 0.8


def half_colours():
    """(old, new) channel values whose mean, weighted with EQUAL confidences as update.vert weights them, times 255 lands exactly on k + .5"""
    c = F(0.75)
    found = []
    for o in range(0, 255):
        n = o + 1
        m = F(F(F(c * F(F(o) / F(255))) + F(c * F(F(n) / F(255)))) / F(c + c))
        if F(m * F(255)) == F(o + 0.5):
            found.append((o, n))
    return found


class MergeScene:
    kind = "fuse"

    def __init__(self, W, H, tick=6):
        import efo
        self.name, self.W, self.H, self.tick = "merge", W, H, tick
        self.cam = _cam(W, H)
        par = tick % 2
        qr = H // 2
        self.idx = np.zeros((H, W), np.uint32)
        self.vc, self.ct, self.nr = (np.zeros((H, W, 4), F) for _ in range(3))
        self.dm = np.full((H, W), 1.0, F)
        self.rgb = np.random.RandomState(W + tick).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
        halves = half_colours()
        assert len(halves) >= 3
        names = ["radius_below", "radius_at", "radius_above", "conf_cancels", "conf_huge", "colour_halves", "colour_255", "colour_25_bits",
                 "normal_cancels", "shared_first", "shared_second", "plain"]
        free = [(qx, qy) for qx in range(2, W // 2 - 2, 2) for qy in range(2, qr - 2, 2)]
        self.anchor = {}
        for k, nm in enumerate(names):
            qx, qy = free[k]
            i, j = 2 * qx + par, 2 * qy + par
            self.dm[j, i] = F(1.5 + 0.25 * k)
            self.anchor[nm] = dict(i=i, j=j, z=self.dm[j, i], r=qx * qr + qy)
        a = self.anchor
        self.rgb[a["colour_halves"]["j"], a["colour_halves"]["i"]] = [halves[0][1], halves[1][1], halves[-1][1]]
        self.rgb[a["colour_255"]["j"], a["colour_255"]["i"]] = 255
        ocam = efo.make_cam(*self.cam)
        # the candidates' confidence and radius, from the oracle's own data pass on an empty index map; a flat filtered depth whose radius r has a
        # float s with 1.5f * s == r exactly
        z4 = np.zeros((H, W, 4), F)
        for flat in (1.0, 1.1, 1.2, 1.3, 0.9, 1.7, 2.3):
            self.dmf = np.full((H, W), flat, F)
            _, nu = efo.fuse(ocam, EYE, tick, self.rgb, self.dm, self.dmf, np.zeros((H, W), np.uint32), z4, z4, z4, MAXD, WEIGHT, np.zeros((1, 12), F))
            assert len(nu) == (W // 2) * qr and (nu[:, 7] == -2).all()
            rad = nu[a["radius_at"]["r"], 11]
            s = F(rad / F(1.5))
            eq = [x for x in (down(down(s)), down(s), s, up(s), up(up(s))) if F(F(1.5) * x) == rad]
            if eq:
                break
        assert eq, "no flat depth gives a candidate radius that 1.5f * s reaches"
        self.probe, self.n0, s_eq = nu, nu[a["plain"]["r"], 8:11].copy(), eq[0]
        s_lo, s_hi = F(nu[a["radius_below"]["r"], 11] / F(1.5)), F(nu[a["radius_above"]["r"], 11] / F(1.5))
        while F(F(1.5) * s_lo) >= nu[a["radius_below"]["r"], 11]:
            s_lo = down(s_lo)
        while F(F(1.5) * s_hi) <= nu[a["radius_above"]["r"], 11]:
            s_hi = up(s_hi)
        assert F(F(1.5) * up(s_lo)) >= nu[a["radius_below"]["r"], 11] and F(F(1.5) * down(s_hi)) <= nu[a["radius_above"]["r"], 11]
        assert abs(self.n0[2]) == 1.0
        self.rows = [np.zeros(12, F)]
        self.sid = {}

        def surfel(nm, conf=2.0, colour=GREY, n=None, rad_=0.05, sid=None):
            an = a[nm]
            xl, yl = (an["i"] + 0.5 - W / 2) / FX, (an["j"] + 0.5 - H / 2) / FY
            vc = np.array([xl * an["z"], yl * an["z"], an["z"], 1.0], F)
            if sid is None:
                sid = len(self.rows)
                self.rows.append(row(vc[:3], conf=conf, colour=colour, t_init=1, t_last=1, n=self.n0 if n is None else n, rad=rad_))
            self.idx[an["j"], an["i"]], self.vc[an["j"], an["i"]], self.nr[an["j"], an["i"]] = sid, vc, (*self.n0, 0.05)
            self.sid[nm] = sid
            return sid

        def cand(nm):
            return nu[a[nm]["r"]]
        surfel("radius_below", rad_=s_lo)
        surfel("radius_at", rad_=s_eq)
        surfel("radius_above", rad_=s_hi)
        surfel("conf_cancels", conf=-cand("conf_cancels")[3])
        surfel("conf_huge", conf=1e30)
        surfel("colour_halves", conf=cand("colour_halves")[3], colour=float((halves[0][0] << 16) | (halves[1][0] << 8) | halves[-1][0]))
        surfel("colour_255", conf=3.0, colour=float(0xFFFFFF))
        surfel("colour_25_bits", colour=float(0x2102030))
        surfel("normal_cancels", conf=cand("normal_cancels")[3], n=-cand("normal_cancels")[8:11])
        surfel("shared_second", sid=surfel("shared_first"))
        surfel("plain")
        assert a["shared_first"]["r"] < a["shared_second"]["r"]
        self.halves = halves
        self.surf = np.stack(self.rows).astype(F)

    def run(self, be, cam):
        return be.fuse(cam, EYE, self.tick, self.rgb, self.dm, self.dmf, self.idx, self.vc, self.ct, self.nr, MAXD, WEIGHT, self.surf)

    def check(self, out):
        s, nu = out
        a, sid, before = self.anchor, self.sid, self.surf
        assert bits_same(nu[:, :7], self.probe[:, :7]) and bits_same(nu[:, 8:], self.probe[:, 8:])
        matched = {an["r"] for an in a.values()}
        assert set(np.nonzero(nu[:, 7] == -1)[0].tolist()) == matched and ((nu[:, 7] == -1) | (nu[:, 7] == -2)).all()
        changed = set(np.nonzero((s.view(np.uint32) != before.view(np.uint32)).any(axis=1))[0].tolist())
        assert changed == set(sid.values()) and 0 not in changed
        full = lambda nm: not bits_same(s[sid[nm], 8:12], before[sid[nm], 8:12])      # the normal / radius row was rewritten
        for nm in sid:
            assert s[sid[nm], 7] == self.tick, nm
        assert not full("radius_below") and not full("radius_at") and full("radius_above")
        for nm in ("radius_below", "radius_at"):    # confidence and time only
            assert bits_same(s[sid[nm], :3], before[sid[nm], :3]) and s[sid[nm], 4] == before[sid[nm], 4]
            assert s[sid[nm], 3] == F(before[sid[nm], 3] + nu[a[nm]["r"], 3])
        assert s[sid["conf_cancels"], 3] == 0 and np.isnan(s[sid["conf_cancels"], :3]).all()
        assert s[sid["conf_cancels"], 4] == -2.0 ** 31            # int() of a mean that is not finite: INT_MIN per channel, the shifts wrap
        assert s[sid["conf_huge"], 3] == F(1e30) and s[sid["conf_huge"], 4] == before[sid["conf_huge"], 4]       # the candidate weighs nothing
        col = int(s[sid["colour_halves"], 4])
        h = self.halves
        assert ((col >> 16) & 255, (col >> 8) & 255, col & 255) == (h[0][1], h[1][1], h[-1][1]), hex(col)      # k + .5 rounds away from zero
        assert s[sid["colour_255"], 4] == float(0xFFFFFF)
        assert s[sid["colour_25_bits"], 4] < float(1 << 24) and full("colour_25_bits")
        assert not np.isfinite(s[sid["normal_cancels"], 8:11]).any() or (s[sid["normal_cancels"], 8:11] == 0).all()
        first = nu[a["shared_first"]["r"]]
        assert s[sid["shared_first"], 3] == F(F(2.0) + first[3])          # the lower slot merged, the other left no trace

    def __repr__(self):
        return f"merge@{self.W}x{self.H}"


# ------------------------------------------------------------------------------------------------------------------------------------
# the deformation graph (clean_deform)
# ------------------------------------------------------------------------------------------------------------------------------------
DTIME = 200
NODE_COUNTS = (1, 3, 4, 5, 10, 11, 19, 20, 21, 48)
STEP = F(2.0 ** -10)


class DeformScene:
    kind = "clean_deform"

    def __init__(self, name, W, H, graph, rows, check, cands=(), depth=None, isFern=0, time=DTIME, cam=None):
        self.name, self.W, self.H, self.time, self.isFern, self._check = name, W, H, time, isFern, check
        self.cam = _cam(W, H) if cam is None else cam
        self.graph = np.ascontiguousarray(np.asarray(graph, F).reshape(-1, 16))
        self.surf = np.ascontiguousarray(np.asarray(rows, F).reshape(-1, 12))
        self.nu = np.ascontiguousarray(np.asarray(cands, F).reshape(-1, 12))
        self.depth = np.full((H, W), 30.0, F) if depth is None else depth
        self.idx = np.zeros((H, W), np.uint32)
        self.z4 = np.zeros((H, W, 4), F)

    def run(self, be, cam):
        return be.clean_deform(cam, EYE, self.time, self.idx, self.z4, self.z4, self.z4, float(CONF), TD_OPEN, MAXD, self.surf, self.nu, self.graph,
                               self.depth, self.isFern)

    def check(self, out):
        assert len(out) == len(self.surf) + len(self.nu), self.name       # empty index images, everything seen lately: all kept
        self._check(out)

    def __repr__(self):
        return f"{self.name}@{self.W}x{self.H}"


def node(p, t, trans=(0, 0, 0), R=None):
    g = np.zeros(16, F)
    g[0:3] = p
    g[3:12] = np.eye(3).reshape(9) if R is None else np.asarray(R).T.reshape(9)     # column-major
    g[12:15] = trans
    g[15] = t
    return g


def window_of(n, found):
    """the nodes deform_vertex collects: up to 10 from `found` backwards, then forwards until 20 are held"""
    back = [j for j in range(found, -1, -1)][:10]
    fwd = [j for j in range(found + 1, n)][:20 - len(back)]
    return back + fwd


def window_scenes(W, H):
    """one vertex at the origin of the node line per scene; node j translates by j * STEP in y with the identity rotation, so the weighted mean of
    the chosen nodes' numbers can be read from the result.  The nodes get NEARER the further they are (in time order) from the found one, so
    the nearest four inside the collected window are its ends and every node just outside it is nearer still."""
    scenes = []
    for n in NODE_COUNTS:
        times = [10 + 2 * j for j in range(n)]
        m = n // 2
        for tname, t, found in (("older", 8, 0), ("newer", 10 + 2 * n + 5, n - 1), ("equal", times[m], m), ("between", times[m] + 1 if m + 1 < n else times[m] - 1, None),
                                ("older_clamped", 3, -1), ("times_equal", 50, None)):
            eq = tname == "times_equal"
            ntimes = [50] * n if eq else times
            if tname == "between":
                found = m + 1 if m + 1 < n else m          # (ties of |time difference| go to imin)
            if eq:                                          # the bisection stops at the first middle it tries, and imin = 0 is as near in time
                found = 0
            centre = max(found, 0)
            g = []
            for j in range(n):
                d = F(3.0 - 0.03125 * abs(j - centre)) if j % 2 else -F(3.0 - 0.03125 * abs(j - centre))
                g.append(node((d, 0, 2), ntimes[j], trans=(0, j * STEP, 0)))
            if tname == "older_clamped":
                g[0][0] = F(3.5)     # the fetch in front of texel 0 clamps onto node 0's x, which truncates to the vertex's init time 3
            v = row((0, 0, 2), t_init=t, t_last=DTIME - 1)
            same = row((0, 0, 2), t_init=DTIME, t_last=DTIME - 1)      # initialised this frame: not deformed
            new = row((0, 0, 2), t_init=DTIME, t_last=-2)
            win = window_of(n, centre) if found != -1 else list(range(min(n, 20)))

            def check(out, n=n, win=win, v=v, same=same, tname=tname):
                assert bits_same(out[1], same) and out[2][7] == DTIME and bits_same(out[2][:7], same[:7])
                got = out[0]
                assert got[6] == v[6] and got[3] == v[3] and got[11] == v[11]
                if n < 4:
                    assert np.isnan(got[8:11]).any(), (tname, n, got)       # node -1 is a singular rotation
                    return
                assert got[0] == 0 and abs(got[2] - 2) < 1e-5 and np.isfinite(got).all()
                mean = float(got[1]) / float(STEP)
                assert min(win) - 1e-3 <= mean <= max(win) + 1e-3, (tname, n, mean, win)
                if n >= 5:
                    assert got[7] == DTIME                                   # seen again: in front of the synthesized depth
            scenes.append(DeformScene(f"window_{n}_{tname}", W, H, g, [v, same], check, cands=[new]))
    return scenes


def rotation(rng):
    w = rng.uniform(-0.05, 0.05, 3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def lattice_scene(W, H, n, seed=11):
    """nodes and vertices on one quarter-unit lattice: exact ties of distance everywhere (two nodes equally far, a vertex ON a node, the fifth
    nearest as far as the fourth), small rotations and translations, node times in runs of equal values"""
    rng = np.random.RandomState(seed + n)
    side = int(np.ceil(np.sqrt(n)))
    pts = [(0.25 * (k % side), 0.25 * (k // side), 1.25) for k in range(n)]
    order = rng.permutation(n)
    g = [node(pts[order[j]], 10 + (j // 3) * 2, trans=rng.uniform(-0.03, 0.03, 3), R=rotation(rng)) for j in range(n)]
    rows = []
    for a in range(-1, 2 * side + 1):
        for b in range(-1, 2 * side + 1):
            rows.append(row((0.125 * a, 0.125 * b, 1.5 if (a + b) % 3 == 1 else 1.25), conf=20.0 if (a * 7 + b) % 4 else 5.0, t_init=int(rng.randint(1, 10 + n)),
                            t_last=DTIME - 3, n=(0, 0.6, -0.8)))
    rows.append(row((0.25, 0.25, 1.25), t_init=DTIME, t_last=DTIME - 3))
    rows = np.stack(rows)
    on_node = [k for k, r in enumerate(rows[:-1]) if any(tuple(r[:3]) == tuple(F(p) for p in q) for q in pts)]
    assert len(on_node) >= 1

    def check(out):
        assert bits_same(out[-1], rows[-1])
        moved = (out[:-1, :3].view(np.uint32) != rows[:-1, :3].view(np.uint32)).any(axis=1)
        assert moved.all() and bits_same(out[:, 3:7], rows[:, 3:7]) and bits_same(out[:, 11], rows[:, 11])
        if n >= 5:
            fin = np.isfinite(out).all(axis=1)
            print(f"lattice_{n}: {int((~fin).sum())} of {len(out)} rows not finite")
            assert fin.mean() > 0.9 and np.abs(out[:-1, :3] - rows[:-1, :3])[fin[:-1]].max() < 0.2
            seen = out[:-1, 7] == DTIME
            assert seen.any() and (~seen).any() and not seen[rows[:-1, 3] < CONF].any()
    return DeformScene(f"lattice_{n}", W, H, g, rows, check)


def seen_again_scenes(W, H):
    """node 0 on the vertex, nodes 1-4 all at the same distance: the weights are (1, 0, 0, 0) and the deformed position is node 0's translation,
    exactly.  The 'seen again' test is then probed at every comparison."""
    scenes = []
    cam = _cam(W, H)

    def one(name, lp, seen, conf=20.0, depth=None, isFern=0):
        d = 0.5
        g = [node((0, 0, 0), 10, trans=lp)] + [node(p, 12 + 2 * k) for k, p in enumerate(((d, 0, 0), (-d, 0, 0), (0, d, 0), (0, -d, 0)))]
        v = row((0, 0, 0), conf=conf, t_init=11, t_last=DTIME - 1)

        def check(out, lp=lp, seen=seen):
            assert bits_same(out[0, :3], np.asarray(lp, F)), (name, out[0, :3], lp)
            assert out[0, 7] == (DTIME if seen else DTIME - 1), name
        scenes.append(DeformScene(f"seen_{name}", W, H, g, [v], check, depth=depth, isFern=isFern, cam=cam))

    mid = at(9.5, 11.5, cam)
    for tag, c, seen in (("below", down(CONF), False), ("at", CONF, False), ("above", up(CONF), True)):
        one(f"conf_{tag}", mid, seen, conf=c)
    one("fern", mid, False, isFern=1)
    one("fern_off", mid, True, isFern=0)
    x_lo, x_hi, y_lo, y_hi = solve(0, Z, FX, cam[4]), solve(W, Z, FX, cam[4]), solve(0, Z, FY, cam[5]), solve(H, Z, FY, cam[5])
    one("x_at_zero", (x_lo, mid[1], Z), False)
    one("x_past_zero", (step_until_changed(x_lo, Z, FX, cam[4], +1), mid[1], Z), True)
    one("x_at_cols", (x_hi, mid[1], Z), False)
    one("x_before_cols", (step_until_changed(x_hi, Z, FX, cam[4], -1), mid[1], Z), True)
    one("y_at_zero", (mid[0], y_lo, Z), False)
    one("y_past_zero", (mid[0], step_until_changed(y_lo, Z, FY, cam[5], +1), Z), True)
    one("y_at_rows", (mid[0], y_hi, Z), False)
    one("y_before_rows", (mid[0], step_until_changed(y_hi, Z, FY, cam[5], -1), Z), True)
    one("z_at_max_depth", (F(0), F(0), F(MAXD)), False)
    one("z_before_max_depth", (F(0), F(0), down(MAXD)), True)
    one("z_zero", (F(0), F(0), F(0)), False)
    hole = np.full((H, W), 30.0, F)
    hole[11, 9] = 0
    one("depth_zero", mid, False, depth=hole)
    near = np.full((H, W), 30.0, F)
    near[11, 9] = 1.25
    lim = F(F(1.25) + F(0.1))
    one("depth_margin_at", at(9.5, 11.5, cam, lim), False, depth=near)
    one("depth_margin_before", at(9.5, 11.5, cam, down(lim)), True, depth=near)
    return scenes


def deform_scenes(W, H):
    return window_scenes(W, H) + [lattice_scene(W, H, n) for n in NODE_COUNTS] + seen_again_scenes(W, H)


# ------------------------------------------------------------------------------------------------------------------------------------
# frame tier: a restored map, one frame with an injected identity pose and a flat depth image 1.5 m away
# ------------------------------------------------------------------------------------------------------------------------------------
DEPTH_MM = 1500
ZD = F(1.5)


class FrameScene:
    """The map IS the scene: the index map the keep-test taps is splatted from it, so an element's neighbours are surfels of their own, each
    alone in its texel, just behind the element.  run() is the frame's map path spelled out with the operators (predictIndices, fuse,
    predictIndices, clean), so that the oracle and the compiled shaders can be compared on it without a GPU; the GPU test restores the same
    map into the engine and into the oracle's Fusion and runs the frame.  Surfel 0 (the index map's background) lies beyond maxDepth."""
    kind = "frame"

    def __init__(self, name, W, H, tick=TIME, conf=CONF, timeDelta=TD_OPEN):
        self.name, self.W, self.H, self.tick, self.conf, self.timeDelta = name, W, H, tick, F(conf), timeDelta
        self.cam = _cam(W, H)
        self.rows, self.keep = [row((0, 0, 1000.0), t_last=tick)], [True]
        self.removed_new = 0              # candidates of this frame that the scene has removed (matched ones, and new points the taps remove)
        self.depth = np.full((H, W), DEPTH_MM, np.uint16)
        self.rgb = np.random.RandomState(W).randint(1, 256, size=(H, W, 3)).astype(np.uint8)
        self.taken = set()
        self.extra = None
        self.new_points = np.zeros((0, 12), F)      # this frame's candidates that a scene puts on a count
        self.tested = []                            # rows under test (a neighbour has nothing behind it: a fifth tap cannot change its verdict)

    def surfel(self, r, kept):
        self.rows.append(np.asarray(r, F))
        self.keep.append(None if kept is None else bool(kept))
        return len(self.rows) - 1

    def neighbour(self, t, z, t_init=4, normal=(0, 0, -1), t_last=None):
        """a surfel alone in texel t, at its centre, that counts for `cnt` against an element in front of it (t_last = this tick, t_init not
        below the element's and more than a centimetre behind it: for `zCount`)"""
        assert t not in self.taken and 0 <= t[0] < self.W and 0 <= t[1] < self.H, t
        self.taken.add(t)
        p = (F((t[0] + 0.5 - self.cam[4]) / FX * float(z)), F((t[1] + 0.5 - self.cam[5]) / FY * float(z)), F(z))     # (the texel's centre, to a rounding)
        return self.surfel(row(p, conf=11.0, t_init=t_init, t_last=self.tick - 1 if t_last is None else t_last, n=normal, rad=0.01), True)

    def element(self, u, v, fill, kept, rule="cnt", **kw):
        """an element at window position (u, v), depth Z, with neighbours on the texels of `fill` ('all': every texel its taps reach)"""
        i, j = int(np.floor(u)), int(np.floor(v))
        assert (i, j) not in self.taken
        self.taken.add((i, j))
        kw.setdefault("rad", 0.05)
        sid = self.surfel(row(at(u, v, self.cam), **kw), kept)
        self.tested.append(sid)
        wts = tap_weights(u, v, self.W, self.H)
        own = wts.pop((i, j))
        assert own == 4
        for t in (sorted(wts) if fill == "all" else fill):
            if rule == "cnt":
                self.neighbour(t, F(Z + F(0.005)))
            else:
                self.neighbour(t, F(Z + F(0.02)), t_init=5, t_last=self.tick)
        return sid

    def done(self):
        self.surf = np.stack(self.rows).astype(F)
        self.four_taps = four_trips(self.surf[self.tested], self.cam) and four_trips(self.new_points, self.cam)
        return self

    def run(self, be, cam):
        dm = be.metricise_depth(self.depth, 3.0)
        dmf = be.metricise_depth(be.filter_depth(self.depth, 3.0), 3.0)
        i1 = be.predict_indices(cam, EYE, self.tick, self.surf, MAXD, self.timeDelta)
        s2, nu = be.fuse(cam, EYE, self.tick, self.rgb, dm, dmf, *i1, MAXD, 1.0, self.surf)
        i2 = be.predict_indices(cam, EYE, self.tick, s2, MAXD, self.timeDelta)
        return be.clean(cam, EYE, self.tick, *i2, float(self.conf), self.timeDelta, MAXD, s2, nu)

    def check(self, out):
        """out: the map after the frame"""
        keep = np.array([k is not False for k in self.keep])
        exact = np.array([k is True for k in self.keep])[keep]
        n_old = int(keep.sum())
        e = self.surf[keep]
        assert len(out) >= n_old and (out[:n_old, 6] != self.tick).all(), (self.name, len(out), n_old)
        assert bits_same(out[:n_old][exact], e[exact]), (self.name, np.nonzero((out[:n_old].view(np.uint32) != e.view(np.uint32)).any(axis=1) & exact)[0][:8])
        new = out[n_old:]
        assert (new[:, 6] == self.tick).all() and (new[:, 7] == self.tick).all()
        assert len(new) == (self.W // 2) * (self.H // 2) - self.removed_new, (self.name, len(new), self.removed_new)
        if self.extra:
            self.extra(out[:n_old], e)

    def __repr__(self):
        return f"{self.name}@{self.W}x{self.H}"


def frame_spots(W, H):
    """element pixels three texels apart, at which the shader's tap loop runs 4 times for every fractional part used"""
    ok = lambda i, n: all(shader_trips(i + f, n) == 4 for f in (0.5, 0.75))
    return [(3 + 4 * a, 3 + 4 * b) for b in range((H - 6) // 4 + 1) for a in range((W - 6) // 4 + 1) if ok(3 + 4 * a, W) and ok(3 + 4 * b, H)]


def frame_tap_scene(W, H):
    """pairs at the cnt 8 | 9 boundary for the four placements whose weight-4 texel is the element's own, and one pair at zCount 4 | 5"""
    sc = FrameScene("frame_taps", W, H)
    sp = iter(frame_spots(W, H))
    for fa in (0.5, 0.75):
        for fb in (0.5, 0.75):
            for total, kept in ((8, True), (9, False)):
                i, j = next(sp)
                wts = tap_weights(i + fa, j + fb, W, H)
                del wts[(i, j)]
                sc.element(i + fa, j + fb, subset_with_sum(wts, total), kept)
    for total, kept in ((4, True), (5, False)):       # zCount: surfels seen this frame, two centimetres behind a steep element
        i, j = next(sp)
        wts = tap_weights(i + 0.5, j + 0.5, W, H)
        del wts[(i, j)]
        sc.element(i + 0.5, j + 0.5, subset_with_sum(wts, total), kept, rule="z")
    i, j = next(sp)
    sc.element(i + 0.5, j + 0.5, "all", False)
    i, j = next(sp)
    sc.element(i + 0.5, j + 0.5, [], True)
    return sc.done()


def frame_time_scenes(W, H):
    scenes = []
    for taps in (False, True):
        sc = FrameScene(f"frame_time_rules_{'taps' if taps else 'silent'}", W, H)
        sp = iter(frame_spots(W, H))
        for name, kw, cand, keep_silent, keep_taps in time_cases():
            if cand or kw.get("t_last") == -1:
                continue                     # (this frame's candidates come from the depth image: frame_candidate_scene)
            i, j = next(sp)
            sc.element(i + 0.5, j + 0.5, "all" if taps else [], keep_taps if taps else keep_silent, **kw)
        scenes.append(sc.done())
    for fills in (False, True):
        sc = FrameScene(f"frame_window_{'filled' if fills else 'empty'}", W, H, timeDelta=25)
        sp = iter(frame_spots(W, H))
        for last, c, kept in ((5, 0.5, False), (4, 0.5, True), (5, 20.0, True), (4, 20.0, True), (0, 0.5, False), (0, 20.0, True), (6, 20.0, not fills)):
            i, j = next(sp)
            sc.element(i + 0.5, j + 0.5, "all" if fills else [], kept, t_last=last, conf=c)
        scenes.append(sc.done())
    return scenes


def frame_candidate_scene(W, H):
    """this frame's own points (even pixels, depth 1.5): a new point with 8 | 9 taps behind it (surfels whose normals keep them from being
    associated), and the update pass at the radius gate: one surfel on the pixel's ray, radius one float below, at and above r / 1.5"""
    import efo
    sc = FrameScene("frame_candidates", W, H)
    ocam = efo.make_cam(*sc.cam)
    dm = efo.metricise_depth(sc.depth, 3.0)
    dmf = efo.metricise_depth(efo.filter_depth(sc.depth, 3.0), 3.0)
    z4 = np.zeros((H, W, 4), F)
    _, nu = efo.fuse(ocam, EYE, sc.tick, sc.rgb, dm, dmf, np.zeros((H, W), np.uint32), z4, z4, z4, MAXD, 1.0, np.zeros((1, 12), F))
    qr = H // 2
    assert len(nu) == (W // 2) * qr and (nu[:, 7] == -2).all() and (nu[:, 2] == ZD).all()
    pix = [(6 + 4 * a, 6 + 4 * b) for b in range((H - 12) // 4 + 1) for a in range((W - 12) // 4 + 1)]
    sp = iter(pix)
    for total, kept in ((8, True), (9, False), (16, False), (0, True)):
        while True:      # (a candidate's window position is i + .5 to a rounding: a pixel where it keeps the (1, 2, 1) x (1, 2, 1) weights)
            i, j = next(sp)
            c = nu[(i // 2) * qr + j // 2]
            wts = tap_weights(proj(c[0], ZD, FX, sc.cam[4]), proj(c[1], ZD, FY, sc.cam[5]), W, H)
            if wts.get((i, j)) == 4 and len(wts) == 9 and four_trips(c, sc.cam):
                break
        sc.new_points = np.concatenate([sc.new_points, c[None]])
        for t in subset_with_sum(wts, total):
            sc.neighbour(t, F(ZD + F(0.005)), normal=tuple(-c[8:11]))
        sc.removed_new += not kept
    merged = {}
    for tag in ("below", "at", "above"):
        i, j = next(sp)
        c = nu[(i // 2) * qr + j // 2]
        rad = c[11]
        s = F(rad / F(1.5))
        if tag == "at":
            eq = [x for x in (down(down(s)), down(s), s, up(s), up(up(s))) if F(F(1.5) * x) == rad]
            assert eq, "1.5f * s does not reach this frame's candidate radius"
            s = eq[0]
        elif tag == "below":
            while F(F(1.5) * s) >= rad:
                s = down(s)
        else:
            while F(F(1.5) * s) <= rad:
                s = up(s)
        sc.taken.add((i, j))
        merged[tag] = (sc.surfel(row(c[:3], conf=20.0, t_init=4, t_last=sc.tick - 1, n=tuple(c[8:11]), rad=s), None), c)
        sc.removed_new += 1

    def extra(got, before, merged=merged, sc=sc):
        pos = {sid: k for k, sid in enumerate(np.nonzero([k is not False for k in sc.keep])[0])}
        for tag, (sid, c) in merged.items():
            g, b = got[pos[sid]], before[pos[sid]]
            assert g[7] == sc.tick and g[3] == F(F(20.0) + c[3]), tag
            assert bits_same(g[8:12], b[8:12]) == (tag != "above"), tag        # the full merge rewrites the normal / radius row
    sc.extra = extra
    return sc.done()


def frame_keep_scenes(W, H):
    return [frame_tap_scene(W, H)] + frame_time_scenes(W, H) + [frame_candidate_scene(W, H)]


def frame_bulk_scene(W, H, n, seed=3):
    """n out-of-view surfels decided by the time rules alone behind surfel 0: whole groups of compaction rows and a partial one"""
    c = compaction_scene(W, H, n - 1, 0, "rand", seed)
    sc = FrameScene(f"frame_bulk_{n}", W, H)
    sc.surf = np.concatenate([np.stack(sc.rows).astype(F), c.surf])
    sc.keep = [True] + c.mask.tolist()
    return sc


def frame_deform_scene(W, H, n):
    """lattice_scene(n)'s surfels and graph as a restored map at tick DTIME"""
    lat = lattice_scene(W, H, n)
    sc = FrameScene(f"frame_deform_{n}", W, H, tick=DTIME)
    sc.surf = np.concatenate([np.stack(sc.rows).astype(F), lat.surf])
    sc.graph = lat.graph
    return sc
