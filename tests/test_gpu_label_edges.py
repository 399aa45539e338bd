"""Surfel IDs and label alignment, fusion and gather at their edges (kernels in elasticfusion_amd/csrc/ef_labels.inc, host code in
ef_host_labels.inc), bit for bit against tests/labelref.py, the numpy statement of include/ef_hip.h.

Every map is built by hand and uploaded into a 52 x 36 context (the table's slack is then 1872 rows); no frame is tracked except where a
test says so.  Every comparison is array_equal on uint32 views and no row is left out of any of them.  A scene's claims (which row is
observed, which is hidden, which projection is an integer) are asserted on the reference before the device is asked.

  numbering   k_ids_assign's 64-way search for the zero suffix at every prefix length around a wave and a step boundary, both arms of
              max(counter, last + 1), k_ids_gather, k_ids_zero, k_ids_check's refusals at pair and grid-stride boundaries, and of an
              upload whose zero suffix could not be numbered without wrapping past 0xFFFFFFFF
  alignment   k_labels_align's two searches and flat copy for C = 1 .. 256, partial tiles, every erase / insert pattern, the ping-pong, and
              labels_reserve's growth from inserts and from frames
  fusion      k_labels_fuse with rows sitting exactly on each gate of the observation test and sums exactly on each gate of the update
  gather      k_labels_gather's first strict maximum on ties, NaNs and negative rows, with either output NULL

The three *_large tests print their wall time, the numpy reference included; each docstring has the time measured on an MI355X.
"""
import ctypes as C
import time

import numpy as np
import pytest

import labelref as L

pytestmark = pytest.mark.gpu

W, H, P = L.W, L.H, L.W * L.H
OTHER = [i for i in range(12) if i != 5]


@pytest.fixture(scope="module")
def api():
    from elasticfusion_amd import api
    return api


def context(api, cap, **kw):
    cam = dict(width=W, height=H, fx=64.0, fy=64.0, cx=26.0, cy=18.0)
    cam.update(kw)
    return api.ElasticFusion(maxSurfels=max(int(cap), P), **cam)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def refused(api, call):
    with pytest.raises(api.EFError, match="error -4"):
        call()


# ------------------------------------------------------------------------------------------------
# a. numbering
# ------------------------------------------------------------------------------------------------
def prefix_lengths(n):
    return sorted({s for s in (0, 1, 63, 64, 65, n - 65, n - 64, n - 63, n - 1, n) if 0 <= s <= n})


def numbering(api, n):
    ef = context(api, n)
    base = L.filler_map(n)
    try:
        ef.setSurfelIds(True)
        counter = 1
        for s in prefix_lengths(n):
            # both arms of max(counter, last + 1): the prefix's largest ID above the counter, then (the counter now past 3 n) below it
            for arm in ("above", "below") if s else ("no prefix",):
                lane = np.zeros(n, np.int64)
                lane[:s] = L.spaced_ids(s, counter + 7 + 3 * n if arm == "above" else 1)
                assert not s or (lane[s - 1] >= counter) == (arm == "above"), (n, s, arm, counter)
                assert L.lane_ok(lane, counter)
                ef.uploadMap(L.with_lane(base, lane))
                exp, counter = L.assign(lane, counter)
                got = ef.surfelIds()
                assert np.array_equal(got, exp), (n, s, arm, np.flatnonzero(got != exp)[:5])
                assert np.array_equal(ef.surfelIds(), exp), (n, s, arm, "a second call changed the lane")
                if n and s in (0, 1, n):
                    m = ef.downloadMap()
                    assert np.array_equal(L.lane_of(m), exp) and np.array_equal(bits(m[:, OTHER]), bits(base[:, OTHER])), (n, s, arm)
        ef.setSurfelIds(False)
        if n:
            m = ef.downloadMap()
            assert m.shape == base.shape and not L.lane_of(m).any(), n
        ef.setSurfelIds(True)   # numbered from the counter, not from 1
        exp, counter = L.assign(np.zeros(n, np.int64), counter)
        assert np.array_equal(ef.surfelIds(), exp), n
    finally:
        ef.close()


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097])
def test_numbering(api, n):
    numbering(api, n)


def test_numbering_large(api):
    """262144 + 257 rows: the 64-way search takes three steps, 4101, 65 and 2 rows wide.  Measured: 0.20 s for all 19 uploads."""
    t = time.perf_counter()
    numbering(api, 262144 + 257)
    print(f"numbering, n = {262144 + 257}: {time.perf_counter() - t:.2f} s")


def bad_lanes(n):
    """(name, lane): shapes the upload must refuse"""
    good = L.spaced_ids(n, 5)
    out = []
    for a, b in sorted({(0, 1), (63, 64), (n - 2, n - 1)}):
        if 0 <= a and b < n:
            lane = good.copy()
            lane[a] = 0
            if a:
                lane[:a] = L.spaced_ids(a, 1)
            out.append((f"zero at {a}, non-zero at {b}", lane))
    for a in sorted({0, 63, n - 2}):
        if 0 <= a < n - 1:
            lane = good.copy()
            lane[a + 1] = lane[a]
            out.append((f"equal at {a}, {a + 1}", lane))
    return out


@pytest.mark.parametrize("n", [2, 65, 257, 4097])
def test_bad_lanes_are_refused(api, n):
    ef = context(api, n)
    base = L.filler_map(n)
    try:
        ef.setSurfelIds(True)
        for name, lane in bad_lanes(n):
            assert not L.lane_ok(lane), name
            ef.uploadMap(L.with_lane(base, lane))
            refused(api, ef.surfelIds)
            refused(api, ef.downloadMap)
            good = L.spaced_ids(n, 3)
            ef.uploadMap(L.with_lane(base, good))   # a valid upload clears it
            assert np.array_equal(ef.surfelIds(), good.astype(np.uint32)), name
    finally:
        ef.close()


def test_bad_lane_at_the_check_stride_large(api):
    """k_ids_check runs 4096 x 256 threads: with more rows its loop strides.  One descending pair across the stride's end (rows 4096*256 - 1 and
    4096*256: the last thread's first pair), one just past it (thread 0's second pair), one at the very end.  Measured: 0.11 s."""
    t = time.perf_counter()
    stride = 4096 * 256
    n = stride + 300
    ef = context(api, n)
    base = L.filler_map(n)
    good = L.spaced_ids(n, 9)
    try:
        ef.setSurfelIds(True)
        for a in (stride - 1, stride, n - 2):
            lane = good.copy()
            lane[a], lane[a + 1] = good[a + 1], good[a]
            assert not L.lane_ok(lane)
            ef.uploadMap(L.with_lane(base, lane))
            refused(api, ef.surfelIds)
        ef.uploadMap(L.with_lane(base, good))
        assert np.array_equal(ef.surfelIds(), good.astype(np.uint32))
    finally:
        ef.close()
    print(f"refusals at the check's stride, n = {n}: {time.perf_counter() - t:.2f} s")


def test_ids_near_the_end_of_uint32(api):
    """An upload whose zero suffix cannot be numbered without leaving uint32 is refused, in a lane of one row too: the numbering would hand
    out 0, or IDs below the prefix.  Where it just fits the upload is kept and the numbering runs to 0xFFFFFFFE.  Both arms again: the room
    is counted from the lane's largest ID and from the context's counter."""
    TOP = 0xFFFFFFFF
    ef = context(api, P)
    try:
        ef.setSurfelIds(True)
        ef.uploadMap(L.filler_map(2))
        counter = int(ef.surfelIds()[-1]) + 1
        # (rows, prefix length, largest ID): one more than fits
        for n, s, top in ((1, 1, TOP), (3, 1, TOP - 1), (2, 1, TOP - 1), (P, 1, TOP - P + 1), (P, P, TOP), (300, 299, TOP - 1), (65, 64, TOP - 1)):
            lane = np.zeros(n, np.int64)
            lane[:s] = L.spaced_ids(s, top - 3 * s)
            lane[s - 1] = top
            assert L.lane_ok(lane) and not L.lane_ok(lane, counter), (n, s, top)
            ef.uploadMap(L.with_lane(L.filler_map(n), lane))
            refused(api, ef.surfelIds)
            refused(api, ef.downloadMap)
            ef.uploadMap(L.filler_map(2))   # a valid upload clears it
            exp, counter = L.assign(np.zeros(2, np.int64), counter)
            assert np.array_equal(ef.surfelIds(), exp)
    finally:
        ef.close()
    # exactly what fits (largest + 1 + suffix = 0xFFFFFFFF): kept, and the numbering continues above the prefix
    for n, s in ((1, 1), (P, P), (300, 299), (65, 1), (P, 1)):
        ef = context(api, P)
        try:
            ef.setSurfelIds(True)
            top = TOP - 1 - (n - s)
            lane = np.zeros(n, np.int64)
            lane[:s] = L.spaced_ids(s, top - 3 * s)
            lane[s - 1] = top
            assert L.lane_ok(lane, 1)
            ef.uploadMap(L.with_lane(L.filler_map(n), lane))
            exp, counter = L.assign(lane, 1)
            got = ef.surfelIds()
            assert np.array_equal(got, exp), (n, s, np.flatnonzero(got != exp)[:5])
            assert (np.diff(got.astype(np.int64)) > 0).all() and got.min() > 0 and int(got[-1]) == TOP - 1 and counter == TOP
            # the counter's arm: it stands at 0xFFFFFFFF now, so no suffix fits any more, whatever the lane holds
            for lane in (np.zeros(1, np.int64), np.array([5, 0], np.int64), np.zeros(P, np.int64)):
                assert L.lane_ok(lane) and not L.lane_ok(lane, counter)
                ef.uploadMap(L.with_lane(L.filler_map(len(lane)), lane))
                refused(api, ef.surfelIds)
            lane = np.array([5, 9], np.int64)   # no suffix: nothing to number, so it fits
            assert L.lane_ok(lane, counter)
            ef.uploadMap(L.with_lane(L.filler_map(2), lane))
            assert np.array_equal(ef.surfelIds(), lane.astype(np.uint32))
        finally:
            ef.close()


# ------------------------------------------------------------------------------------------------
# b. alignment
# ------------------------------------------------------------------------------------------------
class Mirror:
    """what the context must hold, by the header's rules: the ID lane, the counter, and the table of the last label call"""

    def __init__(self, ef, api, Cn):
        self.ef, self.api, self.C = ef, api, Cn
        self.counter, self.calls = 1, 0
        self.lane = np.zeros(0, np.uint32)
        self.ids_prev, self.tab_prev = np.zeros(0, np.uint32), np.zeros((0, Cn), np.float32)

    def number(self):
        self.lane, self.counter = L.assign(self.lane, self.counter)

    def upload(self, m):
        self.ef.uploadMap(m)
        self.lane = L.lane_of(m).copy()
        self.ids_prev, self.tab_prev = np.zeros(0, np.uint32), np.zeros((0, self.C), np.float32)

    def erase_rows_by_id(self, rows):
        """every run of neighbouring rows goes with one EF_SEL_ID range"""
        self.number()
        rows = np.asarray(rows, np.int64)
        keep = np.ones(len(self.lane), bool)
        keep[rows] = False
        if len(rows):
            cut = np.flatnonzero(np.diff(rows) != 1) + 1
            for run in np.split(rows, cut):
                got = self.ef.eraseSurfels(tests=self.api.SEL_ID, id_min=int(self.lane[run[0]]), id_max=int(self.lane[run[-1]]))
                assert got == len(run)
        else:
            assert self.ef.eraseSurfels(tests=self.api.SEL_ID, id_min=1, id_max=0) == 0
        self.lane = self.lane[keep]

    def erase_rows(self, rows):
        self.number()
        keep = np.ones(len(self.lane), bool)
        keep[rows] = False
        assert self.ef.eraseRows(rows) == len(rows)
        self.lane = self.lane[keep]

    def keep_only_id(self, row):
        self.number()
        i = int(self.lane[row])
        assert self.ef.eraseSurfels(tests=self.api.SEL_ID | self.api.SEL_INVERT, id_min=i, id_max=i) == len(self.lane) - 1
        self.lane = self.lane[row:row + 1]

    def insert(self, k, seed=0):
        self.number()
        rec = L.filler_map(k)
        rec[:, 2] += 5.0 + seed
        rec[:, 5] = 123.0   # the record's own lane is not kept
        r = self.ef.insertSurfels(rec, gate=0)
        assert r["inserted"] == k and r["count_after"] == len(self.lane) + k
        self.lane = np.concatenate([self.lane, np.zeros(k, np.uint32)])

    def label_call(self):
        self.number()
        self.tab_prev = L.align(self.ids_prev, self.tab_prev, self.lane, self.C)
        self.ids_prev = self.lane.copy()
        self.calls += 1

    def set_labels(self):
        """the table derived from the current IDs"""
        self.label_call()
        self.tab_prev = L.table_rows(self.lane, self.C)
        self.ef.setLabels(self.tab_prev)

    def check(self, what):
        self.label_call()
        ids, tab = self.ef.labels()
        assert np.array_equal(ids, self.ids_prev), (what, len(ids), len(self.ids_prev))
        assert tab.shape == self.tab_prev.shape, (what, tab.shape)
        bad = np.flatnonzero((bits(tab) != bits(self.tab_prev)).any(1)) if len(tab) else []
        assert len(bad) == 0, (what, len(bad), bad[:5])
        return ids, tab


def every_other_row(m, n):
    # one EF_SEL_ID erase per row up to 513 rows; the 1300 rows of n = 2600 are named by row instead: the alignment sees the same IDs go
    rows = np.arange(0, n, 2)
    m.erase_rows_by_id(rows) if n <= 513 else m.erase_rows(rows)


def everything_then_an_insert(m, n):
    m.erase_rows_by_id(np.arange(n))
    ids, _ = m.check("emptied")
    assert len(ids) == 0
    m.insert(300)


def erase_then_insert(m, n):
    """the tile the erase ends in holds survivors, then new rows"""
    m.erase_rows_by_id(np.arange(n // 3, max(2 * n // 3, n // 3 + 1)))
    m.insert(100)


def insert_then_erase(m, n):
    """runs of survivors and of rows the table has not seen, old and new, in one tile"""
    m.insert(200)
    m.erase_rows_by_id(np.r_[n // 2:n, n + 50:n + 150])
    m.insert(30)


def upload_again(m, n):
    """the previous list is emptied: every row back at the prior, the IDs kept"""
    m.upload(L.with_lane(L.filler_map(n), m.lane))


PATTERNS = [("nothing removed", lambda m, n: m.erase_rows_by_id([])),
            ("first row", lambda m, n: m.erase_rows_by_id([0])),
            ("last row", lambda m, n: m.erase_rows_by_id([n - 1])),
            ("every other row", every_other_row),
            ("one whole tile", lambda m, n: m.erase_rows_by_id(np.arange(256, min(512, n)))),     # (nothing to erase up to 256 rows)
            ("all but one", lambda m, n: m.keep_only_id(n // 2)),
            ("everything, then an insert", everything_then_an_insert),
            ("erase, then an insert", erase_then_insert),
            ("insert, then erase among old and new", insert_then_erase),
            ("no change, twice", lambda m, n: m.check("the first of two")),
            ("an upload of the same rows", upload_again)]


# 41 and 61: of the 38 class counts in 1 .. 256 for which float(f) * (1 / C) lands one row low for some f below 256 C (so that the flat copy's
# correction has work to do: none of the other six needs it), the smallest, wrong from f = 41 on, and the one with the most such f, 240
@pytest.mark.parametrize("Cn", [1, 2, 3, 7, 41, 61, 255, 256])
def test_alignment(api, Cn):
    sizes = [1, 255, 256, 257, 511, 513] + ([2600] if Cn < 255 else [])
    ef = context(api, 4096)
    try:
        ef.enableLabels(Cn)
        mir = Mirror(ef, api, Cn)
        for n in sizes:
            for name, steps in PATTERNS:
                what = (Cn, n, name)
                mir.upload(L.filler_map(n))
                ids, tab = mir.check(what + ("uploaded",))        # every row at the prior
                assert len(ids) == n and (tab == np.float32(1) / np.float32(Cn)).all()
                mir.set_labels()
                mir.check(what + ("set",))
                steps(mir, n)
                ids, tab = mir.check(what)
                if name == "an upload of the same rows":
                    assert len(ids) == n and (tab == np.float32(1) / np.float32(Cn)).all()
    finally:
        ef.close()


def test_alignment_large(api):
    """More than 8192 x 256 rows, C = 1: workgroup 0 takes a second tile.  Rows go from both of its tiles and from the last, partial one.
    Measured: 0.28 s."""
    t = time.perf_counter()
    n = 8192 * 256 + 300
    ef = context(api, n + 64)
    try:
        ef.enableLabels(1)
        mir = Mirror(ef, api, 1)
        mir.upload(L.filler_map(n))
        mir.set_labels()
        mir.check("set")
        mir.erase_rows(np.r_[0, 100:140, 255, 256, 8192 * 256 - 1, 8192 * 256:8192 * 256 + 7, n - 1])
        mir.insert(40)
        ids, tab = mir.check("large")
        assert len(ids) == n - 52 + 40 and (tab[-40:] == 1).all() and (tab[:-40] != 1).all()
    finally:
        ef.close()
    print(f"alignment, n = {n}, C = 1: {time.perf_counter() - t:.2f} s")


def test_table_growth_by_inserts(api):
    """labels_reserve sizes the table n + max(n / 4, width x height) rows at the label call that finds it too small and carries
    the live half over.  Two growths, the live half a different one each time: old rows keep their bits, new rows get the prior."""
    Cn = 3
    ef = context(api, 1 << 14)
    try:
        ef.enableLabels(Cn)
        mir = Mirror(ef, api, Cn)
        mir.upload(L.filler_map(100))
        mir.set_labels()                       # sized here
        rows, grown_at = 100 + max(100 // 4, P), []
        for step in range(2):
            n0 = len(mir.lane)
            mir.insert(rows - n0 + 1, seed=step)
            assert len(mir.lane) == rows + 1   # one row past the table: the next label call grows it
            grown_at.append(mir.calls % 2)     # every label call swaps the halves
            ids, tab = mir.check(("growth", step))
            assert np.array_equal(bits(tab[:n0]), bits(L.table_rows(ids[:n0], Cn))) and (tab[n0:] == np.float32(1) / np.float32(Cn)).all()
            rows = len(ids) + max(len(ids) // 4, P)
            mir.set_labels()                   # the new rows hold something other than the prior
            mir.check(("growth, set", step))
        assert grown_at[0] != grown_at[1], grown_at
    finally:
        ef.close()


def test_table_growth_by_frames(api):
    """The same growth reached through frames: a small map and a checkpoint restored, then frames that bring new surfels.  The bound of the
    count then comes from labels_count_bound's one-image-per-frame term.  A frame of this sequence creates some 440 surfels where the map is
    empty and a handful where it is not, so every frame's pose is injected 10 m from the last: each frame then meets an empty map, and the
    fifth passes the table's 64 + 1872 rows."""
    from elasticfusion_amd import synth
    seq = synth.Sequence(0xEF0001, W, H)

    def pose(k):
        T = seq.pose(k).copy()
        T[0, 3] += 10.0 * (k - 1)
        return T

    cam = dict(fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)
    fr = [seq.frame(k) for k in range(10)]
    a = context(api, 1 << 15, **cam)
    for k in range(2):
        a.processFrame(fr[k][0], fr[k][1], k, in_T_wc=None if k == 0 else seq.pose(k))
    ck = a.checkpoint(fr[1][0], fr[1][1])
    a.close()
    ck["map"] = ck["map"][:64].copy()
    Cn = 4
    ef = context(api, 1 << 15, **cam)
    try:
        ef.enableLabels(Cn)
        ef.restore(ck)
        ids0, tab = ef.labels()               # sized here: 64 + 1872 rows
        rows = 64 + P
        assert len(ids0) == 64 and (tab == np.float32(0.25)).all()
        ids_prev, tab_prev = ids0, L.table_rows(ids0, Cn)
        ef.setLabels(tab_prev)
        grown = False
        for k in range(2, 10):
            ef.processFrame(fr[k][0], fr[k][1], k, in_T_wc=pose(k))
            ids, tab = ef.labels()
            assert np.array_equal(ids, L.lane_of(ef.downloadMap())), k
            exp = L.align(ids_prev, tab_prev, ids, Cn)
            assert np.array_equal(bits(tab), bits(exp)), (k, len(ids))
            new = ~np.isin(ids, ids_prev)
            print(f"frame {k}: {len(ids)} rows, {int(new.sum())} new, table {rows}")
            if len(ids) > rows:
                grown = True
                rows = len(ids) + max(len(ids) // 4, P)
            tab_prev = exp.copy()
            tab_prev[new] = L.table_rows(ids[new], Cn)     # the new rows hold something other than the prior from here on
            ef.setLabels(tab_prev)
            ids_prev = ids
        assert grown, "the map never outgrew the table"
        assert np.isin(ids0, ids_prev).any()
    finally:
        ef.close()


# ------------------------------------------------------------------------------------------------
# c. fusion
# ------------------------------------------------------------------------------------------------
def check_gate_scene():
    """the gate scene's claims in float64: every designed projection is the integer (or half) it was built for"""
    S, claims = L.gate_scene()
    _, u, v = L.project(S, np.eye(4), L.GATE_CAM, np.float64)
    for name, want in (("u=0", (0, 5)), ("u=cols-1", (W - 1, 9)), ("u=cols", (W, 13)), ("v=0", (8, 0)), ("v=rows-1", (12, H - 1)),
                       ("v=rows", (7, H)), ("u=-1/2", (-0.5, 17)), ("v=-1/2", (17, -0.5)), ("corner 0,0", (0, 0)),
                       ("corner cols-1,rows-1", (W - 1, H - 1)), ("hidden", (20, 10)), ("loser", (30.5, 20.5)), ("twin high", (40, 25))):
        r = claims[name][0]
        assert (u[r], v[r]) == want, (name, u[r], v[r])
    return S, claims


SCENES = {"gates": lambda: (L.gate_scene()[0], L.GATE_CAM, L.GATE_VIEW),
          "turned": lambda: (L.turned_scene(), L.TURNED_CAM, L.TURNED_VIEW),
          "corner": lambda: (L.corner_scene(), L.CORNER_CAM, L.CORNER_VIEW)}


def check_scene(name, S, cam, view, I):
    """what the scene was built for, on the reference's own result"""
    T = view["T_wc"]
    in32, u32, v32 = L.pixel_of(S, T, cam, np.float32)
    in64, u64, v64 = L.pixel_of(S, T, cam, np.float64)
    if name != "corner":    # (whose point is a float32 rounding: half the smallest denormal becomes -0)
        assert np.array_equal(in32, in64) and np.array_equal(u32, u64) and np.array_equal(v32, v64), (name, np.flatnonzero((u32 != u64) | (v32 != v64)))
    obs, u, v = L.observed(S, T, cam, I)
    if name == "gates":
        _, claims = check_gate_scene()
        for what, (row, seen) in claims.items():
            assert bool(obs[row]) == seen, (what, row)
        for what in ("hidden", "twin high", "past max_depth", "u=cols", "v=rows", "u=-1/2", "z=0", "z<0", "z=nan", "x=inf"):
            assert not (I == claims[what][0]).any(), what      # not drawn anywhere
        assert (I == claims["loser"][0]).any()                  # drawn, but not at its own pixel
    elif name == "turned":
        assert obs.sum() >= 40 and (in32 & ~obs).sum() >= 10 and (~in32).sum() >= 40, (obs.sum(), (in32 & ~obs).sum(), (~in32).sum())
    else:
        p, uu, vv = L.project(S, T, cam)
        assert np.signbit(uu[0]) and uu[0] == 0 and np.signbit(vv[0]) and vv[0] == 0      # -0, -0
        assert list(obs) == [True, False, True] and (u[0], v[0]) == (0, 0) and uu[1] == -1.0
    return obs, u, v


@pytest.mark.parametrize("Cn", [1, 2, 256])
@pytest.mark.parametrize("name", list(SCENES))
def test_fusion(api, name, Cn):
    S, cam, view = SCENES[name]()
    n = len(S)
    rng = np.random.RandomState(Cn + len(name))
    ef = context(api, n)
    try:
        ef.enableLabels(Cn)
        ef.uploadMap(S)
        I = ef.renderPointCloud(**view, outputs=("index",))["index"]
        obs, u, v = check_scene(name, S, cam, view, I)
        # values: every row and pixel random, then the k-th observed row and its pixel take recipe k
        P0 = rng.uniform(0.01, 1.0, (n, Cn)).astype(np.float32)
        probs = rng.uniform(0.0, 1.0, (Cn, H, W)).astype(np.float32)
        rec = L.fusion_recipes(Cn)
        plan = {}
        for k, s in enumerate(np.flatnonzero(obs)):
            what, row, o, upd = rec[k % len(rec)]
            P0[s], probs[:, v[s], u[s]] = row, o
            plan[s] = (what, upd)
        for k, s in enumerate(np.flatnonzero(~obs)):               # rows that must not move hold the same special values
            P0[s] = rec[k % len(rec)][1]
        exp, obs2, updated = L.fuse(S, view["T_wc"], cam, I, probs, P0)
        assert np.array_equal(obs, obs2)
        for s, (what, upd) in plan.items():
            assert bool(updated[s]) == upd, (what, s)
        if name != "corner":
            assert {w for w, _ in plan.values()} == {r[0] for r in rec}      # every recipe ran
        assert np.array_equal(bits(exp[~updated]), bits(P0[~updated]))

        ef.setLabels(P0)
        ef.fuseLabels(probs, **view)
        ids, P1 = ef.labels()
        assert np.array_equal(ids, np.arange(1, n + 1, dtype=np.uint32))
        bad = np.flatnonzero((bits(P1) != bits(exp)).any(1))
        assert len(bad) == 0, (len(bad), bad[:5], [plan.get(s) for s in bad[:5]])
        ef.setLabels(P0)
        d = api.DevBuf.from_array(probs)
        ef.fuseLabelsDevice(d.p, ef.renderParams(**view))
        _, P2 = ef.labels()
        assert np.array_equal(bits(P2), bits(P1))
    finally:
        ef.close()


# ------------------------------------------------------------------------------------------------
# d. gather
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 3, 256])
def test_gather(api, Cn):
    S, _ = L.gate_scene()
    n = len(S)
    view = L.GATE_VIEW
    ef = context(api, n)
    try:
        ef.enableLabels(Cn)
        ef.uploadMap(S)
        I = ef.renderPointCloud(**view, outputs=("index",))["index"]
        shown = np.unique(I[I != L.NONE])
        assert len(shown) >= 60 and (I == L.NONE).mean() > 0.3
        rec = L.gather_recipes(Cn)
        tab = np.random.RandomState(Cn).uniform(0, 1, (n, Cn)).astype(np.float32)
        want = {}
        for k, s in enumerate(shown):
            what, row, label = rec[k % len(rec)]
            tab[s] = row
            want[int(s)] = (what, label)
        ef.setLabels(tab)
        label, prob = L.gather(I, tab)
        for s, (what, lab) in want.items():
            assert (label[I == s] == lab).all(), (what, s)
        assert (label[I == L.NONE] == -1).all() and not bits(prob[I == L.NONE]).any()

        got_l, got_p = ef.renderLabels(**view)
        assert np.array_equal(got_l, label) and np.array_equal(bits(got_p), bits(prob))
        p = ef.renderParams(**view)
        lib = api.lib()
        for with_l, with_p in ((True, False), (False, True)):
            hl, hp = np.full((H, W), 77, np.int32), np.full((H, W), 77.0, np.float32)
            rc = lib.ef_render_labels(ef.h, C.byref(p), api._ptr(hl) if with_l else None, api._ptr(hp) if with_p else None)
            assert rc == 0
            assert np.array_equal(hl, label) if with_l else (hl == 77).all()
            assert np.array_equal(bits(hp), bits(prob)) if with_p else (hp == 77).all()
        for with_l, with_p in ((True, True), (True, False), (False, True)):
            dl, dp = api.DevBuf(P * 4, fill=0x55), api.DevBuf(P * 4, fill=0x55)
            ef.renderLabelsDevice(p, label=dl.p if with_l else None, prob=dp.p if with_p else None)
            ef.synchronize()
            hl, hp = dl.to_array(np.int32, (H, W)), dp.to_array(np.uint32, (H, W))
            assert np.array_equal(hl, label) if with_l else (hl == 0x55555555).all()
            assert np.array_equal(hp, bits(prob)) if with_p else (hp == 0x55555555).all()
    finally:
        ef.close()
