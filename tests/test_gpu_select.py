"""Select, extract and erase surfels on the device (ef_map_select / ef_map_gather / ef_map_erase, include/ef_hip.h; kernels in
elasticfusion_amd/csrc/ef_select.inc).

The selection is restated in numpy from the header alone (tests/selectref.py): float32, one rounding per operation, NaN comparisons false,
selected = (every enabled test passes) XOR invert.  The device must give the same row lists exactly; gather must equal downloadMap()[rows]
and an erase before[~mask], bit for bit; and a context that erases and keeps mapping must compute what a fresh context computes after
uploadMap(kept rows) + restore, bit for bit.
"""
import numpy as np
import pytest

import selectref as sr
from queryref import MISS, assert_bits_equal, brute

pytestmark = pytest.mark.gpu

F = np.float32
NC = 5   # label classes of the edge scene


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def step(v, up):
    return np.nextafter(F(v), F(np.inf) if up else F(-np.inf))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the edge scene (pure numpy: what it contains is asserted on the CPU before the device is asked anything)
# ---------------------------------------------------------------------------------------------------------------------------------------
def scene_T():
    a, b = 0.7, 0.4
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Rx
    T[:3, 3] = (0.3125, -0.1875, 0.25)   # (short mantissas: the sum with them never falls half-way between two floats)
    return T


# (the bounds and the translation are chosen so that, at every face, the last addition of the box expression does not land in a binade finer
# than its left operand's: only then is every float next to the bound the image of some float32 point)
BOX_LO, BOX_HI = np.array([-1.25, -2.0, 0.5], F), np.array([1.0, 1.5, 3.0], F)
CONF_LO, CONF_HI = F(2.5), F(10.0)
RAD_LO, RAD_HI = F(0.003), F(0.01)
INIT_LO, INIT_HI = 5, 40
LAST_LO, LAST_HI = 17, 90
MIN_PROB = F(0.4)
LABEL_CLASS = 1


def face_points(T):
    """World points whose box coordinate lies exactly on each face of the box and one float to either side of it (the other two coordinates
    well inside): found by moving a point that is close to the face by a few floats per coordinate until the float32 expression of the header
    gives exactly the wanted value."""
    Ti = np.linalg.inv(T)
    mid = ((BOX_LO.astype(np.float64) + BOX_HI) / 2)
    k = np.arange(-6, 7)
    dx, dy, dz = (g.reshape(-1) for g in np.meshgrid(k, k, k, indexing="ij"))
    pts, want = [], []
    for a in range(3):
        for bound in (BOX_LO[a], BOX_HI[a]):
            b = mid.copy()
            b[a] = bound
            p0 = (Ti[:3, :3] @ b + Ti[:3, 3]).astype(F)
            # candidates: p0 moved by up to 6 floats per coordinate
            cand = np.stack([p0[0] + dx * np.spacing(p0[0]), p0[1] + dy * np.spacing(p0[1]), p0[2] + dz * np.spacing(p0[2])], 1).astype(F)
            bc = sr.box_coords(cand, T)[:, a]
            for target in (step(bound, False), F(bound), step(bound, True)):
                hit = np.nonzero(bc == target)[0]
                assert len(hit), ("no float32 point lands on", a, float(bound), float(target))
                pts.append(cand[hit[0]])
                want.append((a, target))
    return np.array(pts, F), want


def edge_scene():
    """(surfels n x 12, label table n x NC): n = 2600 rows, eleven chunks of 256 and not a multiple of them"""
    rng = np.random.default_rng(2024)
    T = scene_T()
    fp, _ = face_points(T)
    n0 = 2600
    S = np.zeros((n0, 12), F)
    S[:, :3] = rng.uniform(-4, 4, (n0, 3))
    # half of the rows in and around the box (drawn in its frame, a margin of half a metre around it)
    inb = rng.uniform(BOX_LO.astype(np.float64) - 0.5, BOX_HI.astype(np.float64) + 0.5, (n0 // 2, 3))
    Ti = np.linalg.inv(T)
    S[1::2, :3] = (inb @ Ti[:3, :3].T + Ti[:3, 3]).astype(F)
    S[:len(fp), :3] = fp
    special = np.array([[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.inf, 0, 0], [0, -np.inf, 0], [np.nan, np.nan, np.nan],
                        [np.inf, np.inf, -np.inf]], F)
    at = 100 + 37 * np.arange(len(special))
    S[at, :3] = special
    conf_edges = np.array([CONF_LO, CONF_HI, step(CONF_LO, False), step(CONF_LO, True), step(CONF_HI, False), step(CONF_HI, True), np.nan, np.inf, 0], F)
    S[:, 3] = np.where(rng.random(n0) < 0.3, rng.choice(conf_edges, n0), rng.uniform(0, 14, n0).astype(F))
    S[:, 4] = rng.integers(0, 1 << 24, n0).astype(F)                 # the packed colour
    rad_edges = np.array([RAD_LO, RAD_HI, step(RAD_LO, False), step(RAD_LO, True), step(RAD_HI, False), step(RAD_HI, True), np.nan], F)
    S[:, 11] = np.where(rng.random(n0) < 0.3, rng.choice(rad_edges, n0), rng.uniform(0.001, 0.02, n0).astype(F))
    S[:, 6] = np.where(rng.random(n0) < 0.4, rng.choice([INIT_LO - 1, INIT_LO, INIT_HI, INIT_HI + 1], n0), rng.integers(1, 60, n0)).astype(F)
    S[:, 7] = np.where(rng.random(n0) < 0.4, rng.choice([LAST_LO - 1, LAST_LO, LAST_HI, LAST_HI + 1], n0), rng.integers(1, 120, n0)).astype(F)
    nrm = rng.normal(size=(n0, 3))
    S[:, 8:11] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    # IDs: strictly increasing, non-zero, with the top bit set at the end (the comparison is unsigned)
    ids = (10 + 3 * np.arange(n0)).astype(np.uint32)
    ids[-2:] = (0x80000005, 0xFFFFFFF0)
    S[:, 5] = ids.view(F)
    # labels: random rows, then the edge rows
    P = rng.dirichlet(np.ones(NC), n0).astype(F)
    lo, hi = step(MIN_PROB, False), step(MIN_PROB, True)
    edge = np.array([[0.1, 0.4, 0.4, 0.05, 0.05],        # classes 1 and 2 tie: class 1, the maximum exactly at the bound
                     [0.4, 0.4, 0.1, 0.05, 0.05],        # classes 0 and 1 tie: class 0
                     [0.1, lo, 0.2, 0.2, 0.1],           # class 1, one float below the bound
                     [0.1, hi, 0.2, 0.2, 0.1],           # class 1, one float above it
                     [0.2, 0.2, 0.2, 0.2, 0.2],          # all equal: class 0
                     [0.05, 0.9, 0.05, 0.0, 0.0],
                     [np.nan, 0.9, 0.05, 0.0, 0.0],      # a NaN first entry is never replaced
                     [0.0, 0.45, np.nan, 0.45, 0.1]], F)  # a NaN later entry never wins; classes 1 and 3 tie
    P[200:200 + len(edge)] = edge
    P[1500:1500 + len(edge)] = edge
    return S, P


def selections():
    """name -> selectref dict: every single test, three combinations, each with and without INVERT, all and none"""
    T = scene_T()
    base = dict(T_bw=T, box_min=BOX_LO, box_max=BOX_HI, conf_min=CONF_LO, conf_max=CONF_HI, init_time_min=INIT_LO, init_time_max=INIT_HI,
                last_time_min=LAST_LO, last_time_max=LAST_HI, radius_min=RAD_LO, radius_max=RAD_HI, id_min=10 + 3 * 100, id_max=0x80000005,
                label_class=LABEL_CLASS, label_min_prob=MIN_PROB)
    single = dict(box=sr.BOX, conf=sr.CONF, init_time=sr.INIT_TIME, last_time=sr.LAST_TIME, radius=sr.RADIUS, id=sr.ID, label=sr.LABEL)
    combos = dict(box_conf=sr.BOX | sr.CONF, last_radius_id=sr.LAST_TIME | sr.RADIUS | sr.ID,
                  all_seven=sr.BOX | sr.CONF | sr.INIT_TIME | sr.LAST_TIME | sr.RADIUS | sr.ID | sr.LABEL)
    out = {"everything": sr.default_selection(), "nothing": sr.default_selection(tests=sr.INVERT)}
    for name, t in {**single, **combos}.items():
        out[name] = sr.default_selection(tests=t, **base)
        out[name + "_inverted"] = sr.default_selection(tests=t | sr.INVERT, **base)
    # a second ID range: both ends of the lane
    out["id_ends"] = sr.default_selection(tests=sr.ID, id_min=10, id_max=0xFFFFFFF0)
    out["id_inside"] = sr.default_selection(tests=sr.ID, id_min=11, id_max=0xFFFFFFEF)
    # a half-space: infinite bounds are allowed
    out["half_space"] = sr.default_selection(tests=sr.BOX, T_bw=T, box_min=[-np.inf, -np.inf, BOX_LO[2]], box_max=[np.inf] * 3)
    return out


def to_api(ef, sel):
    kw = dict(sel)
    kw["tests"] = int(kw["tests"])
    for k in ("conf_min", "conf_max", "radius_min", "radius_max", "label_min_prob"):
        kw[k] = float(kw[k])
    for k in ("init_time_min", "init_time_max", "last_time_min", "last_time_max", "id_min", "id_max", "label_class"):
        kw[k] = int(kw[k])
    return ef.mapSelection(**kw)


def test_the_scene_contains_every_edge_the_header_names():
    """CPU only in effect (no device call): the reference alone shows that the edges are exercised"""
    S, P = edge_scene()
    T = scene_T()
    assert len(S) % 256 and len(S) > 10 * 256
    b = sr.box_coords(S[:, :3], T)
    inside = sr.in_box(b, BOX_LO, BOX_HI)
    for a in range(3):
        for bound, is_lo in ((BOX_LO[a], True), (BOX_HI[a], False)):
            on, below, above = b[:, a] == bound, b[:, a] == step(bound, False), b[:, a] == step(bound, True)
            assert on.any() and below.any() and above.any(), (a, bound)
            assert inside[on].all(), "a point exactly on a face is inside"
            assert (~inside[below]).all() if is_lo else inside[below].all()
            assert inside[above].all() if is_lo else (~inside[above]).all()
    nanpos, infpos = np.isnan(S[:, :3]).any(1), np.isinf(S[:, :3]).any(1)
    assert nanpos.sum() >= 4 and infpos.sum() >= 3 and not inside[nanpos].any()
    sels = selections()
    assert sr.select_mask(S, sels["box_inverted"], P)[nanpos].all(), "under INVERT a NaN position that fails BOX is selected"
    for col, lo, hi in ((3, CONF_LO, CONF_HI), (11, RAD_LO, RAD_HI)):
        for v in (lo, hi, step(lo, False), step(lo, True), step(hi, False), step(hi, True)):
            assert (S[:, col] == v).any(), (col, v)
        assert np.isnan(S[:, col]).any()
    for col, lo, hi in ((6, INIT_LO, INIT_HI), (7, LAST_LO, LAST_HI)):
        for v in (lo - 1, lo, hi, hi + 1):
            assert (S[:, col] == F(v)).any(), (col, v)
    ids = u32(S[:, 5])
    s = sels["id"]
    for v in (s["id_min"] - 3, s["id_min"], s["id_max"], 0xFFFFFFF0):
        assert (ids == v).any(), v
    assert (np.diff(ids.astype(np.int64)) > 0).all() and ids[0] > 0
    best, m = sr.label_argmax(P)
    ties = (P == P.max(1, keepdims=True)).sum(1) >= 2
    assert ties.sum() >= 4 and (best[200:205] == [1, 0, 1, 1, 0]).all() and (best[206:208] == [0, 1]).all()
    assert (m[best == LABEL_CLASS] == MIN_PROB).any() and (m == step(MIN_PROB, False)).any() and (m == step(MIN_PROB, True)).any()
    passed = sr.passes(S, sels["label"], P)[sr.LABEL]
    assert passed[200] and not passed[201] and not passed[202] and passed[203] and not passed[206] and passed[207]
    # every selection selects something and leaves something (but for the two trivial ones)
    for name, sel in sels.items():
        k = int(sr.select_mask(S, sel, P).sum())
        assert (0 < k < len(S)) or name in ("everything", "nothing", "id_ends"), (name, k)


@pytest.fixture(scope="module")
def edge():
    from elasticfusion_amd import api
    S, P = edge_scene()
    ef = api.ElasticFusion()
    ef.setSurfelIds(True)
    ef.enableLabels(NC)
    ef.uploadMap(S)
    ef.setLabels(P)
    yield dict(ef=ef, S=S, P=P)
    ef.close()


def test_select_equals_the_scan_exactly(edge):
    ef, S, P = edge["ef"], edge["S"], edge["P"]
    assert_bits_equal(ef.downloadMap(), S, "the uploaded scene")
    assert_bits_equal(ef.labels()[1], P, "the uploaded labels")
    for name, sel in selections().items():
        want = sr.select_rows(S, sel, P)
        rows, total = ef.selectSurfels(to_api(ef, sel), count=True)
        print(name, "selects", len(want), "of", len(S))
        assert total == len(want), (name, total, len(want))
        assert rows.dtype == np.uint32 and np.array_equal(rows, want), (name, np.setxor1d(rows, want)[:8])
        assert ef.countSurfels(to_api(ef, sel)) == len(want), name


def test_select_device_variant_only_writes_what_it_should(edge):
    from elasticfusion_amd import api
    ef, S, P = edge["ef"], edge["S"], edge["P"]
    sel = selections()["box_conf_inverted"]
    want = sr.select_rows(S, sel, P)
    cap = len(want) - 7
    rows = api.DevBuf.from_array(np.full(cap + 16, 0xABABABAB, np.uint32))
    cnt = api.DevBuf.from_array(np.zeros(1, np.uint32))
    ef.selectSurfelsDevice(to_api(ef, sel), rows.p, cap, cnt.p)
    ef.synchronize()
    got = rows.to_array(np.uint32, cap + 16)
    assert cnt.to_array(np.uint32, 1)[0] == len(want)
    assert np.array_equal(got[:cap], want[:cap]) and (got[cap:] == 0xABABABAB).all()
    ef.selectSurfelsDevice(to_api(ef, sel), None, 0, cnt.p)    # a count only
    ef.synchronize()
    assert cnt.to_array(np.uint32, 1)[0] == len(want)


# ---------------------------------------------------------------------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------------------------------------------------------------------
# 2^20 + 4097 rows are 4113 chunks of 256: the one-workgroup scan of the chunk counts (k_scan_chunks, 1024 counts per trip) takes a first trip,
# full trips with a carry from the trip before, and a last partial trip; every smaller count here takes a single trip
BIG = (1 << 20) + 4097
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, BIG)


def plain_map(n):
    S = np.zeros((n, 12), F)
    i = np.arange(n)
    S[:, 0] = (i % 1000) * F(0.001)
    S[:, 3] = 5
    S[:, 6] = i % 2          # creation time: the parity of the row
    S[:, 7] = 1
    if n:
        S[-1, 7] = 7         # only the last row was seen at tick 7
    S[:, 11] = 0.004
    return S


@pytest.fixture(scope="module")
def sized():
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    yield ef
    ef.close()


@pytest.mark.parametrize("n", COUNTS)
def test_sizes_and_clamping(sized, n):
    ef = sized
    ef.uploadMap(plain_map(n))
    assert ef.lastCount() == n
    every = np.arange(n, dtype=np.uint32)
    cases = dict(all=(ef.mapSelection(), every), none=(ef.mapSelection(tests=sr.INVERT), every[:0]),
                 odd=(ef.mapSelection(tests=sr.INIT_TIME, init_time_min=1, init_time_max=1), every[1::2]),
                 last=(ef.mapSelection(tests=sr.LAST_TIME, last_time_min=7, last_time_max=7), every[n - 1:] if n else every[:0]))
    for name, (sel, want) in cases.items():
        rows, total = ef.selectSurfels(sel, count=True)
        assert total == len(want) and np.array_equal(rows, want), (n, name, total, len(want))
    sel, want = cases["odd"]
    total = len(want)
    for cap in sorted({0, 1, max(total - 1, 0), total, total + 1}):
        rows, got = ef.selectSurfels(sel, max_rows=cap, count=True)
        assert got == total, (n, cap, got, total)          # the count is the total, however short the list
        assert np.array_equal(rows, want[:cap]), (n, cap)


# ---------------------------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_gather_equals_download_rows(edge):
    from elasticfusion_amd import api
    ef, S = edge["ef"], edge["S"]
    n = len(S)
    rng = np.random.default_rng(5)
    rows = rng.integers(0, n, 3001).astype(np.uint32)
    rows[:4] = (n - 1, 0, n - 1, 0)                        # duplicates
    m = ef.downloadMap()
    assert_bits_equal(ef.gatherSurfels(rows), m[rows], "gather")
    assert np.array_equal(u32(ef.gatherSurfels(rows)[:, 5]), ef.surfelIds()[rows])     # with IDs on, lane 5 is the ID
    bad = rows.copy()
    out_of_range = np.array([n, n + 5, 0xFFFFFFFF, 1 << 31], np.uint32)
    bad[10:14] = out_of_range
    g = ef.gatherSurfels(bad)
    ok = np.ones(len(bad), bool)
    ok[10:14] = False
    assert_bits_equal(g[ok], m[bad[ok]], "gather beside rows past the map")
    assert (u32(g[~ok]) == 0).all(), "a row past the map gives twelve zero words"
    assert ef.gatherSurfels(np.zeros(0, np.uint32)).shape == (0, 12)
    d_rows = api.DevBuf.from_array(rows)
    d_out = api.DevBuf(len(rows) * 48 + 64, fill=0xCD)
    ef.gatherSurfelsDevice(d_rows.p, len(rows), d_out.p)
    ef.synchronize()
    raw = d_out.to_array(np.uint8, len(rows) * 48 + 64)
    assert_bits_equal(raw[:len(rows) * 48].view(F).reshape(-1, 12), m[rows], "gather, device variant")
    assert (raw[len(rows) * 48:] == 0xCD).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# erase
# ---------------------------------------------------------------------------------------------------------------------------------------
def fresh_edge():
    from elasticfusion_amd import api
    S, P = edge_scene()
    ef = api.ElasticFusion()
    ef.setSurfelIds(True)
    ef.enableLabels(NC)
    ef.uploadMap(S)
    ef.setLabels(P)
    return ef, S, P


def check_after_erase(ef, S, P, mask, removed, what):
    assert removed == int(mask.sum()) and 0 < removed < len(S), (what, removed, int(mask.sum()))
    kept = S[~mask]
    assert_bits_equal(ef.downloadMap(), kept, what + ": the map is the kept rows in their old order")
    assert np.array_equal(ef.surfelIds(), u32(kept[:, 5])), what
    ids, probs = ef.labels()
    assert np.array_equal(ids, u32(kept[:, 5])), what
    assert_bits_equal(probs, P[~mask], what + ": the labels of the kept rows")
    # the index went stale: a query sees the edited map and never an erased surfel
    fin = np.isfinite(S[:, :3]).all(1)
    pts = np.concatenate([S[mask & fin][:150, :3], S[~mask & fin][:150, :3]])
    row, d2, plane = ef.queryNearestRaw(pts, 0.05, -1.0)
    er, ed, ep, _ = brute(pts, kept, 0.05, -1.0)
    assert_bits_equal(row, er[:, 0], what + ": query rows")
    assert_bits_equal(d2, ed[:, 0], what + ": query dist2")
    assert_bits_equal(plane, ep, what + ": query plane")
    assert (row != MISS).sum() >= 100 and (row[row != MISS] < len(kept)).all()


def test_erase_by_selection():
    ef, S, P = fresh_edge()
    try:
        ef.queryNearestRaw(S[:8, :3], 0.05, -1.0)            # an index built before the erase
        sel = selections()["box_conf"]
        mask = sr.select_mask(S, sel, P)
        removed = ef.eraseSurfels(to_api(ef, sel))
        check_after_erase(ef, S, P, mask, removed, "eraseSurfels")
        # a second erase on the edited map, by label; then one that selects nothing
        S2, P2 = S[~mask], P[~mask]
        sel2 = selections()["label_inverted"]
        mask2 = sr.select_mask(S2, sel2, P2)
        check_after_erase(ef, S2, P2, mask2, ef.eraseSurfels(to_api(ef, sel2)), "eraseSurfels by label")
        assert ef.eraseSurfels(tests=sr.INVERT) == 0 and ef.lastCount() == int((~mask2).sum())
        assert_bits_equal(ef.downloadMap(), S2[~mask2], "an erase of nothing")
    finally:
        ef.close()


@pytest.mark.parametrize("device", (False, True))
def test_erase_rows(device):
    from elasticfusion_amd import api
    ef, S, P = fresh_edge()
    try:
        ef.queryNearestRaw(S[:8, :3], 0.05, -1.0)
        n = len(S)
        rng = np.random.default_rng(9)
        rows = rng.integers(0, n, 900).astype(np.uint32)
        rows = np.concatenate([rows, rows[:100], np.array([n, n + 1, 0xFFFFFFFF, n - 1, 0, 0], np.uint32)])   # duplicates, rows past the map, both ends
        rng.shuffle(rows)
        mask = np.zeros(n, bool)
        mask[rows[rows < n]] = True
        if device:
            d = api.DevBuf.from_array(rows)
            removed = ef.eraseRowsDevice(d.p, len(rows))
        else:
            removed = ef.eraseRows(rows)
        check_after_erase(ef, S, P, mask, removed, "eraseRowsDevice" if device else "eraseRows")
        assert ef.eraseRows(np.zeros(0, np.uint32)) == 0 and ef.lastCount() == n - removed
    finally:
        ef.close()


def test_ids_are_never_reused_after_an_erase(frames):
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    try:
        ef.setSurfelIds(True)
        for k in range(3):
            ef.processFrame(frames[k][0], frames[k][1], k)
        before = ef.downloadMap()               # (numbers the rows the last frame created)
        ids = u32(before[:, 5])
        n = len(ids)
        largest = int(ids.max())
        assert ids[-1] == largest
        rows = np.arange(n - 2000, n, dtype=np.uint32)       # the newest surfels go, the holder of the largest ID among them
        assert ef.eraseRows(rows) == 2000
        assert_bits_equal(ef.downloadMap(), before[:n - 2000], "erase after frames")
        assert int(ef.surfelIds().max()) < largest
        ef.processFrame(frames[3][0], frames[3][1], 3)
        after = ef.surfelIds()
        new = ~np.isin(after, ids)
        print("surfels", n, "erased 2000, after the next frame", len(after), "of them new", int(new.sum()))
        assert new.sum() > 0 and int(after[new].min()) > largest
        assert (np.diff(after.astype(np.int64)) > 0).all()
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# erase, then keep mapping = upload + restore
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sixteen(seq):
    return [seq.frame(k) for k in range(16)]


def state_of(ef):
    return ef.getPoseQT(), np.asarray(ef.trackingStats()[0], F), ef.downloadMap()


@pytest.mark.parametrize("persistent", (True, False))
def test_erase_then_mapping_equals_upload_and_restore(sixteen, persistent):
    from elasticfusion_amd import api
    fr = sixteen

    def context():
        ef = api.ElasticFusion()
        if not persistent:
            ef.setPersistentTracker(0)
        return ef

    def feed(ef, k):
        ef.processFrame(fr[k][0], fr[k][1], k * 33333)

    a, b, plain = context(), context(), context()
    try:
        for k in range(12):
            feed(a, k)
            feed(plain, k)
        thr = a.getConfidenceThreshold()
        # the world half-space x <= 0, AND a confidence below the threshold
        ref = sr.default_selection(tests=sr.BOX | sr.CONF, box_max=[0.0, np.inf, np.inf], conf_max=float(step(thr, False)))
        sel = to_api(a, ref)
        m12 = a.downloadMap()
        mask = sr.select_mask(m12, ref)
        ck = a.checkpoint(fr[11][0], fr[11][1])
        removed = a.eraseSurfels(sel)
        print("frame 12: surfels", len(m12), "erased", removed)
        assert removed == int(mask.sum()) and removed > 1000 and (~mask).sum() > 1000
        kept = a.downloadMap()
        assert_bits_equal(kept, m12[~mask], "the edited map")
        assert a.countSurfels(sel) == 0 and not sr.select_mask(kept, ref).any()         # nothing of the kind is left in the box
        assert a.getTick() == ck["tick"] and np.array_equal(a.getPoseQT(), ck["qt"])
        ck["map"] = m12[~mask]
        b.restore(ck)
        for k in range(12, 16):
            feed(a, k)
            feed(b, k)
            feed(plain, k)
            (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
            assert np.array_equal(qa.view(np.uint64), qb.view(np.uint64)), (k, qa, qb)
            assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), (k, sa, sb)
            assert_bits_equal(ma, mb, f"the map after frame {k}")
        mp = plain.downloadMap()
        assert mp.shape != ma.shape or not np.array_equal(u32(mp), u32(ma)), "the erase mattered"
    finally:
        for ef in (a, b, plain):
            ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals on the device path
# ---------------------------------------------------------------------------------------------------------------------------------------
def refused(fn, code):
    from elasticfusion_amd import api
    with pytest.raises(api.EFError) as e:
        fn()
    assert f"error {code}:" in str(e.value), str(e.value)
    return str(e.value)


def test_state_refusals():
    from elasticfusion_amd import api
    S = plain_map(1000)
    ef = api.ElasticFusion()
    try:
        ef.uploadMap(S)
        for call in (ef.selectSurfels, ef.countSurfels, ef.eraseSurfels):
            assert "IDs are off" in refused(lambda: call(tests=sr.ID), -4)          # EF_ESTATE
            assert "labels are off" in refused(lambda: call(tests=sr.LABEL), -4)
        assert ef.lastCount() == 1000
        ef.enableLabels(3)
        refused(lambda: ef.countSurfels(tests=sr.LABEL, label_class=3), -1)           # EF_EINVAL: outside 0 .. C-1
        assert ef.countSurfels(tests=sr.LABEL, label_class=0, label_min_prob=0.0) == 1000   # the prior 1/3 everywhere: ties go to class 0
        assert ef.countSurfels(tests=sr.LABEL, label_class=2, label_min_prob=0.0) == 0
    finally:
        ef.close()
    ef = api.ElasticFusion(closeLoops=True)
    try:
        ef.uploadMap(S)
        sel = ef.mapSelection(tests=sr.INIT_TIME, init_time_min=1, init_time_max=1)
        assert "close_loops" in refused(lambda: ef.eraseSurfels(sel), -4)
        assert "close_loops" in refused(lambda: ef.eraseRows(np.arange(4, dtype=np.uint32)), -4)
        d = api.DevBuf.from_array(np.arange(4, dtype=np.uint32))
        assert "close_loops" in refused(lambda: ef.eraseRowsDevice(d.p, 4), -4)
        assert ef.lastCount() == 1000
        assert np.array_equal(ef.selectSurfels(sel), np.arange(1, 1000, 2, dtype=np.uint32))      # select and gather work there
        assert_bits_equal(ef.gatherSurfels([5, 999, 5]), S[[5, 999, 5]], "gather on a loop-closing context")
    finally:
        ef.close()
