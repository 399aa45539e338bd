"""Spatial index and nearest-surfel / kNN queries (ef_query_nearest / ef_query_knn, include/ef_hip.h; kernels in
elasticfusion_amd/csrc/ef_query.inc).

The specification is restated here in numpy and evaluated exhaustively (every query against every row):
    d2    = ((qx-px)*(qx-px) + (qy-py)*(qy-py)) + (qz-pz)*(qz-pz)        f32, one rounding per operation
    plane = ((qx-px)*nx + (qy-py)*ny) + (qz-pz)*nz
    eligible iff conf > min_conf and d2 <= r2 (r2 = max_dist * max_dist in f32); order (d2, row), ties to the lower row
and the device must give the same rows, d2 and plane bit for bit, whatever the grid's cell size.  Queries must change nothing a frame
computes, and the index must follow the map.
"""
import ctypes as C
import os

import numpy as np
import pytest

from queryref import MISS, F, assert_bits_equal, brute, default_cell

pytestmark = pytest.mark.gpu


def check_nearest(ef, pts, surfels, max_dist, min_conf, what):
    row, d2, plane = ef.queryNearestRaw(pts, max_dist, min_conf)
    er, ed, ep, _ = brute(pts, surfels, max_dist, min_conf)
    assert_bits_equal(row, er[:, 0], what + " rows")
    assert_bits_equal(d2, ed[:, 0], what + " dist2")
    assert_bits_equal(plane, ep, what + " plane")
    return row, d2, plane


@pytest.fixture(scope="module")
def big(seq):
    from elasticfusion_amd import api, synth
    surfels = synth.sample_surfels(synth.Sequence(0xEF0001), n=1 << 18)
    assert len(surfels) == 261769
    ef = api.ElasticFusion()
    ef.uploadMap(surfels)
    rng = np.random.default_rng(7)
    set1 = (surfels[rng.integers(0, len(surfels), 4096), :3].astype(np.float64) + rng.normal(0, 0.005, (4096, 3))).astype(np.float32)
    lo, hi = surfels[:, :3].min(0).astype(np.float64) - 0.5, surfels[:, :3].max(0).astype(np.float64) + 0.5
    set2 = np.random.default_rng(8).uniform(lo, hi, (4096, 3)).astype(np.float32)
    yield dict(ef=ef, surfels=surfels, set1=set1, set2=set2)
    ef.close()


def test_nearest_equals_exhaustive_f32_bit_for_bit(big):
    ef, S = big["ef"], big["surfels"]
    cell = default_cell()
    ef.setQueryCell(cell)
    row1, d2_1, pl1 = check_nearest(ef, big["set1"], S, 0.02, -1.0, "set one")
    print("set one: hits", int((row1 != MISS).sum()), "largest nearest distance", float(np.sqrt(d2_1[row1 != MISS].max())))
    assert (row1 != MISS).sum() >= 4000
    row2, _, _ = check_nearest(ef, big["set2"], S, 0.02, -1.0, "set two")
    print("set two: hits", int((row2 != MISS).sum()), "misses", int((row2 == MISS).sum()))
    assert (row2 == MISS).any() and (row2 != MISS).any()
    for c in (cell / 4, cell * 4):
        ef.setQueryCell(c)
        r, d, p = ef.queryNearestRaw(big["set1"], 0.02, -1.0)
        assert_bits_equal(r, row1, f"cell {c} rows")
        assert_bits_equal(d, d2_1, f"cell {c} dist2")
        assert_bits_equal(p, pl1, f"cell {c} plane")
    ef.setQueryCell(cell)
    big["nearest1"] = (row1, d2_1)


def test_nearest_against_float64(big):
    ef, S = big["ef"], big["surfels"]
    row, dist, _ = ef.queryNearest(big["set1"], 0.02, -1.0)
    er, ed, _, _ = brute(big["set1"], S, 0.02, -1.0, dtype=np.float64, chunk=32)
    both = (row != MISS) & (er[:, 0] != MISS)
    assert both.sum() >= 4000
    err = np.abs(dist[both].astype(np.float64) - np.sqrt(ed[both, 0]))
    other = int((row != er[:, 0]).sum())   # a miss on one side only counts as well
    print("float64: largest distance difference", float(err.max()), "m; rows that differ", other, "of", len(row))
    assert err.max() <= 1e-7
    assert other <= 4


@pytest.mark.parametrize("k", [1, 4, 8, 16])
def test_knn_equals_exhaustive_f32(big, k):
    ef, S = big["ef"], big["surfels"]
    pts = big["set1"][:1024]
    if "knn16" not in big:
        big["knn16"] = brute(pts, S, 0.03, -1.0, k=16)
    er, ed, _, ec = big["knn16"]
    rows, d2, cnt = ef.queryKnn(pts, k, 0.03, -1.0)
    print("k", k, "eligible min / median / max", int(ec.min()), float(np.median(ec)), int(ec.max()))
    assert_bits_equal(cnt, ec, "count")
    assert_bits_equal(rows, np.ascontiguousarray(er[:, :k]), "rows")
    assert_bits_equal(d2, np.ascontiguousarray(ed[:, :k]), "dist2")
    if k in (4, 8):
        assert (ec > k).any()
    if k == 16:
        assert (rows == MISS).any()
    if k == 1:
        r1, d1, _ = ef.queryNearestRaw(pts, 0.03, -1.0)
        assert_bits_equal(rows[:, 0], r1, "k = 1 rows against nearest")
        assert_bits_equal(d2[:, 0], d1, "k = 1 dist2 against nearest")


def one_surfel(x, y, z, conf=12.0):
    s = np.zeros(12, np.float32)
    s[:3] = x, y, z
    s[3] = conf
    s[6] = s[7] = 1
    s[8:11] = 0.6, 0.0, 0.8
    s[11] = 0.004
    return s


def test_edge_cases():
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    q = np.array([[0.1, 0.2, 1.0]], np.float32)
    # an empty map (before the first frame), and n = 0
    row, dist, plane, ids = None, None, None, None
    row, dist, plane = ef.queryNearest(q, 0.05)
    assert row[0] == MISS and np.isposinf(dist[0]) and plane[0] == 0
    rows, d2, cnt = ef.queryKnn(q, 4, 0.05)
    assert (rows == MISS).all() and np.isposinf(d2).all() and cnt[0] == 0
    row, dist, plane = ef.queryNearest(np.zeros((0, 3), np.float32), 0.05)
    assert len(row) == 0 and len(dist) == 0 and len(plane) == 0
    rows, d2, cnt = ef.queryKnn(np.zeros((0, 3), np.float32), 4, 0.05)
    assert rows.shape == (0, 4) and len(cnt) == 0
    # the same surfel twice in a row: the lower row wins, kNN lists both in row order
    s = one_surfel(0.1, 0.2, 1.004)
    other = one_surfel(0.1, 0.2, 1.3)
    ef.uploadMap(np.stack([other, s, s, other]))
    row, d2, plane = check_nearest(ef, q, np.stack([other, s, s, other]), 0.05, -1.0, "duplicate")
    assert row[0] == 1
    rows, d2k, cnt = ef.queryKnn(q, 4, 0.05)
    assert rows[0].tolist() == [1, 2, MISS, MISS] and cnt[0] == 2 and d2k[0, 0] == d2k[0, 1] == d2[0] and np.isposinf(d2k[0, 2:]).all()
    # ids need the switch
    with pytest.raises(api.EFError, match="error -4"):
        ef.queryNearest(q, 0.05, ids=True)
    # max_dist / cell: 16 is served, more is refused before any GPU work
    ef.setQueryCell(0.0625)
    assert ef.queryNearest(q, 1.0)[0][0] == 1
    with pytest.raises(api.EFError, match="error -1"):
        ef.queryNearest(q, 1.5)
    with pytest.raises(api.EFError, match="error -1"):
        ef.queryKnn(q, 4, 1.5)
    ef.setQueryCell(default_cell())
    # min_conf at, below and above the uploaded confidence (eligible iff conf > min_conf)
    for mc, hit in ((12.0, False), (11.5, True), (12.5, False), (-1.0, True)):
        r = ef.queryNearest(q, 0.05, mc)[0]
        assert (r[0] != MISS) == hit, (mc, r)
    # NaN and inf query coordinates never match; the finite ones beside them do
    bad = np.array([[np.nan, 0.2, 1.0], [0.1, np.inf, 1.0], [0.1, 0.2, -np.inf], [0.1, 0.2, 1.0], [np.nan, np.nan, np.nan]], np.float32)
    row, dist, plane = ef.queryNearest(bad, 0.05)
    assert row.tolist() == [MISS, MISS, MISS, 1, MISS] and np.isposinf(dist[[0, 1, 2, 4]]).all() and (plane[[0, 1, 2, 4]] == 0).all()
    rows, _, cnt = ef.queryKnn(bad, 4, 0.05)
    assert cnt.tolist() == [0, 0, 0, 2, 0]
    # a surfel with a non-finite position is never returned
    S = np.stack([one_surfel(np.nan, 0.2, 1.0), one_surfel(0.1, np.inf, 1.0), s])
    ef.uploadMap(S)
    assert ef.queryNearest(q, 0.05)[0][0] == 2
    # a surfel 1e6 m away (far outside the grid's clamp) with a query beside it
    S = np.stack([one_surfel(1e6, 0.0, 0.0), one_surfel(-1e6, 3e5, -2e6), one_surfel(0.0, 0.0, 1.0)])
    Q = np.array([[1e6, 0.005, 0.0], [-1e6, 3e5, -2e6], [1e6, 0.5, 0.0], [0.0, 0.01, 1.0]], np.float32)
    ef.uploadMap(S)
    row, _, _ = check_nearest(ef, Q, S, 0.02, -1.0, "far away")
    assert row.tolist() == [0, 1, MISS, 2]
    ef.close()


@pytest.mark.parametrize("cell", [0.03125, 0.02, 0.1])
def test_cell_boundaries(cell):
    """surfels and queries on exact multiples of the cell size, positive and negative, and one float to either side; max_dist one and two cells
    and just under: a surfel at exactly max_dist (d2 == r2) is eligible and may lie in the cell beyond the ball's box"""
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    ef.setQueryCell(cell)
    g = np.arange(-3, 4).astype(np.float32) * F(cell)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    S = np.zeros((len(P), 12), np.float32)
    S[:, :3] = P
    S[:, 3] = 12.0
    S[:, 8:11] = 0.0, 0.6, 0.8
    ef.uploadMap(S)
    Q = [P]
    for md in (cell, 2 * cell):
        for ax in range(3):
            for sgn in (-1.0, 1.0):
                off = np.zeros(3, np.float32)
                off[ax] = sgn * F(md)
                for nudge in (0, -1, 1):
                    q = P + off
                    if nudge:
                        q[:, ax] = np.nextafter(q[:, ax], F(nudge) * F(np.inf))
                    Q.append(q)
    Q = np.concatenate(Q).astype(np.float32)
    for md in (cell, 2 * cell, float(np.nextafter(F(cell), F(0)))):
        row, _, _ = check_nearest(ef, Q, S, md, -1.0, f"cell {cell} max_dist {md}")
        rows, d2, cnt = ef.queryKnn(Q, 8, md)
        er, ed, _, ec = brute(Q, S, md, -1.0, k=8)
        assert_bits_equal(cnt, ec, "count")
        assert_bits_equal(rows, er, "knn rows")
        assert_bits_equal(d2, ed, "knn dist2")
        assert (row != MISS).sum() > len(P)
    ef.close()


@pytest.fixture(scope="module")
def live(seq):
    """20 frames of the box sequence.  The confidence threshold is 2 (as the suite's other short runs set it): at the default of 10 no surfel of
    so short a run is stable yet, and the stable-only queries and the accuracy tool would have nothing to find."""
    from elasticfusion_amd import api
    ef = api.ElasticFusion(confidence=2.0)
    ef.setSurfelIds(True)
    for k in range(20):
        rgb, depth, _ = seq.frame(k)
        ef.processFrame(rgb, depth, k)
    yield ef
    ef.close()


def test_live_map_and_stale_index(live, seq):
    ef = live
    rng = np.random.default_rng(5)
    pick = None
    for k in (20, 21):
        S = ef.downloadMap()
        assert len(S) > 100000
        if pick is None:
            pick = rng.integers(0, len(S), 4096)
            pts = (S[pick, :3].astype(np.float64) + rng.normal(0, 0.002, (4096, 3))).astype(np.float32)
        row, _, _ = check_nearest(ef, pts, S, 0.02, -1.0, f"after {k} frames, every surfel")
        rs, _, _ = check_nearest(ef, pts, S, 0.02, float(ef.cfg.confidence), f"after {k} frames, stable surfels")
        print("after", k, "frames:", len(S), "surfels,", int((S[:, 3] > F(ef.cfg.confidence)).sum()), "stable; hits", int((row != MISS).sum()),
              "stable hits", int((rs != MISS).sum()))
        assert (rs != MISS).any() and (rs != row).any()
        assert (row != MISS).sum() > 4000
        r2, _, _, ids = ef.queryNearest(pts, 0.02, -1.0, ids=True)
        assert_bits_equal(r2, row, "rows with ids")
        all_ids = ef.surfelIds()
        hit = row != MISS
        assert_bits_equal(ids[hit], all_ids[row[hit]], "ids")
        assert (ids[~hit] == 0).all() and (ids[hit] > 0).all()
        if k == 20:
            rgb, depth, _ = seq.frame(20)
            ef.processFrame(rgb, depth, 20)   # the index built above is now stale


def _run_sequence(frames, with_queries):
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(-2, 2, (1024, 3)), [[np.nan, 0, 0]]]).astype(np.float32)
    n = len(pts)
    dpts = api.DevBuf.from_array(pts)
    drow, dd2, dpl, dcnt = api.DevBuf(n * 8 * 4), api.DevBuf(n * 8 * 4), api.DevBuf(n * 4), api.DevBuf(n * 4)
    hits = 0
    for k, (rgb, depth, _) in enumerate(frames):
        ef.processFrame(rgb, depth, k)
        if with_queries and k + 1 < len(frames):
            ef.queryNearestDevice(dpts.p, n, 0.05, -1.0, row=drow.p, dist2=dd2.p, plane=dpl.p)   # enqueued behind the frame
            ef.queryKnnDevice(dpts.p, n, 8, 0.05, float(ef.cfg.confidence), rows=drow.p, dist2=dd2.p, count=dcnt.p)
            if k % 3 == 0:
                hits += int((ef.queryNearest(pts, 0.05)[0] != MISS).sum())
                ef.queryKnn(pts, 4, 0.05)
    ef.synchronize()
    res = dict(traj=ef.trajectory()[0], pose=ef.get_T_wc(), map=ef.downloadMap(), count=ef.lastCount(), hits=hits)
    ef.close()
    return res


def test_queries_change_nothing(seq):
    frames = [seq.frame(k) for k in range(40)]
    a = _run_sequence(frames, False)
    b = _run_sequence(frames, True)
    assert a["count"] == b["count"] > 0
    assert_bits_equal(a["traj"].astype(np.float64).view(np.uint64), b["traj"].astype(np.float64).view(np.uint64), "trajectory")
    assert_bits_equal(a["pose"].view(np.uint64), b["pose"].view(np.uint64), "pose")
    assert_bits_equal(a["map"], b["map"], "downloadMap")
    assert b["hits"] > 0


def test_device_variants_equal_host_and_capture_is_refused(live):
    from elasticfusion_amd import api
    ef = live
    S = ef.downloadMap()
    rng = np.random.default_rng(9)
    pts = (S[rng.integers(0, len(S), 2048), :3] + rng.normal(0, 0.003, (2048, 3))).astype(np.float32)
    n = len(pts)
    thr = float(ef.cfg.confidence)
    dpts = api.DevBuf.from_array(pts)
    drow, did, dd2, dpl = (api.DevBuf(n * 4, fill=0x55) for _ in range(4))
    ef.queryNearestDevice(dpts.p, n, 0.02, thr, row=drow.p, ids=did.p, dist2=dd2.p, plane=dpl.p)
    ef.synchronize()
    row, d2, plane = ef.queryNearestRaw(pts, 0.02, thr)
    ids = ef.queryNearest(pts, 0.02, thr, ids=True)[3]
    assert (row != MISS).any()
    assert_bits_equal(drow.to_array(np.uint32, n), row, "rows")
    assert_bits_equal(did.to_array(np.uint32, n), ids, "ids")
    assert_bits_equal(dd2.to_array(np.float32, n), d2, "dist2")
    assert_bits_equal(dpl.to_array(np.float32, n), plane, "plane")
    for k in (3, 8, 16):
        krow, kd2, kcnt = api.DevBuf(n * k * 4, fill=0x55), api.DevBuf(n * k * 4, fill=0x55), api.DevBuf(n * 4, fill=0x55)
        ef.queryKnnDevice(dpts.p, n, k, 0.02, thr, rows=krow.p, dist2=kd2.p, count=kcnt.p)
        ef.synchronize()
        rows, d2k, cnt = ef.queryKnn(pts, k, 0.02, thr)
        assert_bits_equal(krow.to_array(np.uint32, (n, k)), rows, "knn rows")
        assert_bits_equal(kd2.to_array(np.float32, (n, k)), d2k, "knn dist2")
        assert_bits_equal(kcnt.to_array(np.uint32, n), cnt, "knn count")
    # NULL optional outputs
    ef.queryNearestDevice(dpts.p, n, 0.02, thr, row=drow.p)
    ef.queryKnnDevice(dpts.p, n, 4, 0.02, thr, rows=krow.p)
    ef.synchronize()
    import ctypes.util
    name = ctypes.util.find_library("amdhip64") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")
    hip = C.CDLL(name)
    s = C.c_void_p(ef.stream())
    assert hip.hipStreamBeginCapture(s, C.c_int(2)) == 0   # relaxed
    try:
        with pytest.raises(api.EFError, match="error -4"):
            ef.queryNearestDevice(dpts.p, n, 0.02, thr, row=drow.p)
        with pytest.raises(api.EFError, match="error -4"):
            ef.queryKnnDevice(dpts.p, n, 4, 0.02, thr, rows=krow.p)
        with pytest.raises(api.EFError, match="error -4"):
            ef.queryNearest(pts, 0.02)
        with pytest.raises(api.EFError, match="error -4"):
            ef.queryKnn(pts, 4, 0.02)
    finally:
        g = C.c_void_p()
        assert hip.hipStreamEndCapture(s, C.byref(g)) == 0
        if g.value:
            hip.hipGraphDestroy(g)
    ef.synchronize()
    assert_bits_equal(ef.queryNearestRaw(pts, 0.02, thr)[0], row, "usable afterwards")


def _f64_figures(points, target, ok, max_dist):
    """exhaustive float64: each point's nearest target row among ok, then the figures the tool reports"""
    T = target[:, :3].astype(np.float64)
    r2 = np.float64(F(max_dist)) ** 2
    dist, plane = [], []
    miss = 0
    for a in range(0, len(points), 16):
        q = points[a:a + 16].astype(np.float64)
        d = q[:, None, :] - T[None, :, :]
        d2 = (d * d).sum(2)
        d2[:, ~ok] = np.inf
        w = np.argmin(d2, 1)
        for i in range(len(q)):
            if d2[i, w[i]] <= r2:
                dist.append(np.sqrt(d2[i, w[i]]))
                plane.append(abs(float((d[i, w[i]] * target[w[i], 8:11].astype(np.float64)).sum())))
            else:
                miss += 1
    dist, plane = np.array(dist), np.array(plane)
    out = {"miss_share": miss / len(points), "hits": len(dist)}
    for name, v in (("dist", dist), ("plane", plane)):
        out[name + "_mean"], out[name + "_median"], out[name + "_rms"] = v.mean(), np.median(v), np.sqrt((v * v).mean())
    return out


def test_accuracy_tool_against_float64(live, seq):
    from elasticfusion_amd import accuracy, synth
    ef = live
    gt = synth.sample_surfels(seq, n=1 << 18)
    S = ef.downloadMap()
    stable = np.nonzero(S[:, 3] > F(ef.cfg.confidence))[0]
    assert len(stable) > 2048
    rng = np.random.default_rng(11)
    map_rows = np.sort(rng.choice(stable, 2048, replace=False))
    gt_rows = np.sort(rng.choice(len(gt), 2048, replace=False))
    rep = accuracy.map_accuracy(ef, gt, max_dist=0.05, map_rows=map_rows, gt_rows=gt_rows)
    print(accuracy.format_report(rep))
    want = {"accuracy": _f64_figures(S[map_rows, :3], gt, np.ones(len(gt), bool), 0.05),
            "completeness": _f64_figures(gt[gt_rows, :3], S, S[:, 3] > F(ef.cfg.confidence), 0.05)}
    for side in ("accuracy", "completeness"):
        got, exp = rep[side], want[side]
        assert got["points"] == 2048 and got["hits"] == exp["hits"] > 0, (side, got, exp)
        assert got["miss_share"] == pytest.approx(exp["miss_share"], abs=1e-12)
        for key in ("dist_mean", "dist_median", "dist_rms", "plane_mean", "plane_median", "plane_rms"):
            print(side, key, got[key], exp[key])
            assert abs(got[key] - exp[key]) <= 1e-6 * abs(exp[key]), (side, key, got[key], exp[key])
