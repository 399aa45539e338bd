"""Connected components of the map on the device (ef_map_components / ef_map_components_select / ef_map_remove_components, include/ef_hip.h;
kernels in elasticfusion_amd/csrc/ef_components.inc).

The operation is restated in numpy from the header alone (tests/componentref.py: a brute-force f32 distance matrix and a sequential
union-find).  Every output is an integer and is compared EXACTLY: labels, sizes, every field of the result, the row lists and the map a
removal leaves.  The scenes (tests/componentscenes.py) are hand-built; tests/test_components_host.py shows on the CPU that they contain every
edge they claim.  result["status"] == 0 (no loop reached its cap) is part of every comparison of a result.
"""
import ctypes as C

import numpy as np
import pytest

import componentref as cref
import componentscenes as sc
from queryref import assert_bits_equal
from test_gpu_select import refused, sixteen, state_of   # noqa: F401  (sixteen is a fixture)

pytestmark = pytest.mark.gpu

F = np.float32
NONE = cref.NONE


def check(ef, S, what, among=None, among_mask=None, pairs=None, **kw):
    """labels, sizes, the result and both lists of one parameter set against the reference; returns the reference's dict"""
    want = cref.components(S, among=among_mask, pairs=pairs, **{k: v for k, v in kw.items() if k != "cell"})
    label, size, res = ef.components(among=among, result=True, **kw)
    bad = np.nonzero(label != want["label"])[0]
    assert len(bad) == 0, (what, "label", bad[:10], label[bad[:10]], want["label"][bad[:10]])
    assert np.array_equal(size, want["size"]), (what, "size", np.nonzero(size != want["size"])[0][:10])
    assert res == want["result"], (what, res, want["result"])
    for which, key in ((cref.REJECTED, "rejected"), (cref.ACCEPTED, "accepted")):
        rows, total, res = ef.componentSelect(among=among, what=which, count=True, result=True, **kw)
        assert total == len(want[key]) and np.array_equal(rows, want[key]), (what, key, total, len(want[key]))
        assert res == want["result"], (what, key, res, want["result"])
    return want


def context_with(S):
    from elasticfusion_amd import api
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    return ef


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1, 2: chains and the sheet
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ("ascending", "descending", "shuffled"))
def test_a_chain_is_one_component_labelled_by_its_smallest_row(order):
    S, _ = sc.chain(order)
    ef = context_with(S)
    try:
        label, size, res = ef.components(radius=sc.R, cell=sc.R, result=True)
        assert (label == 0).all() and (size == sc.N_CHAIN).all()
        assert res == dict(nodes=sc.N_CHAIN, components=1, largest=sc.N_CHAIN, rejected_rows=0, rejected_components=0, count_after=sc.N_CHAIN, status=0)
        check(ef, S, f"chain {order}", radius=sc.R, cell=sc.R, min_size=1)
        # a radius just below the spacing: 3000 components of one
        label, size = ef.components(radius=0.89 * sc.R, cell=sc.R)
        assert np.array_equal(label, np.arange(sc.N_CHAIN)) and (size == 1).all()
    finally:
        ef.close()


def test_the_sheet_is_one_component_every_time():
    S = sc.sheet()
    n = len(S)
    seen = []
    ef = context_with(S)
    try:
        for _ in range(2):
            seen.append(ef.components(radius=sc.R, cell=sc.R, result=True))
    finally:
        ef.close()
    ef = context_with(S)
    try:
        seen.append(ef.components(radius=sc.R, cell=sc.R, result=True))
    finally:
        ef.close()
    for label, size, res in seen:
        assert (label == 0).all() and (size == n).all()
        assert res == dict(nodes=n, components=1, largest=n, rejected_rows=0, rejected_components=0, count_after=n, status=0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3, 4, 5: threshold edges, rows that are no nodes, the index's edges
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge():
    S, marks = sc.edge_scene()
    ef = context_with(S)
    thr = float(ef.getConfidenceThreshold())
    assert sc.CONF_LOW < thr < sc.CONF_HIGH
    yield dict(ef=ef, S=S, m=marks, thr=thr, want={})
    ef.close()


@pytest.mark.parametrize("cell", (sc.R_EDGE, sc.R_EDGE / 16), ids=("cell=r", "cell=r/16"))
def test_the_edge_scene_equals_the_reference_exactly(edge, cell):
    ef, S, m = edge["ef"], edge["S"], edge["m"]
    want = check(ef, S, f"edge scene, cell {cell}", radius=sc.R_EDGE, cell=cell, min_size=5, max_size=6)
    label, size = want["label"], want["size"]
    # (what the host test shows of the reference, here for the record: the device equals it)
    a, b = m["at_r"]
    assert label[a] == label[b] == min(a, b)
    a, b = m["beyond_r"]
    assert label[a] == a and label[b] == b
    a, b = m["coincident"]
    assert label[a] == label[b] == min(a, b) and size[a] == 2
    assert label[m["lone"][0]] == m["lone"][0] and size[m["lone"][0]] == 1
    assert (label[m["bad"]] == NONE).all() and (size[m["bad"]] == 0).all()
    ga, gb = m["collide"]
    assert (label[ga] == ga.min()).all() and (label[gb] == gb.min()).all() and ga.min() != gb.min()
    assert ef.lastCount() == len(S)
    assert_bits_equal(ef.downloadMap(), S, "the calls change nothing")


def test_a_surfel_that_is_no_node_does_not_bridge(edge):
    from elasticfusion_amd import api
    ef, S, m = edge["ef"], edge["S"], edge["m"]
    left, bridge, right = m["bridge_among"]
    box = sc.bridge_box(S, m)
    for tests, nodes in ((api.SEL_BOX | api.SEL_INVERT, None), (api.SEL_BOX, 1)):
        sel = ef.mapSelection(tests=tests, **box)
        mask = np.zeros(len(S), bool)
        mask[ef.selectSurfels(sel)] = True
        want = check(ef, S, f"among tests={tests:#x}", among=sel, among_mask=mask, radius=sc.R_EDGE, cell=sc.R_EDGE, min_size=2)
        if nodes is None:
            assert want["label"][bridge[0]] == NONE and want["label"][left].tolist() == [left.min()] * 2
            assert want["label"][right].tolist() == [right.min()] * 2 and left.min() != right.min()
        else:
            assert want["result"]["nodes"] == nodes and want["label"][bridge[0]] == bridge[0]
    left, bridge, right = m["bridge_conf"]
    want = check(ef, S, "min_conf", radius=sc.R_EDGE, cell=sc.R_EDGE, min_conf=edge["thr"], min_size=2)
    assert want["label"][bridge[0]] == NONE and want["label"][left].tolist() == [left.min()] * 2 and want["label"][right].tolist() == [right.min()] * 2
    assert want["result"]["nodes"] < len(S) - len(m["bad"]) - 50
    check(ef, S, "min_conf among the inverted box", among=dict(tests=api.SEL_BOX | api.SEL_INVERT, **box),
          among_mask=~((S[:, :3] >= F(box["box_min"])) & (S[:, :3] <= F(box["box_max"]))).all(1), radius=sc.R_EDGE, cell=sc.R_EDGE / 2,
          min_conf=edge["thr"])


@pytest.mark.parametrize("n", sc.SIZES)
def test_sizes_around_the_launch_and_bucket_steps(n):
    S = sc.cloud(n, seed=100 + n)
    ef = context_with(S) if n else None
    try:
        if not n:
            from elasticfusion_amd import api
            ef = api.ElasticFusion()
        want = check(ef, S, f"{n} rows", radius=sc.R_CLOUD, cell=sc.R_CLOUD, min_size=3)
        if n >= 64:
            assert 1 < want["result"]["components"] < n and want["result"]["largest"] > 1
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6: the random cloud
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    S = sc.cloud(sc.N_CLOUD, seed=21)
    node = cref.nodes(S)
    pairs = cref.edges(S, node, sc.R_CLOUD)
    ef = context_with(S)
    yield dict(ef=ef, S=S, pairs=pairs)
    ef.close()


def test_the_random_cloud_equals_the_reference_exactly(big):
    ef, S = big["ef"], big["S"]
    want = check(ef, S, "cloud", pairs=big["pairs"], radius=sc.R_CLOUD, cell=sc.R_CLOUD)
    res = want["result"]
    print("cloud:", res)
    assert res["largest"] > 1000 and res["components"] > 500 and 0 < res["rejected_rows"] < len(S)
    check(ef, S, "cloud, cell = 2 r, an upper bound", pairs=big["pairs"], radius=sc.R_CLOUD, cell=2 * sc.R_CLOUD, min_size=2, max_size=1000)


def test_permuting_the_rows_permutes_the_partition(big):
    S = big["S"]
    label = big["ef"].components(radius=sc.R_CLOUD, cell=sc.R_CLOUD)[0]
    perm = np.random.default_rng(5).permutation(len(S))          # row i of S is row perm[i] of T
    T = np.empty_like(S)
    T[perm] = S
    ef = context_with(T)
    try:
        label_t, size_t, res_t = ef.components(radius=sc.R_CLOUD, cell=sc.R_CLOUD, result=True)
    finally:
        ef.close()
    assert cref.same_partition(label, label_t, perm)
    # canonical: every label is the smallest row of its set in T's own numbering
    low = np.full(len(T), len(T), np.int64)
    np.minimum.at(low, label_t.astype(np.int64), np.arange(len(T)))
    assert np.array_equal(low[label_t.astype(np.int64)], label_t) and res_t["status"] == 0
    assert np.array_equal(np.sort(size_t), np.sort(big["ef"].components(radius=sc.R_CLOUD, cell=sc.R_CLOUD)[1]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7: select
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_sizes_at_the_bounds_are_kept(edge):
    ef, S, m = edge["ef"], edge["S"], edge["m"]
    kw = dict(radius=sc.R_EDGE, cell=sc.R_EDGE, min_size=5, max_size=6)
    rej = ef.componentSelect(what=cref.REJECTED, **kw)
    acc = ef.componentSelect(what=cref.ACCEPTED, **kw)
    c = m["clumps"]
    assert np.isin(c[3], rej).all() and np.isin(c[7], rej).all()                 # below min_size, max_size + 1
    assert np.isin(c[5], acc).all() and np.isin(c[6], acc).all()                 # exactly min_size, exactly max_size
    label, size = ef.components(**kw)
    nodes = np.nonzero(label != NONE)[0]
    assert len(np.intersect1d(rej, acc)) == 0 and np.array_equal(np.union1d(rej, acc), nodes)
    assert not np.isin(m["bad"], np.concatenate([rej, acc])).any()


def test_list_conventions(edge):
    from elasticfusion_amd import api
    ef = edge["ef"]
    kw = dict(radius=sc.R_EDGE, cell=sc.R_EDGE, min_size=5)
    full, total = ef.componentSelect(count=True, **kw)
    assert total == len(full) > 20 and (np.diff(full.astype(np.int64)) > 0).all()
    none, t0 = ef.componentSelect(max_rows=0, count=True, **kw)                      # NULL rows with max_rows 0
    assert len(none) == 0 and t0 == total
    prm = ef.componentParams(**kw)
    rows = np.full(16, 0xABCD1234, np.uint32)
    cnt = C.c_uint32(0)
    api._chk(api.lib().ef_map_components_select(ef.h, C.byref(prm), None, cref.REJECTED, api._ptr(rows), 7, C.byref(cnt), None), ef.h)
    assert cnt.value == total and np.array_equal(rows[:7], full[:7]) and (rows[7:] == 0xABCD1234).all()
    rows[:] = 0xABCD1234
    api._chk(api.lib().ef_map_components_select(ef.h, C.byref(prm), None, cref.REJECTED, api._ptr(rows), 16, C.byref(cnt), None), ef.h)
    assert np.array_equal(rows, full[:16])
    n = ef.lastCount()
    lab = np.full(n + 3, 0x5A5A5A5A, np.uint32)                                    # the labels: min(max_rows, map count) entries
    api._chk(api.lib().ef_map_components(ef.h, C.byref(prm), None, api._ptr(lab), None, 100, None), ef.h)
    assert (lab[100:] == 0x5A5A5A5A).all() and (lab[:100] != 0x5A5A5A5A).all()
    api._chk(api.lib().ef_map_components(ef.h, C.byref(prm), None, api._ptr(lab), None, len(lab), None), ef.h)
    assert (lab[n:] == 0x5A5A5A5A).all() and np.array_equal(lab[:n], ef.components(prm)[0])
    api._chk(api.lib().ef_map_components(ef.h, C.byref(prm), None, None, None, 0, None), ef.h)      # nothing asked for


def test_device_variants_equal_the_host_variants(edge):
    from elasticfusion_amd import api
    ef = edge["ef"]
    n = ef.lastCount()
    for kw in (dict(radius=sc.R_EDGE, cell=sc.R_EDGE, min_size=5, max_size=6), dict(radius=sc.R_EDGE, cell=sc.R_EDGE / 2, min_size=2, min_conf=edge["thr"])):
        prm = ef.componentParams(**kw)
        label, size, res = ef.components(prm, result=True)
        nres = C.sizeof(api.ef_component_result)
        for what in (cref.REJECTED, cref.ACCEPTED):
            rows, total = ef.componentSelect(prm, what=what, count=True)
            d_rows, d_cnt, d_res = api.DevBuf(n * 4, fill=0xEE), api.DevBuf(16), api.DevBuf(nres)
            ef.componentSelectDevice(prm, None, what, d_rows.p, n, d_cnt.p, d_res.p)
            ef.synchronize()
            assert int(d_cnt.to_array(np.uint32, 1)[0]) == total
            got = d_rows.to_array(np.uint32, n)
            assert np.array_equal(got[:total], rows) and (got[total:] == 0xEEEEEEEE).all()
            raw = d_res.to_array(np.uint8, nres).tobytes()
            assert ef._componentResult(api.ef_component_result.from_buffer_copy(raw)) == res
            ef.componentSelectDevice(prm, None, what, None, 0, d_cnt.p)                    # no list, no result
            ef.synchronize()
            assert int(d_cnt.to_array(np.uint32, 1)[0]) == total
        d_label, d_size, d_res = api.DevBuf((n + 2) * 4, fill=0xEE), api.DevBuf((n + 2) * 4, fill=0xEE), api.DevBuf(nres)
        ef.componentsDevice(prm, None, d_label.p, d_size.p, n + 2, d_res.p)
        ef.synchronize()
        gl, gs = d_label.to_array(np.uint32, n + 2), d_size.to_array(np.uint32, n + 2)
        assert np.array_equal(gl[:n], label) and np.array_equal(gs[:n], size) and (gl[n:] == 0xEEEEEEEE).all() and (gs[n:] == 0xEEEEEEEE).all()
        raw = d_res.to_array(np.uint8, nres).tobytes()
        assert ef._componentResult(api.ef_component_result.from_buffer_copy(raw)) == res and res["status"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# 8: removal
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_removal_equals_erasing_the_list(frames):
    from elasticfusion_amd import api
    a, b = api.ElasticFusion(), api.ElasticFusion()
    try:
        for ef in (a, b):
            ef.setSurfelIds(True)
            ef.enableLabels(3)
            for k in range(3):
                ef.processFrame(frames[k][0], frames[k][1], k)
        n = a.lastCount()
        kw = dict(radius=0.006, cell=0.006, min_size=200)
        rows, total, res = a.componentSelect(count=True, result=True, **kw)
        print("surfels", n, "rejected", total, res)
        assert 0 < total < n and res["status"] == 0, (total, n, res)
        got = a.removeComponents(**kw)
        assert b.eraseRows(rows) == total
        want = dict(res, count_after=n - total)
        assert got == want and a.lastCount() == b.lastCount() == n - total, (got, want)
        (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
        assert_bits_equal(ma, mb, "the map after the removal")
        assert a.getTick() == b.getTick()
        assert np.array_equal(a.surfelIds(), b.surfelIds())
        (ia, pa), (ib, pb) = a.labels(), b.labels()
        assert np.array_equal(ia, ib)
        assert_bits_equal(pa, pb, "the labels after the removal")
        # idempotent: every component that stayed keeps its nodes and its verdict
        again = a.removeComponents(**kw)
        assert again["rejected_rows"] == 0 and again["rejected_components"] == 0 and again["count_after"] == n - total
        assert again["nodes"] == res["nodes"] - total and again["components"] == res["components"] - res["rejected_components"]
        assert_bits_equal(a.downloadMap(), mb, "a second removal changes nothing")
        assert a.getTick() == b.getTick()
        for ef in (a, b):
            ef.processFrame(frames[3][0], frames[3][1], 3)
        (qa, sa, ma), (qb, sb, mb) = state_of(a), state_of(b)
        assert np.array_equal(qa.view(np.uint64), qb.view(np.uint64)) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
        assert_bits_equal(ma, mb, "the map after the following frame")
        assert len(ma) > n - total
    finally:
        a.close()
        b.close()


def test_a_loop_closing_context_refuses_the_removal_only():
    from elasticfusion_amd import api
    S, _ = sc.edge_scene()
    ef = api.ElasticFusion(closeLoops=True)
    try:
        ef.uploadMap(S)
        assert "close_loops" in refused(lambda: ef.removeComponents(radius=sc.R_EDGE, cell=sc.R_EDGE), -4)      # EF_ESTATE
        assert ef.lastCount() == len(S)
        assert_bits_equal(ef.downloadMap(), S, "a refused removal")
        check(ef, S, "on a loop-closing context", radius=sc.R_EDGE, cell=sc.R_EDGE, min_size=4)
        refused(lambda: ef.componentSelect(what=2), -1)                                                         # EF_EINVAL
        refused(lambda: ef.componentSelect(radius=1.0, cell=0.01), -1)
        refused(lambda: ef.components(radius=float("nan")), -1)
    finally:
        ef.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 9: end to end
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_injected_blobs_go_by_size_and_the_surface_stays(sixteen):
    from elasticfusion_amd import accuracy, api
    ef = api.ElasticFusion(confidence=2.0)
    try:
        for k in range(16):
            ef.processFrame(sixteen[k][0], sixteen[k][1], k * 33333)
        M = ef.downloadMap()
        n = len(M)
        rng = np.random.default_rng(3)
        blobs, used = [], []
        for count, seed in ((30, 1), (200, 2), (2000, 3)):
            for row in rng.choice(n, 200, replace=False):
                half = 0.012 * max(1.0, (count / 30.0) ** (1 / 3))
                centre = M[row, :3].astype(np.float64) + (0.10 + 1.8 * half) * M[row, 8:11].astype(np.float64)   # the blob's nearest corner 10 cm off
                pts = sc.blob(centre, count, seed)
                if any(np.linalg.norm(centre - c) < 0.3 for c in used):
                    continue
                if (ef.queryNearestRaw(pts.astype(F), 0.06, -1.0)[0] == 0xFFFFFFFF).all():       # nothing of the map within two radii
                    blobs.append(sc.of_points(pts))
                    used.append(centre)
                    break
        assert [len(b) for b in blobs] == [30, 200, 2000]
        both = np.concatenate([M] + blobs)
        ef.uploadMap(both)
        label, size, res = ef.components(min_size=500, result=True)
        assert res["status"] == 0
        at = np.cumsum([n, 30, 200, 2000])
        for lo, hi, count in ((at[0], at[1], 30), (at[1], at[2], 200), (at[2], at[3], 2000)):
            assert (label[lo:hi] == lo).all() and (size[lo:hi] == count).all(), (count, np.unique(size[lo:hi]))
        rows, total = ef.componentSelect(min_size=500, count=True)
        flagged = np.zeros(len(both), bool)
        flagged[rows] = True
        share = flagged[:n].mean()
        main = int(np.bincount(label[:n][label[:n] != NONE]).argmax())
        print(f"map {n} + blobs of 30 / 200 / 2000: {res}; removed share of the original surfels {share:.4f}; the surface's largest component "
              f"{int(size[main])} rows")
        assert flagged[at[0]:at[2]].all() and not flagged[at[2]:].any(), "the two small blobs go, the blob of 2000 stays"
        assert not flagged[main] and size[main] == res["largest"] and share < 0.5
        segs = accuracy.segments(ef, min_size=500)
        assert [len(s) for s in segs] == sorted((len(s) for s in segs), reverse=True) and len(segs[0]) == res["largest"]
        assert any(len(s) == 2000 and np.array_equal(s.view(np.uint32), blobs[2].view(np.uint32)) for s in segs)
        big = accuracy.largest_component(ef)
        assert_bits_equal(big, both[label == main], "largest_component gathers the surface's largest component")
        assert ef.lastCount() == len(both)
        got = ef.removeComponents(min_size=500)
        assert got["rejected_rows"] == total and got["count_after"] == len(both) - total
        assert_bits_equal(ef.downloadMap(), both[~flagged], "the removal")
    finally:
        ef.close()
