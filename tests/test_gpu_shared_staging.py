"""The host-pointer entry points of the map operations share ONE device staging area per context (ef_ctx::stage; host code in
elasticfusion_amd/csrc/ef_host_render.inc, ef_host_labels.inc, ef_host_query.inc, ef_host_register.inc, ef_host_select.inc, ef_host_thin.inc,
ef_host_insert.inc and ef_host_fuse.inc).

One context, one map, and the eight families (query, render, gather / select / erase, registration, labels, thin, insert, fuse) called in one
interleaved sequence whose staging needs grow (7-point query 0.3 kB -> render 135 kB -> kNN 760 kB) and shrink again in between (gather 78 kB,
registration 10 kB, labels 61 kB / 25 kB, selection and thin lists 12 kB, the 7-point query again, 300 inserted or fused records 17 kB): every
host-pointer result must equal, bit for bit, what the same call's _dev variant writes into device buffers on the same context — both run the
same kernels on the same map, so there is no tolerance.  The one map-changing call of the first part (ef_fuse_labels) runs once; the label
renders are compared after it.  The thin lists go through the selection's "list of rows" tier.  The erase near the end stages its rows inside
erase_run and leaves a rebuilt index behind.  The insert and the fuse at the very end change the map, so each tier starts from the same
uploaded map and the maps they leave are compared too: first with IDs and labels on (the appended rows' IDs of the second tier lie exactly
their number above the first's, every other bit is equal), then with the ID lane off (every bit is equal).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NC = 3000, 5
W, H = 64, 48
VIEW = dict(width=W, height=H, fx=52.8, fy=52.8, cx=32.0, cy=24.0, drawUnstable=True)
MISS = 0xFFFFFFFF


def scene():
    """N surfels in front of the 64 x 48 view, facing it"""
    rng = np.random.default_rng(41)
    S = np.zeros((N, 12), np.float32)
    z = rng.uniform(1.0, 3.0, N)
    S[:, 0] = rng.uniform(-0.55, 0.55, N) * z
    S[:, 1] = rng.uniform(-0.42, 0.42, N) * z
    S[:, 2] = z
    S[:, 3] = rng.uniform(0, 14, N)
    S[:, 4] = rng.integers(0, 1 << 24, N)
    S[:, 6] = S[:, 7] = 1
    nrm = np.array([0, 0, -1.0]) + rng.normal(scale=0.2, size=(N, 3))
    S[:, 8:11] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    S[:, 11] = rng.uniform(0.005, 0.02, N)
    return S, rng


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def same(host, dev, what):
    assert len(host) == len(dev), what
    for k, (h, d) in enumerate(zip(host, dev)):
        h, d = np.asarray(h), np.asarray(d)
        assert h.dtype.itemsize == d.dtype.itemsize and h.shape == d.shape, (what, k, h.dtype, d.dtype, h.shape, d.shape)
        assert np.array_equal(bits(h), bits(d)), (what, k, int((bits(h) != bits(d)).sum()))


def test_interleaved_host_pointer_calls_equal_their_device_variants():
    from elasticfusion_amd import api

    S, rng = scene()
    ef = api.ElasticFusion()
    ef.uploadMap(S)
    ef.setSurfelIds(True)
    ef.enableLabels(NC)

    class Out:
        """a zeroed device buffer for an array of this shape and type"""
        def __init__(self, shape, dtype):
            self.shape, self.dtype = shape, np.dtype(dtype)
            self.buf = api.DevBuf(int(np.prod(shape)) * self.dtype.itemsize)
            self.p = self.buf.p

    dev, out = api.DevBuf.from_array, Out

    def back(*ts):
        ef.synchronize()
        return tuple(t.buf.to_array(t.dtype, t.shape) for t in ts)

    def nearest(pts):
        n = len(pts)
        row, dist, plane, ids = ef.queryNearest(pts, 0.05, ids=True)
        p, r, i, d2, pl = dev(pts), out(n, np.uint32), out(n, np.uint32), out(n, np.float32), out(n, np.float32)
        ef.queryNearestDevice(p.p, n, 0.05, row=r.p, ids=i.p, dist2=d2.p, plane=pl.p)
        r, i, d2, pl = back(r, i, d2, pl)
        same((row, dist, plane, ids), (r, np.sqrt(d2), pl, i), "ef_query_nearest")
        return row, dist, plane, ids

    def render():
        names = ("rgba", "depth", "vertex", "normal", "index")
        host = ef.renderPointCloud(outputs=names, **VIEW)
        t = dict(rgba=out((H, W, 4), np.uint8), depth=out((H, W), np.float32), vertex=out((H, W, 4), np.float32),
                 normal=out((H, W, 4), np.float32), index=out((H, W), np.uint32))
        ef.renderPointCloudDevice(ef.renderParams(**VIEW), **{k: v.p for k, v in t.items()})
        same([host[k] for k in names], back(*[t[k] for k in names]), "ef_render_model")
        return host

    def gather(rows):
        host = ef.gatherSurfels(rows)
        r, o = dev(rows), out((len(rows), 12), np.float32)
        ef.gatherSurfelsDevice(r.p, len(rows), o.p)
        same((host,), back(o), "ef_map_gather")
        return host

    def register_step(pts, nrm):
        n = len(pts)
        kw = dict(max_dist=0.05, min_conf=-1.0)
        host = ef.registerStep(pts, nrm, pairs=True, **kw)
        p, q, r, pl = dev(pts), dev(nrm), out(n, np.uint32), out(n, np.float32)
        d = ef.registerStepDevice(p.p, n, normals_dev=q.p, row=r.p, plane=pl.p, **kw)
        r, pl = back(r, pl)
        same((host["A"], host["b"], np.float64(host["e"]), host["row"], host["plane"]), (d["A"], d["b"], np.float64(d["e"]), r, pl),
             "ef_register_step")
        assert (host["pairs"], host["points"]) == (d["pairs"], d["points"])
        return host

    def render_labels():
        label, prob = ef.renderLabels(**VIEW)
        tl, tp = out((H, W), np.uint32), out((H, W), np.float32)
        ef.renderLabelsDevice(ef.renderParams(**VIEW), label=tl.p, prob=tp.p)
        same((label, prob), back(tl, tp), "ef_render_labels")
        return label, prob

    def select(sel):
        rows, total = ef.selectSurfels(sel, count=True)
        tr, tc = out(N, np.uint32), out(4, np.uint32)
        ef.selectSurfelsDevice(sel, tr.p, N, tc.p)
        r, c = back(tr, tc)
        assert total == int(c[0]) and total == len(rows)
        same((rows,), (r[:total],), "ef_map_select")
        return rows

    def knn(pts, k):
        n = len(pts)
        host = ef.queryKnn(pts, k, 0.1)
        p, r, d2, c = dev(pts), out((n, k), np.uint32), out((n, k), np.float32), out(n, np.uint32)
        ef.queryKnnDevice(p.p, n, k, 0.1, rows=r.p, dist2=d2.p, count=c.p)
        same(host, back(r, d2, c), "ef_query_knn")
        return host

    def thin_select(params, among, representatives):
        rows, total = ef.thinSelect(params, among, representatives, count=True)
        tr, tc = out(N, np.uint32), out(4, np.uint32)
        ef.thinSelectDevice(params, among, representatives, tr.p, N, tc.p)
        r, c = back(tr, tc)
        assert total == int(c[0]) and total == len(rows)
        same((rows,), (r[:total],), "ef_map_thin_select")
        return rows

    def append_pair(call, start, rec, what, ids_on=False, **kw):
        """the host tier and the DevBuf tier of insertSurfels / fuseSurfels, each on the freshly uploaded map `start`"""
        got = []
        for records in (rec, api.DevBuf.from_array(rec)):
            ef.uploadMap(start)
            res, *arrays = call(records, rows=True, **kw)
            got.append((list(res), np.array(list(res.values()), np.uint32), *arrays, ef.downloadMap()))
        assert got[0][0] == got[1][0], what
        if ids_on:
            # The ID counter of a context only rises: the download numbers the k appended rows of the first tier c .. c + k - 1, above every ID
            # of `start`, and those of the second tier c + k .. c + 2 k - 1.  That is checked exactly and the lane of the appended rows is
            # then cleared in both maps, so that same() below compares every other bit of them, the old rows' IDs included.
            maps = [g[-1].copy() for g in got]
            ids = [m[len(start):, 5].copy().view(np.uint32) for m in maps]
            k = np.uint32(len(ids[0]))
            assert k > 0 and ids[0][0] > start[:, 5].copy().view(np.uint32).max(), what
            assert np.array_equal(ids[0], ids[0][0] + np.arange(k, dtype=np.uint32)) and np.array_equal(ids[1], ids[0] + k), what
            for m in maps:
                m[len(start):, 5] = 0
            got = [g[:-1] + (m,) for g, m in zip(got, maps)]
        same(got[0][1:], got[1][1:], what)
        return got[0][1:]

    pts7 = (S[::400][:7, :3] + np.float32(0.003)).astype(np.float32)
    first7 = nearest(pts7)                                                  # 1
    assert (first7[0] != MISS).all() and (first7[3] != 0).all()            # (each point has its surfel 5 mm away; IDs are numbered)
    index = render()["index"]                                               # 2: the staging grows
    drawn = index != MISS
    assert drawn.sum() > W * H // 4
    rows = rng.integers(0, N, 1500).astype(np.uint32)
    g = gather(rows)                                                        # 3
    same((g,), (ef.downloadMap()[rows],), "the gathered rows against downloadMap()[rows]")
    pick = rng.integers(0, N, 300)
    reg = register_step((S[pick, :3] + rng.normal(scale=0.004, size=(300, 3))).astype(np.float32), S[pick, 8:11].copy())   # 4
    assert reg["points"] == 300 and reg["pairs"] > 150
    # 5: the one map-changing call.  The same class vector at every pixel: from the uniform prior (class 0 on top) a surfel ends with class 1
    # on top when it was observed, that is when the index image shows it at the pixel its centre falls into (the pose is the identity).
    vec = np.array([0.1, 0.5, 0.2, 0.1, 0.1], np.float32)
    ef.fuseLabels(np.broadcast_to(vec[:, None, None], (NC, H, W)).copy(), **VIEW)
    label, prob = render_labels()                                           # 6
    F = np.float32
    rs = index[drawn]
    u = np.floor((F(VIEW["fx"]) * S[rs, 0]) / S[rs, 2] + F(VIEW["cx"]))
    v = np.floor((F(VIEW["fy"]) * S[rs, 1]) / S[rs, 2] + F(VIEW["cy"]))
    ys, xs = np.nonzero(drawn)
    observed = np.isin(rs, rs[(u == xs) & (v == ys)])
    assert observed.sum() > drawn.sum() // 2
    assert np.array_equal(label[drawn], observed.astype(np.int32)) and (label[~drawn] == -1).all()
    sel = ef.mapSelection(tests=api.SEL_CONF | api.SEL_BOX, conf_min=3.0, conf_max=9.0, box_max=[0.2, np.inf, np.inf])
    chosen = select(sel)                                                    # 7
    want = np.nonzero((S[:, 3] >= 3.0) & (S[:, 3] <= 9.0) & (S[:, 0] <= np.float32(0.2)))[0]
    assert np.array_equal(chosen, want)
    big = (S[rng.integers(0, N, 5000), :3] + rng.normal(scale=0.01, size=(5000, 3))).astype(np.float32)
    kr, kd, kc = knn(big, 16)                                               # 8: the staging grows again
    assert (kc >= 1).mean() > 0.9
    same(first7, nearest(pts7), "the 7-point query after the larger calls") # 9

    # 10: the thin's lists, through the tier ef_map_select uses.  A 0.25 m cell holds several surfels; every participant is in one list
    tp = ef.thinParams(cell=0.25)
    for among, part in ((None, np.arange(N)), (sel, want)):
        removed, reps = thin_select(tp, among, False), thin_select(tp, among, True)
        assert len(removed) > len(part) // 4 and len(reps) > 50
        assert np.array_equal(np.sort(np.concatenate([removed, reps])), part)

    # the erase stages its rows inside erase_run; the queries after it run on a rebuilt index
    before = ef.downloadMap()
    gone = np.setdiff1d(np.array([3, 17, 500, 1234, 2222, N - 1], np.uint32), first7[0])[:4]   # (never one of the 7 nearest)
    gone = np.concatenate([gone[::-1], gone[:1]])                                                  # any order, one of them twice
    assert ef.eraseRows(gone) == 4
    after = ef.downloadMap()
    same((after,), (np.delete(before, gone, axis=0),), "the map after ef_map_erase_rows")
    assert len(after) == N - 4
    last7 = nearest(pts7)
    keep = np.delete(np.arange(N), gone)
    moved = np.searchsorted(keep, first7[0])            # a kept row's place in the compacted map
    same(last7[1:], first7[1:], "distances, planes and IDs of the 7 nearest (none of them erased)")
    assert np.array_equal(last7[0], moved.astype(np.uint32))

    # The insert and the fuse: 300 records made from the map.  100 jittered by under min_separation (0.01 m), a fifth of them aimed at a row
    # another record aims at; 100 lifted 5 cm; 34 non-finite, 33 jittered ones whose confidence cannot compete, 33 repeated records.  First
    # with IDs and labels on (the ID numbering and the label bound of the edit frame), then with the ID lane off, where the two tiers' maps
    # are equal in every bit.
    start = ef.downloadMap()
    M = len(start)
    assert M == N - 4
    pick = rng.integers(0, M, 80)
    near = start[np.concatenate([pick, pick[:20]])].copy()
    near[:, :3] += rng.uniform(-0.003, 0.003, (100, 3)).astype(np.float32)
    near[:, 3] = rng.uniform(0.5, 5.0, 100)
    lifted = start[rng.integers(0, M, 100)].copy()
    lifted[:, 2] += np.float32(0.05)
    broken = start[rng.integers(0, M, 34)].copy()
    broken[np.arange(34), np.arange(34) % 3] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(34) % 3]
    weightless = near[:33].copy()
    weightless[:, 3] = np.array([0.0, -1.0, np.inf, np.nan], np.float32)[np.arange(33) % 4]
    rec = np.ascontiguousarray(np.concatenate([near, lifted, broken, weightless, near[40:73]]), np.float32)
    assert rec.shape == (300, 12)
    T = np.eye(4)
    T[0, 3] = 0.001
    append_pair(ef.insertSurfels, start, rec, "ef_map_insert, IDs on", ids_on=True)
    append_pair(ef.fuseSurfels, start, rec, "ef_map_fuse, IDs on", ids_on=True, T=T)
    ef.uploadMap(start)
    ef.setSurfelIds(False)
    start = ef.downloadMap()
    assert len(start) == M
    res, new_row, match_row, left = append_pair(ef.insertSurfels, start, rec, "ef_map_insert")
    inserted, duplicates, skipped, count_after = (int(v) for v in res)
    assert inserted >= 90 and duplicates >= 150 and skipped == 34 and count_after == M + inserted == len(left)
    same((left[:M],), (start,), "the old rows after ef_map_insert")
    for append in (1, 0):
        res, new_row, match_row, outcome, left = append_pair(ef.fuseSurfels, start, rec, f"ef_map_fuse, append = {append}", T=T, append=append)
        fused, absorbed, weightless_n, novel, skipped, inserted, count_after = (int(v) for v in res)
        assert fused >= 60 and absorbed >= 30 and weightless_n >= 25 and novel >= 90 and skipped == 34
        assert inserted == (novel if append else 0) and count_after == M + inserted == len(left)
        kinds = (api.FUSE_SKIPPED, api.FUSE_WEIGHTLESS, api.FUSE_ABSORBED, api.FUSE_FUSED, api.FUSE_INSERTED if append else api.FUSE_NOVEL)
        assert sorted(set(outcome.tolist())) == sorted(kinds)
        assert (left[:M] != start).any(axis=1).sum() == fused
    ef.close()
