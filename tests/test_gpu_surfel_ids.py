"""Stable surfel IDs (ef_set_surfel_ids / ef_get_surfel_ids, include/ef_hip.h; kernels in elasticfusion_amd/csrc/ef_labels.inc): the ID is
the raw uint32 bit pattern of float 5 of each downloaded surfel, the colour stream's unused lane.  IDs must change no result of a frame,
follow their surfel through fusion, clean and deformation, and survive a download / upload round trip."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = 40
OTHER = [i for i in range(12) if i != 5]


def ids_of(m):
    return np.ascontiguousarray(m[:, 5]).view(np.uint32)


@pytest.fixture(scope="module")
def frames():
    from elasticfusion_amd import synth
    seq = synth.Sequence(0xEF0001, 640, 480)
    return [seq.frame(k) for k in range(FRAMES + 2)]


@pytest.fixture(scope="module")
def runs(frames):
    """the same 40 frames with IDs on (a download after every frame) and off"""
    from elasticfusion_amd import api
    on, off = api.ElasticFusion(), api.ElasticFusion()
    on.setSurfelIds(True)
    rec = []
    for k in range(FRAMES):
        rgb, depth, _ = frames[k]
        on.processFrame(rgb, depth, k)
        off.processFrame(rgb, depth, k)
        rec.append(dict(T_on=on.get_T_wc(), T_off=off.get_T_wc(), m_on=on.downloadMap(), m_off=off.downloadMap()))
    yield on, off, rec
    on.close()
    off.close()


def test_ids_change_no_results(runs):
    _, _, rec = runs
    for k, r in enumerate(rec):
        assert np.array_equal(r["T_on"].view(np.uint64), r["T_off"].view(np.uint64)), k
        a, b = r["m_on"], r["m_off"]
        assert a.shape == b.shape, k
        assert np.array_equal(a[:, OTHER].view(np.uint32), b[:, OTHER].view(np.uint32)), k
        assert not ids_of(b).any(), k


def test_ids_follow_surfels(runs):
    _, _, rec = runs
    init_time, gone, top = {}, set(), 0
    for k, r in enumerate(rec):
        m = r["m_on"]
        ids = ids_of(m)
        assert (ids >= 1).all(), k
        assert (np.diff(ids.astype(np.int64)) > 0).all(), k
        t = np.ascontiguousarray(m[:, 6]).view(np.uint32)
        cur = set(ids.tolist())
        assert not (cur & gone), k
        old = np.array([i in init_time for i in ids.tolist()], bool)
        for i, ti in zip(ids[old].tolist(), t[old].tolist()):
            assert init_time[i] == ti, (k, i)
        new = ids[~old]
        if len(new):
            assert new.min() > top, k
            top = int(new.max())
        for i, ti in zip(new.tolist(), t[~old].tolist()):
            init_time[i] = ti
        gone |= set(init_time) - cur
    assert len(gone) > 0 and top > len(rec[-1]["m_on"])   # surfels did vanish, so the test saw IDs leave


def test_get_surfel_ids_matches_the_download(runs):
    on, _, _ = runs
    assert np.array_equal(on.surfelIds(), ids_of(on.downloadMap()))


def test_deformation_keeps_ids(frames):
    import mapops
    from elasticfusion_amd import api
    ef = api.ElasticFusion(confidence=1.0)
    ef.setSurfelIds(True)
    for k in range(8):
        rgb, depth, T = frames[k]
        if k == 6:
            before = ef.downloadMap()
            g = mapops.make_graph(dict(surf=before, tick=np.int32(ef.getTick())), n_nodes=32)
            ef.setDeformation(g)
        ef.processFrame(rgb, depth, k, in_T_wc=None if k == 0 else T)
    after = ef.downloadMap()
    ef.close()
    ib, ia = ids_of(before), ids_of(after)
    common, xb, xa = np.intersect1d(ib, ia, return_indices=True)
    assert len(common) > 0.5 * len(ib)
    # initTime travels with the ID
    assert np.array_equal(before[xb, 6].view(np.uint32), after[xa, 6].view(np.uint32))
    assert (np.diff(ia.astype(np.int64)) > 0).all()


def test_upload_keeps_ids_and_continues_above_them(runs, frames):
    from elasticfusion_amd import api
    on, _, _ = runs
    m = on.downloadMap()
    ef = api.ElasticFusion()
    ef.setSurfelIds(True)
    ef.uploadMap(m)
    assert np.array_equal(ef.surfelIds(), ids_of(m))
    ck = dict(map=m, tick=on.getTick(), qt=on.getPoseQT(), rgb=frames[FRAMES - 1][0], depth=frames[FRAMES - 1][1])
    ef.restore(ck)
    ef.processFrame(frames[FRAMES][0], frames[FRAMES][1], FRAMES)
    ids = ef.surfelIds()
    ef.close()
    old = np.isin(ids, ids_of(m))
    assert old.any() and (~old).any()
    assert ids[~old].min() > ids_of(m).max()
    assert (np.diff(ids.astype(np.int64)) > 0).all()


def test_upload_with_zero_lane_numbers_the_map(runs):
    from elasticfusion_amd import api
    on, _, _ = runs
    m = on.downloadMap()
    m[:, 5] = 0
    ef = api.ElasticFusion()
    ef.setSurfelIds(True)
    ef.uploadMap(m)
    ids = ef.surfelIds()
    ef.close()
    assert np.array_equal(ids, np.arange(1, len(m) + 1, dtype=np.uint32))


def test_upload_with_a_bad_lane_is_refused(runs):
    from elasticfusion_amd import api
    on, _, _ = runs
    m = on.downloadMap()
    lane = ids_of(m).copy()
    lane[[10, 11]] = lane[[11, 10]]
    m[:, 5] = lane.view(np.float32)
    ef = api.ElasticFusion()
    ef.setSurfelIds(True)
    ef.uploadMap(m)
    with pytest.raises(api.EFError, match="error -4"):
        ef.surfelIds()
    with pytest.raises(api.EFError, match="error -4"):
        ef.downloadMap()
    m[:, 5] = 0   # a valid upload clears it
    ef.uploadMap(m)
    assert len(ef.surfelIds()) == len(m)
    ef.close()


def test_switching_off_equals_never_on(runs):
    on, off, _ = runs
    on.setSurfelIds(False)
    a, b = on.downloadMap(), off.downloadMap()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    on.setSurfelIds(True)   # back on: numbered again, above every earlier ID
    ids = on.surfelIds()
    assert (np.diff(ids.astype(np.int64)) > 0).all() and ids.min() > 1
