"""The stages behind association on hand-built edge scenes (tests/cleanscenes.py), operator tier and frame tier, bit for bit against the
oracle (NaN == NaN, surfel order included).  A scene's check() runs on the oracle's result BEFORE the device is asked.

Operator tier: k_clean_flags<false> / k_clean_scatter with a scanned row offset (tap multiplicities, every comparison of both counting
rules, the gate, the time rules with and without the taps, compaction up to the second trip of the row loop), k_associate<false> +
k_merge (the radius gate, degenerate weights, colours, normals), k_clean_deform (node counts around the collection limits, vertex
times around the node times, ties of distance, the 'seen again' test).

Frame tier: a checkpoint whose map is a scene, restored into the engine and into the oracle's Fusion, then one frame with an injected
identity pose and a flat depth image: clean_test<true> on z-buffer keys, k_associate<true>, the merge inside k_index_splat<true>, and
k_clean_scatter finding its row offset from the group sums (17 000 surfels: two whole groups and a partial one; a million: 128 groups
and the second trip of the row loop).
"""
import functools

import numpy as np
import pytest

import cleanscenes as S
import efo
from test_gpu_ops_tracking import bits_equal

pytestmark = pytest.mark.gpu

SIZE_IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}")
QT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


@pytest.fixture(scope="module")
def api():
    from elasticfusion_amd import api
    return api


@functools.lru_cache(maxsize=None)
def scenes(group, W, H):
    return getattr(S, group)(W, H)


def outputs(out):
    return out if isinstance(out, tuple) else (out,)


def rows_differing(a, b):
    if a.shape != b.shape:
        return f"shapes {a.shape} {b.shape}"
    d = (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).reshape(len(a), -1).any(axis=1)
    return np.nonzero(d)[0][:8].tolist()


def compare(api, sc):
    ref = sc.run(efo, efo.make_cam(*sc.cam))
    sc.check(ref)                                   # the scene does its job on the oracle ...
    got = sc.run(api.ops, api.ef_cam(*sc.cam))      # ... before the device is asked
    return [(str(sc), k, rows_differing(a, b)) for k, (a, b) in enumerate(zip(outputs(got), outputs(ref))) if a.shape != b.shape or not bits_equal(a, b)]


@pytest.mark.parametrize("size", S.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("group", ["tap_scenes", "comparison_scenes", "gate_scenes", "time_rule_scenes", "compaction_scenes", "window_scenes",
                                   "seen_again_scenes"])
def test_operator_scenes(api, size, group):
    bad = []
    for sc in scenes(group, *size):
        bad += compare(api, sc)
    print(f"{group}: {len(scenes(group, *size))} scenes, {len(bad)} differ")
    assert not bad, bad[:12]


@pytest.mark.parametrize("size", S.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("n", S.NODE_COUNTS)
def test_deformation_on_a_lattice_of_ties(api, size, n):
    assert not compare(api, S.lattice_scene(*size, n))


@pytest.mark.parametrize("size", S.SIZES, **SIZE_IDS)
def test_merge_scene(api, size):
    assert not compare(api, S.MergeScene(*size))


def test_million_element_compaction(api):
    """4096 x 256 + 300 out-of-view surfels: the second trip of xcd_row in k_clean_flags and k_clean_scatter; the expected map is a numpy mask"""
    sc = S.big_compaction_scene(*S.SIZES[0])
    got = sc.run(api.ops, api.ef_cam(*sc.cam))
    assert got.shape == (int(sc.mask.sum()), 12) and bits_equal(got, sc.surf[sc.mask])
    assert bits_equal(got, sc.run(efo, efo.make_cam(*sc.cam)))


# ---- frame tier ----
def engines(api, sc, maxSurfels=1 << 16):
    W, H = sc.W, sc.H
    ck = dict(map=sc.surf, tick=sc.tick, qt=QT, rgb=sc.rgb, depth=sc.depth)
    kw = dict(width=W, height=H, fx=S.FX, fy=S.FY, cx=W / 2.0, cy=H / 2.0, confidence=float(sc.conf), timeDelta=sc.timeDelta, maxSurfels=maxSurfels)
    ef, o = api.ElasticFusion(**kw), efo.Fusion(**kw)
    ef.restore(ck)
    o.restore(ck)
    return ef, o


def frame(ef, o, sc, ts=1):
    ef.processFrame(sc.rgb, sc.depth, ts, in_T_wc=np.eye(4))
    o.process_frame(sc.rgb, sc.depth, ts, T_wc=np.eye(4))
    return ef.downloadMap(), o.map()


@pytest.mark.parametrize("size", S.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("k", range(6), ids=["taps", "time_rules_silent", "time_rules_taps", "window_empty", "window_filled", "candidates"])
def test_restored_scene_and_one_frame(api, size, k):
    sc = scenes("frame_keep_scenes", *size)[k]
    ops_ref = sc.run(efo, efo.make_cam(*sc.cam))
    sc.check(ops_ref)
    ops_got = sc.run(api.ops, api.ef_cam(*sc.cam))          # the frame's map path spelled out with the operators
    assert bits_equal(ops_got, ops_ref), rows_differing(ops_got, ops_ref)
    ef, o = engines(api, sc)
    try:
        got, ref = frame(ef, o, sc)
        sc.check(ref)                                       # the whole frame does what the scene was written for, on the oracle
        assert bits_equal(ref, ops_ref)
        assert ef.lastCount() == o.map_count() == len(ref)
        assert bits_equal(got, ref), rows_differing(got, ref)
    finally:
        ef.close()


@pytest.mark.parametrize("n,cap", [(17000, 1 << 16), (S.BIG, 1 << 21)], ids=["17000", "million"])
def test_group_sums_of_a_restored_map(api, n, cap):
    sc = S.frame_bulk_scene(*S.SIZES[0], n)
    ef, o = engines(api, sc, cap)
    try:
        got, ref = frame(ef, o, sc)
        sc.check(ref)
        n_old = int(np.sum(sc.keep))
        assert bits_equal(ref[:n_old], sc.surf[np.array(sc.keep)])          # (a numpy mask, as well as the oracle)
        assert ef.lastCount() == o.map_count() == len(ref)
        assert bits_equal(got, ref), rows_differing(got, ref)
    finally:
        ef.close()


@pytest.mark.parametrize("size", S.SIZES, **SIZE_IDS)
@pytest.mark.parametrize("n", [5, 21])
def test_deformation_of_a_restored_scene_and_the_frame_after_it(api, size, n):
    sc = S.frame_deform_scene(*size, n)
    ef, o = engines(api, sc)
    try:
        ef.setDeformation(sc.graph)
        o.set_deformation(sc.graph)
        got, ref = frame(ef, o, sc)
        n_old = len(sc.surf)
        assert len(ref) > n_old and (ref[1:n_old, :3] != sc.surf[1:, :3]).any(axis=1).mean() > 0.9       # the graph moved the restored surfels
        assert ef.lastCount() == o.map_count() and bits_equal(got, ref), rows_differing(got, ref)
        got, ref = frame(ef, o, sc, 2)
        assert ef.lastCount() == o.map_count() and bits_equal(got, ref), rows_differing(got, ref)
    finally:
        ef.close()
