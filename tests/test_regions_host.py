"""CPU-only checks around the map's smooth regions (include/ef_hip.h, "Segment the map into smooth regions"): the numpy restatement
(tests/regionref.py) on cases whose answers are worked out by hand, that the scenes of tests/test_gpu_regions.py contain what they claim
under that reference, every EF_EINVAL with a NULL context, and the binding of the two new structs, the constants and the defaults."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import normalref as nref
import regionref as rref
import regionscenes as sc
from test_api_binding_host import RAW, defines, header_structs

F = np.float32
NONE = rref.NONE
CORE, BORDER = rref.KIND_CORE, rref.KIND_BORDER


@pytest.fixture(scope="module")
def lib():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    return api.lib()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference on hand-worked cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def grid(nx, ny, x0=0.0, z=0.0, nrm=(0, 0, 1.0)):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return sc.with_normals(np.stack([x0 + i.reshape(-1) * 1.0, j.reshape(-1) * 1.0, np.full(nx * ny, z)], 1), np.tile(nrm, (nx * ny, 1)))


HAND = dict(radius=1.5, k=8, min_neighbors=3, min_size=10)


def test_two_flat_grids_by_hand():
    # two 3 x 3 unit grids in the plane z = 0, 10 apart: flat, so every row is a core with curvature 0; radius 1.5 joins the 8-neighbourhood
    S = np.concatenate([grid(3, 3), grid(3, 3, x0=10.0)])
    r = rref.regions(S, **HAND)
    assert (r["kind"] == CORE).all() and (r["est"]["curvature"] == 0).all()
    assert r["label"].tolist() == [0] * 9 + [9] * 9 and r["size"].tolist() == [9] * 18
    assert r["result"] == dict(nodes=18, cores=18, borders=0, attached=0, unassigned=0, regions=2, largest=9, rejected_rows=18, rejected_regions=2, status=0)
    assert r["rejected"].tolist() == list(range(18)) and len(r["accepted"]) == len(r["unassigned"]) == len(r["borders"]) == 0
    assert rref.result_for(r, rref.REJECTED, 18)["count_after"] == 0 and rref.result_for(r, rref.BORDERS, 18) == dict(r["result"], listed=0, count_after=18)
    r = rref.regions(S, **dict(HAND, min_size=9, max_size=9))
    assert r["accepted"].tolist() == list(range(18)) and r["result"]["rejected_regions"] == 0
    # the second grid moved next to the first (x = 3 .. 5) with stored normals that point the other way: the estimates keep the stored side
    # (KEEP_SIDE), so the signed dot across the seam is -1 with either normal source: two regions, and one with two_sided
    T = np.concatenate([grid(3, 3), grid(3, 3, x0=3.0, nrm=(0, 0, -1.0))])
    assert rref.regions(np.concatenate([grid(3, 3), grid(3, 3, x0=3.0)]), **HAND)["label"].tolist() == [0] * 18
    for source in (rref.ESTIMATED, rref.STORED):
        r = rref.regions(T, normal_source=source, **HAND)
        assert (r["est"]["status"] == nref.ESTIMATED).all()
        assert (r["normal"][:9] == F([0, 0, 1])).all() and (r["normal"][9:] == F([0, 0, -1])).all()
        assert r["label"].tolist() == [0] * 9 + [9] * 9
        assert rref.regions(T, normal_source=source, two_sided=1, **HAND)["label"].tolist() == [0] * 18


def test_a_border_joins_its_nearest_smooth_core_and_bridges_nothing():
    # two 3 x 3 grids, x = 0 .. 2 and x = 4 .. 6, and between them at x = 3 a column of three rows at heights +-0.5: the column and the grids'
    # facing columns x = 2 and x = 4 have a curvature near 0.05 and are borders at max_curvature 0.02; the columns x = 0, 1, 5, 6 are flat
    S = np.concatenate([grid(3, 3), grid(3, 3, x0=4.0), sc.with_normals([(3.0, 0, 0.5), (3.0, 1, -0.5), (3.0, 2, 0.5)], np.tile((0, 0, 1.0), (3, 1)))])
    kw = dict(radius=1.5, k=8, min_neighbors=3, min_size=1, normal_source=rref.STORED, max_curvature=0.02)
    r = rref.regions(S, **kw)
    assert r["kind"].tolist() == [CORE] * 6 + [BORDER] * 3 + [BORDER] * 3 + [CORE] * 6 + [BORDER] * 3
    assert r["label"][:6].tolist() == [0] * 6 and r["label"][12:18].tolist() == [12] * 6, "the borders between them carry no edge"
    # a border of the column x = 2 joins the core of the column x = 1 beside it (d2 = 1; the diagonal ones are at d2 = 2)
    assert r["attach"][6:9].tolist() == [3, 4, 5] and r["attach"][9:12].tolist() == [12, 13, 14]
    assert r["label"][6:12].tolist() == [0] * 3 + [12] * 3 and r["size"][:18].tolist() == [9] * 18
    # the middle column has no core within 1.5 (the columns x = 1 and x = 5 are 2 away): UNASSIGNED although attach_borders is on
    assert r["attach"][18:].tolist() == [-1] * 3 and r["unassigned"].tolist() == [18, 19, 20] and (r["size"][18:] == 0).all()
    assert r["borders"].tolist() == list(range(6, 12)) + [18, 19, 20] and r["result"]["attached"] == 6 and r["result"]["unassigned"] == 3
    off = rref.regions(S, **dict(kw, attach_borders=0))
    assert off["unassigned"].tolist() == off["borders"].tolist() == r["borders"].tolist() and off["result"]["attached"] == 0
    assert off["size"].tolist() == [6] * 6 + [0] * 6 + [6] * 6 + [0] * 3


def test_rows_that_are_no_nodes():
    S = grid(4, 4)
    S[5, 3] = np.nan                      # a NaN confidence: a participant with an estimate, never a node, never a neighbour
    S[6, 0] = np.inf                      # no participant
    r = rref.regions(S, **HAND)
    st = r["est"]["status"]
    assert st[5] == nref.ESTIMATED and st[6] == nref.NONE
    assert r["kind"][[5, 6]].tolist() == [0, 0] and r["label"][[5, 6]].tolist() == [NONE, NONE]
    assert r["result"]["nodes"] == int((st == nref.ESTIMATED).sum()) - 1 >= 10
    mask = np.arange(16) >= 4
    r = rref.regions(S, among=mask, **HAND)                           # the first column does not participate (but still is a neighbour)
    assert (r["kind"][:4] == 0).all() and r["label"][4] == 4 and r["result"]["nodes"] == int(((r["est"]["status"] == nref.ESTIMATED) & mask).sum()) - 1
    line = sc.with_normals([(i, 0, 0) for i in range(8)], np.tile((0, 0, 1.0), (8, 1)))
    r = rref.regions(line, **HAND)                                    # a line has no normal: DEGENERATE rows are no nodes
    assert r["result"]["nodes"] == 0 and (r["label"] == NONE).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the scenes contain what they claim
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_box_corner_is_three_regions_and_its_creases_are_borders():
    S, m = sc.scene("box")
    r = sc.ref_of("box")
    assert r["result"]["regions"] == 3 and r["result"]["rejected_regions"] == 0 and len(S) > 10 * 256
    labels = [np.unique(r["label"][f][r["kind"][f] == CORE]) for f in m["faces"]]
    assert all(len(l) == 1 for l in labels) and len({int(l[0]) for l in labels}) == 3
    assert (r["size"][[int(l[0]) for l in labels]] > 128).all()
    assert (r["kind"][m["bad"][:4]] == 0).all() and (r["label"][m["bad"][:4]] == NONE).all()      # non-finite positions, a NaN confidence
    low = sc.ref_of("box", min_conf=10.0)                                                          # ... and with min_conf the two low ones
    assert (r["kind"][m["bad"][4:]] != 0).all() and (low["kind"][m["bad"]] == 0).all() and low["result"]["regions"] == 3
    # the borders are the crease rows: within 2.5 cm of an edge of the box, and every row within 5 mm of one is a border
    P = S[:, :3].astype(np.float64)
    near = np.sort(P, 1)[:, 1]                                         # the distance to the nearest edge: the second smallest coordinate
    b = r["kind"] == BORDER
    assert b.sum() > 100 and (near[b] < 0.025).all()
    node = r["kind"] != 0
    assert b[node & (near < 0.005)].all()
    # with the stored normals every crease row is smooth with its own face and attached to it
    s = sc.ref_of("box", normal_source=rref.STORED)
    assert s["result"]["regions"] == 3 and s["result"]["unassigned"] == 0 and s["result"]["attached"] == s["result"]["borders"] > 100
    for f, l in zip(m["faces"], labels):
        assert (s["label"][f] == l[0]).all()
    # among, inverted: a band 2 R wide cut out of the face z = 0 leaves four regions
    mask = ~((S[:, :3] >= F(sc.box_band(S)["box_min"])) & (S[:, :3] <= F(sc.box_band(S)["box_max"]))).all(1)
    assert 100 < (~mask).sum() < 300
    a = sc.ref_of("box", among=mask, among_key="band out", normal_source=rref.STORED)
    assert a["result"]["regions"] == 4 and (a["kind"][~mask] == 0).all()


def test_the_cylinder_is_one_region_although_its_normals_turn_all_the_way_round():
    S, m = sc.scene("cylinder")
    r = sc.ref_of("cylinder")
    assert r["result"]["regions"] == 2 and r["result"]["rejected_regions"] == 0
    side = m["side"][r["kind"][m["side"]] == CORE]
    plane = m["plane"][r["kind"][m["plane"]] == CORE]
    ls, lp = np.unique(r["label"][side]), np.unique(r["label"][plane])
    assert len(ls) == len(lp) == 1 and ls[0] != lp[0] and len(side) > 900 and len(plane) > 1500
    n = r["normal"][side]
    assert (n @ n.T).min() < -0.99, "two cores of the one region face opposite ways: smoothness is pairwise"


@pytest.mark.parametrize("source", (rref.ESTIMATED, rref.STORED))
def test_the_thin_wall_is_two_regions_signed_and_one_two_sided(source):
    S, m = sc.scene("wall")
    r = sc.ref_of("wall", normal_source=source)
    lo, hi = m["sheets"]
    assert r["result"]["regions"] == 2 and (r["label"][lo] == lo.min()).all() and (r["label"][hi] == hi.min()).all()
    assert (r["normal"][lo, 2] < -0.9).all() and (r["normal"][hi, 2] > 0.9).all()
    r = sc.ref_of("wall", normal_source=source, two_sided=1)
    assert r["result"]["regions"] == 1 and (r["label"] == 0).all() and r["result"]["largest"] == len(S)


@pytest.mark.parametrize("order", ("ascending", "descending", "shuffled"))
def test_the_core_chain_is_labelled_by_its_smallest_core_row(order):
    S, m = sc.scene("chain_" + order)
    r = sc.ref_of("chain_" + order)
    assert (r["kind"][m["specks"]] == 0).all() and (r["kind"][m["ribbon"]] == CORE).all()
    assert (r["label"][m["ribbon"]] == sc.N_SPECKS).all() and (r["label"][m["specks"]] == NONE).all()
    assert r["result"]["regions"] == 1 and r["result"]["largest"] == len(m["ribbon"]) > 8 * 256


def test_two_patches_that_touch_only_through_borders_stay_two():
    S, m = sc.scene("strip")
    r = sc.ref_of("strip", normal_source=rref.STORED)
    left, right = m["patches"]
    ll, lr = np.unique(r["label"][left]), np.unique(r["label"][right])
    assert r["result"]["regions"] == 2 and len(ll) == len(lr) == 1 and ll[0] != lr[0]
    assert (r["kind"][m["strip"]] == BORDER).mean() > 0.9 and r["result"]["attached"] > 100 and r["result"]["unassigned"] > 20
    # every pair of stored normals is smooth and the strip is dense: were its borders nodes of the graph, the patches would be one region
    import componentref as cref
    assert cref.components(S, radius=sc.R)["result"]["components"] == 1
    off = sc.ref_of("strip", normal_source=rref.STORED, attach_borders=0)
    assert off["result"]["attached"] == 0 and off["result"]["unassigned"] == off["result"]["borders"] == r["result"]["borders"]
    assert np.array_equal(off["unassigned"], r["borders"]) and (off["label"][r["kind"] == BORDER] == NONE).all()


def test_the_threshold_scene_contains_every_edge_it_claims():
    S, m = sc.scene("thresholds")
    kw = sc.THRESHOLD_KW
    s, t = m["dot_pair"]
    c = (S[s, 8] * S[t, 8] + S[s, 9] * S[t, 9]) + S[s, 10] * S[t, 10]
    assert c.dtype == F and 0.98 < c < 0.99
    r = sc.ref_of("thresholds", min_normal_cos=c, **kw)
    assert (r["kind"][[s, t]] == CORE).all() and r["label"][s] == r["label"][t], "dot == min_normal_cos: joined"
    assert [tuple(e) for e in r["pairs"].tolist() if set(e) & set(m["dot_a"].tolist()) and set(e) & set(m["dot_b"].tolist())] == [(max(s, t), min(s, t))]
    up = sc.ref_of("thresholds", min_normal_cos=sc.step(c, True), **kw)
    assert up["label"][s] != up["label"][t] and up["label"][s] == m["dot_a"][up["kind"][m["dot_a"]] == CORE].min()
    assert up["label"][t] == m["dot_b"].min()
    # d2 == r2, and one float beyond
    a, b = m["at_r"]
    d = S[a, :3] - S[b, :3]
    assert ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) == F(F(sc.R_EXACT) * F(sc.R_EXACT))
    assert r["label"][a] == r["label"][b] == min(m["at_r_a"].min(), m["at_r_b"].min())
    a, b = m["beyond"]
    d = S[a, :3] - S[b, :3]
    assert -d[0] == sc.step(sc.R_EXACT, True) and d[1] == d[2] == 0 and ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) > F(F(sc.R_EXACT) * F(sc.R_EXACT))
    assert r["label"][a] == m["beyond_a"].min() and r["label"][b] == m["beyond_b"].min()
    # the tie: a border at equal d2 bits from a core of either region joins the lower row's
    bt, (ta, tc) = m["tie_b"][0], m["tie_cores"]
    assert r["kind"][bt] == BORDER and (r["kind"][[ta, tc]] == CORE).all() and r["label"][ta] != r["label"][tc]
    da, dc = S[bt, :3] - S[ta, :3], S[bt, :3] - S[tc, :3]
    d2a, d2c = (da[0] * da[0] + da[1] * da[1]) + da[2] * da[2], (dc[0] * dc[0] + dc[1] * dc[1]) + dc[2] * dc[2]
    assert d2a.tobytes() == d2c.tobytes()
    cores = np.nonzero(r["kind"] == CORE)[0]
    dd = ((S[cores, :3].astype(np.float64) - S[bt, :3].astype(np.float64)) ** 2).sum(1)
    assert sorted(cores[dd == dd.min()].tolist()) == sorted([ta, tc]), "they are its two nearest cores"
    assert r["attach"][bt] == min(ta, tc) and r["label"][bt] == r["label"][min(ta, tc)]
    # a NaN and a zero stored normal: cores that are smooth with nothing
    for k in ("nan", "zero"):
        x = m[k][0]
        assert r["kind"][x] == CORE and r["label"][x] == x and r["size"][x] == 1
    zero = sc.ref_of("thresholds", min_normal_cos=0.0, **kw)
    assert zero["label"][m["zero"][0]] == zero["label"][s] and zero["label"][m["nan"][0]] == m["nan"][0]     # 0 >= 0 joins; a NaN never
    # max_curvature at a row's own f32 curvature: a core; one float below: a border
    box = sc.ref_of("box")
    cv = box["est"]["curvature"]
    x = int(np.nonzero((box["kind"] == CORE) & (cv > 0.01))[0][0])
    assert sc.ref_of("box", max_curvature=cv[x])["kind"][x] == CORE and sc.ref_of("box", max_curvature=sc.step(cv[x], False))["kind"][x] == BORDER


def test_the_components_edge_scene_has_nodes_non_nodes_and_colliding_groups():
    import componentscenes as csc
    S, m = sc.scene("edge")
    r = sc.ref_of("edge", radius=csc.R_EDGE, **sc.EDGE_KW)
    assert r["result"]["regions"] > 10 and 0 < r["result"]["rejected_rows"] and r["result"]["nodes"] < len(S) - 50
    assert (r["kind"][m["bad"]] == 0).all()
    ga, gb = m["collide"]
    assert (r["kind"][ga] == CORE).all() and (r["kind"][gb] == CORE).all() and not set(r["label"][ga]) & set(r["label"][gb])
    low = sc.ref_of("edge", radius=csc.R_EDGE, min_conf=10.0, **sc.EDGE_KW)
    assert low["result"]["nodes"] < r["result"]["nodes"] - 50 and (low["kind"][S[:, 3] == sc.CONF_LOW] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals, the binding
# ---------------------------------------------------------------------------------------------------------------------------------------
def good_params(**kw):
    from elasticfusion_amd import api
    p = api.ef_region_params(radius=0.03, cell=0.03, min_conf=-1.0, k=12, min_neighbors=5, line_ratio=1e-4, normal_source=0, two_sided=0,
                             min_normal_cos=0.9659258, max_curvature=0.05, attach_borders=1, min_size=50, max_size=0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


NAN = float("nan")
BAD = [(dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=NAN), "radius"), (dict(radius=float("inf")), "radius"),
       (dict(cell=0.0), "cell"), (dict(cell=-0.03), "cell"), (dict(cell=NAN), "cell"), (dict(cell=float("inf")), "cell"),
       (dict(cell=1e-45), "cell"), (dict(radius=0.5, cell=0.03), "radius / cell"), (dict(min_conf=NAN), "min_conf"),
       (dict(k=2), "k must"), (dict(k=17), "k must"), (dict(min_neighbors=1), "min_neighbors"), (dict(min_neighbors=13), "min_neighbors"),
       (dict(line_ratio=NAN), "line_ratio"), (dict(line_ratio=-1e-4), "line_ratio"), (dict(max_curvature=NAN), "max_curvature"),
       (dict(max_curvature=-0.01), "max_curvature"), (dict(min_normal_cos=NAN), "min_normal_cos"), (dict(normal_source=2), "normal_source"),
       (dict(normal_source=-1), "normal_source")]


def test_every_refusal_names_its_argument_with_a_null_context(lib):
    from elasticfusion_amd import api
    EINVAL = -1
    res, cnt, rows = api.ef_region_result(), C.c_uint32(0), (C.c_uint32 * 4)()
    calls = {
        "ef_map_regions": lambda p, a: lib.ef_map_regions(None, p, a, None, None, None, 0, None),
        "ef_map_regions_dev": lambda p, a: lib.ef_map_regions_dev(None, p, a, None, None, None, 0, None),
        "ef_map_regions_select": lambda p, a: lib.ef_map_regions_select(None, p, a, api.REGIONS_BORDERS, rows, 4, C.byref(cnt), None),
        "ef_map_regions_select_dev": lambda p, a: lib.ef_map_regions_select_dev(None, p, a, api.REGIONS_UNASSIGNED, rows, 4, C.byref(cnt), None),
        "ef_map_remove_regions": lambda p, a: lib.ef_map_remove_regions(None, p, a, api.REGIONS_REJECTED, C.byref(res)),
    }

    def refused(rc, fn, word):
        msg = lib.ef_last_error(None).decode()
        assert rc == EINVAL and msg.startswith(fn + ":") and word in msg, (fn, word, rc, msg)

    for fn, call in calls.items():
        refused(call(None, None), fn, "null params")
        for change, word in BAD:
            refused(call(C.byref(good_params(**change)), None), fn, word)
        refused(call(C.byref(good_params(radius=0.48, cell=0.03)), None), fn, "null context")             # a ratio of 16 is allowed
        refused(call(C.byref(good_params(min_normal_cos=-2.0, max_curvature=0.0, k=3, min_neighbors=2)), None), fn, "null context")
        refused(call(C.byref(good_params()), None), fn, "null context")                                    # all is well but the context
        sel = api.ef_map_selection()
        lib.ef_default_map_selection(C.byref(sel))
        sel.tests = 0x8000
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "unknown bits")                            # what ef_map_select refuses
        sel.tests, sel.conf_min = api.SEL_CONF, NAN
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "NaN")
    p = C.byref(good_params())
    for fn in ("ef_map_regions_select", "ef_map_regions_select_dev"):
        call = getattr(lib, fn)
        for what in (4, -1):
            refused(call(None, p, None, what, rows, 4, C.byref(cnt), None), fn, "what")
        refused(call(None, p, None, 0, None, 4, C.byref(cnt), None), fn, "null rows")
        refused(call(None, p, None, 0, rows, 4, None, None), fn, "null count")
        refused(call(None, p, None, 3, None, 0, C.byref(cnt), None), fn, "null context")                  # NULL rows with max_rows 0 is fine
    refused(lib.ef_map_remove_regions(None, p, None, 0, None), "ef_map_remove_regions", "null result")
    for what in (4, -1):
        refused(lib.ef_map_remove_regions(None, p, None, what, C.byref(res)), "ef_map_remove_regions", "what")
    assert lib.ef_default_region_params(None, C.byref(good_params())) == EINVAL and b"null context" in lib.ef_last_error(None)


def test_the_new_structs_constants_and_defaults_are_the_headers():
    from elasticfusion_amd import accuracy, api
    structs = header_structs()
    assert structs["ef_region_params"] == [f for f, _ in api.ef_region_params._fields_]
    assert structs["ef_region_result"] == [f for f, _ in api.ef_region_result._fields_] == [
        "nodes", "cores", "borders", "attached", "unassigned", "regions", "largest", "rejected_rows", "rejected_regions", "listed", "count_after", "status"]
    assert C.sizeof(api.ef_region_params) == 52 and C.sizeof(api.ef_region_result) == 48                  # thirteen and twelve 4-byte fields
    assert api.ef_region_params.min_size.offset == 44 and api.ef_region_result.status.offset == 44
    want = defines("REGION")
    mine = {k: v for k, v in vars(api).items() if k.startswith("REGION") and isinstance(v, int)}
    assert want == dict(REGION_NONE=0xFFFFFFFF, REGION_KIND_NONE=0, REGION_KIND_CORE=1, REGION_KIND_BORDER=2, REGIONS_ESTIMATED=0, REGIONS_STORED=1,
                        REGIONS_REJECTED=0, REGIONS_ACCEPTED=1, REGIONS_UNASSIGNED=2, REGIONS_BORDERS=3) and mine == want, (mine, want)
    assert (rref.NONE, rref.KIND_NONE, rref.KIND_CORE, rref.KIND_BORDER) == (api.REGION_NONE, api.REGION_KIND_NONE, api.REGION_KIND_CORE, api.REGION_KIND_BORDER)
    assert (rref.ESTIMATED, rref.STORED) == (api.REGIONS_ESTIMATED, api.REGIONS_STORED)
    assert (rref.REJECTED, rref.ACCEPTED, rref.UNASSIGNED, rref.BORDERS) == (api.REGIONS_REJECTED, api.REGIONS_ACCEPTED, api.REGIONS_UNASSIGNED, api.REGIONS_BORDERS)
    for name in ("regionParams", "regions", "regionSelect", "regionSelectDevice", "regionsDevice", "removeRegions"):
        assert callable(getattr(api.ElasticFusion, name))
    assert callable(accuracy.smooth_regions)
    # the defaults the header states are the reference's (tests/test_gpu_regions.py compares ef_default_region_params with them on the device)
    text = " ".join(RAW[RAW.index("Defaults (ef_default_region_params)"):RAW.index("Not provided: a model per region")].replace(" * ", " ").split())
    d = rref.DEFAULTS
    for piece in ("radius 0.03 m", "cell 0.03 m", "min_conf -1", "k 12", "min_neighbors 5", "line_ratio 1e-4", "EF_REGIONS_ESTIMATED", "two_sided 0",
                  "min_normal_cos 0.9659258", "max_curvature 0.05", "attach_borders 1", "min_size 50", "max_size 0"):
        assert piece in text, piece
    assert (d["radius"], d["min_conf"], d["k"], d["min_neighbors"], d["line_ratio"], d["normal_source"], d["two_sided"]) == (0.03, -1.0, 12, 5, 1e-4, 0, 0)
    assert (d["min_normal_cos"], d["max_curvature"], d["attach_borders"], d["min_size"], d["max_size"]) == (F(0.9659258), 0.05, 1, 50, 0)
    assert abs(float(F(0.9659258)) - np.cos(np.radians(15.0))) < 1e-7
    # the normals' section no longer lists region growing as missing
    normals = RAW[RAW.index("/* ---- Estimate normals"):RAW.index("/* ---- Segment the map into smooth regions")]
    assert not re.search(r"Not provided:[^.]*region growing itself", normals)
