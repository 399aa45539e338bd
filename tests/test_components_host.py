"""CPU-only checks around the map's connected components (include/ef_hip.h, "Connected components of the map"): the numpy restatement
(tests/componentref.py) on cases whose answers are worked out by hand, that the scenes of tests/test_gpu_components.py contain the edges they
claim (the colliding buckets among them), every EF_EINVAL with a NULL context, the binding of the two new structs and the constants, and the
union-find of csrc/ef_unionfind.hpp on sixteen host threads (tests/uf_threads.cpp, a child process, under the thread sanitizer where the host
compiler has its runtime)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import componentref as cref
import componentscenes as sc
from test_api_binding_host import defines, header_structs

F = np.float32
NONE = cref.NONE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference on hand-worked cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_labels_sizes_and_result_by_hand():
    # rows 0-4-2 are a chain (0.8 apart), row 1 is alone, row 3 is not finite, rows 5 and 6 coincide far away
    S = sc.of_points([(0, 0, 0), (9, 9, 9), (1.6, 0, 0), (np.nan, 0, 0), (0.8, 0, 0), (-5, 0, 0), (-5, 0, 0)])
    r = cref.components(S, radius=1.0, min_size=2, max_size=2)
    assert r["label"].tolist() == [0, 1, 0, NONE, 0, 5, 5]
    assert r["size"].tolist() == [3, 1, 3, 0, 3, 2, 2]
    assert sorted(map(tuple, r["pairs"].tolist())) == [(4, 0), (4, 2), (6, 5)]
    assert r["rejected"].tolist() == [0, 1, 2, 4] and r["accepted"].tolist() == [5, 6]        # 3 > max_size, 1 < min_size, 2 fits
    assert r["result"] == dict(nodes=6, components=3, largest=3, rejected_rows=4, rejected_components=2, count_after=3, status=0)
    r = cref.components(S, radius=1.0, min_size=0, max_size=0)
    assert len(r["rejected"]) == 0 and r["accepted"].tolist() == [0, 1, 2, 4, 5, 6]
    r = cref.components(S, radius=0.5)                                                         # nothing joined but the coincident pair
    assert r["label"].tolist() == [0, 1, 2, NONE, 4, 5, 5] and r["result"]["components"] == 5 and r["result"]["largest"] == 2


def test_the_label_is_the_smallest_row_whatever_the_order():
    S = sc.of_points([(3, 0, 0), (2, 0, 0), (1, 0, 0), (0, 0, 0)])                              # the chain's far end is row 0
    assert cref.components(S, radius=1.0)["label"].tolist() == [0, 0, 0, 0]
    assert cref.components(S[[1, 3, 0, 2]], radius=1.0)["label"].tolist() == [0, 0, 0, 0]       # the same chain in another row order
    S = sc.of_points([(5, 0, 0), (0, 0, 0), (6, 0, 0), (1, 0, 0)])                              # two pairs, interleaved rows
    assert cref.components(S, radius=1.0)["label"].tolist() == [0, 1, 0, 1]


def test_a_row_that_is_no_node_does_not_bridge():
    S = sc.of_points([(0, 0, 0), (1, 0, 0), (2, 0, 0)], conf=[sc.CONF_HIGH, sc.CONF_LOW, sc.CONF_HIGH])
    assert cref.components(S, radius=1.0)["label"].tolist() == [0, 0, 0]
    r = cref.components(S, radius=1.0, min_conf=10.0)
    assert r["label"].tolist() == [0, NONE, 2] and r["size"].tolist() == [1, 0, 1]
    r = cref.components(S, radius=1.0, among=np.array([True, False, True]))
    assert r["label"].tolist() == [0, NONE, 2] and r["result"]["nodes"] == 2
    S[1, 3] = np.nan                                                                           # a NaN confidence passes no comparison
    assert cref.components(S, radius=1.0)["label"].tolist() == [0, NONE, 2]


def test_the_distance_is_symmetric_in_f32():
    rng = np.random.default_rng(1)
    p = (rng.normal(size=(4000, 3)) * 10.0 ** rng.uniform(-3, 5, (4000, 1))).astype(F)
    q = (p + rng.normal(size=p.shape) * 0.03).astype(F)

    def d2(a, b):
        d = a - b
        return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])

    assert d2(p, q).dtype == F and np.array_equal(d2(p, q).view(np.uint32), d2(q, p).view(np.uint32))


def test_same_partition():
    assert cref.same_partition([0, 0, 2, NONE], [NONE, 1, 0, 0], np.array([2, 3, 1, 0]))
    assert not cref.same_partition([0, 0, 2, NONE], [NONE, 1, 0, 0], np.array([1, 3, 2, 0]))
    assert not cref.same_partition([0, 0, 2, 3], [0, 0, 0, 3], np.arange(4))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the scenes of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ("ascending", "descending", "shuffled"))
def test_the_chains_are_one_component_across_many_cells(order):
    S, place = sc.chain(order)
    r = cref.components(S, radius=sc.R)
    assert len(S) == 3000 and len(r["pairs"]) == 2999                                         # neighbours only: 1.8 R is outside
    assert (r["label"] == 0).all() and (r["size"] == 3000).all()
    cells = np.floor(S[:, 0] * F(1 / sc.R))
    assert len(np.unique(cells)) > 2500 and cells.min() < -30 and cells.max() > 2000
    if order == "descending":
        assert place[0] == 2999                                                               # the smallest row stands at the far end
    if order == "shuffled":
        assert place[0] not in (0, 2999)


def test_the_sheet_is_one_component_with_eight_neighbours_inside():
    S = sc.sheet()
    r = cref.components(S, radius=sc.R)
    assert len(S) == 96 * 96 and (r["label"] == 0).all()
    deg = np.bincount(r["pairs"].ravel(), minlength=len(S))
    assert deg.max() == 8 and (deg == 8).sum() == 94 * 94 and deg.min() == 3


def test_the_edge_scene_contains_every_edge_it_claims():
    S, m = sc.edge_scene()
    n = len(S)
    assert n == 700 and sc.query_buckets(n) == 1024
    r = cref.components(S, radius=sc.R_EDGE)
    label, size = r["label"], r["size"]
    a, b = m["at_r"]
    assert F(S[a, 0] - S[b, 0]) ** 2 == F(sc.R_EDGE) * F(sc.R_EDGE) and label[a] == label[b] == min(a, b) and size[a] == 2
    a, b = m["beyond_r"]
    assert abs(float(S[a, 0]) - float(S[b, 0])) > sc.R_EDGE and label[a] == a and label[b] == b and size[a] == size[b] == 1
    a, b = m["coincident"]
    assert (S[a, :3] == S[b, :3]).all() and a != b and label[a] == label[b] == min(a, b) and size[a] == 2
    assert label[m["lone"][0]] == m["lone"][0] and size[m["lone"][0]] == 1
    assert not np.isfinite(S[m["bad"], :3]).all(1).any() and (label[m["bad"]] == NONE).all() and (size[m["bad"]] == 0).all()
    for key in ("bridge_among", "bridge_conf"):                                               # whole: one component of five
        left, bridge, right = m[key]
        rows = np.concatenate([left, bridge, right])
        assert (label[rows] == rows.min()).all() and (size[rows] == 5).all()
    # ... and two of two without the bridge: by confidence, and by a box with its inversion
    left, bridge, right = m["bridge_conf"]
    assert S[bridge[0], 3] == sc.CONF_LOW
    r10 = cref.components(S, radius=sc.R_EDGE, min_conf=10.0)
    assert r10["label"][bridge[0]] == NONE and (r10["label"][left] == left.min()).all() and (r10["label"][right] == right.min()).all()
    left, bridge, right = m["bridge_among"]
    box = sc.bridge_box(S, m)
    inside = ((S[:, :3] >= F(box["box_min"])) & (S[:, :3] <= F(box["box_max"]))).all(1)
    assert np.nonzero(inside)[0].tolist() == bridge.tolist()
    ri = cref.components(S, radius=sc.R_EDGE, among=~inside)
    assert ri["label"][bridge[0]] == NONE and (ri["label"][left] == left.min()).all() and (ri["label"][right] == right.min()).all()
    assert ri["size"][left].tolist() == [2, 2]
    rb = cref.components(S, radius=sc.R_EDGE, among=inside)
    assert rb["result"]["nodes"] == 1 and rb["label"][bridge[0]] == bridge[0]
    # negative coordinates across two cells
    neg = m["negative"]
    assert (S[neg, :3] < 0).all() and len(np.unique(np.floor(S[neg, 0] / F(sc.R_EDGE)))) == 2 and (label[neg] == neg.min()).all() and size[neg[0]] == 3
    # beyond the cell clamp at both cells the tests use: every such position shares the boundary cell
    joined, apart = m["far"]
    for cell in (sc.R_EDGE, sc.R_EDGE / 16):
        assert (np.floor(S[np.concatenate([joined, apart, m["far_negative"]]), :2] * F(1 / cell)).__abs__().max(1) > 2 ** 20).all()
    assert (label[joined] == joined.min()).all() and size[joined[0]] == 2 and label[apart[0]] == apart[0] and size[apart[0]] == 1
    assert (label[m["far_negative"]] == m["far_negative"].min()).all()
    # the colliding buckets: two cells a hundred cells apart in ONE bucket of the 1024, each with a group of six that is one component
    ga, gb = m["collide"]
    mask = sc.query_buckets(n) - 1
    cells = np.floor(np.nan_to_num(S[:, :3], nan=0.0, posinf=0.0, neginf=0.0) * F(1 / sc.R_EDGE)).astype(np.int64)
    assert (cells[ga] == sc.CELL_A).all() and (cells[gb] == m["cell_b"]).all() and abs(m["cell_b"][0] - sc.CELL_A[0]) >= 100
    assert sc.query_hash(sc.CELL_A, mask) == sc.query_hash(m["cell_b"], mask)
    assert (label[ga] == ga.min()).all() and (label[gb] == gb.min()).all() and ga.min() != gb.min() and size[ga[0]] == size[gb[0]] == 6
    # the clumps have exactly their sizes
    for k, rows in m["clumps"].items():
        assert len(rows) == k and (label[rows] == rows.min()).all() and (size[rows] == k).all()
    # the cloud: components of many sizes
    sizes = np.unique(size[m["cloud"]])
    assert sizes.min() == 1 and len(sizes) > 5


def test_the_random_cloud_is_near_the_percolation_threshold():
    S = sc.cloud(sc.N_CLOUD, seed=21)
    r = cref.components(S, radius=sc.R_CLOUD)
    size, res = r["size"], r["result"]
    print("cloud:", res, "mean degree", 2 * len(r["pairs"]) / len(S))
    assert len(S) == 20000 and res["nodes"] == 20000
    assert (size == 1).sum() > 100 and res["largest"] > 1000 and res["largest"] < 19000 and res["components"] > 500
    assert len(np.unique(size)) > 20


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C ABI without a context
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from elasticfusion_amd import api, build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    return api.lib()


def good_params(**kw):
    from elasticfusion_amd import api
    p = api.ef_component_params(radius=0.03, cell=0.03, min_conf=-1.0, min_size=50, max_size=0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD = [(dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=float("nan")), "radius"), (dict(radius=float("inf")), "radius"),
       (dict(cell=0.0), "cell"), (dict(cell=-0.03), "cell"), (dict(cell=float("nan")), "cell"), (dict(cell=float("inf")), "cell"),
       (dict(cell=1e-45), "cell"), (dict(radius=0.5, cell=0.03), "radius / cell"), (dict(min_conf=float("nan")), "min_conf")]


def test_every_refusal_names_its_argument_with_a_null_context(lib):
    from elasticfusion_amd import api
    EINVAL = -1
    res, cnt, rows = api.ef_component_result(), C.c_uint32(0), (C.c_uint32 * 4)()
    calls = {
        "ef_map_components": lambda p, a: lib.ef_map_components(None, p, a, None, None, 0, None),
        "ef_map_components_dev": lambda p, a: lib.ef_map_components_dev(None, p, a, None, None, 0, None),
        "ef_map_components_select": lambda p, a: lib.ef_map_components_select(None, p, a, api.COMPONENTS_ACCEPTED, rows, 4, C.byref(cnt), None),
        "ef_map_components_select_dev": lambda p, a: lib.ef_map_components_select_dev(None, p, a, api.COMPONENTS_REJECTED, rows, 4, C.byref(cnt), None),
        "ef_map_remove_components": lambda p, a: lib.ef_map_remove_components(None, p, a, C.byref(res)),
    }

    def refused(rc, fn, word):
        msg = lib.ef_last_error(None).decode()
        assert rc == EINVAL and msg.startswith(fn + ":") and word in msg, (fn, word, rc, msg)

    for fn, call in calls.items():
        refused(call(None, None), fn, "null params")
        for change, word in BAD:
            refused(call(C.byref(good_params(**change)), None), fn, word)
        refused(call(C.byref(good_params(radius=0.48, cell=0.03)), None), fn, "null context")             # a ratio of 16 is allowed
        refused(call(C.byref(good_params()), None), fn, "null context")                                    # all is well but the context
        sel = api.ef_map_selection()
        lib.ef_default_map_selection(C.byref(sel))
        sel.tests = 0x8000
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "unknown bits")                            # what ef_map_select refuses
        sel.tests, sel.conf_min = api.SEL_CONF, float("nan")
        refused(call(C.byref(good_params()), C.byref(sel)), fn, "NaN")
    p = C.byref(good_params())
    for fn in ("ef_map_components_select", "ef_map_components_select_dev"):
        call = getattr(lib, fn)
        for what in (2, -1):
            refused(call(None, p, None, what, rows, 4, C.byref(cnt), None), fn, "what")
        refused(call(None, p, None, 0, None, 4, C.byref(cnt), None), fn, "null rows")
        refused(call(None, p, None, 0, rows, 4, None, None), fn, "null count")
        refused(call(None, p, None, 1, None, 0, C.byref(cnt), None), fn, "null context")                  # NULL rows with max_rows 0 is fine
    refused(lib.ef_map_remove_components(None, p, None, None), "ef_map_remove_components", "null result")
    assert lib.ef_default_component_params(None, C.byref(good_params())) == EINVAL and b"null context" in lib.ef_last_error(None)


def test_the_new_structs_and_constants_are_the_headers():
    from elasticfusion_amd import accuracy, api
    structs = header_structs()
    assert structs["ef_component_params"] == [f for f, _ in api.ef_component_params._fields_]
    assert structs["ef_component_result"] == [f for f, _ in api.ef_component_result._fields_]
    assert C.sizeof(api.ef_component_params) == 20 and C.sizeof(api.ef_component_result) == 28             # five and seven 4-byte fields
    assert api.ef_component_params.min_size.offset == 12 and api.ef_component_result.status.offset == 24
    want = defines("COMPONENT")
    mine = {k: v for k, v in vars(api).items() if k.startswith("COMPONENT") and isinstance(v, int)}
    assert want == dict(COMPONENT_NONE=0xFFFFFFFF, COMPONENTS_REJECTED=0, COMPONENTS_ACCEPTED=1) and mine == want, (mine, want)
    assert (cref.NONE, cref.REJECTED, cref.ACCEPTED) == (api.COMPONENT_NONE, api.COMPONENTS_REJECTED, api.COMPONENTS_ACCEPTED)
    for name in ("componentParams", "components", "componentSelect", "componentSelectDevice", "componentsDevice", "removeComponents"):
        assert callable(getattr(api.ElasticFusion, name))
    assert callable(accuracy.largest_component) and callable(accuracy.segments)
    # the scenes' restatement of the index's hash is the kernels'
    src = open(os.path.join(ROOT, "elasticfusion_amd", "csrc", "ef_query.inc")).read()
    assert "(unsigned)x * 73856093u) ^ ((unsigned)y * 19349663u) ^ ((unsigned)z * 83492791u)) & mask" in src
    assert "unsigned nb = QUERY_SCAN_TILE;" in src and "QUERY_SCAN_TILE = 1024" in src


# ---------------------------------------------------------------------------------------------------------------------------------------
# the union-find on host threads
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_union_find_on_sixteen_host_threads(tmp_path):
    """tests/uf_threads.cpp: csrc/ef_unionfind.hpp with the compiler's atomic builtins, the chain and sheet scenes' edges dealt round-robin to
    sixteen threads, labels against a sequential union-find.  A stand-alone program in a child process; with the thread sanitizer where a
    trial program links and runs, plain otherwise (the test says which)."""
    src = os.path.join(ROOT, "tests", "uf_threads.cpp")
    inc = os.path.join(ROOT, "elasticfusion_amd", "csrc")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", inc]
    trial = tmp_path / "trial.cpp"
    trial.write_text("#include <thread>\nint main() { int v = 0; std::thread t([&] { v = 1; }); t.join(); return v - 1; }\n")
    tsan = ["-fsanitize=thread"]
    ok = subprocess.run(base + tsan + [str(trial), "-o", str(tmp_path / "trial")], capture_output=True).returncode == 0
    ok = ok and subprocess.run([str(tmp_path / "trial")], capture_output=True).returncode == 0
    exe = tmp_path / "uf_threads"
    subprocess.run(base + (tsan if ok else []) + [src, "-o", str(exe)], check=True)
    print("thread sanitizer:", "on" if ok else "not available, plain build")
    got = subprocess.run([str(exe), "16"], capture_output=True, text=True, timeout=120)
    assert got.returncode == 0 and got.stdout.strip() == "ok 15" and "ThreadSanitizer" not in got.stderr, (got.returncode, got.stdout, got.stderr[-2000:])
