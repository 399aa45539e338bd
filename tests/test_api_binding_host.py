"""CPU-only checks that elasticfusion_amd.api binds the C ABI as include/ef_hip.h declares it: the ctypes.Structure mirrors against the
host compiler's sizeof / offsetof, the signatures api.lib() declares against the header's prototypes, pointer parameters at full
width, and the module's constants and index tables against the header's #defines and enums.  The header is parsed here on its own,
not through api.signatures()."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from elasticfusion_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
RAW = open(os.path.join(INCLUDE, "ef_hip.h")).read()
CODE = re.sub(r"/\*.*?\*/|//[^\n]*", " ", RAW, flags=re.S)          # the header without its comments
ALIASES = {"ef_global_loop": "GlobalLoop", "ef_reloc_state": "RelocState", "ef_local_loop": "LocalLoop", "ef_graph_constraint": "GraphConstraint"}
CALLBACKS = ("ef_fern_tracker", "ef_view_fetch", "ef_loop_solver")


def header_structs():
    """name -> field names in order, of every `typedef struct name { ... } name;`"""
    out = {}
    for name, body, closing in re.findall(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", CODE):
        assert closing == name
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            for piece in decl.split(","):
                fields.append(re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", piece).group(1))
        out[name] = fields
    return out


def header_prototypes():
    """name -> (return type, [parameter declarations]) of every ef_* function; the names are found the way test_capi_host.py finds them"""
    names = sorted(set(re.findall(r"\b(ef_[a-z0-9_]+)\s*\(", RAW)))
    out = {}
    for name in names:
        found = re.findall(r"([\w \t*]+?)\b%s\s*\(([^()]*)\)\s*;" % name, CODE)
        assert len(found) == 1, (name, found)
        ret, params = found[0]
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [] if params in ([""], ["void"]) else params)
    return out


@pytest.fixture(scope="module")
def lib():
    from elasticfusion_amd import build
    if not os.path.exists(api.LIB_PATH):
        build.build()
    return api.lib()


def is_pointer_type(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, (C._Pointer, C._CFuncPtr)))


def test_structure_mirrors_have_the_layout_the_compiler_gives_the_header(tmp_path):
    structs = header_structs()
    assert len(structs) >= 28 and "ef_kernel_time" in structs and "ef_config" in structs
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "ef_hip.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append(f'  printf("{name} %zu 0\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    subprocess.check_call([cc, "-I", INCLUDE, "-o", str(tmp_path / "layout"), str(src)])
    want = {k: (int(a), int(b)) for k, a, b in (l.split() for l in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())}
    assert len(want) == sum(1 + len(f) for f in structs.values())
    bad = []
    for name, fields in structs.items():
        cls = getattr(api, ALIASES.get(name, name), None)
        if not (isinstance(cls, type) and issubclass(cls, C.Structure)):
            bad.append(f"{name}: no mirror in api")
            continue
        mine = [f for f, _ in cls._fields_]
        if mine != fields:
            bad.append(f"{name}: fields {mine} against the header's {fields}")
            continue
        if C.sizeof(cls) != want[name][0]:
            bad.append(f"{name}: sizeof {C.sizeof(cls)} against {want[name][0]}")
        for f in fields:
            d = getattr(cls, f)
            if (d.offset, d.size) != want[f"{name}.{f}"]:
                bad.append(f"{name}.{f}: (offset, size) {(d.offset, d.size)} against {want[f'{name}.{f}']}")
    assert not bad, "\n".join(bad)
    mirrors = {n for n, v in vars(api).items() if isinstance(v, type) and issubclass(v, C.Structure)}
    assert mirrors == {ALIASES.get(n, n) for n in structs}, "a Structure in api that the header does not declare"


def test_every_header_prototype_has_its_signature_declared(lib):
    protos = header_prototypes()
    assert len(protos) == len(api.signatures()) >= 193 and set(protos) == set(api.signatures()), set(protos) ^ set(api.signatures())
    bad = []
    for name, (ret, params) in protos.items():
        fn = getattr(lib, name)
        if fn.argtypes is None or len(fn.argtypes) != len(params):
            bad.append(f"{name}: argtypes {fn.argtypes} for {params}")
            continue
        for p, t in zip(params, fn.argtypes):
            if ("*" in p or p.split()[0] in CALLBACKS) and not is_pointer_type(t):
                bad.append(f"{name}: '{p}' declared {t}")
            if "*" not in p and p.split()[0] not in CALLBACKS and is_pointer_type(t):
                bad.append(f"{name}: scalar '{p}' declared {t}")
        if ret == "void":
            ok = fn.restype is None
        elif ret == "int":
            ok = fn.restype is C.c_int
        elif ret == "float":
            ok = fn.restype is C.c_float
        else:
            assert "*" in ret, (name, ret)
            ok = fn.restype is (C.c_char_p if ret == "const char*" else C.c_void_p)
        if not ok:
            bad.append(f"{name}: returns '{ret}', restype {fn.restype}")
    assert not bad, "\n".join(bad)
    # (spot checks of the scalar kinds)
    assert lib.ef_process_frame_dev.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]
    assert lib.ef_dev_alloc.argtypes == [C.c_void_p, C.c_size_t] and lib.ef_map_upload.argtypes == [C.c_void_p, C.c_void_p, C.c_uint32]
    assert lib.ef_ferns_create.argtypes[-1] is C.c_uint32 and lib.ef_dev_sync.argtypes == []
    assert lib.ef_set_loop_solver.argtypes[1] is api.LOOP_SOLVER and lib.ef_closure_global.argtypes[7] is api.FERN_TRACKER


def test_a_prototype_of_an_unknown_kind_is_refused():
    for decl, table, words in (("long n", api._SCALARS, 2), ("unsigned int n", api._SCALARS, 2), ("double", api._RETURNS, 1), ("ef_cam c", api._SCALARS, 2)):
        with pytest.raises(api.EFError, match="ef_made_up"):
            api._kind(decl, table, words, "int ef_made_up(...)")


def test_device_pointers_pass_at_full_width(lib):
    addr = 0x7F0012345678
    seen = 0
    for name, (_, params) in header_prototypes().items():
        if not name.endswith("_dev"):
            continue
        for p, t in zip(params, getattr(lib, name).argtypes):
            if "*" in p:
                assert "0x%x" % addr in repr(t.from_param(addr)).lower(), (name, p, t)
                seen += 1
    assert seen > 40
    assert "0x%x" % addr not in repr(C.c_int.from_param(addr)).lower()      # what an undeclared parameter made of it
    assert api._dev(None) is None and api._dev(addr) == addr and api._dev(C.c_void_p(addr)).value == addr


def defines(prefix):
    out = {}
    for name, value in re.findall(r"^[ \t]*#define[ \t]+EF_(%s\w*)[ \t]+(\S+)" % prefix, CODE, flags=re.M):
        out[name] = int(value.strip("()").rstrip("uU"), 0)
    return out


def enum(name):
    body = re.search(r"enum\s+%s\s*\{([^{}]*)\}" % name, CODE).group(1)
    out, nxt = {}, 0
    for item in filter(None, (i.strip() for i in body.split(","))):
        key, _, value = (s.strip() for s in item.partition("="))
        out[key] = nxt = int(value, 0) if value else nxt
        nxt += 1
    return out


def test_constants_and_index_tables_match_the_header():
    for prefix in ("SEL_", "REG_", "FUSE_", "THIN_", "INSERT_KEEP", "CARVE_MAX_VIEWS"):
        want = defines(prefix)
        mine = {k: v for k, v in vars(api).items() if k.startswith(prefix) and isinstance(v, int)}
        assert want and mine == want, (prefix, mine, want)
    squash = lambda s: s.lower().replace("_", "")
    linalg = {squash(k[len("EF_LINALG_"):]): v for k, v in enum("ef_linalg_op").items()}
    assert {squash(k): v for k, v in api.ops.LINALG.items()} == linalg
    images = {squash(k[len("EF_IMG_"):]): v for k, v in enum("ef_image").items()}
    mine = {squash(k): which for k, (which, _, _) in api.ElasticFusion.IMAGES.items()}
    assert {("predict" + k if "predict" + k in images else k): v for k, v in mine.items()} == images
    # the tracker's buffers have no enum: the header lists them in the comment above ef_get_tracker_buffer
    listed = RAW[RAW.index("which: 0 vmap_curr"):RAW.index("int ef_get_tracker_buffer(")]
    for name, (which, _, _) in api.ElasticFusion.TRACKER.items():
        assert re.search(r"\b%d %s\b" % (which, name), listed), (which, name)
    assert sorted(w for w, _, _ in api.ElasticFusion.TRACKER.values()) == list(range(len(api.ElasticFusion.TRACKER)))
