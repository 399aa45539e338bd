"""The label code's index arithmetic, executed WITHOUT a GPU: wave_partition_point (the 64-way search behind k_ids_assign and
k_labels_align) and the row-from-float statements of k_labels_align's flat copy are cut out of elasticfusion_amd/csrc/ef_labels.inc and
compiled for the host over tests/wave_emu/hip/hip_runtime.h (tests/wave_emu/label_search_host.cpp: 64 host threads, one per lane, that meet
at every ballot).  The search must return the boundary for EVERY range up to 70 rows and every boundary in it, and around the probe steps
of larger ranges, without ever probing outside [lo, hi); the row must be f / C for every C in 1 .. 256 and every f of a tile.  This pins
the logic of the product's own text; the compiled kernels are tests/test_gpu_label_edges.py's business."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elasticfusion_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "wave_emu")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("label_search"))
    src = open(os.path.join(CSRC, "ef_labels.inc")).read()
    a, b = src.index("template <class Pred>"), src.index("// One workgroup: find the zero suffix")
    search = src[a:b]
    assert "wave_partition_point" in search and "__ballot" in search and search.count("while (lo < hi)") == 1
    a, b = src.index("      unsigned rr = "), src.index("      const unsigned s = s_src[rr];")
    row_of = src[a:b]
    assert row_of.count(";") == 3 and "--rr" in row_of and "++rr" in row_of, row_of
    paths = []
    for name, text in (("partition_cut.inc", search), ("row_of_cut.inc", row_of)):
        paths.append(os.path.join(tmp, name))
        open(paths[-1], "w").write(text)
    so = os.path.join(tmp, "label_search.so")
    cmd = ["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I" + EMU, '-DPARTITION_SOURCE="%s"' % paths[0],
           '-DROW_OF_SOURCE="%s"' % paths[1], os.path.join(EMU, "label_search_host.cpp"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return C.CDLL(so)


def search_cases():
    cases = [(0, n, b) for n in range(71) for b in range(n + 1)]                      # every range from 0, every boundary
    cases += [(lo, lo + n, lo + b) for lo in (1, 63, 64, 1000) for n in (0, 1, 63, 64, 65) for b in range(n + 1)]
    for n in (127, 128, 129, 4095, 4096, 4097, 64 ** 3 - 1, 64 ** 3, 64 ** 3 + 1, 2097152 + 300, 4 * 1024 * 1024):
        step = (n + 63) // 64
        bs = {0, 1, 63, 64, 65, n // 2, n - 65, n - 64, n - 63, n - 1, n}
        bs |= {k * step + d for k in (1, 2, 31, 63, 64) for d in (-1, 0, 1)}
        cases += [(0, n, b) for b in sorted(bs) if 0 <= b <= n]
    return np.array(cases, np.uint32)


def test_the_search_returns_the_boundary_and_stays_inside_the_range(lib):
    cases = search_cases()
    out = np.full((64, len(cases)), 0xFFFFFFFF, np.uint32)
    outside = C.c_uint(7)
    lib.run_partition(cases.ctypes.data_as(C.c_void_p), C.c_int(len(cases)), out.ctypes.data_as(C.c_void_p), C.byref(outside))
    assert (out == out[0]).all(), "the lanes disagree"
    bad = np.flatnonzero(out[0] != cases[:, 2])
    assert len(bad) == 0, (len(bad), cases[bad[:5]], out[0][bad[:5]])
    assert outside.value == 0, outside.value


def test_the_flat_copy_finds_the_row_of_every_float(lib):
    lib.run_row_of.restype = C.c_uint
    uncorrected = C.c_uint(0)
    assert lib.run_row_of(C.c_uint(1), C.c_uint(256), C.c_uint(256), C.byref(uncorrected)) == 0
    assert uncorrected.value > 0      # the estimate alone is not enough: the correction has work to do
