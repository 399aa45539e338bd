"""The depth half of a z-buffer key (elasticfusion_amd/csrc/ef_zkey.hpp), swept on the host.

Since round 9 the association and the keep-test of clean() read a texel's depth OUT OF THE KEY (efm::KeyedIndex) instead of from a resolved
vertex map, so depth_of_key(depth_key(z)) has to give z back bit for bit — for every float, not only the depths a splat lets through — and
depth_key has to keep the order of the floats (nearest wins the atomicMin).  The one exception is the pair of zeros: -0 and +0 compare
equal under the reference's depth test, so they share one key (the lower id wins the tie) and read back as +0.  The two one-line functions are compiled into a small host
translation unit with g++ (the header is plain C++ outside hipcc) and called through ctypes.  No GPU.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elasticfusion_amd", "csrc")

TU = r"""
#include "ef_zkey.hpp"
extern "C" void keys_of(const float* z, uint32_t* k, int n) { for (int i = 0; i < n; ++i) k[i] = efm::depth_key(z[i]); }
extern "C" void depths_of(const uint32_t* k, float* z, int n) { for (int i = 0; i < n; ++i) z[i] = efm::depth_of_key(k[i]); }
"""


@pytest.fixture(scope="module")
def zkey(tmp_path_factory):
    d = tmp_path_factory.mktemp("zkey")
    src, so = d / "zkey_host.cpp", d / "libzkey_host.so"
    src.write_text(TU)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))

    def keys_of(z):
        z = np.ascontiguousarray(z, np.float32)
        k = np.zeros(z.shape, np.uint32)
        lib.keys_of(z.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), C.c_int(z.size))
        return k

    def depths_of(k):
        k = np.ascontiguousarray(k, np.uint32)
        z = np.zeros(k.shape, np.float32)
        lib.depths_of(k.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), C.c_int(k.size))
        return z

    return keys_of, depths_of


def _bits(*patterns):
    return np.array(patterns, np.uint32).view(np.float32)


def sweep():
    """float bit patterns: the named corners, their neighbours, every exponent, a dense stretch around the depth cut-off and a random lot"""
    rng = np.random.RandomState(0xEF09)
    f32 = np.float32
    named = np.concatenate([
        _bits(0x00000000, 0x80000000),                                    # +0, -0
        _bits(0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF),            # smallest and largest denormals
        _bits(0x00800000, 0x80800000),                                    # smallest normals
        _bits(0x7F7FFFFF, 0xFF7FFFFF),                                    # largest finite values
        _bits(0x7F800000, 0xFF800000),                                    # infinities (no splat writes them; the pair must still invert)
        np.array([3.0, 20.0, 0.3, 1.0, -1.0], f32),                       # the depth cut-off (ef_config.depth_cut), maxDepthProcessed, near gate
    ])
    cut = np.array([3.0], f32).view(np.uint32)[0]
    around_cut = (cut + np.arange(-4096, 4097)).astype(np.uint32).view(np.float32)
    exps = (np.arange(0, 255, dtype=np.uint32) << 23)
    every_exp = np.concatenate([(exps | m).view(np.float32) for m in (0, 1, 0x400000, 0x7FFFFF)])
    every_exp = np.concatenate([every_exp, -every_exp])
    rand = rng.randint(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    rand = rand[(rand & 0x7F800000) != 0x7F800000].view(np.float32)     # finite ones (NaN payloads are checked on their own below)
    metric = rng.uniform(0.0, 20.0, 1 << 18).astype(f32)                   # where depths actually lie
    return np.concatenate([named, around_cut, every_exp, rand, metric])


MINUS_ZERO, PLUS_ZERO = 0x80000000, 0x00000000


def test_depth_of_key_inverts_depth_key_bit_for_bit(zkey):
    """... for every float but -0, which shares +0's key and comes back as +0 (the one consumer that hands the sign of a zero on,
    k_depth_resolve, evaluates the winner's fragment again: tests/test_gpu_predict_edges.py, surface_signed_zeros_*)"""
    keys_of, depths_of = zkey
    z = sweep()
    back = depths_of(keys_of(z))
    minus_zero = z.view(np.uint32) == MINUS_ZERO
    assert minus_zero.sum() >= 1 and (z.view(np.uint32) == PLUS_ZERO).sum() >= 1
    assert np.array_equal(back.view(np.uint32)[~minus_zero], z.view(np.uint32)[~minus_zero])
    assert (back.view(np.uint32)[minus_zero] == PLUS_ZERO).all()
    # every bit pattern of a stretch of NaN payloads and the whole top of the key space
    nan = (np.uint32(0x7F800001) + np.arange(0, 1 << 16, dtype=np.uint32)).view(np.float32)
    assert np.array_equal(depths_of(keys_of(nan)).view(np.uint32), nan.view(np.uint32))
    k = np.arange(0xFFFF0000, 0x100000000, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(keys_of(depths_of(k)), k)                         # ... and depth_key inverts depth_of_key
    # around the zeros: every key but the one -0 used to have (0x7FFFFFFF, which no depth maps onto any more) comes back
    k = np.arange(0x7FFF0000, 0x80010000, dtype=np.uint64).astype(np.uint32)
    back = keys_of(depths_of(k))
    assert np.array_equal(back[k != 0x7FFFFFFF], k[k != 0x7FFFFFFF]) and back[k == 0x7FFFFFFF][0] == 0x80000000


def test_depth_key_keeps_the_order_of_the_floats(zkey):
    keys_of, _ = zkey
    z = sweep()
    z = np.unique(z[np.isfinite(z)])                                        # ascending; -0 == +0 collapse to one of them here
    k = keys_of(z).astype(np.int64)
    assert (np.diff(k) > 0).all()
    # no finite or infinite depth maps onto the high word of ZBUF_EMPTY
    assert (keys_of(sweep()) != 0xFFFFFFFF).all() and keys_of(_bits(0x7F800000))[0] != 0xFFFFFFFF


def test_the_two_zeros_tie(zkey):
    """The reference's depth test is `z < zbuf` on floats: -0 and +0 compare equal, so neither beats the other and the earlier draw — the
    lower surfel id, the low word of the 64-bit key — keeps the pixel.  One key for both, strictly between the negative and the positive
    depths; the neighbours of zero keep theirs."""
    keys_of, depths_of = zkey
    kz = keys_of(_bits(MINUS_ZERO, PLUS_ZERO))
    assert kz[0] == kz[1] == 0x80000000
    assert depths_of(kz).view(np.uint32).tolist() == [PLUS_ZERO, PLUS_ZERO]
    around = keys_of(_bits(0x80000001, MINUS_ZERO, PLUS_ZERO, 0x00000001)).astype(np.int64)     # -denorm_min, -0, +0, +denorm_min
    assert around[0] < around[1] == around[2] < around[3]
    # 64-bit keys as the splat builds them: at equal depth halves the id decides, whatever the signs of the zeros
    def key64(z_bits, sid):
        return (int(keys_of(_bits(z_bits))[0]) << 32) | sid
    assert key64(PLUS_ZERO, 3) < key64(MINUS_ZERO, 7) and key64(MINUS_ZERO, 3) < key64(PLUS_ZERO, 7)
    assert key64(0x80000001, 9) < key64(PLUS_ZERO, 0) < key64(0x00000001, 0)
