"""The query specification restated in numpy (include/ef_hip.h, ef_query_nearest / ef_query_knn), shared by test_gpu_query.py and
test_gpu_query_variants.py: the exhaustive scan, the bit comparison, and the index's cell and hash functions (csrc/ef_query.inc)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = 0xFFFFFFFF
F = np.float32


def default_cell():
    hdr = open(os.path.join(ROOT, "include", "ef_hip.h")).read()
    return float(re.search(r"#define EF_QUERY_DEFAULT_CELL ([0-9.]+)f", hdr).group(1))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bits_equal(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    d = bits(a) != bits(b)
    assert not d.any(), (what, int(d.sum()), np.argwhere(d)[:5], a[d][:5], b[d][:5])


def brute(points, surfels, max_dist, min_conf, k=1, dtype=np.float32, chunk=64):
    """exhaustive restatement: (rows n x k, d2 n x k, plane n (of the first), count n)"""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3).astype(dtype)
    S = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
    P, conf, N = S[:, :3].astype(dtype), S[:, 3], S[:, 8:11].astype(dtype)
    r2 = F(max_dist) * F(max_dist) if dtype == np.float32 else np.float64(F(max_dist)) ** 2
    n = len(pts)
    rows = np.full((n, k), MISS, np.uint32)
    d2s = np.full((n, k), np.inf, dtype)
    plane = np.zeros(n, dtype)
    count = np.zeros(n, np.uint32)
    cok = conf > F(min_conf)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, n, chunk):
            q = pts[a:a + chunk]
            dx, dy, dz = (q[:, None, j] - P[None, :, j] for j in range(3)) if len(P) else (np.zeros((len(q), 0), dtype),) * 3
            d2 = (dx * dx + dy * dy) + dz * dz
            ok = cok[None, :] & (d2 <= r2)
            count[a:a + chunk] = ok.sum(1)
            if k == 1:
                if not len(P):
                    continue
                m = np.where(ok, d2, np.inf)
                w = np.argmin(m, 1)   # the first minimum = the lower row
                hit = ok[np.arange(len(q)), w]
                rows[a:a + chunk, 0] = np.where(hit, w, MISS)
                d2s[a:a + chunk, 0] = np.where(hit, d2[np.arange(len(q)), w], np.inf)
            else:
                for i in range(len(q)):
                    e = np.nonzero(ok[i])[0]                      # ascending rows
                    e = e[np.argsort(d2[i, e], kind="stable")][:k]   # stable: ties keep the lower row first
                    rows[a + i, :len(e)] = e
                    d2s[a + i, :len(e)] = d2[i, e]
        hit = rows[:, 0] != MISS
        w = rows[hit, 0].astype(np.int64)
        d = pts[hit] - P[w]
        plane[hit] = (d[:, 0] * N[w, 0] + d[:, 1] * N[w, 1]) + d[:, 2] * N[w, 2]
    return rows, d2s, plane, count


def cells_of(xyz, cell):
    """query_cell per axis (n x 3 int64): floor of the f32 product with f32(1) / f32(cell) (a product, not a quotient), clamped to +-2^20"""
    inv = F(1) / F(cell)
    f = np.floor(np.ascontiguousarray(xyz, F).reshape(-1, 3) * inv)
    return np.clip(f, F(-1048576.0), F(1048576.0)).astype(np.int64)


def hash_of(cells, mask):
    """query_hash: the three coordinates as 32-bit words times their primes (mod 2^32), xor-ed, masked to the bucket count"""
    c = np.asarray(cells, np.int64) & 0xFFFFFFFF
    m = 0xFFFFFFFF
    return ((((c[:, 0] * 73856093) & m) ^ ((c[:, 1] * 19349663) & m) ^ ((c[:, 2] * 83492791) & m)) & mask).astype(np.int64)


def buckets_of(n):
    """query_buckets: the power of two >= n between 2^10 and 2^22"""
    nb = 1024
    while nb < n and nb < (1 << 22):
        nb <<= 1
    return nb
