// Spatial index and nearest-surfel / kNN queries on the map (ef_query_nearest / ef_query_knn, include/ef_hip.h; DESIGN.md §8b).
// Included at the end of ef_map_kernels.hip, after ef_labels.inc.  No frame kernel reads or writes anything here.
//   the index    a uniform grid hashed into a power-of-two number of buckets, built by a counting sort: k_query_count, the scan
//                (k_query_blocksum, k_scan_chunks, k_query_scan), k_query_scatter.  The scatter writes a cell-sorted copy of {x, y, z, conf}
//                and the original row, so that a bucket is one contiguous run of 16-byte records.
//   the query    eligible iff conf > min_conf and d2 <= r2, ordered by (d2, row).  The grid only selects candidates: every candidate is
//                distance-tested with the specification's own arithmetic, and a candidate counts only in the visit of its own cell, so that
//                buckets shared by several cells (hash collisions) cost time and nothing else.
namespace {

constexpr unsigned QUERY_NONE = 0xFFFFFFFFu;
constexpr float QUERY_CLAMP = 1048576.0f;   // cell coordinates are clamped to +-2^20 (everything beyond shares the boundary cells): the conversion to int stays defined, the box bounded
constexpr int QUERY_SCAN_TILE = 1024;       // buckets per workgroup of the scan's two local passes (256 threads x 4)

// the (clamped) cell coordinate of a world coordinate; NaN comes out as -QUERY_CLAMP (fmaxf drops it), callers test finiteness first
__device__ __forceinline__ int query_cell(float v, float inv_cell) {
  const float f = floorf(v * inv_cell);
  return (int)fminf(fmaxf(f, -QUERY_CLAMP), QUERY_CLAMP);
}
__device__ __forceinline__ unsigned query_hash(int x, int y, int z, unsigned mask) {
  return (((unsigned)x * 73856093u) ^ ((unsigned)y * 19349663u) ^ ((unsigned)z * 83492791u)) & mask;
}
__device__ __forceinline__ bool query_finite3(float x, float y, float z) {
  const float big = 3.402823466e38f;
  return fabsf(x) <= big && fabsf(y) <= big && fabsf(z) <= big;
}

// bucket sizes: one coalesced float4 per lane, one integer atomic per surfel (same-address adds of a wave are merged by the compiler)
__global__ void __launch_bounds__(BLK) k_query_count(const float4* __restrict__ pos_conf, unsigned n, float inv_cell, unsigned mask,
                                                     uint32_t* __restrict__ cells) {
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = pos_conf[i];
    if (!query_finite3(p.x, p.y, p.z)) continue;
    atomicAdd(&cells[query_hash(query_cell(p.x, inv_cell), query_cell(p.y, inv_cell), query_cell(p.z, inv_cell), mask)], 1u);
  }
}

// the scan in three launches: per-tile sums, their exclusive scan (k_scan_chunks, one workgroup), the tile-local scan on top of it (in place)
__global__ void __launch_bounds__(BLK) k_query_blocksum(const uint32_t* __restrict__ cells, uint32_t* __restrict__ tile_sum) {
  __shared__ unsigned lds[BLK / 64];
  const uint4 v = reinterpret_cast<const uint4*>(cells)[(size_t)blockIdx.x * BLK + threadIdx.x];
  unsigned tot;
  block_excl_scan(v.x + v.y + v.z + v.w, lds, tot);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(BLK) k_query_scan(uint32_t* __restrict__ cells, const uint32_t* __restrict__ tile_off) {
  __shared__ unsigned lds[BLK / 64];
  uint4* p = reinterpret_cast<uint4*>(cells) + (size_t)blockIdx.x * BLK + threadIdx.x;
  const uint4 v = *p;
  unsigned tot;
  const unsigned b = tile_off[blockIdx.x] + block_excl_scan(v.x + v.y + v.z + v.w, lds, tot);
  *p = make_uint4(b, b + v.x, b + v.x + v.y, b + v.x + v.y + v.z);
}

// cells[b] is bucket b's start on entry and its END on return (every surfel advances its bucket's cursor by one): bucket b is then the run
// [b ? cells[b - 1] : 0, cells[b]) of the sorted copy.  The order inside a bucket is whatever the atomics give; no result depends on it.
__global__ void __launch_bounds__(BLK) k_query_scatter(const float4* __restrict__ pos_conf, unsigned n, float inv_cell, unsigned mask,
                                                       uint32_t* __restrict__ cells, float4* __restrict__ sorted, uint32_t* __restrict__ rows) {
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = pos_conf[i];
    if (!query_finite3(p.x, p.y, p.z)) continue;
    const unsigned at = atomicAdd(&cells[query_hash(query_cell(p.x, inv_cell), query_cell(p.y, inv_cell), query_cell(p.z, inv_cell), mask)], 1u);
    sorted[at] = p;
    rows[at] = i;
  }
}

__device__ __forceinline__ bool query_less(float da, unsigned ra, float db, unsigned rb) { return da < db || (da == db && ra < rb); }

// The cell walk of one lane: lane `sub` of the L that share the query q visits cells sub, sub + L, ... of the query's box (flattened z fastest)
// and calls visit(d2, k) for every record k of the index that is eligible for q, once, in the visit of the record's own cell.  The one
// statement of the walk: query_walk below (k_query, k_register of ef_register.inc, k_outlier_join of ef_outlier.inc) and k_comp_hook
// (ef_components.inc) differ in the visitor only, and the argument below is the only proof that no eligible surfel is missed.  SELF (the
// self-joins only): the query is the index's own record `self`, which is passed over: a map row has exactly one record, so this excludes the
// query's own ROW and nothing else (a coincident surfel in another row stays a candidate).
template <int L, bool SELF, class Visit>
__device__ __forceinline__ void query_visit(const QueryArgs& A, float qx, float qy, float qz, unsigned sub, unsigned self, Visit&& visit) {
  if (A.n_sorted && query_finite3(qx, qy, qz)) {
    // The box: the cells of q -+ rw, rw = max_dist widened by 2^-21 of (max_dist + |q|) per axis.  It cannot miss an eligible surfel p:
    //   d2 <= r2 is decided in f32.  Adding non-negative terms never rounds below a term, so fl(fl(qx-px)^2) <= d2 <= r2 <= max_dist^2 (1+u),
    //   u = 2^-24, hence |qx - px| <= max_dist (1 + 2.1 u) in exact arithmetic (products that underflow: |qx - px| < 1e-18, the last term of rw);
    //   fl(qx - rw) <= (qx - rw) + u |qx - rw| <= qx - max_dist (1 + 2.1 u) <= px, because rw - max_dist >= 7 u (max_dist + |qx|) after its own roundings;
    //   rounding and floor are monotonic, so cell(fl(qx - rw)) <= cell(px), the same function on both sides (clamp included); likewise above.
    const float wx = A.max_dist + ((A.max_dist + fabsf(qx)) * 4.76837158e-7f + 1e-18f);
    const float wy = A.max_dist + ((A.max_dist + fabsf(qy)) * 4.76837158e-7f + 1e-18f);
    const float wz = A.max_dist + ((A.max_dist + fabsf(qz)) * 4.76837158e-7f + 1e-18f);
    const int x0 = query_cell(qx - wx, A.inv_cell), x1 = query_cell(qx + wx, A.inv_cell);
    const int y0 = query_cell(qy - wy, A.inv_cell), y1 = query_cell(qy + wy, A.inv_cell);
    const int z0 = query_cell(qz - wz, A.inv_cell), z1 = query_cell(qz + wz, A.inv_cell);
    const unsigned nz = (unsigned)(z1 - z0 + 1), ny = (unsigned)(y1 - y0 + 1), nx = (unsigned)(x1 - x0 + 1);
    const unsigned ncell = nx * ny * nz;   // at most (2 QUERY_MAX_RATIO + 3)^3: the host refuses larger ratios
    for (unsigned ci = sub; ci < ncell; ci += L) {
      const unsigned cxy = ci / nz;
      const int cz = z0 + (int)(ci - cxy * nz);
      const unsigned cxi = cxy / ny;
      const int cy = y0 + (int)(cxy - cxi * ny), cx = x0 + (int)cxi;
      const unsigned b = query_hash(cx, cy, cz, A.mask);
      const unsigned e1 = A.cells[b], e0 = b ? A.cells[b - 1] : 0u;
      for (unsigned k = e0; k < e1; ++k) {
        if (SELF && k == self) continue;
        const float4 p = A.sorted[k];
        const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
        const float d2 = ((dx * dx + dy * dy) + dz * dz);
        if (!(p.w > A.min_conf && d2 <= A.r2)) continue;
        if (query_cell(p.x, A.inv_cell) != cx || query_cell(p.y, A.inv_cell) != cy || query_cell(p.z, A.inv_cell) != cz) continue;
        visit(d2, k);
      }
    }
  }
}

// query_visit with the top-K visitor: the lane keeps its own K best as sorted (d2, row) keys in bd / br (initialised by the caller) and counts
// every eligible surfel in cnt.
template <int L, int K, bool SELF = false>
__device__ __forceinline__ void query_walk(const QueryArgs& A, float qx, float qy, float qz, unsigned sub, float (&bd)[K], unsigned (&br)[K],
                                           unsigned& cnt, unsigned self = 0u) {
  query_visit<L, SELF>(A, qx, qy, qz, sub, self, [&](float d, unsigned k) {
    ++cnt;
    unsigned r = A.rows[k];
    if (!query_less(d, r, bd[K - 1], br[K - 1])) return;
    bd[K - 1] = d;
    br[K - 1] = r;
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
      if (query_less(bd[j], br[j], bd[j - 1], br[j - 1])) {
        d = bd[j]; bd[j] = bd[j - 1]; bd[j - 1] = d;
        r = br[j]; br[j] = br[j - 1]; br[j - 1] = r;
      }
    }
  });
}

// L lanes share a query: every lane walks its share of the box (query_walk) and keeps its own K best in registers (K is a template parameter:
// every index is a compile-time constant, nothing spills).  The group's
// lists are then merged K times by a butterfly minimum on the key; the lane that owns the winner pops it.  Rows are unique across the group
// because a surfel is only ever accepted in the visit of its own cell.
template <int L, int K>
__global__ void __launch_bounds__(BLK) k_query(const QueryArgs A) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned qi = t / L, sub = t % L;
  const bool live = qi < A.n;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) {
    qx = A.points[(size_t)qi * 3];
    qy = A.points[(size_t)qi * 3 + 1];
    qz = A.points[(size_t)qi * 3 + 2];
  }
  float bd[K];
  unsigned br[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { bd[j] = __builtin_inff(); br[j] = QUERY_NONE; }
  unsigned cnt = 0;
  if (live) query_walk<L, K>(A, qx, qy, qz, sub, bd, br, cnt);
  // merge the group's lists (every lane of the wave takes part in the shuffles, live or not)
  if (L > 1) {
#pragma unroll
    for (int m = 1; m < L; m <<= 1) cnt += __shfl_xor(cnt, m, L);
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float d = bd[0];
    unsigned r = br[0];
    if (L > 1) {
#pragma unroll
      for (int m = 1; m < L; m <<= 1) {
        const float od = __shfl_xor(d, m, L);
        const unsigned orow = __shfl_xor(r, m, L);
        if (query_less(od, orow, d, r)) { d = od; r = orow; }
      }
      if (r != QUERY_NONE && r == br[0]) {
#pragma unroll
        for (int i = 0; i + 1 < K; ++i) { bd[i] = bd[i + 1]; br[i] = br[i + 1]; }
        bd[K - 1] = __builtin_inff();
        br[K - 1] = QUERY_NONE;
      }
    } else {
      d = bd[j];
      r = br[j];
    }
    if (live && sub == 0) {
      const size_t o = (size_t)qi * A.k + j;
      if (j < A.k) {
        A.row[o] = r;
        if (A.dist2) A.dist2[o] = d;
      }
      if (K == 1) {   // the other two streams are touched for the winner only, and only when asked for
        if (A.id) A.id[qi] = r != QUERY_NONE ? __float_as_uint(A.map.col_time[r].y) : 0u;
        if (A.plane) {
          float pl = 0.f;
          if (r != QUERY_NONE) {
            const float4 p = A.map.pos_conf[r], nr = A.map.nrm_rad[r];
            pl = (((qx - p.x) * nr.x + (qy - p.y) * nr.y) + (qz - p.z) * nr.z);
          }
          A.plane[qi] = pl;
        }
      }
    }
  }
  if (live && sub == 0 && A.count) A.count[qi] = cnt;
}

template <int L, int K>
void query_launch(const QueryArgs& a, hipStream_t s) {
  static_assert(BLK % L == 0 && 64 % L == 0, "a group lies inside one wave");
  const unsigned per = BLK / L;
  hipLaunchKernelGGL((k_query<L, K>), dim3((a.n + per - 1) / per), dim3(BLK), 0, s, a);
}

}  // namespace

unsigned query_buckets(unsigned n) {
  unsigned nb = QUERY_SCAN_TILE;
  while (nb < n && nb < (1u << 22)) nb <<= 1;
  return nb;
}

// cells: nb words, zero on entry; tile_sum: 2 (nb / QUERY_SCAN_TILE + 1) words (the tiles' sums, their total, their offsets); sorted / rows: n records
void query_build(SurfelSoA map, unsigned n, float inv_cell, unsigned nb, uint32_t* cells, uint32_t* tile_sum, float4* sorted, uint32_t* rows,
                 hipStream_t s) {
  if (!n) return;
  const int g = min(ceil_div((int)n, BLK), 8192);
  const unsigned tiles = nb / QUERY_SCAN_TILE;
  hipLaunchKernelGGL(k_query_count, dim3(g), dim3(BLK), 0, s, (const float4*)map.pos_conf, n, inv_cell, nb - 1, cells);
  hipLaunchKernelGGL(k_query_blocksum, dim3(tiles), dim3(BLK), 0, s, (const uint32_t*)cells, tile_sum);
  hipLaunchKernelGGL(k_scan_chunks, dim3(1), dim3(1024), 0, s, (const uint32_t*)tile_sum, (const unsigned*)nullptr, tiles, tile_sum + tiles + 1,
                     tile_sum + tiles, (unsigned*)nullptr, 0u, (int*)nullptr, 1u);
  hipLaunchKernelGGL(k_query_scan, dim3(tiles), dim3(BLK), 0, s, cells, (const uint32_t*)(tile_sum + tiles + 1));
  hipLaunchKernelGGL(k_query_scatter, dim3(g), dim3(BLK), 0, s, (const float4*)map.pos_conf, n, inv_cell, nb - 1, cells, sorted, rows);
}

void query_run(const QueryArgs& a, int k, int lanes, hipStream_t s) {
  if (!a.n) return;
  if (lanes == 0) lanes = k == 1 ? 16 : 1;   // measured at 1 M queries on both maps (profiles/r12_query_kernel_times.txt)
  if (k == 1) {
    if (lanes == 1) query_launch<1, 1>(a, s);
    else if (lanes == 16) query_launch<16, 1>(a, s);
    else if (lanes == 64) query_launch<64, 1>(a, s);
    else query_launch<8, 1>(a, s);
  } else if (k <= 4) {
    if (lanes == 1) query_launch<1, 4>(a, s); else query_launch<8, 4>(a, s);
  } else if (k <= 8) {
    if (lanes == 1) query_launch<1, 8>(a, s); else query_launch<8, 8>(a, s);
  } else {
    if (lanes == 1) query_launch<1, 16>(a, s); else query_launch<8, 16>(a, s);
  }
}
