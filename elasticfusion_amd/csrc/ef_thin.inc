// Thin the map to one surfel per voxel (ef_map_thin / ef_map_thin_select, include/ef_hip.h; DESIGN.md §8f).  Included at the end of
// ef_map_kernels.hip, after ef_insert.inc.  It uses the query's index (ef_query.inc: query_cell, the cell-sorted copy) built at the thin's
// cell and the selection's flag -> count -> scan -> scatter chain (ef_select.inc) unchanged.  No frame kernel reads or writes anything here.
//   flags     k_thin_flags: one wave per bucket of the index.  A bucket is a contiguous run of {x, y, z, conf} + rows[] in arbitrary order,
//             shared by the cells that collide in the hash, so every record's cell is recomputed.  The cells of a bucket are taken in
//             ascending (x, y, z) order, one per round: a sweep in strides of 64 forms the key (primary as a monotone uint32, ~row) of every
//             participant of the round's cell and the wave takes the maximum; a second sweep stores one byte per participant of that cell
//             (representative or removed) and finds the next cell, the lowest above the round's.
//   counts    k_select_count + k_scan_chunks over the bytes (flags_count of ef_select.inc), as the insert does; lists and the erase are the selection's.
// Work: a bucket of L records and D distinct cells costs 1 + 2 D sweeps of ceil(L / 64) steps: linear in a cell's occupancy.  Every loop is
// bounded by the bucket's length (sweeps) or its number of distinct cells (rounds: the round's cell strictly ascends).  No workgroup reads
// what another writes (the index, the participant bytes and the map are read, the two byte arrays are written), and there are no atomics.
namespace {

constexpr int THIN_G = 64;                  // lanes per bucket: one wave
constexpr int THIN_NO_CELL = 0x7FFFFFFF;    // above every clamped cell coordinate

// a cell as an ordered pair: x, then y and z (both shifted to 0 .. 2^21) in one word
struct ThinCell {
  int x;
  unsigned long long yz;
};
__device__ __forceinline__ ThinCell thin_cell(float4 p, float inv_cell) {
  const int cy = query_cell(p.y, inv_cell), cz = query_cell(p.z, inv_cell);
  return ThinCell{query_cell(p.x, inv_cell), ((unsigned long long)(unsigned)(cy + (1 << 20)) << 32) | (unsigned)(cz + (1 << 20))};
}
__device__ __forceinline__ bool thin_cell_less(const ThinCell& a, const ThinCell& b) { return a.x < b.x || (a.x == b.x && a.yz < b.yz); }
__device__ __forceinline__ bool thin_cell_same(const ThinCell& a, const ThinCell& b) { return a.x == b.x && a.yz == b.yz; }

__device__ __forceinline__ unsigned long long thin_uniform(unsigned long long v) {
  return ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
}
// the wave's lowest cell, in every lane (and scalar)
__device__ __forceinline__ ThinCell thin_wave_min(ThinCell c) {
#pragma unroll
  for (int m = 1; m < THIN_G; m <<= 1) {
    const ThinCell o{__shfl_xor(c.x, m, THIN_G), __shfl_xor(c.yz, m, THIN_G)};
    if (thin_cell_less(o, c)) c = o;
  }
  return ThinCell{__builtin_amdgcn_readfirstlane(c.x), thin_uniform(c.yz)};
}
__device__ __forceinline__ unsigned long long thin_wave_max(unsigned long long k) {
#pragma unroll
  for (int m = 1; m < THIN_G; m <<= 1) {
    const unsigned long long o = __shfl_xor(k, m, THIN_G);
    if (o > k) k = o;
  }
  return thin_uniform(k);
}

// The f32 order as an unsigned order, on the bits alone (no float comparison: denormals are ordered like every other value): -0 = +0, every
// NaN = -inf.  Never 0: the lowest value, -inf, maps to 0x007FFFFF.
__device__ __forceinline__ unsigned thin_mono(float v) {
  unsigned u = __float_as_uint(v);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) u = 0xFF800000u;   // NaN -> -inf
  if ((u << 1) == 0u) u = 0u;                            // -0 -> +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the key of record k if it participates, else 0: primary in the high word, ~row in the low word (the maximum = the highest primary, then the lowest row)
__device__ __forceinline__ unsigned long long thin_key(const ThinArgs& A, float4 p, unsigned row) {
  if (row >= A.n || (A.part && !A.part[row])) return 0ull;
  unsigned prim = 1u;   // THIN_KEEP_FIRST: a constant
  if (A.keep == THIN_KEEP_MAX_CONF) prim = thin_mono(p.w);
  else if (A.keep == THIN_KEEP_NEWEST) prim = thin_mono(A.q.map.col_time[row].w);
  return ((unsigned long long)prim << 32) | (unsigned)~row;
}

__global__ void __launch_bounds__(BLK) k_thin_flags(const ThinArgs A) {
  const unsigned b = blockIdx.x * (BLK / THIN_G) + threadIdx.x / THIN_G;   // the wave's bucket
  const unsigned lane = threadIdx.x % THIN_G;
  if (b > A.q.mask) return;
  const unsigned e1 = A.q.cells[b], e0 = b ? A.q.cells[b - 1] : 0u;
  if (e1 <= e0 || e1 > A.q.n_sorted) return;   // (an empty bucket: two loads)
  const float inv_cell = A.q.inv_cell;
  ThinCell next{THIN_NO_CELL, 0ull};
  for (unsigned k = e0 + lane; k < e1; k += THIN_G) {
    const ThinCell c = thin_cell(A.q.sorted[k], inv_cell);
    if (thin_cell_less(c, next)) next = c;
  }
  next = thin_wave_min(next);
  // one round per distinct cell of the bucket, in ascending order: at most e1 - e0 of them
  for (unsigned round = 0; round < e1 - e0 && next.x != THIN_NO_CELL; ++round) {
    const ThinCell cur = next;
    unsigned long long best = 0ull;
    for (unsigned k = e0 + lane; k < e1; k += THIN_G) {
      const float4 p = A.q.sorted[k];
      if (!thin_cell_same(thin_cell(p, inv_cell), cur)) continue;
      const unsigned long long key = thin_key(A, p, A.q.rows[k]);
      if (key > best) best = key;
    }
    best = thin_wave_max(best);
    const unsigned winner = ~(unsigned)best;   // (best == 0: the cell has no participant and nothing is stored)
    next = ThinCell{THIN_NO_CELL, 0ull};
    for (unsigned k = e0 + lane; k < e1; k += THIN_G) {
      const float4 p = A.q.sorted[k];
      const ThinCell c = thin_cell(p, inv_cell);
      if (thin_cell_same(c, cur)) {
        const unsigned row = A.q.rows[k];
        if (thin_key(A, p, row) != 0ull) {
          if (row == winner) {
            if (A.rep) A.rep[row] = 1;
          } else if (A.removed) {
            A.removed[row] = 1;
          }
        }
      } else if (thin_cell_less(cur, c) && thin_cell_less(c, next)) {
        next = c;
      }
    }
    next = thin_wave_min(next);
  }
}

}  // namespace

void thin_flags(const ThinArgs& a, hipStream_t s) {
  static_assert(BLK % THIN_G == 0 && QUERY_SCAN_TILE % (BLK / THIN_G) == 0, "the buckets (a multiple of the scan's tile) are whole workgroups of waves");
  if (!a.n || !a.q.n_sorted) return;
  hipLaunchKernelGGL(k_thin_flags, dim3((a.q.mask + 1) / (BLK / THIN_G)), dim3(BLK), 0, s, a);
}
