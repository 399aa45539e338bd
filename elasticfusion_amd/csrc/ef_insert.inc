// Insert surfels into the map (ef_map_insert, include/ef_hip.h; DESIGN.md §8e).  Included at the end of ef_map_kernels.hip, after
// ef_select.inc, whose chunk counts (k_select_count, select_block_rank) it uses beside the query's cell walk (query_walk) and k_scan_chunks.
// No frame kernel reads or writes anything here.
//   gate      k_insert_gate: 16 lanes share a record (the query's measured choice): the moved position, query_walk<16, 1> on the index of the
//             OLD map, the butterfly minimum of k_query, then lane 0 of the group tests the winner's stored normal and writes one flag byte
//             (1 = insert), one duplicate byte and match_row.  k_insert_finite (gate off): one record per lane, the flag is the finiteness of
//             the moved position.
//   offsets   k_select_count per SELECT_ROW records, k_scan_chunks; the same pair once more over the gate's duplicate bytes, for the count alone.
//   scatter   k_insert_scatter: a workgroup takes the SELECT_ROW records of one chunk.  One lane per record ranks the flags (ballot + mbcnt),
//             then three lanes per record move one 16-byte word each: consecutive lanes read consecutive words of the records, and the words of
//             consecutive inserted records are consecutive in each of the three streams.
// The transform is evaluated twice (gate and scatter) with the same expression on the same inputs instead of being carried through memory.
// Nothing waits for another workgroup, every loop is bounded by the record count or the walk's box, and there are no atomics.
namespace {

__device__ __forceinline__ float4 insert_move_pos(const InsertArgs& A, float4 v) {
  if (!A.moved) return v;
  return make_float4(((A.R[0] * v.x + A.R[1] * v.y) + A.R[2] * v.z) + A.t[0], ((A.R[3] * v.x + A.R[4] * v.y) + A.R[5] * v.z) + A.t[1],
                     ((A.R[6] * v.x + A.R[7] * v.y) + A.R[8] * v.z) + A.t[2], v.w);
}
__device__ __forceinline__ float4 insert_move_nrm(const InsertArgs& A, float4 v) {
  if (!A.moved) return v;
  return make_float4((A.R[0] * v.x + A.R[1] * v.y) + A.R[2] * v.z, (A.R[3] * v.x + A.R[4] * v.y) + A.R[5] * v.z,
                     (A.R[6] * v.x + A.R[7] * v.y) + A.R[8] * v.z, v.w);
}

template <int L>
__global__ void __launch_bounds__(BLK) k_insert_gate(const InsertArgs A) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned qi = t / L, sub = t % L;
  const bool live = qi < A.n;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) p = insert_move_pos(A, A.rec[(size_t)qi * 3]);
  float bd[1] = {__builtin_inff()};
  unsigned br[1] = {QUERY_NONE};
  unsigned cnt = 0;
  if (live) query_walk<L, 1>(A.q, p.x, p.y, p.z, sub, bd, br, cnt);   // (a non-finite position walks nothing)
  float d = bd[0];
  unsigned r = br[0];
  // every lane of the wave takes part in the shuffles, live or not
#pragma unroll
  for (int m = 1; m < L; m <<= 1) {
    const float od = __shfl_xor(d, m, L);
    const unsigned orow = __shfl_xor(r, m, L);
    if (query_less(od, orow, d, r)) { d = od; r = orow; }
  }
  if (!live || sub != 0) return;
  bool dup = r != QUERY_NONE;
  if (dup && A.min_normal_cos > -1.0f) {   // only the NEAREST eligible surfel is asked
    const float4 m = insert_move_nrm(A, A.rec[(size_t)qi * 3 + 2]), ns = A.q.map.nrm_rad[r];
    dup = ((m.x * ns.x + m.y * ns.y) + m.z * ns.z) >= A.min_normal_cos;   // NaN: not a duplicate
  }
  A.flags[qi] = (query_finite3(p.x, p.y, p.z) && !dup) ? 1 : 0;
  A.dup[qi] = dup ? 1 : 0;
  if (A.match_row) A.match_row[qi] = dup ? r : QUERY_NONE;
}

__global__ void __launch_bounds__(BLK) k_insert_finite(const InsertArgs A) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const float4 p = insert_move_pos(A, A.rec[(size_t)i * 3]);
  A.flags[i] = query_finite3(p.x, p.y, p.z) ? 1 : 0;
  if (A.match_row) A.match_row[i] = QUERY_NONE;
}

__global__ void __launch_bounds__(BLK) k_insert_scatter(const InsertArgs A, SurfelSoA dst) {
  __shared__ unsigned lds[BLK / 64];
  __shared__ unsigned s_pos[SELECT_ROW];
  const unsigned r0 = blockIdx.x * SELECT_ROW, i = r0 + threadIdx.x;
  const bool f = i < A.n && A.flags[i] != 0;
  unsigned before;
  select_block_rank(f, lds, before);
  const unsigned pos = A.count_before + (A.chunk_offset[blockIdx.x] + before);   // the host has checked the total against the capacity
  s_pos[threadIdx.x] = f ? pos : QUERY_NONE;
  if (i < A.n && A.new_row) A.new_row[i] = f ? pos : QUERY_NONE;
  __syncthreads();
  const unsigned words = min((unsigned)SELECT_ROW, A.n - r0) * 3;
#pragma unroll
  for (int trip = 0; trip < 3; ++trip) {
    const unsigned w = trip * BLK + threadIdx.x;
    if (w >= words) break;
    const unsigned k = w / 3, part = w - k * 3;
    const unsigned at = s_pos[k];
    if (at == QUERY_NONE) continue;
    float4 v = A.rec[(size_t)r0 * 3 + w];
    if (part == 0) {
      dst.pos_conf[at] = insert_move_pos(A, v);
    } else if (part == 1) {
      v.y = 0.f;   // the ID lane: zero bits, numbered by the next ID-consuming call
      if (A.init_time != INSERT_KEEP) v.z = (float)A.init_time;
      if (A.last_time != INSERT_KEEP) v.w = (float)A.last_time;
      dst.col_time[at] = v;
    } else {
      dst.nrm_rad[at] = insert_move_nrm(A, v);
    }
  }
}

}  // namespace

void insert_gate(const InsertArgs& a, const SelectScratch& sc, uint32_t* total, const SelectScratch& dup_sc, uint32_t* dup_total, hipStream_t s) {
  if (a.n) {
    if (a.gate) {
      constexpr unsigned per = BLK / 16;
      hipLaunchKernelGGL((k_insert_gate<16>), dim3((a.n + per - 1) / per), dim3(BLK), 0, s, a);
    } else {
      hipLaunchKernelGGL(k_insert_finite, dim3((a.n + BLK - 1) / BLK), dim3(BLK), 0, s, a);
    }
  }
  flags_count(sc, a.n, 0u, total, s);   // (sc.flags = a.flags)
  // the duplicates (dup_sc.flags = a.dup) are only counted: the result's three numbers are known before anything is written.  Gate off: there
  // are none, and dup_sc is not touched
  if (a.gate) flags_count(dup_sc, a.n, 0u, dup_total, s);
}
void insert_scatter(const InsertArgs& a, SurfelSoA dst, hipStream_t s) {
  static_assert(SELECT_ROW == BLK, "one rank lane per record of a chunk");
  if (a.n) hipLaunchKernelGGL(k_insert_scatter, dim3(select_chunks(a.n)), dim3(BLK), 0, s, a, dst);
}
