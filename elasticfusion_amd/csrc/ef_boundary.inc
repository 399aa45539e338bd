// Find the map's open boundaries and holes by the angle criterion (ef_map_boundaries / ef_map_boundaries_select, include/ef_hip.h; DESIGN.md
// §8o).  Included at the end of ef_map_kernels.hip, after ef_smooth.inc.  It uses the query's index and its cell walk (ef_query.inc: query_walk
// with the self exclusion), the normals' join (ef_normals.inc: normal_join, for EF_BOUNDARY_ESTIMATED), the components' union-find with its
// selection byte (ef_components.inc: component_hook / component_label, which string the boundary rows into loops) and the selection's flag ->
// count -> scan -> list chain (ef_select.inc) unchanged; the gap itself is ef_boundary_gap.hpp.  No frame kernel reads or writes anything here.
//   join      k_boundary_join<K>: the self-join of the map on its own index, with the shape of k_normal_join: one lane per record of the index
//             in index order, the K best (d2, row) in registers (K = 4 / 8 / 16, cut at k).  The lane then gathers the used neighbours'
//             positions from the map by row, runs boundary_gap and stores {gap, count} and the status byte BY ROW.  A slot past the lane's own
//             neighbourhood gathers the lane's own row and is not looked at, so the gather has no divergent branch.  Rows that the index does
//             not hold (a non-finite position) are written by the lane whose number is the row.  No atomics, no LDS, no cross-lane operation;
//             every result is a function of the lane's own sorted neighbour list.
//   flags     k_boundary_flags: the byte "status == what" per row: the loops' selection (what = BOUNDARY) and the four verdict lists.
//   tally     k_boundary_tally: at most 512 workgroups stride the status bytes and add their counts to the zeroed result (integer adds: exact
//             in any order); k_boundary_result adds the loops' counts and the list's total and copies the result out.
//   split     k_boundary_split: the optional per-row outputs.
namespace {

constexpr int BOUNDARY_TALLY_GRID = 512;   // workgroups of k_boundary_tally at most

template <int K>
__global__ void __launch_bounds__(BLK) k_boundary_join(const BoundaryArgs A) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < A.n) {   // a row the index does not hold takes no part: nobody else writes it
    const float4 p = A.q.map.pos_conf[t];
    if (!query_finite3(p.x, p.y, p.z)) {
      A.stat[t] = make_uint2(0u, 0u);
      A.status[t] = (uint8_t)BOUNDARY_NONE;
    }
  }
  const unsigned n_rec = min(A.q.cells[A.q.mask], A.n);   // the records of the index: the end of its last bucket
  if (t >= n_rec) return;
  const float4 q = A.q.sorted[t];
  const unsigned row = A.q.rows[t];
  if (row >= A.n) return;
  const bool estimated = A.normal_source == BOUNDARY_ESTIMATED;
  const unsigned nst = estimated ? (A.nstatus[row] & NORMAL_STATUS_MASK) : NORMAL_NONE;
  // (ESTIMATED: the normals' join took the same participants and left NONE at every other row)
  const bool part = estimated ? nst != NORMAL_NONE : (!A.part_in || A.part_in[row] != 0);
  unsigned cnt = 0, status = BOUNDARY_NONE;
  float gap = 0.f;
  if (part) {
    float bd[K];
    unsigned br[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { bd[j] = __builtin_inff(); br[j] = QUERY_NONE; }
    query_walk<1, K, true>(A.q, q.x, q.y, q.z, 0u, bd, br, cnt, t);
    const unsigned c = min(cnt, (unsigned)A.k);
    if (cnt < A.min_neighbors || nst == NORMAL_SPARSE) {
      status = BOUNDARY_SPARSE;
    } else if (nst == NORMAL_DEGENERATE) {
      status = BOUNDARY_DEGENERATE;
    } else {
      const float4 mw = estimated ? A.nest[row] : A.q.map.nrm_rad[row];
      const float m[3] = {mw.x, mw.y, mw.z}, p[3] = {q.x, q.y, q.z};
      float px[K], py[K], pz[K];
#pragma unroll
      for (int j = 0; j < K; ++j) {   // (j < A.k is uniform across the launch; a slot from c on reads the row itself)
        px[j] = q.x;
        py[j] = q.y;
        pz[j] = q.z;
        if (j < A.k) {
          const unsigned r = (unsigned)j < c && br[j] < A.n ? br[j] : row;
          const float4 v = A.q.map.pos_conf[r];
          px[j] = v.x;
          py[j] = v.y;
          pz[j] = v.z;
        }
      }
      double G = 0.0;
      if (boundary_gap<K>(m, p, px, py, pz, (int)c, &G) == BOUNDARY_GAP_OK) {
        gap = (float)G;
        status = G > (double)A.max_gap ? BOUNDARY_BOUNDARY : BOUNDARY_INTERIOR;
      } else {
        status = BOUNDARY_DEGENERATE;
      }
    }
  }
  A.stat[row] = make_uint2(__float_as_uint(gap), cnt);
  A.status[row] = (uint8_t)status;
}

__global__ void __launch_bounds__(BLK) k_boundary_flags(const uint8_t* __restrict__ status, unsigned n, unsigned what, uint8_t* __restrict__ flags) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  flags[r] = status[r] == what ? 1 : 0;
}

// at most BOUNDARY_TALLY_GRID workgroups stride the rows: every lane counts its rows, a workgroup folds its counts in LDS and adds them to the
// result's words, which the caller has zeroed (integer adds: exact in any order)
__global__ void __launch_bounds__(BLK) k_boundary_tally(const BoundaryArgs A) {
  __shared__ unsigned tot[5];
  const unsigned tid = threadIdx.x;
  if (tid < 5) tot[tid] = 0u;
  __syncthreads();
  unsigned c[5] = {0u, 0u, 0u, 0u, 0u};
  for (unsigned r = blockIdx.x * blockDim.x + tid; r < A.n; r += gridDim.x * blockDim.x) {
    const unsigned st = A.status[r];
    c[0] += st != BOUNDARY_NONE;
    c[1] += st == BOUNDARY_INTERIOR;
    c[2] += st == BOUNDARY_BOUNDARY;
    c[3] += st == BOUNDARY_SPARSE;
    c[4] += st == BOUNDARY_DEGENERATE;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i)
    if (c[i]) atomicAdd(&tot[i], c[i]);
  __syncthreads();
  if (tid >= 5 || !tot[tid]) return;
  uint32_t* word = tid == 0 ? &A.res->participants : tid == 1 ? &A.res->interior : tid == 2 ? &A.res->boundary : tid == 3 ? &A.res->sparse : &A.res->degenerate;
  atomicAdd(word, tot[tid]);
}
// the loops' counts from the components' result, res->listed = *total (0 with total null); then *copy_to = *res unless copy_to is null
__global__ void k_boundary_result(BoundaryResult* res, const ComponentResult* __restrict__ comp, const uint32_t* __restrict__ total,
                                  BoundaryResult* copy_to) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  BoundaryResult r = *res;
  r.loops = comp->components;
  r.accepted = comp->components - comp->rejected_components;
  r.largest = comp->largest;
  r.listed = total ? *total : 0u;
  r.status = comp->status;
  *res = r;
  if (copy_to) *copy_to = r;
}

__global__ void __launch_bounds__(BLK) k_boundary_split(const uint2* __restrict__ stat, const uint8_t* __restrict__ st, const uint32_t* __restrict__ label_in,
                                                        const uint32_t* __restrict__ members, unsigned rows, float* __restrict__ gap,
                                                        uint32_t* __restrict__ count, uint8_t* __restrict__ status, uint32_t* __restrict__ label,
                                                        uint32_t* __restrict__ size) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const uint2 v = stat[r];
  if (gap) gap[r] = __uint_as_float(v.x);
  if (count) count[r] = v.y;
  if (status) status[r] = st[r];
  const unsigned l = label_in[r];
  if (label) label[r] = l;
  if (size) size[r] = l != COMPONENT_NONE ? members[l] : 0u;
}

}  // namespace

void boundary_join(const BoundaryArgs& a, hipStream_t s) {
  if (!a.n) return;
  const dim3 g(ceil_div((int)a.n, BLK)), b(BLK);
  if (a.k <= 4) hipLaunchKernelGGL(k_boundary_join<4>, g, b, 0, s, a);
  else if (a.k <= 8) hipLaunchKernelGGL(k_boundary_join<8>, g, b, 0, s, a);
  else hipLaunchKernelGGL(k_boundary_join<16>, g, b, 0, s, a);
}
void boundary_flags(const BoundaryArgs& a, unsigned what, uint8_t* flags, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_boundary_flags, dim3(ceil_div((int)a.n, BLK)), dim3(BLK), 0, s, (const uint8_t*)a.status, a.n, what, flags);
}
void boundary_tally(const BoundaryArgs& a, const uint32_t* total, BoundaryResult* copy_to, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_boundary_tally, dim3(min(ceil_div((int)a.n, BLK), BOUNDARY_TALLY_GRID)), dim3(BLK), 0, s, a);
  hipLaunchKernelGGL(k_boundary_result, dim3(1), dim3(64), 0, s, a.res, (const ComponentResult*)a.loops.res, total, copy_to);
}
void boundary_split(const BoundaryArgs& a, float* gap, uint32_t* count, uint8_t* status, uint32_t* label, uint32_t* size, unsigned rows,
                    hipStream_t s) {
  rows = rows < a.n ? rows : a.n;
  if (rows && (gap || count || status || label || size))
    hipLaunchKernelGGL(k_boundary_split, dim3(ceil_div((int)rows, BLK)), dim3(BLK), 0, s, (const uint2*)a.stat, (const uint8_t*)a.status,
                       (const uint32_t*)a.loops.label, (const uint32_t*)a.loops.members, rows, gap, count, status, label, size);
}
