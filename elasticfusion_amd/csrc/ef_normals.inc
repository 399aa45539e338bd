// Estimate normals, curvature and spacing from the map's neighbourhoods (ef_map_normals / ef_map_normals_select / ef_map_reestimate_normals,
// include/ef_hip.h; DESIGN.md §8l).  Included at the end of ef_map_kernels.hip, after ef_planes.inc.  It uses the query's index and its cell
// walk (ef_query.inc: query_walk with the self exclusion), the outliers' correctly rounded f32 square root and quotient (ef_outlier.inc), the
// shared eigen-solver (ef_plane_fit.hpp: normal_fit) and the selection's flag -> count -> scan -> list chain (ef_select.inc) unchanged.  No frame
// kernel reads or writes anything here.
//   join      k_normal_join<K>: the self-join of the map on its own index, with the shape of k_outlier_join: one lane per record of the index in
//             index order, the K best (d2, row) in registers (K = 4 / 8 / 16, cut at k).  The lane then gathers the used neighbours' positions
//             from the map by row, forms the nine double sums in neighbour order, runs the eigen-solver and stores {normal, curvature},
//             {spacing, count} and the status byte BY ROW.  A slot past the lane's own neighbourhood gathers the lane's own row, whose
//             difference is an exact +0.0 that changes no sum (a running sum that starts at +0.0 is never -0.0), so the gather has no divergent
//             branch.  Rows that the index does not hold (a non-finite position) are written by the lane whose number is the row.  No atomics, no
//             LDS, no cross-lane operation; every result is a function of the lane's own sorted neighbour list.
//   flags     k_normal_flags: the `what` byte per row.  Counts and lists are flags_count / select_rows, unchanged.
//   tally     k_normal_tally: at most 512 workgroups stride the status bytes and add their counts to the zeroed result (integer adds: exact in
//             any order; one workgroup took 341 us on 1 M rows); k_normal_result adds the list's total and copies the result out.
//   split     k_normal_split: the optional per-row outputs from the packed words.
//   apply     k_normal_apply: one lane per row; an ESTIMATED row's lane is the only writer of that row's normal word.
namespace {

constexpr int NORMAL_TALLY_GRID = 512;   // workgroups of k_normal_tally at most

template <int K>
__global__ void __launch_bounds__(BLK) k_normal_join(const NormalArgs A) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned inf_bits = 0x7F800000u;
  if (t < A.n) {   // a row the index does not hold takes no part: nobody else writes it
    const float4 p = A.q.map.pos_conf[t];
    if (!query_finite3(p.x, p.y, p.z)) {
      A.est[t] = make_float4(0.f, 0.f, 0.f, 0.f);
      A.stat[t] = make_uint2(inf_bits, 0u);
      A.status[t] = (uint8_t)NORMAL_NONE;
    }
  }
  const unsigned n_rec = min(A.q.cells[A.q.mask], A.n);   // the records of the index: the end of its last bucket
  if (t >= n_rec) return;
  const float4 q = A.q.sorted[t];
  const unsigned row = A.q.rows[t];
  if (row >= A.n) return;
  const bool part = !A.part_in || A.part_in[row] != 0;
  unsigned cnt = 0, status = NORMAL_NONE;
  float spacing = __builtin_inff();
  float4 est = make_float4(0.f, 0.f, 0.f, 0.f);
  if (part) {
    float bd[K];
    unsigned br[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { bd[j] = __builtin_inff(); br[j] = QUERY_NONE; }
    query_walk<1, K, true>(A.q, q.x, q.y, q.z, 0u, bd, br, cnt, t);
    const unsigned c = min(cnt, (unsigned)A.k);
    if (c) {
      float sum = outlier_sqrt(bd[0]);
#pragma unroll
      for (int j = 1; j < K; ++j)
        if ((unsigned)j < c) sum = sum + outlier_sqrt(bd[j]);
      spacing = outlier_div(sum, (float)c);
    }
    if (cnt < A.min_neighbors) {
      status = NORMAL_SPARSE;
    } else {
      // the moments about the row's own position, in neighbour order (j < A.k is uniform across the launch; a slot from c on reads the row itself)
      double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      const double ax = (double)q.x, ay = (double)q.y, az = (double)q.z;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (j < A.k) {
          const unsigned r = (unsigned)j < c && br[j] < A.n ? br[j] : row;
          const float4 p = A.q.map.pos_conf[r];
          const double x = (double)p.x - ax, y = (double)p.y - ay, z = (double)p.z - az;
          S[0] = S[0] + x;
          S[1] = S[1] + y;
          S[2] = S[2] + z;
          S[3] = S[3] + x * x;
          S[4] = S[4] + x * y;
          S[5] = S[5] + x * z;
          S[6] = S[6] + y * y;
          S[7] = S[7] + y * z;
          S[8] = S[8] + z * z;
        }
      }
      float hn[3];
      if (A.orientation == NORMALS_VIEWPOINT) {
        hn[0] = A.side * (A.view[0] - q.x);
        hn[1] = A.side * (A.view[1] - q.y);
        hn[2] = A.side * (A.view[2] - q.z);
      } else {
        const float4 m = A.q.map.nrm_rad[row];
        hn[0] = m.x;
        hn[1] = m.y;
        hn[2] = m.z;
      }
      float nrm[3], curv;
      double l[3];
      bool flipped;
      const int fit = normal_fit(S, c + 1u, hn, A.line_ratio, nrm, &curv, &flipped, l);
      if (fit == NORMAL_FIT_ESTIMATED) {
        status = NORMAL_ESTIMATED | (flipped ? NORMAL_FLIPPED : 0u);
        est = make_float4(nrm[0], nrm[1], nrm[2], curv);
      } else {
        status = NORMAL_DEGENERATE;
      }
    }
  }
  A.est[row] = est;
  A.stat[row] = make_uint2(__float_as_uint(spacing), cnt);
  A.status[row] = (uint8_t)status;
}

__device__ __forceinline__ bool normal_listed(const NormalArgs& A, int what, unsigned status, float curvature) {
  const unsigned st = status & NORMAL_STATUS_MASK;
  if (what == NORMALS_CURVED) return st == NORMAL_ESTIMATED && curvature > A.max_curvature;
  if (what == NORMALS_FLAT) return st == NORMAL_ESTIMATED && !(curvature > A.max_curvature);
  return st == (unsigned)what;
}

__global__ void __launch_bounds__(BLK) k_normal_flags(const NormalArgs A, int what, uint8_t* __restrict__ flags) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n) return;
  flags[r] = normal_listed(A, what, A.status[r], A.est[r].w) ? 1 : 0;
}

// at most NORMAL_TALLY_GRID workgroups stride the rows: every lane counts its rows, a workgroup folds its counts in LDS and adds them to the
// result's words, which the caller has zeroed (integer adds: exact in any order)
__global__ void __launch_bounds__(BLK) k_normal_tally(const NormalArgs A) {
  __shared__ unsigned tot[5];
  const unsigned tid = threadIdx.x;
  if (tid < 5) tot[tid] = 0u;
  __syncthreads();
  unsigned c[5] = {0u, 0u, 0u, 0u, 0u};
  for (unsigned r = blockIdx.x * blockDim.x + tid; r < A.n; r += gridDim.x * blockDim.x) {
    const unsigned s = A.status[r], st = s & NORMAL_STATUS_MASK;
    c[0] += st != NORMAL_NONE;
    c[1] += st == NORMAL_ESTIMATED;
    c[2] += st == NORMAL_SPARSE;
    c[3] += st == NORMAL_DEGENERATE;
    c[4] += (s & NORMAL_FLIPPED) != 0u;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i)
    if (c[i]) atomicAdd(&tot[i], c[i]);
  __syncthreads();
  if (tid >= 5 || !tot[tid]) return;
  uint32_t* word = tid == 0 ? &A.res->participants : tid == 1 ? &A.res->estimated : tid == 2 ? &A.res->sparse : tid == 3 ? &A.res->degenerate : &A.res->flipped;
  atomicAdd(word, tot[tid]);
}
// res->listed = *total (0 with total null); then *copy_to = *res unless copy_to is null
__global__ void k_normal_result(NormalResult* res, const uint32_t* __restrict__ total, NormalResult* copy_to) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  NormalResult r = *res;
  r.listed = total ? *total : 0u;
  *res = r;
  if (copy_to) *copy_to = r;
}

__global__ void __launch_bounds__(BLK) k_normal_split(const float4* __restrict__ est, const uint2* __restrict__ stat, const uint8_t* __restrict__ st,
                                                      unsigned rows, float* __restrict__ normals3, float* __restrict__ curvature,
                                                      float* __restrict__ spacing, uint32_t* __restrict__ count, uint8_t* __restrict__ status) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float4 e = est[r];
  const uint2 v = stat[r];
  if (normals3) {
    normals3[(size_t)r * 3] = e.x;
    normals3[(size_t)r * 3 + 1] = e.y;
    normals3[(size_t)r * 3 + 2] = e.z;
  }
  if (curvature) curvature[r] = e.w;
  if (spacing) spacing[r] = __uint_as_float(v.x);
  if (count) count[r] = v.y;
  if (status) status[r] = (uint8_t)(st[r] & NORMAL_STATUS_MASK);
}

__global__ void __launch_bounds__(BLK) k_normal_apply(const NormalArgs A) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n || (A.status[r] & NORMAL_STATUS_MASK) != NORMAL_ESTIMATED) return;
  const float4 e = A.est[r];
  float4 m = A.q.map.nrm_rad[r];
  m.x = e.x;
  m.y = e.y;
  m.z = e.z;
  if (A.set_radius) m.w = A.radius_scale * __uint_as_float(A.stat[r].x);
  A.q.map.nrm_rad[r] = m;
}

}  // namespace

void normal_join(const NormalArgs& a, hipStream_t s) {
  if (!a.n) return;
  const dim3 g(ceil_div((int)a.n, BLK)), b(BLK);
  if (a.k <= 4) hipLaunchKernelGGL(k_normal_join<4>, g, b, 0, s, a);
  else if (a.k <= 8) hipLaunchKernelGGL(k_normal_join<8>, g, b, 0, s, a);
  else hipLaunchKernelGGL(k_normal_join<16>, g, b, 0, s, a);
}
void normal_flags(const NormalArgs& a, int what, uint8_t* flags, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_normal_flags, dim3(ceil_div((int)a.n, BLK)), dim3(BLK), 0, s, a, what, flags);
}
void normal_tally(const NormalArgs& a, const uint32_t* total, NormalResult* copy_to, hipStream_t s) {
  (void)hipMemsetAsync(a.res, 0, sizeof(NormalResult), s);   // (an error of the enqueue surfaces in the caller's hipGetLastError)
  if (a.n) hipLaunchKernelGGL(k_normal_tally, dim3(min(ceil_div((int)a.n, BLK), NORMAL_TALLY_GRID)), dim3(BLK), 0, s, a);
  hipLaunchKernelGGL(k_normal_result, dim3(1), dim3(64), 0, s, a.res, total, copy_to);
}
void normal_split(const NormalArgs& a, float* normals3, float* curvature, float* spacing, uint32_t* count, uint8_t* status, unsigned rows,
                  hipStream_t s) {
  rows = rows < a.n ? rows : a.n;
  if (rows && (normals3 || curvature || spacing || count || status))
    hipLaunchKernelGGL(k_normal_split, dim3(ceil_div((int)rows, BLK)), dim3(BLK), 0, s, (const float4*)a.est, (const uint2*)a.stat,
                       (const uint8_t*)a.status, rows, normals3, curvature, spacing, count, status);
}
void normal_apply(const NormalArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_normal_apply, dim3(ceil_div((int)a.n, BLK)), dim3(BLK), 0, s, a);
}
