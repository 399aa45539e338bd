// Remove outlier surfels: neighbourhood statistics of the map (ef_map_neighbor_stats / ef_map_outliers_select / ef_map_remove_outliers,
// include/ef_hip.h; DESIGN.md §8i).  Included at the end of ef_map_kernels.hip, after ef_carve.inc.  It uses the query's index and its cell
// walk (ef_query.inc: query_walk with the self exclusion) and the selection's flag -> count -> scan -> list chain (ef_select.inc) unchanged.
// No frame kernel reads or writes anything here.
//   join      k_outlier_join<K>: the self-join of the map on its own index.  The queries are the index's own records in index order, one lane
//             per record, so a wave's 64 queries come from one bucket or adjacent buckets and walk nearly the same cells.  Each lane keeps its
//             K best in registers (K = 1 / 4 / 8 / 16, cut at k), then stores {mean, count} and the participant byte BY ROW.  Rows that the
//             index does not hold (a non-finite position) are written by the lane whose number is the row.
//   sums      k_outlier_partials: OUTLIER_SUM_LANES lanes, lane j adds the rows j, j + P, ... in ascending order, in double.
//             k_outlier_finish: one workgroup folds the P partials in twelve rounds of a[i] = a[2i] + a[2i+1] and one lane forms the threshold.
//             Both are pure functions of the per-row values by row: the order inside a bucket never reaches them.  No floating-point atomics.
//   flags     k_outlier_flags: the outlier byte per row.  Counts, lists and the removal are flags_count / select_rows / the erase, unchanged.
namespace {

constexpr int OUTLIER_FINISH = 1024;   // lanes of k_outlier_finish
constexpr int OUTLIER_AHEAD = 8;       // rows a lane of k_outlier_partials has in flight

// Correctly rounded f32 square root and quotient, whatever the build's flags say about f32 division and square roots: the f64 operations are
// always correctly rounded, and rounding their 53-bit result to 24 bits gives the correctly rounded f32 result (53 >= 2 x 24 + 2).
__device__ __forceinline__ float outlier_sqrt(float v) { return (float)__builtin_sqrt((double)v); }
__device__ __forceinline__ float outlier_div(float a, float b) { return (float)((double)a / (double)b); }

template <int K>
__global__ void __launch_bounds__(BLK) k_outlier_join(const OutlierArgs A) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned inf_bits = 0x7F800000u;
  if (t < A.n) {   // a row the index does not hold takes no part: nobody else writes it
    const float4 p = A.q.map.pos_conf[t];
    if (!query_finite3(p.x, p.y, p.z)) {
      A.stat[t] = make_uint2(inf_bits, 0u);
      A.part[t] = 0;
    }
  }
  const unsigned n_rec = min(A.q.cells[A.q.mask], A.n);   // the records of the index: the end of its last bucket
  if (t >= n_rec) return;
  const float4 q = A.q.sorted[t];
  const unsigned row = A.q.rows[t];
  if (row >= A.n) return;
  const bool part = !A.part_in || A.part_in[row] != 0;
  unsigned cnt = 0;
  float mean = __builtin_inff();
  if (part) {
    float bd[K];
    unsigned br[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { bd[j] = __builtin_inff(); br[j] = QUERY_NONE; }
    query_walk<1, K, true>(A.q, q.x, q.y, q.z, 0u, bd, br, cnt, t);
    if (cnt >= (unsigned)A.k) {
      float sum = outlier_sqrt(bd[0]);
#pragma unroll
      for (int j = 1; j < K; ++j)
        if (j < A.k) sum = sum + outlier_sqrt(bd[j]);
      mean = outlier_div(sum, (float)A.k);
    }
  }
  A.stat[row] = make_uint2(__float_as_uint(mean), cnt);
  A.part[row] = part ? 1 : 0;
}

// lane j: the rows j, j + P, j + 2P, ... in ascending order, starting from +0.0 (a row that is not measured adds +0.0: no change)
__global__ void __launch_bounds__(BLK) k_outlier_partials(const OutlierArgs A) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (unsigned)OUTLIER_SUM_LANES) return;
  double s1 = 0.0, s2 = 0.0;
  unsigned parts = 0, measured = 0, sparse = 0;
  // a lane's rows lie OUTLIER_SUM_LANES apart, so its loop is a chain of load latencies: OUTLIER_AHEAD rows are requested together and then
  // added one after the other, in ascending order
  for (unsigned r0 = j; r0 < A.n; r0 += OUTLIER_AHEAD * OUTLIER_SUM_LANES) {
    uint2 v[OUTLIER_AHEAD];
    bool p[OUTLIER_AHEAD];
#pragma unroll
    for (int i = 0; i < OUTLIER_AHEAD; ++i) {
      const unsigned r = r0 + i * OUTLIER_SUM_LANES;
      const bool in = r >= r0 && r < A.n;   // (r >= r0: no wrap past 2^32)
      p[i] = in && A.part[in ? r : 0u] != 0;
      v[i] = A.stat[in ? r : 0u];
    }
#pragma unroll
    for (int i = 0; i < OUTLIER_AHEAD; ++i) {
      if (!p[i]) continue;
      ++parts;
      if (v[i].y >= (unsigned)A.k) {
        ++measured;
        if (A.mode == OUTLIER_STATISTICAL) {
          const double m = (double)__uint_as_float(v[i].x);
          s1 = s1 + m;
          s2 = s2 + m * m;
        }
      } else {
        ++sparse;
      }
    }
  }
  A.partial[j] = s1;
  A.partial[OUTLIER_SUM_LANES + j] = s2;
  A.tally[j] = parts;
  A.tally[OUTLIER_SUM_LANES + j] = measured;
  A.tally[2 * OUTLIER_SUM_LANES + j] = sparse;
}

// one workgroup: twelve rounds of a[i] = a[2i] + a[2i+1] over the P partials of each sum (every round reads, waits, writes), the integer
// tallies (exact in any order), the threshold by lane 0
__global__ void __launch_bounds__(OUTLIER_FINISH) k_outlier_finish(const OutlierArgs A) {
  static_assert(OUTLIER_SUM_LANES == 4096 && OUTLIER_SUM_LANES % OUTLIER_FINISH == 0, "twelve rounds");
  __shared__ double a[OUTLIER_SUM_LANES];
  __shared__ unsigned tot[3];
  const unsigned tid = threadIdx.x;
  double S[2];
  for (int w = 0; w < 2; ++w) {
    for (unsigned i = tid; i < (unsigned)OUTLIER_SUM_LANES; i += OUTLIER_FINISH) a[i] = A.partial[w * OUTLIER_SUM_LANES + i];
    __syncthreads();
    for (unsigned len = OUTLIER_SUM_LANES / 2; len >= 1; len >>= 1) {
      double v[OUTLIER_SUM_LANES / 2 / OUTLIER_FINISH];
#pragma unroll
      for (unsigned e = 0; e < OUTLIER_SUM_LANES / 2 / OUTLIER_FINISH; ++e) {
        const unsigned i = tid + e * OUTLIER_FINISH;
        v[e] = i < len ? a[2 * i] + a[2 * i + 1] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (unsigned e = 0; e < OUTLIER_SUM_LANES / 2 / OUTLIER_FINISH; ++e) {
        const unsigned i = tid + e * OUTLIER_FINISH;
        if (i < len) a[i] = v[e];
      }
      __syncthreads();
    }
    S[w] = a[0];
    __syncthreads();
  }
  if (tid < 3) tot[tid] = 0u;
  __syncthreads();
  for (int w = 0; w < 3; ++w) {
    unsigned sum = 0;
    for (unsigned i = tid; i < (unsigned)OUTLIER_SUM_LANES; i += OUTLIER_FINISH) sum += A.tally[w * OUTLIER_SUM_LANES + i];
    atomicAdd(&tot[w], sum);
  }
  __syncthreads();
  if (tid != 0) return;
  const unsigned N = tot[1];
  float thr = __builtin_inff();
  if (A.mode == OUTLIER_STATISTICAL) {
    if (A.max_mean_dist > 0.f) {
      thr = A.max_mean_dist;
    } else if (N) {
      const double mu = S[0] / (double)N;
      double var = S[1] / (double)N - mu * mu;
      if (var < 0.0) var = 0.0;
      thr = (float)(mu + (double)A.std_ratio * __dsqrt_rn(var));
    }
  }
  OutlierResult r;
  r.sum = S[0];
  r.sum_sq = S[1];
  r.participants = tot[0];
  r.measured = N;
  r.sparse = tot[2];
  r.outliers = 0u;
  r.count_after = A.n;
  r.threshold = thr;
  *A.res = r;
}

__global__ void __launch_bounds__(BLK) k_outlier_flags(const OutlierArgs A, uint8_t* __restrict__ flags) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n) return;
  bool out = false;
  if (A.part[r]) {
    const uint2 v = A.stat[r];
    if (A.mode == OUTLIER_RADIUS) out = v.y < A.min_neighbors;
    else if (v.y >= (unsigned)A.k) out = __uint_as_float(v.x) > A.res->threshold;
    else out = A.flag_sparse != 0;
  }
  flags[r] = out ? 1 : 0;
}

__global__ void k_outlier_tally(OutlierResult* res, unsigned n, const uint32_t* __restrict__ total, OutlierResult* copy_to) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  OutlierResult r = *res;
  r.outliers = *total;
  r.count_after = n - r.outliers;
  *res = r;
  if (copy_to) *copy_to = r;
}

__global__ void __launch_bounds__(BLK) k_outlier_split(const uint2* __restrict__ stat, unsigned rows, float* __restrict__ mean,
                                                       uint32_t* __restrict__ count) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const uint2 v = stat[r];
  if (mean) mean[r] = __uint_as_float(v.x);
  if (count) count[r] = v.y;
}

}  // namespace

void outlier_join(const OutlierArgs& a, hipStream_t s) {
  if (!a.n) return;
  const dim3 g(ceil_div((int)a.n, BLK)), b(BLK);
  if (a.k == 1) hipLaunchKernelGGL(k_outlier_join<1>, g, b, 0, s, a);
  else if (a.k <= 4) hipLaunchKernelGGL(k_outlier_join<4>, g, b, 0, s, a);
  else if (a.k <= 8) hipLaunchKernelGGL(k_outlier_join<8>, g, b, 0, s, a);
  else hipLaunchKernelGGL(k_outlier_join<16>, g, b, 0, s, a);
}
void outlier_reduce(const OutlierArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_outlier_partials, dim3(OUTLIER_SUM_LANES / BLK), dim3(BLK), 0, s, a);
  hipLaunchKernelGGL(k_outlier_finish, dim3(1), dim3(OUTLIER_FINISH), 0, s, a);
}
void outlier_flags(const OutlierArgs& a, uint8_t* flags, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_outlier_flags, dim3(ceil_div((int)a.n, BLK)), dim3(BLK), 0, s, a, flags);
}
void outlier_tally(const OutlierArgs& a, const uint32_t* total, OutlierResult* copy_to, hipStream_t s) {
  hipLaunchKernelGGL(k_outlier_tally, dim3(1), dim3(64), 0, s, a.res, a.n, total, copy_to);
}
void outlier_split(const OutlierArgs& a, float* mean, uint32_t* count, unsigned rows, hipStream_t s) {
  rows = rows < a.n ? rows : a.n;
  if (rows && (mean || count)) hipLaunchKernelGGL(k_outlier_split, dim3(ceil_div((int)rows, BLK)), dim3(BLK), 0, s, (const uint2*)a.stat, rows, mean, count);
}
