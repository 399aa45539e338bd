// Smooth the map's positions by moving least squares (ef_map_smooth / ef_map_smooth_select / ef_map_smooth_apply, include/ef_hip.h; DESIGN.md
// §8n).  Included at the end of ef_map_kernels.hip, after ef_regions.inc.  It uses the query's index and its cell walk (ef_query.inc: query_walk
// with the self exclusion), the outliers' correctly rounded f32 square root (ef_outlier.inc), the shared eigen-solver (ef_plane_fit.hpp:
// smooth_fit) and the selection's flag -> count -> scan -> list chain (ef_select.inc) unchanged.  No frame kernel reads or writes anything here.
//   neighbours  k_smooth_neighbours<K>: the self-join of the map on its own index, with the shape of k_normal_join: one lane per record of the
//               index in index order, the K best (d2, row) in registers (K = 4 / 8 / 16, cut at k).  It stores count_s, the NONE / SPARSE /
//               "is fitted" byte and the used rows, slot-major (nbr[j * stride + row]); a slot past the lane's own neighbourhood holds the
//               lane's own row.  Rows that the index does not hold (a non-finite position) are written by the lane whose number is the row.
//               This is the only launch of a call that walks cells: the neighbourhoods are those of the map's own positions for every iteration.
//   step        k_smooth_step<K>: one launch per iteration, ordered by the stream, one lane per ROW in row order: the list, the row's own
//               position, the outputs and the status byte are coalesced streams, and only the gather of the neighbours' float4 positions (and,
//               with the gate, of their stored normals) is scattered.  It reads the iteration's INPUT buffer (the map itself for the first)
//               and writes the OUTPUT buffer of every row, never in place: ten double sums in neighbour order, smooth_fit, the projection.  A
//               slot from c on gathers the row itself with the weight 0.0: its difference is an exact +0.0, and a running sum that starts at
//               +0.0 is never -0.0, so no sum changes and the gather has no divergent branch.  No atomics, no LDS, no cross-lane operation.
//   finish      k_smooth_finish: shift of every row from the last buffer and the map.
//   flags       k_smooth_flags: the `what` byte per row.  Counts and lists are flags_count / select_rows, unchanged.
//   tally       k_smooth_tally: k_normal_tally's pattern (at most SMOOTH_TALLY_GRID workgroups, integer adds) plus an integer atomicMax on the
//               bits of the shift, a non-negative float: exact in any order.  k_smooth_result adds the list's total and copies the result out.
//   split       k_smooth_split: the optional per-row outputs.
//   apply       k_smooth_apply: one lane per row, the only writer of that row's position and normal words.
namespace {

constexpr int SMOOTH_TALLY_GRID = 512;   // workgroups of k_smooth_tally at most

template <int K>
__global__ void __launch_bounds__(BLK) k_smooth_neighbours(const SmoothArgs A) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < A.n) {   // a row the index does not hold takes no part: nobody else writes it
    const float4 p = A.q.map.pos_conf[t];
    if (!query_finite3(p.x, p.y, p.z)) {
      A.count[t] = 0u;
      A.status[t] = (uint8_t)SMOOTH_NONE;
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (j < A.k) A.nbr[(size_t)j * A.stride + t] = t;
    }
  }
  const unsigned n_rec = min(A.q.cells[A.q.mask], A.n);   // the records of the index: the end of its last bucket
  if (t >= n_rec) return;
  const float4 q = A.q.sorted[t];
  const unsigned row = A.q.rows[t];
  if (row >= A.n) return;
  const bool part = !A.part_in || A.part_in[row] != 0;
  unsigned cnt = 0, status = SMOOTH_NONE;
  float bd[K];
  unsigned br[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { bd[j] = __builtin_inff(); br[j] = QUERY_NONE; }
  if (part) {
    query_walk<1, K, true>(A.q, q.x, q.y, q.z, 0u, bd, br, cnt, t);
    status = cnt < A.min_neighbors ? SMOOTH_SPARSE : SMOOTH_SMOOTHED;
  }
  const unsigned c = min(cnt, (unsigned)A.k);
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (j < A.k) A.nbr[(size_t)j * A.stride + row] = (unsigned)j < c && br[j] < A.n ? br[j] : row;
  A.count[row] = cnt;
  A.status[row] = (uint8_t)status;
}

template <int K>
__global__ void __launch_bounds__(BLK) k_smooth_step(const SmoothArgs A, const float4* __restrict__ in, float4* __restrict__ out) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n) return;
  const float4 p = in[r];
  const unsigned old = A.status[r], st = old & SMOOTH_STATUS_MASK;
  float4 moved = p, est = make_float4(0.f, 0.f, 0.f, 0.f);
  unsigned now = old;
  if (st != SMOOTH_NONE && st != SMOOTH_SPARSE) {
    const unsigned c = min(A.count[r], (unsigned)A.k);
    const float4 ns = A.q.map.nrm_rad[r];
    // the weighted moments about the row's own position, in neighbour order (j < A.k is uniform across the launch; a slot from c on reads the row itself)
    double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, W = 1.0;
    const double ax = (double)p.x, ay = (double)p.y, az = (double)p.z, r2 = (double)A.q.r2;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (j < A.k) {
        const unsigned t = A.nbr[(size_t)j * A.stride + r];
        const float4 pt = in[t];
        double w = (unsigned)j < c ? 1.0 : 0.0;
        if (A.weighting == SMOOTH_COMPACT) {
          const float dx = p.x - pt.x, dy = p.y - pt.y, dz = p.z - pt.z;
          const float d2 = ((dx * dx + dy * dy) + dz * dz);
          const double u = 1.0 - (double)d2 / r2;
          w = (unsigned)j < c && u > 0.0 ? u * u : 0.0;
        }
        if (A.gate) {
          const float4 nt = A.q.map.nrm_rad[t];
          const float dot = (ns.x * nt.x + ns.y * nt.y) + ns.z * nt.z;
          if (!(dot >= A.min_normal_cos)) w = 0.0;
        }
        const double x = (double)pt.x - ax, y = (double)pt.y - ay, z = (double)pt.z - az;
        const double a = w * x, b = w * y, g = w * z;
        S[0] = S[0] + a;
        S[1] = S[1] + b;
        S[2] = S[2] + g;
        S[3] = S[3] + a * x;
        S[4] = S[4] + a * y;
        S[5] = S[5] + a * z;
        S[6] = S[6] + b * y;
        S[7] = S[7] + b * z;
        S[8] = S[8] + g * z;
        W = W + w;
      }
    }
    const float hn[3] = {ns.x, ns.y, ns.z};
    double n[3], mean[3];
    float curv;
    const int fit = smooth_fit(S, W, c + 1u, hn, A.line_ratio, n, mean, &curv);
    now = (old & SMOOTH_CLAMPED_BIT) | SMOOTH_DEGENERATE;
    if (fit == NORMAL_FIT_ESTIMATED) {
      const double t = (n[0] * mean[0] + n[1] * mean[1]) + n[2] * mean[2];
      double s = (double)A.strength * t;
      const double ms = (double)A.max_shift;
      if (s > ms) {
        s = ms;
        now |= SMOOTH_CLAMPED_BIT;
      } else if (s < -ms) {
        s = -ms;
        now |= SMOOTH_CLAMPED_BIT;
      }
      const float fx = (float)(ax + s * n[0]), fy = (float)(ay + s * n[1]), fz = (float)(az + s * n[2]);
      if (query_finite3(fx, fy, fz)) {
        moved = make_float4(fx, fy, fz, p.w);
        est = make_float4((float)n[0], (float)n[1], (float)n[2], curv);
        now = (now & SMOOTH_CLAMPED_BIT) | SMOOTH_SMOOTHED;
      }
    }
  }
  out[r] = moved;
  A.est[r] = est;
  A.status[r] = (uint8_t)now;
}

__global__ void __launch_bounds__(BLK) k_smooth_finish(const SmoothArgs A, const float4* __restrict__ last) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n) return;
  const unsigned st = A.status[r] & SMOOTH_STATUS_MASK;
  float shift = 0.f;
  if (st == SMOOTH_SMOOTHED || st == SMOOTH_DEGENERATE) {   // (every other row has never moved, and a row without a finite position has no distance)
    const float4 a = last[r], b = A.q.map.pos_conf[r];
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    shift = outlier_sqrt(((dx * dx + dy * dy) + dz * dz));
  }
  A.shift[r] = shift;
}

__global__ void __launch_bounds__(BLK) k_smooth_flags(const SmoothArgs A, int what, uint8_t* __restrict__ flags) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n) return;
  const unsigned s = A.status[r];
  bool on;
  if (what == SMOOTH_CLAMPED) on = (s & SMOOTH_CLAMPED_BIT) != 0u;
  else if (what == SMOOTH_SHIFTED) on = A.shift[r] > A.shift_threshold;
  else on = (s & SMOOTH_STATUS_MASK) == (unsigned)what;
  flags[r] = on ? 1 : 0;
}

// k_normal_tally's pattern: at most SMOOTH_TALLY_GRID workgroups stride the rows, a workgroup folds its lanes' counts in LDS and adds them to the
// result's words, which the caller has zeroed (integer adds and an integer maximum of the bits of non-negative floats: exact in any order)
__global__ void __launch_bounds__(BLK) k_smooth_tally(const SmoothArgs A) {
  __shared__ unsigned tot[7];
  const unsigned tid = threadIdx.x;
  if (tid < 7) tot[tid] = 0u;
  __syncthreads();
  unsigned c[6] = {0u, 0u, 0u, 0u, 0u, 0u}, big = 0u;
  for (unsigned r = blockIdx.x * blockDim.x + tid; r < A.n; r += gridDim.x * blockDim.x) {
    const unsigned s = A.status[r], st = s & SMOOTH_STATUS_MASK;
    const float shift = A.shift[r];
    c[0] += st != SMOOTH_NONE;
    c[1] += st == SMOOTH_SMOOTHED;
    c[2] += st == SMOOTH_SPARSE;
    c[3] += st == SMOOTH_DEGENERATE;
    c[4] += (s & SMOOTH_CLAMPED_BIT) != 0u;
    if (shift > 0.f) {
      c[5] += 1u;
      big = max(big, __float_as_uint(shift));
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (c[i]) atomicAdd(&tot[i], c[i]);
  if (big) atomicMax(&tot[6], big);
  __syncthreads();
  if (tid >= 7 || !tot[tid]) return;
  if (tid == 6) {
    atomicMax(reinterpret_cast<unsigned*>(&A.res->largest_shift), tot[6]);
    return;
  }
  uint32_t* word = tid == 0 ? &A.res->participants : tid == 1 ? &A.res->smoothed : tid == 2 ? &A.res->sparse : tid == 3 ? &A.res->degenerate
                   : tid == 4 ? &A.res->clamped : &A.res->moved;
  atomicAdd(word, tot[tid]);
}
// res->listed = *total (0 with total null); then *copy_to = *res unless copy_to is null
__global__ void k_smooth_result(SmoothResult* res, const uint32_t* __restrict__ total, SmoothResult* copy_to) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  SmoothResult r = *res;
  r.listed = total ? *total : 0u;
  *res = r;
  if (copy_to) *copy_to = r;
}

__global__ void __launch_bounds__(BLK) k_smooth_split(const SmoothArgs A, const float4* __restrict__ last, unsigned rows, float* __restrict__ position3,
                                                      float* __restrict__ normal3, float* __restrict__ curvature, float* __restrict__ shift,
                                                      uint32_t* __restrict__ count, uint8_t* __restrict__ status) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  if (position3) {
    const float4 p = last[r];
    position3[(size_t)r * 3] = p.x;
    position3[(size_t)r * 3 + 1] = p.y;
    position3[(size_t)r * 3 + 2] = p.z;
  }
  if (normal3 || curvature) {
    const float4 e = A.est[r];
    if (normal3) {
      normal3[(size_t)r * 3] = e.x;
      normal3[(size_t)r * 3 + 1] = e.y;
      normal3[(size_t)r * 3 + 2] = e.z;
    }
    if (curvature) curvature[r] = e.w;
  }
  if (shift) shift[r] = A.shift[r];
  if (count) count[r] = A.count[r];
  if (status) status[r] = (uint8_t)(A.status[r] & SMOOTH_STATUS_MASK);
}

__global__ void __launch_bounds__(BLK) k_smooth_apply(const SmoothArgs A, const float4* __restrict__ last) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n) return;
  const unsigned st = A.status[r] & SMOOTH_STATUS_MASK;
  if (st == SMOOTH_NONE) return;
  const float4 p = last[r];
  float4 m = A.q.map.pos_conf[r];
  m.x = p.x;
  m.y = p.y;
  m.z = p.z;
  A.q.map.pos_conf[r] = m;
  if (A.set_normal && st == SMOOTH_SMOOTHED) {
    const float4 e = A.est[r];
    float4 nr = A.q.map.nrm_rad[r];
    nr.x = e.x;
    nr.y = e.y;
    nr.z = e.z;
    A.q.map.nrm_rad[r] = nr;
  }
}

}  // namespace

void smooth_neighbours(const SmoothArgs& a, hipStream_t s) {
  if (!a.n) return;
  const dim3 g(ceil_div((int)a.n, BLK)), b(BLK);
  if (a.k <= 4) hipLaunchKernelGGL(k_smooth_neighbours<4>, g, b, 0, s, a);
  else if (a.k <= 8) hipLaunchKernelGGL(k_smooth_neighbours<8>, g, b, 0, s, a);
  else hipLaunchKernelGGL(k_smooth_neighbours<16>, g, b, 0, s, a);
}
void smooth_step(const SmoothArgs& a, int i, hipStream_t s) {
  if (!a.n) return;
  const float4* in = i == 1 ? (const float4*)a.q.map.pos_conf : (const float4*)a.buf[i & 1];
  float4* out = a.buf[(i - 1) & 1];
  const dim3 g(ceil_div((int)a.n, BLK)), b(BLK);
  if (a.k <= 4) hipLaunchKernelGGL(k_smooth_step<4>, g, b, 0, s, a, in, out);
  else if (a.k <= 8) hipLaunchKernelGGL(k_smooth_step<8>, g, b, 0, s, a, in, out);
  else hipLaunchKernelGGL(k_smooth_step<16>, g, b, 0, s, a, in, out);
}
void smooth_finish(const SmoothArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_smooth_finish, dim3(ceil_div((int)a.n, BLK)), dim3(BLK), 0, s, a, smooth_final(a));
}
void smooth_flags(const SmoothArgs& a, int what, uint8_t* flags, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_smooth_flags, dim3(ceil_div((int)a.n, BLK)), dim3(BLK), 0, s, a, what, flags);
}
void smooth_tally(const SmoothArgs& a, const uint32_t* total, SmoothResult* copy_to, hipStream_t s) {
  (void)hipMemsetAsync(a.res, 0, sizeof(SmoothResult), s);   // (an error of the enqueue surfaces in the caller's hipGetLastError)
  if (a.n) hipLaunchKernelGGL(k_smooth_tally, dim3(min(ceil_div((int)a.n, BLK), SMOOTH_TALLY_GRID)), dim3(BLK), 0, s, a);
  hipLaunchKernelGGL(k_smooth_result, dim3(1), dim3(64), 0, s, a.res, total, copy_to);
}
void smooth_split(const SmoothArgs& a, float* position3, float* normal3, float* curvature, float* shift, uint32_t* count, uint8_t* status,
                  unsigned rows, hipStream_t s) {
  rows = rows < a.n ? rows : a.n;
  if (rows && (position3 || normal3 || curvature || shift || count || status))
    hipLaunchKernelGGL(k_smooth_split, dim3(ceil_div((int)rows, BLK)), dim3(BLK), 0, s, a, smooth_final(a), rows, position3, normal3, curvature,
                       shift, count, status);
}
void smooth_apply(const SmoothArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_smooth_apply, dim3(ceil_div((int)a.n, BLK)), dim3(BLK), 0, s, a, smooth_final(a));
}
