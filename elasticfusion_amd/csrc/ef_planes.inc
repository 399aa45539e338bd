// Segment the map into planes by sequential RANSAC (ef_map_planes / ef_map_planes_select / ef_map_remove_planes, include/ef_hip.h;
// DESIGN.md §8k).  Included at the end of ef_map_kernels.hip, after ef_components.inc.  It uses the selection's flag -> count -> scan chain
// (ef_select.inc), the correctly rounded f32 square root and quotient and the summation order of ef_outlier.inc, and the least-squares fit
// of ef_plane_fit.hpp.  No frame kernel reads or writes anything here.  Every f32 expression is written in the header's order and the build
// contracts nothing, so every count below is the integer tests/planeref.py computes.
//   init      k_plane_init: the node byte and label = NONE of every row.
//   round k   k_plane_part (the bytes of the nodes no earlier round labelled, a count per SELECT_ROW rows), the scan (M = their number),
//             k_plane_compact (their positions, and normals when the normal test is on, dense and in ascending row order),
//             k_plane_hyp (H lanes: three hashed samples, the plane through them, four NaNs for an invalid one),
//             k_plane_score (the hot one: every hypothesis against every participant),
//             k_plane_pick (one workgroup: the greatest count, ties to the lowest h; ends the extraction where the header says so),
//             k_plane_moments + k_plane_fit (refine: the nine sums by map row in the outliers' order, folded in twelve rounds, then one lane
//             runs ef_plane_fit.hpp; without refine k_plane_fit only copies the hypothesis) and k_plane_mark (label = k for the participants
//             on the final plane, their number into the model).
//   finish    k_plane_flags (the list's byte per row), k_plane_tally, k_plane_split (the outputs).
// All rounds are enqueued without a host wait: grids are sized by the map's rows, and every kernel of a round reads M and the `done` word
// from device memory and returns at once after the extraction has ended.  Nothing waits for another workgroup; the only atomics are integer
// adds (exact in any order).
//
// k_plane_score: ONE HYPOTHESIS PER LANE.  The lane holds its plane and its count in registers; the workgroup stages SELECT_ROW compacted
// participants in LDS, by component, and every lane reads them back at the same address (a broadcast, no bank conflict: one 16-byte read
// per component and four participants), so the loop has no cross-lane operation and no atomic; the count leaves through one integer
// atomicAdd per lane and workgroup.  The grid is (M / PLANE_CHUNK) x (H / BLK): 1 M rows x 1024 hypotheses are 1956 workgroups.
namespace {

constexpr int PLANE_MARK_BLOCKS = 512;   // k_plane_mark strides the rows: at most this many workgroups add to the model's inlier count

__device__ __forceinline__ unsigned plane_h32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ float plane_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
// |n.p + d| <= distance, and with NRM also |n . normal| >= normal_cos; a NaN fails either
template <bool NRM>
__device__ __forceinline__ bool plane_inlier(const float4 pl, const float4 p, const float4 nr, float distance, float normal_cos) {
  const float e = plane_dot3(pl.x, pl.y, pl.z, p.x, p.y, p.z) + pl.w;
  bool in = fabsf(e) <= distance;
  if (NRM) in = in && fabsf(plane_dot3(pl.x, pl.y, pl.z, nr.x, nr.y, nr.z)) >= normal_cos;
  return in;
}

__global__ void __launch_bounds__(BLK) k_plane_init(const PlaneArgs A) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n) return;
  const float4 p = A.map.pos_conf[r];
  const bool node = (!A.sel || A.sel[r] != 0) && query_finite3(p.x, p.y, p.z) && p.w > A.min_conf;
  A.node[r] = node ? 1 : 0;
  A.label[r] = PLANE_NONE;
}

__global__ void __launch_bounds__(BLK) k_plane_part(const PlaneArgs A) {
  __shared__ unsigned lds[BLK / 64];
  if (A.st->done) return;   // (uniform: the word is written by the launch before this one at the latest)
  const unsigned i = blockIdx.x * SELECT_ROW + threadIdx.x;
  const bool f = i < A.n && A.node[i] != 0 && A.label[i] == PLANE_NONE;
  if (i < A.n) A.part[i] = f ? 1 : 0;
  unsigned before;
  const unsigned tot = select_block_rank(f, lds, before);
  if (threadIdx.x == 0) A.sc.chunk_count[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(BLK) k_plane_compact(const PlaneArgs A) {
  __shared__ unsigned lds[BLK / 64];
  if (A.st->done) return;
  const unsigned i = blockIdx.x * SELECT_ROW + threadIdx.x;
  const bool f = i < A.n && A.part[i] != 0;
  unsigned before;
  select_block_rank(f, lds, before);
  if (!f) return;
  const unsigned pos = A.sc.chunk_offset[blockIdx.x] + before;   // pos <= i < n
  A.cpos[pos] = A.map.pos_conf[i];
  if (A.normal_cos > 0.f) A.cnrm[pos] = A.map.nrm_rad[i];
}

__global__ void __launch_bounds__(BLK) k_plane_hyp(const PlaneArgs A, unsigned k) {
  const unsigned h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= A.H || A.st->done) return;
  const unsigned M = *A.M;
  const float nan = __builtin_nanf("");
  float4 out = make_float4(nan, nan, nan, nan);
  unsigned ia = 0;
  if (M) {
    const unsigned base = plane_h32(A.seed + 0x9E3779B9u * (k + 1u));
    ia = (unsigned)(((unsigned long long)plane_h32(base ^ (3u * h)) * M) >> 32);
    const unsigned ib = (unsigned)(((unsigned long long)plane_h32(base ^ (3u * h + 1u)) * M) >> 32);
    const unsigned ic = (unsigned)(((unsigned long long)plane_h32(base ^ (3u * h + 2u)) * M) >> 32);
    if (ia != ib && ia != ic && ib != ic) {   // (each index < M by construction)
      const float4 a = A.cpos[ia], b = A.cpos[ib], c = A.cpos[ic];
      const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
      const float vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
      const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
      const float l2 = (cx * cx + cy * cy) + cz * cz;
      if (l2 > 0.f && l2 <= 3.402823466e38f) {
        const float len = outlier_sqrt(l2);
        float nx = outlier_div(cx, len), ny = outlier_div(cy, len), nz = outlier_div(cz, len);
        float d = -plane_dot3(nx, ny, nz, a.x, a.y, a.z);
        bool ok = true;
        if (A.axis_mode != PLANE_AXIS_OFF) {
          const float t = plane_dot3(nx, ny, nz, A.axis[0], A.axis[1], A.axis[2]);
          if (t < 0.f) { nx = -nx; ny = -ny; nz = -nz; d = -d; }
          ok = A.axis_mode == PLANE_AXIS_NORMAL ? fabsf(t) >= A.axis_bound : fabsf(t) <= A.axis_bound;
        }
        if (ok) out = make_float4(nx, ny, nz, d);
      }
    }
  }
  A.hyp[h] = out;
  A.hyp_a[h] = ia;
  A.counts[h] = 0u;
}

template <bool NRM>
__global__ void __launch_bounds__(BLK) k_plane_score(const PlaneArgs A) {
  // the tile by component: four consecutive participants' x are one 16-byte read, which the packed f32 multiplies and adds take as they come
  __shared__ __attribute__((aligned(16))) float s_p[3][SELECT_ROW];
  __shared__ __attribute__((aligned(16))) float s_n[NRM ? 3 : 1][NRM ? SELECT_ROW : 4];
  if (A.st->done) return;
  const unsigned M = *A.M;
  const unsigned r0 = blockIdx.x * (unsigned)PLANE_CHUNK;
  if (r0 >= M) return;   // (uniform)
  const unsigned end = min(M, r0 + (unsigned)PLANE_CHUNK);
  const unsigned h = blockIdx.y * blockDim.x + threadIdx.x;
  const float nan = __builtin_nanf("");
  const float4 pl = h < A.H ? A.hyp[h] : make_float4(nan, nan, nan, nan);
  const float distance = A.distance, normal_cos = A.normal_cos;
  unsigned cnt = 0;
  for (unsigned t0 = r0; t0 < end; t0 += SELECT_ROW) {
    __syncthreads();   // the tile before this one has been read by everybody
    const unsigned i = t0 + threadIdx.x;
    if (i < end) {
      const float4 p = A.cpos[i];
      s_p[0][threadIdx.x] = p.x; s_p[1][threadIdx.x] = p.y; s_p[2][threadIdx.x] = p.z;
      if (NRM) {
        const float4 q = A.cnrm[i];
        s_n[0][threadIdx.x] = q.x; s_n[1][threadIdx.x] = q.y; s_n[2][threadIdx.x] = q.z;
      }
    }
    __syncthreads();
    const unsigned m = min((unsigned)SELECT_ROW, end - t0);
#pragma unroll 4
    for (unsigned j = 0; j < m; ++j) {
      const float4 p = make_float4(s_p[0][j], s_p[1][j], s_p[2][j], 0.f);
      const float4 q = NRM ? make_float4(s_n[0][j], s_n[1][j], s_n[2][j], 0.f) : p;
      cnt += plane_inlier<NRM>(pl, p, q, distance, normal_cos) ? 1u : 0u;
    }
  }
  if (h < A.H && cnt) atomicAdd(&A.counts[h], cnt);
}

// one workgroup: the greatest count, ties to the lowest h; the number of valid hypotheses; the verdict on the round
__global__ void __launch_bounds__(BLK) k_plane_pick(const PlaneArgs A, unsigned k) {
  __shared__ unsigned s_cnt[BLK], s_h[BLK], s_valid;
  if (A.st->done) return;
  const unsigned tid = threadIdx.x;
  if (tid == 0) s_valid = 0u;
  __syncthreads();
  unsigned best = 0, best_h = 0xFFFFFFFFu, valid = 0;
  for (unsigned h = tid; h < A.H; h += BLK) {   // (ascending h: a later one wins only when strictly greater)
    const unsigned c = A.counts[h];
    const float x = A.hyp[h].x;
    valid += x == x ? 1u : 0u;
    if (best_h == 0xFFFFFFFFu || c > best) { best = c; best_h = h; }
  }
  s_cnt[tid] = best;
  s_h[tid] = best_h;
  if (valid) atomicAdd(&s_valid, valid);
  __syncthreads();
  for (unsigned len = BLK / 2; len >= 1; len >>= 1) {
    if (tid < len) {
      const unsigned c = s_cnt[tid + len], h = s_h[tid + len];
      if (c > s_cnt[tid] || (c == s_cnt[tid] && h < s_h[tid])) { s_cnt[tid] = c; s_h[tid] = h; }
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const unsigned M = *A.M;
  if (k == 0) A.res->nodes = M;
  best = s_cnt[0];
  best_h = s_h[0];
  PlaneRound st = *A.st;
  if (M == 0u || best == 0u || best < A.min_inliers) {
    st.done = 1u;
  } else {
    const float4 pl = A.hyp[best_h];
    const float4 a = A.cpos[A.hyp_a[best_h]];
    st.count = best; st.h = best_h; st.valid = s_valid; st.M = M;
    st.hn[0] = pl.x; st.hn[1] = pl.y; st.hn[2] = pl.z; st.hd = pl.w;
    st.a[0] = a.x; st.a[1] = a.y; st.a[2] = a.z;
    st.n[0] = pl.x; st.n[1] = pl.y; st.n[2] = pl.z; st.d = pl.w;
  }
  *A.st = st;
}

// The nine sums of the refinement BY MAP ROW, in the outliers' order: lane j adds the rows j, j + P, j + 2P, ... in ascending order from +0.0
// (a row that is no inlier of the winning hypothesis adds +0.0: no change).  q = (double)p - (double)a.
template <bool NRM>
__global__ void __launch_bounds__(BLK) k_plane_moments(const PlaneArgs A) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (unsigned)OUTLIER_SUM_LANES) return;
  const PlaneRound st = *A.st;
  if (st.done || st.count < 3u) return;
  const float4 pl = make_float4(st.hn[0], st.hn[1], st.hn[2], st.hd);
  const double ax = (double)st.a[0], ay = (double)st.a[1], az = (double)st.a[2];
  double s[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) s[i] = 0.0;
  for (unsigned r0 = j; r0 < A.n; r0 += OUTLIER_AHEAD * OUTLIER_SUM_LANES) {
    float4 p[OUTLIER_AHEAD], nr[OUTLIER_AHEAD];
    bool in[OUTLIER_AHEAD];
#pragma unroll
    for (int i = 0; i < OUTLIER_AHEAD; ++i) {
      const unsigned r = r0 + i * OUTLIER_SUM_LANES;
      const bool live = r >= r0 && r < A.n;   // (r >= r0: no wrap past 2^32)
      in[i] = live && A.part[live ? r : 0u] != 0;
      p[i] = A.map.pos_conf[live ? r : 0u];
      nr[i] = NRM ? A.map.nrm_rad[live ? r : 0u] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < OUTLIER_AHEAD; ++i) {
      if (!in[i] || !plane_inlier<NRM>(pl, p[i], nr[i], A.distance, A.normal_cos)) continue;
      const double qx = (double)p[i].x - ax, qy = (double)p[i].y - ay, qz = (double)p[i].z - az;
      s[0] = s[0] + qx; s[1] = s[1] + qy; s[2] = s[2] + qz;
      s[3] = s[3] + qx * qx; s[4] = s[4] + qx * qy; s[5] = s[5] + qx * qz;
      s[6] = s[6] + qy * qy; s[7] = s[7] + qy * qz; s[8] = s[8] + qz * qz;
    }
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) A.partial[i * OUTLIER_SUM_LANES + j] = s[i];
}

// one workgroup: (refine) twelve rounds of a[i] = a[2i] + a[2i+1] over the partials of each of the nine sums, as k_outlier_finish folds its
// two, then lane 0 runs ef_plane_fit.hpp; the round's model
__global__ void __launch_bounds__(OUTLIER_FINISH) k_plane_fit(const PlaneArgs A, unsigned k) {
  static_assert(OUTLIER_SUM_LANES == 4096 && OUTLIER_SUM_LANES % OUTLIER_FINISH == 0, "twelve rounds");
  __shared__ double a[OUTLIER_SUM_LANES];
  __shared__ double s_sum[9];   // (the nine sums, indexed by the loop below: in LDS, so that no lane keeps an indexed array in scratch)
  const unsigned tid = threadIdx.x;
  PlaneRound st = *A.st;
  if (st.done) return;
  const bool refine = A.refine != 0u && st.count >= 3u;   // (uniform)
  if (refine) {
    for (int w = 0; w < 9; ++w) {
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
      if (tid == 0) s_sum[w] = a[0];
      __syncthreads();
    }
  }
  if (tid != 0) return;
  float thickness = 0.f;
  if (refine) {
    double S[9];
#pragma unroll
    for (int w = 0; w < 9; ++w) S[w] = s_sum[w];
    float n[3], d, th;
    if (plane_fit(S, st.count, st.a, st.hn, n, &d, &th)) {
      st.n[0] = n[0]; st.n[1] = n[1]; st.n[2] = n[2]; st.d = d;
      thickness = th;
      *A.st = st;
    }
  }
  PlaneModel m;
  m.normal[0] = st.n[0]; m.normal[1] = st.n[1]; m.normal[2] = st.n[2]; m.d = st.d;
  m.inliers = 0u;   // k_plane_mark adds them up
  m.sampled_inliers = st.count;
  m.hypothesis = st.h;
  m.valid_hypotheses = st.valid;
  m.participants = st.M;
  m.thickness = thickness;
  A.models[k] = m;
  A.res->planes = k + 1u;
}

// The workgroups stride the rows: at most PLANE_MARK_BLOCKS of them add to the model's one word (a word takes about 88 adds per microsecond:
// one add per SELECT_ROW rows made this kernel 49 us on a million rows, profiles/r29_plane_times.txt)
template <bool NRM>
__global__ void __launch_bounds__(BLK) k_plane_mark(const PlaneArgs A, unsigned k) {
  __shared__ unsigned tot;
  const PlaneRound st = *A.st;
  if (st.done) return;
  if (threadIdx.x == 0) tot = 0u;
  __syncthreads();
  const float4 pl = make_float4(st.n[0], st.n[1], st.n[2], st.d);
  unsigned mine = 0;
  for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < A.n; r += gridDim.x * blockDim.x) {
    if (A.part[r] == 0) continue;
    const float4 nr = NRM ? A.map.nrm_rad[r] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (!plane_inlier<NRM>(pl, A.map.pos_conf[r], nr, A.distance, A.normal_cos)) continue;
    A.label[r] = k;
    ++mine;
  }
  if (mine) atomicAdd(&tot, mine);
  __syncthreads();
  if (threadIdx.x == 0 && tot) atomicAdd(&A.models[k].inliers, tot);
}

__global__ void __launch_bounds__(BLK) k_plane_flags(const PlaneArgs A, int what, int which, uint8_t* __restrict__ flags) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n) return;
  const unsigned l = A.label[r];
  const bool on = l != PLANE_NONE && (which < 0 || l == (unsigned)which);
  flags[r] = (what == PLANES_ON ? on : (A.node[r] != 0 && !on)) ? 1 : 0;
}

__global__ void k_plane_tally(const PlaneArgs A, int which) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  PlaneResult r = *A.res;
  r.on_rows = 0u;
  for (unsigned k = 0; k < r.planes; ++k) r.on_rows += A.models[k].inliers;
  r.off_rows = r.nodes - r.on_rows;
  r.count_after = A.n - (which < 0 ? r.on_rows : A.models[which].inliers);   // (which < PLANE_MAX_PLANES; a plane that was not found has 0)
  *A.res = r;
}

__global__ void __launch_bounds__(BLK) k_plane_split(const PlaneArgs A, uint32_t* __restrict__ label, unsigned rows, PlaneModel* models,
                                                     PlaneResult* res) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (label && r < rows) label[r] = A.label[r];
  if (blockIdx.x != 0) return;
  if (models && threadIdx.x < A.max_planes) models[threadIdx.x] = A.models[threadIdx.x];
  if (res && threadIdx.x == 0) *res = *A.res;
}

}  // namespace

void plane_init(const PlaneArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_plane_init, dim3(ceil_div((int)a.n, BLK)), dim3(BLK), 0, s, a);
}
void plane_round(const PlaneArgs& a, unsigned k, hipStream_t s) {
  const bool nrm = a.normal_cos > 0.f;
  if (a.n) hipLaunchKernelGGL(k_plane_part, dim3(select_chunks(a.n)), dim3(BLK), 0, s, a);
  chunk_totals(a.sc, a.n, a.M, s);   // (n = 0: the scan alone writes M = 0)
  if (a.n) hipLaunchKernelGGL(k_plane_compact, dim3(select_chunks(a.n)), dim3(BLK), 0, s, a);
  const unsigned hg = (a.H + BLK - 1) / BLK;
  hipLaunchKernelGGL(k_plane_hyp, dim3(hg), dim3(BLK), 0, s, a, k);
  if (a.n) {
    const dim3 g((a.n + PLANE_CHUNK - 1) / PLANE_CHUNK, hg);
    if (nrm) hipLaunchKernelGGL(k_plane_score<true>, g, dim3(BLK), 0, s, a);
    else hipLaunchKernelGGL(k_plane_score<false>, g, dim3(BLK), 0, s, a);
  }
  hipLaunchKernelGGL(k_plane_pick, dim3(1), dim3(BLK), 0, s, a, k);
  if (a.refine && a.n) {
    if (nrm) hipLaunchKernelGGL(k_plane_moments<true>, dim3(OUTLIER_SUM_LANES / BLK), dim3(BLK), 0, s, a);
    else hipLaunchKernelGGL(k_plane_moments<false>, dim3(OUTLIER_SUM_LANES / BLK), dim3(BLK), 0, s, a);
  }
  hipLaunchKernelGGL(k_plane_fit, dim3(1), dim3(OUTLIER_FINISH), 0, s, a, k);
  if (a.n) {
    const dim3 g(min(select_chunks(a.n), (unsigned)PLANE_MARK_BLOCKS));
    if (nrm) hipLaunchKernelGGL(k_plane_mark<true>, g, dim3(BLK), 0, s, a, k);
    else hipLaunchKernelGGL(k_plane_mark<false>, g, dim3(BLK), 0, s, a, k);
  }
}
void plane_finish(const PlaneArgs& a, int what, int which, uint8_t* flags, hipStream_t s) {
  if (a.n && flags) hipLaunchKernelGGL(k_plane_flags, dim3(ceil_div((int)a.n, BLK)), dim3(BLK), 0, s, a, what, which, flags);
  hipLaunchKernelGGL(k_plane_tally, dim3(1), dim3(64), 0, s, a, which);
}
void plane_split(const PlaneArgs& a, uint32_t* label, unsigned rows, PlaneModel* models, PlaneResult* res, hipStream_t s) {
  rows = rows < a.n ? rows : a.n;
  if (!label) rows = 0;
  if (rows || models || res)
    hipLaunchKernelGGL(k_plane_split, dim3(rows ? ceil_div((int)rows, BLK) : 1), dim3(BLK), 0, s, a, rows ? label : (uint32_t*)nullptr, rows, models, res);
}
