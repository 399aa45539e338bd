// Carve free space: flag the surfels that depth views see through (ef_map_carve / ef_map_carve_select, include/ef_hip.h; DESIGN.md §8h).
// Included at the end of ef_map_kernels.hip, after ef_thin.inc.  It uses the selection's flag -> count -> scan -> list / compact chain
// (ef_select.inc) unchanged.  No frame kernel reads or writes anything here.
//   flags     k_carve_flags: one lane per map row.  The row's {x, y, z, conf} is the only map stream read (coalesced float4).  Per view the
//             twelve floats of T_cw come from the kernel's argument segment by scalar loads (the view index is uniform), the point is
//             projected, and the depth image is gathered with 2-byte loads: the centre texel first and, only where the centre lies behind the
//             surfel, the window, one image row of up to five texels at a time (clamped addresses, so the loads of a row are unconditional
//             and independent).  Two views are in flight per lane: both centre texels are requested before either is used.
//   counts    k_select_count + k_scan_chunks over the bytes (flags_count of ef_select.inc); lists and the erase are the selection's.  With
//             tally set the kernel also leaves, per chunk of SELECT_ROW rows, the number of participants, observed and free-space rows (wave
//             ballots, as k_select_flags counts): chunk_totals scans them.
// Every loop is bounded by the view count or the window; no workgroup reads what another writes; there are no atomics.
namespace {

// d in metres into zo; true iff the texel has data
__device__ __forceinline__ bool carve_data(const CarveArgs& A, unsigned d, float& zo) {
  zo = (float)d / 1000.0f;
  return d != 0u && A.min_depth <= zo && zo <= A.max_depth;
}
__device__ __forceinline__ float carve_tol(const CarveArgs& A, float zo) { return A.margin + (A.margin_quad * zo) * zo; }

// the row's camera-frame depth and texel in view k; false: the view says nothing (behind the camera, outside the image, not a number)
__device__ __forceinline__ bool carve_project(const CarveArgs& A, int k, float4 p, float& z, int& u, int& v) {
  const float* T = A.Tcw[k];
  const float x = ((T[0] * p.x + T[1] * p.y) + T[2] * p.z) + T[3];
  const float y = ((T[4] * p.x + T[5] * p.y) + T[6] * p.z) + T[7];
  z = ((T[8] * p.x + T[9] * p.y) + T[10] * p.z) + T[11];
  u = v = 0;
  if (!(z > 0.f)) return false;
  const float uf = (A.fx * x) / z + A.cx, vf = (A.fy * y) / z + A.cy;
  if (!(uf >= 0.f && uf < (float)A.width && vf >= 0.f && vf < (float)A.height)) return false;
  u = (int)uf;   // 0 <= uf < width <= 4096: inside the image, and truncation is the floor
  v = (int)vf;
  return true;
}

// the view's vote for a row whose centre texel (u, v) of img holds d: 1 = FREE, 0x100 = SUPPORTED, 0 = nothing (the two counts in one word)
constexpr unsigned CARVE_FREE = 1u, CARVE_SUPPORTED = 0x100u;
__device__ __forceinline__ unsigned carve_vote(const CarveArgs& A, const uint16_t* __restrict__ img, float z, int u, int v, unsigned d) {
  float zo;
  if (!carve_data(A, d, zo)) return 0u;
  const float tol = carve_tol(A, zo);
  // the centre is not behind the surfel: supported unless it is in front of it
  if (!((z + tol) < zo)) return (zo + tol) < z ? 0u : CARVE_SUPPORTED;
  // FREE iff every texel of the window that has data lies behind the surfel.  A texel outside the window or the image reads as 0: no data.
  bool all = true;
  const int w = A.window, W = A.width, H = A.height;
  for (int b = -w; b <= w; ++b) {
    const int vv = v + b;
    if (vv < 0 || vv >= H) continue;
    const uint16_t* __restrict__ row = img + (size_t)vv * W;
    unsigned dd[5];
#pragma unroll
    for (int a = -2; a <= 2; ++a) {
      const int uu = u + a;
      const unsigned t = row[min(max(uu, 0), W - 1)];
      dd[a + 2] = (a >= -w && a <= w && uu >= 0 && uu < W) ? t : 0u;
    }
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      float zq;
      if (carve_data(A, dd[a], zq) && !((z + carve_tol(A, zq)) < zq)) all = false;
    }
  }
  return all ? CARVE_FREE : 0u;
}

__global__ void __launch_bounds__(BLK) k_carve_flags(const CarveArgs A) {
  __shared__ unsigned lds[3][BLK / 64];
  static_assert(CARVE_MAX_VIEWS < 0x100, "a row's two vote counts are bytes");
  const unsigned i = blockIdx.x * SELECT_ROW + threadIdx.x;
  const bool live = i < A.n;
  bool part = false;
  unsigned tally = 0;   // FREE views in the low byte, SUPPORTED views in the next (at most 32 of either)
  if (live) {
    const float4 p = A.pos_conf[i];
    part = (!A.part || A.part[i] != 0) && isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    if (part) {
      const int K = A.n_views;
      const size_t P = (size_t)A.width * A.height;
      for (int k = 0; k < K; k += 2) {
        const int k1 = min(k + 1, K - 1);   // (an odd K: the last pair's second view is switched off below)
        float z0, z1;
        int u0, v0, u1, v1;
        const bool hit0 = carve_project(A, k, p, z0, u0, v0);
        const bool hit1 = carve_project(A, k1, p, z1, u1, v1) && k + 1 < K;
        const uint16_t* __restrict__ img0 = A.depth + (size_t)k * P;
        const uint16_t* __restrict__ img1 = A.depth + (size_t)k1 * P;
        // (u, v) is inside the image in every lane: both loads are unconditional and in flight together
        const unsigned d0 = img0[(size_t)v0 * A.width + u0], d1 = img1[(size_t)v1 * A.width + u1];
        if (hit0) tally += carve_vote(A, img0, z0, u0, v0, d0);
        if (hit1) tally += carve_vote(A, img1, z1, u1, v1, d1);
      }
    }
  }
  const unsigned n_free = tally & 0xFFu, n_support = tally >> 8;
  if (live) {
    const bool free_space = part && n_free >= (unsigned)A.min_views;
    A.removed[i] = (free_space && !(A.protect != 0 && n_support > 0)) ? 1 : 0;
    if (A.votes) {
      A.votes[2 * (size_t)i] = (uint8_t)n_free;
      A.votes[2 * (size_t)i + 1] = (uint8_t)n_support;
    }
  }
  if (!A.tally) return;   // (uniform: the whole workgroup leaves)
  const unsigned long long m0 = __ballot(part), m1 = __ballot(part && n_free + n_support > 0),
                           m2 = __ballot(part && n_free >= (unsigned)A.min_views);
  if ((threadIdx.x & 63) == 0) {
    const unsigned w = threadIdx.x >> 6;
    lds[0][w] = (unsigned)__popcll(m0);
    lds[1][w] = (unsigned)__popcll(m1);
    lds[2][w] = (unsigned)__popcll(m2);
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned tot = 0;
#pragma unroll
    for (int w = 0; w < BLK / 64; ++w) tot += lds[threadIdx.x][w];
    A.tally[(size_t)threadIdx.x * A.tally_stride + blockIdx.x] = tot;
  }
}

}  // namespace

void carve_flags(const CarveArgs& a, hipStream_t s) {
  if (!a.n) return;
  hipLaunchKernelGGL(k_carve_flags, dim3(select_chunks(a.n)), dim3(BLK), 0, s, a);
}
void chunk_totals(const SelectScratch& sc, unsigned n, uint32_t* total, hipStream_t s) { select_scan(sc, n, total, nullptr, 0u, s); }
