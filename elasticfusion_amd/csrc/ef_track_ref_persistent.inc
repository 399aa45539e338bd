// THE REFERENCE ORDER as ONE persistent launch (round 5) — included by ef_track_kernels.hip behind k_track_small, reference-order builds only
// (the shipped default: ef_build.hpp).
// ------------------------------------------------------------------------------------------
// Rounds 3-4 ran the reference-rounding build as k_track_small (128 workgroups, counter barriers, a 29.7 KB all-gather per iteration; levels
// 2 and 1 only) followed by three launches per level-0 iteration.  This is the whole call — k_track_begin, the <= 10 SO(3) iterations and EVERY
// Gauss-Newton iteration of every level (4 + 5 + 10 at the defaults) — as one launch of FT_WGS = 256 co-resident workgroups of 512 threads, on
// the tagged-granule exchanges of ef_track_exchange.inc (round 4's machinery, which does not care in which order a build adds), in the
// REFERENCE's summation order (reduce.cu:57-140, 313-317), bit for bit what the launch-per-step script and the compiled reference compute:
//
//   * Work: column c = 4 b + m (workgroup w runs on XCD w % 8 and takes column rt_column(w): the workgroups of one XCD own a contiguous
//     range of reference blocks) owns virtual warps m and m + 4 of reference block b at EVERY level — k_se3_accum's split: 8 wavefronts =
//     {ICP, photometric} x 2 virtual warps x 2 halves of 16 virtual threads in the quad layout (lane = 4 v + j).  A wavefront walks its
//     passes four at a time in a ROLLED loop (accum_quads_rolled: the next step's loads and gathers in flight behind the current step's
//     arithmetic; k_se3_accum unrolls five steps, which one launch that also carries search, solve, tree and exchange code cannot afford:
//     two CUs share a 64 KB instruction cache).  Every accumulator still sees the reference thread's chain of additions in pass order.
//   * Trees inside the workgroup: warpReduceSum (offset 16 = the other half's wavefront through LDS, 8 .. 1 = lane shuffles) and the first
//     level of blockReduceSum's 8-warp tree (x_m + x_{m+4}): ONE value per accumulator and column goes into exchange B.
//   * Reducer a finishes the reference's tree over the 256 columns: (s0 + s2) + (s1 + s3) per block (lane = block), two warp32 shuffle
//     trees, one add (rt_tree == pair_partials_tree == reduceSum<<<1,1024>>> over blockReduceSum's partials).
//   * The correspondence search runs over exactly the pixels the workgroup's own photometric wavefronts visit (64 per pass), so the packed
//     correspondences never cross a workgroup.
//   * State, admission, the one-workgroup fallback (at the head of k_track_ref_end) and the bounded spins: as k_track_fast.
// Same device functions (visit_stage1 / 2a / 2b, quad_outer, solve_step_wave, so3_row, so3_update), same order: every result is
// bit-identical to the launch-per-step script (tests/test_gpu_frame.py::test_persistent_and_per_step_tracker_scripts_agree) and to the
// compiled reference (tests/test_gpu_vs_reference.py).
// ------------------------------------------------------------------------------------------
constexpr int RT_KC = FT_BLOCK / 64;   // SO(3): passes whose rows one sweep of the workgroup's threads stages
__device__ __forceinline__ int rt_column(int wg) { return (wg & 7) * (FT_WGS >> 3) + (wg >> 3); }
__device__ __forceinline__ int rt_vwarp(int col, int wl) { return 8 * (col >> 2) + (col & 3) + 4 * wl; }
// visit idx of a column: pass idx / 64 of virtual thread idx % 64 of the column's two warps (0..31: warp m, 32..63: warp m + 4)
__device__ __forceinline__ int rt_pixel(int col, int idx) { return (idx >> 6) * VTHREADS + rt_vwarp(col, (idx >> 5) & 1) * 32 + (idx & 31); }

// warpReduceSum over each 32-lane half of the wavefront (val += shfl_down(val, offset) for offset = 16 .. 1, reduce.cu:57-95), then lane 0 adds the
// upper half's sum to its own: the operands every lane ON THE PATH TO LANE 0 adds are those of the __shfl_down formulation (round 6: one VALU
// move per step — row / half-wave swaps and in-row DPP shifts — instead of a trip through the LDS crossbar, 6 dependent ds_bpermute ≈ 0.15 us on
// the critical path of every exchange); lanes off that path hold other values than before, nobody reads them
__device__ __forceinline__ float warp32_pair_tree(float x) {
  x += down16(x);        // lanes 0..15 and 32..47: + lane i + 16
  x += row_down<8>(x);
  x += row_down<4>(x);
  x += row_down<2>(x);
  x += row_down<1>(x);   // lanes 0 and 32: the two warp sums
  return x + down32(x);  // lane 0: warp 0 + warp 1
}
// integer sum over the wavefront, in lane 0 (order-free: exact)
__device__ __forceinline__ int wave_sum_lane0(int v) {
  float x = __int_as_float(v);   // (moved as bits: permlane / DPP moves do not interpret them)
  auto add = [](float a, float b) { return __int_as_float(__float_as_int(a) + __float_as_int(b)); };
  x = add(x, down32(x));
  x = add(x, down16(x));
  x = add(x, row_down<8>(x));
  x = add(x, row_down<4>(x));
  x = add(x, row_down<2>(x));
  x = add(x, row_down<1>(x));
  return __float_as_int(x);
}
// the rest of the reference's tree over one accumulator's 256 column sums: lane l holds columns 4 l .. 4 l + 3 = the pair sums s0 .. s3 of
// reference block l; total in lane 0
__device__ __forceinline__ float rt_tree(float s0, float s1, float s2, float s3) {
  float x = (s0 + s2) + (s1 + s3);
  return warp32_pair_tree(x);
}
// ... as a workgroup-wide pass over plain partials P[acc][256] (the one-workgroup fallback; k_track_end after it)
template <int BLOCK>
__device__ __forceinline__ void rt_tree_plain(const float* __restrict__ P, int na, float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int a = wave; a < na; a += BLOCK / 64) {
    const float4 v = *(const float4*)(P + (size_t)a * 256 + 4 * lane);
    const float x = rt_tree(v.x, v.y, v.z, v.w);
    if (lane == 0) out[a] = x;
  }
}
// the reducer's part of exchange B (one converged wavefront of workgroup a < na)
__device__ __forceinline__ void rt_reduce_publish(const unsigned long long* G1, unsigned long long* G2, int a, unsigned epoch, volatile int* dead_s,
                                                  FtSync* Y, float* plain_out) {
  unsigned d[4];
  ft_sweep_row(G1 + (size_t)a * 256, epoch, dead_s, Y, d);
  const float x = rt_tree(__uint_as_float(d[0]), __uint_as_float(d[1]), __uint_as_float(d[2]), __uint_as_float(d[3]));
  const unsigned xb = (unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint(x));
  const int lane = threadIdx.x & 63;
  if (lane < FT_REPL) ft_put(G2 + (size_t)lane * FT_REPL_STRIDE + a, xb, epoch);   // every copy, one store instruction (G2: the first copy)
  if (lane == 0 && plain_out) plain_out[(size_t)a * 256] = x;   // the launch's last iteration: what k_track_end's head reads (ng = 1)
}

// accum_quads (one wavefront = one half of a virtual warp for ONE term, quad layout) with the steps ROLLED: step s = passes 4 s .. 4 s + 3 of the
// 16 virtual threads; the loads of step s + 1 are issued before the arithmetic of step s and its gathers before step s's outer products.
// `wait_sigma()` is called once, with the first step's loads and gathers in flight: the photometric wavefronts of the persistent
// launch wait THERE for the search's global count.  The chain of every accumulator is accum_quads' (passes in order, one product at a time).
template <bool ICP, typename Hook, bool PAIRS = true>
__device__ __forceinline__ void accum_quads_rolled(const IcpView& IV, const RgbView& RV, const IcpPose& P, int gbase, int N, int K, f32x4 (&c)[3],
                                                   Hook wait_sigma) {
  const int S = (K + 3) >> 2;
  const int lane = threadIdx.x & 63;
  const int jl = lane >> 4, g = gbase + (lane & 15);   // load layout (phase A): lane = 16 jl + vl, see accum_quads
  auto pixel = [&](int s) { const int k = 4 * s + jl; return (s < S && k < K) ? k * VTHREADS + g : N; };
#ifdef EF_RT_PAIRS_STREAM
  // two visits per lane (icp2_* / rgb2_rows, ef_track_kernels.hip): an iteration is steps s, s + 1; the next pair's loads are issued before this
  // pair's arithmetic and its gathers before this pair's outer products.  (PAIRS = false: the one-workgroup fallback inside k_track_ref_end, whose
  // registers are spoken for — same rows, bit for bit)
  if constexpr (PAIRS) {
  if constexpr (ICP) {
    const IcpPose Pu = icp_pose_uniform(P);
    IcpLoads2 Ln = icp2_stage1(IV, pixel(0), pixel(1), N);
    p3 vgn, scpn;
    icp2_transform(Pu, Ln, vgn, scpn);
    IcpGathers2 Gn = icp2_stage2a(IV, Ln, scpn);
    (void)wait_sigma();
#pragma unroll 1
    for (int s = 0; s < S; s += 2) {
      const IcpLoads2 L = Ln;
      const IcpGathers2 G = Gn;
      const p3 vg = vgn, scp = scpn;
      Ln = icp2_stage1(IV, pixel(s + 2), pixel(s + 3), N);
      float ra[8], rb[8];
      icp2_stage2b(IV, Pu, L, G, vg, scp, ra, rb);
      icp2_transform(Pu, Ln, vgn, scpn);
      Gn = icp2_stage2a(IV, Ln, scpn);
      quad_rows_accumulate(ra, s, K, c);
      if (s + 1 < S) quad_rows_accumulate(rb, s + 1, K, c);   // uniform
    }
  } else {
    const bufrsrc rc = buf_of(RV.corres, (unsigned)N * 4u), rdx = buf_of(RV.dIdx, (unsigned)N * 2u), rdy = buf_of(RV.dIdy, (unsigned)N * 2u),
                  rd0 = buf_of(RV.lastDepth, (unsigned)N * 4u);
    // one pair deep: the next pair's loads are issued before this pair's rows, its model-depth gather before this pair's outer products.  (Two pairs
    // deep — gather of pair p + 1 and loads of pair p + 2 in flight behind pair p — was built and measured at 1280 x 960: the launch 546.8 us
    // against 545.7, profiles/r07c_1280x960_kernel_stats*.csv: nothing; dropped.)
    struct Rgb2 { uint32_t corr[2]; int gx[2], gy[2]; bool valid[2]; float d0[2]; };
    auto load = [&](int s, Rgb2& X) {
      const int pa = pixel(s), pb = pixel(s + 1);
      X.valid[0] = pa < N; X.valid[1] = pb < N;
      const unsigned qa = (unsigned)(X.valid[0] ? pa : N - 1), qb = (unsigned)(X.valid[1] ? pb : N - 1);
      X.corr[0] = buf_u32(rc, qa * 4u); X.corr[1] = buf_u32(rc, qb * 4u);
      X.gx[0] = buf_i16(rdx, qa * 2u); X.gx[1] = buf_i16(rdx, qb * 2u);
      X.gy[0] = buf_i16(rdy, qa * 2u); X.gy[1] = buf_i16(rdy, qb * 2u);
    };
    auto gather = [&](Rgb2& X) {   // visit_stage2a's photometric half: the model depth behind the correspondence
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        X.valid[e] = X.valid[e] && (X.corr[e] & 0x80000000u);
        const unsigned zi = X.valid[e] ? ((X.corr[e] >> 11) & 0x7FFu) * (unsigned)RV.cols + (X.corr[e] & 0x7FFu) : 0u;
        X.d0[e] = buf_f32(rd0, zi * 4u, 0u);
      }
    };
    Rgb2 X1;
    load(0, X1);
    gather(X1);
    const float sigma = wait_sigma();
#pragma unroll 1
    for (int s = 0; s < S; s += 2) {
      const Rgb2 X = X1;
      load(s + 2, X1);
      float ra[8], rb[8];
      rgb2_rows(RV, sigma, X.corr, X.gx, X.gy, X.d0, X.valid, ra, rb);
      gather(X1);
      quad_rows_accumulate(ra, s, K, c);
      if (s + 1 < S) quad_rows_accumulate(rb, s + 1, K, c);   // uniform
    }
  }
  return;
  }
#endif
  VisitLoads Lnext = visit_stage1<ICP, !ICP>(IV, RV, pixel(0), N);
  VisitGathers Gnext = visit_stage2a<ICP, !ICP>(IV, RV, P, Lnext);
  const float sigma = wait_sigma();
#pragma unroll 1
  for (int s = 0; s < S; ++s) {
    const VisitLoads L = Lnext;
    const VisitGathers G = Gnext;
    Lnext = visit_stage1<ICP, !ICP>(IV, RV, pixel(s + 1), N);
    float irow[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, grow[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float ifound, gfound;
    visit_stage2b<ICP, !ICP>(IV, RV, P, sigma, L, G, irow, ifound, grow, gfound);
    Gnext = visit_stage2a<ICP, !ICP>(IV, RV, P, Lnext);   // (waits for the next step's loads, issued before this step's arithmetic; its gathers fly during the outer products)
    float rows[8];
#pragma unroll
    for (int q = 0; q < 7; ++q) rows[q] = ICP ? irow[q] : grow[q];
    rows[7] = ICP ? ifound : gfound;
    quad_rows_accumulate(rows, s, K, c);
  }
}
struct RtNoWait { float sigma; __device__ __forceinline__ float operator()() const { return sigma; } };

// ------------------------------------------------------------------------------------------
// LEVEL-RESIDENT inputs (round 6).  Everything a pixel visit reads through the pixel's OWN address does not depend on the pose: the current
// vertex / normal maps (ICP), the frame's depth, intensity, photometric mask and Sobel gradients (search + photometric rows).  A column visits
// the same pixels in every iteration of a level, so its wavefronts load them ONCE per level into LDS (the dynamic region `rt_res`, carved per
// level) and the 4 / 5 / 10 iterations of the level read them from there: per iteration only the pose-dependent GATHERS (model vertex / normal
// behind the projective association, model depth / intensity behind the photometric warp) go to memory — one round trip instead of two on the
// ICP side, and the photometric side needs none between its search and its rows (the search keeps the packed correspondence and the model depth
// it gathered in LDS: the rows' "gather" RV.lastDepth[zi] is the search's own lastDepth[gi], zi == gi).  With the pixel-addressed loads gone the
// search no longer needs the ICP wavefronts: the photometric wavefronts search exactly the visits they accumulate afterwards (same lane, same
// step: no barrier between search and rows), the ICP wavefronts start their gathers at once.
//   slot layouts (per wavefront, S = steps of the level):   ICP  float [S][6][64]   vcurr.xyz, ncurr.xyz
//                                                           RGB  u32   [S][8][64]   nextDepth | x, y << 11, nextImage << 22, (in range && mask) << 30 |
//                                                                                   dIdx & 0xffff, dIdy << 16 | packed correspondence | model depth |
//                                                                                   the model point's x | y | 1 / z (rt_rgb_prepare)
// Same device functions on the same values (visit_stage2a / 2b, quad_outer), every accumulator's chain in pass order: bit-identical to
// accum_quads_rolled.  Levels whose slots do not fit the launch's LDS budget (FtArgs::res_bytes) keep the streaming path: mode 2 = both sides
// resident, 1 = the ICP side only (1280 x 960 level 0: 19 steps), 0 = none.
// ------------------------------------------------------------------------------------------
constexpr int RT_RGB_WORDS = 8;   // per visit: 5 words of the search (below) + 3 of rt_rgb_prepare
constexpr int RT_ICP_STEP_BYTES = 4 * 6 * 64 * 4, RT_RGB_STEP_BYTES = 4 * RT_RGB_WORDS * 64 * 4;   // per step, all four wavefronts of a term
constexpr int RT_CH = 5;    // steps whose gathers are in flight together (640 x 480 level 0: all of them)
// Which parts of the launch evaluate two visits per lane.  Measured same-box (profiles/r06u_ab_visit_pairs_by_part.log): the level-resident paths
// at 640 x 480 are one latency chain per iteration, not instruction issue — the packed ICP rows cost 1.5 % (1819 against 1843 frames/s), the
// packed photometric rows 0.6 %, the packed search nothing either way; the streaming paths (1280 x 960 level 0) gain.  So the resident paths
// keep one visit per lane (their two-visit versions: removed, last present in commit 2372c48) and the streaming path takes two.
#ifdef EF_VISIT_PAIRS
#define EF_RT_PAIRS_STREAM 1
#endif
__device__ __forceinline__ int rt_res_mode(bool has_icp, bool has_rgb, int S, unsigned budget) {
  const unsigned ni = has_icp ? (unsigned)S * RT_ICP_STEP_BYTES : 0u, nr = has_rgb ? (unsigned)S * RT_RGB_STEP_BYTES : 0u;
  if (ni + nr <= budget) return 2;
  return (has_icp && ni <= budget) ? 1 : 0;
}
// this lane's visit of step s in the load layout (lane = 16 jl + vl): pixel, or N when the visit does not exist
__device__ __forceinline__ int rt_visit_pixel(int gbase, int s, int S, int K, int N) {
  const int lane = threadIdx.x & 63, k = 4 * s + (lane >> 4);
  return (s < S && k < K) ? k * VTHREADS + gbase + (lane & 15) : N;
}
// level entry: one wavefront fills the ICP slots of the wavefront whose first virtual thread is gbase
__device__ __forceinline__ void rt_fill_icp(const IcpView& IV, const RgbView& RV, float* slots, int gbase, int N, int K) {
  const int S = (K + 3) >> 2, lane = threadIdx.x & 63;
  for (int s0 = 0; s0 < S; s0 += RT_CH) {
    VisitLoads L[RT_CH];
#pragma unroll
    for (int u = 0; u < RT_CH; ++u) L[u] = visit_stage1<true, false>(IV, RV, rt_visit_pixel(gbase, s0 + u, S, K, N), N);
#pragma unroll
    for (int u = 0; u < RT_CH; ++u) {
      if (s0 + u < S) {
        float* p = slots + (size_t)(s0 + u) * 6 * 64 + lane;
        p[0] = L[u].vcurr.x; p[64] = L[u].vcurr.y; p[128] = L[u].vcurr.z;
        p[192] = L[u].ncurr.x; p[256] = L[u].ncurr.y; p[320] = L[u].ncurr.z;
      }
    }
  }
}
__device__ __forceinline__ void rt_fill_rgb(const PtLevel& Lv, uint32_t* slots, int gbase, int N, int K) {
  const int S = (K + 3) >> 2, lane = threadIdx.x & 63;
  for (int s0 = 0; s0 < S; s0 += RT_CH) {
    float nd[RT_CH];
    int mk[RT_CH], ni[RT_CH], gx[RT_CH], gy[RT_CH], qs[RT_CH];
#pragma unroll
    for (int u = 0; u < RT_CH; ++u) {
      const int q = rt_visit_pixel(gbase, s0 + u, S, K, N);
      const int qq = q < N ? q : N - 1;
      qs[u] = q;
      nd[u] = Lv.nextDepth[qq]; mk[u] = Lv.mask[qq]; ni[u] = Lv.nextImage[qq]; gx[u] = Lv.dIdx[qq]; gy[u] = Lv.dIdy[qq];
    }
#pragma unroll
    for (int u = 0; u < RT_CH; ++u) {
      if (s0 + u < S) {
        const int q = qs[u] < N ? qs[u] : N - 1;
        const int y = q / Lv.cols, x = q - y * Lv.cols;
        uint32_t* p = slots + (size_t)(s0 + u) * RT_RGB_WORDS * 64 + lane;
        p[0] = __float_as_uint(nd[u]);
        p[64] = (uint32_t)x | ((uint32_t)y << 11) | ((uint32_t)ni[u] << 22) | ((qs[u] < N && mk[u]) ? (1u << 30) : 0u);
        p[128] = ((uint32_t)gx[u] & 0xFFFFu) | ((uint32_t)gy[u] << 16);
      }
    }
  }
}
// one step's rows -> the three outer products of its (up to) four passes, in pass order (phase B)
__device__ __forceinline__ void rt_rows_to_sums(float (&rows)[8], int s, int K, f32x4 (&c)[3]) { quad_rows_accumulate(rows, s, K, c); }
// accum_quads<ICP> on level-resident pixel data: RT_CH steps' gathers in flight together, the current vertex / normal from LDS
__device__ __forceinline__ void rt_icp_resident(const IcpView& IV, const RgbView& RV, const IcpPose& P, const float* slots, int gbase, int N, int K,
                                                f32x4 (&c)[3]) {
  const int S = (K + 3) >> 2, lane = threadIdx.x & 63;
  auto load = [&](int s) {
    VisitLoads L;
    const float* p = slots + (size_t)(s < S ? s : S - 1) * 6 * 64 + lane;
    L.vcurr = f3{p[0], p[64], p[128]};
    L.ncurr = f3{p[192], p[256], p[320]};
    L.corr = 0u;
    L.gx = L.gy = 0;
    L.inb = rt_visit_pixel(gbase, s, S, K, N) < N;
    return L;
  };
#pragma unroll 1
  for (int s0 = 0; s0 < S; s0 += RT_CH) {
    // what stays in registers across the round trip: the gathered model vertex / normal and their address (vcurr_g is recomputed from the slot:
    // the same operations on the same values).  (Issuing the NEXT round's gathers before this round's rows — a level of several rounds waits a
    // round trip per round — needs a second set of 35 registers: the launch spilt, round 6.)
    f3 vprev[RT_CH], nprev[RT_CH];
    int pidx[RT_CH];
#pragma unroll
    for (int u = 0; u < RT_CH; ++u) {
      const VisitGathers G = visit_stage2a<true, false>(IV, RV, P, load(s0 + u));
      vprev[u] = G.vprev_g; nprev[u] = G.nprev_g; pidx[u] = G.pidx;
    }
#pragma unroll
    for (int u = 0; u < RT_CH; ++u) {
      if (s0 + u < S) {   // uniform
        const VisitLoads L = load(s0 + u);
        VisitGathers G;
        G.vcurr_g = mul(P.Rcurr, L.vcurr) + P.tcurr;   // visit_stage2a's
        G.vprev_g = vprev[u]; G.nprev_g = nprev[u]; G.pidx = pidx[u];
        G.d0 = 0.f; G.zi = -1; G.zx = G.zy = 0;
        float irow[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, grow[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float ifound, gfound;
        visit_stage2b<true, false>(IV, RV, P, 0.f, L, G, irow, ifound, grow, gfound);
        float rows[8] = {irow[0], irow[1], irow[2], irow[3], irow[4], irow[5], irow[6], ifound};
        rt_rows_to_sums(rows, s0 + u, K, c);
      }
    }
  }
}
// the photometric wavefront's search over ITS OWN visits (k_track_step's body / residualKernel, reduce.cu:631-667, on the level-resident pixel
// data): packed correspondence + the model depth it gathered go into the wavefront's slots; returns this lane's {count, sum diff^2}
__device__ __forceinline__ void rt_rgb_search(const PtLevel& Lv, const m33& Km, const f3& kt, uint32_t* slots, int K, int& cnt, int& sq) {
  const int S = (K + 3) >> 2, lane = threadIdx.x & 63, cols = Lv.cols, rows = Lv.rows;
  cnt = sq = 0;
#pragma unroll 1
  for (int s0 = 0; s0 < S; s0 += RT_CH) {
    int u0s[RT_CH], v0s[RT_CH], gi[RT_CH], nis[RT_CH], lis[RT_CH];
    float td1[RT_CH], d0s[RT_CH];
#pragma unroll
    for (int u = 0; u < RT_CH; ++u) {
      const uint32_t* p = slots + (size_t)(s0 + u < S ? s0 + u : S - 1) * RT_RGB_WORDS * 64 + lane;
      const float d1 = __uint_as_float(p[0]);
      const uint32_t w = p[64];
      const int x = (int)(w & 0x7FFu), y = (int)((w >> 11) & 0x7FFu);
      const bool m = s0 + u < S && (w & (1u << 30));
      nis[u] = (int)((w >> 22) & 0xFFu);
      td1[u] = (float)(d1 * (Km.r[2].x * x + Km.r[2].y * y + Km.r[2].z) + kt.z);
      u0s[u] = f2i_rn((d1 * (Km.r[0].x * x + Km.r[0].y * y + Km.r[0].z) + kt.x) / td1[u]);
      v0s[u] = f2i_rn((d1 * (Km.r[1].x * x + Km.r[1].y * y + Km.r[1].z) + kt.y) / td1[u]);
      gi[u] = (m && u0s[u] >= 0 && v0s[u] >= 0 && u0s[u] < cols && v0s[u] < rows) ? v0s[u] * cols + u0s[u] : -1;
      d0s[u] = 0.f;
      lis[u] = 0;
      if (gi[u] >= 0) { d0s[u] = Lv.lastDepth[gi[u]]; lis[u] = Lv.lastImage[gi[u]]; }
    }
#pragma unroll
    for (int u = 0; u < RT_CH; ++u) {
      if (s0 + u < S) {   // uniform
        uint32_t packed = 0u;
        if (gi[u] >= 0 && d0s[u] > 0 && fabsf(td1[u] - d0s[u]) <= 0.07f /* maxDepthDeltaRGB, RGBDOdometry.cpp:41 */ && lis[u] != 0) {
          const int idiff = nis[u] - lis[u];
          packed = pack_corres(u0s[u], v0s[u], idiff);
          cnt += 1;
          sq += idiff * idiff;
        }
        uint32_t* p = slots + (size_t)(s0 + u) * RT_RGB_WORDS * 64 + lane;
        p[192] = packed;
        p[256] = __float_as_uint(d0s[u]);
      }
    }
  }
}
// What the photometric rows need that does NOT depend on sigma — the model point behind the correspondence (projectPointsKernel folded in,
// cudafuncs.cu:670-688) and 1 / z, the one double-precision division of a row (reduce.cu:447) — evaluated by every photometric wavefront for ITS
// visits right behind its search, i.e. while the column's record of exchange A is under way: off the critical path search -> A -> rows -> B.
// Same expressions on the same values as rgb_row; results parked in the wavefront's slots (same lane, same step: no barrier).
__device__ __forceinline__ void rt_rgb_prepare(const RgbView& RV, uint32_t* slots, int K) {
  const int S = (K + 3) >> 2, lane = threadIdx.x & 63;
  const float invFx = 1.0f / RV.k.fx, invFy = 1.0f / RV.k.fy;
#pragma unroll 1
  for (int s0 = 0; s0 < S; s0 += RT_CH) {
    uint32_t corr[RT_CH];
    float d0[RT_CH];
#pragma unroll
    for (int u = 0; u < RT_CH; ++u) {
      const uint32_t* p = slots + (size_t)(s0 + u < S ? s0 + u : S - 1) * RT_RGB_WORDS * 64 + lane;
      corr[u] = p[192];
      d0[u] = __uint_as_float(p[256]);
    }
#pragma unroll
    for (int u = 0; u < RT_CH; ++u) {
      if (s0 + u < S) {   // uniform
        const f3 pt = project_point((int)(corr[u] & 0x7FFu), (int)((corr[u] >> 11) & 0x7FFu), d0[u], invFx, invFy, RV.k.cx, RV.k.cy);
        const float invz = (float)(1.0 / (double)pt.z);
        uint32_t* p = slots + (size_t)(s0 + u) * RT_RGB_WORDS * 64 + lane;
        p[320] = __float_as_uint(pt.x);
        p[384] = __float_as_uint(pt.y);
        p[448] = __float_as_uint(invz);
      }
    }
  }
}
// accum_quads<RGB> on the wavefront's slots: no memory access at all; the rest of rgb_row<true> (reduce.cu:420-476) behind rt_rgb_prepare
__device__ __forceinline__ void rt_rgb_resident(const IcpView& IV, const RgbView& RV, const IcpPose& P, float sigma, const uint32_t* slots, int K,
                                                f32x4 (&c)[3]) {
  (void)IV; (void)P;
  const int S = (K + 3) >> 2, lane = threadIdx.x & 63;
#pragma unroll 1
  for (int s = 0; s < S; ++s) {
    const uint32_t* p = slots + (size_t)s * RT_RGB_WORDS * 64 + lane;
    const uint32_t gxy = p[128], corr = p[192];
    const f3 pt{__uint_as_float(p[320]), __uint_as_float(p[384]), __uint_as_float(p[256])};
    const float invz = __uint_as_float(p[448]);
    float rows[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (corr & 0x80000000u) {
      const int gx = (int)(int16_t)(gxy & 0xFFFFu), gy = (int)(int16_t)(gxy >> 16);
      const float diff = (float)((int)((corr >> 22) & 0x1FFu) - 255);
      float w = sigma + fabsf(diff);
      w = w > 1.19209290E-07F ? 1.0f / w : 1.0f;
      if (sigma == -1) w = 1;
      rows[6] = -w * diff;
      const float dI_dx_val = w * RV.sobelScale * gx;
      const float dI_dy_val = w * RV.sobelScale * gy;
      const float v0 = dI_dx_val * RV.k.fx * invz;
      const float v1 = dI_dy_val * RV.k.fy * invz;
      const float v2 = -(v0 * pt.x + v1 * pt.y) * invz;
      rows[0] = v0; rows[1] = v1; rows[2] = v2;
      rows[3] = -pt.z * v1 + pt.y * v2;
      rows[4] = pt.z * v0 - pt.x * v2;
      rows[5] = -pt.y * v0 + pt.x * v1;
      rows[7] = 1.f;
    }
    rt_rows_to_sums(rows, s, K, c);
  }
}
#define EF_RT_RGB_PREPARE 1

// The trees of one column behind its wavefronts' sums c[] (k_se3_accum's tail): call with the whole workgroup (two __syncthreads inside).
// Wavefront = (term, virtual warp wl, half): 0-3 the launch's first term, 4-7 the second.  On return the lanes 0..3 (v = 0, j = lane) of
// wavefront (term, wl 0, half 0) hold in r[q * 4 + i] the pair sum x_m + x_{m+4} of member quad_member(q, i, j); other lanes hold nothing.
template <int NT>
__device__ __forceinline__ void rt_column_trees(const f32x4 (&c)[3], float* xch /* [2][NT][12][64] */, float* pairx /* [NT][12][4] */, float (&r)[12]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int v = lane >> 2, j = lane & 3;
  const int tix = wave >> 2, rem = wave & 3, wl = rem >> 1, half = rem & 1;
  const bool active = wave < 4 * NT;
  float* xw = xch + (size_t)((active ? wl : 0) * NT + (active ? tix : 0)) * 12 * 64;
  // warpReduceSum, reduce.cu:57-95: val += shfl_down(val, offset) for offset = 16 (the other half's wavefront), 8, 4, 2, 1
  if (active && half == 1) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      xw[(q * 4 + 0) * 64 + lane] = c[q].x; xw[(q * 4 + 1) * 64 + lane] = c[q].y;
      xw[(q * 4 + 2) * 64 + lane] = c[q].z; xw[(q * 4 + 3) * 64 + lane] = c[q].w;
    }
  }
  __syncthreads();
  if (active && half == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      r[q * 4 + 0] = c[q].x + xw[(q * 4 + 0) * 64 + lane]; r[q * 4 + 1] = c[q].y + xw[(q * 4 + 1) * 64 + lane];
      r[q * 4 + 2] = c[q].z + xw[(q * 4 + 2) * 64 + lane]; r[q * 4 + 3] = c[q].w + xw[(q * 4 + 3) * 64 + lane];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {   // offsets 8, 4, 2, 1 in virtual threads = 32, 16, 8, 4 lanes
      r[i] += down32(r[i]);
      r[i] += down16(r[i]);
      r[i] += row_down<8>(r[i]);
      r[i] += row_down<4>(r[i]);
    }
    // blockReduceSum's second stage (reduce.cu:97-117), first level: shfl_down(offset 4) adds warp m + 4 to warp m — the column's pair
    if (wl == 1 && v == 0) {
#pragma unroll
      for (int i = 0; i < 12; ++i) pairx[((size_t)tix * 12 + i) * 4 + j] = r[i];
    }
  }
  __syncthreads();
  if (active && half == 0 && wl == 0 && v == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) r[i] = r[i] + pairx[((size_t)tix * 12 + i) * 4 + j];
  }
}
// One column's share of the normal equations (k_se3_accum's body) on the STREAMING path: call with the whole workgroup (512 threads; two
// __syncthreads inside).  icp_slots != null: the ICP wavefronts read their pixel data from the level-resident slots (mode 1).
template <bool HAS_ICP, bool HAS_RGB, bool PAIRS = true, typename Hook>
__device__ __forceinline__ void rt_accumulate(const IcpView& IV, const RgbView& RV, const IcpPose& P, int col, int N, int K,
                                              float* xch /* [2][NT][12][64] */, float* pairx /* [NT][12][4] */, float (&r)[12], Hook wait_sigma,
                                              const float* icp_slots = nullptr) {
  constexpr int NT = (HAS_ICP && HAS_RGB) ? 2 : 1;
  const int wave = threadIdx.x >> 6;
  const int tix = wave >> 2, rem = wave & 3, wl = rem >> 1, half = rem & 1;
  const bool active = wave < 4 * NT;
  const bool rgb_wave = HAS_RGB && (!HAS_ICP || tix == 1);
  f32x4 c[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) c[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (active) {
    const int gbase = rt_vwarp(col, wl) * 32 + half * 16;
    if (HAS_ICP && !rgb_wave) {
      if (icp_slots) rt_icp_resident(IV, RV, P, icp_slots + (size_t)rem * ((K + 3) >> 2) * 6 * 64, gbase, N, K, c);
      else accum_quads_rolled<true, RtNoWait, PAIRS>(IV, RV, P, gbase, N, K, c, RtNoWait{0.f});
    }
    if (HAS_RGB && rgb_wave) accum_quads_rolled<false, Hook, PAIRS>(IV, RV, P, gbase, N, K, c, wait_sigma);
  }
  rt_column_trees<NT>(c, xch, pairx, r);
}
// SO(3): one column's share of so3Step in the reference's order (so3_accumulate's arithmetic): the rows of RT_KC passes of the column's 64
// virtual threads per sweep, the chains by wavefront 0 (lane = virtual thread: 0..31 warp m, 32..63 warp m + 4), warp32 trees, the pair.
// Call with the whole workgroup; on return lane 0 of wavefront 0 holds the pair sums in z[].
__device__ __forceinline__ void rt_so3_accumulate(const uint8_t* __restrict__ lastImage, const uint8_t* __restrict__ nextImage, int cols, int rows,
                                                  const m33& IB, const m33& KI, const m33& KR, int col, float* lds_rows /* [RT_KC][5][64] */,
                                                  float (&z)[SO3_ACCS]) {
  const int t = threadIdx.x, lane = t & 63, N = cols * rows;
  const int K = (N + VTHREADS - 1) / VTHREADS;
  const int gl = rt_vwarp(col, lane >> 5) * 32 + (lane & 31);
  const int nk = gl < N ? (N - gl + VTHREADS - 1) / VTHREADS : 0;
#pragma unroll
  for (int i = 0; i < SO3_ACCS; ++i) z[i] = 0.f;
  for (int k0 = 0; k0 < K; k0 += RT_KC) {
    const int kc = min(RT_KC, K - k0);
    {
      const int k = t >> 6;
      if (k < kc) {
        const int p = rt_pixel(col, (k0 + k) * 64 + lane);
        float row[4] = {0.f, 0.f, 0.f, 0.f};
        float found = 0.f;
        if (p < N && so3_row(lastImage, nextImage, cols, rows, IB, KI, KR, p, row)) found = 1.f;
        float* rr = lds_rows + (size_t)k * 5 * 64 + lane;
        rr[0] = row[0]; rr[64] = row[1]; rr[128] = row[2]; rr[192] = row[3]; rr[256] = found;
      }
    }
    __syncthreads();
    if (t < 64) {
      const int kend = min(kc, nk - k0);
      for (int k = 0; k < kend; ++k) {
        const float* rr = lds_rows + (size_t)k * 5 * 64 + lane;
        const float r0 = rr[0], r1 = rr[64], r2 = rr[128], r3 = rr[192], f = rr[256];
        z[0] = EF_FMA(r0, r0, z[0]); z[1] = EF_FMA(r0, r1, z[1]); z[2] = EF_FMA(r0, r2, z[2]); z[3] = EF_FMA(r0, r3, z[3]);
        z[4] = EF_FMA(r1, r1, z[4]); z[5] = EF_FMA(r1, r2, z[5]); z[6] = EF_FMA(r1, r3, z[6]);
        z[7] = EF_FMA(r2, r2, z[7]); z[8] = EF_FMA(r2, r3, z[8]);
        z[9] = EF_FMA(r3, r3, z[9]);
        z[10] += f;
      }
    }
    __syncthreads();
  }
  if (t < 64) {
#pragma unroll
    for (int i = 0; i < SO3_ACCS; ++i) {
      z[i] = warp32_pair_tree(z[i]);   // lane 0: x_m + x_{m+4}
    }
  }
}

template <bool HAS_ICP, bool HAS_RGB>
__global__ void __launch_bounds__(FT_BLOCK) k_track_ref(const FtArgs A, TrackState* st) {
  constexpr int NT = (HAS_ICP && HAS_RGB) ? 2 : 1;
  constexpr int NA = NT * SE3_ACCS;
  __shared__ GNState gs[2];
  __shared__ efs::SolveScratch S;
  __shared__ float sums_s[2 * SE3_ACCS];
  __shared__ float bg[24];   // Rprev[9] | tprev[3] | Rprev_inv[9]: constants of the call (k_track_begin)
  __shared__ float xch[2 * 2 * 12 * 64];
  __shared__ float pairx[2 * 12 * 4];
  __shared__ float lds_rows[RT_KC * 5 * 64];
  __shared__ float red[SO3_ACCS];
  __shared__ So3Loop Z;
  __shared__ int ired[2 * FT_BLOCK / 64];
  __shared__ int tot_s[2];           // {count, sum diff^2} of the iteration's search over the whole image
  __shared__ unsigned seen_a[2];     // exchange A relay: {epoch the workgroup's sweeping wavefront has completed, wait abandoned}
  __shared__ int dead_s;
  __shared__ unsigned mode_s;
  __shared__ int wsum[4][2];         // resident levels: {count, sum diff^2} of each photometric wavefront's own search ...
  __shared__ unsigned wtag[4];       // ... tagged with the exchange-A epoch it belongs to
  extern __shared__ __attribute__((aligned(16))) float rt_res[];   // level-resident pixel data (FtArgs::res_bytes; carved per level)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wg = blockIdx.x;
  const int col = rt_column(wg);
  constexpr int RGB_W0 = HAS_ICP ? 4 : 0;   // first photometric wavefront
#ifdef EF_STAGE_CLOCKS
  unsigned long long clk_last2 = 0;         // lane 0 of the first photometric wavefront (resident levels)
#define FT_CLK2(i) do { if (wg == 0 && t == RGB_W0 * 64) { const unsigned long long now_ = wall_clock64(); (void)__hip_atomic_fetch_add(&Y->clk[i], now_ - clk_last2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); clk_last2 = now_; } } while (0)
#else
#define FT_CLK2(i) do { } while (0)
#endif
  unsigned long long* G1 = (unsigned long long*)(A.partials + FT_G1_OFF);
  unsigned long long* G2 = (unsigned long long*)(A.partials + FT_G2R_OFF);   // first of FT_REPL copies (ef_track_exchange.inc)
  unsigned long long* GA = (unsigned long long*)(A.partials + FT_GAR_OFF);
  const unsigned long long* G2_mine = G2 + (size_t)(blockIdx.x & (FT_REPL - 1)) * FT_REPL_STRIDE;   // the copy this workgroup polls
  const unsigned long long* GA_mine = GA + (size_t)(blockIdx.x & (FT_REPL_A - 1)) * FT_REPL_STRIDE;
  FtSync* Y = (FtSync*)(A.partials + FT_SY_OFF);
#ifdef EF_STAGE_CLOCKS
  unsigned long long clk_last = wall_clock64();
  const unsigned long long clk_start = clk_last;
#endif
  // ---- the model side is known to be empty (local loop closure without an inactive surface in view: the common frame): nineteen iterations
  // without a single correspondence leave the state k_track_begin set up, zero sums and zero counts — written here by workgroup 0, at once
  if (A.empty_model_flag && *A.empty_model_flag != A.empty_model_value) {   // uniform: every workgroup reads the same word
    if (wg != 0 || t != 0) return;
    double R[9];
    efl::quat_to_mat<double>(st->q, R);
    GNState& o = st->gn[A.out_cur];
    float Rp[9], Rpi[9];
    for (int i = 0; i < 9; ++i) Rp[i] = o.Rcurr[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) o.tcurr[i] = (float)st->t[i];
    efl::m3_inverse<float>(Rp, Rpi);
    efl::m4_identity(o.resultRt);
    o.rgb_broken = 0;
    o.lastRGBErrorLevel = 0.f;
    compute_krk(o.resultRt, A.L[0].k, o.krkinv, o.kt);
    for (int i = 0; i < 9; ++i) { st->Rprev[i] = Rp[i]; st->Rprev_inv[i] = Rpi[i]; }
    for (int i = 0; i < 3; ++i) st->tprev[i] = o.tcurr[i];
    for (int i = 0; i < 4; ++i) st->q_prev[i] = st->q[i];
    for (int i = 0; i < 3; ++i) st->t_prev[i] = st->t[i];
    for (int i = 0; i < RGB_SLOTS; ++i) st->rgb_slots[0][i][0] = st->rgb_slots[0][i][1] = st->rgb_slots[1][i][0] = st->rgb_slots[1][i][1] = 0;
    st->call_seq += 1u;
    st->so3_iterations = 0;
    st->so3_ticket = 0;
    st->so3_done = 1;
    st->dense_count = 0;
    float* P = A.partials + FT_P_OFF;
    for (int a = 0; a < NA; ++a) P[(size_t)a * 256] = 0.f;   // the totals k_track_end's head reads (ng = 1)
    return;
  }
  // ---- admission (beside k_track_begin below, on other wavefronts): see k_track_fast.  Every workgroup reports in; workgroup 0 waits a
  // bounded time for the whole grid and publishes the verdict: PERSISTENT (everybody is here and stays) or SERIAL (other work holds some
  // of the chip's CUs: every workgroup leaves without having touched the state, and k_track_ref_end, enqueued behind every persistent
  // launch, runs the whole call on its one workgroup: the same bits, no host in the loop)
  if (t == 64) ft_put(&Y->arrive[wg], 1u, A.epoch);
  if (wg == 0 && wave == 7) {
    bool ok[4] = {false, false, false, false};
    bool all = false;
    for (int spin = 0; spin < FT_ADMIT_SPIN && !all; ++spin) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (!ok[i]) ok[i] = (unsigned)(ft_get(&Y->arrive[64 * i + lane]) >> 32) == A.epoch;   // (a load instruction on four whole lines: §5.2d)
      all = __all(ok[0] && ok[1] && ok[2] && ok[3]);
      if (!all && spin > 8) __builtin_amdgcn_s_sleep(2);
    }
    if (!all) {   // (uniform) what the serial run needs to know about this call: the kernel-argument segment, copied AS MEMORY by the wavefront's lanes
      // (`Y->args = A` makes the compiler keep a copy of the by-value argument in scratch for the whole launch: 256 bytes per lane)
      static_assert(sizeof(FtArgs) % 4 == 0, "copied dword by dword");
      typedef const __attribute__((address_space(4))) unsigned* KWords;
      const KWords src = (KWords)__builtin_amdgcn_kernarg_segment_ptr();   // FtArgs is the kernel's FIRST argument
      unsigned* dst = (unsigned*)&Y->args;
      for (int i = lane; i < (int)(sizeof(FtArgs) / 4); i += 64) dst[i] = src[i];
    }
    if (lane == 0 && !all) {
      __hip_atomic_fetch_add(&Y->fallbacks, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      drain_stores();   // (a wait of the whole wavefront: the copy of the arguments above is behind it too)
    }
    // the verdict: one copy per copy of the totals (word FT_MODE_WORD of each: 256 workgroups polled ONE word), and FtSync::mode for the launch behind
    const unsigned verdict = all ? FT_MODE_PERSISTENT : FT_MODE_SERIAL;
    if (lane < FT_REPL) ft_put(G2 + (size_t)lane * FT_REPL_STRIDE + FT_MODE_WORD, verdict, A.epoch);
    if (lane == 0) ft_put(&Y->mode, verdict, A.epoch);
  }
  if (t == 128) {
    unsigned m = 0u;
    for (int spin = 0; spin < FT_SPIN; ++spin) {
      const unsigned long long g = ft_get(G2_mine + FT_MODE_WORD);
      if ((unsigned)(g >> 32) == A.epoch) { m = (unsigned)g; break; }
      if (spin > 8) __builtin_amdgcn_s_sleep(1);
    }
    mode_s = m;   // 0: no verdict within seconds (workgroup 0 never ran?): treated like a time-out below
  }
  // ---- k_track_begin, by every workgroup for itself (LDS only: the global side waits for the verdict) ----
  if (t == 0) {
    dead_s = (int)__hip_atomic_load(&Y->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    seen_a[0] = 0u;
    seen_a[1] = 0u;
    tot_s[0] = tot_s[1] = 0;
    wtag[0] = wtag[1] = wtag[2] = wtag[3] = 0u;
    double R[9];
    efl::quat_to_mat<double>(st->q, R);
    GNState& g = gs[0];
    for (int i = 0; i < 9; ++i) bg[i] = g.Rcurr[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) bg[9 + i] = g.tcurr[i] = (float)st->t[i];
    efl::m3_inverse<float>(bg, bg + 12);
    efl::m4_identity(g.resultRt);
    g.rgb_broken = 0;
    g.lastRGBErrorLevel = 3.402823466e+38f;
    if (!A.so3) compute_krk(g.resultRt, A.kfirst, g.krkinv, g.kt);
  }
  __syncthreads();
  FT_CLK(0);   // begin + admission
  if (dead_s) return;   // an earlier launch of this tracker instance timed out
  if (mode_s == 0u) {   // (bounded like every spin; with the verdict missing nothing can be trusted)
    if (t == 0) __hip_atomic_store(&Y->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (mode_s == FT_MODE_SERIAL) return;   // k_track_ref_end, the launch behind this one, runs the call on its one workgroup first
  if (wg == 0 && t == 0) {   // the global side of k_track_begin (only once the call is known to run here: ADVICE r4)
    for (int i = 0; i < 9; ++i) { st->Rprev[i] = bg[i]; st->Rprev_inv[i] = bg[12 + i]; }
    for (int i = 0; i < 3; ++i) st->tprev[i] = bg[9 + i];
    for (int i = 0; i < 4; ++i) st->q_prev[i] = st->q[i];
    for (int i = 0; i < 3; ++i) st->t_prev[i] = st->t[i];
    for (int i = 0; i < RGB_SLOTS; ++i) st->rgb_slots[0][i][0] = st->rgb_slots[0][i][1] = st->rgb_slots[1][i][0] = st->rgb_slots[1][i][1] = 0;
    st->call_seq += 1u;
    st->so3_iterations = 0;
    st->so3_ticket = 0;
    st->so3_done = 1;
    st->dense_count = 0;
  }
  unsigned epoch = A.epoch;
  int cur = 0;
  // ---- SO(3) pre-alignment, RGBDOdometry.cpp:284-369 ----
  if (A.so3) {
    if (t == 0) {
      efl::m3_identity(Z.resR);
      efl::m3_identity(Z.lastResR);
      for (int i = 0; i < 9; ++i) Z.R_lr[i] = (i % 4 == 0) ? 1.f : 0.f;
      Z.lastError = 3.402823466e+38f / 2;
      Z.lastCount = 3.402823466e+38f / 2;
      Z.done = 0;
      so3_matrices(Z.resR, A.kso3, Z.mats);
    }
    __syncthreads();
    for (int it = 0; it < 10; ++it, ++epoch) {
      {
        const m33 IB = m33_load(Z.mats), KI = m33_load(Z.mats + 9), KR = m33_load(Z.mats + 18);
        float z[SO3_ACCS];
        rt_so3_accumulate(A.so3_last, A.so3_next, A.so3_cols, A.so3_rows, IB, KI, KR, col, lds_rows, z);
        if (t == 0) {
#pragma unroll
          for (int i = 0; i < SO3_ACCS; ++i) ft_put(G1 + (size_t)i * 256 + ft_slot(col), __float_as_uint(z[i]), epoch);
        }
      }
      FT_CLK(1);   // SO(3): rows, chains, publish
      if (wave == 1 && wg < SO3_ACCS) rt_reduce_publish(G1, G2, wg, epoch, &dead_s, Y, nullptr);
      if (wave == 0) {
        float v;
        ft_poll_totals(G2_mine, SO3_ACCS, epoch, &dead_s, Y, v);
        if (lane < SO3_ACCS) red[lane] = v;
      }
      __syncthreads();
      FT_CLK(2);   // SO(3): exchange
      if (t == 0) Z.done = so3_update(Z, red, it, A.kso3, A.kfirst, gs[0]) ? 1 : 0;
      __syncthreads();
      FT_CLK(4);   // SO(3): update
      FT_COUNT(20);
      if (Z.done) { ++epoch; break; }   // every workgroup computes the same bits, so every workgroup leaves in the same iteration
    }
    if (wg == 0 && t == 0) {
      st->lastSO3Error = Z.err;
      st->lastSO3Count = Z.cnt;
      st->so3_iterations = Z.iterations;
    }
  }
  // ---- the Gauss-Newton iterations, RGBDOdometry.cpp:371-553 ----
  for (int it = 0; it < A.n_iter; ++it) {
    const int lvl = ft_level_of(A.levels, it);
#ifdef EF_STAGE_CLOCKS
    const unsigned long long clk_iter = wall_clock64();
#endif
    const PtLevel Lv = ft_load_level((FtArgsK)__builtin_amdgcn_kernarg_segment_ptr(), lvl);   // FtArgs is the kernel's FIRST argument
    const int cols = Lv.cols, rows = Lv.rows, N = cols * rows;
    const int K = (N + VTHREADS - 1) / VTHREADS;
    const bool last = it == A.n_iter - 1;
    // level-resident pixel data (see rt_res_mode): the slots of this level, filled when the level is entered — by every wavefront for itself,
    // wavefront 0's (busy with the update step below) by wavefront 7 — while the update step runs
    const int NS = (K + 3) >> 2;   // steps of the level (four passes each)
    const int res = rt_res_mode(HAS_ICP, HAS_RGB, NS, A.res_bytes);
    float* const icp_res = rt_res;
    uint32_t* const rgb_res = (uint32_t*)(rt_res + (HAS_ICP ? (size_t)NS * (RT_ICP_STEP_BYTES / 4) : 0));
    const IcpView IV{Lv.vmap_curr, Lv.nmap_curr, Lv.vmap_g_prev, Lv.nmap_g_prev, cols, rows, Lv.k, A.distThres, A.angleThres, A.dist2Max, A.sine2Max};
    const RgbView RV{Lv.corres, Lv.lastDepth, nullptr, Lv.dIdx, Lv.dIdy, cols, rows, Lv.k, 1.0f / 8.0f};
    if (res && (it == 0 || lvl != ft_level_of(A.levels, it - 1))) {
      const int nfill = wave == 0 ? 0 : (wave == 7 ? 2 : 1);   // wavefront w: its own slots; wavefront 7: then wavefront 0's
#pragma unroll 1
      for (int f = 0; f < nfill; ++f) {
        const int w = f == 0 ? wave : 0, rem = w & 3;
        const int gbase = rt_vwarp(col, rem >> 1) * 32 + (rem & 1) * 16;
        if (HAS_ICP && w < 4) rt_fill_icp(IV, RV, icp_res + (size_t)rem * NS * 6 * 64, gbase, N, K);
        if (HAS_RGB && res == 2 && w >= RGB_W0 && w < RGB_W0 + 4) rt_fill_rgb(Lv, rgb_res + (size_t)rem * NS * RT_RGB_WORDS * 64, gbase, N, K);
      }
      if (it == 0) __syncthreads();   // (it > 0: the update step's barrier below)
    }
    if (it > 0) {
      // head: the update step of iteration it - 1 (k_track_step's head), by every workgroup on its own state; the sums are in sums_s
      // (hop 2 of the previous iteration's exchange B), the search's totals in tot_s
      StepArgs H{true, false, HAS_ICP, HAS_RGB, false, A.icpWeight, Lv.k, lvl != ft_level_of(A.levels, it - 1), it};
      if (t < 64) {
        efs::SolvePrefetch PF{};
        const GNState& gp = gs[cur];
        PF.rt = gp.resultRt[lane & 15];
        PF.pose = bg[lane < 12 ? lane : 0];
        PF.slot_a = (HAS_RGB && lane == 0) ? tot_s[0] : 0;
        PF.slot_b = (HAS_RGB && lane == 0) ? tot_s[1] : 0;
        PF.lastRGBErrorLevel = gp.lastRGBErrorLevel;
        PF.broken = gp.rgb_broken;
        // (no statistics from inside the loop: lastA / lastb / the six tracker statistics are outputs of the call, and the LAST update step — at the
        // head of k_track_ref_end — writes them; every earlier value would be overwritten there)
        solve_step_wave<true>(st, &gs[cur], &gs[cur ^ 1], true, sums_s, H, S, PF, false);
      }
      __syncthreads();
      // the two tails of the update step — the float pose, K R K^-1 / K t — on two wavefronts side by side (round 6: behind resultRt they
      // share nothing; one after the other on the solving wavefront they were 0.58 + 0.70 us of every iteration)
      if (S.tail_pending) {   // (uniform: LDS)
        if (wave == 0) efs::gn_tail_pose(S, &gs[cur ^ 1], true);
        else if (wave == 1) efs::gn_tail_krk(H.knext, S, &gs[cur ^ 1], true);
        __syncthreads();
      }
      FT_CLK(6);   // SE(3) head: solve
#ifdef EF_STAGE_CLOCKS
      if (wg == 0 && t == 0) {   // phases of that solve (EF_STAMP 3..8, same thread)
        const unsigned long long* c = st->dbg_clock;
        FT_ADD(3, c[4] - c[3]); FT_ADD(5, c[5] - c[4]); FT_ADD(18, c[6] - c[5]); FT_ADD(19, c[7] - c[6]); FT_ADD(23, c[8] - c[7]);
      }
#endif
      cur ^= 1;
    }
    const GNState& G = gs[cur];
    const unsigned epoch_a = epoch;
    if (HAS_RGB && res == 2) {
      ++epoch;   // (exchange A's epoch: the photometric wavefronts search inside their accumulation below)
      FT_CLK(7);
    } else if (HAS_RGB) {
      // correspondence search (k_track_step's body) over exactly the visits of this column's two virtual warps, three in flight per thread
      int cnt = 0, sq = 0;
      const m33 Km = m33_load(G.krkinv);
      const f3 kt{G.kt[0], G.kt[1], G.kt[2]};
      const int npx = 64 * K;
      if (npx > FT_BLOCK) {
#pragma unroll 1
        for (int e0 = t; e0 < npx; e0 += 3 * FT_BLOCK) {
          int qs[3], nis[3], gi[3], u0s[3], v0s[3], lis[3];
          uint8_t m[3];
          float d1s[3], td1[3], d0s[3];
#pragma unroll
          for (int e = 0; e < 3; ++e) {
            const int idx = e0 + e * FT_BLOCK;
            const int q = rt_pixel(col, idx);
            const bool in = idx < npx && q < N;
            const int qq = in ? q : N - 1;
            qs[e] = q;
            m[e] = in ? Lv.mask[qq] : (uint8_t)0;
            d1s[e] = Lv.nextDepth[qq];
            nis[e] = Lv.nextImage[qq];
          }
#pragma unroll
          for (int e = 0; e < 3; ++e) {
            const int q = qs[e];
            const int y = q / cols, x = q - y * cols;
            const float d1 = d1s[e];
            td1[e] = (float)(d1 * (Km.r[2].x * x + Km.r[2].y * y + Km.r[2].z) + kt.z);
            u0s[e] = f2i_rn((d1 * (Km.r[0].x * x + Km.r[0].y * y + Km.r[0].z) + kt.x) / td1[e]);
            v0s[e] = f2i_rn((d1 * (Km.r[1].x * x + Km.r[1].y * y + Km.r[1].z) + kt.y) / td1[e]);
            gi[e] = (m[e] && u0s[e] >= 0 && v0s[e] >= 0 && u0s[e] < cols && v0s[e] < rows) ? v0s[e] * cols + u0s[e] : -1;
            d0s[e] = 0.f;
            lis[e] = 0;
            if (gi[e] >= 0) { d0s[e] = Lv.lastDepth[gi[e]]; lis[e] = Lv.lastImage[gi[e]]; }
          }
#pragma unroll
          for (int e = 0; e < 3; ++e) {
            if (!m[e]) continue;
            uint32_t packed = 0u;
            if (gi[e] >= 0 && d0s[e] > 0 && fabsf(td1[e] - d0s[e]) <= 0.07f /* maxDepthDeltaRGB, RGBDOdometry.cpp:41 */ && lis[e] != 0) {
              const int idiff = nis[e] - lis[e];
              packed = pack_corres(u0s[e], v0s[e], idiff);
              cnt += 1;
              sq += idiff * idiff;
            }
            Lv.corres[qs[e]] = packed;
          }
        }
      } else {
        const int q = rt_pixel(col, t);
        const bool in = t < npx && q < N;
        const int qq = in ? q : N - 1;
        const uint8_t mk = Lv.mask[qq];          // the three pixel-addressed loads together: one round trip, not two
        const float d1 = Lv.nextDepth[qq];
        const int ni = Lv.nextImage[qq];
        if (in && mk) {
          const int y = q / cols, x = q - y * cols;
          const float td = (float)(d1 * (Km.r[2].x * x + Km.r[2].y * y + Km.r[2].z) + kt.z);
          const int u0 = f2i_rn((d1 * (Km.r[0].x * x + Km.r[0].y * y + Km.r[0].z) + kt.x) / td);
          const int v0 = f2i_rn((d1 * (Km.r[1].x * x + Km.r[1].y * y + Km.r[1].z) + kt.y) / td);
          uint32_t packed = 0u;
          if (u0 >= 0 && v0 >= 0 && u0 < cols && v0 < rows) {
            const int gi1 = v0 * cols + u0;
            const float d0 = Lv.lastDepth[gi1];
            const int li = Lv.lastImage[gi1];
            if (d0 > 0 && fabsf(td - d0) <= 0.07f /* maxDepthDeltaRGB, RGBDOdometry.cpp:41 */ && li != 0) {
              const int idiff = ni - li;
              packed = pack_corres(u0, v0, idiff);
              cnt += 1;
              sq += idiff * idiff;
            }
          }
          Lv.corres[q] = packed;
        }
      }
      cnt = wave_sum_lane0(cnt);
      sq = wave_sum_lane0(sq);
      if (lane == 0) { ired[wave * 2] = cnt; ired[wave * 2 + 1] = sq; }
      __syncthreads();   // also: the workgroup's packed correspondences are visible to its photometric wavefronts
      if (t == 0) {
        int sa = 0, sb = 0;
        for (int w = 0; w < FT_BLOCK / 64; ++w) { sa += ired[w * 2]; sb += ired[w * 2 + 1]; }
#pragma unroll
        for (int c = 0; c < FT_REPL_A; ++c) {
          ft_put(GA + (size_t)c * FT_REPL_STRIDE + 2 * col, (unsigned)sa, epoch_a);
          ft_put(GA + (size_t)c * FT_REPL_STRIDE + 2 * col + 1, (unsigned)sb, epoch_a);
        }
      }
      ++epoch;
      FT_CLK(7);   // SE(3): correspondence search + publish A
    }
    const unsigned epoch_b = epoch++;
    // normal equations of the column
    IcpPose P{};
    if (HAS_ICP) {
      P.Rcurr = m33_load(G.Rcurr);
      P.tcurr = {G.tcurr[0], G.tcurr[1], G.tcurr[2]};
      P.Rprev_inv = m33_load(bg + 12);
      P.tprev = {bg[9], bg[10], bg[11]};
      if (res) {   // wave-uniform values (LDS): as scalars they cost the resident path's gathers-in-flight no vector registers
        auto u1 = [](float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); };
        auto u3 = [&](f3 a) { return f3{u1(a.x), u1(a.y), u1(a.z)}; };
        P.Rcurr = m33{{u3(P.Rcurr.r[0]), u3(P.Rcurr.r[1]), u3(P.Rcurr.r[2])}};
        P.tcurr = u3(P.tcurr);
        P.Rprev_inv = m33{{u3(P.Rprev_inv.r[0]), u3(P.Rprev_inv.r[1]), u3(P.Rprev_inv.r[2])}};
        P.tprev = u3(P.tprev);
      }
    }
    // exchange A, called by every photometric wavefront with its first loads and gathers in flight: the first one (warp m, lower half)
    // sweeps the records, the others watch its relay in LDS
    auto wait_sigma = [&]() -> float {
      const bool leader = (wave & 3) == 0;
      if (leader) {
        int sa, sb;
        const bool ok = ft_sweep_records(GA_mine, epoch_a, &dead_s, Y, sa, sb);
        sa = wave_sum_lane0(sa);
        sb = wave_sum_lane0(sb);
        if (lane == 0) {
          tot_s[0] = sa;
          tot_s[1] = sb;
          __hip_atomic_store(&seen_a[1], ok ? 0u : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_store(&seen_a[0], epoch_a, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      } else if (lane == 0) {
        int spins = 0;
        while (__hip_atomic_load(&seen_a[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != epoch_a && ++spins < 64 * FT_SPIN) __builtin_amdgcn_s_sleep(1);
      }
      efs::wave_sync();
      const int rgbSize = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&tot_s[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      const int sqsum = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&tot_s[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      return sigma_from_sums(sqsum, rgbSize, false);
    };
    float r[12];
    if (res == 2) {
      // both sides resident: the ICP wavefronts start at once; every photometric wavefront searches its own visits, the four hand their
      // {count, sum diff^2} to the first one through LDS, which publishes the column's record, sweeps exchange A and relays sigma
      const int rem = wave & 3;
      const int gbase = rt_vwarp(col, rem >> 1) * 32 + (rem & 1) * 16;
      f32x4 c[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) c[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (HAS_ICP && wave < 4) {
        rt_icp_resident(IV, RV, P, icp_res + (size_t)rem * NS * 6 * 64, gbase, N, K, c);
        FT_CLK(8);   // SE(3), resident: the first ICP wavefront's rows
      }
      if (HAS_RGB && wave >= RGB_W0 && wave < RGB_W0 + 4) {
#ifdef EF_STAGE_CLOCKS
        clk_last2 = wall_clock64();
#endif
        uint32_t* slots = rgb_res + (size_t)rem * NS * RT_RGB_WORDS * 64;
        int cnt, sq;
        // (the column's record of exchange A is what every workgroup of the chip waits for: the search wins the SIMD's issue slots over the ICP
        // wavefront it shares them with)
        __builtin_amdgcn_s_setprio(3);
        rt_rgb_search(Lv, m33_load(G.krkinv), f3{G.kt[0], G.kt[1], G.kt[2]}, slots, K, cnt, sq);
        cnt = wave_sum_lane0(cnt);
        sq = wave_sum_lane0(sq);
        if (lane == 0) {
          wsum[rem][0] = cnt;
          wsum[rem][1] = sq;
          __hip_atomic_store(&wtag[rem], epoch_a, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        FT_CLK2(24);   // resident: search
        if (rem == 0 && lane == 0) {
          int sa = 0, sb = 0;
          for (int i = 0; i < 4; ++i) {
            int spins = 0;
            while (__hip_atomic_load(&wtag[i], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != epoch_a && ++spins < 64 * FT_SPIN) __builtin_amdgcn_s_sleep(1);
            sa += wsum[i][0];
            sb += wsum[i][1];
          }
#pragma unroll
          for (int c = 0; c < FT_REPL_A; ++c) {
            ft_put(GA + (size_t)c * FT_REPL_STRIDE + 2 * col, (unsigned)sa, epoch_a);
            ft_put(GA + (size_t)c * FT_REPL_STRIDE + 2 * col + 1, (unsigned)sb, epoch_a);
          }
        }
        __builtin_amdgcn_s_setprio(0);
#ifdef EF_RT_RGB_PREPARE
        rt_rgb_prepare(RV, slots, K);   // (behind the column's record: what the rows need that does not wait for sigma)
#endif
        const float sigma = wait_sigma();
        FT_CLK2(25);   // resident: publish A, sweep, sigma
        rt_rgb_resident(IV, RV, P, sigma, slots, K, c);
        FT_CLK2(26);   // resident: photometric rows
      }
      rt_column_trees<NT>(c, xch, pairx, r);
    } else {
      rt_accumulate<HAS_ICP, HAS_RGB>(IV, RV, P, col, N, K, xch, pairx, r, wait_sigma, (HAS_ICP && res == 1) ? icp_res : nullptr);
    }
    if ((wave & 3) == 0 && wave < 4 * NT && lane < 4) {   // lanes 0..3 of wavefront (term, warp m, lower half): the column's pair sums
      const int tix = wave >> 2;
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int a = quad_member(q, i, lane);
          if (a >= 0) ft_put(G1 + (size_t)(tix * SE3_ACCS + a) * 256 + ft_slot(col), __float_as_uint(r[q * 4 + i]), epoch_b);
        }
    }
    FT_CLK(9);   // SE(3): tasks, trees, publish B
    // exchange B: reducers finish the tree of their accumulator; everybody (the launch's last iteration: nobody — k_track_end reads the
    // plain totals the reducers leave) takes the 58 totals
    if (wave == 1 && wg < NA) rt_reduce_publish(G1, G2, wg, epoch_b, &dead_s, Y, last ? A.partials + FT_P_OFF : nullptr);
    if (!last && wave == 0) {
      float v;
      ft_poll_totals(G2_mine, NA, epoch_b, &dead_s, Y, v);
      if (lane < NA) sums_s[(HAS_ICP ? 0 : SE3_ACCS) + lane] = v;
    }
    __syncthreads();
    FT_CLK(10);   // SE(3): exchange B
    FT_COUNT(21);
#ifdef EF_STAGE_CLOCKS
    if (wg == 0 && t == 0) { FT_ADD(12 + lvl, wall_clock64() - clk_iter); FT_ADD(15 + lvl, 1ull); }
#endif
  }
  // ---- what the launch that follows reads (k_track_end: the update of iteration n_iter - 1 at its head) ----
  if (wg == 0 && t == 0) {
    const GNState& g = gs[cur];
    GNState& o = st->gn[A.out_cur];
    for (int i = 0; i < 9; ++i) { o.Rcurr[i] = g.Rcurr[i]; o.krkinv[i] = g.krkinv[i]; }
    for (int i = 0; i < 3; ++i) { o.tcurr[i] = g.tcurr[i]; o.kt[i] = g.kt[i]; }
    for (int i = 0; i < 16; ++i) o.resultRt[i] = g.resultRt[i];
    o.lastRGBErrorLevel = g.lastRGBErrorLevel;
    o.rgb_broken = g.rgb_broken;
    if (HAS_RGB && A.n_iter > 0) {   // the last search's totals, where the next update step's head looks for them
      const int set = (A.n_iter - 1) & 1;
      st->rgb_slots[set][0][0] = tot_s[0];
      st->rgb_slots[set][0][1] = tot_s[1];
    }
#ifdef EF_STAGE_CLOCKS
    FT_ADD(11, wall_clock64() - clk_start);   // whole launch
    FT_ADD(22, 1ull);
#endif
  }
}

// ------------------------------------------------------------------------------------------
// The call on ONE workgroup: what runs when the persistent launch in front of it left the verdict SERIAL (its grid could not become
// resident: see the admission step).  The same columns, the same pair sums, the same trees — column by column instead of all at once, the
// pair sums in the plain array P[acc][column] (k_se3_accum's layout), the rest of the tree by rt_tree_plain, the update steps by the same
// solve — so the results are the persistent launch's, bit for bit.
// ------------------------------------------------------------------------------------------
struct RtSerialLds {
  GNState gs[2];
  efs::SolveScratch S;
  float sums_s[2 * SE3_ACCS];
  float bg[24];
  float xch[2 * 2 * 12 * 64];
  float pairx[2 * 12 * 4];
  float lds_rows[RT_KC * 5 * 64];
  float red[SO3_ACCS];
  So3Loop Z;
  int ired[2 * FT_BLOCK / 64];
  int tot_s[2];
  double qt[7];   // the tail's pose (quaternion xyzw + translation) on its way to the wavefronts that publish it
};
template <bool HAS_ICP, bool HAS_RGB>
__device__ __forceinline__ void rt_serial_call(const FtArgs& A, TrackState* st, RtSerialLds& M) {
  constexpr int NT = (HAS_ICP && HAS_RGB) ? 2 : 1;
  constexpr int NA = NT * SE3_ACCS;
  GNState (&gs)[2] = M.gs;
  efs::SolveScratch& S = M.S;
  float* sums_s = M.sums_s;
  float* bg = M.bg;
  float* xch = M.xch;
  float* pairx = M.pairx;
  float* lds_rows = M.lds_rows;
  float* red = M.red;
  So3Loop& Z = M.Z;
  int* ired = M.ired;
  int* tot_s = M.tot_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float* P = A.partials + FT_P_OFF;
  // ---- k_track_begin ----
  if (t == 0) {
    double R[9];
    efl::quat_to_mat<double>(st->q, R);
    GNState& g = gs[0];
    for (int i = 0; i < 9; ++i) bg[i] = g.Rcurr[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) bg[9 + i] = g.tcurr[i] = (float)st->t[i];
    efl::m3_inverse<float>(bg, bg + 12);
    efl::m4_identity(g.resultRt);
    g.rgb_broken = 0;
    g.lastRGBErrorLevel = 3.402823466e+38f;
    if (!A.so3) compute_krk(g.resultRt, A.kfirst, g.krkinv, g.kt);
    for (int i = 0; i < 9; ++i) { st->Rprev[i] = bg[i]; st->Rprev_inv[i] = bg[12 + i]; }
    for (int i = 0; i < 3; ++i) st->tprev[i] = bg[9 + i];
    for (int i = 0; i < 4; ++i) st->q_prev[i] = st->q[i];
    for (int i = 0; i < 3; ++i) st->t_prev[i] = st->t[i];
    for (int i = 0; i < RGB_SLOTS; ++i) st->rgb_slots[0][i][0] = st->rgb_slots[0][i][1] = st->rgb_slots[1][i][0] = st->rgb_slots[1][i][1] = 0;
    st->call_seq += 1u;
    st->so3_iterations = 0;
    st->so3_ticket = 0;
    st->so3_done = 1;
    st->dense_count = 0;
    tot_s[0] = tot_s[1] = 0;
  }
  __syncthreads();
  // ---- SO(3) ----
  if (A.so3) {
    if (t == 0) {
      efl::m3_identity(Z.resR);
      efl::m3_identity(Z.lastResR);
      for (int i = 0; i < 9; ++i) Z.R_lr[i] = (i % 4 == 0) ? 1.f : 0.f;
      Z.lastError = 3.402823466e+38f / 2;
      Z.lastCount = 3.402823466e+38f / 2;
      Z.done = 0;
      so3_matrices(Z.resR, A.kso3, Z.mats);
    }
    __syncthreads();
    for (int it = 0; it < 10; ++it) {
      const m33 IB = m33_load(Z.mats), KI = m33_load(Z.mats + 9), KR = m33_load(Z.mats + 18);
#pragma unroll 1
      for (int col = 0; col < FT_WGS; ++col) {
        float z[SO3_ACCS];
        rt_so3_accumulate(A.so3_last, A.so3_next, A.so3_cols, A.so3_rows, IB, KI, KR, col, lds_rows, z);
        if (t == 0) {
#pragma unroll
          for (int i = 0; i < SO3_ACCS; ++i) P[(size_t)i * 256 + col] = z[i];
        }
      }
      __threadfence_block();
      __syncthreads();
      rt_tree_plain<FT_BLOCK>(P, SO3_ACCS, red);
      __syncthreads();
      if (t == 0) Z.done = so3_update(Z, red, it, A.kso3, A.kfirst, gs[0]) ? 1 : 0;
      __syncthreads();
      if (Z.done) break;
    }
    if (t == 0) {
      st->lastSO3Error = Z.err;
      st->lastSO3Count = Z.cnt;
      st->so3_iterations = Z.iterations;
    }
  }
  // ---- the Gauss-Newton iterations ----
  int cur = 0;
  for (int it = 0; it < A.n_iter; ++it) {
    const int lvl = ft_level_of(A.levels, it);
    const PtLevel Lv = A.L[lvl];
    const int cols = Lv.cols, rows = Lv.rows, N = cols * rows;
    const int K = (N + VTHREADS - 1) / VTHREADS;
    if (it > 0) {
      StepArgs H{true, false, HAS_ICP, HAS_RGB, false, A.icpWeight, Lv.k, lvl != ft_level_of(A.levels, it - 1), it};
      if (t < 64) {
        efs::SolvePrefetch PF{};
        const GNState& gp = gs[cur];
        PF.rt = gp.resultRt[lane & 15];
        PF.pose = bg[lane < 12 ? lane : 0];
        PF.slot_a = (HAS_RGB && lane == 0) ? tot_s[0] : 0;
        PF.slot_b = (HAS_RGB && lane == 0) ? tot_s[1] : 0;
        PF.lastRGBErrorLevel = gp.lastRGBErrorLevel;
        PF.broken = gp.rgb_broken;
        solve_step_wave(st, &gs[cur], &gs[cur ^ 1], true, sums_s, H, S, PF, true);
      }
      __syncthreads();
      cur ^= 1;
    }
    const GNState& G = gs[cur];
    float sigma = 0.f;
    if (HAS_RGB) {
      const m33 Km = m33_load(G.krkinv);
      const f3 kt{G.kt[0], G.kt[1], G.kt[2]};
      int cnt = 0, sq = 0;
#pragma unroll 1
      for (int q = t; q < N; q += FT_BLOCK) {
        if (!Lv.mask[q]) continue;
        const float d1 = Lv.nextDepth[q];
        const int ni = Lv.nextImage[q];
        const int y = q / cols, x = q - y * cols;
        const float td = (float)(d1 * (Km.r[2].x * x + Km.r[2].y * y + Km.r[2].z) + kt.z);
        const int u0 = f2i_rn((d1 * (Km.r[0].x * x + Km.r[0].y * y + Km.r[0].z) + kt.x) / td);
        const int v0 = f2i_rn((d1 * (Km.r[1].x * x + Km.r[1].y * y + Km.r[1].z) + kt.y) / td);
        uint32_t packed = 0u;
        if (u0 >= 0 && v0 >= 0 && u0 < cols && v0 < rows) {
          const int gi1 = v0 * cols + u0;
          const float d0 = Lv.lastDepth[gi1];
          const int li = Lv.lastImage[gi1];
          if (d0 > 0 && fabsf(td - d0) <= 0.07f /* maxDepthDeltaRGB, RGBDOdometry.cpp:41 */ && li != 0) {
            const int idiff = ni - li;
            packed = pack_corres(u0, v0, idiff);
            cnt += 1;
            sq += idiff * idiff;
          }
        }
        Lv.corres[q] = packed;
      }
      cnt = wave_sum_lane0(cnt);
      sq = wave_sum_lane0(sq);
      if (lane == 0) { ired[wave * 2] = cnt; ired[wave * 2 + 1] = sq; }
      __threadfence_block();
      __syncthreads();
      if (t == 0) {
        int sa = 0, sb = 0;
        for (int w = 0; w < FT_BLOCK / 64; ++w) { sa += ired[w * 2]; sb += ired[w * 2 + 1]; }
        tot_s[0] = sa;
        tot_s[1] = sb;
      }
      __syncthreads();
      sigma = sigma_from_sums(tot_s[1], tot_s[0], false);
    }
    const IcpView IV{Lv.vmap_curr, Lv.nmap_curr, Lv.vmap_g_prev, Lv.nmap_g_prev, cols, rows, Lv.k, A.distThres, A.angleThres, A.dist2Max, A.sine2Max};
    const RgbView RV{Lv.corres, Lv.lastDepth, nullptr, Lv.dIdx, Lv.dIdy, cols, rows, Lv.k, 1.0f / 8.0f};
    IcpPose P3{};
    if (HAS_ICP) {
      P3.Rcurr = m33_load(G.Rcurr);
      P3.tcurr = {G.tcurr[0], G.tcurr[1], G.tcurr[2]};
      P3.Rprev_inv = m33_load(bg + 12);
      P3.tprev = {bg[9], bg[10], bg[11]};
    }
#pragma unroll 1
    for (int col = 0; col < FT_WGS; ++col) {
      float r[12];
      rt_accumulate<HAS_ICP, HAS_RGB, false>(IV, RV, P3, col, N, K, xch, pairx, r, RtNoWait{sigma});
      if ((wave & 3) == 0 && wave < 4 * NT && lane < 4) {
        const int tix = wave >> 2;
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int a = quad_member(q, i, lane);
            if (a >= 0) P[(size_t)(tix * SE3_ACCS + a) * 256 + col] = r[q * 4 + i];
          }
      }
      __syncthreads();   // (xch / pairx are reused by the next column)
    }
    __threadfence_block();
    __syncthreads();
    rt_tree_plain<FT_BLOCK>(P, NA, sums_s + (HAS_ICP ? 0 : SE3_ACCS));
    __syncthreads();
    if (it == A.n_iter - 1 && t < NA) P[(size_t)t * 256] = sums_s[(HAS_ICP ? 0 : SE3_ACCS) + t];   // what the head of k_track_end reads (ng = 1)
    __syncthreads();
  }
  // ---- what the head of k_track_end reads ----
  if (t == 0) {
    const GNState& g = gs[cur];
    GNState& o = st->gn[A.out_cur];
    for (int i = 0; i < 9; ++i) { o.Rcurr[i] = g.Rcurr[i]; o.krkinv[i] = g.krkinv[i]; }
    for (int i = 0; i < 3; ++i) { o.tcurr[i] = g.tcurr[i]; o.kt[i] = g.kt[i]; }
    for (int i = 0; i < 16; ++i) o.resultRt[i] = g.resultRt[i];
    o.lastRGBErrorLevel = g.lastRGBErrorLevel;
    o.rgb_broken = g.rgb_broken;
    if (HAS_RGB && A.n_iter > 0) {
      const int set = (A.n_iter - 1) & 1;
      st->rgb_slots[set][0][0] = tot_s[0];
      st->rgb_slots[set][0][1] = tot_s[1];
    }
  }
}

// The launch behind every persistent launch of the reference-order build (round 5: ONE launch where rounds 3-4 had k_track_serial + k_track_end):
//   1. when the verdict of the launch in front of it was SERIAL, the whole call on this one workgroup (rt_serial_call);
//   2. k_track_end: the update step of the LAST iteration (totals in column 0 of P: ng = 1), then the tail of getIncrementalTransformation —
//      0.3 m guard and SVD re-orthonormalisation on one lane (RGBDOdometry.cpp:555-570), then, on FOUR wavefronts side by side instead of one
//      lane after the other, the float matrices of the map passes, the velocity weighting (ElasticFusion.cpp:369-383) and the trajectory log:
//      the same scalar code per piece, the same bits;
//   3. the instance's sticky abort flag handed to the host (see k_track_end).
template <bool HAS_ICP, bool HAS_RGB>
__global__ void __launch_bounds__(FT_BLOCK) k_track_ref_end(float* partials, TrackState* st, unsigned persistent_epoch, const StepArgs A, int slots_set,
                                                             bool rgb, float weightMultiplier, double* traj, int slot, unsigned* abort_report) {
  __shared__ RtSerialLds M;
  FtSync* Y = (FtSync*)(partials + FT_SY_OFF);
  const int t = threadIdx.x, wave = t >> 6;
  const unsigned long long verdict = ft_get(&Y->mode);
  const GNState* prev = &st->gn[0];   // (the persistent launch and the serial call both leave their state in buffer FtArgs::out_cur = 0)
  GNState* next = &st->gn[1];
  // what the head reads from memory — the update step's prefetch and the 58 totals (column 0 of P: ng = 1) — is asked for BEHIND the verdict's
  // load, not behind its answer (round 6: one memory round trip less on a launch every frame waits for); a SERIAL verdict (the call runs
  // here first and rewrites all of it) asks again
  const int na = (A.icp ? SE3_ACCS : 0) + (A.rgb ? SE3_ACCS : 0);
  efs::SolvePrefetch PF{};
  float total = 0.f;
  if (A.has_head) {
    if (t < 64) PF = efs::solve_prefetch(st, prev, &st->rgb_slots[slots_set & 1][0][0]);
    if (t < na) total = partials[FT_P_OFF + (size_t)t * 256];
  }
  if ((unsigned)(verdict >> 32) == persistent_epoch && (unsigned)verdict == FT_MODE_SERIAL) {   // uniform
    rt_serial_call<HAS_ICP, HAS_RGB>(Y->args, st, M);
    __threadfence_block();
    __syncthreads();
    if (A.has_head) {
      if (t < 64) PF = efs::solve_prefetch(st, prev, &st->rgb_slots[slots_set & 1][0][0]);
      if (t < na) total = partials[FT_P_OFF + (size_t)t * 256];
    }
  }
  if (A.has_head) {
    if (t < na) M.sums_s[(A.icp ? 0 : SE3_ACCS) + t] = total;   // (head_sums with ng = 1)
    __syncthreads();
    // the update step's two tails on two wavefronts, as inside the persistent loop; the float pose is all the tail below waits for, so
    // wavefront 0 goes on while wavefront 1 evaluates K R K^-1 / K t (the next barrier is the one in front of the four pieces below)
    if (t < 64) solve_step_wave<true>(st, prev, next, true, M.sums_s, A, M.S, PF, true);
    __syncthreads();
    if (M.S.tail_pending) {   // (uniform: LDS)
      if (wave == 0) { efs::gn_tail_pose(M.S, next, true); efs::wave_sync(); }
      else if (wave == 1) efs::gn_tail_krk(A.knext, M.S, next, true);
    }
  } else if (t == 0) {
    for (int i = 0; i < 9; ++i) M.S.Rcurr[i] = prev->Rcurr[i];
    for (int i = 0; i < 3; ++i) M.S.tcurr[i] = prev->tcurr[i];
  }
  if (t == 0) {   // 0.3 m guard, SVD re-orthonormalisation (track_end_tail's first half)
    float Rcurr[9], tcurr[3];
    for (int i = 0; i < 9; ++i) Rcurr[i] = M.S.Rcurr[i];
    for (int i = 0; i < 3; ++i) tcurr[i] = M.S.tcurr[i];
    if (rgb) {
      const float d0 = tcurr[0] - st->tprev[0], d1 = tcurr[1] - st->tprev[1], d2 = tcurr[2] - st->tprev[2];
      if ((double)sqrtf(d0 * d0 + d1 * d1 + d2 * d2) > 0.3) {
        for (int i = 0; i < 9; ++i) Rcurr[i] = st->Rprev[i];
        for (int i = 0; i < 3; ++i) tcurr[i] = st->tprev[i];
      }
    }
    double Rc[9], Rp[9];
    for (int i = 0; i < 9; ++i) Rc[i] = (double)Rcurr[i];
    efl::polar3(Rc, Rp);
    efl::SE3 T;
    efl::se3_set_rotation(T, Rp);
    for (int i = 0; i < 4; ++i) { st->q[i] = T.q[i]; M.qt[i] = T.q[i]; }
    for (int i = 0; i < 3; ++i) { st->t[i] = (double)tcurr[i]; M.qt[4 + i] = (double)tcurr[i]; }
  }
  __syncthreads();
  if ((t & 63) == 0) {   // lane 0 of wavefronts 0..3: one piece each (publish_pose / compute_weighting / log_pose, split)
    efl::SE3 T;
    for (int i = 0; i < 4; ++i) T.q[i] = M.qt[i];
    for (int i = 0; i < 3; ++i) T.t[i] = M.qt[4 + i];
    if (wave == 0) {
      efl::se3_inverse_matrix_f(T, st->T_cw);
    } else if (wave == 1) {
      efl::se3_castf_matrix(T, st->pose_f);
      double R[9];
      efl::quat_to_mat<double>(T.q, R);
      for (int i = 0; i < 9; ++i) st->R_wc_f[i] = (float)R[i];
      for (int i = 0; i < 3; ++i) st->t_wc_f[i] = (float)T.t[i];
    } else if (wave == 2) {
      efl::SE3 Tp;
      for (int i = 0; i < 4; ++i) Tp.q[i] = st->q_prev[i];
      for (int i = 0; i < 3; ++i) Tp.t[i] = st->t_prev[i];
      const efl::SE3 Tcp = efl::se3_mul(efl::se3_inverse(T), Tp);
      const double tn = sqrt(Tcp.t[0] * Tcp.t[0] + Tcp.t[1] * Tcp.t[1] + Tcp.t[2] * Tcp.t[2]);
      const double ln = efl::se3_log_norm(Tcp);
      float weighting = (float)(tn > ln ? tn : ln);
      const float largest = 0.01f, minWeight = 0.5f;
      if (weighting > largest) weighting = largest;
      const float w = 1.0f - (weighting / largest);
      st->weighting = (w > minWeight ? w : minWeight) * weightMultiplier;
    } else if (wave == 3) {
      if (traj) efl::se3_matrix(T, traj + (size_t)slot * 16);
      if (abort_report) {
        const unsigned v = __hip_atomic_load(&Y->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) __hip_atomic_store(abort_report, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

// Host side of the level-resident slots: how many bytes of dynamic LDS a k_track_ref launch may ask for on the current device (0: none — every
// level streams).  gfx950 gives one workgroup up to 160 KB; the kernel's static LDS and a margin stay free.  Asked once per device.
static unsigned rt_res_budget() {
  static std::mutex mu;
  static bool done[64] = {};
  static unsigned budget[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0u;
  std::lock_guard<std::mutex> lk(mu);
  if (!done[dev]) {
    done[dev] = true;
    int per_block = 0;
    hipFuncAttributes fa{};
    if (hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess &&
        hipFuncGetAttributes(&fa, (const void*)k_track_ref<true, true>) == hipSuccess) {
      const long total = per_block > 160 * 1024 ? 160 * 1024 : per_block;
      long want = total - (long)fa.sharedSizeBytes - 1024;
      want = want > 128 * 1024 ? 128 * 1024 : (want / 1024) * 1024;
      if (want > 0 &&
          hipFuncSetAttribute((const void*)k_track_ref<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) == hipSuccess &&
          hipFuncSetAttribute((const void*)k_track_ref<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) == hipSuccess &&
          hipFuncSetAttribute((const void*)k_track_ref<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) == hipSuccess)
        budget[dev] = (unsigned)want;
    }
    (void)hipGetLastError();
  }
  return budget[dev];
}
