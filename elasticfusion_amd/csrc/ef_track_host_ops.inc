// Host code of the tracker, part 1 of 3 (included by ef_track_kernels.hip inside namespace eft, behind all device code): the operator-tier
// launchers (raw device pointers, one reference operator each), the normal-equation accumulation launch both tiers share and the helpers
// every launcher uses.
// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
namespace {
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
}  // namespace

void pyr_down_u16(const uint16_t* src, int scols, int srows, uint16_t* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_pyr_down_u16, tile_grid(scols / 2, srows / 2), tile_block(), 0, s, src, scols, srows, dst);
}
void create_vmap(const uint16_t* depth, int cols, int rows, Intr k, float cutoff, float* vmap, hipStream_t s) {
  hipLaunchKernelGGL(k_create_vmap, tile_grid(cols, rows), tile_block(), 0, s, depth, cols, rows, 1.f / k.fx, 1.f / k.fy, k.cx, k.cy, cutoff, vmap);
}
void create_nmap(const float* vmap, int cols, int rows, float* nmap, hipStream_t s) {
  hipLaunchKernelGGL(k_create_nmap, tile_grid(cols, rows), tile_block(), 0, s, vmap, cols, rows, nmap);
}
void transform_maps(const float* vsrc, const float* nsrc, int cols, int rows, const float* R9_dev, const float* t3_dev, float* vdst,
                    float* ndst, hipStream_t s) {
  hipLaunchKernelGGL(k_transform_maps, tile_grid(cols, rows), tile_block(), 0, s, vsrc, nsrc, cols, rows, R9_dev, t3_dev, vdst, ndst);
}
void copy_maps(const float* vtex, const float* ntex, int cols, int rows, float* vmaps_tmp, float* vmap, float* nmap, hipStream_t s) {
  hipLaunchKernelGGL(k_copy_maps, tile_grid(cols, rows), tile_block(), 0, s, (const float4*)vtex, (const float4*)ntex, cols, rows,
                     (float4*)vmaps_tmp, vmap, nmap);
}
void resize_map(const float* in, int scols, int srows, float* out, bool normalize, hipStream_t s) {
  if (normalize) hipLaunchKernelGGL(k_resize_map<true>, tile_grid(scols / 2, srows / 2), tile_block(), 0, s, in, scols, srows, out);
  else hipLaunchKernelGGL(k_resize_map<false>, tile_grid(scols / 2, srows / 2), tile_block(), 0, s, in, scols, srows, out);
}
void pyr_down_gauss_f(const float* src, int scols, int srows, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_pyr_down_gauss_f, tile_grid(scols / 2, srows / 2), tile_block(), 0, s, src, scols, srows, dst);
}
void pyr_down_uchar_gauss(const uint8_t* src, int scols, int srows, uint8_t* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_pyr_down_uchar_gauss, tile_grid(scols / 2, srows / 2), tile_block(), 0, s, src, scols, srows, dst);
}
void vertices_to_depth(const float* vmaps_tmp, int cols, int rows, float cutoff, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_vertices_to_depth, tile_grid(cols, rows), tile_block(), 0, s, (const float4*)vmaps_tmp, cols, rows, cutoff, dst);
}
void bgr_to_intensity(const uint8_t* src, int channels, int cols, int rows, uint8_t* dst, hipStream_t s) {
  const int n = cols * rows;
  if (channels == 4) hipLaunchKernelGGL(k_bgr_to_intensity<4>, dim3(ceil_div(n, 256)), dim3(256), 0, s, src, n, dst);
  else hipLaunchKernelGGL(k_bgr_to_intensity<3>, dim3(ceil_div(n, 256)), dim3(256), 0, s, src, n, dst);
}
void derivative_images(const uint8_t* src, int cols, int rows, int16_t* dx, int16_t* dy, hipStream_t s) {
  hipLaunchKernelGGL(k_sobel, tile_grid(cols, rows), tile_block(), 0, s, src, cols, rows, dx, dy);
}
void project_to_point_cloud(const float* depth, int cols, int rows, Intr k, float* cloud, hipStream_t s) {
  hipLaunchKernelGGL(k_project_points, tile_grid(cols, rows), tile_block(), 0, s, depth, cols, rows, 1.0f / k.fx, 1.0f / k.fy, k.cx, k.cy, cloud);
}

namespace {
// The term sets a call can have (RGBDOdometry.cpp:266-267: ICP and RGB, ICP alone, RGB alone — never neither): f(HAS_ICP, HAS_RGB) with the
// two as std::bool_constant's, for the kernels that carry them as template arguments
template <class F>
void with_terms(bool icp, bool rgb, F&& f) {
  if (icp && rgb) f(std::true_type{}, std::true_type{});
  else if (icp) f(std::true_type{}, std::false_type{});
  else f(std::false_type{}, std::true_type{});
}
// one normal-equation accumulation launch (either tier); start / stop: optional events that receive the kernel's own begin / end
// timestamps (hipExtLaunchKernelGGL: what rocprofv3 --kernel-trace reports as the dispatch's duration)
template <bool HAS_ICP, bool HAS_RGB, bool PACKED>
void launch_accum(const IcpView& IV, const RgbView& RV, const Se3Inputs& in, int N, const Se3Out& out, hipStream_t s, hipEvent_t start = nullptr,
                  hipEvent_t stop = nullptr) {
#ifdef EF_FAST_ORDER
  {   // one workgroup per group of four tasks, four wavefronts per term (ef_track_fast.inc)
    const FastPlan fp = fast_plan(N);
    const dim3 fgrid(in.xcd_swizzle ? 8 * fast_groups_per_xcd(fp.NG) : fp.NG), fblock(256 * ((HAS_ICP && HAS_RGB) ? 2 : 1));
    hipExtLaunchKernelGGL((k_se3_accum_fast<HAS_ICP, HAS_RGB, PACKED>), fgrid, fblock, 0, s, start, stop, 0, IV, RV, in, out.pairs);
  }
#else
  constexpr int BLOCK = 64 * 2 * ACC_NW * ((HAS_ICP && HAS_RGB) ? 2 : 1);
  const dim3 grid(VWARPS / ACC_NW), block(BLOCK);
  // CH = steps (of four passes) a wavefront has in flight per round: 640x480 has 19 passes = 5 steps = ONE round of CH = 5; 1280x960 has
  // 75 passes = 19 steps = four dependent rounds.  CH = 10 there (two rounds, 231 registers: the launch runs two wavefronts per SIMD
  // anyway) was measured SLOWER: 28.4 vs 25.1 us (profiles/r03f_ab_fused_step_and_ch10.log) — twice the loads per round queue behind each
  // other in the CU's one address pipe for longer than the two saved round trips.
#ifdef EF_VISIT_PAIRS
  // (round 6: two visits per lane — a round is CH / 2 packed evaluations; 640x480: 5 steps = one round of CH = 6, the sixth step empty;
  // 1280x960: 19 steps = five rounds of CH = 4)
  if (HAS_ICP || PACKED) {
    const int S = ((N + VTHREADS - 1) / VTHREADS + 3) >> 2;
    if (S <= 2) hipExtLaunchKernelGGL((k_se3_accum<2, HAS_ICP, HAS_RGB, PACKED>), grid, block, 0, s, start, stop, 0, IV, RV, in, out);
    else if (S % 6 == 0 || S % 6 == 5 || !(S % 4 == 0 || S % 4 == 3)) hipExtLaunchKernelGGL((k_se3_accum<6, HAS_ICP, HAS_RGB, PACKED>), grid, block, 0, s, start, stop, 0, IV, RV, in, out);
    else hipExtLaunchKernelGGL((k_se3_accum<4, HAS_ICP, HAS_RGB, PACKED>), grid, block, 0, s, start, stop, 0, IV, RV, in, out);
    return;
  }
#endif
  if (N > 8 * VTHREADS) hipExtLaunchKernelGGL((k_se3_accum<5, HAS_ICP, HAS_RGB, PACKED>), grid, block, 0, s, start, stop, 0, IV, RV, in, out);
  else hipExtLaunchKernelGGL((k_se3_accum<2, HAS_ICP, HAS_RGB, PACKED>), grid, block, 0, s, start, stop, 0, IV, RV, in, out);
#endif
}
// fast order: groups of a level / workgroups of a so3Step launch (one per group, XCD-contiguous); the reference order ignores the former
inline int op_groups(int N) {
#ifdef EF_FAST_ORDER
  return fast_plan(N).NG;
#else
  (void)N;
  return 0;
#endif
}
inline int so3_grid(int N) {
#ifdef EF_FAST_ORDER
  return 8 * fast_groups_per_xcd(fast_plan(N).NG);
#else
  (void)N;
  return VWARPS / SO3_WPB;
#endif
}
}  // namespace

void icp_step_op(const IcpArgs& a, const float* vmap_curr, const float* nmap_curr, const float* vmap_g_prev,
                 const float* nmap_g_prev, int cols, int rows, float* scratch, float* out29_dev, hipStream_t s) {
  IcpView V{vmap_curr, nmap_curr, vmap_g_prev, nmap_g_prev, cols, rows, a.k, a.distThres, a.angleThres, sq_le_max(a.distThres), sq_lt_max(a.angleThres)};
  RgbView RV{};
  float* pose = scratch + SE3_ACCS * VWARPS;   // 24 floats of parameters behind the partials
  float h[24];
  for (int i = 0; i < 9; ++i) { h[i] = a.Rcurr[i]; h[12 + i] = a.Rprev_inv[i]; }
  for (int i = 0; i < 3; ++i) { h[9 + i] = a.tcurr[i]; h[21 + i] = a.tprev[i]; }
  (void)hipMemcpyAsync(pose, h, sizeof(h), hipMemcpyHostToDevice, s);
  (void)hipStreamSynchronize(s);  // h is a stack buffer
  Se3Inputs in{pose, pose + 9, pose + 12, pose + 21, nullptr, nullptr, 0.f, false};
  launch_accum<true, false, false>(V, RV, in, cols * rows, Se3Out{scratch}, s);
  hipLaunchKernelGGL(k_final_tree_op, dim3(1), dim3(SOLVE_BLOCK), 0, s, (const float*)scratch, SE3_ACCS, op_groups(cols * rows), out29_dev);
}
void rgb_residual_op(const RgbResidualArgs& a, const int16_t* dIdx, const int16_t* dIdy, const float* lastDepth,
                     const float* nextDepth, const uint8_t* lastImage, const uint8_t* nextImage, void* corres, int cols,
                     int rows, int* out2_dev, hipStream_t s) {
  ResidualView V{dIdx, dIdy, lastDepth, nextDepth, lastImage, nextImage, (DataTerm*)corres, cols, rows, a.minScale, a.maxDepthDelta};
  float* params;
  (void)hipMalloc((void**)&params, 12 * sizeof(float));
  float h[12];
  for (int i = 0; i < 9; ++i) h[i] = a.krkinv[i];
  for (int i = 0; i < 3; ++i) h[9 + i] = a.kt[i];
  (void)hipMemcpyAsync(params, h, sizeof(h), hipMemcpyHostToDevice, s);
  (void)hipMemsetAsync(out2_dev, 0, 2 * sizeof(int), s);
  hipLaunchKernelGGL(k_rgb_residual_op, dim3(ceil_div(cols * rows, REDUCE_BLOCK)), dim3(REDUCE_BLOCK), 0, s, V, (const float*)params,
                     (const float*)(params + 9), out2_dev);
  (void)hipStreamSynchronize(s);
  (void)hipFree(params);
}
void rgb_step_op(const void* corres, float sigma, const float* cloud, float fx, float fy, const int16_t* dIdx, const int16_t* dIdy,
                 float sobelScale, int cols, int rows, float* scratch, float* out29_dev, hipStream_t s) {
  IcpView IV{};
  RgbView V{corres, nullptr, cloud, dIdx, dIdy, cols, rows, Intr{fx, fy, 0, 0}, sobelScale};
  Se3Inputs in{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sigma, false};
  launch_accum<false, true, false>(IV, V, in, cols * rows, Se3Out{scratch}, s);
  hipLaunchKernelGGL(k_final_tree_op, dim3(1), dim3(SOLVE_BLOCK), 0, s, (const float*)scratch, SE3_ACCS, op_groups(cols * rows), out29_dev);
}
void so3_step_op(const So3Args& a, const uint8_t* lastImage, const uint8_t* nextImage, int cols, int rows, float* scratch, float* out11_dev,
                 hipStream_t s) {
  hipLaunchKernelGGL(k_so3_op, dim3(so3_grid(cols * rows)), dim3(SO3_BLOCK), 0, s, lastImage, nextImage, cols, rows, a, scratch);
  hipLaunchKernelGGL(k_final_tree_op, dim3(1), dim3(SOLVE_BLOCK), 0, s, (const float*)scratch, SO3_ACCS, op_groups(cols * rows), out11_dev);
}

// ------------------------------------------------------------------------------------------
// probes: the update step and the end of tracking on caller-supplied state
// ------------------------------------------------------------------------------------------
namespace {
// One workgroup runs the head of k_track_step (solve_prefetch, the 58 sums in LDS, solve_step_wave) on a TrackState the host filled in.
// SPLIT_TAIL: 128 threads; the update step stops behind resultRt and its two tails run on wavefronts 0 and 1 side by side.  The three
// lines of that dispatch are restated from k_track_ref's loop (ef_track_ref_persistent.inc) — the one piece of this probe that is a
// copy and not a call.
template <bool SPLIT_TAIL>
__global__ void __launch_bounds__(128) k_gn_update_probe(TrackState* st, const float* __restrict__ sums, const StepArgs A) {
  __shared__ efs::SolveScratch S;
  __shared__ float sums_s[2 * SE3_ACCS];
  const int t = threadIdx.x, wave = t >> 6;
  const GNState* prev = &st->gn[0];
  GNState* next = &st->gn[1];
  efs::SolvePrefetch PF{};
  if (t < 64) PF = efs::solve_prefetch(st, prev, &st->rgb_slots[0][0][0]);
  if (t < 2 * SE3_ACCS) sums_s[t] = sums[t];
  __syncthreads();
  if (t < 64) solve_step_wave<SPLIT_TAIL>(st, prev, next, true, sums_s, A, S, PF, true);
  __syncthreads();
  if (SPLIT_TAIL && S.tail_pending) {   // (uniform: LDS)
    if (wave == 0) efs::gn_tail_pose(S, next, true);
    else if (wave == 1) efs::gn_tail_krk(A.knext, S, next, true);
    __syncthreads();
  }
}
__global__ void k_track_end_tail_probe(TrackState* st, const float* __restrict__ pose12, bool rgb, float weightMultiplier, double* traj) {
  if (threadIdx.x != 0) return;
  track_end_tail(st, pose12, pose12 + 9, rgb, weightMultiplier, traj, 0);
}
}  // namespace

int gn_update_op(const GnUpdateProbe& p, GNState* next_host, double* lastA36, double* lastb6, float* stats4) {
  TrackState* h = new TrackState();
  h->gn[0] = p.prev;
  for (int i = 0; i < 9; ++i) h->Rprev[i] = p.Rprev[i];
  for (int i = 0; i < 3; ++i) h->tprev[i] = p.tprev[i];
  for (int l = 0; l < RGB_SLOTS; ++l) {   // the totals, spread the way the residual pass's workgroups leave them
    h->rgb_slots[0][l][0] = p.count / RGB_SLOTS + (l < p.count % RGB_SLOTS ? 1 : 0);
    h->rgb_slots[0][l][1] = p.sigma / RGB_SLOTS + (l < p.sigma % RGB_SLOTS ? 1 : 0);
  }
  for (int i = 0; i < 36; ++i) h->lastA[i] = lastA36[i];
  for (int i = 0; i < 6; ++i) h->lastb[i] = lastb6[i];
  h->lastICPError = stats4[0]; h->lastICPCount = stats4[1]; h->lastRGBError = stats4[2]; h->lastRGBCount = stats4[3];
  StepArgs A{true, false, p.icp, p.rgb, p.rgbOnly, p.icpWeight, p.knext, p.level_changes, 1};
  TrackState* st = nullptr;
  float* sums = nullptr;
  hipError_t e = hipMalloc((void**)&st, sizeof(TrackState));
  if (e == hipSuccess) e = hipMalloc((void**)&sums, sizeof(p.sums));
  if (e == hipSuccess) e = hipMemcpy(st, h, sizeof(TrackState), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(sums, p.sums, sizeof(p.sums), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    if (p.split_tail) hipLaunchKernelGGL(k_gn_update_probe<true>, dim3(1), dim3(128), 0, 0, st, (const float*)sums, A);
    else hipLaunchKernelGGL(k_gn_update_probe<false>, dim3(1), dim3(64), 0, 0, st, (const float*)sums, A);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(h, st, sizeof(TrackState), hipMemcpyDeviceToHost);
  if (st) (void)hipFree(st);
  if (sums) (void)hipFree(sums);
  if (e == hipSuccess) {
    *next_host = h->gn[1];
    for (int i = 0; i < 36; ++i) lastA36[i] = h->lastA[i];
    for (int i = 0; i < 6; ++i) lastb6[i] = h->lastb[i];
    stats4[0] = h->lastICPError; stats4[1] = h->lastICPCount; stats4[2] = h->lastRGBError; stats4[3] = h->lastRGBCount;
  }
  delete h;
  return (int)e;
}

int track_end_tail_op(TrackState* st_host, const float* pose12, bool rgb, float weightMultiplier, double* logged16) {
  TrackState* st = nullptr;
  float* pose = nullptr;
  double* traj = nullptr;
  hipError_t e = hipMalloc((void**)&st, sizeof(TrackState));
  if (e == hipSuccess) e = hipMalloc((void**)&pose, 12 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&traj, 16 * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(st, st_host, sizeof(TrackState), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(pose, pose12, 12 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_track_end_tail_probe, dim3(1), dim3(64), 0, 0, st, (const float*)pose, rgb, weightMultiplier, traj);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(st_host, st, sizeof(TrackState), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(logged16, traj, 16 * sizeof(double), hipMemcpyDeviceToHost);
  if (st) (void)hipFree(st);
  if (pose) (void)hipFree(pose);
  if (traj) (void)hipFree(traj);
  return (int)e;
}
