// Host code of the tracker, part 2 of 3 (included by ef_track_kernels.hip behind ef_track_host_ops.inc): the frame tier's input launchers — what
// RGBDOdometry::initICP / initICPModel / initRGB / initRGBModel / initFirstRGB do (RGBDOdometry.cpp:121-257), enqueued on device-resident state.
namespace {
// k_model_maps: one lane per level-0 column of a 4-row band (a quad of lanes per 4x4 block)
inline dim3 model_maps_grid(const Pyramid& p) {
  return dim3(ceil_div(p.W(0), 64), ceil_div(p.H(0) / 4, 4));
}
// k_model_maps' arguments for one side of a tracker, from ONE pair of float4 maps (no fill-in choice, no image): the model side writes the
// world-frame vmap_g_prev / nmap_g_prev and lastDepth, the current side (model-to-model tracking) the camera-frame vmap_curr / nmap_curr and nextDepth
ModelMapsArgs model_maps_args(const Pyramid& p, bool model_side, const float* vertex, const float* normal, float maxDepthRGB) {
  ModelMapsArgs A{};
  A.pred_vertex = A.fill_vertex = (const float4*)vertex;
  A.pred_normal = A.fill_normal = (const float4*)normal;
  for (int i = 0; i < NUM_PYRS; ++i) {
    A.vmap[i] = model_side ? p.vmap_g_prev[i] : p.vmap_curr[i];
    A.nmap[i] = model_side ? p.nmap_g_prev[i] : p.nmap_curr[i];
  }
  A.depth0 = model_side ? p.lastDepth[0] : p.nextDepth[0];
  A.cols = p.W(0); A.rows = p.H(0);
  A.maxDepthRGB = maxDepthRGB;
  A.camera_frame = !model_side;
  return A;
}
// One pyramid step (level i -> i + 1) of up to four images of the level's size as ONE launch, blockIdx.z = job (k_pyr_down_multi: each image
// alone is a 5-9 us, launch-bound kernel).  Slots at or beyond the number of jobs are never read.
struct PyrJob { const void* src; void* dst; int type; };
enum { PYR_U16 = 0, PYR_F32 = 1, PYR_U8 = 2 };   // PyrJobs::type
void launch_pyr_step(const Pyramid& p, int i, std::initializer_list<PyrJob> jobs, hipStream_t s) {
  PyrJobs J{};
  int n = 0;
  for (const PyrJob& j : jobs) { J.src[n] = j.src; J.dst[n] = j.dst; J.type[n] = j.type; ++n; }
  J.scols = p.W(i); J.srows = p.H(i);
  dim3 g = tile_grid(p.W(i + 1), p.H(i + 1));
  g.z = n;
  hipLaunchKernelGGL(k_pyr_down_multi, g, tile_block(), 0, s, J);
}
// level i of the frame's u16 depth pyramid: level 0 is the filtered depth image itself (no copy: cudaMemcpy2DFromArray of
// RGBDOdometry.cpp:126-134 existed only to cross the GL/CUDA boundary)
inline const uint16_t* frame_depth(const Pyramid& p, const uint16_t* depth_filtered, int i) { return i == 0 ? depth_filtered : p.depth_tmp[i]; }

SobelLevels sobel_levels_of(const Pyramid& p) {
  SobelLevels L;
  const float minGrad[NUM_PYRS] = {5, 3, 1};  // RGBDOdometry.cpp:112-114
  const float sobelScale = 1.0f / 8.0f;       // RGBDOdometry.cpp:39-40
  for (int i = 0; i < NUM_PYRS; ++i) {
    L.src[i] = p.nextImage[i]; L.dx[i] = p.dIdx[i]; L.dy[i] = p.dIdy[i];
    L.nextDepth[i] = p.nextDepth[i]; L.mask[i] = p.rgbMask[i]; L.corres[i] = p.corres[i];
    L.minScale[i] = (float)(pow((double)minGrad[i], 2.0) / pow((double)sobelScale, 2.0));  // RGBDOdometry.cpp:425
    L.cols[i] = p.W(i); L.rows[i] = p.H(i);
  }
  return L;
}
// the vertex / normal maps of every level of the frame (initICP's second half, RGBDOdometry.cpp:136-147) in one launch
void build_vn_levels(const Pyramid& p, const uint16_t* depth_filtered, Intr k, float cutoff, bool with_sobel, hipStream_t s) {
  VNLevels L;
  for (int i = 0; i < NUM_PYRS; ++i) {
    L.depth[i] = frame_depth(p, depth_filtered, i);
    L.vmap[i] = p.vmap_curr[i];
    L.nmap[i] = p.nmap_curr[i];
    L.cols[i] = p.W(i);
    L.rows[i] = p.H(i);
    L.k[i] = intr_level(k, i);
  }
  L.cutoff = cutoff;
  dim3 g = tile_grid(p.W(0), p.H(0));
  if (with_sobel) {   // init_rgb_sobel's launch rides along
    g.z = 2 * NUM_PYRS;
    hipLaunchKernelGGL(k_vn_sobel_levels, g, tile_block(), 0, s, L, sobel_levels_of(p));
    return;
  }
  g.z = NUM_PYRS;
  hipLaunchKernelGGL(k_vmap_nmap_levels, g, tile_block(), 0, s, L);
}
// the model side's arguments with the fill-in choice, the image and the tally (init_icp_model, model_maps_op)
ModelMapsArgs model_maps_choice_args(const Pyramid& p, bool model_side, const float* pred_vertex, const float* pred_normal, const float* fill_vertex,
                                     const float* fill_normal, const TrackState* st, float maxDepthRGB, const uint8_t* pred_image_rgba,
                                     const uint8_t* fill_image_rgba, bool frameToFrameRGB, bool tally) {
  ModelMapsArgs A = model_maps_args(p, model_side, pred_vertex, pred_normal, maxDepthRGB);
  A.fill_vertex = (const float4*)fill_vertex; A.fill_normal = (const float4*)fill_normal;
  A.pred_image = pred_image_rgba; A.fill_image = fill_image_rgba; A.force_fill_image = frameToFrameRGB;
  A.tally_image = (tally && pred_image_rgba) ? pred_image_rgba : nullptr;
  A.tally_out = const_cast<unsigned*>(&st->dense_count);
  A.last0 = pred_image_rgba ? p.lastImage[0] : nullptr;
  return A;
}
void launch_model_maps(const Pyramid& p, const ModelMapsArgs& A, const TrackState* st, const FramePreprocess* with, hipStream_t s) {
  const dim3 mg = model_maps_grid(p);
  if (with) {   // the frame's depth pre-processing rides on this launch (k_frame_inputs)
    PreArgs P{};
    P.raw = with->raw; P.cols = p.W(0); P.rows = p.H(0); P.maxv = (unsigned)(with->maxD * 1000.0f); P.table = with->table;
    P.filtered = with->filtered; P.metric = with->metric; P.metric_filtered = with->metric_filtered;
    P.rgb3 = with->rgb3; P.next0 = p.nextImage[0]; P.rgb_keep = with->rgb_keep;
    P.tiles_x = (P.cols + pre::PRE_TW - 1) / pre::PRE_TW;
    P.tiles = P.tiles_x * ((P.rows + pre::PRE_TH - 1) / pre::PRE_TH);
    P.mm_x = (int)mg.x;
    hipLaunchKernelGGL(k_frame_inputs, dim3(P.tiles + (int)(mg.x * mg.y)), dim3(64, 4), 0, s, P, A, st);
    return;
  }
  hipLaunchKernelGGL(k_model_maps, mg, dim3(64, 4), 0, s, A, st);
}
}  // namespace

void init_icp_model(const Pyramid& p, const float* pred_vertex, const float* pred_normal, const float* fill_vertex,
                    const float* fill_normal, const TrackState* st, float maxDepthRGB, hipStream_t s, const uint8_t* pred_image_rgba,
                    const uint8_t* fill_image_rgba, bool frameToFrameRGB, const FramePreprocess* with, bool tally) {
  launch_model_maps(p, model_maps_choice_args(p, true, pred_vertex, pred_normal, fill_vertex, fill_normal, st, maxDepthRGB, pred_image_rgba,
                                               fill_image_rgba, frameToFrameRGB, tally), st, with, s);
}
// ef_op_model_maps: init_icp_model's launch on a caller's buffers — a Pyramid that holds nothing but them, a TrackState that holds nothing but
// the pose and the tally
int model_maps_op(const ModelMapsOp& o, unsigned* dense_count_left, hipStream_t s) {
  Pyramid p{};
  p.width = o.cols; p.height = o.rows;
  for (int i = 0; i < NUM_PYRS; ++i) {
    p.vmap_g_prev[i] = p.vmap_curr[i] = o.vmap[i];
    p.nmap_g_prev[i] = p.nmap_curr[i] = o.nmap[i];
  }
  p.lastDepth[0] = p.nextDepth[0] = o.depth0;
  p.lastImage[0] = o.last0;
  p.nextImage[0] = o.next0;
  TrackState* h = new TrackState();
  for (int i = 0; i < 9; ++i) h->R_wc_f[i] = o.R[i];
  for (int i = 0; i < 3; ++i) h->t_wc_f[i] = o.t[i];
  h->dense_count = o.dense_count;
  h->dense_samples = o.dense_samples;
  TrackState* st = nullptr;
  hipError_t e = hipMalloc((void**)&st, sizeof(TrackState));
  if (e == hipSuccess) e = hipMemcpy(st, h, sizeof(TrackState), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launch_model_maps(p, model_maps_choice_args(p, !o.camera_frame, o.pred_vertex, o.pred_normal, o.fill_vertex, o.fill_normal, st, o.maxDepthRGB,
                                                 o.pred_image, o.fill_image, o.force_fill_image, o.tally), st, o.with, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipMemcpy(dense_count_left, &st->dense_count, sizeof(unsigned), hipMemcpyDeviceToHost);
  if (st) (void)hipFree(st);
  delete h;
  return (int)e;
}
void init_icp_maps(const Pyramid& p, const float* vertex, const float* normal, const uint8_t* image_rgba, const TrackState* st,
                   float maxDepthRGB, hipStream_t s) {
  hipLaunchKernelGGL(k_model_maps, model_maps_grid(p), dim3(64, 4), 0, s, model_maps_args(p, false, vertex, normal, maxDepthRGB), st);
  const int n = p.W(0) * p.H(0);
  for (int i = 0; i + 1 < NUM_PYRS; ++i) pyr_down_gauss_f(p.nextDepth[i], p.W(i), p.H(i), p.nextDepth[i + 1], s);
  hipLaunchKernelGGL(k_model_intensity, dim3(ceil_div(n, 256)), dim3(256), 0, s, image_rgba, image_rgba, true, st, n, p.nextImage[0]);
  for (int i = 0; i + 1 < NUM_PYRS; ++i) pyr_down_uchar_gauss(p.nextImage[i], p.W(i), p.H(i), p.nextImage[i + 1], s);
}
// Model-to-model tracking (the local loop closure's second tracker, ElasticFusion.cpp:463-467): initICPModel + initRGBModel on one
// predicted view and init_icp_maps on the other, as FIVE launches instead of twelve — the two k_model_maps, one launch for both level-0
// intensity images, one k_pyr_down_multi per pyramid step over {model depth, current depth, model intensity, current intensity}.  The two
// sides share no buffer (pyr2 / pyr3 keep nextDepth apart from lastDepth), the per-pixel functions are the ones the separate launches
// call: same results (rocprofv3, closed-loop bench: the separate launches were 4.3 + 4.3 + 2.1 per frame, ~76 us).
void init_model_pair(const Pyramid& p, const float* model_vertex, const float* model_normal, const uint8_t* model_image_rgba, const float* cur_vertex,
                     const float* cur_normal, const uint8_t* cur_image_rgba, const TrackState* st, float maxDepthRGB, hipStream_t s) {
  hipLaunchKernelGGL(k_model_maps, model_maps_grid(p), dim3(64, 4), 0, s, model_maps_args(p, true, model_vertex, model_normal, maxDepthRGB), st);
  hipLaunchKernelGGL(k_model_maps, model_maps_grid(p), dim3(64, 4), 0, s, model_maps_args(p, false, cur_vertex, cur_normal, maxDepthRGB), st);
  const int n = p.W(0) * p.H(0);
  hipLaunchKernelGGL(k_rgba_intensity_pair, dim3(ceil_div(n, 256), 2), dim3(256), 0, s, model_image_rgba, cur_image_rgba, n, p.lastImage[0], p.nextImage[0]);
  for (int i = 0; i + 1 < NUM_PYRS; ++i)
    launch_pyr_step(p, i, {{p.lastDepth[i], p.lastDepth[i + 1], PYR_F32}, {p.nextDepth[i], p.nextDepth[i + 1], PYR_F32},
                           {p.lastImage[i], p.lastImage[i + 1], PYR_U8}, {p.nextImage[i], p.nextImage[i + 1], PYR_U8}}, s);
}
// initICP's depth pyramid + the pyramids of populateRGBDData in THREE launches instead of twelve (single-stream frame script; needs
// init_icp_model first): one k_pyr_down_multi per pyramid step over {frame depth u16, model depth f32, model intensity, frame intensity},
// then the per-level vertex / normal maps.  Same per-pixel functions, same results.  Both level-0 intensity images are already there: the
// frame's from the pre-processing launch, the model's from k_model_maps.
void build_pyramids(const Pyramid& p, const uint16_t* depth_filtered, Intr k, float cutoff, hipStream_t s, bool with_sobel) {
  // (both pyramid steps as ONE launch — a workgroup computing the 36 x 36 level-1 pixels its 16 x 16 level-2 tile reads, then the tile — was
  // built and measured in round 6: 25.2 us against 8.0 + 5.4 for the two launches: six dependent 25-tap trips per thread; dropped,
  // profiles/r06q_kernel_stats_fused_pyramid_steps.csv)
  // (one launch per pyramid STAGE — step l -> l + 1 with the maps and the Sobel of level l — measured no faster in round 6: 1934 against 1939
  // frames/s, profiles/r07d_ab_pyramid_stages.log; removed, last present in commit 2372c48)
  for (int i = 0; i + 1 < NUM_PYRS; ++i)
    launch_pyr_step(p, i, {{frame_depth(p, depth_filtered, i), p.depth_tmp[i + 1], PYR_U16}, {p.lastDepth[i], p.lastDepth[i + 1], PYR_F32},
                           {p.lastImage[i], p.lastImage[i + 1], PYR_U8}, {p.nextImage[i], p.nextImage[i + 1], PYR_U8}}, s);
  build_vn_levels(p, depth_filtered, k, cutoff, with_sobel, s);
}
// The two-stream frame script (ef_set_input_overlap; round 6): build_pyramids split by what each kernel READS, so that the half that needs
// nothing but the new frame runs on the input stream beside the previous frame's fusion and prediction.  Same per-pixel functions, same
// results.
//   frame side:  two pyramid steps over {frame depth u16, frame intensity}, the vertex / normal maps of all levels
//   model side:  (behind init_icp_model) two pyramid steps over {model depth f32, model intensity}; the Sobel / photometric-gate launch
//                (init_rgb_sobel) reads both sides (the gate tests the MODEL's depth: quirk Q1) and follows the join
void build_pyramids_frame_side(const Pyramid& p, const uint16_t* depth_filtered, Intr k, float cutoff, hipStream_t s) {
  for (int i = 0; i + 1 < NUM_PYRS; ++i)
    launch_pyr_step(p, i, {{frame_depth(p, depth_filtered, i), p.depth_tmp[i + 1], PYR_U16}, {p.nextImage[i], p.nextImage[i + 1], PYR_U8}}, s);
  build_vn_levels(p, depth_filtered, k, cutoff, false, s);
}
void build_pyramids_model_side(const Pyramid& p, hipStream_t s) {
  for (int i = 0; i + 1 < NUM_PYRS; ++i)
    launch_pyr_step(p, i, {{p.lastDepth[i], p.lastDepth[i + 1], PYR_F32}, {p.lastImage[i], p.lastImage[i + 1], PYR_U8}}, s);
}
void init_rgb_sobel(const Pyramid& p, hipStream_t s) {
  dim3 g = tile_grid(p.W(0), p.H(0));
  g.z = NUM_PYRS;
  hipLaunchKernelGGL(k_sobel_levels, g, tile_block(), 0, s, sobel_levels_of(p));
}
// ef_op_sobel_mask: init_rgb_sobel on a Pyramid that holds nothing but the caller's buffers
void sobel_mask_op(const SobelMaskOp& o, hipStream_t s) {
  Pyramid p{};
  p.width = o.cols; p.height = o.rows;
  for (int i = 0; i < NUM_PYRS; ++i) {
    p.nextImage[i] = const_cast<uint8_t*>(o.nextImage[i]); p.nextDepth[i] = const_cast<float*>(o.nextDepth[i]);
    p.dIdx[i] = o.dIdx[i]; p.dIdy[i] = o.dIdy[i]; p.rgbMask[i] = o.mask[i]; p.corres[i] = o.corres[i];
  }
  init_rgb_sobel(p, s);
}

void init_first_rgb(const Pyramid& p, const uint8_t* rgb3, hipStream_t s) {
  bgr_to_intensity(rgb3, 3, p.W(0), p.H(0), p.lastNextImage[0], s);
  for (int i = 0; i + 1 < NUM_PYRS; ++i) pyr_down_uchar_gauss(p.lastNextImage[i], p.W(i), p.H(i), p.lastNextImage[i + 1], s);
}
