// ================================================================================================
// Looking at a context (include/ef_hip.h): pose, tracking statistics and trajectory, loop-closure state, the map's count, download and the
// two dumps, the images and tracker buffers, stage timers, HIP-event sampling of the dominant kernels, developer hooks.  Nothing of a frame.
// ================================================================================================
namespace {
// an image of ef_get_image / ef_get_image_resized: where it lives (null: not allocated in this context), the bytes of a pixel, and whether
// ef_get_image_resized takes it (the predicted, fill-in and inactive-prediction images); src == nullptr && elem == 0: no such image
struct ImageRef { const void* src; int elem; bool resizable; };
ImageRef image_ref(const ef_ctx* c, int which) {
  switch (which) {
    case EF_IMG_DEPTH_FILTERED: return {c->img.depth_filtered, 2, false};
    case EF_IMG_DEPTH_METRIC: return {c->img.depth_metric, 4, false};
    case EF_IMG_DEPTH_METRIC_FILTERED: return {c->img.depth_metric_filtered, 4, false};
    case EF_IMG_PREDICT_IMAGE: return {c->pm.image, 4, true};
    case EF_IMG_PREDICT_VERTEX: return {c->pm.vertex, 16, true};
    case EF_IMG_PREDICT_NORMAL: return {c->pm.normal, 16, true};
    case EF_IMG_PREDICT_TIME: return {c->pm.time, 2, true};
    case EF_IMG_FILL_IMAGE: return {c->fm.image, 4, true};
    case EF_IMG_FILL_VERTEX: return {c->fm.vertex, 16, true};
    case EF_IMG_FILL_NORMAL: return {c->fm.normal, 16, true};
    case EF_IMG_INDEX: return {c->im.index, 4, false};
    case EF_IMG_VERT_CONF: return {c->im.vert_conf, 16, false};
    case EF_IMG_COLOR_TIME: return {c->im.color_time, 16, false};
    case EF_IMG_NORM_RAD: return {c->im.norm_rad, 16, false};
    case EF_IMG_OLD_IMAGE: return {c->old.image, 4, true};
    case EF_IMG_OLD_VERTEX: return {c->old.vertex, 16, true};
    case EF_IMG_OLD_NORMAL: return {c->old.normal, 16, true};
    case EF_IMG_OLD_TIME: return {c->old.time, 2, true};
    default: return {nullptr, 0, false};
  }
}
}  // namespace

extern "C" {

int ef_get_pose(ef_ctx* c, double* T16) {
  if (!c || !T16) return EF_EINVAL;
  DeviceGuard dg_(c);
  eft::TrackState h;
  EF_TRY(read_state(c, c->st, &h));
  pose_of_state(h, T16);
  return EF_OK;
}
int ef_get_tick(ef_ctx* c, int* tick) { if (!c || !tick) return EF_EINVAL; *tick = c->tick; return EF_OK; }
int ef_get_tracking_stats(ef_ctx* c, float* out6, double* A36, double* b6) {
  if (!c || !out6) return EF_EINVAL;
  DeviceGuard dg_(c);
  eft::TrackState h;
  EF_TRY(read_state(c, c->st, &h));
  out6[0] = h.lastICPError; out6[1] = h.lastICPCount; out6[2] = h.lastRGBError;
  out6[3] = h.lastRGBCount; out6[4] = h.lastSO3Error; out6[5] = h.lastSO3Count;
  if (A36) memcpy(A36, h.lastA, sizeof(h.lastA));
  if (b6) memcpy(b6, h.lastb, sizeof(h.lastb));
  return EF_OK;
}
int ef_get_covariance(ef_ctx* c, double* cov36) {
  if (!c || !cov36) return EF_EINVAL;
  DeviceGuard dg_(c);
  eft::TrackState h;
  EF_TRY(read_state(c, c->st, &h));
  efl::lu_inverse<double, 6>(h.lastA, cov36);   // host side, like the reference (Eigen on the CPU)
  return EF_OK;
}
int ef_get_tracker_fallbacks(ef_ctx* c, int* count) {
  if (!c || !count) return EF_EINVAL;
  DeviceGuard dg_(c);
  int total = 0;
  for (const eft::Pyramid* p : {&c->pyr, &c->pyr2, &c->pyr3}) {
    const int n = eft::tracker_fallbacks(*p, c->stream);
    if (n < 0) { c->err = "reading the tracker's fallback counter failed"; return EF_EHIP; }
    total += n;
  }
  *count = total;
  return EF_OK;
}
// host state only: nothing is enqueued, nothing synchronised
int ef_get_tracker_plan(ef_ctx* c, ef_tracker_plan* out) {
  if (!c || !out) return EF_EINVAL;
  const eft::TrackerPlan& p = c->pyr.plan;
  *out = ef_tracker_plan{p.script, p.n_small, p.n_iter, p.levels, p.res_bytes, p.res_budget};
  return EF_OK;
}
// test hook: raises the sticky abort flag of the frame tracker's persistent launches, as a wait that timed out would
int ef_debug_inject_tracker_abort(ef_ctx* c) {
  if (!c) return EF_EINVAL;
  DeviceGuard dg_(c);
  unsigned* w = eft::tracker_abort_word(c->pyr);
  if (!w) return EF_EINVAL;
  const unsigned one = 1u;
  EF_HIP(c, hipMemcpyAsync(w, &one, sizeof(one), hipMemcpyHostToDevice, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}
// developer instrumentation: per-phase clocks of the persistent small-level launch (-DEF_STAGE_CLOCKS builds; tools/small_clocks.py)
int ef_debug_small_clocks(ef_ctx* c, unsigned long long* out32) {
  if (!c || !out32) return EF_EINVAL;
  DeviceGuard dg_(c);
  return eft::tracker_small_clocks(c->pyr, out32, c->stream) == 0 ? EF_OK : EF_EHIP;
}
int ef_debug_clocks(ef_ctx* c, unsigned long long* out16) {
  if (!c || !out16) return EF_EINVAL;
  DeviceGuard dg_(c);
  eft::TrackState h;
  EF_TRY(read_state(c, c->st, &h));
  memcpy(out16, h.dbg_clock, sizeof(h.dbg_clock));
  return EF_OK;
}
int ef_get_trajectory(ef_ctx* c, double* T16s, int64_t* stamps, int max_frames, int* n_frames) {
  if (!c || !n_frames) return EF_EINVAL;
  DeviceGuard dg_(c);
  int n = (int)c->stamps.size();
  if (n > max_frames) n = max_frames;
  if (T16s && n) {
    const int rf = flush_end_record(c);
    if (rf != EF_OK) return rf;
    EF_HIP(c, hipMemcpyAsync(T16s, c->traj, (size_t)n * 16 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    EF_HIP(c, hipStreamSynchronize(c->stream));
    // "Output deformed pose graph" (ElasticFusion.cpp:107-139): every accepted Deformation::constrain moves the poses logged so far
    // (DeformationGraph::applyGraphToPoses), so with loop closures on the log to hand out is the closure object's copy of t_T_wc — the
    // device log holds each frame's pose as it was when the frame ended.  The closure object logs one pose per frame from the frame
    // ef_enable_global_closure was called before: it covers the LAST `m` frames.
    if (c->closure) {
      const int total = (int)c->stamps.size(), m = ef_closure_trajectory(c->closure, nullptr, 0), first = total - m;
      if (m > 0 && first >= 0 && first < n) {
        std::vector<double> P((size_t)m * 16);
        ef_closure_trajectory(c->closure, P.data(), m);
        memcpy(T16s + (size_t)first * 16, P.data(), (size_t)(n - first) * 16 * sizeof(double));
      }
    }
  }
  if (stamps) for (int i = 0; i < n; ++i) stamps[i] = c->stamps[i];
  *n_frames = n;
  return EF_OK;
}
int ef_get_pose_qt(ef_ctx* c, double* q4_t3) {
  if (!c || !q4_t3) return EF_EINVAL;
  DeviceGuard dg_(c);
  eft::TrackState h;
  EF_TRY(read_state(c, c->st, &h));
  for (int i = 0; i < 4; ++i) q4_t3[i] = h.q[i];
  for (int i = 0; i < 3; ++i) q4_t3[4 + i] = h.t[i];
  return EF_OK;
}
int ef_get_relocalisation(ef_ctx* c, ef_reloc_state* out) {
  if (!c || !out) return EF_EINVAL;
  out->lost = c->lost; out->tracking_ok = c->tracking_ok; out->tracking_count = c->tracking_count; out->last_frame_recovery = c->last_frame_recovery;
  return EF_OK;
}
int ef_get_global_loop(ef_ctx* c, ef_global_loop* info) {
  if (!c || !info) return EF_EINVAL;
  *info = c->gloop;
  return EF_OK;
}
ef_closure* ef_get_closure(ef_ctx* c) {
  if (!c) return nullptr;
  DeviceGuard dg_(c);
  (void)flush_end_record(c);   // the last frame's keyframe decision and trajectory entry are part of what the caller will look at
  return c->closure;
}
int ef_get_local_loop(ef_ctx* c, ef_local_loop* info, double* constraints, int max_constraints, int* n_out) {
  if (!c || !info) return EF_EINVAL;
  *info = c->loop;
  int n = c->loop.n_constraints < max_constraints ? c->loop.n_constraints : max_constraints;
  if (!constraints) n = 0;
  if (n > 0) memcpy(constraints, c->loop_constraints.data(), (size_t)n * 8 * sizeof(double));
  if (n_out) *n_out = n;
  return EF_OK;
}
int ef_sample_graph(ef_ctx* c, float* nodes4, int max_nodes, int* n_out) {
  if (!c || !nodes4 || !n_out || max_nodes <= 0) return EF_EINVAL;
  DeviceGuard dg_(c);
  float* dev = nullptr;
  EF_HIP(c, hipMalloc((void**)&dev, ((size_t)max_nodes * 4 + 4) * sizeof(float)));
  unsigned* n_dev = (unsigned*)(dev + (size_t)max_nodes * 4);
  efm::sample_graph(c->maps[c->cur], &c->st->map_counts[c->cur], 5000, max_nodes, dev, n_dev, c->stream);
  unsigned n = 0;
  hipError_t e = hipMemcpyAsync(&n, n_dev, sizeof(n), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess && n > 0) e = hipMemcpy(nodes4, dev, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  EF_HIP(c, e);
  *n_out = (int)n;
  return EF_OK;
}
int ef_map_count(ef_ctx* c, uint32_t* count) {
  if (!c || !count) return EF_EINVAL;
  DeviceGuard dg_(c);
  return read_count(c, count);
}
int ef_map_download(ef_ctx* c, float* surfels, uint32_t max_surfels, uint32_t* count) {
  if (!c || !count) return EF_EINVAL;
  DeviceGuard dg_(c);
  if (c->labels.ids_on) {   // rows created since the last ID-consuming call get theirs first
    const int ri = ids_prepare(c, "ef_map_download");
    if (ri != EF_OK) return ri;
  }
  uint32_t n = 0;
  int r = ef_map_count(c, &n);
  if (r != EF_OK) return r;
  if (n > max_surfels) n = max_surfels;
  *count = n;
  if (!surfels || !n) return EF_OK;
  // The reference's downloadMap() reads the buffer its update pass wrote — the map BEFORE clean — truncated to the count AFTER
  // clean (quirk Q14); by default this returns model(), the map as it stands; ef_set_reference_download selects the reference's.
  float* tmp = nullptr;
  EF_HIP(c, hipMalloc((void**)&tmp, (size_t)n * 48));
  efm::soa_to_aos(c->reference_download ? c->shadow : c->maps[c->cur], n, tmp, c->stream);
  hipError_t e = hipMemcpyAsync(surfels, tmp, (size_t)n * 48, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  EF_HIP(c, e);
  return EF_OK;
}
// Host-only writers (no context, no GPU): the two dumps of the reference, byte for byte.
//   trajectory: ~ElasticFusion, ElasticFusion.cpp:112-139 — "timestamp tx ty tz qx qy qz qw" per pose, the timestamp as microseconds / 1e6
//     with six decimals, the seven numbers as an ostream prints a double by default (six significant digits, %g);
//   map: ElasticFusion::savePly, :684-781 — binary little-endian PLY of the surfels with confidence above the threshold:
//     x y z, r g b unpacked from the colour float, the NEGATED normal (:741-743), the radius.
int ef_write_freiburg(const char* path, const double* T_wc16_array, const int64_t* timestamps, int n) {
  if (!path || (n > 0 && (!T_wc16_array || !timestamps))) return EF_EINVAL;
  FILE* f = fopen(path, "w");
  if (!f) return EF_EINVAL;
  for (int i = 0; i < n; ++i) {
    const efl::SE3 S = efl::se3_from_matrix(T_wc16_array + (size_t)i * 16);
    fprintf(f, "%.6f %g %g %g %g %g %g %g\n", (double)timestamps[i] / 1000000.0, S.t[0], S.t[1], S.t[2], S.q[0], S.q[1], S.q[2], S.q[3]);
  }
  fclose(f);
  return EF_OK;
}
int ef_write_ply(const char* path, const float* surfels, uint32_t count, float confidence_threshold) {
  if (!path || (count > 0 && !surfels)) return EF_EINVAL;
  uint32_t valid = 0;
  for (uint32_t i = 0; i < count; ++i) valid += surfels[(size_t)i * 12 + 3] > confidence_threshold;
  FILE* f = fopen(path, "wb");
  if (!f) return EF_EINVAL;
  fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %u\nproperty float x\nproperty float y\nproperty float z\n"
             "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty float nx\nproperty float ny\nproperty float nz\n"
             "property float radius\nend_header\n", valid);
  for (uint32_t i = 0; i < count; ++i) {
    const float* s = surfels + (size_t)i * 12;
    if (!(s[3] > confidence_threshold)) continue;
    const int col = (int)s[4];
    const unsigned char rgbc[3] = {(unsigned char)((col >> 16) & 0xFF), (unsigned char)((col >> 8) & 0xFF), (unsigned char)(col & 0xFF)};
    const float nr[4] = {s[8] * -1, s[9] * -1, s[10] * -1, s[11]};
    fwrite(s, sizeof(float), 3, f);
    fwrite(rgbc, 1, 3, f);
    fwrite(nr, sizeof(float), 4, f);
  }
  fclose(f);
  return EF_OK;
}
int ef_save_freiburg(ef_ctx* c, const char* path) {
  if (!c || !path) return EF_EINVAL;
  DeviceGuard dg_(c);
  const int n = (int)c->stamps.size();
  std::vector<double> T((size_t)n * 16);
  int got = 0;
  int r = ef_get_trajectory(c, T.data(), nullptr, n, &got);
  if (r != EF_OK) return r;
  r = ef_write_freiburg(path, T.data(), c->stamps.data(), got);
  if (r != EF_OK) c->err = std::string("cannot open ") + path;
  return r;
}
int ef_save_ply(ef_ctx* c, const char* path) {
  if (!c || !path) return EF_EINVAL;
  DeviceGuard dg_(c);
  uint32_t n = 0;
  int r = ef_map_count(c, &n);
  if (r != EF_OK) return r;
  std::vector<float> m((size_t)n * 12);
  r = ef_map_download(c, m.data(), n, &n);
  if (r != EF_OK) return r;
  r = ef_write_ply(path, m.data(), n, c->cfg.confidence);
  if (r != EF_OK) c->err = std::string("cannot open ") + path;
  return r;
}

// the four index maps of the last fusing frame, resolved now from the keys its second predictIndices left (ef_ctx::zbuf_clean)
static void im_materialise(ef_ctx* c) {
  if (!c->im_pending) return;
  efm::resolve_indices(c->cam, c->im_T16, c->maps[c->im_map], c->zbuf_clean, c->im, c->stream);
  c->im_pending = false;
}
int ef_get_image(ef_ctx* c, int which, void* dst, size_t bytes) {
  if (!c || !dst) return EF_EINVAL;
  DeviceGuard dg_(c);
  const size_t P = (size_t)c->cam.cols * c->cam.rows;
  if (which >= EF_IMG_INDEX && which <= EF_IMG_NORM_RAD) im_materialise(c);
  const ImageRef im = image_ref(c, which);
  if (!im.elem) { c->err = "ef_get_image: unknown image"; return EF_EINVAL; }
  const void* src = im.src;
  const size_t need = P * (size_t)im.elem;
  if (!src) { c->err = "ef_get_image: this image only exists in a close_loops context"; return EF_ESTATE; }
  if (bytes < need) { c->err = "ef_get_image: destination too small"; return EF_EINVAL; }
  void* tmp = nullptr;
  if (c->im.colmajor && which >= EF_IMG_INDEX && which <= EF_IMG_NORM_RAD) {
    EF_HIP(c, hipMalloc(&tmp, need));
    const int W = c->cam.cols, H = c->cam.rows;
    const dim3 g((unsigned)((P + 255) / 256));
    if (which == EF_IMG_INDEX) hipLaunchKernelGGL(k_to_rowmajor<uint32_t>, g, dim3(256), 0, c->stream, (const uint32_t*)src, W, H, (uint32_t*)tmp);
    else hipLaunchKernelGGL(k_to_rowmajor<float4>, g, dim3(256), 0, c->stream, (const float4*)src, W, H, (float4*)tmp);
    src = tmp;
  }
  hipError_t e = hipMemcpyAsync(dst, src, need, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (tmp) (void)hipFree(tmp);
  EF_HIP(c, e);
  return EF_OK;
}
int ef_get_image_resized(ef_ctx* c, int which, int factor, void* dst, size_t bytes) {
  if (!c || !dst || factor < 1) return EF_EINVAL;
  DeviceGuard dg_(c);
  const int W = c->cam.cols, H = c->cam.rows, dw = W / factor, dh = H / factor;
  const ImageRef im = image_ref(c, which);
  if (!im.resizable) { c->err = "ef_get_image_resized: a predicted, fill-in or inactive-prediction image"; return EF_EINVAL; }
  const void* src = im.src;
  const int elem = im.elem;
  if (!src) { c->err = "ef_get_image_resized: this image only exists in a close_loops context"; return EF_ESTATE; }
  const size_t need = (size_t)dw * dh * elem;
  if (dw == 0 || dh == 0 || bytes < need) { c->err = "ef_get_image_resized: destination too small"; return EF_EINVAL; }
  void* tmp = nullptr;
  EF_HIP(c, hipMalloc(&tmp, need));
  const dim3 g((unsigned)((dw * dh + 255) / 256));
  if (elem == 16) hipLaunchKernelGGL(k_resize_nearest<float4>, g, dim3(256), 0, c->stream, (const float4*)src, W, dw, dh, factor, (float4*)tmp);
  else if (elem == 4) hipLaunchKernelGGL(k_resize_nearest<uint32_t>, g, dim3(256), 0, c->stream, (const uint32_t*)src, W, dw, dh, factor, (uint32_t*)tmp);
  else hipLaunchKernelGGL(k_resize_nearest<uint16_t>, g, dim3(256), 0, c->stream, (const uint16_t*)src, W, dw, dh, factor, (uint16_t*)tmp);
  hipError_t e = hipMemcpyAsync(dst, tmp, need, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  EF_HIP(c, e);
  return EF_OK;
}
int ef_get_tracker_buffer(ef_ctx* c, int which, int level, void* dst, size_t bytes) { return ef_get_tracker_buffer_of(c, 0, which, level, dst, bytes); }
int ef_get_tracker_buffer_of(ef_ctx* c, int tracker, int which, int level, void* dst, size_t bytes) {
  if (!c || !dst || level < 0 || level >= eft::NUM_PYRS || tracker < 0 || tracker > 1) return EF_EINVAL;
  DeviceGuard dg_(c);
  const size_t n = (size_t)(c->cam.cols >> level) * (c->cam.rows >> level);
  const void* src = nullptr;
  size_t need = 0;
  const eft::Pyramid& p = tracker == 0 ? c->pyr : c->pyr2;
  if (!p.partials) { c->err = "ef_get_tracker_buffer_of: the model-to-model tracker only exists in a close_loops context"; return EF_ESTATE; }
  switch (which) {
    case 0: src = p.vmap_curr[level]; need = n * 12; break;
    case 1: src = p.nmap_curr[level]; need = n * 12; break;
    case 2: src = p.vmap_g_prev[level]; need = n * 12; break;
    case 3: src = p.nmap_g_prev[level]; need = n * 12; break;
    case 4: src = p.lastDepth[level]; need = n * 4; break;
    case 5: src = p.nextDepth[level]; need = n * 4; break;   // (tracker 0: the same buffers as lastDepth, quirk Q1)
    case 6: src = p.lastImage[level]; need = n; break;
    case 7: src = p.nextImage[level]; need = n; break;
    case 8: src = p.lastNextImage[level]; need = n; break;
    case 9: src = p.dIdx[level]; need = n * 2; break;
    case 10: src = p.dIdy[level]; need = n * 2; break;
    case 11: src = (level == 0 && tracker == 0) ? c->img.depth_filtered : p.depth_tmp[level]; need = n * 2; break;
    case 12: src = p.rgbMask[level]; need = n; break;
    case 13: src = p.corres[level]; need = n * 4; break;
    default: c->err = "ef_get_tracker_buffer: unknown buffer"; return EF_EINVAL;
  }
  if (bytes < need) { c->err = "ef_get_tracker_buffer: destination too small"; return EF_EINVAL; }
  EF_HIP(c, hipMemcpyAsync(dst, src, need, hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}

int ef_enable_timing(ef_ctx* c, int on) { if (!c) return EF_EINVAL; c->timing = on != 0; return EF_OK; }
int ef_get_timings(ef_ctx* c, ef_timing* out, int max, int* n) {
  if (!c || !n) return EF_EINVAL;
  DeviceGuard dg_(c);
  EF_HIP(c, hipStreamSynchronize(c->stream));
  int k = 0;
  for (auto& t : c->timers) {
    if (!t.used || k >= max) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t.a, t.b) != hipSuccess) ms = -1.f;
    if (out) { out[k].name = t.name; out[k].ms = ms; }
    ++k;
  }
  *n = k;
  return EF_OK;
}

// ---- device helpers ----
int ef_kernel_timing(ef_ctx* c, int every_n_frames) {
  if (!c || every_n_frames < 0) return EF_EINVAL;
  DeviceGuard dg_(c);
  EF_HIP(c, hipStreamSynchronize(c->stream));
  c->ktime_every = every_n_frames;
  KernelSampler* const all[3] = {&c->sample_all, &c->sample_splat, &c->sample_step};
  const int capacity[3] = {1024, 1024, 4096};
  for (int i = 0; i < 3; ++i) {
    all[i]->probe.used = 0;
    if (every_n_frames > 0) EF_TRY(all[i]->create(c, capacity[i]));
  }
  return EF_OK;
}
int ef_get_kernel_timing(ef_ctx* c, ef_kernel_time* out) {
  if (!c || !out) return EF_EINVAL;
  DeviceGuard dg_(c);
  EF_TRY(c->sample_step.average_us(c, &out->avg_us));
  const bool icp = !c->cfg.rgb_only && c->cfg.icp_weight > 0, rgb = c->cfg.rgb_only || c->cfg.icp_weight < 100;
#ifdef EF_FAST_ORDER
  out->name = "k_se3_accum_fast (level 0 of the launch-per-step script: icpStep + rgbStep Jacobian rows + fast-order sums)";
#else
  out->name = "k_se3_accum (level 0: icpStep + rgbStep Jacobian rows + reference-order sums)";
#endif
  out->launches = c->sample_step.probe.used;
  // algorithmic bytes of ONE launch of this kernel (DESIGN.md "Roofline accounting"): icpStep 48 B per pixel-visit
  // (4 planar float3 maps, SURVEY.md 8d); rgbStep reads the 4-byte packed correspondence of every pixel — the
  // reference's 16-byte DataTerm + 12-byte cloud are gone, so they are not counted — the ~10 % valid pixels' gathers
  // (depth + 2 gradients) are left out (data dependent): a lower bound, which can only understate `achieved`
  out->bytes_per_launch = (double)c->cam.cols * c->cam.rows * ((icp ? 48.0 : 0.0) + (rgb ? 4.0 : 0.0));
  out->bytes_per_launch_survey = (double)c->cam.cols * c->cam.rows * (icp ? 48.0 : 0.0);   // SURVEY.md 8(d): the ICP reduction alone
  return EF_OK;
}

// the persistent tracker launch (k_track_fast: SO(3) loop + every Gauss-Newton iteration of every level + their update steps)
int ef_get_tracker_timing(ef_ctx* c, ef_kernel_time* out) {
  if (!c || !out) return EF_EINVAL;
  DeviceGuard dg_(c);
  EF_TRY(c->sample_all.average_us(c, &out->avg_us));
  const bool icp = !c->cfg.rgb_only && c->cfg.icp_weight > 0, rgb = c->cfg.rgb_only || c->cfg.icp_weight < 100;
#ifdef EF_FAST_ORDER
  out->name = "k_track_fast (the whole tracker as one persistent launch: SO(3) loop + every ICP+RGB iteration of every level + the update steps)";
#else
  out->name = "k_track_ref (the whole tracker as one persistent launch, reference summation order: SO(3) loop + every ICP+RGB iteration of every level + the update steps)";
#endif
  out->launches = c->sample_all.probe.used;
  // algorithmic bytes of one launch: every iteration visits every pixel of its level once (48 B icpStep + 4 B packed correspondence, as
  // ef_get_kernel_timing counts one level-0 launch); the SO(3) loop's two u8 images are left out (a lower bound)
  const int its[3] = {c->cfg.fast_odom ? 3 : 10, c->cfg.pyramid ? 5 : 0, c->cfg.pyramid ? 4 : 0};
  double visits = 0;
  for (int l = 0; l < 3; ++l) visits += (double)its[l] * (double)(c->cam.cols >> l) * (double)(c->cam.rows >> l);
  out->bytes_per_launch = visits * ((icp ? 48.0 : 0.0) + (rgb ? 4.0 : 0.0));
  out->bytes_per_launch_survey = visits * (icp ? 48.0 : 0.0);
  return EF_OK;
}

int ef_get_splat_timing(ef_ctx* c, ef_kernel_time* out) {
  if (!c || !out) return EF_EINVAL;
  DeviceGuard dg_(c);
  EF_TRY(c->sample_splat.average_us(c, &out->avg_us));
  unsigned count = 0;
  EF_HIP(c, hipMemcpy(&count, &c->st->map_counts[c->cur], sizeof(count), hipMemcpyDeviceToHost));
  out->name = "k_index_splat (IndexMap::predictIndices: per-surfel transform + project + 64-bit atomicMin z-buffer)";
  out->launches = c->sample_splat.probe.used;
  // algorithmic bytes: the two float4 streams the pass needs (position+confidence, colour+times: 32 B / surfel; the
  // reference's vertex shader fetches all 48) + one 8-byte z-buffer update per surfel (an upper bound: culled surfels issue none)
  out->bytes_per_launch = 40.0 * (double)count;
  out->bytes_per_launch_survey = 48.0 * (double)count;   // SURVEY.md 8(d): 48 B per surfel read by the reference's vertex shader
  return EF_OK;
}

}  // extern "C"
