// ================================================================================================
// Box calibration, raw device memory and the operator tier (include/ef_hip.h: ef_dev_*, ef_device_count, ef_set_device, ef_op_*): single
// stages of the frame on caller-owned buffers, no context.  Drives the launchers of ef_track.hpp and ef_map.hpp (kernels in
// ef_track_kernels.hip and ef_map_kernels.hip) plus the three small kernels below.
// ================================================================================================
extern "C" {

// Box calibration for bench.py (GPU boxes of one pool differ by 10-20 %): an EMPTY kernel and a kernel that streams 16 MB in and 16 MB out
// with 16-byte accesses, 200 back-to-back launches each on `stream`, averaged over the batch with two events (so launch gaps are in).
__global__ void k_calib_empty() {}
__global__ void __launch_bounds__(256) k_calib_stream(const float4* __restrict__ src, float4* __restrict__ dst, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[i];
}
int ef_dev_calibrate(void* stream, float* empty_us, float* stream16mb_us) {
  if (!empty_us || !stream16mb_us) return EF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int n = 1 << 20, reps = 200;   // 1 Mi float4 = 16 MiB
  float4 *a = nullptr, *b = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = EF_EHIP;
  float ms = 0;
  if (hipMalloc((void**)&a, (size_t)n * sizeof(float4)) != hipSuccess || hipMalloc((void**)&b, (size_t)n * sizeof(float4)) != hipSuccess) { rc = EF_ENOMEM; goto done; }
  if (hipMemsetAsync(a, 0, (size_t)n * sizeof(float4), s) != hipSuccess) goto done;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) goto done;
  for (int pass = 0; pass < 2; ++pass) {   // pass 0 warms up
    if (hipEventRecord(e0, s) != hipSuccess) goto done;
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_calib_empty, dim3(256), dim3(256), 0, s);
    if (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) goto done;
    *empty_us = 1e3f * ms / reps;
    if (hipEventRecord(e0, s) != hipSuccess) goto done;
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_calib_stream, dim3(2048), dim3(256), 0, s, (const float4*)a, b, n);
    if (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) goto done;
    *stream16mb_us = 1e3f * ms / reps;
  }
  rc = EF_OK;
done:
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (a) (void)hipFree(a);
  if (b) (void)hipFree(b);
  return rc;
}

int ef_dev_alloc(void** dev, size_t bytes) { return hipMalloc(dev, bytes ? bytes : 1) == hipSuccess ? EF_OK : EF_ENOMEM; }
int ef_dev_free(void* dev) { return hipFree(dev) == hipSuccess ? EF_OK : EF_EHIP; }
int ef_dev_upload(void* dev, const void* host, size_t bytes) { return hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice) == hipSuccess ? EF_OK : EF_EHIP; }
int ef_dev_download(void* host, const void* dev, size_t bytes) { return hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) == hipSuccess ? EF_OK : EF_EHIP; }
int ef_dev_memset(void* dev, int value, size_t bytes) { return hipMemset(dev, value, bytes) == hipSuccess ? EF_OK : EF_EHIP; }
int ef_dev_sync(void) { return hipDeviceSynchronize() == hipSuccess ? EF_OK : EF_EHIP; }
int ef_device_count(int* n) { return hipGetDeviceCount(n) == hipSuccess ? EF_OK : EF_EHIP; }
int ef_set_device(int d) { return hipSetDevice(d) == hipSuccess ? EF_OK : EF_EHIP; }

// ---- operator tier: tracking ----
#define OP_TAIL(s)                                                         \
  do {                                                                     \
    hipError_t _e = hipGetLastError();                                     \
    if (_e != hipSuccess) { g_create_error = hipGetErrorString(_e); return EF_EHIP; } \
    return EF_OK;                                                          \
  } while (0)
#define OP_SYNC(s)                                                         \
  do {                                                                     \
    hipError_t _e = hipStreamSynchronize((hipStream_t)(s));                \
    if (_e == hipSuccess) _e = hipGetLastError();                          \
    if (_e != hipSuccess) { g_create_error = hipGetErrorString(_e); return EF_EHIP; } \
  } while (0)

int ef_op_pyr_down(const uint16_t* src, int sc, int sr, uint16_t* dst, void* s) { eft::pyr_down_u16(src, sc, sr, dst, (hipStream_t)s); OP_TAIL(s); }
int ef_op_create_vmap(const ef_intr* k, const uint16_t* depth, int cols, int rows, float cutoff, float* vmap, void* s) {
  eft::create_vmap(depth, cols, rows, eft::Intr{k->fx, k->fy, k->cx, k->cy}, cutoff, vmap, (hipStream_t)s);
  OP_TAIL(s);
}
int ef_op_create_nmap(const float* vmap, int cols, int rows, float* nmap, void* s) { eft::create_nmap(vmap, cols, rows, nmap, (hipStream_t)s); OP_TAIL(s); }
int ef_op_transform_maps(const float* vs, const float* ns, int cols, int rows, const float* R9, const float* t3, float* vd, float* nd, void* s) {
  float* rt = nullptr;
  if (hipMalloc((void**)&rt, 12 * sizeof(float)) != hipSuccess) return EF_ENOMEM;
  float h[12];
  memcpy(h, R9, 36);
  memcpy(h + 9, t3, 12);
  (void)hipMemcpyAsync(rt, h, sizeof(h), hipMemcpyHostToDevice, (hipStream_t)s);
  eft::transform_maps(vs, ns, cols, rows, rt, rt + 9, vd, nd, (hipStream_t)s);
  (void)hipStreamSynchronize((hipStream_t)s);
  (void)hipFree(rt);
  OP_TAIL(s);
}
int ef_op_copy_maps(const float* v4, const float* n4, int cols, int rows, float* tmp, float* vd, float* nd, void* s) {
  eft::copy_maps(v4, n4, cols, rows, tmp, vd, nd, (hipStream_t)s);
  OP_TAIL(s);
}
int ef_op_resize_vmap(const float* in, int sc, int sr, float* out, void* s) { eft::resize_map(in, sc, sr, out, false, (hipStream_t)s); OP_TAIL(s); }
int ef_op_resize_nmap(const float* in, int sc, int sr, float* out, void* s) { eft::resize_map(in, sc, sr, out, true, (hipStream_t)s); OP_TAIL(s); }
int ef_op_pyr_down_gauss_f(const float* src, int sc, int sr, float* dst, void* s) { eft::pyr_down_gauss_f(src, sc, sr, dst, (hipStream_t)s); OP_TAIL(s); }
int ef_op_pyr_down_uchar_gauss(const uint8_t* src, int sc, int sr, uint8_t* dst, void* s) { eft::pyr_down_uchar_gauss(src, sc, sr, dst, (hipStream_t)s); OP_TAIL(s); }
int ef_op_vertices_to_depth(const float* tmp, int cols, int rows, float cutoff, float* dst, void* s) { eft::vertices_to_depth(tmp, cols, rows, cutoff, dst, (hipStream_t)s); OP_TAIL(s); }
int ef_op_image_bgr_to_intensity(const uint8_t* rgba, int cols, int rows, uint8_t* dst, void* s) { eft::bgr_to_intensity(rgba, 4, cols, rows, dst, (hipStream_t)s); OP_TAIL(s); }
int ef_op_compute_derivative_images(const uint8_t* src, int cols, int rows, int16_t* dx, int16_t* dy, void* s) {
  eft::derivative_images(src, cols, rows, dx, dy, (hipStream_t)s);
  OP_TAIL(s);
}
int ef_op_project_to_point_cloud(const float* depth, int cols, int rows, const ef_intr* k0, int level, float* cloud, void* s) {
  eft::project_to_point_cloud(depth, cols, rows, eft::intr_level(eft::Intr{k0->fx, k0->fy, k0->cx, k0->cy}, level), cloud, (hipStream_t)s);
  OP_TAIL(s);
}

static int op_scratch(float** partials, float** out, int nfloats_out) {
  if (hipMalloc((void**)partials, (size_t)eft::OP_SCRATCH_FLOATS * sizeof(float)) != hipSuccess) return EF_ENOMEM;
  if (hipMalloc((void**)out, nfloats_out * sizeof(float)) != hipSuccess) { (void)hipFree(*partials); return EF_ENOMEM; }
  return EF_OK;
}
static void unpack29_host(const float* h, float* A, float* b) {
  int shift = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 7; ++j) {
      const float v = h[shift++];
      if (j == 6) b[i] = v;
      else A[j * 6 + i] = A[i * 6 + j] = v;
    }
}
int ef_op_icp_step(const float* Rc, const float* tc, const float* vc, const float* nc, const float* Rpi, const float* tp, const ef_intr* k,
                   const float* vg, const float* ng, float dist, float ang, int cols, int rows, float* A, float* b, float* res, void* s) {
  if (cols <= 0 || rows <= 0 || cols > 2048 || rows > 2048) return EF_EINVAL;
  eft::IcpArgs a;
  memcpy(a.Rcurr, Rc, 36); memcpy(a.tcurr, tc, 12); memcpy(a.Rprev_inv, Rpi, 36); memcpy(a.tprev, tp, 12);
  a.k = eft::Intr{k->fx, k->fy, k->cx, k->cy};
  a.distThres = dist; a.angleThres = ang;
  float *partials, *out;
  int r = op_scratch(&partials, &out, 32);
  if (r != EF_OK) return r;
  eft::icp_step_op(a, vc, nc, vg, ng, cols, rows, partials, out, (hipStream_t)s);
  float h[32];
  (void)hipMemcpyAsync(h, out, 29 * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)s);
  hipError_t e = hipStreamSynchronize((hipStream_t)s);
  (void)hipFree(partials); (void)hipFree(out);
  if (e != hipSuccess) { g_create_error = hipGetErrorString(e); return EF_EHIP; }
  unpack29_host(h, A, b);
  res[0] = h[27]; res[1] = h[28];
  return EF_OK;
}
int ef_op_compute_rgb_residual(float minScale, const int16_t* dIdx, const int16_t* dIdy, const float* lastDepth, const float* nextDepth,
                               const uint8_t* lastImage, const uint8_t* nextImage, void* corres, float maxDepthDelta, const float* kt,
                               const float* krkinv, int cols, int rows, int* sigma, int* count, void* s) {
  eft::RgbResidualArgs a;
  a.minScale = minScale; a.maxDepthDelta = maxDepthDelta;
  memcpy(a.kt, kt, 12); memcpy(a.krkinv, krkinv, 36);
  int* out;
  if (hipMalloc((void**)&out, 2 * sizeof(int)) != hipSuccess) return EF_ENOMEM;
  eft::rgb_residual_op(a, dIdx, dIdy, lastDepth, nextDepth, lastImage, nextImage, corres, cols, rows, out, (hipStream_t)s);
  int h[2] = {0, 0};
  hipError_t e = hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost);
  (void)hipFree(out);
  if (e != hipSuccess) { g_create_error = hipGetErrorString(e); return EF_EHIP; }
  *count = h[0];
  *sigma = h[1];
  return EF_OK;
}
int ef_op_rgb_step(const void* corres, float sigma, const float* cloud, float fx, float fy, const int16_t* dIdx, const int16_t* dIdy,
                   float sobelScale, int cols, int rows, float* A, float* b, void* s) {
  float *partials, *out;
  int r = op_scratch(&partials, &out, 32);
  if (r != EF_OK) return r;
  eft::rgb_step_op(corres, sigma, cloud, fx, fy, dIdx, dIdy, sobelScale, cols, rows, partials, out, (hipStream_t)s);
  float h[32];
  (void)hipMemcpyAsync(h, out, 29 * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)s);
  hipError_t e = hipStreamSynchronize((hipStream_t)s);
  (void)hipFree(partials); (void)hipFree(out);
  if (e != hipSuccess) { g_create_error = hipGetErrorString(e); return EF_EHIP; }
  unpack29_host(h, A, b);
  return EF_OK;
}
int ef_op_so3_step(const uint8_t* lastImage, const uint8_t* nextImage, const float* ib, const float* kinv, const float* krlr, int cols,
                   int rows, float* A, float* b, float* res, void* s) {
  eft::So3Args a;
  memcpy(a.imageBasis, ib, 36); memcpy(a.kinv, kinv, 36); memcpy(a.krlr, krlr, 36);
  float *partials, *out;
  int r = op_scratch(&partials, &out, 16);
  if (r != EF_OK) return r;
  eft::so3_step_op(a, lastImage, nextImage, cols, rows, partials, out, (hipStream_t)s);
  float h[11];
  (void)hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)s);
  hipError_t e = hipStreamSynchronize((hipStream_t)s);
  (void)hipFree(partials); (void)hipFree(out);
  if (e != hipSuccess) { g_create_error = hipGetErrorString(e); return EF_EHIP; }
  int shift = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 4; ++j) {
      const float v = h[shift++];
      if (j == 3) b[i] = v;
      else A[j * 3 + i] = A[i * 3 + j] = v;
    }
  res[0] = h[9]; res[1] = h[10];
  return EF_OK;
}

// ---- operator tier: the frame tier's fused input launches on caller-owned buffers ----
int ef_op_model_maps(const ef_model_maps_op* a, unsigned* dense_count_left, void* s) {
  if (!a || !dense_count_left || a->cols <= 0 || a->rows <= 0 || a->cols > 2048 || a->rows > 2048 || (a->cols & 3) || (a->rows & 3)) return EF_EINVAL;
  if (!a->pred_vertex || !a->pred_normal || !a->fill_vertex || !a->fill_normal || !a->depth0) return EF_EINVAL;
  if ((a->pred_image == nullptr) != (a->fill_image == nullptr) || (a->pred_image && !a->last0)) return EF_EINVAL;
  for (int i = 0; i < eft::NUM_PYRS; ++i)
    if (!a->vmap[i] || !a->nmap[i]) return EF_EINVAL;
  if (a->joint && (!a->raw || !a->rgb3 || !a->filtered || !a->metric || !a->metric_filtered || !a->next0)) return EF_EINVAL;
  eft::ModelMapsOp o{};
  o.cols = a->cols; o.rows = a->rows;
  o.pred_vertex = a->pred_vertex; o.pred_normal = a->pred_normal; o.fill_vertex = a->fill_vertex; o.fill_normal = a->fill_normal;
  o.pred_image = a->pred_image; o.fill_image = a->fill_image;
  memcpy(o.R, a->R, 36); memcpy(o.t, a->t, 12);
  o.maxDepthRGB = a->max_depth_rgb;
  o.camera_frame = a->camera_frame != 0; o.force_fill_image = a->force_fill_image != 0; o.tally = a->tally != 0;
  o.dense_count = a->dense_count; o.dense_samples = a->dense_samples;
  for (int i = 0; i < eft::NUM_PYRS; ++i) { o.vmap[i] = a->vmap[i]; o.nmap[i] = a->nmap[i]; }
  o.depth0 = a->depth0; o.last0 = a->last0;
  eft::FramePreprocess fp{};
  if (a->joint) {
    fp = eft::FramePreprocess{a->raw, a->depth_cut, efm::bilateral_table(), a->filtered, a->metric, a->metric_filtered, a->rgb3, nullptr};
    if (!fp.table) { g_create_error = "bilateral weight table missing on this device"; return EF_EHIP; }
    o.with = &fp; o.next0 = a->next0;
  }
  const hipError_t e = (hipError_t)eft::model_maps_op(o, dense_count_left, (hipStream_t)s);
  if (e != hipSuccess) { g_create_error = hipGetErrorString(e); return e == hipErrorOutOfMemory ? EF_ENOMEM : EF_EHIP; }
  return EF_OK;
}
int ef_op_sobel_mask(const uint8_t* const* nextImage, const float* const* nextDepth, int cols, int rows, int16_t* const* dIdx, int16_t* const* dIdy,
                     uint8_t* const* mask, uint32_t* const* corres, void* s) {
  if (!nextImage || !nextDepth || !dIdx || !dIdy || !mask || !corres || cols <= 0 || rows <= 0 || cols > 2048 || rows > 2048) return EF_EINVAL;
  eft::SobelMaskOp o{};
  o.cols = cols; o.rows = rows;
  for (int i = 0; i < eft::NUM_PYRS; ++i) {
    if (!nextImage[i] || !nextDepth[i] || !dIdx[i] || !dIdy[i] || !mask[i] || !corres[i]) return EF_EINVAL;
    o.nextImage[i] = nextImage[i]; o.nextDepth[i] = nextDepth[i]; o.dIdx[i] = dIdx[i]; o.dIdy[i] = dIdy[i]; o.mask[i] = mask[i]; o.corres[i] = corres[i];
  }
  eft::sobel_mask_op(o, (hipStream_t)s);
  const hipError_t le = hipGetLastError();   // (a launch that failed: reported as such, not as whatever the synchronise returns)
  if (le != hipSuccess) { g_create_error = hipGetErrorString(le); return EF_EHIP; }
  OP_SYNC(s);
  return EF_OK;
}

// ---- operator tier: the driver's small linear algebra, evaluated on the device ----
}  // extern "C"
namespace {
__global__ void k_linalg_probe(int which, const double* __restrict__ in, double* __restrict__ out) {
  // the two wavefront factorisations of ef_solve_dev.hpp: the earlier one with one element per lane (kept for tests), and the whole matrix in every lane's
  // registers, which is what the update step runs
  if (which == EF_LINALG_LDLT6_WAVE || which == EF_LINALG_LDLT6_EVERY_LANE) {
    __shared__ efs::SolveScratch S;
    const int lane = threadIdx.x;
    if (lane < 6) S.b[lane] = in[36 + lane];
    efs::wave_sync();
    if (which == EF_LINALG_LDLT6_WAVE) efs::ldlt6_wave(in[lane < 36 ? lane : 0], S);
    else efs::ldlt6_every_lane(in[lane < 36 ? lane : 0], S);
    if (lane < 6) out[lane] = S.x[lane];
    return;
  }
  if (threadIdx.x != 0) return;
  switch (which) {
    case EF_LINALG_LDLT6: efl::ldlt_solve<double, 6>(in, in + 36, out); break;
    case EF_LINALG_LDLT3F: {
      float A[9], b[3], x[3];
      for (int i = 0; i < 9; ++i) A[i] = (float)in[i];
      for (int i = 0; i < 3; ++i) b[i] = (float)in[9 + i];
      efl::ldlt_solve<float, 3>(A, b, x);
      for (int i = 0; i < 3; ++i) out[i] = (double)x[i];
      break;
    }
    case EF_LINALG_POLAR3: efl::polar3(in, out); break;
    case EF_LINALG_RODRIGUES: efl::rodrigues(in, out); break;
    case EF_LINALG_SE3_INVERSE: efl::se3_matrix(efl::se3_inverse(efl::se3_from_matrix(in)), out); break;
    case EF_LINALG_SE3_LOG_NORM: out[0] = efl::se3_log_norm(efl::se3_from_matrix(in)); break;
    case EF_LINALG_SCALAR:
      out[0] = sqrt(in[0]); out[1] = in[0] / in[1]; out[2] = sin(in[0]); out[3] = cos(in[0]); out[4] = atan2(in[0], in[1]);
      break;
    case EF_LINALG_MAT_TO_QUAT: {
      efl::mat_to_quat(in, out);
      efl::SE3 T;
      efl::se3_set_rotation(T, in);
      for (int i = 0; i < 4; ++i) out[4 + i] = T.q[i];
      break;
    }
    case EF_LINALG_SE3_MUL: {
      const efl::SE3 T = efl::se3_mul(efl::se3_from_matrix(in), efl::se3_from_matrix(in + 16));
      for (int i = 0; i < 4; ++i) out[i] = T.q[i];
      for (int i = 0; i < 3; ++i) out[4 + i] = T.t[i];
      break;
    }
    case EF_LINALG_SE3_CASTF:
    case EF_LINALG_SE3_INVERSE_F: {
      float M[16];
      if (which == EF_LINALG_SE3_CASTF) efl::se3_castf_matrix(efl::se3_from_matrix(in), M);
      else efl::se3_inverse_matrix_f(efl::se3_from_matrix(in), M);
      for (int i = 0; i < 16; ++i) out[i] = (double)M[i];
      break;
    }
    case EF_LINALG_M4_AFFINE_INVERSE: efl::m4_affine_inverse(in, out); break;
    case EF_LINALG_LDLT_PIVOTS: efl::ldlt_pivots<double, 6>(in, out); break;
    case EF_LINALG_LU_INVERSE6: efl::lu_inverse<double, 6>(in, out); break;
    default: break;
  }
}
}  // namespace
extern "C" {
int ef_op_linalg(int which, const double* in, int n_in, double* out, int n_out) {
  if (!in || !out || n_in <= 0 || n_out <= 0 || n_in > 64 || n_out > 64 || which < 0 || which > EF_LINALG_LU_INVERSE6) return EF_EINVAL;
  double* d;
  if (hipMalloc((void**)&d, 128 * sizeof(double)) != hipSuccess) return EF_ENOMEM;
  (void)hipMemset(d, 0, 128 * sizeof(double));
  (void)hipMemcpy(d, in, n_in * sizeof(double), hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k_linalg_probe, dim3(1), dim3(64), 0, 0, which, (const double*)d, d + 64);
  hipError_t e = hipMemcpy(out, d + 64, n_out * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) { g_create_error = hipGetErrorString(e); return EF_EHIP; }
  return EF_OK;
}

// ---- operator tier: the update step and the end of tracking on caller-supplied state (probes in the tracker's translation unit) ----
static_assert(sizeof(ef_gn_state) == sizeof(eft::GNState), "ef_gn_state is eft::GNState");
int ef_op_gn_update(const ef_gn_update_args* in, ef_gn_state* next, double* lastA36, double* lastb6, float* stats4) {
  if (!in || !next || !lastA36 || !lastb6 || !stats4 || !(in->icp || in->rgb)) return EF_EINVAL;
  eft::GnUpdateProbe p;
  memcpy(p.sums, in->sums, sizeof(p.sums));
  memcpy(&p.prev, &in->prev, sizeof(p.prev));
  memcpy(p.Rprev, in->Rprev, 36); memcpy(p.tprev, in->tprev, 12);
  p.count = in->count; p.sigma = in->sigma;
  p.icp = in->icp != 0; p.rgb = in->rgb != 0; p.rgbOnly = in->rgb_only != 0;
  p.icpWeight = in->icp_weight;
  p.knext = eft::Intr{in->knext.fx, in->knext.fy, in->knext.cx, in->knext.cy};
  p.level_changes = in->level_changes != 0;
  p.split_tail = in->split_tail != 0;
  const hipError_t e = (hipError_t)eft::gn_update_op(p, (eft::GNState*)next, lastA36, lastb6, stats4);
  if (e != hipSuccess) { g_create_error = hipGetErrorString(e); return e == hipErrorOutOfMemory ? EF_ENOMEM : EF_EHIP; }
  return EF_OK;
}
int ef_op_track_end_tail(const float* Rcurr9, const float* tcurr3, const float* Rprev9, const float* tprev3, const double* q_prev4,
                         const double* t_prev3, int rgb, float weight_multiplier, ef_track_end_out* out) {
  if (!Rcurr9 || !tcurr3 || !Rprev9 || !tprev3 || !q_prev4 || !t_prev3 || !out) return EF_EINVAL;
  eft::TrackState* st = new eft::TrackState();
  memcpy(st->Rprev, Rprev9, 36); memcpy(st->tprev, tprev3, 12);
  memcpy(st->q_prev, q_prev4, 32); memcpy(st->t_prev, t_prev3, 24);
  float pose[12];
  memcpy(pose, Rcurr9, 36); memcpy(pose + 9, tcurr3, 12);
  const hipError_t e = (hipError_t)eft::track_end_tail_op(st, pose, rgb != 0, weight_multiplier, out->logged);
  if (e == hipSuccess) {
    memcpy(out->q, st->q, 32); memcpy(out->t, st->t, 24);
    memcpy(out->T_cw, st->T_cw, 64); memcpy(out->pose_f, st->pose_f, 64);
    memcpy(out->R_wc_f, st->R_wc_f, 36); memcpy(out->t_wc_f, st->t_wc_f, 12);
    out->weighting = st->weighting;
  }
  delete st;
  if (e != hipSuccess) { g_create_error = hipGetErrorString(e); return e == hipErrorOutOfMemory ? EF_ENOMEM : EF_EHIP; }
  return EF_OK;
}

// ---- operator tier: pre-processing + map ----
int ef_op_filter_depth(const uint16_t* raw, int cols, int rows, float maxD, uint16_t* filtered, void* s) {
  if (!efm::filter_depth(raw, cols, rows, maxD, filtered, (hipStream_t)s)) return EF_EHIP;   // (no weight table: device ordinal >= 64, allocation or launch failure)
  OP_TAIL(s);
}
int ef_op_metricise_depth(const uint16_t* in, int cols, int rows, float maxD, float* out, void* s) {
  efm::metricise_depth(in, cols, rows, maxD, out, (hipStream_t)s);
  OP_TAIL(s);
}

}  // extern "C"
namespace {
struct OpMap {  // temporary SoA mirror of an AoS surfel list + scratch, for the operator tier
  std::vector<void*> allocs;
  template <typename T>
  T* alloc(size_t n, int fill = 0) {
    void* p = nullptr;
    if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return nullptr;
    (void)hipMemset(p, fill, (n ? n : 1) * sizeof(T));
    allocs.push_back(p);
    return (T*)p;
  }
  efm::SurfelSoA soa(size_t n) { return efm::SurfelSoA{alloc<float4>(n), alloc<float4>(n), alloc<float4>(n)}; }
  ~OpMap() { for (void* p : allocs) (void)hipFree(p); }
};
efm::Cam to_cam(const ef_cam* c) { return efm::Cam{c->cols, c->rows, c->fx, c->fy, c->cx, c->cy}; }
}  // namespace
extern "C" {

int ef_op_seed_map(const ef_cam* cam, const uint8_t* rgb, const float* dm, const float* dmf, int time, float maxDepth, float* surfels,
                   uint32_t* count_host, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  OpMap m;
  const size_t P = (size_t)cam->cols * cam->rows;
  efm::SurfelSoA soa = m.soa(P);
  efm::CompactScratch cs;
  cs.max_chunks = (int)(2 * P / efm::CHUNK + 8);
  cs.flags = m.alloc<uint8_t>(2 * P);
  cs.chunk_count = m.alloc<uint32_t>(cs.max_chunks);
  cs.chunk_offset = m.alloc<uint32_t>(cs.max_chunks);
  cs.totals = m.alloc<uint32_t>(8);
  unsigned* cnt = m.alloc<unsigned>(1);
  efm::seed_map(to_cam(cam), rgb, dm, dmf, time, maxDepth, soa, cnt, cs, s);
  unsigned h = 0;
  (void)hipMemcpyAsync(&h, cnt, sizeof(h), hipMemcpyDeviceToHost, s);
  OP_SYNC(s);
  efm::soa_to_aos(soa, h, surfels, s);
  OP_SYNC(s);
  *count_host = h;
  return EF_OK;
}

int ef_op_predict_indices(const ef_cam* cam, const double* T16, int time, const float* surfels, uint32_t count, float maxDepth, int timeDelta,
                          uint32_t* index, float* vc, float* ct, float* nr, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  OpMap m;
  const size_t P = (size_t)cam->cols * cam->rows;
  efm::SurfelSoA soa = m.soa(count);
  efm::aos_to_soa(surfels, count, soa, s);
  float h[32];
  pose_mats(T16, h, h + 16);
  float* mats = m.alloc<float>(32);
  (void)hipMemcpyAsync(mats, h, sizeof(h), hipMemcpyHostToDevice, s);
  unsigned* cnt = m.alloc<unsigned>(1);
  (void)hipMemcpyAsync(cnt, &count, sizeof(unsigned), hipMemcpyHostToDevice, s);
  unsigned long long* zbuf = m.alloc<unsigned long long>(P, 0xFF);
  efm::IndexMaps im{index, (float4*)vc, (float4*)ct, (float4*)nr};
  efm::predict_indices(to_cam(cam), mats, time, soa, cnt, maxDepth, timeDelta, zbuf, im, s);
  OP_SYNC(s);
  return EF_OK;
}

int ef_op_combined_predict(const ef_cam* cam, const double* T16, const float* surfels, uint32_t count, float maxDepth, float confThreshold,
                           int time, int maxTime, int timeDelta, uint8_t* image, float* vertex, float* normal, uint16_t* timeMap, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  OpMap m;
  const size_t P = (size_t)cam->cols * cam->rows;
  efm::SurfelSoA soa = m.soa(count);
  efm::aos_to_soa(surfels, count, soa, s);
  float h[32];
  pose_mats(T16, h, h + 16);
  float* mats = m.alloc<float>(32);
  (void)hipMemcpyAsync(mats, h, sizeof(h), hipMemcpyHostToDevice, s);
  unsigned* cnt = m.alloc<unsigned>(1);
  (void)hipMemcpyAsync(cnt, &count, sizeof(unsigned), hipMemcpyHostToDevice, s);
  unsigned long long* zbuf = m.alloc<unsigned long long>(P, 0xFF);
  efm::PredictMaps pm{(uchar4*)image, (float4*)vertex, (float4*)normal, timeMap};
  efm::FillMaps none{nullptr, nullptr, nullptr};
  efm::combined_predict(to_cam(cam), mats, soa, cnt, maxDepth, confThreshold, time, maxTime, timeDelta, zbuf, pm, none, nullptr, nullptr, false,
                        nullptr, s);
  OP_SYNC(s);
  return EF_OK;
}

int ef_op_synthesize_depth(const ef_cam* cam, const double* T16, const float* surfels, uint32_t count, float maxDepth, float confThreshold,
                           int time, int maxTime, int timeDelta, float* depth, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  OpMap m;
  const size_t P = (size_t)cam->cols * cam->rows;
  efm::SurfelSoA soa = m.soa(count);
  efm::aos_to_soa(surfels, count, soa, s);
  float h[32];
  pose_mats(T16, h, h + 16);
  float* mats = m.alloc<float>(32);
  (void)hipMemcpyAsync(mats, h, sizeof(h), hipMemcpyHostToDevice, s);
  unsigned* cnt = m.alloc<unsigned>(1);
  (void)hipMemcpyAsync(cnt, &count, sizeof(unsigned), hipMemcpyHostToDevice, s);
  unsigned long long* zbuf = m.alloc<unsigned long long>(P, 0xFF);
  efm::synthesize_depth(to_cam(cam), mats, soa, cnt, maxDepth, confThreshold, time, maxTime, timeDelta, zbuf, depth, s);
  OP_SYNC(s);
  return EF_OK;
}

int ef_op_fill_in(const ef_cam* cam, const uint8_t* image, const float* vertex, const float* normal, const uint16_t* depthFiltered,
                  const uint8_t* rgb, int passthrough, int passthroughImage, uint8_t* fimage, float* fvertex, float* fnormal, void* s_) {
  efm::PredictMaps pm{(uchar4*)image, (float4*)vertex, (float4*)normal, nullptr};
  efm::FillMaps fm{(uchar4*)fimage, (float4*)fvertex, (float4*)fnormal};
  efm::fill_in(to_cam(cam), pm, depthFiltered, rgb, passthrough != 0, passthroughImage != 0, fm, (hipStream_t)s_);
  OP_TAIL(s_);
}

int ef_op_dense_enough(const ef_cam* cam, const uint8_t* image, int* dense_host, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  OpMap m;
  unsigned* cnt = m.alloc<unsigned>(1);
  efm::dense_count(to_cam(cam), (const uchar4*)image, cnt, s);
  unsigned h = 0;
  (void)hipMemcpyAsync(&h, cnt, sizeof(h), hipMemcpyDeviceToHost, s);
  OP_SYNC(s);
  *dense_host = ((float)h / (float)((cam->cols / 20) * (cam->rows / 20)) > 0.75f) ? 1 : 0;
  return EF_OK;
}

int ef_op_fuse(const ef_cam* cam, const double* T16, int time, const uint8_t* rgb, const float* dm, const float* dmf, const uint32_t* index,
               const float* vc, const float* ct, const float* nr, float maxDepth, float weighting, float* surfels, uint32_t count,
               float* newUnstable, uint32_t* newCount, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  OpMap m;
  efm::SurfelSoA soa = m.soa(count);
  efm::aos_to_soa(surfels, count, soa, s);
  float h[33];
  pose_mats(T16, h, h + 16);
  h[32] = weighting;
  float* mats = m.alloc<float>(33);
  (void)hipMemcpyAsync(mats, h, sizeof(h), hipMemcpyHostToDevice, s);
  unsigned* cnt = m.alloc<unsigned>(2);
  (void)hipMemcpyAsync(cnt, &count, sizeof(unsigned), hipMemcpyHostToDevice, s);
  efm::Candidates cand;
  cand.n = (cam->cols / 2) * (cam->rows / 2);
  cand.pos_conf = m.alloc<float4>(cand.n);
  cand.col_time = m.alloc<float4>(cand.n);
  cand.nrm_rad = m.alloc<float4>(cand.n);
  cand.best = m.alloc<uint32_t>(cand.n);
  uint32_t* winner = m.alloc<uint32_t>(count, 0xFF);
  efm::IndexMaps im{(uint32_t*)index, (float4*)vc, (float4*)ct, (float4*)nr};
  efm::fuse(to_cam(cam), mats + 16, time, rgb, dm, dmf, im, maxDepth, mats + 32, soa, cnt, cand, winner, s);
  efm::soa_to_aos(soa, count, surfels, s);
  efm::CompactScratch cs;
  cs.max_chunks = cand.n / efm::CHUNK + 8;
  cs.flags = m.alloc<uint8_t>(cand.n);
  cs.chunk_count = m.alloc<uint32_t>(cs.max_chunks);
  cs.chunk_offset = m.alloc<uint32_t>(cs.max_chunks);
  cs.totals = m.alloc<uint32_t>(8);
  efm::candidates_to_aos(cand, newUnstable, cnt + 1, cs, s);
  unsigned hn = 0;
  (void)hipMemcpyAsync(&hn, cnt + 1, sizeof(hn), hipMemcpyDeviceToHost, s);
  OP_SYNC(s);
  *newCount = hn;
  return EF_OK;
}

}  // extern "C"
namespace {
// scatter an AoS "newUnstable" list (draw order) back into candidate slots 0..n-1: the clean kernels only
// need the relative order, which consecutive slots preserve
__global__ void k_aos_to_cand(const float4* __restrict__ aos, uint32_t n, efm::Candidates cand) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint32_t)cand.n) return;
  if (i < n) {
    cand.pos_conf[i] = aos[(size_t)i * 3];
    cand.col_time[i] = aos[(size_t)i * 3 + 1];
    cand.nrm_rad[i] = aos[(size_t)i * 3 + 2];
  } else {
    cand.col_time[i] = make_float4(0, 0, 0, 0);
  }
}
}  // namespace
extern "C" {

int ef_op_clean_deform(const ef_cam* cam, const double* T16, int time, const uint32_t* index, const float* vc, const float* ct, const float* nr,
                       float confThreshold, int timeDelta, float maxDepth, const float* surfels, uint32_t count, const float* newUnstable,
                       uint32_t newCount, const float* graph, int nodes, const float* depth, int isFern, float* surfels_out,
                       uint32_t* outCount, void* s_) {
  hipStream_t s = (hipStream_t)s_;
  OpMap m;
  const uint32_t cap = count + newCount;
  efm::SurfelSoA soa = m.soa(count), out = m.soa(cap);
  efm::aos_to_soa(surfels, count, soa, s);
  float h[32];
  pose_mats(T16, h, h + 16);
  float* mats = m.alloc<float>(32);
  (void)hipMemcpyAsync(mats, h, sizeof(h), hipMemcpyHostToDevice, s);
  unsigned* cnt = m.alloc<unsigned>(1);
  (void)hipMemcpyAsync(cnt, &count, sizeof(unsigned), hipMemcpyHostToDevice, s);
  efm::Candidates cand;
  cand.n = (int)(newCount ? newCount : 1);
  cand.pos_conf = m.alloc<float4>(cand.n);
  cand.col_time = m.alloc<float4>(cand.n);
  cand.nrm_rad = m.alloc<float4>(cand.n);
  cand.best = m.alloc<uint32_t>(cand.n);
  hipLaunchKernelGGL(k_aos_to_cand, dim3((cand.n + 255) / 256), dim3(256), 0, s, (const float4*)newUnstable, newCount, cand);
  uint32_t* winner = m.alloc<uint32_t>(count, 0xFF);
  efm::CompactScratch cs;
  cs.max_chunks = (int)((cap + 1) / efm::CLEAN_ROW + 8);
  cs.flags = m.alloc<uint8_t>((size_t)cap + 1);
  cs.chunk_count = m.alloc<uint32_t>(cs.max_chunks);
  cs.chunk_offset = m.alloc<uint32_t>(cs.max_chunks);
  cs.totals = m.alloc<uint32_t>(8);
  efm::IndexMaps im{(uint32_t*)index, (float4*)vc, (float4*)ct, (float4*)nr};
  unsigned* cnt_out = m.alloc<unsigned>(1);
  const efm::Deformation def{graph, nodes, depth, isFern, maxDepth};
  efm::clean(to_cam(cam), mats, time, im, confThreshold, timeDelta, soa, cnt, cand, winner, out, cnt_out, cap, cs, nullptr, s,
             nodes > 0 ? &def : nullptr);
  unsigned hn = 0;
  (void)hipMemcpyAsync(&hn, cnt_out, sizeof(hn), hipMemcpyDeviceToHost, s);
  OP_SYNC(s);
  efm::soa_to_aos(out, hn, surfels_out, s);
  OP_SYNC(s);
  *outCount = hn;
  return EF_OK;
}
int ef_op_clean(const ef_cam* cam, const double* T16, int time, const uint32_t* index, const float* vc, const float* ct, const float* nr,
                float confThreshold, int timeDelta, float maxDepth, const float* surfels, uint32_t count, const float* newUnstable,
                uint32_t newCount, float* surfels_out, uint32_t* outCount, void* s_) {
  return ef_op_clean_deform(cam, T16, time, index, vc, ct, nr, confThreshold, timeDelta, maxDepth, surfels, count, newUnstable, newCount,
                            nullptr, 0, nullptr, 0, surfels_out, outCount, s_);
}

}  // extern "C"
