// ================================================================================================
// Rigid registration of a point set against the map (include/ef_hip.h: ef_default_register_params, ef_register_update, ef_register_step[_dev],
// ef_register_cloud[_dev]; kernels in ef_register.inc, the index of ef_host_query.inc; DESIGN.md §8c)
// ================================================================================================
namespace {
struct RegisterCall {
  const char* fn;
  const float* points;
  const float* normals;
  uint32_t n;
  const ef_register_params* p;
  const double* T;   // null = identity
  uint32_t* row;
  float* plane;
};
const double REG_IDENTITY[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
// refusals before any GPU work
int register_check(ef_ctx* c, const RegisterCall& q, const void* out, const char* out_name) {
  std::string& err = c ? c->err : g_create_error;
  const std::string fn = q.fn;
  if (!q.p) { err = fn + ": null params"; return EF_EINVAL; }
  if (!out) { err = fn + ": null " + out_name; return EF_EINVAL; }
  static uint32_t row_stand_in;
  const QueryCall qc{q.fn, q.points, q.n, 1, q.p->max_dist, q.p->min_conf, &row_stand_in, nullptr, nullptr, nullptr, nullptr};
  if (std::isnan(q.p->min_normal_cos)) { err = fn + ": min_normal_cos is NaN"; return EF_EINVAL; }
  if (q.p->max_iterations < 1 || q.p->max_iterations > EF_REGISTER_MAX_ITERATIONS) {
    err = fn + ": max_iterations must lie in 1 .. " + std::to_string(EF_REGISTER_MAX_ITERATIONS);
    return EF_EINVAL;
  }
  if (q.p->min_pairs < 6) { err = fn + ": min_pairs must be at least 6"; return EF_EINVAL; }
  if (!(q.p->stop_translation >= 0.0) || !std::isfinite(q.p->stop_translation) || !(q.p->stop_rotation >= 0.0) ||
      !std::isfinite(q.p->stop_rotation)) {
    err = fn + ": the stop bounds must be finite and not negative";
    return EF_EINVAL;
  }
  if (q.T && !finite16(q.T)) { err = fn + ": T has a non-finite entry"; return EF_EINVAL; }
  return query_check(c, qc);
}
double register_rms(const ef_register_sums& s) { return s.pairs ? std::sqrt(s.e / (double)s.pairs) : 0.0; }
// one step with DEVICE pointers in q; waits for the 29 sums
int register_step_run(ef_ctx* c, const RegisterCall& q, const double* T, ef_register_sums* out) {
  memset(out, 0, sizeof(*out));
  out->points = q.n;
  if (!q.n) return EF_OK;
  int r = query_index(c, c->query.cell);
  if (r != EF_OK) return r;
  const size_t slab_bytes = (size_t)efm::REGISTER_MAX_BLOCKS * efm::REGISTER_SLOTS * sizeof(double);
  r = c->reg.slabs.reserve(c, slab_bytes + efm::REGISTER_SLOTS * sizeof(double), "registration slabs");
  if (r != EF_OK) return r;
  if (!c->reg.sums_h) EF_HIP(c, hipHostMalloc((void**)&c->reg.sums_h, efm::REGISTER_SLOTS * sizeof(double)));
  efm::RegisterArgs a{};
  query_index_args(c, &a.q);
  a.q.points = q.points;
  a.q.n = q.n;
  a.q.k = 1;
  a.q.max_dist = q.p->max_dist;
  a.q.r2 = q.p->max_dist * q.p->max_dist;
  a.q.min_conf = q.p->min_conf;
  a.q.row = q.row;
  a.q.plane = q.plane;
  a.normals = q.normals;
  pose_Rt(T, a.R, a.t);
  a.min_normal_cos = q.p->min_normal_cos;
  a.gate = q.normals && q.p->min_normal_cos > -1.0f;
  a.slabs = c->reg.slabs.as<double>();
  a.sums = (double*)(c->reg.slabs.p + slab_bytes);
  efm::register_step(a, c->stream);
  EF_HIP(c, hipGetLastError());
  EF_HIP(c, hipMemcpyAsync(c->reg.sums_h, a.sums, efm::REGISTER_SLOTS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  const double* v = c->reg.sums_h;
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) out->A[i * 6 + j] = out->A[j * 6 + i] = v[k++];
  for (int i = 0; i < 6; ++i) out->b[i] = v[21 + i];
  out->e = v[27];
  out->pairs = (uint32_t)v[28];
  return EF_OK;
}
// the loop of the header comment; DEVICE pointers in q
int register_loop(ef_ctx* c, const RegisterCall& q, double* T_out, ef_register_result* res) {
  double T[16];
  memcpy(T, q.T ? q.T : REG_IDENTITY, sizeof(T));
  memset(res, 0, sizeof(*res));
  int closing = -1;
  for (bool first = true;; first = false) {
    ef_register_sums s;
    const int r = register_step_run(c, q, T, &s);
    if (r != EF_OK) return r;
    if (first) res->rms_first = register_rms(s);
    res->rms_last = register_rms(s);
    res->pairs = s.pairs;
    memcpy(res->A, s.A, sizeof(res->A));
    if (closing >= 0) { res->status = closing; break; }
    if (s.pairs < (uint32_t)q.p->min_pairs) { res->status = EF_REG_TOO_FEW_PAIRS; break; }
    double Tn[16], xi[6];
    const int u = ef_register_update(&s, T, Tn, xi);
    if (u == EF_REG_DEGENERATE) { res->status = EF_REG_DEGENERATE; break; }
    if (u != EF_OK) { c->err = std::string(q.fn) + ": the update refused its input"; return u; }
    memcpy(T, Tn, sizeof(T));
    ++res->iterations;
    const double dt = std::sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]), dw = std::sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
    if (dt < q.p->stop_translation && dw < q.p->stop_rotation) closing = EF_REG_CONVERGED;
    else if (res->iterations >= q.p->max_iterations) closing = EF_REG_MAX_ITERATIONS;
  }
  memcpy(T_out, T, sizeof(T));
  return EF_OK;
}
// HOST points / normals / row / plane: staged, the device call run, the per-point outputs copied back
template <typename Run>
int register_host(ef_ctx* c, const RegisterCall& q, Run run) {
  const size_t n = q.n;
  const size_t o_pts = 0, o_nrm = o_pts + n * 12, o_row = o_nrm + (q.normals ? n * 12 : 0), o_pl = o_row + n * 4;
  RegisterCall d = q;
  if (n) {
    const int r = c->stage.reserve(c, o_pl + n * 4 + 16, "registration staging");
    if (r != EF_OK) return r;
    uint8_t* st = c->stage.p;
    d.points = (const float*)(st + o_pts);
    d.normals = q.normals ? (const float*)(st + o_nrm) : nullptr;
    d.row = q.row ? (uint32_t*)(st + o_row) : nullptr;
    d.plane = q.plane ? (float*)(st + o_pl) : nullptr;
    EF_HIP(c, hipMemcpyAsync(st + o_pts, q.points, n * 12, hipMemcpyHostToDevice, c->stream));
    if (q.normals) EF_HIP(c, hipMemcpyAsync(st + o_nrm, q.normals, n * 12, hipMemcpyHostToDevice, c->stream));
  }
  const int r = run(d);
  if (r != EF_OK) return r;
  if (n) {
    if (q.row) EF_HIP(c, hipMemcpyAsync(q.row, d.row, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (q.plane) EF_HIP(c, hipMemcpyAsync(q.plane, d.plane, n * 4, hipMemcpyDeviceToHost, c->stream));
    EF_HIP(c, hipStreamSynchronize(c->stream));
  }
  return EF_OK;
}
}  // namespace
extern "C" {

int ef_default_register_params(ef_ctx* c, ef_register_params* p) {
  if (!c) { g_create_error = "ef_default_register_params: null context"; return EF_EINVAL; }
  if (!p) { c->err = "ef_default_register_params: null params"; return EF_EINVAL; }
  memset(p, 0, sizeof(*p));
  p->max_dist = 0.05f;
  p->min_conf = c->cfg.confidence;
  p->min_normal_cos = 0.5f;
  p->max_iterations = 30;
  p->min_pairs = 32;
  p->stop_translation = 1e-6;
  p->stop_rotation = 1e-6;
  return EF_OK;
}
int ef_register_update(const ef_register_sums* s, const double* T_in, double* T_out, double* xi_out) {
  if (!s || !T_out) { g_create_error = "ef_register_update: null sums or T_out"; return EF_EINVAL; }
  const double* T = T_in ? T_in : REG_IDENTITY;
  if (!finite16(T)) { g_create_error = "ef_register_update: T has a non-finite entry"; return EF_EINVAL; }
  double d[6], xi[6];
  efl::ldlt_pivots<double, 6>(s->A, d);
  bool ok = true;
  for (int i = 0; i < 6; ++i) ok = ok && std::isfinite(d[i]) && d[i] > 0.0;
  if (ok) {
    efl::ldlt_solve<double, 6>(s->A, s->b, xi);
    for (int i = 0; i < 6; ++i) ok = ok && std::isfinite(xi[i]);
  }
  if (!ok) {
    double keep[16];
    memcpy(keep, T, sizeof(keep));
    memcpy(T_out, keep, sizeof(keep));
    if (xi_out) for (int i = 0; i < 6; ++i) xi_out[i] = 0.0;
    return EF_REG_DEGENERATE;
  }
  bool none = true;
  for (int i = 0; i < 6; ++i) none = none && xi[i] == 0.0;
  if (none) {   // exp(0) = I: T as it is, bit for bit (a product with I would turn a -0 entry into +0)
    double keep[16];
    memcpy(keep, T, sizeof(keep));
    memcpy(T_out, keep, sizeof(keep));
    if (xi_out) for (int i = 0; i < 6; ++i) xi_out[i] = 0.0;
    return EF_OK;
  }
  // exp(xi): R = I + a W + b W^2, V = I + b W + c W^2
  const double wx = xi[3], wy = xi[4], wz = xi[5];
  const double th2 = wx * wx + wy * wy + wz * wz, th = std::sqrt(th2);
  double a, b, cc;
  if (th < EF_REGISTER_SMALL_ANGLE) {
    a = 1.0 - th2 / 6.0;
    b = 0.5 - th2 / 24.0;
    cc = 1.0 / 6.0 - th2 / 120.0;
  } else {
    a = std::sin(th) / th;
    b = (1.0 - std::cos(th)) / th2;
    cc = (1.0 - a) / th2;
  }
  const double W[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
  double W2[9], R[9], V[9];
  efl::m3_mul(W, W, W2);
  for (int k = 0; k < 9; ++k) {
    const double id = (k % 4 == 0) ? 1.0 : 0.0;
    R[k] = (id + a * W[k]) + b * W2[k];
    V[k] = (id + b * W[k]) + cc * W2[k];
  }
  double tv[3];
  efl::m3_mulv(V, xi, tv);
  double o[16] = {0};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o[i * 4 + j] = (R[i * 3] * T[j] + R[i * 3 + 1] * T[4 + j]) + R[i * 3 + 2] * T[8 + j];
    o[i * 4 + 3] = ((R[i * 3] * T[3] + R[i * 3 + 1] * T[7]) + R[i * 3 + 2] * T[11]) + tv[i];
  }
  o[15] = 1.0;
  memcpy(T_out, o, sizeof(o));
  if (xi_out) for (int i = 0; i < 6; ++i) xi_out[i] = xi[i];
  return EF_OK;
}
int ef_register_step_dev(ef_ctx* c, const float* points3, const float* normals3, uint32_t n, const ef_register_params* p, const double* T,
                         ef_register_sums* out, uint32_t* row, float* plane) {
  const RegisterCall q{"ef_register_step_dev", points3, normals3, n, p, T, row, plane};
  int r = register_check(c, q, out, "out");
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, q.fn);
  if (r != EF_OK) return r;
  return register_step_run(c, q, T ? T : REG_IDENTITY, out);
}
int ef_register_step(ef_ctx* c, const float* points3, const float* normals3, uint32_t n, const ef_register_params* p, const double* T,
                     ef_register_sums* out, uint32_t* row, float* plane) {
  const RegisterCall q{"ef_register_step", points3, normals3, n, p, T, row, plane};
  int r = register_check(c, q, out, "out");
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, q.fn);
  if (r != EF_OK) return r;
  return register_host(c, q, [&](const RegisterCall& d) { return register_step_run(c, d, T ? T : REG_IDENTITY, out); });
}
int ef_register_cloud_dev(ef_ctx* c, const float* points3, const float* normals3, uint32_t n, const ef_register_params* p, const double* T,
                          double* T_out, ef_register_result* res, uint32_t* row, float* plane) {
  const RegisterCall q{"ef_register_cloud_dev", points3, normals3, n, p, T, row, plane};
  int r = register_check(c, q, T_out, "T_out");
  if (r != EF_OK) return r;
  if (!res) { c->err = "ef_register_cloud_dev: null result"; return EF_EINVAL; }
  DeviceGuard dg_(c);
  r = capture_check(c, q.fn);
  if (r != EF_OK) return r;
  return register_loop(c, q, T_out, res);
}
int ef_register_cloud(ef_ctx* c, const float* points3, const float* normals3, uint32_t n, const ef_register_params* p, const double* T,
                      double* T_out, ef_register_result* res, uint32_t* row, float* plane) {
  const RegisterCall q{"ef_register_cloud", points3, normals3, n, p, T, row, plane};
  int r = register_check(c, q, T_out, "T_out");
  if (r != EF_OK) return r;
  if (!res) { c->err = "ef_register_cloud: null result"; return EF_EINVAL; }
  DeviceGuard dg_(c);
  r = capture_check(c, q.fn);
  if (r != EF_OK) return r;
  return register_host(c, q, [&](const RegisterCall& d) { return register_loop(c, d, T_out, res); });
}

}  // extern "C"
