// ================================================================================================
// Smooth the map's positions by moving least squares (include/ef_hip.h: ef_default_smooth_params, ef_map_smooth[_dev],
// ef_map_smooth_select[_dev], ef_map_smooth_apply; kernels in ef_smooth.inc, the index of ef_host_query.inc, the predicate, the lists and the
// edit frame of ef_host_select.inc; DESIGN.md §8n)
// ================================================================================================
namespace {
static_assert(sizeof(efm::SmoothResult) == sizeof(ef_smooth_result) && sizeof(ef_smooth_result) == 8 * sizeof(uint32_t) &&
                  offsetof(efm::SmoothResult, participants) == offsetof(ef_smooth_result, participants) &&
                  offsetof(efm::SmoothResult, moved) == offsetof(ef_smooth_result, moved) &&
                  offsetof(efm::SmoothResult, listed) == offsetof(ef_smooth_result, listed) &&
                  offsetof(efm::SmoothResult, largest_shift) == offsetof(ef_smooth_result, largest_shift) && EF_SMOOTH_UNIFORM == efm::SMOOTH_UNIFORM &&
                  EF_SMOOTH_COMPACT == efm::SMOOTH_COMPACT && EF_SMOOTH_NONE == efm::SMOOTH_NONE && EF_SMOOTH_SMOOTHED == efm::SMOOTH_SMOOTHED &&
                  EF_SMOOTH_SPARSE == efm::SMOOTH_SPARSE && EF_SMOOTH_DEGENERATE == efm::SMOOTH_DEGENERATE && EF_SMOOTH_CLAMPED == efm::SMOOTH_CLAMPED &&
                  EF_SMOOTH_SHIFTED == efm::SMOOTH_SHIFTED,
              "the kernels' result and constants are the header's");
// refusals before any GPU work: the arguments first, the context last (with a NULL context ef_last_error(NULL) names the argument).  out: the
// call's required output (null out_name: it has none); what < 0: the call lists nothing
int smooth_check(ef_ctx* c, const char* fn_, const ef_smooth_params* p, const ef_map_selection* among, const void* out, const char* out_name,
                 int what = -1, const void* rows = nullptr, uint32_t max_rows = 0) {
  std::string& err = c ? c->err : g_create_error;
  const std::string fn = fn_;
  if (!p) { err = fn + ": null params"; return EF_EINVAL; }
  if (out_name && !out) { err = fn + ": null " + out_name; return EF_EINVAL; }
  if (!(p->radius > 0.f) || !std::isfinite(p->radius)) { err = fn + ": radius must be finite and positive"; return EF_EINVAL; }
  if (!(p->cell > 0.f) || !std::isfinite(p->cell) || !std::isfinite(1.0f / p->cell)) { err = fn + ": cell must be finite and positive"; return EF_EINVAL; }
  if (!(p->radius / p->cell <= (float)EF_QUERY_MAX_RATIO)) {
    err = fn + ": radius / cell must not exceed " + std::to_string(EF_QUERY_MAX_RATIO);
    return EF_EINVAL;
  }
  if (std::isnan(p->min_conf)) { err = fn + ": min_conf is NaN"; return EF_EINVAL; }
  if (p->k < 3 || p->k > 16) { err = fn + ": k must lie in 3 .. 16"; return EF_EINVAL; }
  if (p->min_neighbors < 2 || p->min_neighbors > p->k) { err = fn + ": min_neighbors must lie in 2 .. k"; return EF_EINVAL; }
  if (p->iterations < 1 || p->iterations > 16) { err = fn + ": iterations must lie in 1 .. 16"; return EF_EINVAL; }
  if (p->weighting != EF_SMOOTH_UNIFORM && p->weighting != EF_SMOOTH_COMPACT) {
    err = fn + ": weighting must be EF_SMOOTH_UNIFORM or EF_SMOOTH_COMPACT";
    return EF_EINVAL;
  }
  if (p->normal_gate != 0 && p->normal_gate != 1) { err = fn + ": normal_gate must be 0 or 1"; return EF_EINVAL; }
  if (std::isnan(p->min_normal_cos)) { err = fn + ": min_normal_cos is NaN"; return EF_EINVAL; }
  if (!(p->strength > 0.f && p->strength <= 1.f)) { err = fn + ": strength must lie in (0, 1]"; return EF_EINVAL; }
  if (!(p->max_shift > 0.f)) { err = fn + ": max_shift must be positive (+inf: no bound)"; return EF_EINVAL; }
  if (std::isnan(p->line_ratio) || p->line_ratio < 0.f) { err = fn + ": line_ratio must not be negative or NaN"; return EF_EINVAL; }
  if (std::isnan(p->shift_threshold) || p->shift_threshold < 0.f) { err = fn + ": shift_threshold must not be negative or NaN"; return EF_EINVAL; }
  if (what >= 0 && what != EF_SMOOTH_SMOOTHED && what != EF_SMOOTH_SPARSE && what != EF_SMOOTH_DEGENERATE && what != EF_SMOOTH_CLAMPED &&
      what != EF_SMOOTH_SHIFTED) {
    err = fn + ": what must be EF_SMOOTH_SMOOTHED, EF_SMOOTH_SPARSE, EF_SMOOTH_DEGENERATE, EF_SMOOTH_CLAMPED or EF_SMOOTH_SHIFTED";
    return EF_EINVAL;
  }
  if (max_rows && !rows) return select_null(c, fn_, "rows");
  if (among) {
    const int r = select_check(c, among, fn_);
    if (r != EF_OK) return r;
  }
  if (!c) return select_null(c, fn_, "context");
  return EF_OK;
}
// the smoothing's own scratch for n rows and the list slots of k, carved into a (res, the two position buffers, est, nbr, count, shift, status) and
// part_sc (the selection's counts and offsets; its flags are the status bytes, which the neighbours' kernel turns from the selection's bytes
// into the statuses in place).  A failed reservation leaves the scratch as "none": the next call reserves again
int smooth_scratch(ef_ctx* c, uint32_t n, int k, efm::SmoothArgs* a, efm::SelectScratch* part_sc, uint32_t** part_total) {
  const int slots = k <= 4 ? 4 : k <= 8 ? 8 : 16;
  if (n > c->smooth.rows || slots > c->smooth.slots || !c->smooth.scratch.p) {
    const size_t rows = std::max(c->smooth.rows, std::min((size_t)c->capacity, (size_t)n + (size_t)n / 4 + 1024));
    const int keep = std::max(slots, c->smooth.slots);
    c->smooth.rows = 0;
    c->smooth.slots = 0;
    const int r = c->smooth.scratch.reserve(c, 64 + rows * (3 * sizeof(float4) + ((size_t)keep + 2) * sizeof(uint32_t)) + Carver::scan_bytes(rows) + rows + 128,
                                            "smooth scratch");
    if (r != EF_OK) return r;
    c->smooth.rows = rows;
    c->smooth.slots = keep;
  }
  const size_t rows = c->smooth.rows;
  Carver cv(c->smooth.scratch);
  a->res = cv.take<efm::SmoothResult>(1);
  a->buf[0] = cv.take<float4>(rows, 16);
  a->buf[1] = cv.take<float4>(rows);
  a->est = cv.take<float4>(rows);
  a->nbr = cv.take<uint32_t>(rows * (size_t)c->smooth.slots);
  a->stride = (unsigned)rows;
  a->count = cv.take<uint32_t>(rows);
  a->shift = cv.take<float>(rows);
  *part_total = cv.scan_words(rows, part_sc);
  part_sc->flags = cv.take<uint8_t>(rows);
  a->status = part_sc->flags;
  return EF_OK;
}
// Fills a for the n rows of the map and enqueues the neighbours, the iterations and the finish: count, status, est and shift of every row and the
// last position buffer (efm::smooth_final).  Waits for the device only where the selection's preparation, a grown scratch or an index rebuild do.
int smooth_enqueue(ef_ctx* c, const char* fn, const ef_smooth_params* p, const ef_map_selection* among, uint32_t n, efm::SmoothArgs* a) {
  *a = efm::SmoothArgs{};
  efm::SelectScratch part_sc;
  uint32_t* part_total = nullptr;
  if (among) {   // the selection's bytes: its own kernel, into the smoothing's scratch; the neighbours' kernel turns them into the status bytes in place
    efm::SelectArgs sa;
    uint32_t n_sel = 0;
    int r = select_prepare(c, among, fn, &sa, &n_sel);
    if (r != EF_OK) return r;
    if (n_sel != n) { c->err = std::string(fn) + ": internal error (the map count changed inside the call)"; return EF_EHIP; }
    r = smooth_scratch(c, n, p->k, a, &part_sc, &part_total);
    if (r != EF_OK) return r;
    efm::select_flags(sa, part_sc, part_total, c->stream);
    a->part_in = a->status;
  } else {
    const int r = smooth_scratch(c, n, p->k, a, &part_sc, &part_total);
    if (r != EF_OK) return r;
  }
  const int r = query_index(c, p->cell);
  if (r != EF_OK) return r;
  if (c->query.n != n) { c->err = std::string(fn) + ": internal error (the index does not cover the map)"; return EF_EHIP; }
  query_index_args(c, &a->q);
  a->q.max_dist = p->radius;
  a->q.r2 = p->radius * p->radius;
  a->q.min_conf = p->min_conf;
  a->n = n;
  a->k = p->k;
  a->min_neighbors = (uint32_t)p->min_neighbors;
  a->iterations = p->iterations;
  a->weighting = p->weighting;
  a->gate = p->normal_gate;
  a->min_normal_cos = p->min_normal_cos;
  a->strength = p->strength;
  a->max_shift = p->max_shift;
  a->line_ratio = p->line_ratio;
  a->shift_threshold = p->shift_threshold;
  a->set_normal = p->set_normal;
  efm::smooth_neighbours(*a, c->stream);
  for (int i = 1; i <= p->iterations; ++i) efm::smooth_step(*a, i, c->stream);
  efm::smooth_finish(*a, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// device pointers; enqueues only (but for what smooth_enqueue needs)
int smooth_rows_enqueue(ef_ctx* c, const char* fn, const ef_smooth_params* p, const ef_map_selection* among, float* position3, float* normal3,
                        float* curvature, float* shift, uint32_t* count, uint8_t* status, uint32_t max_rows, ef_smooth_result* result_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::SmoothArgs a;
  r = smooth_enqueue(c, fn, p, among, n, &a);
  if (r != EF_OK) return r;
  efm::smooth_split(a, position3, normal3, curvature, shift, count, status, max_rows, c->stream);
  efm::smooth_tally(a, nullptr, (efm::SmoothResult*)result_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
int smooth_select_enqueue(ef_ctx* c, const char* fn, const ef_smooth_params* p, const ef_map_selection* among, int what, uint32_t* rows_dev,
                          uint32_t max_rows, uint32_t* count_dev, ef_smooth_result* result_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::SelectScratch sc;
  uint32_t* total = nullptr;
  r = select_scratch(c, n, &sc, &total);
  if (r != EF_OK) return r;
  efm::SmoothArgs a;
  r = smooth_enqueue(c, fn, p, among, n, &a);
  if (r != EF_OK) return r;
  efm::smooth_flags(a, what, sc.flags, c->stream);
  efm::flags_count(sc, n, 0u, count_dev, c->stream);
  efm::select_rows(sc, n, rows_dev, max_rows, c->stream);
  efm::smooth_tally(a, count_dev, (efm::SmoothResult*)result_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// the call's result, as the kernels left it at the head of the smoothing's scratch (synchronises)
int smooth_result_host(ef_ctx* c, ef_smooth_result* res_or_null) {
  if (res_or_null) EF_HIP(c, hipMemcpyAsync(res_or_null, c->smooth.scratch.p, sizeof(*res_or_null), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}
}  // namespace

extern "C" {

int ef_default_smooth_params(ef_ctx* c, ef_smooth_params* p) {
  if (!c) { g_create_error = "ef_default_smooth_params: null context"; return EF_EINVAL; }
  if (!p) { c->err = "ef_default_smooth_params: null params"; return EF_EINVAL; }
  memset(p, 0, sizeof(*p));
  p->radius = 0.03f;
  p->cell = 0.03f;   // = radius, as the normals'
  p->min_conf = -1.0f;
  p->k = 12;
  p->min_neighbors = 5;
  p->iterations = 1;
  p->weighting = EF_SMOOTH_COMPACT;
  p->normal_gate = 0;
  p->min_normal_cos = 0.9f;
  p->strength = 1.0f;
  p->max_shift = p->radius;
  p->line_ratio = 1e-4f;
  p->set_normal = 0;
  p->shift_threshold = 0.0f;
  return EF_OK;
}

int ef_map_smooth_dev(ef_ctx* c, const ef_smooth_params* p, const ef_map_selection* among, float* position3_dev, float* normal3_dev,
                      float* curvature_dev, float* shift_dev, uint32_t* count_dev, uint8_t* status_dev, uint32_t max_rows,
                      ef_smooth_result* result_dev) {
  int r = smooth_check(c, "ef_map_smooth_dev", p, among, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_smooth_dev");
  if (r != EF_OK) return r;
  return smooth_rows_enqueue(c, "ef_map_smooth_dev", p, among, position3_dev, normal3_dev, curvature_dev, shift_dev, count_dev, status_dev, max_rows,
                             result_dev);
}
int ef_map_smooth(ef_ctx* c, const ef_smooth_params* p, const ef_map_selection* among, float* position3, float* normal3, float* curvature,
                  float* shift, uint32_t* count, uint8_t* status, uint32_t max_rows, ef_smooth_result* result) {
  int r = smooth_check(c, "ef_map_smooth", p, among, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_smooth");
  if (r != EF_OK) return r;
  uint32_t n = 0;
  r = select_count(c, &n);
  if (r != EF_OK) return r;
  const size_t rows = std::min((size_t)max_rows, (size_t)n);
  r = c->stage.reserve(c, 16 + rows * 37, "smooth staging");   // 12 + 12 + 4 + 4 + 4 + 1 bytes per row
  if (r != EF_OK) return r;
  float* d_pos = c->stage.as<float>();
  float* d_nrm = d_pos + rows * 3;
  float* d_curv = d_nrm + rows * 3;
  float* d_shift = d_curv + rows;
  uint32_t* d_count = (uint32_t*)(d_shift + rows);
  uint8_t* d_status = (uint8_t*)(d_count + rows);
  r = smooth_rows_enqueue(c, "ef_map_smooth", p, among, position3 ? d_pos : nullptr, normal3 ? d_nrm : nullptr, curvature ? d_curv : nullptr,
                          shift ? d_shift : nullptr, count ? d_count : nullptr, status ? d_status : nullptr, (uint32_t)rows, nullptr);
  if (r != EF_OK) return r;
  if (rows && position3) EF_HIP(c, hipMemcpyAsync(position3, d_pos, rows * 12, hipMemcpyDeviceToHost, c->stream));
  if (rows && normal3) EF_HIP(c, hipMemcpyAsync(normal3, d_nrm, rows * 12, hipMemcpyDeviceToHost, c->stream));
  if (rows && curvature) EF_HIP(c, hipMemcpyAsync(curvature, d_curv, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && shift) EF_HIP(c, hipMemcpyAsync(shift, d_shift, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && count) EF_HIP(c, hipMemcpyAsync(count, d_count, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && status) EF_HIP(c, hipMemcpyAsync(status, d_status, rows, hipMemcpyDeviceToHost, c->stream));
  return smooth_result_host(c, result);
}

int ef_map_smooth_select_dev(ef_ctx* c, const ef_smooth_params* p, const ef_map_selection* among, int what, uint32_t* rows_dev, uint32_t max_rows,
                             uint32_t* count_dev, ef_smooth_result* result_dev) {
  int r = smooth_check(c, "ef_map_smooth_select_dev", p, among, count_dev, "count", what < 0 ? 0 : what, rows_dev, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_smooth_select_dev");
  if (r != EF_OK) return r;
  return smooth_select_enqueue(c, "ef_map_smooth_select_dev", p, among, what, rows_dev, max_rows, count_dev, result_dev);
}
int ef_map_smooth_select(ef_ctx* c, const ef_smooth_params* p, const ef_map_selection* among, int what, uint32_t* rows, uint32_t max_rows,
                         uint32_t* count, ef_smooth_result* result) {
  int r = smooth_check(c, "ef_map_smooth_select", p, among, count, "count", what < 0 ? 0 : what, rows, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_smooth_select");
  if (r != EF_OK) return r;
  r = rows_list_host(c, "smooth staging", rows, max_rows, count, [&](uint32_t* d_rows, uint32_t cap_rows, uint32_t* d_count) {
    return smooth_select_enqueue(c, "ef_map_smooth_select", p, among, what, d_rows, cap_rows, d_count, nullptr);
  });
  if (r != EF_OK) return r;
  return result ? smooth_result_host(c, result) : (int)EF_OK;   // (rows_list_host has synchronised behind the kernels)
}

int ef_map_smooth_apply(ef_ctx* c, const ef_smooth_params* p, const ef_map_selection* among, ef_smooth_result* res) {
  const char* fn = "ef_map_smooth_apply";
  int r = smooth_check(c, fn, p, among, res, "result");
  if (r != EF_OK) return r;
  memset(res, 0, sizeof(*res));
  DeviceGuard dg_(c);
  // inside the edit frame of ef_host_select.inc, as the normals' write-back is
  uint32_t n = 0;
  r = edit_begin(c, fn, &n);
  if (r != EF_OK) return r;
  efm::SmoothArgs a;
  r = smooth_enqueue(c, fn, p, among, n, &a);   // the moved positions into the scratch: nothing of the map is written
  if (r != EF_OK) return r;
  efm::smooth_tally(a, nullptr, nullptr, c->stream);
  EF_HIP(c, hipGetLastError());
  // every count is known before anything is written
  EF_HIP(c, hipMemcpyAsync(res, a.res, sizeof(*res), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  if ((uint64_t)res->smoothed + res->sparse + res->degenerate != res->participants || res->participants > n || res->moved > res->participants ||
      res->clamped > res->participants) {
    c->err = std::string(fn) + ": internal error (the status counts do not add up)";
    memset(res, 0, sizeof(*res));
    return EF_EHIP;
  }
  res->listed = res->moved;   // the rows whose position changed
  ++c->map_gen;   // the index of the queries is stale: positions move
  if (res->participants) {
    // the write goes to rows of maps[cur]; pending z-buffer keys name rows of maps[im_map]: append_run's condition and its reason
    if (c->im_pending && c->im_map == c->cur) im_materialise(c);
    efm::smooth_apply(a, c->stream);
    EF_HIP(c, hipGetLastError());
  }
  return edit_commit(c, n, /*labels_restart=*/false);
}

}  // extern "C"
