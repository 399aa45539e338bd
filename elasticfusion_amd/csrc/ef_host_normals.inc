// ================================================================================================
// Estimate normals, curvature and spacing from the map's neighbourhoods (include/ef_hip.h: ef_default_normal_params, ef_map_normals[_dev],
// ef_map_normals_select[_dev], ef_map_reestimate_normals; kernels in ef_normals.inc, the index of ef_host_query.inc, the predicate, the lists
// and the edit frame of ef_host_select.inc; DESIGN.md §8l)
// ================================================================================================
namespace {
static_assert(sizeof(efm::NormalResult) == sizeof(ef_normal_result) && offsetof(efm::NormalResult, participants) == offsetof(ef_normal_result, participants) &&
                  offsetof(efm::NormalResult, listed) == offsetof(ef_normal_result, listed) && EF_NORMALS_KEEP_SIDE == efm::NORMALS_KEEP_SIDE &&
                  EF_NORMALS_VIEWPOINT == efm::NORMALS_VIEWPOINT && EF_NORMAL_NONE == efm::NORMAL_NONE && EF_NORMAL_ESTIMATED == efm::NORMAL_ESTIMATED &&
                  EF_NORMAL_SPARSE == efm::NORMAL_SPARSE && EF_NORMAL_DEGENERATE == efm::NORMAL_DEGENERATE && EF_NORMALS_CURVED == efm::NORMALS_CURVED &&
                  EF_NORMALS_FLAT == efm::NORMALS_FLAT,
              "the kernels' result and constants are the header's");
// refusals before any GPU work: the arguments first, the context last (with a NULL context ef_last_error(NULL) names the argument).  out: the
// call's required output (null out_name: it has none); what < 0: the call lists nothing
int normal_check(ef_ctx* c, const char* fn_, const ef_normal_params* p, const ef_map_selection* among, const void* out, const char* out_name,
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
  if (p->orientation != EF_NORMALS_KEEP_SIDE && p->orientation != EF_NORMALS_VIEWPOINT) {
    err = fn + ": orientation must be EF_NORMALS_KEEP_SIDE or EF_NORMALS_VIEWPOINT";
    return EF_EINVAL;
  }
  if (p->side != 1 && p->side != -1) { err = fn + ": side must be +1 or -1"; return EF_EINVAL; }
  if (p->orientation == EF_NORMALS_VIEWPOINT && !(std::isfinite(p->viewpoint[0]) && std::isfinite(p->viewpoint[1]) && std::isfinite(p->viewpoint[2]))) {
    err = fn + ": the viewpoint has a non-finite coordinate";
    return EF_EINVAL;
  }
  if (std::isnan(p->line_ratio) || p->line_ratio < 0.f) { err = fn + ": line_ratio must not be negative or NaN"; return EF_EINVAL; }
  if (std::isnan(p->max_curvature) || p->max_curvature < 0.f) { err = fn + ": max_curvature must not be negative or NaN"; return EF_EINVAL; }
  if (std::isnan(p->radius_scale) || p->radius_scale < 0.f) { err = fn + ": radius_scale must not be negative or NaN"; return EF_EINVAL; }
  if (what >= 0 && what != EF_NORMAL_ESTIMATED && what != EF_NORMAL_SPARSE && what != EF_NORMAL_DEGENERATE && what != EF_NORMALS_CURVED &&
      what != EF_NORMALS_FLAT) {
    err = fn + ": what must be EF_NORMAL_ESTIMATED, EF_NORMAL_SPARSE, EF_NORMAL_DEGENERATE, EF_NORMALS_CURVED or EF_NORMALS_FLAT";
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
// the normals' own scratch for n rows, carved into a (res, est, stat, status) and part_sc (the selection's counts and offsets; its flags are the
// status bytes, which the join turns from the selection's bytes into the statuses in place)
int normal_scratch(ef_ctx* c, uint32_t n, efm::NormalArgs* a, efm::SelectScratch* part_sc, uint32_t** part_total) {
  if (n > c->normals.rows || !c->normals.scratch.p) {
    const size_t rows = std::min((size_t)c->capacity, (size_t)n + (size_t)n / 4 + 1024);
    c->normals.rows = 0;
    const int r = c->normals.scratch.reserve(c, 64 + rows * (sizeof(float4) + sizeof(uint2)) + Carver::scan_bytes(rows) + rows + 64, "normal scratch");
    if (r != EF_OK) return r;
    c->normals.rows = rows;
  }
  Carver cv(c->normals.scratch);
  a->res = cv.take<efm::NormalResult>(1);
  a->est = cv.take<float4>(c->normals.rows, 16);
  a->stat = cv.take<uint2>(c->normals.rows);
  *part_total = cv.scan_words(c->normals.rows, part_sc);
  part_sc->flags = cv.take<uint8_t>(c->normals.rows);
  a->status = part_sc->flags;
  return EF_OK;
}
// Fills a for the n rows of the map and enqueues the join: a.est, a.stat and a.status of every row.  Waits for the device only where the
// selection's preparation, a grown scratch or an index rebuild do.
int normal_join_enqueue(ef_ctx* c, const char* fn, const ef_normal_params* p, const ef_map_selection* among, uint32_t n, efm::NormalArgs* a) {
  *a = efm::NormalArgs{};
  efm::SelectScratch part_sc;
  uint32_t* part_total = nullptr;
  if (among) {   // the selection's bytes: its own kernel, into the normals' scratch; the join turns them into the status bytes in place
    efm::SelectArgs sa;
    uint32_t n_sel = 0;
    int r = select_prepare(c, among, fn, &sa, &n_sel);
    if (r != EF_OK) return r;
    if (n_sel != n) { c->err = std::string(fn) + ": internal error (the map count changed inside the call)"; return EF_EHIP; }
    r = normal_scratch(c, n, a, &part_sc, &part_total);
    if (r != EF_OK) return r;
    efm::select_flags(sa, part_sc, part_total, c->stream);
    a->part_in = a->status;
  } else {
    const int r = normal_scratch(c, n, a, &part_sc, &part_total);
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
  a->orientation = p->orientation;
  a->side = (float)p->side;
  for (int i = 0; i < 3; ++i) a->view[i] = p->viewpoint[i];
  a->line_ratio = p->line_ratio;
  a->max_curvature = p->max_curvature;
  a->set_radius = p->set_radius;
  a->radius_scale = p->radius_scale;
  efm::normal_join(*a, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// device pointers; enqueues only (but for what normal_join_enqueue needs)
int normal_estimate_enqueue(ef_ctx* c, const char* fn, const ef_normal_params* p, const ef_map_selection* among, float* normals3, float* curvature,
                            float* spacing, uint32_t* count, uint8_t* status, uint32_t max_rows) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::NormalArgs a;
  r = normal_join_enqueue(c, fn, p, among, n, &a);
  if (r != EF_OK) return r;
  efm::normal_split(a, normals3, curvature, spacing, count, status, max_rows, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
int normal_select_enqueue(ef_ctx* c, const char* fn, const ef_normal_params* p, const ef_map_selection* among, int what, uint32_t* rows_dev,
                          uint32_t max_rows, uint32_t* count_dev, ef_normal_result* result_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::SelectScratch sc;
  uint32_t* total = nullptr;
  r = select_scratch(c, n, &sc, &total);
  if (r != EF_OK) return r;
  efm::NormalArgs a;
  r = normal_join_enqueue(c, fn, p, among, n, &a);
  if (r != EF_OK) return r;
  efm::normal_flags(a, what, sc.flags, c->stream);
  efm::flags_count(sc, n, 0u, count_dev, c->stream);
  efm::select_rows(sc, n, rows_dev, max_rows, c->stream);
  efm::normal_tally(a, count_dev, (efm::NormalResult*)result_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
}  // namespace

extern "C" {

int ef_default_normal_params(ef_ctx* c, ef_normal_params* p) {
  if (!c) { g_create_error = "ef_default_normal_params: null context"; return EF_EINVAL; }
  if (!p) { c->err = "ef_default_normal_params: null params"; return EF_EINVAL; }
  memset(p, 0, sizeof(*p));
  p->radius = 0.03f;
  p->cell = 0.03f;   // = radius: the outlier filter's measured choice for the same walk (DESIGN.md §8i)
  p->min_conf = -1.0f;
  p->k = 12;
  p->min_neighbors = 5;
  p->orientation = EF_NORMALS_KEEP_SIDE;
  p->side = -1;
  p->line_ratio = 1e-4f;
  p->max_curvature = 0.05f;
  p->set_radius = 0;
  p->radius_scale = 1.0f;
  return EF_OK;
}

int ef_map_normals_dev(ef_ctx* c, const ef_normal_params* p, const ef_map_selection* among, float* normals3_dev, float* curvature_dev,
                       float* spacing_dev, uint32_t* count_dev, uint8_t* status_dev, uint32_t max_rows) {
  int r = normal_check(c, "ef_map_normals_dev", p, among, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_normals_dev");
  if (r != EF_OK) return r;
  return normal_estimate_enqueue(c, "ef_map_normals_dev", p, among, normals3_dev, curvature_dev, spacing_dev, count_dev, status_dev, max_rows);
}
int ef_map_normals(ef_ctx* c, const ef_normal_params* p, const ef_map_selection* among, float* normals3, float* curvature, float* spacing,
                   uint32_t* count, uint8_t* status, uint32_t max_rows) {
  int r = normal_check(c, "ef_map_normals", p, among, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_normals");
  if (r != EF_OK) return r;
  uint32_t n = 0;
  r = select_count(c, &n);
  if (r != EF_OK) return r;
  const size_t rows = std::min((size_t)max_rows, (size_t)n);
  r = c->stage.reserve(c, 16 + rows * 25, "normal staging");   // 12 + 4 + 4 + 4 + 1 bytes per row
  if (r != EF_OK) return r;
  float* d_nrm = c->stage.as<float>();
  float* d_curv = d_nrm + rows * 3;
  float* d_space = d_curv + rows;
  uint32_t* d_count = (uint32_t*)(d_space + rows);
  uint8_t* d_status = (uint8_t*)(d_count + rows);
  r = normal_estimate_enqueue(c, "ef_map_normals", p, among, normals3 ? d_nrm : nullptr, curvature ? d_curv : nullptr, spacing ? d_space : nullptr,
                              count ? d_count : nullptr, status ? d_status : nullptr, (uint32_t)rows);
  if (r != EF_OK) return r;
  if (rows && normals3) EF_HIP(c, hipMemcpyAsync(normals3, d_nrm, rows * 12, hipMemcpyDeviceToHost, c->stream));
  if (rows && curvature) EF_HIP(c, hipMemcpyAsync(curvature, d_curv, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && spacing) EF_HIP(c, hipMemcpyAsync(spacing, d_space, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && count) EF_HIP(c, hipMemcpyAsync(count, d_count, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && status) EF_HIP(c, hipMemcpyAsync(status, d_status, rows, hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}

int ef_map_normals_select_dev(ef_ctx* c, const ef_normal_params* p, const ef_map_selection* among, int what, uint32_t* rows_dev, uint32_t max_rows,
                              uint32_t* count_dev, ef_normal_result* result_dev) {
  int r = normal_check(c, "ef_map_normals_select_dev", p, among, count_dev, "count", what < 0 ? 0 : what, rows_dev, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_normals_select_dev");
  if (r != EF_OK) return r;
  return normal_select_enqueue(c, "ef_map_normals_select_dev", p, among, what, rows_dev, max_rows, count_dev, result_dev);
}
int ef_map_normals_select(ef_ctx* c, const ef_normal_params* p, const ef_map_selection* among, int what, uint32_t* rows, uint32_t max_rows,
                          uint32_t* count, ef_normal_result* result) {
  int r = normal_check(c, "ef_map_normals_select", p, among, count, "count", what < 0 ? 0 : what, rows, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_normals_select");
  if (r != EF_OK) return r;
  r = rows_list_host(c, "normal staging", rows, max_rows, count, [&](uint32_t* d_rows, uint32_t cap_rows, uint32_t* d_count) {
    return normal_select_enqueue(c, "ef_map_normals_select", p, among, what, d_rows, cap_rows, d_count, nullptr);
  });
  if (r != EF_OK) return r;
  if (result) {   // (as the kernels left it at the head of the normals' scratch; rows_list_host has synchronised behind them)
    EF_HIP(c, hipMemcpyAsync(result, c->normals.scratch.p, sizeof(*result), hipMemcpyDeviceToHost, c->stream));
    EF_HIP(c, hipStreamSynchronize(c->stream));
  }
  return EF_OK;
}

int ef_map_reestimate_normals(ef_ctx* c, const ef_normal_params* p, const ef_map_selection* among, ef_normal_result* res) {
  const char* fn = "ef_map_reestimate_normals";
  int r = normal_check(c, fn, p, among, res, "result");
  if (r != EF_OK) return r;
  memset(res, 0, sizeof(*res));
  DeviceGuard dg_(c);
  // inside the edit frame of ef_host_select.inc, as the fuse's in-place merge is (append_run)
  uint32_t n = 0;
  r = edit_begin(c, fn, &n);
  if (r != EF_OK) return r;
  efm::NormalArgs a;
  r = normal_join_enqueue(c, fn, p, among, n, &a);   // the estimates into the scratch, by row: nothing of the map is written
  if (r != EF_OK) return r;
  efm::normal_tally(a, nullptr, nullptr, c->stream);
  EF_HIP(c, hipGetLastError());
  // every count is known before anything is written
  EF_HIP(c, hipMemcpyAsync(res, a.res, sizeof(*res), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  if ((uint64_t)res->estimated + res->sparse + res->degenerate != res->participants || res->participants > n || res->flipped > res->estimated) {
    c->err = std::string(fn) + ": internal error (the status counts do not add up)";
    return EF_EHIP;
  }
  res->listed = res->estimated;   // the rows written
  ++c->map_gen;   // the index of the queries is stale by the edit frame's rule (the positions, and with them its contents, are unchanged)
  if (res->estimated) {
    // the write goes to rows of maps[cur]; pending z-buffer keys name rows of maps[im_map]: append_run's condition and its reason
    if (c->im_pending && c->im_map == c->cur) im_materialise(c);
    efm::normal_apply(a, c->stream);
    EF_HIP(c, hipGetLastError());
  }
  return edit_commit(c, n, /*labels_restart=*/false);
}

}  // extern "C"
