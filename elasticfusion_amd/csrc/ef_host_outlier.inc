// ================================================================================================
// Remove outlier surfels: neighbourhood statistics of the map (include/ef_hip.h: ef_default_outlier_params, ef_map_neighbor_stats[_dev],
// ef_map_outliers_select[_dev], ef_map_remove_outliers; kernels in ef_outlier.inc, the index of ef_host_query.inc, the predicate, the lists and
// the erase of ef_host_select.inc; DESIGN.md §8i)
// ================================================================================================
namespace {
static_assert(sizeof(efm::OutlierResult) == sizeof(ef_outlier_result) && offsetof(efm::OutlierResult, participants) == offsetof(ef_outlier_result, participants) &&
                  offsetof(efm::OutlierResult, threshold) == offsetof(ef_outlier_result, threshold) && EF_OUTLIER_SUM_LANES == efm::OUTLIER_SUM_LANES &&
                  EF_OUTLIER_RADIUS == efm::OUTLIER_RADIUS && EF_OUTLIER_STATISTICAL == efm::OUTLIER_STATISTICAL,
              "the kernels' result and constants are the header's");
// refusals before any GPU work: the arguments first, the context last (with a NULL context ef_last_error(NULL) names the argument).  out: the
// call's required output (null out_name: it has none)
int outlier_check(ef_ctx* c, const char* fn_, const ef_outlier_params* p, const ef_map_selection* among, const void* out, const char* out_name,
                  const void* rows = nullptr, uint32_t max_rows = 0) {
  std::string& err = c ? c->err : g_create_error;
  const std::string fn = fn_;
  if (!p) { err = fn + ": null params"; return EF_EINVAL; }
  if (out_name && !out) { err = fn + ": null " + out_name; return EF_EINVAL; }
  if (p->mode != EF_OUTLIER_RADIUS && p->mode != EF_OUTLIER_STATISTICAL) { err = fn + ": mode must be one of EF_OUTLIER_*"; return EF_EINVAL; }
  if (!(p->radius > 0.f) || !std::isfinite(p->radius)) { err = fn + ": radius must be finite and positive"; return EF_EINVAL; }
  if (!(p->cell > 0.f) || !std::isfinite(p->cell) || !std::isfinite(1.0f / p->cell)) { err = fn + ": cell must be finite and positive"; return EF_EINVAL; }
  if (!(p->radius / p->cell <= (float)EF_QUERY_MAX_RATIO)) {
    err = fn + ": radius / cell must not exceed " + std::to_string(EF_QUERY_MAX_RATIO);
    return EF_EINVAL;
  }
  if (std::isnan(p->min_conf)) { err = fn + ": min_conf is NaN"; return EF_EINVAL; }
  if (p->mode == EF_OUTLIER_STATISTICAL && (p->k < 1 || p->k > 16)) { err = fn + ": k must lie in 1 .. 16"; return EF_EINVAL; }
  if (p->min_neighbors < 0) { err = fn + ": min_neighbors must not be negative"; return EF_EINVAL; }
  if (std::isnan(p->std_ratio) || p->std_ratio < 0.f) { err = fn + ": std_ratio must not be negative or NaN"; return EF_EINVAL; }
  if (std::isnan(p->max_mean_dist) || p->max_mean_dist < 0.f) { err = fn + ": max_mean_dist must not be negative or NaN"; return EF_EINVAL; }
  if (max_rows && !rows) return select_null(c, fn_, "rows");
  if (among) {
    const int r = select_check(c, among, fn_);
    if (r != EF_OK) return r;
  }
  if (!c) return select_null(c, fn_, "context");
  return EF_OK;
}
// the outliers' own scratch for n rows, carved into a (res, partial, tally, stat, part) and part_sc (the selection's counts and offsets)
int outlier_scratch(ef_ctx* c, uint32_t n, efm::OutlierArgs* a, efm::SelectScratch* part_sc, uint32_t** part_total) {
  const size_t P = EF_OUTLIER_SUM_LANES;
  if (n > c->outlier.rows || !c->outlier.scratch.p) {
    const size_t rows = std::min((size_t)c->capacity, (size_t)n + (size_t)n / 4 + 1024);
    c->outlier.rows = 0;
    const int r = c->outlier.scratch.reserve(c, 64 + P * (2 * sizeof(double) + 3 * sizeof(uint32_t)) + rows * sizeof(uint2) + Carver::scan_bytes(rows) + rows + 64,
                                             "outlier scratch");
    if (r != EF_OK) return r;
    c->outlier.rows = rows;
  }
  Carver cv(c->outlier.scratch);
  a->res = cv.take<efm::OutlierResult>(1);
  a->partial = cv.take<double>(2 * P);
  a->tally = cv.take<uint32_t>(3 * P);
  a->stat = cv.take<uint2>(c->outlier.rows);
  *part_total = cv.scan_words(c->outlier.rows, part_sc);
  part_sc->flags = cv.take<uint8_t>(c->outlier.rows);
  a->part = part_sc->flags;
  return EF_OK;
}
// Fills a for the n rows of the map and enqueues the join: a.stat and a.part of every row.  Waits for the device only where the selection's
// preparation, a grown scratch or an index rebuild do.
int outlier_join_enqueue(ef_ctx* c, const char* fn, const ef_outlier_params* p, const ef_map_selection* among, uint32_t n, efm::OutlierArgs* a) {
  *a = efm::OutlierArgs{};
  efm::SelectScratch part_sc;
  uint32_t* part_total = nullptr;
  if (among) {   // the selection's bytes: its own kernel, into the outliers' scratch; the join turns them into the participant bytes in place
    efm::SelectArgs sa;
    uint32_t n_sel = 0;
    int r = select_prepare(c, among, fn, &sa, &n_sel);
    if (r != EF_OK) return r;
    if (n_sel != n) { c->err = std::string(fn) + ": internal error (the map count changed inside the call)"; return EF_EHIP; }
    r = outlier_scratch(c, n, a, &part_sc, &part_total);
    if (r != EF_OK) return r;
    efm::select_flags(sa, part_sc, part_total, c->stream);
    a->part_in = a->part;
  } else {
    const int r = outlier_scratch(c, n, a, &part_sc, &part_total);
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
  a->mode = p->mode;
  a->k = p->mode == EF_OUTLIER_STATISTICAL ? p->k : 1;
  a->min_neighbors = (uint32_t)p->min_neighbors;
  a->flag_sparse = p->flag_sparse;
  a->std_ratio = p->std_ratio;
  a->max_mean_dist = p->max_mean_dist;
  efm::outlier_join(*a, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// the join, the sums and the threshold, then flags[row] = 1 for every outlier
int outlier_mark(ef_ctx* c, const char* fn, const ef_outlier_params* p, const ef_map_selection* among, uint32_t n, uint8_t* flags, efm::OutlierArgs* a) {
  const int r = outlier_join_enqueue(c, fn, p, among, n, a);
  if (r != EF_OK) return r;
  efm::outlier_reduce(*a, c->stream);
  efm::outlier_flags(*a, flags, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// device pointers; enqueues only (but for what outlier_join_enqueue needs)
int outlier_stats_enqueue(ef_ctx* c, const char* fn, const ef_outlier_params* p, const ef_map_selection* among, float* mean_dev, uint32_t* count_dev,
                          uint32_t max_rows) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::OutlierArgs a;
  r = outlier_join_enqueue(c, fn, p, among, n, &a);
  if (r != EF_OK) return r;
  efm::outlier_split(a, mean_dev, count_dev, max_rows, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
int outlier_select_enqueue(ef_ctx* c, const char* fn, const ef_outlier_params* p, const ef_map_selection* among, uint32_t* rows_dev, uint32_t max_rows,
                           uint32_t* count_dev, ef_outlier_result* result_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::SelectScratch sc;
  uint32_t* total = nullptr;
  r = select_scratch(c, n, &sc, &total);
  if (r != EF_OK) return r;
  efm::OutlierArgs a;
  r = outlier_mark(c, fn, p, among, n, sc.flags, &a);
  if (r != EF_OK) return r;
  efm::flags_count(sc, n, 0u, count_dev, c->stream);
  efm::select_rows(sc, n, rows_dev, max_rows, c->stream);
  efm::outlier_tally(a, count_dev, (efm::OutlierResult*)result_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// the call's result, as the kernels left it at the head of the outliers' scratch (after a synchronise behind them)
int outlier_result_host(ef_ctx* c, ef_outlier_result* res) {
  EF_HIP(c, hipMemcpyAsync(res, c->outlier.scratch.p, sizeof(*res), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}
}  // namespace

extern "C" {

int ef_default_outlier_params(ef_ctx* c, ef_outlier_params* p) {
  if (!c) { g_create_error = "ef_default_outlier_params: null context"; return EF_EINVAL; }
  if (!p) { c->err = "ef_default_outlier_params: null params"; return EF_EINVAL; }
  memset(p, 0, sizeof(*p));
  p->mode = EF_OUTLIER_STATISTICAL;
  p->radius = 0.03f;
  p->cell = 0.03f;   // = radius: chosen by measurement among radius / 2, radius and 2 radius (DESIGN.md §8i)
  p->min_conf = -1.0f;
  p->min_neighbors = 4;
  p->k = 8;
  p->std_ratio = 2.0f;
  p->max_mean_dist = 0.0f;
  p->flag_sparse = 1;
  return EF_OK;
}

int ef_map_neighbor_stats_dev(ef_ctx* c, const ef_outlier_params* p, const ef_map_selection* among, float* mean_dev, uint32_t* count_dev,
                              uint32_t max_rows) {
  int r = outlier_check(c, "ef_map_neighbor_stats_dev", p, among, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_neighbor_stats_dev");
  if (r != EF_OK) return r;
  return outlier_stats_enqueue(c, "ef_map_neighbor_stats_dev", p, among, mean_dev, count_dev, max_rows);
}
int ef_map_neighbor_stats(ef_ctx* c, const ef_outlier_params* p, const ef_map_selection* among, float* mean, uint32_t* count, uint32_t max_rows) {
  int r = outlier_check(c, "ef_map_neighbor_stats", p, among, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_neighbor_stats");
  if (r != EF_OK) return r;
  uint32_t n = 0;
  r = select_count(c, &n);
  if (r != EF_OK) return r;
  const size_t rows = std::min((size_t)max_rows, (size_t)n);
  r = c->stage.reserve(c, 16 + rows * 8, "outlier staging");
  if (r != EF_OK) return r;
  float* d_mean = c->stage.as<float>();
  uint32_t* d_count = (uint32_t*)(c->stage.p + rows * 4);
  r = outlier_stats_enqueue(c, "ef_map_neighbor_stats", p, among, mean ? d_mean : nullptr, count ? d_count : nullptr, (uint32_t)rows);
  if (r != EF_OK) return r;
  if (rows && mean) EF_HIP(c, hipMemcpyAsync(mean, d_mean, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && count) EF_HIP(c, hipMemcpyAsync(count, d_count, rows * 4, hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}

int ef_map_outliers_select_dev(ef_ctx* c, const ef_outlier_params* p, const ef_map_selection* among, uint32_t* rows_dev, uint32_t max_rows,
                               uint32_t* count_dev, ef_outlier_result* result_dev) {
  int r = outlier_check(c, "ef_map_outliers_select_dev", p, among, count_dev, "count", rows_dev, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_outliers_select_dev");
  if (r != EF_OK) return r;
  return outlier_select_enqueue(c, "ef_map_outliers_select_dev", p, among, rows_dev, max_rows, count_dev, result_dev);
}
int ef_map_outliers_select(ef_ctx* c, const ef_outlier_params* p, const ef_map_selection* among, uint32_t* rows, uint32_t max_rows, uint32_t* count,
                           ef_outlier_result* result) {
  int r = outlier_check(c, "ef_map_outliers_select", p, among, count, "count", rows, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_outliers_select");
  if (r != EF_OK) return r;
  r = rows_list_host(c, "outlier staging", rows, max_rows, count, [&](uint32_t* d_rows, uint32_t cap_rows, uint32_t* d_count) {
    return outlier_select_enqueue(c, "ef_map_outliers_select", p, among, d_rows, cap_rows, d_count, nullptr);
  });
  if (r != EF_OK) return r;
  return result ? outlier_result_host(c, result) : EF_OK;
}

int ef_map_remove_outliers(ef_ctx* c, const ef_outlier_params* p, const ef_map_selection* among, ef_outlier_result* res) {
  int r = outlier_check(c, "ef_map_remove_outliers", p, among, res, "result");
  if (r != EF_OK) return r;
  memset(res, 0, sizeof(*res));
  DeviceGuard dg_(c);
  uint32_t removed = 0;
  // the flags are 1 for the REMOVED rows: the erase keeps those whose flag differs from 1
  r = erase_run(c, "ef_map_remove_outliers", 1u, &removed, [&](uint32_t n, const efm::SelectScratch& sc, uint32_t* total) {
    // (the pointers of sc and total are into sel.scratch: growing the outliers' own scratch moves none of them)
    efm::OutlierArgs a;
    const int rm = outlier_mark(c, "ef_map_remove_outliers", p, among, n, sc.flags, &a);
    if (rm != EF_OK) return rm;
    efm::flags_count(sc, n, 1u, total, c->stream);
    return (int)EF_OK;
  });
  if (r != EF_OK) return r;
  r = outlier_result_host(c, res);   // (the sums, the threshold and the counts of the map as it was)
  if (r != EF_OK) return r;
  res->outliers = removed;
  res->count_after = c->sel.count;
  return EF_OK;
}

}  // extern "C"
