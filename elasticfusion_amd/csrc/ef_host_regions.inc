// ================================================================================================
// Segment the map into smooth regions (include/ef_hip.h: ef_default_region_params, ef_map_regions[_dev], ef_map_regions_select[_dev],
// ef_map_remove_regions; kernels in ef_regions.inc and the join of ef_normals.inc, the index of ef_host_query.inc, the predicate, the lists and
// the erase of ef_host_select.inc; DESIGN.md §8m)
// ================================================================================================
namespace {
static_assert(sizeof(efm::RegionResult) == sizeof(ef_region_result) && sizeof(ef_region_result) == 12 * sizeof(uint32_t) &&
                  offsetof(efm::RegionResult, largest) == offsetof(ef_region_result, largest) &&
                  offsetof(efm::RegionResult, listed) == offsetof(ef_region_result, listed) &&
                  offsetof(efm::RegionResult, status) == offsetof(ef_region_result, status) && EF_REGION_NONE == efm::REGION_NONE &&
                  EF_REGION_KIND_NONE == efm::REGION_KIND_NONE && EF_REGION_KIND_CORE == efm::REGION_KIND_CORE &&
                  EF_REGION_KIND_BORDER == efm::REGION_KIND_BORDER && EF_REGIONS_ESTIMATED == efm::REGIONS_ESTIMATED &&
                  EF_REGIONS_STORED == efm::REGIONS_STORED && EF_REGIONS_REJECTED == efm::REGIONS_REJECTED &&
                  EF_REGIONS_ACCEPTED == efm::REGIONS_ACCEPTED && EF_REGIONS_UNASSIGNED == efm::REGIONS_UNASSIGNED &&
                  EF_REGIONS_BORDERS == efm::REGIONS_BORDERS,
              "the kernels' result and constants are the header's");
// refusals before any GPU work: the arguments first, the context last (with a NULL context ef_last_error(NULL) names the argument).  out: the
// call's required output (null out_name: it has none); what: EF_REGIONS_* (the calls without one pass EF_REGIONS_REJECTED)
int region_check(ef_ctx* c, const char* fn_, const ef_region_params* p, const ef_map_selection* among, int what, const void* out,
                 const char* out_name, const void* rows = nullptr, uint32_t max_rows = 0) {
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
  if (std::isnan(p->line_ratio) || p->line_ratio < 0.f) { err = fn + ": line_ratio must not be negative or NaN"; return EF_EINVAL; }
  if (p->normal_source != EF_REGIONS_ESTIMATED && p->normal_source != EF_REGIONS_STORED) {
    err = fn + ": normal_source must be EF_REGIONS_ESTIMATED or EF_REGIONS_STORED";
    return EF_EINVAL;
  }
  if (std::isnan(p->min_normal_cos)) { err = fn + ": min_normal_cos is NaN"; return EF_EINVAL; }
  if (std::isnan(p->max_curvature) || p->max_curvature < 0.f) { err = fn + ": max_curvature must not be negative or NaN"; return EF_EINVAL; }
  if (what != EF_REGIONS_REJECTED && what != EF_REGIONS_ACCEPTED && what != EF_REGIONS_UNASSIGNED && what != EF_REGIONS_BORDERS) {
    err = fn + ": what must be one of EF_REGIONS_REJECTED, EF_REGIONS_ACCEPTED, EF_REGIONS_UNASSIGNED, EF_REGIONS_BORDERS";
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
// the regions' own scratch for n rows, carved into a (the result, the join's est / stat / status, the stored-normal word, parent, attach, label,
// members, kind) and part_sc (the selection's counts and offsets; its flags are the status bytes, as in normal_scratch)
int region_scratch(ef_ctx* c, uint32_t n, efm::RegionArgs* a, efm::SelectScratch* part_sc, uint32_t** part_total) {
  if (n > c->regions.rows || !c->regions.scratch.p) {
    const size_t rows = std::min((size_t)c->capacity, (size_t)n + (size_t)n / 4 + 1024);
    c->regions.rows = 0;
    const int r = c->regions.scratch.reserve(c, 64 + rows * (2 * sizeof(float4) + sizeof(uint2) + 4 * sizeof(uint32_t)) + Carver::scan_bytes(rows) + 2 * rows + 128,
                                             "region scratch");
    if (r != EF_OK) return r;
    c->regions.rows = rows;
  }
  const size_t rows = c->regions.rows;
  Carver cv(c->regions.scratch);
  a->res = cv.take<efm::RegionResult>(1);
  a->nrm.est = cv.take<float4>(rows, 16);
  a->stored = cv.take<float4>(rows, 16);
  a->nrm.stat = cv.take<uint2>(rows);
  a->parent = cv.take<uint32_t>(rows);
  a->attach = cv.take<uint32_t>(rows);
  a->label = cv.take<uint32_t>(rows);
  a->members = cv.take<uint32_t>(rows);
  *part_total = cv.scan_words(rows, part_sc);
  part_sc->flags = cv.take<uint8_t>(rows);
  a->nrm.status = part_sc->flags;
  a->kind = cv.take<uint8_t>(rows);
  return EF_OK;
}
// Fills a for the n rows of the map and enqueues the estimate (the normals' join, unchanged, into this scratch), init, first, hook, attach, label
// and finish: label, members and kind of every row, the result but for count_after, and (flags not null) the list's byte of every row.  Waits
// for the device only where the selection's preparation, a grown scratch or an index rebuild do.
int region_enqueue(ef_ctx* c, const char* fn, const ef_region_params* p, const ef_map_selection* among, uint32_t n, int what, uint8_t* flags,
                   efm::RegionArgs* a) {
  *a = efm::RegionArgs{};
  efm::SelectScratch part_sc;
  uint32_t* part_total = nullptr;
  if (among) {   // the selection's bytes: its own kernel, into the regions' scratch; the join turns them into the status bytes in place
    efm::SelectArgs sa;
    uint32_t n_sel = 0;
    int r = select_prepare(c, among, fn, &sa, &n_sel);
    if (r != EF_OK) return r;
    if (n_sel != n) { c->err = std::string(fn) + ": internal error (the map count changed inside the call)"; return EF_EHIP; }
    r = region_scratch(c, n, a, &part_sc, &part_total);
    if (r != EF_OK) return r;
    efm::select_flags(sa, part_sc, part_total, c->stream);
    a->nrm.part_in = a->nrm.status;
  } else {
    const int r = region_scratch(c, n, a, &part_sc, &part_total);
    if (r != EF_OK) return r;
  }
  const int r = query_index(c, p->cell);
  if (r != EF_OK) return r;
  if (c->query.n != n) { c->err = std::string(fn) + ": internal error (the index does not cover the map)"; return EF_EHIP; }
  efm::NormalArgs& m = a->nrm;
  query_index_args(c, &m.q);
  m.q.max_dist = p->radius;
  m.q.r2 = p->radius * p->radius;
  m.q.min_conf = p->min_conf;
  m.n = n;
  m.k = p->k;
  m.min_neighbors = (uint32_t)p->min_neighbors;
  m.orientation = EF_NORMALS_KEEP_SIDE;
  m.side = -1.0f;
  m.line_ratio = p->line_ratio;
  m.max_curvature = p->max_curvature;
  m.radius_scale = 1.0f;
  a->min_normal_cos = p->min_normal_cos;
  a->max_curvature = p->max_curvature;
  a->two_sided = p->two_sided != 0;
  a->normal_source = p->normal_source;
  a->attach_borders = p->attach_borders != 0;
  a->min_size = p->min_size;
  a->max_size = p->max_size;
  a->nw = p->normal_source == EF_REGIONS_STORED ? a->stored : m.est;
  EF_HIP(c, hipMemsetAsync(a->res, 0, sizeof(efm::RegionResult), c->stream));
  efm::normal_join(m, c->stream);
  efm::region_hook(*a, c->stream);
  efm::region_label(*a, what, flags, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// device pointers; enqueues only (but for what region_enqueue needs)
int region_labels_enqueue(ef_ctx* c, const char* fn, const ef_region_params* p, const ef_map_selection* among, uint32_t* label_dev, uint32_t* size_dev,
                          uint8_t* kind_dev, uint32_t max_rows, ef_region_result* result_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::RegionArgs a;
  r = region_enqueue(c, fn, p, among, n, EF_REGIONS_REJECTED, nullptr, &a);
  if (r != EF_OK) return r;
  efm::region_split(a, label_dev, size_dev, kind_dev, max_rows, c->stream);
  efm::region_tally(a, (efm::RegionResult*)result_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
int region_select_enqueue(ef_ctx* c, const char* fn, const ef_region_params* p, const ef_map_selection* among, int what, uint32_t* rows_dev,
                          uint32_t max_rows, uint32_t* count_dev, ef_region_result* result_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::SelectScratch sc;
  uint32_t* total = nullptr;
  r = select_scratch(c, n, &sc, &total);
  if (r != EF_OK) return r;
  efm::RegionArgs a;
  r = region_enqueue(c, fn, p, among, n, what, sc.flags, &a);
  if (r != EF_OK) return r;
  efm::flags_count(sc, n, 0u, count_dev, c->stream);
  efm::select_rows(sc, n, rows_dev, max_rows, c->stream);
  efm::region_tally(a, (efm::RegionResult*)result_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// the call's result, as the kernels left it at the head of the regions' scratch (synchronises); a tripped loop cap is an error of the call
int region_result_host(ef_ctx* c, const char* fn, ef_region_result* res_or_null) {
  ef_region_result res;
  EF_HIP(c, hipMemcpyAsync(&res, c->regions.scratch.p, sizeof(res), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  if (res_or_null) *res_or_null = res;
  if (res.status) { c->err = std::string(fn) + ": internal error (a union-find loop exceeded its bound)"; return EF_EHIP; }
  return EF_OK;
}
}  // namespace

extern "C" {

int ef_default_region_params(ef_ctx* c, ef_region_params* p) {
  if (!c) { g_create_error = "ef_default_region_params: null context"; return EF_EINVAL; }
  if (!p) { c->err = "ef_default_region_params: null params"; return EF_EINVAL; }
  memset(p, 0, sizeof(*p));
  p->radius = 0.03f;
  p->cell = 0.03f;   // = radius, as the normals' and the components'
  p->min_conf = -1.0f;
  p->k = 12;
  p->min_neighbors = 5;
  p->line_ratio = 1e-4f;
  p->normal_source = EF_REGIONS_ESTIMATED;
  p->two_sided = 0;
  p->min_normal_cos = 0.9659258f;   // cos 15 degrees: a definition
  p->max_curvature = 0.05f;         // the normals' default
  p->attach_borders = 1;
  p->min_size = 50u;
  p->max_size = 0u;
  return EF_OK;
}

int ef_map_regions_dev(ef_ctx* c, const ef_region_params* p, const ef_map_selection* among, uint32_t* label_dev, uint32_t* size_dev, uint8_t* kind_dev,
                       uint32_t max_rows, ef_region_result* result_dev) {
  int r = region_check(c, "ef_map_regions_dev", p, among, EF_REGIONS_REJECTED, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_regions_dev");
  if (r != EF_OK) return r;
  return region_labels_enqueue(c, "ef_map_regions_dev", p, among, label_dev, size_dev, kind_dev, max_rows, result_dev);
}
int ef_map_regions(ef_ctx* c, const ef_region_params* p, const ef_map_selection* among, uint32_t* label, uint32_t* size, uint8_t* kind,
                   uint32_t max_rows, ef_region_result* result) {
  int r = region_check(c, "ef_map_regions", p, among, EF_REGIONS_REJECTED, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_regions");
  if (r != EF_OK) return r;
  uint32_t n = 0;
  r = select_count(c, &n);
  if (r != EF_OK) return r;
  const size_t rows = std::min((size_t)max_rows, (size_t)n);
  r = c->stage.reserve(c, 16 + rows * 9, "region staging");   // 4 + 4 + 1 bytes per row
  if (r != EF_OK) return r;
  uint32_t* d_label = c->stage.as<uint32_t>();
  uint32_t* d_size = d_label + rows;
  uint8_t* d_kind = (uint8_t*)(d_size + rows);
  r = region_labels_enqueue(c, "ef_map_regions", p, among, label ? d_label : nullptr, size ? d_size : nullptr, kind ? d_kind : nullptr,
                            (uint32_t)rows, nullptr);
  if (r != EF_OK) return r;
  if (rows && label) EF_HIP(c, hipMemcpyAsync(label, d_label, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && size) EF_HIP(c, hipMemcpyAsync(size, d_size, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && kind) EF_HIP(c, hipMemcpyAsync(kind, d_kind, rows, hipMemcpyDeviceToHost, c->stream));
  return region_result_host(c, "ef_map_regions", result);
}

int ef_map_regions_select_dev(ef_ctx* c, const ef_region_params* p, const ef_map_selection* among, int what, uint32_t* rows_dev, uint32_t max_rows,
                              uint32_t* count_dev, ef_region_result* result_dev) {
  int r = region_check(c, "ef_map_regions_select_dev", p, among, what, count_dev, "count", rows_dev, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_regions_select_dev");
  if (r != EF_OK) return r;
  return region_select_enqueue(c, "ef_map_regions_select_dev", p, among, what, rows_dev, max_rows, count_dev, result_dev);
}
int ef_map_regions_select(ef_ctx* c, const ef_region_params* p, const ef_map_selection* among, int what, uint32_t* rows, uint32_t max_rows,
                          uint32_t* count, ef_region_result* result) {
  int r = region_check(c, "ef_map_regions_select", p, among, what, count, "count", rows, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_regions_select");
  if (r != EF_OK) return r;
  r = rows_list_host(c, "region staging", rows, max_rows, count, [&](uint32_t* d_rows, uint32_t cap_rows, uint32_t* d_count) {
    return region_select_enqueue(c, "ef_map_regions_select", p, among, what, d_rows, cap_rows, d_count, nullptr);
  });
  if (r != EF_OK) return r;
  return region_result_host(c, "ef_map_regions_select", result);
}

int ef_map_remove_regions(ef_ctx* c, const ef_region_params* p, const ef_map_selection* among, int what, ef_region_result* res) {
  int r = region_check(c, "ef_map_remove_regions", p, among, what, res, "result");
  if (r != EF_OK) return r;
  memset(res, 0, sizeof(*res));
  DeviceGuard dg_(c);
  uint32_t removed = 0;
  // the flags are 1 for the REMOVED rows: the erase keeps those whose flag differs from 1
  r = erase_run(c, "ef_map_remove_regions", 1u, &removed, [&](uint32_t n, const efm::SelectScratch& sc, uint32_t* total) {
    // (the pointers of sc and total are into sel.scratch: growing the regions' own scratch moves none of them)
    efm::RegionArgs a;
    int rm = region_enqueue(c, "ef_map_remove_regions", p, among, n, what, sc.flags, &a);
    if (rm != EF_OK) return rm;
    efm::region_tally(a, nullptr, c->stream);
    // the counts of the map as it was, read while no row has changed yet: a tripped cap refuses the removal
    rm = region_result_host(c, "ef_map_remove_regions", res);
    if (rm != EF_OK) return rm;
    efm::flags_count(sc, n, 1u, total, c->stream);
    return (int)EF_OK;
  });
  if (r != EF_OK) return r;
  res->listed = removed;
  res->count_after = c->sel.count;
  return EF_OK;
}

}  // extern "C"
