// ================================================================================================
// Connected components of the map under "closer than r" (include/ef_hip.h: ef_default_component_params, ef_map_components[_dev],
// ef_map_components_select[_dev], ef_map_remove_components; kernels in ef_components.inc, the index of ef_host_query.inc, the predicate, the
// lists and the erase of ef_host_select.inc; DESIGN.md §8j)
// ================================================================================================
namespace {
static_assert(sizeof(efm::ComponentResult) == sizeof(ef_component_result) && offsetof(efm::ComponentResult, largest) == offsetof(ef_component_result, largest) &&
                  offsetof(efm::ComponentResult, status) == offsetof(ef_component_result, status) && EF_COMPONENT_NONE == efm::COMPONENT_NONE &&
                  EF_COMPONENTS_REJECTED == efm::COMPONENTS_REJECTED && EF_COMPONENTS_ACCEPTED == efm::COMPONENTS_ACCEPTED,
              "the kernels' result and constants are the header's");
// refusals before any GPU work: the arguments first, the context last (with a NULL context ef_last_error(NULL) names the argument).  out: the
// call's required output (null out_name: it has none); what: EF_COMPONENTS_* (the calls without one pass EF_COMPONENTS_REJECTED)
int component_check(ef_ctx* c, const char* fn_, const ef_component_params* p, const ef_map_selection* among, int what, const void* out,
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
  if (what != EF_COMPONENTS_REJECTED && what != EF_COMPONENTS_ACCEPTED) { err = fn + ": what must be one of EF_COMPONENTS_*"; return EF_EINVAL; }
  if (max_rows && !rows) return select_null(c, fn_, "rows");
  if (among) {
    const int r = select_check(c, among, fn_);
    if (r != EF_OK) return r;
  }
  if (!c) return select_null(c, fn_, "context");
  return EF_OK;
}
// the components' own scratch for n rows, carved into a (res, parent, label, members, node) and sel_sc (the selection's counts and offsets)
int component_scratch(ef_ctx* c, uint32_t n, efm::ComponentArgs* a, efm::SelectScratch* sel_sc, uint32_t** sel_total) {
  if (n > c->components.rows || !c->components.scratch.p) {
    const size_t rows = std::min((size_t)c->capacity, (size_t)n + (size_t)n / 4 + 1024);
    c->components.rows = 0;
    const int r = c->components.scratch.reserve(c, 64 + 3 * rows * sizeof(uint32_t) + Carver::scan_bytes(rows) + rows + 64, "component scratch");
    if (r != EF_OK) return r;
    c->components.rows = rows;
  }
  Carver cv(c->components.scratch);
  a->res = cv.take<efm::ComponentResult>(1);
  a->parent = cv.take<uint32_t>(c->components.rows, 64);
  a->label = cv.take<uint32_t>(c->components.rows);
  a->members = cv.take<uint32_t>(c->components.rows);
  *sel_total = cv.scan_words(c->components.rows, sel_sc);
  sel_sc->flags = cv.take<uint8_t>(c->components.rows);
  a->node = sel_sc->flags;
  return EF_OK;
}
// Fills a for the n rows of the map and enqueues init, hook, label and finish: label and members of every row, the result but for count_after,
// and (flags not null) the byte of every row.  Waits for the device only where the selection's preparation, a grown scratch or an index rebuild do.
int component_enqueue(ef_ctx* c, const char* fn, const ef_component_params* p, const ef_map_selection* among, uint32_t n, int what, uint8_t* flags,
                      efm::ComponentArgs* a) {
  *a = efm::ComponentArgs{};
  efm::SelectScratch sel_sc;
  uint32_t* sel_total = nullptr;
  if (among) {   // the selection's bytes: its own kernel, into the components' scratch; k_comp_init turns them into the node bytes in place
    efm::SelectArgs sa;
    uint32_t n_sel = 0;
    int r = select_prepare(c, among, fn, &sa, &n_sel);
    if (r != EF_OK) return r;
    if (n_sel != n) { c->err = std::string(fn) + ": internal error (the map count changed inside the call)"; return EF_EHIP; }
    r = component_scratch(c, n, a, &sel_sc, &sel_total);
    if (r != EF_OK) return r;
    efm::select_flags(sa, sel_sc, sel_total, c->stream);
    a->sel = a->node;
  } else {
    const int r = component_scratch(c, n, a, &sel_sc, &sel_total);
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
  a->min_size = p->min_size;
  a->max_size = p->max_size;
  EF_HIP(c, hipMemsetAsync(a->res, 0, sizeof(efm::ComponentResult), c->stream));
  efm::component_hook(*a, c->stream);
  efm::component_label(*a, what, flags, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// device pointers; enqueues only (but for what component_enqueue needs)
int component_labels_enqueue(ef_ctx* c, const char* fn, const ef_component_params* p, const ef_map_selection* among, uint32_t* label_dev,
                             uint32_t* size_dev, uint32_t max_rows, ef_component_result* result_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::ComponentArgs a;
  r = component_enqueue(c, fn, p, among, n, EF_COMPONENTS_REJECTED, nullptr, &a);
  if (r != EF_OK) return r;
  efm::component_split(a, label_dev, size_dev, max_rows, c->stream);
  efm::component_tally(a, (efm::ComponentResult*)result_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
int component_select_enqueue(ef_ctx* c, const char* fn, const ef_component_params* p, const ef_map_selection* among, int what, uint32_t* rows_dev,
                             uint32_t max_rows, uint32_t* count_dev, ef_component_result* result_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::SelectScratch sc;
  uint32_t* total = nullptr;
  r = select_scratch(c, n, &sc, &total);
  if (r != EF_OK) return r;
  efm::ComponentArgs a;
  r = component_enqueue(c, fn, p, among, n, what, sc.flags, &a);
  if (r != EF_OK) return r;
  efm::flags_count(sc, n, 0u, count_dev, c->stream);
  efm::select_rows(sc, n, rows_dev, max_rows, c->stream);
  efm::component_tally(a, (efm::ComponentResult*)result_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// the call's result, as the kernels left it at the head of the components' scratch (synchronises); a tripped loop cap is an error of the call
int component_result_host(ef_ctx* c, const char* fn, ef_component_result* res_or_null) {
  ef_component_result res;
  EF_HIP(c, hipMemcpyAsync(&res, c->components.scratch.p, sizeof(res), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  if (res_or_null) *res_or_null = res;
  if (res.status) { c->err = std::string(fn) + ": internal error (a union-find loop exceeded its bound)"; return EF_EHIP; }
  return EF_OK;
}
}  // namespace

extern "C" {

int ef_default_component_params(ef_ctx* c, ef_component_params* p) {
  if (!c) { g_create_error = "ef_default_component_params: null context"; return EF_EINVAL; }
  if (!p) { c->err = "ef_default_component_params: null params"; return EF_EINVAL; }
  memset(p, 0, sizeof(*p));
  p->radius = 0.03f;
  p->cell = 0.03f;   // = radius, as the outlier filters' (DESIGN.md §8j: the fastest of radius / 2, radius and 2 radius on the larger map, within 4 % of the fastest on the smaller)
  p->min_conf = -1.0f;
  p->min_size = 50u;
  p->max_size = 0u;
  return EF_OK;
}

int ef_map_components_dev(ef_ctx* c, const ef_component_params* p, const ef_map_selection* among, uint32_t* label_dev, uint32_t* size_dev,
                          uint32_t max_rows, ef_component_result* result_dev) {
  int r = component_check(c, "ef_map_components_dev", p, among, EF_COMPONENTS_REJECTED, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_components_dev");
  if (r != EF_OK) return r;
  return component_labels_enqueue(c, "ef_map_components_dev", p, among, label_dev, size_dev, max_rows, result_dev);
}
int ef_map_components(ef_ctx* c, const ef_component_params* p, const ef_map_selection* among, uint32_t* label, uint32_t* size, uint32_t max_rows,
                      ef_component_result* result) {
  int r = component_check(c, "ef_map_components", p, among, EF_COMPONENTS_REJECTED, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_components");
  if (r != EF_OK) return r;
  uint32_t n = 0;
  r = select_count(c, &n);
  if (r != EF_OK) return r;
  const size_t rows = std::min((size_t)max_rows, (size_t)n);
  r = c->stage.reserve(c, 16 + rows * 8, "component staging");
  if (r != EF_OK) return r;
  uint32_t* d_label = c->stage.as<uint32_t>();
  uint32_t* d_size = (uint32_t*)(c->stage.p + rows * 4);
  r = component_labels_enqueue(c, "ef_map_components", p, among, label ? d_label : nullptr, size ? d_size : nullptr, (uint32_t)rows, nullptr);
  if (r != EF_OK) return r;
  if (rows && label) EF_HIP(c, hipMemcpyAsync(label, d_label, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && size) EF_HIP(c, hipMemcpyAsync(size, d_size, rows * 4, hipMemcpyDeviceToHost, c->stream));
  return component_result_host(c, "ef_map_components", result);
}

int ef_map_components_select_dev(ef_ctx* c, const ef_component_params* p, const ef_map_selection* among, int what, uint32_t* rows_dev,
                                 uint32_t max_rows, uint32_t* count_dev, ef_component_result* result_dev) {
  int r = component_check(c, "ef_map_components_select_dev", p, among, what, count_dev, "count", rows_dev, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_components_select_dev");
  if (r != EF_OK) return r;
  return component_select_enqueue(c, "ef_map_components_select_dev", p, among, what, rows_dev, max_rows, count_dev, result_dev);
}
int ef_map_components_select(ef_ctx* c, const ef_component_params* p, const ef_map_selection* among, int what, uint32_t* rows, uint32_t max_rows,
                             uint32_t* count, ef_component_result* result) {
  int r = component_check(c, "ef_map_components_select", p, among, what, count, "count", rows, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_components_select");
  if (r != EF_OK) return r;
  r = rows_list_host(c, "component staging", rows, max_rows, count, [&](uint32_t* d_rows, uint32_t cap_rows, uint32_t* d_count) {
    return component_select_enqueue(c, "ef_map_components_select", p, among, what, d_rows, cap_rows, d_count, nullptr);
  });
  if (r != EF_OK) return r;
  return component_result_host(c, "ef_map_components_select", result);
}

int ef_map_remove_components(ef_ctx* c, const ef_component_params* p, const ef_map_selection* among, ef_component_result* res) {
  int r = component_check(c, "ef_map_remove_components", p, among, EF_COMPONENTS_REJECTED, res, "result");
  if (r != EF_OK) return r;
  memset(res, 0, sizeof(*res));
  DeviceGuard dg_(c);
  uint32_t removed = 0;
  // the flags are 1 for the REMOVED rows: the erase keeps those whose flag differs from 1
  r = erase_run(c, "ef_map_remove_components", 1u, &removed, [&](uint32_t n, const efm::SelectScratch& sc, uint32_t* total) {
    // (the pointers of sc and total are into sel.scratch: growing the components' own scratch moves none of them)
    efm::ComponentArgs a;
    int rm = component_enqueue(c, "ef_map_remove_components", p, among, n, EF_COMPONENTS_REJECTED, sc.flags, &a);
    if (rm != EF_OK) return rm;
    efm::component_tally(a, nullptr, c->stream);
    // the counts of the map as it was, read while no row has changed yet: a tripped cap refuses the removal
    rm = component_result_host(c, "ef_map_remove_components", res);
    if (rm != EF_OK) return rm;
    efm::flags_count(sc, n, 1u, total, c->stream);
    return (int)EF_OK;
  });
  if (r != EF_OK) return r;
  res->rejected_rows = removed;
  res->count_after = c->sel.count;
  return EF_OK;
}

}  // extern "C"
