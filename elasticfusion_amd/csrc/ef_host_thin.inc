// ================================================================================================
// Thin the map to one surfel per voxel (include/ef_hip.h: ef_default_thin_params, ef_map_thin_select[_dev], ef_map_thin; kernels in
// ef_thin.inc, the index of ef_host_query.inc, the predicate, the lists and the erase of ef_host_select.inc; DESIGN.md §8f)
// ================================================================================================
namespace {
// refusals before any GPU work: the arguments first, the context last (with a NULL context ef_last_error(NULL) names the argument)
int thin_check(ef_ctx* c, const char* fn_, const ef_thin_params* p, const ef_map_selection* among, const void* out, const char* out_name) {
  std::string& err = c ? c->err : g_create_error;
  const std::string fn = fn_;
  if (!p) { err = fn + ": null params"; return EF_EINVAL; }
  if (!out) { err = fn + ": null " + out_name; return EF_EINVAL; }
  if (!(p->cell > 0.f) || !std::isfinite(p->cell) || !std::isfinite(1.0f / p->cell)) { err = fn + ": cell must be finite and positive"; return EF_EINVAL; }
  if (p->keep != EF_THIN_KEEP_MAX_CONF && p->keep != EF_THIN_KEEP_NEWEST && p->keep != EF_THIN_KEEP_FIRST) {
    err = fn + ": keep must be one of EF_THIN_KEEP_*";
    return EF_EINVAL;
  }
  return among ? select_check(c, among, fn_) : EF_OK;
}
int thin_select_check(ef_ctx* c, const char* fn, const ef_thin_params* p, const ef_map_selection* among, int what, const uint32_t* rows,
                      uint32_t max_rows, const uint32_t* count) {
  const int r = thin_check(c, fn, p, among, count, "count");
  if (r != EF_OK) return r;
  if (what != EF_THIN_ROWS_REMOVED && what != EF_THIN_ROWS_REPRESENTATIVES) {
    (c ? c->err : g_create_error) = std::string(fn) + ": what must be EF_THIN_ROWS_REMOVED or EF_THIN_ROWS_REPRESENTATIVES";
    return EF_EINVAL;
  }
  if (max_rows && !rows) return select_null(c, fn, "rows");
  if (!c) return select_null(c, fn, "context");
  return EF_OK;
}
// the thin's own scratch for n rows: counts, offsets and one byte per row for the participants (part) and, with the same counts and offsets
// reused behind them on the stream, for the representatives (rep); total[0 .. 3]
int thin_scratch(ef_ctx* c, uint32_t n, efm::SelectScratch* part, efm::SelectScratch* rep, uint32_t** total) {
  if (n > c->thin.rows || !c->thin.scratch.p) {
    const size_t rows = std::min((size_t)c->capacity, (size_t)n + (size_t)n / 4 + 1024);
    c->thin.rows = 0;
    const int r = c->thin.scratch.reserve(c, Carver::scan_bytes(rows) + 2 * rows, "thin scratch");
    if (r != EF_OK) return r;
    c->thin.rows = rows;
  }
  Carver cv(c->thin.scratch);
  *total = cv.scan_words(c->thin.rows, part);
  part->flags = cv.take<uint8_t>(c->thin.rows);
  *rep = *part;   // (the shared counts and offsets)
  rep->flags = cv.take<uint8_t>(c->thin.rows);
  return EF_OK;
}
// Enqueues the bytes of the n rows of the map: removed[row] = 1 for every removed row and rep[row] = 1 for every representative (either may
// be null), 0 for every other row.  Waits for the device only where the selection's preparation or an index rebuild do.
int thin_mark(ef_ctx* c, const char* fn, const ef_thin_params* p, const ef_map_selection* among, uint32_t n, uint8_t* removed, uint8_t* rep) {
  efm::ThinArgs a{};
  if (among) {   // the participant bytes: the selection's own kernel, into the thin's scratch
    efm::SelectArgs sa;
    uint32_t n_sel = 0;
    int r = select_prepare(c, among, fn, &sa, &n_sel);
    if (r != EF_OK) return r;
    if (n_sel != n) { c->err = std::string(fn) + ": internal error (the map count changed inside the call)"; return EF_EHIP; }
    efm::SelectScratch part, unused;
    uint32_t* total = nullptr;
    r = thin_scratch(c, n, &part, &unused, &total);
    if (r != EF_OK) return r;
    efm::select_flags(sa, part, total, c->stream);
    a.part = part.flags;
  }
  if (removed && n) EF_HIP(c, hipMemsetAsync(removed, 0, n, c->stream));
  if (rep && n) EF_HIP(c, hipMemsetAsync(rep, 0, n, c->stream));
  const int r = query_index(c, p->cell);
  if (r != EF_OK) return r;
  if (c->query.n != n) { c->err = std::string(fn) + ": internal error (the index does not cover the map)"; return EF_EHIP; }
  query_index_args(c, &a.q);
  a.n = n;
  a.keep = p->keep;
  a.removed = removed;
  a.rep = rep;
  efm::thin_flags(a, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// device pointers; enqueues only (but for what thin_mark and the scratch need)
int thin_select_enqueue(ef_ctx* c, const char* fn, const ef_thin_params* p, const ef_map_selection* among, int what, uint32_t* rows_dev,
                        uint32_t max_rows, uint32_t* count_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::SelectScratch sc;
  uint32_t* total = nullptr;
  r = select_scratch(c, n, &sc, &total);
  if (r != EF_OK) return r;
  r = thin_mark(c, fn, p, among, n, what == EF_THIN_ROWS_REMOVED ? sc.flags : nullptr, what == EF_THIN_ROWS_REPRESENTATIVES ? sc.flags : nullptr);
  if (r != EF_OK) return r;
  efm::flags_count(sc, n, 0u, count_dev, c->stream);
  efm::select_rows(sc, n, rows_dev, max_rows, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
}  // namespace

extern "C" {

int ef_default_thin_params(ef_ctx* c, ef_thin_params* p) {
  if (!c) { g_create_error = "ef_default_thin_params: null context"; return EF_EINVAL; }
  if (!p) { c->err = "ef_default_thin_params: null params"; return EF_EINVAL; }
  memset(p, 0, sizeof(*p));
  p->cell = EF_QUERY_DEFAULT_CELL;
  p->keep = EF_THIN_KEEP_MAX_CONF;
  return EF_OK;
}

int ef_map_thin_select_dev(ef_ctx* c, const ef_thin_params* p, const ef_map_selection* among, int what, uint32_t* rows_dev, uint32_t max_rows,
                           uint32_t* count_dev) {
  int r = thin_select_check(c, "ef_map_thin_select_dev", p, among, what, rows_dev, max_rows, count_dev);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_thin_select_dev");
  if (r != EF_OK) return r;
  return thin_select_enqueue(c, "ef_map_thin_select_dev", p, among, what, rows_dev, max_rows, count_dev);
}
int ef_map_thin_select(ef_ctx* c, const ef_thin_params* p, const ef_map_selection* among, int what, uint32_t* rows, uint32_t max_rows,
                       uint32_t* count) {
  int r = thin_select_check(c, "ef_map_thin_select", p, among, what, rows, max_rows, count);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_thin_select");
  if (r != EF_OK) return r;
  return rows_list_host(c, "thin staging", rows, max_rows, count, [&](uint32_t* d_rows, uint32_t cap_rows, uint32_t* d_count) {
    return thin_select_enqueue(c, "ef_map_thin_select", p, among, what, d_rows, cap_rows, d_count);
  });
}

int ef_map_thin(ef_ctx* c, const ef_thin_params* p, const ef_map_selection* among, ef_thin_result* res) {
  int r = thin_check(c, "ef_map_thin", p, among, res, "result");
  if (r != EF_OK) return r;
  if (!c) return select_null(c, "ef_map_thin", "context");
  memset(res, 0, sizeof(*res));
  DeviceGuard dg_(c);
  uint32_t removed = 0;
  uint32_t* rep_total = nullptr;
  // the flags are 1 for the REMOVED rows: the erase keeps those whose flag differs from 1
  r = erase_run(c, "ef_map_thin", 1u, &removed, [&](uint32_t n, const efm::SelectScratch& sc, uint32_t* total) {
    // (the pointers of sc and total are into sel.scratch: growing the thin's own scratch moves none of them)
    efm::SelectScratch part, rep;
    uint32_t* tot = nullptr;
    int rm = thin_scratch(c, n, &part, &rep, &tot);
    if (rm != EF_OK) return rm;
    rm = thin_mark(c, "ef_map_thin", p, among, n, sc.flags, rep.flags);
    if (rm != EF_OK) return rm;
    efm::flags_count(sc, n, 1u, total, c->stream);
    rep_total = tot + 1;
    efm::flags_count(rep, n, 0u, rep_total, c->stream);   // the representatives are only counted
    return (int)EF_OK;
  });
  if (r != EF_OK) return r;
  uint32_t cells = 0;   // (erase_run has synchronised behind the count)
  EF_HIP(c, hipMemcpyAsync(&cells, rep_total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  res->cells = cells;
  res->removed = removed;
  res->participants = cells + removed;
  res->count_after = c->sel.count;
  return EF_OK;
}

}  // extern "C"
