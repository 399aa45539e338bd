// ================================================================================================
// Find the map's boundaries by the angle criterion (include/ef_hip.h: ef_default_boundary_params, ef_boundary_gap_from_angle,
// ef_map_boundaries[_dev], ef_map_boundaries_select[_dev]; kernels in ef_boundary.inc, the join of ef_normals.inc and the union-find of
// ef_components.inc, the index of ef_host_query.inc, the predicate and the lists of ef_host_select.inc; DESIGN.md §8o)
// ================================================================================================
namespace {
static_assert(sizeof(efm::BoundaryResult) == sizeof(ef_boundary_result) && sizeof(ef_boundary_result) == 10 * sizeof(uint32_t) &&
                  offsetof(efm::BoundaryResult, participants) == offsetof(ef_boundary_result, participants) &&
                  offsetof(efm::BoundaryResult, loops) == offsetof(ef_boundary_result, loops) &&
                  offsetof(efm::BoundaryResult, listed) == offsetof(ef_boundary_result, listed) &&
                  offsetof(efm::BoundaryResult, status) == offsetof(ef_boundary_result, status) && EF_BOUNDARY_STORED == efm::BOUNDARY_STORED &&
                  EF_BOUNDARY_ESTIMATED == efm::BOUNDARY_ESTIMATED && EF_BOUNDARY_NONE == efm::BOUNDARY_NONE &&
                  EF_BOUNDARY_INTERIOR == efm::BOUNDARY_INTERIOR && EF_BOUNDARY_BOUNDARY == efm::BOUNDARY_BOUNDARY &&
                  EF_BOUNDARY_SPARSE == efm::BOUNDARY_SPARSE && EF_BOUNDARY_DEGENERATE == efm::BOUNDARY_DEGENERATE &&
                  EF_BOUNDARY_LOOPS_ACCEPTED == efm::BOUNDARY_LOOPS_ACCEPTED && EF_BOUNDARY_LOOPS_REJECTED == efm::BOUNDARY_LOOPS_REJECTED,
              "the kernels' result and constants are the header's");
static_assert(sizeof(ef_boundary_params) == 10 * 4 && offsetof(ef_boundary_params, normal_source) == 20 && offsetof(ef_boundary_params, max_gap) == 28 &&
                  offsetof(ef_boundary_params, max_size) == 36,
              "ef_boundary_params is ten words");
// refusals before any GPU work: the arguments first, the context last (with a NULL context ef_last_error(NULL) names the argument).  out: the
// call's required output (null out_name: it has none); what < 0: the call lists nothing
int boundary_check(ef_ctx* c, const char* fn_, const ef_boundary_params* p, const ef_map_selection* among, const void* out, const char* out_name,
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
  if (p->normal_source != EF_BOUNDARY_STORED && p->normal_source != EF_BOUNDARY_ESTIMATED) {
    err = fn + ": normal_source must be EF_BOUNDARY_STORED or EF_BOUNDARY_ESTIMATED";
    return EF_EINVAL;
  }
  if (std::isnan(p->line_ratio) || p->line_ratio < 0.f) { err = fn + ": line_ratio must not be negative or NaN"; return EF_EINVAL; }
  if (!std::isfinite(p->max_gap) || !(p->max_gap > 0.f && p->max_gap < 4.f)) { err = fn + ": max_gap must lie inside (0, 4)"; return EF_EINVAL; }
  if (what >= 0 && what != EF_BOUNDARY_INTERIOR && what != EF_BOUNDARY_BOUNDARY && what != EF_BOUNDARY_SPARSE && what != EF_BOUNDARY_DEGENERATE &&
      what != EF_BOUNDARY_LOOPS_ACCEPTED && what != EF_BOUNDARY_LOOPS_REJECTED) {
    err = fn + ": what must be EF_BOUNDARY_INTERIOR, EF_BOUNDARY_BOUNDARY, EF_BOUNDARY_SPARSE, EF_BOUNDARY_DEGENERATE, EF_BOUNDARY_LOOPS_ACCEPTED or "
               "EF_BOUNDARY_LOOPS_REJECTED";
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
// the boundaries' own scratch for n rows, carved into a (the two results, the estimate's est / stat, {gap, count}, the union-find's parent, label
// and members, the status bytes, the normals' status bytes) and part_sc (the selection's counts and offsets; its flags are `bytes`)
int boundary_scratch(ef_ctx* c, uint32_t n, efm::BoundaryArgs* a, efm::SelectScratch* part_sc, uint32_t** part_total) {
  if (n > c->boundary.rows || !c->boundary.scratch.p) {
    const size_t rows = std::min((size_t)c->capacity, (size_t)n + (size_t)n / 4 + 1024);
    c->boundary.rows = 0;
    const int r = c->boundary.scratch.reserve(c, 128 + rows * (sizeof(float4) + 2 * sizeof(uint2) + 3 * sizeof(uint32_t)) + Carver::scan_bytes(rows) + 2 * rows + 128,
                                              "boundary scratch");
    if (r != EF_OK) return r;
    c->boundary.rows = rows;
  }
  const size_t rows = c->boundary.rows;
  Carver cv(c->boundary.scratch);
  a->res = cv.take<efm::BoundaryResult>(1);
  a->loops.res = cv.take<efm::ComponentResult>(1);
  a->nrm.est = cv.take<float4>(rows, 16);
  a->nrm.stat = cv.take<uint2>(rows);
  a->stat = cv.take<uint2>(rows);
  a->loops.parent = cv.take<uint32_t>(rows);
  a->loops.label = cv.take<uint32_t>(rows);
  a->loops.members = cv.take<uint32_t>(rows);
  *part_total = cv.scan_words(rows, part_sc);
  part_sc->flags = cv.take<uint8_t>(rows);
  a->status = cv.take<uint8_t>(rows);
  return EF_OK;
}
// Fills a for the n rows of the map and enqueues the estimate (ESTIMATED: the normals' join, unchanged, into this scratch), the join, the
// BOUNDARY byte, the components' init, first, hook, label and finish on it, and (flags not null) the list's byte of every row.  Waits for the
// device only where the selection's preparation, a grown scratch or an index rebuild do.
int boundary_enqueue(ef_ctx* c, const char* fn, const ef_boundary_params* p, const ef_map_selection* among, uint32_t n, int what, uint8_t* flags,
                     efm::BoundaryArgs* a) {
  *a = efm::BoundaryArgs{};
  efm::SelectScratch part_sc;
  uint32_t* part_total = nullptr;
  const bool estimated = p->normal_source == EF_BOUNDARY_ESTIMATED;
  if (among) {   // the selection's bytes: its own kernel, into this scratch
    efm::SelectArgs sa;
    uint32_t n_sel = 0;
    int r = select_prepare(c, among, fn, &sa, &n_sel);
    if (r != EF_OK) return r;
    if (n_sel != n) { c->err = std::string(fn) + ": internal error (the map count changed inside the call)"; return EF_EHIP; }
    r = boundary_scratch(c, n, a, &part_sc, &part_total);
    if (r != EF_OK) return r;
    efm::select_flags(sa, part_sc, part_total, c->stream);
    a->part_in = part_sc.flags;
  } else {
    const int r = boundary_scratch(c, n, a, &part_sc, &part_total);
    if (r != EF_OK) return r;
  }
  uint8_t* bytes = part_sc.flags;   // the selection's bytes, then (ESTIMATED) the normals' status bytes in place, then the loops' node bytes
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
  a->normal_source = p->normal_source;
  a->max_gap = p->max_gap;
  EF_HIP(c, hipMemsetAsync(a->res, 0, (char*)(a->loops.res + 1) - (char*)a->res, c->stream));   // both results
  if (estimated) {
    efm::NormalArgs& m = a->nrm;
    m.q = a->q;
    m.n = n;
    m.k = p->k;
    m.min_neighbors = (uint32_t)p->min_neighbors;
    m.orientation = EF_NORMALS_KEEP_SIDE;
    m.side = -1.0f;
    m.line_ratio = p->line_ratio;
    m.radius_scale = 1.0f;
    // part_in == status: sound only because k_normal_join reads and writes a row's byte from the one lane that owns the row's record (a row
    // the index does not hold is written by lane t == row alone and read by nobody).  A change to that kernel that breaks this needs a
    // second byte array here
    m.part_in = a->part_in;
    m.status = bytes;
    a->nest = m.est;
    a->nstatus = bytes;
    efm::normal_join(m, c->stream);
  }
  efm::boundary_join(*a, c->stream);
  // the loops: the components of the BOUNDARY rows.  The join has read `bytes` for the last time: they become the node bytes
  efm::ComponentArgs& l = a->loops;
  l.q = a->q;
  l.n = n;
  l.min_size = p->min_size;
  l.max_size = p->max_size;
  // sel == node: sound only because k_comp_init reads sel[r] and writes node[r] from the one lane r (component_scratch relies on the same)
  l.node = bytes;
  l.sel = bytes;
  efm::boundary_flags(*a, efm::BOUNDARY_BOUNDARY, bytes, c->stream);
  efm::component_hook(l, c->stream);
  const bool loop_list = what == EF_BOUNDARY_LOOPS_ACCEPTED || what == EF_BOUNDARY_LOOPS_REJECTED;
  efm::component_label(l, what == EF_BOUNDARY_LOOPS_ACCEPTED ? efm::COMPONENTS_ACCEPTED : efm::COMPONENTS_REJECTED, loop_list ? flags : nullptr, c->stream);
  if (flags && !loop_list) efm::boundary_flags(*a, (unsigned)what, flags, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// device pointers; enqueues only (but for what boundary_enqueue needs)
int boundary_rows_enqueue(ef_ctx* c, const char* fn, const ef_boundary_params* p, const ef_map_selection* among, float* gap, uint32_t* count,
                          uint8_t* status, uint32_t* label, uint32_t* size, uint32_t max_rows, ef_boundary_result* result_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::BoundaryArgs a;
  r = boundary_enqueue(c, fn, p, among, n, -1, nullptr, &a);
  if (r != EF_OK) return r;
  efm::boundary_split(a, gap, count, status, label, size, max_rows, c->stream);
  efm::boundary_tally(a, nullptr, (efm::BoundaryResult*)result_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
int boundary_select_enqueue(ef_ctx* c, const char* fn, const ef_boundary_params* p, const ef_map_selection* among, int what, uint32_t* rows_dev,
                            uint32_t max_rows, uint32_t* count_dev, ef_boundary_result* result_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::SelectScratch sc;
  uint32_t* total = nullptr;
  r = select_scratch(c, n, &sc, &total);
  if (r != EF_OK) return r;
  efm::BoundaryArgs a;
  r = boundary_enqueue(c, fn, p, among, n, what, sc.flags, &a);
  if (r != EF_OK) return r;
  efm::flags_count(sc, n, 0u, count_dev, c->stream);
  efm::select_rows(sc, n, rows_dev, max_rows, c->stream);
  efm::boundary_tally(a, count_dev, (efm::BoundaryResult*)result_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// the call's result, as the kernels left it at the head of the boundaries' scratch (synchronises); a tripped loop cap is an error of the call
int boundary_result_host(ef_ctx* c, const char* fn, ef_boundary_result* res_or_null) {
  ef_boundary_result res;
  EF_HIP(c, hipMemcpyAsync(&res, c->boundary.scratch.p, sizeof(res), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  if (res_or_null) *res_or_null = res;
  if (res.status) { c->err = std::string(fn) + ": internal error (a union-find loop exceeded its bound)"; return EF_EHIP; }
  return EF_OK;
}
}  // namespace

extern "C" {

int ef_default_boundary_params(ef_ctx* c, ef_boundary_params* p) {
  if (!c) { g_create_error = "ef_default_boundary_params: null context"; return EF_EINVAL; }
  if (!p) { c->err = "ef_default_boundary_params: null params"; return EF_EINVAL; }
  memset(p, 0, sizeof(*p));
  p->radius = 0.03f;
  p->cell = 0.03f;   // = radius, as the normals'
  p->min_conf = -1.0f;
  p->k = 12;
  p->min_neighbors = 5;
  p->normal_source = EF_BOUNDARY_STORED;
  p->line_ratio = 1e-4f;
  p->max_gap = 1.0f;   // a right angle: a definition
  p->min_size = 1u;
  p->max_size = 0u;
  return EF_OK;
}

// plain double on the host: needs neither a context nor a GPU
int ef_boundary_gap_from_angle(double radians, double* gap) {
  if (!gap) { g_create_error = "ef_boundary_gap_from_angle: null gap"; return EF_EINVAL; }
  const double quarter = 1.5707963267948966;   // pi / 2 rounded to double
  if (!(radians > 0.0 && radians < 4.0 * quarter)) { g_create_error = "ef_boundary_gap_from_angle: the angle must lie inside (0, 2 pi)"; return EF_EINVAL; }
  double n = std::floor(radians / quarter);
  if (n > 3.0) n = 3.0;
  const double b = radians - n * quarter, s = std::sin(b), co = std::cos(b);
  *gap = n + s / (s + co);
  return EF_OK;
}

int ef_map_boundaries_dev(ef_ctx* c, const ef_boundary_params* p, const ef_map_selection* among, float* gap_dev, uint32_t* count_dev,
                          uint8_t* status_dev, uint32_t* label_dev, uint32_t* size_dev, uint32_t max_rows, ef_boundary_result* result_dev) {
  int r = boundary_check(c, "ef_map_boundaries_dev", p, among, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_boundaries_dev");
  if (r != EF_OK) return r;
  return boundary_rows_enqueue(c, "ef_map_boundaries_dev", p, among, gap_dev, count_dev, status_dev, label_dev, size_dev, max_rows, result_dev);
}
int ef_map_boundaries(ef_ctx* c, const ef_boundary_params* p, const ef_map_selection* among, float* gap, uint32_t* count, uint8_t* status,
                      uint32_t* label, uint32_t* size, uint32_t max_rows, ef_boundary_result* result) {
  int r = boundary_check(c, "ef_map_boundaries", p, among, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_boundaries");
  if (r != EF_OK) return r;
  uint32_t n = 0;
  r = select_count(c, &n);
  if (r != EF_OK) return r;
  const size_t rows = std::min((size_t)max_rows, (size_t)n);
  r = c->stage.reserve(c, 16 + rows * 17, "boundary staging");   // 4 + 4 + 4 + 4 + 1 bytes per row
  if (r != EF_OK) return r;
  float* d_gap = c->stage.as<float>();
  uint32_t* d_count = (uint32_t*)(d_gap + rows);
  uint32_t* d_label = d_count + rows;
  uint32_t* d_size = d_label + rows;
  uint8_t* d_status = (uint8_t*)(d_size + rows);
  r = boundary_rows_enqueue(c, "ef_map_boundaries", p, among, gap ? d_gap : nullptr, count ? d_count : nullptr, status ? d_status : nullptr,
                            label ? d_label : nullptr, size ? d_size : nullptr, (uint32_t)rows, nullptr);
  if (r != EF_OK) return r;
  if (rows && gap) EF_HIP(c, hipMemcpyAsync(gap, d_gap, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && count) EF_HIP(c, hipMemcpyAsync(count, d_count, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && label) EF_HIP(c, hipMemcpyAsync(label, d_label, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && size) EF_HIP(c, hipMemcpyAsync(size, d_size, rows * 4, hipMemcpyDeviceToHost, c->stream));
  if (rows && status) EF_HIP(c, hipMemcpyAsync(status, d_status, rows, hipMemcpyDeviceToHost, c->stream));
  return boundary_result_host(c, "ef_map_boundaries", result);
}

int ef_map_boundaries_select_dev(ef_ctx* c, const ef_boundary_params* p, const ef_map_selection* among, int what, uint32_t* rows_dev,
                                 uint32_t max_rows, uint32_t* count_dev, ef_boundary_result* result_dev) {
  int r = boundary_check(c, "ef_map_boundaries_select_dev", p, among, count_dev, "count", what < 0 ? 0 : what, rows_dev, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_boundaries_select_dev");
  if (r != EF_OK) return r;
  return boundary_select_enqueue(c, "ef_map_boundaries_select_dev", p, among, what, rows_dev, max_rows, count_dev, result_dev);
}
int ef_map_boundaries_select(ef_ctx* c, const ef_boundary_params* p, const ef_map_selection* among, int what, uint32_t* rows, uint32_t max_rows,
                             uint32_t* count, ef_boundary_result* result) {
  int r = boundary_check(c, "ef_map_boundaries_select", p, among, count, "count", what < 0 ? 0 : what, rows, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_boundaries_select");
  if (r != EF_OK) return r;
  r = rows_list_host(c, "boundary staging", rows, max_rows, count, [&](uint32_t* d_rows, uint32_t cap_rows, uint32_t* d_count) {
    return boundary_select_enqueue(c, "ef_map_boundaries_select", p, among, what, d_rows, cap_rows, d_count, nullptr);
  });
  if (r != EF_OK) return r;
  return boundary_result_host(c, "ef_map_boundaries_select", result);
}

}  // extern "C"
