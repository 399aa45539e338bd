// ================================================================================================
// Segment the map into planes by sequential RANSAC (include/ef_hip.h: ef_default_plane_params, ef_map_planes[_dev],
// ef_map_planes_select[_dev], ef_map_remove_planes; kernels in ef_planes.inc, the predicate, the lists and the erase of ef_host_select.inc;
// DESIGN.md §8k)
// ================================================================================================
namespace {
static_assert(sizeof(efm::PlaneResult) == sizeof(ef_plane_result) && offsetof(efm::PlaneResult, count_after) == offsetof(ef_plane_result, count_after) &&
                  sizeof(efm::PlaneModel) == sizeof(ef_plane_model) && offsetof(efm::PlaneModel, d) == offsetof(ef_plane_model, d) &&
                  offsetof(efm::PlaneModel, inliers) == offsetof(ef_plane_model, inliers) &&
                  offsetof(efm::PlaneModel, thickness) == offsetof(ef_plane_model, thickness) && EF_PLANE_NONE == efm::PLANE_NONE &&
                  EF_PLANE_MAX_PLANES == efm::PLANE_MAX_PLANES && EF_PLANE_MAX_HYPOTHESES == efm::PLANE_MAX_HYPOTHESES &&
                  EF_PLANE_AXIS_OFF == efm::PLANE_AXIS_OFF && EF_PLANE_AXIS_NORMAL == efm::PLANE_AXIS_NORMAL &&
                  EF_PLANE_AXIS_INPLANE == efm::PLANE_AXIS_INPLANE && EF_PLANES_ON == efm::PLANES_ON && EF_PLANES_OFF == efm::PLANES_OFF,
              "the kernels' models, result and constants are the header's");
// refusals before any GPU work: the arguments first, the context last (with a NULL context ef_last_error(NULL) names the argument).  out: the
// call's required output (null out_name: it has none); what / which: the calls without them pass EF_PLANES_ON and -1
int plane_check(ef_ctx* c, const char* fn_, const ef_plane_params* p, const ef_map_selection* among, int what, int which, const void* out,
                const char* out_name, const void* rows = nullptr, uint32_t max_rows = 0) {
  std::string& err = c ? c->err : g_create_error;
  const std::string fn = fn_;
  if (!p) { err = fn + ": null params"; return EF_EINVAL; }
  if (out_name && !out) { err = fn + ": null " + out_name; return EF_EINVAL; }
  if (!(p->distance > 0.f) || !std::isfinite(p->distance)) { err = fn + ": distance must be finite and positive"; return EF_EINVAL; }
  if (!(p->normal_cos >= 0.f && p->normal_cos <= 1.f)) { err = fn + ": normal_cos must lie in [0, 1]"; return EF_EINVAL; }
  if (!(p->axis_bound >= 0.f && p->axis_bound <= 1.f)) { err = fn + ": axis_bound must lie in [0, 1]"; return EF_EINVAL; }
  if (std::isnan(p->min_conf)) { err = fn + ": min_conf is NaN"; return EF_EINVAL; }
  if (p->hypotheses < 1u || p->hypotheses > (uint32_t)EF_PLANE_MAX_HYPOTHESES) {
    err = fn + ": hypotheses must lie in 1 .. " + std::to_string(EF_PLANE_MAX_HYPOTHESES);
    return EF_EINVAL;
  }
  if (p->max_planes < 1u || p->max_planes > (uint32_t)EF_PLANE_MAX_PLANES) {
    err = fn + ": max_planes must lie in 1 .. " + std::to_string(EF_PLANE_MAX_PLANES);
    return EF_EINVAL;
  }
  if (p->refine > 1u) { err = fn + ": refine must be 0 or 1"; return EF_EINVAL; }
  if (p->axis_mode > (uint32_t)EF_PLANE_AXIS_INPLANE) { err = fn + ": axis_mode must be one of EF_PLANE_AXIS_*"; return EF_EINVAL; }
  if (p->axis_mode != (uint32_t)EF_PLANE_AXIS_OFF) {
    const float l2 = (p->axis[0] * p->axis[0] + p->axis[1] * p->axis[1]) + p->axis[2] * p->axis[2];
    if (!(l2 >= 0.99f && l2 <= 1.01f)) { err = fn + ": axis must be a unit vector"; return EF_EINVAL; }
  }
  if (what != EF_PLANES_ON && what != EF_PLANES_OFF) { err = fn + ": what must be one of EF_PLANES_*"; return EF_EINVAL; }
  if (which < -1 || which >= (int)p->max_planes) { err = fn + ": which must lie in -1 .. max_planes - 1"; return EF_EINVAL; }
  if (max_rows && !rows) return select_null(c, fn_, "rows");
  if (among) {
    const int r = select_check(c, among, fn_);
    if (r != EF_OK) return r;
  }
  if (!c) return select_null(c, fn_, "context");
  return EF_OK;
}
// what the host reads back of a call: the head of the planes' scratch
struct PlaneHead {
  efm::PlaneResult res;
  efm::PlaneRound st;
  efm::PlaneModel models[EF_PLANE_MAX_PLANES];
};
// the planes' own scratch for n rows, carved into a
int plane_scratch(ef_ctx* c, uint32_t n, efm::PlaneArgs* a) {
  const size_t H = EF_PLANE_MAX_HYPOTHESES, P = EF_OUTLIER_SUM_LANES;
  if (n > c->planes.rows || !c->planes.scratch.p) {
    const size_t rows = std::min((size_t)c->capacity, (size_t)n + (size_t)n / 4 + 1024);
    c->planes.rows = 0;
    const int r = c->planes.scratch.reserve(c, sizeof(PlaneHead) + 64 + H * (2 * sizeof(uint32_t) + sizeof(float4)) + 9 * P * sizeof(double) +
                                                   rows * (sizeof(uint32_t) + 2 * sizeof(float4)) + Carver::scan_bytes(rows) + 2 * rows + 256,
                                            "plane scratch");
    if (r != EF_OK) return r;
    c->planes.rows = rows;
  }
  const size_t rows = c->planes.rows;
  Carver cv(c->planes.scratch);
  PlaneHead* head = cv.take<PlaneHead>(1);
  a->res = &head->res;
  a->st = &head->st;
  a->models = head->models;
  a->hyp = cv.take<float4>(H, 16);
  a->partial = cv.take<double>(9 * P);
  a->cpos = cv.take<float4>(rows, 16);
  a->cnrm = cv.take<float4>(rows, 16);
  a->counts = cv.take<uint32_t>(H);
  a->hyp_a = cv.take<uint32_t>(H);
  a->label = cv.take<uint32_t>(rows);
  a->M = cv.scan_words(rows, &a->sc);
  a->node = cv.take<uint8_t>(rows);
  a->part = cv.take<uint8_t>(rows);
  a->sc.flags = a->part;
  return EF_OK;
}
// Fills a for the n rows of the map and enqueues every round and the finish: the labels, the models and the result and (flags not null) the
// list's byte of every row.  Waits for the device only where the selection's preparation or a grown scratch do.
int plane_enqueue(ef_ctx* c, const char* fn, const ef_plane_params* p, const ef_map_selection* among, uint32_t n, int what, int which, uint8_t* flags,
                  efm::PlaneArgs* a) {
  *a = efm::PlaneArgs{};
  if (among) {   // the selection's bytes: its own kernel, into the planes' scratch; k_plane_init turns them into the node bytes in place
    efm::SelectArgs sa;
    uint32_t n_sel = 0;
    int r = select_prepare(c, among, fn, &sa, &n_sel);
    if (r != EF_OK) return r;
    if (n_sel != n) { c->err = std::string(fn) + ": internal error (the map count changed inside the call)"; return EF_EHIP; }
    r = plane_scratch(c, n, a);
    if (r != EF_OK) return r;
    efm::SelectScratch sel_sc = a->sc;
    sel_sc.flags = a->node;
    efm::select_flags(sa, sel_sc, a->M, c->stream);
    a->sel = a->node;
  } else {
    const int r = plane_scratch(c, n, a);
    if (r != EF_OK) return r;
  }
  a->map = c->maps[c->cur];
  a->n = n;
  a->distance = p->distance;
  a->normal_cos = p->normal_cos;
  a->min_conf = p->min_conf;
  a->H = p->hypotheses;
  a->seed = p->seed;
  a->max_planes = p->max_planes;
  a->min_inliers = p->min_inliers;
  a->refine = p->refine;
  a->axis_mode = (int)p->axis_mode;
  for (int i = 0; i < 3; ++i) a->axis[i] = p->axis[i];
  a->axis_bound = p->axis_bound;
  EF_HIP(c, hipMemsetAsync(c->planes.scratch.p, 0, sizeof(PlaneHead), c->stream));
  efm::plane_init(*a, c->stream);
  for (uint32_t k = 0; k < p->max_planes; ++k) efm::plane_round(*a, k, c->stream);
  efm::plane_finish(*a, what, which, flags, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// device pointers; enqueues only (but for what plane_enqueue needs)
int plane_labels_enqueue(ef_ctx* c, const char* fn, const ef_plane_params* p, const ef_map_selection* among, uint32_t* plane_dev, uint32_t max_rows,
                         ef_plane_model* models_dev, ef_plane_result* result_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::PlaneArgs a;
  r = plane_enqueue(c, fn, p, among, n, EF_PLANES_ON, -1, nullptr, &a);
  if (r != EF_OK) return r;
  efm::plane_split(a, plane_dev, max_rows, (efm::PlaneModel*)models_dev, (efm::PlaneResult*)result_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
int plane_select_enqueue(ef_ctx* c, const char* fn, const ef_plane_params* p, const ef_map_selection* among, int what, int which, uint32_t* rows_dev,
                         uint32_t max_rows, uint32_t* count_dev, ef_plane_model* models_dev, ef_plane_result* result_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::SelectScratch sc;
  uint32_t* total = nullptr;
  r = select_scratch(c, n, &sc, &total);
  if (r != EF_OK) return r;
  efm::PlaneArgs a;
  r = plane_enqueue(c, fn, p, among, n, what, which, sc.flags, &a);
  if (r != EF_OK) return r;
  efm::flags_count(sc, n, 0u, count_dev, c->stream);
  efm::select_rows(sc, n, rows_dev, max_rows, c->stream);
  efm::plane_split(a, nullptr, 0u, (efm::PlaneModel*)models_dev, (efm::PlaneResult*)result_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// the call's models and result, as the kernels left them at the head of the planes' scratch (synchronises)
int plane_result_host(ef_ctx* c, const ef_plane_params* p, ef_plane_model* models_or_null, ef_plane_result* res_or_null) {
  PlaneHead head;
  EF_HIP(c, hipMemcpyAsync(&head, c->planes.scratch.p, sizeof(head), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  if (res_or_null) memcpy(res_or_null, &head.res, sizeof(*res_or_null));
  if (models_or_null) memcpy(models_or_null, head.models, p->max_planes * sizeof(ef_plane_model));
  return EF_OK;
}
}  // namespace

extern "C" {

int ef_default_plane_params(ef_ctx* c, ef_plane_params* p) {
  if (!c) { g_create_error = "ef_default_plane_params: null context"; return EF_EINVAL; }
  if (!p) { c->err = "ef_default_plane_params: null params"; return EF_EINVAL; }
  memset(p, 0, sizeof(*p));
  p->distance = 0.01f;
  p->normal_cos = 0.f;
  p->min_conf = -1.0f;
  p->hypotheses = 1024u;
  p->seed = 0u;
  p->max_planes = 4u;
  p->min_inliers = 500u;
  p->refine = 1u;
  p->axis_mode = EF_PLANE_AXIS_OFF;
  p->axis[2] = 1.0f;
  p->axis_bound = 0.95f;
  return EF_OK;
}

int ef_map_planes_dev(ef_ctx* c, const ef_plane_params* p, const ef_map_selection* among, uint32_t* plane_dev, uint32_t max_rows,
                      ef_plane_model* models_dev, ef_plane_result* result_dev) {
  int r = plane_check(c, "ef_map_planes_dev", p, among, EF_PLANES_ON, -1, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_planes_dev");
  if (r != EF_OK) return r;
  return plane_labels_enqueue(c, "ef_map_planes_dev", p, among, plane_dev, max_rows, models_dev, result_dev);
}
int ef_map_planes(ef_ctx* c, const ef_plane_params* p, const ef_map_selection* among, uint32_t* plane, uint32_t max_rows, ef_plane_model* models,
                  ef_plane_result* result) {
  int r = plane_check(c, "ef_map_planes", p, among, EF_PLANES_ON, -1, nullptr, nullptr);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_planes");
  if (r != EF_OK) return r;
  uint32_t n = 0;
  r = select_count(c, &n);
  if (r != EF_OK) return r;
  const size_t rows = plane ? std::min((size_t)max_rows, (size_t)n) : 0;
  r = c->stage.reserve(c, 16 + rows * 4, "plane staging");
  if (r != EF_OK) return r;
  uint32_t* d_plane = c->stage.as<uint32_t>();
  r = plane_labels_enqueue(c, "ef_map_planes", p, among, rows ? d_plane : nullptr, (uint32_t)rows, nullptr, nullptr);
  if (r != EF_OK) return r;
  if (rows) EF_HIP(c, hipMemcpyAsync(plane, d_plane, rows * 4, hipMemcpyDeviceToHost, c->stream));
  return plane_result_host(c, p, models, result);
}

int ef_map_planes_select_dev(ef_ctx* c, const ef_plane_params* p, const ef_map_selection* among, int what, int which, uint32_t* rows_dev,
                             uint32_t max_rows, uint32_t* count_dev, ef_plane_model* models_dev, ef_plane_result* result_dev) {
  int r = plane_check(c, "ef_map_planes_select_dev", p, among, what, which, count_dev, "count", rows_dev, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_planes_select_dev");
  if (r != EF_OK) return r;
  return plane_select_enqueue(c, "ef_map_planes_select_dev", p, among, what, which, rows_dev, max_rows, count_dev, models_dev, result_dev);
}
int ef_map_planes_select(ef_ctx* c, const ef_plane_params* p, const ef_map_selection* among, int what, int which, uint32_t* rows, uint32_t max_rows,
                         uint32_t* count, ef_plane_model* models, ef_plane_result* result) {
  int r = plane_check(c, "ef_map_planes_select", p, among, what, which, count, "count", rows, max_rows);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_planes_select");
  if (r != EF_OK) return r;
  r = rows_list_host(c, "plane staging", rows, max_rows, count, [&](uint32_t* d_rows, uint32_t cap_rows, uint32_t* d_count) {
    return plane_select_enqueue(c, "ef_map_planes_select", p, among, what, which, d_rows, cap_rows, d_count, nullptr, nullptr);
  });
  if (r != EF_OK) return r;
  return plane_result_host(c, p, models, result);
}

int ef_map_remove_planes(ef_ctx* c, const ef_plane_params* p, const ef_map_selection* among, int which, ef_plane_model* models, ef_plane_result* res) {
  int r = plane_check(c, "ef_map_remove_planes", p, among, EF_PLANES_ON, which, res, "result");
  if (r != EF_OK) return r;
  memset(res, 0, sizeof(*res));
  DeviceGuard dg_(c);
  uint32_t removed = 0;
  // the flags are 1 for the REMOVED rows: the erase keeps those whose flag differs from 1
  r = erase_run(c, "ef_map_remove_planes", 1u, &removed, [&](uint32_t n, const efm::SelectScratch& sc, uint32_t* total) {
    // (the pointers of sc and total are into sel.scratch: growing the planes' own scratch moves none of them)
    efm::PlaneArgs a;
    int rm = plane_enqueue(c, "ef_map_remove_planes", p, among, n, EF_PLANES_ON, which, sc.flags, &a);
    if (rm != EF_OK) return rm;
    // the models and the counts of the map as it was, read while no row has changed yet
    rm = plane_result_host(c, p, models, res);
    if (rm != EF_OK) return rm;
    efm::flags_count(sc, n, 1u, total, c->stream);
    return (int)EF_OK;
  });
  if (r != EF_OK) return r;
  res->count_after = c->sel.count;
  return EF_OK;
}

}  // extern "C"
