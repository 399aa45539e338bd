// ================================================================================================
// Carve free space (include/ef_hip.h: ef_default_carve_params, ef_map_carve_select[_dev], ef_map_carve[_dev]; the kernel in ef_carve.inc, the
// predicate, the lists and the erase of ef_host_select.inc; DESIGN.md §8h)
// ================================================================================================
namespace {
// refusals before any GPU work: the arguments first, the context last (with a NULL context ef_last_error(NULL) names the argument)
int carve_check(ef_ctx* c, const char* fn_, const ef_carve_params* p, const ef_carve_views* v, const ef_map_selection* among, const void* out,
                const char* out_name) {
  std::string& err = c ? c->err : g_create_error;
  const std::string fn = fn_;
  const char* why = nullptr;
  if (!p) why = "null params";
  else if (!v) why = "null views";
  else if (!out) { err = fn + ": null " + out_name; return EF_EINVAL; }
  else if (v->n < 1 || v->n > EF_CARVE_MAX_VIEWS) why = "views.n must lie in 1 .. EF_CARVE_MAX_VIEWS";
  else if (!v->T_wc16) why = "null views.T_wc16";
  else if (!v->depth) why = "null views.depth";
  if (why) { err = fn + ": " + why; return EF_EINVAL; }
  for (int k = 0; k < v->n; ++k)
    if (!finite16(v->T_wc16 + 16 * k)) { err = fn + ": views.T_wc16 has a non-finite entry"; return EF_EINVAL; }
  if (p->width < 1 || p->width > 4096 || p->height < 1 || p->height > 4096) why = "width and height must lie in 1 .. 4096";
  else if (!std::isfinite(p->fx) || !std::isfinite(p->fy) || !std::isfinite(p->cx) || !std::isfinite(p->cy)) why = "intrinsics must be finite";
  else if (!(p->margin >= 0.f) || !(p->margin_quad >= 0.f)) why = "margin and margin_quad must be non-negative numbers";
  else if (std::isnan(p->min_depth) || std::isnan(p->max_depth) || p->min_depth > p->max_depth) why = "min_depth <= max_depth must hold, neither NaN";
  else if (p->window < 0 || p->window > 2) why = "window must lie in 0 .. 2";
  else if (p->min_views < 1 || p->min_views > v->n) why = "min_views must lie in 1 .. views.n";
  if (why) { err = fn + ": " + why; return EF_EINVAL; }
  return among ? select_check(c, among, fn_) : EF_OK;
}
int carve_select_check(ef_ctx* c, const char* fn, const ef_carve_params* p, const ef_carve_views* v, const ef_map_selection* among,
                       const uint32_t* rows, uint32_t max_rows, const uint32_t* count) {
  const int r = carve_check(c, fn, p, v, among, count, "count");
  if (r != EF_OK) return r;
  if (max_rows && !rows) return select_null(c, fn, "rows");
  if (!c) return select_null(c, fn, "context");
  return EF_OK;
}
// T_cw of a view as the header forms it: the transpose and its product with t in double, each entry rounded to f32 once
void carve_Tcw(const double* T, float* out12) {
  const double t0 = T[3], t1 = T[7], t2 = T[11];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) out12[i * 4 + j] = (float)T[j * 4 + i];
    out12[i * 4 + 3] = (float)(-((T[0 * 4 + i] * t0 + T[1 * 4 + i] * t1) + T[2 * 4 + i] * t2));
  }
}
size_t carve_image_bytes(const ef_carve_params* p, const ef_carve_views* v) { return (size_t)v->n * p->width * p->height * sizeof(uint16_t); }
// the carve's own scratch for n rows: the selection's counts, offsets and total with the participant bytes, and the same three words sets for the
// kernel's tallies (participants, observed, free space)
struct CarveScratch {
  efm::SelectScratch part, tally[3];
  uint32_t *part_total = nullptr, *total[3] = {};
};
int carve_scratch(ef_ctx* c, uint32_t n, CarveScratch* cs) {
  if (n > c->carve.rows || !c->carve.scratch.p) {
    const size_t rows = std::min((size_t)c->capacity, (size_t)n + (size_t)n / 4 + 1024);
    c->carve.rows = 0;
    const int r = c->carve.scratch.reserve(c, 4 * Carver::scan_bytes(rows) + rows, "carve scratch");
    if (r != EF_OK) return r;
    c->carve.rows = rows;
  }
  Carver cv(c->carve.scratch);
  cs->part_total = cv.scan_words(c->carve.rows, &cs->part);
  for (int k = 0; k < 3; ++k) cs->total[k] = cv.scan_words(c->carve.rows, &cs->tally[k]);
  cs->part.flags = cv.take<uint8_t>(c->carve.rows);
  cs->tally[0].flags = cs->tally[1].flags = cs->tally[2].flags = nullptr;
  return EF_OK;
}
// Enqueues the byte of every one of the n rows of the map (removed[row] = 1 for a removed row, else 0), the vote bytes if asked for and, with
// tally given, the three totals (tally->total[0 .. 2]).  depth_dev: the views' images on the device.  Waits for the device only where the
// selection's preparation does.
int carve_mark(ef_ctx* c, const char* fn, const ef_carve_params* p, const ef_carve_views* v, const uint16_t* depth_dev,
               const ef_map_selection* among, uint32_t n, uint8_t* removed, uint8_t* votes, CarveScratch* tally) {
  efm::CarveArgs a{};
  CarveScratch own;
  CarveScratch* cs = tally ? tally : &own;
  if (among || tally) {
    const int r = carve_scratch(c, n, cs);
    if (r != EF_OK) return r;
  }
  if (among) {   // the participant bytes: the selection's own kernel, into the carve's scratch
    efm::SelectArgs sa;
    uint32_t n_sel = 0;
    const int r = select_prepare(c, among, fn, &sa, &n_sel);
    if (r != EF_OK) return r;
    if (n_sel != n) { c->err = std::string(fn) + ": internal error (the map count changed inside the call)"; return EF_EHIP; }
    efm::select_flags(sa, cs->part, cs->part_total, c->stream);
    a.part = cs->part.flags;
  }
  a.pos_conf = c->maps[c->cur].pos_conf;
  a.n = n;
  a.depth = depth_dev;
  a.n_views = v->n;
  a.width = p->width; a.height = p->height;
  a.fx = p->fx; a.fy = p->fy; a.cx = p->cx; a.cy = p->cy;
  a.min_depth = p->min_depth; a.max_depth = p->max_depth;
  a.margin = p->margin; a.margin_quad = p->margin_quad;
  a.window = p->window; a.min_views = p->min_views; a.protect = p->protect;
  a.removed = removed;
  a.votes = votes;
  if (tally) {
    a.tally = cs->tally[0].chunk_count;
    a.tally_stride = (unsigned)(cs->tally[1].chunk_count - cs->tally[0].chunk_count);
  }
  for (int k = 0; k < v->n; ++k) carve_Tcw(v->T_wc16 + 16 * k, a.Tcw[k]);
  efm::carve_flags(a, c->stream);
  if (tally)
    for (int k = 0; k < 3; ++k) efm::chunk_totals(cs->tally[k], n, cs->total[k], c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// device pointers; enqueues only (but for what carve_mark and the scratch need)
int carve_select_enqueue(ef_ctx* c, const char* fn, const ef_carve_params* p, const ef_carve_views* v, const uint16_t* depth_dev,
                         const ef_map_selection* among, uint32_t* rows_dev, uint32_t max_rows, uint32_t* count_dev, uint8_t* votes_dev) {
  uint32_t n = 0;
  int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::SelectScratch sc;
  uint32_t* total = nullptr;
  r = select_scratch(c, n, &sc, &total);
  if (r != EF_OK) return r;
  r = carve_mark(c, fn, p, v, depth_dev, among, n, sc.flags, votes_dev, nullptr);
  if (r != EF_OK) return r;
  efm::flags_count(sc, n, 0u, count_dev, c->stream);
  efm::select_rows(sc, n, rows_dev, max_rows, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// ef_map_carve / ef_map_carve_dev behind their checks: the erase with the flags 1 = removed, then the tallies
int carve_run(ef_ctx* c, const char* fn, const ef_carve_params* p, const ef_carve_views* v, bool depth_on_host, const ef_map_selection* among,
              ef_carve_result* res) {
  memset(res, 0, sizeof(*res));
  DeviceGuard dg_(c);
  uint32_t removed = 0;
  CarveScratch cs;
  int r = erase_run(c, fn, 1u, &removed, [&](uint32_t n, const efm::SelectScratch& sc, uint32_t* total) {
    // (the pointers of sc and total are into sel.scratch: growing the staging or the carve's own scratch moves none of them)
    const uint16_t* depth_dev = v->depth;
    if (depth_on_host) {
      const size_t bytes = carve_image_bytes(p, v);
      const int rg = c->stage.reserve(c, bytes, "carve staging");
      if (rg != EF_OK) return rg;
      EF_HIP(c, hipMemcpyAsync(c->stage.p, v->depth, bytes, hipMemcpyHostToDevice, c->stream));
      depth_dev = c->stage.as<uint16_t>();
    }
    const int rm = carve_mark(c, fn, p, v, depth_dev, among, n, sc.flags, nullptr, &cs);
    if (rm != EF_OK) return rm;
    efm::flags_count(sc, n, 1u, total, c->stream);
    return (int)EF_OK;
  });
  if (r != EF_OK) return r;
  uint32_t t[3] = {};   // (erase_run has synchronised behind the tallies)
  for (int k = 0; k < 3; ++k) EF_HIP(c, hipMemcpyAsync(&t[k], cs.total[k], sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  res->participants = t[0];
  res->observed = t[1];
  res->free_space = t[2];
  res->protected_ = t[2] - removed;
  res->removed = removed;
  res->count_after = c->sel.count;
  return EF_OK;
}
}  // namespace

extern "C" {

int ef_default_carve_params(ef_ctx* c, ef_carve_params* p) {
  if (!c) { g_create_error = "ef_default_carve_params: null context"; return EF_EINVAL; }
  if (!p) { c->err = "ef_default_carve_params: null params"; return EF_EINVAL; }
  memset(p, 0, sizeof(*p));
  p->width = c->cam.cols; p->height = c->cam.rows;
  p->fx = c->cam.fx; p->fy = c->cam.fy; p->cx = c->cam.cx; p->cy = c->cam.cy;
  p->min_depth = 0.3f;
  p->max_depth = c->cfg.depth_cut;
  p->margin = 0.02f;
  p->margin_quad = 0.0025f;
  p->window = 1;
  p->min_views = 1;
  p->protect = 1;
  return EF_OK;
}

int ef_map_carve_select_dev(ef_ctx* c, const ef_carve_params* p, const ef_carve_views* v, const ef_map_selection* among, uint32_t* rows_dev,
                            uint32_t max_rows, uint32_t* count_dev, uint8_t* votes_dev) {
  int r = carve_select_check(c, "ef_map_carve_select_dev", p, v, among, rows_dev, max_rows, count_dev);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_carve_select_dev");
  if (r != EF_OK) return r;
  return carve_select_enqueue(c, "ef_map_carve_select_dev", p, v, v->depth, among, rows_dev, max_rows, count_dev, votes_dev);
}
int ef_map_carve_select(ef_ctx* c, const ef_carve_params* p, const ef_carve_views* v, const ef_map_selection* among, uint32_t* rows,
                        uint32_t max_rows, uint32_t* count, uint8_t* votes) {
  int r = carve_select_check(c, "ef_map_carve_select", p, v, among, rows, max_rows, count);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_carve_select");
  if (r != EF_OK) return r;
  uint32_t n = 0;   // (the vote bytes are sized by the map count)
  r = select_count(c, &n);
  if (r != EF_OK) return r;
  // behind the list in the staging: the images, then the vote bytes
  const size_t img = (carve_image_bytes(p, v) + 15) & ~(size_t)15;
  uint8_t* d_votes = nullptr;
  r = rows_list_host(c, "carve staging", rows, max_rows, count, [&](uint32_t* d_rows, uint32_t cap_rows, uint32_t* d_count) {
    uint8_t* d_img = rows_list_extra(d_rows, cap_rows);
    if (votes) d_votes = d_img + img;
    EF_HIP(c, hipMemcpyAsync(d_img, v->depth, carve_image_bytes(p, v), hipMemcpyHostToDevice, c->stream));
    return carve_select_enqueue(c, "ef_map_carve_select", p, v, (const uint16_t*)d_img, among, d_rows, cap_rows, d_count, d_votes);
  }, img + (votes ? (size_t)n * 2 : 0));
  if (r != EF_OK) return r;
  if (votes && n) {
    EF_HIP(c, hipMemcpyAsync(votes, d_votes, (size_t)n * 2, hipMemcpyDeviceToHost, c->stream));
    EF_HIP(c, hipStreamSynchronize(c->stream));
  }
  return EF_OK;
}

int ef_map_carve_dev(ef_ctx* c, const ef_carve_params* p, const ef_carve_views* v, const ef_map_selection* among, ef_carve_result* res) {
  const int r = carve_check(c, "ef_map_carve_dev", p, v, among, res, "result");
  if (r != EF_OK) return r;
  if (!c) return select_null(c, "ef_map_carve_dev", "context");
  return carve_run(c, "ef_map_carve_dev", p, v, /*depth_on_host=*/false, among, res);
}
int ef_map_carve(ef_ctx* c, const ef_carve_params* p, const ef_carve_views* v, const ef_map_selection* among, ef_carve_result* res) {
  const int r = carve_check(c, "ef_map_carve", p, v, among, res, "result");
  if (r != EF_OK) return r;
  if (!c) return select_null(c, "ef_map_carve", "context");
  return carve_run(c, "ef_map_carve", p, v, /*depth_on_host=*/true, among, res);
}

}  // extern "C"
