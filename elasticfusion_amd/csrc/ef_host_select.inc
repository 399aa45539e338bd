// ================================================================================================
// Select, extract and erase surfels (include/ef_hip.h: ef_default_map_selection, ef_map_select[_dev], ef_map_gather[_dev], ef_map_erase,
// ef_map_erase_rows[_dev]; kernels in ef_select.inc; DESIGN.md §8d)
// ================================================================================================
namespace {
constexpr uint32_t SEL_KNOWN = EF_SEL_BOX | EF_SEL_CONF | EF_SEL_INIT_TIME | EF_SEL_LAST_TIME | EF_SEL_RADIUS | EF_SEL_ID | EF_SEL_LABEL | EF_SEL_INVERT;
// refusals before any GPU work: the selection first, the context last (with a NULL context ef_last_error(NULL) names the argument)
int select_check(ef_ctx* c, const ef_map_selection* s, const char* fn_) {
  std::string& err = c ? c->err : g_create_error;
  const std::string fn = fn_;
  if (!s) { err = fn + ": null selection"; return EF_EINVAL; }
  if (s->tests & ~SEL_KNOWN) { err = fn + ": unknown bits in tests"; return EF_EINVAL; }
  if (s->tests & EF_SEL_BOX) {
    if (!finite16(s->T_bw)) { err = fn + ": T_bw has a non-finite entry"; return EF_EINVAL; }
    for (int a = 0; a < 3; ++a)
      if (std::isnan(s->box_min[a]) || std::isnan(s->box_max[a])) { err = fn + ": a box bound is NaN"; return EF_EINVAL; }
  }
  if ((s->tests & EF_SEL_CONF) && (std::isnan(s->conf_min) || std::isnan(s->conf_max))) { err = fn + ": a confidence bound is NaN"; return EF_EINVAL; }
  if ((s->tests & EF_SEL_RADIUS) && (std::isnan(s->radius_min) || std::isnan(s->radius_max))) { err = fn + ": a radius bound is NaN"; return EF_EINVAL; }
  if (s->tests & EF_SEL_LABEL) {
    if (std::isnan(s->label_min_prob)) { err = fn + ": label_min_prob is NaN"; return EF_EINVAL; }
    if (s->label_class < 0 || (c && c->labels.C && s->label_class >= c->labels.C)) { err = fn + ": label_class outside 0 .. C-1"; return EF_EINVAL; }
  }
  return EF_OK;
}
int select_null(ef_ctx* c, const char* fn, const char* what) {
  (c ? c->err : g_create_error) = std::string(fn) + ": null " + what;
  return EF_EINVAL;
}
// the map count without a device round trip while no call that can change the map has run since it was read
int select_count(ef_ctx* c, uint32_t* n) {
  if (c->sel.gen != c->map_gen) {
    const int r = read_count(c, &c->sel.count);
    if (r != EF_OK) return r;
    c->sel.gen = c->map_gen;
  }
  *n = c->sel.count;
  return EF_OK;
}
// flags, chunk counts and offsets for n rows, and the word the scan leaves the total in
int select_scratch(ef_ctx* c, uint32_t n, efm::SelectScratch* sc, uint32_t** total) {
  if (n > c->sel.rows || !c->sel.scratch.p) {
    const size_t P = (size_t)c->cam.cols * c->cam.rows;
    const size_t rows = std::min((size_t)c->capacity, (size_t)n + std::max((size_t)n / 4, P));
    c->sel.rows = 0;
    const int r = c->sel.scratch.reserve(c, Carver::scan_bytes(rows) + rows, "selection scratch");
    if (r != EF_OK) return r;
    c->sel.rows = rows;
  }
  Carver cv(c->sel.scratch);
  *total = cv.scan_words(c->sel.rows, sc);
  sc->flags = cv.take<uint8_t>(c->sel.rows);
  return EF_OK;
}
// state refusals, ID numbering and label alignment of a selection, then its device form for the n rows of the map
int select_prepare(ef_ctx* c, const ef_map_selection* s, const char* fn, efm::SelectArgs* a, uint32_t* n) {
  if ((s->tests & EF_SEL_ID) && !c->labels.ids_on) { c->err = std::string(fn) + ": EF_SEL_ID while surfel IDs are off (ef_set_surfel_ids)"; return EF_ESTATE; }
  if ((s->tests & EF_SEL_LABEL) && !c->labels.C) { c->err = std::string(fn) + ": EF_SEL_LABEL while labels are off (ef_enable_labels)"; return EF_ESTATE; }
  int r;
  if (s->tests & EF_SEL_LABEL) r = labels_begin(c, fn);   // (numbers the new rows too)
  else if (s->tests & EF_SEL_ID) r = ids_prepare(c, fn);
  else r = EF_OK;
  if (r != EF_OK) return r;
  r = select_count(c, n);
  if (r != EF_OK) return r;
  *a = efm::SelectArgs{};
  a->map = c->maps[c->cur];
  a->n = *n;
  a->tests = s->tests & ~EF_SEL_INVERT;
  a->invert = (s->tests & EF_SEL_INVERT) ? 1u : 0u;
  pose_Rt(s->T_bw, a->R, a->t);
  for (int i = 0; i < 3; ++i) {
    a->box_min[i] = s->box_min[i];
    a->box_max[i] = s->box_max[i];
  }
  a->conf_min = s->conf_min; a->conf_max = s->conf_max;
  a->init_min = (float)s->init_time_min; a->init_max = (float)s->init_time_max;
  a->last_min = (float)s->last_time_min; a->last_max = (float)s->last_time_max;
  a->radius_min = s->radius_min; a->radius_max = s->radius_max;
  a->id_min = s->id_min; a->id_max = s->id_max;
  a->tab = (s->tests & EF_SEL_LABEL) ? c->labels.tab[c->labels.cur] : nullptr;
  a->C = c->labels.C;
  a->label_class = s->label_class;
  a->label_min_prob = s->label_min_prob;
  return EF_OK;
}
// device pointers; enqueues only (but for what select_prepare and the scratch need)
int select_enqueue(ef_ctx* c, const ef_map_selection* s, const char* fn, uint32_t* rows_dev, uint32_t max_rows, uint32_t* count_dev) {
  efm::SelectArgs a;
  uint32_t n = 0;
  int r = select_prepare(c, s, fn, &a, &n);
  if (r != EF_OK) return r;
  efm::SelectScratch sc;
  uint32_t* total = nullptr;
  r = select_scratch(c, n, &sc, &total);
  if (r != EF_OK) return r;
  efm::select_flags(a, sc, count_dev, c->stream);
  efm::select_rows(sc, n, rows_dev, max_rows, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
int gather_enqueue(ef_ctx* c, const char* fn, const uint32_t* rows_dev, uint32_t n_rows, float* out_dev) {
  if (c->labels.ids_on) {
    const int ri = ids_prepare(c, fn);
    if (ri != EF_OK) return ri;
  }
  if (!n_rows) return EF_OK;
  uint32_t n = 0;
  const int r = select_count(c, &n);
  if (r != EF_OK) return r;
  efm::map_gather(c->maps[c->cur], n, rows_dev, n_rows, out_dev, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// ---- The edit frame: the protocol every call that changes the map's rows goes through (DESIGN.md §6).  A verb calls edit_begin, enqueues its
// own work, reads its counts in one synchronise, refuses what it must while nothing has changed, then bumps map_gen, resolves pending z-buffer
// keys before it writes rows, and calls edit_commit.  erase_run and append_run (ef_host_insert.inc) are the only callers.
// Begin: the refusals, the wait for everything in flight, the ID numbering, the map's count.
int edit_begin(ef_ctx* c, const char* fn, uint32_t* n0) {
  int r = capture_check(c, fn);
  if (r != EF_OK) return r;
  if (c->cfg.close_loops) {
    c->err = std::string(fn) + ": the context closes loops (close_loops = 1): its graph nodes, fern keyframes and pending end-of-frame record describe "
             "the unedited map";
    return EF_ESTATE;
  }
  // (every frame, every input stage on in_stream that the last frame's events ordered behind it, and every upload has been waited for by what
  // follows a synchronised stream: no new event logic)
  EF_HIP(c, hipStreamSynchronize(c->stream));
  // the rows created since the last ID-consuming call are numbered before any row can go or come: the counter then stands above every ID handed
  // out (an erase), and the zero suffix stays a suffix (an append)
  if (c->labels.ids_on) {
    r = ids_prepare(c, fn);
    if (r != EF_OK) return r;
  }
  return select_count(c, n0);
}
// Commit: the map now holds `count` rows, and map_gen was bumped since edit_begin.  labels_restart: the label calls' bound of the count (one image
// of new rows per frame) knows nothing of rows that were appended and restarts from the exact count; an erase leaves it alone (fewer rows: the
// bound still holds).
int edit_commit(ef_ctx* c, uint32_t count, bool labels_restart) {
  c->sel.count = count;
  c->sel.gen = c->map_gen;
  if (labels_restart && c->labels.C) {
    c->labels.known = count;
    c->labels.known_frames = c->stamps.size();
    c->labels.ev_pending = false;
  }
  if (c->tick > 1 || !c->stamps.empty()) {   // a frame or a restore has run: the next frame is tracked against a prediction of the edited map
    EF_HIP(c, hipMemsetAsync(&c->st->dense_count, 0, sizeof(unsigned), c->stream));   // (as ef_predict: this prediction's tally replaces the last one's)
    const int r = do_predict(c);
    if (r != EF_OK) return r;
    EF_HIP(c, hipGetLastError());
  }
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}
// The erase, after the arguments were checked.  mark(n, sc, total) enqueues the flags, the chunk counts and offsets of the KEPT rows (those whose
// flag differs from `flip`) and their number into *total.
template <typename Mark>
int erase_run(ef_ctx* c, const char* fn, unsigned flip, uint32_t* removed, Mark mark) {
  uint32_t n = 0;
  int r = edit_begin(c, fn, &n);
  if (r != EF_OK) return r;
  efm::SelectScratch sc;
  uint32_t* total = nullptr;
  r = select_scratch(c, n, &sc, &total);
  if (r != EF_OK) return r;
  r = mark(n, sc, total);
  if (r != EF_OK) return r;
  EF_HIP(c, hipGetLastError());
  uint32_t kept = 0;
  EF_HIP(c, hipMemcpyAsync(&kept, total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  if (kept > n) { c->err = std::string(fn) + ": internal error (more rows kept than the map holds)"; return EF_EHIP; }
  ++c->map_gen;   // the index of the queries is stale
  if (kept < n) {
    // after a keyed frame maps[cur ^ 1] is the buffer the kept z-buffer keys name: the four index maps are resolved from it before it is
    // overwritten, whichever buffer the keys name (unconditionally: the compaction's target is the other buffer, and the swap follows)
    im_materialise(c);
    efm::select_compact(sc, n, flip, c->maps[c->cur], c->maps[c->cur ^ 1], c->stream);
    hipLaunchKernelGGL(k_set_count, dim3(1), dim3(64), 0, c->stream, &c->st->map_counts[c->cur ^ 1], kept);
    EF_HIP(c, hipGetLastError());
    c->cur ^= 1;
  }
  r = edit_commit(c, kept, /*labels_restart=*/false);
  if (r != EF_OK) return r;
  if (removed) *removed = n - kept;
  return EF_OK;
}
// The "list of rows" host tier of ef_map_select and ef_map_thin_select: enqueue(rows_dev, max_rows, count_dev) is the _dev tier's work into the
// staging (named `staging` in an allocation error); the count and the first min(count, max_rows) rows are copied out.  `extra` bytes behind the
// list (rows_list_extra: 16-byte aligned) are the caller's own: the staging is reserved once, for both.
inline uint8_t* rows_list_extra(uint32_t* d_rows, uint32_t cap_rows) { return (uint8_t*)d_rows + (((size_t)cap_rows * 4 + 15) & ~(size_t)15); }
template <typename Enqueue>
int rows_list_host(ef_ctx* c, const char* staging, uint32_t* rows, uint32_t max_rows, uint32_t* count, Enqueue enqueue, size_t extra = 0) {
  // (the list is never longer than the map: the staging is sized by the capacity at most)
  const size_t cap_rows = std::min((size_t)max_rows, (size_t)c->capacity);
  int r = c->stage.reserve(c, extra ? 16 + ((cap_rows * 4 + 15) & ~(size_t)15) + extra : 16 + cap_rows * 4, staging);
  if (r != EF_OK) return r;
  uint32_t* d_count = c->stage.as<uint32_t>();
  uint32_t* d_rows = (uint32_t*)(c->stage.p + 16);
  r = enqueue(d_rows, (uint32_t)cap_rows, d_count);
  if (r != EF_OK) return r;
  EF_HIP(c, hipMemcpyAsync(count, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  const size_t got = std::min((size_t)*count, cap_rows);
  if (got) {
    EF_HIP(c, hipMemcpyAsync(rows, d_rows, got * 4, hipMemcpyDeviceToHost, c->stream));
    EF_HIP(c, hipStreamSynchronize(c->stream));
  }
  return EF_OK;
}
}  // namespace

extern "C" {

void ef_default_map_selection(ef_map_selection* s) {
  if (!s) return;
  memset(s, 0, sizeof(*s));
  const float inf = std::numeric_limits<float>::infinity();
  s->T_bw[0] = s->T_bw[5] = s->T_bw[10] = s->T_bw[15] = 1.0;
  for (int a = 0; a < 3; ++a) { s->box_min[a] = -inf; s->box_max[a] = inf; }
  s->conf_min = -inf; s->conf_max = inf;
  s->init_time_min = s->last_time_min = std::numeric_limits<int>::min();
  s->init_time_max = s->last_time_max = std::numeric_limits<int>::max();
  s->radius_min = -inf; s->radius_max = inf;
  s->id_min = 0u; s->id_max = 0xFFFFFFFFu;
  s->label_class = 0;
  s->label_min_prob = -inf;
}

int ef_map_select_dev(ef_ctx* c, const ef_map_selection* s, uint32_t* rows_dev, uint32_t max_rows, uint32_t* count_dev) {
  int r = select_check(c, s, "ef_map_select_dev");
  if (r != EF_OK) return r;
  if (max_rows && !rows_dev) return select_null(c, "ef_map_select_dev", "rows");
  if (!count_dev) return select_null(c, "ef_map_select_dev", "count");
  if (!c) return select_null(c, "ef_map_select_dev", "context");
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_select_dev");
  if (r != EF_OK) return r;
  return select_enqueue(c, s, "ef_map_select_dev", rows_dev, max_rows, count_dev);
}
int ef_map_select(ef_ctx* c, const ef_map_selection* s, uint32_t* rows, uint32_t max_rows, uint32_t* count) {
  int r = select_check(c, s, "ef_map_select");
  if (r != EF_OK) return r;
  if (max_rows && !rows) return select_null(c, "ef_map_select", "rows");
  if (!count) return select_null(c, "ef_map_select", "count");
  if (!c) return select_null(c, "ef_map_select", "context");
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_select");
  if (r != EF_OK) return r;
  return rows_list_host(c, "selection staging", rows, max_rows, count, [&](uint32_t* d_rows, uint32_t cap_rows, uint32_t* d_count) {
    return select_enqueue(c, s, "ef_map_select", d_rows, cap_rows, d_count);
  });
}

int ef_map_gather_dev(ef_ctx* c, const uint32_t* rows_dev, uint32_t n, float* out_dev) {
  if (n && !rows_dev) return select_null(c, "ef_map_gather_dev", "rows");
  if (n && !out_dev) return select_null(c, "ef_map_gather_dev", "surfels12");
  if (!c) return select_null(c, "ef_map_gather_dev", "context");
  DeviceGuard dg_(c);
  const int r = capture_check(c, "ef_map_gather_dev");
  if (r != EF_OK) return r;
  return gather_enqueue(c, "ef_map_gather_dev", rows_dev, n, out_dev);
}
int ef_map_gather(ef_ctx* c, const uint32_t* rows, uint32_t n, float* out) {
  if (n && !rows) return select_null(c, "ef_map_gather", "rows");
  if (n && !out) return select_null(c, "ef_map_gather", "surfels12");
  if (!c) return select_null(c, "ef_map_gather", "context");
  DeviceGuard dg_(c);
  int r = capture_check(c, "ef_map_gather");
  if (r != EF_OK) return r;
  const size_t o_out = ((size_t)n * 4 + 15) & ~(size_t)15;
  r = c->stage.reserve(c, 16 + o_out + (size_t)n * 48, "selection staging");
  if (r != EF_OK) return r;
  uint32_t* d_rows = c->stage.as<uint32_t>();
  float* d_out = (float*)(c->stage.p + o_out);
  if (n) EF_HIP(c, hipMemcpyAsync(d_rows, rows, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  r = gather_enqueue(c, "ef_map_gather", d_rows, n, d_out);
  if (r != EF_OK) return r;
  if (n) EF_HIP(c, hipMemcpyAsync(out, d_out, (size_t)n * 48, hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}

int ef_map_erase(ef_ctx* c, const ef_map_selection* s, uint32_t* removed) {
  const int r = select_check(c, s, "ef_map_erase");
  if (r != EF_OK) return r;
  if (!c) return select_null(c, "ef_map_erase", "context");
  DeviceGuard dg_(c);
  // the flags are those of the KEPT rows: the selection with its inversion toggled
  ef_map_selection keep = *s;
  keep.tests ^= EF_SEL_INVERT;
  return erase_run(c, "ef_map_erase", 0u, removed, [&](uint32_t, const efm::SelectScratch& sc, uint32_t* total) {
    efm::SelectArgs a;
    uint32_t n = 0;
    const int rp = select_prepare(c, &keep, "ef_map_erase", &a, &n);
    if (rp != EF_OK) return rp;
    efm::select_flags(a, sc, total, c->stream);
    return (int)EF_OK;
  });
}
int ef_map_erase_rows_dev(ef_ctx* c, const uint32_t* rows_dev, uint32_t n_rows, uint32_t* removed) {
  if (n_rows && !rows_dev) return select_null(c, "ef_map_erase_rows_dev", "rows");
  if (!c) return select_null(c, "ef_map_erase_rows_dev", "context");
  DeviceGuard dg_(c);
  return erase_run(c, "ef_map_erase_rows_dev", 1u, removed, [&](uint32_t n, const efm::SelectScratch& sc, uint32_t* total) {
    efm::select_mark_rows(rows_dev, n_rows, n, 1u, sc, total, c->stream);
    return (int)EF_OK;
  });
}
int ef_map_erase_rows(ef_ctx* c, const uint32_t* rows, uint32_t n_rows, uint32_t* removed) {
  if (n_rows && !rows) return select_null(c, "ef_map_erase_rows", "rows");
  if (!c) return select_null(c, "ef_map_erase_rows", "context");
  DeviceGuard dg_(c);
  return erase_run(c, "ef_map_erase_rows", 1u, removed, [&](uint32_t n, const efm::SelectScratch& sc, uint32_t* total) {
    // (the pointers of sc and total are into sel.scratch, never into the staging: growing it here moves none of them)
    const int rg = c->stage.reserve(c, 16 + (size_t)n_rows * 4, "selection staging");
    if (rg != EF_OK) return rg;
    if (n_rows) EF_HIP(c, hipMemcpyAsync(c->stage.p, rows, (size_t)n_rows * 4, hipMemcpyHostToDevice, c->stream));
    efm::select_mark_rows(c->stage.as<uint32_t>(), n_rows, n, 1u, sc, total, c->stream);
    return (int)EF_OK;
  });
}

}  // extern "C"
