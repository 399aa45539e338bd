// ================================================================================================
// Insert surfels into the map (include/ef_hip.h: ef_default_insert_params, ef_map_insert[_dev]; kernels in ef_insert.inc, the index of
// ef_host_query.inc, the count of ef_host_select.inc; DESIGN.md §8e)
// ================================================================================================
namespace {
// refusals before any GPU work: the arguments first, the context last (with a NULL context ef_last_error(NULL) names the argument)
int insert_check(ef_ctx* c, const char* fn_, const float* rec, uint32_t n, const double* T, const ef_insert_params* p, const ef_insert_result* res) {
  std::string& err = c ? c->err : g_create_error;
  const std::string fn = fn_;
  if (!p) { err = fn + ": null params"; return EF_EINVAL; }
  if (!res) { err = fn + ": null result"; return EF_EINVAL; }
  if (n && !rec) { err = fn + ": null surfels12"; return EF_EINVAL; }
  if (n > EF_INSERT_MAX_RECORDS) { err = fn + ": n exceeds EF_INSERT_MAX_RECORDS"; return EF_EINVAL; }   // (16 lanes per record: the gate's thread index is 32 bits)
  if (T && !finite16(T)) { err = fn + ": T has a non-finite entry"; return EF_EINVAL; }
  if (p->gate != 0 && p->gate != 1) { err = fn + ": gate must be 0 or 1"; return EF_EINVAL; }
  if (p->init_time < EF_INSERT_KEEP || p->last_time < EF_INSERT_KEEP) { err = fn + ": a time below EF_INSERT_KEEP"; return EF_EINVAL; }
  if (p->gate) {
    if (std::isnan(p->min_normal_cos)) { err = fn + ": min_normal_cos is NaN"; return EF_EINVAL; }
    static uint32_t row_stand_in;
    static const float point_stand_in[3] = {0.f, 0.f, 0.f};
    const QueryCall qc{fn_, point_stand_in, n, 1, p->min_separation, p->min_conf, &row_stand_in, nullptr, nullptr, nullptr, nullptr};
    return query_check(c, qc);   // (min_separation as max_dist, min_conf, the context, the ratio to the cell)
  }
  if (!c) { err = fn + ": null context"; return EF_EINVAL; }
  return EF_OK;
}
// two sets of {chunk counts, chunk offsets, 4 words (the total), one byte per record} for n records: the insert flags and the duplicate bytes
int insert_scratch(ef_ctx* c, uint32_t n, efm::SelectScratch* sc, uint32_t** total, efm::SelectScratch* dup_sc, uint32_t** dup_total) {
  if (n > c->ins.rows || !c->ins.scratch.p) {
    const size_t rows = ((size_t)n + (size_t)n / 4 + 1024 + 15) & ~(size_t)15;
    const size_t chunks = (rows + 255) / 256 + 1;
    c->ins.rows = 0;
    const int r = c->ins.scratch.reserve(c, 2 * ((2 * chunks + 4) * sizeof(uint32_t) + rows), "insert scratch");
    if (r != EF_OK) return r;
    c->ins.rows = rows;
  }
  const size_t rows = c->ins.rows, chunks = (rows + 255) / 256 + 1;
  uint32_t* w = c->ins.scratch.as<uint32_t>();
  sc->chunk_count = w;
  sc->chunk_offset = w + chunks;
  *total = w + 2 * chunks;
  w += 2 * chunks + 4;
  dup_sc->chunk_count = w;
  dup_sc->chunk_offset = w + chunks;
  *dup_total = w + 2 * chunks;
  sc->flags = (uint8_t*)(w + 2 * chunks + 4);
  dup_sc->flags = sc->flags + rows;
  return EF_OK;
}
// The insert, after the arguments were checked; DEVICE pointers.  Mirrors erase_run.
int insert_run(ef_ctx* c, const char* fn, const float* rec_dev, uint32_t n, const double* T, const ef_insert_params* p, ef_insert_result* res,
               uint32_t* new_row_dev, uint32_t* match_row_dev) {
  memset(res, 0, sizeof(*res));
  int r = capture_check(c, fn);
  if (r != EF_OK) return r;
  if (c->cfg.close_loops) {
    c->err = std::string(fn) + ": the context closes loops (close_loops = 1): its graph nodes, fern keyframes and pending end-of-frame record describe "
             "the unedited map";
    return EF_ESTATE;
  }
  EF_HIP(c, hipStreamSynchronize(c->stream));   // (as erase_run: frames, input stages and uploads are behind a synchronised stream)
  if (c->labels.ids_on) {   // the rows created since the last ID-consuming call are numbered before the append: the zero suffix stays a suffix
    r = ids_prepare(c, fn);
    if (r != EF_OK) return r;
  }
  uint32_t n0 = 0;
  r = select_count(c, &n0);
  if (r != EF_OK) return r;
  res->count_after = n0;
  efm::InsertArgs a{};
  if (p->gate && n) {   // the index of the OLD map, through the query's own path
    r = query_index(c, c->query.cell);
    if (r != EF_OK) return r;
    query_index_args(c, &a.q);
    a.q.max_dist = p->min_separation;
    a.q.r2 = p->min_separation * p->min_separation;
    a.q.min_conf = p->min_conf;
  }
  a.q.map = c->maps[c->cur];
  a.rec = (const float4*)rec_dev;
  a.n = n;
  a.moved = T != nullptr;
  if (T)
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) a.R[i * 3 + j] = (float)T[i * 4 + j];
      a.t[i] = (float)T[i * 4 + 3];
    }
  a.gate = p->gate;
  a.min_normal_cos = p->min_normal_cos;
  a.init_time = p->init_time;
  a.last_time = p->last_time;
  a.count_before = n0;
  a.match_row = match_row_dev;
  a.new_row = new_row_dev;
  efm::SelectScratch sc, dup_sc;
  uint32_t *total = nullptr, *dup_total = nullptr;
  r = insert_scratch(c, n, &sc, &total, &dup_sc, &dup_total);
  if (r != EF_OK) return r;
  a.flags = sc.flags;
  a.dup = dup_sc.flags;
  a.chunk_offset = sc.chunk_offset;
  efm::insert_gate(a, sc, total, dup_sc, dup_total, c->stream);
  EF_HIP(c, hipGetLastError());
  // the number to insert is known before anything is written
  uint32_t ins = 0, dup = 0;
  EF_HIP(c, hipMemcpyAsync(&ins, total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (p->gate) EF_HIP(c, hipMemcpyAsync(&dup, dup_total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  if ((uint64_t)ins + dup > n) { c->err = std::string(fn) + ": internal error (more records flagged than given)"; return EF_EHIP; }
  res->inserted = ins;
  res->duplicates = dup;
  res->skipped = n - ins - dup;
  if ((uint64_t)n0 + ins > c->capacity) {   // nothing has changed: map, count, prediction, index generation
    c->err = std::string(fn) + ": the map's count plus the records to insert exceeds max_surfels";
    return EF_ECAPACITY;
  }
  ++c->map_gen;   // the index of the queries is stale
  if (ins) {
    // The append writes rows >= n0 of maps[cur].  Pending z-buffer keys (im_pending) name rows of maps[im_map], the buffer the last frame's clean()
    // READ: that is maps[cur ^ 1] after the frame's swap, and stays it (an upload and this append write maps[cur]; an erase that swaps resolves
    // the keys first).  So no key names a row written here; should the two ever coincide, the keys are resolved before the rows change.
    if (c->im_pending && c->im_map == c->cur) im_materialise(c);
    efm::insert_scatter(a, c->maps[c->cur], c->stream);
    hipLaunchKernelGGL(k_set_count, dim3(1), dim3(64), 0, c->stream, &c->st->map_counts[c->cur], n0 + ins);
    EF_HIP(c, hipGetLastError());
  } else if (new_row_dev && n) {
    EF_HIP(c, hipMemsetAsync(new_row_dev, 0xFF, (size_t)n * sizeof(uint32_t), c->stream));   // (no record was inserted: every new_row is a miss)
  }
  c->sel.count = n0 + ins;
  c->sel.gen = c->map_gen;
  res->count_after = n0 + ins;
  if (c->labels.C) {   // the label calls' bound of the count (one image of new rows per frame) knows nothing of an append: it restarts from the exact count
    c->labels.known = n0 + ins;
    c->labels.known_frames = c->stamps.size();
    c->labels.ev_pending = false;
  }
  if (c->tick > 1 || !c->stamps.empty()) {   // a frame or a restore has run: the next frame is tracked against a prediction of the edited map
    EF_HIP(c, hipMemsetAsync(&c->st->dense_count, 0, sizeof(unsigned), c->stream));   // (as ef_predict: this prediction's tally replaces the last one's)
    r = do_predict(c);
    if (r != EF_OK) return r;
    EF_HIP(c, hipGetLastError());
  }
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}
}  // namespace

extern "C" {

int ef_default_insert_params(ef_ctx* c, ef_insert_params* p) {
  if (!c) { g_create_error = "ef_default_insert_params: null context"; return EF_EINVAL; }
  if (!p) { c->err = "ef_default_insert_params: null params"; return EF_EINVAL; }
  memset(p, 0, sizeof(*p));
  p->gate = 1;
  p->min_separation = 0.01f;
  p->min_conf = -1.0f;
  p->min_normal_cos = 0.5f;
  p->init_time = p->last_time = c->tick;
  return EF_OK;
}

int ef_map_insert_dev(ef_ctx* c, const float* rec_dev, uint32_t n, const double* T, const ef_insert_params* p, ef_insert_result* res,
                      uint32_t* new_row_dev, uint32_t* match_row_dev) {
  const int r = insert_check(c, "ef_map_insert_dev", rec_dev, n, T, p, res);
  if (r != EF_OK) return r;
  if (((uintptr_t)rec_dev & 15) != 0) { c->err = "ef_map_insert_dev: surfels12_dev is not 16-byte aligned"; return EF_EINVAL; }
  DeviceGuard dg_(c);
  return insert_run(c, "ef_map_insert_dev", rec_dev, n, T, p, res, new_row_dev, match_row_dev);
}
int ef_map_insert(ef_ctx* c, const float* rec, uint32_t n, const double* T, const ef_insert_params* p, ef_insert_result* res, uint32_t* new_row,
                  uint32_t* match_row) {
  int r = insert_check(c, "ef_map_insert", rec, n, T, p, res);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_insert");
  if (r != EF_OK) return r;
  const size_t o_new = (size_t)n * 48, o_match = o_new + (size_t)n * 4;
  r = c->stage.reserve(c, 16 + o_match + (size_t)n * 4, "insert staging");
  if (r != EF_OK) return r;
  uint8_t* st = c->stage.p;
  if (n) EF_HIP(c, hipMemcpyAsync(st, rec, (size_t)n * 48, hipMemcpyHostToDevice, c->stream));
  r = insert_run(c, "ef_map_insert", (const float*)st, n, T, p, res, new_row ? (uint32_t*)(st + o_new) : nullptr,
                 match_row ? (uint32_t*)(st + o_match) : nullptr);
  if (r != EF_OK) return r;
  if (n && new_row) EF_HIP(c, hipMemcpyAsync(new_row, st + o_new, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (n && match_row) EF_HIP(c, hipMemcpyAsync(match_row, st + o_match, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}

}  // extern "C"
