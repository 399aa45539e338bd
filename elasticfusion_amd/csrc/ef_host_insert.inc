// ================================================================================================
// Insert surfels into the map (include/ef_hip.h: ef_default_insert_params, ef_map_insert[_dev]) and the append path it shares with the fuse
// (ef_host_fuse.inc: ef_map_fuse[_dev]): append_run, append_host and both scratch layouts, the fuse's own included (FuseScratch, fuse_scratch:
// append_run carves it).  Kernels in ef_insert.inc and ef_fuse.inc, the index of ef_host_query.inc, the count and the edit frame
// of ef_host_select.inc; DESIGN.md §8e, §8g
// ================================================================================================
namespace {
// refusals before any GPU work: the arguments first, the context last (with a NULL context ef_last_error(NULL) names the argument)
int insert_check(ef_ctx* c, const char* fn_, bool rec_null, uint32_t n, const double* T, const ef_insert_params* p, bool res_null) {
  std::string& err = c ? c->err : g_create_error;
  const std::string fn = fn_;
  if (!p) { err = fn + ": null params"; return EF_EINVAL; }
  if (res_null) { err = fn + ": null result"; return EF_EINVAL; }
  if (n && rec_null) { err = fn + ": null surfels12"; return EF_EINVAL; }
  if (n > EF_INSERT_MAX_RECORDS) { err = fn + ": n exceeds EF_INSERT_MAX_RECORDS"; return EF_EINVAL; }   // (16 lanes per record: the gate's thread index is 32 bits)
  if (T && !finite16(T)) { err = fn + ": T has a non-finite entry"; return EF_EINVAL; }
  if (p->gate != 0 && p->gate != 1) { err = fn + ": gate must be 0 or 1"; return EF_EINVAL; }
  if (p->init_time < EF_INSERT_KEEP || p->last_time < EF_INSERT_KEEP) { err = fn + ": a time below EF_INSERT_KEEP"; return EF_EINVAL; }
  if (p->gate) {
    if (std::isnan(p->min_normal_cos)) { err = fn + ": min_normal_cos is NaN"; return EF_EINVAL; }
    uint32_t row_stand_in = 0;   // (the query's check asks only whether its points and its row output are there)
    const float point_stand_in[3] = {0.f, 0.f, 0.f};
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
    c->ins.rows = 0;
    const int r = c->ins.scratch.reserve(c, 2 * (Carver::scan_bytes(rows) + rows), "insert scratch");
    if (r != EF_OK) return r;
    c->ins.rows = rows;
  }
  Carver cv(c->ins.scratch);
  *total = cv.scan_words(c->ins.rows, sc);
  *dup_total = cv.scan_words(c->ins.rows, dup_sc);
  sc->flags = cv.take<uint8_t>(c->ins.rows);
  dup_sc->flags = cv.take<uint8_t>(c->ins.rows);
  return EF_OK;
}
// the merge's own buffer for n0 map rows and n records: keys (8 n0) | match_row (4 n) | two sets of {chunk counts, chunk offsets, 4 words} |
// outcome bytes (n); every part 16-byte aligned
struct FuseScratch {
  unsigned long long* key;
  uint32_t* match_row;
  efm::SelectScratch not_fused, not_weightless;   // their flags: the outcome bytes
  uint32_t *not_fused_total, *not_weightless_total;
  uint8_t* outcome;
};
int fuse_scratch(ef_ctx* c, uint32_t n0, uint32_t n, FuseScratch* fs) {
  const auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t need = up16((size_t)n0 * 8) + up16((size_t)n * 4) + 2 * up16(Carver::scan_bytes(n)) + up16(n);
  if (need > c->fuse.scratch.bytes) {   // (a quarter of slack: a growing map does not reallocate at every call)
    const int r = c->fuse.scratch.reserve(c, need + need / 4 + 4096, "fuse scratch");
    if (r != EF_OK) return r;
  }
  Carver cv(c->fuse.scratch);
  fs->key = cv.take<unsigned long long>(n0, 16);
  fs->match_row = cv.take<uint32_t>(n, 16);
  fs->not_fused_total = cv.scan_words(n, &fs->not_fused, 16);
  fs->not_weightless_total = cv.scan_words(n, &fs->not_weightless, 16);
  fs->outcome = cv.take<uint8_t>(n, 16);
  return EF_OK;
}
// One call of the append path: what ef_map_insert[_dev] and ef_map_fuse[_dev] differ by
struct AppendCall {
  const char* fn;
  const float* rec;
  uint32_t n;
  const double* T;
  ef_insert_params p;    // the gate (the fuse: always on) and the times
  bool merge;            // the fuse: one matched record per surfel is elected and merged into its row
  bool append;           // the flagged records are appended (the insert: always)
  uint32_t* new_row;     // n or null
  uint32_t* match_row;   // n or null (merge: the scratch's stands in, the election reads it)
  uint8_t* outcome;      // merge only: n or null (the scratch's stands in)
  ef_insert_result* insert_result;   // the caller's result: one of the two
  ef_fuse_result* fuse_result;
};
// both results are filled from the same counts (novel: flagged by the gate; dup: matched; fused + weightless <= dup, zero without the merge)
struct AppendCounts { uint32_t count_after, novel, dup, fused, weightless, skipped; };
void append_report(const AppendCall& q, const AppendCounts& k) {
  const uint32_t inserted = q.append ? k.novel : 0u;
  if (q.insert_result) *q.insert_result = ef_insert_result{inserted, k.dup, k.skipped, k.count_after};
  if (q.fuse_result) *q.fuse_result = ef_fuse_result{k.fused, k.dup - k.fused - k.weightless, k.weightless, k.novel, k.skipped, inserted, k.count_after};
}
// The append path, after the arguments were checked; DEVICE pointers in q.  Inside the edit frame of ef_host_select.inc.
int append_run(ef_ctx* c, const AppendCall& q) {
  AppendCounts k{};
  append_report(q, k);
  const uint32_t n = q.n;
  uint32_t n0 = 0;
  int r = edit_begin(c, q.fn, &n0);
  if (r != EF_OK) return r;
  k.count_after = n0;
  append_report(q, k);
  efm::MapFuseArgs f{};
  efm::InsertArgs& a = f.ins;
  if (q.p.gate && n) {   // the index of the OLD map, through the query's own path
    r = query_index(c, c->query.cell);
    if (r != EF_OK) return r;
    query_index_args(c, &a.q);
    a.q.max_dist = q.p.min_separation;
    a.q.r2 = q.p.min_separation * q.p.min_separation;
    a.q.min_conf = q.p.min_conf;
  }
  a.q.map = c->maps[c->cur];
  a.rec = (const float4*)q.rec;
  a.n = n;
  a.moved = q.T != nullptr;
  if (q.T) pose_Rt(q.T, a.R, a.t);
  a.gate = q.p.gate;
  a.min_normal_cos = q.p.min_normal_cos;
  a.init_time = q.p.init_time;
  a.last_time = q.p.last_time;
  a.count_before = n0;
  a.match_row = q.match_row;
  a.new_row = q.new_row;
  efm::SelectScratch sc, dup_sc;
  uint32_t *total = nullptr, *dup_total = nullptr;
  r = insert_scratch(c, n, &sc, &total, &dup_sc, &dup_total);
  if (r != EF_OK) return r;
  a.flags = sc.flags;
  a.dup = dup_sc.flags;
  a.chunk_offset = sc.chunk_offset;
  FuseScratch fs{};
  if (q.merge) {   // (its own buffer: growing it moves none of the insert scratch's pointers)
    r = fuse_scratch(c, n0, n, &fs);
    if (r != EF_OK) return r;
    if (!a.match_row) a.match_row = fs.match_row;   // (the election reads it: the gate always writes one)
    f.key = fs.key;
    f.append = q.append;
    f.outcome = q.outcome ? q.outcome : fs.outcome;
    fs.not_fused.flags = fs.not_weightless.flags = f.outcome;
  }
  efm::insert_gate(a, sc, total, dup_sc, dup_total, c->stream);
  if (q.merge) {
    if (n && n0) EF_HIP(c, hipMemsetAsync(f.key, 0xFF, (size_t)n0 * sizeof(unsigned long long), c->stream));
    efm::fuse_pick(f, c->stream);
    efm::fuse_outcome(f, c->stream);
    // (k_select_count counts the bytes that DIFFER from a value: n minus the count is the number of records with that outcome)
    efm::flags_count(fs.not_fused, n, efm::FUSE_FUSED, fs.not_fused_total, c->stream);
    efm::flags_count(fs.not_weightless, n, efm::FUSE_WEIGHTLESS, fs.not_weightless_total, c->stream);
  }
  EF_HIP(c, hipGetLastError());
  // every count is known before anything is written
  uint32_t ins = 0, dup = 0, not_fused = n, not_weightless = n;
  EF_HIP(c, hipMemcpyAsync(&ins, total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (q.p.gate) EF_HIP(c, hipMemcpyAsync(&dup, dup_total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (q.merge) {
    EF_HIP(c, hipMemcpyAsync(&not_fused, fs.not_fused_total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    EF_HIP(c, hipMemcpyAsync(&not_weightless, fs.not_weightless_total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  }
  EF_HIP(c, hipStreamSynchronize(c->stream));
  if ((uint64_t)ins + dup > n || not_fused > n || not_weightless > n || (uint64_t)(n - not_fused) + (n - not_weightless) > dup) {
    c->err = std::string(q.fn) + ": internal error (the outcome counts do not add up)";
    return EF_EHIP;
  }
  k = AppendCounts{n0, ins, dup, n - not_fused, n - not_weightless, n - ins - dup};
  append_report(q, k);
  const uint32_t app = q.append ? ins : 0u;
  if ((uint64_t)n0 + app > c->capacity) {   // nothing has changed: map (no row was fused yet), count, prediction, index generation
    c->err = std::string(q.fn) + ": the map's count plus the records to " + (q.merge ? "append" : "insert") + " exceeds max_surfels";
    return EF_ECAPACITY;
  }
  ++c->map_gen;   // the index of the queries is stale
  if (k.fused || app) {
    // The merge writes rows BELOW n0 of maps[cur], the append rows from n0 on.  Pending z-buffer keys (im_pending) name rows of maps[im_map], the
    // buffer the last frame's clean() READ: that is maps[cur ^ 1] after the frame's swap, and stays it (an upload and this call write maps[cur];
    // an erase that swaps resolves the keys first).  Their only reader is im_materialise (the next frame's association and keep-test tap keys
    // that frame's own splats write, from maps[cur] as this call leaves it, and its association only CLEARS the kept ones), so no key names a
    // row written here (DESIGN.md §8e, §8g); should the two buffers ever coincide, the keys are resolved before the rows change.
    if (c->im_pending && c->im_map == c->cur) im_materialise(c);
    if (k.fused) efm::fuse_apply(f, c->stream);
  }
  if (app) {
    efm::insert_scatter(a, c->maps[c->cur], c->stream);
    hipLaunchKernelGGL(k_set_count, dim3(1), dim3(64), 0, c->stream, &c->st->map_counts[c->cur], n0 + app);
  } else if (q.new_row && n) {
    EF_HIP(c, hipMemsetAsync(q.new_row, 0xFF, (size_t)n * sizeof(uint32_t), c->stream));   // (no record was appended: every new_row is a miss)
  }
  EF_HIP(c, hipGetLastError());
  k.count_after = n0 + app;
  append_report(q, k);
  return edit_commit(c, n0 + app, /*labels_restart=*/true);
}
// The host-pointer tier of both: rec | new_row | match_row | outcome (merge only) staged through c->stage (named `staging` in an allocation
// error), the append path on the staged copies, and what the caller asked for copied back.
int append_host(ef_ctx* c, const AppendCall& q, const char* staging) {
  int r = capture_check(c, q.fn);
  if (r != EF_OK) return r;
  const size_t n = q.n, o_new = n * 48, o_match = o_new + n * 4, o_out = o_match + n * 4;
  r = c->stage.reserve(c, 16 + o_out + (q.merge ? n : 0), staging);
  if (r != EF_OK) return r;
  uint8_t* st = c->stage.p;
  if (n) EF_HIP(c, hipMemcpyAsync(st, q.rec, n * 48, hipMemcpyHostToDevice, c->stream));
  AppendCall d = q;
  d.rec = (const float*)st;
  d.new_row = q.new_row ? (uint32_t*)(st + o_new) : nullptr;
  d.match_row = q.match_row ? (uint32_t*)(st + o_match) : nullptr;
  d.outcome = q.outcome ? st + o_out : nullptr;
  r = append_run(c, d);
  if (r != EF_OK) return r;
  if (n && q.new_row) EF_HIP(c, hipMemcpyAsync(q.new_row, d.new_row, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (n && q.match_row) EF_HIP(c, hipMemcpyAsync(q.match_row, d.match_row, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (n && q.outcome) EF_HIP(c, hipMemcpyAsync(q.outcome, d.outcome, n, hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}
AppendCall insert_call(const char* fn, const float* rec, uint32_t n, const double* T, const ef_insert_params* p, ef_insert_result* res,
                       uint32_t* new_row, uint32_t* match_row) {
  return AppendCall{fn, rec, n, T, *p, false, true, new_row, match_row, nullptr, res, nullptr};
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
  const int r = insert_check(c, "ef_map_insert_dev", !rec_dev, n, T, p, !res);
  if (r != EF_OK) return r;
  if (((uintptr_t)rec_dev & 15) != 0) { c->err = "ef_map_insert_dev: surfels12_dev is not 16-byte aligned"; return EF_EINVAL; }
  DeviceGuard dg_(c);
  return append_run(c, insert_call("ef_map_insert_dev", rec_dev, n, T, p, res, new_row_dev, match_row_dev));
}
int ef_map_insert(ef_ctx* c, const float* rec, uint32_t n, const double* T, const ef_insert_params* p, ef_insert_result* res, uint32_t* new_row,
                  uint32_t* match_row) {
  const int r = insert_check(c, "ef_map_insert", !rec, n, T, p, !res);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  return append_host(c, insert_call("ef_map_insert", rec, n, T, p, res, new_row, match_row), "insert staging");
}

}  // extern "C"
