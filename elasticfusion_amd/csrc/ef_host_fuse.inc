// ================================================================================================
// Fuse surfels into the map (include/ef_hip.h: ef_default_fuse_params, ef_map_fuse[_dev]; kernels in ef_fuse.inc, the match, the append and their
// scratch of ef_host_insert.inc, the index of ef_host_query.inc, the counts of ef_host_select.inc; DESIGN.md §8g)
// ================================================================================================
namespace {
ef_insert_params fuse_as_insert(const ef_fuse_params* p) {
  ef_insert_params ip{};
  ip.gate = 1;
  ip.min_separation = p->min_separation;
  ip.min_conf = p->min_conf;
  ip.min_normal_cos = p->min_normal_cos;
  ip.init_time = p->init_time;
  ip.last_time = p->last_time;
  return ip;
}
// refusals before any GPU work: the insert's with the gate on, and append
int fuse_check(ef_ctx* c, const char* fn_, const float* rec, uint32_t n, const double* T, const ef_fuse_params* p, const ef_fuse_result* res) {
  std::string& err = c ? c->err : g_create_error;
  const std::string fn = fn_;
  if (!p) { err = fn + ": null params"; return EF_EINVAL; }
  if (!res) { err = fn + ": null result"; return EF_EINVAL; }
  if (p->append != 0 && p->append != 1) { err = fn + ": append must be 0 or 1"; return EF_EINVAL; }
  const ef_insert_params ip = fuse_as_insert(p);
  static const ef_insert_result result_stand_in{};
  return insert_check(c, fn_, rec, n, T, &ip, &result_stand_in);
}
// the fuse's own buffer for n0 map rows and n records: keys (8 n0) | match_row (4 n) | two sets of {chunk counts, chunk offsets, 4 words} |
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
  const size_t chunks = ((size_t)n + 255) / 256 + 1;
  const size_t b_key = up16((size_t)n0 * 8), b_match = up16((size_t)n * 4), b_count = up16((2 * chunks + 4) * sizeof(uint32_t)), b_out = up16(n);
  const size_t need = b_key + b_match + 2 * b_count + b_out;
  if (need > c->fuse.scratch.bytes) {   // (a quarter of slack: a growing map does not reallocate at every call)
    const int r = c->fuse.scratch.reserve(c, need + need / 4 + 4096, "fuse scratch");
    if (r != EF_OK) return r;
  }
  uint8_t* b = c->fuse.scratch.p;
  fs->key = (unsigned long long*)b;
  fs->match_row = (uint32_t*)(b + b_key);
  uint32_t* w = (uint32_t*)(b + b_key + b_match);
  fs->not_fused.chunk_count = w;
  fs->not_fused.chunk_offset = w + chunks;
  fs->not_fused_total = w + 2 * chunks;
  w = (uint32_t*)(b + b_key + b_match + b_count);
  fs->not_weightless.chunk_count = w;
  fs->not_weightless.chunk_offset = w + chunks;
  fs->not_weightless_total = w + 2 * chunks;
  fs->outcome = b + b_key + b_match + 2 * b_count;
  return EF_OK;
}
// The fuse, after the arguments were checked; DEVICE pointers.  Mirrors insert_run.
int fuse_run(ef_ctx* c, const char* fn, const float* rec_dev, uint32_t n, const double* T, const ef_fuse_params* p, ef_fuse_result* res,
             uint32_t* new_row_dev, uint32_t* match_row_dev, uint8_t* outcome_dev) {
  memset(res, 0, sizeof(*res));
  int r = capture_check(c, fn);
  if (r != EF_OK) return r;
  if (c->cfg.close_loops) {
    c->err = std::string(fn) + ": the context closes loops (close_loops = 1): its graph nodes, fern keyframes and pending end-of-frame record describe "
             "the unedited map";
    return EF_ESTATE;
  }
  EF_HIP(c, hipStreamSynchronize(c->stream));   // (as insert_run)
  if (c->labels.ids_on) {   // the rows created since the last ID-consuming call are numbered before the append: the zero suffix stays a suffix
    r = ids_prepare(c, fn);
    if (r != EF_OK) return r;
  }
  uint32_t n0 = 0;
  r = select_count(c, &n0);
  if (r != EF_OK) return r;
  res->count_after = n0;
  efm::MapFuseArgs f{};
  efm::InsertArgs& a = f.ins;
  if (n) {   // the index of the OLD map, through the query's own path
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
  a.gate = 1;
  a.min_normal_cos = p->min_normal_cos;
  a.init_time = p->init_time;
  a.last_time = p->last_time;
  a.count_before = n0;
  a.new_row = new_row_dev;
  efm::SelectScratch sc, dup_sc;
  uint32_t *total = nullptr, *dup_total = nullptr;
  r = insert_scratch(c, n, &sc, &total, &dup_sc, &dup_total);
  if (r != EF_OK) return r;
  FuseScratch fs;
  r = fuse_scratch(c, n0, n, &fs);
  if (r != EF_OK) return r;
  a.flags = sc.flags;
  a.dup = dup_sc.flags;
  a.chunk_offset = sc.chunk_offset;
  a.match_row = match_row_dev ? match_row_dev : fs.match_row;   // (the election reads it: the gate always writes one)
  f.key = fs.key;
  f.append = p->append;
  f.outcome = outcome_dev ? outcome_dev : fs.outcome;
  fs.not_fused.flags = fs.not_weightless.flags = f.outcome;
  efm::insert_gate(a, sc, total, dup_sc, dup_total, c->stream);
  if (n && n0) EF_HIP(c, hipMemsetAsync(f.key, 0xFF, (size_t)n0 * sizeof(unsigned long long), c->stream));
  efm::fuse_pick(f, c->stream);
  efm::fuse_outcome(f, c->stream);
  // (k_select_count counts the bytes that DIFFER from a value: n minus the count is the number of records with that outcome)
  efm::thin_count(fs.not_fused, n, efm::FUSE_FUSED, fs.not_fused_total, c->stream);
  efm::thin_count(fs.not_weightless, n, efm::FUSE_WEIGHTLESS, fs.not_weightless_total, c->stream);
  EF_HIP(c, hipGetLastError());
  // every count is known before anything is written
  uint32_t ins = 0, dup = 0, not_fused = 0, not_weightless = 0;
  EF_HIP(c, hipMemcpyAsync(&ins, total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipMemcpyAsync(&dup, dup_total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipMemcpyAsync(&not_fused, fs.not_fused_total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipMemcpyAsync(&not_weightless, fs.not_weightless_total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  if ((uint64_t)ins + dup > n || not_fused > n || not_weightless > n || (uint64_t)(n - not_fused) + (n - not_weightless) > dup) {
    c->err = std::string(fn) + ": internal error (the outcome counts do not add up)";
    return EF_EHIP;
  }
  res->fused = n - not_fused;
  res->weightless = n - not_weightless;
  res->absorbed = dup - res->fused - res->weightless;
  res->novel = ins;
  res->skipped = n - ins - dup;
  const uint32_t app = p->append ? ins : 0u;
  res->inserted = app;
  if ((uint64_t)n0 + app > c->capacity) {   // nothing has changed: map (no row was fused yet), count, prediction, index generation
    c->err = std::string(fn) + ": the map's count plus the records to append exceeds max_surfels";
    return EF_ECAPACITY;
  }
  ++c->map_gen;   // the index of the queries is stale
  if (res->fused || app) {
    // The merge writes rows BELOW n0 of maps[cur], the append rows from n0 on.  Pending z-buffer keys (im_pending) name rows of maps[im_map], the
    // buffer the last frame's clean() READ: maps[cur ^ 1] after the frame's swap.  Their only reader is im_materialise (the next frame's
    // association and keep-test tap keys that frame's own splats write, from maps[cur] as this call leaves it, and its association only CLEARS
    // the kept ones), so no key names a row written here (DESIGN.md §8g); should the two buffers ever coincide, the keys are resolved first.
    if (c->im_pending && c->im_map == c->cur) im_materialise(c);
    if (res->fused) efm::fuse_apply(f, c->stream);
  }
  if (app) {
    efm::insert_scatter(a, c->maps[c->cur], c->stream);
    hipLaunchKernelGGL(k_set_count, dim3(1), dim3(64), 0, c->stream, &c->st->map_counts[c->cur], n0 + app);
  } else if (new_row_dev && n) {
    EF_HIP(c, hipMemsetAsync(new_row_dev, 0xFF, (size_t)n * sizeof(uint32_t), c->stream));   // (no record was appended: every new_row is a miss)
  }
  EF_HIP(c, hipGetLastError());
  c->sel.count = n0 + app;
  c->sel.gen = c->map_gen;
  res->count_after = n0 + app;
  if (c->labels.C) {   // (as insert_run: the label calls' bound of the count restarts from the exact count)
    c->labels.known = n0 + app;
    c->labels.known_frames = c->stamps.size();
    c->labels.ev_pending = false;
  }
  if (c->tick > 1 || !c->stamps.empty()) {   // a frame or a restore has run: the next frame is tracked against a prediction of the edited map
    EF_HIP(c, hipMemsetAsync(&c->st->dense_count, 0, sizeof(unsigned), c->stream));
    r = do_predict(c);
    if (r != EF_OK) return r;
    EF_HIP(c, hipGetLastError());
  }
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}
}  // namespace

extern "C" {

int ef_default_fuse_params(ef_ctx* c, ef_fuse_params* p) {
  if (!c) { g_create_error = "ef_default_fuse_params: null context"; return EF_EINVAL; }
  if (!p) { c->err = "ef_default_fuse_params: null params"; return EF_EINVAL; }
  ef_insert_params ip;
  const int r = ef_default_insert_params(c, &ip);
  if (r != EF_OK) return r;
  memset(p, 0, sizeof(*p));
  p->min_separation = ip.min_separation;
  p->min_conf = ip.min_conf;
  p->min_normal_cos = ip.min_normal_cos;
  p->append = 1;
  p->init_time = ip.init_time;
  p->last_time = ip.last_time;
  return EF_OK;
}

int ef_map_fuse_dev(ef_ctx* c, const float* rec_dev, uint32_t n, const double* T, const ef_fuse_params* p, ef_fuse_result* res,
                    uint32_t* new_row_dev, uint32_t* match_row_dev, uint8_t* outcome_dev) {
  const int r = fuse_check(c, "ef_map_fuse_dev", rec_dev, n, T, p, res);
  if (r != EF_OK) return r;
  if (((uintptr_t)rec_dev & 15) != 0) { c->err = "ef_map_fuse_dev: surfels12_dev is not 16-byte aligned"; return EF_EINVAL; }
  DeviceGuard dg_(c);
  return fuse_run(c, "ef_map_fuse_dev", rec_dev, n, T, p, res, new_row_dev, match_row_dev, outcome_dev);
}
int ef_map_fuse(ef_ctx* c, const float* rec, uint32_t n, const double* T, const ef_fuse_params* p, ef_fuse_result* res, uint32_t* new_row,
                uint32_t* match_row, uint8_t* outcome) {
  int r = fuse_check(c, "ef_map_fuse", rec, n, T, p, res);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = capture_check(c, "ef_map_fuse");
  if (r != EF_OK) return r;
  const size_t o_new = (size_t)n * 48, o_match = o_new + (size_t)n * 4, o_out = o_match + (size_t)n * 4;
  r = c->stage.reserve(c, 16 + o_out + n, "fuse staging");
  if (r != EF_OK) return r;
  uint8_t* st = c->stage.p;
  if (n) EF_HIP(c, hipMemcpyAsync(st, rec, (size_t)n * 48, hipMemcpyHostToDevice, c->stream));
  r = fuse_run(c, "ef_map_fuse", (const float*)st, n, T, p, res, new_row ? (uint32_t*)(st + o_new) : nullptr,
               match_row ? (uint32_t*)(st + o_match) : nullptr, outcome ? st + o_out : nullptr);
  if (r != EF_OK) return r;
  if (n && new_row) EF_HIP(c, hipMemcpyAsync(new_row, st + o_new, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (n && match_row) EF_HIP(c, hipMemcpyAsync(match_row, st + o_match, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (n && outcome) EF_HIP(c, hipMemcpyAsync(outcome, st + o_out, n, hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}

}  // extern "C"
