// ================================================================================================
// Spatial index and nearest-surfel / kNN queries (include/ef_hip.h: ef_set_query_cell, ef_debug_query_lanes, ef_query_nearest[_dev],
// ef_query_knn[_dev]; kernels in ef_query.inc; DESIGN.md §8b)
// ================================================================================================
namespace {
struct QueryCall {
  const char* fn;
  const float* points;
  uint32_t n;
  int k;
  float max_dist, min_conf;
  uint32_t* row;
  uint32_t* id;
  float* dist2;
  float* plane;
  uint32_t* count;
};
// refusals before any GPU work
int query_check(ef_ctx* c, const QueryCall& q) {
  std::string& err = c ? c->err : g_create_error;
  const std::string fn = q.fn;
  if (q.k < 1 || q.k > 16) { err = fn + ": k must lie in 1 .. 16"; return EF_EINVAL; }
  if (!(q.max_dist > 0.f) || !std::isfinite(q.max_dist)) { err = fn + ": max_dist must be finite and positive"; return EF_EINVAL; }
  if (std::isnan(q.min_conf)) { err = fn + ": min_conf is NaN"; return EF_EINVAL; }
  if (q.n && !q.points) { err = fn + ": null points"; return EF_EINVAL; }
  if (!q.row) { err = fn + ": null row output"; return EF_EINVAL; }
  if (!c) { err = fn + ": null context"; return EF_EINVAL; }
  if (!(q.max_dist / c->query.cell <= (float)EF_QUERY_MAX_RATIO)) {
    err = fn + ": max_dist / cell must not exceed " + std::to_string(EF_QUERY_MAX_RATIO) + " (ef_set_query_cell)";
    return EF_EINVAL;
  }
  return EF_OK;
}
// the index for the current map at `cell` (the queries pass c->query.cell, a thin its own): reused while neither has changed, else rebuilt
// (waits for the device once: the count sizes it).  built_cell records what was built, so a caller with another cell rebuilds.
int query_index(ef_ctx* c, float cell) {
  if (c->query.gen == c->map_gen && c->query.built_cell == cell) return EF_OK;
  uint32_t n = 0;
  int r = read_count(c, &n);
  if (r != EF_OK) return r;
  const uint32_t nb = efm::query_buckets(n);
  c->query.gen = 0;   // nothing valid until the build below is enqueued
  r = c->query.cells.reserve(c, ((size_t)nb + 2 * ((size_t)nb / 1024 + 1)) * sizeof(uint32_t), "query cells");
  if (r != EF_OK) return r;
  if ((size_t)n * sizeof(float4) > c->query.sorted.bytes) {
    // sorted and rows are only ever reserved here, for the same cap records (rows.bytes == sorted.bytes / 4), so testing one covers both;
    // a failure leaves neither behind (and gen == 0: the next call comes back here)
    const size_t cap = std::min((size_t)c->capacity, (size_t)n + (size_t)n / 4 + 1024);
    r = c->query.sorted.reserve(c, cap * sizeof(float4), "query index");
    if (r == EF_OK) r = c->query.rows.reserve(c, cap * sizeof(uint32_t), "query index");
    if (r != EF_OK) { c->query.sorted.release(); c->query.rows.release(); return r; }
  }
  uint32_t* cells = c->query.cells.as<uint32_t>();
  EF_HIP(c, hipMemsetAsync(cells, 0, (size_t)nb * sizeof(uint32_t), c->stream));
  efm::query_build(c->maps[c->cur], n, 1.0f / cell, nb, cells, cells + nb, c->query.sorted.as<float4>(), c->query.rows.as<uint32_t>(), c->stream);
  EF_HIP(c, hipGetLastError());
  c->query.nb = nb;
  c->query.n = n;
  c->query.built_cell = cell;
  c->query.gen = c->map_gen;
  return EF_OK;
}
// the index half of a query's arguments (after query_index)
void query_index_args(const ef_ctx* c, efm::QueryArgs* a) {
  a->map = c->maps[c->cur];
  a->sorted = c->query.sorted.as<float4>();
  a->rows = c->query.rows.as<uint32_t>();
  a->cells = c->query.cells.as<uint32_t>();
  a->mask = c->query.nb - 1;
  a->n_sorted = c->query.n;
  a->inv_cell = 1.0f / c->query.built_cell;
}
// device pointers in q; enqueues only (but for a rebuild)
int query_enqueue(ef_ctx* c, const QueryCall& q) {
  int r = capture_check(c, q.fn);
  if (r != EF_OK) return r;
  if (q.id) {
    if (!c->labels.ids_on) { c->err = std::string(q.fn) + ": surfel IDs are off (ef_set_surfel_ids)"; return EF_ESTATE; }
    r = ids_prepare(c, q.fn);
    if (r != EF_OK) return r;
  }
  if (!q.n) return EF_OK;
  r = query_index(c, c->query.cell);
  if (r != EF_OK) return r;
  efm::QueryArgs a{};
  query_index_args(c, &a);
  a.points = q.points;
  a.n = q.n;
  a.k = q.k;
  a.max_dist = q.max_dist;
  a.r2 = q.max_dist * q.max_dist;
  a.min_conf = q.min_conf;
  a.row = q.row;
  a.dist2 = q.dist2;
  a.id = q.id;
  a.plane = q.plane;
  a.count = q.count;
  efm::query_run(a, q.k, c->query.lanes, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// host pointers in q: staged, synchronised
int query_host(ef_ctx* c, const QueryCall& q) {
  int r = capture_check(c, q.fn);
  if (r != EF_OK) return r;
  const size_t n = q.n, nk = n * (size_t)q.k;
  const size_t o_pts = 0, o_row = o_pts + n * 12, o_d2 = o_row + nk * 4, o_id = o_d2 + nk * 4, o_pl = o_id + n * 4, o_cnt = o_pl + n * 4;
  r = c->stage.reserve(c, o_cnt + n * 4 + 16, "query staging");
  if (r != EF_OK) return r;
  uint8_t* st = c->stage.p;
  QueryCall d = q;
  d.points = (const float*)(st + o_pts);
  d.row = (uint32_t*)(st + o_row);
  d.dist2 = q.dist2 ? (float*)(st + o_d2) : nullptr;
  d.id = q.id ? (uint32_t*)(st + o_id) : nullptr;
  d.plane = q.plane ? (float*)(st + o_pl) : nullptr;
  d.count = q.count ? (uint32_t*)(st + o_cnt) : nullptr;
  if (n) EF_HIP(c, hipMemcpyAsync(st + o_pts, q.points, n * 12, hipMemcpyHostToDevice, c->stream));
  r = query_enqueue(c, d);
  if (r != EF_OK) return r;
  if (n) {
    EF_HIP(c, hipMemcpyAsync(q.row, d.row, nk * 4, hipMemcpyDeviceToHost, c->stream));
    if (q.dist2) EF_HIP(c, hipMemcpyAsync(q.dist2, d.dist2, nk * 4, hipMemcpyDeviceToHost, c->stream));
    if (q.id) EF_HIP(c, hipMemcpyAsync(q.id, d.id, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (q.plane) EF_HIP(c, hipMemcpyAsync(q.plane, d.plane, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (q.count) EF_HIP(c, hipMemcpyAsync(q.count, d.count, n * 4, hipMemcpyDeviceToHost, c->stream));
  }
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}
}  // namespace
extern "C" {

int ef_set_query_cell(ef_ctx* c, float cell_m) {
  if (!(cell_m > 0.f) || !std::isfinite(cell_m) || !std::isfinite(1.0f / cell_m)) {
    (c ? c->err : g_create_error) = "ef_set_query_cell: cell_m must be finite and positive";
    return EF_EINVAL;
  }
  if (!c) { g_create_error = "ef_set_query_cell: null context"; return EF_EINVAL; }
  c->query.cell = cell_m;
  return EF_OK;
}
int ef_debug_query_lanes(ef_ctx* c, int lanes) {
  if (!c || (lanes != 0 && lanes != 1 && lanes != 8 && lanes != 16 && lanes != 64)) return EF_EINVAL;
  c->query.lanes = lanes;
  return EF_OK;
}
int ef_query_nearest_dev(ef_ctx* c, const float* points3, uint32_t n, float max_dist, float min_conf, uint32_t* row, uint32_t* id, float* dist2,
                         float* plane) {
  const QueryCall q{"ef_query_nearest_dev", points3, n, 1, max_dist, min_conf, row, id, dist2, plane, nullptr};
  const int r = query_check(c, q);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  return query_enqueue(c, q);
}
int ef_query_nearest(ef_ctx* c, const float* points3, uint32_t n, float max_dist, float min_conf, uint32_t* row, uint32_t* id, float* dist2,
                     float* plane) {
  const QueryCall q{"ef_query_nearest", points3, n, 1, max_dist, min_conf, row, id, dist2, plane, nullptr};
  const int r = query_check(c, q);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  return query_host(c, q);
}
int ef_query_knn_dev(ef_ctx* c, const float* points3, uint32_t n, int k, float max_dist, float min_conf, uint32_t* rows, float* dist2,
                     uint32_t* count) {
  const QueryCall q{"ef_query_knn_dev", points3, n, k, max_dist, min_conf, rows, nullptr, dist2, nullptr, count};
  const int r = query_check(c, q);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  return query_enqueue(c, q);
}
int ef_query_knn(ef_ctx* c, const float* points3, uint32_t n, int k, float max_dist, float min_conf, uint32_t* rows, float* dist2,
                 uint32_t* count) {
  const QueryCall q{"ef_query_knn", points3, n, k, max_dist, min_conf, rows, nullptr, dist2, nullptr, count};
  const int r = query_check(c, q);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  return query_host(c, q);
}

}  // extern "C"
