// ================================================================================================
// Stable surfel IDs and per-surfel label fusion (include/ef_hip.h: ef_set_surfel_ids, ef_get_surfel_ids, ef_enable_labels, ef_set_labels,
// ef_get_labels, ef_fuse_labels[_dev], ef_render_labels[_dev]; kernels in ef_labels.inc; DESIGN.md §8a).  ids_prepare and ids_uploaded, which
// the map's download and upload need too, are in ef_context.hip.
// ================================================================================================
namespace {
// An upper bound of the map count without a device round trip: the count a label call left behind (once its event has completed) or an
// upload set, plus one image of new surfels per frame since (the first frame seeds at most width x height, fusion appends fewer).
size_t labels_count_bound(ef_ctx* c) {
  if (c->labels.ev_pending && hipEventQuery(c->labels.ev) == hipSuccess) {
    c->labels.known = *c->labels.count_h;
    c->labels.known_frames = c->labels.ev_frames;
    c->labels.ev_pending = false;
  }
  const size_t P = (size_t)c->cam.cols * c->cam.rows;
  const size_t b = c->labels.known + (c->stamps.size() - c->labels.known_frames) * P;
  return b < c->capacity ? b : c->capacity;
}
void labels_free(ef_ctx* c) {
  for (int k = 0; k < 2; ++k) {
    if (c->labels.tab[k]) (void)hipFree(c->labels.tab[k]);
    if (c->labels.ids[k]) (void)hipFree(c->labels.ids[k]);
    c->labels.tab[k] = nullptr;
    c->labels.ids[k] = nullptr;
  }
  c->labels.rows = 0;
  c->labels.C = 0;
}
// table and ID lists for at least the map count; waits for the device only when the bound outgrows them
int labels_reserve(ef_ctx* c) {
  c->labels.bound = labels_count_bound(c);
  if (c->labels.bound <= c->labels.rows) return EF_OK;
  uint32_t n = 0;
  int r = read_count(c, &n);
  if (r != EF_OK) return r;
  unsigned np[2] = {0, 0};
  EF_HIP(c, hipMemcpy(np, c->labels.ids_state + 2, sizeof(np), hipMemcpyDeviceToHost));
  c->labels.known = n;
  c->labels.known_frames = c->stamps.size();
  c->labels.ev_pending = false;
  c->labels.bound = n;
  if (n <= c->labels.rows) return EF_OK;
  const size_t P = (size_t)c->cam.cols * c->cam.rows, C = (size_t)c->labels.C;
  size_t rows = (size_t)n + std::max((size_t)n / 4, P);
  if (rows > c->capacity) rows = c->capacity;
  float* tab[2] = {};
  uint32_t* ids[2] = {};
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    e = hipMalloc((void**)&tab[k], rows * C * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&ids[k], rows * sizeof(uint32_t));
  }
  if (e != hipSuccess) {
    for (int k = 0; k < 2; ++k) { if (tab[k]) (void)hipFree(tab[k]); if (ids[k]) (void)hipFree(ids[k]); }
    c->err = std::string("hipMalloc (label table): ") + hipGetErrorString(e);
    return EF_ENOMEM;
  }
  const int w = c->labels.cur;   // the live alignment moves over; the other half is rewritten by the next one
  const size_t keep = std::min((size_t)np[w], c->labels.rows);
  if (keep) {
    EF_HIP(c, hipMemcpyAsync(tab[w], c->labels.tab[w], keep * C * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    EF_HIP(c, hipMemcpyAsync(ids[w], c->labels.ids[w], keep * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    EF_HIP(c, hipStreamSynchronize(c->stream));
  }
  const int C_keep = c->labels.C;
  labels_free(c);
  c->labels.C = C_keep;
  for (int k = 0; k < 2; ++k) { c->labels.tab[k] = tab[k]; c->labels.ids[k] = ids[k]; }
  c->labels.rows = rows;
  return EF_OK;
}
// what every label call starts with: IDs for the new rows, then the table re-aligned to the current rows
int labels_begin(ef_ctx* c, const char* fn) {
  int r = capture_check(c, fn);
  if (r != EF_OK) return r;
  if (!c->labels.C) { c->err = std::string(fn) + ": labels are off (ef_enable_labels)"; return EF_ESTATE; }
  r = ids_prepare(c, fn);
  if (r != EF_OK) return r;
  r = labels_reserve(c);
  if (r != EF_OK) return r;
  const int w = c->labels.cur;
  efm::LabelAlign a{c->maps[c->cur], &c->st->map_counts[c->cur], c->labels.ids[w], c->labels.tab[w], c->labels.ids_state + 2 + w,
                    c->labels.ids[w ^ 1], c->labels.tab[w ^ 1], c->labels.ids_state + 2 + (w ^ 1), c->labels.C, 1.0f / (float)c->labels.C};
  efm::labels_align(a, (unsigned)c->labels.bound, c->stream);
  EF_HIP(c, hipGetLastError());
  c->labels.cur ^= 1;
  // the count this call saw, for the next call's bound
  EF_HIP(c, hipMemcpyAsync(c->labels.count_h, &c->st->map_counts[c->cur], sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipEventRecord(c->labels.ev, c->stream));
  c->labels.ev_frames = c->stamps.size();
  c->labels.ev_pending = true;
  return EF_OK;
}
// the view's index image into labels.index, exactly as ef_render_model draws it (every caller has passed labels_begin, which refuses a
// capture under the caller's own name)
int labels_index(ef_ctx* c, const ef_render_params* p) {
  const int r = c->labels.index.reserve(c, (size_t)p->width * p->height * sizeof(uint32_t), "label index image");
  if (r != EF_OK) return r;
  return render_enqueue(c, p, efm::RenderOut{nullptr, nullptr, nullptr, nullptr, c->labels.index.as<uint32_t>()}, "ef_render_model");
}
// refusals before any GPU work; the view is checked with the render's rules
int labels_check(ef_ctx* c, const ef_render_params* view, bool view_required, const void* probs, bool probs_required, const char* fn) {
  std::string& err = c ? c->err : g_create_error;
  if (probs_required && !probs) { err = std::string(fn) + ": null probability image"; return EF_EINVAL; }
  if (view || view_required) return render_check(c, view, fn);
  if (!c) { err = std::string(fn) + ": null context"; return EF_EINVAL; }
  return EF_OK;
}
int labels_view(ef_ctx* c, const ef_render_params* view, ef_render_params* q) {
  if (view) { *q = *view; return EF_OK; }
  const int r = ef_default_render_params(c, q);
  q->draw_unstable = 1;
  return r;
}
int fuse_enqueue(ef_ctx* c, const ef_render_params* q, const float* probs_dev) {
  int r = labels_index(c, q);
  if (r != EF_OK) return r;
  efm::LabelFuse f{};
  f.map = c->maps[c->cur];
  f.count_dev = &c->st->map_counts[c->cur];
  f.cam = render_cam(q, f.Tcw);
  f.index = c->labels.index.as<uint32_t>();
  f.probs = probs_dev;
  f.tab = c->labels.tab[c->labels.cur];
  f.C = c->labels.C;
  efm::labels_fuse(f, (unsigned)c->labels.bound, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
int render_labels_enqueue(ef_ctx* c, const ef_render_params* p, int32_t* label, float* prob) {
  int r = labels_index(c, p);
  if (r != EF_OK) return r;
  efm::labels_gather(c->labels.index.as<uint32_t>(), p->width * p->height, c->labels.tab[c->labels.cur], c->labels.C, label, prob, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
}  // namespace
extern "C" {

int ef_set_surfel_ids(ef_ctx* c, int on) {
  if (!c) { g_create_error = "ef_set_surfel_ids: null context"; return EF_EINVAL; }
  DeviceGuard dg_(c);
  int r = capture_check(c, "ef_set_surfel_ids");
  if (r != EF_OK) return r;
  if ((on != 0) == c->labels.ids_on) return EF_OK;
  if (on && !c->labels.ids_state) {
    const unsigned init[4] = {1u, 0u, 0u, 0u};
    EF_HIP(c, hipMalloc((void**)&c->labels.ids_state, sizeof(init)));
    EF_HIP(c, hipMemcpy(c->labels.ids_state, init, sizeof(init), hipMemcpyHostToDevice));
    EF_HIP(c, hipHostMalloc((void**)&c->labels.count_h, sizeof(unsigned)));
    EF_HIP(c, hipEventCreateWithFlags(&c->labels.ev, hipEventDisableTiming));
  }
  if (!on) labels_free(c);
  // on: the lane is numbered from the counter by the next ID-consuming call (1 .. N the first time); off: as if IDs had never been on
  efm::ids_zero(c->maps[c->cur], &c->st->map_counts[c->cur], c->capacity, c->stream);
  EF_HIP(c, hipGetLastError());
  c->labels.ids_on = on != 0;
  c->labels.ids_bad = false;
  return EF_OK;
}

int ef_get_surfel_ids(ef_ctx* c, uint32_t* ids, uint32_t max_ids, uint32_t* count) {
  if (!c || !count) { (c ? c->err : g_create_error) = c ? "ef_get_surfel_ids: null count" : "ef_get_surfel_ids: null context"; return EF_EINVAL; }
  DeviceGuard dg_(c);
  int r = capture_check(c, "ef_get_surfel_ids");
  if (r != EF_OK) return r;
  if (!c->labels.ids_on) { c->err = "ef_get_surfel_ids: surfel IDs are off (ef_set_surfel_ids)"; return EF_ESTATE; }
  r = ids_prepare(c, "ef_get_surfel_ids");
  if (r != EF_OK) return r;
  uint32_t n = 0;
  r = read_count(c, &n);
  if (r != EF_OK) return r;
  if (n > max_ids) n = max_ids;
  *count = n;
  if (!ids || !n) return EF_OK;
  uint32_t* tmp = nullptr;
  EF_HIP(c, hipMalloc((void**)&tmp, (size_t)n * sizeof(uint32_t)));
  efm::ids_gather(c->maps[c->cur], n, tmp, c->stream);
  hipError_t e = hipMemcpyAsync(ids, tmp, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(tmp);
  EF_HIP(c, e);
  return EF_OK;
}

int ef_enable_labels(ef_ctx* c, int num_classes) {
  if (num_classes < 0 || num_classes > 256) {
    (c ? c->err : g_create_error) = "ef_enable_labels: num_classes must lie in 0 .. 256";
    return EF_EINVAL;
  }
  if (!c) { g_create_error = "ef_enable_labels: null context"; return EF_EINVAL; }
  DeviceGuard dg_(c);
  int r = capture_check(c, "ef_enable_labels");
  if (r != EF_OK) return r;
  labels_free(c);
  if (!num_classes) return EF_OK;
  if (!c->labels.ids_on) {
    r = ef_set_surfel_ids(c, 1);
    if (r != EF_OK) return r;
  }
  EF_HIP(c, hipMemsetAsync(c->labels.ids_state + 2, 0, 2 * sizeof(unsigned), c->stream));   // no previous alignment: every row starts at the prior
  c->labels.C = num_classes;
  c->labels.cur = 0;
  c->labels.ev_pending = false;
  c->labels.known = c->capacity;   // unknown: the first label call reads it
  c->labels.known_frames = c->stamps.size();
  return EF_OK;
}

int ef_set_labels(ef_ctx* c, const float* probs, uint32_t count) {
  int r = labels_check(c, nullptr, false, probs, count != 0, "ef_set_labels");
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = labels_begin(c, "ef_set_labels");
  if (r != EF_OK) return r;
  uint32_t n = 0;
  r = read_count(c, &n);
  if (r != EF_OK) return r;
  if (count != n) { c->err = "ef_set_labels: count must equal the map count (" + std::to_string(n) + ")"; return EF_EINVAL; }
  if (n) {
    EF_HIP(c, hipMemcpyAsync(c->labels.tab[c->labels.cur], probs, (size_t)n * c->labels.C * sizeof(float), hipMemcpyHostToDevice, c->stream));
    EF_HIP(c, hipStreamSynchronize(c->stream));
  }
  return EF_OK;
}

int ef_get_labels(ef_ctx* c, uint32_t* ids, float* probs, uint32_t max_rows, uint32_t* count) {
  if (!c || !count) { (c ? c->err : g_create_error) = c ? "ef_get_labels: null count" : "ef_get_labels: null context"; return EF_EINVAL; }
  DeviceGuard dg_(c);
  int r = labels_begin(c, "ef_get_labels");
  if (r != EF_OK) return r;
  uint32_t n = 0;
  r = read_count(c, &n);
  if (r != EF_OK) return r;
  if (n > max_rows) n = max_rows;
  *count = n;
  if (!n) return EF_OK;
  if (ids) EF_HIP(c, hipMemcpyAsync(ids, c->labels.ids[c->labels.cur], (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (probs)
    EF_HIP(c, hipMemcpyAsync(probs, c->labels.tab[c->labels.cur], (size_t)n * c->labels.C * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}

int ef_fuse_labels_dev(ef_ctx* c, const ef_render_params* view, const float* probs_dev) {
  int r = labels_check(c, view, false, probs_dev, true, "ef_fuse_labels_dev");
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = labels_begin(c, "ef_fuse_labels_dev");
  if (r != EF_OK) return r;
  ef_render_params q;
  r = labels_view(c, view, &q);
  if (r != EF_OK) return r;
  return fuse_enqueue(c, &q, probs_dev);
}

int ef_fuse_labels(ef_ctx* c, const ef_render_params* view, const float* probs_chw) {
  int r = labels_check(c, view, false, probs_chw, true, "ef_fuse_labels");
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = labels_begin(c, "ef_fuse_labels");
  if (r != EF_OK) return r;
  ef_render_params q;
  r = labels_view(c, view, &q);
  if (r != EF_OK) return r;
  const size_t bytes = (size_t)q.width * q.height * c->labels.C * sizeof(float);
  r = c->stage.reserve(c, bytes, "label staging");
  if (r != EF_OK) return r;
  EF_HIP(c, hipMemcpyAsync(c->stage.p, probs_chw, bytes, hipMemcpyHostToDevice, c->stream));
  r = fuse_enqueue(c, &q, c->stage.as<float>());
  if (r != EF_OK) return r;
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}

int ef_render_labels_dev(ef_ctx* c, const ef_render_params* p, int32_t* label_dev, float* prob_dev) {
  int r = labels_check(c, p, true, nullptr, false, "ef_render_labels_dev");
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = labels_begin(c, "ef_render_labels_dev");
  if (r != EF_OK) return r;
  return render_labels_enqueue(c, p, label_dev, prob_dev);
}

int ef_render_labels(ef_ctx* c, const ef_render_params* p, int32_t* label, float* prob) {
  int r = labels_check(c, p, true, nullptr, false, "ef_render_labels");
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  r = labels_begin(c, "ef_render_labels");
  if (r != EF_OK) return r;
  const size_t P = (size_t)p->width * p->height;
  r = c->stage.reserve(c, P * 8, "label staging");
  if (r != EF_OK) return r;
  int32_t* dl = label ? c->stage.as<int32_t>() : nullptr;
  float* dp = prob ? (float*)(c->stage.p + P * 4) : nullptr;
  r = render_labels_enqueue(c, p, dl, dp);
  if (r != EF_OK) return r;
  if (label) EF_HIP(c, hipMemcpyAsync(label, dl, P * 4, hipMemcpyDeviceToHost, c->stream));
  if (prob) EF_HIP(c, hipMemcpyAsync(prob, dp, P * 4, hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}

}  // extern "C"
