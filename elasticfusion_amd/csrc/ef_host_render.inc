// ================================================================================================
// GlobalModel::renderPointCloud without OpenGL (include/ef_hip.h: ef_default_render_params, ef_render_model[_dev]; kernels in ef_render.inc)
// ================================================================================================
namespace {
// the parameters are checked before the context: with a NULL context the message goes where ef_last_error(NULL) finds it
int render_check(ef_ctx* c, const ef_render_params* p, const char* fn) {
  std::string& err = c ? c->err : g_create_error;
  const char* why = nullptr;
  if (!p) why = "null params";
  else if (p->width < 1 || p->width > 4096 || p->height < 1 || p->height > 4096) why = "width and height must lie in 1 .. 4096";
  else if (p->color_type < 0 || p->color_type > 3) why = "color_type must be 0 .. 3";
  else if (!std::isfinite(p->fx) || !std::isfinite(p->fy) || !std::isfinite(p->cx) || !std::isfinite(p->cy) || p->fx == 0.f || p->fy == 0.f)
    why = "intrinsics must be finite with non-zero focal lengths";
  else if (!c) why = "null context";
  if (!why) return EF_OK;
  err = std::string(fn) + ": " + why;
  return EF_EINVAL;
}
// the camera and the float T_wc^-1 of a view
efm::Cam render_cam(const ef_render_params* p, float* Tcw) {
  float pose_f[16];
  pose_mats(p->T_wc, Tcw, pose_f);
  return efm::Cam{p->width, p->height, p->fx, p->fy, p->cx, p->cy};
}
// fn is the name the capture refusal is made under
int render_enqueue(ef_ctx* c, const ef_render_params* p, const efm::RenderOut& out, const char* fn) {
  int r = capture_check(c, fn);
  if (r != EF_OK) return r;
  // the render's z-buffer: grown to P keys, 0xFF bytes (ZBUF_EMPTY) once; every resolve leaves it so
  const size_t zbytes = (size_t)p->width * p->height * sizeof(unsigned long long);
  bool grew = false;
  r = c->render.zbuf.reserve(c, zbytes, "render z-buffer", &grew);
  if (r != EF_OK) return r;
  if (grew) EF_HIP(c, hipMemsetAsync(c->render.zbuf.p, 0xFF, zbytes, c->stream));
  efm::RenderArgs a{};
  a.cam = render_cam(p, a.Tcw);
  a.maxDepth = p->max_depth;
  a.threshold = p->threshold;
  a.drawUnstable = p->draw_unstable != 0;
  a.colorType = p->color_type;
  a.drawWindow = p->draw_window != 0;
  a.time = p->time;
  a.timeDelta = p->time_delta;
  efm::render_model(a, c->maps[c->cur], &c->st->map_counts[c->cur], c->render.zbuf.as<unsigned long long>(), out, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
}  // namespace
extern "C" {

int ef_default_render_params(ef_ctx* c, ef_render_params* p) {
  if (!c) return EF_EINVAL;
  if (!p) { c->err = "ef_default_render_params: null params"; return EF_EINVAL; }
  memset(p, 0, sizeof(*p));
  const int r = ef_get_pose(c, p->T_wc);
  if (r != EF_OK) return r;
  p->width = c->cam.cols; p->height = c->cam.rows;
  p->fx = c->cam.fx; p->fy = c->cam.fy; p->cx = c->cam.cx; p->cy = c->cam.cy;
  p->max_depth = 1000.0f;   // the GUI's far plane
  p->threshold = c->cfg.confidence;
  p->time = c->tick;
  p->time_delta = c->cfg.time_delta;
  return EF_OK;
}
int ef_render_model_dev(ef_ctx* c, const ef_render_params* p, uint8_t* rgba, float* depth, float* vertex, float* normal, uint32_t* index) {
  const int r = render_check(c, p, "ef_render_model_dev");
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  // (the _dev variant has always refused a capture under the name ef_render_model: the text is kept)
  return render_enqueue(c, p, efm::RenderOut{(uchar4*)rgba, depth, (float4*)vertex, (float4*)normal, index}, "ef_render_model");
}
int ef_render_model(ef_ctx* c, const ef_render_params* p, uint8_t* rgba, float* depth, float* vertex, float* normal, uint32_t* index) {
  int r = render_check(c, p, "ef_render_model");
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  const size_t P = (size_t)p->width * p->height;
  // the requested outputs land in the staging area, then are copied out
  const size_t sz[5] = {rgba ? P * 4 : 0, depth ? P * 4 : 0, vertex ? P * 16 : 0, normal ? P * 16 : 0, index ? P * 4 : 0};
  const size_t bytes = sz[0] + sz[1] + sz[2] + sz[3] + sz[4];
  r = c->stage.reserve(c, bytes, "render outputs");
  if (r != EF_OK) return r;
  void* host[5] = {rgba, depth, vertex, normal, index};
  void* dev[5] = {};
  size_t off = 0;
  for (int i = 0; i < 5; ++i) {
    if (sz[i]) dev[i] = c->stage.p + off;
    off += sz[i];
  }
  r = render_enqueue(c, p, efm::RenderOut{(uchar4*)dev[0], (float*)dev[1], (float4*)dev[2], (float4*)dev[3], (uint32_t*)dev[4]}, "ef_render_model");
  if (r != EF_OK) return r;
  for (int i = 0; i < 5; ++i)
    if (sz[i]) EF_HIP(c, hipMemcpyAsync(host[i], dev[i], sz[i], hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}

}  // extern "C"
