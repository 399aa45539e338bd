// ================================================================================================
// Fuse surfels into the map (include/ef_hip.h: ef_default_fuse_params, ef_map_fuse[_dev]): the append path of ef_host_insert.inc with the merge
// on; kernels in ef_fuse.inc; DESIGN.md §8g
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
int fuse_check(ef_ctx* c, const char* fn_, bool rec_null, uint32_t n, const double* T, const ef_fuse_params* p, bool res_null) {
  std::string& err = c ? c->err : g_create_error;
  const std::string fn = fn_;
  if (!p) { err = fn + ": null params"; return EF_EINVAL; }
  if (res_null) { err = fn + ": null result"; return EF_EINVAL; }
  if (p->append != 0 && p->append != 1) { err = fn + ": append must be 0 or 1"; return EF_EINVAL; }
  const ef_insert_params ip = fuse_as_insert(p);
  return insert_check(c, fn_, rec_null, n, T, &ip, false);
}
AppendCall fuse_call(const char* fn, const float* rec, uint32_t n, const double* T, const ef_fuse_params* p, ef_fuse_result* res, uint32_t* new_row,
                     uint32_t* match_row, uint8_t* outcome) {
  return AppendCall{fn, rec, n, T, fuse_as_insert(p), true, p->append != 0, new_row, match_row, outcome, nullptr, res};
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
  const int r = fuse_check(c, "ef_map_fuse_dev", !rec_dev, n, T, p, !res);
  if (r != EF_OK) return r;
  if (((uintptr_t)rec_dev & 15) != 0) { c->err = "ef_map_fuse_dev: surfels12_dev is not 16-byte aligned"; return EF_EINVAL; }
  DeviceGuard dg_(c);
  return append_run(c, fuse_call("ef_map_fuse_dev", rec_dev, n, T, p, res, new_row_dev, match_row_dev, outcome_dev));
}
int ef_map_fuse(ef_ctx* c, const float* rec, uint32_t n, const double* T, const ef_fuse_params* p, ef_fuse_result* res, uint32_t* new_row,
                uint32_t* match_row, uint8_t* outcome) {
  const int r = fuse_check(c, "ef_map_fuse", !rec, n, T, p, !res);
  if (r != EF_OK) return r;
  DeviceGuard dg_(c);
  return append_host(c, fuse_call("ef_map_fuse", rec, n, T, p, res, new_row, match_row, outcome), "fuse staging");
}

}  // extern "C"
