// ================================================================================================
// The loop closures of a frame (ElasticFusion.cpp:392-527) and what they share with the end of the frame: the 1/8-resolution views and fern
// codes of the fill-in maps, the end-of-frame record, the fern-to-view tracker, the global and the local closure.  The host side of the
// closures (fern database, deformation solver) is ef_ferns.hip / ef_deform_solver.hpp; DESIGN_closures.md
// ================================================================================================
namespace {
// The 1/8-resolution views of the fill-in maps (Ferns.cpp:91-93,178-180: Resize::image / Resize::vertex x2) into a pinned buffer
// (image | vertices | normals); enqueued only, the caller synchronises
int enqueue_fern_view(ef_ctx* c, uint8_t* h_dst) {
  hipStream_t s = c->stream;
  const int W = c->cam.cols, dw = c->fern_w, dh = c->fern_h, n = dw * dh;
  const dim3 g((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(k_resize_nearest<uint32_t>, g, dim3(256), 0, s, (const uint32_t*)c->fm.image, W, dw, dh, 8, (uint32_t*)c->view_img_dev);
  hipLaunchKernelGGL(k_resize_nearest<float4>, g, dim3(256), 0, s, (const float4*)c->fm.vertex, W, dw, dh, 8, c->view_vert_dev);
  hipLaunchKernelGGL(k_resize_nearest<float4>, g, dim3(256), 0, s, (const float4*)c->fm.normal, W, dw, dh, 8, c->view_norm_dev);
  EF_HIP(c, hipMemcpyAsync(h_dst, c->view_img_dev, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  EF_HIP(c, hipMemcpyAsync(h_dst + (size_t)n * 4, c->view_vert_dev, (size_t)n * 16, hipMemcpyDeviceToHost, s));
  EF_HIP(c, hipMemcpyAsync(h_dst + (size_t)n * 20, c->view_norm_dev, (size_t)n * 16, hipMemcpyDeviceToHost, s));
  return EF_OK;
}
// the fern codes of the current fill-in maps (k_fern_codes) into a pinned buffer; enqueued only
int enqueue_fern_codes(ef_ctx* c, uint8_t* h_dst) {
  hipStream_t s = c->stream;
  ef_ferns* F = ef_closure_ferns(c->closure);
  if (ef_ferns_table_version(F) != c->fern_table_version) {   // first use, or ef_ferns_set_table since: (rare) synchronous upload
    std::vector<int> t((size_t)c->fern_num * 6);
    if (ef_ferns_get_table(F, t.data()) != EF_OK) { c->err = "ef_ferns_get_table failed"; return EF_EINVAL; }
    EF_HIP(c, hipStreamSynchronize(s));
    EF_HIP(c, hipMemcpy(c->fern_table_dev, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice));
    c->fern_table_version = ef_ferns_table_version(F);
  }
  hipLaunchKernelGGL(k_fern_codes, dim3(1), dim3(FERN_CODES_PAD), 0, s, (const uchar4*)c->fm.image, (const float4*)c->fm.vertex, c->cam.cols, 8,
                     (const int*)c->fern_table_dev, c->fern_num, c->fern_codes_dev);
  EF_HIP(c, hipMemcpyAsync(h_dst, c->fern_codes_dev, FERN_CODES_BYTES, hipMemcpyDeviceToHost, s));
  return EF_OK;
}
// ef_view_fetch of the mid-frame view: Ferns::findFrame asks for it only when a keyframe passed the code gates (one more synchronisation,
// in those frames only); the fill-in maps still hold the mid-frame prediction
int fetch_mid_view(void* user, const uint8_t** rgb, int* ch, const float** verts, const float** norms) {
  ef_ctx* c = (ef_ctx*)user;
  const int r = enqueue_fern_view(c, c->h_view);
  if (r != EF_OK) return r;
  EF_HIP(c, hipStreamSynchronize(c->stream));
  const size_t n = (size_t)c->fern_w * c->fern_h;
  *rgb = c->h_view; *ch = 4; *verts = (const float*)(c->h_view + n * 4); *norms = (const float*)(c->h_view + n * 20);
  return EF_OK;
}
// ... and of the end-of-frame view, which was copied with the end-of-frame record
int fetch_end_view(void* user, const uint8_t** rgb, int* ch, const float** verts, const float** norms) {
  ef_ctx* c = (ef_ctx*)user;
  const size_t n = (size_t)c->fern_w * c->fern_h;
  *rgb = c->h_view_end; *ch = 4; *verts = (const float*)(c->h_view_end + n * 4); *norms = (const float*)(c->h_view_end + n * 20);
  return EF_OK;
}
// End of a frame (ElasticFusion.cpp:588-589, 593, 609-618) — ENQUEUED: fern codes and 1/8 view of the final fill-in maps, the pose, a
// fresh sample of the graph nodes, all into pinned memory behind one event.  Nothing waits for them here.
int enqueue_end_record(ef_ctx* c) {
  hipStream_t s = c->stream;
  int r = enqueue_fern_codes(c, c->h_codes_end);
  if (r != EF_OK) return r;
  if (!c->lost) {   // a lost camera stores no keyframe (:601-604): its view is never asked for
    r = enqueue_fern_view(c, c->h_view_end);
    if (r != EF_OK) return r;
  }
  EF_HIP(c, hipMemcpyAsync(&c->h_states[2], c->st, sizeof(eft::TrackState), hipMemcpyDeviceToHost, s));
  unsigned* n_dev = (unsigned*)(c->nodes_dev + (size_t)1024 * 4);   // Deformation::sampleGraphModel (:593): every 5000th surfel of the new map
  efm::sample_graph(c->maps[c->cur], &c->st->map_counts[c->cur], 5000, 1023, c->nodes_dev, n_dev, s);
  EF_HIP(c, hipMemcpyAsync(c->h_nodes_pinned, c->nodes_dev, ((size_t)1024 * 4 + 1) * sizeof(float), hipMemcpyDeviceToHost, s));
  EF_HIP(c, hipEventRecord(c->ev_end_record, s));
  c->end_pending = true;
  c->end_lost = c->lost;
  c->end_tick = c->tick;
  return EF_OK;
}
// ... and looked at: pose -> trajectory, codes (+ view, if the frame is kept) -> Ferns::addFrame, the node count.  Called at the next
// point where the host waits for the stream anyway (the next frame's closures) and by every getter that shows closure state.
int flush_end_record(ef_ctx* c) {
  if (!c->closure || !c->end_pending) return EF_OK;
  EF_HIP(c, hipEventSynchronize(c->ev_end_record));
  c->end_pending = false;
  double T[16];
  pose_of_state(c->h_states[2], T);
  int good = 0;
  memcpy(&good, c->h_codes_end + FERN_CODES_PAD, sizeof(int));
  const int r = c->end_lost ? ef_closure_log_pose(c->closure, T, c->end_tick)
                            : ef_closure_end_frame_coded(c->closure, c->h_codes_end, good, &fetch_end_view, c, T, c->end_tick);
  unsigned nn = 0;
  memcpy(&nn, c->h_nodes_pinned + (size_t)1024 * 4, sizeof(unsigned));
  c->n_nodes_host = (int)nn;
  if (r < 0) { c->err = "ef_closure_end_frame failed"; return r; }
  return EF_OK;
}

// Ferns.cpp:243-258 on the device: the stored keyframe is the model (initICPModel with its pose), the current view the frame
// (initICP(vertices, normals)); getIncrementalTransformation(T, rgbOnly = false, icpWeight = 100, pyramid = false, fastOdom = false,
// so3 = false) = ten ICP-only iterations at the 1/8 resolution itself.  One synchronisation (pose + statistics back).
void fern_tracker_device(void* user, const float* fv, const float* fn, const double* Tf, const float* cv, const float* cn, double* T_io, float* err,
                         float* cnt) {
  ef_ctx* c = (ef_ctx*)user;
  hipStream_t s = c->stream;
  const size_t n = (size_t)c->fern_w * c->fern_h;
  float4* d_fv = c->fern_maps_dev;
  float4* d_fn = d_fv + n;
  float4* d_cv = d_fn + n;
  float4* d_cn = d_cv + n;
  const uint8_t* zero_image = (const uint8_t*)(d_cn + n);
  // a failed copy or launch must not hand a stale pose and inlier count to Ferns::findFrame's gates: the first HIP error is kept in the
  // context (global_loop_closure returns EF_EHIP for it) and the candidate is rejected (error = +inf, count = 0)
  hipError_t e = hipMemcpyAsync(d_fv, fv, n * 16, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_fn, fn, n * 16, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_cv, cv, n * 16, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(d_cn, cn, n * 16, hipMemcpyHostToDevice, s);
  (void)Tf;   // the caller hands T_io = T_wc_fern in (Ferns.cpp:250); the model maps are transformed with it
  eft::pose_injected(c->st3, T_io, false, 1.0f, false, nullptr, 0, s);
  eft::init_icp_model(c->pyr3, (const float*)d_fv, (const float*)d_fn, (const float*)d_fv, (const float*)d_fn, c->st3, 6.0f, s);
  eft::init_icp_maps(c->pyr3, (const float*)d_cv, (const float*)d_cn, zero_image, c->st3, 6.0f, s);
  eft::TrackParams tp = track_params(c);
  tp.rgbOnly = false; tp.pyramid = false; tp.fastOdom = false; tp.so3 = false; tp.icpWeight = 100.f;
  const eft::TrackTail tail = eft::track(c->pyr3, c->st3, c->intr3, tp, s, nullptr);
  eft::track_end(c->st3, tail, false, 1.0f, nullptr, -1, s, eft::tracker_abort_word(c->pyr3), c->d_abort + 2);
  if (e == hipSuccess) e = hipMemcpyAsync(&c->h_states[1], c->st3, sizeof(eft::TrackState), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) {
    if (c->fern_tracker_error.empty()) c->fern_tracker_error = std::string("fern-to-view registration: ") + hipGetErrorString(e);
    *err = std::numeric_limits<float>::infinity();
    *cnt = 0.f;
    c->gloop.icp_error = *err;
    c->gloop.icp_count = 0.f;
    return;
  }
  const eft::TrackState& h = c->h_states[1];
  pose_of_state(h, T_io);
  *err = h.lastICPError;
  *cnt = h.lastICPCount;
  c->gloop.icp_error = h.lastICPError;
  c->gloop.icp_count = h.lastICPCount;
}

// ElasticFusion.cpp:392-445; *accepted_with_graph = 1 when a fern was matched AND the global deformation accepted with a graph.  A lost
// camera (relocalisation) takes the matched keyframe's registration as its pose instead (:411-413).
int global_loop_closure(ef_ctx* c, int log_slot, int* accepted_with_graph) {
  *accepted_with_graph = 0;
  ef_global_loop& G = c->gloop;
  memset(&G, 0, sizeof(G));
  G.attempted = 1;
  G.closest = -1;
  for (int i = 0; i < 16; ++i) G.T_wc_recovery[i] = (i % 5 == 0) ? 1.0 : 0.0;   // Sophus::SE3d T_wc_est; (Ferns.cpp:236)
  ef_ferns* F = ef_closure_ferns(c->closure);
  // Ferns::findFrame only considers keyframes stored more than 300 ticks ago (Ferns.cpp:218).  While there is none — the host knows: it
  // keeps the database — the answer is -1 whatever the view shows, and nothing has to come back from the device: no synchronisation.
  if (!ef_closure_candidate_possible(c->closure, c->tick)) return EF_OK;
  // otherwise: the view's fern codes, computed on the device, + the pose — one small read-back (0.5 KB + the state)
  int r0 = enqueue_fern_codes(c, c->h_codes);
  if (r0 != EF_OK) return r0;
  EF_HIP(c, hipMemcpyAsync(&c->h_states[0], c->st, sizeof(eft::TrackState), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  r0 = flush_end_record(c);   // the previous frame's keyframe decision first: the database findFrame walks must be complete
  if (r0 != EF_OK) return r0;
  pose_of_state(c->h_states[0], c->h_pose);
  int good = 0;
  memcpy(&good, c->h_codes + FERN_CODES_PAD, sizeof(int));
  if (c->lost) {
    const int r = ef_closure_relocalise_coded(c->closure, c->h_codes, good, &fetch_mid_view, c, c->h_pose, c->tick, &fern_tracker_device, c, G.T_wc_recovery);
    if (!c->fern_tracker_error.empty()) { c->err = c->fern_tracker_error; c->fern_tracker_error.clear(); return EF_EHIP; }
    if (r < 0) { c->err = "ef_closure_relocalise failed"; return r; }
    G.closest = ef_ferns_last_closest(F);
    if (r == 1) {
      eft::pose_injected(c->st, G.T_wc_recovery, false, 1.0f, false, log_slot >= 0 ? c->traj : nullptr, log_slot, c->stream);
      c->last_frame_recovery = true;
    }
    return EF_OK;
  }
  c->loop_graph.assign((size_t)1024 * 16, 0.f);
  int nodes = 0;
  const int r = ef_closure_global_coded(c->closure, c->h_codes, good, &fetch_mid_view, c, c->h_pose, c->tick, &fern_tracker_device, c, c->h_nodes_pinned,
                                        c->n_nodes_host, G.T_wc_recovery, c->loop_graph.data(), &nodes);
  if (!c->fern_tracker_error.empty()) { c->err = c->fern_tracker_error; c->fern_tracker_error.clear(); return EF_EHIP; }
  if (r < 0) { c->err = "ef_closure_global failed"; return r; }
  G.closest = ef_ferns_last_closest(ef_closure_ferns(c->closure));   // Ferns::lastClosest: -1 unless a keyframe passed every gate
  if (G.closest >= 0) {   // the rows handed to the optimiser: two per fern constraint (the constraint and its pin) + the kept relative ones
    const int rows = ef_closure_last_rows(c->closure, nullptr, 0, nullptr, nullptr), rel = ef_closure_relative(c->closure, nullptr, 0);
    G.n_constraints = rows > rel ? (rows - rel) / 2 : 0;
  }
  if (r != 1) return EF_OK;
  if (nodes < 0 || nodes >= 1024) { c->err = "global closure: 0..1023 graph nodes (GlobalModel::MAX_NODES)"; return EF_EINVAL; }
  G.accepted = 1;
  G.graph_nodes = nodes;
  // T_wc := the recovered pose (:429); the frame's logged pose follows (:588); the velocity weighting of :369-383 stays
  eft::pose_injected(c->st, G.T_wc_recovery, false, 1.0f, false, log_slot >= 0 ? c->traj : nullptr, log_slot, c->stream);
  if (nodes > 0) {
    EF_TRY(upload_graph(c, c->loop_graph.data(), nodes));
    c->graph_nodes = nodes;
    c->graph_is_fern = 1;                                                                            // fernAccepted, :441,584
    *accepted_with_graph = 1;
  }
  return EF_OK;
}

// ElasticFusion.cpp:447-527.  The optimisation is the registered solver's, the built-in one's, or — with the global closure enabled —
// the closure object's (keyframe poses follow, relative constraints are kept).  Synchronises once, where the reference reads the
// constraint buffers back (Resize.cpp:108,146).  have_active: the ACTIVE prediction at the new pose (predict() of :387) was already made.
int local_loop_closure(ef_ctx* c, int log_slot, bool have_active) {
  hipStream_t s = c->stream;
  const int W = c->cam.cols, H = c->cam.rows, step = 20 /* consSample, ElasticFusion.cpp:62 */;
  const int cw = W / step, ch = H / step;
  const efm::FillMaps none{nullptr, nullptr, nullptr};
  const unsigned* count = &c->st->map_counts[c->cur];
  // predict() of :387: the ACTIVE view at the pose just estimated (its fill-in only feeds the fern database: made by the caller then)
  if (!have_active)
    efm::combined_predict(c->cam, c->st->T_cw, c->maps[c->cur], count, c->maxDepthProcessed, c->cfg.confidence, c->tick, c->tick, c->cfg.time_delta,
                          c->zbuf, c->pm, none, nullptr, nullptr, false, nullptr, s, nullptr, 0u, nullptr, 0u, c->rays);
  // :451-459, IndexMap::INACTIVE: surfels last seen at or before tick - timeDelta
  // (the prediction stamps st2->model_view_stamp with this frame's value when it shows at least one surfel: the model-to-model tracker's
  // persistent launch leaves at once otherwise — nothing can be registered against an empty view, and the reference's tracker, which runs
  // all the same, ends on zero sums: the stamp only says which frames those are)
  const unsigned view_stamp = (unsigned)c->tick * 2u + 1u;
  efm::combined_predict(c->cam, c->st->T_cw, c->maps[c->cur], count, c->maxDepthProcessed, c->cfg.confidence, 0, c->tick - c->cfg.time_delta,
                        c->cfg.time_delta, c->zbuf, c->old, none, nullptr, nullptr, false, nullptr, s, &c->st2->model_view_stamp, view_stamp, nullptr, 0u,
                        c->rays);
  eft::copy_pose(c->st2, c->st, s);                                                              // :469
  const float maxDepthRGB = 6.0f;                                                                // RGBDOdometry.cpp:42
  // :463 initICPModel(inactive view) + :464 initRGBModel(its image) + :466-467 initICP / initRGB(active view), fused (eft::init_model_pair)
  eft::init_model_pair(c->pyr2, (const float*)c->old.vertex, (const float*)c->old.normal, (const uint8_t*)c->old.image, (const float*)c->pm.vertex,
                       (const float*)c->pm.normal, (const uint8_t*)c->pm.image, c->st2, maxDepthRGB, s);
  eft::init_rgb_sobel(c->pyr2, s);
  eft::TrackParams tp = track_params(c);
  tp.rgbOnly = false; tp.pyramid = c->cfg.pyramid != 0; tp.fastOdom = c->cfg.fast_odom != 0; tp.so3 = false; tp.icpWeight = 10.f;   // :471
  tp.empty_model_flag = &c->st2->model_view_stamp;
  tp.empty_model_value = view_stamp;
  const eft::TrackTail tail2 = eft::track(c->pyr2, c->st2, c->intr, tp, s, nullptr);
  eft::track_end(c->st2, tail2, true, 1.0f, nullptr, -1, s, eft::tracker_abort_word(c->pyr2), c->d_abort + 1);
  eft::sample_constraints((const float*)c->pm.vertex, c->old.time, W, H, step, c->cons_dev, s);  // :485-486
  EF_HIP(c, hipMemcpyAsync(&c->h_states[0], c->st, sizeof(eft::TrackState), hipMemcpyDeviceToHost, s));
  EF_HIP(c, hipMemcpyAsync(&c->h_states[1], c->st2, sizeof(eft::TrackState), hipMemcpyDeviceToHost, s));
  EF_HIP(c, hipMemcpyAsync(c->h_cons, c->cons_dev, (size_t)cw * ch * 4 * sizeof(float), hipMemcpyDeviceToHost, s));
  EF_HIP(c, hipStreamSynchronize(s));
  {
    const int rf = flush_end_record(c);   // the previous frame's end-of-frame record (keyframe decision, graph nodes) has landed by now
    if (rf != EF_OK) return rf;
  }
  ef_local_loop& L = c->loop;
  memset(&L, 0, sizeof(L));
  c->loop_constraints.clear();
  L.attempted = 1;
  L.graph_capacity = 1023;   // GlobalModel::MAX_NODES - 1 (GlobalModel.cpp:24): rows of loop_graph / graph_dev
  const eft::TrackState& hc = c->h_states[0];
  const eft::TrackState& he = c->h_states[1];
  pose_of_state(hc, L.T_wc_curr);
  pose_of_state(he, L.T_wc_est);
  L.stats[0] = he.lastICPError; L.stats[1] = he.lastICPCount; L.stats[2] = he.lastRGBError;
  L.stats[3] = he.lastRGBCount; L.stats[4] = he.lastSO3Error; L.stats[5] = he.lastSO3Count;
  double cov[36];
  efl::lu_inverse<double, 6>(he.lastA, cov);                                                     // :473, getCovariance
  bool covOk = true;
  for (int i = 0; i < 6; ++i) {
    L.cov_diag[i] = cov[i * 6 + i];
    if (cov[i * 6 + i] > (double)c->cov_thresh) { covOk = false; break; }
  }
  L.cov_ok = covOk;
  L.gates_ok = covOk && he.lastICPCount > (float)c->icp_count_thresh && he.lastICPError < c->icp_err_thresh;   // :483-484
  if (!L.gates_ok) return EF_OK;
  const double* M = L.T_wc_curr;
  const double* E = L.T_wc_est;
  for (int i = 0; i < cw; ++i)
    for (int j = 0; j < ch; ++j) {
      const float* v = c->h_cons + (size_t)(i * ch + j) * 4;
      const unsigned tm = (unsigned)v[3];
      if (v[2] > 0 && v[2] < c->maxDepthProcessed && tm > 0) {                                     // :490-492
        double row[8];
        for (int r = 0; r < 3; ++r) {   // T * Vector4d(x, y, z, 1), a 4x4 matrix product evaluated left to right
          row[r] = ((M[r * 4] * (double)v[0] + M[r * 4 + 1] * (double)v[1]) + M[r * 4 + 2] * (double)v[2]) + M[r * 4 + 3] * 1.0;
          row[3 + r] = ((E[r * 4] * (double)v[0] + E[r * 4 + 1] * (double)v[1]) + E[r * 4 + 2] * (double)v[2]) + E[r * 4 + 3] * 1.0;
        }
        row[6] = (double)tm;
        row[7] = c->deforms == 0 ? 1.0 : 0.0;                                                      // :507-508 pinConstraints
        c->loop_constraints.insert(c->loop_constraints.end(), row, row + 8);
      }
    }
  L.n_constraints = (int)(c->loop_constraints.size() / 8);
  if (!c->solver && !c->builtin_solver) return EF_OK;
  c->loop_graph.assign((size_t)1024 * 16, 0.f);
  int nodes = 0;
  bool accepted = false;
  if (c->solver) {
    accepted = c->solver(c->solver_user, &L, c->loop_constraints.data(), L.n_constraints, c->loop_graph.data(), &nodes) != 0;   // :513-514
  } else if (c->closure) {
    // Deformation::constrain in full (:511-526): graph sampled at the end of the previous frame, keyframe poses deformed along,
    // a third of the new relative constraints kept for later global closures
    const int r = ef_closure_local(c->closure, c->loop_constraints.data(), L.n_constraints, c->tick, c->h_nodes_pinned, c->n_nodes_host,
                                   c->loop_graph.data(), &nodes);
    if (r < 0) { c->err = "ef_closure_local failed"; return r; }
    accepted = r == 1;
  } else {
    // the built-in optimiser on the graph Deformation::sampleGraphModel would have sampled at the end of the previous frame
    // (ElasticFusion.cpp:593): every 5000th surfel of the map as it stands now
    const int max_nodes = 1023;
    unsigned* n_dev = (unsigned*)(c->nodes_dev + (size_t)1024 * 4);
    efm::sample_graph(c->maps[c->cur], count, 5000, max_nodes, c->nodes_dev, n_dev, s);
    c->h_nodes.resize((size_t)1024 * 4 + 4);
    EF_HIP(c, hipMemcpyAsync(c->h_nodes.data(), c->nodes_dev, ((size_t)1024 * 4 + 1) * sizeof(float), hipMemcpyDeviceToHost, s));
    EF_HIP(c, hipStreamSynchronize(s));
    unsigned n_nodes = 0;
    memcpy(&n_nodes, &c->h_nodes[(size_t)1024 * 4], sizeof(unsigned));
    const efd::Result r = efd::solve_local(c->h_nodes.data(), (int)n_nodes, c->loop_constraints.data(), L.n_constraints, (uint64_t)c->tick,
                                           (uint64_t)c->last_deform_time, c->loop_graph.data());
    accepted = r.ok;
    nodes = r.ok ? (int)n_nodes : 0;
    if (r.ok) c->last_deform_time = c->tick;   // Deformation.cpp:199-201
  }
  if (accepted) {
    if (nodes < 0 || nodes >= 1024) { c->err = "loop solver: 0..1023 graph nodes (GlobalModel::MAX_NODES)"; return EF_EINVAL; }
    L.applied = 1;
    L.graph_nodes = nodes;
    c->deforms += nodes > 0;                                                                       // :523
    eft::adopt_pose(c->st, c->st2, log_slot >= 0 ? c->traj : nullptr, log_slot, s);                // :525
    if (nodes > 0) EF_TRY(upload_graph(c, c->loop_graph.data(), nodes));
    c->graph_nodes = nodes;
    c->graph_is_fern = 0;
  }
  return EF_OK;
}
}  // namespace
