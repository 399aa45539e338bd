// ================================================================================================
// One frame (include/ef_hip.h: ef_process_frame[_dev], ef_predict): ElasticFusion::processFrame (Core/ElasticFusion.cpp:270-607) as a plan
// made once and a sequence of stages that only ENQUEUE on the context's streams; DESIGN.md §6
// ================================================================================================
namespace {
int do_predict(ef_ctx* c, bool count_dense = true) {
  // ElasticFusion::predict(), ElasticFusion.cpp:621-653: combinedPredict(ACTIVE) + FillIn (fused into the resolve).  Right after a
  // relocalisation the whole model is rendered (time = 0: no surfel is too old); while the camera is lost the fill-in passes the raw
  // frame through (a second, plain fill-in pass over the fused one: the rare path)
  // (a host-pointer frame: this launch, behind every reader of the frame's landing buffers, tells the host that their ring slot is free again)
  efm::combined_predict(c->cam, c->st->T_cw, c->maps[c->cur], &c->st->map_counts[c->cur], c->maxDepthProcessed, c->cfg.confidence,
                        c->last_frame_recovery ? 0 : c->tick, c->tick, c->cfg.time_delta, c->zbuf, c->pm, c->fm, c->img.depth_filtered, c->img.rgb,
                        c->cfg.frame_to_frame_rgb != 0, (count_dense && !c->tally_by_consumer) ? &c->st->dense_count : nullptr, c->stream, nullptr, 0u,
                        (count_dense && c->mark_value) ? c->d_consumed : nullptr, c->mark_value, c->rays);
  if (count_dense) c->mark_value = 0;
  if (count_dense && c->tally_by_consumer) c->tally_pending = true;   // (the next tracked frame's model maps count the samples of this prediction)
  if (c->lost) efm::fill_in(c->cam, c->pm, c->img.depth_filtered, c->img.rgb, true, true, c->fm, c->stream);
  return EF_OK;
}
// RGBDOdometry::getCovariance of the frame-to-model tracker against the gate of ElasticFusion.cpp:330-337,348-355
bool reloc_covariance_ok(const eft::TrackState& h) {
  double cov[36];
  efl::lu_inverse<double, 6>(h.lastA, cov);
  for (int i = 0; i < 6; ++i)
    if (cov[i * 6 + i] > 1e-04) return false;
  return true;
}
// What a frame decides before it enqueues anything, from the context as the frame finds it (FramePlan f{c, kind, pose_given}: each member is
// initialised from the ones above it); the stages below only read it.
struct FramePlan {
  const ef_ctx* c; hipMemcpyKind kind; bool pose_given;   // what the plan is made from
  // Input stage: everything that needs nothing but the new frame.  With overlap on it is enqueued on in_stream and
  // waits only for the previous frame's TRACKER (the last reader of the frame-side pyramids); it then runs concurrently
  // with the previous frame's fusion + prediction on `stream`, which read the other set of frame images.
  bool overlap = c->overlap && !c->timing && c->in_stream != nullptr;
  hipStream_t sb = overlap ? c->in_stream : c->stream;
  // Round 6: the events the second stream waits for are recorded only while the overlap is on — an event record between two kernels of a stream is
  // a barrier packet, measured as a 6 us bubble each (three per frame: profiles/r06f_timeline_single_stream.txt).  The first overlapped frame
  // after a frame that recorded none joins the streams on the host instead.
  bool want_events = c->overlap && c->in_stream != nullptr;
  // (mode 2 would put the bilateral filter on the chip WHILE the persistent tracker launch wants all of its CUs: its admission would fail and the
  // frame would run on the one-workgroup fallback — mode 1 is what such a context gets)
  int overlap_mode = (c->overlap_mode == 2 && c->persistent == 1 && !c->use_graph) ? 1 : c->overlap_mode;
  bool frame_done_event = want_events && c->overlap_mode == 2;   // recorded at the end of the frame: what ef_set_input_overlap(2) asked for, demoted or not
  bool track_this = c->tick > 1 && !pose_given;
  // Frames that are already in HBM are not copied by separate launches in the single-stream script: the bilateral filter
  // reads the caller's depth directly (nothing later needs the raw image) and the RGB copy rides on the intensity kernel.
  bool fold_copies = kind == hipMemcpyDeviceToDevice && track_this;
  // Round 6: in the single-stream script of a tracked frame the pre-processing and the tracker's model-side maps are ONE launch (k_frame_inputs,
  // at init_icp_model): two independent kernels, one bound by LDS look-ups, the other by HBM.
  bool joint_inputs = track_this && !overlap && !c->timing;
  bool sample = c->ktime_every > 0 && (c->tick % c->ktime_every) == 0;   // ef_kernel_timing samples this frame's kernels
  // BASELINE configs[4] is the hipGraph-captured launch-per-step script; the persistent launch takes a fresh exchange epoch
  // per launch as a kernel argument, which a replayed graph cannot give it
  bool replay = c->use_graph && !sample && !c->timing;
  // Round 9: neither predictIndices is resolved — their consumers tap the keys (ef_ctx::zbuf_assoc).  Not with stage timers (the update pass is
  // a launch of its own between the two), the reference's download buffer, or a context that closes loops (a deformation's clean(), the
  // predictions that share c->zbuf): those run the resolve launches as before.
#ifdef EF_KEEP_INDEX_RESOLVE   // (A/B build "resolve": rounds 1-8's two resolve launches per frame)
  bool keyed = false;
#else
  bool keyed = !c->timing && !c->reference_download && !c->cfg.close_loops;
#endif
  // (the update pass — k_merge — rides on the splat of the second predictIndices: one launch less; with stage timers on it stays a launch of
  // its own so that the reference's TICK / TOCK stages keep their meaning)
  bool defer_merge = !c->timing;
};
// The input stage.  *fp: the frame's pre-processing as it was enqueued here, or — joint inputs — as the tracker's first launch will do it.
int input_stage(ef_ctx* c, const FramePlan& f, const uint8_t* rgb_src, const uint16_t* depth_src, hipEvent_t images_ready, eft::FramePreprocess* fp) {
  const int W = c->cam.cols, H = c->cam.rows;
  hipStream_t sb = f.sb;
  if (f.overlap && !c->events_live) EF_HIP(c, hipStreamSynchronize(c->stream));
  std::swap(c->img, c->img_alt);
  c->frame_parity ^= 1;
  if (f.overlap) EF_HIP(c, hipStreamWaitEvent(sb, f.overlap_mode == 2 ? c->ev_frame_done[c->frame_parity] : c->ev_track_done, 0));
  if (images_ready) EF_HIP(c, hipStreamWaitEvent(sb, images_ready, 0));   // (the upload of a host-pointer frame, on copy_stream)
  // the frame images are referenced by later stages of this frame and by the next frame's tracker
  // (fill-in / predict read depth_filtered + rgb), so they are copied into context-owned buffers
  if (!f.fold_copies) {
    EF_HIP(c, hipMemcpyAsync(c->img.rgb, rgb_src, (size_t)W * H * 3, f.kind, sb));
    EF_HIP(c, hipMemcpyAsync(c->img.depth_raw, depth_src, (size_t)W * H * 2, f.kind, sb));
  }
  // (a tracked frame: the level-0 intensity image of the frame and — folded copies — the context's copy of the colours ride on this launch)
  *fp = eft::FramePreprocess{f.fold_copies ? depth_src : c->img.depth_raw, c->cfg.depth_cut, c->bil_table, c->img.depth_filtered, c->img.depth_metric,
                             c->img.depth_metric_filtered, f.fold_copies ? rgb_src : c->img.rgb, f.fold_copies ? c->img.rgb : nullptr};
  timer_begin(c, "Preprocess");
  if (!f.joint_inputs && !efm::preprocess_depth(fp->raw, W, H, fp->maxD, fp->filtered, fp->metric, fp->metric_filtered, sb, 0u,
                                                f.track_this ? fp->rgb3 : nullptr, c->pyr.nextImage[0], fp->rgb_keep, fp->table)) {
    c->err = "bilateral weight table missing on this device";
    return EF_EHIP;
  }
  timer_end(c, "Preprocess");
  if (f.overlap && f.overlap_mode == 2) EF_HIP(c, hipStreamWaitEvent(sb, c->ev_track_done, 0));
  if (f.track_this && f.overlap)   // the single-stream script builds all pyramids together (eft::build_pyramids, track_frame)
    eft::build_pyramids_frame_side(c->pyr, c->img.depth_filtered, c->intr, c->maxDepthProcessed, sb);
  if (f.overlap) EF_HIP(c, hipEventRecord(c->ev_input_done, sb));
  return EF_OK;
}
// ElasticFusion.cpp:290-296: the first frame seeds the map
int first_frame(ef_ctx* c, const FramePlan& f, int log_slot) {
  hipStream_t s = c->stream;
  if (f.overlap) EF_HIP(c, hipStreamWaitEvent(s, c->ev_input_done, 0));
  timer_begin(c, "feedbackBuffers");
  efm::seed_map(c->cam, c->img.rgb, c->img.depth_metric, c->img.depth_metric_filtered, c->tick, c->maxDepthProcessed, c->maps[c->cur],
                &c->st->map_counts[c->cur], c->cs, s);
  eft::init_first_rgb(c->pyr, c->img.rgb, s);
  if (log_slot >= 0) eft::log_pose(c->st, c->traj, log_slot, s);
  if (f.want_events) EF_HIP(c, hipEventRecord(c->ev_track_done, s));
  timer_end(c, "feedbackBuffers");
  return EF_OK;
}
// getIncrementalTransformation as a replayed hipGraph: captured once per pyramid parity (the SO(3) reference / frame intensity buffers swap
// every frame) and set of knobs, replayed from then on
int track_replayed(ef_ctx* c, const eft::TrackParams& tp, eft::TrackTail* tail) {
  hipStream_t s = c->stream;
  // key: which of the two intensity pyramids is "next" this frame + the knobs baked into the launch arguments
  const void* key = c->pyr.nextImage[0];
  ef_ctx::TrackGraph* g = nullptr;
  for (auto& cand : c->tgraph)
    if (cand.exec && cand.key == key && !memcmp(&cand.tp, &tp, sizeof(tp))) g = &cand;
  if (!g) {
    g = (c->tgraph[0].exec && c->tgraph[0].key != key) ? &c->tgraph[1] : &c->tgraph[0];
    if (g->exec) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }
    eft::track_prepare(c->pyr, tp, s);   // (a script switch clears the exchange areas: outside the capture, not replayed with it — ADVICE r5)
    eft::Pyramid pyr_copy = c->pyr;   // track() swaps the copy's pointers; the real swap is done below
    hipGraph_t graph = nullptr;
    EF_HIP(c, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    g->tail = eft::track(pyr_copy, c->st, c->intr, tp, s, nullptr);
    g->plan = pyr_copy.plan;
    hipError_t ce = hipStreamEndCapture(s, &graph);   // always ends the capture, whatever was recorded
    if (ce == hipSuccess) ce = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (ce != hipSuccess) {
      g->exec = nullptr;
      c->err = std::string("hipGraph capture of the tracker: ") + hipGetErrorString(ce);
      return EF_EHIP;
    }
    g->key = key;
    memcpy(&g->tp, &tp, sizeof(tp));
  }
  EF_HIP(c, hipGraphLaunch(g->exec, s));
  eft::track_swap(c->pyr, tp);
  c->pyr.plan = g->plan;
  *tail = g->tail;
  return EF_OK;
}
// The frame-to-model tracker (ElasticFusion.cpp:300-325): model-side maps, pyramids, getIncrementalTransformation, its tail
int track_frame(ef_ctx* c, const FramePlan& f, const eft::FramePreprocess& fp, float weightMultiplier, int log_slot) {
  hipStream_t s = c->stream;
  eft::TrackParams tp = track_params(c);
  tp.rgbOnly = c->cfg.rgb_only != 0; tp.pyramid = c->cfg.pyramid != 0; tp.fastOdom = c->cfg.fast_odom != 0; tp.so3 = c->cfg.so3 != 0;
  tp.icpWeight = c->cfg.icp_weight;
  const bool rgb = tp.rgbOnly || tp.icpWeight < 100;
  timer_begin(c, "odomInit");
  eft::init_icp_model(c->pyr, (const float*)c->pm.vertex, (const float*)c->pm.normal, (const float*)c->fm.vertex,
                      (const float*)c->fm.normal, c->st, 6.0f /* maxDepthRGB, RGBDOdometry.cpp:42 */, s, (const uint8_t*)c->pm.image,
                      (const uint8_t*)c->fm.image, c->cfg.frame_to_frame_rgb != 0, f.joint_inputs ? &fp : nullptr, c->tally_pending);
  c->tally_pending = false;
  if (f.overlap) {
    eft::build_pyramids_model_side(c->pyr, s);
    EF_HIP(c, hipStreamWaitEvent(s, c->ev_input_done, 0));
  } else {
    eft::build_pyramids(c->pyr, c->img.depth_filtered, c->intr, c->maxDepthProcessed, s, rgb);
  }
  if (rgb && f.overlap) eft::init_rgb_sobel(c->pyr, s);
  timer_end(c, "odomInit");
  timer_begin(c, "odom");
  eft::TrackTail tail{};
  if (f.replay) {
    tp.persistent = 0;
    EF_TRY(track_replayed(c, tp, &tail));
  } else {
    tail = eft::track(c->pyr, c->st, c->intr, tp, s, f.sample ? &c->sample_step.probe : nullptr,
                      f.sample && c->sample_all.probe.start ? &c->sample_all.probe : nullptr);
  }
  eft::track_end(c->st, tail, rgb, weightMultiplier, log_slot >= 0 ? c->traj : nullptr, log_slot, s, eft::tracker_abort_word(c->pyr), c->d_abort);
  timer_end(c, "odom");
  return EF_OK;
}
// ElasticFusion.cpp:326-366: the tracker's verdict on itself, read back where the reference reads lastICPError / getCovariance()
int reloc_verdict(ef_ctx* c) {
  c->tracking_ok = true;
  if (!c->reloc) return EF_OK;
  EF_TRY(read_state(c, c->st, &c->h_reloc));
  c->tracking_ok = c->h_reloc.lastICPError < 1e-04;
  if (!c->lost) {
    if (!reloc_covariance_ok(c->h_reloc)) c->tracking_ok = false;
    if (!c->tracking_ok) {
      if (++c->tracking_count > 10) c->lost = true;
    } else {
      c->tracking_count = 0;
    }
  } else if (c->last_frame_recovery) {
    if (!reloc_covariance_ok(c->h_reloc)) c->tracking_ok = false;
    if (c->tracking_ok) {
      c->lost = false;
      c->tracking_count = 0;
    }
    c->last_frame_recovery = false;
  }
  return EF_OK;
}
// ElasticFusion.cpp:387-527: the global closure against the fern database, then — unless it produced a graph — the local one
int close_loops(ef_ctx* c, int log_slot) {
  int fern_graph = 0;
  if (c->closure) {   // :387-445: predict() with its fill-in at the new pose, then the fern database
    timer_begin(c, "globalLoop");
    do_predict(c, false);
    c->last_frame_recovery = false;                                                           // :393
    const int r = global_loop_closure(c, log_slot, &fern_graph);
    timer_end(c, "globalLoop");
    if (r != EF_OK) return r;
  }
  if (c->lost || fern_graph) {   // :447: a lost camera closes no local loop, nor does a frame whose fern left a graph (rawGraph.size() != 0)
    memset(&c->loop, 0, sizeof(c->loop));
    return EF_OK;
  }
  timer_begin(c, "localLoop");
  const int r = local_loop_closure(c, log_slot, c->closure != nullptr);
  timer_end(c, "localLoop");
  return r;
  return EF_OK;
}
// ElasticFusion.cpp:536-585: predictIndices, fuse, predictIndices, a pending deformation, clean
void fuse_frame(ef_ctx* c, const FramePlan& f) {
  hipStream_t s = c->stream;
  const bool keyed = f.keyed, sample_splat = f.sample && c->sample_splat.probe.start;
  timer_begin(c, "indexMap");
  efm::IndexMaps im_assoc = c->im;   // what the association taps: no colour / time stream (the second predictIndices below writes all four maps)
  im_assoc.color_time = nullptr;
  const efm::KeyedIndex key_assoc{c->zbuf_assoc, c->st->T_cw, c->maps[c->cur]}, key_clean{c->zbuf_clean, c->st->T_cw, c->maps[c->cur]};
  efm::predict_indices(c->cam, c->st->T_cw, c->tick, c->maps[c->cur], &c->st->map_counts[c->cur], c->maxDepthProcessed, c->cfg.time_delta,
                       keyed ? c->zbuf_assoc : c->zbuf, im_assoc, s, sample_splat ? &c->sample_splat.probe : nullptr, nullptr, nullptr, !keyed);
  timer_end(c, "indexMap");
  timer_begin(c, "Fuse::Data+Update");
  efm::fuse(c->cam, c->st->pose_f, c->tick, c->img.rgb, c->img.depth_metric, c->img.depth_metric_filtered, c->im, c->maxDepthProcessed,
            &c->st->weighting, c->maps[c->cur], &c->st->map_counts[c->cur], c->cand, c->winner, s, f.defer_merge,
            keyed ? &key_assoc : nullptr, keyed ? c->zbuf_clean : nullptr);
  if (c->reference_download && !f.defer_merge) efm::copy_map(c->maps[c->cur], &c->st->map_counts[c->cur], c->shadow, s);
  timer_end(c, "Fuse::Data+Update");
  timer_begin(c, "indexMap2");
  efm::predict_indices(c->cam, c->st->T_cw, c->tick, c->maps[c->cur], &c->st->map_counts[c->cur], c->maxDepthProcessed, c->cfg.time_delta,
                       keyed ? c->zbuf_clean : c->zbuf, c->im, s, nullptr, f.defer_merge ? &c->cand : nullptr, c->winner, !keyed);
  // (`im` now is what this frame's second predictIndices wrote, or — keyed — is still to be resolved from zbuf_clean when somebody asks)
  c->im_pending = keyed;
  c->im_map = c->cur;
  if (c->reference_download && f.defer_merge) efm::copy_map(c->maps[c->cur], &c->st->map_counts[c->cur], c->shadow, s);
  timer_end(c, "indexMap2");
  // a pending deformation (ElasticFusion.cpp:558-585): re-predict the depth of the surfels outside the time window, then let
  // clean() move every kept surfel with the graph
  efm::Deformation def{c->graph_dev, c->graph_nodes, c->synth_depth, c->graph_is_fern, c->maxDepthProcessed};
  if (c->graph_nodes > 0 && !c->graph_is_fern)
    efm::synthesize_depth(c->cam, c->st->T_cw, c->maps[c->cur], &c->st->map_counts[c->cur], c->maxDepthProcessed, c->cfg.confidence, c->tick,
                          c->tick - c->cfg.time_delta, 65535, c->zbuf, c->synth_depth, s, c->rays);
  timer_begin(c, "Fuse::Copy");
  efm::clean(c->cam, c->st->T_cw, c->tick, c->im, c->cfg.confidence, c->cfg.time_delta, c->maps[c->cur], &c->st->map_counts[c->cur], c->cand,
             c->winner, c->maps[c->cur ^ 1], &c->st->map_counts[c->cur ^ 1], c->capacity, c->cs, c->overflow, s,
             c->graph_nodes > 0 ? &def : nullptr, keyed ? &key_clean : nullptr, keyed ? c->zbuf_assoc : nullptr, keyed ? c->im_T16 : nullptr);
  c->cur ^= 1;
  timer_end(c, "Fuse::Copy");
}
// ElasticFusion.cpp:588-618: predict() for the next frame, the closure's end-of-frame record, the tick
int end_of_frame(ef_ctx* c, const FramePlan& f) {
  timer_begin(c, "IndexMap::ACTIVE");
  do_predict(c);  // ElasticFusion.cpp:599
  timer_end(c, "IndexMap::ACTIVE");
  if (c->closure) {   // :588-589, 593, 609-618: pose -> trajectory, graph nodes re-sampled, final fill-in view -> Ferns::addFrame
    timer_begin(c, "ferns");
    int r = flush_end_record(c);           // (normally long done: the frame's closures synchronised)
    if (r == EF_OK) r = enqueue_end_record(c);   // no synchronisation: looked at when the next frame first waits for the stream
    timer_end(c, "ferns");
    if (r != EF_OK) return r;
  }
  if (f.frame_done_event) EF_HIP(c, hipEventRecord(c->ev_frame_done[c->frame_parity], c->stream));
  c->events_live = f.want_events;
  if (!c->lost) c->tick++;   // :601-604
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// ElasticFusion::processFrame (ElasticFusion.cpp:270-607).  rgb_src / depth_src: host (pinned staging) or device pointers, `kind` says which
int process_frame(ef_ctx* c, const uint8_t* rgb_src, const uint16_t* depth_src, hipMemcpyKind kind, int64_t timestamp,
                  float weightMultiplier, const double* in_T_wc, hipEvent_t images_ready = nullptr) {
  ++c->map_gen;   // fusion, clean and deformations change rows and positions: a spatial index built before this frame is stale
  // a persistent tracker launch of an EARLIER frame gave up waiting after admission (a protocol failure, sticky: every later launch of that
  // instance returns at once): k_track_end has copied the flag into host-mapped memory; reported here, where the front end calls
  // (class ElasticFusion::processFrame throws), without synchronising — ef_synchronize reports the same condition for the frames in flight
  if ((c->h_abort && (c->h_abort[0] | c->h_abort[1] | c->h_abort[2])) || c->pyr.sticky_abort || c->pyr2.sticky_abort || c->pyr3.sticky_abort) {
    c->err = "a persistent tracker launch of an earlier frame timed out waiting for another workgroup after its whole grid had reported in (a protocol "
             "failure, not a busy chip: that case runs on one workgroup, ef_get_tracker_fallbacks): the poses and the map since then are invalid; "
             "recreate the context (ef_set_persistent_tracker(ctx, 0) selects the launch-per-step script)";
    return EF_EHIP;
  }
  const FramePlan f{c, kind, in_T_wc != nullptr};
  eft::FramePreprocess fp;
  EF_TRY(input_stage(c, f, rgb_src, depth_src, images_ready, &fp));
  // t_T_wc.push_back / poseLogTimes.push_back, ElasticFusion.cpp:588-589: the pose is logged by the kernel that produces it
  if ((int)c->stamps.size() >= c->traj_cap) EF_TRY(grow_trajectory(c));   // (t_T_wc grows without bound in the reference: the device log doubles, every 2^16+ frames)
  const int log_slot = (int)c->stamps.size();
  c->stamps.push_back(timestamp);
  if (c->tick == 1) {
    EF_TRY(first_frame(c, f, log_slot));
  } else {
    if (!in_T_wc) {
      EF_TRY(track_frame(c, f, fp, weightMultiplier, log_slot));
      EF_TRY(reloc_verdict(c));
    } else {
      c->tracking_ok = true;   // :300: an injected pose is never judged
      if (f.overlap) EF_HIP(c, hipStreamWaitEvent(c->stream, c->ev_input_done, 0));
      eft::pose_injected(c->st, in_T_wc, true, weightMultiplier, true, log_slot >= 0 ? c->traj : nullptr, log_slot, c->stream);
    }
    // from here on nothing of this frame reads the frame-side pyramids: the next frame's input stage may start
    if (f.want_events) EF_HIP(c, hipEventRecord(c->ev_track_done, c->stream));
    // mid-frame predict() of ElasticFusion.cpp:387 is dead work without loop closure: skipped (DESIGN.md)
    if (c->cfg.close_loops) EF_TRY(close_loops(c, log_slot));
    if (!c->cfg.rgb_only && c->tracking_ok && !c->lost && !c->track_only) fuse_frame(c, f);   // ElasticFusion.cpp:536-585
    c->graph_nodes = 0;   // rawGraph is a local of processFrame: a deformation is applied by this frame's clean() or never
  }
  return end_of_frame(c, f);
}
}  // namespace

extern "C" {

int ef_process_frame(ef_ctx* c, const uint8_t* rgb, const uint16_t* depth, int64_t timestamp, float wm, const double* T) {
  if (!c || !rgb || !depth) return EF_EINVAL;
  DeviceGuard dg_(c);
  const size_t P = (size_t)c->cam.cols * c->cam.rows;
  // The reference uploads inside processFrame (ElasticFusion.cpp:278-280: three texture uploads, blocking).  Here (round 6): the caller's images go
  // into slot r of a ring of pinned staging pairs, are uploaded on copy_stream into the ring's device landing pair — beside the previous
  // frames' kernels — and the frame script reads the landing pair IN PLACE (the bilateral filter reads the depth, the intensity kernel reads the
  // colours and keeps the context's copy: no device-side copy, exactly the device-pointer script).  The compute stream waits for the upload
  // (one barrier packet); nothing waits on the host unless the caller is a whole ring ahead of the GPU: slot r is free once the frame that used
  // it last has been read, which that frame's prediction launch reports through a host-mapped word (no event on the compute stream: an event
  // record there costs a 6 us bubble, profiles/r06f_timeline_single_stream.txt).
  const RingSlot& slot = c->ring[c->host_seq % ef_ctx::RING];
  if (c->host_seq >= (unsigned)ef_ctx::RING) {
    const unsigned need = c->host_seq - ef_ctx::RING + 1u;   // the marker the last user of slot r leaves
    volatile unsigned* seen = c->h_consumed;
    int spins = 0;
    while ((int)(*seen - need) < 0) {
      if (++spins > 20000) {   // (~ms: that frame ended early on an error path, or the marker is not visible: join the streams instead)
        EF_HIP(c, hipStreamSynchronize(c->stream));
        break;
      }
      if (spins > 64) std::this_thread::yield();
    }
  }
  memcpy(slot.h_rgb, rgb, P * 3);
  memcpy(slot.h_depth, depth, P * 2);
  EF_HIP(c, hipMemcpyAsync(slot.d_depth, slot.h_depth, P * 2, hipMemcpyHostToDevice, c->copy_stream));
  EF_HIP(c, hipMemcpyAsync(slot.d_rgb, slot.h_rgb, P * 3, hipMemcpyHostToDevice, c->copy_stream));
  EF_HIP(c, hipEventRecord(slot.ev_h2d, c->copy_stream));
  c->mark_value = c->host_seq + 1u;
  c->host_seq++;
  return process_frame(c, slot.d_rgb, slot.d_depth, hipMemcpyDeviceToDevice, timestamp, wm, T, slot.ev_h2d);
}
int ef_process_frame_dev(ef_ctx* c, const uint8_t* rgb_dev, const uint16_t* depth_dev, int64_t timestamp, float wm, const double* T) {
  if (!c || !rgb_dev || !depth_dev) return EF_EINVAL;
  DeviceGuard dg_(c);
  return process_frame(c, rgb_dev, depth_dev, hipMemcpyDeviceToDevice, timestamp, wm, T);
}
int ef_predict(ef_ctx* c) {
  if (!c) return EF_EINVAL;
  DeviceGuard dg_(c);
  EF_HIP(c, hipMemsetAsync(&c->st->dense_count, 0, sizeof(unsigned), c->stream));
  return do_predict(c);
}

}  // extern "C"
