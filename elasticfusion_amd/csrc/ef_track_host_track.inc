// Host code of the tracker, part 3 of 3 (included by ef_track_kernels.hip behind ef_track_host_inputs.inc): getIncrementalTransformation
// (RGBDOdometry.cpp:259-571) entirely enqueued — the script plan, the three launch routines track() chooses from, the sticky words of the
// persistent launches, track_end and the pose launchers.
namespace {
constexpr int SO3_LEVEL = 2;   // the SO(3) pre-alignment works on the coarsest intensity images (RGBDOdometry.cpp:284-369)

template <int PPT>
void launch_step(const Pyramid& p, TrackState* st, int level, int cur, int slots_out, const StepArgs& A, hipStream_t s) {
  const int cols = p.W(level), rows = p.H(level), N = cols * rows;
  ResidualPackedView RV{p.rgbMask[level], p.lastDepth[level], p.nextDepth[level], p.lastImage[level], p.nextImage[level], p.corres[level], cols, rows,
                        0.07f /* maxDepthDeltaRGB, RGBDOdometry.cpp:41 */};
  const int grid = A.has_body ? ceil_div(N, REDUCE_BLOCK * PPT) : 1;
  hipLaunchKernelGGL(k_track_step<PPT>, dim3(grid), dim3(REDUCE_BLOCK), 0, s, RV, st, (const GNState*)&st->gn[cur], &st->gn[cur ^ 1],
                     (const float*)p.partials, (const int*)&st->rgb_slots[slots_out ^ 1][0][0], &st->rgb_slots[slots_out][0][0], A);
}
// One Gauss-Newton iteration of the launch-per-step script = three launches: the update step of the PREVIOUS iteration on one workgroup
// (k_track_step, head only; none in the call's first iteration), the correspondence search (k_track_step, body only) and the normal equations
// (k_se3_accum); with tp.fused_step two: workgroup 0 of the search launch evaluates the update and hands it to the others in-launch.
// `it` = index of the iteration within the call; cur = GNState buffer to read.  Returns the buffer the NEXT step reads.
int launch_iteration(const Pyramid& p, TrackState* st, int level, Intr kl, const TrackParams& tp, bool icp, bool rgb, int it, int cur,
                     int prev_level, hipStream_t s, KernelProbe* probe) {
  const int cols = p.W(level), rows = p.H(level), N = cols * rows;
  const bool sample = probe && level == 0 && probe->used < probe->capacity;
  const int sp = it & 1;
  const bool level_changes = level != prev_level;
  StepArgs A{it > 0, rgb, icp, rgb, tp.rgbOnly, tp.icpWeight, kl, level_changes, it, op_groups(p.W(prev_level) * p.H(prev_level))};
  // (evaluating the update redundantly at the head of EVERY workgroup of the search launch was built and measured in round 2: 888 vs 1322
  // frames/s, DESIGN.md 6; dropped from the source in round 3)
  if (A.has_head && A.has_body && tp.fused_step && !tp.rgbOnly) {
    if (N >= 256 * 1024) launch_step<2>(p, st, level, cur, sp, A, s);
    else launch_step<1>(p, st, level, cur, sp, A, s);
    cur ^= 1;
  } else {
    if (A.has_head) {
      StepArgs H = A;
      H.has_body = false;
      launch_step<1>(p, st, level, cur, sp, H, s);
      cur ^= 1;
    }
    if (A.has_body) {
      StepArgs B = A;
      B.has_head = false;
      // (four times fewer, four times fatter wavefronts — PPT 8 / 4 — measured 4.5 % slower end to end: DESIGN.md 6)
      if (N >= 256 * 1024) launch_step<2>(p, st, level, cur, sp, B, s);
      else launch_step<1>(p, st, level, cur, sp, B, s);
    }
  }
  const GNState* g = &st->gn[cur];
  IcpView IV{p.vmap_curr[level], p.nmap_curr[level], p.vmap_g_prev[level], p.nmap_g_prev[level], cols, rows, kl, tp.distThres, tp.angleThres, sq_le_max(tp.distThres), sq_lt_max(tp.angleThres)};
  RgbView GV{p.corres[level], p.lastDepth[level], nullptr, p.dIdx[level], p.dIdy[level], cols, rows, kl, 1.0f / 8.0f};
  Se3Inputs in{g->Rcurr, g->tcurr, st->Rprev_inv, st->tprev, &st->rgb_slots[sp][0][0], &g->rgb_broken, 0.f, tp.rgbOnly};
  in.slots_zero = &st->rgb_slots[sp ^ 1][0][0];
  const Se3Out out{p.partials};
  hipEvent_t e0 = sample ? probe->start[probe->used] : nullptr, e1 = sample ? probe->stop[probe->used] : nullptr;
  if (sample) probe->used++;
  with_terms(icp, rgb, [&](auto I, auto R) { launch_accum<decltype(I)::value, decltype(R)::value, true>(IV, GV, in, N, out, s, e0, e1); });
  return cur;
}

std::mutex g_chain_mu;                 // the per-device chain of persistent launches (see launch_persistent())
hipStream_t g_chain_last[64] = {};
bool g_chain_has[64] = {};
hipEvent_t g_chain_ev[64] = {};
inline bool last_valid_other(int dev, hipStream_t s) { return g_chain_has[dev] && g_chain_last[dev] != s; }
}  // namespace
void persistent_chain_forget(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_chain_mu);
  for (int d = 0; d < 64; ++d)
    if (g_chain_has[d] && g_chain_last[d] == s) { g_chain_has[d] = false; g_chain_last[d] = nullptr; }
}

namespace {
// The sticky words of a tracker instance live in its exchange areas (Pyramid::partials), where the script it ran last keeps them: the
// 256-workgroup persistent launches in FtSync; every other state of a reference-order instance means round 3's launch of the small levels
// (k_track_small), which keeps an abort word and clocks of its own in PtSync and counts no fallbacks.
struct StickyWords {
  unsigned* abort;
  unsigned* fallbacks;           // null: this script counts none
  unsigned long long* clk;       // developer instrumentation (-DEF_STAGE_CLOCKS builds)
  int n_clk;
};
StickyWords sticky_base(const Pyramid& p) {
#ifndef EF_FAST_ORDER
  if (p.last_mode != 1) {
    char* y = (char*)(p.partials + 2 * PARTIAL_FLOATS);
    return {(unsigned*)(y + offsetof(PtSync, abort)), nullptr, (unsigned long long*)(y + offsetof(PtSync, clk)), 24};
  }
#endif
  char* y = (char*)(p.partials + FT_SY_OFF);
  return {(unsigned*)(y + offsetof(FtSync, abort)), (unsigned*)(y + offsetof(FtSync, fallbacks)), (unsigned long long*)(y + offsetof(FtSync, clk)), 32};
}
// what device words hold once everything enqueued on s has run; false on a HIP error
bool read_words(void* out, const void* dev, size_t bytes, hipStream_t s) {
  return hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
}
}  // namespace
// device address of the sticky abort word of this tracker instance's persistent launches
unsigned* tracker_abort_word(const Pyramid& p) { return p.partials ? sticky_base(p).abort : nullptr; }
int tracker_aborted(const Pyramid& p, hipStream_t s) {
  if (p.sticky_abort) return 1;   // (carried over a script switch)
  if (!p.partials) return 0;
  unsigned flag = 0;
  if (!read_words(&flag, sticky_base(p).abort, sizeof(flag), s)) return -1;
  return flag != 0 ? 1 : 0;
}
int tracker_fallbacks(const Pyramid& p, hipStream_t s) {
  if (!p.partials || p.last_mode != 1) return (int)p.fallbacks_base;   // (what earlier persistent launches of this instance counted)
  unsigned n = 0;
  if (!read_words(&n, sticky_base(p).fallbacks, sizeof(n), s)) return -1;
  return (int)(n + p.fallbacks_base);
}
// developer instrumentation: the -DEF_STAGE_CLOCKS sums of the script the instance ran last (10 ns ticks; zeros in a normal build), read and reset
int tracker_small_clocks(const Pyramid& p, unsigned long long* out32, hipStream_t s) {
  if (!p.partials) return -1;
  const StickyWords w = sticky_base(p);
  for (int i = 0; i < 32; ++i) out32[i] = 0ull;
  if (!read_words(out32, w.clk, w.n_clk * sizeof(unsigned long long), s)) return -1;
  return hipMemset(w.clk, 0, w.n_clk * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}

// Which script a call runs decides what the exchange areas (Pyramid::partials) hold: 1 = the granules of a 256-workgroup persistent launch, 0 = the
// per-step kernels' plain partials / k_track_small's barrier words.  A context that changes scripts gets the areas cleared (tags must never match
// by accident; the other script's words start from zeros) — and the sticky words they hold, the abort flag and the fallback count, carried over
// on the host first (ADVICE r5: a clear used to erase them silently): one synchronisation per switch, which happens when an option is toggled or
// a sampled frame leaves a graph-replaying context's script, never in a steady replay.  Under a CALLER's capture nothing can be read back: the
// clear is recorded (the caller's graph then runs the launch-per-step script, which keeps no sticky word).
static void switch_script(Pyramid& p, int target, hipStream_t s, bool capturing) {
  if (p.last_mode == target) return;
  if (p.partials) {
    if (!capturing) {
      if (tracker_aborted(p, s) > 0) p.sticky_abort = 1u;
      const int f = tracker_fallbacks(p, s);
      if (f > 0) p.fallbacks_base = (unsigned)f;   // (tracker_fallbacks already includes the earlier base)
    }
    (void)hipMemsetAsync(p.partials, 0, sizeof(float) * PARTIAL_ALLOC_FLOATS, s);
  }
  p.last_mode = target;
}

namespace {
// What one getIncrementalTransformation call runs, decided once from the knobs, the capture state of the stream and the pyramid.
struct ScriptPlan {
  bool icp, rgb;                 // the terms of the normal equations, RGBDOdometry.cpp:266-267
  int iterations[NUM_PYRS];      // per level, RGBDOdometry.cpp:371-373
  int first_level, n_total;      // the coarsest level that iterates; iterations of the call
  // 0: every step is its own launch.
  // 1: the WHOLE call — k_track_begin, the SO(3) loop, every iteration of every level — as one persistent launch of 256 co-resident workgroups
  //    (fast order: k_track_fast, ef_track_fast_persistent.inc; reference order: k_track_ref, ef_track_ref_persistent.inc).
  // 2: (reference-order builds) round 3's launch of the small levels on 128 workgroups (k_track_small): k_track_begin, the SO(3) loop and the
  //    leading iterations whose level fits (coarse to fine: once a level is too large, it and everything after it run one launch per step).
  // All three add in the same order: same results.
  int script;
  int n_small;                   // script 2: iterations inside k_track_small (0 otherwise) ...
  unsigned levels;               // ... and their levels, two bits each (PtArgs::levels)
  int exchange_mode() const { return script == 1 ? 1 : 0; }   // what Pyramid::last_mode becomes (see switch_script)
};
ScriptPlan plan_script(const Pyramid& p, const TrackParams& tp, bool capturing) {
  ScriptPlan sp{};
  sp.icp = !tp.rgbOnly && tp.icpWeight > 0;
  sp.rgb = tp.rgbOnly || tp.icpWeight < 100;
  sp.iterations[0] = tp.fastOdom ? 3 : 10;
  sp.iterations[1] = tp.pyramid ? 5 : 0;
  sp.iterations[2] = tp.pyramid ? 4 : 0;
  for (int i = NUM_PYRS - 1; i >= 0; --i)
    if (sp.iterations[i] > 0) { sp.first_level = i; break; }
  sp.n_total = sp.iterations[0] + sp.iterations[1] + sp.iterations[2];
  int asked = tp.persistent;
#ifdef EF_FAST_ORDER
  if (asked) asked = 1;   // (the fast order has no launch of the small levels: 2 means 1)
#endif
  // A caller capturing the stream into a graph of its own gets the launch-per-step script: the persistent launches take a fresh epoch per launch
  // and wait for the device's chain event, neither of which a replayed graph can carry.  rgbOnly keeps it too: its per-level "break"
  // bookkeeping is not in the persistent kernels.
  if (capturing || tp.rgbOnly) asked = 0;
  if (asked == 1 && sp.n_total <= FT_MAX_ITER) {
    sp.script = 1;
  } else if (asked == 2) {
    bool fits = true;
    for (int i = NUM_PYRS - 1; i >= 0 && fits; --i) {
      if (sp.iterations[i] == 0) continue;
      fits = p.W(i) * p.H(i) <= PT_MAX_PIXELS && sp.n_small + sp.iterations[i] <= PT_MAX_ITER;
      for (int j = 0; fits && j < sp.iterations[i]; ++j) sp.levels |= (unsigned)i << (2 * sp.n_small++);
    }
    if (sp.n_small > 0 || tp.so3) sp.script = 2;   // (nothing for the launch to do otherwise)
  }
  return sp;
}
// the level table and the parameters FtArgs and PtArgs share, by member name (the two structs are kernel ABI and stay apart)
template <class Args>
void fill_track_args(Args& A, const Pyramid& p, Intr k, const TrackParams& tp, const ScriptPlan& sp) {
  for (int i = 0; i < NUM_PYRS; ++i)
    A.L[i] = PtLevel{p.vmap_curr[i], p.nmap_curr[i], p.vmap_g_prev[i], p.nmap_g_prev[i], p.rgbMask[i], p.lastDepth[i], p.nextDepth[i],
                     p.lastImage[i], p.nextImage[i], p.corres[i], p.dIdx[i], p.dIdy[i], p.W(i), p.H(i), intr_level(k, i)};
  A.so3 = tp.so3;
  A.so3_last = p.lastNextImage[SO3_LEVEL];
  A.so3_next = p.nextImage[SO3_LEVEL];
  A.so3_cols = p.W(SO3_LEVEL);
  A.so3_rows = p.H(SO3_LEVEL);
  A.kso3 = intr_level(k, SO3_LEVEL);
  A.kfirst = intr_level(k, sp.first_level);
  A.icpWeight = tp.icpWeight;
  A.distThres = tp.distThres;
  A.angleThres = tp.angleThres;
  A.dist2Max = sq_le_max(tp.distThres);
  A.sine2Max = sq_lt_max(tp.angleThres);
  A.partials = p.partials;
  A.out_cur = 0;
}

// script 1: the persistent launch of the whole call
TrackTail launch_persistent(Pyramid& p, TrackState* st, Intr k, const TrackParams& tp, const ScriptPlan& sp, hipStream_t s, KernelProbe* probe_all) {
  FtArgs FA{};
  fill_track_args(FA, p, k, tp, sp);
  int n = 0;
  for (int i = NUM_PYRS - 1; i >= 0; --i)
    for (int j = 0; j < sp.iterations[i]; ++j) FA.levels |= (unsigned long long)i << (2 * n++);
  FA.n_iter = n;
  if (p.epoch > 0xFFFFFFFFu - 2u * FT_EPOCHS) p.epoch = 1;   // (a slot keeps a 2^32-launch-old tag only if nobody wrote it since)
  FA.epoch = p.epoch;
  p.epoch += FT_EPOCHS;
  FA.empty_model_flag = tp.so3 ? nullptr : tp.empty_model_flag;   // (the SO(3) loop looks at the frame-side images only: not covered by the shortcut)
  FA.empty_model_value = tp.empty_model_value;
#ifndef EF_FAST_ORDER
  // level-resident pixel data (ef_track_ref_persistent.inc, rt_res_mode): the largest need of a level whose slots fit — both sides, or the
  // ICP side alone (1280 x 960 level 0) — under what the chip gives one workgroup beside the kernel's static LDS
  unsigned res_bytes = 0;
  if (!tp.no_resident) p.plan.res_budget = rt_res_budget();
  if (!tp.no_resident && rt_res_budget() > 0) {
    for (int i = 0; i < NUM_PYRS; ++i) {
      if (sp.iterations[i] == 0) continue;
      const unsigned S = (unsigned)(((p.W(i) * p.H(i) + VTHREADS - 1) / VTHREADS + 3) >> 2);
      const unsigned n2 = S * ((sp.icp ? RT_ICP_STEP_BYTES : 0) + (sp.rgb ? RT_RGB_STEP_BYTES : 0)), n1 = sp.icp ? S * RT_ICP_STEP_BYTES : 0u;
      const unsigned need = n2 <= rt_res_budget() ? n2 : (n1 <= rt_res_budget() ? n1 : 0u);
      res_bytes = need > res_bytes ? need : res_bytes;
    }
  }
  FA.res_bytes = res_bytes;
  p.plan.res_bytes = res_bytes;
#endif
  p.plan.levels = FA.levels;
  const bool sample_all = probe_all && probe_all->used < probe_all->capacity;
  hipEvent_t e0 = sample_all ? probe_all->start[probe_all->used] : nullptr, e1 = sample_all ? probe_all->stop[probe_all->used] : nullptr;
  if (sample_all) probe_all->used++;
  {
    // The launch needs its 256 workgroups resident TOGETHER, one per CU.  Two such launches in flight at once (two contexts of this
    // process, each on its own stream) could each hold a part of the chip and wait for the rest for ever, so the persistent launches of
    // a device are chained, in the order the host enqueues them, through one event per device: a launch first waits (on the GPU, not on
    // the host) for the previous one, whatever stream that ran on.  On one stream this is a no-op.  Ordinary kernels of other streams
    // only delay it (they end without waiting for anybody); another PROCESS's persistent kernels are outside this chain: bounded spins,
    // FtSync::abort, tracker_aborted.
    // Round 6: the chain costs nothing while ONE stream launches them (the common case: an event record between two kernels of a stream is a
    // barrier packet, measured as a 6 us bubble behind every tracker launch in profiles/r06f_timeline_single_stream.txt) — the dependency is
    // created by the launch that finds ANOTHER stream's launch before it: it records the event on that stream now (everything enqueued there
    // so far, the persistent launch included) and makes its own stream wait for it.  persistent_chain_forget() drops a stream that is destroyed.
    std::lock_guard<std::mutex> lk(g_chain_mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < 64) {   // (a device index beyond the table: no chain, the bounded spins remain)
      hipStream_t& last = g_chain_last[dev];
      hipEvent_t& ev = g_chain_ev[dev];
      if (last_valid_other(dev, s)) {
        if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
        if (ev && hipEventRecord(ev, last) == hipSuccess) (void)hipStreamWaitEvent(s, ev, 0);
        (void)hipGetLastError();
      }
      last = s;
      g_chain_has[dev] = true;
    }
    with_terms(sp.icp, sp.rgb, [&](auto I, auto R) {
      constexpr bool ICP = decltype(I)::value, RGB = decltype(R)::value;
#ifdef EF_FAST_ORDER
      hipExtLaunchKernelGGL((k_track_fast<ICP, RGB>), dim3(FT_WGS), dim3(FT_BLOCK), 0, s, e0, e1, 0, FA, st);
#else
      hipExtLaunchKernelGGL((k_track_ref<ICP, RGB>), dim3(FT_WGS), dim3(FT_BLOCK), res_bytes, s, e0, e1, 0, FA, st);
#endif
    });
  }
#ifdef EF_FAST_ORDER
  // (returns at once unless the launch above found part of the chip taken: see its admission step)
  with_terms(sp.icp, sp.rgb, [&](auto I, auto R) {
    hipLaunchKernelGGL((k_track_serial<decltype(I)::value, decltype(R)::value>), dim3(1), dim3(REDUCE_BLOCK), 0, s, p.partials, st, FA.epoch);
  });
#endif
  track_swap(p, tp);
  TrackTail tail{0, (n - 1) & 1, n > 0, sp.icp, sp.rgb, tp.rgbOnly, tp.icpWeight, intr_level(k, 0), p.partials + FT_P_OFF};
  tail.ng = 1;   // the reducers of the last iteration left the TOTALS in column 0
#ifndef EF_FAST_ORDER
  tail.merged_end = true;   // (the one-workgroup fallback rides at the head of track_end's launch: k_track_ref_end)
  tail.epoch = FA.epoch;
  tail.partials = p.partials;
#endif
  return tail;
}
// script 0's head: k_track_begin and the SO(3) loop, one launch each
void launch_begin_so3(const Pyramid& p, TrackState* st, Intr k, const TrackParams& tp, const ScriptPlan& sp, hipStream_t s) {
  const Intr kso3 = intr_level(k, SO3_LEVEL), kfirst = intr_level(k, sp.first_level);
  const int cols = p.W(SO3_LEVEL), rows = p.H(SO3_LEVEL);
  hipLaunchKernelGGL(k_track_begin, dim3(1), dim3(64), 0, s, st, tp.so3, kso3, kfirst);
  if (!tp.so3) return;
  for (int i = 0; i < 10; ++i)
    hipLaunchKernelGGL(k_so3_iteration, dim3(so3_grid(cols * rows)), dim3(SO3_BLOCK), 0, s, (const uint8_t*)p.lastNextImage[SO3_LEVEL],
                       (const uint8_t*)p.nextImage[SO3_LEVEL], cols, rows, kso3, kfirst, i, st, p.partials);
}
// script 2's head: k_track_begin, the SO(3) loop and the first sp.n_small iterations in one launch
void launch_small_levels(const Pyramid& p, TrackState* st, Intr k, const TrackParams& tp, const ScriptPlan& sp, hipStream_t s) {
#ifndef EF_FAST_ORDER   // (the fast order has no such kernel: plan_script() plans no script 2 there)
  PtArgs PA{};
  fill_track_args(PA, p, k, tp, sp);
  PA.n_iter = sp.n_small;
  PA.levels = sp.levels;
  with_terms(sp.icp, sp.rgb, [&](auto I, auto R) {
    hipLaunchKernelGGL((k_track_small<decltype(I)::value, decltype(R)::value>), dim3(PT_WGS), dim3(PT_BLOCK), 0, s, PA, st);
  });
#endif
}
// scripts 0 and 2: every iteration the head did not run, one launch per step
TrackTail launch_steps(Pyramid& p, TrackState* st, Intr k, const TrackParams& tp, const ScriptPlan& sp, hipStream_t s, KernelProbe* probe) {
  int it = sp.n_small, cur = 0, done = 0;
  int prev_level = sp.n_small > 0 ? (int)((sp.levels >> (2 * (sp.n_small - 1))) & 3u) : sp.first_level;
  for (int i = NUM_PYRS - 1; i >= 0; --i) {
    const Intr kl = intr_level(k, i);
    for (int j = 0; j < sp.iterations[i]; ++j) {
      if (done++ < sp.n_small) continue;   // ran inside k_track_small
      cur = launch_iteration(p, st, i, kl, tp, sp.icp, sp.rgb, it, cur, prev_level, s, probe);
      prev_level = i;
      ++it;
    }
  }
  track_swap(p, tp);
  // the last iteration's update is evaluated at the head of k_track_end (track_end below)
  TrackTail tail{cur, (it - 1) & 1, it > 0, sp.icp, sp.rgb, tp.rgbOnly, tp.icpWeight, intr_level(k, 0), p.partials};
  tail.ng = op_groups(p.W(prev_level) * p.H(prev_level));
  return tail;
}
inline bool is_capturing(hipStream_t s) {
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &capture) == hipSuccess && capture != hipStreamCaptureStatusNone;
}
}  // namespace

void track_prepare(Pyramid& p, const TrackParams& tp, hipStream_t s) {
  switch_script(p, plan_script(p, tp, false).exchange_mode(), s, false);
}
TrackTail track(Pyramid& p, TrackState* st, Intr k, const TrackParams& tp, hipStream_t s, KernelProbe* probe, KernelProbe* probe_all) {
  const bool capturing = is_capturing(s);
  const ScriptPlan sp = plan_script(p, tp, capturing);
  switch_script(p, sp.exchange_mode(), s, capturing);   // another script of this instance may have left anything in the exchange areas
  p.plan = TrackerPlan{sp.script, sp.n_small, sp.n_total, sp.levels, 0u, p.plan.res_budget};
  if (sp.script == 1) return launch_persistent(p, st, k, tp, sp, s, probe_all);
  if (sp.script == 2) launch_small_levels(p, st, k, tp, sp, s);
  else launch_begin_so3(p, st, k, tp, sp, s);
  return launch_steps(p, st, k, tp, sp, s, probe);
}
// host-side tail of getIncrementalTransformation: the frame's intensity pyramid becomes the SO(3) reference of the next
// (RGBDOdometry.cpp:284-288 swaps lastNextImage / nextImage); separate so that a replayed hipGraph can do it without launching
void track_swap(Pyramid& p, const TrackParams& tp) {
  if (tp.so3)
    for (int i = 0; i < NUM_PYRS; ++i) { uint8_t* tmp = p.lastNextImage[i]; p.lastNextImage[i] = p.nextImage[i]; p.nextImage[i] = tmp; }
}

// exported for the context: finishing kernels
void track_end(TrackState* st, const TrackTail& u, bool rgb, float weightMultiplier, double* traj, int slot, hipStream_t s, const unsigned* abort_word,
               unsigned* abort_report) {
  const StepArgs A{u.has_head, false, u.icp, u.rgb, u.rgbOnly, u.icpWeight, u.k0, true, 63, u.ng};
  unsigned* report = abort_word ? abort_report : nullptr;
#ifndef EF_FAST_ORDER
  if (u.merged_end) {
    with_terms(u.icp, u.rgb, [&](auto I, auto R) {
      hipLaunchKernelGGL((k_track_ref_end<decltype(I)::value, decltype(R)::value>), dim3(1), dim3(FT_BLOCK), 0, s, u.partials, st, u.epoch, A, u.slots, rgb,
                         weightMultiplier, traj, slot, report);
    });
    return;
  }
#endif
  hipLaunchKernelGGL(k_track_end, dim3(1), dim3(REDUCE_BLOCK), 0, s, st, (const GNState*)&st->gn[u.cur], &st->gn[u.cur ^ 1], u.pairs,
                     (const int*)&st->rgb_slots[u.slots & 1][0][0], A, rgb, weightMultiplier, traj, slot, abort_word, report);
}
void pose_injected(TrackState* st, const double* T_wc16, bool save_prev, float weightMultiplier, bool with_weighting, double* traj, int slot,
                   hipStream_t s) {
  hipLaunchKernelGGL(k_pose_injected, dim3(1), dim3(64), 0, s, st, efl::se3_from_matrix(T_wc16), save_prev, weightMultiplier, with_weighting,
                     traj, slot);
}
void pose_restored(TrackState* st, const double* q4, const double* t3, hipStream_t s) {
  efl::SE3 T;
  for (int i = 0; i < 4; ++i) T.q[i] = q4[i];
  for (int i = 0; i < 3; ++i) T.t[i] = t3[i];
  hipLaunchKernelGGL(k_pose_injected, dim3(1), dim3(64), 0, s, st, T, false, 1.0f, false, (double*)nullptr, 0);
}
void copy_pose(TrackState* dst, const TrackState* src, hipStream_t s) { hipLaunchKernelGGL(k_copy_pose, dim3(1), dim3(64), 0, s, dst, src); }
void adopt_pose(TrackState* st, const TrackState* est, double* traj, int slot, hipStream_t s) {
  hipLaunchKernelGGL(k_adopt_pose, dim3(1), dim3(64), 0, s, st, est, traj, slot);
}
void sample_constraints(const float* vertex4, const uint16_t* old_time, int cols, int rows, int step, float* out4, hipStream_t s) {
  const int cw = cols / step, ch = rows / step;
  hipLaunchKernelGGL(k_sample_constraints, dim3(ceil_div(cw * ch, 256)), dim3(256), 0, s, (const float4*)vertex4, old_time, cols, cw, ch, step,
                     (float4*)out4);
}
void log_pose(const TrackState* st, double* traj, int slot, hipStream_t s) { hipLaunchKernelGGL(k_log_pose, dim3(1), dim3(64), 0, s, st, traj, slot); }
