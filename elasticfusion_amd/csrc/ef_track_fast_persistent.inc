// THE FAST ORDER, part 2: the persistent tracker — included by ef_track_kernels.hip behind k_track_small (EF_FAST_ORDER builds only)
// ------------------------------------------------------------------------------------------
// The WHOLE tracker as ONE persistent launch (round 4): k_track_begin, the <= 10 SO(3) iterations and EVERY Gauss-Newton iteration of
// every pyramid level (4 + 5 + 10 at the defaults) — the 1 + 10 + 57 dependent launches of the launch-per-step script — by FT_WGS = 256
// co-resident workgroups of 512 threads, one per CU.
//
//   * Work: workgroup b owns group g(b) of the level (fast_group_of: contiguous image rows per XCD) = the four tasks 4 g .. 4 g + 3 of
//     the fast order: wavefronts 0-3 run them for the ICP term, wavefronts 4-7 for the photometric term; the correspondence search runs
//     over exactly the group's pixels, so the packed correspondences never cross a workgroup.  Levels with fewer than 256 groups leave
//     workgroups without pixels; they still follow the state.
//   * State: every workgroup keeps its own copy of the Gauss-Newton state in LDS and evaluates every update step redundantly (the same
//     wave-parallel solve on the same bits, ef_solve_dev.hpp), so nothing is broadcast; workgroup 0 also leaves the global side.
//   * Exchange: what the reference reduces globally crosses workgroups as tagged 8-byte granules {value, epoch}, one write-through
//     (agent-scope) store each, polled with agent-scope loads — no counter, no fence, no barrier:
//       A  the search's {count, sum diff^2} (sigma, quirk Q2): every workgroup publishes one 16-byte record; the first photometric
//          wavefront of every workgroup sweeps the <= 256 records (its loads and gathers already in flight) and relays through LDS;
//       B  the group partials of the normal equations, in two hops: workgroup a < 58 is the REDUCER of accumulator a — one wavefront
//          sweeps the <= 256 granules G1[a][*] (2 KB), finishes the tree (fast_tree's order) and publishes the total G2[a]; every
//          workgroup polls the 58 totals (464 bytes instead of the 29.7 KB all-gather of round 3).
//     An epoch is used once (the host hands every launch a fresh range), each hop is an all-to-all dependency, so a slot is never
//     rewritten before every reader of its previous value has moved on; a reader waits for `tag == epoch` exactly.
//   * Every spin is bounded; a time-out (the grid was not co-resident) raises FtSync::abort and the launch runs to its end without
//     waiting any more: see tracker_aborted.
//   * Results are bit-identical to the launch-per-step script of the same build (same tasks, same trees).
// ------------------------------------------------------------------------------------------
// Column of a workgroup in an exchange: its group, or — without one at this level — one of the columns behind the NG groups (the NG
// workgroups that own a group and the FT_WGS - NG that do not are both numbered in workgroup order, so the map is a bijection).
// EVERY workgroup publishes into every exchange (zeros when it has no pixels: a running sum that starts at +0 is never -0, so adding
// +0 leaves every bit alone) and every sweep covers all FT_WGS columns: that makes each hop an all-to-all dependency, which is what
// guarantees that no slot is rewritten while a slow workgroup still waits for its previous value.
__device__ __forceinline__ int ft_column(int wg, int g, int NG) {
  if (g >= 0) return g;
  const int per = fast_groups_per_xcd(NG);
  // rank of wg among the workgroups without a group: those with (wg >> 3) >= per, or inside the ragged tail of their XCD's range
  int rank = 0;
  for (int x = 0; x < 8; ++x) {
    const int owned = min(per, max(0, NG - x * per));          // groups XCD-slot x owns: its first `owned` workgroups have one
    const int mine = (FT_WGS >> 3) - owned;                     // ... and this many do not
    if (x < (wg & 7)) rank += mine;
    else if (x == (wg & 7)) rank += (wg >> 3) - owned;
  }
  return NG + rank;
}
// the reducer's part of exchange B (one converged wavefront of workgroup a < na): sweep G1[a][*], finish the tree, publish the total
__device__ __forceinline__ void ft_reduce_publish(const unsigned long long* G1, unsigned long long* G2, int a, unsigned epoch,
                                                  volatile int* dead_s, FtSync* Y, float* plain_out) {
  unsigned d[4];
  ft_sweep(G1 + (size_t)a * 256, 1, FT_WGS, epoch, dead_s, Y, d);
  const float x = lane_tree64((__uint_as_float(d[0]) + __uint_as_float(d[1])) + (__uint_as_float(d[2]) + __uint_as_float(d[3])));
  if ((threadIdx.x & 63) == 0) {
    ft_put(G2 + a, __float_as_uint(x), epoch);
    if (plain_out) plain_out[(size_t)a * 256] = x;   // the launch's last iteration: what k_track_end's head reads (ng = 1)
  }
}

template <bool HAS_ICP, bool HAS_RGB>
__global__ void __launch_bounds__(FT_BLOCK) k_track_fast(const FtArgs A, TrackState* st) {
  constexpr int NT = (HAS_ICP && HAS_RGB) ? 2 : 1;
  constexpr int NA = NT * SE3_ACCS;
  __shared__ GNState gs[2];
  __shared__ efs::SolveScratch S;
  __shared__ float sums_s[2 * SE3_ACCS];
  __shared__ float bg[24];   // Rprev[9] | tprev[3] | Rprev_inv[9]: constants of the call (k_track_begin)
  __shared__ float wsum[2 * 4 * SE3_ACCS];
  __shared__ float red[SO3_ACCS];
  __shared__ So3Loop Z;
  __shared__ int ired[2 * FT_BLOCK / 64];
  __shared__ int tot_s[2];           // {count, sum diff^2} of the iteration's search over the whole image
  __shared__ unsigned seen_a[2];     // exchange A relay: {epoch the workgroup's sweeping wavefront has completed, wait abandoned}
  __shared__ int dead_s;
  __shared__ unsigned mode_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wg = blockIdx.x;
  unsigned long long* G1 = (unsigned long long*)(A.partials + FT_G1_OFF);
  unsigned long long* G2 = (unsigned long long*)(A.partials + FT_G2_OFF);
  unsigned long long* GA = (unsigned long long*)(A.partials + FT_GA_OFF);
  FtSync* Y = (FtSync*)(A.partials + FT_SY_OFF);
#ifdef EF_STAGE_CLOCKS
  unsigned long long clk_last = wall_clock64();
  const unsigned long long clk_start = clk_last;
#endif
  // ---- admission (beside k_track_begin below, on other wavefronts): the exchanges need all FT_WGS workgroups resident TOGETHER.  Every
  // workgroup reports in; workgroup 0 — dispatched first, so resident whenever any other is — waits a bounded time for the whole grid
  // and publishes the verdict every workgroup waits for.  PERSISTENT: everybody is here and stays until the end, no later wait can
  // starve.  SERIAL (other work holds some of the chip's CUs: another process, a long kernel of another stream): every workgroup
  // leaves at once — also those dispatched later, which find the verdict waiting — without having touched the state, and the
  // one-workgroup launch enqueued behind every persistent launch (k_track_serial: returns at once otherwise) finds the verdict and runs the
  // whole call itself, group by group, in the same order of additions (ft_serial_call): ~50x slower, the same bits, no host in the loop.
  // ---- the model side is known to be empty (local loop closure without an inactive surface in view: the common frame): nineteen iterations
  // without a single correspondence leave the state k_track_begin set up, zero sums and zero counts — written here by workgroup 0, at once
  if (A.empty_model_flag && *A.empty_model_flag != A.empty_model_value) {   // uniform: every workgroup reads the same word
    if (wg != 0 || t != 0) return;
    double R[9];
    efl::quat_to_mat<double>(st->q, R);
    GNState& o = st->gn[A.out_cur];
    float Rp[9], Rpi[9];
    for (int i = 0; i < 9; ++i) Rp[i] = o.Rcurr[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) o.tcurr[i] = (float)st->t[i];
    efl::m3_inverse<float>(Rp, Rpi);
    efl::m4_identity(o.resultRt);
    o.rgb_broken = 0;
    o.lastRGBErrorLevel = 0.f;
    compute_krk(o.resultRt, A.L[0].k, o.krkinv, o.kt);
    for (int i = 0; i < 9; ++i) { st->Rprev[i] = Rp[i]; st->Rprev_inv[i] = Rpi[i]; }
    for (int i = 0; i < 3; ++i) st->tprev[i] = o.tcurr[i];
    for (int i = 0; i < 4; ++i) st->q_prev[i] = st->q[i];
    for (int i = 0; i < 3; ++i) st->t_prev[i] = st->t[i];
    for (int i = 0; i < RGB_SLOTS; ++i) st->rgb_slots[0][i][0] = st->rgb_slots[0][i][1] = st->rgb_slots[1][i][0] = st->rgb_slots[1][i][1] = 0;
    st->call_seq += 1u;
    st->so3_iterations = 0;
    st->so3_ticket = 0;
    st->so3_done = 1;
    st->dense_count = 0;
    float* P = A.partials + FT_P_OFF;
    for (int a = 0; a < NA; ++a) P[(size_t)a * 256] = 0.f;   // the totals k_track_end's head reads (ng = 1)
    return;
  }
  if (t == 64) ft_put(&Y->arrive[wg], 1u, A.epoch);
  if (wg == 0 && wave == 7) {
    bool ok[4] = {false, false, false, false};
    bool all = false;
    for (int spin = 0; spin < FT_ADMIT_SPIN && !all; ++spin) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (!ok[i]) ok[i] = (unsigned)(ft_get(&Y->arrive[4 * lane + i]) >> 32) == A.epoch;
      all = __all(ok[0] && ok[1] && ok[2] && ok[3]);
      if (!all && spin > 8) __builtin_amdgcn_s_sleep(2);
    }
    if (!all) {   // (uniform) what the serial run needs to know about this call: the kernel-argument segment, copied AS MEMORY by the wavefront's lanes
      // (`Y->args = A` made the compiler keep a copy of the by-value argument in scratch for the whole launch: 256 bytes per lane, rounds 4-5)
      static_assert(sizeof(FtArgs) % 4 == 0, "copied dword by dword");
      typedef const __attribute__((address_space(4))) unsigned* KWords;
      const KWords src = (KWords)__builtin_amdgcn_kernarg_segment_ptr();   // FtArgs is the kernel's FIRST argument
      unsigned* dst = (unsigned*)&Y->args;
      for (int i = lane; i < (int)(sizeof(FtArgs) / 4); i += 64) dst[i] = src[i];
    }
    if (lane == 0) {
      if (!all) {
        __hip_atomic_fetch_add(&Y->fallbacks, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        drain_stores();
      }
      ft_put(&Y->mode, all ? FT_MODE_PERSISTENT : FT_MODE_SERIAL, A.epoch);
    }
  }
  if (t == 128) {
    unsigned m = 0u;
    for (int spin = 0; spin < FT_SPIN; ++spin) {
      const unsigned long long g = ft_get(&Y->mode);
      if ((unsigned)(g >> 32) == A.epoch) { m = (unsigned)g; break; }
      if (spin > 8) __builtin_amdgcn_s_sleep(1);
    }
    mode_s = m;   // 0: no verdict within seconds (workgroup 0 never ran?): treated like a time-out below
  }
  // ---- k_track_begin, by every workgroup for itself; workgroup 0 also leaves the global side of it ----
  if (t == 0) {
    dead_s = (int)__hip_atomic_load(&Y->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    seen_a[0] = 0u;
    seen_a[1] = 0u;
    tot_s[0] = tot_s[1] = 0;
    double R[9];
    efl::quat_to_mat<double>(st->q, R);
    GNState& g = gs[0];
    for (int i = 0; i < 9; ++i) bg[i] = g.Rcurr[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) bg[9 + i] = g.tcurr[i] = (float)st->t[i];
    efl::m3_inverse<float>(bg, bg + 12);
    efl::m4_identity(g.resultRt);
    g.rgb_broken = 0;
    g.lastRGBErrorLevel = 3.402823466e+38f;
    if (!A.so3) compute_krk(g.resultRt, A.kfirst, g.krkinv, g.kt);
    if (wg == 0) {
      for (int i = 0; i < 9; ++i) { st->Rprev[i] = bg[i]; st->Rprev_inv[i] = bg[12 + i]; }
      for (int i = 0; i < 3; ++i) st->tprev[i] = bg[9 + i];
      for (int i = 0; i < 4; ++i) st->q_prev[i] = st->q[i];
      for (int i = 0; i < 3; ++i) st->t_prev[i] = st->t[i];
      for (int i = 0; i < RGB_SLOTS; ++i) st->rgb_slots[0][i][0] = st->rgb_slots[0][i][1] = st->rgb_slots[1][i][0] = st->rgb_slots[1][i][1] = 0;
      st->call_seq += 1u;
      st->so3_iterations = 0;
      st->so3_ticket = 0;
      st->so3_done = 1;
      st->dense_count = 0;
    }
  }
  __syncthreads();
  FT_CLK(0);   // begin + admission
  if (dead_s) return;   // an earlier launch of this tracker instance timed out
  if (mode_s == 0u) {   // (bounded like every spin; with the verdict missing nothing can be trusted)
    if (t == 0) __hip_atomic_store(&Y->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (mode_s == FT_MODE_SERIAL) return;   // k_track_serial, the launch behind this one, runs the call on its one workgroup
  unsigned epoch = A.epoch;
  int cur = 0;
  // ---- SO(3) pre-alignment, RGBDOdometry.cpp:284-369 ----
  if (A.so3) {
    if (t == 0) {
      efl::m3_identity(Z.resR);
      efl::m3_identity(Z.lastResR);
      for (int i = 0; i < 9; ++i) Z.R_lr[i] = (i % 4 == 0) ? 1.f : 0.f;
      Z.lastError = 3.402823466e+38f / 2;
      Z.lastCount = 3.402823466e+38f / 2;
      Z.done = 0;
      so3_matrices(Z.resR, A.kso3, Z.mats);
    }
    __syncthreads();
    const int N = A.so3_cols * A.so3_rows;
    const FastPlan fp = fast_plan(N);
    const int g = fast_group_of(wg, fp.NG);
    const int col = ft_column(wg, g, fp.NG);
    for (int it = 0; it < 10; ++it, ++epoch) {
      {
        const m33 IB = m33_load(Z.mats), KI = m33_load(Z.mats + 9), KR = m33_load(Z.mats + 18);
        float acc[SO3_ACCS];
#pragma unroll
        for (int i = 0; i < SO3_ACCS; ++i) acc[i] = 0.f;
        if (g >= 0 && wave < 4) {
          fast_task_so3(A.so3_last, A.so3_next, A.so3_cols, A.so3_rows, IB, KI, KR, 4 * g + wave, fp.U, N, acc);
          lane_trees_store<SO3_ACCS>(acc, wsum + wave * SO3_ACCS);
        }
      }
      __syncthreads();
      if (t < SO3_ACCS) {   // (a workgroup without a group publishes zeros into its own column: see "Exchange" above)
        const float z = g >= 0 ? (wsum[t] + wsum[SO3_ACCS + t]) + (wsum[2 * SO3_ACCS + t] + wsum[3 * SO3_ACCS + t]) : 0.f;
        ft_put(G1 + (size_t)t * 256 + col, __float_as_uint(z), epoch);
      }
      FT_CLK(1);   // SO(3): rows, chains, publish
      if (wave == 1 && wg < SO3_ACCS) ft_reduce_publish(G1, G2, wg, epoch, &dead_s, Y, nullptr);
      if (wave == 0) {
        float v;
        ft_poll_totals(G2, SO3_ACCS, epoch, &dead_s, Y, v);
        if (lane < SO3_ACCS) red[lane] = v;
      }
      __syncthreads();
      FT_CLK(2);   // SO(3): exchange
      if (t == 0) Z.done = so3_update(Z, red, it, A.kso3, A.kfirst, gs[0]) ? 1 : 0;
      __syncthreads();
      FT_CLK(4);   // SO(3): update
      FT_COUNT(20);
      if (Z.done) { ++epoch; break; }   // every workgroup computes the same bits, so every workgroup leaves in the same iteration
    }
    if (wg == 0 && t == 0) {
      st->lastSO3Error = Z.err;
      st->lastSO3Count = Z.cnt;
      st->so3_iterations = Z.iterations;
    }
  }
  // ---- the Gauss-Newton iterations, RGBDOdometry.cpp:371-553 ----
  for (int it = 0; it < A.n_iter; ++it) {
    const int lvl = ft_level_of(A.levels, it);
#ifdef EF_STAGE_CLOCKS
    const unsigned long long clk_iter = wall_clock64();
#endif
    const PtLevel Lv = ft_load_level((FtArgsK)__builtin_amdgcn_kernarg_segment_ptr(), lvl);   // FtArgs is the kernel's FIRST argument
    const int cols = Lv.cols, rows = Lv.rows, N = cols * rows;
    const FastPlan fp = fast_plan(N);
    const int g = fast_group_of(wg, fp.NG);
    const int col = ft_column(wg, g, fp.NG);
    const bool last = it == A.n_iter - 1;
    if (it > 0) {
      // head: the update step of iteration it - 1 (k_track_step's head), by every workgroup on its own state; the sums are in sums_s
      // (hop 2 of the previous iteration's exchange B), the search's totals in tot_s
      StepArgs H{true, false, HAS_ICP, HAS_RGB, false, A.icpWeight, Lv.k, lvl != ft_level_of(A.levels, it - 1), it};
      if (t < 64) {
        efs::SolvePrefetch PF{};
        const GNState& gp = gs[cur];
        PF.rt = gp.resultRt[lane & 15];
        PF.pose = bg[lane < 12 ? lane : 0];
        PF.slot_a = (HAS_RGB && lane == 0) ? tot_s[0] : 0;
        PF.slot_b = (HAS_RGB && lane == 0) ? tot_s[1] : 0;
        PF.lastRGBErrorLevel = gp.lastRGBErrorLevel;
        PF.broken = gp.rgb_broken;
        solve_step_wave(st, &gs[cur], &gs[cur ^ 1], true, sums_s, H, S, PF, wg == 0);
      }
      __syncthreads();
      FT_CLK(6);   // SE(3) head: solve
#ifdef EF_STAGE_CLOCKS
      if (wg == 0 && t == 0) {   // phases of that solve (EF_STAMP 3..8, same thread)
        const unsigned long long* c = st->dbg_clock;
        Y->clk[3] += c[4] - c[3]; Y->clk[5] += c[5] - c[4]; Y->clk[18] += c[6] - c[5]; Y->clk[19] += c[7] - c[6]; Y->clk[23] += c[8] - c[7];
      }
#endif
      cur ^= 1;
    }
    const GNState& G = gs[cur];
    const unsigned epoch_a = epoch;
    if (HAS_RGB) {
      // correspondence search (k_track_step's body) over exactly the pixels of this workgroup's group, three visits in flight per thread
      int cnt = 0, sq = 0;
      if (g >= 0) {
        const m33 Km = m33_load(G.krkinv);
        const f3 kt{G.kt[0], G.kt[1], G.kt[2]};
        const int npx = 256 * fp.U, pbase = npx * g;
        // the search sits on the iteration's critical path (search -> exchange A -> photometric rows): where a thread has more than one
        // pixel (level 0: 2.5) its visits' loads and gathers are in flight together; one rolled visit otherwise
        if (npx > FT_BLOCK) {
#pragma unroll 1
          for (int e0 = t; e0 < npx; e0 += 3 * FT_BLOCK) {
            int qs[3], nis[3], gi[3], u0s[3], v0s[3], lis[3];
            uint8_t m[3];
            float d1s[3], td1[3], d0s[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
              const int q = pbase + e0 + e * FT_BLOCK;
              const bool in = e0 + e * FT_BLOCK < npx && q < N;
              const int qq = in ? q : N - 1;
              qs[e] = q;
              m[e] = in ? Lv.mask[qq] : (uint8_t)0;
              d1s[e] = Lv.nextDepth[qq];
              nis[e] = Lv.nextImage[qq];
            }
#pragma unroll
            for (int e = 0; e < 3; ++e) {
              const int q = qs[e];
              const int y = q / cols, x = q - y * cols;
              const float d1 = d1s[e];
              td1[e] = (float)(d1 * (Km.r[2].x * x + Km.r[2].y * y + Km.r[2].z) + kt.z);
              u0s[e] = f2i_rn((d1 * (Km.r[0].x * x + Km.r[0].y * y + Km.r[0].z) + kt.x) / td1[e]);
              v0s[e] = f2i_rn((d1 * (Km.r[1].x * x + Km.r[1].y * y + Km.r[1].z) + kt.y) / td1[e]);
              gi[e] = (m[e] && u0s[e] >= 0 && v0s[e] >= 0 && u0s[e] < cols && v0s[e] < rows) ? v0s[e] * cols + u0s[e] : -1;
              d0s[e] = 0.f;
              lis[e] = 0;
              if (gi[e] >= 0) { d0s[e] = Lv.lastDepth[gi[e]]; lis[e] = Lv.lastImage[gi[e]]; }
            }
#pragma unroll
            for (int e = 0; e < 3; ++e) {
              if (!m[e]) continue;
              uint32_t packed = 0u;
              if (gi[e] >= 0 && d0s[e] > 0 && fabsf(td1[e] - d0s[e]) <= 0.07f /* maxDepthDeltaRGB, RGBDOdometry.cpp:41 */ && lis[e] != 0) {
                const int idiff = nis[e] - lis[e];
                packed = pack_corres(u0s[e], v0s[e], idiff);
                cnt += 1;
                sq += idiff * idiff;
              }
              Lv.corres[qs[e]] = packed;
            }
          }
        } else {
          const int q = pbase + t;
          const bool in = t < npx && q < N;
          const int qq = in ? q : N - 1;
          const uint8_t mk = Lv.mask[qq];          // the three pixel-addressed loads together: one round trip, not two
          const float d1 = Lv.nextDepth[qq];
          const int ni = Lv.nextImage[qq];
          if (in && mk) {
            const int y = q / cols, x = q - y * cols;
            const float td = (float)(d1 * (Km.r[2].x * x + Km.r[2].y * y + Km.r[2].z) + kt.z);
            const int u0 = f2i_rn((d1 * (Km.r[0].x * x + Km.r[0].y * y + Km.r[0].z) + kt.x) / td);
            const int v0 = f2i_rn((d1 * (Km.r[1].x * x + Km.r[1].y * y + Km.r[1].z) + kt.y) / td);
            uint32_t packed = 0u;
            if (u0 >= 0 && v0 >= 0 && u0 < cols && v0 < rows) {
              const int gi1 = v0 * cols + u0;
              const float d0 = Lv.lastDepth[gi1];
              const int li = Lv.lastImage[gi1];
              if (d0 > 0 && fabsf(td - d0) <= 0.07f /* maxDepthDeltaRGB, RGBDOdometry.cpp:41 */ && li != 0) {
                const int idiff = ni - li;
                packed = pack_corres(u0, v0, idiff);
                cnt += 1;
                sq += idiff * idiff;
              }
            }
            Lv.corres[q] = packed;
          }
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_down(cnt, off, 64);
        sq += __shfl_down(sq, off, 64);
      }
      if (lane == 0) { ired[wave * 2] = cnt; ired[wave * 2 + 1] = sq; }
      __syncthreads();   // also: the workgroup's packed correspondences are visible to its photometric wavefronts
      if (t == 0) {   // (zeros from a workgroup without a group)
        int sa = 0, sb = 0;
        for (int w = 0; w < FT_BLOCK / 64; ++w) { sa += ired[w * 2]; sb += ired[w * 2 + 1]; }
        ft_put(GA + 2 * col, (unsigned)sa, epoch_a);
        ft_put(GA + 2 * col + 1, (unsigned)sb, epoch_a);
      }
      ++epoch;
      FT_CLK(7);   // SE(3): correspondence search + publish A
    }
    const unsigned epoch_b = epoch++;
    // normal equations of the workgroup's group: wavefront (term, w4) runs task 4 g + w4 of its term
    const int tix = wave >> 2, w4 = wave & 3;
    const bool active = wave < 4 * NT;
    const bool rgb_wave = HAS_RGB && (!HAS_ICP || tix == 1);
    float acc[SE3_ACCS];
#pragma unroll
    for (int i = 0; i < SE3_ACCS; ++i) acc[i] = 0.f;
    const IcpView IV{Lv.vmap_curr, Lv.nmap_curr, Lv.vmap_g_prev, Lv.nmap_g_prev, cols, rows, Lv.k, A.distThres, A.angleThres, A.dist2Max, A.sine2Max};
    const RgbView RV{Lv.corres, Lv.lastDepth, nullptr, Lv.dIdx, Lv.dIdy, cols, rows, Lv.k, 1.0f / 8.0f};
    if (active && HAS_ICP && !rgb_wave && g >= 0) {
      IcpPose P;
      P.Rcurr = m33_load(G.Rcurr);
      P.tcurr = {G.tcurr[0], G.tcurr[1], G.tcurr[2]};
      P.Rprev_inv = m33_load(bg + 12);
      P.tprev = {bg[9], bg[10], bg[11]};
      fast_task_se3<true, true>(IV, RV, P, 0.f, 4 * g + w4, fp.U, N, acc);
      FT_CLK(8);   // SE(3): ICP task (wavefront 0)
    }
    if (active && HAS_RGB && rgb_wave) {
      // everything of the photometric task that does not need sigma, with its loads and gathers, before the wait (ef_track_fast.inc)
      RgbPre pre[RGB_SPLIT_MAX];
      const bool split = fp.U <= RGB_SPLIT_MAX;
      if (split && g >= 0) rgb_prepare(IV, RV, 4 * g + w4, fp.U, N, pre);
      // exchange A: the first photometric wavefront sweeps the records, the others watch its relay in LDS
      const bool leader = w4 == 0;
      if (leader) {
        int sa, sb;
        const bool ok = ft_sweep_pairs(GA, epoch_a, &dead_s, Y, sa, sb);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          sa += __shfl_down(sa, off, 64);
          sb += __shfl_down(sb, off, 64);
        }
        if (lane == 0) {
          tot_s[0] = sa;
          tot_s[1] = sb;
          __hip_atomic_store(&seen_a[1], ok ? 0u : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_store(&seen_a[0], epoch_a, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      } else if (lane == 0) {
        int spins = 0;
        while (__hip_atomic_load(&seen_a[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != epoch_a && ++spins < 64 * FT_SPIN) __builtin_amdgcn_s_sleep(1);
      }
      efs::wave_sync();
      const int rgbSize = __shfl(lane == 0 ? __hip_atomic_load(&tot_s[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0, 0, 64);
      const int sqsum = __shfl(lane == 0 ? __hip_atomic_load(&tot_s[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0, 0, 64);
      const float sigma = sigma_from_sums(sqsum, rgbSize, false);
      if (g >= 0) {
        if (split) {
          rgb_finish(RV, sigma, fp.U, pre, acc);
        } else {
          IcpPose P{};
          fast_task_se3<false, true>(IV, RV, P, sigma, 4 * g + w4, fp.U, N, acc);
        }
      }
    }
    if (active && g >= 0) lane_trees_store<SE3_ACCS>(acc, wsum + (tix * 4 + w4) * SE3_ACCS);
    __syncthreads();
    if (t < NA) {   // (zeros from a workgroup without a group)
      const int term = t / SE3_ACCS, a = t - term * SE3_ACCS;
      const float* w = wsum + (size_t)term * 4 * SE3_ACCS + a;
      const float v = g >= 0 ? (w[0] + w[SE3_ACCS]) + (w[2 * SE3_ACCS] + w[3 * SE3_ACCS]) : 0.f;
      ft_put(G1 + (size_t)t * 256 + col, __float_as_uint(v), epoch_b);
    }
    FT_CLK(9);   // SE(3): tasks, trees, publish B
    // exchange B: reducers finish the tree of their accumulator; everybody (the launch's last iteration: nobody — k_track_end reads the
    // plain totals the reducers leave) takes the 58 totals
    if (wave == 1 && wg < NA) ft_reduce_publish(G1, G2, wg, epoch_b, &dead_s, Y, last ? A.partials + FT_P_OFF : nullptr);
    if (!last && wave == 0) {
      float v;
      ft_poll_totals(G2, NA, epoch_b, &dead_s, Y, v);
      if (lane < NA) sums_s[(HAS_ICP ? 0 : SE3_ACCS) + lane] = v;
    }
    __syncthreads();
    FT_CLK(10);   // SE(3): exchange B
    FT_COUNT(21);
#ifdef EF_STAGE_CLOCKS
    if (wg == 0 && t == 0) { Y->clk[12 + lvl] += wall_clock64() - clk_iter; Y->clk[15 + lvl] += 1; }
#endif
  }
  // ---- what the launch that follows reads (k_track_end: the update of iteration n_iter - 1 at its head) ----
  if (wg == 0 && t == 0) {
    const GNState& g = gs[cur];
    GNState& o = st->gn[A.out_cur];
    for (int i = 0; i < 9; ++i) { o.Rcurr[i] = g.Rcurr[i]; o.krkinv[i] = g.krkinv[i]; }
    for (int i = 0; i < 3; ++i) { o.tcurr[i] = g.tcurr[i]; o.kt[i] = g.kt[i]; }
    for (int i = 0; i < 16; ++i) o.resultRt[i] = g.resultRt[i];
    o.lastRGBErrorLevel = g.lastRGBErrorLevel;
    o.rgb_broken = g.rgb_broken;
    if (HAS_RGB && A.n_iter > 0) {   // the last search's totals, where the next update step's head looks for them
      const int set = (A.n_iter - 1) & 1;
      st->rgb_slots[set][0][0] = tot_s[0];
      st->rgb_slots[set][0][1] = tot_s[1];
    }
#ifdef EF_STAGE_CLOCKS
    Y->clk[11] += wall_clock64() - clk_start;   // whole launch
    Y->clk[22] += 1;
#endif
  }
}

// ------------------------------------------------------------------------------------------
// The call on ONE workgroup: what k_track_end_fast runs first when the persistent launch in front of it left the verdict SERIAL (its grid
// could not become resident: see the admission step of k_track_fast).  The same tasks, the same group partials, the same trees — group by
// group instead of all at once, the group partials in the plain array P[acc][group] the per-step kernels use, the 256-leaf tree by
// fast_tree, the update steps by the same solve — so the results are the persistent launch's, bit for bit (tests/test_gpu_fallback.py).
// ------------------------------------------------------------------------------------------
struct FtSerialLds {
  GNState gs[2];
  float bg[24];
  float wsum[2 * 4 * SE3_ACCS];
  float red[SO3_ACCS];
  So3Loop Z;
  int ired[2 * REDUCE_BLOCK / 64];
  int tot_s[2];
};
template <bool HAS_ICP, bool HAS_RGB>
__device__ __forceinline__ void ft_serial_call(const FtArgs* Ag, TrackState* st, FtSerialLds& M, efs::SolveScratch& S, float* sums_s) {
  constexpr int NT = (HAS_ICP && HAS_RGB) ? 2 : 1;
  constexpr int NA = NT * SE3_ACCS;
  constexpr int BLOCK = REDUCE_BLOCK;   // k_track_end's block: four wavefronts
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const FtArgs& A = *Ag;
  float* P = A.partials + FT_P_OFF;
  So3Loop& Z = M.Z;
  // ---- k_track_begin ----
  if (t == 0) {
    double R[9];
    efl::quat_to_mat<double>(st->q, R);
    GNState& g = M.gs[0];
    for (int i = 0; i < 9; ++i) M.bg[i] = g.Rcurr[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) M.bg[9 + i] = g.tcurr[i] = (float)st->t[i];
    efl::m3_inverse<float>(M.bg, M.bg + 12);
    efl::m4_identity(g.resultRt);
    g.rgb_broken = 0;
    g.lastRGBErrorLevel = 3.402823466e+38f;
    if (!A.so3) compute_krk(g.resultRt, A.kfirst, g.krkinv, g.kt);
    for (int i = 0; i < 9; ++i) { st->Rprev[i] = M.bg[i]; st->Rprev_inv[i] = M.bg[12 + i]; }
    for (int i = 0; i < 3; ++i) st->tprev[i] = M.bg[9 + i];
    for (int i = 0; i < 4; ++i) st->q_prev[i] = st->q[i];
    for (int i = 0; i < 3; ++i) st->t_prev[i] = st->t[i];
    for (int i = 0; i < RGB_SLOTS; ++i) st->rgb_slots[0][i][0] = st->rgb_slots[0][i][1] = st->rgb_slots[1][i][0] = st->rgb_slots[1][i][1] = 0;
    st->call_seq += 1u;
    st->so3_iterations = 0;
    st->so3_ticket = 0;
    st->so3_done = 1;
    st->dense_count = 0;
    M.tot_s[0] = M.tot_s[1] = 0;
  }
  __syncthreads();
  // ---- SO(3) ----
  if (A.so3) {
    if (t == 0) {
      efl::m3_identity(Z.resR);
      efl::m3_identity(Z.lastResR);
      for (int i = 0; i < 9; ++i) Z.R_lr[i] = (i % 4 == 0) ? 1.f : 0.f;
      Z.lastError = 3.402823466e+38f / 2;
      Z.lastCount = 3.402823466e+38f / 2;
      Z.done = 0;
      so3_matrices(Z.resR, A.kso3, Z.mats);
    }
    __syncthreads();
    const int N = A.so3_cols * A.so3_rows;
    const FastPlan fp = fast_plan(N);
    for (int it = 0; it < 10; ++it) {
      const m33 IB = m33_load(Z.mats), KI = m33_load(Z.mats + 9), KR = m33_load(Z.mats + 18);
#pragma unroll 1
      for (int g = 0; g < fp.NG; ++g) {
        float acc[SO3_ACCS];
#pragma unroll
        for (int i = 0; i < SO3_ACCS; ++i) acc[i] = 0.f;
        fast_task_so3(A.so3_last, A.so3_next, A.so3_cols, A.so3_rows, IB, KI, KR, 4 * g + wave, fp.U, N, acc);
        lane_trees_store<SO3_ACCS>(acc, M.wsum + wave * SO3_ACCS);
        __syncthreads();
        if (t < SO3_ACCS) P[(size_t)t * 256 + g] = (M.wsum[t] + M.wsum[SO3_ACCS + t]) + (M.wsum[2 * SO3_ACCS + t] + M.wsum[3 * SO3_ACCS + t]);
        __syncthreads();
      }
      fast_tree<BLOCK, false>(P, fp.NG, SO3_ACCS, M.red);
      __syncthreads();
      if (t == 0) Z.done = so3_update(Z, M.red, it, A.kso3, A.kfirst, M.gs[0]) ? 1 : 0;
      __syncthreads();
      if (Z.done) break;
    }
    if (t == 0) {
      st->lastSO3Error = Z.err;
      st->lastSO3Count = Z.cnt;
      st->so3_iterations = Z.iterations;
    }
  }
  // ---- the Gauss-Newton iterations ----
  int cur = 0;
  for (int it = 0; it < A.n_iter; ++it) {
    const int lvl = ft_level_of(A.levels, it);
    const PtLevel Lv = A.L[lvl];
    const int cols = Lv.cols, rows = Lv.rows, N = cols * rows;
    const FastPlan fp = fast_plan(N);
    if (it > 0) {
      StepArgs H{true, false, HAS_ICP, HAS_RGB, false, A.icpWeight, Lv.k, lvl != ft_level_of(A.levels, it - 1), it};
      if (t < 64) {
        efs::SolvePrefetch PF{};
        const GNState& gp = M.gs[cur];
        PF.rt = gp.resultRt[lane & 15];
        PF.pose = M.bg[lane < 12 ? lane : 0];
        PF.slot_a = (HAS_RGB && lane == 0) ? M.tot_s[0] : 0;
        PF.slot_b = (HAS_RGB && lane == 0) ? M.tot_s[1] : 0;
        PF.lastRGBErrorLevel = gp.lastRGBErrorLevel;
        PF.broken = gp.rgb_broken;
        solve_step_wave(st, &M.gs[cur], &M.gs[cur ^ 1], true, sums_s, H, S, PF, true);
      }
      __syncthreads();
      cur ^= 1;
    }
    const GNState& G = M.gs[cur];
    float sigma = 0.f;
    if (HAS_RGB) {
      const m33 Km = m33_load(G.krkinv);
      const f3 kt{G.kt[0], G.kt[1], G.kt[2]};
      int cnt = 0, sq = 0;
#pragma unroll 1
      for (int q = t; q < N; q += BLOCK) {
        if (!Lv.mask[q]) continue;
        const float d1 = Lv.nextDepth[q];
        const int ni = Lv.nextImage[q];
        const int y = q / cols, x = q - y * cols;
        const float td = (float)(d1 * (Km.r[2].x * x + Km.r[2].y * y + Km.r[2].z) + kt.z);
        const int u0 = f2i_rn((d1 * (Km.r[0].x * x + Km.r[0].y * y + Km.r[0].z) + kt.x) / td);
        const int v0 = f2i_rn((d1 * (Km.r[1].x * x + Km.r[1].y * y + Km.r[1].z) + kt.y) / td);
        uint32_t packed = 0u;
        if (u0 >= 0 && v0 >= 0 && u0 < cols && v0 < rows) {
          const int gi1 = v0 * cols + u0;
          const float d0 = Lv.lastDepth[gi1];
          const int li = Lv.lastImage[gi1];
          if (d0 > 0 && fabsf(td - d0) <= 0.07f /* maxDepthDeltaRGB, RGBDOdometry.cpp:41 */ && li != 0) {
            const int idiff = ni - li;
            packed = pack_corres(u0, v0, idiff);
            cnt += 1;
            sq += idiff * idiff;
          }
        }
        Lv.corres[q] = packed;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_down(cnt, off, 64);
        sq += __shfl_down(sq, off, 64);
      }
      if (lane == 0) { M.ired[wave * 2] = cnt; M.ired[wave * 2 + 1] = sq; }
      __syncthreads();
      if (t == 0) {
        int sa = 0, sb = 0;
        for (int w = 0; w < BLOCK / 64; ++w) { sa += M.ired[w * 2]; sb += M.ired[w * 2 + 1]; }
        M.tot_s[0] = sa;
        M.tot_s[1] = sb;
      }
      __syncthreads();
      sigma = sigma_from_sums(M.tot_s[1], M.tot_s[0], false);
    }
    const IcpView IV{Lv.vmap_curr, Lv.nmap_curr, Lv.vmap_g_prev, Lv.nmap_g_prev, cols, rows, Lv.k, A.distThres, A.angleThres, A.dist2Max, A.sine2Max};
    const RgbView RV{Lv.corres, Lv.lastDepth, nullptr, Lv.dIdx, Lv.dIdy, cols, rows, Lv.k, 1.0f / 8.0f};
    IcpPose P3{};
    if (HAS_ICP) {
      P3.Rcurr = m33_load(G.Rcurr);
      P3.tcurr = {G.tcurr[0], G.tcurr[1], G.tcurr[2]};
      P3.Rprev_inv = m33_load(M.bg + 12);
      P3.tprev = {M.bg[9], M.bg[10], M.bg[11]};
    }
#pragma unroll 1
    for (int g = 0; g < fp.NG; ++g) {   // four wavefronts = the four tasks of the group, one term after the other
      if (HAS_ICP) {
        float acc[SE3_ACCS];
#pragma unroll
        for (int i = 0; i < SE3_ACCS; ++i) acc[i] = 0.f;
        fast_task_se3<true, true>(IV, RV, P3, 0.f, 4 * g + wave, fp.U, N, acc);
        lane_trees_store<SE3_ACCS>(acc, M.wsum + wave * SE3_ACCS);
      }
      if (HAS_RGB) {
        float acc[SE3_ACCS];
#pragma unroll
        for (int i = 0; i < SE3_ACCS; ++i) acc[i] = 0.f;
        fast_task_se3<false, true>(IV, RV, P3, sigma, 4 * g + wave, fp.U, N, acc);
        lane_trees_store<SE3_ACCS>(acc, M.wsum + ((HAS_ICP ? 4 : 0) + wave) * SE3_ACCS);
      }
      __syncthreads();
      if (t < NA) {
        const int term = t / SE3_ACCS, a = t - term * SE3_ACCS;
        const float* w = M.wsum + (size_t)term * 4 * SE3_ACCS + a;
        P[(size_t)t * 256 + g] = (w[0] + w[SE3_ACCS]) + (w[2 * SE3_ACCS] + w[3 * SE3_ACCS]);
      }
      __syncthreads();
    }
    fast_tree<BLOCK, false>(P, fp.NG, NA, sums_s + (HAS_ICP ? 0 : SE3_ACCS));
    __syncthreads();
    if (it == A.n_iter - 1 && t < NA) P[(size_t)t * 256] = sums_s[(HAS_ICP ? 0 : SE3_ACCS) + t];   // what the head below reads (ng = 1)
    __syncthreads();
  }
  // ---- what the head of k_track_end reads ----
  if (t == 0) {
    const GNState& g = M.gs[cur];
    GNState& o = st->gn[A.out_cur];
    for (int i = 0; i < 9; ++i) { o.Rcurr[i] = g.Rcurr[i]; o.krkinv[i] = g.krkinv[i]; }
    for (int i = 0; i < 3; ++i) { o.tcurr[i] = g.tcurr[i]; o.kt[i] = g.kt[i]; }
    for (int i = 0; i < 16; ++i) o.resultRt[i] = g.resultRt[i];
    o.lastRGBErrorLevel = g.lastRGBErrorLevel;
    o.rgb_broken = g.rgb_broken;
    if (HAS_RGB && A.n_iter > 0) {
      const int set = (A.n_iter - 1) & 1;
      st->rgb_slots[set][0][0] = M.tot_s[0];
      st->rgb_slots[set][0][1] = M.tot_s[1];
    }
  }
  __threadfence_block();
  __syncthreads();
}

// The launch behind every persistent launch: one workgroup that leaves at once unless the verdict of the launch in front of it was SERIAL.
template <bool HAS_ICP, bool HAS_RGB>
__global__ void __launch_bounds__(REDUCE_BLOCK) k_track_serial(float* partials, TrackState* st, unsigned persistent_epoch) {
  __shared__ efs::SolveScratch S;
  __shared__ float sums_s[2 * SE3_ACCS];
  __shared__ FtSerialLds M;
  FtSync* Y = (FtSync*)(partials + FT_SY_OFF);
  const unsigned long long verdict = ft_get(&Y->mode);
  if ((unsigned)(verdict >> 32) != persistent_epoch || (unsigned)verdict != FT_MODE_SERIAL) return;   // uniform
  ft_serial_call<HAS_ICP, HAS_RGB>(&Y->args, st, M, S, sums_s);
}
