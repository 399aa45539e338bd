// Chip-wide exchanges of the persistent tracker launches (round 4; shared by both summation orders since round 5) — included by
// ef_track_kernels.hip behind PtLevel / So3Loop.  What the reference reduces globally crosses workgroups as tagged 8-byte granules
// {value, epoch}, one write-through (agent-scope) store each, polled with agent-scope loads — no counter, no fence, no barrier
// (MI355X_MICROARCH.md "granule"):
//   A  the search's {count, sum diff^2} (sigma, quirk Q2): every workgroup publishes one 16-byte record; one wavefront of every workgroup
//      sweeps the 256 records (its loads and gathers already in flight) and relays through LDS;
//   B  the partial sums of the normal equations, in two hops: workgroup a < 58 is the REDUCER of accumulator a — one wavefront sweeps the
//      256 granules G1[a][*] (2 KB), finishes the tree of its build's summation order and publishes the total G2[a]; every workgroup
//      polls the 58 totals (464 bytes).
// An epoch is used once (the host hands every launch a fresh range), EVERY workgroup publishes into every exchange and every sweep covers
// all 256 columns: each hop is an all-to-all dependency, so a slot is never rewritten before every reader of its previous value has
// moved on; a reader waits for `tag == epoch` exactly.  Every spin is bounded; a time-out raises FtSync::abort (tracker_aborted).
constexpr int FT_WGS = 256, FT_BLOCK = 512, FT_MAX_ITER = 24, FT_SPIN = 1 << 20;
constexpr int FT_P_OFF = 0;                                   // float P[58][256]: what a per-step kernel / k_track_end reads
constexpr int FT_G1_OFF = FT_P_OFF + 2 * SE3_ACCS * 256;      // u64 G1[58][256]
constexpr int FT_G2_OFF = FT_G1_OFF + 2 * 2 * SE3_ACCS * 256; // u64 G2[64]
constexpr int FT_GA_OFF = FT_G2_OFF + 128;                    // u64 GA[256][2]: {count, epoch}, {sum diff^2, epoch}
constexpr int FT_SY_OFF = FT_GA_OFF + 4 * 256;                // FtSync
// Round 6: the two areas EVERY workgroup polls — the 58 totals of exchange B's second hop and the 256 records of exchange A — exist FT_REPL
// times, 8 KB apart; a publisher stores every copy, workgroup w (XCD w % 8) polls copy w % FT_REPL.  A poll goes past the L2s: with one copy,
// 256 wavefronts hammer the same four (B) / thirty-two (A) lines, and the stores they wait for queue behind their requests (the counter-experiment,
// twice the polls: exchange B 3.45 -> 4.96 us, profiles/r08i_*).  (k_track_ref only.)
constexpr int FT_REPL = 64, FT_REPL_A = 2;                    // copies of the totals (B) / of the records (A)
constexpr int FT_REPL_STRIDE = 1024;                          // u64 words between two copies
constexpr int FT_MODE_WORD = 128;                             // word of every copy of the totals that carries the admission verdict (granule {FT_MODE_*, epoch})
constexpr int FT_G2R_OFF = 49152;                             // u64 G2R[FT_REPL <= 64][1024] (64 used per copy)
constexpr int FT_GAR_OFF = FT_G2R_OFF + 2 * 64 * FT_REPL_STRIDE;   // u64 GAR[FT_REPL_A <= 8][1024] (512 used per copy)
static_assert(FT_REPL >= 1 && FT_REPL <= 64 && (FT_REPL & (FT_REPL - 1)) == 0, "copies of the totals: a power of two, one store instruction of a wavefront");
static_assert(FT_REPL_A >= 1 && FT_REPL_A <= 8 && (FT_REPL_A & (FT_REPL_A - 1)) == 0, "copies of the records: a power of two up to the number of XCDs");
static_assert((FT_GAR_OFF + 2 * 8 * FT_REPL_STRIDE) <= PARTIAL_ALLOC_FLOATS, "the copies fit Pyramid::partials");
#ifdef EF_STAGE_CLOCKS
// (atomic adds WITHOUT a returned value: a plain `Y->clk[i] += ...` makes the stamping wavefront wait a global load's round trip — about a
// microsecond — at every stamp)
#define FT_CLK(i) do { if (wg == 0 && t == 0) { const unsigned long long now_ = wall_clock64(); (void)__hip_atomic_fetch_add(&Y->clk[i], now_ - clk_last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); clk_last = now_; } } while (0)
#define FT_COUNT(i) do { if (wg == 0 && t == 0) (void)__hip_atomic_fetch_add(&Y->clk[i], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while (0)
#define FT_ADD(i, v) (void)__hip_atomic_fetch_add(&Y->clk[i], (unsigned long long)(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
#define FT_CLK(i) do { } while (0)
#define FT_COUNT(i) do { } while (0)
#endif
struct FtArgs {
  PtLevel L[NUM_PYRS];
  int n_iter;
  unsigned long long levels;      // level of iteration i in bits 2 i, 2 i + 1
  bool so3;
  const uint8_t* so3_last; const uint8_t* so3_next;
  int so3_cols, so3_rows;
  Intr kso3, kfirst;
  float icpWeight, distThres, angleThres;
  float dist2Max, sine2Max;       // IcpView's gates on squared norms (sq_le_max / sq_lt_max of the two thresholds)
  float* partials;
  unsigned epoch;                 // first of the FT_EPOCHS epochs this launch may use (never 0: the areas are zero-filled at allocation)
  const unsigned* empty_model_flag;   // see TrackParams::empty_model_flag (null: never)
  unsigned empty_model_value;
  int out_cur;
  unsigned res_bytes;             // reference-order launch: dynamic LDS for level-resident pixel data (rt_res_mode; 0 = every level streams)
};
struct FtSync {
  unsigned abort, pad0[31];       // sticky: a wait timed out AFTER admission (cannot happen while the protocol is right: see tracker_aborted)
  unsigned long long clk[32];     // developer instrumentation (-DEF_STAGE_CLOCKS builds): 10 ns ticks per phase, summed over launches
  unsigned long long mode;        // admission verdict of the launch in flight: granule {FT_MODE_*, the launch's first epoch}
  unsigned fallbacks, pad1[29];   // launches that ran on workgroup 0 alone (tracker_fallbacks)
  unsigned long long arrive[FT_WGS];   // admission: granule {1, the launch's first epoch} per workgroup
  FtArgs args;                    // the arguments of the launch whose verdict was SERIAL (for k_track_serial)
};
constexpr unsigned FT_MODE_PERSISTENT = 1u, FT_MODE_SERIAL = 2u;
constexpr int FT_ADMIT_SPIN = 1 << 11;   // polls of ~1 us workgroup 0 gives the grid to become resident before it goes on alone
static_assert(FT_SY_OFF * sizeof(float) + sizeof(FtSync) <= (size_t)FT_G2R_OFF * sizeof(float), "the exchange areas end in front of the copies");
typedef const __attribute__((address_space(4))) FtArgs* FtArgsK;
__device__ __forceinline__ PtLevel ft_load_level(FtArgsK Ak, int lvl) {
  PtLevel L;
  L.vmap_curr = Ak->L[lvl].vmap_curr; L.nmap_curr = Ak->L[lvl].nmap_curr;
  L.vmap_g_prev = Ak->L[lvl].vmap_g_prev; L.nmap_g_prev = Ak->L[lvl].nmap_g_prev;
  L.mask = Ak->L[lvl].mask; L.lastDepth = Ak->L[lvl].lastDepth; L.nextDepth = Ak->L[lvl].nextDepth;
  L.lastImage = Ak->L[lvl].lastImage; L.nextImage = Ak->L[lvl].nextImage;
  L.corres = Ak->L[lvl].corres; L.dIdx = Ak->L[lvl].dIdx; L.dIdy = Ak->L[lvl].dIdy;
  L.cols = Ak->L[lvl].cols; L.rows = Ak->L[lvl].rows;
  L.k.fx = Ak->L[lvl].k.fx; L.k.fy = Ak->L[lvl].k.fy; L.k.cx = Ak->L[lvl].k.cx; L.k.cy = Ak->L[lvl].k.cy;
  return L;
}
__device__ __forceinline__ int ft_level_of(unsigned long long levels, int it) { return (int)((levels >> (2 * it)) & 3ull); }
__device__ __forceinline__ unsigned long long ft_granule(unsigned data, unsigned epoch) { return ((unsigned long long)epoch << 32) | data; }
__device__ __forceinline__ void ft_put(unsigned long long* p, unsigned data, unsigned epoch) {
  __hip_atomic_store(p, ft_granule(data, epoch), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long ft_get(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// One converged wavefront sweeps the granules base[stride * i], i < n <= 256 (lane l: i = 4 l .. 4 l + 3), until every one carries
// `epoch`; data[] receives them (0 beyond n).  Returns false when the wait was abandoned (time-out here or flagged elsewhere).
__device__ __forceinline__ bool ft_sweep(const unsigned long long* base, int stride, int n, unsigned epoch, volatile int* dead_s, FtSync* Y,
                                         unsigned (&data)[4]) {
  const int lane = threadIdx.x & 63;
  bool ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { ok[i] = 4 * lane + i >= n; data[i] = 0u; }
  if (*dead_s) return false;
  // (two sweeps in flight instead of one measured slower: exchange B 3.45 -> 4.96 us, 1942 -> 1828 frames/s, profiles/r08i_*; removed, last
  // present in commit 2372c48)
  for (int spin = 0; spin < FT_SPIN; ++spin) {
    unsigned long long g[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = ok[i] ? 0ull : ft_get(base + (size_t)stride * (4 * lane + i));
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (!ok[i] && (unsigned)(g[i] >> 32) == epoch) { ok[i] = true; data[i] = (unsigned)g[i]; }
    if (__all(ok[0] && ok[1] && ok[2] && ok[3])) { __atomic_signal_fence(__ATOMIC_ACQUIRE); return true; }
    if ((spin & 127) == 127 && (__hip_atomic_load(&Y->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) || *dead_s)) { *dead_s = 1; return false; }
    if (spin > 8) __builtin_amdgcn_s_sleep(1);
  }
  __hip_atomic_store(&Y->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  *dead_s = 1;
  return false;
}
// exchange A: one converged wavefront sweeps the FT_WGS records {count, epoch}{sum, epoch} (lane l: records 4 l .. 4 l + 3, both granules of a
// record in flight together) and returns this lane's share of the two integer sums
__device__ __forceinline__ bool ft_sweep_pairs(const unsigned long long* GA, unsigned epoch, volatile int* dead_s, FtSync* Y, int& sa, int& sb) {
  const int lane = threadIdx.x & 63;
  bool ok[4] = {false, false, false, false};
  sa = sb = 0;
  if (*dead_s) return false;
  for (int spin = 0; spin < FT_SPIN; ++spin) {
    unsigned long long ga[4], gb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ga[i] = ok[i] ? 0ull : ft_get(GA + 2 * (4 * lane + i));
      gb[i] = ok[i] ? 0ull : ft_get(GA + 2 * (4 * lane + i) + 1);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (!ok[i] && (unsigned)(ga[i] >> 32) == epoch && (unsigned)(gb[i] >> 32) == epoch) { ok[i] = true; sa += (int)(unsigned)ga[i]; sb += (int)(unsigned)gb[i]; }
    if (__all(ok[0] && ok[1] && ok[2] && ok[3])) { __atomic_signal_fence(__ATOMIC_ACQUIRE); return true; }
    if ((spin & 127) == 127 && (__hip_atomic_load(&Y->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) || *dead_s)) { *dead_s = 1; return false; }
    if (spin > 8) __builtin_amdgcn_s_sleep(1);
  }
  __hip_atomic_store(&Y->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  *dead_s = 1;
  return false;
}
// Round 6, k_track_ref: the same two sweeps with every load instruction of the wavefront on 64 CONSECUTIVE granules (512 bytes: four whole lines)
// instead of every lane on its own four (ft_sweep: a load instruction touched 16 lines, ft_sweep_pairs: 32 — a sweep asked the memory side for
// 64 / 256 line pieces where 16 / 32 carry everything).  The producers store column c's granule at ft_slot(c) = 64 (c % 4) + c / 4, so lane l
// still ends up with columns 4 l .. 4 l + 3 — what the rest of the tree expects.
// (Every lane on its own four granules, rounds 4-5's addressing: removed, last present in commit 2372c48.)
__device__ __forceinline__ int ft_slot(int col) { return 64 * (col & 3) + (col >> 2); }
__device__ __forceinline__ bool ft_sweep_row(const unsigned long long* row, unsigned epoch, volatile int* dead_s, FtSync* Y, unsigned (&data)[4]) {
  const int lane = threadIdx.x & 63;
  bool ok[4] = {false, false, false, false};
#pragma unroll
  for (int i = 0; i < 4; ++i) data[i] = 0u;
  if (*dead_s) return false;
  for (int spin = 0; spin < FT_SPIN; ++spin) {
    unsigned long long g[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = ok[i] ? 0ull : ft_get(row + 64 * i + lane);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (!ok[i] && (unsigned)(g[i] >> 32) == epoch) { ok[i] = true; data[i] = (unsigned)g[i]; }
    if (__all(ok[0] && ok[1] && ok[2] && ok[3])) { __atomic_signal_fence(__ATOMIC_ACQUIRE); return true; }
    if ((spin & 127) == 127 && (__hip_atomic_load(&Y->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) || *dead_s)) { *dead_s = 1; return false; }
    if (spin > 8) __builtin_amdgcn_s_sleep(1);
  }
  __hip_atomic_store(&Y->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  *dead_s = 1;
  return false;
}
// exchange A: the 512 granules {count}{sum} of the 256 records, granule 64 i + l in lane l: an even lane only ever holds counts, an odd lane sums
// (both integer sums are order-free; every granule carries its own tag and the sweep waits for all of them)
__device__ __forceinline__ bool ft_sweep_records(const unsigned long long* GA, unsigned epoch, volatile int* dead_s, FtSync* Y, int& sa, int& sb) {
  const int lane = threadIdx.x & 63;
  bool ok[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ok[i] = false;
  int acc = 0;
  sa = sb = 0;
  if (*dead_s) return false;
  for (int spin = 0; spin < FT_SPIN; ++spin) {
    unsigned long long g[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) g[i] = ok[i] ? 0ull : ft_get(GA + 64 * i + lane);
    bool all = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (!ok[i] && (unsigned)(g[i] >> 32) == epoch) { ok[i] = true; acc += (int)(unsigned)g[i]; }
      all = all && ok[i];
    }
    if (__all(all)) {
      __atomic_signal_fence(__ATOMIC_ACQUIRE);
      sa = (lane & 1) ? 0 : acc;
      sb = (lane & 1) ? acc : 0;
      return true;
    }
    if ((spin & 127) == 127 && (__hip_atomic_load(&Y->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) || *dead_s)) { *dead_s = 1; return false; }
    if (spin > 8) __builtin_amdgcn_s_sleep(1);
  }
  __hip_atomic_store(&Y->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  *dead_s = 1;
  return false;
}
// hop 2 of exchange B: lanes < na poll the totals G2[lane]
__device__ __forceinline__ bool ft_poll_totals(const unsigned long long* G2, int na, unsigned epoch, volatile int* dead_s, FtSync* Y, float& value) {
  const int lane = threadIdx.x & 63;
  bool ok = lane >= na;
  value = 0.f;
  if (*dead_s) return false;
  for (int spin = 0; spin < FT_SPIN; ++spin) {
    if (!ok) {
      const unsigned long long g = ft_get(G2 + lane);
      if ((unsigned)(g >> 32) == epoch) { ok = true; value = __uint_as_float((unsigned)g); }
    }
    if (__all(ok)) return true;
    if ((spin & 127) == 127 && (__hip_atomic_load(&Y->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) || *dead_s)) { *dead_s = 1; return false; }
    if (spin > 8) __builtin_amdgcn_s_sleep(1);
  }
  __hip_atomic_store(&Y->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  *dead_s = 1;
  return false;
}
