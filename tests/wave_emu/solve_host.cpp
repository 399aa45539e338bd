// TEST INFRASTRUCTURE — the product's wave-parallel 6x6 LDL^T (efs::ldlt6_wave, elasticfusion_amd/csrc/ef_solve_dev.hpp: one matrix
// element per lane, pivot search and row/column swaps through cross-lane shuffles) executed on the host: 64 host threads are the 64
// lanes (tests/wave_emu/hip/hip_runtime.h).  Built by tests/test_wave_emulation.py.
#include <hip/hip_runtime.h>
#include <thread>
#include <vector>
#include "ef_solve_dev.hpp"

extern "C" void run_ldlt6_wave(const double* A36, const double* b6, double* x6) {
  static efs::SolveScratch S;
  for (int i = 0; i < 6; ++i) S.b[i] = b6[i];
  unsigned long long slots[64];
  std::barrier<> bar(64);
  std::vector<std::thread> th;
  for (int l = 0; l < 64; ++l)
    th.emplace_back([&, l] {
      emu::lane.tid = {(unsigned)l, 0, 0};
      emu::lane.bdim = {64, 1, 1};
      emu::wave.barrier = &bar; emu::wave.slots = slots; emu::wave.lane = l;
      efs::ldlt6_wave(l < 36 ? A36[l] : 0.0, S);
    });
  for (auto& t : th) t.join();
  for (int i = 0; i < 6; ++i) x6[i] = S.x[i];
}
// ... and the variant that keeps the whole (lower-triangular) matrix in every lane's registers (efs::ldlt6_every_lane): no cross-lane traffic
// but the LDS round trip that gathers the matrix, so four emulated lanes are as good as 64
extern "C" void run_ldlt6_every_lane(const double* A36, const double* b6, double* x6) {
  static efs::SolveScratch S;
  for (int i = 0; i < 6; ++i) S.b[i] = b6[i];
  unsigned long long slots[64];
  std::barrier<> bar(64);
  std::vector<std::thread> th;
  for (int l = 0; l < 64; ++l)
    th.emplace_back([&, l] {
      emu::lane.tid = {(unsigned)l, 0, 0};
      emu::lane.bdim = {64, 1, 1};
      emu::wave.barrier = &bar; emu::wave.slots = slots; emu::wave.lane = l;
      efs::ldlt6_every_lane(l < 36 ? A36[l] : 0.0, S);
    });
  for (auto& t : th) t.join();
  for (int i = 0; i < 6; ++i) x6[i] = S.x[i];
}
// The whole update step (efs::gauss_newton_update_wave: A and b from the 58 sums, the factorisation, computeUpdateSE3, upd * resultRt, the
// float pose and K R K^-1 / K t of the coming iteration) on 64 emulated lanes, behind the prefetch the kernels do (solve_prefetch /
// solve_prefetch_publish).  split: the SPLIT_TAIL form, whose two tails the caller dispatches — here one after the other on the same lanes.
extern "C" void run_gn_update(int split, const float* sums58, const double* prevRt16, const float* Rprev9, const float* tprev3, int icp, int rgb,
                              int rgbOnly, float icpWeight, const float* knext4, double* resultRt16, float* Rcurr9, float* tcurr3,
                              float* krkinv9, float* kt3, double* lastA36, double* lastb6) {
  static efs::SolveScratch S;
  static eft::TrackState st;
  std::memset(&st, 0, sizeof(st));
  std::memset(&S, 0, sizeof(S));
  for (int i = 0; i < 16; ++i) st.gn[0].resultRt[i] = prevRt16[i];
  for (int i = 0; i < 9; ++i) st.Rprev[i] = Rprev9[i];
  for (int i = 0; i < 3; ++i) st.tprev[i] = tprev3[i];
  const efs::SolveInputs in{icp != 0, rgb != 0, rgbOnly != 0, icpWeight, eft::Intr{knext4[0], knext4[1], knext4[2], knext4[3]}, false};
  unsigned long long slots[64];
  std::barrier<> bar(64);
  std::vector<std::thread> th;
  for (int l = 0; l < 64; ++l)
    th.emplace_back([&, l] {
      emu::lane.tid = {(unsigned)l, 0, 0};
      emu::lane.bdim = {64, 1, 1};
      emu::wave.barrier = &bar; emu::wave.slots = slots; emu::wave.lane = l;
      const efs::SolvePrefetch PF = efs::solve_prefetch(&st, &st.gn[0], &st.rgb_slots[0][0][0]);
      efs::solve_prefetch_publish(PF, S);
      efs::wave_sync();
      if (split) {
        efs::gauss_newton_update_wave<true>(&st, &st.gn[1], true, sums58, in, S, true);
        if (S.tail_pending) {
          efs::gn_tail_pose(S, &st.gn[1], true);
          efs::gn_tail_krk(in.knext, S, &st.gn[1], true);
        }
      } else {
        efs::gauss_newton_update_wave<false>(&st, &st.gn[1], true, sums58, in, S, true);
      }
    });
  for (auto& t : th) t.join();
  const eft::GNState& g = st.gn[1];
  for (int i = 0; i < 16; ++i) resultRt16[i] = g.resultRt[i];
  for (int i = 0; i < 9; ++i) { Rcurr9[i] = g.Rcurr[i]; krkinv9[i] = g.krkinv[i]; }
  for (int i = 0; i < 3; ++i) { tcurr3[i] = g.tcurr[i]; kt3[i] = g.kt[i]; }
  for (int i = 0; i < 36; ++i) lastA36[i] = st.lastA[i];
  for (int i = 0; i < 6; ++i) lastb6[i] = st.lastb[i];
}
// the scalar statement of the same algorithm (efl::ldlt_solve<double, 6>: the Eigen::LDLT restatement the device evaluates on one lane)
extern "C" void run_ldlt6_scalar(const double* A36, const double* b6, double* x6) { efl::ldlt_solve<double, 6>(A36, b6, x6); }
