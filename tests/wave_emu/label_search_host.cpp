// TEST INFRASTRUCTURE — the label code's two pieces of index arithmetic (ef_labels.inc), cut out of the product's source by
// tests/test_label_search_emulation.py and compiled for the host over tests/wave_emu/hip/hip_runtime.h:
//   PARTITION_SOURCE  wave_partition_point, the 64-way search, run by 64 host threads, one per lane, that meet at every ballot
//   ROW_OF_SOURCE     the three statements of k_labels_align's flat copy that recover the row of float f
// What this pins is their LOGIC for every input (the guard p < hi, the K == 0 exit, the step arithmetic; the +-1 correction) — on the CPU, for
// good; what the GPU compiler makes of them is the GPU suite's business (tests/test_gpu_label_edges.py).
#include <algorithm>
#include <barrier>
#include <thread>
#include <vector>

#include "hip/hip_runtime.h"

using std::min;
// every lane publishes its bit, then reads all 64
inline unsigned long long __ballot(int t) {
  emu::Wave& W = emu::wave;
  W.slots[W.lane] = t ? 1ull : 0ull;
  W.barrier->arrive_and_wait();
  unsigned long long m = 0;
  for (int i = 0; i < 64; ++i) m |= W.slots[i] << i;
  W.barrier->arrive_and_wait();
  return m;
}
inline int __popcll(unsigned long long m) { return __builtin_popcountll(m); }

#include PARTITION_SOURCE

// cases: n x {lo, hi, boundary}, the predicate p < boundary.  out[lane * n + i] = what the lane returned; *outside = the number of probes
// outside [lo, hi) (the predicate of the product reads memory there)
extern "C" void run_partition(const unsigned* cases, int n, unsigned* out, unsigned* outside) {
  std::barrier<> bar(64);
  std::vector<unsigned long long> slots(64, 0ull);
  std::vector<unsigned> bad(64, 0u);
  std::vector<std::thread> th;
  for (int l = 0; l < 64; ++l)
    th.emplace_back([&, l] {
      emu::wave = emu::Wave{&bar, slots.data(), l};
      emu::lane.tid = uint3e{(unsigned)l + 64u * (unsigned)(l & 1), 0, 0};   // (odd lanes sit in the second wave of a workgroup: k & 63 is the lane)
      for (int i = 0; i < n; ++i) {
        const unsigned lo = cases[3 * i], hi = cases[3 * i + 1], b = cases[3 * i + 2];
        out[(size_t)l * n + i] = wave_partition_point(lo, hi, [&](unsigned p) {
          if (p < lo || p >= hi) ++bad[l];
          return p < b;
        });
      }
    });
  for (auto& t : th) t.join();
  *outside = 0;
  for (unsigned v : bad) *outside += v;
}

static unsigned row_of(unsigned f, unsigned C, float invC) {
#include ROW_OF_SOURCE
  return rr;
}
// the number of f below tile_rows * C whose row is not f / C, for C = c_lo .. c_hi; *uncorrected = how many of them the estimate alone has wrong
extern "C" unsigned run_row_of(unsigned c_lo, unsigned c_hi, unsigned tile_rows, unsigned* uncorrected) {
  unsigned wrong = 0;
  *uncorrected = 0;
  for (unsigned C = c_lo; C <= c_hi; ++C) {
    const float invC = 1.0f / (float)C;
    for (unsigned f = 0; f < tile_rows * C; ++f) {
      wrong += row_of(f, C, invC) != f / C;
      *uncorrected += (unsigned)((float)f * invC) != f / C;
    }
  }
  return wrong;
}
