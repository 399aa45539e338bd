// Stand-alone driver of normal_fit of elasticfusion_amd/csrc/ef_plane_fit.hpp on the host (tests/test_normals_host.py compiles it with g++
// -ffp-contract=off, and once more with -fsanitize=address,undefined).  One case per input line, every number as the hexadecimal of its bits:
//   m  hn.x hn.y hn.z  line_ratio  S0 .. S8        (m decimal; hn, line_ratio: 32-bit patterns; S: 64-bit patterns)
// One output line per case: "status n.x n.y n.z curvature flipped l0 l1 l2" (status, flipped decimal; n, curvature: 32-bit patterns; l: 64-bit
// patterns), status being normal_fit's return value.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "ef_plane_fit.hpp"

int main() {
  unsigned m;
  uint32_t f[4];
  unsigned long long s[9];
  while (scanf("%u %x %x %x %x %llx %llx %llx %llx %llx %llx %llx %llx %llx", &m, &f[0], &f[1], &f[2], &f[3], &s[0], &s[1], &s[2], &s[3], &s[4], &s[5],
               &s[6], &s[7], &s[8]) == 14) {
    float hn[3], line_ratio, n[3], curv;
    double S[9], l[3];
    bool flipped;
    memcpy(hn, f, sizeof(hn));
    memcpy(&line_ratio, f + 3, 4);
    for (int i = 0; i < 9; ++i) {
      const uint64_t bits = s[i];
      memcpy(&S[i], &bits, sizeof(double));
    }
    const int status = efm::normal_fit(S, m, hn, line_ratio, n, &curv, &flipped, l);
    uint32_t o[4];
    uint64_t lo[3];
    memcpy(o, n, sizeof(n));
    memcpy(o + 3, &curv, 4);
    memcpy(lo, l, sizeof(l));
    printf("%d %08x %08x %08x %08x %d %016llx %016llx %016llx\n", status, o[0], o[1], o[2], o[3], flipped ? 1 : 0, (unsigned long long)lo[0],
           (unsigned long long)lo[1], (unsigned long long)lo[2]);
  }
  return 0;
}
