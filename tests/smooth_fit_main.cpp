// Stand-alone driver of smooth_fit of elasticfusion_amd/csrc/ef_plane_fit.hpp on the host (tests/test_smooth_host.py compiles it with g++
// -ffp-contract=off, and once more with -fsanitize=address,undefined).  One case per input line, every number as the hexadecimal of its bits:
//   m  hn.x hn.y hn.z  line_ratio  W  S0 .. S8        (m decimal; hn, line_ratio: 32-bit patterns; W, S: 64-bit patterns)
// One output line per case: "status n.x n.y n.z mean.x mean.y mean.z curvature" (status decimal; n, mean: 64-bit patterns; curvature: a 32-bit
// pattern), status being smooth_fit's return value.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "ef_plane_fit.hpp"

int main() {
  unsigned m;
  uint32_t f[4];
  unsigned long long w, s[9];
  while (scanf("%u %x %x %x %x %llx %llx %llx %llx %llx %llx %llx %llx %llx %llx", &m, &f[0], &f[1], &f[2], &f[3], &w, &s[0], &s[1], &s[2], &s[3], &s[4],
               &s[5], &s[6], &s[7], &s[8]) == 15) {
    float hn[3], line_ratio, curv;
    double S[9], W, n[3], mean[3];
    memcpy(hn, f, sizeof(hn));
    memcpy(&line_ratio, f + 3, 4);
    const uint64_t wbits = w;
    memcpy(&W, &wbits, sizeof(double));
    for (int i = 0; i < 9; ++i) {
      const uint64_t bits = s[i];
      memcpy(&S[i], &bits, sizeof(double));
    }
    const int status = efm::smooth_fit(S, W, m, hn, line_ratio, n, mean, &curv);
    uint64_t o[6];
    uint32_t c;
    memcpy(o, n, sizeof(n));
    memcpy(o + 3, mean, sizeof(mean));
    memcpy(&c, &curv, 4);
    printf("%d %016llx %016llx %016llx %016llx %016llx %016llx %08x\n", status, (unsigned long long)o[0], (unsigned long long)o[1],
           (unsigned long long)o[2], (unsigned long long)o[3], (unsigned long long)o[4], (unsigned long long)o[5], c);
  }
  return 0;
}
