// Stand-alone driver of elasticfusion_amd/csrc/ef_plane_fit.hpp on the host (tests/test_plane_host.py compiles it with g++ -ffp-contract=off,
// and once more with -fsanitize=address,undefined).  One case per input line, every number as the hexadecimal of its bits:
//   m  a.x a.y a.z  hn.x hn.y hn.z  S0 .. S8        (m decimal; a, hn: 32-bit patterns; S: 64-bit patterns)
// One output line per case: "0" when plane_fit refuses, else "1 n.x n.y n.z d thickness" as 32-bit patterns.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "ef_plane_fit.hpp"

int main() {
  unsigned m;
  uint32_t f[6];
  unsigned long long s[9];
  while (scanf("%u %x %x %x %x %x %x %llx %llx %llx %llx %llx %llx %llx %llx %llx", &m, &f[0], &f[1], &f[2], &f[3], &f[4], &f[5], &s[0], &s[1], &s[2],
               &s[3], &s[4], &s[5], &s[6], &s[7], &s[8]) == 16) {
    float a[3], hn[3], n[3], d, th;
    double S[9];
    memcpy(a, f, sizeof(a));
    memcpy(hn, f + 3, sizeof(hn));
    for (int i = 0; i < 9; ++i) {
      const uint64_t bits = s[i];
      memcpy(&S[i], &bits, sizeof(double));
    }
    if (!efm::plane_fit(S, m, a, hn, n, &d, &th)) {
      printf("0\n");
      continue;
    }
    uint32_t o[5];
    memcpy(o, n, sizeof(n));
    memcpy(o + 3, &d, 4);
    memcpy(o + 4, &th, 4);
    printf("1 %08x %08x %08x %08x %08x\n", o[0], o[1], o[2], o[3], o[4]);
  }
  return 0;
}
