// Stand-alone driver of elasticfusion_amd/csrc/ef_boundary_gap.hpp on the host (tests/test_boundary_host.py compiles it with g++
// -ffp-contract=off, and once more with -fsanitize=address,undefined).  One case per input line, every number as the hexadecimal of its bits:
//   G c  m.x m.y m.z  p.x p.y p.z  then c times  t.x t.y t.z      (c decimal, 0 .. 16; 32-bit patterns): boundary_gap<16> of one row
//   T xj yj xi yi below                                            (64-bit patterns; below decimal 0 / 1): boundary_turn
// One output line per case: "status G" (status decimal: 0 a gap, 1 DEGENERATE; G a 64-bit pattern, 0 when DEGENERATE) or "t" (64-bit pattern).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "ef_boundary_gap.hpp"

static double from_bits(unsigned long long b) {
  const uint64_t u = b;
  double d;
  memcpy(&d, &u, sizeof(d));
  return d;
}
static unsigned long long to_bits(double d) {
  uint64_t u;
  memcpy(&u, &d, sizeof(u));
  return (unsigned long long)u;
}

int main() {
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'T') {
      unsigned long long b[4];
      int below;
      if (scanf("%llx %llx %llx %llx %d", &b[0], &b[1], &b[2], &b[3], &below) != 5) return 2;
      printf("%016llx\n", to_bits(efm::boundary_turn(from_bits(b[0]), from_bits(b[1]), from_bits(b[2]), from_bits(b[3]), below != 0)));
      continue;
    }
    if (kind != 'G') return 2;
    int c;
    uint32_t w[6];
    if (scanf("%d %x %x %x %x %x %x", &c, &w[0], &w[1], &w[2], &w[3], &w[4], &w[5]) != 7 || c < 0 || c > 16) return 2;
    float m[3], p[3], px[16], py[16], pz[16];
    memcpy(m, w, sizeof(m));
    memcpy(p, w + 3, sizeof(p));
    for (int j = 0; j < 16; ++j) { px[j] = p[0]; py[j] = p[1]; pz[j] = p[2]; }   // a slot from c on holds the row itself, as on the device
    for (int j = 0; j < c; ++j) {
      uint32_t t[3];
      if (scanf("%x %x %x", &t[0], &t[1], &t[2]) != 3) return 2;
      memcpy(&px[j], &t[0], 4);
      memcpy(&py[j], &t[1], 4);
      memcpy(&pz[j], &t[2], 4);
    }
    double G = 0.0;
    const int status = efm::boundary_gap<16>(m, p, px, py, pz, c, &G);
    printf("%d %016llx\n", status, status == efm::BOUNDARY_GAP_OK ? to_bits(G) : 0ull);
  }
  return 0;
}
