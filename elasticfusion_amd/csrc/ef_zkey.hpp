// The depth half of a z-buffer key (ef_map_kernels.hip: key = (depth_key(z) << 32) | surfel id, resolved by atomicMin).
// depth_key is an order-preserving map of the floats onto uint32 (negative floats below positive ones) in which -0 and +0 share ONE key, as
// they compare equal under the reference's depth test `z < zbuf`: two fragments at -0 and +0 tie, and the id half of the key gives the pixel
// to the lower surfel id ("Ties at zero").  depth_of_key is its inverse on every other bit pattern, NaN payloads included: a
// consumer of the z-buffer reads the winner's depth out of the key, bit for bit the float the splat put in, except that a zero comes back
// as +0 — a consumer that hands the sign of a zero on (k_depth_resolve) recomputes the winner's fragment.  Plain C++ so that a host
// translation unit can sweep the pair (tests/test_zkey_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EF_ZKEY_HD __host__ __device__ __forceinline__
#else
#define EF_ZKEY_HD inline
#endif

namespace efm {

EF_ZKEY_HD uint32_t depth_key(float z) {  // order-preserving float -> uint
  uint32_t b;
  __builtin_memcpy(&b, &z, 4);
  if (b == 0x80000000u) b = 0u;   // -0 ties with +0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
EF_ZKEY_HD float depth_of_key(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float z;
  __builtin_memcpy(&z, &b, 4);
  return z;
}

}  // namespace efm
