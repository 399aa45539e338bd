// The depth half of a z-buffer key (ef_map_kernels.hip: key = (depth_key(z) << 32) | surfel id, resolved by atomicMin).
// depth_key is an order-preserving map of ALL float bit patterns onto uint32 (negative floats below positive ones, -0 below +0), and
// depth_of_key is its exact inverse: a consumer of the z-buffer reads the winner's depth out of the key, bit for bit the float the splat
// put in.  Plain C++ so that a host translation unit can sweep the pair (tests/test_zkey_host.py).
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
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
EF_ZKEY_HD float depth_of_key(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float z;
  __builtin_memcpy(&z, &b, 4);
  return z;
}

}  // namespace efm
