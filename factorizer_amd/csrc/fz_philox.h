// fz_philox.h — counter-based Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
// SC'11), the generator of the block dropout masks (csrc/dropout.hip).  Host and device: no HIP header is needed, so the
// CPU tests compile this file with a plain C++ compiler and check it against the published known-answer vectors.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FZ_PHILOX_FN __host__ __device__ __forceinline__
#else
#define FZ_PHILOX_FN inline
#endif

namespace fz {

struct philox4x32 {
  uint32_t v[4];
};

FZ_PHILOX_FN void philox_mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
  const uint64_t p = (uint64_t)a * (uint64_t)b;
  hi = (uint32_t)(p >> 32);
  lo = (uint32_t)p;
}

// ten rounds; the key is bumped by the Weyl constants between rounds (the first round uses the key as given)
FZ_PHILOX_FN philox4x32 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0, lo0, hi1, lo1;
    philox_mulhilo(0xD2511F53u, c0, hi0, lo0);
    philox_mulhilo(0xCD9E8D57u, c2, hi1, lo1);
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  philox4x32 out;
  out.v[0] = c0;
  out.v[1] = c1;
  out.v[2] = c2;
  out.v[3] = c3;
  return out;
}

}  // namespace fz
