// inorm_device.h — the device-side helpers the instance norm (csrc/inorm.hip) and the group norm (csrc/gnorm.hip) share:
// 16-byte group loads and stores with the one rounding of inorm_core.h, and the fixed LDS tree over a workgroup.
#pragma once
#include "fz_common.h"
#include "inorm_core.h"

namespace fz {

template <typename T> __device__ __forceinline__ bool inorm_vec(const T* p) { return ((uintptr_t)p & 15u) == 0; }

// elements i0 .. i0 + W - 1 of a plane (those below hi; the others read as 0) as floats; i0 is a multiple of W
template <typename T, int W>
__device__ __forceinline__ void inorm_load(const T* p, int64_t i0, int64_t hi, bool vec, float (&v)[W]) {
  if (vec && i0 + W <= hi) {
    aload<W>(p + i0, v);
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = i0 + k < hi ? aget(p + i0 + k) : 0.0f;
  }
}
__device__ __forceinline__ void inorm_store(float* p, int64_t i0, int64_t hi, bool vec, const double (&r)[4]) {
  float f[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) f[k] = inorm_round_f32(r[k]);
  if (vec && i0 + 4 <= hi) {
    astore<4>(p + i0, f);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k < hi) p[i0 + k] = f[k];
  }
}
__device__ __forceinline__ void inorm_store(bf16* p, int64_t i0, int64_t hi, bool vec, const double (&r)[8]) {
  uint32_t h[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = inorm_round_bf16(r[k]);
  if (vec && i0 + 8 <= hi) {
    *reinterpret_cast<uint4*>(p + i0) = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
  } else {
    uint16_t* q = reinterpret_cast<uint16_t*>(p);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (i0 + k < hi) q[i0 + k] = (uint16_t)h[k];
  }
}

// totals of one pair of values per thread, in every thread: the tree of inorm_core.h over LDS
__device__ __forceinline__ void inorm_block_sum2(double& a, double& b, double (*red)[INORM_THREADS]) {
  const int t = threadIdx.x;
  __syncthreads();   // red may still be read from the previous call
  red[0][t] = a;
  red[1][t] = b;
  __syncthreads();
  for (int w = INORM_THREADS / 2; w > 0; w >>= 1) {
    inorm_tree_step(red[0], t, w);
    inorm_tree_step(red[1], t, w);
    __syncthreads();
  }
  a = red[0][0];
  b = red[1][0];
}

}  // namespace fz
