// seg_labels.h — class-index label maps (B, 1, *S) as the softmax loss (loss.hip) and the argmax metrics (segmetric.hip)
// read them: in their own element type (FZ_LABEL_U8 / _I64 / _F32), converted in registers, never written back.
// The conversion is torch's .long(): a float label truncates toward zero (so every value in (-1, 1) is class 0).  A label
// outside [0, C) — NaN and ±inf included — names no class: label_class returns -1, which equals no channel index, so its
// one-hot row is all zero.  Nothing here traps: an abort on a shared GPU is worse than a documented convention.
#pragma once
#include "fz_common.h"

namespace fz {

__device__ __forceinline__ int label_class(uint8_t v, int C) { return v < C ? (int)v : -1; }
__device__ __forceinline__ int label_class(int64_t v, int C) { return (v >= 0 && v < (int64_t)C) ? (int)v : -1; }
__device__ __forceinline__ int label_class(float v, int C) { return (v > -1.0f && v < (float)C) ? (int)v : -1; }

// the classes of 4 consecutive labels at p: uint8 one 4-byte load, fp32 one 16-byte load, int64 two 16-byte loads
// (p aligned to the load)
__device__ __forceinline__ void label_classes4(const uint8_t* p, int C, int (&k)[4]) {
  const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) k[e] = label_class((uint8_t)((w >> (8 * e)) & 0xffu), C);
}
__device__ __forceinline__ void label_classes4(const float* p, int C, int (&k)[4]) {
  const float4 w = *reinterpret_cast<const float4*>(p);
  k[0] = label_class(w.x, C), k[1] = label_class(w.y, C), k[2] = label_class(w.z, C), k[3] = label_class(w.w, C);
}
__device__ __forceinline__ void label_classes4(const int64_t* p, int C, int (&k)[4]) {
  const longlong2 a = *reinterpret_cast<const longlong2*>(p), b = *reinterpret_cast<const longlong2*>(p + 2);
  k[0] = label_class((int64_t)a.x, C), k[1] = label_class((int64_t)a.y, C);
  k[2] = label_class((int64_t)b.x, C), k[3] = label_class((int64_t)b.y, C);
}

inline bool label_kind_ok(int k) { return k == FZ_LABEL_U8 || k == FZ_LABEL_I64 || k == FZ_LABEL_F32; }
inline int label_esize(int k) { return k == FZ_LABEL_U8 ? 1 : (k == FZ_LABEL_I64 ? 8 : 4); }
// bytes that label_classes4 loads at once
inline int label_vec_bytes(int k) { return k == FZ_LABEL_U8 ? 4 : 16; }

// f(T{}) with T the element type of label kind k
template <typename F>
inline void by_label_kind(int k, F f) {
  if (k == FZ_LABEL_U8) f(uint8_t{});
  else if (k == FZ_LABEL_I64) f(int64_t{});
  else f(float{});
}

}  // namespace fz
