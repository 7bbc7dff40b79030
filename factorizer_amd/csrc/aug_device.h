// aug_device.h — what the augmentation kernels of augment.hip and aug_crop.hip share: the record layout, the noise normals, the
// position arithmetic of the gather (aug_source), its two readers (aug_linear, aug_nearest), the image epilogue (aug_finish) and
// the host-side checks.  Both resample kernels call the SAME device functions with the same roi-sized geometry, so a crop read
// through aug_crop.hip and the same crop copied out and read through augment.hip give the same bits.
#pragma once
#include <string>

#include "fz_common.h"
#include "fz_philox.h"

namespace fz {

// parameter record of one sample: AUG_REC fp32 values (fz_aug_record_floats; layout in include/factorizer_hip.h)
constexpr int AUG_REC = 48;
constexpr int AUG_A = 0, AUG_FLIP = 9, AUG_STD = 12, AUG_GAIN = 13, AUG_OFF = 14, AUG_SLOT = 15, AUG_TAIL = 16, AUG_TAPS = 19;
constexpr uint32_t AUG_STREAM = 0x41554731u;   // fourth counter word: keeps this field apart from the dropout sites 0..2

#if defined(__HIPCC__)
// the four normals of counter (q, c, b): two Box-Muller pairs, accurate logf / sinf / cosf
__device__ __forceinline__ void aug_normals4(uint32_t q, uint32_t c, uint32_t b, uint32_t k0, uint32_t k1, float (&z)[4]) {
  const philox4x32 r = philox4x32_10(q, c, b, AUG_STREAM, k0, k1);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float u0 = ((float)(r.v[2 * i] >> 8) + 0.5f) * 5.9604644775390625e-08f;       // 2^-24; in (0, 1]
    const float u1 = ((float)(r.v[2 * i + 1] >> 8) + 0.5f) * 5.9604644775390625e-08f;
    const float rad = sqrtf(-2.0f * logf(u0));
    const float ang = 6.283185307179586f * u1;
    z[2 * i] = rad * cosf(ang);
    z[2 * i + 1] = rad * sinf(ang);
  }
}

// element k (0..6) of two register quads without dynamic register indexing
__device__ __forceinline__ float aug_pick(const float (&a)[4], const float (&b)[4], int k) {
  float r = a[0];
#pragma unroll
  for (int j = 1; j < 4; ++j) r = k == j ? a[j] : r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r = k == 4 + j ? b[j] : r;
  return r;
}

struct AugCoord {   // clamped source position of one output voxel
  float pz, py, px;
};

// D, H, W: the extents the positions live in (the image, or the crop box of aug_crop.hip)
template <int ND>
__device__ __forceinline__ AugCoord aug_source(const float (&A)[9], int oz, int oy, int ox, int D, int H, int W) {
  const float cz = 0.5f * (float)(D - 1), cy = 0.5f * (float)(H - 1), cx = 0.5f * (float)(W - 1);
  const float d0 = (float)oz - cz, d1 = (float)oy - cy, d2 = (float)ox - cx;   // exact: integers and half-integers below 2^12
  AugCoord p;
  if constexpr (ND == 3) {
    p.pz = __builtin_fmaf(A[0], d0, __builtin_fmaf(A[1], d1, A[2] * d2)) + cz;
    p.py = __builtin_fmaf(A[3], d0, __builtin_fmaf(A[4], d1, A[5] * d2)) + cy;
    p.px = __builtin_fmaf(A[6], d0, __builtin_fmaf(A[7], d1, A[8] * d2)) + cx;
    p.pz = __builtin_fminf(__builtin_fmaxf(p.pz, 0.f), (float)(D - 1));
  } else {
    p.pz = 0.f;
    p.py = __builtin_fmaf(A[4], d1, A[5] * d2) + cy;
    p.px = __builtin_fmaf(A[7], d1, A[8] * d2) + cx;
  }
  p.py = __builtin_fminf(__builtin_fmaxf(p.py, 0.f), (float)(H - 1));
  p.px = __builtin_fminf(__builtin_fmaxf(p.px, 0.f), (float)(W - 1));
  return p;
}

// D, H, W bound the corner indices (the "+1" corner never leaves them); sH, sW are the extents of the memory `src` points into:
// voxel (z, y, x) of the box sits at src[(z sH + y) sW + x].  A dense image passes sH = H, sW = W.
template <typename AT, int ND>
__device__ __forceinline__ float aug_linear(const AT* __restrict__ src, const AugCoord& p, int D, int H, int W, int sH, int sW) {
  const int y0 = (int)p.py, x0 = (int)p.px;                    // p >= 0: truncation is floor
  const float fy = p.py - (float)y0, fx = p.px - (float)x0;
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  if constexpr (ND == 3) {
    const int z0 = (int)p.pz;
    const float fz = p.pz - (float)z0;
    const int z1 = min(z0 + 1, D - 1);
    const int r00 = (z0 * sH + y0) * sW, r01 = (z0 * sH + y1) * sW, r10 = (z1 * sH + y0) * sW, r11 = (z1 * sH + y1) * sW;
    const float v000 = aget(src + r00 + x0), v001 = aget(src + r00 + x1), v010 = aget(src + r01 + x0), v011 = aget(src + r01 + x1);
    const float v100 = aget(src + r10 + x0), v101 = aget(src + r10 + x1), v110 = aget(src + r11 + x0), v111 = aget(src + r11 + x1);
    const float a00 = __builtin_fmaf(fx, v001 - v000, v000), a01 = __builtin_fmaf(fx, v011 - v010, v010);
    const float a10 = __builtin_fmaf(fx, v101 - v100, v100), a11 = __builtin_fmaf(fx, v111 - v110, v110);
    const float b0 = __builtin_fmaf(fy, a01 - a00, a00), b1 = __builtin_fmaf(fy, a11 - a10, a10);
    return __builtin_fmaf(fz, b1 - b0, b0);
  } else {
    const int r0 = y0 * sW, r1 = y1 * sW;
    const float v00 = aget(src + r0 + x0), v01 = aget(src + r0 + x1), v10 = aget(src + r1 + x0), v11 = aget(src + r1 + x1);
    const float a0 = __builtin_fmaf(fx, v01 - v00, v00), a1 = __builtin_fmaf(fx, v11 - v10, v10);
    return __builtin_fmaf(fy, a1 - a0, a0);
  }
}

template <int ND>
__device__ __forceinline__ int aug_nearest(const AugCoord& p, int sH, int sW) {
  const int y = (int)(p.py + 0.5f), x = (int)(p.px + 0.5f);   // p in [0, N - 1]: floor(p + 0.5) <= N - 1
  const int z = ND == 3 ? (int)(p.pz + 0.5f) : 0;
  return (z * sH + y) * sW + x;
}

// What follows the gather of an image lane: v holds the n (VEC: 4) resampled values of output voxels o .. o + n - 1 of plane pl
// of sample b.  Noise of the OUTPUT voxel, then either the fp32 store into the sample's smoothing slot or gain / offset and the
// store to `out`.  V = voxels per output plane.
template <typename AT, bool VEC>
__device__ __forceinline__ void aug_finish(float (&v)[4], int n, int o, int pl, int b, const float* __restrict__ rec,
                                           const int64_t* __restrict__ seed, float* __restrict__ ws, int ns, int C, int V,
                                           AT* __restrict__ out) {
  const float nstd = rec[AUG_STD], gain = rec[AUG_GAIN], off = rec[AUG_OFF];
  const int slot = (int)rec[AUG_SLOT];
  const bool smooth = ws != nullptr && slot >= 0 && slot < ns;
  if (seed != nullptr && nstd > 0.f) {
    const uint64_t s = (uint64_t)*seed;
    const uint32_t k0 = (uint32_t)s, k1 = (uint32_t)(s >> 32);
    const int sh = o & 3;                    // VEC: 0 in every lane
    float za[4], zb[4] = {0.f, 0.f, 0.f, 0.f};
    aug_normals4((uint32_t)(o >> 2), (uint32_t)pl, (uint32_t)b, k0, k1, za);
    if (!VEC && sh != 0) aug_normals4((uint32_t)(o >> 2) + 1u, (uint32_t)pl, (uint32_t)b, k0, k1, zb);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(nstd, VEC ? za[e] : aug_pick(za, zb, sh + e), v[e]);
  }
  if (smooth) {
    float* dst = ws + ((int64_t)slot * C + pl) * V + o;
    if (VEC) astore<4>(dst, v);
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < n) dst[e] = v[e];
    }
    return;
  }
  if (gain != 1.f || off != 0.f) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(v[e], gain, off);
  }
  AT* dst = out + ((int64_t)b * C + pl) * V + o;
  if (VEC) astore<4>(dst, v);
  else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < n) aput(dst + e, v[e]);
  }
}
#endif  // __HIPCC__

inline bool aug_aligned(const void* p, int bytes) { return !p || ((uintptr_t)p % (uintptr_t)bytes) == 0; }

// the checks the batch entry points share (D, H, W: the output geometry); V out: voxels per plane
inline int aug_check_geometry(const char* who, int B, int nd, int D, int H, int W, int64_t* V) {
  const std::string w(who);
  if (nd != 2 && nd != 3) return fail(FZ_E_ARG, (w + ": nd must be 2 or 3 spatial axes").c_str());
  if (B < 1 || B > 65535 || D < 1 || H < 1 || W < 1) return fail(FZ_E_SHAPE, (w + ": sizes must be positive, B <= 65535").c_str());
  if (D > 2048 || H > 2048 || W > 2048) return fail(FZ_E_SHAPE, (w + ": an extent above 2048").c_str());
  if (nd == 2 && D != 1) return fail(FZ_E_SHAPE, (w + ": the lifted axis of a 2-D image must be 1").c_str());
  *V = (int64_t)D * H * W;
  if (*V >= ((int64_t)1 << 31)) return fail(FZ_E_UNSUPPORTED, (w + ": 2^31 or more voxels per plane").c_str());
  return FZ_OK;
}

}  // namespace fz
