// aug_crop.hip — the random training crop of the recipe cut INSIDE the augmentation gather (DESIGN.md §3.13;
// factorizer_amd/augment.py restates the semantics).  `RandSpatialCropd(roi_size, random_size=False)` is the first entry of every
// bundle's `random_transforms` (model_zoo/factorizer_brats23/configs/train.yaml); the rest of that list is augment.hip.  One
// kernel:
//   aug_crop_resample   aug_resample of augment.hip with one difference: sample b is read from ITS OWN source volume
//                  (C, sD, sH, sW) + (L, sD, sH, sW) at ITS OWN integer origin g, both taken from a device table of
//                  fz_aug_source_words() int64 words per sample.  The output (B, C + L, D, H, W) is the roi.  Positions are formed
//                  in crop coordinates by the same aug_source call and clamped to [0, roi - 1]; the corner indices that
//                  aug_linear / aug_nearest derive from them are scaled by the SOURCE row and plane extents, and the origin
//                  enters once, in the plane base pointer — so nothing outside the box [g, g + roi) is read, and the values are
//                  those of aug_resample run on a copy of the box, bit for bit.  Noise counters, smoothing slots and gain /
//                  offset are aug_finish, shared with aug_resample; fz_aug_smooth runs behind it unchanged.
//                  A sample whose table entry is unusable — a null or misaligned base where a plane is expected, a box that
//                  leaves the extents, a source plane of 2^31 voxels or more — is skipped: the test is uniform per workgroup,
//                  nothing is read through the entry and nothing is written for the sample.
//                  VEC (template) is the OUTPUT side: roi W % 4 == 0 and aligned outputs.  On the identity path the SOURCE side
//                  takes one vector load per lane where the sample's origin x, source W and base put every lane's first
//                  element on a 4-BYTE boundary (a multi-dword load needs dword alignment only): always for fp32, even origin
//                  x and source W and a 4-byte aligned base for bf16, multiples of four for the one-byte labels; four scalar
//                  loads otherwise.  Decided per sample, uniform per workgroup, same bits.
// In-plane offsets are 32-bit; the 64-bit plane base is formed once per workgroup from the table.
#include "aug_device.h"

namespace fz {

// source table entry of one sample: AUG_SRC int64 words (fz_aug_source_words; layout in include/factorizer_hip.h)
constexpr int AUG_SRC = 8;
constexpr int SRC_IMG = 0, SRC_LAB = 1, SRC_EXT = 2, SRC_ORG = 5;

// a table word as a pointer into GLOBAL memory (an integer turned into a plain pointer would be read with flat loads)
template <typename T>
__device__ __forceinline__ const T* aug_global(uint64_t address) {
  return (const T*)reinterpret_cast<const __attribute__((address_space(1))) T*>(address);
}

// four consecutive elements from a 4-byte aligned address (aload<4> of fz_common.h wants them aligned to all four)
__device__ __forceinline__ void aug_load4(const float* p, float (&v)[4]) {
  f32v4 t;
  __builtin_memcpy(&t, p, sizeof(t));
  v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
}
__device__ __forceinline__ void aug_load4(const bf16* p, float (&v)[4]) {
  bf16v4 t;
  __builtin_memcpy(&t, __builtin_assume_aligned(p, 4), sizeof(t));
  const f32v4 f = __builtin_convertvector(t, f32v4);
  v[0] = f[0]; v[1] = f[1]; v[2] = f[2]; v[3] = f[3];
}

template <typename AT, int ND, bool VEC>
__global__ __launch_bounds__(256) void aug_crop_resample_kernel(const int64_t* __restrict__ sources, AT* __restrict__ out,
                                                                float* __restrict__ ws, int ns, int C, uint8_t* __restrict__ lab_out,
                                                                int L, const float* __restrict__ table,
                                                                const int64_t* __restrict__ seed, int D, int H, int W, int Wq, int nq) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const int b = blockIdx.z, pl = blockIdx.y;
  // ---- the sample's source: uniform per workgroup
  const int64_t* st = sources + (int64_t)b * AUG_SRC;
  const uint64_t ip = (uint64_t)st[SRC_IMG], lp = (uint64_t)st[SRC_LAB];
  const int64_t sD = st[SRC_EXT], sH = st[SRC_EXT + 1], sW = st[SRC_EXT + 2];
  const int64_t gz = st[SRC_ORG], gy = st[SRC_ORG + 1], gx = st[SRC_ORG + 2];
  constexpr int64_t LIM = (int64_t)1 << 31;
  bool ok = (C == 0 || (ip != 0 && ip % sizeof(AT) == 0)) && (L == 0 || lp != 0);
  ok = ok && sD >= 1 && sD < LIM && sH >= 1 && sH < LIM && sW >= 1 && sW < LIM;
  ok = ok && sH * sW < LIM && sD * (sH * sW) < LIM;            // evaluated only once each factor is below 2^31: no overflow
  ok = ok && gz >= 0 && gz <= sD - D && gy >= 0 && gy <= sH - H && gx >= 0 && gx <= sW - W;
  if (!ok) return;
  const int sHi = (int)sH, sWi = (int)sW;
  const int64_t sV = sD * sH * sW;
  const int org = ((int)gz * sHi + (int)gy) * sWi + (int)gx;   // first voxel of the box inside a source plane
  // identity path: does every lane's first source element sit on a 4-byte boundary (x4 and roi W are multiples of 4 under VEC)
  const bool ivec = VEC && (sizeof(AT) == 4 || (((gx | sW) & 1) == 0 && (ip & 3) == 0));
  const bool lvec = VEC && ((gx | sW) & 3) == 0 && (lp & 3) == 0;

  const float* rec = table + (int64_t)b * AUG_REC;
  float A[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) A[k] = rec[AUG_A + k];
  const bool ident = A[0] == 1.f && A[1] == 0.f && A[2] == 0.f && A[3] == 0.f && A[4] == 1.f && A[5] == 0.f && A[6] == 0.f &&
                     A[7] == 0.f && A[8] == 1.f;
  const bool flz = ND == 3 && rec[AUG_FLIP] != 0.f, fly = rec[AUG_FLIP + 1] != 0.f, flx = rec[AUG_FLIP + 2] != 0.f;
  const int row = q / Wq, x4 = (q - row * Wq) * 4;
  const int z = ND == 3 ? row / H : 0, y = row - z * H;
  const int oz = flz ? D - 1 - z : z, oy = fly ? H - 1 - y : y;
  const int n = min(4, W - x4);
  const int V = D * H * W;
  const int o = row * W + x4;                // flat output voxel of the lane's first element
  const int srow = (oz * sHi + oy) * sWi;    // identity: the row of the box, relative to its first voxel

  if (pl >= C) {   // ---- label plane: nearest
    const uint8_t* src = aug_global<uint8_t>(lp) + (int64_t)(pl - C) * sV + org;
    uint8_t* dst = lab_out + ((int64_t)b * L + (pl - C)) * V;
    if (VEC && ident && lvec) {
      uint32_t w = *reinterpret_cast<const uint32_t*>(src + srow + (flx ? W - 4 - x4 : x4));
      if (flx) w = __builtin_bswap32(w);
      *reinterpret_cast<uint32_t*>(dst + o) = w;
      return;
    }
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < n) {
        const int ox = flx ? W - 1 - (x4 + e) : x4 + e;
        const int si = ident ? srow + ox : aug_nearest<ND>(aug_source<ND>(A, oz, oy, ox, D, H, W), sHi, sWi);
        const uint32_t v = src[si];
        if (VEC) w |= v << (8 * e);
        else dst[o + e] = (uint8_t)v;
      }
    }
    if (VEC) *reinterpret_cast<uint32_t*>(dst + o) = w;
    return;
  }

  // ---- image plane
  const AT* src = aug_global<AT>(ip) + (int64_t)pl * sV + org;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (ident) {
    if (VEC && ivec) {
      float t[4];
      aug_load4(src + srow + (flx ? W - 4 - x4 : x4), t);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = flx ? t[3 - e] : t[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < n) v[e] = aget(src + srow + (flx ? W - 1 - (x4 + e) : x4 + e));
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < n) {
        const int ox = flx ? W - 1 - (x4 + e) : x4 + e;
        v[e] = aug_linear<AT, ND>(src, aug_source<ND>(A, oz, oy, ox, D, H, W), D, H, W, sHi, sWi);
      }
    }
  }
  aug_finish<AT, VEC>(v, n, o, pl, b, rec, seed, ws, ns, C, V, out);
}

template <typename AT, int ND>
static void aug_crop_launch(bool vec, dim3 grid, hipStream_t s, const int64_t* sources, void* out, float* ws, int ns, int C,
                            uint8_t* lab_out, int L, const float* table, const int64_t* seed, int D, int H, int W, int Wq, int nq) {
  if (vec)
    hipLaunchKernelGGL((aug_crop_resample_kernel<AT, ND, true>), grid, dim3(256), 0, s, sources, (AT*)out, ws, ns, C, lab_out, L,
                       table, seed, D, H, W, Wq, nq);
  else
    hipLaunchKernelGGL((aug_crop_resample_kernel<AT, ND, false>), grid, dim3(256), 0, s, sources, (AT*)out, ws, ns, C, lab_out, L,
                       table, seed, D, H, W, Wq, nq);
}

}  // namespace fz

using namespace fz;

extern "C" int fz_aug_source_words(void) { return AUG_SRC; }

extern "C" int fz_aug_crop_resample(const int64_t* sources, void* img_out, int act_dtype, int C, uint8_t* lab_out, int L,
                                    const float* table, const int64_t* seed, float* smooth_ws, int ns, int B, int nd, int D, int H,
                                    int W, fz_stream_t stream) {
  if (!sources) return fail(FZ_E_ARG, "fz_aug_crop_resample: null source table");
  if (!table) return fail(FZ_E_ARG, "fz_aug_crop_resample: null table");
  if (C < 0 || L < 0 || C + L < 1 || C + L > 65535)
    return fail(FZ_E_SHAPE, "fz_aug_crop_resample: 1 <= C + L <= 65535 planes per sample");
  if ((C > 0 && !img_out) || (L > 0 && !lab_out)) return fail(FZ_E_ARG, "fz_aug_crop_resample: null pointer");
  if (C > 0 && act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16) return fail(FZ_E_ARG, "fz_aug_crop_resample: bad act_dtype");
  if (ns < 0 || ns > B || (ns > 0 && !smooth_ws))
    return fail(FZ_E_ARG, "fz_aug_crop_resample: 0 <= ns <= B smoothing slots need a workspace");
  int64_t V = 0;
  const int rc = aug_check_geometry("fz_aug_crop_resample", B, nd, D, H, W, &V);
  if (rc != FZ_OK) return rc;
  const int es = act_dtype == FZ_STORE_BF16 ? 2 : 4;
  if (!aug_aligned(sources, 8) || !aug_aligned(img_out, es) || !aug_aligned(table, 4) || !aug_aligned(seed, 8) ||
      !aug_aligned(smooth_ws, 4))
    return fail(FZ_E_ARG, "fz_aug_crop_resample: pointer not aligned to its element");
  const bool vec = W % 4 == 0 && aug_aligned(img_out, 4 * es) && aug_aligned(smooth_ws, 16) && aug_aligned(lab_out, 4);
  const int Wq = (W + 3) / 4, nq = D * H * Wq;
  const dim3 grid((unsigned)((nq + 255) / 256), C + L, B);
  hipStream_t s = (hipStream_t)stream;
  float* ws = ns > 0 ? smooth_ws : nullptr;
  if (act_dtype == FZ_STORE_BF16 && C > 0) {
    if (nd == 3) aug_crop_launch<bf16, 3>(vec, grid, s, sources, img_out, ws, ns, C, lab_out, L, table, seed, D, H, W, Wq, nq);
    else aug_crop_launch<bf16, 2>(vec, grid, s, sources, img_out, ws, ns, C, lab_out, L, table, seed, D, H, W, Wq, nq);
  } else {
    if (nd == 3) aug_crop_launch<float, 3>(vec, grid, s, sources, img_out, ws, ns, C, lab_out, L, table, seed, D, H, W, Wq, nq);
    else aug_crop_launch<float, 2>(vec, grid, s, sources, img_out, ws, ns, C, lab_out, L, table, seed, D, H, W, Wq, nq);
  }
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
