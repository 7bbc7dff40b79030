// augment.hip — the recipe's random training augmentations on device (factorizer_amd/augment.py restates the
// semantics).  `random_transforms` of every bundle (model_zoo/factorizer_brats23/configs/train.yaml): RandAffined,
// RandGaussianNoised, RandGaussianSmoothd, RandScaleIntensityd, RandShiftIntensityd and one RandFlipd per axis, applied to a
// whole batch (B, C, *S) + label (B, L, *S) that already sits in HBM.  Three kernels:
//   aug_resample   ONE launch for every plane of the batch (grid: voxel quads x (C + L) planes x B samples).  Output voxel o
//                  reads the source position p = A (o' - c) + c (o' = o mirrored on the flipped axes, c the centre), clamped
//                  to the image (border padding): image planes interpolate (bi/tri)linearly in fp32, label planes take the
//                  voxel at floor(p + 0.5).  A sample whose A is exactly the identity takes a path without interpolation
//                  arithmetic — a copy or a mirrored copy, bit for bit, 16-byte vectors where W % 4 == 0.  Noise
//                  (std · Philox / Box-Muller normal of the OUTPUT voxel) and, for samples that do not smooth, gain / offset
//                  ride in the same launch.  Samples that smooth are written as fp32 into their slot of a compact workspace
//                  instead (bf16 images are rounded once, after the smoothing).  In-plane offsets are 32-bit (a plane holds
//                  fewer than 2^31 voxels); the 64-bit plane base is uniform per workgroup.
//   aug_smooth     for the samples of a device index list only: separable 9-tap convolution with zero padding, then gain /
//                  offset, ONE launch: a workgroup stages an output tile plus its 4-voxel halo in LDS and runs the nd passes
//                  there (3-D: 8 x 8 x 16 outputs, 16 x 16 x 24 staged; 2-D: 32 x 32 outputs, 40 x 40 staged).
//   aug_noise      the normal field alone (ft.gaussian_noise_field: what the tests hand to the reference).
// No atomics; every output voxel has one writer, so equal parameters and seed give bitwise equal tensors.
// The device functions of the gather and its epilogue live in aug_device.h: aug_crop.hip (the random crop cut inside the gather)
// calls the same ones.
#include "aug_device.h"

namespace fz {

// VEC: W % 4 == 0 and every tensor base aligned to four elements, so a lane's four x are one vector on both sides.
template <typename AT, int ND, bool VEC>
__global__ __launch_bounds__(256) void aug_resample_kernel(const AT* __restrict__ img, AT* __restrict__ out, float* __restrict__ ws,
                                                           int ns, int C, const uint8_t* __restrict__ lab,
                                                           uint8_t* __restrict__ lab_out, int L, const float* __restrict__ table,
                                                           const int64_t* __restrict__ seed, int D, int H, int W, int Wq, int nq) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const int b = blockIdx.z, pl = blockIdx.y;
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
  const int srow = (oz * H + oy) * W;        // identity: the source row

  if (pl >= C) {   // ---- label plane: nearest
    const int64_t base = ((int64_t)b * L + (pl - C)) * V;
    const uint8_t* src = lab + base;
    uint8_t* dst = lab_out + base;
    if (VEC && ident) {
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
        const int si = ident ? srow + ox : aug_nearest<ND>(aug_source<ND>(A, oz, oy, ox, D, H, W), H, W);
        const uint32_t v = src[si];
        if (VEC) w |= v << (8 * e);
        else dst[o + e] = (uint8_t)v;
      }
    }
    if (VEC) *reinterpret_cast<uint32_t*>(dst + o) = w;
    return;
  }

  // ---- image plane
  const int64_t base = ((int64_t)b * C + pl) * V;
  const AT* src = img + base;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (ident) {
    if (VEC) {
      float t[4];
      aload<4>(src + srow + (flx ? W - 4 - x4 : x4), t);
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
        v[e] = aug_linear<AT, ND>(src, aug_source<ND>(A, oz, oy, ox, D, H, W), D, H, W, H, W);
      }
    }
  }
  aug_finish<AT, VEC>(v, n, o, pl, b, rec, seed, ws, ns, C, V, out);
}

// ---- smoothing ------------------------------------------------------------------------------------------------------------
// src (ns, C, D, H, W) fp32: slot i holds sample list[i].  Tile TZ x TY x TX outputs, halo HZ / 4 / 4 (HZ = 0: 2-D image).
template <typename AT, int TZ, int HZ, int TY, int TX>
__global__ __launch_bounds__(256) void aug_smooth_kernel(const float* __restrict__ src, AT* __restrict__ out, int C,
                                                         const float* __restrict__ table, const int32_t* __restrict__ list, int B,
                                                         int D, int H, int W, int ntx, int nty) {
  constexpr int AZ = TZ + 2 * HZ, AY = TY + 8, AX = TX + 8;
  __shared__ float bufA[AZ * AY * AX];   // staged input; later the y-pass output [AZ][TY][TX]
  __shared__ float bufB[AZ * AY * TX];   // x-pass output
  const int slot = blockIdx.z, c = blockIdx.y, tid = threadIdx.x;
  const int b = list[slot];
  if (b < 0 || b >= B) return;           // uniform: a bad list entry writes nothing
  const float* rec = table + (int64_t)b * AUG_REC;
  int t = blockIdx.x;
  const int x0 = (t % ntx) * TX;
  t /= ntx;
  const int y0 = (t % nty) * TY, z0 = (t / nty) * TZ;
  const int V = D * H * W;
  const float* s = src + ((int64_t)slot * C + c) * V;

  for (int i = tid; i < AZ * AY * AX; i += 256) {
    const int lx = i % AX, ly = (i / AX) % AY, lz = i / (AX * AY);
    const int gx = x0 + lx - 4, gy = y0 + ly - 4, gz = z0 + lz - HZ;
    const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H && gz >= 0 && gz < D;
    bufA[i] = in ? s[(gz * H + gy) * W + gx] : 0.f;   // zero padding
  }
  __syncthreads();

  float w[9];
  // x pass: A[lz][ly][x .. x + 8] -> B[lz][ly][x]
  const bool onx = rec[AUG_TAIL + 2] > 0.f;
#pragma unroll
  for (int j = 0; j < 9; ++j) w[j] = rec[AUG_TAPS + 18 + j];
  for (int i = tid; i < AZ * AY * TX; i += 256) {
    const int lx = i % TX, r = i / TX;
    const float* a = bufA + r * AX + lx;
    float acc = a[4];
    if (onx) {
      acc = w[0] * a[0];
#pragma unroll
      for (int j = 1; j < 9; ++j) acc = __builtin_fmaf(w[j], a[j], acc);
    }
    bufB[i] = acc;
  }
  __syncthreads();
  // y pass: B[lz][y .. y + 8][x] -> A'[lz][y][x]
  const bool ony = rec[AUG_TAIL + 1] > 0.f;
#pragma unroll
  for (int j = 0; j < 9; ++j) w[j] = rec[AUG_TAPS + 9 + j];
  for (int i = tid; i < AZ * TY * TX; i += 256) {
    const int lx = i % TX, ly = (i / TX) % TY, lz = i / (TX * TY);
    const float* a = bufB + (lz * AY + ly) * TX + lx;
    float acc = a[4 * TX];
    if (ony) {
      acc = w[0] * a[0];
#pragma unroll
      for (int j = 1; j < 9; ++j) acc = __builtin_fmaf(w[j], a[j * TX], acc);
    }
    bufA[i] = acc;
  }
  __syncthreads();
  // z pass (3-D only), gain / offset, store
  const bool onz = HZ > 0 && rec[AUG_TAIL] > 0.f;
#pragma unroll
  for (int j = 0; j < 9; ++j) w[j] = rec[AUG_TAPS + j];
  const float gain = rec[AUG_GAIN], off = rec[AUG_OFF];
  AT* dst = out + ((int64_t)b * C + c) * V;
  for (int i = tid; i < TZ * TY * TX; i += 256) {
    const int lx = i % TX, ly = (i / TX) % TY, lz = i / (TX * TY);
    const float* a = bufA + (lz * TY + ly) * TX + lx;
    float acc = a[HZ * TY * TX];
    if (onz) {
      acc = w[0] * a[0];
#pragma unroll
      for (int j = 1; j < 9; ++j) acc = __builtin_fmaf(w[j], a[(HZ ? j : 0) * TY * TX], acc);
    }
    acc = __builtin_fmaf(acc, gain, off);
    const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
    if (gx < W && gy < H && gz < D) aput(dst + (gz * H + gy) * W + gx, acc);
  }
}

// ---- noise field ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aug_noise_kernel(float* __restrict__ out, const int64_t* __restrict__ seed, int C, int64_t V,
                                                        int64_t nq) {
  const uint64_t s = (uint64_t)*seed;
  const uint32_t k0 = (uint32_t)s, k1 = (uint32_t)(s >> 32);
  const int c = blockIdx.y, b = blockIdx.z;
  float* dst = out + ((int64_t)b * C + c) * V;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
    float z[4];
    aug_normals4((uint32_t)q, (uint32_t)c, (uint32_t)b, k0, k1, z);
    const int64_t v = q * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (v + e < V) dst[v + e] = z[e];
  }
}

template <typename AT, int ND>
static void aug_resample_launch(bool vec, dim3 grid, hipStream_t s, const void* img, void* out, float* ws, int ns, int C,
                                const uint8_t* lab, uint8_t* lab_out, int L, const float* table, const int64_t* seed, int D, int H,
                                int W, int Wq, int nq) {
  if (vec)
    hipLaunchKernelGGL((aug_resample_kernel<AT, ND, true>), grid, dim3(256), 0, s, (const AT*)img, (AT*)out, ws, ns, C, lab, lab_out,
                       L, table, seed, D, H, W, Wq, nq);
  else
    hipLaunchKernelGGL((aug_resample_kernel<AT, ND, false>), grid, dim3(256), 0, s, (const AT*)img, (AT*)out, ws, ns, C, lab, lab_out,
                       L, table, seed, D, H, W, Wq, nq);
}

template <typename AT>
static void aug_smooth_launch(int nd, hipStream_t s, const float* src, void* out, int C, const float* table, const int32_t* list,
                              int ns, int B, int D, int H, int W) {
  if (nd == 3) {
    const int ntx = (W + 15) / 16, nty = (H + 7) / 8, ntz = (D + 7) / 8;
    hipLaunchKernelGGL((aug_smooth_kernel<AT, 8, 4, 8, 16>), dim3((unsigned)(ntx * nty * ntz), C, ns), dim3(256), 0, s, src, (AT*)out,
                       C, table, list, B, D, H, W, ntx, nty);
  } else {
    const int ntx = (W + 31) / 32, nty = (H + 31) / 32;
    hipLaunchKernelGGL((aug_smooth_kernel<AT, 1, 0, 32, 32>), dim3((unsigned)(ntx * nty), C, ns), dim3(256), 0, s, src, (AT*)out, C,
                       table, list, B, D, H, W, ntx, nty);
  }
}

}  // namespace fz

using namespace fz;

extern "C" int fz_aug_record_floats(void) { return AUG_REC; }

extern "C" int fz_aug_resample(const void* img, void* img_out, int act_dtype, int C, const uint8_t* lab, uint8_t* lab_out, int L,
                               const float* table, const int64_t* seed, float* smooth_ws, int ns, int B, int nd, int D, int H, int W,
                               fz_stream_t stream) {
  if (!table) return fail(FZ_E_ARG, "fz_aug_resample: null table");
  if (C < 0 || L < 0 || C + L < 1 || C + L > 65535) return fail(FZ_E_SHAPE, "fz_aug_resample: 1 <= C + L <= 65535 planes per sample");
  if ((C > 0 && (!img || !img_out)) || (L > 0 && (!lab || !lab_out))) return fail(FZ_E_ARG, "fz_aug_resample: null pointer");
  if ((C > 0 && img == img_out) || (L > 0 && lab == lab_out)) return fail(FZ_E_ARG, "fz_aug_resample: the output must not alias the input");
  if (C > 0 && act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16) return fail(FZ_E_ARG, "fz_aug_resample: bad act_dtype");
  if (ns < 0 || ns > B || (ns > 0 && !smooth_ws)) return fail(FZ_E_ARG, "fz_aug_resample: 0 <= ns <= B smoothing slots need a workspace");
  int64_t V = 0;
  const int rc = aug_check_geometry("fz_aug_resample", B, nd, D, H, W, &V);
  if (rc != FZ_OK) return rc;
  const int es = act_dtype == FZ_STORE_BF16 ? 2 : 4;
  if (!aug_aligned(img, es) || !aug_aligned(img_out, es) || !aug_aligned(table, 4) || !aug_aligned(seed, 8) || !aug_aligned(smooth_ws, 4))
    return fail(FZ_E_ARG, "fz_aug_resample: pointer not aligned to its element");
  const bool vec = W % 4 == 0 && aug_aligned(img, 4 * es) && aug_aligned(img_out, 4 * es) && aug_aligned(smooth_ws, 16) &&
                   aug_aligned(lab, 4) && aug_aligned(lab_out, 4);
  const int Wq = (W + 3) / 4, nq = D * H * Wq;
  const dim3 grid((unsigned)((nq + 255) / 256), C + L, B);
  hipStream_t s = (hipStream_t)stream;
  float* ws = ns > 0 ? smooth_ws : nullptr;
  if (act_dtype == FZ_STORE_BF16 && C > 0) {
    if (nd == 3) aug_resample_launch<bf16, 3>(vec, grid, s, img, img_out, ws, ns, C, lab, lab_out, L, table, seed, D, H, W, Wq, nq);
    else aug_resample_launch<bf16, 2>(vec, grid, s, img, img_out, ws, ns, C, lab, lab_out, L, table, seed, D, H, W, Wq, nq);
  } else {
    if (nd == 3) aug_resample_launch<float, 3>(vec, grid, s, img, img_out, ws, ns, C, lab, lab_out, L, table, seed, D, H, W, Wq, nq);
    else aug_resample_launch<float, 2>(vec, grid, s, img, img_out, ws, ns, C, lab, lab_out, L, table, seed, D, H, W, Wq, nq);
  }
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_aug_smooth(const float* smooth_ws, void* img_out, int act_dtype, int C, const float* table, const int32_t* list,
                             int ns, int B, int nd, int D, int H, int W, fz_stream_t stream) {
  if (!table || !img_out) return fail(FZ_E_ARG, "fz_aug_smooth: null pointer");
  if (act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16) return fail(FZ_E_ARG, "fz_aug_smooth: bad act_dtype");
  if (C < 1 || C > 65535) return fail(FZ_E_SHAPE, "fz_aug_smooth: 1 <= C <= 65535");
  int64_t V = 0;
  const int rc = aug_check_geometry("fz_aug_smooth", B, nd, D, H, W, &V);
  if (rc != FZ_OK) return rc;
  if (ns < 0 || ns > B) return fail(FZ_E_ARG, "fz_aug_smooth: 0 <= ns <= B");
  if (ns == 0) return FZ_OK;   // no sample drew smoothing: nothing is launched
  if (!smooth_ws || !list) return fail(FZ_E_ARG, "fz_aug_smooth: null pointer");
  if (!aug_aligned(smooth_ws, 4) || !aug_aligned(list, 4) || !aug_aligned(table, 4) || !aug_aligned(img_out, act_dtype == FZ_STORE_BF16 ? 2 : 4))
    return fail(FZ_E_ARG, "fz_aug_smooth: pointer not aligned to its element");
  hipStream_t s = (hipStream_t)stream;
  if (act_dtype == FZ_STORE_BF16) aug_smooth_launch<bf16>(nd, s, smooth_ws, img_out, C, table, list, ns, B, D, H, W);
  else aug_smooth_launch<float>(nd, s, smooth_ws, img_out, C, table, list, ns, B, D, H, W);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_aug_noise_field(float* out, const int64_t* seed, int B, int C, int64_t V, fz_stream_t stream) {
  if (!out || !seed) return fail(FZ_E_ARG, "fz_aug_noise_field: null pointer");
  if (B < 1 || B > 65535 || C < 1 || C > 65535 || V < 1) return fail(FZ_E_SHAPE, "fz_aug_noise_field: 1 <= B, C <= 65535, V >= 1");
  if ((V >> 2) > 0xffffffffLL) return fail(FZ_E_SHAPE, "fz_aug_noise_field: more than 2^34 voxels per plane");
  if (!aug_aligned(out, 4) || !aug_aligned(seed, 8)) return fail(FZ_E_ARG, "fz_aug_noise_field: pointer not aligned to its element");
  const int64_t nq = (V + 3) / 4;
  int64_t blocks = (nq + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(aug_noise_kernel, dim3((unsigned)blocks, C, B), dim3(256), 0, (hipStream_t)stream, out, seed, C, V, nq);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
