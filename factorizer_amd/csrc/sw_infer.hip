// sw_infer.hip — sliding-window inference stitching for 1-D, 2-D and 3-D images.
//
// The BraTS bundle runs the network through MONAI's SlidingWindowInfererAdapt(roi_size 128^3,
// sw_batch_size 2, overlap 0.5, mode "gaussian") (model_zoo/factorizer_brats23/configs/
// inference.yaml:96-102, train.yaml:206-212), the FIVES bundle through the same inferer with
// roi_size 512^2 on 2-D retina images (model_zoo/deconver_fives/configs/inference.yaml:77-83).
// MONAI (pinned monai>=1.3 by the bundle metadata) is not part of this project; its published
// algorithm (monai/inferers/utils.py sliding_window_inference + compute_importance_map) is restated here:
//   windows  = dense grid of roi-sized patches, interval = int(roi * (1 - overlap)), last window
//              shifted back so that it ends at the image border;
//   weights  = separable Gaussian, sigma = 0.125 * roi, centred on the patch, clamped from below
//              at max(min nonzero, 1e-3);
//   output   = Σ_w weights · net(window_w)  /  Σ_w weights.
// Three data movements, all HBM-bound and one launch each per window:
//   gather      window ← image[:, z0:z0+rd, y0:y0+rh, x0:x0+rw]
//   accumulate  out[:, window] += g · prob ; cnt[window] += g      (windows of one call overlap, so
//               they are accumulated by sequential launches: deterministic, no float atomics)
//   finalize    out /= cnt
// Geometry is always (C, D, H, W): a 2-D image is (C, 1, H, W), a 1-D one (C, 1, 1, L), with a unit
// Gaussian factor 1.0 on the added axes.  fz_sw_gather / _accumulate / _finalize are the original
// fp32, 3-D, rw % 4 == 0 entry points; the fz_sw_*2 set below takes any width and origin and fp32 or
// bf16 windows, and accumulates in fp32 whatever the storage type.
#include "fz_common.h"

namespace fz {

struct SwGeom {
  int C;           // channels of the moved tensor
  int D, H, W;     // volume
  int rd, rh, rw;  // window
  int z0, y0, x0;  // window origin
  int aligned;     // W % 4 == 0 && x0 % 4 == 0: 16-byte vectors on the volume side (fz_sw_gather / _accumulate only)
};

// volume-side access of 4 consecutive x: BraTS volumes are 240 x 240 x 155 and the last window of a
// row starts at 155 - 128 = 27, so the vector path cannot be assumed
__device__ __forceinline__ float4 vol_ld4(const float* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void vol_st4(float* p, float4 v, bool aligned) {
  if (aligned) { *reinterpret_cast<float4*>(p) = v; return; }
  p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}

// one thread per 4 consecutive x of the window (rw % 4 == 0 and x0 % 4 == 0 → 16-byte vectors)
__global__ __launch_bounds__(256) void sw_gather_kernel(const float* __restrict__ vol, float* __restrict__ win, SwGeom g) {
  const int64_t qw = g.rw / 4;
  const int64_t total = (int64_t)g.C * g.rd * g.rh * qw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xq = (int)(i % qw);
    int64_t t = i / qw;
    const int y = (int)(t % g.rh); t /= g.rh;
    const int z = (int)(t % g.rd);
    const int c = (int)(t / g.rd);
    const int64_t src = (((int64_t)c * g.D + g.z0 + z) * g.H + g.y0 + y) * g.W + g.x0 + xq * 4;
    *reinterpret_cast<float4*>(win + i * 4) = vol_ld4(vol + src, g.aligned != 0);
  }
}

// gz, gy, gx: the three 1-D factors of the (already clamped-from-below per product) weight map
__global__ __launch_bounds__(256) void sw_accumulate_kernel(const float* __restrict__ prob, float* __restrict__ out,
                                                            float* __restrict__ cnt, const float* __restrict__ gz,
                                                            const float* __restrict__ gy, const float* __restrict__ gx,
                                                            float wmin, SwGeom g) {
  const int64_t qw = g.rw / 4;
  const int64_t plane = (int64_t)g.rd * g.rh * qw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += (int64_t)gridDim.x * blockDim.x) {
    const int xq = (int)(i % qw);
    int64_t t = i / qw;
    const int y = (int)(t % g.rh);
    const int z = (int)(t / g.rh);
    const float wzy = gz[z] * gy[y];
    const float4 wx = *reinterpret_cast<const float4*>(gx + xq * 4);
    float4 w = make_float4(fmaxf(wzy * wx.x, wmin), fmaxf(wzy * wx.y, wmin), fmaxf(wzy * wx.z, wmin), fmaxf(wzy * wx.w, wmin));
    const int64_t dst = (((int64_t)g.z0 + z) * g.H + g.y0 + y) * g.W + g.x0 + xq * 4;
    const bool al = g.aligned != 0;
    float4 cv = vol_ld4(cnt + dst, al);
    cv.x += w.x; cv.y += w.y; cv.z += w.z; cv.w += w.w;
    vol_st4(cnt + dst, cv, al);
    const int64_t V = (int64_t)g.D * g.H * g.W;
    for (int c = 0; c < g.C; ++c) {
      const float4 p = *reinterpret_cast<const float4*>(prob + ((int64_t)c * plane + i) * 4);
      float4 o = vol_ld4(out + c * V + dst, al);
      o.x += w.x * p.x; o.y += w.y * p.y; o.z += w.z * p.z; o.w += w.w * p.w;
      vol_st4(out + c * V + dst, o, al);
    }
  }
}

__global__ __launch_bounds__(256) void sw_finalize_kernel(float* __restrict__ out, const float* __restrict__ cnt, int C,
                                                          int64_t V) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
    const float cv = cnt[i];
    for (int c = 0; c < C; ++c) out[(int64_t)c * V + i] /= cv;
  }
}

// ---- the fz_sw_*2 kernels: any width and origin, fp32 / bf16 storage ---------------------------------------------------
// Per element the same arithmetic as the kernels above — w = fmaxf((gz · gy) · gx, wmin), cnt += w, out += w · p, out / cnt —
// so a 3-D fp32 call returns the bits fz_sw_accumulate / fz_sw_finalize return, whichever body runs.  Every body gives a
// thread four consecutive x of one window row, so consecutive threads walk a row contiguously (coalesced; a FIVES row is
// 512 values) and the index arithmetic is paid once per four elements:
//   SW_VEC   rw, W and x0 multiples of 4, pointers 4-element aligned: 16-byte (fp32) / 8-byte (bf16) vectors on both sides;
//   SW_ROW4  rw a multiple of 4: vectors on the window side, four scalar accesses on the image side (the last window of a
//            240 x 240 x 155 BraTS row starts at x0 = 27; a 1298-wide image under a 512 roi ends at x0 = 786);
//   SW_TAIL  any rw: four scalar accesses on both sides, the last group of a row masked at rw.
enum { SW_TAIL = 0, SW_ROW4 = 1, SW_VEC = 2 };

// gather moves storage bits, not values: fp32 as 32-bit, bf16 as 16-bit words (byte-exact, NaN payloads included)
template <int ES> struct SwBits;
template <> struct SwBits<4> { typedef uint32_t e; typedef uint32_t v4 __attribute__((ext_vector_type(4))); };
template <> struct SwBits<2> { typedef uint16_t e; typedef uint16_t v4 __attribute__((ext_vector_type(4))); };

template <int ES, int MODE>
__global__ __launch_bounds__(256) void sw_gather2_kernel(const typename SwBits<ES>::e* __restrict__ img,
                                                         typename SwBits<ES>::e* __restrict__ win, SwGeom g) {
  typedef typename SwBits<ES>::v4 v4;
  const int64_t qw = (g.rw + 3) / 4;
  const int64_t total = (int64_t)g.C * g.rd * g.rh * qw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % qw) * 4;
    const int64_t row = i / qw;  // (c * rd + z) * rh + y
    const int y = (int)(row % g.rh);
    const int64_t t = row / g.rh;
    const int z = (int)(t % g.rd);
    const int c = (int)(t / g.rd);
    const auto* s = img + (((int64_t)c * g.D + g.z0 + z) * g.H + g.y0 + y) * g.W + g.x0 + x;
    auto* d = win + row * g.rw + x;
    if constexpr (MODE == SW_VEC) {
      *reinterpret_cast<v4*>(d) = *reinterpret_cast<const v4*>(s);
    } else if constexpr (MODE == SW_ROW4) {
      const v4 v = {s[0], s[1], s[2], s[3]};
      *reinterpret_cast<v4*>(d) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < g.rw) d[k] = s[k];
    }
  }
}

// prob (C, rd, rh, rw) in the storage type T; out (C, D, H, W) and cnt (D, H, W) fp32
template <typename T, int MODE>
__global__ __launch_bounds__(256) void sw_accumulate2_kernel(const T* __restrict__ prob, float* __restrict__ out,
                                                             float* __restrict__ cnt, const float* __restrict__ gz,
                                                             const float* __restrict__ gy, const float* __restrict__ gx,
                                                             float wmin, SwGeom g) {
  const int64_t qw = (g.rw + 3) / 4;
  const int64_t plane = (int64_t)g.rd * g.rh * g.rw;  // one channel of the window
  const int64_t V = (int64_t)g.D * g.H * g.W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)g.rd * g.rh * qw;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % qw) * 4;
    const int64_t row = i / qw;  // z * rh + y
    const int y = (int)(row % g.rh);
    const int z = (int)(row / g.rh);
    const float wzy = gz[z] * gy[y];
    const int64_t dst = (((int64_t)g.z0 + z) * g.H + g.y0 + y) * g.W + g.x0 + x;
    const int64_t src = row * g.rw + x;
    if constexpr (MODE == SW_TAIL) {
      const int n = min(4, g.rw - x);
      float w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < n) {
          w[k] = fmaxf(wzy * gx[x + k], wmin);
          cnt[dst + k] += w[k];
        }
      }
      for (int c = 0; c < g.C; ++c) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < n) out[c * V + dst + k] += w[k] * aget(prob + c * plane + src + k);
      }
    } else {
      const bool al = MODE == SW_VEC;
      const float4 wx = *reinterpret_cast<const float4*>(gx + x);
      const float4 w = make_float4(fmaxf(wzy * wx.x, wmin), fmaxf(wzy * wx.y, wmin), fmaxf(wzy * wx.z, wmin),
                                   fmaxf(wzy * wx.w, wmin));
      float4 cv = vol_ld4(cnt + dst, al);
      cv.x += w.x; cv.y += w.y; cv.z += w.z; cv.w += w.w;
      vol_st4(cnt + dst, cv, al);
      for (int c = 0; c < g.C; ++c) {
        const float4 p = ld4(prob + c * plane + src);
        float4 o = vol_ld4(out + c * V + dst, al);
        o.x += w.x * p.x; o.y += w.y * p.y; o.z += w.z * p.z; o.w += w.w * p.w;
        vol_st4(out + c * V + dst, o, al);
      }
    }
  }
}

// res = out / cnt, rounded once to T; res may be out itself (fp32 in place), hence no __restrict__ on the two
template <typename T>
__global__ __launch_bounds__(256) void sw_finalize2_kernel(const float* out, const float* __restrict__ cnt, T* res, int C,
                                                           int64_t V) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
    const float cv = cnt[i];
    for (int c = 0; c < C; ++c) aput(res + (int64_t)c * V + i, out[(int64_t)c * V + i] / cv);
  }
}

static int sw_check_geom(int C, int D, int H, int W, int rd, int rh, int rw, int z0, int y0, int x0) {
  if (C < 1 || D < 1 || H < 1 || W < 1 || rd < 1 || rh < 1 || rw < 1) return fail(FZ_E_SHAPE, "fz_sw: sizes must be positive");
  if (z0 < 0 || y0 < 0 || x0 < 0 || z0 + rd > D || y0 + rh > H || x0 + rw > W)
    return fail(FZ_E_SHAPE, "fz_sw: window outside the volume");
  return FZ_OK;
}

static int sw_check(const char* who, int C, int D, int H, int W, int rd, int rh, int rw, int z0, int y0, int x0) {
  int rc = sw_check_geom(C, D, H, W, rd, rh, rw, z0, y0, x0);
  if (rc != FZ_OK) return rc;
  if (rw % 4) return fail(FZ_E_UNSUPPORTED, "fz_sw: window width must be a multiple of 4");
  (void)who;
  return FZ_OK;
}

static bool sw_store_ok(int act_dtype) { return act_dtype == FZ_STORE_F32 || act_dtype == FZ_STORE_BF16; }

static bool sw_aligned(const void* p, int bytes) { return ((uintptr_t)p % (uintptr_t)bytes) == 0; }

// which body a call takes: SW_VEC needs 4-element alignment of the image-side pointers (img, or out and cnt) and of the
// window-side ones (win, or prob and gx), SW_ROW4 of the window-side ones
static int sw_mode(const SwGeom& g, bool image_side_aligned, bool window_side_aligned) {
  if (g.rw % 4 || !window_side_aligned) return SW_TAIL;
  return (g.W % 4 == 0 && g.x0 % 4 == 0 && image_side_aligned) ? SW_VEC : SW_ROW4;
}

static unsigned sw_grid(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b > 256 * 16) b = 256 * 16;
  return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace fz

using namespace fz;

extern "C" int fz_sw_gather(const float* vol, float* win, int C, int D, int H, int W, int rd, int rh, int rw, int z0,
                            int y0, int x0, fz_stream_t stream) {
  if (!vol || !win) return fail(FZ_E_ARG, "fz_sw_gather: null pointer");
  int rc = sw_check("gather", C, D, H, W, rd, rh, rw, z0, y0, x0);
  if (rc != FZ_OK) return rc;
  SwGeom g{C, D, H, W, rd, rh, rw, z0, y0, x0, ((W % 4) == 0 && (x0 % 4) == 0) ? 1 : 0};
  hipLaunchKernelGGL(sw_gather_kernel, dim3(sw_grid((int64_t)C * rd * rh * rw / 4)), dim3(256), 0, (hipStream_t)stream,
                     vol, win, g);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_sw_accumulate(const float* prob, float* out, float* cnt, const float* gz, const float* gy,
                                const float* gx, float wmin, int C, int D, int H, int W, int rd, int rh, int rw,
                                int z0, int y0, int x0, fz_stream_t stream) {
  if (!prob || !out || !cnt || !gz || !gy || !gx) return fail(FZ_E_ARG, "fz_sw_accumulate: null pointer");
  int rc = sw_check("accumulate", C, D, H, W, rd, rh, rw, z0, y0, x0);
  if (rc != FZ_OK) return rc;
  SwGeom g{C, D, H, W, rd, rh, rw, z0, y0, x0, ((W % 4) == 0 && (x0 % 4) == 0) ? 1 : 0};
  hipLaunchKernelGGL(sw_accumulate_kernel, dim3(sw_grid((int64_t)rd * rh * rw / 4)), dim3(256), 0, (hipStream_t)stream,
                     prob, out, cnt, gz, gy, gx, wmin, g);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_sw_finalize(float* out, const float* cnt, int C, int64_t V, fz_stream_t stream) {
  if (!out || !cnt) return fail(FZ_E_ARG, "fz_sw_finalize: null pointer");
  if (C < 1 || V < 1) return fail(FZ_E_SHAPE, "fz_sw_finalize: sizes must be positive");
  hipLaunchKernelGGL(sw_finalize_kernel, dim3(sw_grid(V)), dim3(256), 0, (hipStream_t)stream, out, cnt, C, V);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

template <int ES>
static void sw_gather2_launch(int mode, const void* img, void* win, const SwGeom& g, hipStream_t s) {
  typedef typename SwBits<ES>::e e;
  const dim3 grid(sw_grid((int64_t)g.C * g.rd * g.rh * ((g.rw + 3) / 4))), block(256);
  const e* a = (const e*)img;
  e* b = (e*)win;
  if (mode == SW_VEC) hipLaunchKernelGGL((sw_gather2_kernel<ES, SW_VEC>), grid, block, 0, s, a, b, g);
  else if (mode == SW_ROW4) hipLaunchKernelGGL((sw_gather2_kernel<ES, SW_ROW4>), grid, block, 0, s, a, b, g);
  else hipLaunchKernelGGL((sw_gather2_kernel<ES, SW_TAIL>), grid, block, 0, s, a, b, g);
}

template <typename T>
static void sw_accumulate2_launch(int mode, const void* prob, float* out, float* cnt, const float* gz, const float* gy,
                                  const float* gx, float wmin, const SwGeom& g, hipStream_t s) {
  const dim3 grid(sw_grid((int64_t)g.rd * g.rh * ((g.rw + 3) / 4))), block(256);
  const T* p = (const T*)prob;
  if (mode == SW_VEC)
    hipLaunchKernelGGL((sw_accumulate2_kernel<T, SW_VEC>), grid, block, 0, s, p, out, cnt, gz, gy, gx, wmin, g);
  else if (mode == SW_ROW4)
    hipLaunchKernelGGL((sw_accumulate2_kernel<T, SW_ROW4>), grid, block, 0, s, p, out, cnt, gz, gy, gx, wmin, g);
  else
    hipLaunchKernelGGL((sw_accumulate2_kernel<T, SW_TAIL>), grid, block, 0, s, p, out, cnt, gz, gy, gx, wmin, g);
}

extern "C" int fz_sw_gather2(const void* img, void* win, int C, int D, int H, int W, int rd, int rh, int rw, int z0, int y0,
                             int x0, int act_dtype, fz_stream_t stream) {
  if (!img || !win) return fail(FZ_E_ARG, "fz_sw_gather2: null pointer");
  if (!sw_store_ok(act_dtype)) return fail(FZ_E_ARG, "fz_sw_gather2: bad act_dtype");
  int rc = sw_check_geom(C, D, H, W, rd, rh, rw, z0, y0, x0);
  if (rc != FZ_OK) return rc;
  const SwGeom g{C, D, H, W, rd, rh, rw, z0, y0, x0, 0};
  const int es = act_dtype == FZ_STORE_BF16 ? 2 : 4;
  const int mode = sw_mode(g, sw_aligned(img, 4 * es), sw_aligned(win, 4 * es));
  if (es == 4) sw_gather2_launch<4>(mode, img, win, g, (hipStream_t)stream);
  else sw_gather2_launch<2>(mode, img, win, g, (hipStream_t)stream);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_sw_accumulate2(const void* prob, float* out, float* cnt, const float* gz, const float* gy, const float* gx,
                                 float wmin, int C, int D, int H, int W, int rd, int rh, int rw, int z0, int y0, int x0,
                                 int act_dtype, fz_stream_t stream) {
  if (!prob || !out || !cnt || !gz || !gy || !gx) return fail(FZ_E_ARG, "fz_sw_accumulate2: null pointer");
  if (!sw_store_ok(act_dtype)) return fail(FZ_E_ARG, "fz_sw_accumulate2: bad act_dtype");
  int rc = sw_check_geom(C, D, H, W, rd, rh, rw, z0, y0, x0);
  if (rc != FZ_OK) return rc;
  const SwGeom g{C, D, H, W, rd, rh, rw, z0, y0, x0, 0};
  const int es = act_dtype == FZ_STORE_BF16 ? 2 : 4;
  const int mode = sw_mode(g, sw_aligned(out, 16) && sw_aligned(cnt, 16), sw_aligned(prob, 4 * es) && sw_aligned(gx, 16));
  if (es == 4) sw_accumulate2_launch<float>(mode, prob, out, cnt, gz, gy, gx, wmin, g, (hipStream_t)stream);
  else sw_accumulate2_launch<bf16>(mode, prob, out, cnt, gz, gy, gx, wmin, g, (hipStream_t)stream);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_sw_finalize2(const float* out, const float* cnt, void* res, int C, int64_t V, int act_dtype,
                               fz_stream_t stream) {
  if (!out || !cnt || !res) return fail(FZ_E_ARG, "fz_sw_finalize2: null pointer");
  if (!sw_store_ok(act_dtype)) return fail(FZ_E_ARG, "fz_sw_finalize2: bad act_dtype");
  if (C < 1 || V < 1) return fail(FZ_E_SHAPE, "fz_sw_finalize2: sizes must be positive");
  if (act_dtype == FZ_STORE_BF16 && res == (const void*)out)
    return fail(FZ_E_ARG, "fz_sw_finalize2: a bf16 result needs its own tensor");
  hipStream_t s = (hipStream_t)stream;
  if (act_dtype == FZ_STORE_F32)
    hipLaunchKernelGGL(sw_finalize2_kernel<float>, dim3(sw_grid(V)), dim3(256), 0, s, out, cnt, (float*)res, C, V);
  else
    hipLaunchKernelGGL(sw_finalize2_kernel<bf16>, dim3(sw_grid(V)), dim3(256), 0, s, out, cnt, (bf16*)res, C, V);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
