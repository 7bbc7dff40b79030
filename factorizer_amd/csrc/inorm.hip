// inorm.hip — instance norm of channels-first activations, forward and backward (semantics:
// factorizer_amd/instance_norm.py).  The block norm of the Deconver bundles (deconver.py norm1 / norm2 / Stem with
// norm: nn.InstanceNorm3d / nn.InstanceNorm2d).
//
// (B, C, *S) is P = B·C contiguous planes of V elements; the kernels do not care about the rank.  Storage fp32 or bf16,
// parameters fp32, every sum and every element in float64, one rounding per stored element (inorm_core.h, which also fixes
// the chunk plan, the visiting order and the order of every reduction).  No atomics: a plane's result depends on nothing but
// the plane.
//   V <= INORM_ONE_PASS_MAX   one launch each way, one workgroup per plane: the plane (backward: the plane of x and of g) is
//                             read once into registers, reduced, and written from there.
//   larger planes             two launches each way over a 1-D grid of (plane, chunk) workgroups: a partials launch writes two
//                             float64 sums per workgroup; the apply launch first re-reduces its plane's partials in a fixed
//                             order (as vol_write does), then writes its chunk.  The apply launch walks the grid in the
//                             opposite direction: it starts on what the partials launch read last and the Infinity Cache
//                             still holds.
//   affine                    the backward leaves two float64 totals per plane; one more small launch sums them over the batch
//                             index in order, one thread per channel.
#include "fz_common.h"
#include "inorm_core.h"
#include "inorm_device.h"

namespace fz {

// ---- one launch: the plane stays in registers ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(INORM_THREADS) void inorm_fwd1_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, T* __restrict__ y,
                                                                   double* __restrict__ stats, int C, int V, double eps) {
  constexpr int W = 16 / (int)sizeof(T), NG = INORM_REG / W;
  __shared__ double red[2][INORM_THREADS];
  const int t = threadIdx.x;
  const int64_t plane = blockIdx.x;
  const T* xp = x + plane * V;
  T* yp = y + plane * V;
  const bool vx = inorm_vec(xp), vy = inorm_vec(yp);
  const double x0 = (double)aget(xp);
  float v[NG][W];
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int n = 0; n < NG; ++n) {
    const int i0 = (n * INORM_THREADS + t) * W;
    if (i0 < V) {
      inorm_load<T, W>(xp, i0, V, vx, v[n]);
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (i0 + k < V) inorm_acc_stat(s1, s2, v[n][k], x0);
    }
  }
  inorm_block_sum2(s1, s2, red);
  const InormStat st = inorm_finish_stat(s1, s2, x0, V, eps);
  if (t == 0) {
    stats[plane * 2] = st.mean;
    stats[plane * 2 + 1] = st.rstd;
  }
  const int c = (int)(plane % C);
  const double ga = gamma ? (double)gamma[c] : 1.0, be = beta ? (double)beta[c] : 0.0;
#pragma unroll
  for (int n = 0; n < NG; ++n) {
    const int i0 = (n * INORM_THREADS + t) * W;
    if (i0 < V) {
      double r[W];
#pragma unroll
      for (int k = 0; k < W; ++k) r[k] = inorm_y(v[n][k], st.mean, st.rstd, ga, be);
      inorm_store(yp, i0, V, vy, r);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(INORM_THREADS) void inorm_bwd1_kernel(const T* __restrict__ x, const T* __restrict__ g,
                                                                   const float* __restrict__ gamma,
                                                                   const double* __restrict__ stats, T* __restrict__ gx,
                                                                   double* __restrict__ totals, int C, int V) {
  constexpr int W = 16 / (int)sizeof(T), NG = INORM_REG / W;
  __shared__ double red[2][INORM_THREADS];
  const int t = threadIdx.x;
  const int64_t plane = blockIdx.x;
  const T* xp = x + plane * V;
  const T* gp = g + plane * V;
  T* op = gx + plane * V;
  const bool vx = inorm_vec(xp), vg = inorm_vec(gp), vo = inorm_vec(op);
  const double mean = stats[plane * 2], rstd = stats[plane * 2 + 1];
  float xv[NG][W], gv[NG][W];
  double sg = 0.0, sgx = 0.0;
#pragma unroll
  for (int n = 0; n < NG; ++n) {
    const int i0 = (n * INORM_THREADS + t) * W;
    if (i0 < V) {
      inorm_load<T, W>(xp, i0, V, vx, xv[n]);
      inorm_load<T, W>(gp, i0, V, vg, gv[n]);
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (i0 + k < V) inorm_acc_grad(sg, sgx, gv[n][k], xv[n][k], mean, rstd);
    }
  }
  inorm_block_sum2(sg, sgx, red);
  if (t == 0) {
    totals[plane * 2] = sg;
    totals[plane * 2 + 1] = sgx;
  }
  const double ga = gamma ? (double)gamma[plane % C] : 1.0;
  const double a = ga * sg / (double)V, b = ga * sgx / (double)V;
#pragma unroll
  for (int n = 0; n < NG; ++n) {
    const int i0 = (n * INORM_THREADS + t) * W;
    if (i0 < V) {
      double r[W];
#pragma unroll
      for (int k = 0; k < W; ++k) r[k] = inorm_gx(gv[n][k], xv[n][k], mean, rstd, ga, a, b);
      inorm_store(op, i0, V, vo, r);
    }
  }
}

// ---- two launches: (plane, chunk) workgroups ----------------------------------------------------------------------------
// BWD = false: sums of d, d^2 about the plane's first element; BWD = true: sums of g, g x̂
template <typename T, bool BWD>
__global__ __launch_bounds__(INORM_THREADS) void inorm_partials_kernel(const T* __restrict__ x, const T* __restrict__ g,
                                                                       const double* __restrict__ stats, int64_t V, int nchunk,
                                                                       double* __restrict__ part) {
  constexpr int W = 16 / (int)sizeof(T);
  __shared__ double red[2][INORM_THREADS];
  const int t = threadIdx.x;
  const int64_t idx = blockIdx.x, plane = idx / nchunk;
  const InormSpan sp = inorm_chunk(V, (int)(idx - plane * nchunk));
  const T* xp = x + plane * V;
  const T* gp = BWD ? g + plane * V : nullptr;
  const bool vx = inorm_vec(xp), vg = BWD && inorm_vec(gp);
  const double p0 = BWD ? stats[plane * 2] : (double)aget(xp), p1 = BWD ? stats[plane * 2 + 1] : 0.0;
  double s1 = 0.0, s2 = 0.0;
  const int64_t ng = inorm_groups(sp, W);
#pragma unroll 2
  for (int64_t j = t; j < ng; j += INORM_THREADS) {
    const int64_t i0 = sp.lo + j * W;
    float xv[W], gv[W];
    inorm_load<T, W>(xp, i0, sp.hi, vx, xv);
    if constexpr (BWD) inorm_load<T, W>(gp, i0, sp.hi, vg, gv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      if (i0 + k < sp.hi) {
        if constexpr (BWD) inorm_acc_grad(s1, s2, gv[k], xv[k], p0, p1);
        else inorm_acc_stat(s1, s2, xv[k], p0);
      }
    }
  }
  inorm_block_sum2(s1, s2, red);
  if (t == 0) {
    part[idx * 2] = s1;
    part[idx * 2 + 1] = s2;
  }
}

template <typename T, bool BWD>
__global__ __launch_bounds__(INORM_THREADS) void inorm_apply_kernel(const T* __restrict__ x, const T* __restrict__ g,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, T* __restrict__ out,
                                                                    double* __restrict__ stats, double* __restrict__ totals,
                                                                    const double* __restrict__ part, int C, int64_t V, int nchunk,
                                                                    double eps) {
  constexpr int W = 16 / (int)sizeof(T);
  __shared__ double red[2][INORM_THREADS];
  const int t = threadIdx.x;
  // descending, against the partials launch: measured 3.5 - 4 % faster at the C = 32 stages in fp32 (profiles/instance_norm.md)
  const int64_t idx = (int64_t)gridDim.x - 1 - blockIdx.x, plane = idx / nchunk;
  const int chunk = (int)(idx - plane * nchunk);
  const InormSpan sp = inorm_chunk(V, chunk);
  const T* xp = x + plane * V;
  const T* gp = BWD ? g + plane * V : nullptr;
  T* op = out + plane * V;
  const bool vx = inorm_vec(xp), vg = BWD && inorm_vec(gp), vo = inorm_vec(op);
  // the plane's totals from its partials, in the order every workgroup and every run uses
  const double* pp = part + plane * nchunk * 2;
  double s1 = inorm_partial_share(pp, nchunk, 2, t), s2 = inorm_partial_share(pp + 1, nchunk, 2, t);
  inorm_block_sum2(s1, s2, red);
  const int c = (int)(plane % C);
  const double ga = gamma ? (double)gamma[c] : 1.0;
  double mean, rstd, a = 0.0, b = 0.0, be = 0.0;
  if constexpr (BWD) {
    mean = stats[plane * 2];
    rstd = stats[plane * 2 + 1];
    a = ga * s1 / (double)V;
    b = ga * s2 / (double)V;
    if (chunk == 0 && t == 0) {
      totals[plane * 2] = s1;
      totals[plane * 2 + 1] = s2;
    }
  } else {
    const InormStat st = inorm_finish_stat(s1, s2, (double)aget(xp), V, eps);
    mean = st.mean;
    rstd = st.rstd;
    be = beta ? (double)beta[c] : 0.0;
    if (chunk == 0 && t == 0) {
      stats[plane * 2] = mean;
      stats[plane * 2 + 1] = rstd;
    }
  }
  const int64_t ng = inorm_groups(sp, W);
#pragma unroll 2
  for (int64_t j = t; j < ng; j += INORM_THREADS) {
    const int64_t i0 = sp.lo + j * W;
    float xv[W], gv[W];
    double r[W];
    inorm_load<T, W>(xp, i0, sp.hi, vx, xv);
    if constexpr (BWD) inorm_load<T, W>(gp, i0, sp.hi, vg, gv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      if constexpr (BWD) r[k] = inorm_gx(gv[k], xv[k], mean, rstd, ga, a, b);
      else r[k] = inorm_y(xv[k], mean, rstd, ga, be);
    }
    inorm_store(op, i0, sp.hi, vo, r);
  }
}

// dβ_c, dγ_c: the plane totals (Σg, Σg x̂) over the batch index, in index order; one thread per channel
__global__ __launch_bounds__(INORM_THREADS) void inorm_wgrad_kernel(const double* __restrict__ totals, int64_t B, int C,
                                                                    float* __restrict__ gweight, float* __restrict__ gbias) {
  const int c = blockIdx.x * INORM_THREADS + threadIdx.x;
  if (c >= C) return;
  if (gbias) gbias[c] = inorm_channel_sum(totals, B, C, c, 0);
  if (gweight) gweight[c] = inorm_channel_sum(totals, B, C, c, 1);
}

// a 1-D grid of 256-thread workgroups holds fewer than 2^32 threads
static bool inorm_fits(int64_t P, int64_t V) {
  return V < ((int64_t)1 << 31) && P < ((int64_t)1 << 24) && P * (int64_t)inorm_chunks(V) < ((int64_t)1 << 24);
}

// what is wrong with (P, C, V, act_dtype), or FZ_OK
static int inorm_check(const char* who, int64_t P, int C, int64_t V, int act_dtype) {
  if (V < 1) {
    last_error() = std::string(who) + ": V must be at least 1";
    return FZ_E_ARG;
  }
  if (P < 1) {
    last_error() = std::string(who) + ": P must be at least 1";
    return FZ_E_ARG;
  }
  if (act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16) {
    last_error() = std::string(who) + ": act_dtype must be FZ_STORE_F32 or FZ_STORE_BF16";
    return FZ_E_UNSUPPORTED;
  }
  if (C < 1 || P % C != 0) {
    last_error() = std::string(who) + ": P must be a multiple of C >= 1";
    return FZ_E_SHAPE;
  }
  if (!inorm_fits(P, V)) {
    last_error() = std::string(who) + ": a plane must hold fewer than 2^31 elements, the grid fewer than 2^24 workgroups";
    return FZ_E_SHAPE;
  }
  return FZ_OK;
}

template <typename T>
static int inorm_fwd_launch(const void* x, const float* weight, const float* bias, void* y, double* stats, int64_t P, int C,
                            int64_t V, double eps, double* part, hipStream_t s) {
  const dim3 block(INORM_THREADS);
  if (V <= INORM_ONE_PASS_MAX) {
    hipLaunchKernelGGL(inorm_fwd1_kernel<T>, dim3((unsigned)P), block, 0, s, (const T*)x, weight, bias, (T*)y, stats, C, (int)V, eps);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
  }
  const int nchunk = inorm_chunks(V);
  const dim3 grid((unsigned)(P * nchunk));
  hipLaunchKernelGGL((inorm_partials_kernel<T, false>), grid, block, 0, s, (const T*)x, (const T*)nullptr, (const double*)nullptr, V, nchunk, part);
  FZ_LAUNCH_CHECK();
  hipLaunchKernelGGL((inorm_apply_kernel<T, false>), grid, block, 0, s, (const T*)x, (const T*)nullptr, weight, bias, (T*)y, stats,
                     (double*)nullptr, (const double*)part, C, V, nchunk, eps);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

template <typename T>
static int inorm_bwd_launch(const void* x, const void* gy, const float* weight, const double* stats, void* gx, int64_t P, int C,
                            int64_t V, double* part, double* totals, hipStream_t s) {
  const dim3 block(INORM_THREADS);
  if (V <= INORM_ONE_PASS_MAX) {
    hipLaunchKernelGGL(inorm_bwd1_kernel<T>, dim3((unsigned)P), block, 0, s, (const T*)x, (const T*)gy, weight, stats, (T*)gx, totals, C, (int)V);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
  }
  const int nchunk = inorm_chunks(V);
  const dim3 grid((unsigned)(P * nchunk));
  hipLaunchKernelGGL((inorm_partials_kernel<T, true>), grid, block, 0, s, (const T*)x, (const T*)gy, stats, V, nchunk, part);
  FZ_LAUNCH_CHECK();
  hipLaunchKernelGGL((inorm_apply_kernel<T, true>), grid, block, 0, s, (const T*)x, (const T*)gy, weight, (const float*)nullptr, (T*)gx,
                     const_cast<double*>(stats), totals, (const double*)part, C, V, nchunk, 0.0);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

}  // namespace fz

using namespace fz;

extern "C" int fz_inorm_one_pass_max(void) { return INORM_ONE_PASS_MAX; }

extern "C" int fz_inorm_chunks(int64_t V) { return V < 1 ? -1 : inorm_chunks(V); }

extern "C" int64_t fz_inorm_workspace_bytes(int64_t P, int64_t V) {
  if (P < 1 || V < 1 || !inorm_fits(P, V)) return -1;
  return (P * inorm_chunks(V) + P) * 2 * (int64_t)sizeof(double);   // the partials, then the plane totals of the backward
}

extern "C" int fz_inorm_fwd(const void* x, const float* weight, const float* bias, void* y, double* stats, int64_t P, int C,
                            int64_t V, double eps, int act_dtype, void* workspace, fz_stream_t stream) {
  if (const int rc = inorm_check("fz_inorm_fwd", P, C, V, act_dtype)) return rc;
  if (!(eps >= 0.0)) return fail(FZ_E_ARG, "fz_inorm_fwd: eps must be non-negative");
  if (!x || !y || !stats || !workspace) return fail(FZ_E_ARG, "fz_inorm_fwd: null pointer");
  const uintptr_t es = act_dtype == FZ_STORE_F32 ? 4 : 2;
  if ((uintptr_t)x % es || (uintptr_t)y % es || (uintptr_t)stats % 8 || (uintptr_t)workspace % 8)
    return fail(FZ_E_ARG, "fz_inorm_fwd: pointer not aligned to its element");
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  return act_dtype == FZ_STORE_F32 ? inorm_fwd_launch<float>(x, weight, bias, y, stats, P, C, V, eps, part, s)
                                   : inorm_fwd_launch<bf16>(x, weight, bias, y, stats, P, C, V, eps, part, s);
}

extern "C" int fz_inorm_bwd(const void* x, const void* gy, const float* weight, const double* stats, void* gx, float* gweight,
                            float* gbias, int64_t P, int C, int64_t V, int act_dtype, void* workspace, fz_stream_t stream) {
  if (const int rc = inorm_check("fz_inorm_bwd", P, C, V, act_dtype)) return rc;
  if (!x || !gy || !stats || !gx || !workspace) return fail(FZ_E_ARG, "fz_inorm_bwd: null pointer");
  const uintptr_t es = act_dtype == FZ_STORE_F32 ? 4 : 2;
  if ((uintptr_t)x % es || (uintptr_t)gy % es || (uintptr_t)gx % es || (uintptr_t)stats % 8 || (uintptr_t)workspace % 8)
    return fail(FZ_E_ARG, "fz_inorm_bwd: pointer not aligned to its element");
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  double* totals = part + P * inorm_chunks(V) * 2;
  const int rc = act_dtype == FZ_STORE_F32 ? inorm_bwd_launch<float>(x, gy, weight, stats, gx, P, C, V, part, totals, s)
                                           : inorm_bwd_launch<bf16>(x, gy, weight, stats, gx, P, C, V, part, totals, s);
  if (rc != FZ_OK) return rc;
  if (gweight || gbias) {
    hipLaunchKernelGGL(inorm_wgrad_kernel, dim3((unsigned)((C + INORM_THREADS - 1) / INORM_THREADS)), dim3(INORM_THREADS), 0, s,
                       (const double*)totals, P / C, C, gweight, gbias);
    FZ_LAUNCH_CHECK();
  }
  return FZ_OK;
}
