// gnorm.hip — group norm of channels-first activations with a fused activation (none / ReLU / LeakyReLU), forward and backward
// (semantics: factorizer_amd/group_norm.py).  The default norm + activation of the CNN blocks
// (factorizer_amd/cnn.py: nn.GroupNorm(8, C) followed by nn.LeakyReLU).
//
// (B, C, *S) with G groups is B·G contiguous spans of n = cg·V elements (cg = C / G planes of V elements).  Storage fp32 or bf16,
// parameters fp32, every sum and every element in float64, one rounding per stored element; visiting order, tree, chunk plan and
// rounding are those of the instance norm (inorm_core.h, inorm_device.h), the channel arithmetic and the formulas are in
// gnorm_core.h.  No atomics: a group's result depends on nothing but the group, every reduction order on (cg, V) alone.
//   n <= GNORM_ONE_PASS_MAX   one launch each way, one workgroup per group: the span (backward: of x and of g) is read once into
//                             registers.  The backward needs Σg' and Σg'x̂ PER CHANNEL (they are dβ, dγ, and γ_c weighs them in
//                             the group's A, Bq): GNORM_CB channels at a time go through one LDS tree.
//   larger spans              forward: a partials launch over (group, chunk) workgroups, an apply launch walking against it.
//                             backward: a partials launch over (plane, chunk-of-plane) workgroups — per-channel sums are per-plane
//                             sums — then an apply launch over (group, chunk) workgroups, walking against it, that first folds
//                             its group's plane partials in a fixed order.
//   parameter gradients       one more small launch sums the plane totals over the batch index in order.
#include "fz_common.h"
#include "gnorm_core.h"
#include "inorm_device.h"

namespace fz {

// the activation and the affine presence of one call
struct GnormPar {
  const float* gamma;
  const float* beta;
  int act;
  double slope;
};
__device__ __forceinline__ double gnorm_ga(const GnormPar& p, int c) { return p.gamma ? (double)p.gamma[c] : 1.0; }
__device__ __forceinline__ double gnorm_be(const GnormPar& p, int c) { return p.beta ? (double)p.beta[c] : 0.0; }

// r[k] = f(k, γ, β) for the elements i0 .. i0 + W - 1 (below hi) of a group whose first channel is c0: γ, β follow the element
template <int W, typename F>
__device__ __forceinline__ void gnorm_each(const GnormPar& p, int c0, int64_t i0, int64_t hi, int V, F f) {
  GnormChan ch = gnorm_chan(i0, V);
  double ga = gnorm_ga(p, c0 + ch.c), be = gnorm_be(p, c0 + ch.c);
#pragma unroll
  for (int k = 0; k < W; ++k) {
    if (i0 + k < hi) {
      if (k > 0 && ch.r == 0) {
        ga = gnorm_ga(p, c0 + ch.c);
        be = gnorm_be(p, c0 + ch.c);
      }
      f(k, ch.c, ga, be);
      gnorm_next(ch, V);
    }
  }
}

// ---- one launch: the span stays in registers ----------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(INORM_THREADS) void gnorm_fwd1_kernel(const T* __restrict__ x, GnormPar par, T* __restrict__ y,
                                                                   double* __restrict__ stats, int G, int cg, int V, int n,
                                                                   double eps) {
  constexpr int W = 16 / (int)sizeof(T), NG = INORM_REG / W;
  __shared__ double red[2][INORM_THREADS];
  const int t = threadIdx.x;
  const int64_t group = blockIdx.x;
  const int c0 = (int)(group % G) * cg;
  const T* xp = x + group * n;
  T* yp = y + group * n;
  const bool vx = inorm_vec(xp), vy = inorm_vec(yp);
  const double x0 = (double)aget(xp);
  float v[NG][W];
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int a = 0; a < NG; ++a) {
    const int i0 = (a * INORM_THREADS + t) * W;
    if (i0 < n) {
      inorm_load<T, W>(xp, i0, n, vx, v[a]);
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (i0 + k < n) inorm_acc_stat(s1, s2, v[a][k], x0);
    }
  }
  inorm_block_sum2(s1, s2, red);
  const InormStat st = inorm_finish_stat(s1, s2, x0, n, eps);
  if (t == 0) {
    stats[group * 2] = st.mean;
    stats[group * 2 + 1] = st.rstd;
  }
#pragma unroll
  for (int a = 0; a < NG; ++a) {
    const int i0 = (a * INORM_THREADS + t) * W;
    if (i0 < n) {
      double r[W];
#pragma unroll
      for (int k = 0; k < W; ++k) r[k] = 0.0;
      gnorm_each<W>(par, c0, i0, n, V, [&](int k, int, double ga, double be) {
        r[k] = gnorm_y(v[a][k], st.mean, st.rstd, ga, be, par.act, par.slope);
      });
      inorm_store(yp, i0, n, vy, r);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(INORM_THREADS) void gnorm_bwd1_kernel(const T* __restrict__ x, const T* __restrict__ g, GnormPar par,
                                                                   const double* __restrict__ stats, T* __restrict__ gx,
                                                                   double* __restrict__ totals, int G, int cg, int V, int n) {
  constexpr int W = 16 / (int)sizeof(T), NG = INORM_REG / W;
  __shared__ double red[2 * GNORM_CB][INORM_THREADS];
  const int t = threadIdx.x;
  const int64_t group = blockIdx.x;
  const int c0 = (int)(group % G) * cg;
  const int64_t plane0 = group * cg;   // (b C + c0)
  const T* xp = x + group * n;
  const T* gp = g + group * n;
  T* op = gx + group * n;
  const bool vx = inorm_vec(xp), vg = inorm_vec(gp), vo = inorm_vec(op);
  const double mean = stats[group * 2], rstd = stats[group * 2 + 1];
  float xv[NG][W], gv[NG][W];
#pragma unroll
  for (int a = 0; a < NG; ++a) {
    const int i0 = (a * INORM_THREADS + t) * W;
    if (i0 < n) {
      inorm_load<T, W>(xp, i0, n, vx, xv[a]);
      inorm_load<T, W>(gp, i0, n, vg, gv[a]);
    }
  }
  double A = 0.0, Bq = 0.0;
  if (cg == 1 || (!par.gamma && !par.beta)) {
    // one channel, or no parameter at all: the group's two sums are all there is
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int a = 0; a < NG; ++a) {
      const int i0 = (a * INORM_THREADS + t) * W;
      if (i0 < n)
        gnorm_each<W>(par, c0, i0, n, V, [&](int k, int, double ga, double be) {
          gnorm_acc_grad(s1, s2, gnorm_gprime(gv[a][k], xv[a][k], mean, rstd, ga, be, par.act, par.slope), xv[a][k], mean, rstd);
        });
    }
    inorm_block_sum2(s1, s2, red);
    if (cg == 1 && t == 0) {
      totals[plane0 * 2] = s1;
      totals[plane0 * 2 + 1] = s2;
    }
    const double ga = cg == 1 ? gnorm_ga(par, c0) : 1.0;
    A = ga * s1;
    Bq = ga * s2;
  } else {
    for (int cb = 0; cb < cg; cb += GNORM_CB) {   // channels cb .. cb + GNORM_CB - 1 of the group
      double s1[GNORM_CB], s2[GNORM_CB];
#pragma unroll
      for (int j = 0; j < GNORM_CB; ++j) s1[j] = s2[j] = 0.0;
      const int64_t lo = (int64_t)cb * V, hi = (int64_t)(cb + GNORM_CB) * V;   // their elements
#pragma unroll
      for (int a = 0; a < NG; ++a) {
        const int i0 = (a * INORM_THREADS + t) * W;
        if (i0 < n && i0 < hi && i0 + W > lo)
          gnorm_each<W>(par, c0, i0, n, V, [&](int k, int c, double ga, double be) {
            const double gpr = gnorm_gprime(gv[a][k], xv[a][k], mean, rstd, ga, be, par.act, par.slope);
#pragma unroll
            for (int j = 0; j < GNORM_CB; ++j)
              if (c == cb + j) gnorm_acc_grad(s1[j], s2[j], gpr, xv[a][k], mean, rstd);
          });
      }
      __syncthreads();   // red may still be read from the previous batch
#pragma unroll
      for (int j = 0; j < GNORM_CB; ++j) {
        red[2 * j][t] = s1[j];
        red[2 * j + 1][t] = s2[j];
      }
      __syncthreads();
      for (int w = INORM_THREADS / 2; w > 0; w >>= 1) {
#pragma unroll
        for (int j = 0; j < 2 * GNORM_CB; ++j) inorm_tree_step(red[j], t, w);
        __syncthreads();
      }
      for (int j = 0; j < GNORM_CB && cb + j < cg; ++j) {   // in channel order, the same in every thread
        const double t1 = red[2 * j][0], t2 = red[2 * j + 1][0], ga = gnorm_ga(par, c0 + cb + j);
        A += ga * t1;
        Bq += ga * t2;
        if (t == 0) {
          totals[(plane0 + cb + j) * 2] = t1;
          totals[(plane0 + cb + j) * 2 + 1] = t2;
        }
      }
    }
  }
  A /= (double)n;
  Bq /= (double)n;
#pragma unroll
  for (int a = 0; a < NG; ++a) {
    const int i0 = (a * INORM_THREADS + t) * W;
    if (i0 < n) {
      double r[W];
#pragma unroll
      for (int k = 0; k < W; ++k) r[k] = 0.0;
      gnorm_each<W>(par, c0, i0, n, V, [&](int k, int, double ga, double be) {
        const double gpr = gnorm_gprime(gv[a][k], xv[a][k], mean, rstd, ga, be, par.act, par.slope);
        r[k] = gnorm_gx(gpr, xv[a][k], mean, rstd, ga, A, Bq);
      });
      inorm_store(op, i0, n, vo, r);
    }
  }
}

// ---- two launches ---------------------------------------------------------------------------------------------------------
// BWD = false: a unit is a group (span n = cg V), sums of d, d² about its first element.
// BWD = true:  a unit is a plane (span V), sums of g', g' x̂ with the statistics of the plane's group and its own γ, β.
template <typename T, bool BWD>
__global__ __launch_bounds__(INORM_THREADS) void gnorm_partials_kernel(const T* __restrict__ x, const T* __restrict__ g, GnormPar par,
                                                                       const double* __restrict__ stats, int C, int cg, int64_t span,
                                                                       int nchunk, double* __restrict__ part) {
  constexpr int W = 16 / (int)sizeof(T);
  __shared__ double red[2][INORM_THREADS];
  const int t = threadIdx.x;
  const int64_t idx = blockIdx.x, unit = idx / nchunk;
  InormSpan sp = inorm_chunk(span, (int)(idx - unit * nchunk));
  const T* xp = x + unit * span;
  const T* gp = BWD ? g + unit * span : nullptr;
  const bool vx = inorm_vec(xp), vg = BWD && inorm_vec(gp);
  double p0, p1 = 0.0, ga = 1.0, be = 0.0;
  if constexpr (BWD) {
    const int64_t group = unit / cg;   // (b C + c) / cg = b G + c / cg
    const int c = (int)(unit % C);
    p0 = stats[group * 2];
    p1 = stats[group * 2 + 1];
    ga = gnorm_ga(par, c);
    be = gnorm_be(par, c);
  } else {
    p0 = (double)aget(xp);
  }
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
        if constexpr (BWD) gnorm_acc_grad(s1, s2, gnorm_gprime(gv[k], xv[k], p0, p1, ga, be, par.act, par.slope), xv[k], p0, p1);
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

// over (group, chunk of the span) workgroups, descending.  pchunk: partials per unit of the partials launch (forward: per group,
// = nchunk; backward: per plane)
template <typename T, bool BWD>
__global__ __launch_bounds__(INORM_THREADS) void gnorm_apply_kernel(const T* __restrict__ x, const T* __restrict__ g, GnormPar par,
                                                                    T* __restrict__ out, const double* __restrict__ stats_in,
                                                                    double* __restrict__ stats_out, double* __restrict__ totals, const double* __restrict__ part, int G,
                                                                    int cg, int V, int64_t n, int nchunk, int pchunk, double eps) {
  constexpr int W = 16 / (int)sizeof(T);
  __shared__ double red[2][INORM_THREADS];
  const int t = threadIdx.x;
  const int64_t idx = (int64_t)gridDim.x - 1 - blockIdx.x, group = idx / nchunk;
  const int chunk = (int)(idx - group * nchunk);
  const InormSpan sp = inorm_chunk(n, chunk);
  const int c0 = (int)(group % G) * cg;
  const T* xp = x + group * n;
  const T* gp = BWD ? g + group * n : nullptr;
  T* op = out + group * n;
  const bool vx = inorm_vec(xp), vg = BWD && inorm_vec(gp), vo = inorm_vec(op);
  double mean, rstd, A = 0.0, Bq = 0.0;
  if constexpr (BWD) {
    // thread t folds the planes t, t + 256, ... of the group: a plane's partials in index order, weighed by its γ
    const int64_t plane0 = group * cg;
    double s1 = 0.0, s2 = 0.0;
    for (int j = t; j < cg; j += INORM_THREADS) {
      const double* pp = part + (plane0 + j) * pchunk * 2;
      const double t1 = gnorm_plane_total(pp, pchunk), t2 = gnorm_plane_total(pp + 1, pchunk), ga = gnorm_ga(par, c0 + j);
      s1 += ga * t1;
      s2 += ga * t2;
      if (chunk == 0) {
        totals[(plane0 + j) * 2] = t1;
        totals[(plane0 + j) * 2 + 1] = t2;
      }
    }
    inorm_block_sum2(s1, s2, red);
    mean = stats_in[group * 2];
    rstd = stats_in[group * 2 + 1];
    A = s1 / (double)n;
    Bq = s2 / (double)n;
  } else {
    const double* pp = part + group * pchunk * 2;
    double s1 = inorm_partial_share(pp, pchunk, 2, t), s2 = inorm_partial_share(pp + 1, pchunk, 2, t);
    inorm_block_sum2(s1, s2, red);
    const InormStat st = inorm_finish_stat(s1, s2, (double)aget(xp), n, eps);
    mean = st.mean;
    rstd = st.rstd;
    if (chunk == 0 && t == 0) {
      stats_out[group * 2] = mean;
      stats_out[group * 2 + 1] = rstd;
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
    for (int k = 0; k < W; ++k) r[k] = 0.0;
    gnorm_each<W>(par, c0, i0, sp.hi, V, [&](int k, int, double ga, double be) {
      if constexpr (BWD) {
        const double gpr = gnorm_gprime(gv[k], xv[k], mean, rstd, ga, be, par.act, par.slope);
        r[k] = gnorm_gx(gpr, xv[k], mean, rstd, ga, A, Bq);
      } else {
        r[k] = gnorm_y(xv[k], mean, rstd, ga, be, par.act, par.slope);
      }
    });
    inorm_store(op, i0, sp.hi, vo, r);
  }
}

// dβ_c, dγ_c: the plane totals (Σg', Σg' x̂) over the batch index, in index order; one thread per channel
__global__ __launch_bounds__(INORM_THREADS) void gnorm_wgrad_kernel(const double* __restrict__ totals, int64_t B, int C,
                                                                    float* __restrict__ gweight, float* __restrict__ gbias) {
  const int c = blockIdx.x * INORM_THREADS + threadIdx.x;
  if (c >= C) return;
  if (gbias) gbias[c] = inorm_channel_sum(totals, B, C, c, 0);
  if (gweight) gweight[c] = inorm_channel_sum(totals, B, C, c, 1);
}

// the grids of both directions: 1-D, fewer than 2^24 workgroups; a span holds fewer than 2^31 elements
static bool gnorm_fits(int64_t B, int64_t C, int64_t G, int64_t V) {
  const int64_t lim = (int64_t)1 << 24, cg = C / G;
  if (V >= ((int64_t)1 << 31) / cg) return false;
  if (B >= lim || B * C >= lim) return false;
  return B * G * (int64_t)gnorm_chunks(cg * V) < lim && B * C * (int64_t)inorm_chunks(V) < lim;
}
static int64_t gnorm_part_doubles(int64_t B, int64_t C, int64_t G, int64_t V) {
  const int64_t f = B * G * gnorm_chunks(C / G * V), b = B * C * inorm_chunks(V);
  return 2 * (f > b ? f : b);
}

// what is wrong with the arguments every entry point shares, or FZ_OK
static int gnorm_check(const char* who, int64_t B, int C, int G, int64_t V, int act, double slope, int act_dtype) {
  const std::string w(who);
  if (B < 1 || V < 1) return fail(FZ_E_ARG, (w + ": B and V must be at least 1").c_str());
  if (act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16)
    return fail(FZ_E_UNSUPPORTED, (w + ": act_dtype must be FZ_STORE_F32 or FZ_STORE_BF16").c_str());
  if (act != GNORM_ACT_NONE && act != GNORM_ACT_RELU && act != GNORM_ACT_LEAKY_RELU)
    return fail(FZ_E_UNSUPPORTED, (w + ": unknown activation id").c_str());
  if (!(slope == slope)) return fail(FZ_E_ARG, (w + ": negative_slope is not a number").c_str());
  if (C < 1 || G < 1 || C % G != 0) return fail(FZ_E_SHAPE, (w + ": C must be a multiple of G >= 1").c_str());
  if (!gnorm_fits(B, C, G, V))
    return fail(FZ_E_SHAPE, (w + ": a group must hold fewer than 2^31 elements, the grid fewer than 2^24 workgroups").c_str());
  return FZ_OK;
}

template <typename T>
static int gnorm_fwd_launch(const void* x, GnormPar par, void* y, double* stats, int64_t B, int C, int G, int64_t V, double eps,
                            double* part, hipStream_t s) {
  const dim3 block(INORM_THREADS);
  const int cg = C / G;
  const int64_t n = (int64_t)cg * V;
  if (n <= GNORM_ONE_PASS_MAX) {
    hipLaunchKernelGGL(gnorm_fwd1_kernel<T>, dim3((unsigned)(B * G)), block, 0, s, (const T*)x, par, (T*)y, stats, G, cg, (int)V, (int)n, eps);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
  }
  const int nchunk = gnorm_chunks(n);
  const dim3 grid((unsigned)(B * G * nchunk));
  hipLaunchKernelGGL((gnorm_partials_kernel<T, false>), grid, block, 0, s, (const T*)x, (const T*)nullptr, par, (const double*)nullptr, C, cg,
                     n, nchunk, part);
  FZ_LAUNCH_CHECK();
  hipLaunchKernelGGL((gnorm_apply_kernel<T, false>), grid, block, 0, s, (const T*)x, (const T*)nullptr, par, (T*)y, (const double*)nullptr, stats, (double*)nullptr,
                     (const double*)part, G, cg, (int)V, n, nchunk, nchunk, eps);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

template <typename T>
static int gnorm_bwd_launch(const void* x, const void* gy, GnormPar par, const double* stats, void* gx, int64_t B, int C, int G,
                            int64_t V, double* part, double* totals, hipStream_t s) {
  const dim3 block(INORM_THREADS);
  const int cg = C / G;
  const int64_t n = (int64_t)cg * V;
  if (n <= GNORM_ONE_PASS_MAX) {
    hipLaunchKernelGGL(gnorm_bwd1_kernel<T>, dim3((unsigned)(B * G)), block, 0, s, (const T*)x, (const T*)gy, par, stats, (T*)gx, totals, G, cg,
                       (int)V, (int)n);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
  }
  const int nchunk = gnorm_chunks(n), pchunk = inorm_chunks(V);
  hipLaunchKernelGGL((gnorm_partials_kernel<T, true>), dim3((unsigned)(B * C * pchunk)), block, 0, s, (const T*)x, (const T*)gy, par, stats, C,
                     cg, V, pchunk, part);
  FZ_LAUNCH_CHECK();
  hipLaunchKernelGGL((gnorm_apply_kernel<T, true>), dim3((unsigned)(B * G * nchunk)), block, 0, s, (const T*)x, (const T*)gy, par, (T*)gx,
                     stats, (double*)nullptr, totals, (const double*)part, G, cg, (int)V, n, nchunk, pchunk, 0.0);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

}  // namespace fz

using namespace fz;

extern "C" int fz_gnorm_one_pass_max(void) { return GNORM_ONE_PASS_MAX; }

extern "C" int fz_gnorm_chunks(int cg, int64_t V) {
  if (cg < 1 || V < 1 || V >= ((int64_t)1 << 31) / cg) return -1;
  return gnorm_chunks((int64_t)cg * V);
}

extern "C" int64_t fz_gnorm_workspace_bytes(int64_t B, int C, int G, int64_t V) {
  if (B < 1 || V < 1 || C < 1 || G < 1 || C % G != 0 || !gnorm_fits(B, C, G, V)) return -1;
  return (gnorm_part_doubles(B, C, G, V) + B * C * 2) * (int64_t)sizeof(double);   // the partials, then the plane totals of the backward
}

extern "C" int fz_gnorm_launches(int cg, int64_t V, int backward, int affine) {
  if (cg < 1 || V < 1 || V >= ((int64_t)1 << 31) / cg) return -1;
  return ((int64_t)cg * V <= GNORM_ONE_PASS_MAX ? 1 : 2) + (backward && affine ? 1 : 0);
}

extern "C" int fz_gnorm_fwd(const void* x, const float* weight, const float* bias, void* y, double* stats, int64_t B, int C, int G,
                            int64_t V, double eps, int act, double negative_slope, int act_dtype, void* workspace,
                            fz_stream_t stream) {
  if (const int rc = gnorm_check("fz_gnorm_fwd", B, C, G, V, act, negative_slope, act_dtype)) return rc;
  if (!(eps >= 0.0)) return fail(FZ_E_ARG, "fz_gnorm_fwd: eps must be non-negative");
  if (!x || !y || !stats || !workspace) return fail(FZ_E_ARG, "fz_gnorm_fwd: null pointer");
  const uintptr_t es = act_dtype == FZ_STORE_F32 ? 4 : 2;
  if ((uintptr_t)x % es || (uintptr_t)y % es || (uintptr_t)stats % 8 || (uintptr_t)workspace % 8)
    return fail(FZ_E_ARG, "fz_gnorm_fwd: pointer not aligned to its element");
  const GnormPar par{weight, bias, act, act == GNORM_ACT_RELU ? 0.0 : negative_slope};
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  return act_dtype == FZ_STORE_F32 ? gnorm_fwd_launch<float>(x, par, y, stats, B, C, G, V, eps, part, s)
                                   : gnorm_fwd_launch<bf16>(x, par, y, stats, B, C, G, V, eps, part, s);
}

extern "C" int fz_gnorm_bwd(const void* x, const void* gy, const float* weight, const float* bias, const double* stats, void* gx,
                            float* gweight, float* gbias, int64_t B, int C, int G, int64_t V, int act, double negative_slope,
                            int act_dtype, void* workspace, fz_stream_t stream) {
  if (const int rc = gnorm_check("fz_gnorm_bwd", B, C, G, V, act, negative_slope, act_dtype)) return rc;
  if (!x || !gy || !stats || !gx || !workspace) return fail(FZ_E_ARG, "fz_gnorm_bwd: null pointer");
  if ((gweight && !weight) || (gbias && !bias)) return fail(FZ_E_ARG, "fz_gnorm_bwd: a parameter gradient without its parameter");
  const uintptr_t es = act_dtype == FZ_STORE_F32 ? 4 : 2;
  if ((uintptr_t)x % es || (uintptr_t)gy % es || (uintptr_t)gx % es || (uintptr_t)stats % 8 || (uintptr_t)workspace % 8)
    return fail(FZ_E_ARG, "fz_gnorm_bwd: pointer not aligned to its element");
  const GnormPar par{weight, bias, act, act == GNORM_ACT_RELU ? 0.0 : negative_slope};
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  double* totals = part + gnorm_part_doubles(B, C, G, V);
  const int rc = act_dtype == FZ_STORE_F32 ? gnorm_bwd_launch<float>(x, gy, par, stats, gx, B, C, G, V, part, totals, s)
                                           : gnorm_bwd_launch<bf16>(x, gy, par, stats, gx, B, C, G, V, part, totals, s);
  if (rc != FZ_OK) return rc;
  if (gweight || gbias) {
    hipLaunchKernelGGL(gnorm_wgrad_kernel, dim3((unsigned)((C + INORM_THREADS - 1) / INORM_THREADS)), dim3(INORM_THREADS), 0, s,
                       (const double*)totals, B, C, gweight, gbias);
    FZ_LAUNCH_CHECK();
  }
  return FZ_OK;
}
