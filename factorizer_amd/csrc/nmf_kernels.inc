// nmf_kernels.inc — gfx950 kernels around the per-wave program of nmf_core.h.
// Included by nmf_r{1..4}.hip / nmf_r{1..4}_bf16.hip with FZ_R (rank) and FZ_AT (storage type of the
// matrices X / Y / GY / GX: float or bf16) defined — one translation unit per (rank, storage type)
// keeps the build parallel.  Those units instantiate MU and HALS; nmf_r{1..4}[_bf16]_cdsmu.hip define
// FZ_NMF_CD_SMU and instantiate CD and SMU.  Whatever the storage type, the wave program runs in fp32: the factors,
// Gram matrices and eps of matrix_factorization.py:200,236 never see bf16 (SURVEY.md §5).  Replaces the reference's per-iteration bmm + elementwise launches
// (factorization/matrix_factorization.py:213-227, 241-247, 514-546).
#include "fz_common.h"
#include "nmf_core.h"
#include "nmf_shapes.h"

namespace fz {

// Device wave context.  FAST: M == Mreal, N == 64*NPL, 16-byte loads (lane l owns columns
// 4l..4l+3 of every 256-column panel: a wave instruction moves 1 KiB contiguous).
// Otherwise: masked, column n = 64*j + lane (256 B contiguous per wave instruction).
template <int M, int NPL, bool FAST>
struct DevWave {
  using F = float;
  int lane, mreal, nreal;

  __device__ __forceinline__ int col(int j) const {
    return FAST ? ((j >> 2) * 256 + lane * 4 + (j & 3)) : (j * 64 + lane);
  }
  __device__ __forceinline__ float sum(float v) const { return wave_sum(v); }
  __device__ __forceinline__ void sum8(float (&v)[8]) const { wave_sum8(v, lane); }
  __device__ __forceinline__ void st_priv(float* base, int idx, float v) const { base[idx * 64 + lane] = v; }
  __device__ __forceinline__ float ld_priv(const float* base, int idx) const { return base[idx * 64 + lane]; }
  __device__ __forceinline__ void st_uni(float* base, int idx, float v) const {
    if (lane == 0) base[idx] = v;
  }
  __device__ __forceinline__ float ld_uni(const float* base, int idx) const { return base[idx]; }
  __device__ __forceinline__ float ld_uni_global(const float* p, int idx) const { return p[idx]; }
  __device__ __forceinline__ float ld_v0(const float* v0, int j, int r, int R) const {
    int n = col(j);
    if (FAST) return v0[n * R + r];
    return n < nreal ? v0[n * R + r] : 0.f;
  }
  __device__ __forceinline__ float keep_col(int j, float v) const {
    if (FAST) return v;
    return col(j) < nreal ? v : 0.f;
  }
  // the history is written by lane 0 / read by all lanes of the same wave: LDS ops of one
  // wave execute in order, the fence only pins the compiler's ordering.
  __device__ __forceinline__ void fence() const { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
  // factor rows distributed over the eight 8-lane groups (nmf_core.h DistRows) — available, OFF for these standalone
  // kernels: the distributed form is the same arithmetic per row but the compiler contracts / schedules the 1-row and the
  // 8-row code differently (results differ in the last bit: 4e-7 relative on y, tools/probes/nmf_ab.py), and
  // tests/test_gpu_parity.py::test_nmf_8x512_vs_oracle[3-mu] sits on its 1e-4 bound for one of 65 536 matrices (2.0e-4
  // with the distributed form).  These kernels are off the hot path; the fused cores (nmf_cf_fwd.hip, nmf_cf_bwd.hip, nmf_pcf.hip), whose
  // rank-2 forms are VALU-bound, use it.
#ifndef FZ_DIST_ROWS
#define FZ_DIST_ROWS 0
#endif
  static constexpr bool kDistRows = FZ_DIST_ROWS != 0;
  __device__ __forceinline__ float sum8_dist(const float (&v)[8]) const { return wave_sum8_dist(v, lane); }
  __device__ __forceinline__ float grp_take(float d, int m) const {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 8 * m));
  }
  __device__ __forceinline__ bool grp_below(int n) const { return (lane >> 3) < n; }
  __device__ __forceinline__ void st_grp(float* base, int i0, int stride, float d) const {
    if ((lane & 7) == 0) base[i0 + (lane >> 3) * stride] = d;
  }
  __device__ __forceinline__ float ld_grp_global(const float* p, int i0, int stride) const { return p[i0 + (lane >> 3) * stride]; }
  __device__ __forceinline__ float ld_grp(const float* base, int i0, int stride) const { return base[i0 + (lane >> 3) * stride]; }
  __device__ __forceinline__ float grp_sum(float d) const { return wave_group_sum(d); }

  template <typename AT>
  __device__ __forceinline__ void load_mat(const AT* __restrict__ X, float (&x)[M][NPL]) const {
    if (FAST) {
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int q = 0; q < NPL / 4; ++q) {
          const float4 t = ld4(X + m * (NPL * 64) + q * 256 + 4 * lane);
          x[m][4 * q + 0] = t.x;
          x[m][4 * q + 1] = t.y;
          x[m][4 * q + 2] = t.z;
          x[m][4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
          int n = j * 64 + lane;
          x[m][j] = (m < mreal && n < nreal) ? aget(X + m * nreal + n) : 0.f;
        }
    }
  }
  template <typename AT>
  __device__ __forceinline__ void store_mat(AT* __restrict__ Y, const float (&x)[M][NPL]) const {
    if (FAST) {
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int q = 0; q < NPL / 4; ++q) {
          float4 t = make_float4(x[m][4 * q], x[m][4 * q + 1], x[m][4 * q + 2], x[m][4 * q + 3]);
          st4(Y + m * (NPL * 64) + q * 256 + 4 * lane, t);
        }
    } else {
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
          int n = j * 64 + lane;
          if (m < mreal && n < nreal) aput(Y + m * nreal + n, x[m][j]);
        }
    }
  }
};

template <int M, int NPL, int R, int SOLVER, bool FAST, typename AT>
__global__ __launch_bounds__(256) void nmf_fwd_kernel(const AT* __restrict__ X,
                                                      const float* __restrict__ u0,
                                                      const float* __restrict__ v0,
                                                      AT* __restrict__ Y, float* __restrict__ Uo,
                                                      float* __restrict__ Vo, int64_t nmat,
                                                      int mreal, int nreal, int T, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t mat = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (mat >= nmat) return;
  DevWave<M, NPL, FAST> w{lane, mreal, nreal};
  float x[M][NPL], u[M][R], v[NPL][R];
  const int64_t off = mat * (int64_t)mreal * nreal;
  w.load_mat(X + off, x);
  nmf_forward_wave<M, NPL, R, SOLVER>(w, u0, v0, x, u, v, mreal, T, eps);
  w.store_mat(Y + off, x);
  if (Uo != nullptr && lane == 0) {
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (m < mreal) Uo[(mat * mreal + m) * R + r] = u[m][r];
  }
  if (Vo != nullptr) {
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      int n = w.col(j);
      if (n < nreal) {
#pragma unroll
        for (int r = 0; r < R; ++r) Vo[(mat * nreal + n) * R + r] = v[j][r];
      }
    }
  }
}

// Waves per SIMD the backward is compiled for: the rank-1 programs fit 256 registers beside two resident waves; rank >= 2 (and
// every M = 32 family) keep X, dL/dY and the per-rank factor rows live at once and are given the whole unified file (512 = 256
// architectural + 256 accumulation registers, which the allocator uses as spill space before it touches scratch memory).
template <int M, int NPL, int R>
constexpr int nmf_bwd_waves_per_simd() { return (R == 1 && M * NPL <= 64) ? 2 : 1; }

template <int M, int NPL, int R, int SOLVER, bool FAST, typename AT>
__global__ __launch_bounds__(256, (nmf_bwd_waves_per_simd<M, NPL, R>())) void nmf_bwd_kernel(const AT* __restrict__ X,
                                                      const float* __restrict__ u0,
                                                      const float* __restrict__ v0,
                                                      const AT* __restrict__ GY,
                                                      const float* __restrict__ GU,
                                                      const float* __restrict__ GV,
                                                      AT* __restrict__ GX, int64_t nmat,
                                                      int mreal, int nreal, int T, int G, float eps) {
  extern __shared__ __attribute__((aligned(16))) float fz_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t mat = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (mat >= nmat) return;
  DevWave<M, NPL, FAST> w{lane, mreal, nreal};
  Hist<M, NPL, R> h;
  h.carve(fz_lds + wave * Hist<M, NPL, R>::floats(G), G);
  float x[M][NPL], g[M][NPL];
  const int64_t off = mat * (int64_t)mreal * nreal;
  w.load_mat(X + off, x);
  if (GY != nullptr) {
    w.load_mat(GY + off, g);
  } else {
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int j = 0; j < NPL; ++j) g[m][j] = 0.f;
  }
  nmf_backward_wave<M, NPL, R, SOLVER>(w, u0, v0, x, g, h, mreal, T, G, eps,
                                       GU ? GU + mat * mreal * R : nullptr,
                                       GV ? GV + mat * (int64_t)nreal * R : nullptr);
  w.store_mat(GX + off, g);
}

// ---- host launchers for this rank -------------------------------------------------------
static constexpr int kMaxLdsBytes = 160 * 1024;

template <int M, int NPL, int SOLVER, bool FAST>
static int launch_fwd_t(const NmfArgs& a) {
  constexpr int R = FZ_R;
  const int wpb = 4;
  dim3 grid((unsigned)((a.nmat + wpb - 1) / wpb)), block(64 * wpb);
  hipLaunchKernelGGL((nmf_fwd_kernel<M, NPL, R, SOLVER, FAST, FZ_AT>), grid, block, 0, a.stream,
                     (const FZ_AT*)a.x, a.u0, a.v0, (FZ_AT*)a.y, a.uo, a.vo, a.nmat, a.M, a.N, a.T, a.eps);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

template <int M, int NPL, int SOLVER, bool FAST>
static int launch_bwd_t(const NmfArgs& a) {
  constexpr int R = FZ_R;
  const int per_wave = Hist<M, NPL, R>::floats(a.G) * (int)sizeof(float);
  if (per_wave > kMaxLdsBytes) return fail(FZ_E_UNSUPPORTED, "fz_nmf_bwd: history exceeds LDS");
  const int wpb = fz_hist_waves_per_block(per_wave);
  const int lds = per_wave * wpb;
  auto kern = nmf_bwd_kernel<M, NPL, R, SOLVER, FAST, FZ_AT>;
  if (lds > 65536)
    FZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  dim3 grid((unsigned)((a.nmat + wpb - 1) / wpb)), block(64 * wpb);
  hipLaunchKernelGGL(kern, grid, block, lds, a.stream, (const FZ_AT*)a.x, a.u0, a.v0, (const FZ_AT*)a.gy,
                     a.gu, a.gv, (FZ_AT*)a.gx, a.nmat, a.M, a.N, a.T, a.G, a.eps);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

template <bool BWD, int M, int NPL, bool FAST>
static int launch_solver(const NmfArgs& a) {
#if FZ_NMF_CD_SMU
  // the CD / SMU units (nmf_r*_cdsmu.hip): their own translation units, so the MU / HALS objects stay as they were and the
  // build stays parallel
  if (a.solver == FZ_SOLVER_CD)
    return BWD ? launch_bwd_t<M, NPL, SOLVER_CD, FAST>(a) : launch_fwd_t<M, NPL, SOLVER_CD, FAST>(a);
  if (a.solver == FZ_SOLVER_SMU)
    return BWD ? launch_bwd_t<M, NPL, SOLVER_SMU, FAST>(a) : launch_fwd_t<M, NPL, SOLVER_SMU, FAST>(a);
  return fail(FZ_E_ARG, "fz_nmf: bad solver");
#else
  if (a.solver == FZ_SOLVER_MU)
    return BWD ? launch_bwd_t<M, NPL, SOLVER_MU, FAST>(a) : launch_fwd_t<M, NPL, SOLVER_MU, FAST>(a);
  return BWD ? launch_bwd_t<M, NPL, SOLVER_HALS, FAST>(a) : launch_fwd_t<M, NPL, SOLVER_HALS, FAST>(a);
#endif
}

template <bool BWD>
static int launch_shape(const NmfArgs& a) {
  // the first row of the shape table (nmf_shapes.h) that holds the matrix; exactly 8x512 has a form without masks
  if (a.M == 8 && a.N == 512) return launch_solver<BWD, 8, 8, true>(a);
#define FZ_NMF_ROW(MP, NPL, MMAX, NMAX) \
  if (a.M <= MMAX && a.N <= NMAX) return launch_solver<BWD, MP, NPL, false>(a);
  FZ_NMF_SHAPES(FZ_NMF_ROW)
#undef FZ_NMF_ROW
  return fail(FZ_E_UNSUPPORTED, "fz_nmf: (M,N) outside the native kernel families");
}

#define FZ_CAT2(a, b) a##b
#define FZ_CAT(a, b) FZ_CAT2(a, b)
#ifndef FZ_AT_TAG
#define FZ_AT_TAG
#endif
int FZ_CAT(FZ_CAT(nmf_launch_fwd_r, FZ_R), FZ_AT_TAG)(const NmfArgs& a) { return launch_shape<false>(a); }
int FZ_CAT(FZ_CAT(nmf_launch_bwd_r, FZ_R), FZ_AT_TAG)(const NmfArgs& a) { return launch_shape<true>(a); }

}  // namespace fz
