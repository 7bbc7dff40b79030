// nmf_global_rank.h — kernels and host paths of the split-N NMF for ranks up to 32 (nmf_global_rank.hip describes the
// scheme).
//
// Everything that touches an ACTIVATION (X, gY, y, gX) is a template on the storage type AT in {float, bf16}
// (fz_common.h): nmf_global_rank.hip instantiates AT = float, nmf_global_rank_bf16.hip AT = bf16.  Only storage differs:
// X and gY become fp32 as they are loaded, every y and gX element is rounded once (RNE) as it is stored; the factors,
// Gram matrices, slab partials, histories and the order of every sum are those of the fp32 instance.  gx_v_kernel and
// gx_bwd_col_kernel own one column per thread, so their bf16 accesses are single elements whatever the alignment;
// gx_prod_kernel stages rows into LDS — a copy, no sum — and takes 8, 4, 2 or 1 elements per access as the address of the
// matrix and N allow (GxJob::l_vec; the element kind is a field of the job: Vᵀ, Ga, G stay fp32 workspace rows).
//
// gX is summed over G + 1 launches.  The bf16 instance keeps that running sum in fp32 in the workspace (`gxacc`:
// nmat·M·N floats that only the bf16 backward layout has) and the last launch stores it as bf16: one rounding per element.
#pragma once
#include "fz_common.h"
#include "nmf_core.h"
#include "nmf_wide.h"

namespace fz {

constexpr int kGxThreads = 256;
constexpr int kGxMinM = 16, kGxMaxM = 512, kGxMaxR = 32;
constexpr int kGxSlab = 1024;    // columns per slab (one workgroup of gx_prod_kernel per slab and row chunk)
constexpr int kGxTile = 128;     // columns staged at a time
constexpr int kGxChunk = 64;     // rows per chunk: one lane each
constexpr int kGxXs = kGxTile + 1;

template <int RR>
__device__ __forceinline__ void gx_ldrow(const float* __restrict__ s, float (&o)[RR]) {
#pragma unroll
  for (int j = 0; j < RR / 4; ++j) {
    const float4 t = *reinterpret_cast<const float4*>(s + 4 * j);
    o[4 * j] = t.x; o[4 * j + 1] = t.y; o[4 * j + 2] = t.z; o[4 * j + 3] = t.w;
  }
}
// acc[r] += x * s[r]
template <int RR>
__device__ __forceinline__ void gx_axpy(float (&acc)[RR], float x, const float* __restrict__ s) {
  float t[RR];
  gx_ldrow<RR>(s, t);
#pragma unroll
  for (int r = 0; r < RR; ++r) acc[r] = acc[r] + x * t[r];
}
// Σ_r s[r] * v[r], first term initialises (u vᵀ of matrix_factorization.py:532-533)
template <int RR>
__device__ __forceinline__ float gx_dot(const float* __restrict__ s, const float (&v)[RR]) {
  float t[RR];
  gx_ldrow<RR>(s, t);
  float acc = t[0] * v[0];
#pragma unroll
  for (int r = 1; r < RR; ++r) acc = acc + t[r] * v[r];
  return acc;
}
// a factor row from global memory, zero beyond R
template <int RR>
__device__ __forceinline__ void gx_ldfac(const float* __restrict__ p, int R, bool ok, float (&o)[RR]) {
#pragma unroll
  for (int r = 0; r < RR; ++r) o[r] = (ok && r < R) ? p[r] : 0.f;
}
template <int RR>
__device__ __forceinline__ void gx_stfac(float* __restrict__ p, int R, const float (&v)[RR]) {
#pragma unroll
  for (int r = 0; r < RR; ++r)
    if (r < R) p[r] = v[r];
}
// NB consecutive rows (m0 < m_hi, m0 + 1, ...) of this thread's column; zero where the column is out (!ok); rows >= m_hi
// are zero or a copy of another row: callers skip them
template <int NB>
__device__ __forceinline__ void gx_ld_col(const float* __restrict__ Xc, int64_t N, int m0, int m_hi, bool ok, int,
                                          float (&xb)[NB]) {
#pragma unroll
  for (int i = 0; i < NB; ++i) xb[i] = (ok && m0 + i < m_hi) ? Xc[(int64_t)(m0 + i) * N] : 0.f;
}
// bf16.  pair (grid-uniform: N even and the matrix 4-byte aligned): threads 2k and 2k + 1 own adjacent columns, so the
// two elements of a row are one aligned 4-byte word.  The even thread loads that word for rows m0, m0 + 2, ..., the odd
// one for rows m0 + 1, m0 + 3, ..., and they exchange halves on the DPP network: half the load instructions at twice the
// bytes each, the same values in the same registers (single 2-byte loads measured 1.2-1.7x the fp32 kernels' time).
// Every thread of the wave must call this (the exchange reads the neighbouring lane).
template <int NB>
__device__ __forceinline__ void gx_ld_col(const bf16* __restrict__ Xc, int64_t N, int m0, int m_hi, bool ok, int pair,
                                          float (&xb)[NB]) {
  if (!pair) {
#pragma unroll
    for (int i = 0; i < NB; ++i) xb[i] = (ok && m0 + i < m_hi) ? aget(Xc + (int64_t)(m0 + i) * N) : 0.f;
    return;
  }
  const int odd = threadIdx.x & 1;
  const bf16* Xe = Xc - odd;   // the even column of the pair
#pragma unroll
  for (int j = 0; j < NB / 2; ++j) {
    // (a row >= m_hi is clamped, not masked — the predicate would differ between the two lanes of a pair; no caller uses
    // the values of such rows)
    const int r = m0 + 2 * j + odd < m_hi ? m0 + 2 * j + odd : m_hi - 1;
    const unsigned w = ok ? *reinterpret_cast<const unsigned*>(Xe + (int64_t)r * N) : 0u;
    const unsigned nb = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
    const unsigned w0 = odd ? nb : w, w1 = odd ? w : nb;   // the words of rows m0 + 2j and m0 + 2j + 1
    xb[2 * j] = __uint_as_float(odd ? (w0 & 0xffff0000u) : (w0 << 16));
    xb[2 * j + 1] = __uint_as_float(odd ? (w1 & 0xffff0000u) : (w1 << 16));
  }
}
// whether the column-local kernels may use word pairs on a bf16 matrix (the fp32 instances ignore it)
inline int gx_pair(const void* p, int64_t N) { return (N % 2 == 0 && reinterpret_cast<uintptr_t>(p) % 4 == 0) ? 1 : 0; }

// stage an R x R matrix of global memory into LDS as RR x RR, zero padded: dst[r][q] = src[r][q], or its transpose
template <int RR>
__device__ __forceinline__ void gx_stage_b(const float* __restrict__ src, int R, float* dst, bool transpose) {
  for (int e = threadIdx.x; e < RR * RR; e += kGxThreads) {
    const int r = e / RR, q = e % RR;
    dst[e] = (r < R && q < R) ? (transpose ? src[q * R + r] : src[r * R + q]) : 0.f;
  }
}
// stage an M x R factor into LDS as M x RR, zero padded
template <int RR>
__device__ __forceinline__ void gx_stage_f(const float* __restrict__ src, int M, int R, float* dst) {
  for (int e = threadIdx.x; e < M * RR; e += kGxThreads) {
    const int m = e / RR, r = e % RR;
    dst[e] = r < R ? src[m * R + r] : 0.f;
  }
}

// ---- w <- update(w; a, b) for one row: update_rows<1, R, SOLVER> of nmf_core.h with b in LDS -------------------------
// sbt[r][q] = b[q][r] (RR x RR, zero padded); w, a zero beyond R.
template <int RR, int SOLVER>
__device__ __forceinline__ void gx_update_row(float (&w)[RR], const float (&a)[RR], const float* __restrict__ sbt, int R,
                                              float eps) {
  if constexpr (SOLVER == SOLVER_MU) {
    float nw[RR];
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      nw[r] = 0.f;
      if (r < R) {
        float bc[RR];
        gx_ldrow<RR>(sbt + r * RR, bc);
        float dn = w[0] * bc[0];
#pragma unroll
        for (int q = 1; q < RR; ++q) dn = dn + w[q] * bc[q];
        nw[r] = (w[r] * a[r] + eps) * fz_rcp(dn + eps);
      }
    }
#pragma unroll
    for (int r = 0; r < RR; ++r) w[r] = nw[r];
  } else {
    if (R == 1) {
      w[0] = fz_relu((a[0] + eps) * fz_rcp(sbt[0] + eps));
      return;
    }
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      if (r < R) {
        float bc[RR];
        gx_ldrow<RR>(sbt + r * RR, bc);
        float s = 0.f;
        bool first = true;
#pragma unroll
        for (int q = 0; q < RR; ++q) {
          if (q == r) continue;
          const float t = w[q] * bc[q];   // columns q < r are already updated (Gauss–Seidel)
          s = first ? t : s + t;
          first = false;
        }
        w[r] = fz_relu((a[r] - s + eps) * fz_rcp(bc[r] + eps));
      }
    }
  }
}

// ---- reverse of one half-step for one row: half_bwd_row of nmf_core.h with b in LDS ----------------------------------
//  in : wold, wnew, a, gwn = dL/dwnew (clobbered); sb[r][q] = b[r][q], sbt[r][q] = b[q][r]
//  out: gwo = dL/dwold, ga = dL/da, gvec = the row's factor of dL/db (MU: gdn, dL/db[q][r] = Σ_rows wold[q] gdn[r];
//       HALS: gnum (= ga), dL/db[q][r] = -Σ_rows (q <= r ? wnew[q] : wold[q]) gnum[r])
template <int RR, int SOLVER>
__device__ __forceinline__ void gx_half_bwd_row(const float (&wold)[RR], const float (&wnew)[RR], const float (&a)[RR],
                                                const float* __restrict__ sb, const float* __restrict__ sbt,
                                                float (&gwn)[RR], float (&gwo)[RR], float (&ga)[RR], float (&gvec)[RR],
                                                int R, float eps) {
  if constexpr (SOLVER == SOLVER_MU) {
    float gn[RR];
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      gn[r] = 0.f;
      gvec[r] = 0.f;
      if (r < R) {
        float bc[RR];
        gx_ldrow<RR>(sbt + r * RR, bc);
        float dn = wold[0] * bc[0];
#pragma unroll
        for (int q = 1; q < RR; ++q) dn = dn + wold[q] * bc[q];
        const float idn = fz_rcp(dn + eps);
        gn[r] = gwn[r] * idn;
        gvec[r] = 0.f - gwn[r] * wnew[r] * idn;
      }
    }
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      gwo[r] = 0.f;
      ga[r] = 0.f;
      if (r < R) {
        float br[RR];
        gx_ldrow<RR>(sb + r * RR, br);
        float t = gn[r] * a[r];
#pragma unroll
        for (int q = 0; q < RR; ++q) t = t + gvec[q] * br[q];
        gwo[r] = t;
        ga[r] = gn[r] * wold[r];
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      gwo[r] = 0.f;
      ga[r] = 0.f;
      gvec[r] = 0.f;
    }
#pragma unroll
    for (int r = RR - 1; r >= 0; --r) {
      if (r < R) {
        float bc[RR];
        gx_ldrow<RR>(sbt + r * RR, bc);
        const float iden = fz_rcp(bc[r] + eps);
        const float gnum = fz_gate(wnew[r], gwn[r]) * iden;
        ga[r] = gnum;
        gvec[r] = gnum;
#pragma unroll
        for (int q = 0; q < RR; ++q) {
          if (q == r) continue;
          if (q < r) gwn[q] = gwn[q] - gnum * bc[q];
          else gwo[q] = gwo[q] - gnum * bc[q];
        }
      }
    }
  }
}

// ---- products that sum over columns ------------------------------------------------------------------------------------
// job: out[row][r] = Σ_n L(row, n) · Rhs[n][r];  L is a row-major rows x N matrix (transposed == 0) or the transpose of
// an N x R factor (transposed == 1: row = factor column).  A job owns whole 64-row chunks, chunk0 = its first.
struct GxJob {
  const void* L;
  const float* Rhs;
  int64_t l_stride, r_stride;   // per matrix (0: shared by all matrices), in elements
  int rows, transposed, out_off, chunk0;
  int l_vec;   // 0: L is fp32.  > 0: L is a bf16 activation matrix, staged l_vec (8, 4, 2, 1) elements per access
};
struct GxProd {
  GxJob job[4];
  int njobs, PE;
};

// rows of a bf16 matrix into the LDS tile, W elements per access (N % W == 0 and the tile starts at a multiple of 128
// columns: an access is all in or all out)
template <int W>
__device__ __forceinline__ void gx_stage_rows(const bf16* __restrict__ Lm, int row0, int nrow, int64_t N, int64_t n0, int nc,
                                              float* xs) {
  constexpr int VPR = kGxTile / W;
  for (int e = threadIdx.x; e < kGxChunk * VPR; e += kGxThreads) {
    const int m = e / VPR, c = (e % VPR) * W;
    float v[W];
#pragma unroll
    for (int i = 0; i < W; ++i) v[i] = 0.f;
    if (m < nrow && c < nc) aload<W>(Lm + (int64_t)(row0 + m) * N + n0 + c, v);
#pragma unroll
    for (int i = 0; i < W; ++i) xs[m * kGxXs + c + i] = v[i];
  }
}

template <int RR, class AT>
__global__ __launch_bounds__(kGxThreads) void gx_prod_kernel(GxProd P, int64_t N, int R, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float xs[4 * kGxChunk * (RR + 1) > kGxChunk * kGxXs ? 4 * kGxChunk * (RR + 1) : kGxChunk * kGxXs];
  __shared__ __attribute__((aligned(16))) float vs[kGxTile * RR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slab = blockIdx.x, nslab = gridDim.x, chunk = blockIdx.y;
  const int64_t mat = blockIdx.z;
  GxJob jb = P.job[0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (j < P.njobs && chunk >= P.job[j].chunk0) jb = P.job[j];
  const int row0 = (chunk - jb.chunk0) * kGxChunk;
  const int nrow = jb.rows - row0 < kGxChunk ? jb.rows - row0 : kGxChunk;
  const float* Lm = static_cast<const float*>(jb.L) + mat * jb.l_stride;
  const float* Rm = jb.Rhs + mat * jb.r_stride;
  const int64_t s0 = (int64_t)slab * kGxSlab;
  const int64_t s1 = s0 + kGxSlab < N ? s0 + kGxSlab : N;

  float acc[RR];
#pragma unroll
  for (int r = 0; r < RR; ++r) acc[r] = 0.f;
  for (int64_t n0 = s0; n0 < s1; n0 += kGxTile) {
    const int nc = s1 - n0 < kGxTile ? (int)(s1 - n0) : kGxTile;
    if (jb.transposed) {
      for (int e = tid; e < kGxTile * R; e += kGxThreads) {
        const int c = e / R, r = e % R;
        xs[r * kGxXs + c] = c < nc ? Lm[(n0 + c) * R + r] : 0.f;
      }
    } else if (sizeof(AT) != sizeof(float) && jb.l_vec > 0) {   // (workgroup-uniform)
      const bf16* Lb = static_cast<const bf16*>(jb.L) + mat * jb.l_stride;
      if (jb.l_vec == 8) gx_stage_rows<8>(Lb, row0, nrow, N, n0, nc, xs);
      else if (jb.l_vec == 4) gx_stage_rows<4>(Lb, row0, nrow, N, n0, nc, xs);
      else if (jb.l_vec == 2) gx_stage_rows<2>(Lb, row0, nrow, N, n0, nc, xs);
      else gx_stage_rows<1>(Lb, row0, nrow, N, n0, nc, xs);
    } else {
      for (int e = tid; e < kGxChunk * kGxTile; e += kGxThreads) {
        const int m = e / kGxTile, c = e % kGxTile;
        xs[m * kGxXs + c] = (m < nrow && c < nc) ? Lm[(int64_t)(row0 + m) * N + n0 + c] : 0.f;
      }
    }
    for (int e = tid; e < kGxTile * RR; e += kGxThreads) {
      const int c = e / RR, r = e % RR;
      vs[e] = (c < nc && r < R) ? Rm[(n0 + c) * R + r] : 0.f;
    }
    __syncthreads();
    const int c0 = wave * (kGxTile / 4);
#pragma unroll 4
    for (int c = c0; c < c0 + kGxTile / 4; ++c) gx_axpy<RR>(acc, xs[lane * kGxXs + c], vs + c * RR);
    __syncthreads();
  }
  // the four waves' column quarters, added in a fixed order
#pragma unroll
  for (int r = 0; r < RR; ++r) xs[(wave * kGxChunk + lane) * (RR + 1) + r] = acc[r];
  __syncthreads();
  float* po = part + (mat * nslab + slab) * P.PE + jb.out_off + row0 * R;
  for (int e = tid; e < nrow * R; e += kGxThreads) {
    const int m = e / R, r = e % R;
    const int i = m * (RR + 1) + r, w = kGxChunk * (RR + 1);
    po[e] = (xs[i] + xs[w + i]) + (xs[2 * w + i] + xs[3 * w + i]);
  }
}

// Σ_slabs part[mat][slab][off + e], slabs in a fixed order (four interleaved running sums, then (0 + 1) + (2 + 3)),
// for the kGxNE elements e0 + i * kGxThreads (those below `lim`) at once: their loads are independent and in flight together
constexpr int kGxNE = 8;
__device__ __forceinline__ void gx_reduce(const float* __restrict__ part, int64_t mat, int nslab, int PE, int off, int e0,
                                          int lim, float (&out)[kGxNE]) {
  const float* p = part + mat * nslab * PE + off + e0;
  float s[kGxNE][4];
#pragma unroll
  for (int i = 0; i < kGxNE; ++i) s[i][0] = s[i][1] = s[i][2] = s[i][3] = 0.f;
  int k = 0;
  for (; k + 4 <= nslab; k += 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < kGxNE; ++i)
        if (e0 + i * kGxThreads < lim) s[i][j] = s[i][j] + p[(int64_t)(k + j) * PE + i * kGxThreads];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (k + j < nslab) {
#pragma unroll
      for (int i = 0; i < kGxNE; ++i)
        if (e0 + i * kGxThreads < lim) s[i][j] = s[i][j] + p[(int64_t)(k + j) * PE + i * kGxThreads];
    }
#pragma unroll
  for (int i = 0; i < kGxNE; ++i) out[i] = (s[i][0] + s[i][1]) + (s[i][2] + s[i][3]);
}

// out[r][q] = Σ_m f[m][r] · g[m][q] for two M x RR factors in LDS (zero padded); thread = (r, four q)
template <int RR>
__device__ __forceinline__ void gx_gram4(const float* __restrict__ f, const float* __restrict__ g, int M, int r, int q4,
                                         float (&o)[4]) {
  o[0] = o[1] = o[2] = o[3] = 0.f;
  for (int m = 0; m < M; ++m) {   // rows in order: reproducible
    const float x = f[m * RR + r];
    const float4 t = *reinterpret_cast<const float4*>(g + m * RR + 4 * q4);
    o[0] = o[0] + x * t.x; o[1] = o[1] + x * t.y; o[2] = o[2] + x * t.z; o[3] = o[3] + x * t.w;
  }
}

// ---- U-update ----------------------------------------------------------------------------------------------------------
// LDS (dynamic): sa[M][RR + 1] | su[M][RR] | sbt[RR][RR]
template <int RR, int SOLVER>
__global__ __launch_bounds__(kGxThreads) void gx_u_kernel(const float* __restrict__ part, int nslab, int M, int R,
                                                          const float* __restrict__ u_prev, int64_t u_prev_stride,
                                                          float* __restrict__ u_new, float* __restrict__ a_hist,
                                                          float* __restrict__ b_hist, float* __restrict__ bu, float eps) {
  extern __shared__ __attribute__((aligned(16))) float fz_lds_gx[];
  constexpr int RP = RR + 1;
  float* su = fz_lds_gx;
  float* sbt = su + M * RR;
  float* sa = sbt + RR * RR;
  const int tid = threadIdx.x;
  const int64_t mat = blockIdx.x;
  const int PE = (M + R) * R;
  for (int e = tid; e < RR * RR; e += kGxThreads) sbt[e] = 0.f;
  __syncthreads();
  for (int e0 = tid; e0 < PE; e0 += kGxNE * kGxThreads) {
    float sv[kGxNE];
    gx_reduce(part, mat, nslab, PE, 0, e0, PE, sv);
#pragma unroll
    for (int i = 0; i < kGxNE; ++i) {
      const int e = e0 + i * kGxThreads;
      if (e >= PE) continue;
      const float s = sv[i];
      const int m = e / R, r = e % R;
      if (m < M) {
        sa[m * RP + r] = s;
        if (a_hist != nullptr) a_hist[mat * M * R + e] = s;
      } else {
        sbt[r * RR + (m - M)] = s;   // b[m - M][r]
        if (b_hist != nullptr) b_hist[mat * R * R + (e - M * R)] = s;
      }
    }
  }
  __syncthreads();
  for (int m = tid; m < M; m += kGxThreads) {
    float w[RR], a[RR];
    gx_ldfac<RR>(u_prev + mat * u_prev_stride + m * R, R, true, w);
#pragma unroll
    for (int r = 0; r < RR; ++r) a[r] = r < R ? sa[m * RP + r] : 0.f;
    gx_update_row<RR, SOLVER>(w, a, sbt, R, eps);
    gx_stfac<RR>(u_new + (mat * M + m) * R, R, w);
#pragma unroll
    for (int r = 0; r < RR; ++r) su[m * RR + r] = w[r];
  }
  __syncthreads();
  // uᵀu of the new u, once for every column slab of the V-update
  if (tid < RR * RR / 4) {
    const int r = tid / (RR / 4), q4 = tid % (RR / 4);
    float o[4];
    gx_gram4<RR>(su, su, M, r, q4, o);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (r < R && 4 * q4 + i < R) bu[mat * R * R + r * R + 4 * q4 + i] = o[i];
  }
}

// ---- V-update (column-local) and y = u vᵀ ------------------------------------------------------------------------------
// rsplit == 1: a workgroup owns 256 columns, one per thread (long N: whole-wave coalesced rows, u staged once per 256
// columns).  rsplit == 4 (N < kGxSplitBelow): a workgroup owns 64 columns and wave w a quarter of the rows: it sums its
// part of a' = Xᵀu, the four parts are added in a fixed order through LDS, every wave then runs the same (cheap) row
// update on the same values and writes its quarter of the rows of y.  A short N (512 columns at M = 512) still gives
// every matrix eight workgroups, and the chain of dependent row loads is a quarter as long.
// LDS (dynamic): su[M][RR] | sbt[RR][RR] | (rsplit == 4) red[4][64][RR + 1].  do_update == 0: v = v_in (a bare
// reconstruction).
constexpr int kGxSplitBelow = 8192;
template <int RR, int SOLVER, int RSPLIT, class AT>
__global__ __launch_bounds__(kGxThreads) void gx_v_kernel(const AT* __restrict__ X, int M, int64_t N, int R,
                                                          const float* __restrict__ u, int64_t u_stride,
                                                          const float* __restrict__ bu, int do_update,
                                                          const float* __restrict__ v_in, int64_t v_in_stride,
                                                          float* __restrict__ v_out, AT* __restrict__ Y, float eps,
                                                          int pair) {
  constexpr int rsplit = RSPLIT;   // a template parameter: the one-thread-per-column form keeps its 57 registers
  extern __shared__ __attribute__((aligned(16))) float fz_lds_gx[];
  constexpr int RP = RR + 1;
  float* su = fz_lds_gx;
  float* sbt = su + M * RR;
  float* red = sbt + RR * RR;
  const int tid = threadIdx.x, cols = kGxThreads / rsplit;
  const int cl = tid % cols, rpart = tid / cols;
  const int64_t mat = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * cols + cl;
  const bool ok = n < N;
  const int Mq = (M + rsplit - 1) / rsplit;
  const int m_lo = rpart * Mq, m_hi = m_lo + Mq < M ? m_lo + Mq : M;
  gx_stage_f<RR>(u + mat * u_stride, M, R, su);
  if (do_update) gx_stage_b<RR>(bu + mat * R * R, R, sbt, true);
  __syncthreads();
  float v[RR];
  gx_ldfac<RR>(v_in + mat * v_in_stride + n * R, R, ok, v);
  const AT* Xc = X + mat * M * N + n;
  if (do_update) {
    float ap[RR];
#pragma unroll
    for (int r = 0; r < RR; ++r) ap[r] = 0.f;
    for (int m0 = m_lo; m0 < m_hi; m0 += 8) {   // 8 row loads in flight
      float xb[8];
      gx_ld_col<8>(Xc, N, m0, m_hi, ok, pair, xb);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (m0 + i < m_hi) gx_axpy<RR>(ap, xb[i], su + (m0 + i) * RR);
    }
    if (rsplit == 4) {
#pragma unroll
      for (int r = 0; r < RR; ++r) red[(rpart * cols + cl) * RP + r] = ap[r];
      __syncthreads();
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        const int i = cl * RP + r, w = cols * RP;
        ap[r] = (red[i] + red[w + i]) + (red[2 * w + i] + red[3 * w + i]);
      }
    }
    gx_update_row<RR, SOLVER>(v, ap, sbt, R, eps);
    if (ok && rpart == 0 && v_out != nullptr) gx_stfac<RR>(v_out + (mat * N + n) * R, R, v);
  }
  if (Y != nullptr && ok) {
    AT* Yc = Y + mat * M * N + n;
    for (int m = m_lo; m < m_hi; ++m) aput(Yc + (int64_t)m * N, gx_dot<RR>(su + m * RR, v));
  }
}

// ---- backward, column-local part -----------------------------------------------------------------------------------------
// One launch = [pending column-local part of the U-update undo of step s+1]  (PEND)
//            + [V-update undo of step s]                                      (VUNDO)
// FIRST (s = T-1): the output layer y = u_T v_Tᵀ feeds gv = gYᵀu_T here (gu = gY v_T is a job of gx_prod_kernel).
// LDS (dynamic): su[M][RR] (u_{s+1}) | sg[M][RR] (pending ga) | sb | sbt (u_{s+1}ᵀu_{s+1}) | sgb (pending gbu + gbuᵀ)
// GXacc: the running fp32 sum of gX between launches (AT == float: GX itself, GXacc unused); the launch without VUNDO is
// the last one of a call and stores GX.
template <int RR, int SOLVER, bool FIRST, bool PEND, bool VUNDO, class AT>
__global__ __launch_bounds__(kGxThreads) void gx_bwd_col_kernel(
    const AT* __restrict__ X, int M, int64_t N, int R, const AT* __restrict__ GY, const float* __restrict__ gv_ext,
    AT* __restrict__ GX, float* __restrict__ GXacc, float* __restrict__ gvbuf, float* __restrict__ gabuf, float* __restrict__ gdbuf,
    const float* __restrict__ ga_p, const float* __restrict__ gbu_p, const float* __restrict__ u_n,
    const float* __restrict__ bu_n, const float* __restrict__ v_old, int64_t v_old_stride,
    const float* __restrict__ v_new, int64_t v_new_stride, float eps, int pair) {
  extern __shared__ __attribute__((aligned(16))) float fz_lds_gx[];
  float* su = fz_lds_gx;
  float* sg = su + M * RR;
  float* sb = sg + M * RR;
  float* sbt = sb + RR * RR;
  float* sgb = sbt + RR * RR;
  const int tid = threadIdx.x;
  const int64_t mat = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * kGxThreads + tid;
  const bool ok = n < N;
  if (FIRST || VUNDO) {
    gx_stage_f<RR>(u_n + mat * M * R, M, R, su);
    gx_stage_b<RR>(bu_n + mat * R * R, R, sb, false);
    gx_stage_b<RR>(bu_n + mat * R * R, R, sbt, true);
  }
  if (PEND) {
    gx_stage_f<RR>(ga_p + mat * M * R, M, R, sg);
    for (int e = tid; e < RR * RR; e += kGxThreads) {
      const int q = e / RR, r = e % RR;
      sgb[e] = (q < R && r < R) ? gbu_p[mat * R * R + q * R + r] + gbu_p[mat * R * R + r * R + q] : 0.f;
    }
  }
  __syncthreads();

  float vn[RR], gv[RR];
  gx_ldfac<RR>(v_new + mat * v_new_stride + n * R, R, ok, vn);   // (stride 0: the broadcast v0 of state 0)
  {
    const float* gp = FIRST ? gv_ext : gvbuf;
    gx_ldfac<RR>(gp != nullptr ? gp + (mat * N + n) * R : nullptr, R, ok && gp != nullptr, gv);
  }
  const AT* Xc = X + mat * M * N + n;
  const AT* GYc = (FIRST && GY != nullptr) ? GY + mat * M * N + n : nullptr;

  // ---- pass A over the rows: everything that must be complete before the per-column undo ----
  float ap[RR];
#pragma unroll
  for (int r = 0; r < RR; ++r) ap[r] = 0.f;
  constexpr int NB = 16;   // row loads in flight
  for (int m0 = 0; m0 < M; m0 += NB) {
    float xb[NB], yb[NB];
    gx_ld_col<NB>(Xc, N, m0, M, ok && (PEND || VUNDO), pair, xb);
    gx_ld_col<NB>(GYc != nullptr ? GYc : Xc, N, m0, M, ok && GYc != nullptr, pair, yb);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      if (m0 + i < M) {
        if (FIRST && GYc != nullptr) gx_axpy<RR>(gv, yb[i], su + (m0 + i) * RR);
        if (PEND) gx_axpy<RR>(gv, xb[i], sg + (m0 + i) * RR);
        if (VUNDO) gx_axpy<RR>(ap, xb[i], su + (m0 + i) * RR);
      }
  }
  if (PEND) {
    // gv_{s+1} += v_{s+1} (gbu + gbuᵀ)   (the old factor of the U-update of step s+1 is v_{s+1}; the sum is symmetric)
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      if (r < R) {
        float br[RR];
        gx_ldrow<RR>(sgb + r * RR, br);
        float acc = gv[r];
#pragma unroll
        for (int q = 0; q < RR; ++q) acc = acc + vn[q] * br[q];
        gv[r] = acc;
      }
    }
  }
  // ---- V-update undo of this column ----
  float gaj[RR];
#pragma unroll
  for (int r = 0; r < RR; ++r) gaj[r] = 0.f;
  if (VUNDO) {
    float vo[RR], gwo[RR], gvec[RR];
    gx_ldfac<RR>(v_old + mat * v_old_stride + n * R, R, ok, vo);
    gx_half_bwd_row<RR, SOLVER>(vo, vn, ap, sb, sbt, gv, gwo, gaj, gvec, R, eps);
    if (ok) {
      gx_stfac<RR>(gvbuf + (mat * N + n) * R, R, gwo);
      gx_stfac<RR>(gabuf + (mat * N + n) * R, R, gaj);
      if (SOLVER == SOLVER_MU) gx_stfac<RR>(gdbuf + (mat * N + n) * R, R, gvec);
    }
  }
  // ---- pass B over the rows: gX ----
  if (!ok) return;
  AT* GXc = GX + mat * M * N + n;
  float* ACCc;   // the running sum
  if constexpr (sizeof(AT) == sizeof(float)) ACCc = reinterpret_cast<float*>(GXc);
  else ACCc = GXacc + mat * M * N + n;
  for (int m0 = 0; m0 < M; m0 += 8) {   // 8 row loads in flight
    float gb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) gb[i] = (!FIRST && m0 + i < M) ? ACCc[(int64_t)(m0 + i) * N] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = m0 + i;
      if (m >= M) continue;
      float acc = gb[i];
      if (PEND) {
        float t[RR];
        gx_ldrow<RR>(sg + m * RR, t);
#pragma unroll
        for (int r = 0; r < RR; ++r) acc = acc + t[r] * vn[r];
      }
      if (VUNDO) {
        float t[RR];
        gx_ldrow<RR>(su + m * RR, t);
#pragma unroll
        for (int r = 0; r < RR; ++r) acc = acc + t[r] * gaj[r];
      }
      if (!VUNDO) aput(GXc + (int64_t)m * N, acc);
      else ACCc[(int64_t)m * N] = acc;
    }
  }
}

// ---- backward, M x R part ------------------------------------------------------------------------------------------------
// gu (dL/du_{s+1}) <- gu + Σ partial(X ga) + u_{s+1}(gb + gbᵀ) with gb from the partial products; then the U-update undo
// of step s: ga (M x R), gbu (R x R) for the column-local part, gu <- dL/du_s.
// partial layout: [X·ga: M x R | P1: R x R | P2: R x R | (FIRST) gY·v_T: M x R]
//   MU: P1 = Woldᵀ·Gdn = dL/db.   HALS: P1 = Wnewᵀ·Gnum, P2 = Woldᵀ·Gnum, dL/db[q][r] = -(q <= r ? P1 : P2)[q][r].
// LDS (dynamic): sgv[M][RR] | sb | sbt | sgs | sp1 | sp2 | sa[M][RR + 1]
template <int RR, int SOLVER, bool FIRST>
__global__ __launch_bounds__(kGxThreads) void gx_bwd_u_kernel(const float* __restrict__ part, int nslab, int M, int R,
                                                              float* __restrict__ gu, const float* __restrict__ gu_ext,
                                                              const float* __restrict__ u_old, int64_t u_old_stride,
                                                              const float* __restrict__ u_new,
                                                              const float* __restrict__ a_s, const float* __restrict__ b_s,
                                                              float* __restrict__ ga, float* __restrict__ gbu, float eps) {
  extern __shared__ __attribute__((aligned(16))) float fz_lds_gx[];
  constexpr int RP = RR + 1;
  float* sgv = fz_lds_gx;
  float* sb = sgv + M * RR;
  float* sbt = sb + RR * RR;
  float* sgs = sbt + RR * RR;
  float* sp1 = sgs + RR * RR;
  float* sp2 = sp1 + RR * RR;
  float* sa = sp2 + RR * RR;
  const int tid = threadIdx.x;
  const int64_t mat = blockIdx.x;
  const int MR = M * R, RQ = R * R;
  const int PE = MR + 2 * RQ + (FIRST ? MR : 0);
  gx_stage_b<RR>(b_s + mat * RQ, R, sb, false);
  gx_stage_b<RR>(b_s + mat * RQ, R, sbt, true);
  for (int e = tid; e < RR * RR; e += kGxThreads) sp1[e] = sp2[e] = 0.f;
  __syncthreads();
  for (int e0 = tid; e0 < MR; e0 += kGxNE * kGxThreads) {
    float sx[kGxNE], s0[kGxNE];
    gx_reduce(part, mat, nslab, PE, 0, e0, MR, sx);
    if (FIRST) gx_reduce(part, mat, nslab, PE, MR + 2 * RQ, e0, MR, s0);
#pragma unroll
    for (int i = 0; i < kGxNE; ++i) {
      const int e = e0 + i * kGxThreads;
      if (e >= MR) continue;
      float base;
      if (FIRST) base = s0[i] + (gu_ext != nullptr ? gu_ext[mat * MR + e] : 0.f);
      else base = gu[mat * MR + e];
      sa[(e / R) * RP + e % R] = base + sx[i];
    }
  }
  const int NP = SOLVER == SOLVER_MU ? RQ : 2 * RQ;   // (MU has no P2)
  for (int e0 = tid; e0 < NP; e0 += kGxNE * kGxThreads) {
    float sv[kGxNE];
    gx_reduce(part, mat, nslab, PE, MR, e0, NP, sv);
#pragma unroll
    for (int i = 0; i < kGxNE; ++i) {
      const int e = e0 + i * kGxThreads;
      if (e >= NP) continue;
      const int j = e % RQ;
      (e < RQ ? sp1 : sp2)[(j / R) * RR + j % R] = sv[i];
    }
  }
  __syncthreads();
  for (int e = tid; e < RR * RR; e += kGxThreads) {
    const int q = e / RR, r = e % RR;
    float gqr, grq;
    if (SOLVER == SOLVER_MU) {
      gqr = sp1[q * RR + r];
      grq = sp1[r * RR + q];
    } else {
      gqr = 0.f - (q <= r ? sp1[q * RR + r] : sp2[q * RR + r]);
      grq = 0.f - (r <= q ? sp1[r * RR + q] : sp2[r * RR + q]);
    }
    sgs[e] = gqr + grq;
  }
  __syncthreads();
  for (int m = tid; m < M; m += kGxThreads) {
    float un[RR], uo[RR], as[RR], gwn[RR], gwo[RR], gam[RR], gvec[RR];
    gx_ldfac<RR>(u_new + (mat * M + m) * R, R, true, un);
    gx_ldfac<RR>(u_old + mat * u_old_stride + m * R, R, true, uo);
    gx_ldfac<RR>(a_s + (mat * M + m) * R, R, true, as);
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      gwn[r] = 0.f;
      if (r < R) {
        float br[RR];
        gx_ldrow<RR>(sgs + r * RR, br);   // symmetric
        float acc = sa[m * RP + r];
#pragma unroll
        for (int q = 0; q < RR; ++q) acc = acc + un[q] * br[q];
        gwn[r] = acc;
      }
    }
    gx_half_bwd_row<RR, SOLVER>(uo, un, as, sb, sbt, gwn, gwo, gam, gvec, R, eps);
    gx_stfac<RR>(ga + (mat * M + m) * R, R, gam);
    gx_stfac<RR>(gu + (mat * M + m) * R, R, gwo);
#pragma unroll
    for (int r = 0; r < RR; ++r) sgv[m * RR + r] = gvec[r];
  }
  __syncthreads();
  // gbu = dL/db of this U-update: rows in order
  if (tid < RR * RR / 4) {
    const int q = tid / (RR / 4), r4 = tid % (RR / 4);
    if (q < R) {
      float on[4] = {0.f, 0.f, 0.f, 0.f}, oo[4] = {0.f, 0.f, 0.f, 0.f};
      const float* pn = u_new + mat * MR + q;
      const float* po = u_old + mat * u_old_stride + q;
      for (int m = 0; m < M; ++m) {
        const float4 t = *reinterpret_cast<const float4*>(sgv + m * RR + 4 * r4);
        const float xo = po[m * R];
        oo[0] = oo[0] + xo * t.x; oo[1] = oo[1] + xo * t.y; oo[2] = oo[2] + xo * t.z; oo[3] = oo[3] + xo * t.w;
        if (SOLVER != SOLVER_MU) {
          const float xn = pn[m * R];
          on[0] = on[0] + xn * t.x; on[1] = on[1] + xn * t.y; on[2] = on[2] + xn * t.z; on[3] = on[3] + xn * t.w;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * r4 + i;
        if (r < R) gbu[mat * RQ + q * R + r] = SOLVER == SOLVER_MU ? oo[i] : 0.f - (q <= r ? on[i] : oo[i]);
      }
    }
  }
}

// ---- workspace layout (floats) -------------------------------------------------------------------------------------------
struct GxWs {
  int64_t uh, vh, ah, bh, buh, part, gvbuf, gabuf, gdbuf, gu, ga, gbu, gxacc, total;
};
inline int gx_nslab(int64_t N) { return (int)((N + kGxSlab - 1) / kGxSlab); }
// acc: the fp32 running sum of gX that a backward on 16-bit activations needs (last, so nothing else moves)
inline GxWs gx_layout(int64_t nmat, int M, int64_t N, int R, int T, bool backward, bool acc) {
  GxWs w;
  WsTake take;
  const int Tn = T > 0 ? T : 1;
  const int64_t MR = (int64_t)M * R, NR = N * R, RQ = (int64_t)R * R;
  w.uh = take((int64_t)Tn * nmat * MR);                       // u_1..u_T
  w.vh = take((backward ? (int64_t)Tn : 2) * nmat * NR);      // v_1..v_T (or a ping-pong pair)
  w.ah = take((backward ? (int64_t)Tn : 0) * nmat * MR);
  w.bh = take((backward ? (int64_t)Tn : 0) * nmat * RQ);
  w.buh = take((backward ? (int64_t)Tn : 1) * nmat * RQ);     // u_tᵀu_t
  w.part = take(nmat * gx_nslab(N) * (2 * MR + 2 * RQ));
  w.gvbuf = take(backward ? nmat * NR : 0);
  w.gabuf = take(backward ? nmat * NR : 0);
  w.gdbuf = take(backward ? nmat * NR : 0);
  w.gu = take(backward ? nmat * MR : 0);
  w.ga = take(backward ? nmat * MR : 0);
  w.gbu = take(backward ? nmat * RQ : 0);
  w.gxacc = take(backward && acc ? nmat * (int64_t)M * N : 0);
  w.total = take.o;
  return w;
}

template <class AT>
struct GxCall {
  const AT* x;
  const float *u0, *v0;
  int64_t nmat;
  int M;
  int64_t N;
  int R, T;
  float eps;
  float* ws;
  hipStream_t st;
  int pair;   // gx_pair of every activation matrix the column-local kernels load (x, gy)
};

inline int gx_chunks(int rows) { return (rows + kGxChunk - 1) / kGxChunk; }
inline void gx_add_job(GxProd& P, int& chunks, const float* L, int64_t l_stride, int transposed, int rows,
                       const float* Rhs, int64_t r_stride, int out_off) {
  P.job[P.njobs++] = GxJob{L, Rhs, l_stride, r_stride, rows, transposed, out_off, chunks, 0};
  chunks += gx_chunks(rows);
}
// a job whose rows are a bf16 activation matrix (rows x N): the access width follows its real alignment and N
inline void gx_add_job(GxProd& P, int& chunks, const bf16* L, int64_t l_stride, int transposed, int rows,
                       const float* Rhs, int64_t r_stride, int out_off) {
  const int64_t N = l_stride / rows;
  const uintptr_t a = reinterpret_cast<uintptr_t>(L);
  const int vec = (N % 8 == 0 && a % 16 == 0) ? 8 : (N % 4 == 0 && a % 8 == 0) ? 4 : (N % 2 == 0 && a % 4 == 0) ? 2 : 1;
  P.job[P.njobs++] = GxJob{L, Rhs, l_stride, r_stride, rows, transposed, out_off, chunks, vec};
  chunks += gx_chunks(rows);
}

template <int RR, class AT>
static int gx_prod(const GxCall<AT>& c, const GxProd& P, int chunks, float* part) {
  hipLaunchKernelGGL((gx_prod_kernel<RR, AT>), dim3(gx_nslab(c.N), chunks, (unsigned)c.nmat), dim3(kGxThreads), 0, c.st, P, c.N,
                     c.R, part);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

template <class K>
static int gx_lds(K kern, size_t bytes) {
  if (bytes > 64 * 1024)
    FZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return FZ_OK;
}
#define FZ_GX_TRY(expr)          \
  do {                           \
    const int rc__ = (expr);     \
    if (rc__ != FZ_OK) return rc__; \
  } while (0)

template <int RR, int SOLVER, class AT>
static int gx_forward_t(const GxCall<AT>& c, const GxWs& L, bool hist, AT* y, float* u_out, float* v_out) {
  const int R = c.R, M = c.M;
  const int64_t MR = (int64_t)M * R, NR = c.N * R, RQ = (int64_t)R * R;
  const int rsplit = c.N < kGxSplitBelow ? 4 : 1, vcols = kGxThreads / rsplit;
  const dim3 block(kGxThreads), vgrid((unsigned)((c.N + vcols - 1) / vcols), (unsigned)c.nmat);
  const size_t v_lds = sizeof(float) * ((size_t)M * RR + RR * RR + (rsplit == 4 ? kGxThreads * (RR + 1) : 0));
  const size_t u_lds = sizeof(float) * ((size_t)M * (2 * RR + 1) + RR * RR);
  FZ_GX_TRY(rsplit == 4 ? gx_lds(gx_v_kernel<RR, SOLVER, 4, AT>, v_lds) : gx_lds(gx_v_kernel<RR, SOLVER, 1, AT>, v_lds));
#define FZ_GX_V(...)                                                                                      \
  do {                                                                                                    \
    if (rsplit == 4) hipLaunchKernelGGL((gx_v_kernel<RR, SOLVER, 4, AT>), vgrid, block, v_lds, c.st, __VA_ARGS__, c.pair); \
    else hipLaunchKernelGGL((gx_v_kernel<RR, SOLVER, 1, AT>), vgrid, block, v_lds, c.st, __VA_ARGS__, c.pair);     \
    FZ_LAUNCH_CHECK();                                                                                    \
  } while (0)
  FZ_GX_TRY(gx_lds(gx_u_kernel<RR, SOLVER>, u_lds));
  float* part = c.ws + L.part;
  auto U = [&](int t) { return c.ws + L.uh + (int64_t)(t - 1) * c.nmat * MR; };                       // t = 1..T
  auto V = [&](int t) { return c.ws + L.vh + (int64_t)(hist ? t - 1 : (t & 1)) * c.nmat * NR; };      // t = 1..T
  auto BU = [&](int t) { return c.ws + L.buh + (int64_t)(hist ? t - 1 : 0) * c.nmat * RQ; };
  if (c.T == 0) {  // y = u0 v0ᵀ
    FZ_GX_V(c.x, M, c.N, R, c.u0, (int64_t)0, (const float*)nullptr, 0, c.v0, (int64_t)0, (float*)nullptr, y, c.eps);
    return FZ_OK;
  }
  for (int t = 1; t <= c.T; ++t) {
    // partial sums of X v_{t-1}, v_{t-1}ᵀ v_{t-1}: the stacked rows [X; Vᵀ] times V
    const float* vp = t == 1 ? c.v0 : V(t - 1);
    const int64_t vps = t == 1 ? 0 : NR;
    GxProd P{};
    int chunks = 0;
    P.PE = (int)(MR + RQ);
    gx_add_job(P, chunks, c.x, (int64_t)M * c.N, 0, M, vp, vps, 0);
    gx_add_job(P, chunks, vp, vps, 1, R, vp, vps, (int)MR);
    FZ_GX_TRY((gx_prod<RR, AT>(c, P, chunks, part)));
    const float* up = t == 1 ? c.u0 : U(t - 1);
    float* un = (t == c.T && u_out != nullptr) ? u_out : U(t);
    hipLaunchKernelGGL((gx_u_kernel<RR, SOLVER>), dim3((unsigned)c.nmat), block, u_lds, c.st, (const float*)part,
                       gx_nslab(c.N), M, R, up, (int64_t)(t == 1 ? 0 : MR), un,
                       hist ? c.ws + L.ah + (int64_t)(t - 1) * c.nmat * MR : (float*)nullptr,
                       hist ? c.ws + L.bh + (int64_t)(t - 1) * c.nmat * RQ : (float*)nullptr, BU(t), c.eps);
    FZ_LAUNCH_CHECK();
    float* vn = (t == c.T && v_out != nullptr) ? v_out : V(t);
    FZ_GX_V(c.x, M, c.N, R, (const float*)un, MR, (const float*)BU(t), 1, vp, vps, vn, t == c.T ? y : (AT*)nullptr,
            c.eps);
  }
#undef FZ_GX_V
  return FZ_OK;
}

template <int RR, int SOLVER, class AT>
static int gx_backward_t(const GxCall<AT>& c, const GxWs& L, int G, const AT* gy, const float* gu_ext, const float* gv_ext,
                         AT* gx) {
  FZ_GX_TRY((gx_forward_t<RR, SOLVER, AT>(c, L, true, nullptr, nullptr, nullptr)));
  const int R = c.R, M = c.M;
  const int64_t MR = (int64_t)M * R, NR = c.N * R, RQ = (int64_t)R * R, XS = (int64_t)M * c.N;
  const dim3 block(kGxThreads), cgrid((unsigned)((c.N + kGxThreads - 1) / kGxThreads), (unsigned)c.nmat);
  const size_t c_lds = sizeof(float) * ((size_t)2 * M * RR + 3 * RR * RR);
  const size_t u_lds = sizeof(float) * ((size_t)M * (2 * RR + 1) + 5 * RR * RR);
  FZ_GX_TRY(gx_lds(gx_bwd_col_kernel<RR, SOLVER, true, false, true, AT>, c_lds));
  FZ_GX_TRY(gx_lds(gx_bwd_col_kernel<RR, SOLVER, false, true, true, AT>, c_lds));
  FZ_GX_TRY(gx_lds(gx_bwd_col_kernel<RR, SOLVER, false, true, false, AT>, c_lds));
  FZ_GX_TRY(gx_lds(gx_bwd_u_kernel<RR, SOLVER, true>, u_lds));
  FZ_GX_TRY(gx_lds(gx_bwd_u_kernel<RR, SOLVER, false>, u_lds));
  float* part = c.ws + L.part;
  float* gvbuf = c.ws + L.gvbuf;
  float* gabuf = c.ws + L.gabuf;
  float* gdbuf = c.ws + L.gdbuf;
  float* gu = c.ws + L.gu;
  float* ga = c.ws + L.ga;
  float* gbu = c.ws + L.gbu;
  float* gxacc = c.ws + L.gxacc;   // (fp32 activations: unused, the sum runs in gx)
  auto U = [&](int t) { return t == 0 ? c.u0 : c.ws + L.uh + (int64_t)(t - 1) * c.nmat * MR; };
  auto V = [&](int t) { return t == 0 ? c.v0 : c.ws + L.vh + (int64_t)(t - 1) * c.nmat * NR; };
  auto BU = [&](int t) { return c.ws + L.buh + (int64_t)(t - 1) * c.nmat * RQ; };   // t = 1..T
#define FZ_GX_COL(FI, PE_, VU, ...)                                                                                    \
  do {                                                                                                                 \
    hipLaunchKernelGGL((gx_bwd_col_kernel<RR, SOLVER, FI, PE_, VU, AT>), cgrid, block, c_lds, c.st, __VA_ARGS__, c.pair); \
    FZ_LAUNCH_CHECK();                                                                                                 \
  } while (0)
  for (int s = c.T - 1; s >= c.T - G; --s) {
    const bool first = s == c.T - 1;
    const int64_t vos = s == 0 ? 0 : NR;
    // state s+1 = (U(s+1), V(s+1)), state s = (U(s), V(s)); a_s, b_s recorded by the U-update of step s
    if (first)
      FZ_GX_COL(true, false, true, c.x, M, c.N, R, gy, gv_ext, gx, gxacc, gvbuf, gabuf, gdbuf, (const float*)nullptr,
                (const float*)nullptr, U(s + 1), (const float*)BU(s + 1), V(s), vos, V(s + 1), NR, c.eps);
    else
      FZ_GX_COL(false, true, true, c.x, M, c.N, R, (const AT*)nullptr, (const float*)nullptr, gx, gxacc, gvbuf, gabuf, gdbuf,
                (const float*)ga, (const float*)gbu, U(s + 1), (const float*)BU(s + 1), V(s), vos, V(s + 1), NR, c.eps);
    GxProd P{};
    int chunks = 0;
    P.PE = (int)(MR + 2 * RQ + (first ? MR : 0));
    gx_add_job(P, chunks, c.x, XS, 0, M, gabuf, NR, 0);
    if (SOLVER == SOLVER_MU) {
      gx_add_job(P, chunks, V(s), vos, 1, R, gdbuf, NR, (int)MR);
    } else {
      gx_add_job(P, chunks, V(s + 1), NR, 1, R, gabuf, NR, (int)MR);
      gx_add_job(P, chunks, V(s), vos, 1, R, gabuf, NR, (int)(MR + RQ));
    }
    if (first && gy != nullptr) gx_add_job(P, chunks, gy, XS, 0, M, V(s + 1), NR, (int)(MR + 2 * RQ));
    if (first && gy == nullptr) {
      // no gY (gradients of `decompose`): no job writes the gY·v_T slot that gx_bwd_u_kernel sums: it must read as zero
      FZ_HIP_OK(hipMemsetAsync(part, 0, sizeof(float) * c.nmat * gx_nslab(c.N) * P.PE, c.st));
    }
    FZ_GX_TRY((gx_prod<RR, AT>(c, P, chunks, part)));
    const float* as = c.ws + L.ah + (int64_t)s * c.nmat * MR;
    const float* bs = c.ws + L.bh + (int64_t)s * c.nmat * RQ;
    if (first)
      hipLaunchKernelGGL((gx_bwd_u_kernel<RR, SOLVER, true>), dim3((unsigned)c.nmat), block, u_lds, c.st, (const float*)part,
                         gx_nslab(c.N), M, R, gu, gu_ext, U(s), (int64_t)(s == 0 ? 0 : MR), U(s + 1), as, bs, ga, gbu, c.eps);
    else
      hipLaunchKernelGGL((gx_bwd_u_kernel<RR, SOLVER, false>), dim3((unsigned)c.nmat), block, u_lds, c.st, (const float*)part,
                         gx_nslab(c.N), M, R, gu, (const float*)nullptr, U(s), (int64_t)(s == 0 ? 0 : MR), U(s + 1), as, bs,
                         ga, gbu, c.eps);
    FZ_LAUNCH_CHECK();
  }
  // column-local part of the last U-update undo (step T-G): gX += ga v_{T-G}ᵀ
  const int s0 = c.T - G;
  FZ_GX_COL(false, true, false, c.x, M, c.N, R, (const AT*)nullptr, (const float*)nullptr, gx, gxacc, gvbuf, gabuf, gdbuf,
            (const float*)ga, (const float*)gbu, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
            (int64_t)0, V(s0), (int64_t)(s0 == 0 ? 0 : NR), c.eps);
#undef FZ_GX_COL
  return FZ_OK;
}

// ---- one validated call (wide_fwd_entry / wide_bwd_entry of nmf_wide.h have checked every argument) -------------------

#define FZ_GX_RANKS(CALL, SS)                  \
  do {                                         \
    if (a.R <= 8) return CALL(8, SS);          \
    if (a.R <= 16) return CALL(16, SS);        \
    if (a.R <= 24) return CALL(24, SS);        \
    return CALL(32, SS);                       \
  } while (0)

template <class AT>
static int gx_run_fwd(const WideArgs& a) {
  const GxWs L = gx_layout(a.nmat, a.M, a.N, a.R, a.T, false, false);
  const GxCall<AT> c{(const AT*)a.x, a.u0, a.v0, a.nmat, a.M, a.N, a.R, a.T, a.eps, (float*)a.ws, (hipStream_t)a.stream,
                     gx_pair(a.x, a.N)};
#define FZ_GX_F(RR, SS) gx_forward_t<RR, SS, AT>(c, L, false, (AT*)a.y, a.u_out, a.v_out)
  if (a.solver == FZ_SOLVER_MU) FZ_GX_RANKS(FZ_GX_F, SOLVER_MU);
  FZ_GX_RANKS(FZ_GX_F, SOLVER_HALS);
#undef FZ_GX_F
}

template <class AT>
static int gx_run_bwd(const WideArgs& a) {
  const GxWs L = gx_layout(a.nmat, a.M, a.N, a.R, a.T, true, sizeof(AT) != sizeof(float));
  const GxCall<AT> c{(const AT*)a.x, a.u0, a.v0, a.nmat, a.M, a.N, a.R, a.T, a.eps, (float*)a.ws, (hipStream_t)a.stream,
                     gx_pair(a.x, a.N) & gx_pair(a.gy, a.N)};
#define FZ_GX_B(RR, SS) gx_backward_t<RR, SS, AT>(c, L, a.G, (const AT*)a.gy, a.gu, a.gv, (AT*)a.gx)
  if (a.solver == FZ_SOLVER_MU) FZ_GX_RANKS(FZ_GX_B, SOLVER_MU);
  FZ_GX_RANKS(FZ_GX_B, SOLVER_HALS);
#undef FZ_GX_B
}
#undef FZ_GX_RANKS

// the bf16 instances (nmf_global_rank_bf16.hip)
int gx_fwd_bf16(const WideArgs& a);
int gx_bwd_bf16(const WideArgs& a);

}  // namespace fz
