// gemm_shared.h — what more than one unit of the fp32-MFMA GEMM family uses (gemm.hip, gemm_p32.hip, the mlp_chain*.hip
// units, gemm_dw.hip):
// the LayerNorm-backward epilogue, the block-dropout arguments, the transposable-tile constants, the knob reader and the
// launchers through which fz_gemm's dispatcher reaches gemm_p32_kernel and the chain kernels.
#pragma once
#include "gemm_common.h"

namespace fz {

// ---- LayerNorm-backward epilogue (M == 32, one row block) ------------------------------------------
// acc[q][r] = gl[row (r,h)][voxel 4j+q].  Everything stays in registers: the channel means are
// sums over the 16 registers + the other lane half; the affine gradients are reduced over the
// 32 lanes of each half on the DPP network, then over the 4 waves through LDS.
__device__ __forceinline__ float half_sum32(float v) {
  v += dpp_take<0xB1, 0xf>(v);   // xor 1
  v += dpp_take<0x4E, 0xf>(v);   // xor 2
  v += dpp_take<0x141, 0xf>(v);  // row_half_mirror
  v += dpp_take<0x140, 0xf>(v);  // row_mirror  -> 16-lane row totals in every lane
  v += dpp_take<0x142, 0xa>(v);  // row_bcast15: rows 1,3 += rows 0,2  -> lanes 16-31 / 48-63 hold the half totals
  return v;
}

template <int NACC, bool GADD, bool GADD_LDS = false, typename AT = float>
__device__ __forceinline__ void lnbwd_block(const GemmArgsT<AT>& p, const f32x16 (&acc)[NACC], int b, int64_t ncol,
                                            bool col_ok, int lane, int wave, float* red /* [4][64] */,
                                            int64_t part_row, const float* g_lds /* gamma[32] in LDS */,
                                            const float* gadd_lds = nullptr /* [32][32*NACC] tile of lnb_gadd */) {
  const int h = lane >> 5;
  const int64_t nc = col_ok ? ncol : 0;
  // row = rbase(r) + 4h: the row part of every address is wave-uniform (scalar base) and ONE
  // 32-bit per-lane offset serves the 16 rows (global_load saddr + voffset; the host bounds Ncol so
  // that 20*Ncol bytes fit) — per-row 64-bit lane addresses cost a VGPR pair per load in flight
  const unsigned lane_off = (unsigned)(4 * h) * (unsigned)p.Ncol + (unsigned)nc;
  const int64_t sample = (int64_t)b * 32 * p.Ncol;
  const float* sp = p.lnb_stats + (int64_t)b * 2 * p.Ncol;
  float mu[NACC], rs[NACC];
  vload<NACC>(sp + nc, mu);
  vload<NACC>(sp + p.Ncol + nc, rs);
  __builtin_amdgcn_sched_barrier(0);  // do not hoist the x loads above the MFMA loop (operand regs still live)
  float xs[16][NACC];  // LayerNorm input rows of this lane (the only big live array besides acc)
  float m1[NACC], m2[NACC];
#pragma unroll
  for (int q = 0; q < NACC; ++q) m1[q] = m2[q] = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rbase = (r & 3) + 8 * (r >> 2);
    vload<NACC>(p.lnb_x + sample + (int64_t)rbase * p.Ncol + lane_off, xs[r]);
  }
  // the added gradient is fetched here, unconditionally and all rows at once: a load behind a
  // runtime `if` inside the row loop compiles to load → s_waitcnt vmcnt(0) per row (16 exposed
  // round trips per tile)
  // (with GADD_LDS the tile is already in LDS: read per row below, no registers held)
  float ga[(GADD && !GADD_LDS) ? 16 : 1][NACC];
  if (GADD && !GADD_LDS) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rbase = (r & 3) + 8 * (r >> 2);
      vload<NACC>(p.lnb_gadd + sample + (int64_t)rbase * p.Ncol + lane_off, ga[(GADD && !GADD_LDS) ? r : 0]);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
    const float gc = g_lds[row];  // (a global load here is a dependent L2 round trip per row)
#pragma unroll
    for (int q = 0; q < NACC; ++q) {
      const float av = acc[q][r] * gc;
      xs[r][q] = (xs[r][q] - mu[q]) * rs[q];  // normalised input, reused below
      m1[q] += av;
      m2[q] += av * xs[r][q];
    }
    __builtin_amdgcn_sched_barrier(0);  // keep rows from interleaving (register pressure)
  }
#pragma unroll
  for (int q = 0; q < NACC; ++q) {
    m1[q] = (m1[q] + __shfl_xor(m1[q], 32, 64)) * (1.0f / 32.0f);
    m2[q] = (m2[q] + __shfl_xor(m2[q], 32, 64)) * (1.0f / 32.0f);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rbase = (r & 3) + 8 * (r >> 2);
    const int row = rbase + 4 * h;
    const int64_t so = sample + (int64_t)rbase * p.Ncol;  // uniform
    const float gc = g_lds[row];  // (a global load here is a dependent L2 round trip per row)
    float v[NACC], nhr[NACC], gl[NACC];
    if (GADD && GADD_LDS) vload<NACC>(gadd_lds + row * (32 * NACC) + NACC * (lane & 31), gl);
#pragma unroll
    for (int q = 0; q < NACC; ++q) {
      nhr[q] = xs[r][q];
      v[q] = rs[q] * (acc[q][r] * gc - m1[q] - nhr[q] * m2[q]);
    }
    if (GADD) {
#pragma unroll
      for (int q = 0; q < NACC; ++q) v[q] += GADD_LDS ? gl[q] : ga[(GADD && !GADD_LDS) ? r : 0][q];
    }
    if (col_ok) vstore<NACC>(p.y + so + lane_off, v);
    // affine-gradient partials of this row over the wave's 32*NACC voxels
    float sg = 0.f, sb = 0.f;
    if (col_ok) {
#pragma unroll
      for (int q = 0; q < NACC; ++q) {
        sg += acc[q][r] * nhr[q];
        sb += acc[q][r];
      }
    }
    sg = half_sum32(sg);
    sb = half_sum32(sb);
    if ((lane & 31) == 31) {
      red[wave * 64 + row] = sg;
      red[wave * 64 + 32 + row] = sb;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int e = threadIdx.x;
    p.lnb_part[part_row * 64 + e] = (red[e] + red[64 + e]) + (red[128 + e] + red[192 + e]);
  }
}

// Block dropout inside the fused launches (csrc/dropout.hip has the contract): keep-bit planes (B, ch, nw) of sites 0..2, bit v & 31
// of word v >> 5 of row (b, ch); a null plane keeps everything.  The dropout forms are separate instantiations of the kernels with
// ONE trailing DropArgs argument (DROP = a non-empty parameter pack): the p = 0 instantiations keep their argument list and code.
struct DropArgs {
  const uint32_t* m[3];   // site 0: out_proj output, site 1: gelu(z1), site 2: fc2 output (C = 32 / hidden 64 / C = 32 channels)
  float s[3];             // 1 / (1 - p)
  int64_t nw;             // words per row: ceil(V / 32)
};
// the keep bits of voxels v, v + 1, ... (v even, NACC <= 2: one word) of row `row` of sample b in a plane of `ch` rows, shifted
// down to bit 0; all ones when the site is not live
__device__ __forceinline__ uint32_t drop_bits(const DropArgs& d, int site, int b, int ch, int row, int64_t v) {
  const uint32_t* m = d.m[site];
  if (m == nullptr) return ~0u;
  return m[((int64_t)b * ch + row) * d.nw + (v >> 5)] >> (v & 31);
}
__device__ __forceinline__ DropArgs drop_of() { return DropArgs{}; }
__device__ __forceinline__ DropArgs drop_of(const DropArgs& d) { return d; }
__device__ __forceinline__ float drop_f(const DropArgs& d, int site, uint32_t bits, int q, float v) {
  return ((bits >> q) & 1u) ? v * d.s[site] : 0.f;
}

// host: the argument of a dropout launch, and the check of a scale that a caller passes
static DropArgs drop_args(const uint32_t* m0, const uint32_t* m1, const uint32_t* m2, float s0, float s1, float s2, int64_t V) {
  DropArgs a;
  a.m[0] = m0; a.m[1] = m1; a.m[2] = m2;
  a.s[0] = m0 ? s0 : 1.f; a.s[1] = m1 ? s1 : 1.f; a.s[2] = m2 ? s2 : 1.f;   // (a site without a plane keeps its values)
  a.nw = (V + 31) / 32;
  return a;
}
static bool drop_scale_ok(const void* m, float s) { return m == nullptr || (s >= 1.f && s < 3.0e38f); }

// gemm_chain_bwd_wg_kernel (mlp_chain_wg.hip) and gemm_dw_kernel (gemm_dw.hip): accumulator of their 16x16 weight-gradient MFMAs, and
// the row stride of the LDS tiles they turn their operands through
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kTS = 66;                       // LDS row stride of the transposable tiles (floats): ≡ 2 (mod 32), even

// Diagnostic environment knobs are read ONCE per process and validated (> 0): the row count that sizes a caller's
// workspace and the grid of the launch that fills it can then never disagree, and an empty / zero value cannot produce
// a zero-sized grid.
// (probe builds only: FZ_KNOB is a compile-time "unset" in the shipped library — fz_common.h)
static int knob_pos(const EnvKnob& k, int dflt) { return k.set && k.val > 0 ? k.val : dflt; }

// fz_gemm, 32 -> 32 without a residual at stage-0 sizes: gemm_p32_kernel (gemm_p32.hip)
template <typename AT>
int gemm_p32_launch(const fz_gemm_desc* d, const GemmArgsT<AT>& a, fz_stream_t stream);

// fz_gemm with EPI_LNBWD and M = K = 64: gemm_chain64_kernel, SINGLE form (mlp_chain64.hip)
template <typename AT>
int chain64_lnb_launch(const fz_gemm_desc* d, const GemmArgsT<AT>& a, fz_stream_t stream);

}  // namespace fz
