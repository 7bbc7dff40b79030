// nmf_cf_gram.hip — backward of the fused FactMixer core for HALS rank 1 behind a ReLU, in the row space (nmf_gram.h).
// Replaces autograd through SWMatricize.forward → NMF(rank 1, "hals") → SWMatricize.inverse_forward
// (factorizer/factorizer.py:41-50; operations.py:417-434; factorization/matrix_factorization.py:210-229,506-533).
//
// relu_gate = 1 promises t = relu(z) >= 0 (factorizer.py:44), which is what lets the iteration be carried by K = X Xᵀ:
// 2 450 instead of 3 600 vector instructions per matrix and no per-column history in LDS (12.7 KB per wave in the general
// kernel: two workgroups per CU).  dL/dY is consumed row by row as it comes out of the exchange, dL/dX is produced row by
// row into it — neither ever occupies 64 registers next to X: <= 168 registers, three workgroups of four waves per CU.
// Same tile / exchange / store scheme as cf_bwd_tile_body (nmf_cf_bwd.hip).
//
// What the launch is bound by (tools/probes/gram_floor.sh, profiles/r05_gram_floor.md): with the arithmetic compiled out
// (-DFZ_PROBE_GRAM_NOMATH: loads, exchanges, stores) it takes 345-357 us for window 0 and 485-493 us for window 1 at stage
// 0, the full kernel 360-370 / 478-487 — the tile's memory skeleton, not the wave program, is what the time is.  Variants
// of how the reads are requested that did not change it: channels 4-7 of dL/da and of the running sum by LDS-DMA
// (global_load_lds_dwordx4 into a swizzled 32 KB image, everything in flight from kernel start), two or three waves per
// SIMD.  Channel planes 4 KiB further apart than the dense 8 MiB: window 0 -10 %.
//
// MODE: CFG_HALVES (fp32) — dL/da four channels at a time through 32 registers, channels 0-3 requested once the 52 partial
// sums of K and s are reduced, 4-7 when 0-3 have left for the exchange; CFG_RAW (bf16 storage) — a lane's four elements are
// 8 bytes: all 8 channels as raw pairs in 32 registers at once.
#include "nmf_cf.h"
#include "nmf_gram.h"

#ifndef FZ_GRAM_WAVES
#define FZ_GRAM_WAVES 3
#endif

namespace fz {

enum { CFG_HALVES = 0, CFG_RAW = 2 };

#ifdef FZ_PROBE_GRAM_NOMATH
#define FZ_GRAM_OUT_ROW(m, grow) probe_acc += grow[(m) & 7]
#else
#define FZ_GRAM_OUT_ROW(m, grow) P.out_row(m, grow)
#endif

// 4 consecutive elements as they lie in memory (no conversion): float4 for fp32, two dwords for bf16
template <typename AT> struct CfRaw;
template <> struct CfRaw<float> { using T = float4; };
template <> struct CfRaw<bf16> { using T = uint2; };

template <bool HALF>
__device__ __forceinline__ float4 cf_ld_raw(const float* p, unsigned o, unsigned o2) { return cf_ld4<HALF>(p, o, o2); }
template <bool HALF>
__device__ __forceinline__ uint2 cf_ld_raw(const bf16* p, unsigned o, unsigned o2) {
  if (HALF) {
    const unsigned a = *reinterpret_cast<const unsigned*>(cf_at(p, o)), b = *reinterpret_cast<const unsigned*>(cf_at(p, o2));
    return make_uint2(a, b);
  }
  return *reinterpret_cast<const uint2*>(cf_at(p, o));
}
__device__ __forceinline__ float4 cf_raw_f4(const float4& v) { return v; }
__device__ __forceinline__ float4 cf_raw_f4(const uint2& v) {
  return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                     __uint_as_float(v.y & 0xffff0000u));
}

// The first window's gated gradient as the plain form leaves it in gt for the second: for bf16 storage rounded once to bf16,
// as the store does
template <typename AT>
__device__ __forceinline__ float cf_as_stored(float v) {
  if constexpr (sizeof(AT) == 2) {
    const f32v4 f = {v, v, v, v};
    const f32v4 r = __builtin_convertvector(__builtin_convertvector(f, bf16v4), f32v4);
    return r[0];
  }
  return v;
}

// One tile (WPB patches along W) of one window.
// FORM (nmf_cf.h), for the two-window pair that hands window 0 to window 1 in factored form (dL/dX of the row-space reverse
// mode IS factored: u_T gcᵀ + gs·1ᵀ + ga₁ v_startᵀ + S X, and X is the t that window 1 loads anyway):
//   CF_STORE_FACTORS  window 0 stops in front of the output stage and writes gc — gcfac (B, heads, D, H, W) fp32, at the
//                     true voxel positions, through one plane of the exchange — and the 88 coefficients of its patch
//                     (cofac, the window's own grid order); gt is not touched;
//   CF_FROM_FACTORS   window 1 does not read gt: every lane rebuilds window 0's gated value of its 2 x 4 columns with
//                     gram_gx_elem — the function gx_row evaluates — from gcfac (coalesced load, exchange), the coefficients
//                     of the window-0 patch each 16-byte chunk lies in (the <= 8 patches a window-1 patch overlaps, staged in
//                     wave-private LDS) and its resident X, and adds it to its own gated row in front of the exchange.
//                     v_start is v0 (G = T), looked up at the chunk's column inside the window-0 patch.
// Both W-axis shifts are multiples of 4 (!HALF), so a chunk lies in one patch of either window.  The pair returns the bits of
// two CF_PLAIN launches (accumulate 0, then 1): same coefficients, same expression, the same two-operand add.
// The body is nmf_cf_gram_body.inc, included by the plain kernel and by the kernel of the two factor forms.
template <int WPB, bool HALF, typename AT, int MODE>
__global__ __launch_bounds__(WPB * 64, WPB == 4 ? FZ_GRAM_WAVES : 1) void nmf_cf_bwd_gram_kernel(
    const AT* __restrict__ t, const float* __restrict__ v0, const AT* __restrict__ ga, AT* __restrict__ gt, CfGeom q,
    int T, int G, float eps, int xcd_remap) {
  extern __shared__ __attribute__((aligned(16))) float fz_lds_cfg[];
  constexpr int FORM = CF_PLAIN;
  float* const gcfac = nullptr;
  float* const cofac = nullptr;
#include "nmf_cf_gram_body.inc"
}

// the factor forms (FORM = CF_STORE_FACTORS: gt unused; CF_FROM_FACTORS: q.ps* = window 0's shift)
template <typename AT, int MODE, int FORM>
__global__ __launch_bounds__(256, FZ_GRAM_WAVES) void nmf_cf_bwd_gram_fac_kernel(
    const AT* __restrict__ t, const float* __restrict__ v0, const AT* __restrict__ ga, AT* __restrict__ gt,
    float* __restrict__ gcfac, float* __restrict__ cofac, CfGeom q, int T, int G, float eps, int xcd_remap) {
  extern __shared__ __attribute__((aligned(16))) float fz_lds_cfg[];
  constexpr int WPB = 4;
  constexpr bool HALF = false;
#include "nmf_cf_gram_body.inc"
}

template <typename AT>
int cf_bwd_gram_launch(const AT* t, const float* v0, const AT* ga, AT* gt, const CfLaunch& a, int T, int G, float eps) {
  const CfGeom& q = a.q;
  const bool half = (q.s2 % 4) != 0;
#ifdef FZ_PROBE_GRAM_WPB   // timing probe (tools/probes/gram_tile.sh): FZ_PROBE_GRAM_WPB patches along W per workgroup instead of 4
  const int twpb = (q.G2 % FZ_PROBE_GRAM_WPB) == 0 ? FZ_PROBE_GRAM_WPB : ((q.G2 % 4) == 0 ? 4 : 1);
#else
  const int twpb = (q.G2 % 4) == 0 ? 4 : 1;
#endif
  constexpr bool kF32 = sizeof(AT) == 4;
#ifdef FZ_PROBE_GRAM_WPB
  const int stage = twpb == FZ_PROBE_GRAM_WPB ? CfTile<FZ_PROBE_GRAM_WPB>::STAGE_FLOATS : (twpb == 4 ? CfTile<4>::STAGE_FLOATS : CfTile<1>::STAGE_FLOATS);
#else
  const int stage = twpb == 4 ? CfTile<4>::STAGE_FLOATS : CfTile<1>::STAGE_FLOATS;
#endif
  const int glds = (stage + twpb * gram_hist_floats(G - 1)) * (int)sizeof(float);
#ifndef FZ_PROBE_GRAM_WPB
  if (glds > 64 * 1024) return FZ_E_UNSUPPORTED;
#endif
  const unsigned nblk = (unsigned)(a.nmat / twpb);
#define FZ_CF_BWD_GRAM(WW, HH, MM) \
  hipLaunchKernelGGL((nmf_cf_bwd_gram_kernel<WW, HH, AT, MM>), dim3(nblk), dim3(64 * WW), glds, a.st, t, v0, ga, gt, q, T, G, eps, a.xr)
  constexpr int kRegMode = kF32 ? CFG_HALVES : CFG_RAW;
#ifdef FZ_PROBE_GRAM_WPB
  if (!half && twpb == FZ_PROBE_GRAM_WPB) {
    auto kern = nmf_cf_bwd_gram_kernel<FZ_PROBE_GRAM_WPB, false, AT, kRegMode>;
    if (glds > 64 * 1024) FZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, glds));
    FZ_CF_BWD_GRAM(FZ_PROBE_GRAM_WPB, false, kRegMode);
    FZ_LAUNCH_CHECK();
    return FZ_OK;
  }
#endif
  if (half) { if (twpb == 4) FZ_CF_BWD_GRAM(4, true, kRegMode); else FZ_CF_BWD_GRAM(1, true, kRegMode); }
  else if (twpb == 4) FZ_CF_BWD_GRAM(4, false, kRegMode);
  else return FZ_E_UNSUPPORTED;
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
template <typename AT>
int cf_bwd_gram_factors_launch(const AT* t, const float* v0, const AT* ga, AT* gt, float* gcfac, float* cofac, const CfLaunch& a,
                               int form, int T, int G, float eps) {
  const CfGeom& q = a.q;
  if ((q.s2 % 4) || (q.ps2 % 4) || (q.G2 % 4) || G != T || G < 1) return FZ_E_UNSUPPORTED;
  int glds = (CfTile<4>::STAGE_FLOATS + 4 * gram_hist_floats(G - 1)) * (int)sizeof(float);
  if (form == CF_FROM_FACTORS) glds += 4 * 8 * CFG_COFAC * (int)sizeof(float);
  if (glds > 64 * 1024) return FZ_E_UNSUPPORTED;
  const unsigned nblk = (unsigned)(a.nmat / 4);
  constexpr int kRegMode = sizeof(AT) == 4 ? CFG_HALVES : CFG_RAW;
  if (form == CF_STORE_FACTORS)
    hipLaunchKernelGGL((nmf_cf_bwd_gram_fac_kernel<AT, kRegMode, CF_STORE_FACTORS>), dim3(nblk), dim3(256), glds, a.st, t, v0, ga,
                       gt, gcfac, cofac, q, T, G, eps, a.xr);
  else
    hipLaunchKernelGGL((nmf_cf_bwd_gram_fac_kernel<AT, kRegMode, CF_FROM_FACTORS>), dim3(nblk), dim3(256), glds, a.st, t, v0, ga,
                       gt, gcfac, cofac, q, T, G, eps, a.xr);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
template int cf_bwd_gram_factors_launch<float>(const float*, const float*, const float*, float*, float*, float*, const CfLaunch&, int, int, int, float);
template int cf_bwd_gram_factors_launch<bf16>(const bf16*, const float*, const bf16*, bf16*, float*, float*, const CfLaunch&, int, int, int, float);

template int cf_bwd_gram_launch<float>(const float*, const float*, const float*, float*, const CfLaunch&, int, int, float);
template int cf_bwd_gram_launch<bf16>(const bf16*, const float*, const bf16*, bf16*, const CfLaunch&, int, int, float);

}  // namespace fz
