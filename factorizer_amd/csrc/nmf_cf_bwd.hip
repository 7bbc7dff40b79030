// nmf_cf_bwd.hip — backward of the fused FactMixer core (nmf_cf_fwd.hip) for every solver and rank it runs: the wave
// program of nmf_core.h replayed from its history in LDS, one kernel per window.  The general kernels, and the launcher that
// chooses between them and the row-space kernel of nmf_cf_gram.hip; the entry points are in nmf_cf.hip.
#include "nmf_cf.h"

namespace fz {

// backward: gY = gather_w(ga) / W ; gt (+)= [t > 0] ∘ scatter_w(gX)
template <int R, int SOLVER, typename AT>
// (launched with 64 .. 256 threads; everything but the hot HALS rank-1 form runs one wave per SIMD rather than spill; CD rank 1,
// the same program without the gate, shares its bound)
__global__ __launch_bounds__(256, (R == 1 && (SOLVER == SOLVER_HALS || SOLVER == SOLVER_CD)) ? 2 : 1) void nmf_cf_bwd_kernel(const AT* __restrict__ t, const float* __restrict__ u0,
                                                            const float* __restrict__ v0,
                                                            const AT* __restrict__ ga, AT* __restrict__ gt,
                                                            CfGeom q, int64_t nmat, int T, int G, float eps,
                                                            int relu_gate, int xcd_remap) {
  extern __shared__ __attribute__((aligned(16))) float fz_lds_cf[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t mat = cf_logical_block(xcd_remap) * (blockDim.x >> 6) + wave;
  if (mat >= nmat) return;
  CfWave w{lane};
  CfAddr a;
  cf_decode(q, mat, lane, a);
  Hist<8, 8, R> h;
  h.carve(fz_lds_cf + wave * Hist<8, 8, R>::floats(G), G);
  float x[8][8], g[8][8];
  cf_load(t, a, x);
  cf_load(ga, a, g);
  cf_divide(g, q.gscale_div);
  nmf_backward_wave<8, 8, R, SOLVER>(w, u0, v0, x, g, h, 8, T, G, eps, nullptr, nullptr);
#pragma unroll
  for (int dd = 0; dd < 8; ++dd)
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
      AT* p = gt + a.base + dd * a.V + a.off[jp];
      float r[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gv = g[dd][jp * 4 + e];
        r[e] = (!relu_gate || x[dd][jp * 4 + e] > 0.f) ? gv : 0.f;
      }
      if (q.accumulate) {
        const float4 o = ld4(p);
        r[0] += o.x; r[1] += o.y; r[2] += o.z; r[3] += o.w;
      }
      st4(p, make_float4(r[0], r[1], r[2], r[3]));
    }
}

// line-coalesced backward: same exchange for t and for the incoming gradient, ReLU gate applied on
// the owner side before the exchange back, read-modify-write of gt with the coalesced map
template <int R, int SOLVER, int WPB, bool HALF, typename AT>
__device__ __forceinline__ void cf_bwd_tile_body(const AT* __restrict__ t, const float* __restrict__ u0,
                                                 const float* __restrict__ v0, const AT* __restrict__ ga,
                                                 AT* __restrict__ gt, const CfGeom& q, const CfTileId& id, int T, int G, float eps,
                                                 int relu_gate, float* S) {
  using TL = CfTile<WPB>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t base, V;
  unsigned off[2], off2[2];
  int lidx[2];
  cf_tile_decode<WPB>(q, id, tid, base, V, off, lidx, off2);
  const int own0 = cf_owner_lidx<WPB>(lane, wave, 0), own1 = cf_owner_lidx<WPB>(lane, wave, 1);
  Hist<8, 8, R> h;
  h.carve(S + TL::STAGE_FLOATS + wave * Hist<8, 8, R>::floats(G), G);

  // (loads and the staged store spelled out as in cf_fwd_tile_body, nmf_cf_fwd.hip: shared helpers changed the machine code)
  float x[8][8], g[8][8];
#pragma unroll
  for (int dd = 0; dd < 8; ++dd)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float4 v = cf_ld4<HALF>(t + base + dd * V, off[k], off2[k]);
      x[dd][k * 4 + 0] = v.x; x[dd][k * 4 + 1] = v.y; x[dd][k * 4 + 2] = v.z; x[dd][k * 4 + 3] = v.w;
    }
#pragma unroll
  for (int dd = 0; dd < 8; ++dd)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float4 v = cf_ld4<HALF>(ga + base + dd * V, off[k], off2[k]);
      g[dd][k * 4 + 0] = v.x; g[dd][k * 4 + 1] = v.y; g[dd][k * 4 + 2] = v.z; g[dd][k * 4 + 3] = v.w;
    }
  cf_to_owner<WPB>(S, lidx, own0, own1, x);
  cf_to_owner<WPB>(S, lidx, own0, own1, g);
  cf_divide(g, q.gscale_div);
  CfWave w{lane};
  nmf_backward_wave<8, 8, R, SOLVER>(w, u0, v0, x, g, h, 8, T, G, eps, nullptr, nullptr);

  // gate first (frees x), then ALL loads of the running sum at once: one exposed round trip, not four
  if (relu_gate) {
#pragma unroll
    for (int dd = 0; dd < 8; ++dd)
#pragma unroll
      for (int e = 0; e < 8; ++e) g[dd][e] = x[dd][e] > 0.f ? g[dd][e] : 0.f;
  }
  // (the plane base back in a scalar register pair: after the wave program the compiler otherwise carries it in vector
  // registers and every epilogue access pays a 64-bit vector address)
  asm volatile("" : "+s"(base));
  float4 old[8][2];
  if (q.accumulate) {
#pragma unroll
    for (int dd = 0; dd < 8; ++dd)
#pragma unroll
      for (int k = 0; k < 2; ++k) old[dd][k] = cf_ld4<HALF>(gt + base + dd * V, off[k], off2[k]);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      *reinterpret_cast<float4*>(S + c * 64 * TL::LW + own0) =
          make_float4(g[2 * s + c][0], g[2 * s + c][1], g[2 * s + c][2], g[2 * s + c][3]);
      *reinterpret_cast<float4*>(S + c * 64 * TL::LW + own1) =
          make_float4(g[2 * s + c][4], g[2 * s + c][5], g[2 * s + c][6], g[2 * s + c][7]);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        float4 z = *reinterpret_cast<const float4*>(S + c * 64 * TL::LW + lidx[k]);
        if (q.accumulate) {
          const float4 o = old[2 * s + c][k];
          z.x += o.x; z.y += o.y; z.z += o.z; z.w += o.w;
        }
        cf_st4<HALF>(gt + base + (2 * s + c) * V, off[k], off2[k], z);
      }
    __syncthreads();
  }
}

template <int R, int SOLVER, int WPB, bool HALF, typename AT>
__global__ __launch_bounds__(WPB * 64, (R == 1 && (SOLVER == SOLVER_HALS || SOLVER == SOLVER_CD) && (WPB == 4 || WPB == 1)) ? 2 : 1) void nmf_cf_bwd_tile_kernel(
    const AT* __restrict__ t, const float* __restrict__ u0, const float* __restrict__ v0,
    const AT* __restrict__ ga, AT* __restrict__ gt, CfGeom q, int T, int G, float eps, int relu_gate,
    int xcd_remap) {
  extern __shared__ __attribute__((aligned(16))) float fz_lds_cf[];
  cf_bwd_tile_body<R, SOLVER, WPB, HALF, AT>(t, u0, v0, ga, gt, q, cf_tile_id<WPB>(q, cf_logical_block(xcd_remap)), T, G, eps,
                                             relu_gate, fz_lds_cf);
}

// One launch.  HALS rank 1 behind a ReLU takes the row-space kernel (nmf_cf_gram.hip) where it applies and wins; everything
// else the line-coalesced general kernel, or the direct-gather one where the tile does not apply or its history does not fit.
template <typename AT>
int cf_bwd_launch(const AT* t, const float* u0, const float* v0, const AT* ga, AT* gt, const CfLaunch& a, int relu_gate, int R,
                  int T, int G, int solver, float eps) {
  const CfGeom& q = a.q;
  const int per_wave = (R == 1 ? Hist<8, 8, 1>::floats(G) : Hist<8, 8, 2>::floats(G)) * (int)sizeof(float);
  if (per_wave > 160 * 1024) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_bwd: history exceeds LDS");
  const int tile = FZ_KNOB("FZ_CF_TILE_BWD").set ? FZ_KNOB("FZ_CF_TILE_BWD").val : 1;
  const bool half = (q.s2 % 4) != 0;
  if (half || (tile && (q.G2 % 4) == 0)) {
    const int twpb = (q.G2 % 4) == 0 ? 4 : 1;
    // HALS rank 1 behind a ReLU (t >= 0 by the relu_gate contract): the row-space reverse mode, no per-column history
    const bool gram_on = !(FZ_KNOB("FZ_CF_GRAM").set && FZ_KNOB("FZ_CF_GRAM").val == 0);   // probe builds: 0 = the general kernel
    // (measured, tools/probes/gram_floor.sh: both kernels sit on the tile's memory skeleton; the row-space one is 6-11 % faster
    //  everywhere except fp32 windows w > 0 of >= 2^15 matrices, where the general kernel's single late burst of
    //  running-sum reads is 3-5 % ahead: 461-464 against 478-487 us at the README's stage 0)
    // (probe builds: 2 = the row-space kernel wherever it applies — what the factor pair of nmf_cf_gram.hip is compared with)
    const bool gram_wins = !(sizeof(AT) == 4 && q.accumulate && a.nmat >= 32768) || (FZ_KNOB("FZ_CF_GRAM").set && FZ_KNOB("FZ_CF_GRAM").val == 2);
    if (gram_on && gram_wins && R == 1 && solver == FZ_SOLVER_HALS && relu_gate && G >= 1) {
      const int rc = cf_bwd_gram_launch<AT>(t, v0, ga, gt, a, T, G, eps);
      if (rc != FZ_E_UNSUPPORTED) return rc;
    }
    const int tlds = (twpb == 4 ? CfTile<4>::STAGE_FLOATS : CfTile<1>::STAGE_FLOATS) * (int)sizeof(float) + per_wave * twpb;
    if (tlds > 160 * 1024) {
      if (half) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_bwd: history exceeds LDS for a W-axis shift of 2 (mod 4)");
    } else {
      const unsigned nblk = (unsigned)(a.nmat / twpb);
#define FZ_CF_BWD_TILE(RR, SS, WW, HH)                                                                      \
  do {                                                                                                      \
    auto kern = nmf_cf_bwd_tile_kernel<RR, SS, WW, HH, AT>;                                                    \
    if (tlds > 65536)                                                                                       \
      FZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                                    \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, tlds));                     \
    hipLaunchKernelGGL(kern, dim3(nblk), dim3(64 * WW), tlds, a.st, t, u0, v0, ga, gt, q, T, G, eps, relu_gate, a.xr); \
  } while (0)
#define FZ_CF_BWD_TILE_W(RR, SS)                                                                            \
  do {                                                                                                      \
    if (half) { if (twpb == 4) FZ_CF_BWD_TILE(RR, SS, 4, true); else FZ_CF_BWD_TILE(RR, SS, 1, true); }     \
    else FZ_CF_BWD_TILE(RR, SS, 4, false);                                                                  \
  } while (0)
      if (R == 1) { FZ_SOLVER_CASES(FZ_CF_BWD_TILE_W, 1); }
      else { FZ_SOLVER_CASES(FZ_CF_BWD_TILE_W, 2); }
      FZ_LAUNCH_CHECK();
      return FZ_OK;
    }
  }
  // direct gather: as many patches per workgroup as keep the histories within 64 KB, at most four
  int wpb = 65536 / per_wave;
  if (wpb > 4) wpb = 4;
  if (wpb < 1) wpb = 1;
  const int lds = per_wave * wpb;
  dim3 grid((unsigned)((a.nmat + wpb - 1) / wpb)), block(64 * wpb);
#define FZ_CF_BWD(RR, SS)                                                                                 \
  do {                                                                                                    \
    auto kern = nmf_cf_bwd_kernel<RR, SS, AT>;                                                          \
    if (lds > 65536)                                                                                      \
      FZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                                  \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, lds));                    \
    hipLaunchKernelGGL(kern, grid, block, lds, a.st, t, u0, v0, ga, gt, q, a.nmat, T, G, eps, relu_gate, a.xr); \
  } while (0)
  if (R == 1) { FZ_SOLVER_CASES(FZ_CF_BWD, 1); }
  else { FZ_SOLVER_CASES(FZ_CF_BWD, 2); }
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
template int cf_bwd_launch<float>(const float*, const float*, const float*, const float*, float*, const CfLaunch&, int, int, int, int, int, float);
template int cf_bwd_launch<bf16>(const bf16*, const float*, const float*, const bf16*, bf16*, const CfLaunch&, int, int, int, int, int, float);

}  // namespace fz
