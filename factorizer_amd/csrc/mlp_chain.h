// mlp_chain.h — what the units of the chained block MLP share (mlp_chain.hip: host dispatch of fz_mlp_chain; mlp_chain32.hip,
// mlp_chain64.hip, mlp_chain_wg.hip: one kernel and its launcher each): the chain's argument block, the start stagger, the
// dynamic-LDS sizes that a kernel and its launcher both state, the probe knobs more than one unit reads, and the launchers.
#pragma once
#include "gemm_bx.h"       // split-bf16 operand helpers for the fused kernels (brings gemm_common.h)
#include "gemm_shared.h"   // half_sum32, lnbwd_block, DropArgs, kTS, knob_pos

namespace fz {

template <typename AT>
struct ChainArgsT {
  const float* wB;     // GEMM 2 weights: A[m][k] = wB_t ? wB[k*ldwB + m] : wB[m*ldwB + k]   (m < 32, k < 64)
  int wB_t, ldwB;
  const float* biasB;  // forward: [32] or null
  AT* side;            // (B, 64, V)
  // PRE (forward, round 5): the block's out-projection in front of the chain — x1 = preW · preA + preB + preRes is formed on
  // the accumulators, written to preOut (the backward needs it) and normalised in place: x1 is never read back
  const AT* preA;      // (B, 32, V) the core's output a
  const float* preW;   // (32, 32) out_proj weight W[m][k]
  const float* preB;   // (32) or null
  const AT* preRes;    // (B, 32, V) the block input x (residual)
  AT* preOut;          // (B, 32, V) x1
  // POST (forward, with PRE): the network's head Linear(32 -> postM <= 4) on the chain's output while it is in registers
  const float* postW;  // (postM, 32)
  const float* postB;  // (postM) or null
  AT* postOut;         // (B, postM, V) or null
  int postM;
  int stagger;         // start delay of the workgroups beyond the first 256, in units of 8 192 cycles per 256 workgroups (timing only)
};

// Resident workgroups of one launch start together and walk tiles of equal length: the waves that share a SIMD then sit in
// the same phase of the tile (all in their MFMA chains, or all in the GELU / epilogue VALU phase), and the matrix pipe idles
// while the vector pipe is contended (MI355X_MICROARCH.md "two waves that run the SAME program ... try a stagger").  Workgroups
// 256 .. 511 (the second resident workgroup of every CU under round-robin placement: speed only) start `stagger` sleep
// quanta later, workgroups 512 .. twice that.  Results do not depend on it.
__device__ __forceinline__ void chain_stagger(int stagger) {
  const int n = stagger * (int)(blockIdx.x >> 8);
  for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(127);
}

// ---- dynamic LDS (floats) of the kernels that carve it: the kernel asserts that its carve-up ends here, the launcher asks for it ----
// gemm_chain64_kernel: two weight images (+ the W_o image and its bias under PRE) | tW [128] | tB [64] | red [4][128] per 4-wave half
constexpr int chain64_lds_floats(bool p512, bool pre) {
  return 2 * (p512 ? 12288 : 8192) + (pre ? 6144 + 64 : 0) + 128 + 64 + (p512 ? 2 : 1) * 512;
}
// gemm_chain_bwd_wg_kernel: two staged weight blocks | gamma [32] | red [4][64] | four wave regions (Bf | T, or the WGB planes)
constexpr int chain_wg_lds_floats(bool bx, bool wgb) {
  return 2 * (bx ? 3072 : 2048) + 32 + 256 + 4 * (wgb ? 3072 : 48 * kTS);
}

// one launch of a kernel with `lds_floats` of dynamic LDS
template <typename... KArgs, typename... Args>
static int launch_lds(void (*kern)(KArgs...), dim3 grid, dim3 block, int lds_floats, hipStream_t st, Args... args) {
  const int lds = lds_floats * (int)sizeof(float);
  FZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

// ---- probe knobs that more than one unit reads (FZ_KNOB is a compile-time "unset" in the shipped library) ----
static int knob_chain64_p512() { return knob_pos(FZ_KNOB("FZ_CHAIN64_P512"), 1) == 1; }   // 2 = off (A/B runs)
static int knob_chain_fwd_bx() { const auto& k = FZ_KNOB("FZ_CHAIN_FWD_BX"); return k.set ? k.val : 1; }   // 0: the fp32-MFMA forward chain
static int knob_mlp_wgs(int dflt) { return knob_pos(FZ_KNOB("FZ_MLP_WGS"), dflt); }

// ---- the launchers: fz_mlp_chain's dispatcher (mlp_chain.hip) has checked the descriptor and filled the argument blocks ----
// C = 32, modes 0 and 1: gemm_chain_kernel (mlp_chain32.hip); `drop` is null unless a dropout plane is live, `fac` unless the
// out-projection's operand comes as the core's factors (fz_mlp_chain_fac)
template <typename AT>
int chain32_launch(const fz_mlp_desc* d, const fz_mlp_dropout* drop, const fz_outproj_fac* fac, const GemmArgsT<AT>& a, const ChainArgsT<AT>& c,
                   fz_stream_t stream);
// C = 64, modes 0 and 1: gemm_chain64_kernel (mlp_chain64.hip)
template <typename AT>
int chain64_launch(const fz_mlp_desc* d, const GemmArgsT<AT>& a, const ChainArgsT<AT>& c, fz_stream_t stream);
// C = 32, mode 2: gemm_chain_bwd_wg_kernel and the finish jobs that add its rows (mlp_chain_wg.hip)
template <typename AT>
int chain_wg_launch(const fz_mlp_desc* d, const GemmArgsT<AT>& a, const ChainArgsT<AT>& c, fz_stream_t stream);

}  // namespace fz
