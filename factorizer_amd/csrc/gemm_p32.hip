// gemm_p32.hip — the persistent 32 -> 32 kernel of the fp32-MFMA GEMM family (gemm.hip has the family's layers and MFMA mapping)
// and its host launcher, reached from fz_gemm's dispatcher.
#include "gemm_bx.h"       // uload (brings gemm_common.h)
#include "gemm_shared.h"   // knob_pos, gemm_p32_launch

namespace fz {

// =================================================================================================
// Kernel A' — the 32 -> 32 layers of stage 0 without a residual (LayerNorm + Linear in-projection, plain projections):
// PERSISTENT waves.  The weights are this lane's 16 A operands for the whole walk (registers, no LDS image, no barrier in
// the loop), every wave walks 128-column tiles with the operand of its next TWO tiles in flight — the one-tile-per-workgroup
// forms (Kernel A, the streaming ring) pay the load round trip of every tile in the open (wait share 0.4-0.7, profile 8).
// Arithmetic as Kernel A: exact two-pass LayerNorm, K-steps in ascending order on v_mfma_f32_32x32x2_f32.
// Host-checked: M <= 32, K == Cin == 32, plain loader and epilogue, no gate, no residual, Ncol % 4 == 0.
// =================================================================================================
// (The split-bf16 form of this kernel — 48 bf16 MFMAs + operand splits instead of 64 fp32 MFMAs, DESIGN §10.4a — needs ~20 registers
// more than the 240 of two operand tiles in flight + 64 accumulators leave at two waves per SIMD: 10-16 spilled; computing and storing the
// tile two column groups at a time — 32 accumulators, 8-byte stores, split weights in LDS — fits and is SLOWER: ln_linear_32->32 0.51 -> 0.84 ms per
// step fp32, 0.57 -> 0.58 bf16.  Not built in.)
template <int PF, typename AT>
__global__ __launch_bounds__(256, 2) void gemm_p32_kernel(GemmArgsT<AT> p, unsigned ntiles) {
  constexpr bool ACTIN = (PF & 1) != 0, LNP = (PF & 2) != 0;
  // (only PF 0 and 2 are instantiated: gemm_p32_launch.  The ACTIN arms below are kept as the resident kernel's are, unreachable here)
  __shared__ float tW[32];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int j = lane & 31, h = lane >> 5;
  const unsigned tps = (unsigned)((p.Ncol + 127) / 128);

  // (M <= 32: rows beyond M have zero weights and are not stored — the 32 -> 3 head)
  if (threadIdx.x < 32) {
    float t = 0.f;
    if ((int)threadIdx.x < p.M) {
      t = p.bias ? p.bias[threadIdx.x] : 0.f;
      if (LNP)
        for (int k = 0; k < 32; ++k) t += weight_at(p, (int)threadIdx.x, k) * p.ln_b[k];
    }
    tW[threadIdx.x] = t;
  }
  float aw[16];   // A operand of K-step s: W[row j][channel 2s + h] (x gamma)
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    aw[s] = j < p.M ? weight_at(p, j, 2 * s + h) : 0.f;
    if (LNP) aw[s] *= p.ln_g[2 * s + h];
  }
  __syncthreads();
  float add[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) add[r] = tW[(r & 3) + 8 * (r >> 2) + 4 * h];

  typedef float BvT[16][4];
  auto fetch = [&](unsigned t, BvT& bv) {
    // every address = wave-uniform base (sample, channel pair: SGPRs) + ONE 32-bit lane offset (channel parity h, column)
    const unsigned b = t / tps;
    const int64_t col = (int64_t)(t - b * tps) * 128 + 4 * j;
    const unsigned xoff = (unsigned)(((int64_t)h * p.Vin + (col < p.Ncol ? col : 0)) * (int64_t)sizeof(AT));
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int c = 2 * s;   // (c0 is even: both channels of the pair come from the same source)
      const bool first = c < p.c0;
      const AT* base = first ? p.x[0] : p.x[1];
      const int cs = first ? p.c0 : 32 - p.c0;
      const int ci = first ? c : c - p.c0;
      uload<4>(base + ((int64_t)b * cs + ci) * p.Vin, xoff, bv[s]);
    }
  };
  const unsigned tstep = gridDim.x * 4;
  auto run = [&](unsigned t, BvT& bv) {
    const unsigned b = t / tps;
    const int64_t col_off = (int64_t)(t - b * tps) * 128 + 4 * j;
    const bool col_ok = col_off < p.Ncol;
    if (LNP) {
      float mu[4], rs[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) v += bv[s][e];
        v += __shfl_xor(v, 32, 64);
        mu[e] = v / 32.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const float d = bv[s][e] - mu[e];
          v += d * d;
        }
        v += __shfl_xor(v, 32, 64);
        rs[e] = 1.0f / sqrtf(v / 32.f + p.ln_eps);
      }
#pragma unroll
      for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[s][e] = (bv[s][e] - mu[e]) * rs[e];
      if (p.stats_out != nullptr && h == 0 && col_ok) {
        float* so = p.stats_out + (int64_t)b * 2 * p.Vin;
        *reinterpret_cast<float4*>(so + col_off) = make_float4(mu[0], mu[1], mu[2], mu[3]);
        *reinterpret_cast<float4*>(so + p.Vin + col_off) = make_float4(rs[0], rs[1], rs[2], rs[3]);
      }
    }
    if (ACTIN && p.bact == ACT_GELU) {
#pragma unroll
      for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[s][e] = gelu_f(bv[s][e]);
    } else if (ACTIN && p.bact == ACT_RELU) {
#pragma unroll
      for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[s][e] = bv[s][e] > 0.f ? bv[s][e] : 0.f;
    }
    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[s], bv[s][q], acc[q], 0, 0, 0);
    if (t + 2 * tstep < ntiles) fetch(t + 2 * tstep, bv);   // the operand registers are free: the tile two steps ahead
    if (col_ok) {
      const unsigned yoff = (unsigned)(((int64_t)4 * h * p.Ncol + col_off) * (int64_t)sizeof(AT));
      AT* yb = p.y + (int64_t)b * p.M * p.Ncol;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if ((r & 3) + 8 * (r >> 2) + 4 * h >= p.M) continue;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = acc[q][r] + add[r];
        if (p.eact) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = act_f(p.eact, v[q]);
        }
        vstore<4>(reinterpret_cast<AT*>(reinterpret_cast<char*>(yb + (int64_t)((r & 3) + 8 * (r >> 2)) * p.Ncol) + yoff), v);
      }
    }
  };

  BvT bvA, bvB;
  unsigned tile = blockIdx.x * 4 + (unsigned)wave;
  if (tile < ntiles) fetch(tile, bvA);
  if (tile + tstep < ntiles) fetch(tile + tstep, bvB);
  for (; tile < ntiles; tile += 2 * tstep) {
    run(tile, bvA);
    if (tile + tstep < ntiles) run(tile + tstep, bvB);
  }
}

static int knob_p32_wgs() { return knob_pos(FZ_KNOB("FZ_GEMM_P32_WGS"), 512); }           // resident: 2 per CU

// Host side of Kernel A': gemm_launch (gemm.hip) decides that the layer is one of this kernel's and comes here with the filled
// argument block.
template <typename AT>
int gemm_p32_launch(const fz_gemm_desc* d, const GemmArgsT<AT>& a, fz_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  const unsigned ntiles = (unsigned)(d->B * ((d->Ncol + 127) / 128));
  const unsigned cap = (unsigned)knob_p32_wgs();
  const unsigned wgs = (ntiles + 3) / 4 < cap ? (ntiles + 3) / 4 : cap;
  // (gemm_launch sends no input activation here: alone it stays with the resident kernel, behind a LayerNorm it is refused)
  const int pf = d->ln ? 2 : 0;
  dim3 grid(wgs), block(256);
  if (gemm_plan_only()) return gemm_plan_form("p32 pf%d grid=%ux1", pf, grid.x);   // (fz_gemm_plan's dry run)
  if (pf == 0) hipLaunchKernelGGL((gemm_p32_kernel<0, AT>), grid, block, 0, st, a, ntiles);
  else hipLaunchKernelGGL((gemm_p32_kernel<2, AT>), grid, block, 0, st, a, ntiles);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
template int gemm_p32_launch<float>(const fz_gemm_desc*, const GemmArgsT<float>&, fz_stream_t);
template int gemm_p32_launch<bf16>(const fz_gemm_desc*, const GemmArgsT<bf16>&, fz_stream_t);

}  // namespace fz
