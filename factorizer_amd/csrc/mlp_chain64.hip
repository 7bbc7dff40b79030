// mlp_chain64.hip — the chained MLP of the C = 64 blocks on the matrix cores (gemm.hip has the MFMA mapping it shares):
// gemm_chain64_kernel, its host launcher, reached from fz_mlp_chain's dispatcher (mlp_chain.hip), and the launcher of its SINGLE
// form, reached from fz_gemm's dispatcher (gemm.hip).
#include "mlp_chain.h"     // ChainArgsT, chain64_lds_floats, launch_lds, knob_mlp_wgs, knob_chain64_p512, chain64_launch

namespace fz {

// Eight K-steps of two of an fp32-MFMA loop as ONE split-bf16 K-step (gemm_bx.hip) for NRB row blocks x NQ column blocks:
// load_a(rb, a8) = the lane's weights of the eight steps (fp32, from the LDS operand image of the fp32 form, split here),
// get_x(q, x8) = the column operands of the same steps.  Element e of lane half h of v_mfma_f32_32x32x16_bf16 = step e of the
// group: any assignment of reduction indices to (half, element) slots is valid as long as both operands use the same one.
// HOIST splits the column operands once for all row blocks (NQ x NTB x 4 more live registers); without it they are split
// per row block (the fp32 chain kernels sit at the 256-register limit).
template <bool HOIST, int NRB, int NQ, int NTA, int NTB, typename FA, typename FX>
__device__ __forceinline__ void bx_group(f32x16 (&acc)[NRB][NQ], FA load_a, FX get_x) {
  if constexpr (HOIST) {
    bx8 bop[NQ][NTB];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float x8[8];
      get_x(q, x8);
      bx_split<NTB>(x8, bop[q]);
    }
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      float a8[8];
      load_a(rb, a8);
      bx8 aop[NTA];
      bx_split<NTA>(a8, aop);
#pragma unroll
      for (int q = 0; q < NQ; ++q) bx_mfma<NTA, NTB>(acc[rb][q], aop, bop[q]);
    }
  } else {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      bx8 bop[NTB];
      {
        float x8[8];
        get_x(q, x8);
        bx_split<NTB>(x8, bop);
      }
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        float a8[8];
        load_a(rb, a8);
        bx8 aop[NTA];
        bx_split<NTA>(a8, aop);
        bx_mfma<NTA, NTB>(acc[rb][q], aop, bop);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// The same group with the row operands PRE-SPLIT in LDS (load_term(rb, t) = level t of the row operand, one ds_read_b128):
// no weight split on the VALU; the levels are fetched one at a time — a_0 (b_0 + b_1 + b_2), a_1 (b_0 + b_1), a_2 b_0, small
// products first within a level — so only four operand registers are live next to the split column operand.
template <int NRB, int NQ, int NTB, typename FA, typename FX>
__device__ __forceinline__ void bx_group_ps(f32x16 (&acc)[NRB][NQ], FA load_term, FX get_x) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    bx8 bop[NTB];
    {
      float x8[8];
      get_x(q, x8);
      bx_split<NTB>(x8, bop);
    }
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
#pragma unroll
      for (int t = 2; t >= 0; --t) {
        const bx8 a = load_term(rb, t);
#pragma unroll
        for (int jj = NTB - 1; jj >= 0; --jj)
          if (t + jj <= 2) acc[rb][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bop[jj], acc[rb][q], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);   // (keeps the operand reads of the next row block from being hoisted: registers)
    }
  }
}

// =================================================================================================
// MLP chain for C = 64, hidden 128 (stage 1 of the README model): the same two chained GEMMs as gemm_chain_kernel,
// with the hidden tensor produced and consumed in TWO passes of 64 rows — 64 accumulator registers for the pass,
// 64 for the 64-row result that GEMM 2 accumulates over both passes, 64 for the operand tile — so the chain still
// fits 256 VGPRs at two workgroups per CU with 8-byte lane loads.  Weights of both GEMMs (2 x 32 KB) sit in LDS in
// operand order; the residual (forward) / added gradient and the LayerNorm input (backward) are re-read in the
// accumulator layout (L2 / MALL) instead of being stashed.
//   forward : z = W1·LN(x1) + b1 -> side ; out = x1 + W2·gelu(z) + b2          5 plane-sets against 7 unfused
//   backward: gz = (W2ᵀ g2) ∘ gelu'(z) -> side ; out = LNbwd(W1ᵀ gz) + g2      8 against 12 (+ dγ, dβ partial rows)
// =================================================================================================
// SINGLE (BWD only): ONE 64 -> 64 input-gradient GEMM (in_proj of a C = 64 block) in front of the same LayerNorm-backward
// epilogue — fz_gemm with EPI_LNBWD and M = K = 64: the pre-LayerNorm gradient never reaches HBM.
// BX: every GEMM of the chain on split-bf16 products — the weights stay fp32 in LDS (64 KB: a pre-split image would be 96 KB
// and halve the occupancy) and are split per use, the column operands once per group of eight steps.
// P512 (BX, not SINGLE; both storage types): the fp32-weight form above does not fit 256 registers once the operand splits are
// added (6 / 23 spilled), so the split-bf16 chain runs as ONE workgroup of 512 threads per CU — two independent 4-wave
// halves, each walking its own tiles — sharing a PRE-SPLIT weight image (bf16x8 triples in operand order: 2 x 48 KB):
// same two waves per SIMD, no weight splits on the VALU, 3 ds_read_b128 per row operand instead of 8 ds_read_b32.
// PRE (forward, P512) [r5]: the block's out-projection in front of the chain, as gemm_chain_kernel<.., PRE> does at C = 32 —
// the tile loaded is a, GEMM 0 forms x1 = W_o·a + b_o + x on 64 accumulator registers (rounded to the stored value under bf16
// storage), x1 goes to preOut, is normalised in place and feeds GEMM 1 as the column operand in the ACCUMULATOR layout (the W1
// image is staged in that k order: the order the W2 image always had); the residual of the epilogue re-reads the lane's own x1.
// A third pre-split image (W_o: 24 KB) joins the two: 121 KB of LDS.
template <bool BWD, typename AT, bool SINGLE = false, bool BX = false, bool P512 = false, bool PRE = false>
__global__ __launch_bounds__(P512 ? 512 : 256, 2) void gemm_chain64_kernel(GemmArgsT<AT> p, ChainArgsT<AT> c, int ntiles) {
  constexpr int NACC = 2, C = 64, HID = 128;
  constexpr int NTA = BxTerms<AT>::A, NTB = bx_terms_b<AT>(BXPRO_GELU);
  constexpr bool HOIST = SINGLE || sizeof(AT) == 2;
  static_assert(!P512 || (BX && !SINGLE), "P512: the split-bf16 chain around a pre-split weight image");
  static_assert(!PRE || (P512 && !BWD), "PRE: the forward chain around the pre-split images");
  constexpr int NA = P512 ? 12288 : 8192;   // floats of one weight image (P512: [16 (group, row block)][3 terms][64 lanes] x 16 B)
  constexpr int NA0 = PRE ? 6144 : 0;       // the W_o image: [8 (group, row block)][3 terms][64 lanes] x 16 B
  extern __shared__ __attribute__((aligned(16))) float fz_lds_c64[];
  float* As1 = fz_lds_c64;            // [32 steps][4 row blocks][64]
  float* As2 = As1 + NA;              // [4 x 16 (rb, r) steps][2 row blocks][64]
  float* tW = As2 + NA + NA0;         // [128]
  float* tB = tW + 128;               // [64]
  float* tB0 = tB + 64;               // [64] (PRE: the out-projection's bias)
  const int half = P512 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8)) : 0;   // P512: which 4-wave half of the workgroup (wave-uniform)
  float* red = tB + 64 + (PRE ? 64 : 0) + half * 512;  // [4][128] per half
  static_assert(2 * NA + NA0 + 128 + 64 + (PRE ? 64 : 0) + (P512 ? 2 : 1) * 512 == chain64_lds_floats(P512, PRE), "the launcher's dynamic LDS ends where this carve-up does");
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6) & 3);
  const int j = lane & 31, h = lane >> 5;
  const int tiles_per_sample = (int)((p.Ncol + 128 * NACC - 1) / (128 * NACC));
  // P512 operand reads: ONE opaque per-lane base per image + compile-time element offsets (ds_read_b128 immediates; left
  // to itself the optimiser materialises a loop-invariant VGPR address per (slot, level) — 40 of them — and spills)
  // P512 operand reads: one OPAQUE per-lane float index per image + compile-time slot offsets (ds_read_b128 immediates are
  // 16 bits: the second image starts at 48 KB, and left to itself the optimiser keeps one loop-invariant VGPR address for
  // every slot beyond 64 KB — 32 of them — and spills)
  int lane4 = lane * 4, lane4b = lane * 4 + NA, lane4c = lane * 4 + 2 * NA;
  if constexpr (P512) {
    asm volatile("" : "+v"(lane4));
    asm volatile("" : "+v"(lane4b));
    if constexpr (PRE) asm volatile("" : "+v"(lane4c));
  }
  auto ld_a1 = [&](int slot3) { return *reinterpret_cast<const bx8*>(As1 + slot3 * 256 + lane4); };
  auto ld_a2 = [&](int slot3) { return *reinterpret_cast<const bx8*>(As1 + slot3 * 256 + lane4b); };
  auto ld_a0 = [&](int slot3) { return *reinterpret_cast<const bx8*>(As1 + slot3 * 256 + lane4c); };
  (void)ld_a0; (void)lane4c; (void)tB0;

  if constexpr (P512) {
    // item = (image, slot [16], lane): eight weights -> three bf16 levels -> three 16-byte stores
    for (int item = threadIdx.x; item < (PRE ? 2560 : 2048); item += 512) {
      const int l = item & 63, slot = (item >> 6) & 15, img = item >> 10;
      float a8[8];
      if (img == 0) {        // slot = g*4 + rb: A1[m = rb*32 + (l & 31)][k = 2 (8g + e) + (l >> 5)]
        const int g = slot >> 2, rb = slot & 3;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          // PRE: the column operand of GEMM 1 is the accumulator tile of GEMM 0 — k = row (mb = g >> 1, r = 8 (g & 1) + e, lane half)
          const int rr = 8 * (g & 1) + e;
          const int k = PRE ? (g >> 1) * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * (l >> 5) : 2 * (8 * g + e) + (l >> 5);
          a8[e] = weight_at(p, rb * 32 + (l & 31), k);
          if (!BWD) a8[e] *= p.ln_g[k];
        }
      } else if (PRE && img == 2) {   // slot = g*2 + mb: A0[m = mb*32 + (l & 31)][k = 2 (8g + e) + (l >> 5)] = W_o[m][k]
        const int g = slot >> 1, mb = slot & 1;
#pragma unroll
        for (int e = 0; e < 8; ++e) a8[e] = c.preW[(int64_t)(mb * 32 + (l & 31)) * 64 + 2 * (8 * g + e) + (l >> 5)];
      } else {               // slot = (rb4*2 + g8)*2 + mb: A2[m = mb*32 + (l & 31)][k = rb4*32 + row(r = 8 g8 + e) + 4 (l >> 5)]
        const int mb = slot & 1, g8 = (slot >> 1) & 1, rb4 = slot >> 2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int r = 8 * g8 + e;
          const int k = rb4 * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), m = mb * 32 + (l & 31);
          a8[e] = c.wB_t ? c.wB[(int64_t)k * c.ldwB + m] : c.wB[(int64_t)m * c.ldwB + k];
        }
      }
      bx8 t3[3];
      bx_split<3>(a8, t3);
      bx8* dst = reinterpret_cast<bx8*>(img == 0 ? As1 : (img == 1 ? As2 : As2 + NA)) + (slot * 3) * 64 + l;
      dst[0] = t3[0]; dst[64] = t3[1]; dst[128] = t3[2];
    }
  }
  for (int base = threadIdx.x; !P512 && base < (SINGLE ? 4096 : 16384); base += 256 * 8) {
    float tmp[8];
#pragma unroll
    for (int uu = 0; uu < 8; ++uu) {
      const int idx = base + uu * 256;
      float wv;
      if (SINGLE) {   // A[m = mb*32 + (l & 31)][k = 2a + (l >> 5)], [32 steps][2 row blocks][64]
        const int l = idx & 63, mb = (idx >> 6) & 1, a = idx >> 7;
        wv = weight_at(p, mb * 32 + (l & 31), 2 * a + (l >> 5));
      } else if (idx < 8192) {
        const int l = idx & 63, rb = (idx >> 6) & 3, a = idx >> 8;
        const int m = rb * 32 + (l & 31), k = 2 * a + (l >> 5);
        wv = weight_at(p, m, k);
        if (!BWD) wv *= p.ln_g[k];
      } else {
        const int i2 = idx - 8192;
        const int l = i2 & 63, mb = (i2 >> 6) & 1, s2 = i2 >> 7;
        const int r = s2 & 15, rb = s2 >> 4;
        const int k = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), m = mb * 32 + (l & 31);
        wv = c.wB_t ? c.wB[(int64_t)k * c.ldwB + m] : c.wB[(int64_t)m * c.ldwB + k];
      }
      tmp[uu] = wv;
    }
#pragma unroll
    for (int uu = 0; uu < 8; ++uu) fz_lds_c64[base + uu * 256] = tmp[uu];
  }
  if (BWD) {
    if (threadIdx.x < C) tB[threadIdx.x] = p.lnb_g[threadIdx.x];
  } else {
    for (int r = threadIdx.x; r < HID; r += blockDim.x) {
      float t = 0.f;
      for (int k = 0; k < C; ++k) t += weight_at(p, r, k) * p.ln_b[k];
      tW[r] = t + (p.bias ? p.bias[r] : 0.f);
      if (r < C) tB[r] = c.biasB ? c.biasB[r] : 0.f;
      if (PRE && r < C) tB0[r] = c.preB ? c.preB[r] : 0.f;
    }
  }

  // P512: the halves take tiles 2 i and 2 i + 1 (ntiles is even — host-checked — so both run the same number of rounds
  // and meet at the same barriers)
  const int tstep = P512 ? 2 * (int)gridDim.x : (int)gridDim.x;
  int tile = P512 ? 2 * (int)blockIdx.x + half : (int)blockIdx.x;
  float bv[32][NACC];
  auto fetch_tile = [&](int t) {
    const int bt = t / tiles_per_sample;
    const int64_t ct = ((int64_t)(t % tiles_per_sample) * 4 + wave) * (32 * NACC) + NACC * j;
    const unsigned lo = (unsigned)h * (unsigned)p.Ncol + (unsigned)(ct < p.Ncol ? ct : 0);
    const AT* xb = (PRE ? c.preA : p.x[0]) + (int64_t)bt * C * p.Ncol;
#pragma unroll
    for (int s = 0; s < 32; ++s) vload<NACC>(xb + (int64_t)(2 * s) * p.Ncol + lo, bv[s]);
  };
  fetch_tile(tile);
  __syncthreads();

  for (; tile < ntiles; tile += tstep) {
    asm volatile("" ::: "memory");
    const int b = tile / tiles_per_sample;
    const int64_t col_off = ((int64_t)(tile % tiles_per_sample) * 4 + wave) * (32 * NACC) + NACC * j;
    const bool col_ok = col_off < p.Ncol;
    const int64_t nc = col_ok ? col_off : 0;
    const unsigned lane_row = (unsigned)(4 * h) * (unsigned)p.Ncol + (unsigned)nc;

    f32x16 acc0[PRE ? 2 : 1][NACC];   // PRE: x1, then LN(x1), rows (mb, r, lane half) x the lane's two voxels
    if constexpr (PRE) {
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int q = 0; q < NACC; ++q)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc0[mb][q][r] = 0.f;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bx_group_ps<2, NACC, NTB>(acc0,
            [&](int mb, int t) { return ld_a0((g * 2 + mb) * 3 + t); },
            [&](int q, float (&x8)[8]) {
#pragma unroll
              for (int e = 0; e < 8; ++e) x8[e] = bv[8 * g + e][q];
            });
        __builtin_amdgcn_sched_barrier(0);
      }
      const int64_t smp = (int64_t)b * C * p.Ncol;
      float s1[NACC] = {0.f, 0.f};
#pragma unroll
      for (int g8 = 0; g8 < 4; ++g8) {
        float e[8][NACC];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int rr = g8 * 8 + i, mb = rr >> 4, r = rr & 15;
          vload<NACC>(c.preRes + smp + (int64_t)(mb * 32 + (r & 3) + 8 * (r >> 2)) * p.Ncol + lane_row, e[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int rr = g8 * 8 + i, mb = rr >> 4, r = rr & 15;
          const int rbase = mb * 32 + (r & 3) + 8 * (r >> 2);
          const float add = tB0[rbase + 4 * h];
          float v[NACC];
#pragma unroll
          for (int q = 0; q < NACC; ++q) v[q] = acc0[mb][q][r] + add + e[i][q];
          if (col_ok) vstore<NACC>(c.preOut + smp + (int64_t)rbase * p.Ncol + lane_row, v);
#pragma unroll
          for (int q = 0; q < NACC; ++q) {
            if constexpr (sizeof(AT) == 2) v[q] = (float)(AT)v[q];   // the MLP sees the STORED x1, as the two-launch form does
            acc0[mb][q][r] = v[q];
            s1[q] += v[q];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      float mu[NACC], rs[NACC];
#pragma unroll
      for (int q = 0; q < NACC; ++q) {
        s1[q] += __shfl_xor(s1[q], 32, 64);
        mu[q] = s1[q] / 64.0f;
        float t = 0.f;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float dd = acc0[mb][q][r] - mu[q];
            t += dd * dd;
          }
        t += __shfl_xor(t, 32, 64);
        rs[q] = 1.0f / sqrtf(t / 64.0f + p.ln_eps);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc0[mb][q][r] = (acc0[mb][q][r] - mu[q]) * rs[q];
      }
      if (p.stats_out != nullptr && h == 0 && col_ok) {
        float* so = p.stats_out + (int64_t)b * 2 * p.Vin;
        vstore<NACC>(so + col_off, mu);
        vstore<NACC>(so + p.Vin + col_off, rs);
      }
    }

    if (!BWD && !PRE) {
      float mu[NACC], rs[NACC];
#pragma unroll
      for (int e = 0; e < NACC; ++e) {
        float t = 0.f;
#pragma unroll
        for (int s = 0; s < 32; ++s) t += bv[s][e];
        t += __shfl_xor(t, 32, 64);
        mu[e] = t / 64.0f;
      }
#pragma unroll
      for (int e = 0; e < NACC; ++e) {
        float t = 0.f;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
          const float d = bv[s][e] - mu[e];
          t += d * d;
        }
        t += __shfl_xor(t, 32, 64);
        rs[e] = 1.0f / sqrtf(t / 64.0f + p.ln_eps);
      }
#pragma unroll
      for (int s = 0; s < 32; ++s)
#pragma unroll
        for (int e = 0; e < NACC; ++e) bv[s][e] = (bv[s][e] - mu[e]) * rs[e];
      if (p.stats_out != nullptr && h == 0 && col_ok) {
        float* so = p.stats_out + (int64_t)b * 2 * p.Vin;
        vstore<NACC>(so + col_off, mu);
        vstore<NACC>(so + p.Vin + col_off, rs);
      }
    }

    f32x16 acc2[2][NACC];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[mb][q][r] = 0.f;

    if (SINGLE) {
      if constexpr (BX) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bx_group<HOIST, 2, NACC, NTA, NTB>(acc2,
              [&](int mb, float (&a8)[8]) {
#pragma unroll
                for (int e = 0; e < 8; ++e) a8[e] = As1[((8 * g + e) * 2 + mb) * 64 + lane];
              },
              [&](int q, float (&x8)[8]) {
#pragma unroll
                for (int e = 0; e < 8; ++e) x8[e] = bv[8 * g + e][q];
              });
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
#pragma unroll
      for (int s = 0; s < 32; ++s) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
          const float av = As1[(s * 2 + mb) * 64 + lane];
#pragma unroll
          for (int q = 0; q < NACC; ++q) acc2[mb][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[s][q], acc2[mb][q], 0, 0, 0);
        }
        if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
      }
      fetch_tile(tile + tstep < ntiles ? tile + tstep : tile);
    }
#pragma unroll
    for (int p2 = 0; p2 < (SINGLE ? 0 : 2); ++p2) {
      // ---- GEMM 1, hidden rows 64·p2 .. 64·p2 + 63 ----
      f32x16 acc1[2][NACC];
#pragma unroll
      for (int rbl = 0; rbl < 2; ++rbl)
#pragma unroll
        for (int q = 0; q < NACC; ++q)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc1[rbl][q][r] = 0.f;
      if constexpr (BX) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          if constexpr (P512)
            bx_group_ps<2, NACC, NTB>(acc1,
                [&](int rbl, int t) { return ld_a1((g * 4 + 2 * p2 + rbl) * 3 + t); },
                [&](int q, float (&x8)[8]) {
#pragma unroll
                  for (int e = 0; e < 8; ++e) x8[e] = PRE ? acc0[PRE ? (g >> 1) : 0][q][8 * (g & 1) + e] : bv[8 * g + e][q];
                });
          else
          bx_group<HOIST, 2, NACC, NTA, NTB>(acc1,
              [&](int rbl, float (&a8)[8]) {
#pragma unroll
                for (int e = 0; e < 8; ++e) a8[e] = As1[((8 * g + e) * 4 + 2 * p2 + rbl) * 64 + lane];
              },
              [&](int q, float (&x8)[8]) {
#pragma unroll
                for (int e = 0; e < 8; ++e) x8[e] = bv[8 * g + e][q];
              });
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
#pragma unroll
      for (int s = 0; s < 32; ++s) {
#pragma unroll
        for (int rbl = 0; rbl < 2; ++rbl) {
          const float av = As1[(s * 4 + 2 * p2 + rbl) * 64 + lane];
#pragma unroll
          for (int q = 0; q < NACC; ++q) acc1[rbl][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[s][q], acc1[rbl][q], 0, 0, 0);
        }
        if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
      }
      if (p2 == 1) fetch_tile(tile + tstep < ntiles ? tile + tstep : tile);   // the operand tile is consumed

      // ---- hidden rows: transform in registers, copy to HBM for the other pass ----
      if (!BWD) {
#pragma unroll
        for (int rbl = 0; rbl < 2; ++rbl)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int rbase = (2 * p2 + rbl) * 32 + (r & 3) + 8 * (r >> 2);
            const float add = tW[rbase + 4 * h];
            float v[NACC];
#pragma unroll
            for (int q = 0; q < NACC; ++q) v[q] = acc1[rbl][q][r] + add;
            if (col_ok) vstore<NACC>(c.side + ((int64_t)b * HID + rbase) * p.Ncol + lane_row, v);
            if constexpr (NACC == 2) {
              float gq[2];
              gelu2_f(v, gq);
              acc1[rbl][0][r] = gq[0]; acc1[rbl][1][r] = gq[1];
            } else {
#pragma unroll
              for (int q = 0; q < NACC; ++q) acc1[rbl][q][r] = gelu_f(v[q]);
            }
          }
      } else {
#pragma unroll
        for (int g8 = 0; g8 < 4; ++g8) {
          float e[8][NACC];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int rr = g8 * 8 + i, rbl = rr >> 4, r = rr & 15;
            const int rbase = (2 * p2 + rbl) * 32 + (r & 3) + 8 * (r >> 2);
            vload<NACC>(p.emul + ((int64_t)b * HID + rbase) * p.Ncol + lane_row, e[i]);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int rr = g8 * 8 + i, rbl = rr >> 4, r = rr & 15;
            const int rbase = (2 * p2 + rbl) * 32 + (r & 3) + 8 * (r >> 2);
            float v[NACC];
#pragma unroll
            for (int q = 0; q < NACC; ++q) v[q] = acc1[rbl][q][r] * gelu_grad_f(e[i][q]);
            if (col_ok) vstore<NACC>(c.side + ((int64_t)b * HID + rbase) * p.Ncol + lane_row, v);
#pragma unroll
            for (int q = 0; q < NACC; ++q) acc1[rbl][q][r] = v[q];
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }

      // ---- GEMM 2 += (64 result rows) x (these 64 hidden rows), straight from the accumulators ----
      if constexpr (BX) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {   // steps (rbl, r) = (g >> 1, 8 (g & 1) + e): accumulator registers as the column operand
          if constexpr (P512)
            bx_group_ps<2, NACC, NTB>(acc2,
                [&](int mb, int t) { return ld_a2((((2 * p2 + (g >> 1)) * 2 + (g & 1)) * 2 + mb) * 3 + t); },
                [&](int q, float (&x8)[8]) {
#pragma unroll
                  for (int e = 0; e < 8; ++e) x8[e] = acc1[g >> 1][q][8 * (g & 1) + e];
                });
          else
          bx_group<HOIST, 2, NACC, NTA, NTB>(acc2,
              [&](int mb, float (&a8)[8]) {
#pragma unroll
                for (int e = 0; e < 8; ++e) a8[e] = As2[(((2 * p2 + (g >> 1)) * 16 + 8 * (g & 1) + e) * 2 + mb) * 64 + lane];
              },
              [&](int q, float (&x8)[8]) {
#pragma unroll
                for (int e = 0; e < 8; ++e) x8[e] = acc1[g >> 1][q][8 * (g & 1) + e];
              });
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
#pragma unroll
      for (int rbl = 0; rbl < 2; ++rbl)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
          for (int mb = 0; mb < 2; ++mb) {
            const float av = As2[(((2 * p2 + rbl) * 16 + r) * 2 + mb) * 64 + lane];
#pragma unroll
            for (int q = 0; q < NACC; ++q) acc2[mb][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, acc1[rbl][q][r], acc2[mb][q], 0, 0, 0);
          }
          if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
      }
    }

    const int64_t sample = (int64_t)b * C * p.Ncol;
    if (!BWD) {
      // out = acc2 + b2 + x1 (residual re-read in the accumulator layout), 8 rows at a time
#pragma unroll
      for (int g8 = 0; g8 < 4; ++g8) {
        float e[8][NACC];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int rr = g8 * 8 + i, mb = rr >> 4, r = rr & 15;
          vload<NACC>(p.res + sample + (int64_t)(mb * 32 + (r & 3) + 8 * (r >> 2)) * p.Ncol + lane_row, e[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int rr = g8 * 8 + i, mb = rr >> 4, r = rr & 15;
          const int rbase = mb * 32 + (r & 3) + 8 * (r >> 2);
          const float add = tB[rbase + 4 * h];
          float v[NACC];
#pragma unroll
          for (int q = 0; q < NACC; ++q) v[q] = acc2[mb][q][r] + add + e[i][q];
          if (col_ok) vstore<NACC>(p.y + sample + (int64_t)rbase * p.Ncol + lane_row, v);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      // LayerNorm backward over the 64 channels of this lane's voxels (rows (mb, r, h)) + added gradient
      const float* sp = p.lnb_stats + (int64_t)b * 2 * p.Ncol;
      float mu[NACC], rs[NACC];
      vload<NACC>(sp + nc, mu);
      vload<NACC>(sp + p.Ncol + nc, rs);
      float xs[32][NACC];
      float m1[NACC] = {0.f, 0.f}, m2[NACC] = {0.f, 0.f};
#pragma unroll
      for (int g8 = 0; g8 < 4; ++g8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int rr = g8 * 8 + i, mb = rr >> 4, r = rr & 15;
          vload<NACC>(p.lnb_x + sample + (int64_t)(mb * 32 + (r & 3) + 8 * (r >> 2)) * p.Ncol + lane_row, xs[rr]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int rr = g8 * 8 + i, mb = rr >> 4, r = rr & 15;
          const float gc = tB[mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
#pragma unroll
          for (int q = 0; q < NACC; ++q) {
            const float av = acc2[mb][q][r] * gc;
            xs[rr][q] = (xs[rr][q] - mu[q]) * rs[q];
            m1[q] += av;
            m2[q] += av * xs[rr][q];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int q = 0; q < NACC; ++q) {
        m1[q] = (m1[q] + __shfl_xor(m1[q], 32, 64)) * (1.0f / 64.0f);
        m2[q] = (m2[q] + __shfl_xor(m2[q], 32, 64)) * (1.0f / 64.0f);
      }
#pragma unroll
      for (int g8 = 0; g8 < 4; ++g8) {
        float ga[8][NACC];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int rr = g8 * 8 + i, mb = rr >> 4, r = rr & 15;
          vload<NACC>(p.lnb_gadd + sample + (int64_t)(mb * 32 + (r & 3) + 8 * (r >> 2)) * p.Ncol + lane_row, ga[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int rr = g8 * 8 + i, mb = rr >> 4, r = rr & 15;
          const int rbase = mb * 32 + (r & 3) + 8 * (r >> 2);
          const int row = rbase + 4 * h;
          const float gc = tB[row];
          float v[NACC];
#pragma unroll
          for (int q = 0; q < NACC; ++q) v[q] = rs[q] * (acc2[mb][q][r] * gc - m1[q] - xs[rr][q] * m2[q]) + ga[i][q];
          if (col_ok) vstore<NACC>(p.y + sample + (int64_t)rbase * p.Ncol + lane_row, v);
          float sg = col_ok ? acc2[mb][0][r] * xs[rr][0] + acc2[mb][1][r] * xs[rr][1] : 0.f;
          float sb = col_ok ? acc2[mb][0][r] + acc2[mb][1][r] : 0.f;
          sg = half_sum32(sg);
          sb = half_sum32(sb);
          if ((lane & 31) == 31) {
            red[wave * 128 + row] = sg;
            red[wave * 128 + 64 + row] = sb;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
      if ((threadIdx.x & 255) < 128) {
        const int e = threadIdx.x & 255;
        p.lnb_part[(int64_t)tile * 128 + e] = (red[e] + red[128 + e]) + (red[256 + e] + red[384 + e]);
      }
      __syncthreads();
    }
  }
}

// Host side: fz_mlp_chain modes 0 and 1 at C = 64 (mlp_launch, mlp_chain.hip, has checked the descriptor and filled a and c).
template <typename AT>
int chain64_launch(const fz_mlp_desc* d, const GemmArgsT<AT>& a, const ChainArgsT<AT>& c, fz_stream_t stream) {
  const int ntiles = (int)fz_mlp_partials(d->B, d->V);
  const bool bwd = d->mode != 0, pre = d->pre_in != nullptr;
  // split-bf16 products: ONE 512-thread workgroup per CU around a pre-split weight image, its two halves walking the tiles in
  // pairs; an odd tile count, and fp32-MFMA products, take the 256-thread fp32-MFMA form (with split products in 256 threads
  // the kernel does not stay inside 256 registers: 6 / 23 spilled)
  const bool p512 = products_split(d->products) && ntiles % 2 == 0 && knob_chain64_p512();
  if (pre && !p512) return fail(FZ_E_UNSUPPORTED, "fz_mlp_chain: the fused out-projection at C == 64 needs an even number of tiles");
  void (*kern)(GemmArgsT<AT>, ChainArgsT<AT>, int) =
      pre ? gemm_chain64_kernel<false, AT, false, true, true, true>
      : p512 ? (bwd ? gemm_chain64_kernel<true, AT, false, true, true> : gemm_chain64_kernel<false, AT, false, true, true>)
             : (bwd ? gemm_chain64_kernel<true, AT, false, false> : gemm_chain64_kernel<false, AT, false, false>);
  const int work = p512 ? ntiles / 2 : ntiles, wgs = p512 ? 256 : knob_mlp_wgs(512);
  return launch_lds(kern, dim3((unsigned)(work < wgs ? work : wgs)), dim3(p512 ? 512 : 256), chain64_lds_floats(p512, pre),
                    (hipStream_t)stream, a, c, ntiles);
}
template int chain64_launch<float>(const fz_mlp_desc*, const GemmArgsT<float>&, const ChainArgsT<float>&, fz_stream_t);
template int chain64_launch<bf16>(const fz_mlp_desc*, const GemmArgsT<bf16>&, const ChainArgsT<bf16>&, fz_stream_t);

// 64 -> 64 input gradient + LayerNorm backward over 64 channels: gemm_chain64_kernel, SINGLE form (from gemm_launch, gemm.hip)
template <typename AT>
int chain64_lnb_launch(const fz_gemm_desc* d, const GemmArgsT<AT>& a, fz_stream_t stream) {
  if (d->Ncol % 4 != 0) return fail(FZ_E_UNSUPPORTED, "fz_gemm: voxel count must be a multiple of 4");
  if (!d->lnb_gadd) return fail(FZ_E_UNSUPPORTED, "fz_gemm: the 64-channel LayerNorm-backward epilogue needs the added gradient");
  ChainArgsT<AT> c = {};
  const int ntiles = (int)fz_mlp_partials(d->B, d->Ncol);
  if (gemm_plan_only())   // (fz_gemm_plan's dry run)
    return gemm_plan_form("chain64_lnb %s grid=%dx1", products_split(d->products) ? "split" : "fp32", ntiles < 512 ? ntiles : 512);
  auto kern = products_split(d->products) ? gemm_chain64_kernel<true, AT, true, true> : gemm_chain64_kernel<true, AT, true, false>;
  return launch_lds(kern, dim3((unsigned)(ntiles < 512 ? ntiles : 512)), dim3(256), chain64_lds_floats(false, false),
                    (hipStream_t)stream, a, c, ntiles);
}
template int chain64_lnb_launch<float>(const fz_gemm_desc*, const GemmArgsT<float>&, fz_stream_t);
template int chain64_lnb_launch<bf16>(const fz_gemm_desc*, const GemmArgsT<bf16>&, fz_stream_t);

}  // namespace fz
