// mlp_chain32.hip — the chained MLP of the C = 32 blocks on the matrix cores (gemm.hip has the MFMA mapping it shares):
// gemm_chain_kernel and its host launcher, reached from fz_mlp_chain's dispatcher (mlp_chain.hip).
#include "mlp_chain.h"     // ChainArgsT, chain_stagger, knob_mlp_wgs, knob_chain_fwd_bx, chain32_launch
#include "outproj_fac.h"   // FacArgs, fac_fetch, fac_build: the core's output as the factors of its two windows

namespace fz {

// =================================================================================================
// Kernel C — two chained GEMMs for the C = 32 MLP (layers/mlp.py:54-63 behind the second pre-norm
// residual, factorizer.py:76): the 64-row hidden tensor is produced in the accumulators of GEMM 1,
// transformed in registers and consumed as the B operand of GEMM 2 WITHOUT leaving the wave.
//
// Why no data movement is needed: after GEMM 1 register r of lane (j, h) holds row
// (r&3) + 8(r>>2) + 4h of the row block at column j — and an MFMA K-step wants B[k = h-th of a
// pair][column j].  So accumulator register r IS the operand of K-step r if the A operand (the
// weights, staged in LDS) is laid out with k(step r, half h) = (r&3) + 8(r>>2) + 4h.  The order
// of a reduction is free.
//
//   forward  (BWD = false): z = W1·LN(x1) + b1 → side (kept for the backward);
//                           out = x1 + W2·gelu(z) + b2
//   backward (BWD = true):  gz = (W2ᵀ·g2) ∘ gelu'(z) → side (kept for the weight gradients);
//                           out = LayerNormBackward(W1ᵀ·gz; x1, stats, γ) + g2   (+ dγ, dβ partials)
// Saves one write + one read of the 64-channel tensor per direction against the unfused layers.
// =================================================================================================
// HB = 32-row blocks of the hidden tensor: 2 (mlp_ratio 2, the README model) or 4 (mlp_ratio 4, the
// BraTS bundle, train.yaml:62)
// BX: both GEMMs as split-bf16 products (gemm_bx.h: three-level operands, six products of v_mfma_f32_32x32x16_bf16), weights
// pre-split in LDS as bf16x8 triples (12 KB per GEMM at HB = 2 instead of 8: two workgroups per CU instead of three).  Why: an fp32
// MFMA blocks the SIMD's vector issue for its whole duration — the 128 fp32 MFMAs of a tile were 48 % of this
// kernel's time with nothing running beside them — a bf16 MFMA for a quarter of its own.
// FAC (a trailing FacArgs, with PRE, fp32 storage): the core's output a is not a tensor — GEMM 0's operand tile is rebuilt from
// the rank-1 factors of the core's two windows (outproj_fac.h), fetched one tile ahead like the tile of a they replace and
// staged through the wave's stash rows, which are free until GEMM 0's epilogue writes x1 there.
// (Six-wave workgroups — 73 KB, two per CU, three waves per SIMD again — were tried and are slower than these four-wave ones at two
// waves per SIMD: 1.06 against 0.97 ms per step for the two launches, fp32 form 1.09; profiles/r04_chain_fwd_bx_ab.log.)
template <bool BWD, int NACC, int HB, typename AT = float, bool BX = false, bool PRE = false, typename... DropX>
__global__ __launch_bounds__(256, (NACC == 2 && HB == 2 && !BWD && !BX) ? 3 : 2) void gemm_chain_kernel(GemmArgsT<AT> p, ChainArgsT<AT> c, int ntiles, DropX... dx) {
  constexpr bool FAC = is_fac_v<DropX...>;      // the factor form: one trailing FacArgs
  constexpr bool DROP = sizeof...(DropX) > 0 && !FAC;   // the block-dropout form: one trailing DropArgs (the p = 0 kernels have no such argument)
  const DropArgs dr = drop_of(dx...);
  const FacArgs fa = fac_of(dx...);
  static_assert(!FAC || (PRE && !BWD && NACC == 2 && sizeof(AT) == 4), "factors: the forward chain with the out-projection in front, fp32 storage");
  static_assert(kFacLds <= 32 * 32 * NACC, "the factor staging area lives in the wave's stash rows");
  static_assert(!DROP || (PRE && !BWD && NACC == 2), "dropout: the forward chain with the out-projection in front");
  constexpr int NW = 4;
  constexpr int HID = 32 * HB, N1 = BX ? 1536 * HB : 16 * HB * 64;  // hidden rows; floats of each staged weight block
  static_assert(!BX || (!BWD && NACC == 2), "the split-bf16 form is the forward chain");
  static_assert(!PRE || (BX && HB == 2), "the out-projection in front of the chain: split-bf16 forward, hidden 64");
  __shared__ __attribute__((aligned(16))) float As1[N1];
  __shared__ __attribute__((aligned(16))) float As2[N1];
  __shared__ __attribute__((aligned(16))) float As0[PRE ? 1536 : 4];   // (PRE) out_proj weights, pre-split: [g (2)][level][lane] x 16 B
  __shared__ float tW[HID];
  __shared__ float tB[32];
  __shared__ float tB0[32];                                              // (PRE) out_proj bias
  __shared__ float tP[PRE ? 4 * 32 + 4 : 1];                             // (PRE + head) head weights, rows >= postM zero | bias
  __shared__ float red[256];
  // raw operand tile of each wave (32 channels x 32*NACC columns): the epilogue needs the SAME tensor
  // again in the accumulator layout (residual x1 / added gradient g2) — served from LDS instead of a
  // second global read (PMC: 1 of 5 resp. 8 plane-sets of traffic)
  __shared__ __attribute__((aligned(16))) float stash[NW][32][32 * NACC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int tiles_per_sample = (int)((p.Ncol + 32 * NW * NACC - 1) / (32 * NW * NACC));
  chain_stagger(c.stagger);

  if constexpr (BX) {
    // operand items of 8 steps each: As1x[g (2)][rb (HB)][level][lane], As2x[g (2 HB)][level][lane]
    for (int it = threadIdx.x; it < (PRE ? 4 * HB + 2 : 4 * HB) * 64; it += 64 * NW) {
      float wv[8];
      const int l = it & 63;
      __bf16* dst;
      if (PRE && it >= 4 * HB * 64) {   // GEMM 0: element e of lane half h = channel 2 (8g + e) + h of a (the operand tile's order)
        const int g = (it - 4 * HB * 64) >> 6;
#pragma unroll
        for (int e = 0; e < 8; ++e) wv[e] = c.preW[(l & 31) * 32 + 2 * (8 * g + e) + (l >> 5)];
        dst = reinterpret_cast<__bf16*>(As0) + (g * 3 * 64 + l) * 8;
      } else if (it < 2 * HB * 64) {
        const int rb = (it >> 6) % HB, g = it / (64 * HB);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          // (PRE: the column operand of GEMM 1 is x̂ in the ACCUMULATOR layout of GEMM 0 — register r = 8g + e of lane half h is
          //  channel (r & 3) + 8 (r >> 2) + 4h, the order GEMM 2 uses for the hidden tensor)
          const int r = 8 * g + e;
          const int kk = PRE ? (r & 3) + 8 * (r >> 2) + 4 * (l >> 5) : 2 * r + (l >> 5);
          wv[e] = weight_at(p, rb * 32 + (l & 31), kk) * p.ln_g[kk];
        }
        dst = reinterpret_cast<__bf16*>(As1) + ((g * HB + rb) * 3 * 64 + l) * 8;
      } else {
        const int g = (it - 2 * HB * 64) >> 6;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int s2 = 8 * g + e, r = s2 & 15, rb = s2 >> 4;
          const int kk = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), m = l & 31;
          wv[e] = c.wB_t ? c.wB[(int64_t)kk * c.ldwB + m] : c.wB[(int64_t)m * c.ldwB + kk];
        }
        dst = reinterpret_cast<__bf16*>(As2) + (g * 3 * 64 + l) * 8;
      }
      bx8 t3[3];
      bx_split<3>(wv, t3);
#pragma unroll
      for (int i = 0; i < 3; ++i) *reinterpret_cast<bx8*>(dst + i * 64 * 8) = t3[i];
    }
  } else
  // weights in operand order (8 independent loads per thread before the LDS stores)
  for (int base = threadIdx.x; base < 2 * N1; base += 256 * 8) {
    float tmp[8];
#pragma unroll
    for (int uu = 0; uu < 8; ++uu) {
      const int idx = base + uu * 256;
      float wv;
      if (idx < N1) {  // GEMM 1: step a, row block rb
        const int l = idx & 63, rb = (idx >> 6) % HB, a = idx / (64 * HB);
        const int m = rb * 32 + (l & 31), k = 2 * a + (l >> 5);
        wv = weight_at(p, m, k);
        if (!BWD) wv *= p.ln_g[k];
      } else {           // GEMM 2: step (rb, r) consumes accumulator register r of row block rb
        const int i2 = idx - N1;
        const int l = i2 & 63, s2 = i2 >> 6;
        const int r = s2 & 15, rb = s2 >> 4;
        const int k = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), m = l & 31;
        wv = c.wB_t ? c.wB[(int64_t)k * c.ldwB + m] : c.wB[(int64_t)m * c.ldwB + k];
      }
      tmp[uu] = wv;
    }
#pragma unroll
    for (int uu = 0; uu < 8; ++uu) {
      const int idx = base + uu * 256;
      if (idx < N1) As1[idx] = tmp[uu]; else As2[idx - N1] = tmp[uu];
    }
  }
  if (BWD) {
    if (threadIdx.x < 32) tB[threadIdx.x] = p.lnb_g[threadIdx.x];
  } else {
    for (int r = threadIdx.x; r < HID; r += blockDim.x) {
      float t = 0.f;
      for (int k = 0; k < 32; ++k) t += weight_at(p, r, k) * p.ln_b[k];
      tW[r] = t + (p.bias ? p.bias[r] : 0.f);
      if (r < 32) tB[r] = c.biasB ? c.biasB[r] : 0.f;
      if (PRE && r < 32) tB0[r] = c.preB ? c.preB[r] : 0.f;
    }
    if constexpr (PRE) {
      if (c.postOut != nullptr && threadIdx.x < 4 * 32 + 4) {
        const int i = threadIdx.x;
        if (i < 128) tP[i] = (i >> 5) < c.postM ? c.postW[i] : 0.f;
        else tP[i] = ((i - 128) < c.postM && c.postB) ? c.postB[i - 128] : 0.f;
      }
    }
  }

  // persistent over column tiles: the operand of the NEXT tile is fetched as soon as GEMM 1 has
  // consumed the current one, so its latency hides behind the transform, GEMM 2 and the epilogue
  int tile = blockIdx.x;
  float bv[16][NACC];
  float xr[PRE ? 16 : 1][NACC];   // (PRE) residual rows of the NEXT / current tile
  FacTile ft;                     // (FAC) the factors of the NEXT / current tile
  // operand loads: channel 2s + h → uniform part (b*32 + 2s)*V in scalar registers + ONE lane offset
  auto fetch_tile = [&](int t) {
    const int bt = t / tiles_per_sample;
    const int64_t ct = ((int64_t)(t % tiles_per_sample) * NW + wave) * (32 * NACC) + NACC * j;
    const unsigned lo = (unsigned)h * (unsigned)p.Ncol + (unsigned)(ct < p.Ncol ? ct : 0);
    if constexpr (FAC) {
      const int64_t n0 = ((int64_t)(t % tiles_per_sample) * NW + wave) * (32 * NACC);
      fac_fetch(fa, bt, (unsigned)(n0 < p.Ncol ? n0 : 0), lane, ft);
    } else {
    const AT* xb = (PRE ? c.preA : p.x[0]) + (int64_t)bt * 32 * p.Ncol;
#pragma unroll
    for (int s = 0; s < 16; ++s) vload<NACC>(xb + (int64_t)(2 * s) * p.Ncol + lo, bv[s]);
    }
    if constexpr (PRE) {   // the residual rows of x in the accumulator layout (row (r & 3) + 8 (r >> 2) + 4h)
      const unsigned lr = (unsigned)(4 * h) * (unsigned)p.Ncol + (unsigned)(ct < p.Ncol ? ct : 0);
      const AT* rb0 = c.preRes + (int64_t)bt * 32 * p.Ncol;
#pragma unroll
      for (int r = 0; r < 16; ++r) vload<NACC>(rb0 + (int64_t)((r & 3) + 8 * (r >> 2)) * p.Ncol + lr, xr[PRE ? r : 0]);
    }
  };
  fetch_tile(tile);
  __syncthreads();

  for (; tile < ntiles; tile += gridDim.x) {
    // compiler-only fence: without it the loop-invariant LDS reads (row constants, 48 per lane) are
    // hoisted out of the tile loop and kept in VGPRs, which spills the accumulators
    asm volatile("" ::: "memory");
    const int b = tile / tiles_per_sample;
    const int64_t col_off = ((int64_t)(tile % tiles_per_sample) * NW + wave) * (32 * NACC) + NACC * j;
    const bool col_ok = col_off < p.Ncol;
    const int64_t nc = col_ok ? col_off : 0;
    const unsigned lane_row = (unsigned)(4 * h) * (unsigned)p.Ncol + (unsigned)nc;
    if constexpr (PRE) {
      // ---- GEMM 0: x1 = W_o a + b_o + x on the accumulators; x1 -> HBM (for the backward) and -> stash (the chain's residual);
      //      bv becomes x̂ in the ACCUMULATOR layout (register r = row (r & 3) + 8 (r >> 2) + 4h) — GEMM 1's weights are staged
      //      in that order ----
      if constexpr (FAC) fac_build(fa, ft, &stash[wave][0][0], lane, bv);
      f32x16 acc0[NACC];
#pragma unroll
      for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[q][r] = 0.f;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        bx8 aop[3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
          aop[i] = *reinterpret_cast<const bx8*>(reinterpret_cast<const __bf16*>(As0) + ((g * 3 + i) * 64 + lane) * 8);
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
          float x8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) x8[e] = bv[8 * g + e][q];
          bx8 bop[3];
          bx_split<3>(x8, bop);
          bx_mfma<3, 3>(acc0[q], aop, bop);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rbase = (r & 3) + 8 * (r >> 2);
        const int row = rbase + 4 * h;
        const float add = tB0[row];
        uint32_t dk = 0;
        if constexpr (DROP) dk = drop_bits(dr, 0, b, 32, row, nc);
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
          float v;
          if constexpr (DROP) v = drop_f(dr, 0, dk, q, acc0[q][r] + add) + xr[PRE ? r : 0][q];
          else v = acc0[q][r] + add + xr[PRE ? r : 0][q];
          // bf16 storage: everything downstream (LayerNorm, the chain's residual, the backward) sees the STORED x1, as in the
          // two-launch form where the chain reads it back
          if constexpr (sizeof(AT) == 2) v = (float)(AT)v;
          bv[r][q] = v;
        }
        vstore<NACC>(&stash[wave][row][NACC * j], bv[r]);
        if (col_ok) vstore<NACC>(c.preOut + ((int64_t)b * 32 + rbase) * p.Ncol + lane_row, bv[r]);
      }
    } else {
#pragma unroll
    for (int s = 0; s < 16; ++s) vstore<NACC>(&stash[wave][2 * s + h][NACC * j], bv[s]);
    }

    if (!BWD) {
      // exact two-pass LayerNorm statistics (this lane holds the parity-h half of the channels; PRE: rows 4h + ...: also half)
      float mu[NACC], rs[NACC];
#pragma unroll
      for (int e = 0; e < NACC; ++e) {
        float t = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) t += bv[s][e];
        t += __shfl_xor(t, 32, 64);
        mu[e] = t / 32.0f;
      }
#pragma unroll
      for (int e = 0; e < NACC; ++e) {
        float t = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const float d = bv[s][e] - mu[e];
          t += d * d;
        }
        t += __shfl_xor(t, 32, 64);
        rs[e] = 1.0f / sqrtf(t / 32.0f + p.ln_eps);
      }
#pragma unroll
      for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int e = 0; e < NACC; ++e) bv[s][e] = (bv[s][e] - mu[e]) * rs[e];
      if (p.stats_out != nullptr && h == 0 && col_ok) {
        float* so = p.stats_out + (int64_t)b * 2 * p.Vin;
        vstore<NACC>(so + col_off, mu);
        vstore<NACC>(so + p.Vin + col_off, rs);
      }
    }

    // ---- GEMM 1: 64 rows x 128 columns per wave ----
    f32x16 acc1[HB][NACC];
#pragma unroll
    for (int rb = 0; rb < HB; ++rb)
#pragma unroll
      for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[rb][q][r] = 0.f;
    if constexpr (BX) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {   // element e of lane half h = K-step 8g + e of the fp32 form (channel 2 (8g + e) + h)
        bx8 bop[NACC][3];
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
          float x8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) x8[e] = bv[8 * g + e][q];
          bx_split<3>(x8, bop[q]);
        }
#pragma unroll
        for (int rb = 0; rb < HB; ++rb) {
          bx8 aop[3];
#pragma unroll
          for (int i = 0; i < 3; ++i)
            aop[i] = *reinterpret_cast<const bx8*>(reinterpret_cast<const __bf16*>(As1) + (((g * HB + rb) * 3 + i) * 64 + lane) * 8);
#pragma unroll
          for (int q = 0; q < NACC; ++q) bx_mfma<3, 3>(acc1[rb][q], aop, bop[q]);
        }
      }
    } else {
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int rb = 0; rb < HB; ++rb) {
        const float av = As1[(s * HB + rb) * 64 + lane];
#pragma unroll
        for (int q = 0; q < NACC; ++q) acc1[rb][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[s][q], acc1[rb][q], 0, 0, 0);
      }
    }

    // ---- prefetch the operand of the next tile (clamped re-read of this one on the last pass) ----
    fetch_tile(tile + gridDim.x < ntiles ? tile + gridDim.x : tile);

    // ---- hidden tensor: transform in registers, keep a copy in HBM for the other pass ----
    if (!BWD) {
#pragma unroll
      for (int rb = 0; rb < HB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rbase = rb * 32 + (r & 3) + 8 * (r >> 2);
          const int row = rbase + 4 * h;
          const int64_t ob = ((int64_t)b * HID + rbase) * p.Ncol;  // uniform row part; + one 32-bit lane offset
          float v[NACC];
          const float add = tW[row];
#pragma unroll
          for (int q = 0; q < NACC; ++q) v[q] = acc1[rb][q][r] + add;
          if (col_ok && c.side != nullptr) vstore<NACC>(c.side + ob + lane_row, v);   // (null: timing probe FZ_CHAIN_NOZ1)
          if constexpr (NACC == 2) {
            float gq[2];
            gelu2_f(v, gq);
            if constexpr (DROP) {
              const uint32_t dk = drop_bits(dr, 1, b, HID, row, nc);
              gq[0] = drop_f(dr, 1, dk, 0, gq[0]);
              gq[1] = drop_f(dr, 1, dk, 1, gq[1]);
            }
            acc1[rb][0][r] = gq[0]; acc1[rb][1][r] = gq[1];
          } else {
#pragma unroll
            for (int q = 0; q < NACC; ++q) acc1[rb][q][r] = gelu_f(v[q]);
          }
        }
    } else {
      // groups of 8 rows: 8 loads of the saved pre-activation in flight, then 8 transforms + stores
      // (bounded on purpose: the scheduler otherwise hoists all 32 loads and spills accumulators)
#pragma unroll
      for (int g8 = 0; g8 < 2 * HB; ++g8) {
        float e[8][NACC];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int rr = g8 * 8 + i, rb = rr >> 4, r = rr & 15;
          const int rbase = rb * 32 + (r & 3) + 8 * (r >> 2);
          vload<NACC>(p.emul + ((int64_t)b * HID + rbase) * p.Ncol + lane_row, e[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int rr = g8 * 8 + i, rb = rr >> 4, r = rr & 15;
          const int rbase = rb * 32 + (r & 3) + 8 * (r >> 2);
          float v[NACC];
#pragma unroll
          for (int q = 0; q < NACC; ++q) v[q] = acc1[rb][q][r] * gelu_grad_f(e[i][q]);
          if (col_ok) vstore<NACC>(c.side + ((int64_t)b * HID + rbase) * p.Ncol + lane_row, v);
#pragma unroll
          for (int q = 0; q < NACC; ++q) acc1[rb][q][r] = v[q];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    // ---- GEMM 2: 32 rows, K = 64 straight from the accumulators of GEMM 1 ----
    f32x16 acc2[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[q][r] = 0.f;
    if constexpr (BX) {
#pragma unroll
      for (int g = 0; g < 2 * HB; ++g) {   // steps (rb, r) = (g >> 1, 8 (g & 1) + e): accumulator registers as the column operand
        bx8 aop[3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
          aop[i] = *reinterpret_cast<const bx8*>(reinterpret_cast<const __bf16*>(As2) + ((g * 3 + i) * 64 + lane) * 8);
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
          float x8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) x8[e] = acc1[g >> 1][q][8 * (g & 1) + e];
          bx8 bop[3];
          bx_split<3>(x8, bop);
          bx_mfma<3, 3>(acc2[q], aop, bop);
        }
      }
    } else {
#pragma unroll
    for (int rb = 0; rb < HB; ++rb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float av = As2[(rb * 16 + r) * 64 + lane];
#pragma unroll
        for (int q = 0; q < NACC; ++q) acc2[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, acc1[rb][q][r], acc2[q], 0, 0, 0);
      }
    }

    if (BWD) {
      lnbwd_block<NACC, true, true>(p, acc2, b, col_off, col_ok, lane, wave, red, tile, tB, &stash[wave][0][0]);
      __syncthreads();  // red is reused by the next tile
    } else if (col_ok) {
      const bool post = PRE && c.postOut != nullptr;   // uniform
      float pl[4][NACC] = {};
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rbase = (r & 3) + 8 * (r >> 2);
        const int row = rbase + 4 * h;
        const int64_t ob = ((int64_t)b * 32 + rbase) * p.Ncol;
        const float add = tB[row];
        float e[NACC], v[NACC];
        vload<NACC>(&stash[wave][row][NACC * j], e);
        if constexpr (DROP) {
          const uint32_t dk = drop_bits(dr, 2, b, 32, row, nc);
#pragma unroll
          for (int q = 0; q < NACC; ++q) v[q] = drop_f(dr, 2, dk, q, acc2[q][r] + add) + e[q];
        } else {
#pragma unroll
        for (int q = 0; q < NACC; ++q) v[q] = acc2[q][r] + add + e[q];
        }
        vstore<NACC>(p.y + ob + lane_row, v);
        if (PRE && post) {   // the head sees what a separate launch would read back: the STORED value (bf16 storage: rounded)
#pragma unroll
          for (int q = 0; q < NACC; ++q) {
            const float vs = sizeof(AT) == 2 ? (float)(AT)v[q] : v[q];
#pragma unroll
            for (int o = 0; o < 4; ++o) pl[o][q] += tP[o * 32 + row] * vs;
          }
        }
      }
      if (PRE && post) {   // rows 4h + ... of this lane + the other half's (same column: both lanes are active together)
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          float v[NACC];
#pragma unroll
          for (int q = 0; q < NACC; ++q) v[q] = pl[o][q] + __shfl_xor(pl[o][q], 32, 64) + tP[128 + o];
          if (h == 0 && o < c.postM) vstore<NACC>(c.postOut + ((int64_t)b * c.postM + o) * p.Ncol + nc, v);
        }
      }
    }
  }
}

// Host side: fz_mlp_chain modes 0 and 1 at C = 32 (mlp_launch, mlp_chain.hip, has checked the descriptor and filled a and c).
// Replaces, per FactorizerBlock, Linear∘LayerNorm + Linear∘GELU + residual (layers/mlp.py:54-63, factorizer.py:76) in the
// forward and the two input-gradient GEMMs + LayerNorm backward in the backward.
template <typename AT>
int chain32_launch(const fz_mlp_desc* d, const fz_mlp_dropout* drop, const fz_outproj_fac* fac, const GemmArgsT<AT>& a, const ChainArgsT<AT>& c,
                   fz_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  const int ntiles = (int)fz_mlp_partials(d->B, d->V);
  const bool bwd = d->mode != 0, pre = d->pre_in != nullptr || fac;   // (fac: the out-projection's operand as the core's factors)
  // forward at hidden 64 on split-bf16 products (FZ_CHAIN_FWD_BX=0 in a probe build: the fp32-MFMA forward chain)
  const bool bx = !bwd && d->H == 64 && products_split(d->products) && knob_chain_fwd_bx();
  // resident workgroups, each walking tiles with a stride of the grid: three per CU for the fp32-MFMA forms at hidden 64,
  // two for hidden 128 and for the split-bf16 form (12 KB of LDS per GEMM instead of 8)
  const int wgs = knob_mlp_wgs(d->H == 128 || bx ? 512 : 768);
  const dim3 grid((unsigned)(ntiles < wgs ? ntiles : wgs)), block(256);
  if (bwd) {
    if (d->H == 128) hipLaunchKernelGGL((gemm_chain_kernel<true, 2, 4>), grid, block, 0, st, a, c, ntiles);
    else hipLaunchKernelGGL((gemm_chain_kernel<true, 2, 2>), grid, block, 0, st, a, c, ntiles);
  } else if (d->H == 128) hipLaunchKernelGGL((gemm_chain_kernel<false, 2, 4>), grid, block, 0, st, a, c, ntiles);
  else if (!bx) hipLaunchKernelGGL((gemm_chain_kernel<false, 2, 2>), grid, block, 0, st, a, c, ntiles);
  else if (!pre) hipLaunchKernelGGL((gemm_chain_kernel<false, 2, 2, AT, true>), grid, block, 0, st, a, c, ntiles);
  else if (fac) {   // (mlp_check has refused the factor form outside fp32 storage, hidden 64, split-bf16 products, no dropout)
    if constexpr (sizeof(AT) == 4) {
      FacArgs fa;
      const int rc = fac_args(fac, d->V, "fz_mlp_chain_fac", fa);
      if (rc != FZ_OK) return rc;
      hipLaunchKernelGGL((gemm_chain_kernel<false, 2, 2, AT, true, true, FacArgs>), grid, block, 0, st, a, c, ntiles, fa);
    } else {
      return fail(FZ_E_UNSUPPORTED, "fz_mlp_chain_fac: fp32 storage only");
    }
  }
  else if (!drop) hipLaunchKernelGGL((gemm_chain_kernel<false, 2, 2, AT, true, true>), grid, block, 0, st, a, c, ntiles);
  else
    hipLaunchKernelGGL((gemm_chain_kernel<false, 2, 2, AT, true, true, DropArgs>), grid, block, 0, st, a, c, ntiles,
                       drop_args(drop->m0, drop->m1, drop->m2, drop->s0, drop->s1, drop->s2, d->V));
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
template int chain32_launch<float>(const fz_mlp_desc*, const fz_mlp_dropout*, const fz_outproj_fac*, const GemmArgsT<float>&, const ChainArgsT<float>&, fz_stream_t);
template int chain32_launch<bf16>(const fz_mlp_desc*, const fz_mlp_dropout*, const fz_outproj_fac*, const GemmArgsT<bf16>&, const ChainArgsT<bf16>&, fz_stream_t);

}  // namespace fz
