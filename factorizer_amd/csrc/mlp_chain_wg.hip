// mlp_chain_wg.hip — the C = 32 MLP backward chain that also forms the weight gradients (gemm.hip has the MFMA mapping it shares):
// gemm_chain_bwd_wg_kernel, the row count of its workspace, and its host launcher, reached from fz_mlp_chain's dispatcher
// (mlp_chain.hip).
#include "mlp_chain.h"     // ChainArgsT, chain_stagger, chain_wg_lds_floats, launch_lds, chain_wg_launch
#include "finish.h"        // kWgRow and the job that adds the weight-gradient rows

namespace fz {

// =================================================================================================
// MLP backward chain WITH the two weight gradients (C = 32, hidden 64): the unfused step reads g2 and z1
// again for dW2 = g2 ⊗ gelu(z1) and writes + re-reads gz1 for dW1 = gz1 ⊗ LN(x1) — 13 plane-sets of traffic per
// block (7 chain + 3 + 3) where 5 suffice (g2, z1 ×2, x1 in; gx1 out).  A weight gradient reduces over VOXELS, so
// its MFMA operands need the channel on the lane axis; everything in the chain has the voxel there.  Each wave
// turns its tile through wave-private LDS ([channel][voxel] rows, stride 66 ≡ 2 (mod 32): ds_read_b32 banks are
// (a/4) mod 32 per 32-lane half, and the (channel16, k4 ∈ {0,1} resp. {2,3}) lanes of a v_mfma_f32_16x16x4_f32 operand
// read then hit 32 different banks; the 8-byte tile writes / accumulator-layout reads are conflict-free at any stride):
//   Bf  32 x 64: g2 (operand of dW2) during the first pass, then LN-normalised x1 (operand of dW1, and the
//                LayerNorm backward reads it back in the accumulator layout);
//   T   16 x 64: one 16-channel block of gelu(z1) (pass A) resp. gz1 (pass B) at a time.
// The (dW2 | dW1 | db2 | db1) sums stay in registers across the tiles of the persistent workgroup, are added
// over its four waves through LDS at the end and leave as one row of `wpart` per workgroup;
// the FK_CHAIN_WG job of the finish kernel (finish.h) adds the rows in index order (no float atomics) and applies the LayerNorm affine to dW1.
// 13 KB of LDS per wave + 64 accumulator registers: two workgroups per CU (the plain chain runs three).
// =================================================================================================
// (kWgRow — floats of one wpart row: dW2 [32][64] | S1 [64][32] | db2 | db1 | dγ | dβ — lives in finish.h with the job that adds the rows)

// gelu(x) and gelu'(x) with ONE exponential: erf(x/√2) by Abramowitz-Stegun 7.1.26 (fast_erf, fz_common.h) needs
// exp(−x²/2), which is also the Gaussian density of gelu'
__device__ __forceinline__ void gelu_both(float x, float& g, float& dg) {
  const float ax = fabsf(x) * 0.70710678118654752f;
  const float E = __expf(-0.5f * x * x);
  const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * ax);
  const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
  const float r = 1.0f - poly * E;                       // erf(|x|/√2)
  const float cdf = 0.5f * (1.0f + __builtin_copysignf(r, x));
  g = x * cdf;
  dg = cdf + x * (0.3989422804014327f * E);
}

// The same for the lane's two voxels at once on packed fp32 (v_pk_fma_f32 / v_pk_mul_f32: two lanes' worth of fp32 per
// issue slot; the exponentials and reciprocals stay scalar) — same operations in the same order, so the results are
// those of gelu_both; ≈ 23 instead of 44 VALU instructions per voxel pair in the VALU-heaviest phase of the fused kernel.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <bool SEL = false>   // SEL: sign by compare + select (the two-launch hidden-128 form keeps its round-3 register allocation)
__device__ __forceinline__ void gelu_both2(const float (&x)[2], float (&g)[2], float (&dg)[2]) {
  const f32x2 xv = {x[0], x[1]};
  const f32x2 ax = f32x2{fabsf(x[0]), fabsf(x[1])} * 0.70710678118654752f;
  const f32x2 xx = (xv * -0.5f) * xv;
  const f32x2 E = {__expf(xx[0]), __expf(xx[1])};
  const f32x2 den = ax * 0.3275911f + 1.0f;
  const f32x2 t = {__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
  const f32x2 poly = t * (t * (t * (t * (t * 1.061405429f + -1.453152027f) + 1.421413741f) + -0.284496736f) + 0.254829592f);
  const f32x2 r = 1.0f - poly * E;
  f32x2 rs;
  if constexpr (SEL) rs = f32x2{x[0] < 0.f ? -r[0] : r[0], x[1] < 0.f ? -r[1] : r[1]};
  else rs = f32x2{__builtin_copysignf(r[0], x[0]), __builtin_copysignf(r[1], x[1])};   // one v_bfi_b32 instead of compare + select (fast_erf, fz_common.h)
  const f32x2 cdf = (rs + 1.0f) * 0.5f;
  const f32x2 gv = xv * cdf;
  const f32x2 dv = cdf + xv * (E * 0.3989422804014327f);
  g[0] = gv[0]; g[1] = gv[1];
  dg[0] = dv[0]; dg[1] = dv[1];
}

// (HALVES / HALF are compile-time: with a run-time half the one-launch form lost its spill-free register allocation —
// 32 spilled VGPRs, 0.94 -> 1.03 ms per launch, 215 MB of scratch writes in the WRITE_SIZE counter.)
// BX: the two input-gradient GEMMs (half of the kernel's matrix work) run as split-bf16 products (gemm_bx.hip): the K-steps
// of two of the fp32 form are packed eight at a time — element e of lane half h of a 32x32x16 bf16 MFMA = step 8g + e —
// with the weights pre-split in LDS (As1 / As2 hold bf16x8 triples instead of floats: 12 KB each instead of 8).  The two
// weight-gradient passes keep their transposed fp32 operands (v_mfma_f32_16x16x4_f32).
// WGB [r6]: the two weight-gradient passes on the bf16 matrix pipe as well.  Each value that enters a voxel reduction (g2, gelu(z1),
// x̂, gz1) is split ONCE, by the lane that holds it, into two bf16 levels (hi = rne(x), lo = rne(x - hi): 16 significand bits) and
// parked in wave-private LDS as a hi plane and a lo plane of [channel][64 voxels] bf16 — 2 x 2 bytes per value, the fp32 footprint —
// with the 16-byte voxel chunks of a row XOR-swizzled by (row & 7): the pair stores of the voxel-owner lanes and the 16-byte operand
// reads of the channel-owner lanes (lane (l16, k4) = channel l16, voxels 32 ks + 8 k4 .. + 7: one ds_read_b128 per level) are both
// conflict-free.  a·b = a_lo·b_hi + a_hi·b_lo + a_hi·b_hi on v_mfma_f32_16x16x32_bf16: 96 MFMAs of 16 cycles per tile that overlap
// the other wave's vector work, in place of 256 exclusive v_mfma_f32_16x16x4_f32 of 32 cycles.  The accumulator layout of the
// 16x16 tile does not depend on K: dW2 / dW1 registers, the partial rows and the finish job are unchanged.  g2's two levels are the
// ones GEMM 1 splits anyway; the bias sums Σ_v g2, Σ_v gz1 come from the same operand registers through v_dot2c_f32_bf16.
// Error: each product carries 2^-16 relative (the dropped a_lo·b_lo and third levels), random in sign over the >= 10^5 voxels of a
// sum (tests/test_gpu_dense.py: against float64 next to the fp32-MFMA form).
typedef __bf16 wg2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void wg_split2(float x0, float x1, unsigned& hi, unsigned& lo) {
  fx2 v = {x0, x1};
  const wg2 a = __builtin_convertvector(v, wg2);
  v = v - __builtin_convertvector(a, fx2);
  const wg2 b = __builtin_convertvector(v, wg2);
  hi = __builtin_bit_cast(unsigned, a);
  lo = __builtin_bit_cast(unsigned, b);
}
__device__ __forceinline__ float2 wg_join2(unsigned hi, unsigned lo) {   // the two values a (hi, lo) dword pair stands for
  return make_float2(__uint_as_float(hi << 16) + __uint_as_float(lo << 16),
                     __uint_as_float(hi & 0xffff0000u) + __uint_as_float(lo & 0xffff0000u));
}
__device__ __forceinline__ float wg_sum8(const bx8& hi, const bx8& lo, float acc) {   // acc + Σ of the 8 values of a level pair
  const wg2 one = {(__bf16)1.0f, (__bf16)1.0f};
  struct Q { wg2 p[4]; };
  const Q h = __builtin_bit_cast(Q, hi), l = __builtin_bit_cast(Q, lo);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc = __builtin_amdgcn_fdot2_f32_bf16(l.p[i], one, acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(h.p[i], one, acc, false);
  }
  return acc;
}
__device__ __forceinline__ void wg_mfma3(f32x4& acc, const bx8& ah, const bx8& al, const bx8& bh, const bx8& bl) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
}

template <typename AT, int HALVES = 1, int HALF = 0, bool BX = false, bool WGB = false>
__global__ __launch_bounds__(256, 2) void gemm_chain_bwd_wg_kernel(GemmArgsT<AT> p, ChainArgsT<AT> c, int ntiles, float* wpart,
                                                                   float* glp) {
  static_assert(!WGB || (BX && HALVES == 1), "WGB: the one-launch split-bf16 form");
  constexpr int NACC = 2, HB = 2, HID = 64 * HALVES, N1 = BX ? 3072 : 16 * HB * 64;   // floats of each staged weight block
  constexpr int NTA = BxTerms<AT>::A, NTB = bx_terms_b<AT>(BXPRO_GELU);
  // WGF: GEMM 2's K-groups run inside pass B and its operand split also feeds the planes (fp32 storage; the bf16-storage
  // instantiation has no 32 registers for acc2 across pass B — 2 spilled registers — and splits gz1 a second time instead)
  constexpr bool WGF = WGB && sizeof(AT) == 4;
  constexpr int half = HALF;
  constexpr int hoff = 64 * HALF;             // first hidden row of this launch
  constexpr bool last = HALF == HALVES - 1;   // this launch ends with the LayerNorm backward
  constexpr int kWave = WGB ? 3072 : 48 * kTS;   // floats of one wave's (Bf | T) region (WGB: hi | lo planes of 32 + 16 rows x 128 B)
  extern __shared__ __attribute__((aligned(16))) float fz_lds_cw[];
  float* As1 = fz_lds_cw;
  float* As2 = As1 + N1;
  float* tB = As2 + N1;                       // gamma[32]
  float* red = tB + 32;                       // [4][64]
  float* R = red + 256;                       // 4 wave regions
  static_assert(2 * N1 + 32 + 256 + 4 * kWave == chain_wg_lds_floats(BX, WGB), "the launcher's dynamic LDS ends where this carve-up does");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int l16 = lane & 15, k4 = lane >> 4;
  float* Bf = R + wave * kWave;
  float* T = Bf + 32 * kTS;
  // WGB planes of this wave (bytes): GH [0, 4096) g2 / x̂ hi, GL [4096, 8192) lo, TH [8192, 10240) the 16-row group hi, TL lo.
  // element (row, voxel v) of a plane: row * 128 + (((v >> 3) ^ (row & 7)) << 4) + (v & 7) * 2
  char* const PL = reinterpret_cast<char*>(Bf);
  constexpr int kGL = 4096, kTH = 8192, kTL = 10240;
  // voxel-owner stores of the pair (2j, 2j+1): rows 2s + h (operand layout) at wop[s & 3] + s * 256; rows (i & 3) + 8 (i >> 2) + 4h
  // (accumulator layout) at wac[i & 3] + (i & 3) * 128 + (i >> 2) * 1024; channel-owner reads of block b, k-step ks at rd[ks] + b * 2048
  unsigned wop[4], wac[4], rd[2];
  if constexpr (WGB) {
    const unsigned ob = (unsigned)h * 128u + ((((unsigned)j >> 2) ^ (unsigned)h) << 4) + ((unsigned)j & 3u) * 4u;
    const unsigned ab = (unsigned)h * 512u + ((((unsigned)j >> 2) ^ (4u * (unsigned)h)) << 4) + ((unsigned)j & 3u) * 4u;
#pragma unroll
    for (int q = 0; q < 4; ++q) { wop[q] = ob ^ ((unsigned)q << 5); wac[q] = ab ^ ((unsigned)q << 4); }
    rd[0] = (unsigned)l16 * 128u + ((((unsigned)k4) ^ ((unsigned)l16 & 7u)) << 4);
    rd[1] = rd[0] ^ 64u;
  }
  const int tiles_per_sample = (int)((p.Ncol + 128 * NACC - 1) / (128 * NACC));
  chain_stagger(c.stagger);

  if constexpr (BX) {
    // 512 operand items of 8 steps each: As1x[g (2)][rb (2)][term][lane], As2x[g (4)][term][lane]
    for (int it = threadIdx.x; it < 512; it += 256) {
      float wv[8];
      const int l = it & 63;
      __bf16* dst;
      if (it < 256) {
        const int rb = (it >> 6) & 1, g = it >> 7;
#pragma unroll
        for (int e = 0; e < 8; ++e) wv[e] = weight_at(p, hoff + rb * 32 + (l & 31), 2 * (8 * g + e) + (l >> 5));
        dst = reinterpret_cast<__bf16*>(As1) + ((g * HB + rb) * NTA * 64 + l) * 8;
      } else {
        const int g = (it - 256) >> 6;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int s2 = 8 * g + e, r = s2 & 15, rb = s2 >> 4;
          const int k = hoff + rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), m = l & 31;
          wv[e] = c.wB_t ? c.wB[(int64_t)k * c.ldwB + m] : c.wB[(int64_t)m * c.ldwB + k];
        }
        dst = reinterpret_cast<__bf16*>(As2) + (g * NTA * 64 + l) * 8;
      }
      bx8 t3[NTA];
      bx_split<NTA>(wv, t3);
#pragma unroll
      for (int i = 0; i < NTA; ++i) *reinterpret_cast<bx8*>(dst + i * 64 * 8) = t3[i];
    }
  } else {
  for (int base = threadIdx.x; base < 2 * N1; base += 256 * 8) {
    float tmp[8];
#pragma unroll
    for (int uu = 0; uu < 8; ++uu) {
      const int idx = base + uu * 256;
      float wv;
      if (idx < N1) {
        const int l = idx & 63, rb = (idx >> 6) % HB, a = idx / (64 * HB);
        wv = weight_at(p, hoff + rb * 32 + (l & 31), 2 * a + (l >> 5));
      } else {
        const int i2 = idx - N1;
        const int l = i2 & 63, s2 = i2 >> 6;
        const int r = s2 & 15, rb = s2 >> 4;
        const int k = hoff + rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), m = l & 31;
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
  }
  if (threadIdx.x < 32) tB[threadIdx.x] = p.lnb_g[threadIdx.x];

  f32x4 dW2[2][4], dW1[4][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b4 = 0; b4 < 4; ++b4)
#pragma unroll
      for (int v = 0; v < 4; ++v) { dW2[a][b4][v] = 0.f; dW1[b4][a][v] = 0.f; }
  float db2[2] = {0.f, 0.f}, db1[4] = {0.f, 0.f, 0.f, 0.f};
  float gln = 0.f;   // threads 0..63: running (dγ | dβ) sum of this workgroup's tiles, tiles in walking order

  int tile = blockIdx.x;
  float bv[16][NACC];
  auto fetch_tile = [&](int t) {
    const int bt = t / tiles_per_sample;
    const int64_t ct = ((int64_t)(t % tiles_per_sample) * 4 + wave) * (32 * NACC) + NACC * j;
    const unsigned lo = (unsigned)h * (unsigned)p.Ncol + (unsigned)(ct < p.Ncol ? ct : 0);
    const AT* xb = p.x[0] + (int64_t)bt * 32 * p.Ncol;
#pragma unroll
    for (int s = 0; s < 16; ++s) vload<NACC>(xb + (int64_t)(2 * s) * p.Ncol + lo, bv[s]);
  };
  fetch_tile(tile);
  __syncthreads();

  for (; tile < ntiles; tile += gridDim.x) {
    asm volatile("" ::: "memory");   // keep loop-invariant LDS reads out of VGPRs (see gemm_chain_kernel)
    const int b = tile / tiles_per_sample;
    const int64_t col_off = ((int64_t)(tile % tiles_per_sample) * 4 + wave) * (32 * NACC) + NACC * j;
    const bool col_ok = col_off < p.Ncol;
    const int64_t nc = col_ok ? col_off : 0;
    const unsigned lane_row = (unsigned)(4 * h) * (unsigned)p.Ncol + (unsigned)nc;
    const unsigned lane_par = (unsigned)h * (unsigned)p.Ncol + (unsigned)nc;
    const int64_t sample = (int64_t)b * 32 * p.Ncol;

    // Lanes past the last column (ragged last tile only: their loads are clamped to column 0) must contribute zero to the
    // voxel sums.  Zeroing g2 HERE, once, does it for every sum of the tile: gh = W2ᵀ·0 = 0 makes gz1 = gh∘gelu' = 0 (db1, dW1,
    // and through GEMM 2 the LayerNorm sums), g2 = 0 itself covers dW2 and db2 — gelu(z1) and x̂ of such a lane stay finite and
    // meet a zero factor.  (Rounds 2-3 selected on every LDS store instead: 224 v_cndmask per tile, 10 % of the VALU stream.)
    // (hidden 128, two launches: the second half adds to a parked part read at a clamped address, and its register
    // allocation does not survive the change — that form keeps the per-store selects, ZSEL)
    constexpr bool ZSEL = HALVES == 2;
    auto zs = [&](float v) { return (ZSEL && !col_ok) ? 0.f : v; };
    if (!ZSEL && __builtin_amdgcn_ballot_w64(!col_ok) != 0) {
#pragma unroll
      for (int s = 0; s < 16; ++s) { bv[s][0] = col_ok ? bv[s][0] : 0.f; bv[s][1] = col_ok ? bv[s][1] : 0.f; }
    }
    // ---- Bf <- g2 (WGB: the hi / lo planes are written from GEMM 1's own operand split below) ----
    if constexpr (!WGB) {
#pragma unroll
    for (int s = 0; s < 16; ++s)
      *reinterpret_cast<float2*>(Bf + (2 * s + h) * kTS + 2 * j) = make_float2(zs(bv[s][0]), zs(bv[s][1]));
    }

    // Every global operand of the tile is requested one phase AHEAD of its use (two waves per SIMD cannot hide a
    // memory round trip per phase): z1 block g+1 during block g, x1 during the last z1 block, the residual rows before
    // GEMM 2.
    float e[2][8][NACC];
    auto fetch_z1 = [&](int g8, float (&dst)[8][NACC]) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int rr = g8 * 8 + i, rb = rr >> 4, r = rr & 15;
        const int rbase = hoff + rb * 32 + (r & 3) + 8 * (r >> 2);
        vload<NACC>(p.emul + ((int64_t)b * HID + rbase) * p.Ncol + lane_row, dst[i]);
      }
    };
    float xv[2][8][NACC];
    auto fetch_x1 = [&](int hf, float (&dst)[8][NACC]) {
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) vload<NACC>(p.lnb_x + sample + (int64_t)(2 * (hf * 8 + s8)) * p.Ncol + lane_par, dst[s8]);
    };
    const float* sp = p.lnb_stats + (int64_t)b * 2 * p.Ncol;
    float mu[NACC], rs[NACC];
    vload<NACC>(sp + nc, mu);
    vload<NACC>(sp + p.Ncol + nc, rs);
    fetch_z1(0, e[0]);

    // ---- GEMM 1: gh = W2ᵀ g2 ----
    f32x16 acc1[HB][NACC];
#pragma unroll
    for (int rb = 0; rb < HB; ++rb)
#pragma unroll
      for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[rb][q][r] = 0.f;
    if constexpr (BX) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        bx8 bop[NACC][NTB];
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
          float x8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) x8[e] = bv[8 * g + e][q];
          bx_split<NTB>(x8, bop[q]);
        }
        if constexpr (WGB) {   // levels 0 and 1 of g2, as (voxel 2j, voxel 2j+1) pairs of channel 2s + h, into the planes
          static_assert(!WGB || NTB >= 2, "two levels of the column operand");
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int s = 8 * g + e;
            const wg2 ph = {bop[0][0][e], bop[1][0][e]};
            const wg2 pl = {bop[0][NTB >= 2 ? 1 : 0][e], bop[1][NTB >= 2 ? 1 : 0][e]};
            *reinterpret_cast<wg2*>(PL + wop[s & 3] + s * 256) = ph;
            *reinterpret_cast<wg2*>(PL + kGL + wop[s & 3] + s * 256) = pl;
          }
        }
#pragma unroll
        for (int rb = 0; rb < HB; ++rb) {
          bx8 aop[NTA];
#pragma unroll
          for (int i = 0; i < NTA; ++i)
            aop[i] = *reinterpret_cast<const bx8*>(reinterpret_cast<const __bf16*>(As1) + (((g * HB + rb) * NTA + i) * 64 + lane) * 8);
#pragma unroll
          for (int q = 0; q < NACC; ++q) bx_mfma<NTA, NTB>(acc1[rb][q], aop, bop[q]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int rb = 0; rb < HB; ++rb) {
        const float av = As1[(s * HB + rb) * 64 + lane];
#pragma unroll
        for (int q = 0; q < NACC; ++q) acc1[rb][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[s][q], acc1[rb][q], 0, 0, 0);
        if (rb == HB - 1 && (s & 1) == 1) __builtin_amdgcn_sched_barrier(0);
      }
    }
    // (the next tile's operand is requested after GEMM 2: its 32 registers would otherwise be live next to the 64
    // gz1 accumulators and the 64 weight-gradient accumulators; the epilogue and the other resident waves cover
    // the round trip)

    // ---- pass A: 16 hidden channels at a time: gz1 = gh ∘ gelu'(z1) (kept in acc1); gelu(z1) -> T; dW2 += g2 ⊗ gelu(z1) ----
#pragma unroll
    for (int g8 = 0; g8 < 4; ++g8) {
      // (compiler-only fence: the g2 operand reads below are the same for every group — left alone they are read once
      // and kept in 32 registers across all four)
      asm volatile("" ::: "memory");
      if (g8 < 3) fetch_z1(g8 + 1, e[(g8 + 1) & 1]);
      else { fetch_x1(0, xv[0]); fetch_x1(1, xv[1]); }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int rr = g8 * 8 + i, rb = rr >> 4, r = rr & 15;
        float gl[NACC], dg[NACC];
        gelu_both2<HALVES == 2>(e[g8 & 1][i], gl, dg);
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
          float gz = acc1[rb][q][r] * dg[q];
          // pin the product HERE: its only readers are pass B and GEMM 2, and the optimiser otherwise sinks the
          // gelu' evaluation (and with it the liveness of all 64 z1 values) down to them
          asm volatile("" : "+v"(gz));
          acc1[rb][q][r] = gz;
        }
        if constexpr (WGB) {
          unsigned ph, pl;
          wg_split2(gl[0], gl[1], ph, pl);
          *reinterpret_cast<unsigned*>(PL + kTH + wac[i & 3] + (i & 3) * 128 + (i >> 2) * 1024) = ph;
          *reinterpret_cast<unsigned*>(PL + kTL + wac[i & 3] + (i & 3) * 128 + (i >> 2) * 1024) = pl;
        } else {
        const int loc = (i & 3) + 8 * (i >> 2) + 4 * h;
        *reinterpret_cast<float2*>(T + loc * kTS + 2 * j) = make_float2(zs(gl[0]), zs(gl[1]));
        }
      }
      if constexpr (WGB) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {   // 32 voxels per MFMA: six 16-byte operands in flight, then 6 MFMAs
          const bx8 bh = *reinterpret_cast<const bx8*>(PL + kTH + rd[ks]);
          const bx8 bl = *reinterpret_cast<const bx8*>(PL + kTL + rd[ks]);
          const bx8 a0h = *reinterpret_cast<const bx8*>(PL + rd[ks]);
          const bx8 a0l = *reinterpret_cast<const bx8*>(PL + kGL + rd[ks]);
          const bx8 a1h = *reinterpret_cast<const bx8*>(PL + 2048 + rd[ks]);
          const bx8 a1l = *reinterpret_cast<const bx8*>(PL + kGL + 2048 + rd[ks]);
          wg_mfma3(dW2[0][g8], a0h, a0l, bh, bl);
          wg_mfma3(dW2[1][g8], a1h, a1l, bh, bl);
          if (g8 == 0) {   // db2 = Σ_v g2 from the operands of the first group
            db2[0] = wg_sum8(a0h, a0l, db2[0]);
            db2[1] = wg_sum8(a1h, a1l, db2[1]);
            asm volatile("" : "+v"(db2[0]), "+v"(db2[1]));
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
#pragma unroll
      for (int tc = 0; tc < 2; ++tc) {   // 8 voxel quads at a time: 24 LDS operands in flight, then 16 MFMAs
        float bq[8], a0[8], a1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int t = tc * 8 + u;
          bq[u] = T[l16 * kTS + 4 * t + k4];
          a0[u] = Bf[l16 * kTS + 4 * t + k4];
          a1[u] = Bf[(16 + l16) * kTS + 4 * t + k4];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          dW2[0][g8] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], bq[u], dW2[0][g8], 0, 0, 0);
          dW2[1][g8] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[u], bq[u], dW2[1][g8], 0, 0, 0);
        }
        if (g8 == 0 && (HALVES == 1 || half == 0)) {   // db2 = Σ_v g2 from the operands of the first group (pinned: the optimiser otherwise postpones
                         // the sums — and keeps the operands alive — to the end of the tile)
          db2[0] += ((a0[0] + a0[1]) + (a0[2] + a0[3])) + ((a0[4] + a0[5]) + (a0[6] + a0[7]));
          db2[1] += ((a1[0] + a1[1]) + (a1[2] + a1[3])) + ((a1[4] + a1[5]) + (a1[6] + a1[7]));
          asm volatile("" : "+v"(db2[0]), "+v"(db2[1]));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      }
      __builtin_amdgcn_sched_barrier(0);
    }

    // the residual rows g2 in the ACCUMULATOR layout, read back from Bf before x̂ replaces it there (rounds 2-3 re-read them
    // from global memory before GEMM 2: 0.54 GB per launch that did not hit the caches — PMC traffic 1.22x algorithmic)
    // (BX form only: the fp32-MFMA form of the kernel — fz_gemm_bx_enable(0), diagnostics — has no 32 registers to spare
    // across pass B and keeps the global re-read)
    float ga[2][8][NACC];
    if (last && BX) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float2 gv;
        if constexpr (WGB)
          gv = wg_join2(*reinterpret_cast<const unsigned*>(PL + wac[r & 3] + (r & 3) * 128 + (r >> 2) * 1024),
                        *reinterpret_cast<const unsigned*>(PL + kGL + wac[r & 3] + (r & 3) * 128 + (r >> 2) * 1024));
        else
          gv = *reinterpret_cast<const float2*>(Bf + ((r & 3) + 8 * (r >> 2) + 4 * h) * kTS + 2 * j);
        ga[r >> 3][r & 7][0] = gv.x; ga[r >> 3][r & 7][1] = gv.y;
      }
      asm volatile("" ::: "memory");   // (the reads must stay ahead of the x̂ stores below: same addresses)
    }

    // ---- Bf <- LN-normalised x1 (requested during the last z1 block) ----
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) {
        if constexpr (WGB) {
          const int s = hf * 8 + s8;
          unsigned ph, pl;
          wg_split2((xv[hf][s8][0] - mu[0]) * rs[0], (xv[hf][s8][1] - mu[1]) * rs[1], ph, pl);
          *reinterpret_cast<unsigned*>(PL + wop[s & 3] + s * 256) = ph;
          *reinterpret_cast<unsigned*>(PL + kGL + wop[s & 3] + s * 256) = pl;
        } else
        *reinterpret_cast<float2*>(Bf + (2 * (hf * 8 + s8) + h) * kTS + 2 * j) =
            make_float2(zs((xv[hf][s8][0] - mu[0]) * rs[0]), zs((xv[hf][s8][1] - mu[1]) * rs[1]));
      }

    f32x16 acc2[NACC];
    if constexpr (WGF) {
#pragma unroll
      for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[q][r] = 0.f;
    }
    // ---- pass B: gz1 block -> T; S1 += gz1 ⊗ x̂, db1 += Σ gz1 (WGB: and GEMM 2's K-group of the same channels) ----
#pragma unroll
    for (int g8 = 0; g8 < 4; ++g8) {
      asm volatile("" ::: "memory");   // as in pass A: re-read the x̂ operands per group instead of holding 32 registers
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int rr = g8 * 8 + i, rb = rr >> 4, r = rr & 15;
        if constexpr (WGF) {
          // (the two levels come from GEMM 2's own three-level split of this group, below)
        } else if constexpr (WGB) {
          unsigned ph, pl;
          wg_split2(acc1[rb][0][r], acc1[rb][1][r], ph, pl);
          *reinterpret_cast<unsigned*>(PL + kTH + wac[i & 3] + (i & 3) * 128 + (i >> 2) * 1024) = ph;
          *reinterpret_cast<unsigned*>(PL + kTL + wac[i & 3] + (i & 3) * 128 + (i >> 2) * 1024) = pl;
        } else {
        const int loc = (i & 3) + 8 * (i >> 2) + 4 * h;
        *reinterpret_cast<float2*>(T + loc * kTS + 2 * j) = make_float2(zs(acc1[rb][0][r]), zs(acc1[rb][1][r]));
        }
      }
      if constexpr (WGB) {
        // K-group g8 of GEMM 2 (gl += W1ᵀ gz1) IS this group of hidden channels: split it once, multiply, and park levels 0 / 1
        if constexpr (WGF) {
          bx8 aop[NTA];
#pragma unroll
          for (int i = 0; i < NTA; ++i)
            aop[i] = *reinterpret_cast<const bx8*>(reinterpret_cast<const __bf16*>(As2) + ((g8 * NTA + i) * 64 + lane) * 8);
          bx8 bop[NACC][NTB];
#pragma unroll
          for (int q = 0; q < NACC; ++q) {
            float x8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x8[e] = acc1[g8 >> 1][q][8 * (g8 & 1) + e];
            bx_split<NTB>(x8, bop[q]);
            bx_mfma<NTA, NTB>(acc2[q], aop, bop[q]);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const wg2 ph = {bop[0][0][i], bop[1][0][i]};
            const wg2 pl = {bop[0][1][i], bop[1][1][i]};
            *reinterpret_cast<wg2*>(PL + kTH + wac[i & 3] + (i & 3) * 128 + (i >> 2) * 1024) = ph;
            *reinterpret_cast<wg2*>(PL + kTL + wac[i & 3] + (i & 3) * 128 + (i >> 2) * 1024) = pl;
          }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bx8 ah = *reinterpret_cast<const bx8*>(PL + kTH + rd[ks]);
          const bx8 al = *reinterpret_cast<const bx8*>(PL + kTL + rd[ks]);
          const bx8 b0h = *reinterpret_cast<const bx8*>(PL + rd[ks]);
          const bx8 b0l = *reinterpret_cast<const bx8*>(PL + kGL + rd[ks]);
          const bx8 b1h = *reinterpret_cast<const bx8*>(PL + 2048 + rd[ks]);
          const bx8 b1l = *reinterpret_cast<const bx8*>(PL + kGL + 2048 + rd[ks]);
          wg_mfma3(dW1[g8][0], ah, al, b0h, b0l);
          wg_mfma3(dW1[g8][1], ah, al, b1h, b1l);
          db1[g8] = wg_sum8(ah, al, db1[g8]);
          asm volatile("" : "+v"(db1[g8]));
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
#pragma unroll
      for (int tc = 0; tc < 2; ++tc) {
        float aq[8], b0[8], b1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int t = tc * 8 + u;
          aq[u] = T[l16 * kTS + 4 * t + k4];
          b0[u] = Bf[l16 * kTS + 4 * t + k4];
          b1[u] = Bf[(16 + l16) * kTS + 4 * t + k4];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          dW1[g8][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[u], b0[u], dW1[g8][0], 0, 0, 0);
          dW1[g8][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[u], b1[u], dW1[g8][1], 0, 0, 0);
        }
        db1[g8] += ((aq[0] + aq[1]) + (aq[2] + aq[3])) + ((aq[4] + aq[5]) + (aq[6] + aq[7]));
        asm volatile("" : "+v"(db1[g8]));
        __builtin_amdgcn_sched_barrier(0);
      }
      }
      __builtin_amdgcn_sched_barrier(0);
    }


    if (last && !BX) {   // residual rows (g2 again: L2 / MALL), requested before GEMM 2
#pragma unroll
      for (int r = 0; r < 16; ++r)
        vload<NACC>(p.lnb_gadd + sample + (int64_t)((r & 3) + 8 * (r >> 2)) * p.Ncol + lane_row, ga[r >> 3][r & 7]);
    }

    // ---- GEMM 2: gl = W1ᵀ gz1 straight from the accumulators (second half: on top of the first half's part) ----
    if constexpr (WGF) {
      // (done inside pass B)
    } else if (HALVES == 2 && half == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v[NACC];
        vload<NACC>(glp + sample + (int64_t)((r & 3) + 8 * (r >> 2)) * p.Ncol + lane_row, v);
        acc2[0][r] = v[0]; acc2[1][r] = v[1];
      }
    } else {
#pragma unroll
      for (int q = 0; q < NACC; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[q][r] = 0.f;
    }
    if constexpr (WGF) {
    } else if constexpr (BX) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {   // steps (rb, r) = (g >> 1, 8 (g & 1) + e): accumulator registers as the column operand
        bx8 aop[NTA];
#pragma unroll
        for (int i = 0; i < NTA; ++i)
          aop[i] = *reinterpret_cast<const bx8*>(reinterpret_cast<const __bf16*>(As2) + ((g * NTA + i) * 64 + lane) * 8);
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
          float x8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) x8[e] = acc1[g >> 1][q][8 * (g & 1) + e];
          bx8 bop[NTB];
          bx_split<NTB>(x8, bop);
          bx_mfma<NTA, NTB>(acc2[q], aop, bop);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
    for (int rb = 0; rb < HB; ++rb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float av = As2[(rb * 16 + r) * 64 + lane];
#pragma unroll
        for (int q = 0; q < NACC; ++q) acc2[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, acc1[rb][q][r], acc2[q], 0, 0, 0);
        if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
    }
    fetch_tile(tile + gridDim.x < ntiles ? tile + gridDim.x : tile);

    if (HALVES == 2 && !last) {   // first half: park the partial W1ᵀ·gz1 (fp32), no epilogue
      if (col_ok) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v[NACC] = {acc2[0][r], acc2[1][r]};
          vstore<NACC>(glp + sample + (int64_t)((r & 3) + 8 * (r >> 2)) * p.Ncol + lane_row, v);
        }
      }
      continue;
    }
    // ---- LayerNorm backward + residual gradient (x̂ from Bf in the accumulator layout, g2 re-read: L2 / MALL) ----
    float m1[NACC] = {0.f, 0.f}, m2[NACC] = {0.f, 0.f};
    float xkeep[WGB ? 16 : 1][2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
      const float gc = tB[row];
      float2 xh;
      if constexpr (WGB) {   // (rebuilt from its two levels once and kept: the registers of gz1 are free by now)
        xh = wg_join2(*reinterpret_cast<const unsigned*>(PL + wac[r & 3] + (r & 3) * 128 + (r >> 2) * 1024),
                      *reinterpret_cast<const unsigned*>(PL + kGL + wac[r & 3] + (r & 3) * 128 + (r >> 2) * 1024));
        xkeep[r][0] = xh.x; xkeep[r][1] = xh.y;
      } else
        xh = *reinterpret_cast<const float2*>(Bf + row * kTS + 2 * j);
      const float a0 = acc2[0][r] * gc, a1 = acc2[1][r] * gc;
      m1[0] += a0; m1[1] += a1;
      m2[0] += a0 * xh.x; m2[1] += a1 * xh.y;
    }
#pragma unroll
    for (int q = 0; q < NACC; ++q) {
      m1[q] = (m1[q] + __shfl_xor(m1[q], 32, 64)) * (1.0f / 32.0f);
      m2[q] = (m2[q] + __shfl_xor(m2[q], 32, 64)) * (1.0f / 32.0f);
    }
#pragma unroll
    for (int r8 = 0; r8 < 2; ++r8) {
      float sgv[8], sbv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int r = r8 * 8 + i;
        const int rbase = (r & 3) + 8 * (r >> 2);
        const int row = rbase + 4 * h;
        const float gc = tB[row];
        float2 xh;
        if constexpr (WGB)
          xh = make_float2(xkeep[r][0], xkeep[r][1]);
        else
          xh = *reinterpret_cast<const float2*>(Bf + row * kTS + 2 * j);
        float v[NACC];
        v[0] = rs[0] * (acc2[0][r] * gc - m1[0] - xh.x * m2[0]) + ga[r8][i][0];
        v[1] = rs[1] * (acc2[1][r] * gc - m1[1] - xh.y * m2[1]) + ga[r8][i][1];
        if (col_ok) vstore<NACC>(p.y + sample + (int64_t)rbase * p.Ncol + lane_row, v);
        float sg = acc2[0][r] * xh.x + acc2[1][r] * xh.y;   // (lanes past the last column: acc2 = 0, see the top of the tile)
        float sb = acc2[0][r] + acc2[1][r];
        sg = zs(sg);
        sb = zs(sb);
        if constexpr (WGF) {   // the eight rows of the block are reduced together below (multi-value butterfly: 19 operations for
          sgv[i] = sg;         // sixteen half-wave sums instead of 5 per sum; fp32 storage: the bf16 instantiation spills with it)
          sbv[i] = sb;
        } else {
        sg = half_sum32(sg);
        sb = half_sum32(sb);
        if ((lane & 31) == 31) {
          red[wave * 64 + row] = sg;
          red[wave * 64 + 32 + row] = sb;
        }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (WGF) {
        const float tg = half_sum8_dist(sgv, lane), tb = half_sum8_dist(sbv, lane);   // 4-lane group i of a half holds row i's total
        const int gi = (lane >> 2) & 7, rr = r8 * 8 + gi;
        if ((lane & 3) == 0) {
          const int rw = (rr & 3) + 8 * (rr >> 2) + 4 * h;
          red[wave * 64 + rw] = tg;
          red[wave * 64 + 32 + rw] = tb;
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      const int e = threadIdx.x;
      gln += (red[e] + red[64 + e]) + (red[128 + e] + red[192 + e]);
    }
    __syncthreads();
  }

  // ---- the workgroup's (dW2 | S1 | db2 | db1 | dγ | dβ) row: add the four waves through LDS, waves in index order ----
  float* row = wpart + (int64_t)blockIdx.x * kWgRow;
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int v = 0; v < 4; ++v) R[(wave * 32 + (a * 4 + cb) * 4 + v) * 64 + lane] = dW2[a][cb][v];
  __syncthreads();
  for (int e = threadIdx.x; e < 2048; e += 256) {
    const int idx = e >> 6, l = e & 63;
    const int a = idx >> 4, cb = (idx >> 2) & 3, v = idx & 3;
    const float t = (R[e] + R[2048 + e]) + (R[4096 + e] + R[6144 + e]);
    row[(16 * a + 4 * (l >> 4) + v) * 64 + 16 * cb + (l & 15)] = t;
  }
  __syncthreads();
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int v = 0; v < 4; ++v) R[(wave * 32 + (cb * 2 + kh) * 4 + v) * 64 + lane] = dW1[cb][kh][v];
  __syncthreads();
  for (int e = threadIdx.x; e < 2048; e += 256) {
    const int idx = e >> 6, l = e & 63;
    const int cb = idx >> 3, kh = (idx >> 2) & 1, v = idx & 3;
    const float t = (R[e] + R[2048 + e]) + (R[4096 + e] + R[6144 + e]);
    row[2048 + (16 * cb + 4 * (l >> 4) + v) * 32 + 16 * kh + (l & 15)] = t;
  }
  __syncthreads();
  R[(wave * 6 + 0) * 64 + lane] = db2[0];
  R[(wave * 6 + 1) * 64 + lane] = db2[1];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) R[(wave * 6 + 2 + cb) * 64 + lane] = db1[cb];
  __syncthreads();
  if (threadIdx.x < 96) {
    const int e = threadIdx.x, slot = e >> 4, i16 = e & 15;   // slots 0,1: db2 halves; 2..5: db1 blocks
    float t = 0.f;
    for (int w = 0; w < 4; ++w)
      for (int kk = 0; kk < 4; ++kk) t += R[(w * 6 + slot) * 64 + kk * 16 + i16];
    row[4096 + e] = t;
  }
  if (threadIdx.x < 64) row[4096 + 96 + threadIdx.x] = gln;
}

// (the rows are added, and the LayerNorm affine applied to dW1, by the FK_CHAIN_WG job of the finish kernel: finish.h)

static int knob_mlp_wg_wgs() { return knob_pos(FZ_KNOB("FZ_MLP_WG_WGS"), 512); }
static int knob_chain_wgb() { const auto& k = FZ_KNOB("FZ_CHAIN_WGB"); return k.set ? k.val : 1; }   // 0: fp32-MFMA weight-gradient passes

}  // namespace fz

using namespace fz;

// rows of `wpart` (fz_mlp_desc mode 2): one per resident workgroup (two per CU), kWgRow floats each — the grid of chain_wg_launch
extern "C" int fz_mlp_wgrad_rows(int B, int64_t V) {
  const int64_t nt = fz_mlp_partials(B, V);
  const int wgs = knob_mlp_wg_wgs();
  return (int)(nt < wgs ? nt : wgs);
}
extern "C" int64_t fz_mlp_wgrad_workspace_bytes(int B, int64_t V) {
  return 2 * (int64_t)fz_mlp_wgrad_rows(B, V) * kWgRow * (int64_t)sizeof(float);   // two row blocks (hidden 128 runs in two halves)
}

namespace fz {

// Host side: fz_mlp_chain mode 2 (mlp_launch, mlp_chain.hip, has checked the descriptor and filled a and c).  Hidden 64 is one
// launch; hidden 128 one launch per 64-row half, each with its own row block of wpart.  After every launch an FK_CHAIN_WG job
// of the finish kernel adds the rows of its block.
template <typename AT>
int chain_wg_launch(const fz_mlp_desc* d, const GemmArgsT<AT>& a, const ChainArgsT<AT>& c, fz_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  const int ntiles = (int)fz_mlp_partials(d->B, d->V), rows = fz_mlp_wgrad_rows(d->B, d->V);
  const int halves = d->H / 64;
  const bool bx = products_split(d->products);
  // split products at hidden 64: the weight-gradient passes on the bf16 pipe too (WGB, two operand levels); FZ_CHAIN_WGB=0 in a
  // probe build keeps them on v_mfma_f32_16x16x4_f32 (same-box A/B)
  const bool wgb = bx && halves == 1 && knob_chain_wgb();
  void (*kern[2])(GemmArgsT<AT>, ChainArgsT<AT>, int, float*, float*) = {
      halves == 2 ? (bx ? gemm_chain_bwd_wg_kernel<AT, 2, 0, true> : gemm_chain_bwd_wg_kernel<AT, 2, 0, false>)
      : wgb       ? gemm_chain_bwd_wg_kernel<AT, 1, 0, true, true>
                  : (bx ? gemm_chain_bwd_wg_kernel<AT, 1, 0, true> : gemm_chain_bwd_wg_kernel<AT, 1, 0, false>),
      bx ? gemm_chain_bwd_wg_kernel<AT, 2, 1, true> : gemm_chain_bwd_wg_kernel<AT, 2, 1, false>};
  for (int half = 0; half < halves; ++half) {
    float* wp = (float*)d->wpart + (int64_t)half * rows * kWgRow;
    int rc = launch_lds(kern[half], dim3((unsigned)rows), dim3(256), chain_wg_lds_floats(bx, wgb), st, a, c, ntiles, wp,
                        halves == 2 ? d->glp : (float*)nullptr);
    if (rc != FZ_OK) return rc;
    FinishJob fj = finish_job(FK_CHAIN_WG, kWgRow / 16);
    fj.u.cw = FinChainWg{(const float*)wp, d->ln_g, d->ln_b, d->gw1 + half * 64 * 32, d->gb1 + half * 64, d->gw2 + half * 64,
                         half == 0 ? d->gb2 : (float*)nullptr, half == halves - 1 ? d->gln : (float*)nullptr, rows, d->H};
    rc = finish_run(&fj, 1, st);
    if (rc != FZ_OK) return rc;
  }
  return FZ_OK;
}
template int chain_wg_launch<float>(const fz_mlp_desc*, const GemmArgsT<float>&, const ChainArgsT<float>&, fz_stream_t);
template int chain_wg_launch<bf16>(const fz_mlp_desc*, const GemmArgsT<bf16>&, const ChainArgsT<bf16>&, fz_stream_t);

}  // namespace fz
