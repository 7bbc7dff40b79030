// gemm.hip — channels-first GEMM family on the fp32 matrix cores (v_mfma_f32_32x32x2_f32).
//
//   Out[m, n] = epilogue( Σ_k A[m, k] · prologue(In)[k, n] )        n = voxel (column)
//
// One kernel template serves every dense layer of the Factorizer U-shape and their input
// gradients (reference call sites, paths relative to the reference root):
//   * Linear / in_proj / out_proj / adapter / MLP / head : Conv1d(k=1) on flatten(2)
//       layers/linear.py:53-58, factorizer.py:38,53,116, layers/mlp.py:54-60, unet.py:253
//   * downsample Conv3d(k=2, stride=2)        unet.py:53   (space-to-depth loader)
//   * upsample  ConvTranspose3d(k=2, stride=2) unet.py:123 (depth-to-space epilogue)
//   * LayerNorm over channels fused as a prologue (layers/norm.py:29-34), ReLU/GELU, bias,
//     residual add (factorizer.py:75-76) and window averaging (operations.py:426-433) fused
//     as prologue/epilogue so each full-resolution tensor is read/written once per layer.
//
// MFMA mapping (wave64, 32x32x2 f32): lane l = (j = l&31, h = l>>5).  The B operand of K-step
// s is In[k = 2s+h][column j]; each lane loads ONE 16-byte vector = 4 consecutive voxels of
// channel 2s+h, and the 4 components feed 4 MFMAs (column groups q = 0..3, voxel 4j+q), so
// global loads are 1 KiB-per-wave coalesced and no LDS staging of activations is needed.
// Weights (the A operand) are staged once per workgroup in LDS in operand order.
// The accumulator tile has its row in (register, h) and its column in j, so the epilogue
// stores 16-byte vectors (4 voxels) per register: 512 B contiguous per output row.
//
// This unit: the register-resident kernel (A) and the dispatcher of fz_gemm.  The persistent 32 -> 32 kernel (A') lives in
// gemm_p32.hip, the streaming kernel (B) in gemm_stream.hip, the chained MLP kernels in mlp_chain32.hip, mlp_chain64.hip and
// mlp_chain_wg.hip (host dispatch: mlp_chain.hip), the fused input + weight gradient in gemm_dw.hip.
#include "gemm_bx.h"       // uload (brings gemm_common.h)
#include "gemm_shared.h"   // LayerNorm-backward epilogue, knob_pos, gemm_p32_launch, chain64_lnb_launch

namespace fz {

// =================================================================================================
// Kernel A — register-resident operand, K <= 2*NSTEP (the HBM-bound layers, C <= 64).
// Every lane issues ALL its operand loads up front (NSTEP x 16 B in flight per lane), applies the
// prologue in registers (exact two-pass LayerNorm), then walks the RB row blocks of the
// workgroup sequentially with one accumulator set: the input is read from HBM exactly once for
// all output rows and 10+ KiB per wave are in flight.
// =================================================================================================
// RESPF (one 32-row block, plain epilogue): the residual tile is requested with the operand, before the products — in the
// epilogue its loads were a second exposed round trip per workgroup (wait share 0.72 of the wave lifetime, round-3 profile 8)
template <int NSTEP, int EPI, bool BMUL, bool GADD = false, typename AT = float, int PF = 3, bool RESPF = false>
// (waves per SIMD chosen so that NO variant needs scratch: see the note on scratch and concurrent streams in nmf_pcf.hip)
__global__ __launch_bounds__(256, ((NSTEP <= 16 && EPI == EPI_PLAIN && !BMUL && !(PF & 2) && !RESPF) ? 3 : (NSTEP <= 16 ? 2 : 1))) void gemm_resident_kernel(GemmArgsT<AT> p, int RB) {
  // PF: prologue code compiled in — bit 0 input activation, bit 1 LayerNorm.  A runtime branch alone keeps a second copy
  // of the operand registers alive (normalised / activated next to raw): the K <= 32 form spilled because of it.
  constexpr bool ACTIN = (PF & 1) != 0, LNP = (PF & 2) != 0;
  extern __shared__ __attribute__((aligned(16))) float lds_a[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int nA = (p.K + 1) / 2;
  float* As = lds_a;                      // [nA][RB][64]
  float* tW = lds_a + nA * RB * 64;       // [32*RB]
  const int tiles_per_sample = (int)((p.Ncol + 511) / 512);
  int bid = blockIdx.x;
  if (p.tile_map == 1) {         // XCD-contiguous: each XCD walks its own eighth of the tiles
    const int nb = gridDim.x, q8 = nb / 8, r8 = nb % 8, xcd = bid % 8, i8 = bid / 8;
    if (nb >= 16) bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + i8;
  } else if (p.tile_map == 2) {  // scattered: odd-multiplier permutation of a power-of-two grid
    const int nb = gridDim.x;
    if ((nb & (nb - 1)) == 0) bid = (int)(((unsigned)bid * 40503u) & (unsigned)(nb - 1));
  }
  const int b = bid / tiles_per_sample;
  const int64_t n0 = ((int64_t)(bid % tiles_per_sample) * 4 + wave) * 128;
  const int m0 = blockIdx.y * 32 * RB;

  // the column operand (and the residual tile) first: the weight fill below runs under their latency
  const int64_t col_off = n0 + 4 * j;
  const bool col_ok = col_off < p.Ncol;
  // (K <= 32 forms; the K <= 64 ones keep the loads behind the fill: one of them needed scratch with the operand live across it)
  constexpr bool kEarly = NSTEP <= 16;
  float bv[NSTEP][4];
  float rv[RESPF ? 16 : 1][4];
  auto load_operands = [&]() {
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) fetch_plain<4, BMUL>(p, b, 2 * s + h, col_off, col_ok, bv[s]);
    if (RESPF) {   // host-checked: M == 32, p.res != null
#pragma unroll
      for (int r = 0; r < 16; ++r)
        vload<4>(p.res + ((int64_t)b * p.M + (r & 3) + 8 * (r >> 2) + 4 * h) * p.Ncol + (col_ok ? col_off : 0), rv[RESPF ? r : 0]);
    }
  };
  if (kEarly) load_operands();

  // batched fill (8 independent loads per thread before the LDS stores)
  constexpr int kFill = (NSTEP <= 16 && EPI == EPI_PLAIN && !BMUL) ? 4 : 8;   // independent loads per thread and round
  for (int base = threadIdx.x; base < nA * RB * 64; base += blockDim.x * kFill) {
    float tmp[kFill];
#pragma unroll
    for (int uu = 0; uu < kFill; ++uu) {
      const int idx = base + uu * blockDim.x;
      const bool in = idx < nA * RB * 64;
      const int ii = in ? idx : 0;
      const int l = ii & 63;
      const int rb = (ii >> 6) % RB;
      const int a = ii / (64 * RB);
      const int m = m0 + rb * 32 + (l & 31);
      const int k = 2 * a + (l >> 5);
      const bool ok = in && m < p.M && k < p.K;
      const int mc = m < p.M ? m : p.M - 1, kc = k < p.K ? k : p.K - 1;
      float wv = weight_at(p, mc, kc);
      if (LNP && p.ln) wv *= p.ln_g[kc];
      tmp[uu] = ok ? wv : 0.f;
    }
#pragma unroll
    for (int uu = 0; uu < kFill; ++uu) {
      const int idx = base + uu * blockDim.x;
      if (idx < nA * RB * 64) As[idx] = tmp[uu];
    }
  }
  if (LNP && p.ln) {
    for (int r = threadIdx.x; r < 32 * RB; r += blockDim.x) {
      const int m = m0 + r;
      float t = 0.f;
      if (m < p.M)
        for (int k = 0; k < p.K; ++k) t += weight_at(p, m, k) * p.ln_b[k];
      tW[r] = t;
    }
  }

  if (EPI == EPI_LNBWD) {  // gamma of the fused LayerNorm backward (tW is free: no LN prologue here)
    if (threadIdx.x < 32) tW[threadIdx.x] = p.lnb_g[threadIdx.x];
  }

  if (!kEarly) load_operands();

  if (LNP && p.ln) {
    // exact two-pass statistics over the Cin channels (this lane holds the parity-h half)
    float mu[4], rs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = 0.f;
#pragma unroll
      for (int s = 0; s < NSTEP; ++s) t += bv[s][e];
      t += __shfl_xor(t, 32, 64);
      mu[e] = t / (float)p.Cin;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = 0.f;
#pragma unroll
      for (int s = 0; s < NSTEP; ++s) {
        const float d = (2 * s + h < p.Cin) ? bv[s][e] - mu[e] : 0.f;
        t += d * d;
      }
      t += __shfl_xor(t, 32, 64);
      rs[e] = 1.0f / sqrtf(t / (float)p.Cin + p.ln_eps);
    }
#pragma unroll
    for (int s = 0; s < NSTEP; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[s][e] = (2 * s + h < p.Cin) ? (bv[s][e] - mu[e]) * rs[e] : 0.f;
    if (p.stats_out != nullptr && blockIdx.y == 0 && h == 0 && col_ok) {
      float* so = p.stats_out + (int64_t)b * 2 * p.Vin;
      *reinterpret_cast<float4*>(so + col_off) = make_float4(mu[0], mu[1], mu[2], mu[3]);
      *reinterpret_cast<float4*>(so + p.Vin + col_off) = make_float4(rs[0], rs[1], rs[2], rs[3]);
    }
  }
  // (ACTIN = false: no input-activation code at all — the runtime branch alone kept a second copy of the 64 operand
  // registers alive and spilled the K <= 32 form)
  if (ACTIN && p.bact == ACT_GELU) {
#pragma unroll
    for (int s = 0; s < NSTEP; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[s][e] = gelu_f(bv[s][e]);
  } else if (ACTIN && p.bact == ACT_RELU) {
#pragma unroll
    for (int s = 0; s < NSTEP; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[s][e] = bv[s][e] > 0.f ? bv[s][e] : 0.f;
  }
  __syncthreads();

  // NOTE: every lane must stay active through the MFMAs (the A operand lives in all 64 lanes);
  // lanes whose columns fall outside the tensor only skip the stores.
  // EPI_LNBWD is host-checked to M == 32 and K == 2*NSTEP: one row block, no tail guards — this
  // keeps the register allocation of the (register-heavy) fused epilogue free of dead paths
  constexpr bool kExact = (EPI == EPI_LNBWD);
  const int RBn = kExact ? 1 : RB;
  for (int rb = 0; rb < RBn; ++rb) {
    if (!kExact && m0 + rb * 32 >= p.M) break;
    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {
      if (kExact || s < nA) {
        const float av = As[(s * RBn + rb) * 64 + lane];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[s][q], acc[q], 0, 0, 0);
      }
      // (at most 4 weight operands requested ahead: all NSTEP of them in flight cost the registers that put the K <= 32
      // form one over the 168 of three waves per SIMD — it spilled 3 of them to scratch)
      if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    if (EPI == EPI_LNBWD) {
      lnbwd_block<4, GADD>(p, acc, b, col_off, col_ok, lane, wave, tW + 32 * RB, blockIdx.x, tW);
    } else if (RESPF) {   // store_block's plain form with the residual already in registers (same order of additions)
      if (col_ok) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;
          float add = p.bias ? p.bias[rl] : 0.f;
          if (LNP && p.ln) add += tW[rl];
          float v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = acc[q][r] + add;
          if (p.eact) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = act_f(p.eact, v[q]);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] += rv[RESPF ? r : 0][q];
          vstore<4>(p.y + ((int64_t)b * p.M + rl) * p.Ncol + col_off, v);
        }
      }
    } else {
      if (col_ok) store_block<4, (EPI == EPI_LNBWD ? EPI_PLAIN : EPI), false>(p, acc, b, m0 + rb * 32, col_off, h, (LNP && p.ln) ? tW + rb * 32 : nullptr);
    }
  }
}


}  // namespace fz

using namespace fz;

// process-wide switch of the split-bf16 MFMA family: FZ_GEMM_BX (read once) unless fz_gemm_bx_enable() set it
static std::atomic<int> g_bx_on{-1};
// (the knob reader and why a knob is read once: knob_pos, gemm_shared.h)
static int knob_res_prefetch() { return knob_pos(FZ_KNOB("FZ_RES_PREFETCH"), 1) == 1; }   // 2 = off
static int knob_p32() { return knob_pos(FZ_KNOB("FZ_GEMM_P32"), 1) == 1; }                // 2 = off
static int knob_head_fwd() { const auto& k = FZ_KNOB("FZ_HEAD_FWD"); return k.set ? k.val : 1; }   // 0: the head through gemm_p32

static int gemm_bx_enabled() {
  int v = g_bx_on.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("FZ_GEMM_BX");
    v = e ? (atoi(e) != 0) : 1;
    g_bx_on.store(v, std::memory_order_relaxed);
  }
  return v;
}
extern "C" int fz_gemm_bx_enable(int on) {
  const int prev = gemm_bx_enabled();
  if (on >= 0) g_bx_on.store(on != 0, std::memory_order_relaxed);
  return prev;
}

// Flat C view of GemmArgsT for the ABI (see include/factorizer_hip.h: fz_gemm_desc).
template <typename AT>
static int gemm_launch(const fz_gemm_desc* d, fz_stream_t stream) {
  if (!d->x[0] || !d->w || !d->y) return fail(FZ_E_ARG, "fz_gemm: null pointer");
  if (d->loader < LOAD_PLAIN || d->loader > LOAD_K3_2D) return fail(FZ_E_ARG, "fz_gemm: bad loader");
  if (d->epilogue < EPI_PLAIN || d->epilogue > EPI_D2S_2D) return fail(FZ_E_ARG, "fz_gemm: bad epilogue");
  {
    // the 2-D forms (Conv2d k2s2 / k3p1, ConvTranspose2d k2s2): one loader OR one epilogue, no prologue, one source
    const bool l2 = d->loader == LOAD_S2D_2D || d->loader == LOAD_K3_2D, e2 = d->epilogue == EPI_D2S_2D;
    if ((l2 || e2) && ((l2 && d->epilogue != EPI_PLAIN) || (e2 && d->loader != LOAD_PLAIN) || d->ln || d->bact || d->bmul ||
                       d->emul || d->eact || d->nsrc != 1 || d->src_mode != 0 || d->stats_out))
      return fail(FZ_E_ARG, "fz_gemm: a 2-D loader / epilogue takes one source, a plain partner and no prologue / activation");
    if (d->loader == LOAD_S2D_2D && (d->K != 4 * d->Cin || (d->Wo & 1) || d->Ho < 1 || d->Wo < 1 || d->Hi != 2 * d->Ho ||
                                     d->Wi != 2 * d->Wo || d->Ncol != (int64_t)d->Ho * d->Wo || d->Vin != (int64_t)d->Hi * d->Wi ||
                                     d->res))
      return fail(FZ_E_SHAPE, "fz_gemm: 2-D space-to-depth needs K = 4*Cin, (Hi, Wi) = 2*(Ho, Wo), even Wo, Ncol = Ho*Wo");
    if (d->loader == LOAD_K3_2D && (d->K != 9 * d->Cin || (d->Cin & 1) || d->Hi < 1 || d->Wi < 4 || (d->Wi & 3) ||
                                    d->Ncol != (int64_t)d->Hi * d->Wi || d->Vin != d->Ncol || d->res))
      return fail(FZ_E_SHAPE, "fz_gemm: 2-D 3x3 loader needs K = 9*Cin, even Cin, W % 4 == 0, Ncol = Vin = H*W");
    if (e2 && (d->M % 4 != 0 || d->Ho < 1 || d->Wo < 1 || d->Ncol != (int64_t)d->Ho * d->Wo || d->Vin != d->Ncol || (d->Ncol & 3)))
      return fail(FZ_E_SHAPE, "fz_gemm: 2-D depth-to-space needs M = 4*O, Ncol = Vin = Ho*Wo, a multiple of 4");
  }
  const bool lnb64 = d->epilogue == EPI_LNBWD && d->M == 64 && d->K == 64 && d->nsrc == 1 && !d->bmul;
  if (d->epilogue == EPI_LNBWD && ((!lnb64 && (d->M != 32 || (d->K != 32 && d->K != 64))) || d->loader != LOAD_PLAIN || !d->lnb_x || !d->lnb_stats ||
                                   !d->lnb_g || !d->lnb_part || d->bias || d->res || d->emul || d->eact || d->ln))
    return fail(FZ_E_UNSUPPORTED, "fz_gemm: LayerNorm-backward epilogue needs M == 32 (K = 32 or 64) or M == K == 64, plain loader");
  if (d->epilogue == EPI_LNBWD && d->Ncol > ((int64_t)1 << 27)) return fail(FZ_E_UNSUPPORTED, "fz_gemm: LayerNorm-backward epilogue: more than 2^27 voxels per sample");
  if (d->B < 0 || d->Cin < 1 || d->M < 1 || d->K < 1) return fail(FZ_E_SHAPE, "fz_gemm: sizes must be positive");
  if ((d->K & 1) && (d->loader != LOAD_PLAIN || d->ln))
    return fail(FZ_E_UNSUPPORTED, "fz_gemm: odd K only with the plain loader and no LayerNorm prologue");
  if (d->loader == LOAD_K3 && (d->epilogue != EPI_PLAIN || d->ln || d->src_mode != 0 || d->nsrc != 1 ||
                               (d->Wi & 3) || d->K != 27 * d->Cin || (d->Cin & 1)))
    return fail(FZ_E_UNSUPPORTED, "fz_gemm: k3 loader needs W % 4 == 0, even Cin, K = 27*Cin, plain epilogue");
  if (d->bmul && (d->loader != LOAD_PLAIN || d->src_mode != 0 || d->nsrc != 1))
    return fail(FZ_E_UNSUPPORTED, "fz_gemm: bmul needs the plain single-source loader");
  if (d->Ncol % 4 != 0 && d->loader != LOAD_S2D) return fail(FZ_E_UNSUPPORTED, "fz_gemm: voxel count must be a multiple of 4");
  if (d->loader == LOAD_S2D && ((d->Wo & 1) || d->epilogue != EPI_PLAIN || d->ln || d->src_mode != 0 || d->nsrc != 1))
    return fail(FZ_E_UNSUPPORTED, "fz_gemm: space-to-depth loader needs even coarse width, plain epilogue");
  if (d->epilogue == EPI_D2S && (d->M % 8 != 0)) return fail(FZ_E_SHAPE, "fz_gemm: depth-to-space rows must be 8*C");
  if (d->nsrc < 1 || d->nsrc > 2 || d->src_mode != 0)
    return fail(FZ_E_UNSUPPORTED, "fz_gemm: one source, or two sources concatenated along channels");
  if (d->bmul && d->bmul_kind != ACT_RELU) return fail(FZ_E_UNSUPPORTED, "fz_gemm: bmul supports the ReLU gate");
  // (the gate is applied as the operand is fetched: in front of a LayerNorm or an activation it would gate their INPUT, which
  // is not what the header promises and what no layer asks for; the streaming kernels refuse the pairing anyway)
  if (d->bmul && (d->ln || d->bact)) return fail(FZ_E_UNSUPPORTED, "fz_gemm: bmul with a LayerNorm or activation prologue");
  // ---- no field is dropped: what no kernel of the family reads for this loader / epilogue is refused, and so is what would
  // send a kernel through a null pointer (fetch_plain reads x[1] for every channel >= c0) ----
  if (d->nsrc == 2 && !d->x[1]) return fail(FZ_E_ARG, "fz_gemm: two sources need x[1]");
  if (d->nsrc == 2 && (d->c0 <= 0 || d->c0 >= d->Cin))
    return fail(FZ_E_UNSUPPORTED, "fz_gemm: two sources need 0 < c0 < Cin (x[0] holds c0 channels, x[1] the other Cin - c0)");
  if (d->nsrc == 1 && d->c0 != 0 && d->c0 != d->Cin) return fail(FZ_E_UNSUPPORTED, "fz_gemm: one source takes c0 = 0 (or Cin)");
  if (d->bact < ACT_NONE || d->bact > ACT_GELU || d->eact < ACT_NONE || d->eact > ACT_GELU || (d->emul && (d->emul_kind < ACT_NONE || d->emul_kind > ACT_GELU)))
    return fail(FZ_E_ARG, "fz_gemm: bact / eact / emul_kind must be FZ_ACT_NONE, FZ_ACT_RELU or FZ_ACT_GELU");
  if (d->ln && (!d->ln_g || !d->ln_b)) return fail(FZ_E_ARG, "fz_gemm: the LayerNorm prologue needs ln_g and ln_b");
  // (every kernel folds the LayerNorm affine into its staged weights, W·diag(γ) and W·β: an activation would have to sit between
  // the affine and the product.  The resident and the persistent kernel used to accept the pair and compute W·(γ ∘ act(x̂)) + W·β)
  if (d->ln && d->bact) return fail(FZ_E_UNSUPPORTED, "fz_gemm: an input activation behind the LayerNorm prologue is not computed");
  // (gemm_chain64_kernel reads no input activation; the M = 32 form on the resident kernel applies it)
  if (lnb64 && d->bact)
    return fail(FZ_E_UNSUPPORTED, "fz_gemm: the 64-channel LayerNorm-backward epilogue takes no input activation");
  if (d->stats_out && !d->ln) return fail(FZ_E_UNSUPPORTED, "fz_gemm: stats_out without the LayerNorm prologue (nothing writes it)");
  if (d->epilogue == EPI_D2S && (d->eact || d->emul))
    return fail(FZ_E_UNSUPPORTED, "fz_gemm: depth-to-space epilogue takes bias and res, no eact / emul");
  // (store_block's depth-to-space form has no W·β row term: the resident kernel used to accept the pair and drop β)
  if (d->epilogue == EPI_D2S && d->ln) return fail(FZ_E_UNSUPPORTED, "fz_gemm: depth-to-space epilogue behind a LayerNorm prologue");
  if ((d->loader == LOAD_S2D || d->loader == LOAD_K3) && d->bact)
    return fail(FZ_E_UNSUPPORTED, "fz_gemm: space-to-depth and k3 loaders take no input activation");
  if (d->B == 0) return FZ_OK;
  GemmArgsT<AT> a;
  for (int i = 0; i < 4; ++i) a.x[i] = (const AT*)d->x[i];
  a.nsrc = d->nsrc; a.src_mode = d->src_mode; a.c0 = d->c0 > 0 ? d->c0 : d->Cin; a.Cin = d->Cin;
  a.Vin = d->Vin; a.Di = d->Di; a.Hi = d->Hi; a.Wi = d->Wi; a.bmul = (const AT*)d->bmul; a.bmul_kind = d->bmul_kind;
  a.w = d->w; a.w_t = d->w_t; a.ldw = d->ldw; a.M = d->M; a.K = d->K;
  a.bias = d->bias; a.ln = d->ln; a.ln_g = d->ln_g; a.ln_b = d->ln_b; a.ln_eps = d->ln_eps;
  a.stats_out = d->stats_out; a.bact = d->bact; a.eact = d->eact; a.res = (const AT*)d->res; a.emul = (const AT*)d->emul;
  a.emul_kind = d->emul_kind; a.y = (AT*)d->y; a.Ncol = d->Ncol; a.Ho = d->Ho; a.Wo = d->Wo; a.B = d->B;
  if (d->loader == LOAD_S2D_2D || d->loader == LOAD_K3_2D) a.Di = 1;   // the kernels' depth bound of a 2-D grid
  a.dbg = 0; a.tile_map = 1;
  a.ygroups = 0; a.xtiles = 0; a.tune = d->tune;
  a.lnb_x = (const AT*)d->lnb_x; a.lnb_stats = d->lnb_stats; a.lnb_g = d->lnb_g; a.lnb_gadd = (const AT*)d->lnb_gadd; a.lnb_part = d->lnb_part;
  hipStream_t st = (hipStream_t)stream;
  const int mblocks = (d->M + 31) / 32;
  if (lnb64) return chain64_lnb_launch<AT>(d, a, stream);   // 64 -> 64 input gradient + LayerNorm backward over 64 channels

  // ---- split-bf16 MFMA family (gemm_bx.hip): every layer with a reduction length >= 64 (stages 1-4 of the U-shape) ----
  // fp32 products as six exact bf16 products on the bf16 matrix pipe (6/16 of the fp32-MFMA time, error <= the fp32
  // MFMA's own: tools/probes/bx6_accuracy.hip); FZ_GEMM_BX=0 keeps every GEMM on v_mfma_f32_32x32x2_f32
  {
    const int bx_on = products_split(d->products);
    const int pro_bx = d->ln ? 1 : (d->bact == ACT_GELU ? 2 : (d->bmul ? 3 : 0));
    const bool one_pro = (d->ln != 0) + (d->bact != 0) + (d->bmul != nullptr) <= 1;
    // (bf16 storage, no prologue: from K = 32 — three bf16 products per fp32 product; the stage-0 layers are matrix-pipe
    // bound there once their bytes are halved.  With a LayerNorm / GELU prologue the K = 32 half chunk would cost as
    // much as the fp32 MFMAs it replaces; fp32 storage: those layers are HBM-bound on the fp32 MFMA)
    const int bx_kmin = (sizeof(AT) == 2 && !d->ln && d->bact == 0) ? 32 : 64;
    if (bx_on && one_pro && d->bact != ACT_RELU && d->K >= bx_kmin && d->M >= 32 && (d->loader == LOAD_PLAIN || d->loader == LOAD_S2D) &&
        (d->epilogue == EPI_PLAIN || d->epilogue == EPI_D2S) && !(d->loader == LOAD_S2D && pro_bx) && !(d->epilogue == EPI_D2S && pro_bx))
    {
      const int rc = gemm_bx_launch<AT>(a, d->loader, d->epilogue, pro_bx, stream);
      if (rc != FZ_E_UNSUPPORTED) return rc;   // shapes outside the family (K % 64, M % 32, alignment): the kernels below
    }
  }

  // ---- the head: Linear(32 -> M <= 4), nothing fused: 32·M FMAs per voxel on the VALU, bandwidth-bound (headbwd.hip) ----
  if (knob_head_fwd() && d->loader == LOAD_PLAIN && d->epilogue == EPI_PLAIN && d->M <= 4 && d->K == 32 && d->Cin == 32 && a.c0 == 32 &&
      !d->ln && !d->bact && !d->eact && !d->res && !d->bmul && !d->emul && !d->w_t && d->ldw == 32 && d->Ncol == d->Vin && d->Ncol % 4 == 0 &&
      d->Ncol / 4 < ((int64_t)1 << 31) && (int64_t)d->B * (d->Ncol / 4) < ((int64_t)1 << 31) && d->stats_out == nullptr)
    return fz_head_fwd(d->x[0], d->w, d->bias, d->y, d->B, d->M, 32, d->Ncol, d->act_dtype, stream);

  // ---- Kernel A': persistent 32 -> 32 without a residual (stage 0: LayerNorm + in-projection, plain projections) ----
  if (knob_p32() && d->loader == LOAD_PLAIN && d->epilogue == EPI_PLAIN && d->M <= 32 && d->K == 32 && d->Cin == 32 && (a.c0 & 1) == 0 && d->Vin < ((int64_t)1 << 28) &&
      (int64_t)5 * d->Ncol * (int64_t)sizeof(AT) < ((int64_t)1 << 32) /* 32-bit store offsets (4·h·Ncol + col)·es */ && !d->res && !d->bmul &&
      !d->emul && d->Ncol % 4 == 0 && d->Ncol == d->Vin && d->B * ((d->Ncol + 127) / 128) >= 4096 && d->B * ((d->Ncol + 127) / 128) < ((int64_t)1 << 30) &&
      !(d->bact && !d->ln) /* the activation-only form needs scratch at two waves per SIMD: Kernel A keeps it */) {
    return gemm_p32_launch<AT>(d, a, stream);
  }

  // ---- Kernel A: whole operand in registers (K <= 64, plain loader) ----
  // measured (round-1/2 probe `gemm_probe5`): the register-resident kernel wins for K <= 32, the
  // streaming ring for K = 64 (4.4 vs 3.3 TB/s at 64->32, 128^3)
  int res_maxk = 32;
  if (d->epilogue == EPI_LNBWD) res_maxk = 64;
  // ... except one 32-row block without a residual or gate: with the ring refills pinned the streaming
  // kernel overlaps its MFMAs with the loads still in flight, which the LayerNorm prologue of the
  // resident kernel cannot (it needs the whole column first): 32->32 at 128^3, LayerNorm + ReLU 345 -> 274 us,
  // plain 278 -> 248 us; with a residual (357 vs 362 us) or two row blocks (391 vs 439 us) the resident
  // kernel stays ahead (round-1/2 probe `gemm_probe9`)
  const bool stream_small = mblocks == 1 && d->K >= 16 && d->K <= 32 && !d->res && !d->bmul && !d->emul &&
                            d->epilogue == EPI_PLAIN && d->bact == 0;
  if (d->loader == LOAD_PLAIN && d->K <= res_maxk && !stream_small && d->epilogue != EPI_D2S_2D) {
    const int nA = (d->K + 1) / 2;
    int RB = mblocks < 8 ? mblocks : 8;
    while ((size_t)(nA * RB * 64 + 32 * RB) * sizeof(float) > 65536) --RB;
    const size_t lds = (size_t)(nA * RB * 64 + 32 * RB + (d->epilogue == EPI_LNBWD ? 256 : 0)) * sizeof(float);
    const int64_t tiles = (d->Ncol + 511) / 512;
    dim3 grid((unsigned)(tiles * d->B), (unsigned)((mblocks + RB - 1) / RB)), block(256);
// (fz_gemm_plan's dry run, fz_common.h: the form is named and nothing is launched)
#define FZ_RES_FORM(NS, E, PFv, EXTRA)                                                                                          \
  if (gemm_plan_only())                                                                                                       \
    return gemm_plan_form("resident ns%d plain%s pf%d%s rb=%d grid=%ux%u", NS, gemm_epi_name(E), PFv, EXTRA, RB, grid.x, grid.y)
#define FZ_RES_PF(NS, E, BM, PFv)                                                                                              \
  do { FZ_RES_FORM(NS, E, PFv, BM ? " bmul" : ""); hipLaunchKernelGGL((gemm_resident_kernel<NS, E, BM, false, AT, PFv>), grid, block, lds, st, a, RB); } while (0)
#define FZ_RES(NS, E, BM)                                                  \
  do {                                                                    \
    const int pf = (d->bact ? 1 : 0) | (d->ln ? 2 : 0);                   \
    if (pf == 0) FZ_RES_PF(NS, E, BM, 0);                                 \
    else if (pf == 1) FZ_RES_PF(NS, E, BM, 1);                            \
    else FZ_RES_PF(NS, E, BM, 2); /* (pf 3, LayerNorm + activation, is refused in gemm_launch) */ \
  } while (0)
    if (d->epilogue == EPI_LNBWD) {
      if (d->bmul) return fail(FZ_E_UNSUPPORTED, "fz_gemm: bmul with LayerNorm-backward epilogue");
#define FZ_RES_LNB(NS, GA)                                                                                                     \
  do { FZ_RES_FORM(NS, EPI_LNBWD, 3, GA ? " gadd" : ""); hipLaunchKernelGGL((gemm_resident_kernel<NS, EPI_LNBWD, false, GA>), grid, block, lds, st, a, RB); } while (0)
      if (d->lnb_gadd) { if (nA <= 16) FZ_RES_LNB(16, true); else FZ_RES_LNB(32, true); }
      else { if (nA <= 16) FZ_RES_LNB(16, false); else FZ_RES_LNB(32, false); }
    } else if (d->epilogue == EPI_D2S) {
      if (d->bmul) return fail(FZ_E_UNSUPPORTED, "fz_gemm: bmul with depth-to-space epilogue");
      if (nA <= 16) FZ_RES(16, EPI_D2S, false); else FZ_RES(32, EPI_D2S, false);
    } else if (d->bmul) {
      if (nA <= 16) FZ_RES(16, EPI_PLAIN, true); else FZ_RES(32, EPI_PLAIN, true);
    } else if (d->res && !d->emul && d->M == 32 && nA <= 16 && !d->ln && knob_res_prefetch()) {
#define FZ_RES_RESPF(PFv)                                                                                                      \
  do { FZ_RES_FORM(16, EPI_PLAIN, PFv, " respf"); hipLaunchKernelGGL((gemm_resident_kernel<16, EPI_PLAIN, false, false, AT, PFv, true>), grid, block, lds, st, a, RB); } while (0)
      if (d->bact) FZ_RES_RESPF(1); else FZ_RES_RESPF(0);
    } else {
      if (nA <= 16) FZ_RES(16, EPI_PLAIN, false); else FZ_RES(32, EPI_PLAIN, false);
    }
    FZ_LAUNCH_CHECK();
    return FZ_OK;
  }

  // ---- Kernel B: streaming (gemm_stream.hip) ----
  return gemm_stream_launch<AT>(d, a, stream);
}

extern "C" int fz_gemm(const fz_gemm_desc* d, fz_stream_t stream) {
  if (!d) return fail(FZ_E_ARG, "fz_gemm: null descriptor");
  if (d->act_dtype == FZ_STORE_F32) return gemm_launch<float>(d, stream);
  if (d->act_dtype == FZ_STORE_BF16) return gemm_launch<bf16>(d, stream);
  return fail(FZ_E_ARG, "fz_gemm: act_dtype must be FZ_STORE_F32 or FZ_STORE_BF16");
}

// Dry run: fz_gemm itself with this thread's plan flag set — every launch site names its form and returns in place of
// launching (gemm_plan_only, fz_common.h), so the form reported is the form fz_gemm launches.
extern "C" int fz_gemm_plan(const fz_gemm_desc* d, char* form, int cap) {
  GemmPlan& pl = gemm_plan();
  pl.only = true;
  pl.form[0] = 0;
  const int rc = fz_gemm(d, nullptr);
  pl.only = false;
  if (form && cap > 0) snprintf(form, (size_t)cap, "%s", rc == FZ_OK ? pl.form : "");
  return rc;
}

extern "C" int64_t fz_gemm_lnbwd_partials(const fz_gemm_desc* d) {
  if (!d) return -1;
  if (d->M == 64) return fz_mlp_partials(d->B, d->Ncol);   // 256-voxel tiles, rows of 128 floats
  return ((d->Ncol + 511) / 512) * d->B;  // one row per workgroup of the resident kernel (rows of 64 floats)
}
