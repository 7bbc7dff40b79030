// mlp_chain.hip — host side of the chained block MLP: fz_mlp_chain and its companions check a descriptor, fill the argument
// blocks and hand them to the launcher of the kernel that runs it — gemm_chain_kernel (C = 32, mlp_chain32.hip),
// gemm_chain64_kernel (C = 64, mlp_chain64.hip) or gemm_chain_bwd_wg_kernel (backward with the weight gradients, mlp_chain_wg.hip).
#include "mlp_chain.h"     // ChainArgsT, the knobs, chain32_launch, chain64_launch, chain_wg_launch

using namespace fz;

// Columns per lane of every chain kernel (a workgroup walks tiles of 128 times as many columns).
// 2: 64-column wave tiles, <= 168 VGPRs → 3 waves/SIMD with the next-tile prefetch
// (4 columns per lane: 0.71 / 1.38 ms against 0.63 / 1.00 ms, round-1/2 probe `mlp_probe`)
static int mlp_nacc() { return 2; }

extern "C" int64_t fz_mlp_partials(int B, int64_t V) {
  const int64_t tw = 128 * mlp_nacc();
  return ((V + tw - 1) / tw) * (int64_t)B;
}

extern "C" int fz_mlp_pre_supported(int C, int H, int64_t V, int products) {
  if (!(V > 0 && (V % 4) == 0 && V <= ((int64_t)1 << 27) && products_split(products))) return 0;
  if (C == 32 && H == 64) return knob_chain_fwd_bx() ? 1 : 0;
  // C = 64: the 512-thread form around the pre-split images, which walks the tiles in pairs (an even number per sample)
  if (C == 64 && H == 128) return (((V + 255) / 256) % 2 == 0 && knob_chain64_p512()) ? 1 : 0;
  return 0;
}

// where both consumers of the core's output a at C = 32 — this chain's GEMM 0 and fz_gemm_dw's q operand — rebuild a from the
// factors of the core's two windows (outproj_fac.h) and a is never stored
extern "C" int fz_outproj_factors_supported(int C, int Hd, int D, int H, int W, int d, int pd, int ph, int pw, int R, int T, int Tgrad,
                                            int nshift, const int* shifts, int act_dtype, int products, int dropout) {
  if (C != 32 || Hd != 64 || act_dtype != FZ_STORE_F32 || dropout || nshift != 2) return 0;
  if (!fz_nmf_cf_factors_supported(C, D, H, W, d, pd, ph, pw, R, T, Tgrad, nshift, shifts)) return 0;
  return fz_mlp_pre_supported(C, Hd, (int64_t)D * H * W, products);   // split-bf16 products, V <= 2^27 (fz_gemm_dw's bound too)
}

extern "C" int fz_mlp_supported(int C, int H, int64_t V) {
  const bool shape = (C == 32 && (H == 64 || H == 128)) || (C == 64 && H == 128);
  return (shape && V > 0 && (V % 4) == 0 && V <= ((int64_t)1 << 27)) ? 1 : 0;
}

extern "C" int fz_mlp_drop_supported(int C, int H, int64_t V, int products) {
  return (C == 32 && H == 64 && fz_mlp_supported(C, H, V) && fz_mlp_pre_supported(C, H, V, products) && products_split(products)
          && knob_chain_fwd_bx()) ? 1 : 0;
}

// The argument blocks of the chain (GemmArgsT: GEMM 1 and the epilogue; ChainArgsT: GEMM 2 and the fused neighbours).
// forward: A1[m][k] = W1[m][k] behind the LayerNorm, A2[m][k] = W2[m][k]; z1 goes to `side`
template <typename AT>
static void forward_args(const fz_mlp_desc* d, bool fac, int ldw, int ldwB, GemmArgsT<AT>& a, ChainArgsT<AT>& c) {
  a.w = d->w1; a.w_t = 0; a.ldw = ldw;
  a.bias = d->b1; a.ln = 1; a.ln_g = d->ln_g; a.ln_b = d->ln_b; a.ln_eps = d->ln_eps; a.stats_out = d->stats;
  a.res = (const AT*)d->in; a.y = (AT*)d->out;
  c.wB = d->w2; c.wB_t = 0; c.ldwB = ldwB; c.biasB = d->b2; c.side = (AT*)d->z1;
  if (d->pre_in || fac) {   // the block's out-projection in front of the chain (x1 is then an OUTPUT), at C = 32 the head behind it; fac: pre_in stays null
    c.preA = (const AT*)d->pre_in; c.preW = d->pre_w; c.preB = d->pre_b; c.preRes = (const AT*)d->pre_res; c.preOut = (AT*)d->pre_out;
    if (d->C == 64) a.res = (const AT*)d->pre_out;   // the epilogue's residual: the lane's own x1, written a moment earlier
    else { c.postW = d->post_w; c.postB = d->post_b; c.postOut = (AT*)d->post_out; c.postM = d->post_m; }
  }
}
// backward: A1[m = hidden][k = c] = W2[c][hidden], A2[m = c][k = hidden] = W1[hidden][c]; `side` takes gz1 (null: not stored)
template <typename AT>
static void backward_args(const fz_mlp_desc* d, int ldw, int ldwB, AT* side, GemmArgsT<AT>& a, ChainArgsT<AT>& c) {
  a.w = d->w2; a.w_t = 1; a.ldw = ldw;
  a.emul = (const AT*)d->z1; a.y = (AT*)d->out;
  a.lnb_x = (const AT*)d->x1; a.lnb_stats = d->stats; a.lnb_g = d->ln_g; a.lnb_gadd = (const AT*)d->in; a.lnb_part = d->part;
  c.wB = d->w1; c.wB_t = 1; c.ldwB = ldwB; c.side = side;
}

// what fz_mlp_chain refuses, in the order its callers see it
static int mlp_check(const fz_mlp_desc* d, const fz_mlp_dropout* dd, bool drop, bool fac) {
  if (!fz_mlp_supported(d->C, d->H, d->V)) return fail(FZ_E_UNSUPPORTED, "fz_mlp_chain: needs (C, H) in {(32, 64), (32, 128), (64, 128)}, V % 4 == 0");
  if (drop) {
    if (!fz_mlp_drop_supported(d->C, d->H, d->V, d->products) || d->mode != 0 || !d->pre_in)
      return fail(FZ_E_UNSUPPORTED, "fz_mlp_chain: dropout needs (C, H) = (32, 64), split-bf16 products, mode 0 with pre_in (fz_mlp_drop_supported)");
    if (!drop_scale_ok(dd->m0, dd->s0) || !drop_scale_ok(dd->m1, dd->s1) || !drop_scale_ok(dd->m2, dd->s2))
      return fail(FZ_E_ARG, "fz_mlp_chain: a dropout scale 1 / (1 - p) must be >= 1 and finite");
  }
  if (d->C == 64 && d->mode == 2) return fail(FZ_E_UNSUPPORTED, "fz_mlp_chain: the fused weight gradients need C == 32, H == 64");
  if (d->B < 0) return fail(FZ_E_SHAPE, "fz_mlp_chain: negative batch");
  // the factor form of pre_in (fz_mlp_chain_fac: the core's output as the rank-1 factors of its two windows) exists for one
  // kernel; every other launch that brings factors is refused, never run on a tensor that is not there
  if (fac && (d->C != 32 || d->H != 64 || d->mode != 0 || d->act_dtype != FZ_STORE_F32 || drop || d->pre_in
              || !fz_mlp_pre_supported(d->C, d->H, d->V, d->products)))
    return fail(FZ_E_UNSUPPORTED, "fz_mlp_chain_fac: needs (C, H) = (32, 64), mode 0, fp32 storage, split-bf16 products, pre_in == NULL (fz_outproj_factors_supported)");
  const bool pre = d->pre_in != nullptr || fac;   // the block's out-projection in front of the forward chain (x1 is then an OUTPUT)
  if (pre && (d->mode != 0 || !d->pre_w || !d->pre_res || !d->pre_out))
    return fail(FZ_E_ARG, "fz_mlp_chain: pre_in needs mode 0, pre_w, pre_res, pre_out (see fz_mlp_pre_supported)");
  if (pre && !fz_mlp_pre_supported(d->C, d->H, d->V, d->products))
    return fail(FZ_E_UNSUPPORTED, "fz_mlp_chain: the fused out-projection runs on split-bf16 products only (fz_mlp_pre_supported)");
  if (d->post_out && (!pre || d->C != 32 || !d->post_w || d->post_m < 1 || d->post_m > 4))
    return fail(FZ_E_ARG, "fz_mlp_chain: post_out needs pre_in, C == 32, post_w and 1 <= post_m <= 4");
  if ((!d->in && !pre) || !d->w1 || !d->w2 || !d->out || !d->z1 || !d->stats)
    return fail(FZ_E_ARG, "fz_mlp_chain: null pointer");
  if (d->mode == 0 && (!d->ln_g || !d->ln_b)) return fail(FZ_E_ARG, "fz_mlp_chain: forward needs the LayerNorm affine");
  if (d->mode == 1 && (!d->gz1 || !d->x1 || !d->ln_g || !d->part)) return fail(FZ_E_ARG, "fz_mlp_chain: backward needs gz1, x1, gamma, part");
  if (d->mode == 2 && (!d->x1 || !d->ln_g || !d->ln_b || !d->gln || !d->wpart || !d->gw1 || !d->gb1 || !d->gw2 || !d->gb2))
    return fail(FZ_E_ARG, "fz_mlp_chain: backward with weight gradients needs x1, gamma, beta, gln, wpart, gw1, gb1, gw2, gb2");
  if (d->mode == 2 && d->H == 128 && !d->glp) return fail(FZ_E_ARG, "fz_mlp_chain: the fused weight gradients at H == 128 need the glp buffer");
  if (d->mode < 0 || d->mode > 2) return fail(FZ_E_ARG, "fz_mlp_chain: bad mode");
  return FZ_OK;
}

template <typename AT>
static int mlp_launch(const fz_mlp_desc* d, const fz_mlp_dropout* dd, const fz_outproj_fac* fac, fz_stream_t stream) {
  const bool drop = dd && (dd->m0 || dd->m1 || dd->m2);   // block dropout: the DROP form of mode 0 with pre_in
  const int rc = mlp_check(d, dd, drop, fac != nullptr);
  if (rc != FZ_OK) return rc;
  if (d->B == 0) {
    if (d->mode == 2) {   // no voxels: the sums are empty
      hipStream_t s0 = (hipStream_t)stream;
      FZ_HIP_OK(hipMemsetAsync(d->gw1, 0, sizeof(float) * d->H * 32, s0));
      FZ_HIP_OK(hipMemsetAsync(d->gw2, 0, sizeof(float) * d->H * 32, s0));
      FZ_HIP_OK(hipMemsetAsync(d->gb1, 0, sizeof(float) * d->H, s0));
      FZ_HIP_OK(hipMemsetAsync(d->gb2, 0, sizeof(float) * 32, s0));
      FZ_HIP_OK(hipMemsetAsync(d->gln, 0, sizeof(float) * 64, s0));
    }
    return FZ_OK;
  }
  GemmArgsT<AT> a = {};
  ChainArgsT<AT> c = {};
  a.x[0] = (const AT*)d->in; a.nsrc = 1; a.c0 = d->C; a.Cin = d->C; a.Vin = d->V; a.M = d->H; a.K = d->C; a.Ncol = d->V; a.B = d->B;
  if (d->mode == 0) forward_args(d, fac != nullptr, d->C, d->H, a, c);
  else backward_args(d, d->H, d->C, d->mode == 1 ? (AT*)d->gz1 : (AT*)nullptr, a, c);   // (mode 2 keeps gz1 on chip)
  if (d->C == 64) return chain64_launch(d, a, c, stream);
  if (d->mode == 2) return chain_wg_launch(d, a, c, stream);
  return chain32_launch(d, drop ? dd : nullptr, fac, a, c, stream);
}

extern "C" int fz_mlp_chain(const fz_mlp_desc* d, fz_stream_t stream) {
  if (!d) return fail(FZ_E_ARG, "fz_mlp_chain: null descriptor");
  if (d->act_dtype == FZ_STORE_F32) return mlp_launch<float>(d, nullptr, nullptr, stream);
  if (d->act_dtype == FZ_STORE_BF16) return mlp_launch<bf16>(d, nullptr, nullptr, stream);
  return fail(FZ_E_ARG, "fz_mlp_chain: act_dtype must be FZ_STORE_F32 or FZ_STORE_BF16");
}

extern "C" int fz_mlp_chain_fac(const fz_mlp_desc* d, const fz_outproj_fac* fac, fz_stream_t stream) {
  if (!d || !fac) return fail(FZ_E_ARG, "fz_mlp_chain_fac: null descriptor");
  if (d->act_dtype == FZ_STORE_F32) return mlp_launch<float>(d, nullptr, fac, stream);
  if (d->act_dtype == FZ_STORE_BF16) return mlp_launch<bf16>(d, nullptr, fac, stream);   // (refused by the checks: fp32 storage only)
  return fail(FZ_E_ARG, "fz_mlp_chain_fac: act_dtype must be FZ_STORE_F32 or FZ_STORE_BF16");
}

extern "C" int fz_mlp_chain_drop(const fz_mlp_desc* d, const fz_mlp_dropout* drop, fz_stream_t stream) {
  if (!d || !drop) return fail(FZ_E_ARG, "fz_mlp_chain_drop: null descriptor");
  if (d->act_dtype == FZ_STORE_F32) return mlp_launch<float>(d, drop, nullptr, stream);
  if (d->act_dtype == FZ_STORE_BF16) return mlp_launch<bf16>(d, drop, nullptr, stream);
  return fail(FZ_E_ARG, "fz_mlp_chain_drop: act_dtype must be FZ_STORE_F32 or FZ_STORE_BF16");
}
