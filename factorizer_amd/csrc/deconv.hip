// deconv.hip — the C entry points of the grouped "same" cross-correlation (kernels and launchers: deconv_kernels.h) and its
// fp32 instantiations; the bf16 ones are compiled in deconv_bf16.hip.
#include "deconv_kernels.h"

using namespace fz;

extern "C" int fz_gcorr_supported(int Ci, int Co, int kd, int kh, int kw) {
  if (Ci < 1 || Co < 1) return 0;
  return gc_odd7(kd) && gc_odd7(kh) && gc_odd7(kw) ? 1 : 0;   // (the generic kernels take what the instantiations do not)
}

// the checks every form of the forward launch shares; > 0: nothing to do (B == 0)
static int gc_check(const char* who, int B, int G, int Ci, int Co, int D, int H, int W, int kd, int kh, int kw, int act_dtype) {
  auto say = [&](int code, const char* what) { return fail(code, (std::string(who) + ": " + what).c_str()); };
  if (B < 0 || G < 1 || D < 1 || H < 1 || W < 1) return say(FZ_E_SHAPE, "bad sizes");
  if (!fz_gcorr_supported(Ci, Co, kd, kh, kw)) return say(FZ_E_UNSUPPORTED, "needs odd kernel extents <= 7");
  if (act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16) return say(FZ_E_UNSUPPORTED, "act_dtype must be FZ_STORE_F32 or FZ_STORE_BF16");
  if (B == 0) return 1;
  if (G > 65535 || B > 65535) return say(FZ_E_UNSUPPORTED, "more than 65535 groups / samples");
  return FZ_OK;
}

template <typename AT>
static GcArgs<AT> gc_args(const void* in, const float* w, void* out, const void* mul_a, const void* mul_b, const void* mul_c,
                          void* out2, void* out3, int B, int G, int Ci, int Co, int D, int H, int W, int w_batched, int epilogue,
                          float add_eps) {
  return GcArgs<AT>{(const AT*)in, w, (AT*)out, (const AT*)mul_a, (const AT*)mul_b, (const AT*)mul_c, (AT*)out2, (AT*)out3,
                    B, G, Ci, Co, D, H, W, w_batched ? 1 : 0, epilogue, add_eps, 0, 0, 0};
}

// out = corr(in, w) [+ eps]  or, with mul_a / mul_b, the fused multiplicative update  mul_a ∘ mul_b / (corr + eps).
// in (B, G·Ci, D, H, W); w (Bw, G, Co, Ci, kd, kh, kw) with Bw = B if w_batched else 1, fp32; out (B, G·Co, D, H, W).
// in / out / mul_a / mul_b: float or bf16 by act_dtype.
extern "C" int fz_gcorr_act(const void* in, const float* w, void* out, const void* mul_a, const void* mul_b, int B, int G,
                            int Ci, int Co, int D, int H, int W, int kd, int kh, int kw, int w_batched, float add_eps,
                            int act_dtype, fz_stream_t stream) {
  if (!in || !w || !out || ((mul_a == nullptr) != (mul_b == nullptr))) return fail(FZ_E_ARG, "fz_gcorr: null pointer");
  const int rc = gc_check("fz_gcorr", B, G, Ci, Co, D, H, W, kd, kh, kw, act_dtype);
  if (rc) return rc > 0 ? FZ_OK : rc;
  const int ep = mul_a ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (act_dtype == FZ_STORE_BF16)
    return gcorr_launch_bf16(gc_args<bf16>(in, w, out, mul_a, mul_b, nullptr, nullptr, nullptr, B, G, Ci, Co, D, H, W, w_batched, ep, add_eps),
                             kd, kh, kw, st);
  return gcorr_launch<float>(gc_args<float>(in, w, out, mul_a, mul_b, nullptr, nullptr, nullptr, B, G, Ci, Co, D, H, W, w_batched, ep, add_eps),
                             kd, kh, kw, st);
}

extern "C" int fz_gcorr(const float* in, const float* w, float* out, const float* mul_a, const float* mul_b, int B, int G,
                        int Ci, int Co, int D, int H, int W, int kd, int kh, int kw, int w_batched, float add_eps,
                        fz_stream_t stream) {
  return fz_gcorr_act(in, w, out, mul_a, mul_b, B, G, Ci, Co, D, H, W, kd, kh, kw, w_batched, add_eps, FZ_STORE_F32, stream);
}

// Backward of the multiplicative update s' = s ∘ num / den, den = corr(r, wT) + eps, in one launch: den is recomputed in the
// accumulators and, from g = dL/ds',  ds = g ∘ num / den,  dnum = g ∘ s / den,  dden = −g ∘ s ∘ num / den²  are written (each
// output may be null and is then skipped, not all three).  r (B, G·Ci, D, H, W); g, s, num, ds, dnum, dden (B, G·Co, D, H, W).
extern "C" int fz_gcorr_mu_bwd(const void* r, const float* wT, const void* g, const void* s, const void* num, void* ds, void* dnum,
                               void* dden, int B, int G, int Ci, int Co, int D, int H, int W, int kd, int kh, int kw,
                               int w_batched, float eps, int act_dtype, fz_stream_t stream) {
  if (!r || !wT || !g || !s || !num || (!ds && !dnum && !dden)) return fail(FZ_E_ARG, "fz_gcorr_mu_bwd: null pointer");
  const int rc = gc_check("fz_gcorr_mu_bwd", B, G, Ci, Co, D, H, W, kd, kh, kw, act_dtype);
  if (rc) return rc > 0 ? FZ_OK : rc;
  hipStream_t st = (hipStream_t)stream;
  if (act_dtype == FZ_STORE_BF16)
    return gcorr_launch_bf16(gc_args<bf16>(r, wT, ds, g, s, num, dnum, dden, B, G, Ci, Co, D, H, W, w_batched, 2, eps), kd, kh, kw, st);
  return gcorr_launch<float>(gc_args<float>(r, wT, ds, g, s, num, dnum, dden, B, G, Ci, Co, D, H, W, w_batched, 2, eps), kd, kh, kw, st);
}

extern "C" int64_t fz_gcorr_wgrad_workspace_bytes(int B, int G, int Ci, int Co, int D, int H, int W, int kd, int kh, int kw) {
  if (B < 1 || G < 1 || Ci < 1 || Co < 1 || D < 1 || H < 1 || W < 1) return 0;
  const int ntiles = ((D + kTD - 1) / kTD) * ((H + kTH - 1) / kTH) * ((W + kTW - 1) / kTW);
  return (int64_t)B * G * gcw_chunks(B, G, Ci, ntiles) * Co * Ci * kd * kh * kw * (int64_t)sizeof(float);
}

// Filter gradient of fz_gcorr: gw (Bw, G, Co, Ci, kd, kh, kw), fp32, from in (B, G·Ci, D, H, W) and gout (B, G·Co, D, H, W),
// float or bf16 by act_dtype; ws: fz_gcorr_wgrad_workspace_bytes(...) bytes (the same for both storage types).
extern "C" int fz_gcorr_wgrad_act(const void* in, const void* gout, float* gw, void* ws, int B, int G, int Ci, int Co, int D,
                                  int H, int W, int kd, int kh, int kw, int w_batched, int act_dtype, fz_stream_t stream) {
  if (!in || !gout || !gw || !ws) return fail(FZ_E_ARG, "fz_gcorr_wgrad: null pointer");
  if (B < 1 || G < 1 || D < 1 || H < 1 || W < 1) return fail(FZ_E_SHAPE, "fz_gcorr_wgrad: bad sizes");
  if (!fz_gcorr_supported(Ci, Co, kd, kh, kw))
    return fail(FZ_E_UNSUPPORTED, "fz_gcorr_wgrad: needs odd kernel extents <= 7");
  if (act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16)
    return fail(FZ_E_UNSUPPORTED, "fz_gcorr_wgrad: act_dtype must be FZ_STORE_F32 or FZ_STORE_BF16");
  if ((int64_t)G * Ci > 65535 || B > 65535) return fail(FZ_E_UNSUPPORTED, "fz_gcorr_wgrad: more than 65535 (group, channel) pairs / samples");
  hipStream_t st = (hipStream_t)stream;
  if (act_dtype == FZ_STORE_BF16)
    return gcorr_wgrad_launch_bf16((const bf16*)in, (const bf16*)gout, gw, ws, B, G, Ci, Co, D, H, W, kd, kh, kw, w_batched, st);
  return gcorr_wgrad_launch<float>((const float*)in, (const float*)gout, gw, ws, B, G, Ci, Co, D, H, W, kd, kh, kw, w_batched, st);
}

extern "C" int fz_gcorr_wgrad(const float* in, const float* gout, float* gw, void* ws, int B, int G, int Ci, int Co, int D,
                              int H, int W, int kd, int kh, int kw, int w_batched, fz_stream_t stream) {
  return fz_gcorr_wgrad_act(in, gout, gw, ws, B, G, Ci, Co, D, H, W, kd, kh, kw, w_batched, FZ_STORE_F32, stream);
}
