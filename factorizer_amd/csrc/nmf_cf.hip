// nmf_cf.hip — host side of the fused FactMixer core on channels-first tensors (hot shape: head_dim 8, patch 8x8x8): the
// geometry, the predicates and the six launch entry points of include/factorizer_hip.h.  An entry point checks its arguments,
// fills the launchers' argument block and calls one launcher of nmf_cf.h; the kernels are in nmf_cf_fwd.hip, nmf_cf_bwd.hip
// and nmf_cf_gram.hip.  No device code here.
#include "nmf_cf.h"

namespace fz {

static void cf_norm_shift(const int* shift, int D, int H, int W, int (&s)[3]) {
  const int S[3] = {D, H, W};
  for (int i = 0; i < 3; ++i) { s[i] = shift[i] % S[i]; if (s[i] < 0) s[i] += S[i]; }
}

// prev_shift (may be null): the shift of the window that stored the factors a CF_FROM_FACTORS launch reads
static int cf_geom(CfGeom& q, int B, int C, int D, int H, int W, const int* shift, const int* prev_shift, int accumulate,
                   int divisor) {
  if (B < 0 || C < 8 || (C % 8) || D < 8 || H < 8 || W < 8 || (D % 8) || (H % 8) || (W % 8))
    return fail(FZ_E_SHAPE, "fz_nmf_cf: needs C % 8 == 0 and spatial dims multiples of 8");
  if (!shift) return fail(FZ_E_ARG, "fz_nmf_cf: shift is null");
  if ((int64_t)D * H * W >= ((int64_t)1 << 30)) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf: 2^30 or more voxels per channel plane");   // 32-bit lane offsets
  q.B = B; q.C = C; q.D = D; q.H = H; q.W = W; q.h = C / 8; q.G0 = D / 8; q.G1 = H / 8; q.G2 = W / 8;
  int s[3], ps[3] = {0, 0, 0};
  cf_norm_shift(shift, D, H, W, s);
  if (s[2] % 2) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf: W-axis shift must be even");
  if (prev_shift) cf_norm_shift(prev_shift, D, H, W, ps);
  q.s0 = s[0]; q.s1 = s[1]; q.s2 = s[2];
  q.ps0 = ps[0]; q.ps1 = ps[1]; q.ps2 = ps[2];
  q.accumulate = accumulate; q.divisor = divisor; q.gscale_div = 1.0f;
  q.plane = (int64_t)D * H * W;
#ifdef FZ_PROBE_PLANE_PAD   // timing probe (tools/probes/gram_floor.sh): channel planes FZ_PROBE_PLANE_PAD elements further apart
  q.plane += FZ_PROBE_PLANE_PAD;
#endif
  return FZ_OK;
}

// Fills the launchers' argument block.  The order is what a caller sees when more than one argument is wrong: the geometry,
// then `checks(q)` — the entry point's own checks, in its order — then the matrix count.  B == 0 leaves a.nmat == 0: nothing
// to launch.
template <class Checks>
static int cf_prepare(CfLaunch& a, int B, int C, int D, int H, int W, const int* shift, const int* prev_shift, int accumulate,
                      int divisor, fz_stream_t stream, Checks checks) {
  int rc = cf_geom(a.q, B, C, D, H, W, shift, prev_shift, accumulate, divisor);
  if (rc == FZ_OK) rc = checks(a.q);
  if (rc != FZ_OK) return rc;
  a.nmat = (int64_t)B * a.q.h * a.q.G0 * a.q.G1 * a.q.G2;
  if (a.nmat >= (int64_t)1 << 31) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf: more than 2^31 matrices");
  // patch neighbours on the same XCD share its L2 (shifted windows straddle lines): 1.31 -> 1.17 ms
  a.xr = 1 | (tile_order() << 1);
  a.st = (hipStream_t)stream;
  return FZ_OK;
}

// f(AT{}) with AT the storage type that act_dtype names
template <class F>
static int cf_with_dtype(int act_dtype, const char* bad, F f) {
  if (act_dtype == FZ_STORE_F32) return f(float{});
  if (act_dtype == FZ_STORE_BF16) return f(bf16{});
  return fail(FZ_E_ARG, bad);
}

}  // namespace fz

using namespace fz;

extern "C" int fz_nmf_cf_supported(int C, int D, int H, int W, int d, int pd, int ph, int pw, int R, int T, int Tgrad) {
  if (d != 8 || pd != 8 || ph != 8 || pw != 8 || (C % 8) || (D % 8) || (H % 8) || (W % 8)) return 0;
  if (R < 1 || R > 2 || T < 0 || (int64_t)D * H * W >= ((int64_t)1 << 30)) return 0;
  const int G = Tgrad < 0 ? 0 : (Tgrad > T ? T : Tgrad);
  const int per_wave = (R == 1 ? Hist<8, 8, 1>::floats(G) : Hist<8, 8, 2>::floats(G)) * (int)sizeof(float);
  return per_wave <= 160 * 1024 ? 1 : 0;
}

// ---- the plain windows ------------------------------------------------------------------------------------------------
extern "C" int fz_nmf_cf_fwd(const void* t, const float* u0, const float* v0, void* out, int B, int C, int D,
                             int H, int W, const int* shift, int accumulate, int divisor, int R, int T,
                             int solver, float eps, int act_dtype, fz_stream_t stream) {
  return cf_with_dtype(act_dtype, "fz_nmf_cf_fwd: bad act_dtype", [&](auto at) {
    using AT = decltype(at);
    CfLaunch a;
    const int rc = cf_prepare(a, B, C, D, H, W, shift, nullptr, accumulate, divisor, stream, [&](const CfGeom&) {
      if (!t || !u0 || !v0 || !out) return fail(FZ_E_ARG, "fz_nmf_cf_fwd: null pointer");
      if (R < 1 || R > 2) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_fwd: rank 1..2");
      if (solver < FZ_SOLVER_MU || solver > FZ_SOLVER_SMU) return fail(FZ_E_ARG, "fz_nmf_cf_fwd: bad solver");
      return (int)FZ_OK;
    });
    if (rc != FZ_OK || a.nmat == 0) return rc;
    return cf_fwd_launch<AT>((const AT*)t, u0, v0, (AT*)out, nullptr, nullptr, a, CF_PLAIN, R, T, solver, eps);
  });
}

extern "C" int fz_nmf_cf_bwd(const void* t, const float* u0, const float* v0, const void* ga, void* gt, int B,
                             int C, int D, int H, int W, const int* shift, int accumulate, int nshift,
                             int relu_gate, int R, int T, int Tgrad, int solver, float eps, int act_dtype,
                             fz_stream_t stream) {
  return cf_with_dtype(act_dtype, "fz_nmf_cf_bwd: bad act_dtype", [&](auto at) {
    using AT = decltype(at);
    CfLaunch a;
    const int rc = cf_prepare(a, B, C, D, H, W, shift, nullptr, accumulate, 1, stream, [&](const CfGeom&) {
      if (!t || !u0 || !v0 || !ga || !gt) return fail(FZ_E_ARG, "fz_nmf_cf_bwd: null pointer");
      if (R < 1 || R > 2) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_bwd: rank 1..2");
      if (solver < FZ_SOLVER_MU || solver > FZ_SOLVER_SMU) return fail(FZ_E_ARG, "fz_nmf_cf_bwd: bad solver");
      return (int)FZ_OK;
    });
    if (rc != FZ_OK || a.nmat == 0) return rc;
    a.q.gscale_div = (float)(nshift > 1 ? nshift : 1);
    const int G = Tgrad < 0 ? 0 : (Tgrad > T ? T : Tgrad);
    return cf_bwd_launch<AT>((const AT*)t, u0, v0, (const AT*)ga, (AT*)gt, a, relu_gate, R, T, G, solver, eps);
  });
}

// ---- a two-window rank-1 forward that keeps the first window as its factors ------------------------------------------
extern "C" int fz_nmf_cf_factors_supported(int C, int D, int H, int W, int d, int pd, int ph, int pw, int R, int T, int Tgrad,
                                           int nshift, const int* shifts) {
  if (!fz_nmf_cf_supported(C, D, H, W, d, pd, ph, pw, R, T, Tgrad)) return 0;
  if (R != 1 || nshift != 2 || !shifts || (W % 64)) return 0;
  for (int w = 0; w < 2; ++w) {
    int s[3];
    cf_norm_shift(shifts + 3 * w, D, H, W, s);
    if (s[2] % 4) return 0;
  }
  return 1;
}

// form: CF_STORE_FACTORS (out, prev_shift unused) or CF_FROM_FACTORS (prev_shift = the shift of the window that stored the factors)
static int cf_fwd_factors(const void* t, const float* u0, const float* v0, void* out, float* vfac, float* ufac, int B, int C,
                          int D, int H, int W, const int* shift, const int* prev_shift, int form, int divisor, int R, int T,
                          int solver, float eps, int act_dtype, fz_stream_t stream, const char* null_msg, const char* dtype_msg) {
  return cf_with_dtype(act_dtype, dtype_msg, [&](auto at) {
    using AT = decltype(at);
    CfLaunch a;
    const int rc = cf_prepare(a, B, C, D, H, W, shift, prev_shift, form == CF_FROM_FACTORS, divisor, stream, [&](const CfGeom& q) {
      if (!t || !u0 || !v0 || !vfac || !ufac || (form == CF_FROM_FACTORS && (!out || !prev_shift))) return fail(FZ_E_ARG, null_msg);
      if (R != 1) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_fwd factor forms: rank 1 only");
      if (W % 64) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_fwd factor forms: W must be a multiple of 64");
      if (solver < FZ_SOLVER_MU || solver > FZ_SOLVER_SMU) return fail(FZ_E_ARG, "fz_nmf_cf_fwd factor forms: bad solver");
      if (divisor < 1) return fail(FZ_E_ARG, "fz_nmf_cf_fwd factor forms: divisor < 1");
      if ((q.s2 % 4) || (q.ps2 % 4)) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_fwd factor forms: W-axis shift must be a multiple of 4");
      return (int)FZ_OK;
    });
    if (rc != FZ_OK || a.nmat == 0) return rc;
    return cf_fwd_launch<AT>((const AT*)t, u0, v0, (AT*)out, vfac, ufac, a, form, R, T, solver, eps);
  });
}

extern "C" int fz_nmf_cf_fwd_store_factors(const void* t, const float* u0, const float* v0, float* vfac, float* ufac, int B,
                                           int C, int D, int H, int W, const int* shift, int R, int T, int solver, float eps,
                                           int act_dtype, fz_stream_t stream) {
  return cf_fwd_factors(t, u0, v0, nullptr, vfac, ufac, B, C, D, H, W, shift, nullptr, CF_STORE_FACTORS, 1, R, T, solver, eps,
                        act_dtype, stream, "fz_nmf_cf_fwd_store_factors: null pointer (t, u0, v0, vfac or ufac)",
                        "fz_nmf_cf_fwd_store_factors: bad act_dtype");
}

extern "C" int fz_nmf_cf_fwd_from_factors(const void* t, const float* u0, const float* v0, const float* vfac,
                                          const float* ufac, void* out, int B, int C, int D, int H, int W, const int* shift,
                                          const int* prev_shift, int divisor, int R, int T, int solver, float eps, int act_dtype,
                                          fz_stream_t stream) {
  return cf_fwd_factors(t, u0, v0, out, const_cast<float*>(vfac), const_cast<float*>(ufac), B, C, D, H, W, shift, prev_shift,
                        CF_FROM_FACTORS, divisor, R, T, solver, eps, act_dtype, stream,
                        "fz_nmf_cf_fwd_from_factors: null pointer (t, u0, v0, vfac, ufac, out or prev_shift)",
                        "fz_nmf_cf_fwd_from_factors: bad act_dtype");
}

// the tensor of a forward whose two windows BOTH left their factors (two fz_nmf_cf_fwd_store_factors launches): the bits of
// fz_nmf_cf_fwd_store_factors + fz_nmf_cf_fwd_from_factors with divisor 2
extern "C" int fz_nmf_cf_factors_to_tensor(const float* vfac0, const float* ufac0, const float* vfac1, const float* ufac1, void* out,
                                           int B, int C, int D, int H, int W, const int* shift0, const int* shift1, int act_dtype,
                                           fz_stream_t stream) {
  if (act_dtype == FZ_STORE_BF16) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_factors_to_tensor: fp32 storage only");
  if (act_dtype != FZ_STORE_F32) return fail(FZ_E_ARG, "fz_nmf_cf_factors_to_tensor: bad act_dtype");
  CfLaunch a;
  const int rc = cf_prepare(a, B, C, D, H, W, shift0, shift1, 0, 2, stream, [&](const CfGeom& q) {
    if (!vfac0 || !ufac0 || !vfac1 || !ufac1 || !out || !shift1)
      return fail(FZ_E_ARG, "fz_nmf_cf_factors_to_tensor: null pointer (vfac0, ufac0, vfac1, ufac1, out or shift1)");
    if (W % 64) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_factors_to_tensor: W must be a multiple of 64");
    if ((q.s2 % 4) || (q.ps2 % 4)) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_factors_to_tensor: W-axis shift must be a multiple of 4");
    return (int)FZ_OK;
  });
  if (rc != FZ_OK || a.nmat == 0) return rc;
  return cf_factors_to_tensor_launch(vfac0, ufac0, vfac1, ufac1, (float*)out, a);
}

// ---- a two-window HALS rank-1 backward behind the ReLU that keeps the first window's gradient as its factors --------
extern "C" int fz_nmf_cf_bwd_factors_supported(int C, int D, int H, int W, int d, int pd, int ph, int pw, int R, int T, int Tgrad,
                                               int solver, int relu_gate, int nshift, const int* shifts) {
  if (FZ_KNOB("FZ_CF_BWD_FACTORS").set && FZ_KNOB("FZ_CF_BWD_FACTORS").val == 0) return 0;   // probe builds: 0 = the plain launches
  if (!fz_nmf_cf_factors_supported(C, D, H, W, d, pd, ph, pw, R, T, Tgrad, nshift, shifts)) return 0;
  if (solver != FZ_SOLVER_HALS || !relu_gate) return 0;
  if (T < 1 || Tgrad < T) return 0;           // 1 <= G = T: v_start is v0.  G < T: a per-patch vector, the plain launches
  if ((C / 8) * (int64_t)(D / 8) * (H / 8) * (W / 8) >= ((int64_t)1 << 31)) return 0;   // cofac rows of one sample
  const int lds = (CfTile<4>::STAGE_FLOATS + 4 * gram_hist_floats(T - 1) + 4 * 8 * CFG_COFAC) * (int)sizeof(float);
  return lds <= 64 * 1024 ? 1 : 0;
}

static int cf_bwd_factors(const void* t, const float* v0, const void* ga, void* gt, float* gcfac, float* cofac, int B, int C,
                          int D, int H, int W, const int* shift, const int* prev_shift, int form, int nshift, int T, int Tgrad,
                          float eps, int act_dtype, fz_stream_t stream, const char* null_msg, const char* dtype_msg) {
  return cf_with_dtype(act_dtype, dtype_msg, [&](auto at) {
    using AT = decltype(at);
    CfLaunch a;
    int rc = cf_prepare(a, B, C, D, H, W, shift, prev_shift, form == CF_FROM_FACTORS, 1, stream, [&](const CfGeom& q) {
      if (!t || !v0 || !ga || !gcfac || !cofac || (form == CF_FROM_FACTORS && (!gt || !prev_shift))) return fail(FZ_E_ARG, null_msg);
      if (W % 64) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_bwd factor forms: W must be a multiple of 64");
      if (nshift != 2) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_bwd factor forms: exactly two windows");
      if (T < 1 || Tgrad < T) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_bwd factor forms: every iteration graded (1 <= T <= Tgrad)");
      if ((q.s2 % 4) || (q.ps2 % 4)) return fail(FZ_E_UNSUPPORTED, "fz_nmf_cf_bwd factor forms: W-axis shift must be a multiple of 4");
      return (int)FZ_OK;
    });
    if (rc != FZ_OK || a.nmat == 0) return rc;
    a.q.gscale_div = (float)nshift;
    rc = cf_bwd_gram_factors_launch<AT>((const AT*)t, v0, (const AT*)ga, (AT*)gt, gcfac, cofac, a, form, T, T, eps);
    if (rc == FZ_E_UNSUPPORTED) return fail(rc, "fz_nmf_cf_bwd factor forms: history exceeds the LDS budget");
    return rc;
  });
}

extern "C" int fz_nmf_cf_bwd_store_factors(const void* t, const float* v0, const void* ga, float* gcfac, float* cofac, int B,
                                           int C, int D, int H, int W, const int* shift, int nshift, int T, int Tgrad,
                                           float eps, int act_dtype, fz_stream_t stream) {
  return cf_bwd_factors(t, v0, ga, nullptr, gcfac, cofac, B, C, D, H, W, shift, nullptr, CF_STORE_FACTORS, nshift, T, Tgrad, eps,
                        act_dtype, stream, "fz_nmf_cf_bwd_store_factors: null pointer (t, v0, ga, gcfac or cofac)",
                        "fz_nmf_cf_bwd_store_factors: bad act_dtype");
}

extern "C" int fz_nmf_cf_bwd_from_factors(const void* t, const float* v0, const void* ga, const float* gcfac,
                                          const float* cofac, void* gt, int B, int C, int D, int H, int W, const int* shift,
                                          const int* prev_shift, int nshift, int T, int Tgrad, float eps, int act_dtype,
                                          fz_stream_t stream) {
  return cf_bwd_factors(t, v0, ga, gt, const_cast<float*>(gcfac), const_cast<float*>(cofac), B, C, D, H, W, shift, prev_shift,
                        CF_FROM_FACTORS, nshift, T, Tgrad, eps, act_dtype, stream,
                        "fz_nmf_cf_bwd_from_factors: null pointer (t, v0, ga, gcfac, cofac, gt or prev_shift)",
                        "fz_nmf_cf_bwd_from_factors: bad act_dtype");
}
