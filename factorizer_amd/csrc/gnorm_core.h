// gnorm_core.h — everything of the group norm with a fused activation (csrc/gnorm.hip) that can be wrong
// without a GPU, as __host__ __device__ inline code on top of inorm_core.h (rounding, the tree, the chunk arithmetic):
// which channel an element of a group belongs to, the activation and its gate, the element formulas and the fixed order of the
// per-channel and per-group sums.  tests/emul/emul_gnorm.cpp runs the same code for every "thread" on the host.
//
// A group of a channels-first tensor (B, C, *S) with G groups is cg = C / G adjacent planes of V elements: one contiguous span
// of n = cg V elements.  Statistics are those of the instance norm over the span (sums of d = x − x0 and d² about the group's
// first element, visiting order of inorm_core.h counted from the group's first element).  The affine pair changes every V
// elements, and a 16-byte access straddles two channels (or more, when V < W) whenever V is no multiple of W: γ, β and the
// per-channel totals of the backward belong to ELEMENTS, never to accesses.
#pragma once
#include "inorm_core.h"

namespace fz {

constexpr int GNORM_ACT_NONE = 0, GNORM_ACT_RELU = 1, GNORM_ACT_LEAKY_RELU = 2;
constexpr int GNORM_ONE_PASS_MAX = INORM_ONE_PASS_MAX;   // spans up to here are read once and kept in registers
constexpr int GNORM_CB = 8;                              // channels whose totals one LDS tree of the one-launch backward carries

// chunks of the span n = cg V on the two-launch path (forward partials, both apply launches); the backward partials run over
// planes: inorm_chunks(V) per plane
INORM_HD int gnorm_chunks(int64_t n) { return inorm_chunks(n); }

// ---- which channel of its group an element belongs to ------------------------------------------------------------------
struct GnormChan { int c, r; };   // channel within the group, index within the plane
INORM_HD GnormChan gnorm_chan(int64_t i, int64_t V) {
  GnormChan ch;
  ch.c = (int)((uint32_t)i / (uint32_t)V);   // i < n < 2^31
  ch.r = (int)(i - (int64_t)ch.c * V);
  return ch;
}
INORM_HD void gnorm_next(GnormChan& ch, int V) {
  if (++ch.r == V) {
    ch.r = 0;
    ++ch.c;
  }
}

// ---- activation ----------------------------------------------------------------------------------------------------------
INORM_HD double gnorm_act(double z, int act, double slope) {
  if (act == GNORM_ACT_NONE) return z;
  if (act == GNORM_ACT_RELU) return z <= 0.0 ? 0.0 : z;   // (a NaN passes)
  return z > 0.0 ? z : z * slope;
}
// dact/dz; closed at z == 0 as in the framework; slope is 0 for ReLU
INORM_HD double gnorm_gate(double z, int act, double slope) { return act == GNORM_ACT_NONE || z > 0.0 ? 1.0 : slope; }

INORM_HD double gnorm_y(float x, double mean, double rstd, double gamma, double beta, int act, double slope) {
  return gnorm_act(inorm_y(x, mean, rstd, gamma, beta), act, slope);
}
// g' = g gate(z)
INORM_HD double gnorm_gprime(float g, float x, double mean, double rstd, double gamma, double beta, int act, double slope) {
  return (double)g * gnorm_gate(inorm_y(x, mean, rstd, gamma, beta), act, slope);
}
// sums of g' and g' x̂
INORM_HD void gnorm_acc_grad(double& s1, double& s2, double gp, float x, double mean, double rstd) {
  s1 += gp;
  s2 = __builtin_fma(gp, inorm_xhat(x, mean, rstd), s2);
}
// gx = (g' γ_c − A − x̂ Bq) rstd
INORM_HD double gnorm_gx(double gp, float x, double mean, double rstd, double gamma, double a, double bq) {
  return (gp * gamma - a - inorm_xhat(x, mean, rstd) * bq) * rstd;
}

// a plane's totals from the partials of its chunks, in index order
INORM_HD double gnorm_plane_total(const double* p, int nchunk) {
  double s = 0.0;
  for (int k = 0; k < nchunk; ++k) s += p[2 * k];
  return s;
}

}  // namespace fz
