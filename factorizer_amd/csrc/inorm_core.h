// inorm_core.h — everything of the instance norm (csrc/inorm.hip) that can be wrong without a GPU, as
// __host__ __device__ inline code: the chunk plan, which element a thread visits in which order, the fixed-order reduction of
// the partials, and the element formulas.  tests/emul/emul_inorm.cpp runs the same code for every "thread" on the host.
//
// A channels-first tensor (B, C, *S) is P = B·C contiguous planes of V = ∏S elements.  All arithmetic is float64; a stored
// element is rounded exactly once (float64 -> fp32, or float64 -> bf16 without passing through a rounded fp32).
//
// Visiting order.  A plane (or a chunk of it) [lo, hi) is cut into groups of W consecutive elements COUNTED FROM THE PLANE'S
// FIRST ELEMENT (W = 4 fp32, 8 bf16: 16 bytes); thread t of the 256 visits groups t, t + 256, ... and the elements of a group
// in index order, adding each to its own float64 accumulators; the 256 accumulators then meet in a fixed tree.  Nothing in
// the order depends on the address of the plane, so a plane's result has the same bits wherever the plane lies in memory and
// whatever else is in the batch.  A plane that starts on a 16-byte boundary reads and writes a group as one vector access;
// any other plane (odd V, a storage offset) reads and writes the same groups element by element.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define INORM_HD __host__ __device__ __forceinline__
#else
#define INORM_HD inline
#endif

namespace fz {

constexpr int INORM_THREADS = 256;
constexpr int INORM_REG = 32;                                    // elements of a plane one thread keeps in registers
constexpr int INORM_ONE_PASS_MAX = INORM_THREADS * INORM_REG;    // 8192: planes up to here are read once and kept on chip
constexpr int INORM_CHUNK = 16384;                               // elements per workgroup of the two-launch path
constexpr int INORM_MAX_CHUNKS = 256;                            // partials per plane at most: the chunk grows beyond it

// ---- chunk plan: a function of V alone ----------------------------------------------------------------------------------
INORM_HD int64_t inorm_chunk_len(int64_t V) {
  int64_t L = INORM_CHUNK;
  if ((V + L - 1) / L > INORM_MAX_CHUNKS) {
    L = (V + INORM_MAX_CHUNKS - 1) / INORM_MAX_CHUNKS;
    L = (L + INORM_CHUNK - 1) / INORM_CHUNK * INORM_CHUNK;       // chunk starts stay multiples of the group width
  }
  return L;
}
INORM_HD int inorm_chunks(int64_t V) {
  if (V <= INORM_ONE_PASS_MAX) return 1;
  const int64_t L = inorm_chunk_len(V);
  return (int)((V + L - 1) / L);
}
struct InormSpan { int64_t lo, hi; };   // element indices of a plane
INORM_HD InormSpan inorm_chunk(int64_t V, int c) {
  const int64_t L = inorm_chunk_len(V), lo = (int64_t)c * L;
  InormSpan s;
  s.lo = lo < V ? lo : V;
  s.hi = lo + L < V ? lo + L : V;
  return s;
}
// groups of W elements in a span whose lo is a multiple of W; group j starts at lo + W j
INORM_HD int64_t inorm_groups(InormSpan s, int W) { return (s.hi - s.lo + W - 1) / W; }

// ---- accumulators ------------------------------------------------------------------------------------------------------
// forward: sums of d = x - x0 and of d^2, x0 the plane's first element
INORM_HD void inorm_acc_stat(double& s1, double& s2, float x, double x0) {
  const double d = (double)x - x0;
  s1 += d;
  s2 = __builtin_fma(d, d, s2);
}
struct InormStat { double mean, rstd; };
INORM_HD InormStat inorm_finish_stat(double s1, double s2, double x0, int64_t V, double eps) {
  const double m = s1 / (double)V;
  double var = s2 / (double)V - m * m;
  if (!(var > 0.0)) var = 0.0;
  InormStat st;
  st.mean = x0 + m;
  st.rstd = 1.0 / __builtin_sqrt(var + eps);
  return st;
}
INORM_HD double inorm_xhat(float x, double mean, double rstd) { return ((double)x - mean) * rstd; }
INORM_HD double inorm_y(float x, double mean, double rstd, double gamma, double beta) {
  return __builtin_fma(inorm_xhat(x, mean, rstd), gamma, beta);
}
// backward: sums of g and of g x̂ (γ is constant over a plane and multiplies the totals)
INORM_HD void inorm_acc_grad(double& sg, double& sgx, float g, float x, double mean, double rstd) {
  sg += (double)g;
  sgx = __builtin_fma((double)g, inorm_xhat(x, mean, rstd), sgx);
}
INORM_HD double inorm_gx(float g, float x, double mean, double rstd, double gamma, double a, double b) {
  return ((double)g * gamma - a - inorm_xhat(x, mean, rstd) * b) * rstd;
}

// ---- the fixed-order reductions ----------------------------------------------------------------------------------------
// thread t's share of n partials p[0], p[stride], ...: t, t + 256, ... in index order
INORM_HD double inorm_partial_share(const double* p, int n, int stride, int t) {
  double s = 0.0;
  for (int i = t; i < n; i += INORM_THREADS) s += p[(int64_t)i * stride];
  return s;
}
// one step of the tree over red[0 .. 255]: widths 128, 64, ..., 1, every thread, a barrier after each step.  (On the host the
// threads of a step run one after the other: a step reads only slots >= w and writes only slots < w.)
INORM_HD void inorm_tree_step(double* red, int t, int w) {
  if (t < w) red[t] += red[t + w];
}
// sum over the batch index of the plane totals q[(b C + c) 2 + k], b = 0 .. B - 1 in index order, rounded once
INORM_HD float inorm_channel_sum(const double* q, int64_t B, int C, int c, int k) {
  double s = 0.0;
  for (int64_t b = 0; b < B; ++b) s += q[(b * C + c) * 2 + k];
  return (float)s;
}

// ---- the one rounding of a stored element ------------------------------------------------------------------------------
INORM_HD uint32_t inorm_f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
INORM_HD float inorm_u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
INORM_HD float inorm_round_f32(double v) { return (float)v; }
// float64 -> bf16, round to nearest even in ONE rounding: first to fp32 with round-to-odd (truncate towards zero, set the last
// bit if anything was lost — fp32 keeps 16 more bits than bf16, so the sticky bit decides every tie correctly), then to bf16
INORM_HD uint16_t inorm_round_bf16(double v) {
  const float f = (float)v;
  uint32_t u = inorm_f2u(f);
  if (v != v) return (uint16_t)((u >> 16) | 0x40u);
  const double back = (double)f;
  if (back != v) {
    const double av = v < 0.0 ? -v : v, ab = back < 0.0 ? -back : back;
    if (ab > av) u -= 1;   // rounded away from zero: one step back (an infinity becomes the largest finite value)
    u |= 1u;
  }
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
INORM_HD float inorm_bf16_to_f32(uint16_t h) { return inorm_u2f((uint32_t)h << 16); }

}  // namespace fz
