// emul_inorm.cpp — host run of the instance norm kernels' plan, visiting order, reductions and formulas
// (factorizer_amd/csrc/inorm_core.h, the code csrc/inorm.hip compiles for gfx950), one "thread" after the other.
// Built with g++ and loaded through ctypes by tests/test_instance_norm_cpu.py.  dt: 0 = fp32 storage, 1 = bf16 (uint16 bits).
#include <vector>

#include "../../factorizer_amd/csrc/inorm_core.h"

using namespace fz;

static float ld(const void* p, int dt, int64_t i) {
  return dt ? inorm_bf16_to_f32(((const uint16_t*)p)[i]) : ((const float*)p)[i];
}
static void st(void* p, int dt, int64_t i, double v) {
  if (dt) ((uint16_t*)p)[i] = inorm_round_bf16(v);
  else ((float*)p)[i] = inorm_round_f32(v);
}

static void tree(double* r1, double* r2) {
  for (int w = INORM_THREADS / 2; w > 0; w >>= 1)
    for (int t = 0; t < INORM_THREADS; ++t) {
      inorm_tree_step(r1, t, w);
      inorm_tree_step(r2, t, w);
    }
}

// the two totals of a span as one workgroup forms them: every thread over its groups in order, then the tree
template <class Acc>
static void span_sums(InormSpan sp, int W, Acc acc, double& s1, double& s2) {
  double r1[INORM_THREADS], r2[INORM_THREADS];
  const int64_t ng = inorm_groups(sp, W);
  for (int t = 0; t < INORM_THREADS; ++t) {
    double a = 0.0, b = 0.0;
    for (int64_t j = t; j < ng; j += INORM_THREADS)
      for (int k = 0; k < W; ++k) {
        const int64_t i = sp.lo + j * W + k;
        if (i < sp.hi) acc(a, b, i);
      }
    r1[t] = a;
    r2[t] = b;
  }
  tree(r1, r2);
  s1 = r1[0];
  s2 = r2[0];
}

// the totals of a plane: one span on the one-launch path, else the partials of its chunks re-reduced as the apply launch does
template <class Acc>
static void plane_sums(int64_t V, int W, Acc acc, double& s1, double& s2) {
  if (V <= INORM_ONE_PASS_MAX) {
    InormSpan sp;
    sp.lo = 0;
    sp.hi = V;
    span_sums(sp, W, acc, s1, s2);
    return;
  }
  const int n = inorm_chunks(V);
  std::vector<double> part(2 * (size_t)n);
  for (int c = 0; c < n; ++c) span_sums(inorm_chunk(V, c), W, acc, part[2 * c], part[2 * c + 1]);
  double r1[INORM_THREADS], r2[INORM_THREADS];
  for (int t = 0; t < INORM_THREADS; ++t) {
    r1[t] = inorm_partial_share(part.data(), n, 2, t);
    r2[t] = inorm_partial_share(part.data() + 1, n, 2, t);
  }
  tree(r1, r2);
  s1 = r1[0];
  s2 = r2[0];
}

extern "C" {

int emu_inorm_one_pass_max() { return INORM_ONE_PASS_MAX; }
int emu_inorm_chunks(int64_t V) { return inorm_chunks(V); }
void emu_inorm_chunk(int64_t V, int c, int64_t* lo, int64_t* hi) {
  const InormSpan s = inorm_chunk(V, c);
  *lo = s.lo;
  *hi = s.hi;
}
unsigned emu_inorm_round_bf16(double v) { return inorm_round_bf16(v); }

// marks every element a workgroup's threads visit: count[i] += 1 for the elements of plane length V
void emu_inorm_visits(int64_t V, int W, int* count) {
  const int n = inorm_chunks(V);
  for (int c = 0; c < n; ++c) {
    InormSpan sp = inorm_chunk(V, c);
    if (V <= INORM_ONE_PASS_MAX) { sp.lo = 0; sp.hi = V; }
    const int64_t ng = inorm_groups(sp, W);
    for (int t = 0; t < INORM_THREADS; ++t)
      for (int64_t j = t; j < ng; j += INORM_THREADS)
        for (int k = 0; k < W; ++k)
          if (sp.lo + j * W + k < sp.hi) count[sp.lo + j * W + k] += 1;
  }
}

void emu_inorm_fwd(const void* x, const float* weight, const float* bias, void* y, double* stats, int64_t P, int C, int64_t V,
                   double eps, int dt) {
  const int W = dt ? 8 : 4;
  for (int64_t p = 0; p < P; ++p) {
    const int64_t o = p * V;
    const double x0 = (double)ld(x, dt, o);
    double s1, s2;
    plane_sums(V, W, [&](double& a, double& b, int64_t i) { inorm_acc_stat(a, b, ld(x, dt, o + i), x0); }, s1, s2);
    const InormStat stt = inorm_finish_stat(s1, s2, x0, V, eps);
    stats[2 * p] = stt.mean;
    stats[2 * p + 1] = stt.rstd;
    const double ga = weight ? (double)weight[p % C] : 1.0, be = bias ? (double)bias[p % C] : 0.0;
    for (int64_t i = 0; i < V; ++i) st(y, dt, o + i, inorm_y(ld(x, dt, o + i), stt.mean, stt.rstd, ga, be));
  }
}

void emu_inorm_bwd(const void* x, const void* g, const float* weight, const double* stats, void* gx, float* gweight,
                   float* gbias, int64_t P, int C, int64_t V, int dt) {
  const int W = dt ? 8 : 4;
  std::vector<double> totals(2 * (size_t)P);
  for (int64_t p = 0; p < P; ++p) {
    const int64_t o = p * V;
    const double mean = stats[2 * p], rstd = stats[2 * p + 1];
    double sg, sgx;
    plane_sums(V, W, [&](double& a, double& b, int64_t i) { inorm_acc_grad(a, b, ld(g, dt, o + i), ld(x, dt, o + i), mean, rstd); },
               sg, sgx);
    totals[2 * p] = sg;
    totals[2 * p + 1] = sgx;
    const double ga = weight ? (double)weight[p % C] : 1.0;
    const double a = ga * sg / (double)V, b = ga * sgx / (double)V;
    for (int64_t i = 0; i < V; ++i) st(gx, dt, o + i, inorm_gx(ld(g, dt, o + i), ld(x, dt, o + i), mean, rstd, ga, a, b));
  }
  for (int c = 0; c < C; ++c) {
    if (gbias) gbias[c] = inorm_channel_sum(totals.data(), P / C, C, c, 0);
    if (gweight) gweight[c] = inorm_channel_sum(totals.data(), P / C, C, c, 1);
  }
}

}  // extern "C"
