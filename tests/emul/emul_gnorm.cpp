// emul_gnorm.cpp — host run of the group norm kernels' plan, visiting order, reductions and formulas
// (factorizer_amd/csrc/gnorm_core.h on inorm_core.h, the code csrc/gnorm.hip compiles for gfx950), one "thread" after the other.
// Built with g++ and loaded through ctypes by tests/test_group_norm_cpu.py.  dt: 0 = fp32 storage, 1 = bf16 (uint16 bits).
#include <vector>

#include "../../factorizer_amd/csrc/gnorm_core.h"

using namespace fz;

static float ld(const void* p, int dt, int64_t i) {
  return dt ? inorm_bf16_to_f32(((const uint16_t*)p)[i]) : ((const float*)p)[i];
}
static void st(void* p, int dt, int64_t i, double v) {
  if (dt) ((uint16_t*)p)[i] = inorm_round_bf16(v);
  else ((float*)p)[i] = inorm_round_f32(v);
}

static void tree(double* r) {
  for (int w = INORM_THREADS / 2; w > 0; w >>= 1)
    for (int t = 0; t < INORM_THREADS; ++t) inorm_tree_step(r, t, w);
}

// the two totals of the elements [sp.lo, sp.hi) that `take` accepts, as one workgroup forms them: every thread over its accesses
// in order, then the tree.  acc(a, b, i) adds element i.
template <class Take, class Acc>
static void span_sums(InormSpan sp, int W, Take take, Acc acc, double& s1, double& s2) {
  double r1[INORM_THREADS], r2[INORM_THREADS];
  const int64_t ng = inorm_groups(sp, W);
  for (int t = 0; t < INORM_THREADS; ++t) {
    double a = 0.0, b = 0.0;
    for (int64_t j = t; j < ng; j += INORM_THREADS)
      for (int k = 0; k < W; ++k) {
        const int64_t i = sp.lo + j * W + k;
        if (i < sp.hi && take(i)) acc(a, b, i);
      }
    r1[t] = a;
    r2[t] = b;
  }
  tree(r1);
  tree(r2);
  s1 = r1[0];
  s2 = r2[0];
}
static bool all(int64_t) { return true; }

extern "C" {

int emu_gnorm_one_pass_max() { return GNORM_ONE_PASS_MAX; }
int emu_gnorm_chunks(int cg, int64_t V) { return gnorm_chunks((int64_t)cg * V); }

void emu_gnorm_fwd(const void* x, const float* weight, const float* bias, void* y, double* stats, int64_t B, int C, int G, int64_t V,
                   double eps, int act, double slope, int dt) {
  const int W = dt ? 8 : 4, cg = C / G;
  const int64_t n = (int64_t)cg * V;
  if (act == GNORM_ACT_RELU) slope = 0.0;
  for (int64_t grp = 0; grp < B * G; ++grp) {
    const int64_t o = grp * n;
    const int c0 = (int)(grp % G) * cg;
    const double x0 = (double)ld(x, dt, o);
    auto acc = [&](double& a, double& b, int64_t i) { inorm_acc_stat(a, b, ld(x, dt, o + i), x0); };
    double s1, s2;
    if (n <= GNORM_ONE_PASS_MAX) {
      InormSpan sp;
      sp.lo = 0;
      sp.hi = n;
      span_sums(sp, W, all, acc, s1, s2);
    } else {
      const int nc = gnorm_chunks(n);
      std::vector<double> part(2 * (size_t)nc);
      for (int c = 0; c < nc; ++c) span_sums(inorm_chunk(n, c), W, all, acc, part[2 * c], part[2 * c + 1]);
      double r1[INORM_THREADS], r2[INORM_THREADS];
      for (int t = 0; t < INORM_THREADS; ++t) {
        r1[t] = inorm_partial_share(part.data(), nc, 2, t);
        r2[t] = inorm_partial_share(part.data() + 1, nc, 2, t);
      }
      tree(r1);
      tree(r2);
      s1 = r1[0];
      s2 = r2[0];
    }
    const InormStat stt = inorm_finish_stat(s1, s2, x0, n, eps);
    stats[2 * grp] = stt.mean;
    stats[2 * grp + 1] = stt.rstd;
    for (int64_t i = 0; i < n; ++i) {
      const int c = c0 + gnorm_chan(i, V).c;
      const double ga = weight ? (double)weight[c] : 1.0, be = bias ? (double)bias[c] : 0.0;
      st(y, dt, o + i, gnorm_y(ld(x, dt, o + i), stt.mean, stt.rstd, ga, be, act, slope));
    }
  }
}

void emu_gnorm_bwd(const void* x, const void* g, const float* weight, const float* bias, const double* stats, void* gx,
                   float* gweight, float* gbias, int64_t B, int C, int G, int64_t V, int act, double slope, int dt) {
  const int W = dt ? 8 : 4, cg = C / G;
  const int64_t n = (int64_t)cg * V;
  if (act == GNORM_ACT_RELU) slope = 0.0;
  std::vector<double> totals(2 * (size_t)(B * C), 0.0);
  for (int64_t grp = 0; grp < B * G; ++grp) {
    const int64_t o = grp * n, plane0 = grp * cg;
    const int c0 = (int)(grp % G) * cg;
    const double mean = stats[2 * grp], rstd = stats[2 * grp + 1];
    auto ga_of = [&](int c) { return weight ? (double)weight[c] : 1.0; };
    auto be_of = [&](int c) { return bias ? (double)bias[c] : 0.0; };
    auto gprime = [&](int64_t i) {   // i: element of the group
      const int c = c0 + gnorm_chan(i, V).c;
      return gnorm_gprime(ld(g, dt, o + i), ld(x, dt, o + i), mean, rstd, ga_of(c), be_of(c), act, slope);
    };
    auto acc = [&](double& a, double& b, int64_t i) { gnorm_acc_grad(a, b, gprime(i), ld(x, dt, o + i), mean, rstd); };
    double A = 0.0, Bq = 0.0;
    if (n <= GNORM_ONE_PASS_MAX) {
      InormSpan sp;
      sp.lo = 0;
      sp.hi = n;
      if (cg == 1 || (!weight && !bias)) {
        double s1, s2;
        span_sums(sp, W, all, acc, s1, s2);
        if (cg == 1) {
          totals[2 * plane0] = s1;
          totals[2 * plane0 + 1] = s2;
        }
        const double ga = cg == 1 ? ga_of(c0) : 1.0;
        A = ga * s1;
        Bq = ga * s2;
      } else {
        for (int j = 0; j < cg; ++j) {   // every thread's share of channel j over the accesses of the GROUP, then the tree
          double t1, t2;
          span_sums(sp, W, [&](int64_t i) { return gnorm_chan(i, V).c == j; }, acc, t1, t2);
          A += ga_of(c0 + j) * t1;
          Bq += ga_of(c0 + j) * t2;
          totals[2 * (plane0 + j)] = t1;
          totals[2 * (plane0 + j) + 1] = t2;
        }
      }
    } else {
      // partials per (plane, chunk of the plane), accesses counted from the PLANE's first element; thread t folds the planes
      // t, t + 256, ... of the group, then the tree
      const int pc = inorm_chunks(V);
      double r1[INORM_THREADS], r2[INORM_THREADS];
      for (int t = 0; t < INORM_THREADS; ++t) r1[t] = r2[t] = 0.0;
      for (int j = 0; j < cg; ++j) {
        std::vector<double> part(2 * (size_t)pc);
        auto pacc = [&](double& a, double& b, int64_t i) { acc(a, b, (int64_t)j * V + i); };
        for (int c = 0; c < pc; ++c) span_sums(inorm_chunk(V, c), W, all, pacc, part[2 * c], part[2 * c + 1]);
        const double t1 = gnorm_plane_total(part.data(), pc), t2 = gnorm_plane_total(part.data() + 1, pc);
        totals[2 * (plane0 + j)] = t1;
        totals[2 * (plane0 + j) + 1] = t2;
        r1[j % INORM_THREADS] += ga_of(c0 + j) * t1;
        r2[j % INORM_THREADS] += ga_of(c0 + j) * t2;
      }
      tree(r1);
      tree(r2);
      A = r1[0];
      Bq = r2[0];
    }
    A /= (double)n;
    Bq /= (double)n;
    for (int64_t i = 0; i < n; ++i) {
      const int c = c0 + gnorm_chan(i, V).c;
      st(gx, dt, o + i, gnorm_gx(gprime(i), ld(x, dt, o + i), mean, rstd, ga_of(c), A, Bq));
    }
  }
  for (int c = 0; c < C; ++c) {
    if (gbias) gbias[c] = inorm_channel_sum(totals.data(), B, C, c, 0);
    if (gweight) gweight[c] = inorm_channel_sum(totals.data(), B, C, c, 1);
  }
}

}  // extern "C"
