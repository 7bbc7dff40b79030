// TEST INFRASTRUCTURE — host lock-step emulation of the per-wave NMF program for the CD and SMU solvers
// (factorizer_amd/csrc/nmf_core.h, SOLVER_CD = 2, SOLVER_SMU = 3).  Reuses the lane-vector policy of emul.cpp and adds the one
// per-lane primitive only these solvers use (the square root of SMU).  Never shipped, never used by the product path; built by
// tests/test_nmf_solvers_cpu.py (and, with asan_solvers_main, under AddressSanitizer + UBSan).
#include <cmath>

#include "emul.cpp"

// found by argument-dependent lookup where nmf_core.h calls fz_sqrt on a lane vector
inline V64 fz_sqrt(const V64& v) { V64 r; for (int i = 0; i < 64; ++i) r.a[i] = std::sqrt(v.a[i]); return r; }

#define DISPATCH_RS(FN, M, NPL, ...)                                           \
  switch (R * 2 + (solver - 2)) {                                              \
    case 2: FN<M, NPL, 1, 2>(__VA_ARGS__); return 0;                           \
    case 3: FN<M, NPL, 1, 3>(__VA_ARGS__); return 0;                           \
    case 4: FN<M, NPL, 2, 2>(__VA_ARGS__); return 0;                           \
    case 5: FN<M, NPL, 2, 3>(__VA_ARGS__); return 0;                           \
    case 6: FN<M, NPL, 3, 2>(__VA_ARGS__); return 0;                           \
    case 7: FN<M, NPL, 3, 3>(__VA_ARGS__); return 0;                           \
    case 8: FN<M, NPL, 4, 2>(__VA_ARGS__); return 0;                           \
    case 9: FN<M, NPL, 4, 3>(__VA_ARGS__); return 0;                           \
    default: return -2;                                                        \
  }

extern "C" int emu_solver_fwd(const float* x, const float* u0, const float* v0, float* y, float* uo, float* vo,
                              int64_t nmat, int M, int N, int R, int T, int solver, float eps) {
  if (solver != 2 && solver != 3) return -3;
  if (M <= 8 && N <= 64) { DISPATCH_RS(run_fwd, 8, 1, x, u0, v0, y, uo, vo, nmat, M, N, T, eps) }
  if (M <= 8 && N <= 128) { DISPATCH_RS(run_fwd, 8, 2, x, u0, v0, y, uo, vo, nmat, M, N, T, eps) }
  if (M <= 8 && N <= 192) { DISPATCH_RS(run_fwd, 8, 3, x, u0, v0, y, uo, vo, nmat, M, N, T, eps) }
  if (M <= 8 && N <= 256) { DISPATCH_RS(run_fwd, 8, 4, x, u0, v0, y, uo, vo, nmat, M, N, T, eps) }
  if (M <= 8 && N <= 512) { DISPATCH_RS(run_fwd, 8, 8, x, u0, v0, y, uo, vo, nmat, M, N, T, eps) }
  if (M <= 16 && N <= 64) { DISPATCH_RS(run_fwd, 16, 1, x, u0, v0, y, uo, vo, nmat, M, N, T, eps) }
  if (M <= 16 && N <= 256) { DISPATCH_RS(run_fwd, 16, 4, x, u0, v0, y, uo, vo, nmat, M, N, T, eps) }
  if (M <= 32 && N <= 64) { DISPATCH_RS(run_fwd, 32, 1, x, u0, v0, y, uo, vo, nmat, M, N, T, eps) }
  if (M <= 32 && N <= 128) { DISPATCH_RS(run_fwd, 32, 2, x, u0, v0, y, uo, vo, nmat, M, N, T, eps) }
  return -2;
}

extern "C" int emu_solver_bwd(const float* x, const float* u0, const float* v0, const float* gy, const float* gu,
                              const float* gv, float* gx, int64_t nmat, int M, int N, int R, int T, int G,
                              int solver, float eps) {
  if (solver != 2 && solver != 3) return -3;
  if (M <= 8 && N <= 64) { DISPATCH_RS(run_bwd, 8, 1, x, u0, v0, gy, gu, gv, gx, nmat, M, N, T, G, eps) }
  if (M <= 8 && N <= 128) { DISPATCH_RS(run_bwd, 8, 2, x, u0, v0, gy, gu, gv, gx, nmat, M, N, T, G, eps) }
  if (M <= 8 && N <= 192) { DISPATCH_RS(run_bwd, 8, 3, x, u0, v0, gy, gu, gv, gx, nmat, M, N, T, G, eps) }
  if (M <= 8 && N <= 256) { DISPATCH_RS(run_bwd, 8, 4, x, u0, v0, gy, gu, gv, gx, nmat, M, N, T, G, eps) }
  if (M <= 8 && N <= 512) { DISPATCH_RS(run_bwd, 8, 8, x, u0, v0, gy, gu, gv, gx, nmat, M, N, T, G, eps) }
  if (M <= 16 && N <= 64) { DISPATCH_RS(run_bwd, 16, 1, x, u0, v0, gy, gu, gv, gx, nmat, M, N, T, G, eps) }
  if (M <= 16 && N <= 256) { DISPATCH_RS(run_bwd, 16, 4, x, u0, v0, gy, gu, gv, gx, nmat, M, N, T, G, eps) }
  if (M <= 32 && N <= 64) { DISPATCH_RS(run_bwd, 32, 1, x, u0, v0, gy, gu, gv, gx, nmat, M, N, T, G, eps) }
  if (M <= 32 && N <= 128) { DISPATCH_RS(run_bwd, 32, 2, x, u0, v0, gy, gu, gv, gx, nmat, M, N, T, G, eps) }
  return -2;
}

#ifdef FZ_EMUL_SOLVERS_MAIN
// the sanitizer run: ragged shapes, ranks 1-4, both solvers, signed input, the decompose-gradient form, an all-zero matrix;
// exact-size buffers, so one element past any of them is a report
#include <cstdio>
#include <random>

int main() {
  std::mt19937 rng(11);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  struct Case { int M, N, R, T, G, solver; };
  const Case cases[] = {{8, 512, 1, 5, 5, 2}, {8, 512, 2, 5, 5, 3}, {8, 150, 2, 10, 10, 2}, {8, 64, 3, 5, 2, 3},
                        {5, 37, 2, 4, 4, 2},  {5, 100, 4, 4, 2, 3}, {8, 200, 1, 3, 1, 3},  {16, 256, 4, 3, 3, 2},
                        {1, 1, 1, 2, 2, 3}};
  int bad = 0;
  for (const Case& c : cases) {
    const int64_t nmat = 3;
    std::vector<float> x(nmat * c.M * c.N), gy(x.size()), y(x.size()), gx(x.size()), u0(c.M * c.R), v0(c.N * c.R),
        uo(nmat * c.M * c.R), vo(nmat * c.N * c.R);
    for (auto& v : x) v = U(rng) - (c.solver == 3 ? 0.5f : 0.f);
    for (auto& v : gy) v = U(rng) - 0.5f;
    for (auto& v : u0) v = U(rng);
    for (auto& v : v0) v = U(rng);
    for (int k = 0; k < c.M * c.N; ++k) x[k] = 0.f;   // an all-zero matrix (eps paths)
    int rc = emu_solver_fwd(x.data(), u0.data(), v0.data(), y.data(), uo.data(), vo.data(), nmat, c.M, c.N, c.R, c.T, c.solver, 1e-16f);
    if (rc != 0) { std::printf("fwd rc %d for %dx%d R%d\n", rc, c.M, c.N, c.R); ++bad; }
    rc = emu_solver_bwd(x.data(), u0.data(), v0.data(), gy.data(), nullptr, nullptr, gx.data(), nmat, c.M, c.N, c.R, c.T, c.G,
                        c.solver, 1e-16f);
    if (rc != 0) { std::printf("bwd rc %d for %dx%d R%d\n", rc, c.M, c.N, c.R); ++bad; }
    rc = emu_solver_bwd(x.data(), u0.data(), v0.data(), nullptr, uo.data(), vo.data(), gx.data(), nmat, c.M, c.N, c.R, c.T, c.G,
                        c.solver, 1e-16f);
    if (rc != 0) { std::printf("bwd(gu, gv) rc %d for %dx%d R%d\n", rc, c.M, c.N, c.R); ++bad; }
  }
  std::printf("asan solvers driver: %d problem(s)\n", bad);
  return bad ? 1 : 0;
}
#endif
