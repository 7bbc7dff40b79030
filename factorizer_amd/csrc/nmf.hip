// nmf.hip — C-ABI entry points fz_nmf_fwd / fz_nmf_bwd (include/factorizer_hip.h); the
// kernels live in nmf_kernels.inc, one translation unit per rank.
#include "nmf_shapes.h"
#include "nmf_wide.h"   // nmf_grad_steps, entry_fail

namespace fz {
// one row per translation-unit group nmf_r{1..4}<tag>.hip, in the order [bwd][cd/smu][bf16] of the table below
#define FZ_NMF_UNITS(X) \
  X(fwd, ) X(fwd, _bf16) X(fwd, _cdsmu) X(fwd, _bf16_cdsmu) X(bwd, ) X(bwd, _bf16) X(bwd, _cdsmu) X(bwd, _bf16_cdsmu)
#define FZ_NMF_DECLARE(dir, tag)                     \
  int nmf_launch_##dir##_r1##tag(const NmfArgs&);    \
  int nmf_launch_##dir##_r2##tag(const NmfArgs&);    \
  int nmf_launch_##dir##_r3##tag(const NmfArgs&);    \
  int nmf_launch_##dir##_r4##tag(const NmfArgs&);
#define FZ_NMF_ROW(dir, tag) \
  {nmf_launch_##dir##_r1##tag, nmf_launch_##dir##_r2##tag, nmf_launch_##dir##_r3##tag, nmf_launch_##dir##_r4##tag},
FZ_NMF_UNITS(FZ_NMF_DECLARE)
static int (*const kLaunch[8][4])(const NmfArgs&) = {FZ_NMF_UNITS(FZ_NMF_ROW)};
#undef FZ_NMF_ROW
#undef FZ_NMF_DECLARE
#undef FZ_NMF_UNITS

// `fn`: the entry point named in the error message
static int dispatch(const char* fn, bool bwd, int act_dtype, int R, const NmfArgs& a) {
  if (act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16) return entry_fail(FZ_E_ARG, fn, "bad act_dtype");
  const bool cdsmu = a.solver == FZ_SOLVER_CD || a.solver == FZ_SOLVER_SMU;
  return kLaunch[4 * bwd + 2 * cdsmu + (act_dtype == FZ_STORE_BF16)][R - 1](a);
}

// floats of LDS history per matrix in the kernel family that launch_shape (nmf_kernels.inc) takes; -1: no family
static int hist_floats(int M, int N, int R, int G) {
#define FZ_NMF_ROW(MP, NPL, MMAX, NMAX) \
  if (M <= MMAX && N <= NMAX) return (G + 1) * R * NPL * 64 + (G + 1) * MP * R + G * (MP * R + R * R);
  FZ_NMF_SHAPES(FZ_NMF_ROW)
#undef FZ_NMF_ROW
  return -1;
}
}  // namespace fz

static int check_common(int64_t nmat, int M, int N, int R, int T, int solver) {
  if (nmat < 0 || M < 1 || N < 1 || T < 0) return fz::fail(FZ_E_SHAPE, "fz_nmf: bad sizes");
  if (solver != FZ_SOLVER_MU && solver != FZ_SOLVER_HALS && solver != FZ_SOLVER_CD && solver != FZ_SOLVER_SMU)
    return fz::fail(FZ_E_ARG, "fz_nmf: bad solver");
  if (R < 1 || R > 4) return fz::fail(FZ_E_UNSUPPORTED, "fz_nmf: rank outside 1..4");
  if (fz::hist_floats(M, N, R, 0) < 0) return fz::fail(FZ_E_UNSUPPORTED, "fz_nmf: (M,N) outside the native kernel families");
  return FZ_OK;
}

extern "C" int fz_nmf_supported(int M, int N, int R, int T, int Tgrad) {
  if (R < 1 || R > 4 || M < 1 || N < 1 || T < 0) return 0;
  int f = fz::hist_floats(M, N, R, fz::nmf_grad_steps(T, Tgrad));
  return (f > 0 && f * 4 <= 160 * 1024) ? 1 : 0;
}

extern "C" int fz_nmf_fwd(const void* x, const float* u0, const float* v0, void* y, float* u_out,
                          float* v_out, int64_t nmat, int M, int N, int R, int T, int solver, float eps,
                          int act_dtype, fz_stream_t stream) {
  int rc = check_common(nmat, M, N, R, T, solver);
  if (rc != FZ_OK) return rc;
  if (!x || !u0 || !v0 || !y) return fz::fail(FZ_E_ARG, "fz_nmf_fwd: null pointer");
  if (nmat == 0) return FZ_OK;
  fz::NmfArgs a{x, u0, v0, nullptr, nullptr, nullptr, y, u_out, v_out, nullptr, nmat, M, N, T, 0, solver, eps,
                (hipStream_t)stream};
  return fz::dispatch("fz_nmf_fwd", false, act_dtype, R, a);
}

extern "C" int fz_nmf_bwd(const void* x, const float* u0, const float* v0, const void* gy, const float* gu,
                          const float* gv, void* gx, int64_t nmat, int M, int N, int R, int T, int Tgrad,
                          int solver, float eps, int act_dtype, fz_stream_t stream) {
  int rc = check_common(nmat, M, N, R, T, solver);
  if (rc != FZ_OK) return rc;
  if (!x || !u0 || !v0 || !gx || (!gy && !gu && !gv)) return fz::fail(FZ_E_ARG, "fz_nmf_bwd: null pointer");
  if (nmat == 0) return FZ_OK;
  fz::NmfArgs a{x, u0, v0, gy, gu, gv, nullptr, nullptr, nullptr, gx, nmat, M, N, T, fz::nmf_grad_steps(T, Tgrad), solver,
                eps, (hipStream_t)stream};
  return fz::dispatch("fz_nmf_bwd", true, act_dtype, R, a);
}
