// nmf_wide.h — the host path that the two split-N NMF families share (nmf_global.{h,hip}: M <= 64, rank <= 4;
// nmf_global_rank.{h,hip}: 16 <= M <= 512, rank <= 32): one argument struct, one order of argument checks, one workspace
// allocator.  A family is a WideFamily descriptor; its entry points are one line each.  No device code here.
#pragma once
#include "fz_common.h"

namespace fz {

// iterations that carry gradient: Tgrad clamped to 0..T (also the wave-resident entry points, nmf.hip)
inline int nmf_grad_steps(int T, int Tgrad) { return Tgrad < 0 ? 0 : (Tgrad > T ? T : Tgrad); }

// "<entry point>: <what>"
inline int entry_fail(int code, const char* fn, const char* what) { return fail(code, (std::string(fn) + ": " + what).c_str()); }

// workspace offsets in floats, every block padded to 16 bytes; `o` ends as the total
struct WsTake {
  int64_t o = 0;
  int64_t operator()(int64_t n) {
    const int64_t at = o;
    o += (n + 3) / 4 * 4;
    return at;
  }
};

// ---- one call: x, y, gy, gx in the activation storage type, everything else fp32 ----------------------------------------
struct WideArgs {
  const void *x, *gy;
  const float *u0, *v0, *gu, *gv;
  void *y, *gx;
  float *u_out, *v_out;
  int64_t nmat;
  int M;
  int64_t N;
  int R, T, G, solver;
  float eps;
  void* ws;
  fz_stream_t stream;
};

inline WideArgs wide_fwd_args(const void* x, const float* u0, const float* v0, void* y, float* u_out, float* v_out, int64_t nmat,
                              int M, int64_t N, int R, int T, int solver, float eps, void* workspace, fz_stream_t stream) {
  return WideArgs{x, nullptr, u0, v0, nullptr, nullptr, y, nullptr, u_out, v_out, nmat, M, N, R, T, 0, solver, eps, workspace, stream};
}
inline WideArgs wide_bwd_args(const void* x, const float* u0, const float* v0, const void* gy, const float* gu, const float* gv,
                              void* gx, int64_t nmat, int M, int64_t N, int R, int T, int solver, float eps, void* workspace,
                              fz_stream_t stream) {
  return WideArgs{x, gy, u0, v0, gu, gv, nullptr, gx, nullptr, nullptr, nmat, M, N, R, T, 0, solver, eps, workspace, stream};
}

struct WideFamily {
  int (*supported)(int M, int64_t N, int R, int T, int Tgrad);
  bool (*solver_ok)(int solver);
  const char *needs, *bad_solver;           // what the two refusals above say
  int (*run[2][2])(const WideArgs&);        // [backward][bf16]; backward reads a.G >= 1
};

// the checks of both directions, in this order; `fn`: the entry point named in the error message
inline int wide_check(const char* fn, const WideFamily& f, const WideArgs& a, int Tgrad, int act_dtype, bool pointers) {
  if (!f.supported(a.M, a.N, a.R, a.T, Tgrad)) return entry_fail(FZ_E_UNSUPPORTED, fn, f.needs);
  if (!f.solver_ok(a.solver)) return entry_fail(FZ_E_ARG, fn, f.bad_solver);
  if (act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16)
    return entry_fail(FZ_E_ARG, fn, "act_dtype must be FZ_STORE_F32 or FZ_STORE_BF16");
  if (a.nmat < 0 || a.nmat > 65535) return entry_fail(FZ_E_SHAPE, fn, "0 <= nmat <= 65535");
  if (!a.x || !a.u0 || !a.v0 || !a.ws || !pointers) return entry_fail(FZ_E_ARG, fn, "null pointer");
  return FZ_OK;
}

inline int wide_fwd_entry(const char* fn, const WideFamily& f, const WideArgs& a, int act_dtype) {
  const int rc = wide_check(fn, f, a, a.T, act_dtype, a.y != nullptr);
  if (rc != FZ_OK || a.nmat == 0) return rc;
  return f.run[0][act_dtype == FZ_STORE_BF16](a);
}

inline int wide_bwd_entry(const char* fn, const WideFamily& f, WideArgs a, int Tgrad, int act_dtype) {
  const int rc = wide_check(fn, f, a, Tgrad, act_dtype, a.gx && (a.gy || a.gu || a.gv));
  if (rc != FZ_OK) return rc;
  a.G = nmf_grad_steps(a.T, Tgrad);
  if (a.G < 1) return entry_fail(FZ_E_ARG, fn, "no iteration carries gradient (the caller returns zeros)");
  if (a.nmat == 0) return FZ_OK;
  return f.run[1][act_dtype == FZ_STORE_BF16](a);
}

}  // namespace fz
