// nmf_global.hip — split-N NMF: matrices too wide for one wavefront.
//
// The reference's DEFAULT FactMixer reshape is the global Matricize(num_heads=1, grid_size=1)
// (factorizer/factorizer.py:17; its own tests run it: tests/test_factorizer.py:25 — x (1,16,64³) →
// ONE 16 x 262 144 matrix), and `num_heads=` forms give M != 8 (tests/test_factorizer.py:123).  The
// wave-resident kernels (nmf_kernels.inc: M <= 32, N <= 512) cannot hold such a matrix, so the columns are
// split over workgroups ("slabs" of 1024 columns) and one iteration of MatrixFactorization.decompose
// (matrix_factorization.py:514-530) becomes
//
//     gn_u_kernel   (1 workgroup / matrix)   a = Σ_slabs partial(X v),  b = Σ_slabs partial(vᵀv)   [fixed order]
//                                            u ← update(u; a, b)                                   (:241-247, :210-229)
//     gn_fwd_kernel (1 workgroup / slab)     v ← update(v; Xᵀu, uᵀu) on its columns (local: a column's
//                                            update needs no other column), then the partial sums of X v and
//                                            vᵀv of the NEW v for the next iteration; the last one writes
//                                            y = u vᵀ (:532-533)
//
// i.e. 2T + 1 launches per forward instead of ~60 framework launches, X read twice per iteration (16 MB for
// the test shape: it lives in the 256 MB Infinity Cache), no float atomics: the cross-workgroup reductions
// are two-stage sums in a fixed order, so results are bitwise reproducible.  The kernel boundary is the
// inter-workgroup synchronisation (1.5-2 us each; a software grid barrier costs 4-10 us on this chip,
// MI355X_MICROARCH.md "barrier-xcd").
//
// Backward: the forward is recomputed with the (u_t, v_t, a_t, b_t) history kept in the workspace (v_t: N·R
// floats per state), then the reverse sweep of SURVEY.md Appendix A runs as the same alternation: the column-
// local parts (V-update undo, gX, gV) in gn_bwd_kernel, the M x R parts (gU, U-update undo) in gn_bwd_u_kernel,
// with `half_bwd_row` of nmf_core.h — the very code the wave kernels run — for the per-row algebra.
//
// The kernels and launch sequences are in nmf_global.h, templates on the activation storage type; this unit holds the fp32
// instances and the entry points, nmf_global_bf16.hip the bf16 instances.  The argument checks of the entry points are those of
// nmf_wide.h, shared with nmf_global_rank.hip: this family is the descriptor kGn.
#include "nmf_global.h"

using namespace fz;

extern "C" int fz_gnmf_supported(int M, int64_t N, int R, int T, int Tgrad) {
  (void)Tgrad;
  return (M >= 1 && M <= kGnMaxM && N >= 1 && R >= 1 && R <= kGnMaxR && T >= 0) ? 1 : 0;
}

extern "C" int64_t fz_gnmf_workspace_bytes(int64_t nmat, int M, int64_t N, int R, int T, int backward) {
  return fz_gnmf_workspace_bytes_act(nmat, M, N, R, T, backward, FZ_STORE_F32);
}

// a backward on bf16 activations also holds the fp32 running sum of gX (nmat·M·N floats); everything else, and every
// fp32 size, is independent of the storage type
extern "C" int64_t fz_gnmf_workspace_bytes_act(int64_t nmat, int M, int64_t N, int R, int T, int backward, int act_dtype) {
  if (!fz_gnmf_supported(M, N, R, T, T) || nmat < 0) return -1;
  if (act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16) return -1;
  return gn_layout(nmat, M, N, R, T, backward != 0, act_dtype == FZ_STORE_BF16).total * (int64_t)sizeof(float);
}

// number of kernel launches of one call (tests assert it against fz_launch_count)
extern "C" int fz_gnmf_launches(int T, int Tgrad, int backward) {
  const int fwd = T == 0 ? 1 : 2 * T + 1;
  return backward ? fwd + 2 * nmf_grad_steps(T, Tgrad) + 1 : fwd;
}

static const WideFamily kGn{fz_gnmf_supported,
                            [](int solver) { return solver >= FZ_SOLVER_MU && solver <= FZ_SOLVER_SMU; },
                            "needs 1 <= M <= 64, 1 <= R <= 4",
                            "bad solver",
                            {{gn_run_fwd<float>, gn_fwd_bf16}, {gn_run_bwd<float>, gn_bwd_bf16}}};

extern "C" int fz_gnmf_fwd_act(const void* x, const float* u0, const float* v0, void* y, float* u_out, float* v_out,
                               int64_t nmat, int M, int64_t N, int R, int T, int solver, float eps, int act_dtype,
                               void* workspace, fz_stream_t stream) {
  return wide_fwd_entry("fz_gnmf_fwd_act", kGn,
                        wide_fwd_args(x, u0, v0, y, u_out, v_out, nmat, M, N, R, T, solver, eps, workspace, stream), act_dtype);
}

extern "C" int fz_gnmf_bwd_act(const void* x, const float* u0, const float* v0, const void* gy, const float* gu,
                               const float* gv, void* gx, int64_t nmat, int M, int64_t N, int R, int T, int Tgrad, int solver,
                               float eps, int act_dtype, void* workspace, fz_stream_t stream) {
  return wide_bwd_entry("fz_gnmf_bwd_act", kGn,
                        wide_bwd_args(x, u0, v0, gy, gu, gv, gx, nmat, M, N, R, T, solver, eps, workspace, stream), Tgrad, act_dtype);
}

extern "C" int fz_gnmf_fwd(const float* x, const float* u0, const float* v0, float* y, float* u_out, float* v_out,
                           int64_t nmat, int M, int64_t N, int R, int T, int solver, float eps, void* workspace,
                           fz_stream_t stream) {
  return wide_fwd_entry("fz_gnmf_fwd", kGn,
                        wide_fwd_args(x, u0, v0, y, u_out, v_out, nmat, M, N, R, T, solver, eps, workspace, stream), FZ_STORE_F32);
}

extern "C" int fz_gnmf_bwd(const float* x, const float* u0, const float* v0, const float* gy, const float* gu,
                           const float* gv, float* gx, int64_t nmat, int M, int64_t N, int R, int T, int Tgrad,
                           int solver, float eps, void* workspace, fz_stream_t stream) {
  return wide_bwd_entry("fz_gnmf_bwd", kGn,
                        wide_bwd_args(x, u0, v0, gy, gu, gv, gx, nmat, M, N, R, T, solver, eps, workspace, stream), Tgrad, FZ_STORE_F32);
}
