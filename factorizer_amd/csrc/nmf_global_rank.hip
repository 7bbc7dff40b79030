// nmf_global_rank.hip — split-N NMF for ranks up to 32 and matrices up to 512 rows.
//
// The reference's default-constructed model (Matricize(num_heads=1, grid_size=1), rank=None -> ceil(MN / 10(M+N)),
// HALS, 5 iterations) gives stages such as 64 x 262 144 R 7, 128 x 32 768 R 13, 256 x 4 096 R 25, 512 x 512 R 26.
// nmf_global.hip keeps v[CV][R], a[CV][R], b[R][R] in registers and reduces M·R + R·R partials per wave through LDS:
// neither scales to R = 26, M = 512.  Here the rank is a loop bound over LDS-resident factors, not a register extent:
//
//   gx_prod_kernel   (column slabs x 64-row chunks)  every product that sums over columns: A = X·V and B = VᵀV forward;
//                    X·Ga, Wnewᵀ·G, Woldᵀ·G and gY·V backward.  The operand rows are "stacked" ([X; Vᵀ] etc.): a
//                    128-column tile of them and of the right-hand factor is staged in LDS, a lane owns one ROW and a
//                    wave a fixed quarter of the tile's columns, so a thread sums its (row, 0..R) outputs over the
//                    columns in a fixed order; the four waves are added in a fixed order.  No wave-wide reduction.
//   gx_u_kernel      (1 workgroup / matrix)  sums the slab partials in slab order, u <- update(u; A, B), keeps (A, B)
//                    for the backward and forms UᵀU once for all column slabs.
//   gx_v_kernel      (1 thread / column; below 8192 columns 64 columns / workgroup and a quarter of the rows / wave)
//                    a' = Xᵀu per column (u broadcast from LDS), v <- update(v; a', UᵀU); the last one writes y = u vᵀ.
//
// 3T launches forward.  The update rules and reverse steps are update_rows / half_bwd_row of nmf_core.h restated with
// the row vectors in registers (padded to a multiple of 8, every index a compile-time constant: no private segment)
// and b read from LDS: same order of operations, Gauss-Seidel order, R == 1 shortcut and eps placement.  dL/db, which
// half_bwd_row accumulates per row, is a product over rows here (MU: Woldᵀ·Gdn; HALS: -(Wnewᵀ·Gnum) on and above the
// diagonal, -(Woldᵀ·Gnum) below) and goes through gx_prod_kernel like A and B.  No float atomics; every cross-workgroup
// sum is two-stage in a fixed order, so results replay bit for bit and do not depend on the rest of the batch.
//
// The kernels and launch sequences are in nmf_global_rank.h, templates on the activation storage type; this unit holds the fp32
// instances and the entry points, nmf_global_rank_bf16.hip the bf16 instances.  The argument checks of the entry points are those
// of nmf_wide.h, shared with nmf_global.hip: this family is the descriptor kGx.
#include "nmf_global_rank.h"

using namespace fz;

extern "C" int fz_gnmfx_supported(int M, int64_t N, int R, int T, int Tgrad) {
  (void)Tgrad;
  if (!(M >= kGxMinM && M <= kGxMaxM && R >= 1 && R <= kGxMaxR && R <= M && N >= 1 && T >= 0)) return 0;
  return (R > 4 || M > 64) ? 1 : 0;   // the rest belongs to fz_gnmf_* / fz_nmf_*
}

extern "C" int64_t fz_gnmfx_workspace_bytes(int64_t nmat, int M, int64_t N, int R, int T, int backward) {
  return fz_gnmfx_workspace_bytes_act(nmat, M, N, R, T, backward, FZ_STORE_F32);
}

// a backward on bf16 activations also holds the fp32 running sum of gX (nmat·M·N floats); everything else, and every
// fp32 size, is independent of the storage type
extern "C" int64_t fz_gnmfx_workspace_bytes_act(int64_t nmat, int M, int64_t N, int R, int T, int backward, int act_dtype) {
  if (!fz_gnmfx_supported(M, N, R, T, T) || nmat < 0) return -1;
  if (act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16) return -1;
  return gx_layout(nmat, M, N, R, T, backward != 0, act_dtype == FZ_STORE_BF16).total * (int64_t)sizeof(float);
}

// number of kernel launches of one call (tests assert it against fz_launch_count)
extern "C" int fz_gnmfx_launches(int M, int64_t N, int R, int T, int Tgrad, int backward) {
  (void)M; (void)N; (void)R;
  const int fwd = T == 0 ? 1 : 3 * T;
  return backward ? fwd + 3 * nmf_grad_steps(T, Tgrad) + 1 : fwd;
}

static const WideFamily kGx{fz_gnmfx_supported,
                            [](int solver) { return solver == FZ_SOLVER_MU || solver == FZ_SOLVER_HALS; },
                            "needs 16 <= M <= 512, 1 <= R <= min(32, M), and R > 4 or M > 64",
                            "solver must be MU or HALS",
                            {{gx_run_fwd<float>, gx_fwd_bf16}, {gx_run_bwd<float>, gx_bwd_bf16}}};

extern "C" int fz_gnmfx_fwd_act(const void* x, const float* u0, const float* v0, void* y, float* u_out, float* v_out,
                                int64_t nmat, int M, int64_t N, int R, int T, int solver, float eps, int act_dtype,
                                void* workspace, fz_stream_t stream) {
  return wide_fwd_entry("fz_gnmfx_fwd_act", kGx,
                        wide_fwd_args(x, u0, v0, y, u_out, v_out, nmat, M, N, R, T, solver, eps, workspace, stream), act_dtype);
}

extern "C" int fz_gnmfx_bwd_act(const void* x, const float* u0, const float* v0, const void* gy, const float* gu,
                                const float* gv, void* gx, int64_t nmat, int M, int64_t N, int R, int T, int Tgrad, int solver,
                                float eps, int act_dtype, void* workspace, fz_stream_t stream) {
  return wide_bwd_entry("fz_gnmfx_bwd_act", kGx,
                        wide_bwd_args(x, u0, v0, gy, gu, gv, gx, nmat, M, N, R, T, solver, eps, workspace, stream), Tgrad, act_dtype);
}

extern "C" int fz_gnmfx_fwd(const float* x, const float* u0, const float* v0, float* y, float* u_out, float* v_out,
                            int64_t nmat, int M, int64_t N, int R, int T, int solver, float eps, void* workspace,
                            fz_stream_t stream) {
  return wide_fwd_entry("fz_gnmfx_fwd", kGx,
                        wide_fwd_args(x, u0, v0, y, u_out, v_out, nmat, M, N, R, T, solver, eps, workspace, stream), FZ_STORE_F32);
}

extern "C" int fz_gnmfx_bwd(const float* x, const float* u0, const float* v0, const float* gy, const float* gu,
                            const float* gv, float* gx, int64_t nmat, int M, int64_t N, int R, int T, int Tgrad,
                            int solver, float eps, void* workspace, fz_stream_t stream) {
  return wide_bwd_entry("fz_gnmfx_bwd", kGx,
                        wide_bwd_args(x, u0, v0, gy, gu, gv, gx, nmat, M, N, R, T, solver, eps, workspace, stream), Tgrad, FZ_STORE_F32);
}
