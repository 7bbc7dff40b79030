/* factorizer_hip.h — C ABI of libfactorizer_hip.so (MI355X / gfx950).
 *
 * The reference (pashtari/factorizer) has no FFI of its own: the boundary its hot path sits
 * behind is the Python nn.Module API.  The entry points below are what the
 * host-side mirrors of those modules (factorizer_amd/*.py) bind through ctypes; each comment
 * names the reference code the entry point replaces (paths relative to the reference root).
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes; pointers are DEVICE pointers unless marked host.
 *   - return 0 on success, <0 on error (FZ_E_*); never throw, never abort.
 *   - never allocate or free caller memory; workspaces are passed in.
 *   - asynchronous on the passed hipStream_t (void*); no host synchronisation inside.
 *   - re-entrant and thread-safe.  Process-wide state is exactly: the launch counter (atomic), the per-stream queues of
 *     deferred finish jobs (mutex-guarded; fz_finish_* below), the FZ_GEMM_BX default read once.  Per-thread state: the last
 *     error string, the `products` default (fz_set_products), the tile order (fz_set_tile_order), the defer flag
 *     (fz_finish_defer).  Nothing else outlives a call.
 *   - tensors are dense, contiguous, row-major ("channels-first": B,C,D,H,W).
 *
 * This header is the only statement of the ABI: factorizer_amd/_header.py reads it and factorizer_amd/_native.py derives the
 * ctypes binding (argument lists, descriptor layouts, constants) from what it reads.  It refuses a declaration that it has no
 * rule for, so declarations keep to these forms: `#define FZ_NAME <integer>` or `(<-integer>)`; `typedef struct fz_x { ... }
 * fz_x;` with fields `T a;`, `T a, b;` or `T a[N];`; `RET fz_name(T a, ...);` with RET one of int, int64_t, const char*.
 * How a type is bound:
 *   int, int64_t, float, double                            the scalar
 *   fz_stream_t                                            an opaque pointer
 *   const char* (return)                                   a C string
 *   pointer to a struct of this header                     pointer to that descriptor
 *   pointer to void or float                               DEVICE buffer: an opaque pointer
 *   pointer to uint8_t, int32_t, uint32_t, int64_t, double DEVICE buffer: an opaque pointer
 *   int*, const int*                                       HOST array of int
 *   pointer to pointer                                     HOST array of opaque pointers / of descriptor pointers
 * A fixed-width element type therefore says "device memory" and plain int says "host memory".  The arguments that do not
 * follow this are listed one by one, each with its reason, in factorizer_amd/_native.py (_ARG_EXCEPTIONS).
 */
#ifndef FACTORIZER_HIP_H
#define FACTORIZER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FZ_OK 0
#define FZ_E_SHAPE (-1)       /* inconsistent / non-divisible shapes            */
#define FZ_E_UNSUPPORTED (-2) /* valid request outside the compiled kernel set  */
#define FZ_E_HIP (-3)         /* a HIP runtime call failed                      */
#define FZ_E_ARG (-4)         /* null pointer / bad enum                        */

/* Storage type of ACTIVATION tensors (inputs, outputs, their gradients, saved pre-activations).
 * FZ_STORE_BF16 is the mixed-precision mode of BASELINE configs[4]: activations live in HBM as bf16,
 * every kernel converts to fp32 on load and rounds to nearest-even on store; parameters, LayerNorm
 * statistics, weight gradients and all arithmetic — MFMA accumulation, the NMF factors / Gram
 * matrices / eps (matrix_factorization.py:200,236) — stay fp32.  Pointers documented as "activation"
 * below are `void*`: float* or (bf16) uint16_t* according to the call's act_dtype. */
#define FZ_STORE_F32 0
#define FZ_STORE_BF16 1

#define FZ_SOLVER_MU 0   /* matrix_factorization.py:232-247 MultiplicativeUpdate        */
#define FZ_SOLVER_HALS 1 /* matrix_factorization.py:194-229 CoordinateDescent + ReLU    */
#define FZ_SOLVER_CD 2   /* matrix_factorization.py:194-229 CoordinateDescent, no projection (X, U, V of any sign) */
#define FZ_SOLVER_SMU 3  /* matrix_factorization.py:319-341 SemiMultiplicativeUpdate (X of any sign) */
/* Every NMF entry point takes one of these four; an older library rejects CD / SMU with FZ_E_ARG ("bad solver"). */

typedef void* fz_stream_t; /* hipStream_t */

/* Library version (major*10000 + minor*100 + patch). */
int fz_version(void);
/* ABI revision: bumped whenever an entry point's signature or a descriptor's layout changes (a caller built against another
 * revision would pass a stream where an int is expected, or leave new trailing descriptor fields uninitialised).  A binding
 * compares fz_abi_version() with the FZ_ABI_VERSION of the header it was written against BEFORE the first call and refuses
 * to run on a mismatch (factorizer_amd/_native.py does).  History: 3 = round 3; 4 = round 4 (`products` / `tune` descriptor
 * fields, `products` argument of fz_conv3_*); 5 = round 5 (the two-window entry points fz_nmf_cf_fwd2 / _bwd2 removed, this
 * function added); 6 = round 6 (fz_finish_defer is per THREAD, one finish queue per stream, fz_finish_flush_all added, fz_gemm_dw_desc.ldw); 7 = block dropout (fz_dropout_* and fz_mlp_drop_supported, fz_mlp_chain_drop added, fz_gemm_dw_desc.drop_m / drop_s appended); entry points added since without touching an existing signature or descriptor (fz_vol_*, fz_vol_respace / fz_vol_unspace, fz_aug_crop_resample / fz_aug_source_words; fz_gcorr_act / fz_gcorr_wgrad_act / fz_gcorr_mu_bwd: the grouped correlations on bf16 storage; fz_dice_bce_ds_* / fz_dice_ce_ds_*: the deep-supervision levels of the loss; fz_gemm_plan: the dry run of fz_gemm's dispatcher; fz_gnmf_fwd_act / _bwd_act / _workspace_bytes_act and fz_gnmfx_fwd_act / _bwd_act / _workspace_bytes_act: the split-N NMF families on bf16 storage) leave it at 7. */
#define FZ_ABI_VERSION 7
int fz_abi_version(void);
/* Walking order of the fused-core launches (fz_nmf_cf_fwd / fz_nmf_cf_bwd) this THREAD issues from now on: 0 = ascending over
 * the patch tiles (the default), 1 = descending; < 0 only queries.  Returns the previous setting.  Results do not depend on it.
 * Why it exists: the windows of one SWMatricize are separate launches that read the SAME tensors; a window that walks them in
 * the direction opposite to the previous window starts at the part the 256 MiB Infinity Cache still holds — measured on
 * fz_nmf_cf_bwd: 3 % less time at the README model's stage 0 (537 MB tensors), 10 % at stage 1 (134 MB),
 * profiles/r05_tile_order.md.  (Reading a tensor backwards right after the launch that WROTE it gains nothing measurable: the
 * whole-step A/B with every streaming kernel alternating was -0.13 ms of 17.4, all of it from the window pairs.) */
int fz_set_tile_order(int descending);
/* Deferred finishes.  Every weight-gradient entry point (fz_wgrad, fz_wgrad_group, fz_gemm_dw, fz_mlp_chain mode 2, fz_ln_bwd with
 * affine gradients, fz_reduce_rows, fz_rowsum, fz_chunk_reduce, fz_upcat_wgrads) ends with a tiny launch that adds per-workgroup
 * partial rows in a fixed order.  Those launches produce PARAMETER gradients — nothing in a backward pass reads them — but each
 * one is a 5-10 us serial slot of the stream (54 per README training step: 0.33 ms).  fz_finish_defer(1) makes the calls that
 * follow ON THIS THREAD queue them instead (the descriptors only; nothing is copied), fz_finish_defer(0) stops queueing; both
 * return the previous setting, fz_finish_defer(-1) only queries.  There is one queue per stream the deferred calls were given
 * (a stream belongs to one device).  fz_finish_flush(stream) runs what is queued for THAT stream, on it, as one or two grids
 * and returns how many jobs that was (0: nothing queued for it; < 0: an error code).  fz_finish_flush_all(waiter) runs every
 * queue on its own stream and makes `waiter` wait (event) for each queue whose stream is another one: the caller that is about
 * to read the gradients on `waiter` is ordered behind all of them; returns the total.  fz_finish_pending() counts queued jobs
 * over all queues.  While finishes are queued the caller keeps alive, and does not touch, every buffer handed to those calls
 * (workspaces, gradient outputs); a call that ACCUMULATES into its output drains its stream's queue and runs at once.  The
 * sums and their order are the same deferred or not: bit-identical.  Reference counterpart: none — autograd launches one
 * reduction kernel per gradient as it goes. */
int fz_finish_defer(int on);
int fz_finish_pending(void);
int fz_finish_flush(fz_stream_t stream);
int fz_finish_flush_all(fz_stream_t waiter);
/* Message for the last error returned on this thread ("" if none). */
const char* fz_last_error_string(void);
/* Number of kernel launches issued through this library by this process (test hook that
 * proves the native path ran). */
int64_t fz_launch_count(void);

/* ---- shifted-window matricize --------------------------------------------------------
 * Replaces SWMatricize.forward = per window torch.roll + einops rearrange, then torch.cat
 * (factorization/operations.py:266-272, 321-325, 417-421).
 *   x: (B, C, D, H, W)   y: (nshift*B*(C/d), G, d, P),  G=(D/pd)(H/ph)(W/pw), P=pd*ph*pw
 *   y[w*B*h + b*h + hh, g, dd, p] = x[b, hh*d+dd, (g_i*p_i + p_i - s_w,i) mod S_i] * (1/div)
 *   shifts: HOST pointer, nshift*3 ints (0 for an unshifted window).
 *   elem_bytes: 4 (fp32) or 2 (16-bit words: moved as opaque bits — bf16 or fp16 alike — unless relu/div
 *               ask for arithmetic, in which case they are taken to be bf16).
 *   relu: if nonzero apply max(.,0) while moving — FactMixer.act, factorizer.py:44.
 *   div: if >1 divide by it — used as the backward of fz_swm_inv.
 */
int fz_swm_fwd(const void* x, void* y, int B, int C, int D, int H, int W, int d, int pd,
               int ph, int pw, int nshift, const int* shifts, int elem_bytes, int relu,
               int div, fz_stream_t stream);

/* Replaces SWMatricize.inverse_forward (operations.py:274-280, 423-434):
 *   x = (((0.0 + z_0) + z_1) + ...) / nshift, z_w = inverse window of chunk w of y (fp32; with
 *   act_dtype FZ_STORE_BF16 the sum and the division are fp32 and the result is rounded once).
 *   average: 1 → divide by nshift (the module's forward); 0 → plain sum (backward of fwd).
 *   gate: optional (may be NULL) tensor shaped like y; when given, element e of y counts
 *         only where gate[e] > 0 (fused ReLU backward for the relu=1 forward).
 */
int fz_swm_inv(const void* y, void* x, int B, int C, int D, int H, int W, int d, int pd,
               int ph, int pw, int nshift, const int* shifts, int average, const void* gate,
               int act_dtype, fz_stream_t stream);

/* ---- batched NMF ---------------------------------------------------------------------
 * Replaces MatrixFactorization.forward = decompose (init → T × [update U, update V]) then
 * reconstruct u @ v.mT (matrix_factorization.py:514-546) for solver "mu" (:241-247) or
 * "hals" (:210-229), RandomInit broadcast buffers u0 (M,R), v0 (N,R) (:52-58).
 *   x, y: (nmat, M, N) activations (act_dtype: fp32, or bf16 storage with the whole factorisation —
 *   u, v, Gram matrices, eps — in fp32);  u_out (nmat,M,R) / v_out (nmat,N,R) fp32, optional (NULL to skip).
 * Supported natively: M <= 32, N <= 64*floor(64/Mpad) (8x512, 16x256, 32x128 families),
 * 1 <= R <= 4; anything else returns FZ_E_UNSUPPORTED (the Python layer then uses its
 * composed path).
 */
int fz_nmf_fwd(const void* x, const float* u0, const float* v0, void* y, float* u_out,
               float* v_out, int64_t nmat, int M, int N, int R, int T, int solver, float eps,
               int act_dtype, fz_stream_t stream);

/* Backward of fz_nmf_fwd w.r.t. x (what autograd does through the unrolled iterations,
 * matrix_factorization.py:522-533; formulas: SURVEY.md Appendix A).  The forward is
 * recomputed inside the kernel; only the last Tgrad iterations carry gradient
 * (num_grad_steps, matrix_factorization.py:476,506-512).
 *   gy: (nmat,M,N) grad of y, may be NULL if gu/gv given;  gu (nmat,M,R), gv (nmat,N,R):
 *   optional grads of the decompose() outputs (NULL to skip);  gx: (nmat,M,N) out.
 */
int fz_nmf_bwd(const void* x, const float* u0, const float* v0, const void* gy,
               const float* gu, const float* gv, void* gx, int64_t nmat, int M, int N, int R,
               int T, int Tgrad, int solver, float eps, int act_dtype, fz_stream_t stream);

/* 1 if (M,N,R,T,Tgrad) is covered by the native kernels (fwd and bwd), else 0. */
int fz_nmf_supported(int M, int N, int R, int T, int Tgrad);

/* ---- split-N NMF: matrices too wide for one wavefront ----------------------------
 * The reference's default FactMixer reshape Matricize(num_heads=1, grid_size=1) (factorizer/factorizer.py:17;
 * tests/test_factorizer.py:25: one 16 x 262 144 matrix) and `num_heads=` forms with M != 8
 * (tests/test_factorizer.py:123).  Same semantics and argument meaning as fz_nmf_fwd / fz_nmf_bwd
 * (matrix_factorization.py:514-546; backward: SURVEY.md Appendix A), fp32, 1 <= M <= 64, any N, 1 <= R <= 4;
 * the columns are split over workgroups, cross-workgroup sums are two-stage and fixed-order (no float atomics:
 * bitwise reproducible).  One call issues fz_gnmf_launches(T, Tgrad, backward) kernels (2T+1 forward).
 * workspace: fz_gnmf_workspace_bytes(nmat, M, N, R, T, backward) bytes of device memory, caller-owned. */
int fz_gnmf_supported(int M, int64_t N, int R, int T, int Tgrad);
int64_t fz_gnmf_workspace_bytes(int64_t nmat, int M, int64_t N, int R, int T, int backward);
int fz_gnmf_launches(int T, int Tgrad, int backward);
int fz_gnmf_fwd(const float* x, const float* u0, const float* v0, float* y, float* u_out, float* v_out,
                int64_t nmat, int M, int64_t N, int R, int T, int solver, float eps, void* workspace,
                fz_stream_t stream);
int fz_gnmf_bwd(const float* x, const float* u0, const float* v0, const float* gy, const float* gu,
                const float* gv, float* gx, int64_t nmat, int M, int64_t N, int R, int T, int Tgrad, int solver,
                float eps, void* workspace, fz_stream_t stream);
/* The same on either activation storage type: x, gy, y, gx are (nmat, M, N) fp32 (FZ_STORE_F32) or bf16 (FZ_STORE_BF16)
 * matrices; any other act_dtype is refused (FZ_E_ARG).  Only storage differs: x and gy become fp32 as they are loaded, each
 * y and gx element is rounded to nearest-even once as it is stored, and u0, v0, u_out, v_out, gu, gv, the factors, Gram
 * matrices and the order of every sum are those of the fp32 call — y and gx are the fp32 call's results on the same values,
 * rounded.  A bf16 matrix needs 2-byte alignment only (wider accesses are used where base and N allow them).
 * fz_gnmf_fwd / fz_gnmf_bwd are these with FZ_STORE_F32; supported shapes, refusals and launch counts do not depend on
 * act_dtype.  workspace: fz_gnmf_workspace_bytes_act(..., act_dtype) bytes; with FZ_STORE_F32 that is
 * fz_gnmf_workspace_bytes(...), and so it is for a bf16 forward; a bf16 BACKWARD adds nmat*M*N floats, the fp32 running
 * sum of gx over the launches that add to it (-1: unsupported shape, nmat < 0 or an act_dtype outside FZ_STORE_*). */
int64_t fz_gnmf_workspace_bytes_act(int64_t nmat, int M, int64_t N, int R, int T, int backward, int act_dtype);
int fz_gnmf_fwd_act(const void* x, const float* u0, const float* v0, void* y, float* u_out, float* v_out,
                    int64_t nmat, int M, int64_t N, int R, int T, int solver, float eps, int act_dtype,
                    void* workspace, fz_stream_t stream);
int fz_gnmf_bwd_act(const void* x, const float* u0, const float* v0, const void* gy, const float* gu, const float* gv,
                    void* gx, int64_t nmat, int M, int64_t N, int R, int T, int Tgrad, int solver, float eps,
                    int act_dtype, void* workspace, fz_stream_t stream);

/* ---- split-N NMF for ranks up to 32 and matrices up to 512 rows (csrc/nmf_global_rank.hip) -------------
 * The reference's default-constructed model: Matricize(num_heads=1, grid_size=1) with rank=None, i.e.
 * rank = ceil(M N / (10 (M + N))) (matrix_factorization.py:406-408), e.g. 64 x 262 144 R 7, 256 x 4 096 R 25,
 * 512 x 512 R 26.  Same semantics and argument lists as fz_gnmf_fwd / fz_gnmf_bwd; fp32; solvers FZ_SOLVER_MU and
 * FZ_SOLVER_HALS only (anything else is refused, FZ_E_ARG).  fz_gnmfx_supported: 16 <= M <= 512, 1 <= R <= min(32, M),
 * N >= 1, T >= 0, and R > 4 or M > 64 (the shapes fz_gnmf_* takes are refused here); nmat <= 65535.  No float atomics,
 * every cross-workgroup sum two-stage in a fixed order: results replay bit for bit and do not depend on the other
 * matrices of the batch.  One call issues fz_gnmfx_launches(M, N, R, T, Tgrad, backward) kernels (3T forward, 1 for
 * T = 0; 3T + 3G + 1 backward).  workspace: fz_gnmfx_workspace_bytes(...) bytes of device memory, caller-owned. */
int fz_gnmfx_supported(int M, int64_t N, int R, int T, int Tgrad);
int64_t fz_gnmfx_workspace_bytes(int64_t nmat, int M, int64_t N, int R, int T, int backward);
int fz_gnmfx_launches(int M, int64_t N, int R, int T, int Tgrad, int backward);
int fz_gnmfx_fwd(const float* x, const float* u0, const float* v0, float* y, float* u_out, float* v_out,
                 int64_t nmat, int M, int64_t N, int R, int T, int solver, float eps, void* workspace,
                 fz_stream_t stream);
int fz_gnmfx_bwd(const float* x, const float* u0, const float* v0, const float* gy, const float* gu,
                 const float* gv, float* gx, int64_t nmat, int M, int64_t N, int R, int T, int Tgrad, int solver,
                 float eps, void* workspace, fz_stream_t stream);
/* The same on either activation storage type, exactly as fz_gnmf_fwd_act / fz_gnmf_bwd_act / fz_gnmf_workspace_bytes_act
 * relate to fz_gnmf_*: fz_gnmfx_fwd / fz_gnmfx_bwd are these with FZ_STORE_F32, and a bf16 backward's workspace holds
 * nmat*M*N more floats. */
int64_t fz_gnmfx_workspace_bytes_act(int64_t nmat, int M, int64_t N, int R, int T, int backward, int act_dtype);
int fz_gnmfx_fwd_act(const void* x, const float* u0, const float* v0, void* y, float* u_out, float* v_out,
                     int64_t nmat, int M, int64_t N, int R, int T, int solver, float eps, int act_dtype,
                     void* workspace, fz_stream_t stream);
int fz_gnmfx_bwd_act(const void* x, const float* u0, const float* v0, const void* gy, const float* gu, const float* gv,
                     void* gx, int64_t nmat, int M, int64_t N, int R, int T, int Tgrad, int solver, float eps,
                     int act_dtype, void* workspace, fz_stream_t stream);

/* ---- FactMixer core on channels-first tensors (hot shape: head_dim 8, patch 8x8x8) -----------
 * One launch per shift window performs SWMatricize.forward → NMF.forward →
 * SWMatricize.inverse_forward (factorizer.py:41-50; operations.py:417-434;
 * matrix_factorization.py:514-546) without materialising the matricized tensors:
 *   fwd: out = ((0 + z_0) + z_1 + ...) / nshift, z_w = scatter_w(NMF(gather_w(t)));
 *        call once per window in order with accumulate = (w > 0), divisor = nshift on the last
 *        window (1 otherwise).
 *   bwd: gt (+)= [t > 0 if relu_gate] * scatter_w(dNMF(gather_w(t); gather_w(ga) / nshift));
 *        call once per window with accumulate = (w > 0).  relu_gate = 1 is the CONTRACT "t = relu(z) >= 0 and gt is the
 *        gradient with respect to z" (factorizer.py:44): for HALS rank 1 the backward then runs in the 8-dimensional row space
 *        (csrc/nmf_gram.h — for a non-negative matrix no ReLU of the iteration ever clips, and v can be eliminated); a t with
 *        negative entries must be passed with relu_gate = 0.
 * t, out, ga, gt: (B, C, D, H, W) activations (act_dtype: fp32, or bf16 storage — the running window sum is
 * then rounded to bf16 between windows, the factorisation itself stays fp32); shift: HOST pointer to 3 ints
 * (W-axis shift even).
 */
int fz_nmf_cf_supported(int C, int D, int H, int W, int d, int pd, int ph, int pw, int R, int T, int Tgrad);
int fz_nmf_cf_fwd(const void* t, const float* u0, const float* v0, void* out, int B, int C, int D,
                  int H, int W, const int* shift, int accumulate, int divisor, int R, int T,
                  int solver, float eps, int act_dtype, fz_stream_t stream);
int fz_nmf_cf_bwd(const void* t, const float* u0, const float* v0, const void* ga, void* gt, int B,
                  int C, int D, int H, int W, const int* shift, int accumulate, int nshift,
                  int relu_gate, int R, int T, int Tgrad, int solver, float eps, int act_dtype,
                  fz_stream_t stream);

/* Rank-1 forward of a TWO-window SWMatricize that hands the first window to the second as its factors, not as u vᵀ.
 * With rank 1 the first window's output is an outer product per 8 x 512 matrix: 520 numbers standing for 4096.
 * fz_nmf_cf_fwd_store_factors runs the first window and writes only
 *   vfac (B, C/8, D, H, W) fp32: v of every voxel, at the voxel's TRUE position (one eighth of t),
 *   ufac (B·C/8·(D/8)·(H/8)·(W/8), 8) fp32: u of every patch, patches in the window's own (shifted) grid order;
 * fz_nmf_cf_fwd_from_factors runs the second (last) window, rebuilds (0 + u v) of the first from the two workspaces
 * (prev_shift = the shift fz_nmf_cf_fwd_store_factors was called with) and writes out = ((0 + z_0) + z_1) / divisor.
 * The pair moves 3.26 tensors where two fz_nmf_cf_fwd calls move 5, and returns the same bits: the product is rounded before
 * the add, and for bf16 storage the first window's value is rounded to bf16 once, as the stored running sum was.
 * fz_nmf_cf_factors_supported (shifts: HOST pointer to nshift·3 ints) is 1 only for rank 1, exactly two windows,
 * W % 64 == 0, both W-axis shifts multiples of 4 and a geometry fz_nmf_cf_supported accepts; the launch functions return
 * FZ_E_UNSUPPORTED / FZ_E_ARG outside it.  Everything else (rank 2, four windows, W < 64, W-axis shifts of 2) calls
 * fz_nmf_cf_fwd once per window.  The backward recomputes from t either way (fz_nmf_cf_bwd, or the pair below). */
int fz_nmf_cf_factors_supported(int C, int D, int H, int W, int d, int pd, int ph, int pw, int R, int T, int Tgrad,
                                int nshift, const int* shifts);
/* a = ((0 + u0 v0^T) + u1 v1^T) / 2 in one pass from the factors that fz_nmf_cf_fwd_store_factors left for window 0
 * (shift0) and for window 1 (shift1): bit for bit the `out` of fz_nmf_cf_fwd_store_factors + fz_nmf_cf_fwd_from_factors with
 * divisor 2.  fp32 storage only (FZ_E_UNSUPPORTED for bf16); same shape conditions as the pair. */
int fz_nmf_cf_factors_to_tensor(const float* vfac0, const float* ufac0, const float* vfac1, const float* ufac1, void* out,
                                int B, int C, int D, int H, int W, const int* shift0, const int* shift1, int act_dtype,
                                fz_stream_t stream);
/* 1 where the out-projection's two launches at C = 32 take a as those factors and a is never stored (fz_mlp_chain_fac,
 * fz_gemm_dw_fac): fz_nmf_cf_factors_supported holds, C == 32, hidden Hd == 64, fp32 storage, split-bf16 products
 * (fz_mlp_pre_supported), no live dropout, exactly two windows. */
int fz_outproj_factors_supported(int C, int Hd, int D, int H, int W, int d, int pd, int ph, int pw, int R, int T, int Tgrad,
                                 int nshift, const int* shifts, int act_dtype, int products, int dropout);
int fz_nmf_cf_fwd_store_factors(const void* t, const float* u0, const float* v0, float* vfac, float* ufac, int B,
                                int C, int D, int H, int W, const int* shift, int R, int T, int solver, float eps,
                                int act_dtype, fz_stream_t stream);
int fz_nmf_cf_fwd_from_factors(const void* t, const float* u0, const float* v0, const float* vfac, const float* ufac,
                               void* out, int B, int C, int D, int H, int W, const int* shift, const int* prev_shift,
                               int divisor, int R, int T, int solver, float eps, int act_dtype, fz_stream_t stream);

/* HALS rank-1 backward behind the ReLU (relu_gate = 1) of a TWO-window SWMatricize that hands the first window's gradient
 * to the second in factored form, not as a tensor.  The row-space reverse mode (csrc/nmf_gram.h) produces a window's
 * dL/dt per 8 x 512 matrix as u_T gcᵀ + gs 1ᵀ + ga1 v0ᵀ + S t: one value gc per voxel and 88 coefficients per patch.
 * fz_nmf_cf_bwd_store_factors runs the first window and writes only
 *   gcfac (B, C/8, D, H, W) fp32: gc of every voxel, at the voxel's TRUE position (one eighth of t),
 *   cofac (B·C/8·(D/8)·(H/8)·(W/8), 88) fp32: u_T[8], gs[8], ga1[8], S[8][8] of every patch, patches in the window's own
 *         (shifted) grid order;
 * fz_nmf_cf_bwd_from_factors runs the second (last) window, rebuilds the first window's gated gradient of every voxel from
 * the two workspaces and the t it holds anyway (prev_shift = the shift fz_nmf_cf_bwd_store_factors was called with) and
 * writes gt = g_0 + g_1 without reading gt.  The pair moves 5.3 tensors where two fz_nmf_cf_bwd calls move 7, and returns
 * the bits of two row-space launches: the same coefficients go through the same expression, and for bf16 storage the first
 * window's value is rounded to bf16 once, as the stored tensor was.  (fz_nmf_cf_bwd itself takes the general kernel for an
 * accumulating fp32 window of 2^15 or more matrices; against that kernel the pair agrees to rounding, not to the bit.)
 * fz_nmf_cf_bwd_factors_supported (shifts: HOST pointer to nshift·3 ints) is 1 only where fz_nmf_cf_factors_supported is
 * (rank 1, exactly two windows, W % 64 == 0, both W-axis shifts multiples of 4) and the solver is FZ_SOLVER_HALS,
 * relu_gate = 1, every iteration is graded (1 <= T <= Tgrad: v_start is then v0) and one sample has fewer than 2^31 patches
 * (the predicate takes no B: the launch functions enforce the total, B·C/8·(D/8)·(H/8)·(W/8) cofac rows < 2^31);
 * the launch functions return FZ_E_UNSUPPORTED / FZ_E_ARG outside what they can see of it (they take no rank, solver or
 * gate: rank 1, HALS, relu_gate = 1 are what they compute).  Everything else calls fz_nmf_cf_bwd once per window. */
int fz_nmf_cf_bwd_factors_supported(int C, int D, int H, int W, int d, int pd, int ph, int pw, int R, int T, int Tgrad,
                                    int solver, int relu_gate, int nshift, const int* shifts);
int fz_nmf_cf_bwd_store_factors(const void* t, const float* v0, const void* ga, float* gcfac, float* cofac, int B, int C,
                                int D, int H, int W, const int* shift, int nshift, int T, int Tgrad, float eps,
                                int act_dtype, fz_stream_t stream);
int fz_nmf_cf_bwd_from_factors(const void* t, const float* v0, const void* ga, const float* gcfac, const float* cofac,
                               void* gt, int B, int C, int D, int H, int W, const int* shift, const int* prev_shift,
                               int nshift, int T, int Tgrad, float eps, int act_dtype, fz_stream_t stream);

/* The same fused core for ANY patch (pd, ph, pw) with head_dim 8 and at most 256 voxels per patch (csrc/nmf_pcf.hip:
 * BASELINE configs[4] uses patch (5,6,5) because 160x192x160 is not divisible by 8; the p = 4 test configurations):
 * same call protocol and semantics as fz_nmf_cf_fwd / fz_nmf_cf_bwd, any shift parity. */
int fz_nmf_pcf_supported(int C, int D, int H, int W, int d, int pd, int ph, int pw, int R, int T, int Tgrad);
int fz_nmf_pcf_fwd(const void* t, const float* u0, const float* v0, void* out, int B, int C, int D, int H, int W,
                   int pd, int ph, int pw, const int* shift, int accumulate, int divisor, int R, int T, int solver,
                   float eps, int act_dtype, fz_stream_t stream);
int fz_nmf_pcf_bwd(const void* t, const float* u0, const float* v0, const void* ga, void* gt, int B, int C, int D,
                   int H, int W, int pd, int ph, int pw, const int* shift, int accumulate, int nshift, int relu_gate,
                   int R, int T, int Tgrad, int solver, float eps, int act_dtype, fz_stream_t stream);
/* Windows w > 0 of the generic-patch backward: accumulate = 1 is a scattered read-modify-write of gt.  Where
 * fz_nmf_pcf_bwd_prefers_separate() returns 1 (129..160 voxels per patch, bf16 storage: measured) it is cheaper to
 * give the window its own buffer (accumulate = 0) and add it with fz_act_add (dst += src, n elements of act_dtype, both
 * 16-byte aligned) — what the reference's modular chain does anyway: every window's inverse_forward term is a tensor of its
 * own before the sum (factorizer/layers/reshape/operations.py:423-434, autograd of it). */
int fz_nmf_pcf_bwd_prefers_separate(int pd, int ph, int pw, int act_dtype);
int fz_act_add(void* dst, const void* src, int64_t n, int act_dtype, fz_stream_t stream);

/* ---- channels-first GEMM family (1x1 layers, k2s2 conv / transposed conv, input grads) ----
 * Out[m, n] = epilogue( sum_k A[m,k] * prologue(In)[k,n] ), n = voxel.  One descriptor drives
 * every dense layer of the block and of the U-shape:
 *   Linear (Conv1d k=1 on flatten(2))      layers/linear.py:53-58
 *   LayerNorm over channels as a prologue  layers/norm.py:29-34
 *   MLP Linear-GELU-Linear                 layers/mlp.py:54-60
 *   adapter on cat([skip, up])             unet.py:128 + factorizer.py:116 (two sources, no cat)
 *   Conv3d(k=2,s=2) downsample             unet.py:53   (loader = FZ_LOAD_S2D)
 *   ConvTranspose3d(k=2,s=2) upsample      unet.py:123  (epilogue = FZ_EPI_D2S)
 *   head Conv3d(k=1)                       unet.py:253
 *   the same layers of a 2-D U-shape: Conv2d(k=2,s=2) (FZ_LOAD_S2D_2D), ConvTranspose2d(k=2,s=2) (FZ_EPI_D2S_2D), the
 *   Conv2d(k=3,p=1) stem (FZ_LOAD_K3_2D)   unet.py:53,123, factorizer.py:145-149, deconver.py Deconver(spatial_dims=2)
 * and, with w_t (use the weight transposed), the input gradient of each of them.
 * The 2-D forms take one source, no prologue / activation and the plain partner (loader or epilogue); Di is ignored.
 * A wrong pairing returns FZ_E_ARG, inconsistent sizes (K, an odd Wo, grid / column counts) FZ_E_SHAPE.
 */
#define FZ_LOAD_PLAIN 0 /* In[k][n] = x[b, k, n]                                             */
#define FZ_LOAD_S2D 1   /* In[(c,td,th,tw)][coarse n] = x[b, c, 2d+td, 2h+th, 2w+tw]         */
#define FZ_LOAD_K3 2    /* In[(c,kd,kh,kw)][n] = x[b, c, d+kd-1, h+kh-1, w+kw-1], zero padded  */
#define FZ_EPI_PLAIN 0  /* y[b, m, n]                                                         */
#define FZ_EPI_D2S 1    /* rows m = (o, td,th,tw): y[b, o, 2d+td, 2h+th, 2w+tw]               */
#define FZ_EPI_LNBWD 2  /* M == 32: result = dL/d(LayerNorm out); y = LayerNorm backward of it  */
#define FZ_LOAD_S2D_2D 3 /* In[(c,th,tw)][coarse n] = x[b, c, 2h+th, 2w+tw]; K = 4*Cin, Ncol = Ho*Wo, even Wo     */
#define FZ_LOAD_K3_2D 4  /* In[(c,kh,kw)][n] = x[b, c, h+kh-1, w+kw-1], zero padded; K = 9*Cin, even Cin, W % 4 == 0 */
#define FZ_EPI_D2S_2D 3  /* rows m = (o, th,tw): y[b, o, 2h+th, 2w+tw]; M = 4*O, bias [M/4], res = fine tensor    */
#define FZ_ACT_NONE 0
#define FZ_ACT_RELU 1
#define FZ_ACT_GELU 2 /* exact erf GELU, layers/mlp.py:56 */

/* How a layer forms its fp32 products: field `products` of fz_gemm_desc / fz_mlp_desc / fz_wgrad_desc and the last int of
 * fz_conv3_fwd / fz_conv3_wgrad_partials.  A descriptor left zero-initialised follows the process default. */
#define FZ_PRODUCTS_DEFAULT 0    /* fz_gemm_bx_enable()'s setting (environment FZ_GEMM_BX read once, else split-bf16) */
#define FZ_PRODUCTS_SPLIT_BF16 1 /* six exact bf16 products per fp32 product on the bf16 matrix cores (csrc/gemm_bx.h)  */
#define FZ_PRODUCTS_FP32_MFMA 2  /* v_mfma_f32_32x32x2_f32 / _16x16x4_f32                                               */

typedef struct fz_gemm_desc {
  const void* x[4];    /* activation: input source tensors (B, C_i, Vin); x[0], and x[1] when nsrc == 2: x[2], x[3] are not read */
  int nsrc;            /* number of sources: 1, or 2 (plain loader without bmul only)          */
  int src_mode;        /* 0: channel concat of x[0] (c0 channels) and x[1] (Cin - c0); anything else: FZ_E_UNSUPPORTED */
  int c0;              /* nsrc == 2: channels of x[0], 0 < c0 < Cin; nsrc == 1: 0 (or Cin)     */
  int Cin;             /* input channels                                                       */
  int64_t Vin;         /* voxels per sample of the input                                       */
  int Di, Hi, Wi;      /* input D, H, W (FZ_LOAD_S2D: fine grid; FZ_LOAD_K3)                   */
  const float* w;      /* weights                                                              */
  int w_t, ldw;        /* A[m][k] = w_t ? w[k*ldw + m] : w[m*ldw + k]                          */
  int M, K;            /* output rows, reduction length (odd: plain loader without ln only)    */
  const float* bias;   /* [M] (plain) / [M/8] (d2s) / [M/4] (2-D d2s) or NULL                  */
  int ln;              /* LayerNorm prologue over Cin                                          */
  const float* ln_g;
  const float* ln_b;
  float ln_eps;
  float* stats_out;    /* (B, 2, Vin): mean, rstd of the LN prologue, or NULL                  */
  int bact;            /* activation applied to the input operand                              */
  const void* bmul;    /* activation: input operand *= act'(bmul) (same shape as the input) or NULL        */
  int bmul_kind;
  int eact;            /* activation applied to the result                                     */
  const void* res;     /* activation: residual added to the result (same shape as y; with FZ_EPI_D2S: the fine-
                          resolution tensor, e.g. the skip-connection gradient) or NULL            */
  const void* emul;    /* activation: result *= act'(emul) (same shape as y) or NULL                       */
  int emul_kind;
  void* y;             /* activation */
  int64_t Ncol;        /* columns per sample: Vin (plain) or coarse voxel count (s2d)          */
  int Ho, Wo;          /* coarse H, W (s2d columns / d2s input grid)                           */
  int B;
  int loader, epilogue;
  /* FZ_EPI_LNBWD (M = 32 with K = 32 or 64; or M = K = 64 with the added gradient): LayerNorm input x (B,M,V),
   * saved stats (B,2,V), gamma (M), gradient added to the result (optional for M = 32), and a partial buffer of
   * fz_gemm_lnbwd_partials(desc) x 2*M floats that receives per-workgroup (dgamma | dbeta) sums (reduce over
   * rows in order). */
  const void* lnb_x;      /* activation */
  const float* lnb_stats;
  const float* lnb_g;
  const void* lnb_gadd;   /* activation */
  float* lnb_part;
  int act_dtype;          /* FZ_STORE_F32 / FZ_STORE_BF16: element type of every "activation" pointer */
  int products;           /* FZ_PRODUCTS_* */
  int tune;               /* 0 = the library chooses the tile.  Timing probes (tools/probes/gemm_bx_bench.py; results do not depend
                             on it): split-bf16 family only — 100 + 10*nacc + mb = streaming form with that tile (nacc 2|4, mb 1|2),
                             200 + 10*nacc + mb = K-split form (nacc 1|2, mb 1|2), 300 = streaming form, library's tile */
} fz_gemm_desc;

/* number of 64-float partial rows fz_gemm writes to lnb_part for this descriptor */
int64_t fz_gemm_lnbwd_partials(const fz_gemm_desc* desc);
/* out[e] = sum over rows of part[row][e], fixed order (rows x n floats); tmp: 64 x n floats of
 * scratch for the two-stage path (rows > 512), may be NULL */
int fz_reduce_rows(const float* part, int64_t rows, int n, float* out, float* tmp, fz_stream_t stream);

int fz_gemm(const fz_gemm_desc* desc, fz_stream_t stream);
/* No field of the descriptor is dropped silently.  Besides the pairings above fz_gemm refuses, before any launch:
 *   FZ_E_ARG          nsrc == 2 with x[1] == NULL; ln without ln_g / ln_b; bact / eact / emul_kind outside FZ_ACT_*
 *   FZ_E_UNSUPPORTED  nsrc == 2 with c0 outside (0, Cin); nsrc == 1 with c0 not in {0, Cin}; eact, emul or ln with FZ_EPI_D2S;
 *                     stats_out without ln; bact with FZ_LOAD_S2D / FZ_LOAD_K3; bmul with ln or bact; bact with FZ_EPI_LNBWD at M = K = 64 (that kernel has no input activation); bact with ln
 *                     (the LayerNorm affine is folded into the staged weights: nothing can act between them); more than one of ln / bact / bmul where the
 *                     layer is not on the register-resident kernel (K <= 32), bact = FZ_ACT_RELU there likewise.
 * Dry run of the dispatcher: the code fz_gemm runs up to, not including, the launch.  Returns what fz_gemm would return for
 * this descriptor (same last-error string) and writes the name of the kernel form it would launch into form[cap]:
 * family, template choices, then the launch geometry as key=value, e.g. "bx_stream mb2 nacc4 plain gelu wt rd1 grid=512x1",
 * "bxk mb1 nacc1 plain rd4 grid=...", "resident ns16 plain pf2 rb=1 grid=...", "stream mb1 nacc2 s2d ks4 grid=...",
 * "p32 pf2 grid=...", "head m4 grid=...", "chain64_lnb split grid=...".  Nothing is dereferenced and nothing is launched: the
 * pointers need only be non-null and aligned as the real ones would be.  (tests/gemm_cases.py maps its cases to forms with it.) */
int fz_gemm_plan(const fz_gemm_desc* desc, char* form, int cap);
/* fz_gemm runs layers with a reduction length >= 64 on the bf16 matrix cores with every fp32 operand split into three
 * bf16 values and six exact products per fp32 product (csrc/gemm_bx.hip: fp32 accuracy at 6/16 of the fp32-MFMA time).
 * on = 0 keeps them on v_mfma_f32_32x32x2_f32, on = 1 enables, on < 0 only queries; returns the previous setting.
 * Default: environment FZ_GEMM_BX (read once), else enabled.  This is only the DEFAULT for descriptors whose `products`
 * field is FZ_PRODUCTS_DEFAULT: a caller that wants two models of one process to differ sets the field. */
int fz_gemm_bx_enable(int on);

/* ---- MLP chain ((C, H) = (32, 64), (32, 128) or (64, 128)): two GEMMs, hidden tensor stays in the accumulators
 * (modes 0 and 1; part rows are 2*C floats: dgamma | dbeta)
 * Replaces per FactorizerBlock (factorizer.py:76, layers/mlp.py:54-63, layers/norm.py:29-34):
 *   mode 0  out = in + W2·gelu(W1·LN(in) + b1) + b2 ; z1 = W1·LN(in) + b1 and stats (mean, rstd)
 *           are written for the backward
 *   mode 1  gz1 = (W2ᵀ·in) ∘ gelu'(z1)  (written for the weight gradients) ;
 *           out = LayerNormBackward(W1ᵀ·gz1; x1, stats, gamma) + in ; part receives
 *           fz_mlp_partials(B, V) rows of 64 floats (dgamma | dbeta partial sums, reduce with
 *           fz_reduce_rows)
 *   mode 2  (C = 32; H = 64 in one launch, H = 128 in one launch per 64-row half of the hidden tensor) mode 1 WITH
 *           the two weight gradients and bias gradients of the MLP, gz1 never reaching
 *           HBM: gw2 (C, H) = sum_v in[.,v] gelu(z1[.,v])^T, gb2 (C) = sum_v in, gb1 (H) = sum_v gz1,
 *           gw1 (H, C) = sum_v gz1 (ln_g * xhat + ln_b)^T.  wpart: fz_mlp_wgrad_workspace_bytes(B, V) bytes of
 *           caller workspace (one row of partial sums per resident workgroup, added in row order).
 */
typedef struct fz_mlp_desc {
  int mode;
  const void* in;     /* activation; mode 0: x1 (B, C, V) ; mode 1: g2 = dL/d(out of the block) (B, C, V)  */
  const float* w1;    /* (H, C)                                                              */
  const float* w2;    /* (C, H)                                                              */
  const float* b1;    /* (H) or NULL, mode 0                                                 */
  const float* b2;    /* (C) or NULL, mode 0                                                 */
  const float* ln_g;  /* (C)                                                                 */
  const float* ln_b;  /* (C), mode 0                                                         */
  float ln_eps;
  float* stats;       /* (B, 2, V): written in mode 0, read in mode 1                        */
  void* z1;           /* activation (B, H, V): written in mode 0, read in mode 1                        */
  void* gz1;          /* activation (B, H, V): written in mode 1                                        */
  const void* x1;     /* activation (B, C, V): the LayerNorm input, mode 1                              */
  void* out;          /* activation (B, C, V)                                                */
  float* part;        /* mode 1: fz_mlp_partials(B, V) x 64 floats                           */
  int B, C, H;
  int64_t V;
  int act_dtype;      /* FZ_STORE_F32 / FZ_STORE_BF16                                        */
  void* wpart;        /* mode 2: workspace, fz_mlp_wgrad_workspace_bytes(B, V)                */
  float* gw1;         /* mode 2: (H, C)                                                      */
  float* gb1;         /* mode 2: (H)                                                         */
  float* gw2;         /* mode 2: (C, H)                                                      */
  float* gb2;         /* mode 2: (C)                                                         */
  float* gln;         /* mode 2: (2*C) dgamma | dbeta of the LayerNorm (part is not used)    */
  float* glp;         /* mode 2, H = 128: (B, C, V) fp32 scratch (the first half's part of W1^T gz1) */
  int products;       /* FZ_PRODUCTS_* */
  /* [r5] mode 0, (C, H) = (32, 64) or (64, 128: an even number of 256-voxel tiles per sample), split-bf16 products
   * (fz_mlp_pre_supported answers for a shape): the block's out-projection in front of the chain,
   * x1 = pre_w . pre_in + pre_b + pre_res (factorizer.py:53,75) formed on the accumulators, written to pre_out and
   * normalised in registers — `in` is ignored, x1 is never read back by another launch (6 instead of 7 tensor passes for
   * steps 3 + 4 of the block at C = 32; at C = 64 the epilogue re-reads the lane's own x1 from L2).  pre_in == NULL: the
   * plain chain on `in`. */
  const void* pre_in;   /* activation (B, C, V): the core's output a, or NULL                 */
  const float* pre_w;   /* (C, C) out_proj weight                                              */
  const float* pre_b;   /* (C) or NULL                                                         */
  const void* pre_res;  /* activation (B, C, V): the block input x                             */
  void* pre_out;        /* activation (B, C, V): x1                                            */
  /* [r5] with pre_in and C = 32: the network's head Linear(C -> post_m <= 4, k1) (unet.py:253,274) applied to `out` while it is in
   * registers — the launch that would read the block output back (fz_head_fwd) disappears.  post_out == NULL: no head. */
  const float* post_w;  /* (post_m, C)                                                         */
  const float* post_b;  /* (post_m) or NULL                                                    */
  void* post_out;       /* activation (B, post_m, V) or NULL                                   */
  int post_m;
} fz_mlp_desc;
/* [ABI 7] block dropout inside the forward chain: fz_mlp_chain_drop(desc, drop, stream) is fz_mlp_chain with the three sites of
 * FactorizerBlock applied in the launch, where fz_mlp_drop_supported(C, H, V, products) — (C, H) = (32, 64), split-bf16
 * products, mode 0 with pre_in:  x1 = x + M0 s0 (pre_w pre_in + pre_b); z1 = W1 LN(x1) + b1 (stored unmasked);
 * out = x1 + M2 s2 (W2 M1 s1 gelu(z1) + b2).  m* = fz_dropout_keep_bits planes ((B, C), (B, H), (B, C) rows of ceil(V / 32)
 * uint32 words) or NULL (no dropout at that site); s* = 1 / (1 - p). */
typedef struct fz_mlp_dropout {
  const uint32_t* m0;   /* site 0: on the out-projection, before + pre_res */
  const uint32_t* m1;   /* site 1: on gelu(z1), before fc2                 */
  const uint32_t* m2;   /* site 2: on fc2's output, before + x1            */
  float s0, s1, s2;
} fz_mlp_dropout;

/* ---- input gradient AND weight gradient of a 32 -> 32 1x1 layer in one pass (in_proj behind LayerNorm, out_proj;
 * factorizer.py:38,53 + norm.py:29-34 as autograd sees them):
 *   y = W^T g                                  (ln: then LayerNormBackward(.; q, stats, ln_g) + gadd; gln receives
 *                                               dgamma | dbeta)
 *   gw (32, 32) = sum_v g[m,v] * in[k,v]       (ln: in = ln_g * xhat(q) + ln_b, the LayerNorm output)
 *   gb (32)     = sum_v g[m,v]                 (optional)
 * wpart: fz_gemm_dw_workspace_bytes(B, V) bytes of caller workspace; rows are added in index order. */
typedef struct fz_gemm_dw_desc {
  const void* g;       /* activation (B, 32, V): gradient of the layer output                 */
  const void* q;       /* activation (B, 32, V): layer input (ln: the LayerNorm input)        */
  const float* w;      /* (32, 32) forward weight                                             */
  int ln;
  const float* stats;  /* ln: (B, 2, V) mean, rstd                                            */
  const float* ln_g;   /* ln: (32)                                                            */
  const float* ln_b;   /* ln: (32)                                                            */
  const void* gadd;    /* ln: activation (B, 32, V) added to y, or NULL                       */
  void* y;             /* activation (B, 32, V)                                               */
  float* gln;          /* ln: (64) dgamma | dbeta                                             */
  void* wpart;
  float* gw;           /* (32, 32), row stride ldgw                                           */
  float* gb;           /* (32) or NULL                                                        */
  int B, C;
  int64_t V;
  int act_dtype;
  int ldgw;            /* floats between rows of gw; 0 = 32 (a column block of a wider weight gradient: its width) */
  int ldw;             /* floats between rows of w;  0 = 32 (a column block of a wider weight, read in place)  [ABI 6] */
  /* [ABI 7] block dropout on g (out_proj under FactorizerBlock site 0; not with ln): the kernel uses drop_s * keep * g for y, gw
   * and gb; drop_m = a fz_dropout_keep_bits plane (B, 32, ceil(V / 32)) or NULL */
  const uint32_t* drop_m;
  float drop_s;
} fz_gemm_dw_desc;
int fz_gemm_dw_rows(int B, int64_t V);
int64_t fz_gemm_dw_workspace_bytes(int B, int64_t V);
int fz_gemm_dw(const fz_gemm_dw_desc* desc, fz_stream_t stream);

/* ---- the out-projection on the core's rank-1 factors (C = 32, where fz_outproj_factors_supported) ----
 * The core's output a is not a tensor but the factors that BOTH windows of the core left (fz_nmf_cf_fwd_store_factors called
 * once per window); the two launches that read a rebuild their operand tiles of it in registers, with the bits of
 * fz_nmf_cf_factors_to_tensor, so every value behind them is the one the stored tensor gives.
 *   fz_mlp_chain_fac: fz_mlp_chain mode 0 with the out-projection in front (pre_w, pre_b, pre_res, pre_out, post_* as with
 *     pre_in; pre_in itself NULL).  Refused with FZ_E_UNSUPPORTED outside (C, H) = (32, 64), mode 0, fp32 storage,
 *     split-bf16 products (fz_mlp_pre_supported); there is no dropout form.
 *   fz_gemm_dw_fac: fz_gemm_dw with q NULL (the layer input is a).  Refused with FZ_E_UNSUPPORTED with ln, drop_m or bf16
 *     storage.
 * Both check the factors against the launch: heads == 4, dims multiples of 8 with W % 64 == 0 and D H W == V, W-axis shifts
 * multiples of 4.  Descriptor layouts and the entry points that take a stored tensor are unchanged (no ABI revision). */
typedef struct fz_outproj_fac {
  const float* v[2];  /* per window: (B, heads, D, H, W) v at the true voxel positions   */
  const float* u[2];  /* per window: (B * heads * D/8 * H/8 * W/8, 8) u per patch         */
  int dims[3];        /* D, H, W                                                          */
  int heads;          /* C / 8 = 4                                                        */
  int shift[6];       /* the two windows' shifts, three ints each                         */
} fz_outproj_fac;
int fz_mlp_chain_fac(const fz_mlp_desc* desc, const fz_outproj_fac* fac, fz_stream_t stream);
int fz_gemm_dw_fac(const fz_gemm_dw_desc* desc, const fz_outproj_fac* fac, fz_stream_t stream);

/* ---- backward of a Linear(32 -> M), M <= 4, in one pass (the network's head: factorizer/unet.py:253) ----
 * gx = W^T gy (activation, (B, 32, V)); weight and bias gradient as fz_head_bwd_rows() partial rows of 132 floats
 * (gW[m][c] at m*32 + c, gb[m] at 128 + m) for fz_chunk_reduce(part, rows, 132, out132, 0, stream). */
int fz_head_bwd_rows(void);
int64_t fz_head_bwd_workspace_bytes(void);
int fz_head_bwd(const void* gy, const void* x, const float* w, void* gx, float* part, int B, int M, int C, int64_t V,
                int act_dtype, fz_stream_t stream);
/* forward of the same layer: y = W x + b (w row-major [M][32], bias [M] or null), (B, 32, V) -> (B, M, V); fz_gemm takes this
 * path by itself for a plain Linear(32 -> M <= 4) without LayerNorm / activation / residual. */
int fz_head_fwd(const void* x, const float* w, const float* bias, void* y, int B, int M, int C, int64_t V, int act_dtype,
                fz_stream_t stream);

/* ---- decoder level forward in one pass ---------------------------------------------------
 * out = adapter(cat([skip, ConvTranspose3d(k2, s2)(deep)], 1))  (factorizer/unet.py:125-127 with the stage adapter of
 * factorizer.py:116) without forming the up-sampled tensor: the caller passes the composed weights
 * wbt[tap][m][k] = sum_c W_b[m][c] W_t[k][c][tap] (tap = kd*4 + kh*2 + kw), the skip half W_a (row stride lda) and
 * bias' = b_ad + W_b b_t (or NULL).  C = 32 skip / output channels, Cd = 64 deep channels, (D, H, W) = coarse extent. */
/* the weight compositions of that node (a few Mflop; device pointers, fp32):
 *   compose: wc[k][m][t] = sum_c w_t[k][c][t] w_b[m][c] (and/or wbt[t][m][k], bias'[m] = b_ad[m] + sum_c w_b[m][c] b_t[c]; outputs may be NULL)
 *   wgrads : from gt[k][m][t] = sum_n deep[k][n] g[m][fine(n,t)]:  gw_t = w_b^T gt,  gw_b = gt . w_t + gb_ad (x) b_t (row stride ldg),
 *            gb_t = w_b^T gb_ad                                                                      */
int fz_upcat_compose(const float* w_t, const float* w_b, int ldb, const float* b_t, const float* b_ad, float* wc, float* wbt, float* bias,
                     int Cd, int O, int M, fz_stream_t stream);
int fz_upcat_wgrads(const float* gt, const float* w_t, const float* w_b, int ldb, const float* gb_ad, const float* b_t, float* gw_t,
                    float* gw_b, int ldg, float* gb_t, int Cd, int O, int M, fz_stream_t stream);
int fz_upcat_supported(int C, int Cd, int D, int H, int W);
int fz_upcat(const void* skip, const void* deep, const float* wa, int lda, const float* wbt, const float* bias, void* out,
             int B, int C, int Cd, int D, int H, int W, int act_dtype, fz_stream_t stream);
/* ---- decoder level backward in one pass over g = dL/d(out) ---------------------------------
 * For the node above with 32 adapter outputs, C1 = 32 skip channels, Cd = 64 deep channels, fine W % 64 == 0 and fp32 storage
 * (fz_upcat_bwd_supported; act_dtype FZ_STORE_BF16 answers 0: that storage keeps the three launches), ONE launch reads g, skip
 * and deep once and forms
 *   g_skip[c][v] = sum_m wa[m][c] g[m][v],   g_deep[k][n] = sum_{m,t} wc[k][m][t] g[m][fine(n,t)]   (wc from fz_upcat_compose)
 * and, through per-workgroup partial rows in `workspace` (fz_upcat_bwd_workspace_bytes) that finish jobs add in index order
 * (deferrable, see fz_finish_defer),
 *   gw_a[m][c] = sum_v g[m][v] skip[c][v] (row stride ldg),  gb[m] = sum_v g[m][v],  gt[k][m][t] = sum_n deep[k][n] g[m][fine(n,t)]
 * — the inputs of fz_upcat_wgrads.  g, skip, g_skip 8-byte aligned; deep, g_deep, workspace 16-byte aligned.
 * (D, H, W) = coarse extent.  Outside the predicate: FZ_E_UNSUPPORTED; null pointer: FZ_E_ARG; B < 1: FZ_E_SHAPE. */
int fz_upcat_bwd_supported(int C1, int Cd, int D, int H, int W, int act_dtype);
int64_t fz_upcat_bwd_workspace_bytes(int B, int D, int H, int W);
int fz_upcat_bwd(const void* g, const void* skip, const void* deep, const float* wa, int lda, const float* wc, void* g_skip,
                 void* g_deep, void* workspace, float* gw_a, int ldg, float* gb, float* gt, int B, int C1, int Cd, int D, int H,
                 int W, int act_dtype, fz_stream_t stream);
/* [r5] The first layer of the FactorizerBlock that CONSUMES a 32-channel tensor, t = relu(in_proj(LayerNorm1(x)))
 * (factorizer.py:38,44,75; norm.py:29-34; in_proj has no bias), applied by the launch that PRODUCES x while the tile is in
 * registers: the launch that would read x back disappears (x itself is still written: the block's backward and its residual
 * read it).  t: activation (B, 32, V) of the launch's storage type; stats: (B, 2, V) fp32 mean | rstd of every voxel, as
 * fz_gemm's stats_out.  Producers that take it: fz_upcat2 (a decoder level's output), fz_conv3_fwd2 (the stem). */
typedef struct fz_block_prologue {
  const float* ln_g;  /* (32) */
  const float* ln_b;  /* (32) */
  float ln_eps;
  const float* w;     /* (32, 32) in_proj weight */
  void* t;
  float* stats;
} fz_block_prologue;
int fz_upcat2(const void* skip, const void* deep, const float* wa, int lda, const float* wbt, const float* bias, void* out,
              int B, int C, int Cd, int D, int H, int W, int act_dtype, const fz_block_prologue* pro, fz_stream_t stream);

int fz_mlp_supported(int C, int H, int64_t V);
int fz_mlp_pre_supported(int C, int H, int64_t V, int products);
int fz_mlp_drop_supported(int C, int H, int64_t V, int products);   /* [ABI 7] 1: fz_mlp_chain_drop takes this shape */
int64_t fz_mlp_partials(int B, int64_t V);
int fz_mlp_wgrad_rows(int B, int64_t V);
int64_t fz_mlp_wgrad_workspace_bytes(int B, int64_t V);
int fz_mlp_chain(const fz_mlp_desc* desc, fz_stream_t stream);
int fz_mlp_chain_drop(const fz_mlp_desc* desc, const fz_mlp_dropout* drop, fz_stream_t stream);   /* [ABI 7] */

/* ---- weight gradients of the GEMM family ------------------------------------------------
 * GW[m,k] = sum_{b,n} P[b,m,n] * Q(In)[b,k,n] — what autograd computes for the weights of
 * Conv1d(k=1) (layers/linear.py:44-58), Conv3d k2s2 / ConvTranspose3d k2s2 (unet.py:53,123)
 * and the k3 stem (factorizer.py:145-149).  Deterministic two-stage reduction; the caller
 * passes a workspace of fz_wgrad_workspace_bytes().
 */
#define FZ_QL_PLAIN 0 /* Q[k][n] = in[b,k,n]                                     */
#define FZ_QL_S2D 1   /* Q[(c,td,th,tw)][coarse n] = in[b,c,2d+td,2h+th,2w+tw]   */
#define FZ_QL_K3 2    /* Q[(c,kd,kh,kw)][n] = in[b,c,d+kd-1,h+kh-1,w+kw-1] (zero pad) */
#define FZ_QL_S2D_2D 3 /* Q[(c,th,tw)][coarse n] = in[b,c,2h+th,2w+tw]: K = 4*Cin, N = Ho*Wo, even Wo */
#define FZ_QL_K3_2D 4  /* Q[(c,kh,kw)][n] = in[b,c,h+kh-1,w+kw-1] (zero pad): K = 9*Cin, N = H*W    */

typedef struct fz_wgrad_desc {
  const void* p;      /* activation (B, M, N) output-side gradient                                    */
  int M;
  const void* pmul;   /* activation, optional: P *= act'(pmul)                                      */
  int pmul_kind;      /* FZ_ACT_RELU / FZ_ACT_GELU                                           */
  const void* q[4];   /* activation: input sources; q[0] and, with nsrc == 2, q[1] are read                */
  int nsrc, src_mode, c0; /* nsrc 1 or 2; src_mode 0; nsrc == 1: c0 = 0; nsrc == 2: channel concat, q[0] holds channels [0, c0),
                           * 0 < c0 < Cin.  The s2d / k3 loaders take nsrc == 1 and neither stats nor qact.  Outside that:
                           * FZ_E_UNSUPPORTED (the 2-D loaders with a second source, stats or qact, and a null q[1]: FZ_E_ARG). */
  int Cin;            /* input channels                                                      */
  int K;              /* Q rows: Cin / 8*Cin / 27*Cin (2-D: 4*Cin / 9*Cin)                   */
  int64_t Vq;         /* voxels per sample of the input                                      */
  int D, H, W;        /* input grid (s2d: fine grid; k3)                                     */
  int64_t N;          /* reduction columns per sample                                        */
  int Ho, Wo;         /* coarse grid (s2d)                                                   */
  const float* stats; /* (B,2,Vq) mean/rstd: Q = (in-mean)*rstd, or NULL                     */
  int qact;           /* activation applied to Q                                             */
  const float* ln_g;  /* with stats: gw[m][k] = ln_g[k]*acc + ln_b[k]*rowsum(P)[m]           */
  const float* ln_b;
  float* gw;          /* (M, K) out                                                          */
  float* gbias;       /* (M) row sums of P, or NULL                                          */
  int accumulate;     /* add into gw/gbias instead of overwriting                            */
  int B;
  int loader;
  int act_dtype;      /* FZ_STORE_F32 / FZ_STORE_BF16; with bf16 the products run on bf16 MFMAs (fp32 accumulation) */
  int products;       /* FZ_PRODUCTS_* (fp32 activations) */
} fz_wgrad_desc;

int64_t fz_wgrad_workspace_bytes(const fz_wgrad_desc* desc);
int fz_wgrad(const fz_wgrad_desc* desc, void* workspace, fz_stream_t stream);
/* Up to 4 weight-gradient problems in ONE partial-sum grid (same results as n fz_wgrad calls, bit for bit): the four dense
 * layers of a FactorizerBlock at C >= 64 — fc2, fc1 behind LayerNorm (mlp.py:54-63), out_proj, in_proj behind LayerNorm
 * (factorizer.py:38,53) — whose single launches each leave half of every CU's workgroup slots empty.  Problems that do not
 * take the 64 x 64 register-operand kernel are launched one by one, in order.  workspaces[i] >= fz_wgrad_workspace_bytes(descs[i]). */
int fz_wgrad_group(const fz_wgrad_desc* const* descs, void* const* workspaces, int n, fz_stream_t stream);

/* ---- channels-first LayerNorm (layers/norm.py:29-34), standalone ---------------------------
 * fwd: y = (x-mean)*rstd*gamma + beta over C per voxel; stats (B,2,V) = (mean, rstd) optional.
 * bwd: gx = rstd*(gl*gamma - mean_c(gl*gamma) - n*mean_c(gl*gamma*n)) [+ gadd]; the parameter
 * gradients come from the same pass (C <= 64) or from fz_wgrad (diag of P=gl, Q=normalised x).
 */
int fz_ln_fwd(const void* x /* activation */, const float* gamma, const float* beta, void* y /* activation */,
              float* stats, int B, int C, int64_t V, float eps, int act_dtype, fz_stream_t stream);
/* gparams (optional): [gamma grad (C) | beta grad (C)] computed in the same pass; needs a
 * workspace of fz_ln_bwd_workspace_bytes2(B, C, V). */
int64_t fz_ln_bwd_workspace_bytes(int C);                        /* C <= 64 */
int64_t fz_ln_bwd_workspace_bytes2(int B, int C, int64_t V);     /* any C   */
int fz_ln_bwd(const void* gl, const void* x, const float* stats, const float* gamma,
              const void* gadd, void* gx /* gl, x, gadd, gx: activations */, float* gparams, void* workspace,
              int B, int C, int64_t V, int act_dtype, fz_stream_t stream);

/* ---- stem: Conv3d(kernel 3, padding 1) (factorizer/factorizer.py:145-149 → unet.py:231,261) ----
 * fwd: y = conv3d(x, w) [+ bias]; needs even C_in, W % 4 == 0.
 * wgrad: per-workgroup partial sums part[nchunk][M][27*C_in], part_bias[nchunk][M]
 * (nchunk = fz_conv3_wgrad_chunks), reduced in a fixed order by fz_chunk_reduce; needs
 * W % 32 == 0 and 27*C_in <= 128. */
int fz_conv3_fwd(const void* x /* activation */, const float* w, const float* bias, void* y /* activation */,
                 int B, int Cin, int M, int D, int H, int W, int act_dtype, int products, fz_stream_t stream);
/* [r5] the same with the consuming block's first layer applied to the output tile (fz_block_prologue, below): C_in = 4,
 * M = 32, split-bf16 products (fz_conv3_prologue_supported); pro == NULL: fz_conv3_fwd. */
struct fz_block_prologue;
int fz_conv3_prologue_supported(int Cin, int M, int W, int products);
int fz_conv3_fwd2(const void* x, const float* w, const float* bias, void* y, int B, int Cin, int M, int D, int H, int W,
                  int act_dtype, int products, const struct fz_block_prologue* pro, fz_stream_t stream);
int fz_conv3_wgrad_chunks(int B, int D, int H, int W);
int fz_conv3_wgrad_partials(const void* gy, const void* x /* activations */, float* part, float* part_bias, int B,
                            int Cin, int M, int D, int H, int W, int act_dtype, int products, fz_stream_t stream);
int fz_chunk_reduce(const float* part, int nchunk, int64_t n, float* out, int accumulate, fz_stream_t stream);
/* the same over rows `ld` floats apart (ld >= n): a column block of wider partial rows (the head's 132-float rows: weight block
 * and bias block into their own gradient tensors) */
int fz_chunk_reduce_ld(const float* part, int nchunk, int64_t n, int64_t ld, float* out, int accumulate, fz_stream_t stream);

/* out[c] = sum over batch and voxels of x[b,c,v] (bias gradient of ConvTranspose3d, unet.py:123);
 * part: workspace of B * fz_rowsum_chunks(V) * C floats. */
int fz_rowsum_chunks(int64_t V);
int fz_rowsum(const void* x /* activation */, float* part, float* out, int B, int C, int64_t V, int act_dtype,
              fz_stream_t stream);

/* ---- grouped "same" cross-correlation of the Deconver family ----------------------------
 * The one operator of the reference's blind-deconvolution updates (factorizer/factorization/deconvolution.py:
 * 21-40 `conv`, 136-156 `update_s`): out[b, g*Co+o, v] = sum_i sum_t in[b, g*Ci+i, v+t-p] * w[b or 0, g, o, i, t],
 * zero padding p = k/2 — used as H, as H^T (channel-transposed, flipped filters) and for input gradients.
 *   in (B, G*Ci, D, H, W); w (Bw, G, Co, Ci, kd, kh, kw), Bw = B if w_batched else 1; out (B, G*Co, D, H, W); fp32.
 *   mul_a, mul_b: both NULL -> out = corr + add_eps; both given (shape of out) -> the fused multiplicative update
 *   out = mul_a * mul_b / (corr + add_eps)  (s * (H^T x + eps) / (H^T H s + eps)).
 * Supported: any odd kernel extent <= 7 per axis (2-D layers as D = 1, kd = 1) and any channel counts.  Compile-time
 * instantiations serve Co <= 16 per group with cubic / depth-1 square 3-5-7 kernels (the reference's defaults); everything else —
 * anisotropic kernels such as (5, 3, 3) of the reference's tests/test_deconver.py, more channels per group — runs the run-time-extent
 * kernels (eight output channels per workgroup) [r6]. */
int fz_gcorr_supported(int Ci, int Co, int kd, int kh, int kw);
int fz_gcorr(const float* in, const float* w, float* out, const float* mul_a, const float* mul_b, int B, int G,
             int Ci, int Co, int D, int H, int W, int kd, int kh, int kw, int w_batched, float add_eps,
             fz_stream_t stream);
/* Filter gradient of fz_gcorr (what autograd derives through F.conv{2,3}d in the reference, deconvolution.py:21-40):
 * gw[bw, g, o, i, t] = sum_b sum_v gout[b, g*Co+o, v] * in[b, g*Ci+i, v+t-p]  (b = bw for per-sample filters).
 * Deterministic two-stage reduction; ws: fz_gcorr_wgrad_workspace_bytes(...) bytes of caller workspace. */
int64_t fz_gcorr_wgrad_workspace_bytes(int B, int G, int Ci, int Co, int D, int H, int W, int kd, int kh, int kw);
int fz_gcorr_wgrad(const float* in, const float* gout, float* gw, void* ws, int B, int G, int Ci, int Co, int D, int H,
                   int W, int kd, int kh, int kw, int w_batched, fz_stream_t stream);
/* The same operators on either activation storage type (act_dtype FZ_STORE_F32 / FZ_STORE_BF16; anything else is
 * FZ_E_UNSUPPORTED): in, out, mul_a, mul_b and gout are activations (float* or bf16 by act_dtype, all of one type); the
 * filters w, the filter gradient gw and the workspace are always fp32.  bf16 values are converted to fp32 as the tile is
 * staged, every product and accumulator is fp32 (the fused update is computed in fp32 as well), and each stored element is
 * rounded to nearest-even once.  fz_gcorr / fz_gcorr_wgrad are these with FZ_STORE_F32.  The filter gradient adds in a fixed
 * order for both types: repeated calls agree bit for bit. */
int fz_gcorr_act(const void* in, const float* w, void* out, const void* mul_a, const void* mul_b, int B, int G,
                 int Ci, int Co, int D, int H, int W, int kd, int kh, int kw, int w_batched, float add_eps,
                 int act_dtype, fz_stream_t stream);
int fz_gcorr_wgrad_act(const void* in, const void* gout, float* gw, void* ws, int B, int G, int Ci, int Co, int D, int H,
                       int W, int kd, int kh, int kw, int w_batched, int act_dtype, fz_stream_t stream);
/* Backward of the fused multiplicative update s' = s * num / den, den = corr(r, wT) + eps, in ONE launch: den is recomputed in
 * the accumulators (it is never stored), and from g = dL/ds'
 *   ds = g * num / den,   dnum = g * s / den,   dden = -g * s * num / den^2
 * are written.  r (B, G*Ci, D, H, W); g, s, num, ds, dnum, dden (B, G*Co, D, H, W), activations of act_dtype; wT as w above.
 * Each of ds / dnum / dden may be NULL and is then not written (at least one must be given).  The gradients of r and wT follow
 * from dden: fz_gcorr_act(dden, adjoint filters) and fz_gcorr_wgrad_act(r, dden). */
int fz_gcorr_mu_bwd(const void* r, const float* wT, const void* g, const void* s, const void* num, void* ds, void* dnum,
                    void* dden, int B, int G, int Ci, int Co, int D, int H, int W, int kd, int kh, int kw, int w_batched,
                    float eps, int act_dtype, fz_stream_t stream);

/* ---- fused soft-Dice + BCE-with-logits loss (training step; the form of the bundle's
 * DiceCELoss(sigmoid=True, squared_pred=True), model_zoo/factorizer_brats23/configs/train.yaml:67-70).
 * sums: part (planes, fz_dice_bce_chunks(V), 4) = {sum p*t, sum p^2, sum t^2, sum bce} per (b,c) plane.
 * grad: gz = gscale * (cd * dDice/dz + cb * dBCE/dz) with coef (planes,2) = {2*inter+s, den+s}. */
int fz_dice_bce_chunks(int64_t V);
int fz_dice_bce_sums(const float* z, const float* t, float* part, int planes, int64_t V, fz_stream_t stream);
int fz_dice_bce_grad(const float* z, const float* t, const float* coef, float* gz, int planes, int64_t V,
                     float cd, float cb, const float* gscale, fz_stream_t stream);

/* DiceCELoss(sigmoid=True, squared_pred=True) as MONAI 1.4 evaluates it for C > 1 channels (the bundle
 * pins monai==1.4.0, model_zoo/factorizer_brats23/docs/requirements.txt:11; train.yaml:67-70): soft Dice on
 * sigmoid(z) per (b,c) plane + nn.CrossEntropyLoss over the channel softmax with the float target as class
 * probabilities.  z, t: (B, C, V), 2 <= C <= 8.
 * sums: part (B, fz_dice_bce_chunks(V), 3C+1) = per channel {sum p*t, sum p^2, sum t^2}, then sum CE.
 * grad: gz = gscale * (cd * dDice/dz + cb * (softmax_c * sum_c' t_c' - t_c)), coef (B*C, 2) = {2*inter+s, den+s}. */
int fz_dice_ce_sums(const float* z, const float* t, float* part, int B, int C, int64_t V, fz_stream_t stream);
/* loss (1 float) = mean_{b,c}(1 - num/den) + sum(CE)/(B V) and coef (B*C, 2) = {num, den} from the partial sums of
 * fz_dice_ce_sums, chunks added in a fixed order; B <= 8 (larger batches: reduce `part` with framework ops) */
int fz_dice_ce_finish(const float* part, int B, int C, int64_t V, float smooth, float* loss, float* coef, fz_stream_t stream);
int fz_dice_ce_grad(const float* z, const float* t, const float* coef, float* gz, int B, int C, int64_t V,
                    float cd, float cb, const float* gscale, fz_stream_t stream);

/* ---- the same four passes for one COARSE level of a deep-supervision head list (MONAI 1.4 DeepSupervisionLoss, restated in
 * factorizer_amd/losses.py): z (planes | B, C; Ld, Lh, Lw) fp32 at the level's extents, t at the TARGET's extents
 * (.., Td, Th, Tw) with Tk a multiple of Lk on every axis (1-D / 2-D: leading extents 1), contiguous, of element kind tkind =
 * FZ_SEG_F32 / FZ_SEG_BF16 / FZ_SEG_U8 (one byte: uint8 or bool).  The level's target value is the nearest-exact pick
 * t[.., r_z*z + r_z/2, r_y*y + r_y/2, r_x*x + r_x/2], r_k = Tk / Lk, loaded in its own type through 64-bit element offsets
 * and converted in registers; no down-sampled target exists in memory.  V = Ld*Lh*Lw must be a multiple of 4 below 2^31.
 * part and coef have the layouts of the dense entry points at that V, so fz_dice_ce_finish (or the caller's own reduction)
 * serves both; arithmetic per voxel, chunking and summation order are the dense kernels'. */
int fz_dice_bce_ds_sums(const float* z, const void* t, float* part, int planes, int Td, int Th, int Tw, int Ld, int Lh, int Lw,
                        int tkind, fz_stream_t stream);
int fz_dice_bce_ds_grad(const float* z, const void* t, const float* coef, float* gz, int planes, int Td, int Th, int Tw,
                        int Ld, int Lh, int Lw, int tkind, float cd, float cb, const float* gscale, fz_stream_t stream);
int fz_dice_ce_ds_sums(const float* z, const void* t, float* part, int B, int C, int Td, int Th, int Tw, int Ld, int Lh, int Lw,
                       int tkind, fz_stream_t stream);
int fz_dice_ce_ds_grad(const float* z, const void* t, const float* coef, float* gz, int B, int C, int Td, int Th, int Tw,
                       int Ld, int Lh, int Lw, int tkind, float cd, float cb, const float* gscale, fz_stream_t stream);

/* ---- the class-index form: DiceCELoss(softmax=True, to_onehot_y=True, include_background, squared_pred) of MONAI 1.4 as
 * restated in factorizer_amd/losses.py.  z (B, C, V) fp32 logits, 2 <= C <= 16, V a positive multiple of
 * 4; y (B, 1, V) a class-index label map of element kind ykind = FZ_LABEL_U8 / FZ_LABEL_I64 / FZ_LABEL_F32, 16-byte aligned
 * (4 for uint8), read in its own type: a float label truncates toward zero, a label outside [0, C) (NaN included) matches no
 * class — its one-hot row is all zero and its CE term is 0, yet it counts in the CE mean's B*V.  With p = softmax_c(z), the
 * maximum subtracted first, and t_c = [y == c] (never stored):
 * sums: part (B, fz_dice_bce_chunks(V), 3C+1) = per channel {sum p t, sum p^2 (sq != 0) or sum p, sum t}, then
 *   sum (logsumexp_c z - z_y).  All C channels are summed; the finish and the gradient leave out those below c0.
 * finish: loss = mean_{b, c >= c0}(1 - num/den) + sum(CE)/(B V), coef (B*C, 2) = {num = 2 inter + s, den = pred + ground + s}
 *   ({0, 1} for c < c0), chunks added in a fixed order; B <= 8, c0 = 0 (include_background) or 1.
 * grad: gz_k = gscale * [ p_k (a_k - sum_c a_c p_c) + cb (p_k - t_k) ],  a_c = cd (-2 t_c/den_c + num_c (sq ? 2 p_c : 1)/den_c^2)
 *   for c >= c0, else 0;  cd = 1/(B (C - c0)), cb = 1/(B V), taken as 0 at a voxel whose label matches no class.
 * ds: one coarse deep-supervision level against the full-resolution label map (B, 1, Td, Th, Tw), geometry and index map as
 *   fz_dice_ce_ds_*; layouts, chunking and summation order are the dense passes'.
 * FZ_E_ARG: null or misaligned pointer, bad ykind, c0 outside {0, 1}; FZ_E_UNSUPPORTED: C outside 2..16 (finish: B > 8);
 * FZ_E_SHAPE: V % 4 != 0, a level of 2^31 voxels or more, extents that do not divide. */
#define FZ_LABEL_U8 0
#define FZ_LABEL_I64 1
#define FZ_LABEL_F32 2
int fz_dice_sce_sums(const float* z, const void* y, float* part, int B, int C, int64_t V, int ykind, int sq,
                     fz_stream_t stream);
int fz_dice_sce_finish(const float* part, int B, int C, int64_t V, int c0, float smooth, float* loss, float* coef,
                       fz_stream_t stream);
int fz_dice_sce_grad(const float* z, const void* y, const float* coef, float* gz, int B, int C, int64_t V, int ykind, int sq,
                     int c0, float cd, float cb, const float* gscale, fz_stream_t stream);
int fz_dice_sce_ds_sums(const float* z, const void* y, float* part, int B, int C, int Td, int Th, int Tw, int Ld, int Lh,
                        int Lw, int ykind, int sq, fz_stream_t stream);
int fz_dice_sce_ds_grad(const float* z, const void* y, const float* coef, float* gz, int B, int C, int Td, int Th, int Tw,
                        int Ld, int Lh, int Lw, int ykind, int sq, int c0, float cd, float cb, const float* gscale,
                        fz_stream_t stream);

/* ---- sliding-window inference stitching -------------------------------------
 * What MONAI's SlidingWindowInfererAdapt(roi 128^3, sw_batch 2, overlap 0.5, mode "gaussian") does
 * around the network (model_zoo/factorizer_brats23/configs/inference.yaml:96-102, train.yaml:206-212):
 * per window  gather: win (C, rd, rh, rw) <- vol (C, D, H, W)[:, z0:, y0:, x0:]
 *             accumulate: out (C, D, H, W)[window] += g * prob (C, rd, rh, rw) ; cnt (D, H, W)[window] += g
 *             with g[z,y,x] = max(gz[z]*gy[y]*gx[x], wmin)  (separable Gaussian importance map)
 * and once    finalize: out /= cnt.
 * One sample per call; rw a multiple of 4 (16-byte vectors on the volume side when W and x0 are
 * too).  Windows must be accumulated by separate
 * (stream-ordered) calls: they overlap. */
int fz_sw_gather(const float* vol, float* win, int C, int D, int H, int W, int rd, int rh, int rw, int z0, int y0,
                 int x0, fz_stream_t stream);
int fz_sw_accumulate(const float* prob, float* out, float* cnt, const float* gz, const float* gy, const float* gx,
                     float wmin, int C, int D, int H, int W, int rd, int rh, int rw, int z0, int y0, int x0,
                     fz_stream_t stream);
int fz_sw_finalize(float* out, const float* cnt, int C, int64_t V, fz_stream_t stream);
/* The same three steps for 1-D, 2-D and 3-D images, any window width and origin, fp32 or bf16 windows (FIVES:
 * SlidingWindowInfererAdapt(roi 512^2, overlap 0.5, mode "gaussian"), model_zoo/deconver_fives/configs/inference.yaml:77-83).
 * A 2-D image is passed as (C, 1, H, W) with gz = {1.0f}, a 1-D one as (C, 1, 1, L) with gz = gy = {1.0f}: the weight
 * (1 * gy) * gx is gy * gx bit for bit.  act_dtype (FZ_STORE_F32 / FZ_STORE_BF16) is the storage type of `img` / `win`
 * (gather: a byte-exact copy), of `prob` (accumulate) and of `res` (finalize); `out` and `cnt` are always fp32, so the
 * overlapping windows are summed in fp32 and the result is rounded once.  finalize writes out / cnt into `res`: fp32 may
 * be `out` itself (in place), bf16 needs a tensor of its own.  With 3-D fp32 data the results equal those of the three
 * calls above bit for bit.  FZ_E_SHAPE for a window outside the image, FZ_E_ARG for a null pointer or another act_dtype. */
int fz_sw_gather2(const void* img, void* win, int C, int D, int H, int W, int rd, int rh, int rw, int z0, int y0, int x0,
                  int act_dtype, fz_stream_t stream);
int fz_sw_accumulate2(const void* prob, float* out, float* cnt, const float* gz, const float* gy, const float* gx,
                      float wmin, int C, int D, int H, int W, int rd, int rh, int rw, int z0, int y0, int x0, int act_dtype,
                      fz_stream_t stream);
int fz_sw_finalize2(const float* out, const float* cnt, void* res, int C, int64_t V, int act_dtype, fz_stream_t stream);

/* ---- segmentation metrics of the recipe (csrc/segmetric.hip) -------------------------------------------------------
 * Every training iteration: Activationsd(sigmoid) -> AsDiscreted(threshold=0.5) -> MeanDice(include_background=True)
 * (model_zoo/factorizer_brats23/configs/train.yaml:215-243); every validation pass: the same Dice and
 * MeanHausdorffDistance(percentile=95) on the stitched prediction (train.yaml:245-287).
 *
 * fz_seg_counts: pred, label (planes, V) dense.  Element kinds FZ_SEG_F32 / FZ_SEG_BF16 / FZ_SEG_U8 (one byte: uint8 or
 *   bool).  A float pred element is foreground iff (float)x >= bound — the caller moves the threshold through the inverse
 *   sigmoid, bound = log(t / (1 - t)), so no transcendental runs on device; a FZ_SEG_U8 pred is a discrete mask, foreground
 *   iff non-zero (bound unused).  A label element counts iff it is non-zero, whatever its kind.  label may be NULL (its
 *   counts are then 0).  mask (planes, V) uint8, optional: the 0 / 1 decision, written by the same pass.  counts
 *   (planes, 3) int64, optional: {|P and Y|, |P|, |Y|}, exact integers, bitwise reproducible (no float atomics: uint32
 *   partials per workgroup in `workspace`, fz_seg_counts_workspace_bytes(planes, V) bytes, always required, added in a
 *   fixed order by a second launch).  16-byte loads when every plane starts 16-byte aligned and holds a multiple of 8
 *   elements (or planes == 1: the last V % 8 elements take a masked tail); any other V or alignment runs one element per
 *   lane.  FZ_E_ARG: null pred / workspace, neither output requested, bad kind, NaN bound; FZ_E_SHAPE: sizes.
 * fz_mask_edges: mask, edges (planes, D, H, W) uint8 (distinct buffers); nd = 1, 2 or 3 spatial axes, a 2-D image passed
 *   as (1, H, W), a 1-D one as (1, 1, L).  edges = 1 where the mask is non-zero and one of the 2 nd face neighbours is
 *   zero or outside the image (mask ^ binary_erosion(mask), cross element, zero border), else 0; counts (planes) int64 =
 *   edge voxels per plane (zeroed by the call).
 * fz_edge_min_dist2: q (nq, 4), t (nt, 4) fp32, 16-byte aligned: integer voxel coordinates in columns 0..2, 0 in unused
 *   columns.  out (nq) = min over t of w0 dx^2 + w1 dy^2 + w2 dz^2 with w = spacing^2, in fp32; independent of the order
 *   of either list.  With w = (1, 1, 1) and coordinates below 2048 every intermediate is an integer < 2^24: exact.
 *   Long target lists are split over fz_edge_min_dist2_splits(nq, nt) workgroup rows whose partial minima (workspace:
 *   fz_edge_min_dist2_workspace_bytes(nq, nt) bytes, 0 when there is one split) are combined in split order. */
#define FZ_SEG_F32 0
#define FZ_SEG_BF16 1
#define FZ_SEG_U8 2
int fz_seg_counts_chunks(int64_t V);
int64_t fz_seg_counts_workspace_bytes(int planes, int64_t V);
int fz_seg_counts(const void* pred, int pred_kind, const void* label, int label_kind, float bound, uint8_t* mask,
                  void* workspace, int64_t* counts, int planes, int64_t V, fz_stream_t stream);
int fz_mask_edges(const uint8_t* mask, uint8_t* edges, int64_t* counts, int planes, int nd, int D, int H, int W,
                  fz_stream_t stream);
int fz_edge_min_dist2_splits(int64_t nq, int64_t nt);
int64_t fz_edge_min_dist2_workspace_bytes(int64_t nq, int64_t nt);
int fz_edge_min_dist2(const float* q, int64_t nq, const float* t, int64_t nt, float w0, float w1, float w2, float* out,
                      void* workspace, fz_stream_t stream);
/* fz_seg_argmax: the multi-class post-processing AsDiscrete(argmax=True[, to_onehot=C]) and the counts of the multi-class
 *   DiceMetric in one streaming pass.  pred: logits (B, C, V) of kind FZ_SEG_F32 / FZ_SEG_BF16 — the class
 *   of a voxel is the argmax over channels, ties to the LOWEST index, the comparison strict on the stored values (z_c > best),
 *   so a NaN never wins and an all-NaN voxel is class 0 — or, with FZ_SEG_U8, an already discrete label map (B, 1, V) whose
 *   value is the class (a value >= C matches no class).  label (B, 1, V), optional, of kind FZ_LABEL_*: converted as the
 *   loss converts it.  Outputs, each optional, at least one required: map (B, 1, V) uint8 class indices; onehot (B, C, V)
 *   uint8 0 / 1; counts (B, C, 3) int64 = {|P = c and Y = c|, |P = c|, |Y = c|}, exact: uint32 partials (B, C, chunks, 3)
 *   per workgroup in `workspace` (fz_seg_argmax_workspace_bytes(B, C, V) bytes, required with counts), summed in a fixed
 *   order by a second launch.  Any V >= 1; 4 voxels per lane when V % 4 == 0 and every pointer is 16-byte aligned, else
 *   one.  2 <= C <= 16.  FZ_E_ARG: null pred, no output, bad kind, null workspace with counts, a pointer not aligned to
 *   its element; FZ_E_UNSUPPORTED: C outside 2..16; FZ_E_SHAPE: B < 1, B > 65535 or V < 1. */
int64_t fz_seg_argmax_workspace_bytes(int B, int C, int64_t V);
int fz_seg_argmax(const void* pred, int pred_kind, const void* label, int label_kind, uint8_t* map, uint8_t* onehot,
                  void* workspace, int64_t* counts, int B, int C, int64_t V, fz_stream_t stream);

/* ---- random training augmentations of the recipe, on device (csrc/augment.hip; semantics: factorizer_amd/augment.py) ----
 * `random_transforms` of every bundle (model_zoo/factorizer_brats23/configs/train.yaml): RandAffined, RandGaussianNoised,
 * RandGaussianSmoothd, RandScaleIntensityd, RandShiftIntensityd, one RandFlipd per axis — for a whole batch at once.
 * image (B, C, D, H, W) of act_dtype, label (B, L, D, H, W) uint8 (or bool); nd = 2 or 3 spatial axes, a 2-D image is passed
 * as D = 1; every extent <= 2048 and fewer than 2^31 voxels per plane (FZ_E_UNSUPPORTED beyond: in-plane offsets are 32-bit).
 * table: B records of fz_aug_record_floats() = 48 fp32 values in DEVICE memory (one host-to-device copy per batch):
 *   [0..8]   A, 3 x 3 row-major over (z, y, x); a 2-D matrix sits in rows / columns 1..2 with A[0] = 1
 *   [9..11]  flip of z, y, x (non-zero: flipped)          [12] noise std (<= 0: none)      [13] gain      [14] offset
 *   [15]     smoothing slot of the sample (0 .. ns - 1), -1: the sample does not smooth
 *   [16..18] tail of the z, y, x taps (0: that axis is not smoothed; at most 4)
 *   [19..45] taps of z, y, x, nine each, centre at index 4, zeros beyond the tail        [46..47] unused
 * fz_aug_resample: output voxel o reads the source position p = A (o' - c) + c with o' = o mirrored on the flipped axes and
 *   c_k = (N_k - 1) / 2, clamped per axis to [0, N_k - 1] (border padding).  Image planes: (bi/tri)linear, fp32 weights and
 *   sums; label planes: the voxel at floor(p + 0.5).  A record whose A is exactly the identity copies (or mirrors) without
 *   arithmetic: bit for bit.  Then image += std z(b, c, v) where seed != NULL and std > 0 — z: word v & 3 of Philox4x32-10
 *   (csrc/fz_philox.h) with counter (v >> 2, c, b, 0x41554731) and key (seed lo, seed hi) of the int64 at `seed` (device
 *   memory), turned into normals by two Box-Muller pairs per counter: u_i = ((w_i >> 8) + 0.5) 2^-24,
 *   (z0, z1) = sqrt(-2 ln u0) (cos, sin)(2 pi u1), likewise (u2, u3) -> (z2, z3); v is the flat OUTPUT voxel.  A sample
 *   without a smoothing slot then stores image gain + offset (one FMA; skipped when gain = 1 and offset = 0) to img_out; a
 *   sample with slot i stores its fp32 values to smooth_ws (ns, C, D, H, W) slot i instead and leaves img_out to
 *   fz_aug_smooth.  One launch covers all planes of all samples.  C = 0 (no image) or L = 0 (no label) is allowed, not both.
 * fz_aug_smooth: for i < ns, sample b = list[i] (device int32; entries outside 0 .. B - 1 are skipped): separable
 *   convolution of smooth_ws slot i with the record's taps along every axis whose tail is > 0, zero padding, fp32, then
 *   gain / offset, stored to img_out sample b in act_dtype (one rounding).  One launch: a workgroup holds an output tile and
 *   its 4-voxel halo in LDS for all passes.  ns = 0 launches nothing.
 * fz_aug_noise_field: out (B, C, V) fp32 = z(b, c, v) alone.
 * fz_aug_crop_resample: fz_aug_resample with the random crop of the recipe (RandSpatialCropd(roi_size, random_size=False), the
 *   first entry of `random_transforms`) cut inside the gather: D, H, W are the ROI = the output extents, and sample b is read
 *   from its own source volume at its own integer origin.  `sources`: B entries of fz_aug_source_words() = 8 int64 words in
 *   DEVICE memory, 8-byte aligned (factorizer_amd/augment.py puts them in front of the records, in the same host-to-device
 *   copy):
 *     [0] address of the sample's image (C, sD, sH, sW) of act_dtype, dense   (ignored when C = 0)
 *     [1] address of the sample's label (L, sD, sH, sW) uint8 / bool, dense   (ignored when L = 0)
 *     [2..4] source extents sD, sH, sW     [5..7] origin gz, gy, gx of the box [g, g + roi) inside the source
 *   A 2-D source is passed as sD = 1, gz = 0.  Output voxel o of sample b reads box position p = A (o' - c) + c with
 *   c_k = (roi_k - 1) / 2, clamped to [0, roi_k - 1]: the arithmetic of fz_aug_resample in crop coordinates (border padding
 *   at the CROP's border); the integer corner indices derived from p are then offset by g.  No voxel outside the box is read,
 *   and the result equals fz_aug_resample run on a dense copy of the boxes, bit for bit; noise counters (the flat OUTPUT
 *   voxel), smoothing slots and gain / offset as there, fz_aug_smooth follows unchanged.  Source extents are not limited to
 *   2048, only to fewer than 2^31 voxels per source plane (in-plane offsets are 32-bit; the 64-bit plane base is formed once
 *   per workgroup).  The kernel SKIPS a sample — reads nothing through its entry, writes nothing for it — whose entry has a
 *   null base where a plane is expected (or an image base not aligned to its element), a box that does not lie inside the
 *   extents, or a source plane of 2^31 voxels or more.  On the identity path a sample whose gx, sW and base put every
 *   lane's first element on a 4-byte boundary (fp32: always; bf16: gx and sW even, base 4-byte aligned; label: gx, sW and
 *   base multiples of 4) is read with one vector load per lane, any other with four scalar loads: same bits.
 * FZ_E_ARG: null pointer or table, aliasing input / output, bad act_dtype, nd outside {2, 3}; FZ_E_SHAPE: sizes, an (output)
 * extent above 2048. */
int fz_aug_record_floats(void);
int fz_aug_resample(const void* img, void* img_out, int act_dtype, int C, const uint8_t* lab, uint8_t* lab_out, int L,
                    const float* table, const int64_t* seed, float* smooth_ws, int ns, int B, int nd, int D, int H, int W,
                    fz_stream_t stream);
int fz_aug_smooth(const float* smooth_ws, void* img_out, int act_dtype, int C, const float* table, const int32_t* list, int ns,
                  int B, int nd, int D, int H, int W, fz_stream_t stream);
int fz_aug_noise_field(float* out, const int64_t* seed, int B, int C, int64_t V, fz_stream_t stream);
int fz_aug_source_words(void);
int fz_aug_crop_resample(const int64_t* sources, void* img_out, int act_dtype, int C, uint8_t* lab_out, int L, const float* table,
                         const int64_t* seed, float* smooth_ws, int ns, int B, int nd, int D, int H, int W, fz_stream_t stream);

/* ---- volume preparation and prediction restore of the recipe, on device (csrc/volprep.hip; semantics:
 * factorizer_amd/volume.py) ----
 * `deterministic_transforms` of the bundles (model_zoo/factorizer_brats23/configs/train.yaml:86-116, inference.yaml:57-83):
 * CropForegroundd(margin) -> NormalizeIntensityd(nonzero, channel_wise) -> BraTSOneHotEncoderd -> SpatialPadd(roi); and the
 * inference `postprocessing` (inference.yaml:104-125): MeanEnsembled -> Activationsd(sigmoid) -> Invertd -> AsDiscreted ->
 * label map.  An image is (C, D, H, W) dense with nd = 1, 2 or 3 spatial axes, a 2-D image passed as (1, H, W), a 1-D one as
 * (1, 1, L).  Element kinds FZ_VOL_*; fz_vol_kind_ok(role, kind) says which kinds a role reads or writes: image in fp32 /
 * int16, image out fp32 / bf16 (round to nearest even), label in uint8 / int16, logits fp32 / bf16.
 * fz_vol_geom (axes lifted to three, z, y, x): `size` the image extent; [start, end) the crop box in image coordinates, which
 *   may reach outside the image (those voxels read as 0); `pad` the zero voxels in front of the box in the prepared volume;
 *   `out` its extent, out >= pad + end - start.  A lifted axis has size 1, start 0, end 1, pad 0, out 1.  The box must contain
 *   at least one voxel of the image and every plane fewer than 2^31 voxels.  Anything else: FZ_E_ARG.
 * fz_vol_bbox: box (6 int32, device) = {min z, y, x, max z, y, x} over the voxels where any channel is > 0; min > max when
 *   there is none.  Integer atomics only: independent of the order.
 * fz_vol_stats: per channel (channel_wise) or over all channels, the elements of the box that are selected — != 0 with
 *   nonzero, else every one, the out-of-image zeros included — as float64 partials per workgroup in `workspace`
 *   (fz_vol_workspace_bytes(C, geom) bytes): (count, sum), then the sum of squares about the float64 mean.  Two launches, no
 *   float atomics; the partial count depends on the box shape alone and every reduction runs in a fixed order.
 * fz_vol_write: out (C, out) of out_kind = 0 outside the box, x where x is not selected, else (x - mean) / std (IEEE
 *   division) with mean, std = the float64 statistics rounded once to fp32; std = 1 when it rounds to 0 or nothing is
 *   selected (then mean = 0).  mean, std (C) fp32 are written too.  The same launch encodes the label: label_channels = 0:
 *   label is a class map (D, H, W) of label_kind and label_out (nclass, out) uint8 = 1 where the class id is in the set k
 *   (class_ids holds the sets one after another, class_counts[k] ids each, 0 <= id < 32, nclass <= 8); label_channels = L > 0:
 *   label is (L, D, H, W) uint8, cropped and padded as it is.  label = NULL: no label.
 * fz_vol_restore: logits[k] (C, out) of `kind`, k < K <= 8; value = (sum in list order) * (1 / K) in fp32, foreground iff
 *   value >= bound.  label_values = NULL: result (C, size) uint8 mask; else (C <= 8) result (size) uint8 = label_values[c] of
 *   the first foreground channel, 0 when there is none.  Voxels outside the box are 0; every voxel of the result is written. */
#define FZ_VOL_F32 0
#define FZ_VOL_BF16 1
#define FZ_VOL_U8 2
#define FZ_VOL_I16 3
#define FZ_VOL_ROLE_IMAGE_IN 0
#define FZ_VOL_ROLE_IMAGE_OUT 1
#define FZ_VOL_ROLE_LABEL_IN 2
#define FZ_VOL_ROLE_LOGITS 3
typedef struct fz_vol_geom {
  int nd;
  int size[3];
  int start[3];
  int end[3];
  int pad[3];
  int out[3];
} fz_vol_geom;
int fz_vol_kind_ok(int role, int kind);
int fz_vol_bbox(const void* image, int kind, int C, int nd, int D, int H, int W, int32_t* box, fz_stream_t stream);
int64_t fz_vol_workspace_bytes(int C, const fz_vol_geom* geom);
int fz_vol_stats(const void* image, int kind, int C, const fz_vol_geom* geom, int nonzero, int channel_wise, void* workspace,
                 fz_stream_t stream);
int fz_vol_write(const void* image, int kind, void* out, int out_kind, int C, const void* label, int label_kind,
                 int label_channels, const int* class_ids, const int* class_counts, int nclass, uint8_t* label_out,
                 const fz_vol_geom* geom, int nonzero, int channel_wise, const void* workspace, float* mean, float* stdev,
                 fz_stream_t stream);
int fz_vol_restore(const void* const* logits, int K, int kind, int C, const fz_vol_geom* geom, float bound,
                   const uint8_t* label_values, uint8_t* result, fz_stream_t stream);

/* ---- resampling to the recipe's voxel spacing and back, on device (csrc/respace.hip; semantics:
 * factorizer_amd/respace.py) ----
 * Orientationd(axcodes) -> Spacingd(pixdim, [bilinear, nearest], align_corners=True, padding_mode="border") -> SpatialPadd of
 * the ISLES22 bundles (model_zoo/factorizer_isles22/configs/train.yaml:97-116) and the Invertd(nearest_interp=false) ->
 * AsDiscreted of their postprocessing (inference.yaml:103-121).  Reorientation and respacing of a grid compose to a monomial
 * map: every axis of the result reads ONE axis of the source at a position that is linear in its own index.
 * fz_respace_geom (axes lifted to three, z, y, x; the host forms every number in it in float64):
 *   src_size   the grid that is resampled (the crop box of the file's grid), in its own axis order;
 *   src_axis   resampled axis w reads source axis src_axis[w] (a permutation); flip[w] != 0: against its direction;
 *   res_size   the resampled extent; index o of axis w reads the ORIENTED position p = scale[w] * o (scale = pixdim / zoom),
 *              clamped to [0, n - 1] with n = src_size[src_axis[w]]; oriented index i is source index flip ? n - 1 - i : i;
 *   inv_scale  the way back: oriented index i reads resampled position inv_scale[w] * i (zoom / pixdim), clamped to
 *              [0, res_size[w] - 1];
 *   pad, out   zero voxels in front of the resampled grid in the padded volume and its extent, out >= pad + res_size;
 *   orig_size, box_start   the file's grid and where src_size starts in it (source axis order; the box may leave the grid).
 *   A lifted axis has size 1 everywhere, reads itself, is not flipped, pad 0, scales 1.  Every plane holds fewer than 2^31
 *   voxels.  Anything else: FZ_E_ARG.
 * Sampling: bilinear takes i0 = floor(p), i1 = min(i0 + 1, n - 1), weight (float)(p - i0), and lerps as fma(f, v1 - v0, v0)
 *   in fp32 along the contiguous axis of the written grid's source order first (resampled axis 2, then 1, then 0); nearest
 *   takes rint(p) (half to even).  Positions are float64.  When every scale is exactly 1 the bilinear mode runs the nearest
 *   kernel: a copy, bit-identical to indexing.
 * fz_vol_respace: image (C, src_size) fp32 -> out (C, out) of out_kind (fp32 / bf16, round to nearest even) in `mode`; label
 *   (L, src_size) uint8 -> label_out (L, out), always nearest; L = 0: no label.  Pad voxels are written as 0; one launch.
 * fz_vol_unspace: logits[k] (C, out) of `kind` (fp32 / bf16), k < K <= 8.  Per corner value = (sum in list order) * (1 / K)
 *   in fp32, through 1 / (1 + exp(-value)) when sigmoid != 0; the corners are interpolated bilinearly through the inverse map
 *   onto orig_size.  discretize != 0: result (C, orig_size) uint8 = value >= threshold; else fp32 values.  Voxels outside the
 *   box are 0; every voxel of the result is written; one launch. */
#define FZ_RESPACE_BILINEAR 0
#define FZ_RESPACE_NEAREST 1
typedef struct fz_respace_geom {
  int nd;
  int src_size[3];
  int src_axis[3];
  int flip[3];
  int res_size[3];
  int pad[3];
  int out[3];
  int orig_size[3];
  int box_start[3];
  double scale[3];
  double inv_scale[3];
} fz_respace_geom;
int fz_vol_respace(const float* image, int C, void* out, int out_kind, const uint8_t* label, int L, uint8_t* label_out,
                   const fz_respace_geom* geom, int mode, fz_stream_t stream);
int fz_vol_unspace(const void* const* logits, int K, int kind, int C, const fz_respace_geom* geom, int sigmoid, int discretize,
                   float threshold, void* result, fz_stream_t stream);

/* ---- instance norm of channels-first activations (csrc/inorm.hip, csrc/inorm_core.h; semantics:
 * factorizer_amd/instance_norm.py) ----
 * The block norm of the Deconver bundles (deconver.py:50-66 norm1 / norm2 and :129-138 Stem with norm: nn.InstanceNorm3d /
 * nn.InstanceNorm2d).  x, y, gy, gx: (B, C, *S) contiguous of act_dtype, seen as P = B C planes of V elements, element-aligned
 * (any storage offset, any V); weight, bias (C) fp32 or NULL (1 and 0); stats (P, 2) float64 = (mean, 1 / sqrt(var + eps)) per
 * plane, written by the forward and read by the backward.  All arithmetic is float64, one rounding per stored element:
 *   mean = x0 + Σd / V, var = max(Σd² / V − (Σd / V)², 0) with d = x − x0, x0 the plane's first element (biased variance);
 *   y = (x − mean) rstd γ_c + β_c;   gx = (g γ_c − a − x̂ b) rstd with x̂ = (x − mean) rstd, a = γ_c Σg / V, b = γ_c Σg x̂ / V;
 *   gbias_c = Σ_b Σ_v g, gweight_c = Σ_b Σ_v g x̂ (either may be NULL), per-plane totals summed over b in index order.
 * No atomics: every sum has a fixed order that depends on V alone, so results repeat bit for bit and a plane's result does not
 * depend on the other planes or on its address.  Planes of V <= fz_inorm_one_pass_max() take one launch each way; larger ones
 * two over fz_inorm_chunks(V) workgroups per plane; gweight / gbias add one.  workspace: fz_inorm_workspace_bytes(P, V) bytes,
 * 8-byte aligned, scratch of one call (-1: P < 1, V < 1 or too large).  V < 1, P < 1: FZ_E_ARG; act_dtype outside FZ_STORE_*:
 * FZ_E_UNSUPPORTED; P not a multiple of C, V >= 2^31, 2^24 or more workgroups (P fz_inorm_chunks(V)): FZ_E_SHAPE — all before anything touches the device. */
int fz_inorm_one_pass_max(void);
int fz_inorm_chunks(int64_t V);
int64_t fz_inorm_workspace_bytes(int64_t P, int64_t V);
int fz_inorm_fwd(const void* x, const float* weight, const float* bias, void* y, double* stats, int64_t P, int C, int64_t V,
                 double eps, int act_dtype, void* workspace, fz_stream_t stream);
int fz_inorm_bwd(const void* x, const void* gy, const float* weight, const double* stats, void* gx, float* gweight,
                 float* gbias, int64_t P, int C, int64_t V, int act_dtype, void* workspace, fz_stream_t stream);

/* ---- group norm of channels-first activations with a fused activation (csrc/gnorm.hip, csrc/gnorm_core.h; semantics:
 * factorizer_amd/group_norm.py) ----
 * The default norm + activation of the CNN blocks (factorizer_amd/cnn.py: nn.GroupNorm(8, C), nn.LeakyReLU).  x, y, gy, gx:
 * (B, C, *S) contiguous of act_dtype, element-aligned (any storage offset, any V); with G groups a group is cg = C / G adjacent
 * planes of V elements, one span of n = cg V elements.  weight, bias (C) fp32 or NULL (1 and 0); stats (B G, 2) float64 =
 * (mean, 1 / sqrt(var + eps)) per group, written by the forward and read by the backward.  All arithmetic is float64, one
 * rounding per stored element, sums about the group's first element as for the instance norm above:
 *   z = (x − mean) rstd γ_c + β_c;  y = act(z), act: 0 none, 1 ReLU, 2 LeakyReLU(negative_slope) (FZ_GNORM_ACT_*);
 *   g' = g (z > 0 ? 1 : slope) (slope 0 for ReLU, no gate for none; closed at z == 0);  per (b, c): s1 = Σ_v g', s2 = Σ_v g' x̂;
 *   gbias_c = Σ_b s1, gweight_c = Σ_b s2 in batch-index order (either NULL, or its parameter must be given);
 *   A = Σ_{c in group} γ_c s1 / n, Bq = Σ γ_c s2 / n;  gx = (g' γ_c − A − x̂ Bq) rstd.
 * No atomics: every sum has a fixed order that depends on (cg, V) and on which parameters are present alone, so results repeat
 * bit for bit and a group's result depends neither on the rest of the batch nor on its address.  Spans n <=
 * fz_gnorm_one_pass_max() take one launch each way; larger ones two (fz_gnorm_chunks(cg, V) workgroups per group in the forward
 * and in the backward's apply launch); gweight / gbias add one: fz_gnorm_launches(cg, V, backward, affine).  workspace:
 * fz_gnorm_workspace_bytes(B, C, G, V) bytes, 8-byte aligned, scratch of one call (-1: out of range).  B < 1, V < 1, a null
 * pointer: FZ_E_ARG; act_dtype outside FZ_STORE_*, an unknown activation: FZ_E_UNSUPPORTED; C no multiple of G, n >= 2^31, 2^24
 * or more workgroups: FZ_E_SHAPE — all before anything touches the device. */
#define FZ_GNORM_ACT_NONE 0
#define FZ_GNORM_ACT_RELU 1
#define FZ_GNORM_ACT_LEAKY_RELU 2
int fz_gnorm_one_pass_max(void);
int fz_gnorm_chunks(int cg, int64_t V);
int64_t fz_gnorm_workspace_bytes(int64_t B, int C, int G, int64_t V);
int fz_gnorm_launches(int cg, int64_t V, int backward, int affine);
int fz_gnorm_fwd(const void* x, const float* weight, const float* bias, void* y, double* stats, int64_t B, int C, int G,
                 int64_t V, double eps, int act, double negative_slope, int act_dtype, void* workspace, fz_stream_t stream);
int fz_gnorm_bwd(const void* x, const void* gy, const float* weight, const float* bias, const double* stats, void* gx,
                 float* gweight, float* gbias, int64_t B, int C, int G, int64_t V, int act, double negative_slope,
                 int act_dtype, void* workspace, fz_stream_t stream);

/* ---- AdamW over one flat buffer (torch.optim.AdamW of the training recipe,
 * model_zoo/factorizer_brats23/configs/train.yaml:72-76).  step >= 1 is the 1-based update count;
 * grad_scale multiplies the gradient first (1/world after a summed all-reduce). */
int fz_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                  fz_stream_t stream);

/* ---- block dropout in training mode (FactorizerBlock: factorizer.py:53-56,69,72; mlp.py:54-60) ----
 * Sites: 0 = fact.dropout on out_proj(a) + b_out, 1 = mlp.block[2] on gelu(z1), 2 = mlp.block[4] on fc2(h) + b2.
 * Mask generator: Philox4x32-10 (csrc/fz_philox.h), key = (seed & 0xffffffff, seed >> 32) of the int64 at `seed` (device
 * memory: read by the kernel, never by the host), counter (v >> 2, c, b, site) for voxel v of channel c of sample b.  The
 * element is kept iff output word v & 3 < floor((1 - p) 2^32): keep probability exactly that / 2^32; p = 0 keeps all.
 * Bits: one plane of fz_dropout_bits_words(B, ch, V) uint32 words, (B, ch, ceil(V / 32)) row-major, bit v & 31 of word
 * v >> 5 of row (b, ch); padding bits are 0.  Returns -1 for a negative shape.
 * fz_dropout_keep_bits: 0 <= p < 1, site in 0..2, every argument checked on the host before any device work.
 * fz_dropout_apply: y (B, ch, V activation of act_dtype, V % 4 == 0, 16-byte aligned for fp32 / 8 for bf16), with
 * s = 1 / (1 - p) and keep = the element's bit:
 *   FZ_DROP_RES      y = aux + keep s t        (aux NULL: y = keep s t — also the gradient g <- keep s g)
 *   FZ_DROP_GELU     y = keep s gelu(t)
 *   FZ_DROP_GELU_BWD y = keep s t gelu'(aux)   (t = dL/dh, aux = z1: dL/dz1) */
#define FZ_DROP_RES 0
#define FZ_DROP_GELU 1
#define FZ_DROP_GELU_BWD 2
int64_t fz_dropout_bits_words(int B, int ch, int64_t V);
int fz_dropout_keep_bits(const int64_t* seed, int site, int B, int ch, int64_t V, float p, uint32_t* out, fz_stream_t stream);
int fz_dropout_apply(int kind, const uint32_t* bits, float p, const void* t, const void* aux, void* y, int B, int ch, int64_t V,
                     int act_dtype, fz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FACTORIZER_HIP_H */
