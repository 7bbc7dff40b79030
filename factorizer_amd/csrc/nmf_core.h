// nmf_core.h — the per-wavefront NMF program (forward iterations + reverse sweep).
//
// One wave64 owns one M×N matrix: every lane keeps NPL = N/64 columns of X (all M rows) in
// registers, its NPL rows of V, and a replicated copy of U.  X·V and VᵀV are lane-local partial
// sums followed by a wave reduction; XᵀU and UᵀU are purely lane-local.  X is read from HBM
// exactly once for all T iterations (the reference re-reads it in ~4T bmm launches,
// factorization/matrix_factorization.py:213,243).
//
// The program is written once against a "wave context" W so that the same source compiles
//   * for gfx950 (W::F = float, one lane per thread; csrc/nmf.hip), and
//   * for the host lock-step emulation used by the CPU tests (W::F = 64-lane vector;
//     tests/emul/emul.cpp) — that build exists only to test this file without a GPU.
//
// Update rules restated from the reference (paths relative to the reference root):
//   MU   factorization/matrix_factorization.py:241-247
//   HALS factorization/matrix_factorization.py:210-229 (CoordinateDescent, project=ReLU)
//   CD   factorization/matrix_factorization.py:210-229 (CoordinateDescent, project=Identity)
//   SMU  factorization/matrix_factorization.py:319-341 (SemiMultiplicativeUpdate; X of any sign)
//   alternation U then V with the new U: :122-136 ; reconstruct u @ v.mT: :532-533
// Reverse sweep: SURVEY.md Appendix A (hand-derived; checked against autograd by the oracle); CD / SMU: DESIGN.md §7.1.
#pragma once

#if defined(__HIPCC__)
#define FZ_HD __host__ __device__ __forceinline__
#else
#define FZ_HD inline
#endif

namespace fz {

constexpr int SOLVER_MU = 0;
constexpr int SOLVER_HALS = 1;
constexpr int SOLVER_CD = 2;
constexpr int SOLVER_SMU = 3;
template <int SOLVER>
constexpr bool fz_known_solver() { return SOLVER == SOLVER_MU || SOLVER == SOLVER_HALS || SOLVER == SOLVER_CD || SOLVER == SOLVER_SMU; }

// host dispatch of a launch macro on the run-time id `solver` (FZ_SOLVER_*, checked by the entry point):
// MACRO(args..., SOLVER_x); an id the entry point let through that is none of MU / CD / SMU runs HALS, as before CD / SMU.
#define FZ_SOLVER_CASES(MACRO, ...)                                         \
  do {                                                                      \
    switch (solver) {                                                       \
      case FZ_SOLVER_MU: MACRO(__VA_ARGS__, SOLVER_MU); break;              \
      case FZ_SOLVER_CD: MACRO(__VA_ARGS__, SOLVER_CD); break;              \
      case FZ_SOLVER_SMU: MACRO(__VA_ARGS__, SOLVER_SMU); break;            \
      default: MACRO(__VA_ARGS__, SOLVER_HALS); break;                      \
    }                                                                       \
  } while (0)

// reciprocal: v_rcp_f32 on device (1 ulp) instead of the ~10-instruction IEEE division sequence —
// the HALS/MU ratios need 1e-4 parity, not correct rounding, and the backward kernel is VALU-bound
#if defined(__HIP_DEVICE_COMPILE__)
FZ_HD float fz_rcp(float v) { return __builtin_amdgcn_rcpf(v); }
// square root of the SMU ratio n/d (n, d >= eps): v_sqrt_f32 (1 ulp), same reasoning as fz_rcp
FZ_HD float fz_sqrt(float v) { return __builtin_amdgcn_sqrtf(v); }
#else
FZ_HD float fz_rcp(float v) { return 1.0f / v; }
FZ_HD float fz_sqrt(float v) { return __builtin_sqrtf(v); }
#endif
FZ_HD float fz_relu(float v) { return v > 0.f ? v : 0.f; }
// gate(w, g) = g where w > 0 else 0  (ReLU mask taken from the forward value)
FZ_HD float fz_gate(float w, float g) { return w > 0.f ? g : 0.f; }

// ---- optional policy capability: factor rows DISTRIBUTED over lane groups ---------------------------------
// A policy with `static constexpr bool kDistRows = true` provides, for M = 8 rows:
//   F    sum8_dist(const F (&v)[8])             eight wave totals, total m left in every lane of lane group m
//   F    grp_take(F d, int m)                   the value lane group m holds, uniform
//   bool grp_below(int n)                       this lane's group index < n
//   void st_grp(float* base, int i0, int stride, F d)    base[i0 + group·stride] = d   (one lane per group)
//   F    ld_grp_global(const float* p, int i0, int stride)  p[i0 + group·stride]
//   F    ld_grp(const float* base, int i0, int stride)      the same from the wave's LDS history
//   F    grp_sum(F d)                                        total over the eight groups of a group-constant value, uniform
// The U half-step then runs ONCE with one row per lane group instead of eight times on wave-uniform values in all 64
// lanes (a third of the VALU instructions of a rank-2 iteration).  The arithmetic of every row is unchanged, but the
// compiler contracts and schedules the one-row and the eight-row code separately: the two forms agree to the last bit
// or two (4e-7 relative, tools/probes/nmf_ab.py), not bit for bit.  Policies without the flag (the host emulation among
// them) take the uniform form.
template <class W, class = void>
struct DistRows { static constexpr bool value = false; };
template <class W>
struct DistRows<W, decltype((void)W::kDistRows)> { static constexpr bool value = W::kDistRows; };

// ---- wave totals of K independent per-lane partial sums, eight at a time where K allows -----------
template <int K, class W, class F>
FZ_HD void sum_all(W& w, F (&acc)[K]) {
  if constexpr (K % 8 == 0) {
#pragma unroll
    for (int k0 = 0; k0 < K; k0 += 8) {
      F t[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) t[i] = acc[k0 + i];
      w.sum8(t);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[k0 + i] = t[i];
    }
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = w.sum(acc[k]);
  }
}

// ---- one half-step on K independent rows of a factor:  w' = update(w; a, b) ------------
template <int K, int R, int SOLVER, class F>
FZ_HD void update_rows(F (&w)[K][R], const F (&a)[K][R], const F (&b)[R][R], float eps) {
  static_assert(fz_known_solver<SOLVER>(), "update_rows: unknown solver id");
  if constexpr (SOLVER == SOLVER_MU) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      F nw[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        F dn = w[k][0] * b[0][r];
#pragma unroll
        for (int q = 1; q < R; ++q) dn = dn + w[k][q] * b[q][r];
        nw[r] = (w[k][r] * a[k][r] + eps) * fz_rcp(dn + eps);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) w[k][r] = nw[r];
    }
  } else if constexpr (SOLVER == SOLVER_SMU) {
    // semi-NMF: n = relu(a) + w relu(-b) + eps, d = relu(-a) + w relu(b) + eps, w' = w sqrt(n / d) (Jacobi: the old w
    // throughout the row).  The split of b by sign is shared by all K rows.
    F bpos[R][R], bneg[R][R];
#pragma unroll
    for (int q = 0; q < R; ++q)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        bpos[q][r] = fz_relu(b[q][r]);
        bneg[q][r] = fz_relu(F(0.f) - b[q][r]);
      }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      F nw[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        F nu = fz_relu(a[k][r]);
        F de = fz_relu(F(0.f) - a[k][r]);
#pragma unroll
        for (int q = 0; q < R; ++q) {
          nu = nu + w[k][q] * bneg[q][r];
          de = de + w[k][q] * bpos[q][r];
        }
        nw[r] = w[k][r] * fz_sqrt((nu + eps) * fz_rcp(de + eps));
      }
#pragma unroll
      for (int r = 0; r < R; ++r) w[k][r] = nw[r];
    }
  } else {
    // HALS, and CD (the same rule without the projection)
    constexpr bool kProj = SOLVER == SOLVER_HALS;
    // the denominators b[r][r] + eps are shared by all K rows: one reciprocal per column
    F inv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) inv[r] = fz_rcp(b[r][r] + eps);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (R == 1) {
        const F t = (a[k][0] + eps) * inv[0];
        if constexpr (kProj) w[k][0] = fz_relu(t);
        else w[k][0] = t;
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          F s = F(0.f);
          bool first = true;
#pragma unroll
          for (int q = 0; q < R; ++q) {
            if (q == r) continue;
            F t = w[k][q] * b[q][r];  // columns q < r are already updated (Gauss–Seidel)
            s = first ? t : s + t;
            first = false;
          }
          const F t = (a[k][r] - s + eps) * inv[r];
          if constexpr (kProj) w[k][r] = fz_relu(t);
          else w[k][r] = t;
        }
      }
    }
  }
}

// ---- reverse of one half-step for ONE row --------------------------------------------
//  in : wold, wnew (forward values), a (row of Z s), b = sᵀs, gwn = dL/dwnew (clobbered)
//  out: gwo = dL/dwold, ga = dL/da (row), gb += this row's contribution to dL/db
template <int R, int SOLVER, class F>
FZ_HD void half_bwd_row(const F (&wold)[R], const F (&wnew)[R], const F (&a)[R],
                        const F (&b)[R][R], F (&gwn)[R], F (&gwo)[R], F (&ga)[R],
                        F (&gb)[R][R], float eps) {
  static_assert(fz_known_solver<SOLVER>(), "half_bwd_row: unknown solver id");
  if constexpr (SOLVER == SOLVER_MU) {
    F gn[R], gdn[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      F dn = wold[0] * b[0][r];
#pragma unroll
      for (int q = 1; q < R; ++q) dn = dn + wold[q] * b[q][r];
      const F idn = fz_rcp(dn + eps);
      gn[r] = gwn[r] * idn;
      gdn[r] = F(0.f) - gwn[r] * wnew[r] * idn;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      F t = gn[r] * a[r];
#pragma unroll
      for (int q = 0; q < R; ++q) t = t + gdn[q] * b[r][q];
      gwo[r] = t;
      ga[r] = gn[r] * wold[r];
#pragma unroll
      for (int q = 0; q < R; ++q) gb[q][r] = gb[q][r] + wold[q] * gdn[r];
    }
  } else if constexpr (SOLVER == SOLVER_SMU) {
    // w'_r = w_r s_r, s_r = sqrt(n_r / d_r):  gn_r = g_r w'_r / (2 n_r), gd_r = -g_r w'_r / (2 d_r),
    // dL/dw_r = g_r s_r + sum_c (gn_c relu(-b_rc) + gd_c relu(b_rc)),  dL/da_r = gn_r [a_r > 0] - gd_r [a_r < 0],
    // dL/db_qr += w_q (gd_r [b_qr > 0] - gn_r [b_qr < 0])   (relu'(0) = 0)
    F gn[R], gd[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      F nu = fz_relu(a[r]);
      F de = fz_relu(F(0.f) - a[r]);
#pragma unroll
      for (int q = 0; q < R; ++q) {
        nu = nu + wold[q] * fz_relu(F(0.f) - b[q][r]);
        de = de + wold[q] * fz_relu(b[q][r]);
      }
      const F ide = fz_rcp(de + eps);
      const F inu = fz_rcp(nu + eps);
      const F h = gwn[r] * wnew[r] * 0.5f;
      gwo[r] = gwn[r] * fz_sqrt((nu + eps) * ide);
      gn[r] = h * inu;
      gd[r] = F(0.f) - h * ide;
      ga[r] = fz_gate(a[r], gn[r]) - fz_gate(F(0.f) - a[r], gd[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      F t = gwo[r];
#pragma unroll
      for (int c = 0; c < R; ++c) t = t + gn[c] * fz_relu(F(0.f) - b[r][c]) + gd[c] * fz_relu(b[r][c]);
      gwo[r] = t;
#pragma unroll
      for (int q = 0; q < R; ++q)
        gb[q][r] = gb[q][r] + wold[q] * (fz_gate(b[q][r], gd[r]) - fz_gate(F(0.f) - b[q][r], gn[r]));
    }
  } else {
    // HALS, and CD: the same reverse step without the ReLU gate
#pragma unroll
    for (int r = 0; r < R; ++r) gwo[r] = F(0.f);
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {
      const F iden = fz_rcp(b[r][r] + eps);
      F gq;
      if constexpr (SOLVER == SOLVER_HALS) gq = fz_gate(wnew[r], gwn[r]);
      else gq = gwn[r];
      F gnum = gq * iden;
      gb[r][r] = gb[r][r] - (gq * wnew[r]) * iden;
      ga[r] = gnum;
#pragma unroll
      for (int q = 0; q < R; ++q) {
        if (q == r) continue;
        if (q < r) {
          gb[q][r] = gb[q][r] - gnum * wnew[q];
          gwn[q] = gwn[q] - gnum * b[q][r];
        } else {
          gb[q][r] = gb[q][r] - gnum * wold[q];
          gwo[q] = gwo[q] - gnum * b[q][r];
        }
      }
    }
  }
}

// ---- per-wave history kept in LDS for the reverse sweep --------------------------------
// state s = 0..G holds (u, v) after iteration T-G+s; step s = 0..G-1 holds the (a, b) of the
// U-update that produced state s+1.
template <int M, int NPL, int R>
struct Hist {
  float* vh;  // lane-private: [(G+1)][R][NPL] × 64 lanes
  float* uh;  // uniform:      [(G+1)][M][R]
  float* ah;  // uniform:      [G][M][R]
  float* bh;  // uniform:      [G][R][R]
  static FZ_HD int floats(int G) {
    return (G + 1) * R * NPL * 64 + (G + 1) * M * R + G * (M * R + R * R);
  }
  FZ_HD void carve(float* base, int G) {
    vh = base;
    uh = vh + (G + 1) * R * NPL * 64;
    ah = uh + (G + 1) * M * R;
    bh = ah + G * M * R;
  }
};

// waves per workgroup of a backward launch whose history needs `per_wave` bytes of LDS per wave: the count (1..4) that
// puts the most waves on a CU (160 KB of LDS), larger workgroups on ties.  (A fixed 64 KB budget per workgroup left
// the R = 2, T = 10 history of BASELINE configs[4] — 18.4 KB per wave — at 3 waves x 2 workgroups = 6 waves per CU; 4 x 2 = 8.)
static inline int fz_hist_waves_per_block(int per_wave) {
  int best = 1, best_waves = 0;
  for (int wv = 1; wv <= 4; ++wv) {
    const int lds = per_wave * wv;
    if (lds > 160 * 1024) break;
    const int waves = (160 * 1024 / lds) * wv;
    if (waves >= best_waves) { best_waves = waves; best = wv; }
  }
  return best;
}

template <int M, int NPL, int R, class W>
FZ_HD void save_state(W& w, const Hist<M, NPL, R>& h, int s, const typename W::F (&u)[M][R],
                      const typename W::F (&v)[NPL][R]) {
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) w.st_uni(h.uh, (s * M + m) * R + r, u[m][r]);
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int j = 0; j < NPL; ++j) w.st_priv(h.vh, (s * R + r) * NPL + j, v[j][r]);
}

template <int M, int NPL, int R, class W>
FZ_HD void save_state_dist(W& w, const Hist<M, NPL, R>& h, int s, const typename W::F (&ud)[R],
                           const typename W::F (&v)[NPL][R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) w.st_grp(h.uh, s * M * R + r, R, ud[r]);
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int j = 0; j < NPL; ++j) w.st_priv(h.vh, (s * R + r) * NPL + j, v[j][r]);
}

// ---- one full iteration: U-update then V-update ---------------------------------------
// step >= 0: also record (a, b) of the U-update as step `step` and the new state as step+1.
// ud (policies with kDistRows, M = 8): the CURRENT u in distributed form, ud[r] of lane group m = u[m][r]; kept in step
// with the uniform copy `u` that the column work reads.
template <int M, int NPL, int R, int SOLVER, class W>
FZ_HD void nmf_step(W& w, const typename W::F (&x)[M][NPL], typename W::F (&u)[M][R],
                    typename W::F (&v)[NPL][R], int mreal, float eps,
                    const Hist<M, NPL, R>* h, int step, typename W::F (*ud)[R] = nullptr) {
  using F = typename W::F;
  if constexpr (DistRows<W>::value && M == 8) {
    F ad[1][R];
    F b[R][R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      F col[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        F acc = x[m][0] * v[0][r];
#pragma unroll
        for (int j = 1; j < NPL; ++j) acc = acc + x[m][j] * v[j][r];
        col[m] = acc;
      }
      ad[0][r] = w.sum8_dist(col);
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = r; q < R; ++q) {
        F acc = v[0][r] * v[0][q];
#pragma unroll
        for (int j = 1; j < NPL; ++j) acc = acc + v[j][r] * v[j][q];
        F t = w.sum(acc);
        b[r][q] = t;
        b[q][r] = t;
      }
    if (h != nullptr && step >= 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) w.st_grp(h->ah, step * M * R + r, R, ad[0][r]);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < R; ++q) w.st_uni(h->bh, (step * R + r) * R + q, b[r][q]);
    }
    update_rows<1, R, SOLVER, F>(*reinterpret_cast<F (*)[1][R]>(ud), ad, b, eps);
#pragma unroll
    for (int r = 0; r < R; ++r) (*ud)[r] = w.grp_below(mreal) ? (*ud)[r] : F(0.f);
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int r = 0; r < R; ++r) u[m][r] = w.grp_take((*ud)[r], m);
  } else {
    F a[M][R];
    F b[R][R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      F col[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        F acc = x[m][0] * v[0][r];
#pragma unroll
        for (int j = 1; j < NPL; ++j) acc = acc + x[m][j] * v[j][r];
        col[m] = acc;
      }
      sum_all<M, W, F>(w, col);
#pragma unroll
      for (int m = 0; m < M; ++m) a[m][r] = col[m];
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = r; q < R; ++q) {
        F acc = v[0][r] * v[0][q];
#pragma unroll
        for (int j = 1; j < NPL; ++j) acc = acc + v[j][r] * v[j][q];
        F t = w.sum(acc);
        b[r][q] = t;
        b[q][r] = t;
      }
    if (h != nullptr && step >= 0) {
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) w.st_uni(h->ah, (step * M + m) * R + r, a[m][r]);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < R; ++q) w.st_uni(h->bh, (step * R + r) * R + q, b[r][q]);
    }
    update_rows<M, R, SOLVER, F>(u, a, b, eps);
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int r = 0; r < R; ++r) u[m][r] = (m < mreal) ? u[m][r] : F(0.f);
  }
  {
    F ap[NPL][R];
    F bp[R][R];
#pragma unroll
    for (int j = 0; j < NPL; ++j)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        F acc = x[0][j] * u[0][r];
#pragma unroll
        for (int m = 1; m < M; ++m) acc = acc + x[m][j] * u[m][r];
        ap[j][r] = acc;
      }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = r; q < R; ++q) {
        F acc = u[0][r] * u[0][q];
#pragma unroll
        for (int m = 1; m < M; ++m) acc = acc + u[m][r] * u[m][q];
        bp[r][q] = acc;
        bp[q][r] = acc;
      }
    update_rows<NPL, R, SOLVER, F>(v, ap, bp, eps);
#pragma unroll
    for (int j = 0; j < NPL; ++j)
#pragma unroll
      for (int r = 0; r < R; ++r) v[j][r] = w.keep_col(j, v[j][r]);
  }
  if (h != nullptr && step >= 0) {
    if constexpr (DistRows<W>::value && M == 8) save_state_dist<M, NPL, R, W>(w, *h, step + 1, *ud, v);
    else save_state<M, NPL, R, W>(w, *h, step + 1, u, v);
  }
}

// ---- initial factors: the broadcast RandomInit buffers (matrix_factorization.py:52-58) --
template <int M, int NPL, int R, class W>
FZ_HD void nmf_init(W& w, const float* u0, const float* v0, typename W::F (&u)[M][R],
                    typename W::F (&v)[NPL][R], int mreal) {
  using F = typename W::F;
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) u[m][r] = (m < mreal) ? w.ld_uni_global(u0, m * R + r) : F(0.f);
#pragma unroll
  for (int j = 0; j < NPL; ++j)
#pragma unroll
    for (int r = 0; r < R; ++r) v[j][r] = w.ld_v0(v0, j, r, R);
}

// distributed copy of the initial u (policies with kDistRows)
template <int M, int R, class W>
FZ_HD void nmf_init_dist(W& w, const float* u0, typename W::F (&ud)[R], int mreal) {
  using F = typename W::F;
  if constexpr (DistRows<W>::value && M == 8) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const F t = w.ld_grp_global(u0, r, R);
      ud[r] = w.grp_below(mreal) ? t : F(0.f);
    }
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) ud[r] = F(0.f);
  }
}

// ---- forward: T iterations, then y = u vᵀ ---------------------------------------------
template <int M, int NPL, int R, int SOLVER, class W>
FZ_HD void nmf_forward_wave(W& w, const float* u0, const float* v0,
                            typename W::F (&x)[M][NPL], typename W::F (&u)[M][R],
                            typename W::F (&v)[NPL][R], int mreal, int T, float eps) {
  nmf_init<M, NPL, R, W>(w, u0, v0, u, v, mreal);
  typename W::F ud[R];
  nmf_init_dist<M, R, W>(w, u0, ud, mreal);
  for (int t = 0; t < T; ++t)
    nmf_step<M, NPL, R, SOLVER, W>(w, x, u, v, mreal, eps, nullptr, -1, &ud);
  // x becomes y
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      typename W::F acc = u[m][0] * v[j][0];
#pragma unroll
      for (int r = 1; r < R; ++r) acc = acc + u[m][r] * v[j][r];
      x[m][j] = acc;
    }
}

// ---- backward: recompute forward with history, then the reverse sweep ------------------
//  x: the matrix;  g: on entry dL/dy (zeros if only gu/gv are given), on exit dL/dx.
//  gu_ext / gv_ext: optional extra gradients of the decompose() outputs (device: global
//  pointers for this matrix, may be nullptr).
template <int M, int NPL, int R, int SOLVER, class W>
FZ_HD void nmf_backward_wave(W& w, const float* u0, const float* v0,
                             const typename W::F (&x)[M][NPL], typename W::F (&g)[M][NPL],
                             const Hist<M, NPL, R>& h, int mreal, int T, int G, float eps,
                             const float* gu_ext, const float* gv_ext) {
  using F = typename W::F;
  // The reverse sweep on distributed rows adds the rows' contributions to dL/db in a tree over the lane groups instead of
  // row by row.  MU keeps the row-by-row (uniform) reverse sweep (its ε⁻¹-scaled gradients are the most sensitive to
  // rounding order in the oracle tests); its forward recomputation is distributed where the policy asks for it.  SMU keeps it
  // too, for the same reason: its reverse step scales by 1 / (2 n) and 1 / (2 d), which sit at eps for rows whose numerator or
  // denominator vanishes.  CD has HALS's reverse step without the gate and takes the distributed sweep like HALS.
  constexpr bool kDistBwd = DistRows<W>::value && M == 8 && SOLVER != SOLVER_MU && SOLVER != SOLVER_SMU;
  // MU and HALS give a padded row / column (forced to zero by the forward) a zero gradient through their algebra or the ReLU
  // gate whatever arrives there; CD (no gate) and SMU (the sqrt(n / d) factor) would pass it on, so their incoming gradients
  // are masked once here, and the sweep keeps them zero (x, u and v vanish on the padding).
  constexpr bool kMaskPad = SOLVER == SOLVER_CD || SOLVER == SOLVER_SMU;
  F gu[M][R];
  F gud[R];      // (kDistBwd) dL/du in distributed form: lane group m holds row m
  F gv[NPL][R];
  {
    F u[M][R];
    F v[NPL][R];
    nmf_init<M, NPL, R, W>(w, u0, v0, u, v, mreal);
    F ud[R];
    nmf_init_dist<M, R, W>(w, u0, ud, mreal);
    for (int t = 0; t < T - G; ++t)
      nmf_step<M, NPL, R, SOLVER, W>(w, x, u, v, mreal, eps, nullptr, -1, &ud);
    save_state<M, NPL, R, W>(w, h, 0, u, v);
    for (int s = 0; s < G; ++s) nmf_step<M, NPL, R, SOLVER, W>(w, x, u, v, mreal, eps, &h, s, &ud);
    // output layer  y = u_T v_Tᵀ :  gu = gY v_T ,  gv = gYᵀ u_T
#pragma unroll
    for (int r = 0; r < R; ++r) {
      F col[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        F acc = g[m][0] * v[0][r];
#pragma unroll
        for (int j = 1; j < NPL; ++j) acc = acc + g[m][j] * v[j][r];
        col[m] = acc;
      }
      if constexpr (kDistBwd) {
        gud[r] = w.sum8_dist(col);
        if (gu_ext != nullptr) gud[r] = gud[r] + (w.grp_below(mreal) ? w.ld_grp_global(gu_ext, r, R) : F(0.f));
      } else {
      sum_all<M, W, F>(w, col);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        gu[m][r] = col[m];
        if (gu_ext != nullptr && m < mreal) gu[m][r] = gu[m][r] + w.ld_uni_global(gu_ext, m * R + r);
      }
      }
    }
#pragma unroll
    for (int j = 0; j < NPL; ++j)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        F acc = g[0][j] * u[0][r];
#pragma unroll
        for (int m = 1; m < M; ++m) acc = acc + g[m][j] * u[m][r];
        gv[j][r] = acc;
        if (gv_ext != nullptr) gv[j][r] = gv[j][r] + w.ld_v0(gv_ext, j, r, R);
        if constexpr (kMaskPad) gv[j][r] = w.keep_col(j, gv[j][r]);
      }
    if constexpr (kMaskPad) {
      if constexpr (kDistBwd) {
#pragma unroll
        for (int r = 0; r < R; ++r) gud[r] = w.grp_below(mreal) ? gud[r] : F(0.f);
      } else {
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
          for (int r = 0; r < R; ++r) gu[m][r] = (m < mreal) ? gu[m][r] : F(0.f);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int j = 0; j < NPL; ++j) g[m][j] = F(0.f);
  w.fence();

  for (int s = G - 1; s >= 0; --s) {
    // ---- undo the V-update of this iteration: v_{s+1} = upd(xᵀ; v_s, u_{s+1}) ----
    F un[M][R];
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int r = 0; r < R; ++r) un[m][r] = w.ld_uni(h.uh, ((s + 1) * M + m) * R + r);
    F bp[R][R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = r; q < R; ++q) {
        F acc = un[0][r] * un[0][q];
#pragma unroll
        for (int m = 1; m < M; ++m) acc = acc + un[m][r] * un[m][q];
        bp[r][q] = acc;
        bp[q][r] = acc;
      }
    F gb[R][R];
    F gup[M][R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < R; ++q) gb[r][q] = F(0.f);
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int r = 0; r < R; ++r) gup[m][r] = F(0.f);
    F gvold[NPL][R];
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      F vold[R], vnew[R], apj[R], gwn[R], gwo[R], gaj[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        vold[r] = w.ld_priv(h.vh, (s * R + r) * NPL + j);
        vnew[r] = w.ld_priv(h.vh, ((s + 1) * R + r) * NPL + j);
        F acc = x[0][j] * un[0][r];
#pragma unroll
        for (int m = 1; m < M; ++m) acc = acc + x[m][j] * un[m][r];
        apj[r] = acc;
        gwn[r] = gv[j][r];
      }
      half_bwd_row<R, SOLVER, F>(vold, vnew, apj, bp, gwn, gwo, gaj, gb, eps);
#pragma unroll
      for (int r = 0; r < R; ++r) gvold[j][r] = gwo[r];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        F acc = g[m][j];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          acc = acc + un[m][r] * gaj[r];
          gup[m][r] = gup[m][r] + x[m][j] * gaj[r];
        }
        g[m][j] = acc;
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < R; ++q) gb[r][q] = w.sum(gb[r][q]);
    F und[R];    // (kDistRows) u_{s+1} of this lane group's row
    if constexpr (kDistBwd) {
#pragma unroll
      for (int r = 0; r < R; ++r) und[r] = w.ld_grp(h.uh, (s + 1) * M * R + r, R);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        F col[M];
#pragma unroll
        for (int m = 0; m < M; ++m) col[m] = gup[m][r];
        F acc = gud[r] + w.sum8_dist(col);
#pragma unroll
        for (int q = 0; q < R; ++q) acc = acc + und[q] * (gb[q][r] + gb[r][q]);
        gud[r] = acc;
      }
    } else {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      F col[M];
#pragma unroll
      for (int m = 0; m < M; ++m) col[m] = gup[m][r];
      sum_all<M, W, F>(w, col);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        F acc = gu[m][r] + col[m];
#pragma unroll
        for (int q = 0; q < R; ++q) acc = acc + un[m][q] * (gb[q][r] + gb[r][q]);
        gu[m][r] = acc;
      }
    }
    }

    // ---- undo the U-update: u_{s+1} = upd(x; u_s, v_s) ----
    F bs[R][R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < R; ++q) bs[r][q] = w.ld_uni(h.bh, (s * R + r) * R + q);
    F ga[M][R];
    F gbu[R][R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < R; ++q) gbu[r][q] = F(0.f);
    if constexpr (kDistBwd) {
      // one row per lane group: the reverse half-step once instead of eight times on uniform values; the rows'
      // contributions to dL/db are added over the groups in a fixed tree (the uniform form adds them row by row: the
      // results differ by rounding only, both orders are deterministic)
      F uold[R], as[R], gwn[R], gwo[R], gam[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        uold[r] = w.ld_grp(h.uh, s * M * R + r, R);
        as[r] = w.ld_grp(h.ah, s * M * R + r, R);
        gwn[r] = gud[r];
      }
      half_bwd_row<R, SOLVER, F>(uold, und, as, bs, gwn, gwo, gam, gbu, eps);
#pragma unroll
      for (int r = 0; r < R; ++r) gud[r] = gwo[r];  // gradient handed to u_s
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < R; ++q) gbu[r][q] = w.grp_sum(gbu[r][q]);
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) ga[m][r] = w.grp_take(gam[r], m);
    } else {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      F uold[R], as[R], gwn[R], gwo[R], gam[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        uold[r] = w.ld_uni(h.uh, (s * M + m) * R + r);
        as[r] = w.ld_uni(h.ah, (s * M + m) * R + r);
        gwn[r] = gu[m][r];
      }
      half_bwd_row<R, SOLVER, F>(uold, un[m], as, bs, gwn, gwo, gam, gbu, eps);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        ga[m][r] = gam[r];
        gu[m][r] = gwo[r];  // gradient handed to u_s
      }
    }
    }
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      F vold[R];
#pragma unroll
      for (int r = 0; r < R; ++r) vold[r] = w.ld_priv(h.vh, (s * R + r) * NPL + j);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        F acc = g[m][j];
#pragma unroll
        for (int r = 0; r < R; ++r) acc = acc + ga[m][r] * vold[r];
        g[m][j] = acc;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        F acc = gvold[j][r];
#pragma unroll
        for (int m = 0; m < M; ++m) acc = acc + x[m][j] * ga[m][r];
#pragma unroll
        for (int q = 0; q < R; ++q) acc = acc + vold[q] * (gbu[q][r] + gbu[r][q]);
        gv[j][r] = acc;
      }
    }
  }
}

}  // namespace fz
