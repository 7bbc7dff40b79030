// outproj_fac.h — the core's output a as an operand that is never stored: what the two C = 32 consumers of a (GEMM 0 of
// gemm_chain_kernel, mlp_chain32.hip; the q operand of gemm_dw_kernel<false>, gemm_dw.hip) share to rebuild their wave tile of a
// from the rank-1 factors that both windows of the forward core left (fz_nmf_cf_fwd_store_factors twice).
//
// Both kernels give a wave 64 consecutive voxels (W % 64 == 0: one half W-row or less, so the wave's (d, h) and with them the
// patch rows of both windows are wave-uniform) and lane (j, h) the channels 2s + h, s < 16, of the voxels 2j, 2j + 1.  Per
// window the wave needs four v planes at its voxels (one float2 per lane and head) and the u rows of the patches it touches
// along W: 8, or 9 when the window's W-axis shift is 4 (mod 8).  The u rows are fetched ONCE per wave — 144 float4 for both
// windows, at most three per lane, one tile ahead like the operand they replace — and reach the lanes through wave-private LDS
// (a region the kernel owns anyway and does not use at that point), de-interleaved so that a lane reads its 16 channels of a
// patch as four 16-byte words.  The value is cf_two_window_value (cf_patch.h): the bits the core's launch pair stores.
#pragma once
#include <string>
#include <type_traits>

#include "cf_patch.h"
#include "gemm_shared.h"   // DropArgs

namespace fz {

struct FacArgs {
  const float* v[2];   // (B, 4, D, H, W) per window: v at the true voxel positions
  const float* u[2];   // (B · 4 · D/8 · H/8 · W/8, 8) per window: u per patch
  int D, H, W;
  int s[2][3];         // the windows' shifts, normalised to [0, size)
};
template <class... X>
constexpr bool is_fac_v = (std::is_same<X, FacArgs>::value || ... || false);
__device__ __forceinline__ DropArgs drop_of(const FacArgs&) { return DropArgs{}; }
__device__ __forceinline__ FacArgs fac_of() { return FacArgs{}; }
__device__ __forceinline__ FacArgs fac_of(const DropArgs&) { return FacArgs{}; }
__device__ __forceinline__ FacArgs fac_of(const FacArgs& f) { return f; }

// host: checks a caller's fz_outproj_fac (include/factorizer_hip.h) against the launch's voxel count and fills the kernel's argument
static int fac_args(const fz_outproj_fac* d, int64_t V, const char* who, FacArgs& f) {
  auto bad = [&](int code, const char* what) { return fail(code, (std::string(who) + ": " + what).c_str()); };
  if (!d->v[0] || !d->v[1] || !d->u[0] || !d->u[1]) return bad(FZ_E_ARG, "null factor pointer (v[0..1], u[0..1])");
  const int D = d->dims[0], H = d->dims[1], W = d->dims[2];
  if (d->heads != 4) return bad(FZ_E_UNSUPPORTED, "needs heads == 4 (C = 32, head_dim 8)");
  if (D < 8 || H < 8 || W < 64 || (D % 8) || (H % 8) || (W % 64) || (int64_t)D * H * W != V)
    return bad(FZ_E_UNSUPPORTED, "needs dims multiples of 8, W % 64 == 0, D H W == V");
  f.D = D; f.H = H; f.W = W;
  const int S[3] = {D, H, W};
  for (int w = 0; w < 2; ++w) {
    f.v[w] = d->v[w]; f.u[w] = d->u[w];
    for (int i = 0; i < 3; ++i) {
      int s = d->shift[3 * w + i] % S[i];
      f.s[w][i] = s < 0 ? s + S[i] : s;
    }
    if (f.s[w][2] % 4) return bad(FZ_E_UNSUPPORTED, "needs W-axis shifts that are multiples of 4");
  }
  return FZ_OK;
}

constexpr int kFacRow = 36;              // floats of one patch's 32 channels in the staging area: 4 banks on per patch (16-byte reads)
constexpr int kFacWin = 9 * kFacRow;      // one window: up to 9 patches
constexpr int kFacLds = 2 * kFacWin;      // floats of wave-private LDS that fac_build uses

struct FacTile {
  float4 ur[3];       // staging items lane, lane + 64, lane + 128 (< 144): (window, patch, head, half) -> four u
  float2 vv[2][4];    // v of both windows at this lane's two voxels, four heads
};

// the loads of the wave tile that starts at voxel n0 (wave-uniform, a multiple of 64) of sample b
__device__ __forceinline__ void fac_fetch(const FacArgs& f, int b, unsigned n0, int lane, FacTile& t) {
  const unsigned vol = (unsigned)(f.D * f.H * f.W);
  const int w0 = (int)(n0 % (unsigned)f.W), hh = (int)((n0 / (unsigned)f.W) % (unsigned)f.H), d = (int)(n0 / (unsigned)(f.W * f.H));
  const int G1 = f.H >> 3, G2 = f.W >> 3;
  const unsigned npatch = (unsigned)((f.D >> 3) * G1 * G2);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int id = lane + 64 * k;
    if (id < 144) {
      const int win = id >= 72, rem = id - 72 * win, i = rem >> 3, head = (rem >> 1) & 3, half = rem & 1;
      // the row of patches the wave's voxels lie in, and the i-th patch along W from the first voxel's
      const unsigned row = cf_voxel_patch(d, hh, w0, f.D, f.H, f.W, f.s[win][0], f.s[win][1], f.s[win][2]);
      const int g2 = (int)(row % (unsigned)G2);
      int g2i = g2 + i; if (g2i >= G2) g2i -= G2;
      const int64_t patch = (int64_t)(b * 4 + head) * npatch + (row - (unsigned)g2 + (unsigned)g2i);
      t.ur[k] = *reinterpret_cast<const float4*>(f.u[win] + (patch << 3) + 4 * half);
    } else {
      t.ur[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  const unsigned vo = n0 + 2u * (unsigned)(lane & 31);
#pragma unroll
  for (int win = 0; win < 2; ++win)
#pragma unroll
    for (int head = 0; head < 4; ++head)
      t.vv[win][head] = *reinterpret_cast<const float2*>(f.v[win] + (int64_t)(b * 4 + head) * vol + vo);
}

// bv[s][q] = a[channel 2s + h][voxel 2j + q] of the fetched tile; S: kFacLds floats of LDS that only this wave touches
__device__ __forceinline__ void fac_build(const FacArgs& f, const FacTile& t, float* S, int lane, float (&bv)[16][2]) {
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int id = lane + 64 * k;
    if (id < 144) {
      const int win = id >= 72, rem = id - 72 * win, i = rem >> 3, head = (rem >> 1) & 3, half = rem & 1;
      // channels 8 head + 4 half + e = 2s + parity: e = 0, 2 -> parity 0, rows s0, s0 + 1; e = 1, 3 -> parity 1
      float* dst = S + win * kFacWin + i * kFacRow + head * 4 + half * 2;
      *reinterpret_cast<float2*>(dst) = make_float2(t.ur[k].x, t.ur[k].z);
      *reinterpret_cast<float2*>(dst + 16) = make_float2(t.ur[k].y, t.ur[k].w);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  float u[2][16];
#pragma unroll
  for (int win = 0; win < 2; ++win) {
    const int i = ((f.s[win][2] & 7) + 2 * j) >> 3;   // this lane's patch along W, counted from the first voxel's
    const float* src = S + win * kFacWin + i * kFacRow + h * 16;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float4 x = *reinterpret_cast<const float4*>(src + 4 * c);
      u[win][4 * c + 0] = x.x; u[win][4 * c + 1] = x.y; u[win][4 * c + 2] = x.z; u[win][4 * c + 3] = x.w;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const float2 a = t.vv[0][s >> 2], b = t.vv[1][s >> 2];
    bv[s][0] = cf_two_window_value(u[0][s], a.x, u[1][s], b.x);
    bv[s][1] = cf_two_window_value(u[0][s], a.y, u[1][s], b.y);
  }
}

}  // namespace fz
