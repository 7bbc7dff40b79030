// nmf_cf_fwd.hip — forward of the FactMixer core on channels-first tensors: shifted-window matricize → NMF →
// inverse matricize in ONE kernel per window (hot shape: head_dim 8, patch 8x8x8).  The kernels and their launcher; the
// entry points are in nmf_cf.hip, the backward in nmf_cf_bwd.hip and nmf_cf_gram.hip.
//
// Replaces the chain SWMatricize.forward → NMF.forward → SWMatricize.inverse_forward
// (factorizer/factorizer.py:41-50; operations.py:417-434; matrix_factorization.py:514-546):
// the (W·B·h, G, 8, 512) matricized tensors are never materialised.  A wave gathers its 8x512
// matrix straight from t (B, C, D, H, W) with the window's cyclic shift, runs the per-wave NMF
// program of nmf_core.h with X in registers, and scatters u vᵀ back to the same voxels of the
// averaged output a:  window 0 stores (0 + z_0), window w>0 adds z_w, the last window divides by
// the number of windows — the reference's ((0.0 + z_0) + z_1 + …) / W order (operations.py:426-433).
// Windows are separate launches on one stream, so the accumulation is deterministic.
//
// Rank 1, exactly two windows, W % 64 == 0, W-axis shifts ≡ 0 (mod 4) (fz_nmf_cf_factors_supported — the README model's
// stages 0 and 1): the first window does not write u vᵀ (one tensor) for the second to read back.  It writes its FACTORS —
// v as a (B, heads, D, H, W) fp32 field at the true voxel positions (one eighth of t), u as 8 floats per patch — and the
// second window rebuilds (0 + u·v) per 16-byte chunk from one float4 of v and the u of the first window's patch the chunk
// lies in (cache resident: 1 MB at stage 0).  2 + 3 tensor passes become 1.13 + 2.13, the result keeps its bits: the product
// is rounded before the add (cf_first_window, nmf_cf.h), bf16 storage rounds the first window's value once as the stored
// running sum was.  Both are forms (template parameter FORM) of the line-coalesced forward kernel.
//
// Lane map: lane l = (p0 & 3 = l>>4, p1 = (l>>1)&7, half = l&1); for every channel dd and
// p0-group jp the lane moves one 16-byte vector = voxels p2 = 4·half..4·half+3 of patch row
// (p0 = 4·jp + (l>>4), p1).  Column index of local element (jp, e): n = (p0·8 + p1)·8 + 4·half + e.
#include "nmf_cf.h"

namespace fz {

// direct gather: one wave per patch, loads and stores with the patch-owner map
template <int R, int SOLVER, typename AT>
__global__ __launch_bounds__(1024) void nmf_cf_fwd_kernel(const AT* __restrict__ t, const float* __restrict__ u0,
                                                          const float* __restrict__ v0, AT* __restrict__ out,
                                                          CfGeom q, int64_t nmat, int T, float eps, int xcd_remap) {
  const int lane = threadIdx.x & 63;
  const int64_t mat = cf_logical_block(xcd_remap) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (mat >= nmat) return;
  CfWave w{lane};
  CfAddr a;
  cf_decode(q, mat, lane, a);
  float x[8][8], u[8][R], v[8][R];
  cf_load(t, a, x);
  nmf_forward_wave<8, 8, R, SOLVER>(w, u0, v0, x, u, v, 8, T, eps);
  const float dv = (float)q.divisor;
  const bool dv_pow2 = cf_pow2(dv);
#pragma unroll
  for (int dd = 0; dd < 8; ++dd)
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
      AT* p = out + a.base + dd * a.V + a.off[jp];
      float4 o;
      if (q.accumulate) {
        o = ld4(p);
        o.x += x[dd][jp * 4 + 0]; o.y += x[dd][jp * 4 + 1]; o.z += x[dd][jp * 4 + 2]; o.w += x[dd][jp * 4 + 3];
      } else {
        o = make_float4(0.0f + x[dd][jp * 4 + 0], 0.0f + x[dd][jp * 4 + 1], 0.0f + x[dd][jp * 4 + 2],
                        0.0f + x[dd][jp * 4 + 3]);
      }
      if (q.divisor > 1) o = cf_divide4(o, dv, dv_pow2);
      st4(p, o);
    }
}

// One tile (WPB patches along W) of one window of the forward.
// FORM (nmf_cf.h): CF_STORE_FACTORS writes the window's rank-1 factors — v as a (B, heads, D, H, W) fp32 field at the true
// voxel positions, u as 8 floats per patch — and nothing else; CF_FROM_FACTORS rebuilds the previous window's value of every
// voxel from them instead of reading the running sum.  Both give the bits of two CF_PLAIN launches.
template <int R, int SOLVER, int WPB, bool HALF, typename AT, int FORM>
__device__ __forceinline__ void cf_fwd_tile_body(const AT* __restrict__ t, const float* __restrict__ u0,
                                                 const float* __restrict__ v0, AT* __restrict__ out, float* vfac, float* ufac,
                                                 const CfGeom& q, const CfTileId& id, int T, float eps, float* S) {
  static_assert(FORM == CF_PLAIN || (R == 1 && WPB == 8 && !HALF), "the factor forms: rank 1, 8 patches per workgroup, W-axis shifts = 0 (mod 4)");
  using TL = CfTile<WPB>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t base, V;
  unsigned off[2], off2[2];
  int lidx[2];
  cf_tile_decode<WPB>(q, id, tid, base, V, off, lidx, off2);
  const int own0 = cf_owner_lidx<WPB>(lane, wave, 0), own1 = cf_owner_lidx<WPB>(lane, wave, 1);

  // (the eight-plane load and the staged store at the end are spelled out, here and in cf_bwd_tile_body: with a shared
  // __forceinline__ load helper 62 of the family's 160 kernels compiled to other machine code, with a store helper as well 118
  // — profiles/nmf_cf_split.md)
  float x[8][8];
#pragma unroll
  for (int dd = 0; dd < 8; ++dd)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float4 v = cf_ld4<HALF>(t + base + dd * V, off[k], off2[k]);
      x[dd][k * 4 + 0] = v.x; x[dd][k * 4 + 1] = v.y; x[dd][k * 4 + 2] = v.z; x[dd][k * 4 + 3] = v.w;
    }
  cf_to_owner<WPB>(S, lidx, own0, own1, x);

  CfWave w{lane};
  float u[8][R], v[8][R];
  nmf_forward_wave<8, 8, R, SOLVER>(w, u0, v0, x, u, v, 8, T, eps);

  const int64_t bh = (int64_t)id.b * q.h + id.hh;             // (sample, head): one plane of vfac, G0·G1·G2 rows of ufac
  const int64_t vol = (int64_t)q.D * q.H * q.W;
  if constexpr (FORM == CF_STORE_FACTORS) {
    // v through one plane of the exchange (the column layout of one x[dd] row), stored with the coalesced map; u (wave-uniform)
    // by one lane
    *reinterpret_cast<float4*>(S + own0) = make_float4(v[0][0], v[1][0], v[2][0], v[3][0]);
    *reinterpret_cast<float4*>(S + own1) = make_float4(v[4][0], v[5][0], v[6][0], v[7][0]);
    __syncthreads();
    float* vp = vfac + bh * vol;
#pragma unroll
    for (int k = 0; k < 2; ++k) st4(cf_at(vp, off[k]), *reinterpret_cast<const float4*>(S + lidx[k]));
    if (lane == 0) {
      float* up = ufac + ((((bh * q.G0 + id.g0) * q.G1 + id.g1) * q.G2 + id.gq * WPB + wave) << 3);
      st4(up, make_float4(u[0][0], u[1][0], u[2][0], u[3][0]));
      st4(up + 4, make_float4(u[4][0], u[5][0], u[6][0], u[7][0]));
    }
    return;
  }

  // owner → coalesced, then the (read-modify-)write of the running window average; all loads of
  // the running sum are issued at once (one exposed round trip)
  const float dv = (float)q.divisor;
  const bool dv_pow2 = cf_pow2(dv);
  // (the plane base back in a scalar register pair: after the wave program the compiler otherwise carries it in vector
  // registers and every epilogue access pays a 64-bit vector address)
  asm volatile("" : "+s"(base));
  float4 old[8][2];
  float4 pv[2];      // CF_FROM_FACTORS: the previous window's v at this thread's two chunks,
  float pu[2][8];    // and the u of the patch of that window each chunk lies in
  if constexpr (FORM == CF_FROM_FACTORS) {
    const float* vp = vfac + bh * vol;
    const float* up = ufac + ((bh * q.G0 * q.G1 * q.G2) << 3);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      pv[k] = ld4(cf_at(vp, off[k]));
      const float* pk = up + (cf_prev_patch<WPB>(q, id, tid, k) << 3);
      const float4 a = ld4(pk), b = ld4(pk + 4);
      pu[k][0] = a.x; pu[k][1] = a.y; pu[k][2] = a.z; pu[k][3] = a.w;
      pu[k][4] = b.x; pu[k][5] = b.y; pu[k][6] = b.z; pu[k][7] = b.w;
    }
  } else if (q.accumulate) {
#pragma unroll
    for (int dd = 0; dd < 8; ++dd)
#pragma unroll
      for (int k = 0; k < 2; ++k) old[dd][k] = cf_ld4<HALF>(out + base + dd * V, off[k], off2[k]);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      *reinterpret_cast<float4*>(S + c * 64 * TL::LW + own0) =
          make_float4(x[2 * s + c][0], x[2 * s + c][1], x[2 * s + c][2], x[2 * s + c][3]);
      *reinterpret_cast<float4*>(S + c * 64 * TL::LW + own1) =
          make_float4(x[2 * s + c][4], x[2 * s + c][5], x[2 * s + c][6], x[2 * s + c][7]);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float4 z = *reinterpret_cast<const float4*>(S + c * 64 * TL::LW + lidx[k]);
        float4 o;
        if constexpr (FORM == CF_FROM_FACTORS) {
          o = cf_first_window<AT>(pu[k][2 * s + c], pv[k]);
          o.x += z.x; o.y += z.y; o.z += z.z; o.w += z.w;
        } else if (q.accumulate) {
          o = old[2 * s + c][k];
          o.x += z.x; o.y += z.y; o.z += z.z; o.w += z.w;
        } else {
          o = make_float4(0.0f + z.x, 0.0f + z.y, 0.0f + z.z, 0.0f + z.w);
        }
        if (q.divisor > 1) o = cf_divide4(o, dv, dv_pow2);
        cf_st4<HALF>(out + base + (2 * s + c) * V, off[k], off2[k], o);
      }
    __syncthreads();
  }
}

template <int R, int SOLVER, int WPB, bool HALF, typename AT, int FORM>
// (second launch-bounds argument = minimum WAVES PER SIMD in HIP, not workgroups per CU: 8 capped the one-patch variant
// at 64 VGPRs — 170 spilled registers)
// (rank 2 needs more than the 128 registers of four waves per SIMD: two — NO variant may spill to scratch, see nmf_pcf.hip)
__global__ __launch_bounds__(WPB * 64, (WPB == 8 || R >= 2) ? 2 : 4) void nmf_cf_fwd_tile_kernel(const AT* __restrict__ t,
                                                                   const float* __restrict__ u0,
                                                                   const float* __restrict__ v0,
                                                                   AT* __restrict__ out, float* vfac, float* ufac,
                                                                   CfGeom q, int T, float eps, int xcd_remap) {
  extern __shared__ __attribute__((aligned(16))) float fz_lds_tile[];
  cf_fwd_tile_body<R, SOLVER, WPB, HALF, AT, FORM>(t, u0, v0, out, vfac, ufac, q, cf_tile_id<WPB>(q, cf_logical_block(xcd_remap)), T, eps,
                                                   fz_lds_tile);
}

// One launch: the line-coalesced kernel in the form asked for, or the direct-gather kernel where the tile does not apply.
template <typename AT>
int cf_fwd_launch(const AT* t, const float* u0, const float* v0, AT* out, float* vfac, float* ufac, const CfLaunch& a, int form,
                  int R, int T, int solver, float eps) {
  const CfGeom& q = a.q;
  const int tile = FZ_KNOB("FZ_CF_TILE").set ? FZ_KNOB("FZ_CF_TILE").val : 1;   // probe builds: 0 = the direct-gather kernels
  const bool half = (q.s2 % 4) != 0;  // W-axis shift ≡ 2 (mod 4): only the line-coalesced kernels handle it
  // line-coalesced kernel: WPB patches along W per workgroup.  8 patches per workgroup, two
  // workgroups per CU out of phase: 0.524 ms vs 0.554 (16) vs 0.747 (direct gather) at stage 0
  const int twpb = (q.G2 % 8) == 0 ? 8 : ((q.G2 % 4) == 0 ? 4 : 1);
#define FZ_CF_TILE(RR, WW, HH, FF, SS)                                                                                  \
  hipLaunchKernelGGL((nmf_cf_fwd_tile_kernel<RR, SS, WW, HH, AT, FF>), dim3((unsigned)(a.nmat / WW)), dim3(64 * WW),    \
                     CfTile<WW>::STAGE_FLOATS * (int)sizeof(float), a.st, t, u0, v0, out, vfac, ufac, q, T, eps, a.xr)
#define FZ_CF_TILE_W(RR, SS)                                                                                            \
  do {                                                                                                                  \
    if (half) { if (twpb == 8) FZ_CF_TILE(RR, 8, true, CF_PLAIN, SS); else if (twpb == 4) FZ_CF_TILE(RR, 4, true, CF_PLAIN, SS); else FZ_CF_TILE(RR, 1, true, CF_PLAIN, SS); } \
    else FZ_CF_TILE(RR, 8, false, CF_PLAIN, SS);                                                                        \
  } while (0)
  if (form == CF_STORE_FACTORS) {
    FZ_SOLVER_CASES(FZ_CF_TILE, 1, 8, false, CF_STORE_FACTORS);
  } else if (form == CF_FROM_FACTORS) {
    FZ_SOLVER_CASES(FZ_CF_TILE, 1, 8, false, CF_FROM_FACTORS);
  } else if (half || (tile && (q.G2 % 8) == 0)) {
    if (R == 1) { FZ_SOLVER_CASES(FZ_CF_TILE_W, 1); }
    else { FZ_SOLVER_CASES(FZ_CF_TILE_W, 2); }
  } else {
    // measured on MI355X (round-1/2 probe `cf_probe`): a workgroup = one full row of patches along W
    // (up to 16 waves) consumes whole 128-B lines inside one CU: 0.856 -> 0.725 ms at stage 0
    const int wpb = q.G2 < 16 ? q.G2 : 16;
    dim3 grid((unsigned)((a.nmat + wpb - 1) / wpb)), block(64 * wpb);
#define FZ_CF_FWD(RR, SS) hipLaunchKernelGGL((nmf_cf_fwd_kernel<RR, SS, AT>), grid, block, 0, a.st, t, u0, v0, out, q, a.nmat, T, eps, a.xr)
    if (R == 1) { FZ_SOLVER_CASES(FZ_CF_FWD, 1); }
    else { FZ_SOLVER_CASES(FZ_CF_FWD, 2); }
  }
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
template int cf_fwd_launch<float>(const float*, const float*, const float*, float*, float*, float*, const CfLaunch&, int, int, int, int, float);
template int cf_fwd_launch<bf16>(const bf16*, const float*, const float*, bf16*, float*, float*, const CfLaunch&, int, int, int, int, float);

// a = ((0 + u0 v0ᵀ) + u1 v1ᵀ) / 2 from the factors of BOTH windows (two CF_STORE_FACTORS launches), in one pass: what the
// out-projection's kernels rebuild in registers (mlp_chain32.hip, gemm_dw.hip), materialised for a caller that wants the tensor
// after all.  A thread owns one 16-byte chunk of voxels of one (sample, head) — with both W-axis shifts ≡ 0 (mod 4) the four
// voxels lie in one patch of either window — and writes it in the head's eight channel planes.
__global__ __launch_bounds__(256) void nmf_cf_factors_to_tensor_kernel(const float* __restrict__ vf0, const float* __restrict__ uf0,
                                                                       const float* __restrict__ vf1, const float* __restrict__ uf1,
                                                                       float* __restrict__ out, CfGeom q, int64_t nchunk) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nchunk) return;
  const unsigned vol = (unsigned)(q.D * q.H * q.W), per = vol >> 2;
  const int64_t bh = i / per;
  const unsigned vox = (unsigned)(i % per) << 2;
  const int w = (int)(vox % (unsigned)q.W), hh = (int)((vox / (unsigned)q.W) % (unsigned)q.H), d = (int)(vox / (unsigned)(q.W * q.H));
  const int64_t npatch = (int64_t)q.G0 * q.G1 * q.G2;
  const float* up0 = uf0 + ((bh * npatch + cf_voxel_patch(d, hh, w, q.D, q.H, q.W, q.s0, q.s1, q.s2)) << 3);
  const float* up1 = uf1 + ((bh * npatch + cf_voxel_patch(d, hh, w, q.D, q.H, q.W, q.ps0, q.ps1, q.ps2)) << 3);
  const float4 v0 = ld4(vf0 + bh * vol + vox), v1 = ld4(vf1 + bh * vol + vox);
  const float4 a0 = ld4(up0), b0 = ld4(up0 + 4), a1 = ld4(up1), b1 = ld4(up1 + 4);
  const float u0[8] = {a0.x, a0.y, a0.z, a0.w, b0.x, b0.y, b0.z, b0.w};
  const float u1[8] = {a1.x, a1.y, a1.z, a1.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
  for (int dd = 0; dd < 8; ++dd)
    st4(out + (bh * 8 + dd) * vol + vox,
        make_float4(cf_two_window_value(u0[dd], v0.x, u1[dd], v1.x), cf_two_window_value(u0[dd], v0.y, u1[dd], v1.y),
                    cf_two_window_value(u0[dd], v0.z, u1[dd], v1.z), cf_two_window_value(u0[dd], v0.w, u1[dd], v1.w)));
}

int cf_factors_to_tensor_launch(const float* vf0, const float* uf0, const float* vf1, const float* uf1, float* out, const CfLaunch& a) {
  const CfGeom& q = a.q;
  const int64_t nchunk = (int64_t)q.B * q.h * ((int64_t)q.D * q.H * q.W / 4);
  if (nchunk == 0) return FZ_OK;
  hipLaunchKernelGGL(nmf_cf_factors_to_tensor_kernel, dim3((unsigned)((nchunk + 255) / 256)), dim3(256), 0, a.st, vf0, uf0, vf1, uf1,
                     out, q, nchunk);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

}  // namespace fz
