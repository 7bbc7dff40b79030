// upcat_bwd.hip — backward of the full-resolution decoder node in ONE pass over g = dL/dy (the forward is upcat.hip):
//   g_skip[c][v] = Σ_m W_a[m][c]·g[m][v]                              (written)
//   g_deep[k][n] = Σ_{m,tap} Wc[k][m][tap]·g[m][fine(n,tap)]          (written; Wc from fz_upcat_compose)
//   dW_a[m][c] = Σ_v g[m][v]·skip[c][v],  Σ_v g[m],  Gt[k][m][tap] = Σ_n deep[k][n]·g[m][fine(n,tap)]   (partial rows)
// Replaces three launches that each read g (gemm_dw on the skip half, the k2s2 correlation GEMM, the k2s2 weight-gradient
// partial kernel): 3.5 U of traffic (g, skip, deep in; g_skip, g_deep out; U = one full-resolution activation tensor) instead
// of 5.5 U.  fp32 storage, 32 adapter outputs, 32 skip channels, 64 deep channels, fine W % 64 == 0.
//
// Mapping.  One PERSISTENT workgroup of 256 threads per CU, one wave per SIMD.  A workgroup tile is one segment of 32 coarse
// voxels of one coarse row (d, h); its four waves take the four fine rows (2d + td, 2h + th), wave = 2 td + th, of that
// segment: 64 fine voxels each.  Lane (j, half) holds the fine voxels 2j, 2j + 1 of its row — taps tw = 0, 1 of coarse voxel
// j, as in the forward — so (td, th) is fixed per wave for the whole walk and the wave's weights (W_a and its two taps of Wc,
// three bf16 levels each) stay in registers.  All products are six exact bf16 products of three-level splits (gemm_bx.h).
//   channel contractions (g_skip, g_deep): g is the column operand straight from its load registers (voxel on the lane axis);
//     the four waves' partial g_deep tiles (64 x 32) meet in LDS and are added in wave order 0..3 behind one barrier.
//   voxel reductions (dW_a, Gt): g and skip tiles go through wave-private LDS and come back with the channel on the lane
//     axis (as gemm_dw.hip), the shared deep tile is staged once per workgroup; the sums stay in registers across tiles.
//     A wave's Gt share is its own two taps (td, th, 0 / 1): no other wave adds to them.
// Partial rows: Gt one row per workgroup (added by a FK_ROWS finish job), dW_a | Σg one kDwRow row per WAVE (FK_DW job).
#include "gemm_bx.h"
#include "finish.h"

namespace fz {

struct UpcatBwdArgs {
  const float* g;      // (B, 32, 2D, 2H, 2W)
  const float* skip;   // (B, 32, 2D, 2H, 2W)
  const float* deep;   // (B, 64, D, H, W)
  const float* wa;     // W_a[m][c]: (32, lda)
  const float* wc;     // Wc[k][m][tap]: (64, 32, 8)
  float* g_skip;       // (B, 32, 2D, 2H, 2W)
  float* g_deep;       // (B, 64, D, H, W)
  float* part_gt;      // [gridDim.x][kUbGt]
  float* part_dw;      // [gridDim.x * 4][kDwRow]
  int lda;
  int B, D, H, W;      // coarse extent
};

constexpr int kUbGt = 64 * 32 * 8;             // floats of one Gt row
constexpr int kUbTS = 36;                      // LDS row stride (floats): 16-byte rows, conflict-free 16-byte reads down the rows
constexpr int kUbTile = 2 * 32 * kUbTS;        // one wave's g (or skip) tile: [parity q][channel][coarse voxel]
constexpr int kUbDeep = 64 * kUbTS;            // the workgroup's deep tile [k][coarse voxel]
constexpr int kUbPart = 64 * 32;               // one wave's partial g_deep tile [k][coarse voxel]
constexpr int kUbLds = (4 * 2 * kUbTile + kUbDeep + 4 * kUbPart) * (int)sizeof(float);   // 115 712 B
constexpr int kUbMaxWgs = 256;                 // one per CU

__global__ __launch_bounds__(256, 1) void upcat_bwd_kernel(UpcatBwdArgs p, unsigned ntiles) {
  extern __shared__ __attribute__((aligned(16))) float fz_lds_ub[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int j = lane & 31, hk = lane >> 5;
  const int td = wave >> 1, th = wave & 1;
  float* Gl = fz_lds_ub + wave * 2 * kUbTile;
  float* Sl = Gl + kUbTile;
  float* Dl = fz_lds_ub + 4 * 2 * kUbTile;
  float* Pl = Dl + kUbDeep;
  const int Wf = 2 * p.W, Hf = 2 * p.H;
  const int64_t Vc = (int64_t)p.D * p.H * p.W, Vf = 8 * Vc;
  const unsigned nseg = (unsigned)p.W / 32u;

  // ---- the wave's weights -> three bf16 levels -> registers (once) ----
  bx8 wsk[2][3];          // row operand of g_skip: A[c = j][m = 16 g + 8 hk + e] = W_a[m][c]
  bx8 wdp[2][2][2][3];    // row operand of g_deep, tap (td, th, q): A[k = 32 mb + j][m = 16 g + 8 hk + e] = Wc[k][m][tap]
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    float a8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a8[e] = p.wa[(int64_t)(16 * g + 8 * hk + e) * p.lda + j];
    bx_split<3>(a8, wsk[g]);
  }
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        float a8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a8[e] = p.wc[((32 * mb + j) * 32 + 16 * g + 8 * hk + e) * 8 + td * 4 + th * 2 + q];
        bx_split<3>(a8, wdp[q][mb][g]);
      }

  // ---- sums carried across tiles ----
  f32x16 gta[2][2];   // Gt[k = 32 mb + row][m = j][tap (td, th, q)]
  f32x16 dwa;         // dW_a[m = row][c = j]
  float db = 0.f;     // Σ g[m = j] over this lane half's voxels
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    dwa[r] = 0.f;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int q = 0; q < 2; ++q) gta[mb][q][r] = 0.f;
  }

  // tile -> (sample, fine voxel of the wave's row segment, coarse voxel of the segment)
  auto locate = [&](unsigned t, unsigned& b, int64_t& f0, int64_t& n0) {
    const unsigned seg = t % nseg, row = t / nseg;
    const unsigned h = row % (unsigned)p.H, r2 = row / (unsigned)p.H;
    const unsigned d = r2 % (unsigned)p.D;
    b = r2 / (unsigned)p.D;
    f0 = ((int64_t)(2 * d + td) * Hf + (2 * h + th)) * Wf + 64 * seg;
    n0 = ((int64_t)d * p.H + h) * p.W + 32 * seg;
  };

  // operand registers of one tile: g and skip (channel 16 g + 8 hk + e, the lane's two voxels), a quarter of the deep tile
  float gv[2][8][2], sv[2][8][2], dv[2][4];
  auto fetch = [&](unsigned t) {
    unsigned b;
    int64_t f0, n0;
    locate(t, b, f0, n0);
    const float* gp = p.g + ((int64_t)b * 32 + 8 * hk) * Vf + f0 + 2 * j;
    const float* sp = p.skip + ((int64_t)b * 32 + 8 * hk) * Vf + f0 + 2 * j;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) vload<2>(gp + (int64_t)(16 * g + e) * Vf, gv[g][e]);
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) vload<2>(sp + (int64_t)(16 * g + e) * Vf, sv[g][e]);
    const float* dp = p.deep + ((int64_t)b * 64 + 16 * wave + (lane >> 3)) * Vc + n0 + 4 * (lane & 7);
#pragma unroll
    for (int i = 0; i < 2; ++i) vload<4>(dp + (int64_t)(8 * i) * Vc, dv[i]);
  };

  unsigned tile = blockIdx.x;
  fetch(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    unsigned b;
    int64_t f0, n0;
    locate(tile, b, f0, n0);

    // ---- tiles -> LDS: g and skip de-interleaved by voxel parity [q][channel][j], the deep quarter [k][n] ----
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int o = (q * 32 + 16 * g + 8 * hk + e) * kUbTS + j;
          Gl[o] = gv[g][e][q];
          Sl[o] = sv[g][e][q];
        }
#pragma unroll
    for (int i = 0; i < 2; ++i)
      *reinterpret_cast<float4*>(Dl + (16 * wave + 8 * i + (lane >> 3)) * kUbTS + 4 * (lane & 7)) =
          make_float4(dv[i][0], dv[i][1], dv[i][2], dv[i][3]);
    // column operand of the channel contractions: B[m = 8 hk + e of group g][voxel 2j + q]
    bx8 bs[2][2][3];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        float x8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x8[e] = gv[g][e][q];
        bx_split<3>(x8, bs[g][q]);
      }
    // the next tile's operands are in flight during everything below (the last tile re-requests itself: no branch round a load)
    fetch(tile + gridDim.x < ntiles ? tile + gridDim.x : tile);

    // ---- g_skip = W_aᵀ g ----
    {
      f32x16 acc[2];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int q = 0; q < 2; ++q) bx_mfma<3, 3>(acc[q], wsk[g], bs[g][q]);
      float* yp = p.g_skip + ((int64_t)b * 32 + 4 * hk) * Vf + f0 + 2 * j;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v[2] = {acc[0][r], acc[1][r]};
        vstore<2>(yp + (int64_t)((r & 3) + 8 * (r >> 2)) * Vf, v);
      }
    }
    // ---- this wave's part of g_deep: its taps (td, th, 0 / 1) of Wc on its fine row ----
    {
      f32x16 ad[2];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) ad[mb][r] = 0.f;
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int q = 0; q < 2; ++q) bx_mfma<3, 3>(ad[mb], wdp[q][mb][g], bs[g][q]);
      float* pw = Pl + wave * kUbPart;
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) pw[(32 * mb + (r & 3) + 8 * (r >> 2) + 4 * hk) * 32 + j] = ad[mb][r];
    }
    __syncthreads();   // the deep tile and the four partial g_deep tiles are complete

    // ---- voxel reductions, channel on the lane axis: element e of lane half hk = coarse voxel 16 kg + 8 hk + e ----
    {
      bx8 dsp[2][2][3];   // deep as the row operand of Gt: A[k = 32 mb + j][n]
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int kg = 0; kg < 2; ++kg) {
          float d8[8];
          vload<8>(Dl + (32 * mb + j) * kUbTS + 16 * kg + 8 * hk, d8);
          bx_split<3>(d8, dsp[mb][kg]);
        }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int q = kk >> 1, kg = kk & 1;
        float g8[8], s8[8];
        vload<8>(Gl + (q * 32 + j) * kUbTS + 16 * kg + 8 * hk, g8);
        vload<8>(Sl + (q * 32 + j) * kUbTS + 16 * kg + 8 * hk, s8);
        bx8 ga[3], sb[3];
        bx_split<3>(g8, ga);
        bx_split<3>(s8, sb);
        bx_mfma<3, 3>(dwa, ga, sb);                       // dW_a[m][c] += g[m][v]·skip[c][v]
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) bx_mfma<3, 3>(gta[mb][q], dsp[mb][kg], ga);   // Gt[k][m][q] += deep[k][n]·g[m][2n + q]
        db += ((g8[0] + g8[1]) + (g8[2] + g8[3])) + ((g8[4] + g8[5]) + (g8[6] + g8[7]));
      }
    }
    // ---- g_deep: the four partial tiles added in wave order, 8 coarse voxels of one channel per thread ----
    {
      const int k = (int)threadIdx.x >> 2, n8 = 8 * ((int)threadIdx.x & 3);
      float* yp = p.g_deep + ((int64_t)b * 64 + k) * Vc + n0 + n8;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float* pp = Pl + k * 32 + n8 + 4 * i;
        const float4 a0 = *reinterpret_cast<const float4*>(pp), a1 = *reinterpret_cast<const float4*>(pp + kUbPart);
        const float4 a2 = *reinterpret_cast<const float4*>(pp + 2 * kUbPart), a3 = *reinterpret_cast<const float4*>(pp + 3 * kUbPart);
        *reinterpret_cast<float4*>(yp + 4 * i) = make_float4(((a0.x + a1.x) + a2.x) + a3.x, ((a0.y + a1.y) + a2.y) + a3.y,
                                                             ((a0.z + a1.z) + a2.z) + a3.z, ((a0.w + a1.w) + a2.w) + a3.w);
      }
    }
    __syncthreads();   // before the next tile overwrites the deep tile and the partial tiles
  }

  // ---- partial rows.  Gt: the wave's two taps of the workgroup row [k][m][tap]; dW_a | Σg: one row per wave ----
  float* gr = p.part_gt + (int64_t)blockIdx.x * kUbGt + td * 4 + th * 2;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = 32 * mb + (r & 3) + 8 * (r >> 2) + 4 * hk;
      const float v[2] = {gta[mb][0][r], gta[mb][1][r]};
      vstore<2>(gr + (k * 32 + j) * 8, v);
    }
  float* wr = p.part_dw + ((int64_t)blockIdx.x * 4 + wave) * kDwRow;
#pragma unroll
  for (int r = 0; r < 16; ++r) wr[((r & 3) + 8 * (r >> 2) + 4 * hk) * 32 + j] = dwa[r];
  const float dbt = db + __shfl_xor(db, 32, 64);
  if (hk == 0) wr[1024 + j] = dbt;
  wr[1024 + 32 + lane] = 0.f;   // (the LayerNorm slots of a gemm_dw row: read by the finish job, unused here)
}

}  // namespace fz

using namespace fz;

static int64_t upcat_bwd_tiles(int B, int D, int H, int W) { return (int64_t)B * D * H * (W / 32); }

extern "C" int fz_upcat_bwd_supported(int C1, int Cd, int D, int H, int W, int act_dtype) {
  // (coarse extent) segments of 32 coarse = 64 fine voxels along W; fp32 storage only
  return act_dtype == FZ_STORE_F32 && C1 == 32 && Cd == 64 && D >= 1 && H >= 1 && W >= 32 && W % 32 == 0 &&
         (int64_t)64 * D * H * W * 8 * 4 < ((int64_t)1 << 31);
}

static int upcat_bwd_rows(int B, int D, int H, int W) {   // workgroups of the launch = partial rows
  if (B < 1 || D < 1 || H < 1 || W < 32) return 0;
  const int64_t nt = upcat_bwd_tiles(B, D, H, W);
  return (int)(nt < kUbMaxWgs ? nt : kUbMaxWgs);
}

extern "C" int64_t fz_upcat_bwd_workspace_bytes(int B, int D, int H, int W) {
  return (int64_t)upcat_bwd_rows(B, D, H, W) * (kUbGt + 4 * kDwRow) * (int64_t)sizeof(float);
}

extern "C" int fz_upcat_bwd(const void* g, const void* skip, const void* deep, const float* wa, int lda, const float* wc, void* g_skip,
                            void* g_deep, void* workspace, float* gw_a, int ldg, float* gb, float* gt, int B, int C1, int Cd, int D,
                            int H, int W, int act_dtype, fz_stream_t stream) {
  if (!g || !skip || !deep || !wa || !wc || !g_skip || !g_deep || !workspace || !gw_a || !gb || !gt)
    return fail(FZ_E_ARG, "fz_upcat_bwd: null pointer");
  if (act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16) return fail(FZ_E_ARG, "fz_upcat_bwd: act_dtype must be FZ_STORE_F32 or FZ_STORE_BF16");
  if (!fz_upcat_bwd_supported(C1, Cd, D, H, W, act_dtype) || lda < 32 || ldg < 32)
    return fail(FZ_E_UNSUPPORTED, "fz_upcat_bwd: needs fp32 storage, 32 skip / 64 deep channels, 2W % 64 == 0, lda, ldg >= 32");
  if (B < 1) return fail(FZ_E_SHAPE, "fz_upcat_bwd: needs B >= 1");
  if ((((uintptr_t)g | (uintptr_t)skip | (uintptr_t)g_skip) & 7) || (((uintptr_t)deep | (uintptr_t)g_deep | (uintptr_t)workspace) & 15))
    return fail(FZ_E_ARG, "fz_upcat_bwd: g, skip, g_skip must be 8-byte, deep, g_deep, workspace 16-byte aligned");
  const int64_t ntiles = upcat_bwd_tiles(B, D, H, W);
  if (ntiles >= ((int64_t)1 << 30)) return fail(FZ_E_SHAPE, "fz_upcat_bwd: more than 2^30 tiles");
  const int rows = upcat_bwd_rows(B, D, H, W);
  UpcatBwdArgs a;
  a.g = (const float*)g; a.skip = (const float*)skip; a.deep = (const float*)deep; a.wa = wa; a.wc = wc;
  a.g_skip = (float*)g_skip; a.g_deep = (float*)g_deep;
  a.part_gt = (float*)workspace; a.part_dw = a.part_gt + (int64_t)rows * kUbGt;
  a.lda = lda; a.B = B; a.D = D; a.H = H; a.W = W;
  hipStream_t st = (hipStream_t)stream;
  FZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(upcat_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kUbLds));
  hipLaunchKernelGGL(upcat_bwd_kernel, dim3((unsigned)rows), dim3(256), kUbLds, st, a, (unsigned)ntiles);
  FZ_LAUNCH_CHECK();
  // rows added in index order: Gt by a row-sum job, dW_a | Σg by the gemm_dw row job (four rows per workgroup)
  FinishJob fj[2];
  fj[0] = finish_job(FK_ROWS, kUbGt / 32);
  fj[0].u.rows = FinRows{a.part_gt, gt, rows, kUbGt, rows, kUbGt / 32};
  fj[1] = finish_job(FK_DW, kDwRow / 16);
  fj[1].u.dw = FinDw{a.part_dw, nullptr, nullptr, gw_a, gb, nullptr, 4 * rows, ldg};
  return finish_run(fj, 2, st);
}
