// gemm_dw.hip — input gradient and weight gradient of a 32 -> 32 layer in one pass (gemm.hip has the MFMA mapping): gemm_dw_kernel
// and fz_gemm_dw.
#include "gemm_bx.h"       // split-bf16 operand helpers (brings gemm_common.h)
#include "gemm_shared.h"   // half_sum32, DropArgs, kTS, knob_pos
#include "finish.h"        // kDwRow and the job that adds the weight-gradient rows
#include "outproj_fac.h"   // FacArgs, fac_fetch, fac_build: the core's output as the factors of its two windows

namespace fz {

// =================================================================================================
// Input gradient AND weight gradient of a 32 -> 32 layer in one pass (C = 32: in_proj behind LayerNorm, out_proj):
//   y  = Wᵀ g                                   (LNB: then the LayerNorm backward on the accumulators, + gadd)
//   dW = Σ_v g[m][v] · q[k][v],  db = Σ_v g     (LNB: q = LN-normalised x; the affine is applied by the finish kernel)
// Unfused, the weight-gradient launch reads g and q a second time (2 of the 6 resp. 4 plane-sets of the pair).  Both
// MFMA operands of dW come straight from memory in [channel][voxel] order, so each wave parks its g tile and its q
// tile in LDS (stride kTS) and reads them back with the channel on the lane axis — no register transposes.
// Persistent workgroups (two per CU), sums carried in registers across tiles, one wpart row per workgroup.
// FAC (a trailing FacArgs; out_proj, fp32 storage): q is the core's output a, which is not stored — the wave rebuilds its q tile
// from the rank-1 factors of the core's two windows (outproj_fac.h), fetched one tile ahead beside g and staged through the
// wave's Qb rows before the rebuilt rows are written there.
// =================================================================================================
// (kDwRow — floats of one wpart row: dW [32][32] | db [32] | dγ [32] | dβ [32] (LNB) — lives in finish.h)

template <typename AT>
struct DwArgsT {
  const AT* g;        // (B, 32, V) gradient of the layer output
  const AT* q;        // (B, 32, V) layer input (LNB: the LayerNorm input)
  const float* w;     // (32, 32) forward weight W[m][k], row stride ldw
  int ldw;
  const float* stats; // LNB: (B, 2, V)
  const float* ln_g;  // LNB: gamma
  const AT* gadd;     // LNB: (B, 32, V) added to y, or null
  AT* y;              // (B, 32, V)
  float* wpart;       // [gridDim.x][kDwRow]
  int64_t V;
  int B;
};

template <bool LNB, typename AT, typename... DropX>
__global__ __launch_bounds__(256, 2) void gemm_dw_kernel(DwArgsT<AT> p, int ntiles, DropX... dx) {
  constexpr bool FAC = is_fac_v<DropX...>;      // the factor form: one trailing FacArgs
  constexpr bool DROP = sizeof...(DropX) > 0 && !FAC;   // the block-dropout form (one trailing DropArgs): g is read as M0 s0 g
  const DropArgs dr = drop_of(dx...);
  const FacArgs fa = fac_of(dx...);
  static_assert(!FAC || (!LNB && sizeof(AT) == 4), "factors: the out-projection pair, fp32 storage");
  static_assert(kFacLds <= 32 * kTS, "the factor staging area lives in the wave's Qb rows");
  constexpr int NACC = 2;
  constexpr int kWave = 64 * kTS;             // floats of one wave's (Gb | Qb) region
  // BXB (bf16 storage): both GEMMs on the bf16 matrix pipe with fp32-accurate products — the activations are exact bf16
  // terms, the weights and the LayerNorm-normalised input three levels (gemm_bx.h): 12 + 4 (LNB: 12) MFMAs of 32 cycles per
  // tile instead of 32 + 64 fp32 MFMAs; with half the bytes this kernel is matrix-pipe bound otherwise.  fp32 storage: it
  // is HBM-bound on the fp32 MFMAs and keeps them.
  constexpr bool BXB = sizeof(AT) == 2;
  extern __shared__ __attribute__((aligned(16))) float fz_lds_dw[];
  float* As = fz_lds_dw;                      // [16][64] operand order: A[m][k] = W[k][m]  (BXB: [2 groups][3 levels][64] x 16 B)
  float* tB = As + 1536;                      // gamma[32]
  float* red = tB + 32;                       // [4][64]
  float* R = red + 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int l16 = lane & 15, k4 = lane >> 4;
  float* Gb = R + wave * kWave;
  float* Qb = Gb + 32 * kTS;
  const int tiles_per_sample = (int)((p.V + 128 * NACC - 1) / (128 * NACC));

  if constexpr (BXB) {
    if (threadIdx.x < 128) {   // item (group g, lane l): the eight steps 8g + e of the fp32 form, split in three levels
      const int l = threadIdx.x & 63, g = threadIdx.x >> 6;
      float a8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a8[e] = p.w[(int64_t)(2 * (8 * g + e) + (l >> 5)) * p.ldw + (l & 31)];
      bx8 t3[3];
      bx_split<3>(a8, t3);
      bx8* dst = reinterpret_cast<bx8*>(As) + (g * 3) * 64 + l;
      dst[0] = t3[0]; dst[64] = t3[1]; dst[128] = t3[2];
    }
  } else {
  for (int idx = threadIdx.x; idx < 1024; idx += 256) {
    const int l = idx & 63, a = idx >> 6;
    As[idx] = p.w[(int64_t)(2 * a + (l >> 5)) * p.ldw + (l & 31)];   // A[m = l&31][k = 2a + h] = W[k][m]
  }
  }
  if (LNB && threadIdx.x < 32) tB[threadIdx.x] = p.ln_g[threadIdx.x];

  f32x4 dW[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2)
#pragma unroll
      for (int v = 0; v < 4; ++v) dW[a][b2][v] = 0.f;
  f32x16 dWx;                                   // BXB: the 32 x 32 sum as ONE accumulator tile (row = g channel, column = q channel)
#pragma unroll
  for (int r = 0; r < 16; ++r) dWx[r] = 0.f;
  float db[2] = {0.f, 0.f};
  float gln = 0.f;   // threads 0..63 (LNB): running (dγ | dβ) sum of this workgroup's tiles

  int tile = blockIdx.x;
  float bv[16][NACC];
  FacTile ft;   // (FAC) the factors of the NEXT / current q tile
  auto fetch_tile = [&](int t) {
    const int bt = t / tiles_per_sample;
    const int64_t ct = ((int64_t)(t % tiles_per_sample) * 4 + wave) * (32 * NACC) + NACC * j;
    if constexpr (FAC) {
      const int64_t n0 = ((int64_t)(t % tiles_per_sample) * 4 + wave) * (32 * NACC);
      fac_fetch(fa, bt, (unsigned)(n0 < p.V ? n0 : 0), lane, ft);
    }
    const unsigned lo = (unsigned)h * (unsigned)p.V + (unsigned)(ct < p.V ? ct : 0);
    const AT* xb = p.g + (int64_t)bt * 32 * p.V;
#pragma unroll
    for (int s = 0; s < 16; ++s) vload<NACC>(xb + (int64_t)(2 * s) * p.V + lo, bv[s]);
  };
  fetch_tile(tile);
  __syncthreads();

  for (; tile < ntiles; tile += gridDim.x) {
    asm volatile("" ::: "memory");
    const int b = tile / tiles_per_sample;
    const int64_t col_off = ((int64_t)(tile % tiles_per_sample) * 4 + wave) * (32 * NACC) + NACC * j;
    const bool col_ok = col_off < p.V;
    const int64_t nc = col_ok ? col_off : 0;
    const unsigned lane_row = (unsigned)(4 * h) * (unsigned)p.V + (unsigned)nc;
    const unsigned lane_par = (unsigned)h * (unsigned)p.V + (unsigned)nc;
    const int64_t sample = (int64_t)b * 32 * p.V;
    if constexpr (DROP) {   // g_o = M0 s0 g: the input gradient, dW and db all read the operand registers
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const uint32_t dk = drop_bits(dr, 0, b, 32, 2 * s + h, nc);
        bv[s][0] = drop_f(dr, 0, dk, 0, bv[s][0]);
        bv[s][1] = drop_f(dr, 0, dk, 1, bv[s][1]);
      }
    }

    // ---- q tile -> Qb (LNB: normalised), in two halves of 8 loads ----
    float mu[NACC] = {0.f, 0.f}, rs[NACC] = {1.f, 1.f};
    if (LNB) {
      const float* sp = p.stats + (int64_t)b * 2 * p.V;
      vload<NACC>(sp + nc, mu);
      vload<NACC>(sp + p.V + nc, rs);
    }
    if constexpr (FAC) {
      float qv[16][NACC];
      fac_build(fa, ft, Qb, lane, qv);
#pragma unroll
      for (int s = 0; s < 16; ++s)
        *reinterpret_cast<float2*>(Qb + (2 * s + h) * kTS + 2 * j) = make_float2(col_ok ? qv[s][0] : 0.f, col_ok ? qv[s][1] : 0.f);
    } else
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      float xv[8][NACC];
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) vload<NACC>(p.q + sample + (int64_t)(2 * (hf * 8 + s8)) * p.V + lane_par, xv[s8]);
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8)
        *reinterpret_cast<float2*>(Qb + (2 * (hf * 8 + s8) + h) * kTS + 2 * j) =
            make_float2(col_ok ? (xv[s8][0] - mu[0]) * rs[0] : 0.f, col_ok ? (xv[s8][1] - mu[1]) * rs[1] : 0.f);
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- g tile -> Gb ----
#pragma unroll
    for (int s = 0; s < 16; ++s)
      *reinterpret_cast<float2*>(Gb + (2 * s + h) * kTS + 2 * j) = make_float2(col_ok ? bv[s][0] : 0.f, col_ok ? bv[s][1] : 0.f);

    // ---- y = Wᵀ g ----
    f32x16 acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    if constexpr (BXB) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        bx8 bop[NACC][1];
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
          float x8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) x8[e] = bv[8 * g + e][q];
          bx_split<1>(x8, bop[q]);               // bf16 storage: exact
        }
#pragma unroll
        for (int t = 2; t >= 0; --t) {
          const bx8 aw = reinterpret_cast<const bx8*>(As)[(g * 3 + t) * 64 + lane];
#pragma unroll
          for (int q = 0; q < NACC; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aw, bop[q][0], acc[q], 0, 0, 0);
        }
      }
    } else {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float av = As[s * 64 + lane];
#pragma unroll
      for (int q = 0; q < NACC; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[s][q], acc[q], 0, 0, 0);
    }
    }
    fetch_tile(tile + gridDim.x < ntiles ? tile + gridDim.x : tile);

    // ---- dW += g ⊗ q, db += Σ g ----
    if constexpr (BXB) {
      // operand element e of lane half h4 = voxel 16 gk + 8 h4 + e of the wave tile, for both operands (any assignment of
      // reduction indices to slots is valid); rows are 8-byte aligned (stride 66 floats): four ds_read_b64 per operand
      const int rowo = (lane & 31) * kTS + 8 * (lane >> 5);
#pragma unroll
      for (int gk = 0; gk < 4; ++gk) {
        float g8[8], q8[8];
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          const float2 gv = *reinterpret_cast<const float2*>(Gb + rowo + 16 * gk + 2 * e2);
          const float2 qv = *reinterpret_cast<const float2*>(Qb + rowo + 16 * gk + 2 * e2);
          g8[2 * e2] = gv.x; g8[2 * e2 + 1] = gv.y;
          q8[2 * e2] = qv.x; q8[2 * e2 + 1] = qv.y;
        }
        bx8 ga[1];
        bx_split<1>(g8, ga);                     // the stored gradient: exact
        constexpr int NTQ = LNB ? 3 : 1;         // LNB: the normalised input is a computed fp32 value
        bx8 qb[NTQ];
        bx_split<NTQ>(q8, qb);
#pragma unroll
        for (int t = NTQ - 1; t >= 0; --t) dWx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[0], qb[t], dWx, 0, 0, 0);
        db[0] += ((g8[0] + g8[1]) + (g8[2] + g8[3])) + ((g8[4] + g8[5]) + (g8[6] + g8[7]));
        asm volatile("" : "+v"(db[0]));
        __builtin_amdgcn_sched_barrier(0);
      }
    } else
#pragma unroll
    for (int tc = 0; tc < 2; ++tc) {
      float a0[8], a1[8], b0[8], b1[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = tc * 8 + u;
        a0[u] = Gb[l16 * kTS + 4 * t + k4];
        a1[u] = Gb[(16 + l16) * kTS + 4 * t + k4];
        b0[u] = Qb[l16 * kTS + 4 * t + k4];
        b1[u] = Qb[(16 + l16) * kTS + 4 * t + k4];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        dW[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], b0[u], dW[0][0], 0, 0, 0);
        dW[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], b1[u], dW[0][1], 0, 0, 0);
        dW[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[u], b0[u], dW[1][0], 0, 0, 0);
        dW[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[u], b1[u], dW[1][1], 0, 0, 0);
      }
      db[0] += ((a0[0] + a0[1]) + (a0[2] + a0[3])) + ((a0[4] + a0[5]) + (a0[6] + a0[7]));
      db[1] += ((a1[0] + a1[1]) + (a1[2] + a1[3])) + ((a1[4] + a1[5]) + (a1[6] + a1[7]));
      asm volatile("" : "+v"(db[0]), "+v"(db[1]));
      __builtin_amdgcn_sched_barrier(0);
    }

    if (!LNB) {
      if (col_ok) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rbase = (r & 3) + 8 * (r >> 2);
          float v[NACC] = {acc[0][r], acc[1][r]};
          vstore<NACC>(p.y + sample + (int64_t)rbase * p.V + lane_row, v);
        }
      }
    } else {
      float m1[NACC] = {0.f, 0.f}, m2[NACC] = {0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float gc = tB[row];
        const float2 xh = *reinterpret_cast<const float2*>(Qb + row * kTS + 2 * j);
        const float a0 = acc[0][r] * gc, a1 = acc[1][r] * gc;
        m1[0] += a0; m1[1] += a1;
        m2[0] += a0 * xh.x; m2[1] += a1 * xh.y;
      }
#pragma unroll
      for (int q = 0; q < NACC; ++q) {
        m1[q] = (m1[q] + __shfl_xor(m1[q], 32, 64)) * (1.0f / 32.0f);
        m2[q] = (m2[q] + __shfl_xor(m2[q], 32, 64)) * (1.0f / 32.0f);
      }
#pragma unroll
      for (int r8 = 0; r8 < 2; ++r8) {
        float ga[8][NACC];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int r = r8 * 8 + i;
          if (p.gadd != nullptr) vload<NACC>(p.gadd + sample + (int64_t)((r & 3) + 8 * (r >> 2)) * p.V + lane_row, ga[i]);
          else ga[i][0] = ga[i][1] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int r = r8 * 8 + i;
          const int rbase = (r & 3) + 8 * (r >> 2);
          const int row = rbase + 4 * h;
          const float gc = tB[row];
          const float2 xh = *reinterpret_cast<const float2*>(Qb + row * kTS + 2 * j);
          float v[NACC];
          v[0] = rs[0] * (acc[0][r] * gc - m1[0] - xh.x * m2[0]) + ga[i][0];
          v[1] = rs[1] * (acc[1][r] * gc - m1[1] - xh.y * m2[1]) + ga[i][1];
          if (col_ok) vstore<NACC>(p.y + sample + (int64_t)rbase * p.V + lane_row, v);
          float sg = col_ok ? acc[0][r] * xh.x + acc[1][r] * xh.y : 0.f;
          float sb = col_ok ? acc[0][r] + acc[1][r] : 0.f;
          sg = half_sum32(sg);
          sb = half_sum32(sb);
          if ((lane & 31) == 31) {
            red[wave * 64 + row] = sg;
            red[wave * 64 + 32 + row] = sb;
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      __syncthreads();
      if (threadIdx.x < 64) {
        const int e = threadIdx.x;
        gln += (red[e] + red[64 + e]) + (red[128 + e] + red[192 + e]);
      }
      __syncthreads();
    }
  }

  // ---- workgroup row: (dW | db), waves added in index order ----
  float* row = p.wpart + (int64_t)blockIdx.x * kDwRow;
  __syncthreads();
  if constexpr (BXB) {
#pragma unroll
    for (int r = 0; r < 16; ++r) R[(wave * 16 + r) * 64 + lane] = dWx[r];
  } else {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b2 = 0; b2 < 2; ++b2)
#pragma unroll
      for (int v = 0; v < 4; ++v) R[(wave * 16 + (a * 2 + b2) * 4 + v) * 64 + lane] = dW[a][b2][v];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 1024; e += 256) {
    const int idx = e >> 6, l = e & 63;
    const float t = (R[e] + R[1024 + e]) + (R[2048 + e] + R[3072 + e]);
    if constexpr (BXB) {   // accumulator register idx of lane l: row (g channel) = (idx & 3) + 8 (idx >> 2) + 4 (l >> 5), column = l & 31
      row[((idx & 3) + 8 * (idx >> 2) + 4 * (l >> 5)) * 32 + (l & 31)] = t;
    } else {
      const int a = idx >> 3, b2 = (idx >> 2) & 1, v = idx & 3;
      row[(16 * a + 4 * (l >> 4) + v) * 32 + 16 * b2 + (l & 15)] = t;
    }
  }
  __syncthreads();
  R[(wave * 2 + 0) * 64 + lane] = db[0];
  R[(wave * 2 + 1) * 64 + lane] = db[1];
  __syncthreads();
  if (threadIdx.x < 32) {
    const int e = threadIdx.x, slot = e >> 4, i16 = e & 15;
    float t = 0.f;
    if constexpr (BXB) {   // db[0] of lane l = partial sum of g channel l & 31 over its half of the voxels
      for (int w = 0; w < 4; ++w) t += R[(w * 2) * 64 + e] + R[(w * 2) * 64 + 32 + e];
    } else {
      for (int w = 0; w < 4; ++w)
        for (int kk = 0; kk < 4; ++kk) t += R[(w * 2 + slot) * 64 + kk * 16 + i16];
    }
    row[1024 + e] = t;
  }
  if (threadIdx.x < 64) row[1024 + 32 + threadIdx.x] = gln;
}

// (rows added in slice order, LayerNorm affine applied, by the FK_DW job of the finish kernel: finish.h)

}  // namespace fz

using namespace fz;

static int knob_gemm_dw_wgs() { return knob_pos(FZ_KNOB("FZ_GEMM_DW_WGS"), 512); }

extern "C" int fz_gemm_dw_rows(int B, int64_t V);
template <typename AT>
static int gemm_dw_launch(const fz_gemm_dw_desc* d, const fz_outproj_fac* fac, fz_stream_t stream) {
  DwArgsT<AT> a;
  a.g = (const AT*)d->g; a.q = (const AT*)d->q; a.w = d->w; a.ldw = d->ldw > 0 ? d->ldw : 32; a.stats = d->stats; a.ln_g = d->ln_g; a.gadd = (const AT*)d->gadd;
  a.y = (AT*)d->y; a.wpart = (float*)d->wpart; a.V = d->V; a.B = d->B;
  const int ntiles = (int)fz_mlp_partials(d->B, d->V);
  const int rows = fz_gemm_dw_rows(d->B, d->V);
  constexpr int lds = (1536 + 32 + 256 + 4 * 64 * kTS) * (int)sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (fac) {   // (gemm_dw_entry has refused the factor form with ln, dropout or bf16 storage)
    if constexpr (sizeof(AT) == 4) {
      FacArgs fa;
      const int rc = fac_args(fac, d->V, "fz_gemm_dw_fac", fa);
      if (rc != FZ_OK) return rc;
      auto kern = gemm_dw_kernel<false, AT, FacArgs>;
      FZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      hipLaunchKernelGGL(kern, dim3((unsigned)rows), dim3(256), lds, st, a, ntiles, fa);
    } else {
      return fail(FZ_E_UNSUPPORTED, "fz_gemm_dw_fac: fp32 storage only");
    }
  } else if (d->drop_m) {   // site 0 on g (out_proj: no LayerNorm form)
    auto kern = gemm_dw_kernel<false, AT, DropArgs>;
    FZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)rows), dim3(256), lds, st, a, ntiles, drop_args(d->drop_m, nullptr, nullptr, d->drop_s, 1.f, 1.f, d->V));
  } else if (d->ln) {
    auto kern = gemm_dw_kernel<true, AT>;
    FZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)rows), dim3(256), lds, st, a, ntiles);
  } else {
    auto kern = gemm_dw_kernel<false, AT>;
    FZ_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)rows), dim3(256), lds, st, a, ntiles);
  }
  FZ_LAUNCH_CHECK();
  FinishJob fj = finish_job(FK_DW, kDwRow / 16);
  fj.u.dw = FinDw{(const float*)d->wpart, d->ln ? d->ln_g : (const float*)nullptr, d->ln_b, d->gw, d->gb, d->ln ? d->gln : (float*)nullptr,
                  rows, d->ldgw > 0 ? d->ldgw : 32};
  return finish_run(&fj, 1, st);
}

extern "C" int fz_gemm_dw_rows(int B, int64_t V) {
  const int64_t nt = fz_mlp_partials(B, V);
  const int wgs = knob_gemm_dw_wgs();
  return (int)(nt < wgs ? nt : wgs);
}
extern "C" int64_t fz_gemm_dw_workspace_bytes(int B, int64_t V) {
  return (int64_t)fz_gemm_dw_rows(B, V) * kDwRow * (int64_t)sizeof(float);
}

// fac (fz_gemm_dw_fac): q as the rank-1 factors of the core's two windows, q itself null
static int gemm_dw_entry(const fz_gemm_dw_desc* d, const fz_outproj_fac* fac, fz_stream_t stream) {
  if (!d) return fail(FZ_E_ARG, "fz_gemm_dw: null descriptor");
  if (fac && (d->q || d->ln || d->drop_m || d->act_dtype != FZ_STORE_F32 || d->C != 32))
    return fail(FZ_E_UNSUPPORTED, "fz_gemm_dw_fac: needs q == NULL, no LayerNorm form, no dropout, fp32 storage, C == 32 (fz_outproj_factors_supported)");
  if (!d->g || (!d->q && !fac) || !d->w || !d->y || !d->wpart || !d->gw) return fail(FZ_E_ARG, "fz_gemm_dw: null pointer");
  if (d->ln && (!d->stats || !d->ln_g || !d->ln_b || !d->gln)) return fail(FZ_E_ARG, "fz_gemm_dw: the LayerNorm form needs stats, gamma, beta, gln");
  if (!d->ln && d->gadd) return fail(FZ_E_UNSUPPORTED, "fz_gemm_dw: gadd only with the LayerNorm backward");
  if (d->drop_m && d->ln) return fail(FZ_E_UNSUPPORTED, "fz_gemm_dw: dropout on g only without the LayerNorm backward");
  if (!drop_scale_ok(d->drop_m, d->drop_s)) return fail(FZ_E_ARG, "fz_gemm_dw: the dropout scale 1 / (1 - p) must be >= 1 and finite");
  if (d->C != 32) return fail(FZ_E_UNSUPPORTED, "fz_gemm_dw: needs C == 32");
  if (d->ldgw != 0 && d->ldgw < 32) return fail(FZ_E_ARG, "fz_gemm_dw: ldgw must be 0 (= 32) or >= 32");
  if (d->ldw != 0 && d->ldw < 32) return fail(FZ_E_ARG, "fz_gemm_dw: ldw must be 0 (= 32) or >= 32");
  if (d->B < 1 || d->V < 1 || d->V % 4 != 0 || d->V > ((int64_t)1 << 27)) return fail(FZ_E_UNSUPPORTED, "fz_gemm_dw: needs B >= 1, V % 4 == 0, V <= 2^27");
  if (d->act_dtype == FZ_STORE_F32) return gemm_dw_launch<float>(d, fac, stream);
  if (d->act_dtype == FZ_STORE_BF16) return gemm_dw_launch<bf16>(d, fac, stream);
  return fail(FZ_E_ARG, "fz_gemm_dw: act_dtype must be FZ_STORE_F32 or FZ_STORE_BF16");
}

extern "C" int fz_gemm_dw(const fz_gemm_dw_desc* d, fz_stream_t stream) { return gemm_dw_entry(d, nullptr, stream); }

extern "C" int fz_gemm_dw_fac(const fz_gemm_dw_desc* d, const fz_outproj_fac* fac, fz_stream_t stream) {
  if (!fac) return fail(FZ_E_ARG, "fz_gemm_dw_fac: null factor block");
  return gemm_dw_entry(d, fac, stream);
}
