// gemm_stream.hip — the streaming kernel of the fp32-MFMA GEMM family (gemm.hip has the family's layers and MFMA mapping)
// and its host launcher, reached from fz_gemm's dispatcher.
#include "gemm_common.h"

namespace fz {

// =================================================================================================
// Kernel B — streaming operand with a PF-deep register prefetch ring, any K, all loaders.
// NACC = consecutive voxels per lane (4/2/1 → 128/64/32-column wave tiles): small tiles give the
// deep, narrow stages (8^3..32^3 voxels, C = 128..512) enough workgroups to fill 256 CUs.
// =================================================================================================
constexpr int kAChunk = 64;  // A-operand steps staged in LDS at a time

// PRO = compile-time prologue: a runtime branch inside the K loop splits every step into its own
// basic block (ds_read → wait → MFMA serialised), so the variants are separate instantiations.
enum { PRO_NONE = 0, PRO_LN = 1, PRO_GELU = 2, PRO_BMUL = 3 };

// KS = 4: the four waves of a workgroup share ONE column tile and split the K steps between them
// (groups of kPF steps, round-robin), then add their accumulators through LDS.  For the deep
// stages (8^3, 16^3 voxels; K = 256..2048) this gives 4x the workgroups and 4x shorter dependent
// MFMA chains: 512->512 at 8^3 is 128 workgroups x 256 serial steps without it.
// (2 workgroups per CU: 3 or 4 — narrower tiles under tighter launch bounds — measured no faster,
// an occupancy sweep: the operand traffic of these launches runs at 4.1-5.1 TB/s even with the
// MFMAs compiled out (round-1/2 probe `gemm_probe7`), the fp32 MFMA time comes largely on top of it.)
template <int MB, int NACC, int LOADER, int EPI, int PRO, int KS = 1, typename AT = float>
__global__ __launch_bounds__(256, ((MB == 2 && NACC == 4 && PRO == 3 /* gate operand in the ring */) ? 1 : 2)) void gemm_stream_kernel(GemmArgsT<AT> p) {
  constexpr int TN = 32 * NACC;
  // the 2-D loaders (LOAD_S2D_2D, LOAD_K3_2D) share the column decode, ring and MFMA order of their 3-D forms
  constexpr bool S2DL = LOADER == LOAD_S2D || LOADER == LOAD_S2D_2D;
  constexpr bool K3L = LOADER == LOAD_K3 || LOADER == LOAD_K3_2D;
  constexpr int NL = S2DL ? 4 : NACC;  // floats fetched per load step
  // operand prefetch depth (load steps): narrow tiles are latency-bound (L2 round trip ≈ 500-900
  // cycles vs 64·NACC MFMA cycles per step), so they keep more loads in flight
  constexpr int kPF = (NL == 4) ? 8 : 16;
  // Without the K-split the weight chunks are DOUBLE-BUFFERED: the next chunk's weights travel global →
  // registers while the MFMAs of the current chunk run, and are stored to the other LDS buffer
  // afterwards (one barrier per chunk).  Exposed fills were 15-20 % of the K >= 256 GEMMs and convs.
  constexpr bool DB = (KS == 1);
  constexpr int CH = DB ? kAChunk / 2 : kAChunk;                 // A steps per chunk
  constexpr int kBufFloats = CH * MB * 64;
  constexpr int NWR = kBufFloats / 256;                          // staged weights per thread and chunk
  constexpr int kRedFloats = (KS > 1) ? (KS - 1) * (MB * NACC * 16 + 2 * NACC) * 64 : 0;
  constexpr int kAsFloats = (DB ? 2 : 1) * kBufFloats > kRedFloats ? (DB ? 2 : 1) * kBufFloats : kRedFloats;
  __shared__ float As[kAsFloats];
  __shared__ float sW[32 * MB];
  __shared__ float tW[32 * MB];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  constexpr int WT = (KS > 1) ? 1 : 4;  // column tiles per workgroup
  const int tiles_per_sample = (int)((p.Ncol + TN * WT - 1) / (TN * WT));
  // Workgroup -> (column tile bx, row-block group by).  With several row-block groups (M > 32·MB) the
  // grid is 1-D and XCD-aware: workgroups are dealt round-robin over the 8 XCDs, so the `ygroups`
  // groups of ONE column tile are given consecutive slots of the SAME XCD — they run concurrently and
  // share the operand tile in that XCD's L2 instead of each pulling it from HBM / Infinity Cache.
  int bx = blockIdx.x, by = blockIdx.y;
  if (p.ygroups > 1) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    by = slot % p.ygroups;
    bx = (slot / p.ygroups) * 8 + xcd;
    if (bx >= p.xtiles) return;  // padding of the last round (before any barrier)
  }
  const int b = bx / tiles_per_sample;
  const int64_t n0 = ((int64_t)(bx % tiles_per_sample) * WT + (KS > 1 ? 0 : wave)) * TN;
  const int m0 = by * 32 * MB;
  // A steps: two channels per step, and the space-to-depth loaders walk the taps of a channel PAIR together (a_k) — with an odd
  // Cin the last pair is half empty but still takes all its tap steps ((K + 1) / 2 = 4·Cin stopped after taps 0..3 of the last
  // channel; tests/test_gpu_gemm.py str_s2d); the empty half has zero weights (load_chunk: kk < K) and a masked operand
  const int nA = LOADER == LOAD_S2D ? 8 * ((p.Cin + 1) / 2) : (LOADER == LOAD_S2D_2D ? 4 * ((p.Cin + 1) / 2) : (p.K + 1) / 2);

  if (PRO == PRO_LN) {
    // s[m] = Σ_k W[m][k]·γ[k], t[m] = Σ_k W[m][k]·β[k]: 8 threads per row, k interleaved (a single
    // thread per row is K dependent-latency loads: 60-110 us at K = 512..1024)
    for (int r0 = 0; r0 < 32 * MB; r0 += 32) {
      const int r = r0 + (threadIdx.x >> 3), part = threadIdx.x & 7;
      const int m = m0 + r;
      float s = 0.f, t = 0.f;
      if (m < p.M)
        for (int k = part; k < p.K; k += 8) {
          const float wv = weight_at(p, m, k);
          s += wv * p.ln_g[k];
          t += wv * p.ln_b[k];
        }
      s += __shfl_xor(s, 1, 64); t += __shfl_xor(t, 1, 64);
      s += __shfl_xor(s, 2, 64); t += __shfl_xor(t, 2, 64);
      s += __shfl_xor(s, 4, 64); t += __shfl_xor(t, 4, 64);
      if (part == 0) { sW[r] = s; tW[r] = t; }
    }
  }

  // ---- per-lane input addressing ----
  int64_t col_off;
  bool col_ok;
  int kw0 = 0, kh0 = 0, kd0 = 0;
  if (S2DL) {
    const int64_t n = n0 + 2 * j;  // coarse voxel pair (wo even)
    col_ok = n < p.Ncol;
    const int64_t nn = col_ok ? n : 0;
    const int wo = (int)(nn % p.Wo);
    const int64_t t2 = nn / p.Wo;
    const int ho = (int)(t2 % p.Ho);
    const int dz = (int)(t2 / p.Ho);
    col_off = ((int64_t)(2 * dz) * p.Hi + 2 * ho) * p.Wi + 2 * wo;
  } else {
    col_off = n0 + NACC * j;
    col_ok = col_off < p.Ncol;
    if (K3L) {
      const int64_t nn = col_ok ? col_off : 0;
      kw0 = (int)(nn % p.Wi);
      kh0 = (int)((nn / p.Wi) % p.Hi);
      kd0 = (int)(nn / ((int64_t)p.Wi * p.Hi));
    }
  }

  constexpr int NR = (PRO == PRO_BMUL) ? 2 * NL : NL;  // ring slot: operand (+ gate operand)
  auto fetch = [&](int s, float (&v)[NR]) {
    if constexpr (LOADER == LOAD_PLAIN) {
      fetch_plain_raw<NL, PRO == PRO_BMUL>(p, b, 2 * s + h, col_off, col_ok, v);
    } else if constexpr (LOADER == LOAD_S2D_2D) {
      // rows k = (c, th, tw): load step s = (channel pair, th); 4 fine pixels = (tw 0, 1) of two coarse pixels
      const int c = 2 * (s >> 1) + h;
      const bool ok = col_ok && c < p.Cin;
      const int cc = c < p.Cin ? c : p.Cin - 1;
      const int64_t off = (col_ok ? col_off : 0) + (int64_t)(s & 1) * p.Wi;
      vload<NL>(p.x[0] + ((int64_t)b * p.Cin + cc) * p.Vin + off, v);
#pragma unroll
      for (int e = 0; e < NL; ++e) v[e] = ok ? v[e] : 0.f;
    } else if constexpr (LOADER == LOAD_S2D) {
      const int c = 2 * (s >> 2) + h;
      const bool ok = col_ok && c < p.Cin;
      const int cc = c < p.Cin ? c : p.Cin - 1;
      const int64_t off = (col_ok ? col_off : 0) + (int64_t)((s >> 1) & 1) * p.Hi * p.Wi + (int64_t)(s & 1) * p.Wi;
      vload<NL>(p.x[0] + ((int64_t)b * p.Cin + cc) * p.Vin + off, v);
#pragma unroll
      for (int e = 0; e < NL; ++e) v[e] = ok ? v[e] : 0.f;
    } else {
      // LOAD_K3 (NL == 4): taps of the 3x3x3 stencil, zero padding — clamped addresses + selects.
      // LOAD_K3_2D: the 3x3 stencil on a depth-1 grid (Di = 1): taps (kh, kw), the depth tap fixed at the centre
      constexpr int NT = (LOADER == LOAD_K3_2D) ? 9 : 27;
      const int c = 2 * (s / NT) + h;
      const int tap = s % NT;
      const int kd = (NT == 9) ? 1 : tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
      const int zd = kd0 + kd - 1, zh = kh0 + kh - 1;
      const bool ok = col_ok && c < p.Cin && zd >= 0 && zd < p.Di && zh >= 0 && zh < p.Hi;
      const int cc = c < p.Cin ? c : p.Cin - 1;
      const int zdc = zd < 0 ? 0 : (zd >= p.Di ? p.Di - 1 : zd);
      const int zhc = zh < 0 ? 0 : (zh >= p.Hi ? p.Hi - 1 : zh);
      const AT* row = p.x[0] + ((int64_t)b * p.Cin + cc) * p.Vin + ((int64_t)zdc * p.Hi + zhc) * p.Wi;
      float t4[4];
      vload<4>(row + kw0, t4);
      const float4 t = make_float4(t4[0], t4[1], t4[2], t4[3]);
      const float lft = aget(row + (kw0 > 0 ? kw0 - 1 : 0));
      const float rgt = aget(row + (kw0 + 4 < p.Wi ? kw0 + 4 : kw0));
      const float l0 = kw0 > 0 ? lft : 0.f;
      const float r0 = kw0 + 4 < p.Wi ? rgt : 0.f;
      float o0, o1, o2, o3;
      if (kw == 1) { o0 = t.x; o1 = t.y; o2 = t.z; o3 = t.w; }
      else if (kw == 0) { o0 = l0; o1 = t.x; o2 = t.y; o3 = t.z; }
      else { o0 = t.y; o1 = t.z; o2 = t.w; o3 = r0; }
      v[0] = ok ? o0 : 0.f; v[1 % NL] = ok ? o1 : 0.f; v[2 % NL] = ok ? o2 : 0.f; v[3 % NL] = ok ? o3 : 0.f;
    }
  };

  f32x16 acc[MB][NACC];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int q = 0; q < NACC; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][q][r] = 0.f;

  float s1[NACC], s2[NACC], shift[NACC];
#pragma unroll
  for (int e = 0; e < NACC; ++e) s1[e] = s2[e] = shift[e] = 0.f;

  const int nload = S2DL ? nA / 2 : nA;
  float ring[kPF][NR];
  // unconditional, clamped prefetch: a load inside a branch costs an s_waitcnt vmcnt(0)
#pragma unroll
  for (int i = 0; i < kPF; ++i) {
    const int si = (KS > 1 ? wave * kPF : 0) + i;
    fetch(si < nload ? si : nload - 1, ring[i]);
  }
  if (PRO == PRO_LN) {
    // pivot = channel-0 value (held by half 0 in ring[0]): well-conditioned single-pass variance
    if (KS > 1) {
      float pv[NR];
      fetch(0, pv);  // every wave needs the SAME pivot
#pragma unroll
      for (int e = 0; e < NACC; ++e) shift[e] = __shfl(pv[e % NL], j, 64);
    } else {
#pragma unroll
      for (int e = 0; e < NACC; ++e) shift[e] = __shfl(ring[0][e % NL], j, 64);
    }
  }

  constexpr int kGroup = kPF * (S2DL ? 2 : 1);
  static_assert(CH % (KS * kGroup) == 0, "chunk must hold whole rounds of (K-split) prefetch groups");
  // steps are processed in groups of kPF*ASTEP with NO per-step guard (a guard turns every K-step into
  // its own basic block: ds_read → s_waitcnt lgkmcnt(0) → MFMA, fully serialised); the tail of the
  // last group gets zero weights instead
  float wreg[NWR];
  // weights of chunk [a0, a0+an) in operand order → registers; branch-free (clamped address + select)
  auto load_chunk = [&](int a0, int an) {
#pragma unroll
    for (int uu = 0; uu < NWR; ++uu) {
      const int idx = threadIdx.x + uu * 256;
      const int l = idx & 63;
      const int mb = (idx >> 6) % MB;
      const int a = a0 + idx / (64 * MB);
      const int m = m0 + mb * 32 + (l & 31);
      const int kk = a_k<LOADER>(a, l >> 5);
      const bool ok = idx < an * MB * 64 && m < p.M && kk < p.K;
      const int mc = m < p.M ? m : p.M - 1, kc = kk < p.K ? kk : p.K - 1;
      float wv = weight_at(p, mc, kc);
      if (PRO == PRO_LN) wv *= p.ln_g[kc];
      wreg[uu] = ok ? wv : 0.f;
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int uu = 0; uu < NWR; ++uu) As[buf * kBufFloats + threadIdx.x + uu * 256] = wreg[uu];
  };

  __syncthreads();  // sW / tW (and the previous use of LDS) settled
  load_chunk(0, min(CH, nA));
  store_chunk(0);
  __syncthreads();
  int cbuf = 0;
  for (int a0 = 0; a0 < nA; a0 += CH) {
    const int an = min(CH, nA - a0);
    const int an_pad = ((an + KS * kGroup - 1) / (KS * kGroup)) * (KS * kGroup);
    const bool more = a0 + CH < nA;
    if (DB && more) load_chunk(a0 + CH, min(CH, nA - a0 - CH));  // in flight during the MFMAs below
    const float* Ab = As + cbuf * kBufFloats;
    constexpr int ASTEP = S2DL ? 2 : 1;
    // kAChunk is a multiple of kPF*ASTEP, so the ring slot of a step is static after unrolling
    for (int al = (KS > 1 ? wave * kPF * ASTEP : 0); al < an_pad; al += KS * kPF * ASTEP) {
#pragma unroll
      for (int u = 0; u < kPF; ++u) {
        const int ali = al + u * ASTEP;
        const int s = (a0 + ali) / ASTEP;
        float cur[NR];
#pragma unroll
        for (int e = 0; e < NR; ++e) cur[e] = ring[u][e];
        {
          if (S2DL) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
              const float av0 = Ab[(ali * MB + mb) * 64 + lane];        // tw = 0
              const float av1 = Ab[((ali + 1) * MB + mb) * 64 + lane];  // tw = 1
              acc[mb][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, cur[0], acc[mb][0], 0, 0, 0);
              acc[mb][1 % NACC] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, cur[2 % NL], acc[mb][1 % NACC], 0, 0, 0);
              acc[mb][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, cur[1 % NL], acc[mb][0], 0, 0, 0);
              acc[mb][1 % NACC] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, cur[3 % NL], acc[mb][1 % NACC], 0, 0, 0);
            }
          } else {
            float bvv[NACC];
            // deferred masking of the raw ring slot: lanes past the last column and the odd-K pad
            // channel contribute zero (their clamped re-reads are finite; weights of the pad are 0)
            const bool cok = col_ok && (2 * s + h) < p.Cin;
#pragma unroll
            for (int e = 0; e < NACC; ++e) {
              float t = cur[e % NL];
              if (LOADER == LOAD_PLAIN) {
                if (PRO == PRO_BMUL) t = cur[(NL + e) % NR] > 0.f ? t : 0.f;
                t = cok ? t : 0.f;
              }
              if (PRO == PRO_LN) {
                t = cok ? t - shift[e] : 0.f;  // padded steps / lanes must not enter the statistics
                s1[e] += t;
                s2[e] += t * t;
              }
              bvv[e] = t;
            }
            if (PRO == PRO_GELU) {
#pragma unroll
              for (int e = 0; e < NACC; ++e) bvv[e] = gelu_f(bvv[e]);
            }
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
              const float av = Ab[(ali * MB + mb) * 64 + lane];
#pragma unroll
              for (int q = 0; q < NACC; ++q) {
#if defined(FZ_PROBE_MFMA_NONE)
                acc[mb][q][0] += av * bvv[q];  // diagnostics build: operand traffic only
#elif defined(FZ_PROBE_MFMA_HALF)
                if (q & 1) acc[mb][q][0] += av * bvv[q];
                else acc[mb][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bvv[q], acc[mb][q], 0, 0, 0);
#elif defined(FZ_PROBE_MFMA_AGPR)
                asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+a"(acc[mb][q]) : "v"(av), "v"(bvv[q]));
#else
                acc[mb][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bvv[q], acc[mb][q], 0, 0, 0);
#endif
              }
            }
          }
        }
        // Refill the slot right behind the MFMAs that consumed it, and pin it there: the slot registers
        // are the MFMA operands, so the refill cannot be issued earlier; left alone, the scheduler sinks
        // all kPF refills of a group to the bottom of the unrolled body and the first slot of the next
        // group is awaited right after it was requested — one exposed memory round trip per group.
        {
          const int sn = s + KS * kPF;
          fetch(sn < nload ? sn : nload - 1, ring[u]);  // tail: harmless re-read of the last step
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // next chunk: registers → the other buffer (double-buffered) or, with the K-split, a plain refill
    if (more) {
      if (DB) {
        store_chunk(cbuf ^ 1);
        cbuf ^= 1;
      } else {
        __syncthreads();  // everyone is done reading the single buffer
        load_chunk(a0 + CH, min(CH, nA - a0 - CH));
        store_chunk(0);
      }
      __syncthreads();
    }
  }

  if (KS > 1) {
    // add the K-slices: waves 1..KS-1 park their accumulators (and LN sums) in LDS, wave 0 finishes
    __syncthreads();  // everyone is done reading As
    constexpr int kPer = (MB * NACC * 16 + 2 * NACC) * 64;
    if (wave > 0) {
      float* dst = As + (wave - 1) * kPer + lane;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int q = 0; q < NACC; ++q)
#pragma unroll
          for (int r = 0; r < 16; ++r) dst[((mb * NACC + q) * 16 + r) * 64] = acc[mb][q][r];
#pragma unroll
      for (int e = 0; e < NACC; ++e) {
        dst[(MB * NACC * 16 + e) * 64] = s1[e];
        dst[(MB * NACC * 16 + NACC + e) * 64] = s2[e];
      }
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < KS - 1; ++w) {
      const float* src = As + w * kPer + lane;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int q = 0; q < NACC; ++q)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mb][q][r] += src[((mb * NACC + q) * 16 + r) * 64];
#pragma unroll
      for (int e = 0; e < NACC; ++e) {
        s1[e] += src[(MB * NACC * 16 + e) * 64];
        s2[e] += src[(MB * NACC * 16 + NACC + e) * 64];
      }
    }
  }

  float mu_d[NACC], rstd[NACC];
  if (PRO == PRO_LN) {
#pragma unroll
    for (int e = 0; e < NACC; ++e) {
      const float t1 = s1[e] + __shfl_xor(s1[e], 32, 64);
      const float t2 = s2[e] + __shfl_xor(s2[e], 32, 64);
      const float inv = 1.0f / (float)p.Cin;
      const float md = t1 * inv;
      float var = t2 * inv - md * md;
      var = var > 0.f ? var : 0.f;
      mu_d[e] = md;
      rstd[e] = 1.0f / sqrtf(var + p.ln_eps);
    }
    if (p.stats_out != nullptr && by == 0 && h == 0 && col_ok) {
      float mean[NACC];
#pragma unroll
      for (int e = 0; e < NACC; ++e) mean[e] = shift[e] + mu_d[e];
      float* so = p.stats_out + (int64_t)b * 2 * p.Vin;
      vstore<NACC>(so + col_off, mean);
      vstore<NACC>(so + p.Vin + col_off, rstd);
    }
  }
  if (!col_ok) return;
  const int64_t ncol = S2DL ? n0 + 2 * j : col_off;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    if (PRO == PRO_LN) {
      // y = rstd·(acc − μ_d·s[m]) + t[m]
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float sw = sW[mb * 32 + rl];
#pragma unroll
        for (int q = 0; q < NACC; ++q) acc[mb][q][r] = rstd[q] * (acc[mb][q][r] - mu_d[q] * sw);
      }
    }
    store_block<NACC, EPI, S2DL>(p, acc[mb], b, m0 + mb * 32, ncol, h,
                                                PRO == PRO_LN ? tW + mb * 32 : nullptr);
  }
}

// Host side of Kernel B: gemm_launch (gemm.hip) comes here with a validated descriptor and the filled argument block when
// no other kernel took the layer.
template <typename AT>
int gemm_stream_launch(const fz_gemm_desc* d, GemmArgsT<AT> a, fz_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  const int mblocks = (d->M + 31) / 32;
  // (A persistent variant of the streaming kernel — whole weight block resident, the prefetch ring running
  // across tile boundaries — was measured for 32 < K <= 128 at stages 0/1 and was not faster:
  // those GEMMs sit at 56-71 TFLOP/s of fp32 MFMA with the operand loads as the stall reason, not the
  // per-tile prologue / epilogue.)
  // ---- Kernel B: streaming; pick the column-tile width so the grid fills the chip ----
  // tile choice from a sweep on MI355X (round-1/2 probe `gemm_probe3`, FZ_GEMM_CFG): take the widest
  // column tile that still gives >= 256 workgroups (one per CU); two row blocks per workgroup only
  // when that still leaves >= 512 workgroups
  int nacc = 4, MBsel = mblocks >= 2 ? 2 : 1;
  if (d->loader == LOAD_S2D || d->loader == LOAD_S2D_2D) { nacc = 2; MBsel = 1; }
  else {
    const bool narrow_ok = d->loader == LOAD_PLAIN && d->epilogue == EPI_PLAIN;
    auto wgs = [&](int na, int mb) {
      const int64_t t = (d->Ncol + 32 * na * 4 - 1) / (32 * na * 4);
      return t * d->B * ((mblocks + mb - 1) / mb);
    };
    if (wgs(nacc, MBsel) < 512 && MBsel == 2) MBsel = 1;
    if (narrow_ok) {
      if (wgs(nacc, MBsel) < 256) nacc = 2;
      // (when even 32-voxel tiles cannot give one workgroup per CU — the 8^3 bottleneck — stay with 64-voxel tiles and
      // let the K-split below fill the chip: 8-byte lane loads; 512->1024 at 2 x 8^3: 33 against 43 us, round-1/2 probe `gemm_deep`)
      if (wgs(nacc, MBsel) < 256 && !(wgs(1, MBsel) < 256 && d->K >= 256)) nacc = 1;
      const char* e = FZ_KNOB("FZ_GEMM_CFG").str;  // probe builds: "<nacc><mb>", e.g. 42
      if (e && e[0] && e[1]) { nacc = e[0] - '0'; MBsel = e[1] - '0'; if (MBsel == 2 && (nacc != 4 || mblocks < 2)) MBsel = 1; }
    }
  }
  const int TN = 32 * nacc;
  // K-split across the waves of a workgroup when the plain decomposition leaves most CUs idle
  // and K is long enough to give every wave whole prefetch groups
  int ks = 1;
  {
    const int64_t wg1 = ((d->Ncol + TN * 4 - 1) / (TN * 4)) * d->B * ((mblocks + MBsel - 1) / MBsel);
    const bool shape_ok = MBsel == 1 && ((d->loader == LOAD_PLAIN && d->epilogue == EPI_PLAIN && nacc <= 2) ||
                                         d->loader == LOAD_S2D || d->loader == LOAD_S2D_2D);
    if (shape_ok && wg1 < 256 && d->K >= 256) ks = 4;
  }
  const int WT = ks > 1 ? 1 : 4;
  const int64_t tiles = (d->Ncol + TN * WT - 1) / (TN * WT);
  const int ygr = (mblocks + MBsel - 1) / MBsel;
  int xcd_grid = 1;
  // (only where the COLUMN operand dominates the traffic: few row-block groups, many column tiles;
  // with e.g. 32 groups x 16 tiles — the deep transposed convs — the weights dominate and the
  // x-fastest order, which runs equal-weight workgroups together, is the better one: 61 vs 105 us)
  a.ygroups = (xcd_grid && ygr > 1 && ygr <= 8 && tiles * d->B >= 64) ? ygr : 0;
  a.xtiles = (int)(tiles * d->B);
  dim3 grid((unsigned)(tiles * d->B), (unsigned)ygr), block(256);
  if (a.ygroups > 1) grid = dim3((unsigned)(((tiles * d->B + 7) / 8) * 8 * ygr), 1);
// (fz_gemm_plan's dry run, fz_common.h: the form is named and nothing is launched)
#define FZ_STR_FORM(MB, NA, L, E, PR, KS)                                                                           \
  if (gemm_plan_only())                                                                                             \
    return gemm_plan_form("stream mb%d nacc%d %s%s%s%s grid=%ux%u", MB, NA, gemm_loader_name(L), gemm_epi_name(E),   \
                          gemm_pro_name(PR), KS, grid.x, grid.y)
#define FZ_STR(MB, NA, L, E, PR)                                                                                    \
  do { FZ_STR_FORM(MB, NA, L, E, PR, ""); hipLaunchKernelGGL((gemm_stream_kernel<MB, NA, L, E, PR>), grid, block, 0, st, a); } while (0)
#define FZ_STRK(MB, NA, L, E, PR)                                                                                   \
  do { FZ_STR_FORM(MB, NA, L, E, PR, " ks4"); hipLaunchKernelGGL((gemm_stream_kernel<MB, NA, L, E, PR, 4>), grid, block, 0, st, a); } while (0)
  if (d->bact == ACT_RELU) return fail(FZ_E_UNSUPPORTED, "fz_gemm: ReLU input prologue is not compiled (streaming)");
  const int pro = d->ln ? PRO_LN : (d->bact == ACT_GELU ? PRO_GELU : (d->bmul ? PRO_BMUL : PRO_NONE));
  // (at most one of them is set: gemm_launch refuses bact behind ln and bmul beside either)
  if (d->loader == LOAD_S2D) { if (ks == 4) FZ_STRK(1, 2, LOAD_S2D, EPI_PLAIN, PRO_NONE); else FZ_STR(1, 2, LOAD_S2D, EPI_PLAIN, PRO_NONE); }
  else if (d->loader == LOAD_S2D_2D) { if (ks == 4) FZ_STRK(1, 2, LOAD_S2D_2D, EPI_PLAIN, PRO_NONE); else FZ_STR(1, 2, LOAD_S2D_2D, EPI_PLAIN, PRO_NONE); }
  else if (d->loader == LOAD_K3_2D) { if (MBsel == 2) FZ_STR(2, 4, LOAD_K3_2D, EPI_PLAIN, PRO_NONE); else FZ_STR(1, 4, LOAD_K3_2D, EPI_PLAIN, PRO_NONE); }
  else if (d->epilogue == EPI_D2S_2D) { if (MBsel == 2) FZ_STR(2, 4, LOAD_PLAIN, EPI_D2S_2D, PRO_NONE); else FZ_STR(1, 4, LOAD_PLAIN, EPI_D2S_2D, PRO_NONE); }
  else if (d->loader == LOAD_K3) { if (MBsel == 2) FZ_STR(2, 4, LOAD_K3, EPI_PLAIN, PRO_NONE); else FZ_STR(1, 4, LOAD_K3, EPI_PLAIN, PRO_NONE); }
  else if (d->epilogue == EPI_D2S) {
    if (pro != PRO_NONE) return fail(FZ_E_UNSUPPORTED, "fz_gemm: prologue with depth-to-space epilogue");
    if (MBsel == 2) FZ_STR(2, 4, LOAD_PLAIN, EPI_D2S, PRO_NONE); else FZ_STR(1, 4, LOAD_PLAIN, EPI_D2S, PRO_NONE);
  } else {
#define FZ_STR_SHAPES(PR)                                                                                   \
  do {                                                                                                      \
    if (nacc == 4) { if (MBsel == 2) FZ_STR(2, 4, LOAD_PLAIN, EPI_PLAIN, PR); else FZ_STR(1, 4, LOAD_PLAIN, EPI_PLAIN, PR); } \
    else if (nacc == 2) { if (ks == 4) FZ_STRK(1, 2, LOAD_PLAIN, EPI_PLAIN, PR); else FZ_STR(1, 2, LOAD_PLAIN, EPI_PLAIN, PR); } \
    else { if (ks == 4) FZ_STRK(1, 1, LOAD_PLAIN, EPI_PLAIN, PR); else FZ_STR(1, 1, LOAD_PLAIN, EPI_PLAIN, PR); } \
  } while (0)
    if (pro == PRO_LN) FZ_STR_SHAPES(PRO_LN);
    else if (pro == PRO_GELU) FZ_STR_SHAPES(PRO_GELU);
    else if (pro == PRO_BMUL) FZ_STR_SHAPES(PRO_BMUL);
    else FZ_STR_SHAPES(PRO_NONE);
  }
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

template int gemm_stream_launch<float>(const fz_gemm_desc*, GemmArgsT<float>, fz_stream_t);
template int gemm_stream_launch<bf16>(const fz_gemm_desc*, GemmArgsT<bf16>, fz_stream_t);

}  // namespace fz
