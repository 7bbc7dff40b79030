// dropout.hip — the three dropout sites of FactorizerBlock in training mode (factorizer.py:53-56,69,72; mlp.py:54-60):
//   site 0  fact.dropout   on out_proj(a) + b_out, before the first residual add
//   site 1  mlp.block[2]   on gelu(z1), before fc2
//   site 2  mlp.block[4]   on fc2(h) + b2, before the second residual add
//
// Masks.  Element (site s, sample b, channel c, voxel v) is kept iff word v & 3 of Philox4x32-10 (fz_philox.h) with counter
// (v >> 2, c, b, s) and key (seed & 0xffffffff, seed >> 32) is below thr = floor((1 - p) 2^32): the keep probability is
// thr / 2^32 exactly.  The seed is an int64 that lives on the device (drawn by a torch op from the device generator, so
// drawing it needs no host sync and torch.manual_seed makes runs repeat).  The masks are stored once per forward as packed
// bits, one plane (B, ch, ceil(V / 32)) of uint32 words per live site: bit v & 31 of word v >> 5, padding bits 0.  The
// backward reads the same bits; nothing is regenerated.
//
// The elementwise kernels below apply a plane where the block's GEMM launches cannot (every shape: the dense layers run as
// separate fz_gemm / fz_wgrad / fz_gemm_dw launches under live dropout and these kernels sit between them).
#include <cstdlib>

#include "fz_common.h"
#include "fz_philox.h"
#include "gemm_common.h"

namespace fz {

__global__ __launch_bounds__(256) void dropout_bits_kernel(const int64_t* __restrict__ seed, int site, int B, int ch, int64_t V,
                                                           int64_t nw, uint64_t thr, uint32_t* __restrict__ out) {
  const uint64_t s = (uint64_t)*seed;
  const uint32_t k0 = (uint32_t)s, k1 = (uint32_t)(s >> 32);
  const int64_t total = (int64_t)B * ch * nw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t row = i / nw, j = i - row * nw;
    const uint32_t c = (uint32_t)(row % ch), b = (uint32_t)(row / ch);
    const int64_t v0 = j * 32;
    uint32_t word = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t v = v0 + 4 * q;
      if (v < V) {
        const philox4x32 r = philox4x32_10((uint32_t)(v >> 2), c, b, (uint32_t)site, k0, k1);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (v + e < V && (uint64_t)r.v[e] < thr) word |= 1u << (4 * q + e);
      }
    }
    out[i] = word;
  }
}

// kind: FZ_DROP_RES   y = aux + keep s t  (aux == NULL: y = keep s t)
//       FZ_DROP_GELU  y = keep s gelu(t)
//       FZ_DROP_GELU_BWD y = keep s t gelu'(aux)
// Four consecutive voxels of one row per lane (V % 4 == 0): their four bits sit in one word.
template <typename AT, int KIND>
__global__ __launch_bounds__(256) void dropout_apply_kernel(const uint32_t* __restrict__ bits, float scale, const AT* __restrict__ t,
                                                            const AT* __restrict__ aux, AT* __restrict__ y, int64_t rows, int64_t V,
                                                            int64_t nw) {
  const int64_t nq = rows * (V >> 2);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += stride) {
    const int64_t i = q * 4;
    const int64_t row = i / V, v = i - row * V;
    const uint32_t k = bits[row * nw + (v >> 5)] >> (v & 31);
    float a[4], r[4];
    aload<4>(t + i, a);
    if (KIND == FZ_DROP_RES) {
      if (aux != nullptr) {
        aload<4>(aux + i, r);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] += ((k >> e) & 1u) ? scale * a[e] : 0.f;
    } else if (KIND == FZ_DROP_GELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = ((k >> e) & 1u) ? scale * gelu_f(a[e]) : 0.f;
    } else {
      float z[4];
      aload<4>(aux + i, z);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = ((k >> e) & 1u) ? scale * a[e] * gelu_grad_f(z[e]) : 0.f;
    }
    astore<4>(y + i, r);
  }
}

static unsigned grid_for(int64_t n) {
  int64_t nb = (n + 255) / 256;
  if (nb < 1) nb = 1;
  if (nb > 256 * 16) nb = 256 * 16;
  return (unsigned)nb;
}

template <typename AT>
static int apply_launch(int kind, const uint32_t* bits, float scale, const void* t, const void* aux, void* y, int64_t rows, int64_t V,
                        hipStream_t st) {
  const int64_t nw = fz_dropout_bits_words(1, 1, V);
  const dim3 g(grid_for(rows * (V >> 2))), b(256);
  const AT* tt = (const AT*)t;
  const AT* aa = (const AT*)aux;
  AT* yy = (AT*)y;
  if (kind == FZ_DROP_RES) hipLaunchKernelGGL((dropout_apply_kernel<AT, FZ_DROP_RES>), g, b, 0, st, bits, scale, tt, aa, yy, rows, V, nw);
  else if (kind == FZ_DROP_GELU) hipLaunchKernelGGL((dropout_apply_kernel<AT, FZ_DROP_GELU>), g, b, 0, st, bits, scale, tt, aa, yy, rows, V, nw);
  else hipLaunchKernelGGL((dropout_apply_kernel<AT, FZ_DROP_GELU_BWD>), g, b, 0, st, bits, scale, tt, aa, yy, rows, V, nw);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

}  // namespace fz

using namespace fz;

extern "C" int64_t fz_dropout_bits_words(int B, int ch, int64_t V) {
  if (B < 0 || ch < 0 || V < 0) return -1;
  return (int64_t)B * ch * ((V + 31) / 32);
}

extern "C" int fz_dropout_keep_bits(const int64_t* seed, int site, int B, int ch, int64_t V, float p, uint32_t* out,
                                    fz_stream_t stream) {
  if (!seed || !out) return fail(FZ_E_ARG, "fz_dropout_keep_bits: null pointer");
  if (!(p >= 0.f && p < 1.f)) return fail(FZ_E_ARG, "fz_dropout_keep_bits: p must lie in [0, 1)");
  if (site < 0 || site > 2) return fail(FZ_E_ARG, "fz_dropout_keep_bits: site must be 0, 1 or 2");
  if (B < 0 || ch < 0 || V < 0) return fail(FZ_E_SHAPE, "fz_dropout_keep_bits: negative shape");
  if ((V >> 2) > 0xffffffffLL) return fail(FZ_E_SHAPE, "fz_dropout_keep_bits: more than 2^34 voxels per sample");
  const int64_t n = fz_dropout_bits_words(B, ch, V);
  if (n == 0) return FZ_OK;
  // thr = floor((1 - p) 2^32) in double (exact for a float p); p = 0 keeps every element (thr = 2^32)
  const uint64_t thr = (uint64_t)((1.0 - (double)p) * 4294967296.0);
  hipLaunchKernelGGL(dropout_bits_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, seed, site, B, ch, V,
                     (V + 31) / 32, thr, out);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_dropout_apply(int kind, const uint32_t* bits, float p, const void* t, const void* aux, void* y, int B, int ch,
                                int64_t V, int act_dtype, fz_stream_t stream) {
  if (kind != FZ_DROP_RES && kind != FZ_DROP_GELU && kind != FZ_DROP_GELU_BWD) return fail(FZ_E_ARG, "fz_dropout_apply: bad kind");
  if (!bits || !t || !y || (kind == FZ_DROP_GELU_BWD && !aux)) return fail(FZ_E_ARG, "fz_dropout_apply: null pointer");
  if (!(p >= 0.f && p < 1.f)) return fail(FZ_E_ARG, "fz_dropout_apply: p must lie in [0, 1)");
  if (B < 0 || ch < 0 || V < 0 || V % 4) return fail(FZ_E_SHAPE, "fz_dropout_apply: negative shape or V not a multiple of 4");
  const uintptr_t al = reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(aux) | reinterpret_cast<uintptr_t>(y);
  if (act_dtype != FZ_STORE_F32 && act_dtype != FZ_STORE_BF16) return fail(FZ_E_ARG, "fz_dropout_apply: bad act_dtype");
  if (al & (act_dtype == FZ_STORE_F32 ? 15 : 7)) return fail(FZ_E_ARG, "fz_dropout_apply: four-element alignment");
  const int64_t rows = (int64_t)B * ch;
  if (rows * V == 0) return FZ_OK;
  const float scale = (float)(1.0 / (1.0 - (double)p));
  if (act_dtype == FZ_STORE_F32) return apply_launch<float>(kind, bits, scale, t, aux, y, rows, V, (hipStream_t)stream);
  return apply_launch<bf16>(kind, bits, scale, t, aux, y, rows, V, (hipStream_t)stream);
}
