// loss_ds.hip — the Dice + CE / Dice + BCE passes of loss.hip for one COARSE level of a deep-supervision head list
// (ft.DeepSupervisionLoss): logits (B, C, Ld, Lh, Lw), target at FULL resolution (B, C, Td, Th, Tw) with Tk = rk·Lk on every
// axis.  The level's target is the nearest-exact down-sampling of MONAI 1.4 DeepSupervisionLoss — for an integer ratio the
// strided pick  t_l[z, y, x] = t[rz·z + rz/2, ry·y + ry/2, rx·x + rx/2]  — read THROUGH that index map, in the target's own
// element type (fp32, bf16, one byte), converted in registers: no down-sampled target is ever written.
// Everything else is loss.hip's: the arithmetic per voxel, the chunking (fz_dice_bce_chunks), the order of every sum and the
// layout of the partials, so fz_dice_ce_finish and the host finish turn these partials into the loss and the coefficients
// unchanged.  No atomics: one partial per (plane | batch item, chunk), combined in a fixed order.
#include "fz_common.h"

namespace fz {

// target extents (the depth extent is implied: plane = Td·Th·Tw), level extents and the ratios, axes lifted to three
struct DsGeom {
  int64_t plane;   // Td·Th·Tw: elements of one (b, c) target plane
  int Th, Tw, Lh, Lw, rz, ry, rx;
};

__device__ __forceinline__ float ds_tval(const float* p) { return *p; }
__device__ __forceinline__ float ds_tval(const bf16* p) { return (float)*p; }
__device__ __forceinline__ float ds_tval(const uint8_t* p) { return (float)*p; }

// Offsets into a target plane of the 4 consecutive level elements v .. v + 3: ONE division chain for the first, the other
// three by carry (a level row may be shorter than 4, so every step can carry).  Offsets are 64-bit: a 2^31-element target
// plane is a 1290^3 volume, the level itself (V < 2^31, checked by the host) is indexed in 32 bits.
__device__ __forceinline__ void ds_offsets(uint32_t v, const DsGeom& g, int64_t (&off)[4]) {
  const uint32_t hw = (uint32_t)g.Lh * (uint32_t)g.Lw;
  int z = (int)(v / hw);
  const uint32_t r = v - (uint32_t)z * hw;
  int y = (int)(r / (uint32_t)g.Lw);
  int x = (int)(r - (uint32_t)y * (uint32_t)g.Lw);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    off[e] = ((int64_t)(g.rz * z + (g.rz >> 1)) * g.Th + (g.ry * y + (g.ry >> 1))) * g.Tw + (g.rx * x + (g.rx >> 1));
    if (++x == g.Lw) {
      x = 0;
      if (++y == g.Lh) y = 0, ++z;
    }
  }
}

// ---- one prediction channel per plane: dice_bce_sums_kernel / dice_bce_grad_kernel of loss.hip ----
template <typename TT>
__global__ __launch_bounds__(256) void dice_bce_ds_sums_kernel(const float* __restrict__ z, const TT* __restrict__ t,
                                                               float* __restrict__ part, int64_t V, int nchunk, DsGeom g) {
  __shared__ float red[4][4];
  const int plane = blockIdx.x, chunk = blockIdx.y;
  const int64_t per = ((V / 4 + nchunk - 1) / nchunk) * 4;
  const int64_t v0 = chunk * per, v1 = min(V, v0 + per);
  const float* zp = z + (int64_t)plane * V;
  const TT* tp = t + (int64_t)plane * g.plane;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t v = v0 + threadIdx.x * 4; v < v1; v += 1024) {
    const float4 zz = *reinterpret_cast<const float4*>(zp + v);
    int64_t off[4];
    ds_offsets((uint32_t)v, g, off);
    const float zs[4] = {zz.x, zz.y, zz.z, zz.w};
    const float ts[4] = {ds_tval(tp + off[0]), ds_tval(tp + off[1]), ds_tval(tp + off[2]), ds_tval(tp + off[3])};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float az = fabsf(zs[e]);
      const float ex = __expf(-az);                 // e^{-|z|}
      const float p = zs[e] >= 0.f ? 1.0f / (1.0f + ex) : ex / (1.0f + ex);
      s[0] += p * ts[e];
      s[1] += p * p;
      s[2] += ts[e] * ts[e];
      s[3] += fmaxf(zs[e], 0.f) - zs[e] * ts[e] + log1pf(ex);  // stable BCE with logits
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float r = wave_sum(s[e]);
    if (lane == 0) red[wave][e] = r;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int e = threadIdx.x;
    part[((int64_t)plane * nchunk + chunk) * 4 + e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
  }
}

template <typename TT>
__global__ __launch_bounds__(256) void dice_bce_ds_grad_kernel(const float* __restrict__ z, const TT* __restrict__ t,
                                                               const float* __restrict__ coef, float* __restrict__ gz,
                                                               int64_t V, int64_t total, float cd, float cb,
                                                               const float* __restrict__ gscale, DsGeom g) {
  const float gs = gscale ? gscale[0] : 1.0f;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < total;
       i += (int64_t)gridDim.x * blockDim.x * 4) {
    const int plane = (int)(i / V);
    const float num = coef[plane * 2], den = coef[plane * 2 + 1];
    const float4 zz = *reinterpret_cast<const float4*>(z + i);
    const TT* tp = t + (int64_t)plane * g.plane;
    int64_t off[4];
    ds_offsets((uint32_t)(i - (int64_t)plane * V), g, off);
    const float zs[4] = {zz.x, zz.y, zz.z, zz.w};
    const float ts[4] = {ds_tval(tp + off[0]), ds_tval(tp + off[1]), ds_tval(tp + off[2]), ds_tval(tp + off[3])};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ex = __expf(-fabsf(zs[e]));
      const float p = zs[e] >= 0.f ? 1.0f / (1.0f + ex) : ex / (1.0f + ex);
      const float ddp = -2.0f * ts[e] / den + num * 2.0f * p / (den * den);
      o[e] = gs * (cd * ddp * p * (1.0f - p) + cb * (p - ts[e]));
    }
    *reinterpret_cast<float4*>(gz + i) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ---- C = 2 .. 8 channels: dice_ce_sums_kernel / dice_ce_grad_kernel of loss.hip; the C channels of a voxel share its offset ----
template <int C, typename TT>
__global__ __launch_bounds__(256) void dice_ce_ds_sums_kernel(const float* __restrict__ z, const TT* __restrict__ t,
                                                              float* __restrict__ part, int64_t V, int nchunk, DsGeom g) {
  __shared__ float red[4][3 * C + 1];
  const int b = blockIdx.x, chunk = blockIdx.y;
  const int64_t per = ((V / 4 + nchunk - 1) / nchunk) * 4;
  const int64_t v0 = chunk * per, v1 = min(V, v0 + per);
  const float* zp = z + (int64_t)b * C * V;
  const TT* tp = t + (int64_t)b * C * g.plane;
  float s[3 * C + 1];
#pragma unroll
  for (int i = 0; i < 3 * C + 1; ++i) s[i] = 0.f;
  for (int64_t v = v0 + threadIdx.x * 4; v < v1; v += 1024) {
    int64_t off[4];
    ds_offsets((uint32_t)v, g, off);
    float zs[C][4], ts[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float4 zz = *reinterpret_cast<const float4*>(zp + c * V + v);
      zs[c][0] = zz.x, zs[c][1] = zz.y, zs[c][2] = zz.z, zs[c][3] = zz.w;
#pragma unroll
      for (int e = 0; e < 4; ++e) ts[c][e] = ds_tval(tp + c * g.plane + off[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float mx = zs[0][e];
#pragma unroll
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, zs[c][e]);
      float se = 0.f, st = 0.f, stz = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float zc = zs[c][e], tc = ts[c][e];
        se += __expf(zc - mx);
        st += tc;
        stz += tc * zc;
        const float ex = __expf(-fabsf(zc));
        const float p = zc >= 0.f ? 1.0f / (1.0f + ex) : ex / (1.0f + ex);
        s[3 * c + 0] += p * tc;
        s[3 * c + 1] += p * p;
        s[3 * c + 2] += tc * tc;
      }
      s[3 * C] += st * (mx + __logf(se)) - stz;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 3 * C + 1; ++i) {
    const float r = wave_sum(s[i]);
    if (lane == 0) red[wave][i] = r;
  }
  __syncthreads();
  if (threadIdx.x < 3 * C + 1) {
    const int i = threadIdx.x;
    part[((int64_t)b * nchunk + chunk) * (3 * C + 1) + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
  }
}

template <int C, typename TT>
__global__ __launch_bounds__(256) void dice_ce_ds_grad_kernel(const float* __restrict__ z, const TT* __restrict__ t,
                                                              const float* __restrict__ coef, float* __restrict__ gz,
                                                              int64_t V, int B, float cd, float cb,
                                                              const float* __restrict__ gscale, DsGeom g) {
  const float gs = gscale ? gscale[0] : 1.0f;
  const int64_t total = (int64_t)B * V;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < total;
       i += (int64_t)gridDim.x * blockDim.x * 4) {
    const int b = (int)(i / V);
    const int64_t v = i - (int64_t)b * V;
    const int64_t base = (int64_t)b * C * V + v;
    const TT* tp = t + (int64_t)b * C * g.plane;
    int64_t off[4];
    ds_offsets((uint32_t)v, g, off);
    float zs[C][4], ts[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float4 zz = *reinterpret_cast<const float4*>(z + base + c * V);
      zs[c][0] = zz.x, zs[c][1] = zz.y, zs[c][2] = zz.z, zs[c][3] = zz.w;
#pragma unroll
      for (int e = 0; e < 4; ++e) ts[c][e] = ds_tval(tp + c * g.plane + off[e]);
    }
    float o[C][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float mx = zs[0][e];
#pragma unroll
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, zs[c][e]);
      float ez[C], se = 0.f, st = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        ez[c] = __expf(zs[c][e] - mx);
        se += ez[c];
        st += ts[c][e];
      }
      const float inv = st / se;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float zc = zs[c][e], tc = ts[c][e];
        const float num = coef[(b * C + c) * 2], den = coef[(b * C + c) * 2 + 1];
        const float ex = __expf(-fabsf(zc));
        const float p = zc >= 0.f ? 1.0f / (1.0f + ex) : ex / (1.0f + ex);
        const float ddp = -2.0f * tc / den + num * 2.0f * p / (den * den);
        o[c][e] = gs * (cd * ddp * p * (1.0f - p) + cb * (ez[c] * inv - tc));
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
      *reinterpret_cast<float4*>(gz + base + c * V) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
  }
}

// Geometry from the plain ints of the ABI; 0 on success.  V: the level's voxels per plane.
static int ds_geom(const char* who, int Td, int Th, int Tw, int Ld, int Lh, int Lw, int tkind, DsGeom* g, int64_t* V) {
  const char* why = nullptr;
  if (Td < 1 || Th < 1 || Tw < 1 || Ld < 1 || Lh < 1 || Lw < 1) why = "extents must be positive";
  else if (Td % Ld || Th % Lh || Tw % Lw) why = "every target extent must be a multiple of the level's";
  else if (tkind != FZ_SEG_F32 && tkind != FZ_SEG_BF16 && tkind != FZ_SEG_U8) why = "target kind must be FZ_SEG_F32 / _BF16 / _U8";
  else {
    *V = (int64_t)Ld * Lh * Lw;
    if (*V < 4 || (*V % 4) || *V > INT32_MAX) why = "level voxels must be a multiple of 4 below 2^31";
  }
  if (why) return fail(FZ_E_SHAPE, (std::string(who) + ": " + why).c_str());
  g->plane = (int64_t)Td * Th * Tw;
  g->Th = Th, g->Tw = Tw, g->Lh = Lh, g->Lw = Lw;
  g->rz = Td / Ld, g->ry = Th / Lh, g->rx = Tw / Lw;
  return FZ_OK;
}

}  // namespace fz

using namespace fz;

// Host dispatch over the target's element kind and the channel count: f(DsType<TT>{}) / f(DsInt<C>{}).
template <typename T> struct DsType { using type = T; };
template <int N> struct DsInt { static constexpr int value = N; };
template <typename F>
static void ds_by_kind(int tkind, F f) {
  if (tkind == FZ_SEG_F32) f(DsType<float>{});
  else if (tkind == FZ_SEG_BF16) f(DsType<bf16>{});
  else f(DsType<uint8_t>{});
}
template <typename F>
static bool ds_by_channels(int C, F f) {
  switch (C) {
    case 2: f(DsInt<2>{}); return true;
    case 3: f(DsInt<3>{}); return true;
    case 4: f(DsInt<4>{}); return true;
    case 5: f(DsInt<5>{}); return true;
    case 6: f(DsInt<6>{}); return true;
    case 7: f(DsInt<7>{}); return true;
    case 8: f(DsInt<8>{}); return true;
    default: return false;
  }
}

// part: (planes, fz_dice_bce_chunks(V), 4) as fz_dice_bce_sums writes it
extern "C" int fz_dice_bce_ds_sums(const float* z, const void* t, float* part, int planes, int Td, int Th, int Tw, int Ld,
                                   int Lh, int Lw, int tkind, fz_stream_t stream) {
  if (!z || !t || !part) return fail(FZ_E_ARG, "fz_dice_bce_ds_sums: null pointer");
  if (planes < 1) return fail(FZ_E_SHAPE, "fz_dice_bce_ds_sums: bad sizes");
  DsGeom g;
  int64_t V;
  if (int rc = ds_geom("fz_dice_bce_ds_sums", Td, Th, Tw, Ld, Lh, Lw, tkind, &g, &V)) return rc;
  const int nchunk = fz_dice_bce_chunks(V);
  ds_by_kind(tkind, [&](auto tt) {
    using TT = typename decltype(tt)::type;
    hipLaunchKernelGGL(dice_bce_ds_sums_kernel<TT>, dim3(planes, nchunk), dim3(256), 0, (hipStream_t)stream, z,
                       static_cast<const TT*>(t), part, V, nchunk, g);
  });
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_dice_bce_ds_grad(const float* z, const void* t, const float* coef, float* gz, int planes, int Td, int Th,
                                   int Tw, int Ld, int Lh, int Lw, int tkind, float cd, float cb, const float* gscale,
                                   fz_stream_t stream) {
  if (!z || !t || !coef || !gz) return fail(FZ_E_ARG, "fz_dice_bce_ds_grad: null pointer");
  if (planes < 1) return fail(FZ_E_SHAPE, "fz_dice_bce_ds_grad: bad sizes");
  DsGeom g;
  int64_t V;
  if (int rc = ds_geom("fz_dice_bce_ds_grad", Td, Th, Tw, Ld, Lh, Lw, tkind, &g, &V)) return rc;
  const int64_t total = (int64_t)planes * V;
  int64_t blocks = (total / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  ds_by_kind(tkind, [&](auto tt) {
    using TT = typename decltype(tt)::type;
    hipLaunchKernelGGL(dice_bce_ds_grad_kernel<TT>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z,
                       static_cast<const TT*>(t), coef, gz, V, total, cd, cb, gscale, g);
  });
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

// part: (B, fz_dice_bce_chunks(V), 3C+1) as fz_dice_ce_sums writes it
extern "C" int fz_dice_ce_ds_sums(const float* z, const void* t, float* part, int B, int C, int Td, int Th, int Tw, int Ld,
                                  int Lh, int Lw, int tkind, fz_stream_t stream) {
  if (!z || !t || !part) return fail(FZ_E_ARG, "fz_dice_ce_ds_sums: null pointer");
  if (B < 1) return fail(FZ_E_SHAPE, "fz_dice_ce_ds_sums: bad sizes");
  DsGeom g;
  int64_t V;
  if (int rc = ds_geom("fz_dice_ce_ds_sums", Td, Th, Tw, Ld, Lh, Lw, tkind, &g, &V)) return rc;
  const int nchunk = fz_dice_bce_chunks(V);
  const bool ok = ds_by_channels(C, [&](auto cc) {
    ds_by_kind(tkind, [&](auto tt) {
      using TT = typename decltype(tt)::type;
      hipLaunchKernelGGL((dice_ce_ds_sums_kernel<decltype(cc)::value, TT>), dim3(B, nchunk), dim3(256), 0,
                         (hipStream_t)stream, z, static_cast<const TT*>(t), part, V, nchunk, g);
    });
  });
  if (!ok) return fail(FZ_E_UNSUPPORTED, "fz_dice_ce_ds_sums: 2 <= C <= 8");
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_dice_ce_ds_grad(const float* z, const void* t, const float* coef, float* gz, int B, int C, int Td, int Th,
                                  int Tw, int Ld, int Lh, int Lw, int tkind, float cd, float cb, const float* gscale,
                                  fz_stream_t stream) {
  if (!z || !t || !coef || !gz) return fail(FZ_E_ARG, "fz_dice_ce_ds_grad: null pointer");
  if (B < 1) return fail(FZ_E_SHAPE, "fz_dice_ce_ds_grad: bad sizes");
  DsGeom g;
  int64_t V;
  if (int rc = ds_geom("fz_dice_ce_ds_grad", Td, Th, Tw, Ld, Lh, Lw, tkind, &g, &V)) return rc;
  int64_t blocks = ((int64_t)B * V / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  const bool ok = ds_by_channels(C, [&](auto cc) {
    ds_by_kind(tkind, [&](auto tt) {
      using TT = typename decltype(tt)::type;
      hipLaunchKernelGGL((dice_ce_ds_grad_kernel<decltype(cc)::value, TT>), dim3((unsigned)blocks), dim3(256), 0,
                         (hipStream_t)stream, z, static_cast<const TT*>(t), coef, gz, V, B, cd, cb, gscale, g);
    });
  });
  if (!ok) return fail(FZ_E_UNSUPPORTED, "fz_dice_ce_ds_grad: 2 <= C <= 8");
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
