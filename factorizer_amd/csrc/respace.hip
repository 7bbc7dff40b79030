// respace.hip — resampling of a volume to the recipe's voxel spacing and of a prediction back to the file's grid, on device
// (semantics: factorizer_amd/respace.py).
//
// Orientationd(axcodes) -> Spacingd(pixdim, mode=[bilinear, nearest], align_corners=True, padding_mode="border") ->
// SpatialPadd(roi) of the ISLES22 bundles (model_zoo/factorizer_isles22/configs/train.yaml:97-116) and the
// Invertd(nearest_interp=false) -> AsDiscreted(threshold) of their postprocessing (inference.yaml:103-121).  Reorientation is
// a signed permutation of the axes and the respacing of an affine grid a scaling per axis, so the chain crop -> orient ->
// space -> pad and its inverse are MONOMIAL maps: each axis of the written grid reads one axis of the read grid, at a position
// that is linear in its own index.  Two kernel roles, both gathers with one writer per voxel and no atomics:
//   respace_fwd  walks the padded output: C image planes (bilinear or nearest, fp32 -> fp32 / bf16) and behind them L label
//                planes (uint8, nearest) in one launch; a pad voxel writes 0 without reading.
//   respace_inv  walks the file's grid: per corner the mean of K logit tensors (sum in list order times 1 / K), optionally
//                through the sigmoid; the corners interpolated; the value or `value >= threshold` written; a voxel outside
//                the box writes 0 without reading.
// A lane owns four voxels of one row of the written grid: the taps of the two slow axes are formed once per lane, those of
// the contiguous axis per voxel.  Positions are float64 (scale * index, clamped to the read extent), only the weight is
// rounded to fp32; the lerps are fma(f, v1 - v0, v0) in fp32 along the written grid's read axes 2, 1, 0 in that order.
// A full group is one vector store when the row length is a multiple of four and the base is aligned to the vector; plane
// bases are 64-bit and uniform per workgroup, offsets inside a plane 32-bit.  Where the axes are permuted so that the rows of
// the written grid read a strided axis, the workgroups take 2-D tiles that also span the written axis which reads the
// contiguous one (RespaceCover): neighbouring lanes then share cache lines again (profiles/respace.md).
#include <cmath>

#include "fz_common.h"

namespace fz {

// written axis w: indices lo .. lo + cnt - 1 have a source, o = index - lo (cnt - 1 - o with oflip) reads position scale * o
// of an axis of extent n whose elements lie `stride` apart (negative: the axis is read against its direction; `base` then
// starts at its far end)
struct RespaceGeomD {
  double scale[3];
  int out[3], lo[3], cnt[3], oflip[3], n[3], stride[3];
  int rd[3];   // read axis r (0 slowest, 2 contiguous) is supplied by written axis rd[r]
  int base;
};
struct RespacePtrs { const void* p[8]; };

struct RsTap { int a0, a1; float f; };   // element offsets of the two taps along one axis, weight of the second

template <bool NEAREST, int W>
__device__ __forceinline__ bool rs_tap(const RespaceGeomD& g, int idx, RsTap& t) {
  t.a0 = t.a1 = 0;
  t.f = 0.0f;
  const int64_t o64 = (int64_t)idx - g.lo[W];
  if (o64 < 0 || o64 >= g.cnt[W]) return false;
  const int o = (int)o64;
  const int oo = g.oflip[W] ? g.cnt[W] - 1 - o : o;
  const double top = (double)(g.n[W] - 1);
  double p = g.scale[W] * (double)oo;   // scale is finite and positive: p >= 0, never NaN
  p = p > top ? top : p;
  if constexpr (NEAREST) {
    t.a0 = t.a1 = (int)__builtin_rint(p) * g.stride[W];   // half to even; 0 <= rint(p) <= n - 1
  } else {
    const double fl = __builtin_floor(p);
    const int i0 = (int)fl, i1 = min(i0 + 1, g.n[W] - 1);
    t.a0 = i0 * g.stride[W];
    t.a1 = i1 * g.stride[W];
    t.f = (float)(p - fl);
  }
  return true;
}

__device__ __forceinline__ float rs_lerp(float f, float v0, float v1) { return fmaf(f, v1 - v0, v0); }

// the tap of written axis `ax` (0: z, 1: y, 2: x)
__device__ __forceinline__ RsTap rs_pick(int ax, const RsTap& tz, const RsTap& ty, const RsTap& tx) {
  return ax == 0 ? tz : (ax == 1 ? ty : tx);
}

__device__ __forceinline__ void rs_stv(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void rs_stv(bf16* p, const float (&v)[4]) {
  const f32v4 f = {v[0], v[1], v[2], v[3]};
  *reinterpret_cast<bf16v4*>(p) = __builtin_convertvector(f, bf16v4);   // round to nearest even
}
__device__ __forceinline__ void rs_stv(uint8_t* p, const float (&v)[4]) {
  *reinterpret_cast<unsigned*>(p) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
}
__device__ __forceinline__ void rs_st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void rs_st1(bf16* p, float v) { *p = (bf16)v; }
__device__ __forceinline__ void rs_st1(uint8_t* p, float v) { *p = (uint8_t)v; }

// the four voxels x0 .. x0 + 3 of row `row` of a plane: one vector store, or element by element up to the row's end
template <typename OT>
__device__ __forceinline__ void rs_store(OT* plane, int row, int x0, int Wd, bool vec, const float (&v)[4]) {
  OT* p = plane + (int64_t)row * Wd + x0;
  if (vec) {
    rs_stv(p, v);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x0 + k < Wd) rs_st1(p + k, v[k]);
  }
}

// How the lanes of a launch cover a written plane.  caxis < 0: linearly, 256 consecutive groups of four along the rows — right
// when the rows of the written grid read the contiguous axis of the read grid.  caxis = 0 / 1: that axis is read by written
// axis `caxis` instead, and a workgroup takes a tile of 16 groups along the row by 16 indices along `caxis`, each wave an
// 8 x 8 quarter of it: the eight lanes that are neighbours along `caxis` read neighbouring addresses (the same cache lines),
// the eight along the row still store 128 contiguous bytes.  nbx / nbc: tiles along the row / along caxis.
struct RespaceCover { int caxis, nbx, nbc, G, items; };

// this lane's row (z, y) and the first voxel x0 of its group; false when it has none
__device__ __forceinline__ bool rs_item(const RespaceGeomD& g, const RespaceCover& cv, int& row, int& z, int& y, int& x0) {
  if (cv.caxis < 0) {
    const int item = blockIdx.x * 256 + threadIdx.x;   // items < 2^30 + 2^28 (host-checked)
    if (item >= cv.items) return false;
    row = item / cv.G;
    x0 = 4 * (item - row * cv.G);
    z = row / g.out[1];
    y = row - z * g.out[1];
    return true;
  }
  const int t = threadIdx.x, wv = t >> 6, l = t & 63;
  int b = blockIdx.x;
  const int bo = b / (cv.nbx * cv.nbc);   // the index along the third axis
  b -= bo * cv.nbx * cv.nbc;
  const int bc = b / cv.nbx, bx = b - bc * cv.nbx;
  const int gx = bx * 16 + (wv & 1) * 8 + (l & 7), c = bc * 16 + (wv >> 1) * 8 + (l >> 3);
  if (gx >= cv.G || c >= (cv.caxis == 0 ? g.out[0] : g.out[1])) return false;
  z = cv.caxis == 0 ? c : bo;
  y = cv.caxis == 0 ? bo : c;
  row = z * g.out[1] + y;
  x0 = 4 * gx;
  return true;
}

// ---- respace_fwd ----------------------------------------------------------------------------------------------------------
template <typename OT, bool NEAREST>
__global__ __launch_bounds__(256) void respace_fwd_kernel(const float* __restrict__ img, OT* __restrict__ out,
                                                          const uint8_t* __restrict__ lab, uint8_t* __restrict__ lab_out,
                                                          int C, RespaceGeomD g, int64_t SV, int64_t PV, RespaceCover cv,
                                                          int vec_img, int vec_lab) {
  int row, z, y, x0;
  if (!rs_item(g, cv, row, z, y, x0)) return;
  const int plane = blockIdx.y, Wd = g.out[2];
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (plane < C) {
    RsTap tz, ty;
    const bool zin = rs_tap<NEAREST, 0>(g, z, tz), yin = rs_tap<NEAREST, 1>(g, y, ty);
    if (zin && yin) {
      const float* s = img + (int64_t)plane * SV + g.base;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        RsTap tx;
        if (x0 + k < Wd && rs_tap<NEAREST, 2>(g, x0 + k, tx)) {
          if constexpr (NEAREST) {
            v[k] = s[tz.a0 + ty.a0 + tx.a0];
          } else {
            const int r00 = tz.a0 + ty.a0, r01 = tz.a0 + ty.a1, r10 = tz.a1 + ty.a0, r11 = tz.a1 + ty.a1;
            const float c00 = rs_lerp(tx.f, s[r00 + tx.a0], s[r00 + tx.a1]);
            const float c01 = rs_lerp(tx.f, s[r01 + tx.a0], s[r01 + tx.a1]);
            const float c10 = rs_lerp(tx.f, s[r10 + tx.a0], s[r10 + tx.a1]);
            const float c11 = rs_lerp(tx.f, s[r11 + tx.a0], s[r11 + tx.a1]);
            v[k] = rs_lerp(tz.f, rs_lerp(ty.f, c00, c01), rs_lerp(ty.f, c10, c11));
          }
        }
      }
    }
    rs_store(out + (int64_t)plane * PV, row, x0, Wd, vec_img != 0, v);
  } else {
    const int kc = plane - C;
    RsTap tz, ty;
    const bool zin = rs_tap<true, 0>(g, z, tz), yin = rs_tap<true, 1>(g, y, ty);
    if (zin && yin) {
      const uint8_t* s = lab + (int64_t)kc * SV + g.base;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        RsTap tx;
        if (x0 + k < Wd && rs_tap<true, 2>(g, x0 + k, tx)) v[k] = (float)s[tz.a0 + ty.a0 + tx.a0];
      }
    }
    rs_store(lab_out + (int64_t)kc * PV, row, x0, Wd, vec_lab != 0, v);
  }
}

// ---- respace_inv ----------------------------------------------------------------------------------------------------------
// the ensemble value of one corner: fp32 sum in list order times 1 / K, optionally through the sigmoid
template <typename T>
__device__ __forceinline__ float rs_corner(const RespacePtrs& lp, int K, float inv_k, int sigmoid, int64_t pb, int at) {
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < K) s += (float)(static_cast<const T*>(lp.p[j]) + pb)[at];   // pb: the plane, uniform
  s *= inv_k;
  return sigmoid ? 1.0f / (1.0f + expf(-s)) : s;
}

template <typename T, typename OT>
__global__ __launch_bounds__(256) void respace_inv_kernel(RespacePtrs lp, int K, float inv_k, int sigmoid, RespaceGeomD g,
                                                          int64_t SV, int64_t PV, RespaceCover cv, float threshold,
                                                          OT* __restrict__ res, int vec) {
  int row, z, y, x0;
  if (!rs_item(g, cv, row, z, y, x0)) return;
  const int plane = blockIdx.y, Wd = g.out[2];
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  RsTap tz, ty;
  const bool zin = rs_tap<false, 0>(g, z, tz), yin = rs_tap<false, 1>(g, y, ty);
  if (zin && yin) {
    const int64_t pb = (int64_t)plane * SV + g.base;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      RsTap tx;
      if (x0 + k < Wd && rs_tap<false, 2>(g, x0 + k, tx)) {
        // corners and lerps in the axis order of the grid that is read (its contiguous axis first), whichever written axis
        // supplies each: g.rd is uniform, the picks are selects
        const RsTap t0 = rs_pick(g.rd[0], tz, ty, tx), t1 = rs_pick(g.rd[1], tz, ty, tx), t2 = rs_pick(g.rd[2], tz, ty, tx);
        const int r00 = t0.a0 + t1.a0, r01 = t0.a0 + t1.a1, r10 = t0.a1 + t1.a0, r11 = t0.a1 + t1.a1;
        const float c00 = rs_lerp(t2.f, rs_corner<T>(lp, K, inv_k, sigmoid, pb, r00 + t2.a0), rs_corner<T>(lp, K, inv_k, sigmoid, pb, r00 + t2.a1));
        const float c01 = rs_lerp(t2.f, rs_corner<T>(lp, K, inv_k, sigmoid, pb, r01 + t2.a0), rs_corner<T>(lp, K, inv_k, sigmoid, pb, r01 + t2.a1));
        const float c10 = rs_lerp(t2.f, rs_corner<T>(lp, K, inv_k, sigmoid, pb, r10 + t2.a0), rs_corner<T>(lp, K, inv_k, sigmoid, pb, r10 + t2.a1));
        const float c11 = rs_lerp(t2.f, rs_corner<T>(lp, K, inv_k, sigmoid, pb, r11 + t2.a0), rs_corner<T>(lp, K, inv_k, sigmoid, pb, r11 + t2.a1));
        const float r = rs_lerp(t0.f, rs_lerp(t1.f, c00, c01), rs_lerp(t1.f, c10, c11));
        if constexpr (sizeof(OT) == 1) v[k] = r >= threshold ? 1.0f : 0.0f;
        else v[k] = r;
      }
    }
  }
  rs_store(res + (int64_t)plane * PV, row, x0, Wd, vec != 0, v);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static const char* respace_geom_error(const fz_respace_geom* g) {
  if (!g) return "null geometry";
  if (g->nd < 1 || g->nd > 3) return "1 <= nd <= 3 spatial axes";
  int seen = 0;
  int64_t SV = 1, PV = 1, OV = 1;
  for (int w = 0; w < 3; ++w) {
    const int a = g->src_axis[w];
    if (a < 0 || a > 2 || ((seen >> a) & 1)) return "src_axis must be a permutation of the axes";
    seen |= 1 << a;
    if (g->src_size[w] < 1 || g->res_size[w] < 1 || g->out[w] < 1 || g->orig_size[w] < 1 || g->pad[w] < 0)
      return "sizes must be positive, pads non-negative";
    if ((int64_t)g->pad[w] + g->res_size[w] > g->out[w]) return "pad + resampled size exceeds the padded extent";
    if (!(g->scale[w] > 0.0) || !(g->inv_scale[w] > 0.0) || !std::isfinite(g->scale[w]) || !std::isfinite(g->inv_scale[w]))
      return "scales must be positive and finite";
    if (g->box_start[w] < -(1 << 30) || g->box_start[w] > (1 << 30)) return "box out of range";
    if (w < 3 - g->nd && (a != w || g->src_size[w] != 1 || g->res_size[w] != 1 || g->out[w] != 1 || g->orig_size[w] != 1 ||
                          g->pad[w] != 0 || g->box_start[w] != 0 || g->flip[w] != 0 || g->scale[w] != 1.0 ||
                          g->inv_scale[w] != 1.0))
      return "the lifted axes of a 1-D / 2-D grid must be size 1, unpermuted, unflipped, pad 0, scale 1";
    SV *= g->src_size[w];
    PV *= g->out[w];
    OV *= g->orig_size[w];
    if (SV >= ((int64_t)1 << 31) || PV >= ((int64_t)1 << 31) || OV >= ((int64_t)1 << 31))
      return "a plane must hold fewer than 2^31 voxels";
  }
  return nullptr;
}

// the cover of a written (n0, n1, n2) plane whose axis `caxis` reads the contiguous axis of the read grid (2: its rows do) and
// the workgroups it takes; false when the plane is too large
static bool respace_cover(const int* n, int caxis, RespaceCover* cv, unsigned* blocks) {
  cv->G = (n[2] + 3) / 4;
  const int64_t it = (int64_t)n[0] * n[1] * cv->G;
  if (it >= ((int64_t)1 << 30) + ((int64_t)1 << 28)) return false;
  cv->items = (int)it;
  cv->caxis = caxis == 2 ? -1 : caxis;
  cv->nbx = (cv->G + 15) / 16;
  cv->nbc = cv->caxis < 0 ? 1 : (n[cv->caxis] + 15) / 16;
  const int64_t nb = cv->caxis < 0 ? (it + 255) / 256 : (int64_t)cv->nbx * cv->nbc * n[1 - cv->caxis];
  if (nb >= ((int64_t)1 << 31)) return false;
  *blocks = (unsigned)nb;
  return true;
}

// the forward map: the padded resampled grid reads the source grid
static RespaceGeomD respace_fwd_geom(const fz_respace_geom* g) {
  RespaceGeomD d;
  const int sstride[3] = {g->src_size[1] * g->src_size[2], g->src_size[2], 1};
  d.base = 0;
  for (int w = 0; w < 3; ++w) {
    const int a = g->src_axis[w];
    d.scale[w] = g->scale[w];
    d.out[w] = g->out[w]; d.lo[w] = g->pad[w]; d.cnt[w] = g->res_size[w]; d.oflip[w] = 0;
    d.n[w] = g->src_size[a];
    d.stride[w] = g->flip[w] ? -sstride[a] : sstride[a];
    if (g->flip[w]) d.base += (g->src_size[a] - 1) * sstride[a];
    d.rd[w] = w;   // the lerps run in the order of the written (oriented) axes
  }
  return d;
}

// the inverse map: the file's grid reads the padded resampled grid
static RespaceGeomD respace_inv_geom(const fz_respace_geom* g) {
  RespaceGeomD d;
  const int pstride[3] = {g->out[1] * g->out[2], g->out[2], 1};
  d.base = 0;
  for (int w = 0; w < 3; ++w) {
    const int a = g->src_axis[w];
    d.scale[a] = g->inv_scale[w];
    d.out[a] = g->orig_size[a]; d.lo[a] = g->box_start[a]; d.cnt[a] = g->src_size[a]; d.oflip[a] = g->flip[w] ? 1 : 0;
    d.n[a] = g->res_size[w];
    d.stride[a] = pstride[w];
    d.base += g->pad[w] * pstride[w];
    d.rd[w] = a;
  }
  return d;
}

}  // namespace fz

using namespace fz;

extern "C" int fz_vol_respace(const float* image, int C, void* out, int out_kind, const uint8_t* label, int L,
                              uint8_t* label_out, const fz_respace_geom* geom, int mode, fz_stream_t stream) {
  if (const char* e = respace_geom_error(geom)) {
    last_error() = std::string("fz_vol_respace: ") + e;
    return FZ_E_ARG;
  }
  if (mode != FZ_RESPACE_BILINEAR && mode != FZ_RESPACE_NEAREST) return fail(FZ_E_ARG, "fz_vol_respace: mode must be bilinear or nearest");
  if (out_kind != FZ_VOL_F32 && out_kind != FZ_VOL_BF16) return fail(FZ_E_ARG, "fz_vol_respace: out kind must be fp32 or bf16");
  if (C < 1 || L < 0 || C + L > 65535) return fail(FZ_E_SHAPE, "fz_vol_respace: 1 <= C, 0 <= L, C + L <= 65535");
  if (!image || !out) return fail(FZ_E_ARG, "fz_vol_respace: null pointer");
  if (L > 0 && (!label || !label_out)) return fail(FZ_E_ARG, "fz_vol_respace: label and label_out go together");
  const int oes = out_kind == FZ_VOL_F32 ? 4 : 2;
  if (((uintptr_t)image % 4) != 0 || ((uintptr_t)out % (uintptr_t)oes) != 0) return fail(FZ_E_ARG, "fz_vol_respace: pointer not aligned to its element");
  int caxis = 2;   // the resampled axis that reads the source's contiguous axis
  for (int w = 0; w < 3; ++w)
    if (geom->src_axis[w] == 2) caxis = w;
  RespaceCover cv;
  unsigned blocks;
  if (!respace_cover(geom->out, caxis, &cv, &blocks)) return fail(FZ_E_SHAPE, "fz_vol_respace: padded plane too large");
  const RespaceGeomD gd = respace_fwd_geom(geom);
  const int64_t SV = (int64_t)geom->src_size[0] * geom->src_size[1] * geom->src_size[2];
  const int64_t PV = (int64_t)geom->out[0] * geom->out[1] * geom->out[2];
  const bool rows4 = geom->out[2] % 4 == 0;   // then every row of every plane starts a multiple of four elements from the base
  const int vec_img = rows4 && ((uintptr_t)out % (uintptr_t)(4 * oes)) == 0;
  const int vec_lab = rows4 && L > 0 && ((uintptr_t)label_out % 4) == 0;
  bool unit = true;
  for (int w = 0; w < 3; ++w) unit = unit && geom->scale[w] == 1.0;
  const bool nearest = mode == FZ_RESPACE_NEAREST || unit;   // unit scales: every position is an index, the copy is exact
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(blocks, (unsigned)(C + L)), block(256);
  if (out_kind == FZ_VOL_F32) {
    if (nearest) hipLaunchKernelGGL((respace_fwd_kernel<float, true>), grid, block, 0, s, image, (float*)out, label, label_out, C, gd, SV, PV, cv, vec_img, vec_lab);
    else hipLaunchKernelGGL((respace_fwd_kernel<float, false>), grid, block, 0, s, image, (float*)out, label, label_out, C, gd, SV, PV, cv, vec_img, vec_lab);
  } else {
    if (nearest) hipLaunchKernelGGL((respace_fwd_kernel<bf16, true>), grid, block, 0, s, image, (bf16*)out, label, label_out, C, gd, SV, PV, cv, vec_img, vec_lab);
    else hipLaunchKernelGGL((respace_fwd_kernel<bf16, false>), grid, block, 0, s, image, (bf16*)out, label, label_out, C, gd, SV, PV, cv, vec_img, vec_lab);
  }
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_vol_unspace(const void* const* logits, int K, int kind, int C, const fz_respace_geom* geom, int sigmoid,
                              int discretize, float threshold, void* result, fz_stream_t stream) {
  if (K < 1 || K > 8) return fail(FZ_E_ARG, "fz_vol_unspace: 1 <= K <= 8 logit tensors");
  if (const char* e = respace_geom_error(geom)) {
    last_error() = std::string("fz_vol_unspace: ") + e;
    return FZ_E_ARG;
  }
  if (kind != FZ_VOL_F32 && kind != FZ_VOL_BF16) return fail(FZ_E_ARG, "fz_vol_unspace: logits must be fp32 or bf16");
  if (threshold != threshold) return fail(FZ_E_ARG, "fz_vol_unspace: threshold is NaN");
  if (C < 1 || C > 65535) return fail(FZ_E_SHAPE, "fz_vol_unspace: 1 <= C <= 65535");
  if (!logits || !result) return fail(FZ_E_ARG, "fz_vol_unspace: null pointer");
  const int es = kind == FZ_VOL_F32 ? 4 : 2;
  RespacePtrs lp;
  for (int k = 0; k < 8; ++k) {
    lp.p[k] = k < K ? logits[k] : nullptr;
    if (k < K && (!logits[k] || ((uintptr_t)logits[k] % (uintptr_t)es) != 0)) return fail(FZ_E_ARG, "fz_vol_unspace: null or unaligned logits");
  }
  if (!discretize && ((uintptr_t)result % 4) != 0) return fail(FZ_E_ARG, "fz_vol_unspace: pointer not aligned to its element");
  RespaceCover cv;
  unsigned blocks;   // the file's axis src_axis[2] reads the contiguous axis of the logits
  if (!respace_cover(geom->orig_size, geom->src_axis[2], &cv, &blocks)) return fail(FZ_E_SHAPE, "fz_vol_unspace: plane too large");
  const RespaceGeomD gd = respace_inv_geom(geom);
  const int64_t SV = (int64_t)geom->out[0] * geom->out[1] * geom->out[2];
  const int64_t PV = (int64_t)geom->orig_size[0] * geom->orig_size[1] * geom->orig_size[2];
  const int vec = geom->orig_size[2] % 4 == 0 && ((uintptr_t)result % (uintptr_t)(discretize ? 4 : 16)) == 0;
  const float inv_k = (float)(1.0 / K);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(blocks, (unsigned)C), block(256);
  if (kind == FZ_VOL_F32) {
    if (discretize) hipLaunchKernelGGL((respace_inv_kernel<float, uint8_t>), grid, block, 0, s, lp, K, inv_k, sigmoid, gd, SV, PV, cv, threshold, (uint8_t*)result, vec);
    else hipLaunchKernelGGL((respace_inv_kernel<float, float>), grid, block, 0, s, lp, K, inv_k, sigmoid, gd, SV, PV, cv, threshold, (float*)result, vec);
  } else {
    if (discretize) hipLaunchKernelGGL((respace_inv_kernel<bf16, uint8_t>), grid, block, 0, s, lp, K, inv_k, sigmoid, gd, SV, PV, cv, threshold, (uint8_t*)result, vec);
    else hipLaunchKernelGGL((respace_inv_kernel<bf16, float>), grid, block, 0, s, lp, K, inv_k, sigmoid, gd, SV, PV, cv, threshold, (float*)result, vec);
  }
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
