// volprep.hip — volume preparation and prediction restore of the recipe on device (semantics:
// factorizer_amd/volume.py).
//
// `deterministic_transforms` of the bundles (model_zoo/factorizer_brats23/configs/train.yaml:86-116, inference.yaml:57-83):
// CropForegroundd(margin) -> NormalizeIntensityd(nonzero, channel_wise) -> BraTSOneHotEncoderd -> SpatialPadd(roi), and the
// inference `postprocessing` (inference.yaml:104-125): MeanEnsembled -> Activationsd(sigmoid) -> Invertd -> AsDiscreted ->
// label map.  Four kernel roles, all streaming:
//   vol_bbox     one pass over the image: a voxel counts when its value is > 0 (the hull over all channels is the box of "any
//                channel > 0"); integer min / max per axis per lane -> per wave -> LDS atomics -> six global atomicMin / atomicMax.
//   vol_stats    two passes over the part of the box inside the image: float64 (count, sum) per workgroup, then the sum of
//                squares about the float64 mean, which every workgroup first forms from the (count, sum) partials in a fixed
//                order.  No float atomics; the number of partials follows from the box shape alone.
//   vol_write    prologue: mean and std from the partials (fixed order), rounded once to fp32; body: the cropped, normalised
//                ((x - mean) / std, IEEE division), zero-padded image, and in the same launch the encoded, cropped, padded
//                label (class sets as 32-bit membership masks).
//   vol_restore  the mean of K logit tensors (sum in list order times 1 / K), the decision value >= bound, pasted through the
//                box into the original extent — every voxel of the result is written, so nothing is cleared first.
// The input passes (bbox, stats) walk rows of the region in groups of four elements aligned to 16 bytes (fp32; 8 bytes
// int16) IN MEMORY, whatever the row length and the alignment of the buffer: a group that lies wholly inside its row is one
// vector load, the at most two groups per row that straddle its ends read element by element under a bounds test.  The
// output passes (write, restore) walk the OUTPUT in such groups (one vector store each) and read their sources element by
// element: consecutive lanes read consecutive addresses, but source and destination rows are not aligned to each other.
#include <climits>

#include "fz_common.h"

namespace fz {

constexpr int VOL_ITEMS = 2048;        // groups of four elements per workgroup of the input passes (8 per thread)
constexpr int VOL_MAX_CHUNKS = 1024;   // partials per channel at most: the per-workgroup items grow beyond it

// the part of a plane an input pass walks: nd x nh rows of nw elements from (z0, y0, x0) of a (., H, W) plane of V voxels
struct VolRegion {
  int H, W, z0, y0, x0, nh, nw, G;   // G: groups per row, (nw + 3) / 4 + 1 covers every alignment of a row start
  int64_t V;
};

// geometry of vol_write / vol_restore (fz_vol_geom with the box as start + extent)
struct VolGeomD {
  int size[3], start[3], bs[3], pad[3], out[3];
};
struct VolMasks { unsigned m[8]; };
struct VolPtrs { const void* p[8]; };
struct VolVals { unsigned char v[8]; };

template <typename T> __device__ __forceinline__ unsigned vol_mis(const T* p) {
  return (unsigned)((uintptr_t)p / sizeof(T)) & 3u;   // elements between the last 4-element boundary of memory and p
}

__device__ __forceinline__ void vol_ldv(const float* p, float (&v)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void vol_ldv(const int16_t* p, float (&v)[4]) {
  const uint2 w = *reinterpret_cast<const uint2*>(p);
  v[0] = (float)(int16_t)(w.x & 0xffffu); v[1] = (float)(int16_t)(w.x >> 16);
  v[2] = (float)(int16_t)(w.y & 0xffffu); v[3] = (float)(int16_t)(w.y >> 16);
}

// elements g .. g + 3 of base as floats; bit k of the result says element k lies in [lo, hi) (others read as 0, untouched)
template <typename T>
__device__ __forceinline__ unsigned vol_load4(const T* base, int64_t g, int64_t lo, int64_t hi, float (&v)[4]) {
  if (g >= lo && g + 4 <= hi) {
    vol_ldv(base + g, v);
    return 0xfu;
  }
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = g + k;
    const bool ok = i >= lo && i < hi;
    v[k] = ok ? (float)base[i] : 0.0f;
    m |= (unsigned)ok << k;
  }
  return m;
}

// item -> its row (z, y relative to the region) and the group g with its row bounds [lo, hi), all as element indices of base
__device__ __forceinline__ void vol_item(const VolRegion& rg, int plane, unsigned mis, int item, int& z, int& y, int64_t& g,
                                         int64_t& lo, int64_t& hi) {
  const int r = item / rg.G, j = item - r * rg.G;
  z = r / rg.nh;
  y = r - z * rg.nh;
  lo = (int64_t)plane * rg.V + ((int64_t)(rg.z0 + z) * rg.H + (rg.y0 + y)) * rg.W + rg.x0;
  hi = lo + rg.nw;
  g = ((lo + mis) & ~(int64_t)3) - mis + 4 * (int64_t)j;
}

// ---- vol_bbox -----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void vol_bbox_kernel(const T* __restrict__ img, VolRegion rg, int items, int per,
                                                       int* __restrict__ box) {
  __shared__ int sb[6];
  const int t = threadIdx.x, plane = blockIdx.y;
  if (t < 6) sb[t] = t < 3 ? INT_MAX : -1;
  __syncthreads();
  const unsigned mis = vol_mis(img);
  int mnz = INT_MAX, mny = INT_MAX, mnx = INT_MAX, mxz = -1, mxy = -1, mxx = -1;
  const int i1 = min(items, (int)min((int64_t)INT_MAX, ((int64_t)blockIdx.x + 1) * per));
  for (int it = blockIdx.x * per + t; it < i1; it += 256) {
    int z, y;
    int64_t g, lo, hi;
    vol_item(rg, plane, mis, it, z, y, g, lo, hi);
    if (g >= hi || g + 4 <= lo) continue;
    float v[4];
    const unsigned m = vol_load4(img, g, lo, hi, v);
    unsigned pos = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) pos |= (unsigned)(v[k] > 0.0f) << k;
    pos &= m;
    if (pos) {
      const int x = (int)(g - lo);   // region x of element 0 of the group (>= -3)
      mnx = min(mnx, x + (int)__builtin_ctz(pos));
      mxx = max(mxx, x + 31 - (int)__builtin_clz(pos));
      mny = min(mny, y); mxy = max(mxy, y);
      mnz = min(mnz, z); mxz = max(mxz, z);
    }
  }
  // the wave's extremes by butterfly (64 lanes on one LDS word would take their turns), then one lane per wave
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    mnz = min(mnz, __shfl_xor(mnz, d)); mny = min(mny, __shfl_xor(mny, d)); mnx = min(mnx, __shfl_xor(mnx, d));
    mxz = max(mxz, __shfl_xor(mxz, d)); mxy = max(mxy, __shfl_xor(mxy, d)); mxx = max(mxx, __shfl_xor(mxx, d));
  }
  if ((t & 63) == 0 && mxx >= 0) {   // integer atomics: the result does not depend on the order
    atomicMin(&sb[0], mnz + rg.z0); atomicMin(&sb[1], mny + rg.y0); atomicMin(&sb[2], mnx + rg.x0);
    atomicMax(&sb[3], mxz + rg.z0); atomicMax(&sb[4], mxy + rg.y0); atomicMax(&sb[5], mxx + rg.x0);
  }
  __syncthreads();
  if (t < 6 && sb[5] >= 0) {
    // a minimum only falls and a maximum only rises: a workgroup that cannot move the value it reads skips its atomic (a few
    // thousand workgroups on six words of one cache line otherwise queue behind each other)
    const int cur = __hip_atomic_load(box + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t < 3) {
      if (sb[t] < cur) atomicMin(box + t, sb[t]);
    } else {
      if (sb[t] > cur) atomicMax(box + t, sb[t]);
    }
  }
}

// ---- vol_stats ----------------------------------------------------------------------------------------------------------
// total of one value per thread, in every thread: a fixed tree over LDS
__device__ __forceinline__ double vol_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();   // red may still be read from the previous call
  red[t] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  return red[0];
}
// sum of n doubles p[0], p[stride], ...: thread t adds t, t + 256, ... in index order, then the tree
__device__ __forceinline__ double vol_sum_partials(const double* p, int n, int stride, double* red) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += p[(int64_t)i * stride];
  return vol_block_sum(s, red);
}

// workspace: cs (C, nchunk, 2) float64 = (count, sum) of a workgroup, then ss (C, nchunk) = its centred sum of squares.
// The statistics of channel c run over the partials of c (channel_wise) or of all channels; `extra`: the selected zeros the
// box holds outside the image (nonzero = 0 only), which add to the count and, each with mean^2, to the sum of squares.
struct VolStat { double count, mean; };
__device__ __forceinline__ VolStat vol_mean(const double* ws, int c, int C, int nchunk, int channel_wise, double extra,
                                            double* red) {
  const double* cs = ws + (channel_wise ? (int64_t)c * nchunk * 2 : 0);
  const int n = channel_wise ? nchunk : C * nchunk;
  VolStat st;
  st.count = vol_sum_partials(cs, n, 2, red) + extra;
  const double sum = vol_sum_partials(cs + 1, n, 2, red);
  st.mean = st.count > 0.0 ? sum / st.count : 0.0;
  return st;
}

template <typename T, int PASS>
__global__ __launch_bounds__(256) void vol_stats_kernel(const T* __restrict__ img, VolRegion rg, int items, int per,
                                                        int nchunk, int C, int nonzero, int channel_wise, double extra,
                                                        double* __restrict__ ws) {
  __shared__ double red[256];
  const int t = threadIdx.x, plane = blockIdx.y, chunk = blockIdx.x;
  double mean = 0.0;
  if constexpr (PASS == 2) mean = vol_mean(ws, plane, C, nchunk, channel_wise, extra, red).mean;
  const unsigned mis = vol_mis(img);
  double acc = 0.0;
  unsigned cnt = 0;
  const int i1 = min(items, (int)min((int64_t)INT_MAX, ((int64_t)chunk + 1) * per));
  for (int it = chunk * per + t; it < i1; it += 256) {
    int z, y;
    int64_t g, lo, hi;
    vol_item(rg, plane, mis, it, z, y, g, lo, hi);
    if (g >= hi || g + 4 <= lo) continue;
    float v[4];
    const unsigned m = vol_load4(img, g, lo, hi, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool sel = ((m >> k) & 1u) && (!nonzero || v[k] != 0.0f);
      if constexpr (PASS == 1) {
        acc += sel ? (double)v[k] : 0.0;
        cnt += sel;
      } else {
        const double d = (double)v[k] - mean;
        acc += sel ? d * d : 0.0;
      }
    }
  }
  const double total = vol_block_sum(acc, red);
  if constexpr (PASS == 1) {
    const double n = vol_block_sum((double)cnt, red);   // a workgroup sees fewer than 2^32 elements: exact
    if (t == 0) {
      ws[((int64_t)plane * nchunk + chunk) * 2] = n;
      ws[((int64_t)plane * nchunk + chunk) * 2 + 1] = total;
    }
  } else {
    if (t == 0) ws[(int64_t)C * nchunk * 2 + (int64_t)plane * nchunk + chunk] = total;
  }
}

// ---- vol_write ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void vol_stv(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void vol_stv(bf16* p, const float (&v)[4]) {
  const f32v4 f = {v[0], v[1], v[2], v[3]};
  *reinterpret_cast<bf16v4*>(p) = __builtin_convertvector(f, bf16v4);   // round to nearest even
}
__device__ __forceinline__ void vol_st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void vol_st1(bf16* p, float v) { *p = (bf16)v; }

// walks the flat indices q, q + 1, ... of a (n0, n1, n2) volume: coordinates of the current one, then a step
struct VolWalk {
  int c0, c1, c2, n1, n2;
  __device__ __forceinline__ VolWalk(int64_t q, int n1_, int n2_) : n1(n1_), n2(n2_) {
    const unsigned q32 = (unsigned)q, r = q32 / (unsigned)n2_;   // a plane holds fewer than 2^31 voxels (host-checked)
    c2 = (int)(q32 - r * (unsigned)n2_);
    c0 = (int)(r / (unsigned)n1_);
    c1 = (int)(r - (unsigned)c0 * (unsigned)n1_);
  }
  __device__ __forceinline__ void step() {
    if (++c2 == n2) {
      c2 = 0;
      if (++c1 == n1) { c1 = 0; ++c0; }
    }
  }
};

// source of a prepared voxel (p0, p1, p2): inbox, and its in-plane image offset (or -1 where the box leaves the image)
__device__ __forceinline__ bool vol_source(const VolGeomD& g, int p0, int p1, int p2, int64_t& src) {
  const int b0 = p0 - g.pad[0], b1 = p1 - g.pad[1], b2 = p2 - g.pad[2];
  const bool inbox = b0 >= 0 && b0 < g.bs[0] && b1 >= 0 && b1 < g.bs[1] && b2 >= 0 && b2 < g.bs[2];
  src = -1;
  if (inbox) {   // only here is b + start an image coordinate (within the box it cannot overflow)
    const int i0 = b0 + g.start[0], i1 = b1 + g.start[1], i2 = b2 + g.start[2];
    if (i0 >= 0 && i0 < g.size[0] && i1 >= 0 && i1 < g.size[1] && i2 >= 0 && i2 < g.size[2])
      src = ((int64_t)i0 * g.size[1] + i1) * g.size[2] + i2;
  }
  return inbox;
}

template <typename T, typename OT, typename LT>
__global__ __launch_bounds__(256) void vol_write_kernel(const T* __restrict__ img, OT* __restrict__ out,
                                                        const LT* __restrict__ lab, unsigned char* __restrict__ lab_out,
                                                        VolMasks masks, int label_channels, int C, VolGeomD g, int nchunk,
                                                        int nonzero, int channel_wise, double extra,
                                                        const double* __restrict__ ws, float* __restrict__ mean_out,
                                                        float* __restrict__ std_out) {
  __shared__ double red[256];
  const int t = threadIdx.x, plane = blockIdx.y;
  const int64_t V = (int64_t)g.size[0] * g.size[1] * g.size[2], PV = (int64_t)g.out[0] * g.out[1] * g.out[2];
  if (plane < C) {
    // statistics of the channel from the partials, in the order every workgroup and every run uses
    const VolStat st = vol_mean(ws, plane, C, nchunk, channel_wise, extra, red);
    const double* ss = ws + (int64_t)C * nchunk * 2 + (channel_wise ? (int64_t)plane * nchunk : 0);
    const double sq = vol_sum_partials(ss, channel_wise ? nchunk : C * nchunk, 1, red) + extra * st.mean * st.mean;
    float mean = 0.0f, sd = 1.0f;
    if (st.count > 0.0) {
      mean = (float)st.mean;
      sd = (float)sqrt(sq / st.count);
      if (sd == 0.0f) sd = 1.0f;
    }
    if (blockIdx.x == 0 && t == 0) { mean_out[plane] = mean; std_out[plane] = sd; }
    const unsigned mis = vol_mis(out);
    const int64_t lo = (int64_t)plane * PV, hi = lo + PV;
    const int64_t g0 = ((lo + mis) & ~(int64_t)3) - mis;
    const int64_t ngroups = (hi - g0 + 3) / 4;
    const T* ip = img + (int64_t)plane * V;
    for (int64_t gi = (int64_t)blockIdx.x * 256 + t; gi < ngroups; gi += (int64_t)gridDim.x * 256) {
      const int64_t a = g0 + 4 * gi;
      VolWalk w(max(a, lo) - lo, g.out[1], g.out[2]);
      float v[4];
      unsigned m = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = a + k >= lo && a + k < hi;
        float r = 0.0f;
        if (ok) {
          int64_t src;
          const bool inbox = vol_source(g, w.c0, w.c1, w.c2, src);
          const float x = src >= 0 ? (float)ip[src] : 0.0f;
          r = inbox ? ((!nonzero || x != 0.0f) ? (x - mean) / sd : x) : 0.0f;
          w.step();
        }
        v[k] = r;
        m |= (unsigned)ok << k;
      }
      if (m == 0xfu) {
        vol_stv(out + a, v);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if ((m >> k) & 1u) vol_st1(out + a + k, v[k]);
      }
    }
  } else {
    const int kc = plane - C;
    unsigned cm = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j == kc) cm = masks.m[j];
    const unsigned mis = vol_mis(lab_out);
    const int64_t lo = (int64_t)kc * PV, hi = lo + PV;
    const int64_t g0 = ((lo + mis) & ~(int64_t)3) - mis;
    const int64_t ngroups = (hi - g0 + 3) / 4;
    const LT* lp = lab + (label_channels ? (int64_t)kc * V : 0);
    for (int64_t gi = (int64_t)blockIdx.x * 256 + t; gi < ngroups; gi += (int64_t)gridDim.x * 256) {
      const int64_t a = g0 + 4 * gi;
      VolWalk w(max(a, lo) - lo, g.out[1], g.out[2]);
      unsigned word = 0, m = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = a + k >= lo && a + k < hi;
        unsigned r = 0;
        if (ok) {
          int64_t src;
          vol_source(g, w.c0, w.c1, w.c2, src);
          if (src >= 0) {
            const int l = (int)lp[src];
            if (label_channels) r = (unsigned)l & 0xffu;
            else r = (l >= 0 && l < 32) ? (cm >> l) & 1u : 0u;
          }
          w.step();
        }
        word |= r << (8 * k);
        m |= (unsigned)ok << k;
      }
      if (m == 0xfu) {
        *reinterpret_cast<unsigned*>(lab_out + a) = word;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if ((m >> k) & 1u) lab_out[a + k] = (unsigned char)((word >> (8 * k)) & 0xffu);
      }
    }
  }
}

// ---- vol_restore --------------------------------------------------------------------------------------------------------
template <typename T, bool MAP>
__global__ __launch_bounds__(256) void vol_restore_kernel(VolPtrs lp, int K, float inv_k, int C, VolGeomD g, float bound,
                                                          VolVals vals, unsigned char* __restrict__ res) {
  const int t = threadIdx.x, plane = blockIdx.y;
  const int64_t V = (int64_t)g.size[0] * g.size[1] * g.size[2], PV = (int64_t)g.out[0] * g.out[1] * g.out[2];
  const unsigned mis = vol_mis(res);
  const int64_t lo = (int64_t)plane * V, hi = lo + V;
  const int64_t g0 = ((lo + mis) & ~(int64_t)3) - mis;
  const int64_t ngroups = (hi - g0 + 3) / 4;
  for (int64_t gi = (int64_t)blockIdx.x * 256 + t; gi < ngroups; gi += (int64_t)gridDim.x * 256) {
    const int64_t a = g0 + 4 * gi;
    VolWalk w(max(a, lo) - lo, g.size[1], g.size[2]);
    unsigned word = 0, m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = a + k >= lo && a + k < hi;
      unsigned r = 0;
      if (ok) {
        // start + bs is the box end (<= 2^30, host-checked); the differences are formed inside the box only
        if (w.c0 >= g.start[0] && w.c0 < g.start[0] + g.bs[0] && w.c1 >= g.start[1] && w.c1 < g.start[1] + g.bs[1] &&
            w.c2 >= g.start[2] && w.c2 < g.start[2] + g.bs[2]) {
          const int b0 = w.c0 - g.start[0], b1 = w.c1 - g.start[1], b2 = w.c2 - g.start[2];
          const int64_t src = ((int64_t)(b0 + g.pad[0]) * g.out[1] + (b1 + g.pad[1])) * g.out[2] + (b2 + g.pad[2]);
          if constexpr (MAP) {
            bool found = false;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
              if (c < C) {
                float s = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                  if (j < K) s += (float)static_cast<const T*>(lp.p[j])[(int64_t)c * PV + src];
                if (!found && s * inv_k >= bound) { r = vals.v[c]; found = true; }
              }
            }
          } else {
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (j < K) s += (float)static_cast<const T*>(lp.p[j])[(int64_t)plane * PV + src];
            r = s * inv_k >= bound ? 1u : 0u;
          }
        }
        w.step();
      }
      word |= r << (8 * k);
      m |= (unsigned)ok << k;
    }
    if (m == 0xfu) {
      *reinterpret_cast<unsigned*>(res + a) = word;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((m >> k) & 1u) res[a + k] = (unsigned char)((word >> (8 * k)) & 0xffu);
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static int vol_esize(int kind) { return kind == FZ_VOL_F32 ? 4 : (kind == FZ_VOL_U8 ? 1 : 2); }
static bool vol_aligned(const void* p, int kind) { return ((uintptr_t)p % (uintptr_t)vol_esize(kind)) == 0; }

// nullptr when the geometry is consistent, else what is wrong with it
static const char* vol_geom_error(const fz_vol_geom* g) {
  if (!g) return "null geometry";
  if (g->nd < 1 || g->nd > 3) return "1 <= nd <= 3 spatial axes";
  int64_t V = 1, PV = 1;
  for (int a = 0; a < 3; ++a) {
    if (g->size[a] < 1 || g->out[a] < 1 || g->pad[a] < 0) return "sizes must be positive, pads non-negative";
    if (g->end[a] <= g->start[a]) return "empty box";
    if (g->start[a] < -(1 << 30) || g->end[a] > (1 << 30)) return "box out of range";
    if (g->start[a] >= g->size[a] || g->end[a] <= 0) return "the box holds no voxel of the image";
    if ((int64_t)g->pad[a] + (g->end[a] - g->start[a]) > g->out[a]) return "pad + box exceeds the prepared extent";
    if (a < 3 - g->nd && (g->size[a] != 1 || g->start[a] != 0 || g->end[a] != 1 || g->pad[a] != 0 || g->out[a] != 1))
      return "the lifted axes of a 1-D / 2-D image must be size 1, box [0, 1), pad 0, out 1";
    V *= g->size[a];
    PV *= g->out[a];
    if (V >= ((int64_t)1 << 31) || PV >= ((int64_t)1 << 31)) return "a plane must hold fewer than 2^31 voxels";
  }
  return nullptr;
}

static VolGeomD vol_geom_device(const fz_vol_geom* g) {
  VolGeomD d;
  for (int a = 0; a < 3; ++a) {
    d.size[a] = g->size[a]; d.start[a] = g->start[a]; d.bs[a] = g->end[a] - g->start[a];
    d.pad[a] = g->pad[a]; d.out[a] = g->out[a];
  }
  return d;
}

// the region [lo, hi) of a (D, H, W) plane and its split into workgroups; false when its items do not fit 31 bits
static bool vol_region(const int* size, const int* lo, const int* hi, VolRegion* rg, int* items, int* per, int* nchunk) {
  rg->H = size[1]; rg->W = size[2];
  rg->z0 = lo[0]; rg->y0 = lo[1]; rg->x0 = lo[2];
  rg->nh = hi[1] - lo[1]; rg->nw = hi[2] - lo[2];
  rg->G = (rg->nw + 3) / 4 + 1;
  rg->V = (int64_t)size[0] * size[1] * size[2];
  const int64_t n = (int64_t)(hi[0] - lo[0]) * rg->nh * rg->G;
  if (n >= ((int64_t)1 << 31) - 4096) return false;
  int64_t p = VOL_ITEMS;
  if ((n + p - 1) / p > VOL_MAX_CHUNKS) p = (((n + VOL_MAX_CHUNKS - 1) / VOL_MAX_CHUNKS + 255) / 256) * 256;
  *items = (int)n;
  *per = (int)p;
  *nchunk = (int)((n + p - 1) / p);
  return true;
}

// the box clipped to the image, as a region; extra = box voxels outside the image (per channel)
static bool vol_box_region(const fz_vol_geom* g, VolRegion* rg, int* items, int* per, int* nchunk, double* extra) {
  int lo[3], hi[3];
  double in = 1.0, all = 1.0;
  for (int a = 0; a < 3; ++a) {
    lo[a] = g->start[a] > 0 ? g->start[a] : 0;
    hi[a] = g->end[a] < g->size[a] ? g->end[a] : g->size[a];
    in *= hi[a] - lo[a];
    all *= (double)g->end[a] - g->start[a];
  }
  if (extra) *extra = all - in;
  return vol_region(g->size, lo, hi, rg, items, per, nchunk);
}

template <typename T, typename OT>
static void vol_write_launch(int label_kind, dim3 grid, hipStream_t s, const void* img, void* out, const void* lab,
                             uint8_t* lab_out, const VolMasks& masks, int label_channels, int C, const VolGeomD& gd,
                             int nchunk, int nonzero, int channel_wise, double extra, const double* ws, float* mean,
                             float* sd) {
  if (label_kind == FZ_VOL_I16)
    hipLaunchKernelGGL((vol_write_kernel<T, OT, int16_t>), grid, dim3(256), 0, s, (const T*)img, (OT*)out,
                       (const int16_t*)lab, lab_out, masks, label_channels, C, gd, nchunk, nonzero, channel_wise, extra, ws,
                       mean, sd);
  else
    hipLaunchKernelGGL((vol_write_kernel<T, OT, uint8_t>), grid, dim3(256), 0, s, (const T*)img, (OT*)out,
                       (const uint8_t*)lab, lab_out, masks, label_channels, C, gd, nchunk, nonzero, channel_wise, extra, ws,
                       mean, sd);
}

}  // namespace fz

using namespace fz;

extern "C" int fz_vol_kind_ok(int role, int kind) {
  switch (role) {
    case FZ_VOL_ROLE_IMAGE_IN: return kind == FZ_VOL_F32 || kind == FZ_VOL_I16;
    case FZ_VOL_ROLE_IMAGE_OUT: return kind == FZ_VOL_F32 || kind == FZ_VOL_BF16;
    case FZ_VOL_ROLE_LABEL_IN: return kind == FZ_VOL_U8 || kind == FZ_VOL_I16;
    case FZ_VOL_ROLE_LOGITS: return kind == FZ_VOL_F32 || kind == FZ_VOL_BF16;
    default: return 0;
  }
}

extern "C" int fz_vol_bbox(const void* image, int kind, int C, int nd, int D, int H, int W, int32_t* box,
                           fz_stream_t stream) {
  if (nd < 1 || nd > 3) return fail(FZ_E_ARG, "fz_vol_bbox: 1 <= nd <= 3 spatial axes");
  if (!fz_vol_kind_ok(FZ_VOL_ROLE_IMAGE_IN, kind)) return fail(FZ_E_ARG, "fz_vol_bbox: image kind must be fp32 or int16");
  if (C < 1 || C > 65535 || D < 1 || H < 1 || W < 1) return fail(FZ_E_SHAPE, "fz_vol_bbox: sizes must be positive, C <= 65535");
  if ((nd < 3 && D != 1) || (nd < 2 && H != 1)) return fail(FZ_E_SHAPE, "fz_vol_bbox: the lifted axes of a 1-D / 2-D image must be 1");
  if ((int64_t)D * H * W >= ((int64_t)1 << 31)) return fail(FZ_E_SHAPE, "fz_vol_bbox: a plane must hold fewer than 2^31 voxels");
  if (!image || !box) return fail(FZ_E_ARG, "fz_vol_bbox: null pointer");
  if (!vol_aligned(image, kind) || ((uintptr_t)box % 4) != 0) return fail(FZ_E_ARG, "fz_vol_bbox: pointer not aligned to its element");
  const int size[3] = {D, H, W}, lo[3] = {0, 0, 0};
  VolRegion rg;
  int items, per, nchunk;
  if (!vol_region(size, lo, size, &rg, &items, &per, &nchunk)) return fail(FZ_E_SHAPE, "fz_vol_bbox: image too large");
  hipStream_t s = (hipStream_t)stream;
  FZ_HIP_OK(hipMemsetAsync(box, 0x7f, 3 * sizeof(int32_t), s));        // minima: 0x7f7f7f7f, above every coordinate
  FZ_HIP_OK(hipMemsetAsync(box + 3, 0xff, 3 * sizeof(int32_t), s));    // maxima: -1
  const dim3 grid(nchunk, C), block(256);
  if (kind == FZ_VOL_F32) hipLaunchKernelGGL(vol_bbox_kernel<float>, grid, block, 0, s, (const float*)image, rg, items, per, box);
  else hipLaunchKernelGGL(vol_bbox_kernel<int16_t>, grid, block, 0, s, (const int16_t*)image, rg, items, per, box);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int64_t fz_vol_workspace_bytes(int C, const fz_vol_geom* geom) {
  if (C < 1 || C > 65535 || vol_geom_error(geom)) return -1;
  VolRegion rg;
  int items, per, nchunk;
  if (!vol_box_region(geom, &rg, &items, &per, &nchunk, nullptr)) return -1;
  return (int64_t)C * nchunk * 3 * (int64_t)sizeof(double);
}

extern "C" int fz_vol_stats(const void* image, int kind, int C, const fz_vol_geom* geom, int nonzero, int channel_wise,
                            void* workspace, fz_stream_t stream) {
  if (const char* e = vol_geom_error(geom)) {
    last_error() = std::string("fz_vol_stats: ") + e;
    return FZ_E_ARG;
  }
  if (!fz_vol_kind_ok(FZ_VOL_ROLE_IMAGE_IN, kind)) return fail(FZ_E_ARG, "fz_vol_stats: image kind must be fp32 or int16");
  if (C < 1 || C > 65535) return fail(FZ_E_SHAPE, "fz_vol_stats: 1 <= C <= 65535");
  if (!image || !workspace) return fail(FZ_E_ARG, "fz_vol_stats: null pointer");
  if (!vol_aligned(image, kind) || ((uintptr_t)workspace % 8) != 0) return fail(FZ_E_ARG, "fz_vol_stats: pointer not aligned to its element");
  VolRegion rg;
  int items, per, nchunk;
  double extra;
  if (!vol_box_region(geom, &rg, &items, &per, &nchunk, &extra)) return fail(FZ_E_SHAPE, "fz_vol_stats: box too large");
  extra = nonzero ? 0.0 : (channel_wise ? extra : extra * C);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(nchunk, C), block(256);
  double* ws = (double*)workspace;
  if (kind == FZ_VOL_F32) {
    hipLaunchKernelGGL((vol_stats_kernel<float, 1>), grid, block, 0, s, (const float*)image, rg, items, per, nchunk, C, nonzero, channel_wise, extra, ws);
    FZ_LAUNCH_CHECK();
    hipLaunchKernelGGL((vol_stats_kernel<float, 2>), grid, block, 0, s, (const float*)image, rg, items, per, nchunk, C, nonzero, channel_wise, extra, ws);
    FZ_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL((vol_stats_kernel<int16_t, 1>), grid, block, 0, s, (const int16_t*)image, rg, items, per, nchunk, C, nonzero, channel_wise, extra, ws);
    FZ_LAUNCH_CHECK();
    hipLaunchKernelGGL((vol_stats_kernel<int16_t, 2>), grid, block, 0, s, (const int16_t*)image, rg, items, per, nchunk, C, nonzero, channel_wise, extra, ws);
    FZ_LAUNCH_CHECK();
  }
  return FZ_OK;
}

extern "C" int fz_vol_write(const void* image, int kind, void* out, int out_kind, int C, const void* label, int label_kind,
                            int label_channels, const int* class_ids, const int* class_counts, int nclass,
                            uint8_t* label_out, const fz_vol_geom* geom, int nonzero, int channel_wise,
                            const void* workspace, float* mean, float* stdev, fz_stream_t stream) {
  if (const char* e = vol_geom_error(geom)) {
    last_error() = std::string("fz_vol_write: ") + e;
    return FZ_E_ARG;
  }
  if (!fz_vol_kind_ok(FZ_VOL_ROLE_IMAGE_IN, kind) || !fz_vol_kind_ok(FZ_VOL_ROLE_IMAGE_OUT, out_kind))
    return fail(FZ_E_ARG, "fz_vol_write: image kind must be fp32 or int16, out kind fp32 or bf16");
  if (C < 1 || C > 65535) return fail(FZ_E_SHAPE, "fz_vol_write: 1 <= C <= 65535");
  VolMasks masks;
  for (int k = 0; k < 8; ++k) masks.m[k] = 0;
  int lplanes = 0;
  if (label || label_out) {
    if (label_channels < 0 || C + label_channels > 65535) return fail(FZ_E_SHAPE, "fz_vol_write: bad label_channels");
    if (label_channels == 0) {
      if (nclass < 1 || nclass > 8) return fail(FZ_E_ARG, "fz_vol_write: 1 <= class sets <= 8");
      if (!class_ids || !class_counts) return fail(FZ_E_ARG, "fz_vol_write: null class table");
      int at = 0;
      for (int k = 0; k < nclass; ++k) {
        if (class_counts[k] < 0 || class_counts[k] > 32) return fail(FZ_E_ARG, "fz_vol_write: bad class count");
        for (int j = 0; j < class_counts[k]; ++j, ++at) {
          if (class_ids[at] < 0 || class_ids[at] >= 32) return fail(FZ_E_ARG, "fz_vol_write: class id must be in 0 .. 31");
          masks.m[k] |= 1u << class_ids[at];
        }
      }
      if (!fz_vol_kind_ok(FZ_VOL_ROLE_LABEL_IN, label_kind)) return fail(FZ_E_ARG, "fz_vol_write: label kind must be uint8 or int16");
      lplanes = nclass;
    } else {
      if (label_kind != FZ_VOL_U8) return fail(FZ_E_ARG, "fz_vol_write: a channel-first label must be uint8");
      lplanes = label_channels;
    }
    if (!label || !label_out) return fail(FZ_E_ARG, "fz_vol_write: label and label_out go together");
    if (!vol_aligned(label, label_kind)) return fail(FZ_E_ARG, "fz_vol_write: pointer not aligned to its element");
  }
  if (!image || !out || !workspace || !mean || !stdev) return fail(FZ_E_ARG, "fz_vol_write: null pointer");
  if (!vol_aligned(image, kind) || !vol_aligned(out, out_kind) || ((uintptr_t)workspace % 8) != 0 ||
      ((uintptr_t)mean % 4) != 0 || ((uintptr_t)stdev % 4) != 0)
    return fail(FZ_E_ARG, "fz_vol_write: pointer not aligned to its element");
  VolRegion rg;
  int items, per, nchunk;
  double extra;
  if (!vol_box_region(geom, &rg, &items, &per, &nchunk, &extra)) return fail(FZ_E_SHAPE, "fz_vol_write: box too large");
  extra = nonzero ? 0.0 : (channel_wise ? extra : extra * C);
  const VolGeomD gd = vol_geom_device(geom);
  const int64_t PV = (int64_t)gd.out[0] * gd.out[1] * gd.out[2];
  int64_t blocks = (PV / 4 + 1 + 2047) / 2048;   // eight groups per thread: the prologue is paid once per 8192 elements
  if (blocks > 1024) blocks = 1024;
  const dim3 grid((unsigned)blocks, C + lplanes);
  hipStream_t s = (hipStream_t)stream;
  const double* ws = (const double*)workspace;
  if (kind == FZ_VOL_F32) {
    if (out_kind == FZ_VOL_F32)
      vol_write_launch<float, float>(label_kind, grid, s, image, out, label, label_out, masks, label_channels, C, gd, nchunk, nonzero, channel_wise, extra, ws, mean, stdev);
    else
      vol_write_launch<float, bf16>(label_kind, grid, s, image, out, label, label_out, masks, label_channels, C, gd, nchunk, nonzero, channel_wise, extra, ws, mean, stdev);
  } else {
    if (out_kind == FZ_VOL_F32)
      vol_write_launch<int16_t, float>(label_kind, grid, s, image, out, label, label_out, masks, label_channels, C, gd, nchunk, nonzero, channel_wise, extra, ws, mean, stdev);
    else
      vol_write_launch<int16_t, bf16>(label_kind, grid, s, image, out, label, label_out, masks, label_channels, C, gd, nchunk, nonzero, channel_wise, extra, ws, mean, stdev);
  }
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_vol_restore(const void* const* logits, int K, int kind, int C, const fz_vol_geom* geom, float bound,
                              const uint8_t* label_values, uint8_t* result, fz_stream_t stream) {
  if (K < 1 || K > 8) return fail(FZ_E_ARG, "fz_vol_restore: 1 <= K <= 8 logit tensors");
  if (const char* e = vol_geom_error(geom)) {
    last_error() = std::string("fz_vol_restore: ") + e;
    return FZ_E_ARG;
  }
  if (!fz_vol_kind_ok(FZ_VOL_ROLE_LOGITS, kind)) return fail(FZ_E_ARG, "fz_vol_restore: logits must be fp32 or bf16");
  if (bound != bound) return fail(FZ_E_ARG, "fz_vol_restore: bound is NaN");
  if (C < 1 || C > 65535) return fail(FZ_E_SHAPE, "fz_vol_restore: 1 <= C <= 65535");
  if (label_values && C > 8) return fail(FZ_E_UNSUPPORTED, "fz_vol_restore: the label map form takes at most 8 channels");
  if (!logits || !result) return fail(FZ_E_ARG, "fz_vol_restore: null pointer");
  VolPtrs lp;
  for (int k = 0; k < 8; ++k) {
    lp.p[k] = k < K ? logits[k] : nullptr;
    if (k < K && (!logits[k] || !vol_aligned(logits[k], kind))) return fail(FZ_E_ARG, "fz_vol_restore: null or unaligned logits");
  }
  VolVals vals;
  for (int c = 0; c < 8; ++c) vals.v[c] = label_values && c < C ? label_values[c] : 0;
  const VolGeomD gd = vol_geom_device(geom);
  const int64_t V = (int64_t)gd.size[0] * gd.size[1] * gd.size[2];
  int64_t blocks = (V / 4 + 1 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  const float inv_k = (float)(1.0 / K);
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(256);
  if (label_values) {
    const dim3 grid((unsigned)blocks, 1);
    if (kind == FZ_VOL_F32) hipLaunchKernelGGL((vol_restore_kernel<float, true>), grid, block, 0, s, lp, K, inv_k, C, gd, bound, vals, result);
    else hipLaunchKernelGGL((vol_restore_kernel<bf16, true>), grid, block, 0, s, lp, K, inv_k, C, gd, bound, vals, result);
  } else {
    const dim3 grid((unsigned)blocks, C);
    if (kind == FZ_VOL_F32) hipLaunchKernelGGL((vol_restore_kernel<float, false>), grid, block, 0, s, lp, K, inv_k, C, gd, bound, vals, result);
    else hipLaunchKernelGGL((vol_restore_kernel<bf16, false>), grid, block, 0, s, lp, K, inv_k, C, gd, bound, vals, result);
  }
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
