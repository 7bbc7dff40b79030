// loss.hip — fused Dice + BCE-with-logits / Dice + CE loss for the segmentation head (training step of
// BASELINE configs[3]).  Restates the bundle's DiceCELoss(sigmoid=True, squared_pred=True)
// (model_zoo/factorizer_brats23/configs/train.yaml:67-70; MONAI is not importable, so the exact
// reduction conventions are this build's: mean over (b,c) of the soft-Dice term + mean BCE):
//   p = sigmoid(z);  dice_bc = 1 - (2 Σ p t + s) / (Σ p² + Σ t² + s);  L = mean(dice_bc) + mean(bce)
// One pass produces, per (b, c) plane and chunk, the four sums {Σ p t, Σ p², Σ t², Σ bce};
// a second elementwise pass produces dL/dz from the per-plane scalars.
//
// Every pass is written ONCE and reads its target through a reader (DenseRead / LevelRead below):
//  * dense: the target is fp32 at the logits' own extents (fz_dice_{bce,ce}_{sums,grad});
//  * level: ONE COARSE level of a deep-supervision head list (ft.DeepSupervisionLoss): logits (B, C, Ld, Lh, Lw), target
//    at FULL resolution (B, C, Td, Th, Tw) with Tk = rk·Lk on every axis (fz_dice_{bce,ce}_ds_{sums,grad}).  The level's
//    target is the nearest-exact down-sampling of MONAI 1.4 DeepSupervisionLoss — for an integer ratio the strided pick
//    t_l[z, y, x] = t[rz·z + rz/2, ry·y + ry/2, rx·x + rx/2]  — read THROUGH that index map, in the target's own element
//    type (fp32, bf16, one byte), converted in registers: no down-sampled target is ever written.
// The arithmetic per voxel, the chunking (fz_dice_bce_chunks), the order of every sum and the layout of the partials do
// not depend on the reader, so fz_dice_ce_finish and the host finish serve both.  No atomics: one partial per
// (plane | batch item, chunk), combined in a fixed order.
#include "fz_common.h"
#include "seg_labels.h"

namespace fz {

// ---- target readers: how a thread gets the target values of its 4 consecutive voxels v .. v + 3 of one plane ----
// elem: the target's element type; plane(V): elements between two (b, c) planes of the target; locate(v): where the 4
// voxels are, found once and shared by all channels; fetch(tp, at): what one load brings of them from the plane that
// starts at tp; value(q, at, e): the e-th of them.  The kernels loop over e themselves: a reader function that loads all 4
// made the compiler fold the channel's base into the last multiply-add of every level offset — one 64-bit VGPR pair per
// channel, 52 -> 67 VGPRs in the byte-target CE sums at C = 3 and 107 -> 170 at C = 8 (profiles/loss_fold.md).
struct DenseRead {
  using elem = float;
  using pos = int64_t;
  __device__ __forceinline__ int64_t plane(int64_t V) const { return V; }
  __device__ __forceinline__ pos locate(int64_t v) const { return v; }
  struct got { float a[4]; };
  __device__ __forceinline__ got fetch(const float* tp, pos at) const {
    const float4 tt = *reinterpret_cast<const float4*>(tp + at);   // one 16-byte load
    return {{tt.x, tt.y, tt.z, tt.w}};
  }
  __device__ __forceinline__ float value(const got& q, pos, int e) const { return q.a[e]; }
};

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

template <typename TT>
struct LevelRead {
  using elem = TT;
  struct pos { int64_t off[4]; };
  DsGeom g;
  __device__ __forceinline__ int64_t plane(int64_t) const { return g.plane; }
  __device__ __forceinline__ pos locate(int64_t v) const {
    pos at;
    ds_offsets((uint32_t)v, g, at.off);
    return at;
  }
  using got = const TT*;
  __device__ __forceinline__ got fetch(const TT* tp, const pos&) const { return tp; }
  __device__ __forceinline__ float value(got q, const pos& at, int e) const { return ds_tval(q + at.off[e]); }
};

__device__ __forceinline__ void load4(const float* zp, float (&zs)[4]) {
  const float4 zz = *reinterpret_cast<const float4*>(zp);
  zs[0] = zz.x, zs[1] = zz.y, zs[2] = zz.z, zs[3] = zz.w;
}

// ---- the per-voxel formulas ----
// p = sigmoid(z) from ex = e^{-|z|}, which never overflows and which the stable BCE term uses again
__device__ __forceinline__ float sigmoid(float z, float& ex) {
  ex = __expf(-fabsf(z));
  return z >= 0.f ? 1.0f / (1.0f + ex) : ex / (1.0f + ex);
}

// dL/dz = g·[ cd·(dDice/dp)·p(1−p) + cb·dce ],  dDice/dp = −(2 t / den) + (2 inter + s)·2 p / den²  with the plane's
// coef = {num = 2 inter + s, den};  dce = d(cross-entropy term)/dz: p − t (BCE), softmax_c·Σ_c' t_c' − t_c (CE)
__device__ __forceinline__ float loss_grad(float g, float cd, float cb, float t, float p, float num, float den, float dce) {
  const float ddp = -2.0f * t / den + num * 2.0f * p / (den * den);
  return g * (cd * ddp * p * (1.0f - p) + cb * dce);
}

// voxels [v0, v1) of chunk `chunk` of a plane of V: whole groups of 4
__device__ __forceinline__ void chunk_bounds(int64_t V, int nchunk, int chunk, int64_t& v0, int64_t& v1) {
  const int64_t per = ((V / 4 + nchunk - 1) / nchunk) * 4;
  v0 = chunk * per, v1 = min(V, v0 + per);
}

// The workgroup's N sums in a fixed order — wave butterfly, then the four waves pairwise — to out[0 .. N)
template <int N>
__device__ __forceinline__ void reduce_store(const float (&s)[N], float* __restrict__ out) {
  __shared__ float red[4][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float r = wave_sum(s[i]);
    if (lane == 0) red[wave][i] = r;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int i = threadIdx.x;
    out[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
  }
}

// ---- one prediction channel per plane: Dice + BCE with logits ----
template <typename RD>
__global__ __launch_bounds__(256) void dice_bce_sums(const float* __restrict__ z, const typename RD::elem* __restrict__ t,
                                                     float* __restrict__ part, int64_t V, int nchunk, RD rd) {
  const int plane = blockIdx.x, chunk = blockIdx.y;
  int64_t v0, v1;
  chunk_bounds(V, nchunk, chunk, v0, v1);
  const float* zp = z + (int64_t)plane * V;
  const typename RD::elem* tp = t + (int64_t)plane * rd.plane(V);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t v = v0 + threadIdx.x * 4; v < v1; v += 1024) {
    float zs[4], ts[4];
    load4(zp + v, zs);
    const typename RD::pos at = rd.locate(v);
    const typename RD::got tq = rd.fetch(tp, at);
#pragma unroll
    for (int e = 0; e < 4; ++e) ts[e] = rd.value(tq, at, e);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float ex;
      const float p = sigmoid(zs[e], ex);
      s[0] += p * ts[e];
      s[1] += p * p;
      s[2] += ts[e] * ts[e];
      s[3] += fmaxf(zs[e], 0.f) - zs[e] * ts[e] + log1pf(ex);  // stable BCE with logits
    }
  }
  reduce_store(s, part + ((int64_t)plane * nchunk + chunk) * 4);
}

// coef (planes, 2) = {2·inter + smooth, den + smooth} per plane
template <typename RD>
__global__ __launch_bounds__(256) void dice_bce_grad(const float* __restrict__ z, const typename RD::elem* __restrict__ t,
                                                     const float* __restrict__ coef, float* __restrict__ gz, int64_t V,
                                                     int64_t total, float cd, float cb, const float* __restrict__ gscale,
                                                     RD rd) {
  const float g = gscale ? gscale[0] : 1.0f;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < total;
       i += (int64_t)gridDim.x * blockDim.x * 4) {
    const int plane = (int)(i / V);
    const float num = coef[plane * 2], den = coef[plane * 2 + 1];
    float zs[4], ts[4], o[4];
    load4(z + i, zs);
    const typename RD::pos at = rd.locate(i - (int64_t)plane * V);
    const typename RD::got tq = rd.fetch(t + (int64_t)plane * rd.plane(V), at);
#pragma unroll
    for (int e = 0; e < 4; ++e) ts[e] = rd.value(tq, at, e);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float ex;
      const float p = sigmoid(zs[e], ex);
      o[e] = loss_grad(g, cd, cb, ts[e], p, num, den, p - ts[e]);
    }
    *reinterpret_cast<float4*>(gz + i) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ---- DiceCELoss(sigmoid=True, squared_pred=True) for C > 1 channels, as MONAI 1.4 evaluates it
// (the bundle pins monai==1.4.0, docs/requirements.txt:11; train.yaml:67-70): soft Dice on
// sigmoid(z) per (b, c) plane + nn.CrossEntropyLoss over the CHANNEL softmax with the float
// multi-label target as class "probabilities":  CE = mean_{b,v} Σ_c t_c · (logsumexp_c'(z) − z_c).
// One pass: per batch item and chunk the 3·C Dice sums {Σ p t, Σ p², Σ t²}_c and Σ CE.
template <int C, typename RD>
__global__ __launch_bounds__(256) void dice_ce_sums(const float* __restrict__ z, const typename RD::elem* __restrict__ t,
                                                    float* __restrict__ part, int64_t V, int nchunk, RD rd) {
  const int b = blockIdx.x, chunk = blockIdx.y;
  int64_t v0, v1;
  chunk_bounds(V, nchunk, chunk, v0, v1);
  const float* zp = z + (int64_t)b * C * V;
  const typename RD::elem* tp = t + (int64_t)b * C * rd.plane(V);
  float s[3 * C + 1];
#pragma unroll
  for (int i = 0; i < 3 * C + 1; ++i) s[i] = 0.f;
  for (int64_t v = v0 + threadIdx.x * 4; v < v1; v += 1024) {
    const typename RD::pos at = rd.locate(v);
    float zs[C][4], ts[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      load4(zp + c * V + v, zs[c]);
      const typename RD::got tq = rd.fetch(tp + c * rd.plane(V), at);
#pragma unroll
      for (int e = 0; e < 4; ++e) ts[c][e] = rd.value(tq, at, e);
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
        float ex;
        const float p = sigmoid(zc, ex);
        s[3 * c + 0] += p * tc;
        s[3 * c + 1] += p * p;
        s[3 * c + 2] += tc * tc;
      }
      s[3 * C] += st * (mx + __logf(se)) - stz;
    }
  }
  reduce_store(s, part + ((int64_t)b * nchunk + chunk) * (3 * C + 1));
}

// coef (B·C, 2) as in dice_bce_grad
template <int C, typename RD>
__global__ __launch_bounds__(256) void dice_ce_grad(const float* __restrict__ z, const typename RD::elem* __restrict__ t,
                                                    const float* __restrict__ coef, float* __restrict__ gz, int64_t V, int B,
                                                    float cd, float cb, const float* __restrict__ gscale, RD rd) {
  const float g = gscale ? gscale[0] : 1.0f;
  const int64_t total = (int64_t)B * V;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < total;
       i += (int64_t)gridDim.x * blockDim.x * 4) {
    const int b = (int)(i / V);
    const int64_t v = i - (int64_t)b * V;
    const int64_t base = (int64_t)b * C * V + v;
    const typename RD::elem* tp = t + (int64_t)b * C * rd.plane(V);
    const typename RD::pos at = rd.locate(v);
    float zs[C][4], ts[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      load4(z + base + c * V, zs[c]);
      const typename RD::got tq = rd.fetch(tp + c * rd.plane(V), at);
#pragma unroll
      for (int e = 0; e < 4; ++e) ts[c][e] = rd.value(tq, at, e);
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
        const float tc = ts[c][e];
        float ex;
        const float p = sigmoid(zs[c][e], ex);
        o[c][e] = loss_grad(g, cd, cb, tc, p, coef[(b * C + c) * 2], coef[(b * C + c) * 2 + 1], ez[c] * inv - tc);
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
      *reinterpret_cast<float4*>(gz + base + c * V) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
  }
}

// The finish of the class-index form (dice_sce_* at the end of this section), as dice_ce_finish_kernel below: the Dice mean runs over the channels c >= c0 (B·(C − c0) planes), the planes
// below c0 get the inert coefficients {0, 1}
__global__ __launch_bounds__(256) void dice_sce_finish_kernel(const float* __restrict__ part, int nchunk, int B, int C, int c0,
                                                              float inv_bv, float smooth, float* __restrict__ loss,
                                                              float* __restrict__ coef) {
  __shared__ float cols[8 * 49];   // (B <= 8) x (3C + 1 <= 49) column totals
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ncol = 3 * C + 1;
  for (int col = wave; col < B * ncol; col += 4) {
    const int b = col / ncol, k = col % ncol;
    float t = 0.f;
    for (int ch = lane; ch < nchunk; ch += 64) t += part[((int64_t)b * nchunk + ch) * ncol + k];
    t = wave_sum(t);
    if (lane == 0) cols[col] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float dice = 0.f, ce = 0.f;
    for (int b = 0; b < B; ++b) {
      for (int c = 0; c < C; ++c) {
        float num = 0.f, den = 1.f;
        if (c >= c0) {
          num = 2.0f * cols[b * ncol + 3 * c] + smooth;
          den = cols[b * ncol + 3 * c + 1] + cols[b * ncol + 3 * c + 2] + smooth;
          dice += 1.0f - num / den;
        }
        coef[(b * C + c) * 2] = num;
        coef[(b * C + c) * 2 + 1] = den;
      }
      ce += cols[b * ncol + 3 * C];
    }
    loss[0] = dice / (float)(B * (C - c0)) + ce * inv_bv;
  }
}

// One workgroup turns the partial sums into the loss and the Dice coefficients of the gradient pass: replaces a dozen
// launch-bound framework kernels (sum over chunks, 2·inter + smooth, den + smooth, 1 - num/den, means) between the two
// passes.  Chunks are added in a fixed order: lane-strided partial sums, then the wave butterfly of fz_common.h.
__global__ __launch_bounds__(256) void dice_ce_finish_kernel(const float* __restrict__ part, int nchunk, int B, int C, float inv_bv,
                                                             float smooth, float* __restrict__ loss, float* __restrict__ coef) {
  __shared__ float cols[8 * 25 + 8];   // (B <= 8) x (3C + 1 <= 25) column totals
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ncol = 3 * C + 1;
  for (int col = wave; col < B * ncol; col += 4) {
    const int b = col / ncol, k = col % ncol;
    float t = 0.f;
    for (int ch = lane; ch < nchunk; ch += 64) t += part[((int64_t)b * nchunk + ch) * ncol + k];
    t = wave_sum(t);
    if (lane == 0) cols[col] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float dice = 0.f, ce = 0.f;
    for (int b = 0; b < B; ++b) {
      for (int c = 0; c < C; ++c) {
        const float num = 2.0f * cols[b * ncol + 3 * c] + smooth;
        const float den = cols[b * ncol + 3 * c + 1] + cols[b * ncol + 3 * c + 2] + smooth;
        coef[(b * C + c) * 2] = num;
        coef[(b * C + c) * 2 + 1] = den;
        dice += 1.0f - num / den;
      }
      ce += cols[b * ncol + 3 * C];
    }
    loss[0] = dice / (float)(B * C) + ce * inv_bv;
  }
}

// ---- the class-index form: DiceCELoss(softmax=True, to_onehot_y=True, include_background, squared_pred)
// p = softmax_c(z), t_c = [y == c] from a label map (B, 1, *S) read in its own element type (seg_labels.h) and never
// stored.  Label readers, as the target readers above: classes(yp, at, C, k) gives the classes of the 4 voxels at `at`.
template <typename YT>
struct DenseLabels {
  using elem = YT;
  using pos = int64_t;
  __device__ __forceinline__ int64_t plane(int64_t V) const { return V; }
  __device__ __forceinline__ pos locate(int64_t v) const { return v; }
  __device__ __forceinline__ void classes(const YT* yp, pos at, int C, int (&k)[4]) const { label_classes4(yp + at, C, k); }
};

template <typename YT>
struct LevelLabels {
  using elem = YT;
  struct pos { int64_t off[4]; };
  DsGeom g;
  __device__ __forceinline__ int64_t plane(int64_t) const { return g.plane; }
  __device__ __forceinline__ pos locate(int64_t v) const {
    pos at;
    ds_offsets((uint32_t)v, g, at.off);
    return at;
  }
  __device__ __forceinline__ void classes(const YT* yp, const pos& at, int C, int (&k)[4]) const {
#pragma unroll
    for (int e = 0; e < 4; ++e) k[e] = label_class(yp[at.off[e]], C);
  }
};

// The kernels are compiled for CP = 2 / 3 / 4 / 8 / 16 channel slots; C <= CP is a run-time, workgroup-uniform count.  A slot
// c >= C loads channel C − 1 again (a valid address, a cache hit) and takes the logit −inf, whose exponential, probability
// and every sum term are 0: no branch separates the loads of one trip from the arithmetic of another.  Such a slot is never
// stored.
template <int CP>
__device__ __forceinline__ void load_logits(const float* zp, int64_t V, int64_t v, int C, float (&zs)[CP][4]) {
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    load4(zp + (c < C ? c : C - 1) * V + v, zs[c]);
#pragma unroll
    for (int e = 0; e < 4; ++e) zs[c][e] = c < C ? zs[c][e] : -__builtin_huge_valf();
  }
}

// In place: zs[c][e] <- e^{z_c − mx}, mx = max_c z_c; returns their sum.
template <int CP>
__device__ __forceinline__ float softmax_exps(float (&zs)[CP][4], int e, float mx) {
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    zs[c][e] = __expf(zs[c][e] - mx);
    se += zs[c][e];
  }
  return se;
}
template <int CP>
__device__ __forceinline__ float logit_max(const float (&zs)[CP][4], int e) {
  float mx = zs[0][e];
#pragma unroll
  for (int c = 1; c < CP; ++c) mx = fmaxf(mx, zs[c][e]);
  return mx;
}

// The workgroup's sums in the fixed order of reduce_store: the 3·C channel sums s[0 .. 3C) to out[0 .. 3C), s[3·CP] to out[3C]
template <int CP>
__device__ __forceinline__ void reduce_store_channels(const float (&s)[3 * CP + 1], int C, float* __restrict__ out) {
  constexpr int N = 3 * CP + 1;
  __shared__ float red[4][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i)
    if (i < 3 * C || i == N - 1) {
      const float r = wave_sum(s[i]);
      if (lane == 0) red[wave][i] = r;
    }
  __syncthreads();
  const int i = threadIdx.x;
  if (i < 3 * C || i == N - 1) out[i < 3 * C ? i : 3 * C] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

// part (B, nchunk, 3C + 1): per channel {Σ p t, Σ p² (sq) or Σ p, Σ t}, then Σ CE with CE = log Σ_c e^{z_c − mx} − (z_y − mx),
// which a common shift of the logits leaves as it is; 0 for a label that names no class
template <int CP, typename RD>
__global__ __launch_bounds__(256) void dice_sce_sums(const float* __restrict__ z, const typename RD::elem* __restrict__ y,
                                                     float* __restrict__ part, int64_t V, int nchunk, int C, int sq, RD rd) {
  const int b = blockIdx.x, chunk = blockIdx.y;
  int64_t v0, v1;
  chunk_bounds(V, nchunk, chunk, v0, v1);
  const float* zp = z + (int64_t)b * C * V;
  const typename RD::elem* yp = y + (int64_t)b * rd.plane(V);
  constexpr int SUMS_TRIPS = CP <= 8 ? 2 : 1;
  float s[3 * CP + 1];
#pragma unroll
  for (int i = 0; i < 3 * CP + 1; ++i) s[i] = 0.f;
  // two trips at a time where the registers allow it: the pass is one wave per SIMD at the chunk counts of
  // fz_dice_bce_chunks, so the loads of the second trip in flight during the first one's exponentials are what hides the
  // memory latency
#pragma unroll SUMS_TRIPS
  for (int64_t v = v0 + threadIdx.x * 4; v < v1; v += 1024) {
    float zs[CP][4];
    load_logits<CP>(zp, V, v, C, zs);
    int k[4];
    rd.classes(yp, rd.locate(v), C, k);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float mx = logit_max<CP>(zs, e);
      float dk = mx;   // z_y
#pragma unroll
      for (int c = 0; c < CP; ++c) dk = k[e] == c ? zs[c][e] : dk;
      dk -= mx;        // z_y − mx
      const float se = softmax_exps<CP>(zs, e, mx);
      const float inv = 1.0f / se;
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const float p = zs[c][e] * inv;
        const bool hit = k[e] == c;
        s[3 * c + 0] += hit ? p : 0.f;
        s[3 * c + 1] += sq ? p * p : p;
        s[3 * c + 2] += hit ? 1.f : 0.f;
      }
      s[3 * CP] += k[e] >= 0 ? __logf(se) - dk : 0.f;
    }
  }
  reduce_store_channels<CP>(s, C, part + ((int64_t)b * nchunk + chunk) * (3 * C + 1));
}

// coef (B·C, 2) = {num, den};  gz_k = g·[ p_k (a_k − Σ_c a_c p_c) + cb (p_k − t_k) ]  (cb = 0 at a label that names no class),
// a_c = t_c·A_c + (sq ? p_c : 1)·Q_c with A_c = −2 cd/den_c, Q_c = (sq ? 2 : 1)·cd·num_c/den_c² for c >= c0, else both 0.
// One batch item per blockIdx.y, so the 2·C plane scalars are workgroup-uniform; the grid-stride loop over the item's V
// starts past 4096 · 1024 voxels.
template <int CP, typename RD>
__global__ __launch_bounds__(256) void dice_sce_grad(const float* __restrict__ z, const typename RD::elem* __restrict__ y,
                                                     const float* __restrict__ coef, float* __restrict__ gz, int64_t V, int C,
                                                     int sq, int c0, float cd, float cb, const float* __restrict__ gscale,
                                                     RD rd) {
  const int b = blockIdx.y;
  const float g = gscale ? gscale[0] : 1.0f;
  float A[CP], Q[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    A[c] = 0.f, Q[c] = 0.f;
    if (c < C && c >= c0) {
      const float num = coef[(b * C + c) * 2], den = coef[(b * C + c) * 2 + 1];
      A[c] = -2.0f * cd / den;
      Q[c] = (sq ? 2.0f : 1.0f) * cd * num / (den * den);
    }
  }
  const float* zp = z + (int64_t)b * C * V;
  float* gp = gz + (int64_t)b * C * V;
  const typename RD::elem* yp = y + (int64_t)b * rd.plane(V);
  for (int64_t v = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; v < V; v += (int64_t)gridDim.x * 1024) {
    float zs[CP][4];
    load_logits<CP>(zp, V, v, C, zs);
    int k[4];
    rd.classes(yp, rd.locate(v), C, k);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float inv = 1.0f / softmax_exps<CP>(zs, e, logit_max<CP>(zs, e));
      const float cbv = k[e] >= 0 ? cb : 0.f;   // a label that names no class has no CE term
      float dot = 0.f;                          // Σ_c a_c p_c
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const float p = zs[c][e] * inv;
        zs[c][e] = p;
        const float a = (k[e] == c ? A[c] : 0.f) + (sq ? p * Q[c] : Q[c]);
        dot += a * p;
      }
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const float p = zs[c][e];
        const bool hit = k[e] == c;
        const float a = (hit ? A[c] : 0.f) + (sq ? p * Q[c] : Q[c]);
        zs[c][e] = g * (p * (a - dot) + cbv * (p - (hit ? 1.f : 0.f)));
      }
    }
#pragma unroll
    for (int c = 0; c < CP; ++c)
      if (c < C) *reinterpret_cast<float4*>(gp + c * V + v) = make_float4(zs[c][0], zs[c][1], zs[c][2], zs[c][3]);
  }
}

// Level geometry from the plain ints of the ABI; 0 on success.  V: the level's voxels per plane.
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

// ---- host launchers, one per pass: f(rd) for the level reader of the target's element kind, f(IntC<C>{}) for the
// channel count (false: no kernel for this C) ----
template <int N> struct IntC { static constexpr int value = N; };
template <typename F>
static void by_kind(int tkind, const DsGeom& g, F f) {
  if (tkind == FZ_SEG_F32) f(LevelRead<float>{g});
  else if (tkind == FZ_SEG_BF16) f(LevelRead<bf16>{g});
  else f(LevelRead<uint8_t>{g});
}
template <typename F>
static bool by_channels(int C, F f) {
  switch (C) {
    case 2: f(IntC<2>{}); return true;
    case 3: f(IntC<3>{}); return true;
    case 4: f(IntC<4>{}); return true;
    case 5: f(IntC<5>{}); return true;
    case 6: f(IntC<6>{}); return true;
    case 7: f(IntC<7>{}); return true;
    case 8: f(IntC<8>{}); return true;
    default: return false;
  }
}

static int grad_blocks(int64_t total) {
  const int64_t blocks = (total / 4 + 255) / 256;
  return blocks > 4096 ? 4096 : (int)blocks;
}

template <typename RD>
static void launch_bce_sums(RD rd, const float* z, const void* t, float* part, int planes, int64_t V, fz_stream_t stream) {
  const int nchunk = fz_dice_bce_chunks(V);
  hipLaunchKernelGGL(dice_bce_sums<RD>, dim3(planes, nchunk), dim3(256), 0, (hipStream_t)stream, z,
                     static_cast<const typename RD::elem*>(t), part, V, nchunk, rd);
}

template <typename RD>
static void launch_bce_grad(RD rd, const float* z, const void* t, const float* coef, float* gz, int planes, int64_t V,
                            float cd, float cb, const float* gscale, fz_stream_t stream) {
  const int64_t total = (int64_t)planes * V;
  hipLaunchKernelGGL(dice_bce_grad<RD>, dim3(grad_blocks(total)), dim3(256), 0, (hipStream_t)stream, z,
                     static_cast<const typename RD::elem*>(t), coef, gz, V, total, cd, cb, gscale, rd);
}

template <typename RD>
static bool launch_ce_sums(RD rd, const float* z, const void* t, float* part, int B, int C, int64_t V, fz_stream_t stream) {
  const int nchunk = fz_dice_bce_chunks(V);
  return by_channels(C, [&](auto cc) {
    hipLaunchKernelGGL((dice_ce_sums<decltype(cc)::value, RD>), dim3(B, nchunk), dim3(256), 0, (hipStream_t)stream, z,
                       static_cast<const typename RD::elem*>(t), part, V, nchunk, rd);
  });
}

template <typename RD>
static bool launch_ce_grad(RD rd, const float* z, const void* t, const float* coef, float* gz, int B, int C, int64_t V,
                           float cd, float cb, const float* gscale, fz_stream_t stream) {
  return by_channels(C, [&](auto cc) {
    hipLaunchKernelGGL((dice_ce_grad<decltype(cc)::value, RD>), dim3(grad_blocks((int64_t)B * V)), dim3(256), 0,
                       (hipStream_t)stream, z, static_cast<const typename RD::elem*>(t), coef, gz, V, B, cd, cb, gscale, rd);
  });
}

// ---- the class-index form: f(IntC<CP>{}) for the channel slots, rd(YT{}) the label reader of the element kind ----
template <typename F>
static void by_slots(int C, F f) {
  if (C == 2) f(IntC<2>{});
  else if (C == 3) f(IntC<3>{});
  else if (C <= 4) f(IntC<4>{});
  else if (C <= 8) f(IntC<8>{});
  else f(IntC<16>{});
}

// what every fz_dice_sce_* pass refuses; 0 when the call may launch
static int sce_check(const char* who, bool null, const void* y, int B, int C, int64_t V, int ykind, int c0) {
  const char* why = nullptr;
  int code = FZ_E_ARG;
  if (null) why = "null pointer";
  else if (!label_kind_ok(ykind)) why = "label kind must be FZ_LABEL_U8 / _I64 / _F32";
  else if (c0 != 0 && c0 != 1) why = "c0 must be 0 (include_background) or 1";
  else if (C < 2 || C > 16) why = "2 <= C <= 16", code = FZ_E_UNSUPPORTED;
  else if (B < 1 || B > 65535) why = "1 <= B <= 65535", code = FZ_E_SHAPE;
  else if (V < 4 || (V % 4)) why = "V must be a positive multiple of 4", code = FZ_E_SHAPE;
  else if ((uintptr_t)y % (uintptr_t)label_esize(ykind)) why = "label map not aligned to its element";
  if (why) return fail(code, (std::string(who) + ": " + why).c_str());
  return FZ_OK;
}

template <typename MK>
static void launch_sce_sums(MK rd_of, int ykind, const float* z, const void* y, float* part, int B, int C, int64_t V, int sq,
                            fz_stream_t stream) {
  const int nchunk = fz_dice_bce_chunks(V);
  by_label_kind(ykind, [&](auto yt) {
    auto rd = rd_of(yt);
    using RD = decltype(rd);
    by_slots(C, [&](auto cp) {
      hipLaunchKernelGGL((dice_sce_sums<decltype(cp)::value, RD>), dim3(B, nchunk), dim3(256), 0, (hipStream_t)stream, z,
                         static_cast<const typename RD::elem*>(y), part, V, nchunk, C, sq, rd);
    });
  });
}

template <typename MK>
static void launch_sce_grad(MK rd_of, int ykind, const float* z, const void* y, const float* coef, float* gz, int B, int C,
                            int64_t V, int sq, int c0, float cd, float cb, const float* gscale, fz_stream_t stream) {
  by_label_kind(ykind, [&](auto yt) {
    auto rd = rd_of(yt);
    using RD = decltype(rd);
    by_slots(C, [&](auto cp) {
      hipLaunchKernelGGL((dice_sce_grad<decltype(cp)::value, RD>), dim3(grad_blocks(V), B), dim3(256), 0, (hipStream_t)stream,
                         z, static_cast<const typename RD::elem*>(y), coef, gz, V, C, sq, c0, cd, cb, gscale, rd);
    });
  });
}

}  // namespace fz

using namespace fz;

extern "C" int fz_dice_bce_chunks(int64_t V) {
  int64_t n = V / 32768;
  if (n < 1) n = 1;
  if (n > 64) n = 64;
  return (int)n;
}

// ---- dense target ----
// part: (planes, nchunk, 4) partial sums {Σ p t, Σ p², Σ t², Σ bce}
extern "C" int fz_dice_bce_sums(const float* z, const float* t, float* part, int planes, int64_t V,
                                fz_stream_t stream) {
  if (!z || !t || !part) return fail(FZ_E_ARG, "fz_dice_bce_sums: null pointer");
  if (planes < 1 || V < 4 || (V % 4)) return fail(FZ_E_SHAPE, "fz_dice_bce_sums: bad sizes");
  launch_bce_sums(DenseRead{}, z, t, part, planes, V, stream);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

// coef: (planes, 2) = {2·inter + smooth, den + smooth};  cd = 1/planes, cb = 1/(planes·V);
// gscale: optional device scalar multiplying the gradient (upstream dL)
extern "C" int fz_dice_bce_grad(const float* z, const float* t, const float* coef, float* gz, int planes, int64_t V,
                                float cd, float cb, const float* gscale, fz_stream_t stream) {
  if (!z || !t || !coef || !gz) return fail(FZ_E_ARG, "fz_dice_bce_grad: null pointer");
  if (planes < 1 || V < 4 || (V % 4)) return fail(FZ_E_SHAPE, "fz_dice_bce_grad: bad sizes");
  launch_bce_grad(DenseRead{}, z, t, coef, gz, planes, V, cd, cb, gscale, stream);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

// multi-channel DiceCE (C in 2..8).  part: (B, nchunk, 3C+1) = per channel {Σ p t, Σ p², Σ t²}, then Σ CE
extern "C" int fz_dice_ce_sums(const float* z, const float* t, float* part, int B, int C, int64_t V,
                               fz_stream_t stream) {
  if (!z || !t || !part) return fail(FZ_E_ARG, "fz_dice_ce_sums: null pointer");
  if (B < 1 || V < 4 || (V % 4)) return fail(FZ_E_SHAPE, "fz_dice_ce_sums: bad sizes");
  if (!launch_ce_sums(DenseRead{}, z, t, part, B, C, V, stream)) return fail(FZ_E_UNSUPPORTED, "fz_dice_ce: 2 <= C <= 8");
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_dice_ce_finish(const float* part, int B, int C, int64_t V, float smooth, float* loss, float* coef,
                                 fz_stream_t stream) {
  if (!part || !loss || !coef) return fail(FZ_E_ARG, "fz_dice_ce_finish: null pointer");
  if (B < 1 || B > 8 || C < 2 || C > 8) return fail(FZ_E_UNSUPPORTED, "fz_dice_ce_finish: 1 <= B <= 8, 2 <= C <= 8");
  hipLaunchKernelGGL(dice_ce_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, fz_dice_bce_chunks(V), B, C,
                     1.0f / ((float)B * (float)V), smooth, loss, coef);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

// coef: (B·C, 2) = {2·inter + smooth, den + smooth};  cd = 1/(B·C), cb = 1/(B·V)
extern "C" int fz_dice_ce_grad(const float* z, const float* t, const float* coef, float* gz, int B, int C, int64_t V,
                               float cd, float cb, const float* gscale, fz_stream_t stream) {
  if (!z || !t || !coef || !gz) return fail(FZ_E_ARG, "fz_dice_ce_grad: null pointer");
  if (B < 1 || V < 4 || (V % 4)) return fail(FZ_E_SHAPE, "fz_dice_ce_grad: bad sizes");
  if (!launch_ce_grad(DenseRead{}, z, t, coef, gz, B, C, V, cd, cb, gscale, stream))
    return fail(FZ_E_UNSUPPORTED, "fz_dice_ce: 2 <= C <= 8");
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

// ---- one coarse level against the full-resolution target: partials and coefficients laid out as above ----
extern "C" int fz_dice_bce_ds_sums(const float* z, const void* t, float* part, int planes, int Td, int Th, int Tw, int Ld,
                                   int Lh, int Lw, int tkind, fz_stream_t stream) {
  if (!z || !t || !part) return fail(FZ_E_ARG, "fz_dice_bce_ds_sums: null pointer");
  if (planes < 1) return fail(FZ_E_SHAPE, "fz_dice_bce_ds_sums: bad sizes");
  DsGeom g;
  int64_t V;
  if (int rc = ds_geom("fz_dice_bce_ds_sums", Td, Th, Tw, Ld, Lh, Lw, tkind, &g, &V)) return rc;
  by_kind(tkind, g, [&](auto rd) { launch_bce_sums(rd, z, t, part, planes, V, stream); });
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
  by_kind(tkind, g, [&](auto rd) { launch_bce_grad(rd, z, t, coef, gz, planes, V, cd, cb, gscale, stream); });
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_dice_ce_ds_sums(const float* z, const void* t, float* part, int B, int C, int Td, int Th, int Tw, int Ld,
                                  int Lh, int Lw, int tkind, fz_stream_t stream) {
  if (!z || !t || !part) return fail(FZ_E_ARG, "fz_dice_ce_ds_sums: null pointer");
  if (B < 1) return fail(FZ_E_SHAPE, "fz_dice_ce_ds_sums: bad sizes");
  DsGeom g;
  int64_t V;
  if (int rc = ds_geom("fz_dice_ce_ds_sums", Td, Th, Tw, Ld, Lh, Lw, tkind, &g, &V)) return rc;
  bool ok = false;
  by_kind(tkind, g, [&](auto rd) { ok = launch_ce_sums(rd, z, t, part, B, C, V, stream); });
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
  bool ok = false;
  by_kind(tkind, g, [&](auto rd) { ok = launch_ce_grad(rd, z, t, coef, gz, B, C, V, cd, cb, gscale, stream); });
  if (!ok) return fail(FZ_E_UNSUPPORTED, "fz_dice_ce_ds_grad: 2 <= C <= 8");
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

// ---- the class-index form (softmax, label map): dense, finish, one coarse level ----
extern "C" int fz_dice_sce_sums(const float* z, const void* y, float* part, int B, int C, int64_t V, int ykind, int sq,
                                fz_stream_t stream) {
  if (int rc = sce_check("fz_dice_sce_sums", !z || !y || !part, y, B, C, V, ykind, 0)) return rc;
  if ((uintptr_t)y % (uintptr_t)label_vec_bytes(ykind) || (uintptr_t)z % 16)
    return fail(FZ_E_ARG, "fz_dice_sce_sums: logits and label map must be aligned to their 16-byte (uint8: 4-byte) loads");
  launch_sce_sums([](auto yt) { return DenseLabels<decltype(yt)>{}; }, ykind, z, y, part, B, C, V, sq, stream);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_dice_sce_finish(const float* part, int B, int C, int64_t V, int c0, float smooth, float* loss, float* coef,
                                  fz_stream_t stream) {
  if (!part || !loss || !coef) return fail(FZ_E_ARG, "fz_dice_sce_finish: null pointer");
  if (c0 != 0 && c0 != 1) return fail(FZ_E_ARG, "fz_dice_sce_finish: c0 must be 0 (include_background) or 1");
  if (B < 1 || B > 8 || C < 2 || C > 16) return fail(FZ_E_UNSUPPORTED, "fz_dice_sce_finish: 1 <= B <= 8, 2 <= C <= 16");
  if (V < 4 || (V % 4)) return fail(FZ_E_SHAPE, "fz_dice_sce_finish: V must be a positive multiple of 4");
  hipLaunchKernelGGL(dice_sce_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, fz_dice_bce_chunks(V), B, C, c0,
                     1.0f / ((float)B * (float)V), smooth, loss, coef);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_dice_sce_grad(const float* z, const void* y, const float* coef, float* gz, int B, int C, int64_t V, int ykind,
                                int sq, int c0, float cd, float cb, const float* gscale, fz_stream_t stream) {
  if (int rc = sce_check("fz_dice_sce_grad", !z || !y || !coef || !gz, y, B, C, V, ykind, c0)) return rc;
  if ((uintptr_t)y % (uintptr_t)label_vec_bytes(ykind) || (uintptr_t)z % 16 || (uintptr_t)gz % 16)
    return fail(FZ_E_ARG, "fz_dice_sce_grad: logits, gradient and label map must be aligned to their 16-byte (uint8: 4-byte) loads");
  launch_sce_grad([](auto yt) { return DenseLabels<decltype(yt)>{}; }, ykind, z, y, coef, gz, B, C, V, sq, c0, cd, cb, gscale,
                  stream);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_dice_sce_ds_sums(const float* z, const void* y, float* part, int B, int C, int Td, int Th, int Tw, int Ld,
                                   int Lh, int Lw, int ykind, int sq, fz_stream_t stream) {
  DsGeom g;
  int64_t V;
  if (int rc = ds_geom("fz_dice_sce_ds_sums", Td, Th, Tw, Ld, Lh, Lw, FZ_SEG_F32, &g, &V)) return rc;
  if (int rc = sce_check("fz_dice_sce_ds_sums", !z || !y || !part, y, B, C, V, ykind, 0)) return rc;
  if ((uintptr_t)z % 16) return fail(FZ_E_ARG, "fz_dice_sce_ds_sums: logits must be 16-byte aligned");
  launch_sce_sums([&](auto yt) { return LevelLabels<decltype(yt)>{g}; }, ykind, z, y, part, B, C, V, sq, stream);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_dice_sce_ds_grad(const float* z, const void* y, const float* coef, float* gz, int B, int C, int Td, int Th,
                                   int Tw, int Ld, int Lh, int Lw, int ykind, int sq, int c0, float cd, float cb,
                                   const float* gscale, fz_stream_t stream) {
  DsGeom g;
  int64_t V;
  if (int rc = ds_geom("fz_dice_sce_ds_grad", Td, Th, Tw, Ld, Lh, Lw, FZ_SEG_F32, &g, &V)) return rc;
  if (int rc = sce_check("fz_dice_sce_ds_grad", !z || !y || !coef || !gz, y, B, C, V, ykind, c0)) return rc;
  if ((uintptr_t)z % 16 || (uintptr_t)gz % 16) return fail(FZ_E_ARG, "fz_dice_sce_ds_grad: logits and gradient must be 16-byte aligned");
  launch_sce_grad([&](auto yt) { return LevelLabels<decltype(yt)>{g}; }, ykind, z, y, coef, gz, B, C, V, sq, c0, cd, cb, gscale,
                  stream);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}
