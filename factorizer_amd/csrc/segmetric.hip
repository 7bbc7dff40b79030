// segmetric.hip — the recipe's segmentation metrics on device: thresholded Dice counts and the edge /
// distance kernels of the 95th-percentile Hausdorff distance.
//
// Every training iteration of the bundles runs Activationsd(sigmoid) -> AsDiscreted(threshold=0.5) ->
// MeanDice(include_background=True) (model_zoo/factorizer_brats23/configs/train.yaml:215-243), every validation pass the
// same Dice plus MeanHausdorffDistance(percentile=95) on the stitched prediction (train.yaml:245-287).  MONAI is not part of
// this project; the published semantics are restated in factorizer_amd/metrics.py.  Three kernels:
//   seg_counts     one streaming pass over logits and labels: foreground iff logit >= bound (the threshold moved through the
//                  inverse sigmoid on the host, so no transcendental runs here), |P ∧ Y|, |P|, |Y| per (b, c) plane as
//                  integers — wave ballots + popcounts, uint32 partials per workgroup, summed in a fixed order by a second
//                  launch; no float atomics, nothing rounded, so the counts are exact and replay bit for bit.  The same pass
//                  optionally writes the uint8 mask (ft.discretize; the input of the Hausdorff path).
//   mask_edges     mask -> edge mask (foreground with a background or out-of-image face neighbour: mask ^ erosion by the
//                  cross element with a zero border) for 1 to 3 spatial axes, plus the edge count of every plane.
//   edge_min_dist2 for the edge voxels of one plane: min over the target list of the squared spacing-scaled distance from
//                  every query.  Each lane owns MD_QPL queries and their running minima in registers; the workgroup walks
//                  the targets in LDS tiles that every lane reads at the same address (a broadcast, one ds_read_b128 per
//                  target and 4 queries); long target lists are split over blockIdx.y and the partial minima combined in
//                  split order.  fp32: with unit spacing every difference, square and sum is an integer < 2^24 while no
//                  axis exceeds 2048 (3 · 2047² = 12 570 627), so the result is exact whatever the order.
// and for mutually exclusive classes (AsDiscrete(argmax=True, to_onehot=C) and the multi-class DiceMetric):
//   seg_argmax     one streaming pass over the C logit planes of a batch item (or an already discrete label map) and,
//                  optionally, a class-index label map: the uint8 class map, the uint8 one-hot mask and the three integer
//                  counts of every class, chunked, reduced and finished as seg_counts does.
#include "fz_common.h"
#include "seg_labels.h"

namespace fz {

// ---- seg_counts ---------------------------------------------------------------------------------------------------------
// predicate of one stored element: GE = (float)x >= bound (logits / probabilities), otherwise x != 0 (labels, discrete masks)
template <bool GE> __device__ __forceinline__ bool seg_test(float x, float bound) { return GE ? x >= bound : x != 0.0f; }

// eight consecutive elements -> bit k = predicate of element k; 16-byte loads (fp32: two, bf16: one), 8 bytes for uint8
template <bool GE> __device__ __forceinline__ unsigned seg_bits8(const float* p, float bound) {
  float v[8];
  aload<8>(p, v);
  unsigned b = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) b |= (unsigned)seg_test<GE>(v[k], bound) << k;
  return b;
}
template <bool GE> __device__ __forceinline__ unsigned seg_bits8(const bf16* p, float bound) {
  float v[8];
  aload<8>(p, v);
  unsigned b = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) b |= (unsigned)seg_test<GE>(v[k], bound) << k;
  return b;
}
template <bool GE> __device__ __forceinline__ unsigned seg_bits8(const uint8_t* p, float) {
  const uint2 w = *reinterpret_cast<const uint2*>(p);
  unsigned b = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    b |= (unsigned)(((w.x >> (8 * k)) & 0xffu) != 0) << k;
    b |= (unsigned)(((w.y >> (8 * k)) & 0xffu) != 0) << (k + 4);
  }
  return b;
}
template <bool GE> __device__ __forceinline__ bool seg_bit1(const float* p, float bound) { return seg_test<GE>(*p, bound); }
template <bool GE> __device__ __forceinline__ bool seg_bit1(const bf16* p, float bound) { return seg_test<GE>((float)*p, bound); }
template <bool GE> __device__ __forceinline__ bool seg_bit1(const uint8_t* p, float) { return *p != 0; }

// the low four bits of b as four 0 / 1 bytes: bit k lands on bit 8k (k + 7j = 8k iff j = k; no two pairs collide)
__device__ __forceinline__ unsigned seg_spread4(unsigned b) { return ((b & 0xfu) * 0x00204081u) & 0x01010101u; }

constexpr int SEG_CHUNK = 16384;   // elements of a plane per workgroup (8 groups of 8 per thread); a multiple of 8

// part (planes, nchunk, 3) uint32 = {|P ∧ Y|, |P|, |Y|} of the chunk.  VEC: every plane starts 16-byte aligned in all three
// tensors and holds a multiple of 8 elements, or there is one plane (then its last V % 8 elements go through the masked tail).
// The loops run a wave-uniform number of times, so the ballots see every lane and the three counters stay scalar.
template <typename PT, bool PGE, typename LT, bool VEC>
__global__ __launch_bounds__(256) void seg_counts_kernel(const PT* __restrict__ pred, const LT* __restrict__ label,
                                                         uint8_t* __restrict__ mask, uint32_t* __restrict__ part,
                                                         float bound, int64_t V, int64_t per, int nchunk) {
  __shared__ uint32_t red[4][3];
  const int chunk = blockIdx.x, plane = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t v0 = (int64_t)chunk * per, v1 = min(V, v0 + per);
  const PT* pp = pred + (int64_t)plane * V;
  const LT* lp = label ? label + (int64_t)plane * V : nullptr;
  uint8_t* mp = mask ? mask + (int64_t)plane * V : nullptr;
  uint32_t ni = 0, np = 0, ny = 0;
  int64_t tail0 = v0;   // [tail0, v1): one element per lane
  if constexpr (VEC) {
    const int64_t g1 = v0 + ((v1 - v0) & ~(int64_t)7);   // whole groups of 8 (v0 is a multiple of 8)
    for (int64_t base = v0 + wave * 512; base < g1; base += 2048) {
      const int64_t v = base + lane * 8;
      unsigned pb = 0, yb = 0;
      if (v < g1) {
        pb = seg_bits8<PGE>(pp + v, bound);
        if (lp) yb = seg_bits8<false>(lp + v, 0.f);
        if (mp) *reinterpret_cast<uint2*>(mp + v) = make_uint2(seg_spread4(pb), seg_spread4(pb >> 4));
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const unsigned long long bp = __ballot((pb >> k) & 1u), by = __ballot((yb >> k) & 1u);
        np += __popcll(bp);
        ny += __popcll(by);
        ni += __popcll(bp & by);
      }
    }
    tail0 = g1;
  }
  for (int64_t base = tail0 + wave * 64; base < v1; base += 256) {
    const int64_t v = base + lane;
    bool p = false, y = false;
    if (v < v1) {
      p = seg_bit1<PGE>(pp + v, bound);
      if (lp) y = seg_bit1<false>(lp + v, 0.f);
      if (mp) mp[v] = p ? 1 : 0;
    }
    const unsigned long long bp = __ballot(p), by = __ballot(y);
    np += __popcll(bp);
    ny += __popcll(by);
    ni += __popcll(bp & by);
  }
  if (lane == 0) { red[wave][0] = ni; red[wave][1] = np; red[wave][2] = ny; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int e = threadIdx.x;
    part[((int64_t)plane * nchunk + chunk) * 3 + e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
  }
}

// counts (planes, 3) int64 <- the chunk partials of a plane: thread t adds chunks t, t + 256, ..., then a fixed tree
__global__ __launch_bounds__(256) void seg_counts_finish_kernel(const uint32_t* __restrict__ part, int nchunk,
                                                                int64_t* __restrict__ counts) {
  __shared__ unsigned long long red[3][256];
  const int plane = blockIdx.x, t = threadIdx.x;
  unsigned long long s[3] = {0, 0, 0};
  for (int c = t; c < nchunk; c += 256) {
#pragma unroll
    for (int e = 0; e < 3; ++e) s[e] += part[((int64_t)plane * nchunk + c) * 3 + e];
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) red[e][t] = s[e];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
#pragma unroll
      for (int e = 0; e < 3; ++e) red[e][t] += red[e][t + w];
    }
    __syncthreads();
  }
  if (t < 3) counts[plane * 3 + t] = (int64_t)red[t][0];
}

// ---- seg_argmax ---------------------------------------------------------------------------------------------------------
// The classes of NV consecutive voxels of one batch item.  Logits: argmax over the C planes, the running best starting at
// -inf with class 0 and replaced only by a strictly greater value — ties go to the lowest index, a NaN never wins, an all-NaN
// (or all -inf) voxel is class 0; bf16 values are compared as stored (their conversion to fp32 is exact).  A uint8 input is a
// label map already: the class is the stored value (one >= C equals no channel index below).
template <int NV, typename PT>
__device__ __forceinline__ void pred_classes(const PT* pp, int64_t V, int64_t v, int C, int CP, int (&pc)[NV]) {
  float best[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) best[e] = -__builtin_huge_valf(), pc[e] = 0;
#pragma unroll 16
  for (int c = 0; c < CP; ++c)
    if (c < C) {
      float x[NV];
      aload<NV>(pp + c * V + v, x);
#pragma unroll
      for (int e = 0; e < NV; ++e)
        if (x[e] > best[e]) best[e] = x[e], pc[e] = c;
    }
}
template <int NV>
__device__ __forceinline__ void pred_classes(const uint8_t* pp, int64_t, int64_t v, int, int, int (&pc)[NV]) {
  if constexpr (NV == 4) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(pp + v);
#pragma unroll
    for (int e = 0; e < 4; ++e) pc[e] = (int)((w >> (8 * e)) & 0xffu);
  } else {
    pc[0] = pp[v];
  }
}

// NV voxels of every lane of the wave (`on`: this lane has some): classes, the optional outputs, the ballots of the counts
template <int NV, int CP, typename PT, typename LT>
__device__ __forceinline__ void argmax_step(bool on, const PT* pp, const LT* lp, uint8_t* mp, uint8_t* op, int64_t V, int64_t v,
                                            int C, bool count, uint32_t (&n)[CP][3]) {
  int pc[NV], yc[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) pc[e] = -1, yc[e] = -1;
  if (on) {
    pred_classes<NV>(pp, V, v, C, CP, pc);
    if (lp) {
      if constexpr (NV == 4) label_classes4(lp + v, C, yc);
      else yc[0] = label_class(lp[v], C);
    }
    if (mp) {
      if constexpr (NV == 4)
        *reinterpret_cast<uint32_t*>(mp + v) = (uint32_t)pc[0] | ((uint32_t)pc[1] << 8) | ((uint32_t)pc[2] << 16) | ((uint32_t)pc[3] << 24);
      else mp[v] = (uint8_t)pc[0];
    }
    if (op) {
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C) {
          if constexpr (NV == 4)
            *reinterpret_cast<uint32_t*>(op + c * V + v) = (uint32_t)(pc[0] == c) | ((uint32_t)(pc[1] == c) << 8) |
                                                           ((uint32_t)(pc[2] == c) << 16) | ((uint32_t)(pc[3] == c) << 24);
          else op[c * V + v] = pc[0] == c ? 1 : 0;
        }
    }
  }
  if (count) {
#pragma unroll
    for (int c = 0; c < CP; ++c)
      if (c < C) {
#pragma unroll
        for (int e = 0; e < NV; ++e) {
          const unsigned long long bp = __ballot(pc[e] == c), by = __ballot(yc[e] == c);
          n[c][0] += __popcll(bp & by);
          n[c][1] += __popcll(bp);
          n[c][2] += __popcll(by);
        }
      }
  }
}

// grid (nchunk, B); pred (B, C, V) logits or (B, 1, V) uint8 classes; part (B·C, nchunk, 3) uint32, the layout that
// seg_counts_finish_kernel sums.  CP = 4 / 8 / 16 channel slots, C <= CP at run time.  VEC: V % 4 == 0 and every base pointer
// is 16-byte aligned: groups of 4 voxels per lane, then (as in seg_counts_kernel) the rest of the chunk one voxel per lane.
template <typename PT, typename LT, int CP, bool VEC>
__global__ __launch_bounds__(256) void seg_argmax_kernel(const PT* __restrict__ pred, const LT* __restrict__ label,
                                                         uint8_t* __restrict__ map, uint8_t* __restrict__ onehot,
                                                         uint32_t* __restrict__ part, int64_t V, int64_t per, int nchunk, int C) {
  __shared__ uint32_t red[4][CP * 3];
  constexpr bool LOGITS = !std::is_same<PT, uint8_t>::value;
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t v0 = (int64_t)chunk * per, v1 = min(V, v0 + per);
  const PT* pp = pred + (int64_t)b * (LOGITS ? C : 1) * V;
  const LT* lp = label ? label + (int64_t)b * V : nullptr;
  uint8_t* mp = map ? map + (int64_t)b * V : nullptr;
  uint8_t* op = onehot ? onehot + (int64_t)b * C * V : nullptr;
  const bool count = part != nullptr;
  uint32_t n[CP][3];
#pragma unroll
  for (int c = 0; c < CP; ++c) n[c][0] = n[c][1] = n[c][2] = 0;
  int64_t tail0 = v0;
  if constexpr (VEC) {
    const int64_t g1 = v0 + ((v1 - v0) & ~(int64_t)3);   // whole groups of 4 (v0 is a multiple of 4)
    for (int64_t base = v0 + wave * 256; base < g1; base += 1024) {
      const int64_t v = base + lane * 4;
      argmax_step<4, CP>(v < g1, pp, lp, mp, op, V, v, C, count, n);
    }
    tail0 = g1;
  }
  for (int64_t base = tail0 + wave * 64; base < v1; base += 256) {
    const int64_t v = base + lane;
    argmax_step<1, CP>(v < v1, pp, lp, mp, op, V, v, C, count, n);
  }
  if (count) {
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < CP; ++c)
#pragma unroll
        for (int e = 0; e < 3; ++e) red[wave][c * 3 + e] = n[c][e];
    }
    __syncthreads();
    if (threadIdx.x < 3 * C) {
      const int c = threadIdx.x / 3, e = threadIdx.x % 3;
      part[(((int64_t)b * C + c) * nchunk + chunk) * 3 + e] =
          (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    }
  }
}

// ---- mask_edges ---------------------------------------------------------------------------------------------------------
// axes: bit 0 = W, bit 1 = H, bit 2 = D is a spatial axis of the image (a lifted unit axis has no neighbours to test)
__global__ __launch_bounds__(256) void mask_edges_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ edges,
                                                         unsigned long long* __restrict__ counts, int D, int H, int W,
                                                         int axes) {
  __shared__ uint32_t red[4];
  const int plane = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t HW = (int64_t)H * W, V = HW * D;
  const uint8_t* m = mask + (int64_t)plane * V;
  uint8_t* o = edges + (int64_t)plane * V;
  uint32_t n = 0;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < V; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    bool e = false;
    if (i < V) {
      if (m[i] != 0) {
        const int x = (int)(i % W);
        const int64_t r = i / W;
        const int y = (int)(r % H), z = (int)(r / H);
        if (axes & 1) e = e || x == 0 || x == W - 1 || m[i - 1] == 0 || m[i + 1] == 0;
        if (axes & 2) e = e || y == 0 || y == H - 1 || m[i - W] == 0 || m[i + W] == 0;
        if (axes & 4) e = e || z == 0 || z == D - 1 || m[i - HW] == 0 || m[i + HW] == 0;
      }
      o[i] = e ? 1 : 0;
    }
    n += __popcll(__ballot(e));
  }
  if (lane == 0) red[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t s = (red[0] + red[1]) + (red[2] + red[3]);
    if (s) atomicAdd(counts + plane, (unsigned long long)s);   // integer: the total does not depend on the order
  }
}

// ---- edge_min_dist2 -----------------------------------------------------------------------------------------------------
constexpr int MD_TILE = 1024;   // targets per LDS tile (16 KiB)
constexpr int MD_QPL = 4;       // queries per lane
constexpr int MD_QPB = 256 * MD_QPL;

// q, t: (n, 4) fp32 = integer voxel coordinates on up to three axes, 0 in the unused columns.  out (nsplit, nq): the minimum
// over the targets [split · per, min(nt, (split + 1) · per)) of Σ_k w_k (q_k − t_k)², w = spacing².  UNIT: w = 1, three
// subtractions, a product and two FMAs per pair; otherwise the three exact squares are weighted: d = w0 dx² + w1 dy² + w2 dz².
template <bool UNIT>
__global__ __launch_bounds__(256) void edge_min_dist2_kernel(const float4* __restrict__ q, int64_t nq,
                                                             const float4* __restrict__ t, int64_t nt, float w0, float w1,
                                                             float w2, float* __restrict__ out, int64_t per) {
  __shared__ float4 tile[MD_TILE];
  const int64_t t0 = (int64_t)blockIdx.y * per, t1 = min(nt, t0 + per);
  const int64_t q0 = (int64_t)blockIdx.x * MD_QPB + threadIdx.x;
  float qx[MD_QPL], qy[MD_QPL], qz[MD_QPL], m[MD_QPL];
#pragma unroll
  for (int k = 0; k < MD_QPL; ++k) {
    const float4 v = q[min(q0 + k * 256, nq - 1)];
    qx[k] = v.x; qy[k] = v.y; qz[k] = v.z;
    m[k] = __builtin_huge_valf();
  }
  for (int64_t tb = t0; tb < t1; tb += MD_TILE) {
    const int n = (int)min((int64_t)MD_TILE, t1 - tb);
    const int n4 = (n + 3) & ~3;                       // padded with copies of the last target: the minimum ignores them
    __syncthreads();
    for (int j = threadIdx.x; j < n4; j += 256) tile[j] = t[tb + min(j, n - 1)];
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < n4; ++j) {
      const float4 p = tile[j];
#pragma unroll
      for (int k = 0; k < MD_QPL; ++k) {
        const float dx = qx[k] - p.x, dy = qy[k] - p.y, dz = qz[k] - p.z;
        float d;
        if constexpr (UNIT) d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
        else d = __builtin_fmaf(w2, dz * dz, __builtin_fmaf(w1, dy * dy, w0 * (dx * dx)));
        m[k] = __builtin_fminf(m[k], d);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < MD_QPL; ++k) {
    const int64_t i = q0 + k * 256;
    if (i < nq) out[(int64_t)blockIdx.y * nq + i] = m[k];
  }
}

// out[i] = min over the splits, taken in split order
__global__ __launch_bounds__(256) void edge_min_combine_kernel(const float* __restrict__ part, int nsplit, int64_t nq,
                                                               float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) {
    float m = part[i];
    for (int s = 1; s < nsplit; ++s) m = __builtin_fminf(m, part[(int64_t)s * nq + i]);
    out[i] = m;
  }
}

static bool seg_kind_ok(int k) { return k == FZ_SEG_F32 || k == FZ_SEG_BF16 || k == FZ_SEG_U8; }
static int seg_esize(int k) { return k == FZ_SEG_F32 ? 4 : (k == FZ_SEG_BF16 ? 2 : 1); }
static bool seg_aligned(const void* p, int bytes) { return !p || ((uintptr_t)p % (uintptr_t)bytes) == 0; }

// elements of a plane per workgroup: SEG_CHUNK, grown in multiples of 2048 once a plane would need more than 4096 chunks
static int64_t seg_per(int64_t V) {
  int64_t per = SEG_CHUNK;
  if ((V + per - 1) / per > 4096) per = (((V + 4095) / 4096 + 2047) / 2048) * 2048;
  return per;
}

template <typename PT, bool PGE, typename LT>
static void seg_counts_launch(bool vec, const void* pred, const void* label, uint8_t* mask, uint32_t* part, float bound,
                              int planes, int64_t V, hipStream_t s) {
  const int64_t per = seg_per(V);
  const int nchunk = (int)((V + per - 1) / per);
  const dim3 grid(nchunk, planes), block(256);
  if (vec)
    hipLaunchKernelGGL((seg_counts_kernel<PT, PGE, LT, true>), grid, block, 0, s, (const PT*)pred, (const LT*)label, mask,
                       part, bound, V, per, nchunk);
  else
    hipLaunchKernelGGL((seg_counts_kernel<PT, PGE, LT, false>), grid, block, 0, s, (const PT*)pred, (const LT*)label, mask,
                       part, bound, V, per, nchunk);
}

template <typename PT, bool PGE>
static void seg_counts_label(int label_kind, bool vec, const void* pred, const void* label, uint8_t* mask, uint32_t* part,
                             float bound, int planes, int64_t V, hipStream_t s) {
  if (label_kind == FZ_SEG_F32) seg_counts_launch<PT, PGE, float>(vec, pred, label, mask, part, bound, planes, V, s);
  else if (label_kind == FZ_SEG_BF16) seg_counts_launch<PT, PGE, bf16>(vec, pred, label, mask, part, bound, planes, V, s);
  else seg_counts_launch<PT, PGE, uint8_t>(vec, pred, label, mask, part, bound, planes, V, s);
}

template <typename PT, typename LT>
static void seg_argmax_launch(bool vec, const void* pred, const void* label, uint8_t* map, uint8_t* onehot, uint32_t* part,
                              int B, int C, int64_t V, hipStream_t s) {
  const int64_t per = seg_per(V);
  const int nchunk = (int)((V + per - 1) / per);
  const dim3 grid(nchunk, B), block(256);
  auto go = [&](auto cp, auto vc) {
    hipLaunchKernelGGL((seg_argmax_kernel<PT, LT, decltype(cp)::value, decltype(vc)::value>), grid, block, 0, s, (const PT*)pred,
                       (const LT*)label, map, onehot, part, V, per, nchunk, C);
  };
  auto slots = [&](auto vc) {
    if (C <= 4) go(std::integral_constant<int, 4>{}, vc);
    else if (C <= 8) go(std::integral_constant<int, 8>{}, vc);
    else go(std::integral_constant<int, 16>{}, vc);
  };
  if (vec) slots(std::true_type{});
  else slots(std::false_type{});
}

// target splits of a (nq, nt) problem: enough workgroups for the chip (about 1024) when the query blocks alone are few, never
// more than the target tiles or 64; `per` targets per split, a multiple of the tile
static int md_splits(int64_t nq, int64_t nt, int64_t* per_out) {
  const int64_t qblocks = (nq + MD_QPB - 1) / MD_QPB, tiles = (nt + MD_TILE - 1) / MD_TILE;
  int64_t want = (1024 + qblocks - 1) / qblocks;
  if (want > tiles) want = tiles;
  if (want > 64) want = 64;
  if (want < 1) want = 1;
  const int64_t per = ((tiles + want - 1) / want) * MD_TILE;
  if (per_out) *per_out = per;
  return (int)((nt + per - 1) / per);
}

}  // namespace fz

using namespace fz;

extern "C" int fz_seg_counts_chunks(int64_t V) {
  if (V < 1) return 0;
  const int64_t per = seg_per(V);
  return (int)((V + per - 1) / per);
}

extern "C" int64_t fz_seg_counts_workspace_bytes(int planes, int64_t V) {
  if (planes < 1 || V < 1) return -1;
  return (int64_t)planes * fz_seg_counts_chunks(V) * 3 * (int64_t)sizeof(uint32_t);
}

extern "C" int fz_seg_counts(const void* pred, int pred_kind, const void* label, int label_kind, float bound, uint8_t* mask,
                             void* workspace, int64_t* counts, int planes, int64_t V, fz_stream_t stream) {
  if (!pred) return fail(FZ_E_ARG, "fz_seg_counts: null pred");
  if (!seg_kind_ok(pred_kind) || (label && !seg_kind_ok(label_kind))) return fail(FZ_E_ARG, "fz_seg_counts: bad kind");
  if (!mask && !counts) return fail(FZ_E_ARG, "fz_seg_counts: neither mask nor counts requested");
  if (!workspace) return fail(FZ_E_ARG, "fz_seg_counts: null workspace");   // the chunk partials are always written
  if (bound != bound) return fail(FZ_E_ARG, "fz_seg_counts: bound is NaN");
  if (planes < 1 || planes > 65535 || V < 1) return fail(FZ_E_SHAPE, "fz_seg_counts: 1 <= planes <= 65535, V >= 1");
  if (!seg_aligned(pred, seg_esize(pred_kind)) || (label && !seg_aligned(label, seg_esize(label_kind))))
    return fail(FZ_E_ARG, "fz_seg_counts: pointer not aligned to its element");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = (planes == 1 || V % 8 == 0) && V >= 8 && seg_aligned(pred, 16) && seg_aligned(label, 16) &&
                   seg_aligned(mask, 16);
  uint32_t* part = (uint32_t*)workspace;
  if (pred_kind == FZ_SEG_F32) seg_counts_label<float, true>(label_kind, vec, pred, label, mask, part, bound, planes, V, s);
  else if (pred_kind == FZ_SEG_BF16) seg_counts_label<bf16, true>(label_kind, vec, pred, label, mask, part, bound, planes, V, s);
  else seg_counts_label<uint8_t, false>(label_kind, vec, pred, label, mask, part, bound, planes, V, s);
  FZ_LAUNCH_CHECK();
  if (counts) {
    hipLaunchKernelGGL(seg_counts_finish_kernel, dim3(planes), dim3(256), 0, s, part, fz_seg_counts_chunks(V), counts);
    FZ_LAUNCH_CHECK();
  }
  return FZ_OK;
}

extern "C" int64_t fz_seg_argmax_workspace_bytes(int B, int C, int64_t V) {
  if (B < 1 || C < 1 || V < 1) return -1;
  return (int64_t)B * C * fz_seg_counts_chunks(V) * 3 * (int64_t)sizeof(uint32_t);
}

extern "C" int fz_seg_argmax(const void* pred, int pred_kind, const void* label, int label_kind, uint8_t* map, uint8_t* onehot,
                             void* workspace, int64_t* counts, int B, int C, int64_t V, fz_stream_t stream) {
  if (!pred) return fail(FZ_E_ARG, "fz_seg_argmax: null pred");
  if (!seg_kind_ok(pred_kind)) return fail(FZ_E_ARG, "fz_seg_argmax: pred kind must be FZ_SEG_F32 / _BF16 / _U8");
  if (label && !label_kind_ok(label_kind)) return fail(FZ_E_ARG, "fz_seg_argmax: label kind must be FZ_LABEL_U8 / _I64 / _F32");
  if (!map && !onehot && !counts) return fail(FZ_E_ARG, "fz_seg_argmax: no output requested");
  if (counts && !workspace) return fail(FZ_E_ARG, "fz_seg_argmax: counts need the workspace");
  if (C < 2 || C > 16) return fail(FZ_E_UNSUPPORTED, "fz_seg_argmax: 2 <= C <= 16");
  if (B < 1 || B > 65535 || V < 1) return fail(FZ_E_SHAPE, "fz_seg_argmax: 1 <= B <= 65535, V >= 1");
  if (!seg_aligned(pred, seg_esize(pred_kind)) || (label && !seg_aligned(label, label_esize(label_kind))) ||
      !seg_aligned(counts, 8) || !seg_aligned(workspace, 4))
    return fail(FZ_E_ARG, "fz_seg_argmax: pointer not aligned to its element");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = V % 4 == 0 && seg_aligned(pred, 16) && seg_aligned(label, 16) && seg_aligned(map, 16) && seg_aligned(onehot, 16);
  uint32_t* part = counts ? (uint32_t*)workspace : nullptr;
  const int lk = label ? label_kind : FZ_LABEL_U8;
  by_label_kind(lk, [&](auto yt) {
    using LT = decltype(yt);
    if (pred_kind == FZ_SEG_F32) seg_argmax_launch<float, LT>(vec, pred, label, map, onehot, part, B, C, V, s);
    else if (pred_kind == FZ_SEG_BF16) seg_argmax_launch<bf16, LT>(vec, pred, label, map, onehot, part, B, C, V, s);
    else seg_argmax_launch<uint8_t, LT>(vec, pred, label, map, onehot, part, B, C, V, s);
  });
  FZ_LAUNCH_CHECK();
  if (counts) {
    hipLaunchKernelGGL(seg_counts_finish_kernel, dim3(B * C), dim3(256), 0, s, part, fz_seg_counts_chunks(V), counts);
    FZ_LAUNCH_CHECK();
  }
  return FZ_OK;
}

extern "C" int fz_mask_edges(const uint8_t* mask, uint8_t* edges, int64_t* counts, int planes, int nd, int D, int H, int W,
                             fz_stream_t stream) {
  if (!mask || !edges || !counts) return fail(FZ_E_ARG, "fz_mask_edges: null pointer");
  if (mask == edges) return fail(FZ_E_ARG, "fz_mask_edges: edges must not alias the mask");
  if (nd < 1 || nd > 3) return fail(FZ_E_ARG, "fz_mask_edges: 1 <= nd <= 3 spatial axes");
  if (planes < 1 || planes > 65535 || D < 1 || H < 1 || W < 1) return fail(FZ_E_SHAPE, "fz_mask_edges: sizes must be positive, planes <= 65535");
  if ((nd < 3 && D != 1) || (nd < 2 && H != 1)) return fail(FZ_E_SHAPE, "fz_mask_edges: the lifted axes of a 1-D / 2-D image must be 1");
  const int64_t V = (int64_t)D * H * W;
  if (V >= ((int64_t)1 << 40)) return fail(FZ_E_SHAPE, "fz_mask_edges: image too large");
  hipStream_t s = (hipStream_t)stream;
  FZ_HIP_OK(hipMemsetAsync(counts, 0, (size_t)planes * sizeof(int64_t), s));
  int64_t blocks = (V + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(mask_edges_kernel, dim3((unsigned)blocks, planes), dim3(256), 0, s, mask, edges,
                     (unsigned long long*)counts, D, H, W, (1 << nd) - 1);
  FZ_LAUNCH_CHECK();
  return FZ_OK;
}

extern "C" int fz_edge_min_dist2_splits(int64_t nq, int64_t nt) {
  if (nq < 1 || nt < 1) return 0;
  return md_splits(nq, nt, nullptr);
}

extern "C" int64_t fz_edge_min_dist2_workspace_bytes(int64_t nq, int64_t nt) {
  if (nq < 1 || nt < 1) return -1;
  const int ns = md_splits(nq, nt, nullptr);
  return ns > 1 ? (int64_t)ns * nq * (int64_t)sizeof(float) : 0;
}

extern "C" int fz_edge_min_dist2(const float* q, int64_t nq, const float* t, int64_t nt, float w0, float w1, float w2,
                                 float* out, void* workspace, fz_stream_t stream) {
  if (!q || !t || !out) return fail(FZ_E_ARG, "fz_edge_min_dist2: null pointer");
  if (nq < 1 || nt < 1 || nq > 0x7fffffff || nt > 0x7fffffff) return fail(FZ_E_SHAPE, "fz_edge_min_dist2: 1 <= nq, nt < 2^31");
  if (!(w0 >= 0.f && w1 >= 0.f && w2 >= 0.f) || w0 > 3e38f || w1 > 3e38f || w2 > 3e38f)
    return fail(FZ_E_ARG, "fz_edge_min_dist2: weights (spacing squared) must be finite and non-negative");
  if (!seg_aligned(q, 16) || !seg_aligned(t, 16)) return fail(FZ_E_ARG, "fz_edge_min_dist2: coordinate lists must be 16-byte aligned");
  int64_t per = 0;
  const int ns = md_splits(nq, nt, &per);
  if (ns > 1 && !workspace) return fail(FZ_E_ARG, "fz_edge_min_dist2: null workspace");
  hipStream_t s = (hipStream_t)stream;
  float* dst = ns > 1 ? (float*)workspace : out;
  const dim3 grid((unsigned)((nq + MD_QPB - 1) / MD_QPB), ns), block(256);
  const float4* q4 = (const float4*)q;
  const float4* t4 = (const float4*)t;
  if (w0 == 1.f && w1 == 1.f && w2 == 1.f)
    hipLaunchKernelGGL(edge_min_dist2_kernel<true>, grid, block, 0, s, q4, nq, t4, nt, w0, w1, w2, dst, per);
  else
    hipLaunchKernelGGL(edge_min_dist2_kernel<false>, grid, block, 0, s, q4, nq, t4, nt, w0, w1, w2, dst, per);
  FZ_LAUNCH_CHECK();
  if (ns > 1) {
    int64_t blocks = (nq + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(edge_min_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)workspace, ns, nq, out);
    FZ_LAUNCH_CHECK();
  }
  return FZ_OK;
}
