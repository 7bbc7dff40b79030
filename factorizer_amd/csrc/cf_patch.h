// cf_patch.h — the voxel → patch map of one shifted window of the fused FactMixer core (8x8x8 patches), for host and device:
// nmf_cf.h brings it to the kernels, tests/emul/emul_cf_patch.cpp compiles it with g++ against the gather formula.
#pragma once

#if defined(__HIPCC__)
#define FZ_CF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FZ_CF_HD inline
#endif

namespace fz {

// Index, inside one (sample, head), of the patch of a window that holds the TRUE voxel (d, h, w) of a (D, H, W) volume:
// patch (g0, g1, g2) of a window with cyclic shift (s0, s1, s2), normalised to [0, size), gathers the voxels
// (8 g + p − s) mod size (cf_chunk_voxel), so a voxel lies in patch ((z + s) mod size) / 8 on every axis.  The voxel-map
// analogue of cf_prev_patch, which starts from a tile's chunk.
FZ_CF_HD unsigned cf_voxel_patch(int d, int h, int w, int D, int H, int W, int s0, int s1, int s2) {
  d += s0; if (d >= D) d -= D;
  h += s1; if (h >= H) h -= H;
  w += s2; if (w >= W) w -= W;
  return (unsigned)(((d >> 3) * (H >> 3) + (h >> 3)) * (W >> 3) + (w >> 3));
}

#if defined(__HIPCC__)
// One value of the core's output a of a rank-1, two-window SWMatricize from the factors of both windows, with the bits that the
// launch pair fz_nmf_cf_fwd_store_factors + fz_nmf_cf_fwd_from_factors (divisor 2) stores: window 0 as cf_first_window forms it
// — (0.0f + fl(u0·v0)), the 0.0f turning a −0 product into +0 — then + fl(u1·v1), the product that window 1's wave program
// rounds into its registers, then cf_divide4's exact halving.  Both products are rounded BEFORE the adds: the empty asm keeps
// the compiler from contracting either into an FMA, which -ffp-contract=fast allows.  fp32 storage only (bf16 storage rounds
// the first window once more).
__device__ inline __attribute__((always_inline)) float cf_two_window_value(float u0, float v0, float u1, float v1) {
  float p0 = u0 * v0, p1 = u1 * v1;
  asm("" : "+v"(p0), "+v"(p1));
  return ((0.0f + p0) + p1) * 0.5f;
}
#endif

}  // namespace fz
