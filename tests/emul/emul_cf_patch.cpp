// emul_cf_patch.cpp — host build of the voxel → patch map that the consumers of the core's factor pair use
// (factorizer_amd/csrc/cf_patch.h, the code the kernels compile for gfx950).  Built with g++ and loaded through ctypes by
// tests/test_outproj_factors_cpu.py.
#include <cstdint>

#include "../../factorizer_amd/csrc/cf_patch.h"

// out[(d·H + h)·W + w] = patch index of every voxel of a (D, H, W) volume for a window with the normalised shift (s0, s1, s2)
extern "C" void emu_cf_voxel_patch(int D, int H, int W, int s0, int s1, int s2, int32_t* out) {
  for (int d = 0; d < D; ++d)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w) out[((int64_t)d * H + h) * W + w] = (int32_t)fz::cf_voxel_patch(d, h, w, D, H, W, s0, s1, s2);
}
