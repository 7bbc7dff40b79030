// deconv_bf16.hip — the grouped-correlation kernels of deconv_kernels.h on bf16 activation storage (a translation unit of its
// own, so the two storage types compile side by side; the entry points are in deconv.hip).
#include "deconv_kernels.h"

namespace fz {

int gcorr_launch_bf16(const GcArgs<bf16>& a, int kd, int kh, int kw, hipStream_t st) { return gcorr_launch<bf16>(a, kd, kh, kw, st); }

int gcorr_wgrad_launch_bf16(const bf16* in, const bf16* gout, float* gw, void* ws, int B, int G, int Ci, int Co, int D, int H,
                            int W, int kd, int kh, int kw, int w_batched, hipStream_t st) {
  return gcorr_wgrad_launch<bf16>(in, gout, gw, ws, B, G, Ci, Co, D, H, W, kd, kh, kw, w_batched, st);
}

}  // namespace fz
