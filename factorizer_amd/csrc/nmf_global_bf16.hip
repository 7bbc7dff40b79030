// nmf_global_bf16.hip — the split-N NMF kernels (M <= 64, rank <= 4) on bf16 activation storage: the instances of
// nmf_global.h with AT = bf16, in a translation unit of their own so that they compile beside the fp32 ones.
#include "nmf_global.h"

namespace fz {
int gn_fwd_bf16(const WideArgs& a) { return gn_run_fwd<bf16>(a); }
int gn_bwd_bf16(const WideArgs& a) { return gn_run_bwd<bf16>(a); }
}  // namespace fz
