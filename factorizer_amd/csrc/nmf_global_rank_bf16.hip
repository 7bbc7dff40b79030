// nmf_global_rank_bf16.hip — the split-N NMF kernels for ranks up to 32 on bf16 activation storage: the instances of
// nmf_global_rank.h with AT = bf16, in a translation unit of their own so that they compile beside the fp32 ones.
#include "nmf_global_rank.h"

namespace fz {
int gx_fwd_bf16(const WideArgs& a) { return gx_run_fwd<bf16>(a); }
int gx_bwd_bf16(const WideArgs& a) { return gx_run_bwd<bf16>(a); }
}  // namespace fz
