// topk_sets16.hip -- blp_topk_sets_typed's selection kernel over a 16-BIT candidate table (table_elem.h: IEEE half or
// bfloat16): the instantiations of topk_sets_kernel (topk_sets_kernel.h) for the two 16-bit storage types, next to the f32 ones
// of topk_sets.hip.  topk_sets.hip has the description of the call and launches everything else (coefficient rows, the cleared
// partial buffer, the unit prefix, merge, rescore).  No kernel uses scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "rank_common.h"
#include "table_elem.h"
#include "topk_sets_kernel.h"

#pragma clang fp contract(off)

namespace blp {

hipError_t launch_topk_sets_pass16(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, const TopkSetsWorkspace& w,
                                   int64_t q_head, const SetLookup& sets, int q_chunk, int s_max, int k, const FilterSpec& filter,
                                   int n_cu, hipStream_t stream) {
#define BLP_TOPK_SETS16_CASE(M, DD)                                                                                              \
    if (model == M && D == DD) {                                                                                                 \
        if (dtype == kTableF16)                                                                                                  \
            return topk_sets_pass<M, DD>(static_cast<const _Float16*>(table), N, ld, w, q_head, sets, q_chunk, s_max, k, filter, \
                                         n_cu, stream);                                                                          \
        if (dtype == kTableBF16)                                                                                                 \
            return topk_sets_pass<M, DD>(static_cast<const __bf16*>(table), N, ld, w, q_head, sets, q_chunk, s_max, k, filter,   \
                                         n_cu, stream);                                                                          \
        return hipErrorInvalidValue;                                                                                             \
    }
#define BLP_TOPK_SETS16_MODEL(M) BLP_TOPK_SETS16_CASE(M, 64) BLP_TOPK_SETS16_CASE(M, 128) BLP_TOPK_SETS16_CASE(M, 256)
    BLP_TOPK_SETS16_MODEL(TRANSE) BLP_TOPK_SETS16_MODEL(DISTMULT) BLP_TOPK_SETS16_MODEL(COMPLEX) BLP_TOPK_SETS16_MODEL(SIMPLE)
#undef BLP_TOPK_SETS16_MODEL
#undef BLP_TOPK_SETS16_CASE
    return hipErrorInvalidValue;
}

}  // namespace blp
