// rank_sets16.hip -- blp_rank_sets_typed's kernels over a 16-BIT candidate table (table_elem.h: IEEE half or bfloat16): the
// instantiations of rank_sets_kernel (rank_sets_kernel.h) and of the set-aware filter_finalize_kernel (filter_finalize.h) for
// the two 16-bit storage types, next to the f32 ones of rank_sets.hip and rank_all.hip.  rank_sets.hip has the description of
// the call and launches everything else (true keys, coefficient rows, the unit prefix).  No kernel uses scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "filter_finalize.h"
#include "launch.h"
#include "rank_common.h"
#include "rank_sets_kernel.h"
#include "table_elem.h"

#pragma clang fp contract(off)

namespace blp {

template <int MODEL, int D, class TE>
static hipError_t filter_finalize_sets16_impl(const TE* table, int64_t N, int64_t ld, const QRows q_fixed, const QRows q_rel,
                                              const float* key_true, int64_t q_head, int64_t q_tail, const FilterSpec& filter,
                                              const SetLookup& sets, const unsigned long long* acc, int32_t* counts, hipStream_t stream) {
    filter_finalize_kernel<MODEL, D, TE, SetLookup><<<(int)((q_head + q_tail + kSweepQueries - 1) / kSweepQueries), 256, 0, stream>>>(
        table, N, ld, q_fixed, q_rel, key_true, q_head, q_tail, filter, acc, 1, counts, 0, sets);
    return hipGetLastError();
}

#define BLP_SETS16_TYPED(FN, M, DD, ...)                                                                     \
    if (model == M && D == DD) {                                                                             \
        if (dtype == kTableF16) return FN<M, DD>(static_cast<const _Float16*>(table), __VA_ARGS__);          \
        if (dtype == kTableBF16) return FN<M, DD>(static_cast<const __bf16*>(table), __VA_ARGS__);           \
        return hipErrorInvalidValue;                                                                         \
    }
#define BLP_SETS16_MODEL(FN, M, ...) \
    BLP_SETS16_TYPED(FN, M, 64, __VA_ARGS__) BLP_SETS16_TYPED(FN, M, 128, __VA_ARGS__) BLP_SETS16_TYPED(FN, M, 256, __VA_ARGS__)
#define BLP_SETS16_DISPATCH(FN, ...)                                                             \
    BLP_SETS16_MODEL(FN, TRANSE, __VA_ARGS__) BLP_SETS16_MODEL(FN, DISTMULT, __VA_ARGS__)        \
    BLP_SETS16_MODEL(FN, COMPLEX, __VA_ARGS__) BLP_SETS16_MODEL(FN, SIMPLE, __VA_ARGS__)         \
    return hipErrorInvalidValue;

hipError_t launch_rank_sets_pass16(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, const SetsWorkspace& w,
                                   int64_t q_head, const SetLookup& sets, int n_cu, hipStream_t stream) {
    BLP_SETS16_DISPATCH(rank_sets_pass, N, ld, w, q_head, sets, n_cu, stream)
}

hipError_t launch_filter_finalize_sets16(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, const QRows q_fixed,
                                         const QRows q_rel, const float* key_true, int64_t q_head, int64_t q_tail,
                                         const FilterSpec& filter, const SetLookup& sets, const unsigned long long* acc,
                                         int32_t* counts, hipStream_t stream) {
    if (!filter.on()) return hipErrorInvalidValue;
    BLP_SETS16_DISPATCH(filter_finalize_sets16_impl, N, ld, q_fixed, q_rel, key_true, q_head, q_tail, filter, sets, acc, counts, stream)
}

#undef BLP_SETS16_DISPATCH
#undef BLP_SETS16_MODEL
#undef BLP_SETS16_TYPED

}  // namespace blp
