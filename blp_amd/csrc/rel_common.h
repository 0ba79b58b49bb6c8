// rel_common.h -- what the relation-prediction kernels share (rank_rels.hip: a lane holds a whole relation row, D in {64, 128,
// 256}; rank_rels_wide.hip: a lane holds a slab of the row's columns, TransE at any width): the queries' addressing, the filter
// test of a lane's relation and the grid rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"

namespace blp {

constexpr int kRelMaxGroups = 1024;    // workgroups of a launch (they stride over the query chunks)

struct RelQueries {
    const float* source;
    int64_t ld;
    const int64_t* head_row;
    const int64_t* tail_row;
    __device__ __forceinline__ const float* head(int64_t q) const { return source + head_row[q] * ld; }
    __device__ __forceinline__ const float* tail(int64_t q) const { return source + tail_row[q] * ld; }
};
// (the kernels take the four fields as __restrict__ parameters: the query vectors are then provably untouched by the kernel's
//  stores, which is what lets a wave-uniform read of them be a scalar load)
#define REL_QUERY_PARAMS \
    const float* __restrict__ source, int64_t ld_src, const int64_t* __restrict__ head_row, const int64_t* __restrict__ tail_row
#define REL_QUERY_ARGS(qs) (qs).source, (qs).ld, (qs).head_row, (qs).tail_row

// Does query q's filter segment remove relation `rel`?  Wave-uniform walk (scalar loads); exclude[q] is never removed, an id
// outside [0, R) matches no lane.
__device__ __forceinline__ bool rel_removed(const FilterSpec& f, int64_t q, int64_t rel) {
    const int64_t lo = f.lo[q], hi = f.hi[q];
    const int64_t keep = f.exclude ? f.exclude[q] : -1;
    bool removed = false;
    for (int64_t c = lo; c < hi; ++c) {
        const int64_t v = f.val[c];
        removed |= v == rel && v != keep;
    }
    return removed;
}

static inline unsigned rel_grid(int64_t n_chunks) { return (unsigned)(n_chunks < kRelMaxGroups ? n_chunks : kRelMaxGroups); }

}  // namespace blp
