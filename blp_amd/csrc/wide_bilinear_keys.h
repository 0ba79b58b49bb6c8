// wide_bilinear_keys.h -- the first kernel of the exact passes for DistMult / ComplEx / SimplE at run-time width
// (rank_all_wide.hip: the whole table; rank_sets_wide_bilinear.hip: shared candidate sets): the true entities' keys by the
// pass's own arithmetic (wide_bilinear.h: wide_pair_score) and the queries' accumulators zeroed.  Internal linkage: every file
// that includes it gets its own copy in its own code object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "wide_bilinear.h"

#pragma clang fp contract(off)

namespace blp {

namespace {

// True-entity keys, eight lanes per query (wide_pair_score); the queries' accumulators start at zero.
template <int MODEL>
__global__ __launch_bounds__(256) void wide_bilinear_true_key_kernel(int D, const QRows q_fixed, const QRows q_rel, const QRows q_true,
                                                                     int64_t q_head, int64_t Q, float* __restrict__ key_true,
                                                                     unsigned long long* __restrict__ acc) {
    const int sub = threadIdx.x & 7;
    for (int64_t q0 = blockIdx.x * 32ll; q0 < Q; q0 += gridDim.x * 32ll) {  // workgroup-uniform
        const int64_t qq = q0 + (threadIdx.x >> 3), q = qq < Q ? qq : Q - 1;
        const float* e = q_true.row(q);
        const float* f = q_fixed.row(q);
        const float* r = q_rel.row(q);
        const bool head = q0 + 31 < q_head ? true : (q0 >= q_head ? false : q < q_head);
        float key;
        if (q0 + 31 < q_head || q0 >= q_head) {  // wave-uniform side (all but the one group that straddles q_head)
            key = head ? wide_pair_score<MODEL, HEAD>(e, f, r, D, sub) : wide_pair_score<MODEL, TAIL>(e, f, r, D, sub);
        } else {  // both sides by every lane, each lane keeps its own
            const float kh = wide_pair_score<MODEL, HEAD>(e, f, r, D, sub);
            const float kt = wide_pair_score<MODEL, TAIL>(e, f, r, D, sub);
            key = head ? kh : kt;
        }
        if (sub == 0 && qq < Q) {
            key_true[qq] = key;
            acc[qq] = 0;
        }
    }
}

}  // namespace

}  // namespace blp
