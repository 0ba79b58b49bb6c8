// lists_step.h -- one 64-entry STEP of a per-query candidate list for lists_topk.hip (the k best entries of each list): lane l
// takes entry l of the step, and every lane ends up with score_fn's value of ITS entry against the step's query, bit for bit
// (sign of zero included).
//   A row outside [row_base, row_base + N) (-1 padding, another shard's row) is skipped: its score is NaN, its lane reads
//   the row of the step's first valid lane instead (nothing is read if no lane is valid).
//   TransE (any D % 4 == 0, D <= 1024): transe_key_64_one_query_rt -- the 64 rows fetched in whole 128-byte lines, 32
//     columns at a time, transposed through a wave-private LDS slab; the L1 chain of a pair stays in one lane.
//   bilinear models (D = 64 / 128 / 256): 32 lanes per pair in torch.sum's order (exact_coop.h: coop_score, here with the
//     reference's literal "0 + first term" additions, Scorer<>::score<true>: the stored score carries the reference's
//     sign of zero; comparisons do not see it).  Half-wave h takes entries 32 h + i, i = 0 .. 31.
// The query's two vectors are staged once per (wave, query) in LDS (lists_stage_query); the filter walk (lists_unfiltered)
// looks lanes up in the query's filter segment.
// rank_lists.hip's kernel holds the SAME step, statement for statement, inline in its loop (a fix here belongs there too).  It
// does not include this header: with the step called from here its kernels did not compile to the instructions they had
// (DESIGN 4.9.1), and an entry point that exists may not change.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exact_coop.h"
#include "launch.h"
#include "rank_common.h"
#include "score_core.h"
#include "table_elem.h"

#pragma clang fp contract(off)

namespace blp {

typedef unsigned long long u64;

constexpr int kListsWaves = 4;     // waves per workgroup (TransE wider than kListsWideFrom: 2, the LDS of the staged queries)
constexpr int kListsWideFrom = 512;

// coop_score (exact_coop.h) with the literal zeros of Scorer<>::score<true>: lane j is accumulator A[j] = 0 + term j, ...
template <int MODEL, int SIDE, int D, class TE>
__device__ __forceinline__ float coop_score_lz(const TE* __restrict__ e, const float* f, const float* r, int sub) {
    constexpr int NT = MODEL == DISTMULT ? D : D / 2;
    float a = 0.0f + score_term<MODEL, SIDE, D>(e, f, r, sub);
#pragma unroll
    for (int k = 1; k < NT / 32; ++k) a = a + score_term<MODEL, SIDE, D>(e, f, r, 32 * k + sub);
    float v = a + __shfl_down(a, 8, 32);
    v = v + __shfl_down(a, 16, 32);
    v = v + __shfl_down(a, 24, 32);
    float s = 0.0f + __shfl(v, 0, 32);
#pragma unroll
    for (int l = 1; l < 8; ++l) s = s + __shfl(v, l, 32);
    return MODEL == SIMPLE ? s / 2.0f : s;
}

// The lanes of `mask` whose entry (table row `row` of the lane) query q's filter segment does NOT remove.
__device__ __forceinline__ u64 lists_unfiltered(const FilterSpec& f, int64_t q, int64_t N, int row, u64 mask, int lane) {
    const int64_t lo = f.lo[q], hi = f.hi[q];
    for (int64_t c = lo; c < hi && mask; c += 64) {
        const int v = c + lane < hi ? (int)filter_row(f, q, c + lane, N) : -1;
        u64 m = mask;
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            if (__ballot(v == __shfl(row, b))) mask &= ~(1ull << b);
        }
    }
    return mask;
}

// Query q's two vectors into the wave's LDS (qa, qb: Dr floats each); the caller fences before and after (wave_lds_sync).
// MODEL == TRANSE: D = 0, the width is the run-time Dr
template <int MODEL, int D>
__device__ __forceinline__ void lists_stage_query(const QRows& q_fixed, const QRows& q_rel, int64_t q, int Dr, bool head, float* qa,
                                                  float* qb, int lane) {
    if constexpr (MODEL == TRANSE) {
        stage_query_rt(q_fixed.row(q), q_rel.row(q), Dr, head, qa, qb, lane);
    } else {
        const float* f = q_fixed.row(q);
        const float* r = q_rel.row(q);
        for (int c = 4 * lane; c < D; c += 256) {
            *reinterpret_cast<float4*>(qa + c) = *reinterpret_cast<const float4*>(f + c);
            *reinterpret_cast<float4*>(qb + c) = *reinterpret_cast<const float4*>(r + c);
        }
    }
}

// The step: entry p of list_row (this lane's; live: p is inside the query's list) -> row (local to the shard; valid: inside
// it) and the entry's score (NaN for a lane that is not valid).
template <int MODEL, int D, class TE>
__device__ __forceinline__ float lists_step(const TE* __restrict__ table, int64_t N, int64_t ld, int64_t row_base,
                                            const int64_t* __restrict__ list_row, int64_t p, bool live, const float* qa,
                                            const float* qb, int Dr, bool head, float* slab, int lane, int64_t& row, bool& valid) {
    const float nan = __uint_as_float(0x7fc00000u);
    row = live ? list_row[p] - row_base : -1;
    valid = (uint64_t)row < (uint64_t)N;
    const u64 vmask = __ballot(valid);
    float s = nan;
    if (vmask) {
        const int src = __builtin_ctzll(vmask);
        const int lrow = (int)row;  // N < 2^31
        const TE* pe = table + (int64_t)(valid ? lrow : __shfl(lrow, src)) * ld;
        if constexpr (MODEL == TRANSE) {
            s = transe_key_64_one_query_rt<TE>(pe, qa, qb, Dr, head, slab, lane);
        } else {
            const int half = lane >> 5, sub = lane & 31;
            const unsigned either = (unsigned)vmask | (unsigned)(vmask >> 32);
#pragma unroll 2
            for (int j = 0; j < 32; ++j) {
                if (!((either >> j) & 1u)) continue;  // wave-uniform: neither half has a valid entry here
                const TE* e = shfl_ptr(pe, 32 * half + j);
                const float v = head ? coop_score_lz<MODEL, HEAD, D>(e, qa, qb, sub) : coop_score_lz<MODEL, TAIL, D>(e, qa, qb, sub);
                if (sub == j) s = v;
            }
        }
        if (!valid) s = nan;
    }
    return s;
}

}  // namespace blp
