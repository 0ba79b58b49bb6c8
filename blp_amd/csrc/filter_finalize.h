// filter_finalize.h -- the last kernel of a ranking call: the filtered setting's removed candidates re-scored against the true
// entity, then counts[q] = {gt, ge, gt - fgt, ge - fge} from the packed accumulators.  A template over the candidate table's
// storage type (table_elem.h) and over the candidate-set lookup (rank_common.h: NoSets / SetLookup), instantiated where it is
// launched: rank_all.hip (every path without sets, and f32 tables with sets) and rank_sets16.hip (16-bit tables with sets).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exact_coop.h"
#include "launch.h"
#include "rank_common.h"
#include "score_core.h"

#pragma clang fp contract(off)

namespace blp {

// Packed counts of query q_base + (threadIdx.x & 63) summed over the n_partials slots acc[p * Q + q] -- workgroup of four
// waves: wave w adds the slots p = w (mod 4), the first wave gets the total (the others: garbage).  Ends with a barrier.
__device__ __forceinline__ unsigned long long sum_partials(const unsigned long long* __restrict__ acc, int n_partials,
                                                           int64_t Q, int64_t q_base,
                                                           unsigned long long (&sums)[3][kSweepQueries]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = q_base + lane;
    unsigned long long a = 0;
    if (q < Q) {
        int p = wave;
#pragma unroll 1
        for (; p + 28 < n_partials; p += 32) {  // eight independent loads in flight
            unsigned long long v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = acc[(int64_t)(p + 4 * k) * Q + q];
#pragma unroll
            for (int k = 0; k < 8; ++k) a += v[k];
        }
        for (; p < n_partials; p += 4) a += acc[(int64_t)p * Q + q];
    }
    if (wave > 0) sums[wave - 1][lane] = a;
    __syncthreads();
    if (wave == 0) a += sums[0][lane] + sums[1][lane] + sums[2][lane];
    return a;
}

// ------------------------------------------------------------------------------------------------
// Last kernel of a call.  Filtered setting (train.py:159-171): a workgroup of four waves owns 64 consecutive queries.
// Its first wave reads their filter segments and scans the segment lengths; the workgroup's entries -- the rows the
// filter removes, usually few: most evaluation queries have none -- are then numbered 0 .. total - 1 across the 64
// queries and scored by the cooperative exact routines of exact_coop.h (TransE: 64 entries per wave and step, one
// lane each, rows gathered in whole lines; bilinear models: one entry per 32-lane half-wave), each entry finding its
// query by a binary search in the scanned lengths.  Entries at or above the true entity are counted per query in
// LDS; finally thread q writes query q's four counts.  (One wave per query, one lane per entry with its own
// row-by-row loads: 127 us for the 105 740 queries of the FB15k-237 block, of which 9 % have an entry.)
// Which side a query replaces: plain blocks -- queries [0, q_head) the head --, or the reference loop's layout
// (blp_rank_all_batches: batch after batch of `batch` triples, each batch as [its head queries | its tail queries]).
__host__ __device__ inline bool replaces_head(int64_t q, int64_t q_head, int64_t Q, int64_t batch) {
    if (batch <= 0) return q < q_head;
    const int64_t first = q / (2 * batch) * batch, n = Q / 2, nb = n - first < batch ? n - first : batch;
    return q - 2 * first < nb;
}

// SETS (rank_common.h: NoSets / SetLookup): with candidate sets an entry is removed only if its row is in the query's set.
template <int MODEL, int D, class TE = float, class SETS = NoSets>  // TE: the candidate table's storage type (table_elem.h)
__global__ __launch_bounds__(256) void filter_finalize_kernel(
    const TE* __restrict__ table, int64_t N, int64_t ld, const QRows q_fixed,
    const QRows q_rel, const float* __restrict__ key_true, int64_t q_head,
    int64_t q_tail, const FilterSpec filter, const unsigned long long* __restrict__ acc, int n_partials,
    int32_t* __restrict__ counts, int64_t batch, const SETS sets) {
    __shared__ unsigned long long partial_sums[3][kSweepQueries];
    __shared__ int64_t set_lo[SETS::on ? kSweepQueries : 1], set_hi[SETS::on ? kSweepQueries : 1];  // the queries' sets (entries of set_row)
    __shared__ int prefix[kSweepQueries + 1];
    __shared__ unsigned removed[kSweepQueries][2];
    __shared__ __attribute__((aligned(16))) float slabs[MODEL == TRANSE ? 4 * 64 * kRefStride : 4];
    const int64_t Q = q_head + q_tail, q_base = (int64_t)blockIdx.x * kSweepQueries;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ const float* frow[kSweepQueries];  // the queries' two vectors: looked up once (indexed queries: a
    __shared__ const float* rrow[kSweepQueries];  // dependent load each), not once per filter entry
    if (threadIdx.x < 64) {
        const int64_t q = q_base + lane;
        frow[lane] = q_fixed.row(q < Q ? q : 0);
        rrow[lane] = q_rel.row(q < Q ? q : 0);
        int n = q < Q ? (int)(filter.hi[q] - filter.lo[q]) : 0;
        n = n > 0 ? n : 0;
        removed[lane][0] = removed[lane][1] = 0;
        if constexpr (SETS::on) {
            int64_t lo = 0, hi = 0;
            if (q < Q && n > 0) sets.set_of(q, q_head, lo, hi);
            set_lo[lane] = lo;
            set_hi[lane] = hi;
        }
        int incl = n;  // inclusive scan over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        prefix[lane + 1] = incl;
        if (lane == 0) prefix[0] = 0;
    }
    __syncthreads();
    const int total = prefix[kSweepQueries];
    auto locate = [&](int x, int64_t& q, int64_t& row, int& slot) {  // entry number x of this workgroup
        int lo = 0, hi = kSweepQueries;                                // largest slot with prefix[slot] <= x
#pragma unroll
        for (int step = 0; step < 6; ++step) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= x) lo = mid; else hi = mid;
        }
        slot = lo;
        q = q_base + slot;
        row = filter_row(filter, q, filter.lo[q] + (x - prefix[slot]), N);
        if constexpr (SETS::on)
            if (row >= 0 && !sets.contains(set_lo[slot], set_hi[slot], row + sets.row_base)) row = -1;
    };
    if constexpr (MODEL == TRANSE) {
        float* slab = slabs + wave * 64 * kRefStride;
        for (int x0 = wave * 64; x0 < total; x0 += 4 * 64) {  // wave-uniform
            const int x = x0 + lane;
            int64_t q = q_base < Q ? q_base : 0, row = -1;
            int slot = 0;
            if (x < total) locate(x, q, row, slot);
            const bool live = row >= 0, head = replaces_head(q, q_head, Q, batch);
            const float key = transe_key_64<D, TE>(table + (live ? row : 0) * ld, frow[slot], rrow[slot], head, slab, lane);
            const float kt = key_true[q];
            if (live && key > kt) atomicAdd(&removed[slot][0], 1u);
            if (live && key >= kt) atomicAdd(&removed[slot][1], 1u);
        }
    } else {
        const int half = lane >> 5, sub = lane & 31;
        for (int x0 = wave * 2; x0 < total; x0 += 4 * 2) {  // wave-uniform; each half-wave takes one entry
            const int x = x0 + half;
            int64_t q = q_base < Q ? q_base : 0, row = -1;
            int slot = 0;
            if (x < total) locate(x, q, row, slot);
            const bool live = row >= 0, head = replaces_head(q, q_head, Q, batch);
            const TE* e = table + (live ? row : 0) * ld;
            float key;
            if (head) key = coop_score<MODEL, HEAD, D>(e, frow[slot], rrow[slot], sub);
            else key = coop_score<MODEL, TAIL, D>(e, frow[slot], rrow[slot], sub);
            const float kt = key_true[q];
            if (sub == 0 && live && key > kt) atomicAdd(&removed[slot][0], 1u);
            if (sub == 0 && live && key >= kt) atomicAdd(&removed[slot][1], 1u);
        }
    }
    const unsigned long long a = sum_partials(acc, n_partials, Q, q_base, partial_sums);  // ends with a barrier
    if (threadIdx.x < 64 && q_base + lane < Q) {
        const int64_t q = q_base + lane;
        const int32_t all_gt = (int32_t)(a & 0xffffffffull), all_ge = (int32_t)(a >> 32);
        reinterpret_cast<int4*>(counts)[q] =
            make_int4(all_gt, all_ge, all_gt - (int32_t)removed[lane][0], all_ge - (int32_t)removed[lane][1]);
    }
}

}  // namespace blp
