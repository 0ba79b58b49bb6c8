// rank_lists.hip -- rank and score link-prediction queries against PER-QUERY candidate lists (include/blp_hip.h:
// blp_rank_lists): query q owns entries [list_ptr[q], list_ptr[q + 1]) of list_row (int64 global table rows) -- the sampled
// negatives of an evaluation at Wikidata5M scale, the candidates of a first-stage retrieval, or any sparse set of (query,
// entity) pairs.  Only the listed rows are read: nnz x D elements instead of a pass over the table per four queries.
//
// Per query: counts {gt, ge, gt_filt, ge_filt} of the list's entries against the true entity's key (blp_rank_all's four
// columns, over the list instead of the table), and / or the score of every entry (score_fn's value bit for bit).
//
// Kernels of one call (all on the caller's stream):
//   1. lists_true_key  the true entities' keys, as rank_all.hip's true_key_kernel computes them (exact_coop.h).
//   2. rank_lists      a workgroup owns kListsChunk consecutive ENTRIES of list_row, whatever queries they belong to: it
//                      finds the query of its first entry by a binary search in list_ptr and walks on from there.  The
//                      part of a query's list inside the chunk is cut into steps of 64 entries, and the steps of the chunk
//                      are dealt to the workgroup's waves in turn.  A long list simply spans several workgroups; a
//                      workgroup adds its partial counts to counts[q] with integer atomics (the call zeroes counts first),
//                      so the result does not depend on the grid.
//   A step: lane l takes entry l.  A row outside [row_base, row_base + N) (-1 padding, another shard's row) is skipped: it
//   counts nowhere, its score is NaN; its lane reads the row of the step's first valid lane instead (nothing is read if no
//   lane is valid).  The query's two vectors are staged once per (wave, query) in LDS.
//     TransE (any D % 4 == 0, D <= 1024): transe_key_64_one_query_rt -- the 64 rows fetched in whole 128-byte lines, 32
//       columns at a time, transposed through a wave-private LDS slab; the L1 chain of a pair stays in one lane.
//     bilinear models (D = 64 / 128 / 256): 32 lanes per pair in torch.sum's order (exact_coop.h: coop_score, here with the
//       reference's literal "0 + first term" additions, Scorer<>::score<true>: the stored score carries the reference's
//       sign of zero; comparisons do not see it).  Half-wave h takes entries 32 h + i, i = 0 .. 31.
//   Filter: only entries that score at least the true key are looked up in the query's filter segment, 64 filter entries
//   per trip through filter_row (exclude, ent2idx, row_base as blp_rank_all applies them), one compare + ballot per
//   (admitted entry, trip) -- topk.hip's walk with the rows per lane.  A list is a multiset: a filter entry removes every
//   copy of its row.
// A 16-bit table (table_elem.h) is widened as its rows are read (exactly); source and rel_emb stay f32.
// No kernel uses scratch memory.  Workspace: Q floats (the true keys).
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

constexpr int kListsChunk = 1024;  // entries of list_row per workgroup (16 steps of 64)
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

// MODEL == TRANSE: D = 0, the width is the run-time Dr
template <int MODEL, int D>
__global__ __launch_bounds__(64) void lists_true_key_kernel(const QRows q_true, const QRows q_fixed, const QRows q_rel, int Dr,
                                                            int64_t q_head, int64_t Q, float* __restrict__ key_true) {
    constexpr int QB = MODEL == TRANSE ? 64 : 4;
    const int64_t q0 = blockIdx.x * (int64_t)QB;
    const int lane = threadIdx.x;
    if constexpr (MODEL == TRANSE) {
        __shared__ __attribute__((aligned(16))) float slab[64 * kRefStride];
        const int64_t q = q0 + lane < Q ? q0 + lane : Q - 1;
        const float key = transe_key_64_rt(q_true.row(q), q_fixed.row(q), q_rel.row(q), Dr, q < q_head, slab, lane);
        if (q0 + lane < Q) key_true[q] = key;
    } else {
        const int half = lane >> 5, sub = lane & 31;
        for (int i = 0; i < QB / 2; ++i) {  // wave-uniform
            const int64_t qq = q0 + 2 * i + half, q = qq < Q ? qq : Q - 1;
            const float* e = q_true.row(q);
            const float* f = q_fixed.row(q);
            const float* r = q_rel.row(q);
            const float key = q < q_head ? coop_score<MODEL, HEAD, D>(e, f, r, sub) : coop_score<MODEL, TAIL, D>(e, f, r, sub);
            if (sub == 0 && qq < Q) key_true[qq] = key;
        }
    }
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

template <int MODEL, int D, class TE>
__global__ __launch_bounds__(kListsWaves * 64) void rank_lists_kernel(
    const TE* __restrict__ table, int64_t N, int64_t ld, int64_t row_base, const QRows q_fixed, const QRows q_rel, int Dr,
    int64_t q_head, int64_t Q, const int64_t* __restrict__ list_ptr, const int64_t* __restrict__ list_row, int64_t nnz,
    const float* __restrict__ key_true, const FilterSpec filter, int32_t* __restrict__ counts, float* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves = blockDim.x >> 6;  // a power of two
    const int per_wave = 2 * Dr + (MODEL == TRANSE ? 64 * kRefStride : 0);
    float* qa = smem + wave * per_wave;
    float* qb = qa + Dr;
    float* slab = qb + Dr;
    (void)slab;

    const int64_t c_lo = (int64_t)blockIdx.x * kListsChunk, c_hi = c_lo + kListsChunk < nnz ? c_lo + kListsChunk : nnz;
    int64_t q_lo = 0, q_hi = Q;  // list_ptr[q_lo] <= c_lo < list_ptr[q_hi]: the query that owns entry c_lo
    while (q_hi - q_lo > 1) {
        const int64_t mid = (q_lo + q_hi) >> 1;
        if (list_ptr[mid] <= c_lo) q_lo = mid; else q_hi = mid;
    }
    const float nan = __uint_as_float(0x7fc00000u);
    int turn = 0;  // steps of the chunk dealt so far, modulo the number of waves
    for (int64_t q = q_lo; q < Q; ++q) {
        const int64_t p0 = list_ptr[q];
        if (p0 >= c_hi) break;
        const int64_t p1 = list_ptr[q + 1];
        const int64_t a = p0 > c_lo ? p0 : c_lo, b = p1 < c_hi ? p1 : c_hi;
        if (a >= b) continue;
        const int n_steps = (int)((b - a + 63) >> 6);
        const int first = (wave - turn) & (waves - 1);
        turn = (turn + n_steps) & (waves - 1);
        if (first >= n_steps) continue;

        const bool head = q < q_head;
        const float kt = counts ? key_true[q] : 0.0f;
        wave_lds_sync();  // the previous query's reads are done before its vectors are replaced
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
        wave_lds_sync();

        unsigned gt = 0, ge = 0, gtf = 0, gef = 0;
        for (int i = first; i < n_steps; i += waves) {
            const int64_t p = a + 64 * (int64_t)i + lane;
            const bool live = p < b;
            const int64_t row = live ? list_row[p] - row_base : -1;
            const bool valid = (uint64_t)row < (uint64_t)N;
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
            if (scores && live) scores[p] = s;
            if (counts) {
                u64 gem = __ballot(valid && s >= kt), gtm = __ballot(valid && s > kt);
                ge += __popcll(gem);
                gt += __popcll(gtm);
                if (filter.on() && gem) {
                    const u64 keep = lists_unfiltered(filter, q, N, (int)row, gem, lane);
                    gem &= keep;
                    gtm &= keep;
                }
                gef += __popcll(gem);
                gtf += __popcll(gtm);
            }
        }
        if (counts && lane == 0) {
            int32_t* c = counts + 4 * q;
            if (gt) atomicAdd(c + 0, (int32_t)gt);
            if (ge) atomicAdd(c + 1, (int32_t)ge);
            if (gtf) atomicAdd(c + 2, (int32_t)gtf);
            if (gef) atomicAdd(c + 3, (int32_t)gef);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool rank_lists_supported(int model, int dtype, int D) {
    if (dtype != kTableF32 && dtype != kTableF16 && dtype != kTableBF16) return false;
    if (model == TRANSE) return D >= 4 && D % 4 == 0 && D <= 1024;
    return model >= DISTMULT && model <= SIMPLE && (D == 64 || D == 128 || D == 256);
}

size_t rank_lists_workspace_bytes(int64_t q_head, int64_t q_tail) { return align_up((size_t)(q_head + q_tail) * 4, 256); }

template <int MODEL, int D, class TE>
static hipError_t rank_lists_impl(const TE* table, int64_t N, int64_t ld, int64_t row_base, int Dr, const QRows& q_fixed,
                                  const QRows& q_rel, const QRows& q_true, int64_t q_head, int64_t q_tail, const int64_t* list_ptr,
                                  const int64_t* list_row, int64_t nnz, const FilterSpec& filter, int32_t* counts, float* scores,
                                  void* workspace, hipStream_t stream) {
    const int64_t Q = q_head + q_tail;
    float* key_true = static_cast<float*>(workspace);
    if (counts) {
        hipError_t err = hipMemsetAsync(counts, 0, (size_t)Q * 16, stream);
        if (err != hipSuccess) return err;
        constexpr int QB = MODEL == TRANSE ? 64 : 4;
        lists_true_key_kernel<MODEL, D><<<(unsigned)((Q + QB - 1) / QB), 64, 0, stream>>>(q_true, q_fixed, q_rel, Dr, q_head, Q,
                                                                                          key_true);
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    if (nnz == 0) return hipSuccess;
    const int waves = MODEL == TRANSE && Dr > kListsWideFrom ? kListsWaves / 2 : kListsWaves;
    const size_t lds = (size_t)waves * (2 * Dr + (MODEL == TRANSE ? 64 * kRefStride : 0)) * 4;
    const unsigned grid = (unsigned)((nnz + kListsChunk - 1) / kListsChunk);
    rank_lists_kernel<MODEL, D, TE><<<grid, waves * 64, lds, stream>>>(table, N, ld, row_base, q_fixed, q_rel, Dr, q_head, Q, list_ptr,
                                                                        list_row, nnz, key_true, filter, counts, scores);
    return hipGetLastError();
}

hipError_t launch_rank_lists(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, int64_t row_base,
                             const QRows q_fixed, const QRows q_rel, const QRows q_true, int64_t q_head, int64_t q_tail,
                             const int64_t* list_ptr, const int64_t* list_row, int64_t nnz, const FilterSpec& filter, int32_t* counts,
                             float* scores, void* workspace, hipStream_t stream) {
#define BLP_LISTS_TYPED(M, DD, TT)                                                                                              \
    return rank_lists_impl<M, DD>(static_cast<const TT*>(table), N, ld, row_base, D, q_fixed, q_rel, q_true, q_head, q_tail,    \
                                  list_ptr, list_row, nnz, filter, counts, scores, workspace, stream);
#define BLP_LISTS_CASE(M, DD)                                        \
    {                                                                \
        if (dtype == kTableF32) BLP_LISTS_TYPED(M, DD, float)        \
        if (dtype == kTableF16) BLP_LISTS_TYPED(M, DD, _Float16)     \
        if (dtype == kTableBF16) BLP_LISTS_TYPED(M, DD, __bf16)      \
        return hipErrorInvalidValue;                                 \
    }
#define BLP_LISTS_MODEL(M)                        \
    if (model == M && D == 64) BLP_LISTS_CASE(M, 64)   \
    if (model == M && D == 128) BLP_LISTS_CASE(M, 128) \
    if (model == M && D == 256) BLP_LISTS_CASE(M, 256)
    if (!rank_lists_supported(model, dtype, D)) return hipErrorInvalidValue;
    if (model == TRANSE) BLP_LISTS_CASE(TRANSE, 0)
    BLP_LISTS_MODEL(DISTMULT) BLP_LISTS_MODEL(COMPLEX) BLP_LISTS_MODEL(SIMPLE)
#undef BLP_LISTS_MODEL
#undef BLP_LISTS_CASE
#undef BLP_LISTS_TYPED
    return hipErrorInvalidValue;
}

}  // namespace blp
