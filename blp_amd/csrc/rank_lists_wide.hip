// rank_lists_wide.hip -- rank and score queries against PER-QUERY candidate lists for DistMult / ComplEx / SimplE at ANY width
// (include/blp_hip.h: blp_rank_lists_wide): D % 4 == 0, 4 <= D <= 1024 -- the BOW / DKRL encoders' 300 and 768 --, an f32, f16
// or bf16 table.  The contract is blp_rank_lists' word for word (rank_lists.hip): query q owns entries [list_ptr[q],
// list_ptr[q + 1]) of list_row (int64 global rows, a multiset); an entry outside [row_base, row_base + N) is skipped -- it
// counts nowhere and its score slot holds exactly 0x7fc00000 --; counts (Q, 4) {gt, ge, gt_filt, ge_filt} against the true
// entity's key and / or scores (nnz,), score_fn's f32 value bit for bit, sign of zero included; the filter as blp_rank_all
// applies it (filter_row), a filter entry removing every copy of its row.  At 64 / 128 / 256 this is a second implementation
// of rank_lists.hip's bits.
//
// The arithmetic is wide_bilinear.h's: eight lanes per (entry, query) pair, lane `sub` owning accumulators 4 sub .. 4 sub + 3
// of torch's 32, the cascade at n >= 512, the leftover vectors of 8 in lanes 0 / 1, the n % 8 tail terms first, wide_fold.
// Every chain starts from +0.0f, so the argument of topk_wide.hip's header holds: the number is the reference's bit for bit.
//
// Kernels of one call (all on the caller's stream; the call zeroes counts first):
//   1. lists_wide_true_key   (only with counts) the true entities' keys, eight lanes per query, by wide_pair_score.
//   2. rank_lists_wide       rank_lists_kernel's structure: a workgroup owns kListsWideChunk consecutive ENTRIES of list_row
//                            whatever queries they belong to, finds the query of its first entry by a binary search in
//                            list_ptr, cuts each query's part into steps of 64 entries and deals the steps to its waves in
//                            turn.  The query's coefficients (WideTerm<>::coef: K arrays of n4 floats, at most 2 D floats)
//                            are staged once per (wave, query) in LDS, all of it dynamic.
//   A step: lane l holds entry l's row, range-checked as (uint64_t)row < (uint64_t)N before anything is addressed through it;
//   an invalid lane reads the row of the step's first valid lane, a step with no valid lane reads nothing.  The step runs as
//   eight sub-steps: in sub-step j group g (lanes 8 g .. 8 g + 7) scores entry 8 j + g, whose row pointer comes by a shuffle;
//   a sub-step none of whose eight entries is valid is skipped.  The score, valid in lanes 0 .. 3 of a group, goes back to
//   lane 8 j + g by one shuffle.  After the eight sub-steps the wave is in rank_lists_kernel's layout: a coalesced scores[p]
//   store, ballots against the true key, the filter looked up only for lanes that score >= the true key, one atomic add per
//   non-zero column and (wave, query) by lane 0: integer atomics onto zeroed counts, nothing depends on the grid.
//
// Rules:
//   - every lane of a wave reaches every fold (wide_fold's DPP row shifts read neighbouring lanes): invalid lanes score a
//     valid row and are masked afterwards, never branched around;
//   - the side (head / tail) is a property of the query, hence wave-uniform;
//   - the only early exits are wave-uniform (the query loop's, a skipped step, a skipped sub-step: ballots);
//   - row offsets are 64-bit: a table may exceed 2^31 bytes;
//   - #pragma clang fp contract(off) is in force: no FMA;
//   - no kernel uses scratch memory;
//   - D is a kernel argument: one code object per (model, element type, cascade) for both sides and every width.
// A 16-bit table (table_elem.h) is widened exactly as it is read; source and rel_emb stay f32.  Workspace: Q floats (the true
// keys), needed only with counts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "exact_coop.h"
#include "launch.h"
#include "rank_common.h"
#include "score_core.h"
#include "table_elem.h"
#include "wide_bilinear.h"

#pragma clang fp contract(off)

namespace blp {

namespace {

typedef unsigned long long u64;

constexpr int kListsWideChunk = 1024;  // entries of list_row per workgroup (16 steps of 64): rank_lists.hip's kListsChunk
constexpr int kListsWideWaves = 4;     // waves per workgroup

// floats of one wave's staged query: the larger K of the two sides
__host__ __device__ inline int lists_wide_coef_floats(int model, int D) {
    const int k = model == DISTMULT ? 2 : (model == COMPLEX ? 4 : 3);
    return k * wide_n4(model, D);
}

// True-entity keys, eight lanes per query (wide_bilinear_keys.h's kernel without the accumulators).
template <int MODEL>
__global__ __launch_bounds__(256) void lists_wide_true_key_kernel(int D, const QRows q_fixed, const QRows q_rel, const QRows q_true,
                                                                  int64_t q_head, int64_t Q, float* __restrict__ key_true) {
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
        if (sub == 0 && qq < Q) key_true[qq] = key;
    }
}

// The lanes of `mask` whose entry (table row `row` of the lane) query q's filter segment does NOT remove (rank_lists.hip's
// lists_unfiltered, restated with internal linkage).
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

template <int MODEL, class TE, bool CASCADE>
__global__ __launch_bounds__(kListsWideWaves * 64) void rank_lists_wide_kernel(
    const TE* __restrict__ table, int64_t N, int64_t ld, int64_t row_base, const QRows q_fixed, const QRows q_rel, int D,
    int64_t q_head, int64_t Q, const int64_t* __restrict__ list_ptr, const int64_t* __restrict__ list_row, int64_t nnz,
    const float* __restrict__ key_true, const FilterSpec filter, int32_t* __restrict__ counts, float* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) float lw_coef[];  // [wave][K][n4]
    const int lane = threadIdx.x & 63, grp = lane >> 3, sub = lane & 7;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int waves = kListsWideWaves;
    float* coef = lw_coef + wave * lists_wide_coef_floats(MODEL, D);

    const int64_t c_lo = (int64_t)blockIdx.x * kListsWideChunk, c_hi = c_lo + kListsWideChunk < nnz ? c_lo + kListsWideChunk : nnz;
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

        const bool head = q < q_head;  // wave-uniform: a property of the query
        const float kt = counts ? key_true[q] : 0.0f;
        wave_lds_sync();  // the previous query's reads are done before its coefficients are replaced
        if (head) wide_stage_coef_wave<MODEL, HEAD>(coef, q_fixed.row(q), q_rel.row(q), D, lane);
        else wide_stage_coef_wave<MODEL, TAIL>(coef, q_fixed.row(q), q_rel.row(q), D, lane);
        wave_lds_sync();

        unsigned gt = 0, ge = 0, gtf = 0, gef = 0;
        for (int i = first; i < n_steps; i += waves) {
            const int64_t p = a + 64 * (int64_t)i + lane;
            const bool live = p < b;
            const int64_t row = live ? list_row[p] - row_base : -1;
            const bool valid = (uint64_t)row < (uint64_t)N;
            const u64 vmask = __ballot(valid);
            float s = nan;
            if (vmask) {  // wave-uniform
                const int src = __builtin_ctzll(vmask);
                const int lrow = (int)row;  // N < 2^31
                const TE* pe = table + (int64_t)(valid ? lrow : __shfl(lrow, src)) * ld;
#pragma unroll 1
                for (int j = 0; j < 8; ++j) {
                    if (!((vmask >> (8 * j)) & 0xffull)) continue;  // wave-uniform: none of entries 8 j .. 8 j + 7 is valid
                    const TE* e = shfl_ptr(pe, 8 * j + grp);
                    const float v = head ? wide_pair_staged<MODEL, HEAD, CASCADE, TE>(e, coef, D, sub)
                                         : wide_pair_staged<MODEL, TAIL, CASCADE, TE>(e, coef, D, sub);
                    const float back = __shfl(v, 8 * sub);  // lane 8 j + g <- lane 0 of group g
                    if (grp == j) s = back;
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
template <int MODEL, class TE>
hipError_t rank_lists_wide_impl(const TE* table, int64_t N, int64_t ld, int64_t row_base, int D, const QRows& q_fixed,
                                const QRows& q_rel, const QRows& q_true, int64_t q_head, int64_t q_tail, const int64_t* list_ptr,
                                const int64_t* list_row, int64_t nnz, const FilterSpec& filter, int32_t* counts, float* scores,
                                void* workspace, hipStream_t stream) {
    const int64_t Q = q_head + q_tail;
    float* key_true = static_cast<float*>(workspace);
    if (counts) {
        hipError_t err = hipMemsetAsync(counts, 0, (size_t)Q * 16, stream);
        if (err != hipSuccess) return err;
        const int64_t key_blocks = (Q + 31) / 32;
        lists_wide_true_key_kernel<MODEL><<<(unsigned)(key_blocks < 65536 ? key_blocks : 65536), 256, 0, stream>>>(
            D, q_fixed, q_rel, q_true, q_head, Q, key_true);
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    if (nnz == 0) return hipSuccess;
    const size_t lds = (size_t)kListsWideWaves * lists_wide_coef_floats(MODEL, D) * sizeof(float);  // <= 32 KiB: K n4 <= 2048
    const unsigned grid = (unsigned)((nnz + kListsWideChunk - 1) / kListsWideChunk);
    if (wide_terms(MODEL, D) >= 512)
        rank_lists_wide_kernel<MODEL, TE, true><<<grid, kListsWideWaves * 64, lds, stream>>>(
            table, N, ld, row_base, q_fixed, q_rel, D, q_head, Q, list_ptr, list_row, nnz, key_true, filter, counts, scores);
    else
        rank_lists_wide_kernel<MODEL, TE, false><<<grid, kListsWideWaves * 64, lds, stream>>>(
            table, N, ld, row_base, q_fixed, q_rel, D, q_head, Q, list_ptr, list_row, nnz, key_true, filter, counts, scores);
    return hipGetLastError();
}

}  // namespace

bool rank_lists_wide_supported(int model, int dtype, int D) {
    if (dtype != kTableF32 && dtype != kTableF16 && dtype != kTableBF16) return false;
    return (model == DISTMULT || model == COMPLEX || model == SIMPLE) && D >= 4 && D <= kAwMaxD && D % 4 == 0;
}

size_t rank_lists_wide_workspace_bytes(int64_t q_head, int64_t q_tail) { return align_up((size_t)(q_head + q_tail) * 4, 256); }

hipError_t launch_rank_lists_wide(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, int64_t row_base,
                                  const QRows q_fixed, const QRows q_rel, const QRows q_true, int64_t q_head, int64_t q_tail,
                                  const int64_t* list_ptr, const int64_t* list_row, int64_t nnz, const FilterSpec& filter,
                                  int32_t* counts, float* scores, void* workspace, hipStream_t stream) {
#define BLP_LISTS_WIDE_TYPED(M, TT)                                                                                              \
    return rank_lists_wide_impl<M>(static_cast<const TT*>(table), N, ld, row_base, D, q_fixed, q_rel, q_true, q_head, q_tail,   \
                                   list_ptr, list_row, nnz, filter, counts, scores, workspace, stream);
#define BLP_LISTS_WIDE_MODEL(M)                                  \
    if (model == M) {                                            \
        if (dtype == kTableF32) BLP_LISTS_WIDE_TYPED(M, float)   \
        if (dtype == kTableF16) BLP_LISTS_WIDE_TYPED(M, _Float16) \
        if (dtype == kTableBF16) BLP_LISTS_WIDE_TYPED(M, __bf16) \
    }
    if (!rank_lists_wide_supported(model, dtype, D)) return hipErrorInvalidValue;
    BLP_LISTS_WIDE_MODEL(DISTMULT) BLP_LISTS_WIDE_MODEL(COMPLEX) BLP_LISTS_WIDE_MODEL(SIMPLE)
#undef BLP_LISTS_WIDE_MODEL
#undef BLP_LISTS_WIDE_TYPED
    return hipErrorInvalidValue;
}

}  // namespace blp
