// rank_rels_wide_bilinear.hip -- relation prediction for DistMult / ComplEx / SimplE at ANY width (include/blp_hip.h:
// blp_rank_relations_wide_bilinear, blp_topk_relations_wide_bilinear): D % 4 == 0, 4 <= D <= 1024 -- the BOW / DKRL encoders' 300
// and 768, where rank_rels.hip's layout (a lane holds a whole relation row in D VGPRs, one code object per width) does not fit.
// The contract is blp_rank_relations' / blp_topk_relations' word for word; 64 / 128 / 256 are taken too, as a second
// implementation of the same bits.
//
// Arithmetic: wide_bilinear.h's as it stands, with the RELATION row as the candidate row (WideTerm<MODEL, REL>: the candidate
// sits in the middle of the reference's expressions, nothing is hoisted; the staged "coefficients" are the pair's head and tail
// vectors as they are).  Eight lanes per relation row restate torch's sum(dim=-1) order, kAwRows rows of a group against the
// kAwQueries = 8 pairs of the workgroup's chunk; QRows{source, head_row, ld_src} serves as q_fixed, QRows{source, tail_row,
// ld_src} as q_rel.  A workgroup of kAwWaves waves owns a chunk, walks all R relation rows in trips of kAwBlockRows = 64 and
// strides over the chunks; the relation table (R x D floats: 237 x 768 x 4 = 0.7 MB) stays in cache.  Every query has exactly
// one owning workgroup: nothing depends on the grid, there are no global atomics.
//
// Kernels (D is a run-time argument; templates: the model, the cascade for >= 512 terms, the output form):
//   rel_true_key_wb   counts only: wide_pair_score<MODEL, REL> on rel_emb[true_rel[q]], eight lanes per query -- the number
//                     the pass gives that row, bit for bit; 4 Q bytes of workspace
//   rank_rels_wb      <COUNTS, SCORES>.  scores: lane r of a group stores row r's value.  counts: lane 0 of a group compares
//                     with the true key, the wave counts by ballot into scalar counters (rel_removed, rel_common.h, takes the
//                     filter's relations out of gt_filt / ge_filt); after the last trip the four waves add theirs into 32
//                     LDS counters that REUSE the head of the coefficient area behind a barrier (the coefficients alone fill
//                     64 KiB at D = 1024), one int4 store per query
//   topk_rels_wb      topk_wide.hip's selection: per (wave, query) a sorted list of k keys in LDS behind the coefficients
//                     (topk_lists.h), lane r of a group offers row r, the filter is looked up only for the lanes above the
//                     list's threshold (unfiltered_rows: a removed relation is dropped, never demoted), the four waves'
//                     lists are folded and the winners written straight from the keys.  There is no re-scoring launch: the
//                     pass's number is score_fn's bit for bit and the key carries it exactly, sign of zero included
//                     (topk_wide.hip's header gives the argument).  No workspace.
// Rows past R read row R - 1 and are masked everywhere.  Every lane of every wave calls wide_trip / wide_pair_score (the folds
// read neighbouring lanes by DPP); the trip loop's bound is workgroup-uniform in its count of barriers: none inside it.
//
// LDS: the coefficients, 8 x K x n4 floats (K n4 = 2 D for all three models: 64 KiB at D = 1024), in the top-k kernel followed
// by the lists, kAwWaves x 8 x k keys (64 KiB at k = 256) -- 128 KiB of the CU's 160 KiB at the two extremes together; above
// 64 KiB the launch raises the kernel's dynamic-LDS limit and returns a failure to do so, as topk_wide.hip does.  The rank
// kernel never needs more than 64 KiB.  No kernel of this file uses scratch memory: the [q][r] arrays are indexed by unrolled
// loops only.
//
// Grid: min(chunks, kRelMaxGroups = 1024) workgroups (rel_common.h's rule, as the other relation kernels): four per CU of the
// 256, at least what registers and LDS let be resident at once, so the stride evens out the chunks.  Not tuned: no other cap
// has been measured.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "rank_common.h"
#include "rel_common.h"
#include "score_core.h"
#include "topk_lists.h"
#include "wide_bilinear.h"

#pragma clang fp contract(off)

namespace blp {

namespace {

constexpr size_t kRwbDefaultLds = 64 << 10;  // dynamic LDS a kernel may use without raising its limit

template <int MODEL>
__global__ __launch_bounds__(256) void rel_true_key_wb_kernel(int D, const QRows q_head, const QRows q_tail, int64_t Q,
                                                              const float* __restrict__ rel_emb, const int64_t* __restrict__ true_rel,
                                                              float* __restrict__ key_true) {
    const int sub = threadIdx.x & 7;
    for (int64_t q0 = blockIdx.x * 32ll; q0 < Q; q0 += gridDim.x * 32ll) {  // workgroup-uniform
        const int64_t qq = q0 + (threadIdx.x >> 3), q = qq < Q ? qq : Q - 1;
        const float key = wide_pair_score<MODEL, REL>(rel_emb + true_rel[q] * D, q_head.row(q), q_tail.row(q), D, sub);
        if (sub == 0 && qq < Q) key_true[qq] = key;
    }
}

template <int MODEL, bool CASCADE, bool COUNTS, bool SCORES>
__global__ __launch_bounds__(kAwWaves * 64) void rank_rels_wb_kernel(const float* __restrict__ rel_emb, int64_t R, int D,
                                                                     const QRows q_head, const QRows q_tail, int64_t Q,
                                                                     const float* __restrict__ key_true, const FilterSpec filter,
                                                                     int32_t* __restrict__ counts, float* __restrict__ scores,
                                                                     int64_t ld_scores) {
    constexpr int QC = kAwQueries, NR = kAwRows;
    extern __shared__ __attribute__((aligned(16))) float rwb_coef[];  // [query of the chunk][K][n4]; then, reused, 4 QC counters
    unsigned* cnt = reinterpret_cast<unsigned*>(rwb_coef);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), grp = lane >> 3, sub = lane & 7;
    const int64_t n_chunks = (Q + QC - 1) / QC;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t q0 = chunk * QC;
        const int live_q = (int)(Q - q0 < QC ? Q - q0 : QC);
        __syncthreads();  // the previous chunk's coefficients (counters) have been read
        wide_stage_coef<MODEL, REL>(rwb_coef, q_head, q_tail, q0, live_q, D);
        __syncthreads();
        float kt[QC];
        unsigned cgt[QC], cge[QC], fgt[QC], fge[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) {
            kt[q] = COUNTS ? key_true[q0 + (q < live_q ? q : 0)] : 0.0f;
            cgt[q] = cge[q] = fgt[q] = fge[q] = 0;
        }

        for (int64_t rb = wave * (8 * NR); rb < R; rb += kAwBlockRows) {  // wave-uniform
            const float* base[NR];  // the group's rows (past R: the last row, masked)
            bool live[NR];
            int64_t row[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                row[r] = rb + grp + 8 * r;
                live[r] = row[r] < R;
                base[r] = rel_emb + (live[r] ? row[r] : R - 1) * D;
            }
            float s[QC][NR];
            wide_trip<MODEL, REL, CASCADE>(s, base, rwb_coef, D, sub);
#pragma unroll
            for (int q = 0; q < QC; ++q) {
                if (q < live_q) {  // workgroup-uniform
#pragma unroll
                    for (int r = 0; r < NR; ++r) {
                        if constexpr (SCORES) {
                            if (sub == r && live[r]) scores[(q0 + q) * ld_scores + row[r]] = s[q][r];
                        }
                        if constexpr (COUNTS) {
                            const bool mine = live[r] && sub == 0;  // lane 0 of a group compares with the true key
                            const bool gt = mine && s[q][r] > kt[q], ge = mine && s[q][r] >= kt[q];
                            const bool kept = !(filter.on() && rel_removed(filter, q0 + q, row[r]));
                            cgt[q] += (unsigned)__popcll(__ballot(gt));
                            cge[q] += (unsigned)__popcll(__ballot(ge));
                            fgt[q] += (unsigned)__popcll(__ballot(gt && kept));
                            fge[q] += (unsigned)__popcll(__ballot(ge && kept));
                        }
                    }
                }
            }
        }

        if constexpr (COUNTS) {
            __syncthreads();  // every wave is done with the coefficients: their first 4 QC words become the counters
            if (threadIdx.x < QC * 4) cnt[threadIdx.x] = 0u;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < QC; ++q) {
                if (lane < 4)  // ds_add_u32 without return, one instruction for the query's four counters
                    __hip_atomic_fetch_add(cnt + 4 * q + lane, lane == 0 ? cgt[q] : lane == 1 ? cge[q] : lane == 2 ? fgt[q] : fge[q],
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            __syncthreads();
            if ((int)threadIdx.x < live_q) {
                const int t = threadIdx.x;
                reinterpret_cast<int4*>(counts)[q0 + t] =
                    make_int4((int)cnt[4 * t], (int)cnt[4 * t + 1], (int)cnt[4 * t + 2], (int)cnt[4 * t + 3]);
            }
        }
    }
}

template <int MODEL, bool CASCADE>
__global__ __launch_bounds__(kAwWaves * 64) void topk_rels_wb_kernel(const float* __restrict__ rel_emb, int64_t R, int D,
                                                                     const QRows q_head, const QRows q_tail, int64_t Q, int k,
                                                                     const FilterSpec filter, int64_t* __restrict__ rels,
                                                                     float* __restrict__ scores) {
    using T = WideTerm<MODEL, REL>;
    constexpr int QC = kAwQueries, NR = kAwRows;
    extern __shared__ __attribute__((aligned(16))) float rwb_smem[];  // coefficients [query of the chunk][K][n4], then the lists
    const int n4 = wide_n4(MODEL, D);
    u64* lists_all = reinterpret_cast<u64*>(rwb_smem + QC * T::K * n4);  // [wave][query of the chunk][k]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), grp = lane >> 3, sub = lane & 7;
    u64* lists = lists_all + (size_t)wave * QC * k;
    const int64_t n_chunks = (Q + QC - 1) / QC;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t q0 = chunk * QC;
        const int live_q = (int)(Q - q0 < QC ? Q - q0 : QC);
        __syncthreads();  // the previous chunk's coefficients and lists have been read
        wide_stage_coef<MODEL, REL>(rwb_smem, q_head, q_tail, q0, live_q, D);
        for (int i = lane; i < live_q * k; i += 64) lists[i] = 0ull;
        __syncthreads();

        for (int64_t rb = wave * (8 * NR); rb < R; rb += kAwBlockRows) {  // wave-uniform
            const float* base[NR];  // the group's rows (past R: the last row, not offered)
            u64 slot = 0ull;        // lane r of the eight offers row r: its relation id + 1, 0 = nothing to offer
            int lrow = 0;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int64_t row = rb + grp + 8 * r;
                const bool live = row < R;
                base[r] = rel_emb + (live ? row : R - 1) * D;
                if (sub == r && live) {
                    slot = (u64)row + 1ull;
                    lrow = (int)row;  // R < 2^31
                }
            }
            float s[QC][NR];
            wide_trip<MODEL, REL, CASCADE>(s, base, rwb_smem, D, sub);
#pragma unroll
            for (int q = 0; q < QC; ++q) {
                if (q < live_q) {  // workgroup-uniform
                    float mine = s[q][0];
#pragma unroll
                    for (int r = 1; r < NR; ++r) mine = sub == r ? s[q][r] : mine;
                    const u64 key = slot ? topk_key(mine, (int64_t)(slot - 1ull)) : 0ull;
                    list_offer(lists + q * k, k, key, lane,
                               [&](u64 m) { return filter.on() ? unfiltered_rows(filter, q0 + q, R, lrow, m, lane) : m; });
                }
            }
        }

        __syncthreads();
        // fold the other waves' lists into wave 0's, query j by wave j % kAwWaves; write the query's result
        for (int j = wave; j < live_q; j += kAwWaves) {
            u64* L = lists_all + (size_t)j * k;
            for (int w = 1; w < kAwWaves; ++w) {
                const u64* src = lists_all + ((size_t)w * QC + j) * k;
                for (int c = 0; c < k; c += 64)
                    list_offer(L, k, c + lane < k ? src[c + lane] : 0ull, lane, [](u64 m) { return m; });
            }
            for (int i = lane; i < k; i += 64) {
                const u64 key = L[i];
                rels[(q0 + j) * k + i] = key_row(key);
                // (on the bits: key_score's NaN is 0x7fc00000, and a float store of it is the compiler's to canonicalise)
                reinterpret_cast<unsigned*>(scores)[(q0 + j) * k + i] = __float_as_uint(key_score(key));
            }
        }
    }
}

size_t coef_bytes(int model, int D) {
    const int K = model == DISTMULT ? 2 : 4;  // WideTerm<model, REL>::K
    return (size_t)kAwQueries * K * wide_n4(model, D) * sizeof(float);
}

template <int MODEL, bool CASCADE>
hipError_t rank_launch(int D, const QRows& qh, const QRows& qt, int64_t Q, const float* rel_emb, int64_t R, const float* key_true,
                       const FilterSpec& filter, int32_t* counts, float* scores, int64_t ld_scores, hipStream_t stream) {
    const dim3 grid(rel_grid((Q + kAwQueries - 1) / kAwQueries));
    const size_t lds = coef_bytes(MODEL, D);  // <= 64 KiB; >= 4 kAwQueries counters: K n4 >= 8 floats per query
    if (counts && scores)
        rank_rels_wb_kernel<MODEL, CASCADE, true, true><<<grid, kAwWaves * 64, lds, stream>>>(rel_emb, R, D, qh, qt, Q, key_true, filter, counts, scores, ld_scores);
    else if (counts)
        rank_rels_wb_kernel<MODEL, CASCADE, true, false><<<grid, kAwWaves * 64, lds, stream>>>(rel_emb, R, D, qh, qt, Q, key_true, filter, counts, nullptr, 0);
    else
        rank_rels_wb_kernel<MODEL, CASCADE, false, true><<<grid, kAwWaves * 64, lds, stream>>>(rel_emb, R, D, qh, qt, Q, nullptr, filter, nullptr, scores, ld_scores);
    return hipGetLastError();
}

template <int MODEL>
hipError_t rank_impl(int D, const QRows& qh, const QRows& qt, int64_t Q, const float* rel_emb, int64_t R, const int64_t* true_rel,
                     const FilterSpec& filter, int32_t* counts, float* scores, int64_t ld_scores, void* workspace, hipStream_t stream) {
    float* key_true = static_cast<float*>(workspace);
    if (counts) {
        const int64_t blocks = (Q + 31) / 32;
        rel_true_key_wb_kernel<MODEL><<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, stream>>>(D, qh, qt, Q, rel_emb, true_rel, key_true);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return wide_terms(MODEL, D) >= 512
               ? rank_launch<MODEL, true>(D, qh, qt, Q, rel_emb, R, key_true, filter, counts, scores, ld_scores, stream)
               : rank_launch<MODEL, false>(D, qh, qt, Q, rel_emb, R, key_true, filter, counts, scores, ld_scores, stream);
}

template <int MODEL>
hipError_t topk_impl(int D, const QRows& qh, const QRows& qt, int64_t Q, const float* rel_emb, int64_t R, int k, const FilterSpec& filter,
                     int64_t* rels, float* scores, hipStream_t stream) {
    const dim3 grid(rel_grid((Q + kAwQueries - 1) / kAwQueries));
    const size_t lds = coef_bytes(MODEL, D) + (size_t)kAwWaves * kAwQueries * k * sizeof(u64);
    auto launch = [&](auto kernel) {
        if (lds > kRwbDefaultLds) {
            const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (err != hipSuccess) return err;
        }
        kernel<<<grid, kAwWaves * 64, lds, stream>>>(rel_emb, R, D, qh, qt, Q, k, filter, rels, scores);
        return hipGetLastError();
    };
    return wide_terms(MODEL, D) >= 512 ? launch(topk_rels_wb_kernel<MODEL, true>) : launch(topk_rels_wb_kernel<MODEL, false>);
}

}  // namespace

bool rank_relations_wide_bilinear_supported(int model, int D) {
    return (model == DISTMULT || model == COMPLEX || model == SIMPLE) && D >= 4 && D <= kAwMaxD && D % 4 == 0;
}
bool topk_relations_wide_bilinear_supported(int model, int D, int k) {
    return rank_relations_wide_bilinear_supported(model, D) && k >= 1 && k <= kTopkMaxK;
}

hipError_t launch_rank_relations_wide_bilinear(int model, int D, const float* source, int64_t ld_src, const int64_t* head_row,
                                               const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R,
                                               const int64_t* true_rel, const FilterSpec& filter, int32_t* counts, float* scores,
                                               int64_t ld_scores, void* workspace, hipStream_t stream) {
    if (Q == 0) return hipSuccess;
    if (!rank_relations_wide_bilinear_supported(model, D)) return hipErrorInvalidValue;
    const QRows qh = QRows::rows_of(source, head_row, ld_src), qt = QRows::rows_of(source, tail_row, ld_src);
    if (model == DISTMULT) return rank_impl<DISTMULT>(D, qh, qt, Q, rel_emb, R, true_rel, filter, counts, scores, ld_scores, workspace, stream);
    if (model == COMPLEX) return rank_impl<COMPLEX>(D, qh, qt, Q, rel_emb, R, true_rel, filter, counts, scores, ld_scores, workspace, stream);
    return rank_impl<SIMPLE>(D, qh, qt, Q, rel_emb, R, true_rel, filter, counts, scores, ld_scores, workspace, stream);
}

hipError_t launch_topk_relations_wide_bilinear(int model, int D, const float* source, int64_t ld_src, const int64_t* head_row,
                                               const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R, int k,
                                               const FilterSpec& filter, int64_t* rels, float* scores, hipStream_t stream) {
    if (Q == 0) return hipSuccess;
    if (!topk_relations_wide_bilinear_supported(model, D, k)) return hipErrorInvalidValue;
    const QRows qh = QRows::rows_of(source, head_row, ld_src), qt = QRows::rows_of(source, tail_row, ld_src);
    if (model == DISTMULT) return topk_impl<DISTMULT>(D, qh, qt, Q, rel_emb, R, k, filter, rels, scores, stream);
    if (model == COMPLEX) return topk_impl<COMPLEX>(D, qh, qt, Q, rel_emb, R, k, filter, rels, scores, stream);
    return topk_impl<SIMPLE>(D, qh, qt, Q, rel_emb, R, k, filter, rels, scores, stream);
}

}  // namespace blp
