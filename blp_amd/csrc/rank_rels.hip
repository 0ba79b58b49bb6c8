// rank_rels.hip -- relation prediction (include/blp_hip.h: blp_rank_relations, blp_topk_relations): for a pair (h, ?, t) the
// score_fn value (models.py:222-248) of every row of rel_emb, as rank counts against the true relation, as the (Q, R) score
// matrix, or as the k best relations -- without scoring through memory.
//
// Layout: rank_tiles' (rank_tiles.h) with the roles swapped.  The CANDIDATES are the R rows of rel_emb: a wave holds a tile of
// 64 of them, one row per lane, in D VGPRs (tile.h); the QUERIES stream: query q's two vectors, rows head_row[q] and
// tail_row[q] of `source`, are wave-uniform, fetched by scalar loads and used as SGPR operands (rel_scorer.h: one per VALU
// instruction in every expression).  A workgroup of four waves owns a chunk of queries and walks the relation table in groups
// of 4 x 64 rows; with R <= 256 there is one group, the tiles are loaded once and stay in registers while the workgroup
// strides over its chunks.  Lanes past R are masked: they count nowhere, are never admitted, never written.
//
// Kernels:
//   rel_true_key     counts only: the true triple's score, score_direct on (h, t, rel_emb[true_rel]) -- 4 Q bytes of workspace
//   rank_rels        per (tile, query) the score; scores: one contiguous 64-float store; counts: compare with the true key,
//                    ballot, popcount, added to the workgroup's LDS counters (integer adds), stored once per chunk -- every
//                    query has exactly one owner, so nothing depends on the grid
//   topk_rels        per (wave, query) an LDS list of the best k keys (topk_lists.h), folded over the four waves at the end
//                    of the chunk and written as rels / scores: no partial lists, no merge launch, no workspace
//   topk_rels_rescore  the winners re-scored by RelScorer<>::score<true> (the keys hold -0 == +0; the output carries the
//                    reference's sign of zero)
// Filter: the lane's relation is tested against the query's segment in the kernel (a wave-uniform walk of the segment: the
// known relations of one pair are a handful), so filtered relations leave the last two counts / are never offered to a list.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "rank_common.h"
#include "rel_common.h"
#include "rel_scorer.h"
#include "score_core.h"
#include "score_direct.h"
#include "tile.h"
#include "topk_lists.h"

#pragma clang fp contract(off)

namespace blp {

constexpr int kRelChunk = 64;          // queries per workgroup pass of rank_rels: 4 counters each = one per thread

// (D a template parameter: score_direct's sums then run from registers -- its run-time-width routine keeps them in scratch)
template <int MODEL, int D>
__global__ __launch_bounds__(256) void rel_true_key_kernel(REL_QUERY_PARAMS, int64_t Q, const float* __restrict__ rel_emb,
                                                           const int64_t* __restrict__ true_rel, float* __restrict__ key_true) {
    const RelQueries qs{source, ld_src, head_row, tail_row};
    const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (q >= Q) return;
    key_true[q] = score_direct<MODEL>(qs.head(q), qs.tail(q), rel_emb + true_rel[q] * D, D);
}

// The wave's tile of group g: rows 64 (4 g + wave) .. of rel_emb; (re)loaded unless it is the one already held.
template <int D>
__device__ __forceinline__ void take_tile(float (&e)[D], bool& have, bool single, const float* __restrict__ rel_emb, int64_t R,
                                          int64_t tile, float* slab, int lane) {
    if (have && single) return;
    load_tile<D, false>(e, rel_emb, R, D, tile * kTileRows, slab, lane);
    have = true;
}

template <int MODEL, int D, bool COUNTS, bool SCORES>
__global__ __launch_bounds__(kWaves * 64, (D == 256 ? 1 : 2)) void rank_rels_kernel(
    REL_QUERY_PARAMS, int64_t Q, const float* __restrict__ rel_emb, int64_t R, const float* __restrict__ key_true,
    const FilterSpec filter, int32_t* __restrict__ counts, float* __restrict__ scores, int64_t ld_scores) {
    const RelQueries qs{source, ld_src, head_row, tail_row};
    __shared__ __attribute__((aligned(16))) float slabs[kWaves * kSlabFloats];
    __shared__ unsigned cnt[kRelChunk * 4];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int64_t n_tiles = (R + kTileRows - 1) / kTileRows, n_groups = (n_tiles + kWaves - 1) / kWaves;
    const int64_t n_chunks = (Q + kRelChunk - 1) / kRelChunk;
    using S = RelScorer<MODEL, D>;

    float e[D];
    bool have = false;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t qa = chunk * kRelChunk;
        const int nq = (int)(Q - qa < kRelChunk ? Q - qa : kRelChunk);
        if constexpr (COUNTS) {
            __syncthreads();  // the previous chunk's counters have been stored
            cnt[tid] = 0u;
            __syncthreads();
        }
        for (int64_t g = 0; g < n_groups; ++g) {
            const int64_t tile = g * kWaves + wave;
            if (tile >= n_tiles) continue;
            take_tile<D>(e, have, n_groups == 1, rel_emb, R, tile, slabs + wave * kSlabFloats, lane);
            const int64_t rel = tile * kTileRows + lane;
            const bool valid = rel < R;
            for (int j = 0; j < nq; ++j) {
                const int64_t q = qa + j;
                const PtrCoef h{qs.head(q)}, t{qs.tail(q)};
                // with the scores written the value must be the reference's, sign of zero included; for the comparisons
                // alone the shorter form does (-0 == +0)
                const float s = S::template score<SCORES>(e, h, t);
                if constexpr (SCORES) {
                    if (valid) scores[q * ld_scores + rel] = s;
                }
                if constexpr (COUNTS) {
                    const float kt = key_true[q];
                    const bool kept = valid && !(filter.on() && rel_removed(filter, q, rel));
                    const unsigned gt = __popcll(__ballot(valid && s > kt)), ge = __popcll(__ballot(valid && s >= kt));
                    const unsigned fgt = __popcll(__ballot(kept && s > kt)), fge = __popcll(__ballot(kept && s >= kt));
                    if (lane < 4)  // ds_add_u32 without return, one instruction for the four counters
                        __hip_atomic_fetch_add(cnt + 4 * j + lane, lane == 0 ? gt : lane == 1 ? ge : lane == 2 ? fgt : fge,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        if constexpr (COUNTS) {
            __syncthreads();
            if (tid < nq * 4) counts[qa * 4 + tid] = (int32_t)cnt[tid];
        }
    }
}

template <int MODEL, int D>
__global__ __launch_bounds__(kTopkWaves * 64, (D == 256 ? 1 : 2)) void topk_rels_kernel(
    REL_QUERY_PARAMS, int64_t Q, const float* __restrict__ rel_emb, int64_t R, int q_chunk, int k, const FilterSpec filter,
    int64_t* __restrict__ rels, float* __restrict__ scores) {
    const RelQueries qs{source, ld_src, head_row, tail_row};
    extern __shared__ __attribute__((aligned(16))) float smem[];
    static_assert(kTopkWaves == kWaves, "one tile per wave of a group");
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    u64* lists_all = reinterpret_cast<u64*>(smem + kWaves * kSlabFloats);
    u64* lists = lists_all + (size_t)wave * q_chunk * k;
    const int64_t n_tiles = (R + kTileRows - 1) / kTileRows, n_groups = (n_tiles + kWaves - 1) / kWaves;
    const int64_t n_chunks = (Q + q_chunk - 1) / q_chunk;
    using S = RelScorer<MODEL, D>;

    float e[D];
    bool have = false;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t qa = chunk * q_chunk;
        const int nq = (int)(Q - qa < q_chunk ? Q - qa : q_chunk);
        __syncthreads();  // the previous chunk's fold has read every wave's lists
        for (int i = lane; i < nq * k; i += 64) lists[i] = 0ull;
        wave_lds_sync();
        for (int64_t g = 0; g < n_groups; ++g) {
            const int64_t tile = g * kWaves + wave;
            if (tile >= n_tiles) continue;
            take_tile<D>(e, have, n_groups == 1, rel_emb, R, tile, smem + wave * kSlabFloats, lane);
            const int64_t rel = tile * kTileRows + lane;
            const bool valid = rel < R;
            for (int j = 0; j < nq; ++j) {
                const int64_t q = qa + j;
                const PtrCoef h{qs.head(q)}, t{qs.tail(q)};
                const float s = S::template score<false>(e, h, t);
                const bool kept = valid && !(filter.on() && rel_removed(filter, q, rel));  // removed before admission
                list_offer(lists + j * k, k, kept ? topk_key(s, rel) : 0ull, lane, [](u64 m) { return m; });
            }
        }
        __syncthreads();
        // fold the other waves' lists into wave 0's, query j by wave j % kWaves; write the query's result
        for (int j = wave; j < nq; j += kWaves) {
            u64* L = lists_all + (size_t)j * k;
            for (int w = 1; w < kWaves; ++w) {
                const u64* src = lists_all + ((size_t)w * q_chunk + j) * k;
                for (int c = 0; c < k; c += 64)
                    list_offer(L, k, c + lane < k ? src[c + lane] : 0ull, lane, [](u64 m) { return m; });
            }
            for (int i = lane; i < k; i += 64) {
                const u64 key = L[i];
                rels[(qa + j) * k + i] = key_row(key);
                scores[(qa + j) * k + i] = key_score(key);
            }
        }
    }
}

// One lane per output slot: RelScorer<>::score<true> of the selected relation from the query's own vectors -- score_fn's
// value bit for bit.  Empty slots keep their NaN.  (One lane per slot, the relation row read from memory: k x Q slots are few
// next to the R x Q pairs of the selection.)
template <int MODEL, int D>
__global__ __launch_bounds__(64) void topk_rels_rescore_kernel(REL_QUERY_PARAMS, int64_t Q, const float* __restrict__ rel_emb, int k,
                                                               const int64_t* __restrict__ rels, float* __restrict__ scores) {
    const RelQueries qs{source, ld_src, head_row, tail_row};
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= Q * k) return;
    const int64_t r = rels[i];
    if (r < 0) return;
    const int64_t q = i / k;
    float e[D];
    load_row<D>(e, rel_emb + r * D);
    const float s = RelScorer<MODEL, D>::template score<true>(e, PtrCoef{qs.head(q)}, PtrCoef{qs.tail(q)});
    // every NaN leaves as the quiet NaN 0x7fc00000, whatever its sign and payload (TransE's negation sets the sign) -- on the
    // bits: a floating-point select between two NaNs is the compiler's to fold away
    const unsigned bits = __float_as_uint(s);
    reinterpret_cast<unsigned*>(scores)[i] = (bits & 0x7fffffffu) > 0x7f800000u ? 0x7fc00000u : bits;
}

// ------------------------------------------------------------------------------------------------ host side
bool rank_relations_supported(int model, int D) {
    return model >= TRANSE && model <= SIMPLE && (D == 64 || D == 128 || D == 256);
}
bool topk_relations_supported(int model, int D, int k) { return rank_relations_supported(model, D) && k >= 1 && k <= kTopkMaxK; }

// the true keys, one float per query (used with counts only)
size_t rank_relations_workspace_bytes(int64_t Q) { return align_up((size_t)Q * 4, 256); }

template <int MODEL, int D>
static hipError_t rank_rels_impl(const RelQueries& qs, int64_t Q, const float* rel_emb, int64_t R, const int64_t* true_rel,
                                 const FilterSpec& filter, int32_t* counts, float* scores, int64_t ld_scores, void* workspace,
                                 hipStream_t stream) {
    float* key_true = static_cast<float*>(workspace);
    if (counts) {
        rel_true_key_kernel<MODEL, D><<<dim3((unsigned)((Q + 255) / 256)), 256, 0, stream>>>(REL_QUERY_ARGS(qs), Q, rel_emb, true_rel, key_true);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    const dim3 grid(rel_grid((Q + kRelChunk - 1) / kRelChunk));
    if (counts && scores)
        rank_rels_kernel<MODEL, D, true, true><<<grid, kWaves * 64, 0, stream>>>(REL_QUERY_ARGS(qs), Q, rel_emb, R, key_true, filter, counts, scores, ld_scores);
    else if (counts)
        rank_rels_kernel<MODEL, D, true, false><<<grid, kWaves * 64, 0, stream>>>(REL_QUERY_ARGS(qs), Q, rel_emb, R, key_true, filter, counts, nullptr, 0);
    else
        rank_rels_kernel<MODEL, D, false, true><<<grid, kWaves * 64, 0, stream>>>(REL_QUERY_ARGS(qs), Q, rel_emb, R, nullptr, filter, nullptr, scores, ld_scores);
    return hipGetLastError();
}

template <int MODEL, int D>
static hipError_t topk_rels_impl(const RelQueries& qs, int64_t Q, const float* rel_emb, int64_t R, int k, const FilterSpec& filter,
                                 int64_t* rels, float* scores, hipStream_t stream) {
    const int q_chunk = topk_chunk(k);
    const size_t lds = (size_t)kWaves * kSlabFloats * 4 + (size_t)kWaves * q_chunk * k * 8;
    topk_rels_kernel<MODEL, D><<<dim3(rel_grid((Q + q_chunk - 1) / q_chunk)), kWaves * 64, lds, stream>>>(REL_QUERY_ARGS(qs), Q, rel_emb, R, q_chunk, k,
                                                                                                         filter, rels, scores);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const int64_t slots = Q * k;
    topk_rels_rescore_kernel<MODEL, D><<<dim3((unsigned)((slots + 63) / 64)), 64, 0, stream>>>(REL_QUERY_ARGS(qs), Q, rel_emb, k, rels, scores);
    return hipGetLastError();
}

#define BLP_REL_MODEL(M) BLP_REL_CASE(M, 64) BLP_REL_CASE(M, 128) BLP_REL_CASE(M, 256)
#define BLP_REL_ALL BLP_REL_MODEL(TRANSE) BLP_REL_MODEL(DISTMULT) BLP_REL_MODEL(COMPLEX) BLP_REL_MODEL(SIMPLE)

hipError_t launch_rank_relations(int model, int D, const float* source, int64_t ld_src, const int64_t* head_row, const int64_t* tail_row,
                                 int64_t Q, const float* rel_emb, int64_t R, const int64_t* true_rel, const FilterSpec& filter,
                                 int32_t* counts, float* scores, int64_t ld_scores, void* workspace, hipStream_t stream) {
    if (Q == 0) return hipSuccess;
    const RelQueries qs{source, ld_src, head_row, tail_row};
#define BLP_REL_CASE(M, DD) \
    if (model == M && D == DD) return rank_rels_impl<M, DD>(qs, Q, rel_emb, R, true_rel, filter, counts, scores, ld_scores, workspace, stream);
    BLP_REL_ALL
#undef BLP_REL_CASE
    return hipErrorInvalidValue;
}

hipError_t launch_topk_relations(int model, int D, const float* source, int64_t ld_src, const int64_t* head_row, const int64_t* tail_row,
                                 int64_t Q, const float* rel_emb, int64_t R, int k, const FilterSpec& filter, int64_t* rels, float* scores,
                                 hipStream_t stream) {
    if (Q == 0) return hipSuccess;
    const RelQueries qs{source, ld_src, head_row, tail_row};
#define BLP_REL_CASE(M, DD) \
    if (model == M && D == DD) return topk_rels_impl<M, DD>(qs, Q, rel_emb, R, k, filter, rels, scores, stream);
    BLP_REL_ALL
#undef BLP_REL_CASE
    return hipErrorInvalidValue;
}

#undef BLP_REL_ALL
#undef BLP_REL_MODEL

}  // namespace blp
