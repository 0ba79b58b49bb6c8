// rank_rels_wide.hip -- relation prediction for TransE at ANY width (include/blp_hip.h: blp_rank_relations_wide,
// blp_topk_relations_wide): D % 4 == 0, 4 <= D <= 1024 -- the BOW / DKRL encoders' 300 and 768, where rank_rels.hip's layout (a
// lane holds a whole relation row in D VGPRs) does not fit.
//
// Layout: rank_rels.hip's with the resident operand inverted.  A wave still owns a tile of 64 relations, one per lane, but holds
// only a SLAB of kWideCols = 64 columns of the row in VGPRs at a time (tile.h: coalesced 16-byte loads transposed through the
// wave's LDS slab); what stays resident across the slabs is one f32 accumulator per query of the workgroup's chunk of
// kWideChunk = 16 queries.  For each slab, for each query of the chunk, the chain
//     acc = acc + |(h[d] + e[d]) - t[d]|
// continues over the slab's columns in ascending d, h and t wave-uniform (scalar loads, one SGPR operand per VALU instruction).
// TransE's sum is strictly left to right (score_direct.h), so the accumulator carried from slab to slab is the reference's
// running sum at every column and -acc after the last one is score_fn's value bit for bit; every chain starts from a literal
// 0.0f, so an all-zero sum leaves as -0.0 like the reference's.  The last slab of a row may be partial (300 = 4 x 64 + 44):
// the columns left are taken in pieces of 32 / 16 / 8 / 4 read straight from the lane's row.  The chunk loop is fully unrolled:
// the accumulators are never dynamically indexed, nothing lives in scratch.
//
// Kernels (one code object for every width: D is a run-time argument):
//   rel_true_key_wide   counts only: the true triple's score, score_direct<TRANSE> on (h, t, rel_emb[true_rel]) at run-time
//                       width -- 4 Q bytes of workspace
//   rank_rels_wide      per (tile, chunk) the 16 scores; scores: contiguous 64-float stores; counts: compare with the true key,
//                       ballot, popcount, added to the workgroup's LDS counters, stored once per chunk -- every query has exactly
//                       one owning workgroup, so nothing depends on the grid and there are no global atomics
//   topk_rels_wide      per (wave, query) an LDS list of the best k keys (topk_lists.h), folded over the four waves at the end
//                       of the chunk.  The score offered IS the reference's value (sign of zero included: the key keeps it), so
//                       the winners are written straight from the keys, NaN as 0x7fc00000: no re-scoring launch, no workspace
// Filter: rel_common.h's rel_removed, as in rank_rels.hip.  Lanes past R are masked everywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "rank_common.h"
#include "rel_common.h"
#include "score_core.h"
#include "score_direct.h"
#include "tile.h"
#include "topk_lists.h"

#pragma clang fp contract(off)

namespace blp {

constexpr int kWideCols = 64;     // columns of its relation row a lane holds at a time
constexpr int kWideChunk = 16;    // queries per workgroup pass: one accumulator per lane each
constexpr int kWideMaxD = 1024;

static_assert(kWideCols % kSubCols == 0, "a slab is whole LDS passes of load_tile");
static_assert(kWideChunk * 4 <= kWaves * 64, "one thread per counter");

__global__ __launch_bounds__(256) void rel_true_key_wide_kernel(REL_QUERY_PARAMS, int D, int64_t Q, const float* __restrict__ rel_emb,
                                                                const int64_t* __restrict__ true_rel, float* __restrict__ key_true) {
    const RelQueries qs{source, ld_src, head_row, tail_row};
    const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (q >= Q) return;
    key_true[q] = score_direct<TRANSE>(qs.head(q), qs.tail(q), rel_emb + true_rel[q] * D, D);
}

// One query's chain over the W columns e[] = columns [col, col + W) of the lane's row; h, t: the query's vectors at column
// `col` (wave-uniform).  The differences run kPipe columns ahead of the dependent adds, as in RelScorer<TRANSE>.
template <int W>
__device__ __forceinline__ float transe_slab(float acc, const float (&e)[W], const float* __restrict__ h, const float* __restrict__ t) {
    constexpr int P = W < kPipe ? W : kPipe;
    float x[P];
    static_for<P>([&](auto k) {
        constexpr int d = decltype(k)::value;
        const float y = h[d] + e[d];
        x[d] = y - t[d];
    });
    static_for<W>([&](auto k) {
        constexpr int d = decltype(k)::value;
        const float cur = fabsf(x[d % P]);
        if constexpr (d + P < W) {
            const float y = h[d + P] + e[d + P];
            x[d % P] = y - t[d + P];
        }
        acc = acc + cur;
    });
    return acc;
}

// The chunk's nq <= kWideChunk chains, each continued over the slab (fully unrolled: acc[] stays in registers).
template <int W>
__device__ __forceinline__ void chunk_step(float (&acc)[kWideChunk], const float (&e)[W], const RelQueries& qs, int64_t qa, int nq,
                                           int col) {
    static_for<kWideChunk>([&](auto jj) {
        constexpr int j = decltype(jj)::value;
        if (j < nq) acc[j] = transe_slab<W>(acc[j], e, qs.head(qa + j) + col, qs.tail(qa + j) + col);
    });
}

// W < kWideCols columns left at the end of a row: read from the lane's own row (16-byte loads)
template <int W>
__device__ __forceinline__ void tail_step(float (&acc)[kWideChunk], const float* __restrict__ row, const RelQueries& qs, int64_t qa,
                                          int nq, int D, int& col) {
    if (!(D & W)) return;
    float e[W];
    load_row<W>(e, row + col);
    chunk_step<W>(acc, e, qs, qa, nq, col);
    col += W;
}

// acc[j] = sum over all D columns of |(h_j + e) - t_j| for the lane's relation (row 64 tile + lane of rel_emb, clamped to the
// last row: the caller masks lanes past R) and the nq queries from qa on.
__device__ __forceinline__ void chunk_sums(float (&acc)[kWideChunk], const RelQueries& qs, int64_t qa, int nq, int D,
                                           const float* __restrict__ rel_emb, int64_t R, int64_t tile, float* slab, int lane) {
    static_for<kWideChunk>([&](auto jj) { acc[decltype(jj)::value] = 0.0f; });
    const int64_t row0 = tile * kTileRows;
    const int n_full = D / kWideCols;
    for (int s = 0; s < n_full; ++s) {
        float e[kWideCols];
        wave_lds_sync();  // the previous slab's reads of the LDS slab are done before it is rewritten
        load_tile<kWideCols, false>(e, rel_emb + s * kWideCols, R, D, row0, slab, lane);
        chunk_step<kWideCols>(acc, e, qs, qa, nq, s * kWideCols);
    }
    int col = n_full * kWideCols;
    const int64_t r = row0 + lane < R ? row0 + lane : R - 1;
    const float* row = rel_emb + r * D;
    tail_step<32>(acc, row, qs, qa, nq, D, col);
    tail_step<16>(acc, row, qs, qa, nq, D, col);
    tail_step<8>(acc, row, qs, qa, nq, D, col);
    tail_step<4>(acc, row, qs, qa, nq, D, col);
}

template <bool COUNTS, bool SCORES>
__global__ __launch_bounds__(kWaves * 64, 2) void rank_rels_wide_kernel(
    REL_QUERY_PARAMS, int D, int64_t Q, const float* __restrict__ rel_emb, int64_t R, const float* __restrict__ key_true,
    const FilterSpec filter, int32_t* __restrict__ counts, float* __restrict__ scores, int64_t ld_scores) {
    const RelQueries qs{source, ld_src, head_row, tail_row};
    __shared__ __attribute__((aligned(16))) float slabs[kWaves * kSlabFloats];
    __shared__ unsigned cnt[kWideChunk * 4];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int64_t n_tiles = (R + kTileRows - 1) / kTileRows, n_groups = (n_tiles + kWaves - 1) / kWaves;
    const int64_t n_chunks = (Q + kWideChunk - 1) / kWideChunk;

    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t qa = chunk * kWideChunk;
        const int nq = (int)(Q - qa < kWideChunk ? Q - qa : kWideChunk);
        if constexpr (COUNTS) {
            __syncthreads();  // the previous chunk's counters have been stored
            if (tid < kWideChunk * 4) cnt[tid] = 0u;
            __syncthreads();
        }
        for (int64_t g = 0; g < n_groups; ++g) {
            const int64_t tile = g * kWaves + wave;
            if (tile >= n_tiles) continue;
            float acc[kWideChunk];
            chunk_sums(acc, qs, qa, nq, D, rel_emb, R, tile, slabs + wave * kSlabFloats, lane);
            const int64_t rel = tile * kTileRows + lane;
            const bool valid = rel < R;
            static_for<kWideChunk>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                if (j < nq) {
                    const int64_t q = qa + j;
                    const float s = -acc[j];
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
            });
        }
        if constexpr (COUNTS) {
            __syncthreads();
            if (tid < nq * 4) counts[qa * 4 + tid] = (int32_t)cnt[tid];
        }
    }
}

// q_chunk <= kWideChunk queries per pass: what the lists' LDS holds at this k (topk_lists.h: topk_chunk)
__global__ __launch_bounds__(kTopkWaves * 64, 2) void topk_rels_wide_kernel(
    REL_QUERY_PARAMS, int D, int64_t Q, const float* __restrict__ rel_emb, int64_t R, int q_chunk, int k, const FilterSpec filter,
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

    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t qa = chunk * q_chunk;
        const int nq = (int)(Q - qa < q_chunk ? Q - qa : q_chunk);
        __syncthreads();  // the previous chunk's fold has read every wave's lists
        for (int i = lane; i < nq * k; i += 64) lists[i] = 0ull;
        wave_lds_sync();
        for (int64_t g = 0; g < n_groups; ++g) {
            const int64_t tile = g * kWaves + wave;
            if (tile >= n_tiles) continue;
            float acc[kWideChunk];
            chunk_sums(acc, qs, qa, nq, D, rel_emb, R, tile, smem + wave * kSlabFloats, lane);
            const int64_t rel = tile * kTileRows + lane;
            const bool valid = rel < R;
            static_for<kWideChunk>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                if (j < nq) {
                    const bool kept = valid && !(filter.on() && rel_removed(filter, qa + j, rel));  // removed before admission
                    list_offer(lists + j * k, k, kept ? topk_key(-acc[j], rel) : 0ull, lane, [](u64 m) { return m; });
                }
            });
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
                // (on the bits: key_score's NaN is 0x7fc00000, and a float store of it is the compiler's to canonicalise)
                reinterpret_cast<unsigned*>(scores)[(qa + j) * k + i] = __float_as_uint(key_score(key));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool rank_relations_wide_supported(int model, int D) { return model == TRANSE && D >= 4 && D <= kWideMaxD && D % 4 == 0; }
bool topk_relations_wide_supported(int model, int D, int k) {
    return rank_relations_wide_supported(model, D) && k >= 1 && k <= kTopkMaxK;
}

static int wide_topk_chunk(int k) {
    const int c = topk_chunk(k);
    return c < kWideChunk ? c : kWideChunk;
}

hipError_t launch_rank_relations_wide(int model, int D, const float* source, int64_t ld_src, const int64_t* head_row,
                                      const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R, const int64_t* true_rel,
                                      const FilterSpec& filter, int32_t* counts, float* scores, int64_t ld_scores, void* workspace,
                                      hipStream_t stream) {
    if (Q == 0) return hipSuccess;
    if (!rank_relations_wide_supported(model, D)) return hipErrorInvalidValue;
    const RelQueries qs{source, ld_src, head_row, tail_row};
    float* key_true = static_cast<float*>(workspace);
    if (counts) {
        rel_true_key_wide_kernel<<<dim3((unsigned)((Q + 255) / 256)), 256, 0, stream>>>(REL_QUERY_ARGS(qs), D, Q, rel_emb, true_rel, key_true);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    const dim3 grid(rel_grid((Q + kWideChunk - 1) / kWideChunk));
    if (counts && scores)
        rank_rels_wide_kernel<true, true><<<grid, kWaves * 64, 0, stream>>>(REL_QUERY_ARGS(qs), D, Q, rel_emb, R, key_true, filter, counts, scores, ld_scores);
    else if (counts)
        rank_rels_wide_kernel<true, false><<<grid, kWaves * 64, 0, stream>>>(REL_QUERY_ARGS(qs), D, Q, rel_emb, R, key_true, filter, counts, nullptr, 0);
    else
        rank_rels_wide_kernel<false, true><<<grid, kWaves * 64, 0, stream>>>(REL_QUERY_ARGS(qs), D, Q, rel_emb, R, nullptr, filter, nullptr, scores, ld_scores);
    return hipGetLastError();
}

hipError_t launch_topk_relations_wide(int model, int D, const float* source, int64_t ld_src, const int64_t* head_row,
                                      const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R, int k, const FilterSpec& filter,
                                      int64_t* rels, float* scores, hipStream_t stream) {
    if (Q == 0) return hipSuccess;
    if (!topk_relations_wide_supported(model, D, k)) return hipErrorInvalidValue;
    const RelQueries qs{source, ld_src, head_row, tail_row};
    const int q_chunk = wide_topk_chunk(k);
    const size_t lds = (size_t)kWaves * kSlabFloats * 4 + (size_t)kWaves * q_chunk * k * 8;
    topk_rels_wide_kernel<<<dim3(rel_grid((Q + q_chunk - 1) / q_chunk)), kWaves * 64, lds, stream>>>(REL_QUERY_ARGS(qs), D, Q, rel_emb, R, q_chunk, k,
                                                                                                   filter, rels, scores);
    return hipGetLastError();
}

}  // namespace blp
