// lists_topk.hip -- filtered, deterministic top-k inside PER-QUERY candidate lists (include/blp_hip.h: blp_topk_lists): query
// q owns entries [list_ptr[q], list_ptr[q + 1]) of list_row (int64 global table rows), as in rank_lists.hip; the call returns
// the k entries of each list with the highest score_fn value, the rows a filter names removed.  Only the listed rows are
// read, the selection stays in LDS, and (Q, k) rows / scores are all that is written.
//
// Order: topk.hip's 64-bit keys (topk_lists.h) -- descending score by IEEE comparison (-0 == +0), ties by ascending row, NaN
// after every number, key 0 = an empty slot.  A list is a multiset: every valid entry competes, the copies of a row carry the
// same key and come out in adjacent slots.  A query's result is the multiset of its k largest keys, whatever the grid.
//
// Kernels of one call (all on the caller's stream):
//   1. topk_lists   UNIT = one wave = (query q, slab s), unit = q x S + s; a workgroup is kListsWaves (TransE wider than
//                   kListsWideFrom: half as many) consecutive units, with no barrier and no fold between its waves.  The wave
//                   stages its query's two vectors in LDS, takes steps s, s + S, ... of the query's list (lists_step.h: 64
//                   entries, one exact score per lane -- the value that is stored, so nothing is re-scored), makes
//                   topk_key(score, global row) (a skipped lane: key 0) and offers the keys to its sorted list of k keys in LDS
//                   (list_offer).  The filter walk is the drop callback: only lanes above the list's threshold are looked up.
//                   S == 1: the wave decodes its list into rows / scores.  S > 1: it writes slot (q, s) of the (Q, S, k) key
//                   buffer in the workspace (a slab without steps: empty keys).
//   2. topk_merge   (topk.hip: launch_topk_merge_keys), S > 1 only: the k best of a query's S lists -> rows / scores.
// S is computed on the host from Q and nnz alone (topk_lists_slabs): 1 once the queries alone give kTopkListsTargetWaves
// waves; otherwise enough slabs to reach that, at most one per kListsWaves steps of the MEAN list, at most kTopkListsMaxSlabs.
// Lists of very different lengths are therefore imbalanced (a long list among short ones gets the mean's slabs), not wrong.
// LDS of a wave: the two query vectors, the TransE transpose slab, k keys.  No kernel uses scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "lists_step.h"
#include "rank_common.h"
#include "score_core.h"
#include "table_elem.h"
#include "topk_lists.h"

#pragma clang fp contract(off)

namespace blp {

constexpr int kTopkListsTargetWaves = 2048;  // units (waves) that fill the machine: 256 compute units x 8
constexpr int kTopkListsMaxSlabs = 256;

// slabs per query (1: no key buffer, no merge)
static int64_t topk_lists_slabs(int64_t Q, int64_t nnz) {
    if (Q <= 0 || Q >= kTopkListsTargetWaves) return 1;
    const int64_t by_queries = (kTopkListsTargetWaves + Q - 1) / Q;
    const int64_t mean_steps = (nnz + 64 * Q - 1) / (64 * Q);
    int64_t by_steps = (mean_steps + kListsWaves - 1) / kListsWaves;
    if (by_steps < 1) by_steps = 1;
    int64_t s = by_queries < by_steps ? by_queries : by_steps;
    return s > kTopkListsMaxSlabs ? kTopkListsMaxSlabs : s;
}

// floats of LDS per wave: qa, qb, the TransE slab, k keys (rounded so that the next wave's vectors stay 16-byte aligned)
__host__ __device__ inline int topk_lists_wave_floats(bool transe, int Dr, int k) {
    return 2 * Dr + (transe ? 64 * kRefStride : 0) + 2 * ((k + 1) & ~1);
}

template <int MODEL, int D, class TE>
__global__ __launch_bounds__(kListsWaves * 64) void topk_lists_kernel(
    const TE* __restrict__ table, int64_t N, int64_t ld, int64_t row_base, const QRows q_fixed, const QRows q_rel, int Dr,
    int64_t q_head, int64_t Q, const int64_t* __restrict__ list_ptr, const int64_t* __restrict__ list_row, int n_slabs, int k,
    const FilterSpec filter, u64* __restrict__ partial, int64_t* __restrict__ rows, float* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves = blockDim.x >> 6;
    float* qa = smem + wave * topk_lists_wave_floats(MODEL == TRANSE, Dr, k);
    float* qb = qa + Dr;
    float* slab = qb + Dr;
    u64* L = reinterpret_cast<u64*>(slab + (MODEL == TRANSE ? 64 * kRefStride : 0));

    // the wave's unit (wave-uniform: list_ptr and the query's rows are read through scalar loads)
    const int64_t unit = (int64_t)blockIdx.x * waves + wave;
    int64_t q = unit;
    int s = 0;
    if (n_slabs > 1) {  // Q x n_slabs < 2^31 (Q < kTopkListsTargetWaves)
        q = (int)unit / n_slabs;
        s = (int)unit - (int)q * n_slabs;
    }
    if (q >= Q) return;  // no barrier in this kernel: a wave may leave

    for (int i = lane; i < k; i += 64) L[i] = 0ull;
    const int64_t p0 = list_ptr[q], p1 = list_ptr[q + 1];
    const int n_steps = (int)((p1 - p0 + 63) >> 6);  // nnz < 2^31
    if (s < n_steps) {
        const bool head = q < q_head;
        lists_stage_query<MODEL, D>(q_fixed, q_rel, q, Dr, head, qa, qb, lane);
        wave_lds_sync();
        for (int i = s; i < n_steps; i += n_slabs) {
            const int64_t p = p0 + 64 * (int64_t)i + lane;
            int64_t row;
            bool valid;
            const float v = lists_step<MODEL, D, TE>(table, N, ld, row_base, list_row, p, p < p1, qa, qb, Dr, head, slab, lane, row, valid);
            const u64 key = valid ? topk_key(v, row_base + row) : 0ull;
            list_offer(L, k, key, lane, [&](u64 m) { return filter.on() ? lists_unfiltered(filter, q, N, (int)row, m, lane) : m; });
        }
    }
    wave_lds_sync();
    if (n_slabs == 1) {
        for (int i = lane; i < k; i += 64) {
            const u64 key = L[i];
            rows[q * k + i] = key_row(key);
            scores[q * k + i] = key_score(key);
        }
    } else {
        u64* out = partial + ((size_t)q * n_slabs + s) * k;
        for (int i = lane; i < k; i += 64) out[i] = L[i];
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool topk_lists_supported(int model, int dtype, int D, int k) {
    return rank_lists_supported(model, dtype, D) && k >= 1 && k <= kTopkMaxK;
}

size_t topk_lists_workspace_bytes(int64_t q_head, int64_t q_tail, int64_t nnz, int k) {
    const int64_t Q = q_head + q_tail, S = topk_lists_slabs(Q, nnz);
    return S > 1 ? align_up((size_t)Q * S * k * 8, 256) : 0;
}

template <int MODEL, int D, class TE>
static hipError_t topk_lists_impl(const TE* table, int64_t N, int64_t ld, int64_t row_base, int Dr, const QRows& q_fixed,
                                  const QRows& q_rel, int64_t q_head, int64_t q_tail, const int64_t* list_ptr,
                                  const int64_t* list_row, int64_t nnz, int k, const FilterSpec& filter, int64_t* rows, float* scores,
                                  void* workspace, hipStream_t stream) {
    const int64_t Q = q_head + q_tail;
    if (Q == 0) return hipSuccess;
    const int64_t S = topk_lists_slabs(Q, nnz);
    const int waves = MODEL == TRANSE && Dr > kListsWideFrom ? kListsWaves / 2 : kListsWaves;
    const size_t lds = (size_t)waves * topk_lists_wave_floats(MODEL == TRANSE, Dr, k) * 4;
    const int64_t units = Q * S;
    const unsigned grid = (unsigned)((units + waves - 1) / waves);
    u64* partial = S > 1 ? static_cast<u64*>(workspace) : nullptr;
    topk_lists_kernel<MODEL, D, TE><<<grid, waves * 64, lds, stream>>>(table, N, ld, row_base, q_fixed, q_rel, Dr, q_head, Q, list_ptr,
                                                                        list_row, (int)S, k, filter, partial, rows, scores);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || S == 1) return err;
    return launch_topk_merge_keys(partial, Q, S * k, k, rows, scores, stream);
}

hipError_t launch_topk_lists(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, int64_t row_base,
                             const QRows q_fixed, const QRows q_rel, int64_t q_head, int64_t q_tail, const int64_t* list_ptr,
                             const int64_t* list_row, int64_t nnz, int k, const FilterSpec& filter, int64_t* rows, float* scores,
                             void* workspace, hipStream_t stream) {
#define BLP_TOPK_LISTS_TYPED(M, DD, TT)                                                                                          \
    return topk_lists_impl<M, DD>(static_cast<const TT*>(table), N, ld, row_base, D, q_fixed, q_rel, q_head, q_tail, list_ptr,   \
                                  list_row, nnz, k, filter, rows, scores, workspace, stream);
#define BLP_TOPK_LISTS_CASE(M, DD)                                     \
    {                                                                  \
        if (dtype == kTableF32) BLP_TOPK_LISTS_TYPED(M, DD, float)     \
        if (dtype == kTableF16) BLP_TOPK_LISTS_TYPED(M, DD, _Float16)  \
        if (dtype == kTableBF16) BLP_TOPK_LISTS_TYPED(M, DD, __bf16)   \
        return hipErrorInvalidValue;                                   \
    }
#define BLP_TOPK_LISTS_MODEL(M)                              \
    if (model == M && D == 64) BLP_TOPK_LISTS_CASE(M, 64)    \
    if (model == M && D == 128) BLP_TOPK_LISTS_CASE(M, 128)  \
    if (model == M && D == 256) BLP_TOPK_LISTS_CASE(M, 256)
    if (!topk_lists_supported(model, dtype, D, k)) return hipErrorInvalidValue;
    if (model == TRANSE) BLP_TOPK_LISTS_CASE(TRANSE, 0)
    BLP_TOPK_LISTS_MODEL(DISTMULT) BLP_TOPK_LISTS_MODEL(COMPLEX) BLP_TOPK_LISTS_MODEL(SIMPLE)
#undef BLP_TOPK_LISTS_MODEL
#undef BLP_TOPK_LISTS_CASE
#undef BLP_TOPK_LISTS_TYPED
    return hipErrorInvalidValue;
}

}  // namespace blp
