// topk_sets_kernel.h -- the selection kernel of blp_topk_sets / blp_topk_sets_typed (topk_sets.hip has the description) as a
// template over the candidate table's storage type, and its launch.  Instantiated where it is launched: topk_sets.hip (f32
// tables) and topk_sets16.hip (IEEE half / bfloat16 tables).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "knobs.h"
#include "launch.h"
#include "rank_common.h"
#include "score_core.h"
#include "table_elem.h"
#include "tile.h"
#include "tile16.h"
#include "topk_lists.h"

#pragma clang fp contract(off)

namespace blp {

__device__ __forceinline__ int64_t topk_sets_uniform(int64_t v) {  // a wave-uniform value, into scalar registers
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((u64)v & 0xffffffffull));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((u64)v >> 32));
    return (int64_t)(((u64)hi << 32) | lo);
}

__host__ __device__ inline int64_t topk_sets_chunks(int64_t n_queries, int q_chunk) {
    return n_queries > 0 ? (n_queries + q_chunk - 1) / q_chunk : 0;
}
// slabs of a set of n > 0 entries
__host__ __device__ inline int64_t topk_sets_slabs_of(int64_t n, int s_max) {
    const int64_t tiles = (n + kTileRows - 1) / kTileRows;
    const int64_t s = (tiles + kTopkWaves - 1) / kTopkWaves;
    return s < 1 ? 1 : (s > s_max ? s_max : s);
}

// nq queries of one side, q0 .. (the call's numbering), against the wave's gathered tile; coef = the coefficient row of q0
template <int MODEL, int SIDE, int D>
__device__ __forceinline__ void topk_sets_side(const float (&e)[D], bool valid, int lrow, int64_t row_base, int64_t N,
                                               const float* __restrict__ coef, int64_t q0, int nq, u64* lists, int k,
                                               const FilterSpec& f, int lane) {
    using S = Scorer<MODEL, SIDE, D>;
    for (int j = 0; j < nq; ++j) {
        const float s = S::template score<false>(e, PtrCoef{coef + (int64_t)j * S::C});
        const u64 key = valid ? topk_key(s, row_base + lrow) : 0ull;
        list_offer(lists + j * k, k, key, lane, [&](u64 m) { return f.on() ? unfiltered_rows(f, q0 + j, N, lrow, m, lane) : m; });
    }
}

// TE: the candidate table's storage type (table_elem.h); ld in elements.  A 16-bit tile arrives through tile16.h: whole
// 128-byte lines of 64 columns, the 16-bit words through the slab, widened after the transpose into the same e[D].
template <int MODEL, int D, class TE = float>
__global__ __launch_bounds__(kTopkWaves * 64, (D == 256 ? 1 : 2)) void topk_sets_kernel(
    const TE* __restrict__ table, int64_t N, int64_t ld, const float* __restrict__ coef_head,
    const float* __restrict__ coef_tail, int64_t q_head, const SetLookup sets, const int64_t* __restrict__ prefix, int q_chunk,
    int s_max, int k, const FilterSpec filter, u64* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    float* slab = smem + wave * kSlabFloats;
    u64* lists_all = reinterpret_cast<u64*>(smem + kTopkWaves * kSlabFloats);
    u64* lists = lists_all + (size_t)wave * q_chunk * k;

    const int64_t G = sets.G, n_units = prefix[G];
    for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {  // workgroup-uniform
        int64_t g_lo = 0, g_hi = G;  // prefix[g_lo] <= unit < prefix[g_hi]: the last set that starts at or before the unit
        while (g_hi - g_lo > 1) {
            const int64_t mid = (g_lo + g_hi) >> 1;
            if (prefix[mid] <= unit) g_lo = mid; else g_hi = mid;
        }
        const int64_t g = topk_sets_uniform(g_lo);
        const int64_t p0 = sets.set_ptr[g], p1 = sets.set_ptr[g + 1];
        const int64_t h0 = sets.qptr_head[g], h1 = sets.qptr_head[g + 1], t0 = sets.qptr_tail[g], t1 = sets.qptr_tail[g + 1];
        const int64_t ch_head = topk_sets_chunks(h1 - h0, q_chunk), chunks = ch_head + topk_sets_chunks(t1 - t0, q_chunk);
        const int64_t n_tiles = (p1 - p0 + kTileRows - 1) / kTileRows;
        const int64_t n_slabs = topk_sets_slabs_of(p1 - p0, s_max);
        const int64_t local = unit - prefix[g], s = local / chunks, chunk = local - s * chunks;
        const bool head = chunk < ch_head;
        // the chunk's queries: [q0, q0 + nq) of the call, side query number s0 (its coefficient row)
        const int64_t s0 = topk_sets_uniform(head ? h0 + chunk * q_chunk : t0 + (chunk - ch_head) * q_chunk);
        const int64_t left = (head ? h1 : t1) - s0;
        const int nq = __builtin_amdgcn_readfirstlane((int)(left < q_chunk ? left : q_chunk));
        const int64_t q0 = head ? s0 : q_head + s0;

        for (int i = lane; i < nq * k; i += 64) lists[i] = 0ull;
        wave_lds_sync();

        for (int64_t t = s * kTopkWaves + wave; t < n_tiles; t += n_slabs * kTopkWaves) {
            // the wave's 64 entries of the set -> rows of this shard
            const int64_t p = topk_sets_uniform(p0 + t * kTileRows) + lane;
            const int64_t row = p < p1 ? sets.set_row[p] - sets.row_base : -1;
            const bool valid = (uint64_t)row < (uint64_t)N;
            const u64 vmask = __ballot(valid);
            if (!vmask) continue;
            int lrow = (int)row;  // N < 2^31
            if (!valid) lrow = __shfl(lrow, __builtin_ctzll(vmask));
            float e[D];
            const int sub_row = lane >> 3, sub_col = (lane & 7) * 4;
            if constexpr (std::is_same<TE, float>::value) {
                tile_fetch_from<D, false>(e, [&](auto ii) {
                    constexpr int i = decltype(ii)::value;
                    return table + (int64_t)__shfl(lrow, 8 * i + sub_row) * ld + sub_col;
                });
                tile_transpose<D>(e, slab, lane);
            } else {
                u32x4 w[D / 64][8];
                const char* bytes = reinterpret_cast<const char*>(table);
                tile16_fetch_from<D>(w, [&](auto ii) {
                    constexpr int i = decltype(ii)::value;
                    return bytes + (int64_t)__shfl(lrow, 8 * i + sub_row) * ld * 2 + sub_col * 4;
                });
                tile16_transpose_widen<D, TE>(e, w, slab, lane);
            }
            if (head)
                topk_sets_side<MODEL, HEAD, D>(e, valid, lrow, sets.row_base, N, coef_head + s0 * Scorer<MODEL, HEAD, D>::C, q0, nq,
                                               lists, k, filter, lane);
            else
                topk_sets_side<MODEL, TAIL, D>(e, valid, lrow, sets.row_base, N, coef_tail + s0 * Scorer<MODEL, TAIL, D>::C, q0, nq,
                                               lists, k, filter, lane);
        }

        __syncthreads();
        // fold the other waves' lists into wave 0's, query j by wave j % kTopkWaves; write the unit's list
        for (int j = wave; j < nq; j += kTopkWaves) {
            u64* L = lists_all + (size_t)j * k;
            for (int w = 1; w < kTopkWaves; ++w) {
                const u64* src = lists_all + ((size_t)w * q_chunk + j) * k;
                for (int c = 0; c < k; c += 64)
                    list_offer(L, k, c + lane < k ? src[c + lane] : 0ull, lane, [](u64 m) { return m; });
            }
            u64* out = partial + ((size_t)(q0 + j) * s_max + s) * k;
            for (int i = lane; i < k; i += 64) out[i] = L[i];
        }
        __syncthreads();  // the lists are zeroed again by their own waves only after every fold has read them
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct TopkSetsWorkspace {
    float* coef_head;
    float* coef_tail;
    int64_t* prefix;
    u64* partial;
    size_t partial_bytes;
    size_t bytes;
};

template <int MODEL, int D, class TE>
static hipError_t topk_sets_pass(const TE* table, int64_t N, int64_t ld, const TopkSetsWorkspace& w, int64_t q_head,
                                 const SetLookup& sets, int q_chunk, int s_max, int k, const FilterSpec& filter, int n_cu,
                                 hipStream_t stream) {
    // persistent workgroups, as many per compute unit as the kernel's registers and LDS let reside (knob topk_sets_grid: any
    // other number -- a query's keys are a set, the result does not depend on it)
    int64_t grid = (int64_t)(n_cu > 0 ? n_cu : 1) * (D == 256 ? 1 : 2);
    if (const long long forced = knob(KNOB_TOPK_SETS_GRID); forced > 0 && forced < (1ll << 20)) grid = forced;
    const size_t lds = (size_t)kTopkWaves * kSlabFloats * 4 + (size_t)kTopkWaves * q_chunk * k * 8;
    topk_sets_kernel<MODEL, D, TE><<<dim3((unsigned)grid), kTopkWaves * 64, lds, stream>>>(
        table, N, ld, w.coef_head, w.coef_tail, q_head, sets, w.prefix, q_chunk, s_max, k, filter, w.partial);
    return hipGetLastError();
}

// S_max, the partial lists per query, for chunks of q_chunk queries: n_slabs x (a lower bound of the chunks) <=
// max(chunks, kTopkTargetGroups), and at most one per kTopkWaves tiles of all the sets' entries together -- topk_slabs' rule
// (topk.hip) with nnz in N's place.  From Q, nnz and q_chunk alone: computed on the host.
inline int64_t topk_sets_slabs_rule(int64_t Q, int64_t nnz, int q_chunk) {
    const int64_t chunks = (Q + q_chunk - 1) / q_chunk;
    const int64_t tiles = (nnz + kTileRows - 1) / kTileRows;
    int64_t s = chunks > 0 ? kTopkTargetGroups / chunks : 1;
    const int64_t cap = (tiles + kTopkWaves - 1) / kTopkWaves;
    if (s > cap) s = cap;
    return s < 1 ? 1 : s;
}

// topk_sets.hip: topk_sets_unit_prefix_kernel's launch (one workgroup; G + 1 values into prefix), for topk_sets_wide.hip too
hipError_t launch_topk_sets_unit_prefix(const SetLookup& sets, int q_chunk, int s_max, int64_t* prefix, hipStream_t stream);

// topk_sets16.hip: the selection pass over a 16-bit table (dtype: kTableF16 / kTableBF16; ld in elements)
hipError_t launch_topk_sets_pass16(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, const TopkSetsWorkspace& w,
                                   int64_t q_head, const SetLookup& sets, int q_chunk, int s_max, int k, const FilterSpec& filter,
                                   int n_cu, hipStream_t stream);

}  // namespace blp
