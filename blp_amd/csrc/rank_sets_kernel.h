// rank_sets_kernel.h -- the ranking kernel of blp_rank_sets / blp_rank_sets_typed (rank_sets.hip has the description) as a template
// over the candidate table's storage type, and its launch.  Instantiated where it is launched: rank_sets.hip (f32 tables) and
// rank_sets16.hip (IEEE half / bfloat16 tables).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "knobs.h"
#include "launch.h"
#include "rank_common.h"
#include "rank_tiles.h"
#include "score_core.h"
#include "table_elem.h"
#include "tile.h"
#include "tile16.h"

#pragma clang fp contract(off)

namespace blp {

typedef unsigned long long u64;

__device__ __forceinline__ int64_t uniform64(int64_t v) {  // a wave-uniform value, into scalar registers
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((u64)v & 0xffffffffull));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((u64)v >> 32));
    return (int64_t)(((u64)hi << 32) | lo);
}

__host__ __device__ inline int64_t set_chunks(int64_t n_queries) { return n_queries > 0 ? (n_queries + kQueryChunk - 1) / kQueryChunk : 0; }

// TE: the candidate table's storage type (table_elem.h); ld in elements.  A 16-bit tile arrives through tile16.h: whole
// 128-byte lines of 64 columns, the 16-bit words through the slab, widened after the transpose into the same e[D].
template <int MODEL, int D, class TE = float>
__global__ __launch_bounds__(kWaves * 64, (D == 256 ? 1 : (MODEL == TRANSE ? 3 : 2))) void rank_sets_kernel(
    const TE* __restrict__ table, int64_t N, int64_t ld, const float* __restrict__ coef_head,
    const float* __restrict__ coef_tail, const float* __restrict__ key_true, int64_t q_head, const SetLookup sets,
    const int64_t* __restrict__ prefix, u64* __restrict__ acc) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    float* slab = smem + wave * kSlabFloats;
    float* cbuf = smem + kWaves * kSlabFloats;
    unsigned* cnt = reinterpret_cast<unsigned*>(cbuf + 2 * kQB * kMaxCoef(D)) + wave * (2 * kQueryChunk);

    for (int i = lane; i < 2 * kQueryChunk; i += 64) cnt[i] = 0;
    wave_lds_sync();

    const int64_t G = sets.G, n_units = prefix[G];
    for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        int64_t g_lo = 0, g_hi = G;  // prefix[g_lo] <= unit < prefix[g_hi]: the last set that starts at or before the unit
        while (g_hi - g_lo > 1) {
            const int64_t mid = (g_lo + g_hi) >> 1;
            if (prefix[mid] <= unit) g_lo = mid; else g_hi = mid;
        }
        const int64_t g = uniform64(g_lo);
        const int64_t p0 = sets.set_ptr[g], p1 = sets.set_ptr[g + 1];
        const int64_t h0 = sets.qptr_head[g], h1 = sets.qptr_head[g + 1], t0 = sets.qptr_tail[g], t1 = sets.qptr_tail[g + 1];
        const int64_t ch_head = set_chunks(h1 - h0), chunks = ch_head + set_chunks(t1 - t0);
        const int64_t local = unit - prefix[g], tile = local / chunks, chunk = local - tile * chunks;
        const bool head = chunk < ch_head;
        // the chunk's queries: [q0, q0 + nq) of the call, side query number s0 (its coefficient row)
        const int64_t s0 = uniform64(head ? h0 + chunk * kQueryChunk : t0 + (chunk - ch_head) * kQueryChunk);
        const int64_t left = (head ? h1 : t1) - s0;
        const int nq = __builtin_amdgcn_readfirstlane((int)(left < kQueryChunk ? left : kQueryChunk));
        const int64_t q0 = head ? s0 : q_head + s0;

        // the wave's 64 entries of the set -> rows of this shard
        const int64_t p = uniform64(p0 + (tile * kWaves + wave) * kTileRows) + lane;
        const int64_t row = p < p1 ? sets.set_row[p] - sets.row_base : -1;
        const bool valid = (uint64_t)row < (uint64_t)N;
        const u64 vmask = __ballot(valid);
        if (MODEL != TRANSE || vmask) {  // (the bilinear models' waves meet at apply_queries' barriers whatever they hold)
            int lrow = (int)row;  // N < 2^31
            if (!valid) lrow = vmask ? __shfl(lrow, __builtin_ctzll(vmask)) : 0;
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
            if constexpr (MODEL == TRANSE) {
                if (head)
                    score_batch_transe_sgpr<HEAD, D>(e, valid, coef_head + s0 * Scorer<TRANSE, HEAD, D>::C, nq, key_true + q0, cnt, wave, lane);
                else
                    score_batch_transe_sgpr<TAIL, D>(e, valid, coef_tail + s0 * Scorer<TRANSE, TAIL, D>::C, nq, key_true + q0, cnt, wave, lane);
            } else {
                if (head)
                    apply_queries<MODEL, HEAD, D>(e, valid, coef_head + s0 * Scorer<MODEL, HEAD, D>::C, key_true + q0, nq, cbuf, cnt, wave, lane);
                else
                    apply_queries<MODEL, TAIL, D>(e, valid, coef_tail + s0 * Scorer<MODEL, TAIL, D>::C, key_true + q0, nq, cbuf, cnt, wave, lane);
            }
            wave_lds_sync();
            for (int j = lane; j < nq; j += 64) {
                const u64 v = (u64)cnt[2 * j] | ((u64)cnt[2 * j + 1] << 32);
                if (v) {
                    atomicAdd(acc + q0 + j, v);
                    cnt[2 * j] = cnt[2 * j + 1] = 0;
                }
            }
            wave_lds_sync();
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct SetsWorkspace {
    float* key_true;
    u64* acc;
    float* coef_head;
    float* coef_tail;
    int64_t* prefix;
    size_t bytes;
};

template <int MODEL, int D, class TE>
static hipError_t rank_sets_pass(const TE* table, int64_t N, int64_t ld, const SetsWorkspace& w, int64_t q_head, const SetLookup& sets,
                                 int n_cu, hipStream_t stream) {
    // persistent workgroups, three per compute unit as rank_tiles' resident set (knob rank_sets_grid: any other number -- the
    // counts are integer sums over the units and do not depend on it)
    int64_t grid = (int64_t)(n_cu > 0 ? n_cu : 1) * 3;
    if (const long long forced = knob(KNOB_RANK_SETS_GRID); forced > 0 && forced < (1ll << 20)) grid = forced;
    const size_t lds = (size_t)kWaves * kSlabFloats * 4 + (size_t)2 * kQB * kMaxCoef(D) * 4 + (size_t)kWaves * 2 * kQueryChunk * 4;
    rank_sets_kernel<MODEL, D, TE><<<dim3((unsigned)grid), kWaves * 64, lds, stream>>>(table, N, ld, w.coef_head, w.coef_tail, w.key_true,
                                                                                   q_head, sets, w.prefix, w.acc);
    return hipGetLastError();
}

// rank_sets16.hip: the ranking pass and the filter + finalize step (launch_filter_finalize_sets, filter.on()) over a 16-bit
// table (dtype: kTableF16 / kTableBF16; ld in elements)
hipError_t launch_rank_sets_pass16(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, const SetsWorkspace& w,
                                   int64_t q_head, const SetLookup& sets, int n_cu, hipStream_t stream);
hipError_t launch_filter_finalize_sets16(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, const QRows q_fixed,
                                         const QRows q_rel, const float* key_true, int64_t q_head, int64_t q_tail,
                                         const FilterSpec& filter, const SetLookup& sets, const unsigned long long* acc,
                                         int32_t* counts, hipStream_t stream);

}  // namespace blp
