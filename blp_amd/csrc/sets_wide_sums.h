// sets_wide_sums.h -- TransE's running sums at RUN-TIME width for a wave's 64 gathered set rows and a chunk of up to 16 queries
// of one side: the arithmetic half of rank_sets_wide.hip (counts inside shared candidate sets) and of topk_sets_wide.hip (top-k
// inside them).  rank_sets_wide.hip's header has the description of the layout: a lane holds a slab of kSetsWideCols = 64
// columns of its row at a time, what stays resident across the slabs is one f32 running sum per query of the chunk, the
// coefficient rows are wave-uniform (scalar loads), the last columns of a row go in pieces of 32 / 16 / 8 / 4.  -acc after the
// last column is the reference's score_fn value bit for bit.  Nothing here is dynamically indexed: no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rank_common.h"
#include "score_core.h"
#include "table_elem.h"
#include "tile.h"
#include "tile16.h"

#pragma clang fp contract(off)

namespace blp {

typedef unsigned long long u64;

constexpr int kSetsWideCols = 64;    // columns of its set row a lane holds at a time
constexpr int kSetsWideChunk = 16;   // queries per work unit: one running sum per lane each
constexpr int kSetsWideMaxD = 1024;

static_assert(kSetsWideCols == 64, "a slab is one 128-byte line of a 16-bit row, two LDS passes of an f32 row");

__device__ __forceinline__ int64_t wide_uniform64(int64_t v) {  // a wave-uniform value, into scalar registers
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((u64)v & 0xffffffffull));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((u64)v >> 32));
    return (int64_t)(((u64)hi << 32) | lo);
}

// One query's chain over the W columns e[]; c: the query's coefficient row at the slab's first column (wave-uniform).  The
// differences run kPipe columns ahead of the dependent adds, as in Scorer<TRANSE, *, D>.
template <int SIDE, int d, int W>
__device__ __forceinline__ float sets_wide_diff(const float (&e)[W], const float* __restrict__ c, int D) {
    if constexpr (SIDE == TAIL) {
        return c[d] - e[d];  // (h + r) - e, h + r hoisted
    } else {
        const float y = e[d] + c[d];  // (e + r) - t
        return y - c[D + d];
    }
}

template <int SIDE, int W>
__device__ __forceinline__ float sets_wide_slab(float acc, const float (&e)[W], const float* __restrict__ c, int D) {
    constexpr int P = W < kPipe ? W : kPipe;
    float x[P];
    static_for<P>([&](auto k) {
        constexpr int d = decltype(k)::value;
        x[d] = sets_wide_diff<SIDE, d>(e, c, D);
    });
    static_for<W>([&](auto k) {
        constexpr int d = decltype(k)::value;
        const float cur = fabsf(x[d % P]);
        if constexpr (d + P < W) x[d % P] = sets_wide_diff<SIDE, d + P>(e, c, D);
        acc = acc + cur;
    });
    return acc;
}

// The chunk's nq <= kSetsWideChunk chains, each continued over the slab (fully unrolled: acc[] stays in registers).  coef: the
// first query's coefficient row at column `col`; C floats per query.
template <int SIDE, int W>
__device__ __forceinline__ void sets_wide_step(float (&acc)[kSetsWideChunk], const float (&e)[W], const float* __restrict__ coef, int nq,
                                               int D) {
    const int C = SIDE == TAIL ? D : 2 * D;
    static_for<kSetsWideChunk>([&](auto jj) {
        constexpr int j = decltype(jj)::value;
        if (j < nq) acc[j] = sets_wide_slab<SIDE, W>(acc[j], e, coef + (int64_t)j * C, D);
    });
}

// W < kSetsWideCols columns left at the end of a row: read from the lane's own row
template <int SIDE, int W, class TE>
__device__ __forceinline__ void sets_wide_tail(float (&acc)[kSetsWideChunk], const TE* __restrict__ row, const float* __restrict__ coef,
                                               int nq, int D, int& col) {
    if (!(D & W)) return;
    float e[W];
    static_for<W / 4>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        const float4 v = load4<TE>(row + col + 4 * k);  // (a 16-bit row: widened here, exactly)
        e[4 * k] = v.x; e[4 * k + 1] = v.y; e[4 * k + 2] = v.z; e[4 * k + 3] = v.w;
    });
    sets_wide_step<SIDE, W>(acc, e, coef + col, nq, D);
    col += W;
}

// acc[j] = sum over all D columns for the lane's row (row lrow of the table; every lane passes a row inside the table) and the
// nq queries whose coefficient rows start at coef.
template <int SIDE, class TE>
__device__ __forceinline__ void sets_wide_sums(float (&acc)[kSetsWideChunk], const TE* __restrict__ table, int64_t ld, int lrow,
                                               const float* __restrict__ coef, int nq, int D, float* slab, int lane) {
    static_for<kSetsWideChunk>([&](auto jj) { acc[decltype(jj)::value] = 0.0f; });
    const int sub_row = lane >> 3, sub_col = (lane & 7) * 4;
    const int n_full = D / kSetsWideCols;
    for (int s = 0; s < n_full; ++s) {
        float e[kSetsWideCols];
        wave_lds_sync();  // the previous slab's reads of the LDS slab are done before it is rewritten
        if constexpr (std::is_same<TE, float>::value) {
            tile_fetch_from<kSetsWideCols, false>(e, [&](auto ii) {
                constexpr int i = decltype(ii)::value;
                return table + (int64_t)__shfl(lrow, 8 * i + sub_row) * ld + s * kSetsWideCols + sub_col;
            });
            tile_transpose<kSetsWideCols>(e, slab, lane);
        } else {
            u32x4 w[1][8];
            const char* bytes = reinterpret_cast<const char*>(table);
            tile16_fetch_from<kSetsWideCols>(w, [&](auto ii) {
                constexpr int i = decltype(ii)::value;
                return bytes + ((int64_t)__shfl(lrow, 8 * i + sub_row) * ld + s * kSetsWideCols) * 2 + sub_col * 4;
            });
            tile16_transpose_widen<kSetsWideCols, TE>(e, w, slab, lane);
        }
        sets_wide_step<SIDE, kSetsWideCols>(acc, e, coef + s * kSetsWideCols, nq, D);
    }
    int col = n_full * kSetsWideCols;
    const TE* row = table + (int64_t)lrow * ld;
    sets_wide_tail<SIDE, 32>(acc, row, coef, nq, D, col);
    sets_wide_tail<SIDE, 16>(acc, row, coef, nq, D, col);
    sets_wide_tail<SIDE, 8>(acc, row, coef, nq, D, col);
    sets_wide_tail<SIDE, 4>(acc, row, coef, nq, D, col);
}

}  // namespace blp
