// tile16.h -- a wavefront's tile of 64 rows of a 16-BIT table (table_elem.h: IEEE half or bfloat16), one row per lane, widened
// into the D VGPRs the f32 kernels score (tile.h).  A row-piece is 64 columns per 128-byte line (rank_stream16.hip's layout):
// one load instruction reads 8 rows x 128 B, the loads and the transposing LDS slab carry the 16-bit words, and a lane widens
// its row (exactly) only after the transpose.  Which row step i of a lane group reads is the caller's (rank_sets_kernel.h: the
// rows of a candidate set).  The body is topk.hip's Rows16 with the row source taken out; Rows16 itself keeps its own text:
// routed through these functions topk_tiles16 came out with another register allocation, and its code is pinned.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rank_common.h"
#include "score_core.h"
#include "table_elem.h"
#include "tile.h"

namespace blp {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // 16 bytes of a 16-bit row: 8 elements

// 1. every global load of the tile up front: w[s][i] = this lane's 16 bytes of piece s (columns 64 s ..) of row
//    (8 i + lane / 8) of the tile.  src_of(ic<i>): the address of that row's bytes 16 (lane % 8) .. + 15 -- piece 0.
template <int D, class Src>
__device__ __forceinline__ void tile16_fetch_from(u32x4 (&w)[D / 64][8], Src src_of) {
    static_for<8>([&](auto ii) {
        constexpr int i = decltype(ii)::value;
        const char* src = src_of(ii);
        static_for<D / 64>([&](auto ss) {
            constexpr int s = decltype(ss)::value;
            w[s][i] = *reinterpret_cast<const u32x4*>(src + s * 128);
        });
    });
}

// 2. transpose a piece at a time through the wave's slab and widen: afterwards lane l holds row l of the tile in e[]
template <int D, class T>
__device__ __forceinline__ void tile16_transpose_widen(float (&e)[D], const u32x4 (&w)[D / 64][8], float* slab, int lane) {
    float* wr = slab + (lane >> 3) * kLdsStride + (lane & 7) * 4;
    const float* rd = slab + lane * kLdsStride;
    static_for<D / 64>([&](auto ss) {
        constexpr int s = decltype(ss)::value;
        if (s > 0) wave_lds_sync();  // the previous piece's reads are done before the slab is rewritten
        static_for<8>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            *reinterpret_cast<u32x4*>(wr + 8 * i * kLdsStride) = w[s][i];
        });
        wave_lds_sync();
        static_for<8>([&](auto jj) {  // the lane's row, columns 64 s + 8 j .. + 7 (element 2 m in word m's low half)
            constexpr int j = decltype(jj)::value, c = 64 * s + 8 * j;
            const u32x4 v = *reinterpret_cast<const u32x4*>(rd + 4 * j);
            widen_pair<T>(v.x, e[c], e[c + 1]);
            widen_pair<T>(v.y, e[c + 2], e[c + 3]);
            widen_pair<T>(v.z, e[c + 4], e[c + 5]);
            widen_pair<T>(v.w, e[c + 6], e[c + 7]);
        });
    });
}

}  // namespace blp
