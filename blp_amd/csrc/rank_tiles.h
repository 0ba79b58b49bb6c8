// rank_tiles.h -- the inner body of the exact f32 ranking kernel (rank_all.hip: rank_tiles_kernel), shared with the kernels
// that run the same body over other tiles (rank_sets.hip: tiles gathered from a candidate set): a wave's 64 rows in registers
// (tile.h), the queries of a chunk applied to them -- TransE from hand-pipelined scalar loads, the bilinear models from
// LDS-staged coefficient rows (DppCoef) or scalar-cache rows --, two rank counts per query added to the wave's LDS counters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rank_common.h"
#include "score_core.h"
#include "tile.h"

#pragma clang fp contract(off)

namespace blp {

constexpr int kQueryChunk = 128;     // queries per workgroup pass over its tiles
constexpr int kQB = 4;               // queries staged per LDS coefficient batch
__host__ __device__ constexpr int kMaxCoef(int D) { return 2 * D; }

// Stage `count` floats (a multiple of 4, at most 2 * 4 * 256) from global memory into LDS with
// LDS-DMA (global_load_lds_dwordx4: 16 B per lane straight into LDS at wave-uniform base + lane * 16,
// no VGPR round trip).  The copy stays in flight until the caller's `s_waitcnt vmcnt(0)` + barrier.
__device__ __forceinline__ void stage_dma(const float* __restrict__ src, float* dst, int count, int wave, int lane) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int base = (k * kWaves + wave) * 256;  // floats: 64 lanes x 4 per wave instruction
        if (base + lane * 4 < count)
            __builtin_amdgcn_global_load_lds((global_cptr)(src + base + lane * 4), (lds_ptr)(dst + base), 16, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------------
// TransE with scalar-cache coefficients, hand-pipelined (many-query mode).  Scalar loads return out of
// order, so every s_waitcnt on them is a full drain; the compiler issues the next chunk's load in the
// middle of a chunk and waits a few instructions later, exposing the scalar-cache latency 8-16 times
// per query.  Here the 64-byte chunk k+1 (and, on the last chunk, chunk 0 of the NEXT query) is
// requested before chunk k's 32-48 VALU instructions and drained after them, and one dword of every
// line of the query after next is touched once per query so that those requests hit the scalar cache.
template <int D, int CHUNK0, class Get>
__device__ __forceinline__ void l1_chunk(const float (&e)[D], float& acc, bool first, Get x_of) {
    // 16 elements starting at CHUNK0: differences kPipe ahead of the dependent |x| adds
    float x[kPipe];
    static_for<kPipe>([&](auto k) { x[k] = x_of(k); });
    static_for<16>([&](auto k) {
        constexpr int i = decltype(k)::value;
        const float cur = fabsf(x[i % kPipe]);
        if constexpr (i + kPipe < 16) x[i % kPipe] = x_of(ic<i + kPipe>{});
        acc = (first && i == 0) ? cur : acc + cur;
    });
}

// tail-replacing query: coefficient row = h + r (D floats).  `cur` holds chunk 0 on entry and chunk 0
// of `next_row` on exit.
template <int D>
__device__ __forceinline__ float transe_tail_sgpr(const float (&e)[D], sf16& cur, const float* row,
                                                  const float* next_row, const float* touch_row) {
    float acc = 0.f;
    static_for<D / 16>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        sf16 nxt;
        if constexpr (k + 1 < D / 16) nxt = sload16<(k + 1) * 64>(row); else nxt = sload16<0>(next_row);
        if constexpr (k == 0) stouch<D * 4>(touch_row);
        l1_chunk<D, 16 * k>(e, acc, k == 0, [&](auto ii) { return cur[decltype(ii)::value] - e[16 * k + decltype(ii)::value]; });
        sdrain(nxt);
        cur = nxt;
    });
    return -acc;
}

// head-replacing query: coefficient row = r (D floats) then t (D floats): (e + r) - t
template <int D>
__device__ __forceinline__ float transe_head_sgpr(const float (&e)[D], sf16& cur_r, sf16& cur_t, const float* row,
                                                  const float* next_row, const float* touch_row) {
    float acc = 0.f;
    static_for<D / 16>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        sf16 nr, nt;
        if constexpr (k + 1 < D / 16) { nr = sload16<(k + 1) * 64>(row); nt = sload16<D * 4 + (k + 1) * 64>(row); }
        else { nr = sload16<0>(next_row); nt = sload16<D * 4>(next_row); }
        if constexpr (k == 0) stouch<2 * D * 4>(touch_row);
        l1_chunk<D, 16 * k>(e, acc, k == 0, [&](auto ii) {
            constexpr int i = decltype(ii)::value;
            const float y = e[16 * k + i] + cur_r[i];
            return y - cur_t[i];
        });
        sdrain(nr, nt);
        cur_r = nr;
        cur_t = nt;
    });
    return -acc;
}

template <int SIDE, int D>
__device__ __forceinline__ void score_batch_transe_sgpr(const float (&e)[D], bool valid, const float* rows, int nq,
                                                        const float* __restrict__ key_true, unsigned* cnt, int wave,
                                                        int lane) {
    constexpr int C = Scorer<TRANSE, SIDE, D>::C;
    if (nq <= 0) return;
    // (no copy of `a` before its wait: between a hand-issued scalar load and its s_waitcnt the registers hold nothing yet --
    //  tests/test_abi.py reads the disassembly for exactly that)
    sf16 a = sload16<0>(rows), b;
    if constexpr (SIDE == HEAD) {
        b = sload16<D * 4>(rows);
        sdrain(a, b);
    } else {
        sdrain(a);
        b = a;  // (unused on this side)
    }
    for (int j = 0; j < nq; ++j) {
        const float* row = rows + (size_t)j * C;
        const float* next_row = rows + (size_t)(j + 1 < nq ? j + 1 : j) * C;
        // the four waves of a workgroup walk the same rows: they take turns touching the lines of the
        // query three ahead, so each wave pays the scalar-cache miss drain once every four queries
        const float* touch_row = ((j & 3) == wave && j + 3 < nq) ? rows + (size_t)(j + 3) * C : row;
        const float key = SIDE == HEAD ? transe_head_sgpr<D>(e, a, b, row, next_row, touch_row)
                                       : transe_tail_sgpr<D>(e, a, row, next_row, touch_row);
        const float kt = key_true[j];
        const unsigned gt = __popcll(__ballot(valid && key > kt));
        const unsigned ge = __popcll(__ballot(valid && key >= kt));
        if (lane == 0) {
            __hip_atomic_fetch_add(cnt + 2 * j, gt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            __hip_atomic_fetch_add(cnt + 2 * j + 1, ge, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
    }
}

// Score nq queries of one side against the wave's tile and add the two rank counts of each to the
// wave's LDS counters.  USE_SGPR = false: coefficient rows are staged in LDS at `cur` (DppCoef).
// USE_SGPR = true: `cur` is the wave-uniform global address of the rows, so the compiler fetches them
// with scalar loads and they are SGPR operands of full-rate VALU instructions -- the right choice
// when the whole query block (a few KB) stays resident in the scalar cache (STATIC mode); DPP
// operands issue at roughly a third of the plain VALU rate on gfx950 (tools/valu_ubench.hip).
template <int MODEL, int SIDE, int D, bool USE_SGPR>
__device__ __forceinline__ void score_batch(const float (&e)[D], bool valid, const float* cur, int nq,
                                            const float* __restrict__ key_true, unsigned* cnt, int lane) {
    using S = Scorer<MODEL, SIDE, D>;
    for (int j = 0; j < nq; ++j) {
        float key;
        if constexpr (USE_SGPR) {
            key = S::template score<false>(e, PtrCoef{cur + (size_t)j * S::C});
        } else {
            key = S::template score<false>(e, DppCoef{reinterpret_cast<const float4*>(cur + j * S::C) + (lane & 3)});
        }
        const float kt = key_true[j];
        const unsigned gt = __popcll(__ballot(valid && key > kt));
        const unsigned ge = __popcll(__ballot(valid && key >= kt));
        if (lane == 0) {  // ds_add_u32 without return: fire and forget
            __hip_atomic_fetch_add(cnt + 2 * j, gt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            __hip_atomic_fetch_add(cnt + 2 * j + 1, ge, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
    }
}

// Apply the n queries of one side (coefficient rows coef[0..n), C floats each, contiguous in global
// memory) to the wave's tile.  The workgroup stages kQB queries at a time into a double-buffered LDS
// block shared by its four waves (LDS-DMA, in flight under the previous batch's arithmetic); one
// barrier per batch.  Every wave of the workgroup calls this with the same n.
template <int MODEL, int SIDE, int D>
__device__ __forceinline__ void apply_queries(const float (&e)[D], bool valid, const float* __restrict__ coef,
                                              const float* __restrict__ key_true, int n, float* cbuf,
                                              unsigned* cnt, int wave, int lane) {
    using S = Scorer<MODEL, SIDE, D>;
    constexpr int C = S::C;
    static_assert(C % 16 == 0 && kQB * C <= 2 * kWaves * 256, "coefficient batch does not fit the staging plan");
    if (n <= 0) return;
    const int nb = (n + kQB - 1) / kQB;
    stage_dma(coef, cbuf, (n < kQB ? n : kQB) * C, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int b = 0; b < nb; ++b) {
        const float* cur = cbuf + (b & 1) * (kQB * kMaxCoef(D));
        const int nq = n - b * kQB < kQB ? n - b * kQB : kQB;
        const int next = n - (b + 1) * kQB < kQB ? n - (b + 1) * kQB : kQB;  // <= 0 on the last batch
        // the other buffer was last read in batch b-1, which every wave left through the barrier below
        if (next > 0) stage_dma(coef + (size_t)(b + 1) * kQB * C, cbuf + ((b + 1) & 1) * (kQB * kMaxCoef(D)), next * C, wave, lane);
        score_batch<MODEL, SIDE, D, false>(e, valid, cur, nq, key_true + b * kQB, cnt + 2 * b * kQB, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of the next batch has landed
        __syncthreads();
    }
}

}  // namespace blp
