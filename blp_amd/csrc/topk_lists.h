// topk_lists.h -- the selection machinery of the top-k kernels (topk.hip: the whole table; topk_sets.hip: inside candidate
// sets): the 64-bit keys and the per-(wave, query) sorted lists in LDS.  topk.hip's header comment describes the order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rank_common.h"
#include "score_core.h"

namespace blp {

typedef unsigned long long u64;

constexpr int kTopkWaves = 4;               // waves per workgroup of topk_tiles
constexpr int kTopkMaxChunk = 32;           // queries per workgroup
constexpr int kTopkListBytes = 24576;       // LDS for the lists of one workgroup (kTopkWaves x chunk x k keys)
constexpr int kTopkTargetGroups = 512;      // workgroups of topk_tiles when the queries alone give fewer
constexpr int kTopkMaxK = 256;
constexpr int kTopkMergeMaxWaves = 16;

__host__ __device__ inline int topk_chunk(int k) {
    const int c = kTopkListBytes / (kTopkWaves * 8 * k);
    return c < 1 ? 1 : (c > kTopkMaxChunk ? kTopkMaxChunk : c);
}

__device__ __forceinline__ u64 topk_key(float s, int64_t row) {
    unsigned b = __float_as_uint(s);
    const unsigned neg0 = b == 0x80000000u;
    unsigned hi;
    if (__builtin_isnan(s)) {
        hi = 1u;
    } else {
        if (neg0) b = 0u;
        hi = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    const unsigned lo = ((0x7fffffffu - (unsigned)row) << 1) | neg0;
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ int64_t key_row(u64 key) { return key ? (int64_t)(0x7fffffffu - ((unsigned)key >> 1)) : -1; }
__device__ __forceinline__ float key_score(u64 key) {
    const unsigned hi = (unsigned)(key >> 32);
    if (hi <= 1u) return __uint_as_float(0x7fc00000u);
    unsigned b = (hi & 0x80000000u) ? (hi & 0x7fffffffu) : ~hi;
    if (key & 1ull) b = 0x80000000u;
    return __uint_as_float(b);
}

// Insert x (wave-uniform) into the list L[0, n) in LDS, sorted descending, dropping its last entry.  Lane l moves slots
// l, l + 64, ... (n <= kTopkMaxK: four per lane, statically indexed).
__device__ __forceinline__ void list_insert(u64* L, int n, u64 x, int lane) {
    u64 nv[kTopkMaxK / 64];
    static_for<kTopkMaxK / 64>([&](auto jj) {
        constexpr int j = decltype(jj)::value;
        const int p = lane + 64 * j;
        if (p < n) {
            const u64 old = L[p];
            const u64 prev = p > 0 ? L[p - 1] : ~0ull;
            nv[j] = old > x ? old : (prev > x ? x : prev);
        }
    });
    wave_lds_sync();
    static_for<kTopkMaxK / 64>([&](auto jj) {
        constexpr int j = decltype(jj)::value;
        const int p = lane + 64 * j;
        if (p < n) L[p] = nv[j];
    });
    wave_lds_sync();
}

// Offer the wave's 64 keys (one per lane; 0 = none) to the list L[0, n): lanes above its last entry, minus those
// drop(mask) removes, are inserted.
template <class Drop>
__device__ __forceinline__ void list_offer(u64* L, int n, u64 key, int lane, Drop drop) {
    u64 thr = L[n - 1];
    u64 mask = __ballot(key > thr);
    if (!mask) return;
    mask = drop(mask);
    while (mask) {
        const int b = __builtin_ctzll(mask);
        mask &= mask - 1;
        const u64 x = __shfl(key, b);
        if (x <= thr) continue;
        list_insert(L, n, x, lane);
        thr = L[n - 1];
    }
}

// unfiltered() (topk.hip) for a gathered tile: the lanes of `mask` whose candidate -- lane b holds table row lrow of ITS OWN,
// not row0 + b -- query q's filter segment does NOT remove.  The segment is read 64 entries at a time (filter_row: exclude,
// ent2idx, row_base as filter_finalize applies them); every admitted lane's row is broadcast with one shuffle and looked up
// with one compare + ballot per chunk of the segment.
__device__ __forceinline__ u64 unfiltered_rows(const FilterSpec& f, int64_t q, int64_t N, int lrow, u64 mask, int lane) {
    const int64_t lo = f.lo[q], hi = f.hi[q];
    for (int64_t c = lo; c < hi && mask; c += 64) {
        const int64_t v = c + lane < hi ? filter_row(f, q, c + lane, N) : -1;
        u64 m = mask;
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            if (__ballot(v == (int64_t)__shfl(lrow, b))) mask &= ~(1ull << b);
        }
    }
    return mask;
}

}  // namespace blp
