// topk_wide.hip -- filtered, deterministic top-k entity prediction over the whole candidate table for DistMult / ComplEx /
// SimplE at ANY width (include/blp_hip.h: blp_topk_wide): D % 4 == 0, 4 <= D <= 1024 -- the bag-of-words / DKRL encoders' 300
// and 768, where topk.hip's layout (a lane holds a whole row in D VGPRs, one code object per width) does not fit.  The
// contract is blp_topk's word for word: queries as rows of `source` / rel_emb, row_base shards, the filter rules, the (Q, k)
// rows and scores -- descending score, ties by ascending row, NaN last, -1 / quiet NaN beyond the candidates left.
//
// The kernel joins two halves the tree already has.  The arithmetic is rank_all_wide.hip's (wide_bilinear.h): eight lanes per
// candidate row restate torch's sum(dim=-1) order from registers, kAwRows rows of a group against the kAwQueries queries of the
// workgroup's chunk, the coefficients in LDS.  The selection is topk.hip's (topk_lists.h): 64-bit keys, per-(wave, query)
// sorted lists of k keys in LDS, the list's last entry as the admission threshold, the filter looked up only for the lanes
// above it (unfiltered_rows: a lane offers a row of its own, not row0 + lane), the fold of the four waves' lists, one list
// of k keys per (query, slab) in the workspace, topk.hip's merge kernel.
//
// Launch chain of a call (the caller's stream, no host sync, no allocation), at most three launches:
//   1. topk_wide_kernel   head-replacing queries: (query chunks) x (candidate slabs)
//   2. topk_wide_kernel   tail-replacing queries
//   3. topk_merge<keys>   (topk.hip) per query the k best of its n_slabs lists -> rows / scores
// Every (chunk, slab) workgroup writes the lists of its queries, empty ones included: the workspace is never cleared.
//
// A trip of a wave is 8 groups x kAwRows rows; after wide_trip the scores of a group's rows are valid in lanes 0 .. 3 of its
// eight, so lane r of a group offers row r: one list_offer per query and trip carries the wave's 16 keys.
//
// There is NO re-scoring launch and none is needed: the pass's number is score_fn's bit for bit, sign of zero included.  The
// pass differs from the reference's order only in dropping additions of all-zero upper cascade levels (wide_bilinear.h), and
// those cannot change a bit: every chain starts from +0.0f, and x + y is -0 only when x and y both are, so no accumulator and
// no partial sum of either order is ever -0; for every other z, z + (+0) == z.  (A zero score is therefore always +0, unless
// SimplE's final s / 2 underflows a negative s -- the reference's own last operation, done here on the same s.)  The key
// carries the score exactly (topk_lists.h: the low bit keeps the sign of zero, a NaN comes out as 0x7fc00000).  The device
// tests hold the scores to the oracle's bits, zero scores of negative products among them.
//
// LDS of a workgroup: the coefficients, kAwQueries x K x n4 floats (K n4 <= 2 D: at most 64 KiB, ComplEx at D = 1024), then
// the lists, kAwWaves x kAwQueries x k keys (at most 64 KiB, k = 256): at most 128 KiB of the CU's 160 KiB with the
// chunk of 8 queries the registers are laid out for, so the chunk never has to shrink (topk_wide_lds_bytes; above 64 KiB the
// launch raises the kernel's dynamic-LDS limit and returns a failure to do so).  Registers: wide_trip's accumulators (64, or
// 128 with the cascade) and the double-buffered columns, as in rank_all_wide_kernel; the 16 scores of a trip outlive them
// only while the lists are offered.  No kernel of this file uses scratch memory.
//
// Grid: x = query chunks of one side (at most kTwMaxGridX, the workgroup strides), y = candidate slabs.  The slabs of a call:
// min(kTwTargetGroups / chunks, trips of the table), at least 1 -- few queries against a long table: many slabs of few
// trips; many queries: one slab per chunk, the table re-read from L2 / Infinity Cache by every chunk.  A query's top k are
// its k largest keys, a set that does not depend on the order the keys are seen in: the result does not depend on the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "rank_common.h"
#include "score_core.h"
#include "topk_lists.h"
#include "wide_bilinear.h"

#pragma clang fp contract(off)

namespace blp {

namespace {

constexpr int64_t kTwTargetGroups = 2048;  // (chunk, slab) workgroups of a call when the chunks alone give fewer
constexpr int64_t kTwMaxGridX = 32768;
constexpr size_t kTwDefaultLds = 64 << 10;  // dynamic LDS a kernel may use without raising its limit

template <int MODEL, int SIDE, bool CASCADE>
__global__ __launch_bounds__(kAwWaves * 64) void topk_wide_kernel(const float* __restrict__ table, int64_t N, int64_t ld, int D,
                                                                  int64_t row_base, const QRows q_fixed, const QRows q_rel,
                                                                  int64_t q_off, int64_t nq, int64_t slab_rows, int k,
                                                                  const FilterSpec filter, u64* __restrict__ partial) {
    using T = WideTerm<MODEL, SIDE>;
    constexpr int QC = kAwQueries, R = kAwRows;
    extern __shared__ __attribute__((aligned(16))) float tw_smem[];  // coefficients [query of the chunk][K][n4], then the lists
    const int n4 = wide_n4(MODEL, D);
    u64* lists_all = reinterpret_cast<u64*>(tw_smem + QC * T::K * n4);  // [wave][query of the chunk][k]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), grp = lane >> 3, sub = lane & 7;
    u64* lists = lists_all + (size_t)wave * QC * k;
    const int64_t row_lo = (int64_t)blockIdx.y * slab_rows, row_hi = row_lo + slab_rows < N ? row_lo + slab_rows : N;
    const int64_t n_chunks = (nq + QC - 1) / QC;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t q0 = q_off + chunk * QC;
        const int live_q = (int)(q_off + nq - q0 < QC ? q_off + nq - q0 : QC);
        __syncthreads();  // the previous chunk's coefficients and lists have been read
        wide_stage_coef<MODEL, SIDE>(tw_smem, q_fixed, q_rel, q0, live_q, D);
        for (int i = lane; i < live_q * k; i += 64) lists[i] = 0ull;
        __syncthreads();

        for (int64_t rb = row_lo + wave * (8 * R); rb < row_hi; rb += kAwBlockRows) {  // wave-uniform
            const float* base[R];  // the group's rows (past the slab: its last row, not offered)
            u64 slot = 0ull;       // lane r of the eight offers row r: its global row + 1, 0 = nothing to offer
            int lrow = 0;          // ... and its row of this shard
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t row = rb + grp + 8 * r;
                const bool live = row < row_hi;
                base[r] = table + (live ? row : row_hi - 1) * ld;
                if (sub == r && live) {
                    slot = (u64)(row_base + row) + 1ull;
                    lrow = (int)row;  // N <= 2^31
                }
            }
            float s[QC][R];
            wide_trip<MODEL, SIDE, CASCADE>(s, base, tw_smem, D, sub);
#pragma unroll
            for (int q = 0; q < QC; ++q) {
                if (q < live_q) {  // workgroup-uniform
                    float mine = s[q][0];
#pragma unroll
                    for (int r = 1; r < R; ++r) mine = sub == r ? s[q][r] : mine;
                    const u64 key = slot ? topk_key(mine, (int64_t)(slot - 1ull)) : 0ull;
                    list_offer(lists + q * k, k, key, lane,
                               [&](u64 m) { return filter.on() ? unfiltered_rows(filter, q0 + q, N, lrow, m, lane) : m; });
                }
            }
        }

        __syncthreads();
        // fold the other waves' lists into wave 0's, query j by wave j % kAwWaves; write the (chunk, slab)'s list
        for (int j = wave; j < live_q; j += kAwWaves) {
            u64* L = lists_all + (size_t)j * k;
            for (int w = 1; w < kAwWaves; ++w) {
                const u64* src = lists_all + ((size_t)w * QC + j) * k;
                for (int c = 0; c < k; c += 64)
                    list_offer(L, k, c + lane < k ? src[c + lane] : 0ull, lane, [](u64 m) { return m; });
            }
            u64* out = partial + ((size_t)(q0 + j) * gridDim.y + blockIdx.y) * k;
            for (int i = lane; i < k; i += 64) out[i] = L[i];
        }
    }
}

// candidate slabs of a call: from N, the query counts and nothing else (the workspace is sized by it)
int64_t topk_wide_slabs(int64_t N, int64_t q_head, int64_t q_tail) {
    const int64_t chunks = (q_head + kAwQueries - 1) / kAwQueries + (q_tail + kAwQueries - 1) / kAwQueries;
    const int64_t n_trips = (N + kAwBlockRows - 1) / kAwBlockRows;
    int64_t s = chunks > 0 ? kTwTargetGroups / chunks : 1;
    if (s > n_trips) s = n_trips;
    return s < 1 ? 1 : s;
}

template <int MODEL, int SIDE>
hipError_t launch_side(const float* table, int64_t N, int64_t ld, int D, int64_t row_base, const QRows& q_fixed, const QRows& q_rel,
                       int64_t q_off, int64_t nq, int64_t n_slabs, int k, const FilterSpec& filter, u64* partial, hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    const int64_t n_chunks = (nq + kAwQueries - 1) / kAwQueries, n_trips = (N + kAwBlockRows - 1) / kAwBlockRows;
    const int64_t trips = (n_trips + n_slabs - 1) / n_slabs;  // (a slab past the table's end writes empty lists)
    const dim3 grid((unsigned)(n_chunks < kTwMaxGridX ? n_chunks : kTwMaxGridX), (unsigned)n_slabs);
    const size_t lds = topk_wide_lds_bytes(MODEL, SIDE, D, k);
    auto launch = [&](auto kernel) {
        if (lds > kTwDefaultLds) {
            const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (err != hipSuccess) return err;
        }
        kernel<<<grid, kAwWaves * 64, lds, stream>>>(table, N, ld, D, row_base, q_fixed, q_rel, q_off, nq, trips * kAwBlockRows, k, filter,
                                                     partial);
        return hipGetLastError();
    };
    return wide_terms(MODEL, D) >= 512 ? launch(topk_wide_kernel<MODEL, SIDE, true>) : launch(topk_wide_kernel<MODEL, SIDE, false>);
}

template <int MODEL>
hipError_t topk_wide_impl(int D, const float* table, int64_t N, int64_t ld, int64_t row_base, const QRows& q_fixed, const QRows& q_rel,
                          int64_t q_head, int64_t q_tail, int k, const FilterSpec& filter, int64_t* rows, float* scores, u64* partial,
                          hipStream_t stream) {
    const int64_t Q = q_head + q_tail;
    if (N == 0) return launch_topk_merge_keys(partial, Q, 0, k, rows, scores, stream);  // every slot empty
    const int64_t n_slabs = topk_wide_slabs(N, q_head, q_tail);
    hipError_t err = launch_side<MODEL, HEAD>(table, N, ld, D, row_base, q_fixed, q_rel, 0, q_head, n_slabs, k, filter, partial, stream);
    if (err != hipSuccess) return err;
    err = launch_side<MODEL, TAIL>(table, N, ld, D, row_base, q_fixed, q_rel, q_head, q_tail, n_slabs, k, filter, partial, stream);
    if (err != hipSuccess) return err;
    return launch_topk_merge_keys(partial, Q, n_slabs * k, k, rows, scores, stream);
}

}  // namespace

bool topk_wide_supported(int model, int D, int k) {
    return (model == DISTMULT || model == COMPLEX || model == SIMPLE) && D >= 4 && D <= kAwMaxD && D % 4 == 0 && k >= 1 && k <= kTopkMaxK;
}

size_t topk_wide_lds_bytes(int model, int side, int D, int k) {
    const int K = model == DISTMULT ? (side == HEAD ? 2 : 1) : (model == COMPLEX ? 4 : 3);  // WideTerm<model, side>::K
    return (size_t)kAwQueries * K * wide_n4(model, D) * sizeof(float) + (size_t)kAwWaves * kAwQueries * k * sizeof(u64);
}

size_t topk_wide_workspace_bytes(int64_t N, int64_t q_head, int64_t q_tail, int k) {
    return align_up((size_t)(q_head + q_tail) * topk_wide_slabs(N, q_head, q_tail) * k * sizeof(u64), 256);
}

hipError_t launch_topk_wide(int model, int D, const float* table, int64_t N, int64_t ld, int64_t row_base, const QRows q_fixed,
                            const QRows q_rel, int64_t q_head, int64_t q_tail, int k, const FilterSpec& filter, int64_t* rows,
                            float* scores, void* workspace, hipStream_t stream) {
    if (!topk_wide_supported(model, D, k)) return hipErrorInvalidValue;
    if (q_head + q_tail == 0) return hipSuccess;
    u64* partial = static_cast<u64*>(workspace);
    if (model == DISTMULT)
        return topk_wide_impl<DISTMULT>(D, table, N, ld, row_base, q_fixed, q_rel, q_head, q_tail, k, filter, rows, scores, partial, stream);
    if (model == COMPLEX)
        return topk_wide_impl<COMPLEX>(D, table, N, ld, row_base, q_fixed, q_rel, q_head, q_tail, k, filter, rows, scores, partial, stream);
    return topk_wide_impl<SIMPLE>(D, table, N, ld, row_base, q_fixed, q_rel, q_head, q_tail, k, filter, rows, scores, partial, stream);
}

}  // namespace blp
