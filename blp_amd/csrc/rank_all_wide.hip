// rank_all_wide.hip -- all-entities ranking for DistMult / ComplEx / SimplE at any width (D % 4 == 0, 4 <= D <= 1024: the
// bag-of-words / DKRL encoders' 300 and 768) on gfx950: the exact f32 table pass, no (Q, N) array anywhere
// (include/blp_hip.h: blp_rank_all_wide).  First version: no pre-pass in front of it.
//
// Launch chain of a call (the caller's stream, no host sync, no allocation):
//   1. wide_bilinear_true_key   eight lanes per query: the true entity's key by the pass's own arithmetic (wide_pair_score);
//                               zeroes the accumulators
//   2. rank_all_wide_kernel     head-replacing queries: (query chunks) x (candidate slabs)
//   3. rank_all_wide_kernel     tail-replacing queries
//   4. wide_bilinear_filter_finalize   64 queries per workgroup: the filter's rows re-scored by wide_pair_score,
//                                      counts[q] = {gt, ge, gt - fgt, ge - fge}
//
// The table pass.  wide_bilinear.h holds its arithmetic (shared with topk_wide.hip): the reference's sum order mapped onto
// eight lanes per candidate row, kAwRows rows of a group against the kAwQueries queries of the workgroup's chunk, the
// coefficients in LDS (wide_stage_coef), the scores of a trip in registers (wide_trip).  Here lane 0 of a group compares
// with the true key and the wave counts by ballot into scalar counters, flushed once per (chunk, slab) with a 64-bit atomic
// (gt low word, ge high word).
//
// Grid: x = query chunks (at most kAwMaxGridX, the workgroup strides), y = candidate slabs of about kAwSlabBytes (one
// slab stays in an XCD's L2 while the chunks that run together stream it), fewer rows per slab when there are few chunks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "rank_common.h"
#include "score_core.h"
#include "wide_bilinear.h"
#include "wide_bilinear_keys.h"

#pragma clang fp contract(off)

namespace blp {

namespace {

constexpr int64_t kAwSlabBytes = 2 << 20;
constexpr int64_t kAwMaxGridX = 32768, kAwMaxGridY = 32768;

template <int MODEL, int SIDE, bool CASCADE>
__global__ __launch_bounds__(kAwWaves * 64) void rank_all_wide_kernel(const float* __restrict__ table, int64_t N, int64_t ld, int D,
                                                                      const QRows q_fixed, const QRows q_rel,
                                                                      const float* __restrict__ key_true, int64_t q_off, int64_t nq,
                                                                      int64_t slab_rows, unsigned long long* __restrict__ acc_out) {
    constexpr int QC = kAwQueries, R = kAwRows;
    extern __shared__ __attribute__((aligned(16))) float aw_coef[];  // [query of the chunk][K][n4]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 3, sub = lane & 7;
    const int64_t row_lo = (int64_t)blockIdx.y * slab_rows, row_hi = row_lo + slab_rows < N ? row_lo + slab_rows : N;
    const int64_t n_chunks = (nq + QC - 1) / QC;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t q0 = q_off + chunk * QC;
        const int live_q = (int)(q_off + nq - q0 < QC ? q_off + nq - q0 : QC);
        __syncthreads();  // the previous chunk's coefficients have been read
        wide_stage_coef<MODEL, SIDE>(aw_coef, q_fixed, q_rel, q0, live_q, D);
        __syncthreads();
        float kt[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) kt[q] = key_true[q0 + (q < live_q ? q : 0)];
        unsigned cgt[QC], cge[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) cgt[q] = cge[q] = 0;

        for (int64_t rb = row_lo + wave * (8 * R); rb < row_hi; rb += kAwBlockRows) {  // wave-uniform
            const float* base[R];  // the group's rows (past the slab: its last row, not counted)
            bool live[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t row = rb + grp + 8 * r;
                live[r] = row < row_hi;
                base[r] = table + (live[r] ? row : row_hi - 1) * ld;
            }
            float s[QC][R];
            wide_trip<MODEL, SIDE, CASCADE>(s, base, aw_coef, D, sub);
            // lane 0 of a group compares with the true key; the wave counts by ballot
#pragma unroll
            for (int q = 0; q < QC; ++q) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const bool mine = live[r] && sub == 0;
                    cgt[q] += (unsigned)__popcll(__ballot(mine && s[q][r] > kt[q]));
                    cge[q] += (unsigned)__popcll(__ballot(mine && s[q][r] >= kt[q]));
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < QC; ++q)
                if (q < live_q && (cgt[q] | cge[q]) != 0)
                    atomicAdd(acc_out + q0 + q, (unsigned long long)cgt[q] | ((unsigned long long)cge[q] << 32));
        }
    }
}

// (wide_bilinear_true_key_kernel: wide_bilinear_keys.h, shared with rank_sets_wide_bilinear.hip)

// Last kernel of a call (as rank_all.hip's filter_finalize_kernel, run-time width): a workgroup owns 64 queries, its
// waves take the ones that have filter entries in turn (eight entries per step, eight lanes each: wide_pair_score), thread
// q writes query q's four counts.
template <int MODEL>
__global__ __launch_bounds__(256) void wide_bilinear_filter_finalize_kernel(const float* __restrict__ table, int64_t N, int64_t ld, int D,
                                                                            const QRows q_fixed, const QRows q_rel,
                                                                            const float* __restrict__ key_true, int64_t q_head, int64_t Q,
                                                                            const FilterSpec filter,
                                                                            const unsigned long long* __restrict__ acc,
                                                                            int32_t* __restrict__ counts) {
    __shared__ int list[kSweepQueries], n_list;
    __shared__ unsigned removed[kSweepQueries][2];
    const int64_t q_base = (int64_t)blockIdx.x * kSweepQueries;
    const int lane = threadIdx.x & 63, grp = lane >> 3, sub = lane & 7;
    if (threadIdx.x < 64) {
        const int64_t q = q_base + lane;
        const bool any = filter.on() && N > 0 && q < Q && filter.hi[q] > filter.lo[q];
        removed[lane][0] = removed[lane][1] = 0;
        const unsigned long long mask = __ballot(any);
        if (any) list[__popcll(mask & ((1ull << lane) - 1ull))] = lane;
        if (lane == 0) n_list = __popcll(mask);
    }
    __syncthreads();
    for (int i = threadIdx.x >> 6; i < n_list; i += 4) {  // wave-uniform
        const int slot = list[i];
        const int64_t q = q_base + slot;
        const float kt = key_true[q];
        const float* f = q_fixed.row(q);
        const float* r = q_rel.row(q);
        const int64_t lo = filter.lo[q], hi = filter.hi[q];
        unsigned gt = 0, ge = 0;
        for (int64_t k0 = lo; k0 < hi; k0 += 8) {  // wave-uniform
            const int64_t row = k0 + grp < hi ? filter_row(filter, q, k0 + grp, N) : -1;
            const float* e = table + (row >= 0 ? row : 0) * ld;  // (N > 0 here: row 0 exists)
            const float key = q < q_head ? wide_pair_score<MODEL, HEAD>(e, f, r, D, sub) : wide_pair_score<MODEL, TAIL>(e, f, r, D, sub);
            const bool mine = row >= 0 && sub == 0;
            gt += (unsigned)__popcll(__ballot(mine && key > kt));
            ge += (unsigned)__popcll(__ballot(mine && key >= kt));
        }
        if (lane == 0) { removed[slot][0] = gt; removed[slot][1] = ge; }
    }
    __syncthreads();
    if (threadIdx.x < 64 && q_base + lane < Q) {
        const int64_t q = q_base + lane;
        const unsigned long long a = acc[q];
        const int32_t all_gt = (int32_t)(a & 0xffffffffull), all_ge = (int32_t)(a >> 32);
        reinterpret_cast<int4*>(counts)[q] =
            make_int4(all_gt, all_ge, all_gt - (int32_t)removed[lane][0], all_ge - (int32_t)removed[lane][1]);
    }
}

template <int MODEL, int SIDE>
hipError_t launch_side(const float* table, int64_t N, int64_t ld, int D, const QRows& q_fixed, const QRows& q_rel,
                       const float* key_true, int64_t q_off, int64_t nq, unsigned long long* acc, int n_cu, hipStream_t stream) {
    if (nq == 0 || N == 0) return hipSuccess;
    const int n = MODEL == DISTMULT ? D : D / 2, n4 = (n + 3) & ~3;
    const int64_t n_chunks = (nq + kAwQueries - 1) / kAwQueries, n_trips = (N + kAwBlockRows - 1) / kAwBlockRows;
    // trips of a slab: what keeps the slab in L2; fewer when the chunks alone would not fill the chip; more when the
    // slabs would outnumber the grid's y extent
    int64_t trips = kAwSlabBytes / ((int64_t)D * 4 * kAwBlockRows);
    const int64_t fill = n_trips * n_chunks / (8ll * (n_cu > 0 ? n_cu : 256));
    if (trips > fill) trips = fill;
    if (trips < (n_trips + kAwMaxGridY - 1) / kAwMaxGridY) trips = (n_trips + kAwMaxGridY - 1) / kAwMaxGridY;
    if (trips < 1) trips = 1;
    const int64_t n_slabs = (n_trips + trips - 1) / trips;
    const dim3 grid((unsigned)(n_chunks < kAwMaxGridX ? n_chunks : kAwMaxGridX), (unsigned)n_slabs);
    const size_t lds = (size_t)kAwQueries * WideTerm<MODEL, SIDE>::K * n4 * sizeof(float);  // <= 64 KiB: K n4 <= 2 D
    if (n >= 512)
        rank_all_wide_kernel<MODEL, SIDE, true><<<grid, kAwWaves * 64, lds, stream>>>(table, N, ld, D, q_fixed, q_rel, key_true, q_off, nq,
                                                                                      trips * kAwBlockRows, acc);
    else
        rank_all_wide_kernel<MODEL, SIDE, false><<<grid, kAwWaves * 64, lds, stream>>>(table, N, ld, D, q_fixed, q_rel, key_true, q_off, nq,
                                                                                       trips * kAwBlockRows, acc);
    return hipGetLastError();
}

struct AllWideWorkspace {
    float* key_true;
    unsigned long long* acc;
    size_t bytes;
};

AllWideWorkspace carve_all_wide(void* base, int64_t Q) {
    AllWideWorkspace w;
    char* p = static_cast<char*>(base);
    size_t off = 0;
    w.key_true = reinterpret_cast<float*>(p + off);
    off += align_up((size_t)Q * sizeof(float), 256);
    w.acc = reinterpret_cast<unsigned long long*>(p + off);
    off += align_up((size_t)Q * sizeof(unsigned long long), 256);
    w.bytes = off;
    return w;
}

template <int MODEL>
hipError_t rank_all_wide_impl(int D, const float* table, int64_t N, int64_t ld, const QRows& q_fixed, const QRows& q_rel,
                              const QRows& q_true, int64_t q_head, int64_t q_tail, const FilterSpec& filter, int32_t* counts,
                              void* workspace, int n_cu, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
    const int64_t Q = q_head + q_tail;
    const AllWideWorkspace w = carve_all_wide(workspace, Q);
    const int64_t key_blocks = (Q + 31) / 32;
    wide_bilinear_true_key_kernel<MODEL><<<(unsigned)(key_blocks < 65536 ? key_blocks : 65536), 256, 0, stream>>>(
        D, q_fixed, q_rel, q_true, q_head, Q, w.key_true, w.acc);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    if (ev_start) (void)hipEventRecord(ev_start, stream);
    err = launch_side<MODEL, HEAD>(table, N, ld, D, q_fixed, q_rel, w.key_true, 0, q_head, w.acc, n_cu, stream);
    if (err != hipSuccess) return err;
    err = launch_side<MODEL, TAIL>(table, N, ld, D, q_fixed, q_rel, w.key_true, q_head, q_tail, w.acc, n_cu, stream);
    if (err != hipSuccess) return err;
    if (ev_stop) (void)hipEventRecord(ev_stop, stream);
    wide_bilinear_filter_finalize_kernel<MODEL><<<(unsigned)((Q + kSweepQueries - 1) / kSweepQueries), 256, 0, stream>>>(
        table, N, ld, D, q_fixed, q_rel, w.key_true, q_head, Q, filter, w.acc, counts);
    return hipGetLastError();
}

}  // namespace

bool rank_all_wide_supported(int model, int D) {
    return (model == DISTMULT || model == COMPLEX || model == SIMPLE) && D >= 4 && D <= kAwMaxD && D % 4 == 0;
}

size_t rank_all_wide_workspace_bytes(int64_t q_head, int64_t q_tail) { return carve_all_wide(nullptr, q_head + q_tail).bytes; }

hipError_t launch_rank_all_wide(int model, int D, const float* table, int64_t N, int64_t ld, const QRows q_fixed, const QRows q_rel,
                                const QRows q_true, int64_t q_head, int64_t q_tail, const FilterSpec& filter, int32_t* counts,
                                void* workspace, int n_cu, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (!rank_all_wide_supported(model, D)) return hipErrorInvalidValue;
    if (model == DISTMULT)
        return rank_all_wide_impl<DISTMULT>(D, table, N, ld, q_fixed, q_rel, q_true, q_head, q_tail, filter, counts, workspace, n_cu,
                                            stream, ev_start, ev_stop);
    if (model == COMPLEX)
        return rank_all_wide_impl<COMPLEX>(D, table, N, ld, q_fixed, q_rel, q_true, q_head, q_tail, filter, counts, workspace, n_cu,
                                           stream, ev_start, ev_stop);
    return rank_all_wide_impl<SIMPLE>(D, table, N, ld, q_fixed, q_rel, q_true, q_head, q_tail, filter, counts, workspace, n_cu, stream,
                                      ev_start, ev_stop);
}

}  // namespace blp
