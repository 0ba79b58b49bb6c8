// rank_sets_wide_bilinear.hip -- rank against candidate sets SHARED between queries for DistMult / ComplEx / SimplE at ANY
// width (include/blp_hip.h: blp_rank_sets_wide_bilinear): D % 4 == 0, 4 <= D <= 1024 -- the BOW / DKRL encoders' 300 and 768 --,
// an f32 table.  The contract is blp_rank_sets_wide's word for word: the sets CSR of strictly ascending global rows, row_base
// shards, the query grouping, the filter and true-entity rules, the (Q, 4) counts -- the reference's bit for bit.
//
// The arithmetic is wide_bilinear.h's (the table pass of rank_all_wide.hip: eight lanes per candidate row, kAwRows rows of a
// group against the kAwQueries queries of a chunk, the coefficients in LDS); its candidate rows arrive as base pointers, here
// the gathered rows of a set.  The set machinery is rank_sets_wide.hip's: the SetLookup CSR, a unit prefix over the sets,
// persistent workgroups that find their unit by a binary search, set membership in the finalize step.
//
// Kernels of one call (one code object per model for every width: D is a kernel argument; nothing about set or group sizes
// is known on the host):
//   1. wide_bilinear_true_key         (wide_bilinear_keys.h) true keys by wide_pair_score, zeroed accumulators
//   2. sets_wb_unit_prefix            one workgroup: two exclusive prefixes over the sets, one per side, of tiles_g x chunks_g:
//                                     tiles_g = tiles of kSetsWbTile entries, chunks_g = the <= kAwQueries-query chunks of the
//                                     side's run of set g
//   3. rank_sets_wide_bilinear        once per side: a fixed grid of persistent workgroups of kAwWaves waves; a unit (set,
//                                     tile, chunk) is found by a binary search in the side's prefix.  Per unit the workgroup
//                                     stages the chunk's coefficients in LDS (between two barriers), then takes the tile in
//                                     kSetsWbTrips trips of kAwBlockRows entries: an eight-lane group takes kAwRows entries,
//                                     set_row[p] - row_base range-checked against [0, N) before anything is addressed through
//                                     it; an entry past the end of the set or outside the shard reads row 0 and is not
//                                     counted.  Lane 0 of a group compares with the true key, the wave counts by ballot into
//                                     scalar counters and adds them once per unit with 64-bit integer atomics (gt low word,
//                                     ge high word): nothing depends on the grid.
//   4. sets_wb_finalize               64 queries per workgroup: the filter entries whose row is in the query's set
//                                     (SetLookup: binary search in the sorted set) re-scored by wide_pair_score, eight
//                                     entries per step, and subtracted; one int4 of counts per query.
// Every lane of every wave calls wide_trip / wide_pair_score (their folds read neighbouring lanes by DPP), and every wave of a
// workgroup reaches the two barriers of every unit: the only early exits are wave-uniform and inside the trip loop, which has
// no barrier.  No kernel uses scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knobs.h"
#include "launch.h"
#include "rank_common.h"
#include "score_core.h"
#include "table_elem.h"
#include "wide_bilinear.h"
#include "wide_bilinear_keys.h"

#pragma clang fp contract(off)

namespace blp {

namespace {

constexpr int kSetsWbTrips = 4;                             // trips of a tile
constexpr int kSetsWbTile = kSetsWbTrips * kAwBlockRows;    // entries of a set per work unit
constexpr int kSetsWbGridPerCu = 2;                         // persistent workgroups per compute unit
constexpr int kSetsWbScanThreads = 1024;

__host__ __device__ inline int64_t sets_wb_chunks(int64_t n_queries) { return n_queries > 0 ? (n_queries + kAwQueries - 1) / kAwQueries : 0; }

// ------------------------------------------------------------------------------------------------ 2. work units
// prefix_head[g] / prefix_tail[g]: the units of sets 0 .. g - 1 of that side; entry G: the side's total
__global__ __launch_bounds__(kSetsWbScanThreads) void sets_wb_unit_prefix_kernel(const int64_t* __restrict__ set_ptr,
                                                                                 const int64_t* __restrict__ qptr_head,
                                                                                 const int64_t* __restrict__ qptr_tail, int64_t G,
                                                                                 int64_t* __restrict__ prefix_head,
                                                                                 int64_t* __restrict__ prefix_tail) {
    __shared__ int64_t wave_sum[2][kSetsWbScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry_h = 0, carry_t = 0;
    for (int64_t g0 = 0; g0 < G; g0 += kSetsWbScanThreads) {  // workgroup-uniform
        const int64_t g = g0 + tid;
        int64_t units_h = 0, units_t = 0;
        if (g < G) {
            const int64_t n = set_ptr[g + 1] - set_ptr[g];
            const int64_t tiles = n > 0 ? (n + kSetsWbTile - 1) / kSetsWbTile : 0;
            units_h = tiles * sets_wb_chunks(qptr_head[g + 1] - qptr_head[g]);
            units_t = tiles * sets_wb_chunks(qptr_tail[g + 1] - qptr_tail[g]);
        }
        int64_t incl_h = units_h, incl_t = units_t;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t up_h = __shfl_up(incl_h, off), up_t = __shfl_up(incl_t, off);
            if (lane >= off) { incl_h += up_h; incl_t += up_t; }
        }
        if (lane == 63) { wave_sum[0][wave] = incl_h; wave_sum[1][wave] = incl_t; }
        __syncthreads();
        int64_t before_h = carry_h, before_t = carry_t, total_h = 0, total_t = 0;
        for (int w = 0; w < kSetsWbScanThreads / 64; ++w) {
            if (w < wave) { before_h += wave_sum[0][w]; before_t += wave_sum[1][w]; }
            total_h += wave_sum[0][w];
            total_t += wave_sum[1][w];
        }
        if (g < G) {
            prefix_head[g] = before_h + incl_h - units_h;
            prefix_tail[g] = before_t + incl_t - units_t;
        }
        carry_h += total_h;
        carry_t += total_t;
        __syncthreads();
    }
    if (tid == 0) { prefix_head[G] = carry_h; prefix_tail[G] = carry_t; }
}

// ------------------------------------------------------------------------------------------------ 3. the ranking kernel
// prefix: the side's.  Everything that steers the unit loop -- the unit, its set, tile and chunk -- is workgroup-uniform.
template <int MODEL, int SIDE, bool CASCADE>
__global__ __launch_bounds__(kAwWaves * 64) void rank_sets_wide_bilinear_kernel(const float* __restrict__ table, int64_t N, int64_t ld,
                                                                                int D, const QRows q_fixed, const QRows q_rel,
                                                                                const float* __restrict__ key_true, int64_t q_head,
                                                                                const SetLookup sets, const int64_t* __restrict__ prefix,
                                                                                unsigned long long* __restrict__ acc_out) {
    constexpr int QC = kAwQueries, R = kAwRows;
    extern __shared__ __attribute__((aligned(16))) float wb_coef[];  // [query of the chunk][K][n4]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 3, sub = lane & 7;
    const int64_t* __restrict__ qptr = SIDE == HEAD ? sets.qptr_head : sets.qptr_tail;
    const int64_t G = sets.G, n_units = prefix[G];
    for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        int64_t g_lo = 0, g_hi = G;  // prefix[g_lo] <= unit < prefix[g_hi]: the last set that starts at or before the unit
        while (g_hi - g_lo > 1) {
            const int64_t mid = (g_lo + g_hi) >> 1;
            if (prefix[mid] <= unit) g_lo = mid; else g_hi = mid;
        }
        const int64_t g = g_lo;
        const int64_t p0 = sets.set_ptr[g], p1 = sets.set_ptr[g + 1], s0 = qptr[g], s1 = qptr[g + 1];
        const int64_t chunks = sets_wb_chunks(s1 - s0);  // (> 0: the set has units)
        const int64_t local = unit - prefix[g], tile = local / chunks, chunk = local - tile * chunks;
        const int64_t sq0 = s0 + chunk * QC;                              // the chunk's first query within its side
        const int live_q = (int)(s1 - sq0 < QC ? s1 - sq0 : QC);
        const int64_t q0 = (SIDE == HEAD ? 0 : q_head) + sq0;            // ... within the call
        __syncthreads();  // the previous unit's coefficients have been read
        wide_stage_coef<MODEL, SIDE>(wb_coef, q_fixed, q_rel, q0, live_q, D);
        __syncthreads();
        float kt[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) kt[q] = key_true[q0 + (q < live_q ? q : 0)];
        unsigned cgt[QC], cge[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) cgt[q] = cge[q] = 0;

        const int64_t t_lo = p0 + tile * kSetsWbTile, t_end = t_lo + kSetsWbTile < p1 ? t_lo + kSetsWbTile : p1;
        for (int64_t pb = t_lo + wave * (8 * R); pb < t_end; pb += kAwBlockRows) {  // wave-uniform; no barrier inside
            const float* base[R];  // the group's rows (masked entries: row 0, not counted; N > 0)
            bool live[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t p = pb + grp + 8 * r;
                const int64_t row = p < t_end ? sets.set_row[p] - sets.row_base : -1;
                live[r] = (uint64_t)row < (uint64_t)N;
                base[r] = table + (live[r] ? row : 0) * ld;
            }
            bool any = false;
#pragma unroll
            for (int r = 0; r < R; ++r) any = any || live[r];
            if (!__ballot(any)) continue;  // the wave's entries all outside the shard (wave-uniform: the whole wave skips the trip)
            float s[QC][R];
            wide_trip<MODEL, SIDE, CASCADE>(s, base, wb_coef, D, sub);
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

// ------------------------------------------------------------------------------------------------ 4. filter + finalize
// wide_bilinear_filter_finalize_kernel (rank_all_wide.hip) with sets_wide_finalize_kernel's membership test: a workgroup
// owns 64 queries, its waves take the ones that have filter entries in turn -- eight entries per step, eight lanes each; an
// entry whose row is not in the query's set is masked out of the comparison, never out of wide_pair_score --, thread q writes
// query q's four counts.  use_sets false (nothing was ranked): the filter removes nothing.
template <int MODEL>
__global__ __launch_bounds__(256) void sets_wb_finalize_kernel(const float* __restrict__ table, int64_t N, int64_t ld, int D,
                                                               const QRows q_fixed, const QRows q_rel, const float* __restrict__ key_true,
                                                               int64_t q_head, int64_t Q, const FilterSpec filter, const SetLookup sets,
                                                               bool use_sets, const unsigned long long* __restrict__ acc,
                                                               int32_t* __restrict__ counts) {
    __shared__ int list[kSweepQueries], n_list;
    __shared__ unsigned removed[kSweepQueries][2];
    const int64_t q_base = (int64_t)blockIdx.x * kSweepQueries;
    const int lane = threadIdx.x & 63, grp = lane >> 3, sub = lane & 7;
    if (threadIdx.x < 64) {
        const int64_t q = q_base + lane;
        const bool any = filter.on() && use_sets && q < Q && filter.hi[q] > filter.lo[q];
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
        int64_t s_lo, s_hi;
        sets.set_of(q, q_head, s_lo, s_hi);
        unsigned gt = 0, ge = 0;
        for (int64_t k0 = lo; k0 < hi; k0 += 8) {  // wave-uniform
            int64_t row = k0 + grp < hi ? filter_row(filter, q, k0 + grp, N) : -1;
            if (row >= 0 && !sets.contains(s_lo, s_hi, row + sets.row_base)) row = -1;
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

// ------------------------------------------------------------------------------------------------ host side
struct SetsWbWorkspace {
    float* key_true;
    unsigned long long* acc;
    int64_t* prefix_head;
    int64_t* prefix_tail;
    size_t bytes;
};

SetsWbWorkspace carve_sets_wb(void* base, int64_t q_head, int64_t q_tail, int64_t G) {
    SetsWbWorkspace w;
    char* p = static_cast<char*>(base);
    const int64_t Q = q_head + q_tail;
    size_t off = 0;
    w.key_true = reinterpret_cast<float*>(p + off);       off = align_up(off + (size_t)Q * 4, 256);
    w.acc = reinterpret_cast<unsigned long long*>(p + off); off = align_up(off + (size_t)Q * 8, 256);
    w.prefix_head = reinterpret_cast<int64_t*>(p + off);  off = align_up(off + (size_t)(G + 1) * 8, 256);
    w.prefix_tail = reinterpret_cast<int64_t*>(p + off);  off = align_up(off + (size_t)(G + 1) * 8, 256);
    w.bytes = off;
    return w;
}

template <int MODEL, int SIDE>
hipError_t launch_sets_wb_side(const float* table, int64_t N, int64_t ld, int D, const QRows& q_fixed, const QRows& q_rel,
                               const float* key_true, int64_t q_head, int64_t nq, const SetLookup& sets, const int64_t* prefix,
                               unsigned long long* acc, unsigned grid, hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    const int n = MODEL == DISTMULT ? D : D / 2, n4 = (n + 3) & ~3;
    const size_t lds = (size_t)kAwQueries * WideTerm<MODEL, SIDE>::K * n4 * sizeof(float);  // <= 64 KiB: K n4 <= 2 D
    if (n >= 512)
        rank_sets_wide_bilinear_kernel<MODEL, SIDE, true><<<grid, kAwWaves * 64, lds, stream>>>(table, N, ld, D, q_fixed, q_rel, key_true,
                                                                                                q_head, sets, prefix, acc);
    else
        rank_sets_wide_bilinear_kernel<MODEL, SIDE, false><<<grid, kAwWaves * 64, lds, stream>>>(table, N, ld, D, q_fixed, q_rel, key_true,
                                                                                                 q_head, sets, prefix, acc);
    return hipGetLastError();
}

template <int MODEL>
hipError_t rank_sets_wb_impl(const float* table, int D, int64_t N, int64_t ld, const QRows& q_fixed, const QRows& q_rel,
                             const QRows& q_true, int64_t q_head, int64_t q_tail, const SetLookup& sets, int64_t nnz,
                             const FilterSpec& filter, int32_t* counts, const SetsWbWorkspace& w, int n_cu, hipStream_t stream) {
    const int64_t Q = q_head + q_tail;
    const bool ranked = N > 0 && nnz > 0 && sets.G > 0;
    const int64_t key_blocks = (Q + 31) / 32;
    wide_bilinear_true_key_kernel<MODEL><<<(unsigned)(key_blocks < 65536 ? key_blocks : 65536), 256, 0, stream>>>(
        D, q_fixed, q_rel, q_true, q_head, Q, w.key_true, w.acc);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    if (ranked) {
        sets_wb_unit_prefix_kernel<<<1, kSetsWbScanThreads, 0, stream>>>(sets.set_ptr, sets.qptr_head, sets.qptr_tail, sets.G, w.prefix_head,
                                                                         w.prefix_tail);
        if ((err = hipGetLastError()) != hipSuccess) return err;
        // persistent workgroups (knob rank_sets_grid: any other number -- the counts are integer sums over the units)
        int64_t grid = (int64_t)(n_cu > 0 ? n_cu : 1) * kSetsWbGridPerCu;
        if (const long long forced = knob(KNOB_RANK_SETS_GRID); forced > 0 && forced < (1ll << 20)) grid = forced;
        err = launch_sets_wb_side<MODEL, HEAD>(table, N, ld, D, q_fixed, q_rel, w.key_true, q_head, q_head, sets, w.prefix_head, w.acc,
                                               (unsigned)grid, stream);
        if (err != hipSuccess) return err;
        err = launch_sets_wb_side<MODEL, TAIL>(table, N, ld, D, q_fixed, q_rel, w.key_true, q_head, q_tail, sets, w.prefix_tail, w.acc,
                                               (unsigned)grid, stream);
        if (err != hipSuccess) return err;
    }
    sets_wb_finalize_kernel<MODEL><<<(unsigned)((Q + kSweepQueries - 1) / kSweepQueries), 256, 0, stream>>>(
        table, N, ld, D, q_fixed, q_rel, w.key_true, q_head, Q, filter, sets, ranked, w.acc, counts);
    return hipGetLastError();
}

}  // namespace

bool rank_sets_wide_bilinear_supported(int model, int dtype, int D) {
    return (model == DISTMULT || model == COMPLEX || model == SIMPLE) && dtype == kTableF32 && D >= 4 && D <= kAwMaxD && D % 4 == 0;
}

size_t rank_sets_wide_bilinear_workspace_bytes(int64_t q_head, int64_t q_tail, int64_t G) {
    return carve_sets_wb(nullptr, q_head, q_tail, G).bytes;
}

hipError_t launch_rank_sets_wide_bilinear(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, const QRows q_fixed,
                                          const QRows q_rel, const QRows q_true, int64_t q_head, int64_t q_tail, const SetLookup& sets,
                                          int64_t nnz, const FilterSpec& filter, int32_t* counts, void* workspace, int n_cu,
                                          hipStream_t stream) {
    if (!rank_sets_wide_bilinear_supported(model, dtype, D)) return hipErrorInvalidValue;
    if (q_head + q_tail == 0) return hipSuccess;
    const SetsWbWorkspace w = carve_sets_wb(workspace, q_head, q_tail, sets.G);
    const float* t = static_cast<const float*>(table);
    if (model == DISTMULT)
        return rank_sets_wb_impl<DISTMULT>(t, D, N, ld, q_fixed, q_rel, q_true, q_head, q_tail, sets, nnz, filter, counts, w, n_cu, stream);
    if (model == COMPLEX)
        return rank_sets_wb_impl<COMPLEX>(t, D, N, ld, q_fixed, q_rel, q_true, q_head, q_tail, sets, nnz, filter, counts, w, n_cu, stream);
    return rank_sets_wb_impl<SIMPLE>(t, D, N, ld, q_fixed, q_rel, q_true, q_head, q_tail, sets, nnz, filter, counts, w, n_cu, stream);
}

}  // namespace blp
