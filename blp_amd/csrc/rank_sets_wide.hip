// rank_sets_wide.hip -- rank against candidate sets SHARED between queries for TransE at ANY width (include/blp_hip.h:
// blp_rank_sets_wide): D % 4 == 0, 4 <= D <= 1024 -- the BOW / DKRL encoders' 300 and 768, where rank_sets_kernel.h's layout (a
// lane holds a whole set row in D VGPRs, one code object per width) does not fit.  The contract is blp_rank_sets_typed's word
// for word: the sets CSR of strictly ascending global rows, row_base shards, the query grouping, the filter and true-entity
// rules, the (Q, 4) counts -- the reference's bit for bit (on a 16-bit table: of the table widened to f32).
//
// Layout: rank_rels_wide.hip's, turned to gathered set rows.  A wave owns 64 entries of a set, one per lane, as
// rank_sets_kernel.h gathers them, but holds only a SLAB of kSetsWideCols = 64 columns of the row in VGPRs at a time: f32 rows
// in whole 128-byte lines (tile.h: tile_fetch_from, the row of a line taken per 8-lane group, transposed through the wave's LDS
// slab), 16-bit rows in whole 128-byte lines of 64 columns (tile16.h), widened after the transpose.  What stays resident across
// the slabs is one f32 running sum per query of the unit's chunk of kSetsWideChunk = 16 queries, all of one side:
//     head-replacing   acc = acc + |(e[d] + r[d]) - t[d]|        tail-replacing   acc = acc + |c[d] - e[d]|, c = h + r
// in ascending d, r / t / c wave-uniform (scalar loads from the query's coefficient row, one SGPR operand per VALU
// instruction).  TransE's sum is strictly left to right (score_direct.h), so the sum carried from slab to slab is the
// reference's running sum at every column and -acc after the last one is score_fn's value bit for bit; every chain starts from
// a literal 0.0f.  The last slab may be partial (300 = 4 x 64 + 44): the columns left are taken in pieces of 32 / 16 / 8 / 4
// read straight from the lane's row (16-byte loads; a 16-bit row: 8-byte loads, widened as they are read).  The chunk loop is
// fully unrolled: the sums are never dynamically indexed, nothing lives in scratch.
//
// Kernels of one call (one code object for every width: D is a kernel argument; nothing about set or group sizes is known on
// the host):
//   1. sets_wide_prep         true keys (score_direct<TRANSE> on the query's rows), zeroed accumulators, the coefficient rows:
//                             head-replacing [r | t] (2 D floats), tail-replacing h + r (D floats, rounded once as the
//                             reference's first operation)
//   2. sets_wide_unit_prefix  one workgroup: the exclusive prefix over the sets of tiles_g x chunks_g, tiles_g = workgroup tiles
//                             of kWaves x 64 entries, chunks_g = the <= 16-query chunks of the head run plus those of the tail run
//   3. rank_sets_wide         a fixed grid of persistent workgroups; a unit (set, tile, chunk) is found by a binary search in
//                             the prefix.  Entries past the end of the set or outside [row_base, row_base + N) are masked and
//                             read a valid lane's row; set_row is range-checked before anything is addressed through it.
//                             Each wave adds its packed gt | ge << 32 sums to the queries' 64-bit accumulators with integer
//                             atomics: nothing depends on the grid.
//   4. sets_wide_finalize     one wave per query: the filter entries whose row is in the query's set (SetLookup: binary search
//                             in the sorted set) re-scored by score_direct<TRANSE> and subtracted; counts written.
// No kernel uses scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "knobs.h"
#include "launch.h"
#include "rank_common.h"
#include "score_core.h"
#include "score_direct.h"
#include "sets_wide_sums.h"
#include "table_elem.h"
#include "tile.h"
#include "tile16.h"

#pragma clang fp contract(off)

namespace blp {

constexpr int kSetsWideTile = kWaves * kTileRows;  // entries of a set per work unit
constexpr int kSetsWideGridPerCu = 3;              // persistent workgroups per compute unit: what the f32 kernel's registers let reside
constexpr int kSetsWideScanThreads = 1024;

static_assert(kSetsWideChunk <= 64, "one lane per query of the chunk adds the wave's sums");

__host__ __device__ inline int64_t sets_wide_chunks(int64_t n_queries) {
    return n_queries > 0 ? (n_queries + kSetsWideChunk - 1) / kSetsWideChunk : 0;
}

// ------------------------------------------------------------------------------------------------ 1. preparation
__global__ __launch_bounds__(256) void sets_wide_prep_kernel(const QRows q_fixed, const QRows q_rel, const QRows q_true, int D,
                                                             int64_t q_head, int64_t Q, float* __restrict__ key_true,
                                                             u64* __restrict__ acc, float* __restrict__ coef_head,
                                                             float* __restrict__ coef_tail) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    for (int64_t q = i0; q < Q; q += stride) {
        acc[q] = 0;
        const float* e = q_true.row(q);
        const float* f = q_fixed.row(q);
        const float* r = q_rel.row(q);
        key_true[q] = q < q_head ? score_direct<TRANSE>(e, f, r, D) : score_direct<TRANSE>(f, e, r, D);
    }
    const int D4 = D / 4;
    for (int64_t i = i0; i < Q * D4; i += stride) {
        const int64_t q = i / D4;
        const int c = (int)(i - q * D4) * 4;
        const float4 f = *reinterpret_cast<const float4*>(q_fixed.row(q) + c);
        const float4 r = *reinterpret_cast<const float4*>(q_rel.row(q) + c);
        if (q < q_head) {
            float* row = coef_head + q * 2 * D;
            *reinterpret_cast<float4*>(row + c) = r;
            *reinterpret_cast<float4*>(row + D + c) = f;
        } else {
            *reinterpret_cast<float4*>(coef_tail + (q - q_head) * D + c) = make_float4(f.x + r.x, f.y + r.y, f.z + r.z, f.w + r.w);
        }
    }
}

// ------------------------------------------------------------------------------------------------ 2. work units
__global__ __launch_bounds__(kSetsWideScanThreads) void sets_wide_unit_prefix_kernel(const int64_t* __restrict__ set_ptr,
                                                                                     const int64_t* __restrict__ qptr_head,
                                                                                     const int64_t* __restrict__ qptr_tail, int64_t G,
                                                                                     int64_t* __restrict__ prefix) {
    __shared__ int64_t wave_sum[kSetsWideScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = 0;
    for (int64_t g0 = 0; g0 < G; g0 += kSetsWideScanThreads) {  // workgroup-uniform
        const int64_t g = g0 + tid;
        int64_t units = 0;
        if (g < G) {
            const int64_t n = set_ptr[g + 1] - set_ptr[g];
            const int64_t tiles = n > 0 ? (n + kSetsWideTile - 1) / kSetsWideTile : 0;
            units = tiles * (sets_wide_chunks(qptr_head[g + 1] - qptr_head[g]) + sets_wide_chunks(qptr_tail[g + 1] - qptr_tail[g]));
        }
        int64_t incl = units;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int64_t before = carry, total = 0;
        for (int w = 0; w < kSetsWideScanThreads / 64; ++w) {
            if (w < wave) before += wave_sum[w];
            total += wave_sum[w];
        }
        if (g < G) prefix[g] = before + incl - units;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) prefix[G] = carry;
}

// ------------------------------------------------------------------------------------------------ 3. the ranking kernel
// (the running sums -- sets_wide_sums<SIDE, TE> and its helpers -- are sets_wide_sums.h's, shared with topk_sets_wide.hip)
template <class TE>  // TE: the candidate table's storage type (table_elem.h); ld in elements
__global__ __launch_bounds__(kWaves * 64, 2) void rank_sets_wide_kernel(const TE* __restrict__ table, int64_t N, int64_t ld, int D,
                                                                        const float* __restrict__ coef_head,
                                                                        const float* __restrict__ coef_tail,
                                                                        const float* __restrict__ key_true, int64_t q_head,
                                                                        const SetLookup sets, const int64_t* __restrict__ prefix,
                                                                        u64* __restrict__ acc_out) {
    __shared__ __attribute__((aligned(16))) float slabs[kWaves * kSlabFloats];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    float* slab = slabs + wave * kSlabFloats;

    const int64_t G = sets.G, n_units = prefix[G];
    for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        int64_t g_lo = 0, g_hi = G;  // prefix[g_lo] <= unit < prefix[g_hi]: the last set that starts at or before the unit
        while (g_hi - g_lo > 1) {
            const int64_t mid = (g_lo + g_hi) >> 1;
            if (prefix[mid] <= unit) g_lo = mid; else g_hi = mid;
        }
        const int64_t g = wide_uniform64(g_lo);
        const int64_t p0 = sets.set_ptr[g], p1 = sets.set_ptr[g + 1];
        const int64_t h0 = sets.qptr_head[g], h1 = sets.qptr_head[g + 1], t0 = sets.qptr_tail[g], t1 = sets.qptr_tail[g + 1];
        const int64_t ch_head = sets_wide_chunks(h1 - h0), chunks = ch_head + sets_wide_chunks(t1 - t0);
        const int64_t local = unit - prefix[g], tile = local / chunks, chunk = local - tile * chunks;
        const bool head = chunk < ch_head;
        // the chunk's queries: [q0, q0 + nq) of the call, side query number s0 (its coefficient row)
        const int64_t s0 = wide_uniform64(head ? h0 + chunk * kSetsWideChunk : t0 + (chunk - ch_head) * kSetsWideChunk);
        const int64_t left = (head ? h1 : t1) - s0;
        const int nq = __builtin_amdgcn_readfirstlane((int)(left < kSetsWideChunk ? left : kSetsWideChunk));
        const int64_t q0 = wide_uniform64(head ? s0 : q_head + s0);

        // the wave's 64 entries of the set -> rows of this shard
        const int64_t p = wide_uniform64(p0 + (tile * kWaves + wave) * kTileRows) + lane;
        const int64_t row = p < p1 ? sets.set_row[p] - sets.row_base : -1;
        const bool valid = (uint64_t)row < (uint64_t)N;
        const u64 vmask = __ballot(valid);
        if (!vmask) continue;  // (wave-uniform; no workgroup barrier anywhere in the loop)
        int lrow = (int)row;  // N < 2^31
        const int first_valid = __shfl(lrow, __builtin_ctzll(vmask));  // (every lane takes part in the shuffle)
        if (!valid) lrow = first_valid;

        float acc[kSetsWideChunk];
        if (head) sets_wide_sums<HEAD, TE>(acc, table, ld, lrow, coef_head + s0 * 2 * D, nq, D, slab, lane);
        else sets_wide_sums<TAIL, TE>(acc, table, ld, lrow, coef_tail + s0 * D, nq, D, slab, lane);

        u64 mine = 0;  // lane j: the wave's packed sums of query q0 + j
        static_for<kSetsWideChunk>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            if (j < nq) {
                const float s = -acc[j], kt = key_true[q0 + j];
                const u64 gt = __popcll(__ballot(valid && s > kt)), ge = __popcll(__ballot(valid && s >= kt));
                if (lane == j) mine = gt | (ge << 32);
            }
        });
        if (lane < nq && mine) atomicAdd(acc_out + q0 + lane, mine);
    }
}

// ------------------------------------------------------------------------------------------------ 4. filter + finalize
// One wave per query.  Lane l takes the query's filter entries l, l + 64, ...: an entry whose row is in this shard and in the
// query's set is re-scored from its row (widened exactly) and counted if it scores above / at least the true entity.
template <class TE>
__global__ __launch_bounds__(256) void sets_wide_finalize_kernel(const TE* __restrict__ table, int64_t N, int64_t ld, int D,
                                                                 const QRows q_fixed, const QRows q_rel,
                                                                 const float* __restrict__ key_true, int64_t q_head, int64_t Q,
                                                                 const FilterSpec filter, const SetLookup sets, bool use_sets,
                                                                 const u64* __restrict__ acc, int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t q = wide_uniform64(blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6));
    if (q >= Q) return;
    unsigned fgt = 0, fge = 0;
    if (filter.on() && use_sets) {
        const int64_t lo = filter.lo[q], hi = filter.hi[q];
        if (lo < hi) {
            int64_t s_lo, s_hi;
            sets.set_of(q, q_head, s_lo, s_hi);
            const float* f = q_fixed.row(q);
            const float* r = q_rel.row(q);
            const float kt = key_true[q];
            const bool head = q < q_head;
            for (int64_t k0 = lo; k0 < hi; k0 += 64) {  // wave-uniform
                const int64_t k = k0 + lane;
                int64_t row = k < hi ? filter_row(filter, q, k, N) : -1;
                if (row >= 0 && !sets.contains(s_lo, s_hi, row + sets.row_base)) row = -1;
                bool gt = false, ge = false;
                if (row >= 0) {
                    const RowF<TE> e{table + row * ld};
                    const float key = head ? score_direct<TRANSE>(e, f, r, D) : score_direct<TRANSE>(f, e, r, D);
                    gt = key > kt;
                    ge = key >= kt;
                }
                fgt += __popcll(__ballot(gt));
                fge += __popcll(__ballot(ge));
            }
        }
    }
    if (lane == 0) {
        const u64 a = acc[q];
        const int32_t all_gt = (int32_t)(a & 0xffffffffull), all_ge = (int32_t)(a >> 32);
        reinterpret_cast<int4*>(counts)[q] = make_int4(all_gt, all_ge, all_gt - (int32_t)fgt, all_ge - (int32_t)fge);
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool rank_sets_wide_supported(int model, int dtype, int D) {
    return model == TRANSE && (dtype == kTableF32 || dtype == kTableF16 || dtype == kTableBF16) && D >= 4 && D <= kSetsWideMaxD &&
           D % 4 == 0;
}

namespace {
struct SetsWideWorkspace {
    float* key_true;
    u64* acc;
    float* coef_head;
    float* coef_tail;
    int64_t* prefix;
    size_t bytes;
};

SetsWideWorkspace carve_sets_wide(void* base, int D, int64_t q_head, int64_t q_tail, int64_t G) {
    SetsWideWorkspace w;
    char* p = static_cast<char*>(base);
    const int64_t Q = q_head + q_tail;
    size_t off = 0;
    w.key_true = reinterpret_cast<float*>(p + off);  off = align_up(off + (size_t)Q * 4, 256);
    w.acc = reinterpret_cast<u64*>(p + off);         off = align_up(off + (size_t)Q * 8, 256);
    w.coef_head = reinterpret_cast<float*>(p + off); off = align_up(off + (size_t)q_head * 2 * D * 4, 256);
    w.coef_tail = reinterpret_cast<float*>(p + off); off = align_up(off + (size_t)q_tail * D * 4, 256);
    w.prefix = reinterpret_cast<int64_t*>(p + off);  off = align_up(off + (size_t)(G + 1) * 8, 256);
    w.bytes = off;
    return w;
}

template <class TE>
hipError_t rank_sets_wide_impl(const TE* table, int D, int64_t N, int64_t ld, const QRows& q_fixed, const QRows& q_rel,
                               const QRows& q_true, int64_t q_head, int64_t q_tail, const SetLookup& sets, int64_t nnz,
                               const FilterSpec& filter, int32_t* counts, const SetsWideWorkspace& w, int n_cu, hipStream_t stream) {
    const int64_t Q = q_head + q_tail;
    const bool ranked = N > 0 && nnz > 0 && sets.G > 0;
    const int64_t prep_items = Q * (D / 4);
    const unsigned prep_grid = (unsigned)((prep_items + 255) / 256 < 65536 ? (prep_items + 255) / 256 : 65536);
    sets_wide_prep_kernel<<<prep_grid, 256, 0, stream>>>(q_fixed, q_rel, q_true, D, q_head, Q, w.key_true, w.acc, w.coef_head, w.coef_tail);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    if (ranked) {
        sets_wide_unit_prefix_kernel<<<1, kSetsWideScanThreads, 0, stream>>>(sets.set_ptr, sets.qptr_head, sets.qptr_tail, sets.G, w.prefix);
        if ((err = hipGetLastError()) != hipSuccess) return err;
        // persistent workgroups (knob rank_sets_grid: any other number -- the counts are integer sums over the units)
        int64_t grid = (int64_t)(n_cu > 0 ? n_cu : 1) * kSetsWideGridPerCu;
        if (const long long forced = knob(KNOB_RANK_SETS_GRID); forced > 0 && forced < (1ll << 20)) grid = forced;
        rank_sets_wide_kernel<TE><<<dim3((unsigned)grid), kWaves * 64, 0, stream>>>(table, N, ld, D, w.coef_head, w.coef_tail, w.key_true,
                                                                                 q_head, sets, w.prefix, w.acc);
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    sets_wide_finalize_kernel<TE><<<(unsigned)((Q + 3) / 4), 256, 0, stream>>>(table, N, ld, D, q_fixed, q_rel, w.key_true, q_head, Q, filter,
                                                                             sets, ranked, w.acc, counts);
    return hipGetLastError();
}
}  // namespace

size_t rank_sets_wide_workspace_bytes(int D, int64_t q_head, int64_t q_tail, int64_t G) {
    return carve_sets_wide(nullptr, D, q_head, q_tail, G).bytes;
}

hipError_t launch_rank_sets_wide(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, const QRows q_fixed,
                                 const QRows q_rel, const QRows q_true, int64_t q_head, int64_t q_tail, const SetLookup& sets,
                                 int64_t nnz, const FilterSpec& filter, int32_t* counts, void* workspace, int n_cu, hipStream_t stream) {
    if (!rank_sets_wide_supported(model, dtype, D)) return hipErrorInvalidValue;
    if (q_head + q_tail == 0) return hipSuccess;
    const SetsWideWorkspace w = carve_sets_wide(workspace, D, q_head, q_tail, sets.G);
#define BLP_SETS_WIDE(TT) \
    return rank_sets_wide_impl(static_cast<const TT*>(table), D, N, ld, q_fixed, q_rel, q_true, q_head, q_tail, sets, nnz, filter, counts, w, n_cu, stream);
    if (dtype == kTableF32) BLP_SETS_WIDE(float)
    if (dtype == kTableF16) BLP_SETS_WIDE(_Float16)
    BLP_SETS_WIDE(__bf16)
#undef BLP_SETS_WIDE
}

}  // namespace blp
