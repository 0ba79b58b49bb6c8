// rank_sets.hip -- rank link-prediction queries against candidate SETS that many queries share (include/blp_hip.h:
// blp_rank_sets): type-constrained evaluation (a head query of relation r against the entities seen as heads of r), per-type
// or per-language pools, a first stage that proposes one pool for a group of queries.  G sets as a CSR of sorted global table
// rows; within each side the queries are grouped by set (qset_ptr_head / qset_ptr_tail give each set's run of queries).
//
// Kernels of one call (all on the caller's stream, nothing about set or group sizes is known on the host):
//   1. true keys + zeroed accumulators, coefficient rows   rank_all.hip's launch_true_keys / launch_prep_coef, unchanged
//   2. sets_unit_prefix   one workgroup: the exclusive prefix over the sets of tiles_g x chunks_g -- tiles_g = workgroup
//                         tiles of kWaves x kTileRows entries of set g, chunks_g = the <= kQueryChunk-query chunks of its
//                         head run plus those of its tail run -- G + 1 values in the workspace
//   3. rank_sets          a fixed grid of persistent workgroups; workgroup b takes units b, b + gridDim.x, ... and finds
//                         (set, tile, chunk) of a unit by a binary search in the prefix.  A unit is rank_tiles_kernel's body
//                         (rank_tiles.h) over a GATHERED tile: lane l of a wave holds entry l of the wave's 64 entries of
//                         set_row, the rows are fetched in whole 128-byte lines (tile.h: tile_fetch_from, the row of a
//                         line taken per 8-lane group) and transposed through the wave's LDS slab; then the chunk's queries
//                         run past them -- TransE from the scalar cache (score_batch_transe_sgpr), the bilinear models from
//                         LDS-staged coefficient rows (apply_queries).  A chunk is of one side only.  Entries past the end
//                         of the set or outside [row_base, row_base + N) are masked (valid = false) and read a valid
//                         lane's row.  Each wave adds its packed gt | ge << 32 sums to the queries' 64-bit accumulators
//                         with integer atomics: the result does not depend on the grid.
//   4. filter + finalize  rank_all.hip's filter_finalize_kernel with one more condition (SetLookup): a filter entry is
//                         re-scored and subtracted only if its row is in the query's set (binary search in the sorted set).
// No kernel uses scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knobs.h"
#include "launch.h"
#include "rank_common.h"
#include "rank_tiles.h"
#include "score_core.h"
#include "tile.h"

#pragma clang fp contract(off)

namespace blp {

typedef unsigned long long u64;

constexpr int kUnitScanThreads = 1024;

__device__ __forceinline__ int64_t uniform64(int64_t v) {  // a wave-uniform value, into scalar registers
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((u64)v & 0xffffffffull));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((u64)v >> 32));
    return (int64_t)(((u64)hi << 32) | lo);
}

__host__ __device__ inline int64_t set_chunks(int64_t n_queries) { return n_queries > 0 ? (n_queries + kQueryChunk - 1) / kQueryChunk : 0; }

__global__ __launch_bounds__(kUnitScanThreads) void sets_unit_prefix_kernel(const int64_t* __restrict__ set_ptr,
                                                                            const int64_t* __restrict__ qptr_head,
                                                                            const int64_t* __restrict__ qptr_tail, int64_t G,
                                                                            int64_t* __restrict__ prefix) {
    __shared__ int64_t wave_sum[kUnitScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = 0;
    for (int64_t g0 = 0; g0 < G; g0 += kUnitScanThreads) {  // workgroup-uniform
        const int64_t g = g0 + tid;
        int64_t units = 0;
        if (g < G) {
            const int64_t n = set_ptr[g + 1] - set_ptr[g];
            const int64_t tiles = n > 0 ? (n + kWaves * kTileRows - 1) / (kWaves * kTileRows) : 0;
            units = tiles * (set_chunks(qptr_head[g + 1] - qptr_head[g]) + set_chunks(qptr_tail[g + 1] - qptr_tail[g]));
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
        for (int w = 0; w < kUnitScanThreads / 64; ++w) {
            if (w < wave) before += wave_sum[w];
            total += wave_sum[w];
        }
        if (g < G) prefix[g] = before + incl - units;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) prefix[G] = carry;
}

template <int MODEL, int D>
__global__ __launch_bounds__(kWaves * 64, (D == 256 ? 1 : (MODEL == TRANSE ? 3 : 2))) void rank_sets_kernel(
    const float* __restrict__ table, int64_t N, int64_t ld, const float* __restrict__ coef_head,
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
            tile_fetch_from<D, false>(e, [&](auto ii) {
                constexpr int i = decltype(ii)::value;
                return table + (int64_t)__shfl(lrow, 8 * i + sub_row) * ld + sub_col;
            });
            tile_transpose<D>(e, slab, lane);
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
bool rank_sets_supported(int model, int D) { return model >= TRANSE && model <= SIMPLE && (D == 64 || D == 128 || D == 256); }

struct SetsWorkspace {
    float* key_true;
    u64* acc;
    float* coef_head;
    float* coef_tail;
    int64_t* prefix;
    size_t bytes;
};

static SetsWorkspace carve_sets(void* base, int D, int64_t q_head, int64_t q_tail, int64_t G) {
    SetsWorkspace w;
    char* p = static_cast<char*>(base);
    const int64_t Q = q_head + q_tail;
    size_t off = 0;
    w.key_true = reinterpret_cast<float*>(p + off);  off = align_up(off + (size_t)Q * 4, 256);
    w.acc = reinterpret_cast<u64*>(p + off);         off = align_up(off + (size_t)Q * 8, 256);
    w.coef_head = reinterpret_cast<float*>(p + off); off = align_up(off + (size_t)q_head * max_coef(D) * 4, 256);
    w.coef_tail = reinterpret_cast<float*>(p + off); off = align_up(off + (size_t)q_tail * max_coef(D) * 4, 256);
    w.prefix = reinterpret_cast<int64_t*>(p + off);  off = align_up(off + (size_t)(G + 1) * 8, 256);
    w.bytes = off;
    return w;
}

size_t rank_sets_workspace_bytes(int D, int64_t q_head, int64_t q_tail, int64_t G) { return carve_sets(nullptr, D, q_head, q_tail, G).bytes; }

template <int MODEL, int D>
static hipError_t rank_sets_pass(const float* table, int64_t N, int64_t ld, const SetsWorkspace& w, int64_t q_head, const SetLookup& sets,
                                 int n_cu, hipStream_t stream) {
    // persistent workgroups, three per compute unit as rank_tiles' resident set (knob rank_sets_grid: any other number -- the
    // counts are integer sums over the units and do not depend on it)
    int64_t grid = (int64_t)(n_cu > 0 ? n_cu : 1) * 3;
    if (const long long forced = knob(KNOB_RANK_SETS_GRID); forced > 0 && forced < (1ll << 20)) grid = forced;
    const size_t lds = (size_t)kWaves * kSlabFloats * 4 + (size_t)2 * kQB * kMaxCoef(D) * 4 + (size_t)kWaves * 2 * kQueryChunk * 4;
    rank_sets_kernel<MODEL, D><<<dim3((unsigned)grid), kWaves * 64, lds, stream>>>(table, N, ld, w.coef_head, w.coef_tail, w.key_true,
                                                                                   q_head, sets, w.prefix, w.acc);
    return hipGetLastError();
}

hipError_t launch_rank_sets(int model, int D, const float* table, int64_t N, int64_t ld, const QRows q_fixed, const QRows q_rel,
                            const QRows q_true, int64_t q_head, int64_t q_tail, const SetLookup& sets, int64_t nnz,
                            const FilterSpec& filter, int32_t* counts, void* workspace, int n_cu, hipStream_t stream) {
    if (!rank_sets_supported(model, D)) return hipErrorInvalidValue;
    if (q_head + q_tail == 0) return hipSuccess;
    const SetsWorkspace w = carve_sets(workspace, D, q_head, q_tail, sets.G);
    hipError_t err = launch_true_keys(model, D, q_fixed, q_rel, q_head, q_tail, q_true, w.key_true, w.acc, stream);
    if (err != hipSuccess) return err;
    if (N > 0 && nnz > 0 && sets.G > 0) {
        if ((err = launch_prep_coef(model, D, q_fixed, q_rel, q_head, q_tail, w.coef_head, w.coef_tail, stream)) != hipSuccess) return err;
        sets_unit_prefix_kernel<<<1, kUnitScanThreads, 0, stream>>>(sets.set_ptr, sets.qptr_head, sets.qptr_tail, sets.G, w.prefix);
        if ((err = hipGetLastError()) != hipSuccess) return err;
#define BLP_SETS_CASE(M, DD) \
    if (model == M && D == DD) err = rank_sets_pass<M, DD>(table, N, ld, w, q_head, sets, n_cu, stream);
#define BLP_SETS_MODEL(M) BLP_SETS_CASE(M, 64) BLP_SETS_CASE(M, 128) BLP_SETS_CASE(M, 256)
        BLP_SETS_MODEL(TRANSE) BLP_SETS_MODEL(DISTMULT) BLP_SETS_MODEL(COMPLEX) BLP_SETS_MODEL(SIMPLE)
#undef BLP_SETS_MODEL
#undef BLP_SETS_CASE
        if (err != hipSuccess) return err;
    }
    if (!filter.on() || N == 0 || nnz == 0 || sets.G == 0)  // (nothing to remove from: a plain unpack of the accumulators)
        return launch_filter_finalize(model, D, table, N, ld, q_fixed, q_rel, w.key_true, q_head, q_tail, FilterSpec(), w.acc, counts, stream);
    return launch_filter_finalize_sets(model, D, table, N, ld, q_fixed, q_rel, w.key_true, q_head, q_tail, filter, sets, w.acc, counts,
                                       stream);
}

}  // namespace blp
