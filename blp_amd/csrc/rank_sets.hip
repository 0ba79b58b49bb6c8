// rank_sets.hip -- rank link-prediction queries against candidate SETS that many queries share (include/blp_hip.h:
// blp_rank_sets, blp_rank_sets_typed): type-constrained evaluation (a head query of relation r against the entities seen as heads of r), per-type
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
//
// A 16-BIT TABLE (blp_rank_sets_typed; table_elem.h).  Kernels 3 and 4 are templates over the table's storage type (3:
// rank_sets_kernel.h, 4: filter_finalize.h); this file instantiates them for f32, rank_sets16.hip for IEEE half and bfloat16.
// The 16-bit rank_sets_kernel fetches the wave's 64 gathered rows in whole 128-byte lines of 64 columns (tile16.h: the loader
// topk_tiles16 reads consecutive rows with), the row of a line taken per 8-lane group exactly as above; the 16-bit words pass
// through the slab and a lane widens its row after the transpose into the same e[D].  Everything after that, and kernels 1
// and 2 (the queries' vectors stay f32), is shared: the counts are blp_rank_sets' on the table widened to f32, bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knobs.h"
#include "launch.h"
#include "rank_common.h"
#include "rank_sets_kernel.h"

#pragma clang fp contract(off)

namespace blp {

constexpr int kUnitScanThreads = 1024;

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

// ------------------------------------------------------------------------------------------------ host side
bool rank_sets_supported(int model, int D) { return model >= TRANSE && model <= SIMPLE && (D == 64 || D == 128 || D == 256); }
bool rank_sets_typed_supported(int model, int dtype, int D) {
    return (dtype == kTableF32 || dtype == kTableF16 || dtype == kTableBF16) && rank_sets_supported(model, D);
}

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

hipError_t launch_rank_sets(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, const QRows q_fixed,
                            const QRows q_rel, const QRows q_true, int64_t q_head, int64_t q_tail, const SetLookup& sets, int64_t nnz,
                            const FilterSpec& filter, int32_t* counts, void* workspace, int n_cu, hipStream_t stream) {
    if (!rank_sets_typed_supported(model, dtype, D)) return hipErrorInvalidValue;
    if (q_head + q_tail == 0) return hipSuccess;
    const float* table32 = dtype == kTableF32 ? static_cast<const float*>(table) : nullptr;
    const SetsWorkspace w = carve_sets(workspace, D, q_head, q_tail, sets.G);
    hipError_t err = launch_true_keys(model, D, q_fixed, q_rel, q_head, q_tail, q_true, w.key_true, w.acc, stream);
    if (err != hipSuccess) return err;
    if (N > 0 && nnz > 0 && sets.G > 0) {
        if ((err = launch_prep_coef(model, D, q_fixed, q_rel, q_head, q_tail, w.coef_head, w.coef_tail, stream)) != hipSuccess) return err;
        sets_unit_prefix_kernel<<<1, kUnitScanThreads, 0, stream>>>(sets.set_ptr, sets.qptr_head, sets.qptr_tail, sets.G, w.prefix);
        if ((err = hipGetLastError()) != hipSuccess) return err;
        if (dtype != kTableF32) {
            err = launch_rank_sets_pass16(model, D, dtype, table, N, ld, w, q_head, sets, n_cu, stream);
        } else {
#define BLP_SETS_CASE(M, DD) \
    if (model == M && D == DD) err = rank_sets_pass<M, DD>(table32, N, ld, w, q_head, sets, n_cu, stream);
#define BLP_SETS_MODEL(M) BLP_SETS_CASE(M, 64) BLP_SETS_CASE(M, 128) BLP_SETS_CASE(M, 256)
            BLP_SETS_MODEL(TRANSE) BLP_SETS_MODEL(DISTMULT) BLP_SETS_MODEL(COMPLEX) BLP_SETS_MODEL(SIMPLE)
#undef BLP_SETS_MODEL
#undef BLP_SETS_CASE
        }
        if (err != hipSuccess) return err;
    }
    if (!filter.on() || N == 0 || nnz == 0 || sets.G == 0)  // (nothing to remove from: a plain unpack of the accumulators, no table read)
        return launch_filter_finalize(model, D, table32, N, ld, q_fixed, q_rel, w.key_true, q_head, q_tail, FilterSpec(), w.acc, counts, stream);
    if (dtype != kTableF32)
        return launch_filter_finalize_sets16(model, D, dtype, table, N, ld, q_fixed, q_rel, w.key_true, q_head, q_tail, filter, sets,
                                             w.acc, counts, stream);
    return launch_filter_finalize_sets(model, D, table32, N, ld, q_fixed, q_rel, w.key_true, q_head, q_tail, filter, sets, w.acc, counts,
                                       stream);
}

}  // namespace blp
