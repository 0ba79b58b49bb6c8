// topk_sets.hip -- filtered, deterministic top-k prediction INSIDE candidate sets that queries share (include/blp_hip.h:
// blp_topk_sets, blp_topk_sets_typed): blp_topk's selection (topk.hip: 64-bit keys, per-(wave, query) sorted LDS lists;
// topk_lists.h) over blp_rank_sets' sets, grouping and gathered tiles (rank_sets.hip).  "The 10 best tails of (h, r, ?) among the entities that
// can be a tail of r": a row of a set is fetched once per (set, chunk of topk_chunk(k) queries of its group), no score is
// written out and nothing is sorted.
//
// Kernels of one call (all on the caller's stream, nothing about set or group sizes is known on the host):
//   1. prep_coef             (rank_all.hip) the queries' coefficient rows
//   2. the partial buffer cleared: (Q, S_max, k) keys, 0 = an empty slot -- the slots no unit writes (queries of empty sets,
//                            sets of fewer than S_max slabs) must read as empty
//   3. topk_sets_unit_prefix one workgroup: the exclusive prefix over the sets of chunks_g x slabs_g -- chunks_g = the
//                            <= topk_chunk(k)-query chunks of set g's head run plus those of its tail run, slabs_g =
//                            clamp(ceil(tiles_g / kTopkWaves), 1, S_max) over its tiles_g wave tiles of 64 entries; 0 for a
//                            set without entries or without queries -- G + 1 values in the workspace.  S_max comes from Q, k
//                            and nnz alone (topk_sets_slabs: few queries against long sets still fill the device).
//   4. topk_sets             a fixed grid of persistent workgroups; workgroup b takes units b, b + gridDim.x, ... and finds
//                            (set, chunk, slab) of a unit by a binary search in the prefix.  A unit is topk_tiles' body over
//                            GATHERED tiles: wave w takes tiles slab x kTopkWaves + w, + slabs_g x kTopkWaves, ... of the set;
//                            lane l holds entry l of the tile's 64 entries of set_row, the rows fetched in whole 128-byte
//                            lines and transposed through the wave's LDS slab exactly as rank_sets_kernel does.  Entries past
//                            the end of the set or outside [row_base, row_base + N) are masked (key 0) and read a valid
//                            lane's row.  The chunk's queries (one side only) run past the tile with Scorer<>::score<false>
//                            on their coefficient rows (wave-uniform: scalar loads); lanes above a list's threshold are
//                            checked against the query's filter segment (unfiltered_rows: each admitted lane's OWN row, one
//                            shuffle per lane) and inserted.  The workgroup folds its four waves' lists and writes the k keys
//                            to slot (query, slab) of the partial buffer.
//   5. topk_merge<keys>      (topk.hip) per query the k best of its S_max lists -> rows / scores
//   6. topk_rescore          (topk.hip) the winners re-scored with the reference's literal-zero additions (sign of zero)
// The top k of a query are its k largest keys -- a set that does not depend on the order the keys are seen in, so the result
// does not depend on the grid (knob topk_sets_grid).  No kernel of this file uses scratch memory.
//
// A 16-BIT TABLE (blp_topk_sets_typed; table_elem.h).  Kernel 4 is a template over the table's storage type
// (topk_sets_kernel.h): the f32 instantiations are this file's, the IEEE half / bfloat16 ones topk_sets16.hip's
// (launch_topk_sets_pass16), their tiles fetched and widened through tile16.h; kernel 6 re-scores the widened rows
// (topk_rescore_kernel<MODEL, D, T>, launch_topk_rescore_typed).  Kernels 1, 2, 3 and 5 do not read the table and are the
// same whatever its type; so is the workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knobs.h"
#include "launch.h"
#include "rank_common.h"
#include "score_core.h"
#include "table_elem.h"
#include "tile.h"
#include "topk_lists.h"
#include "topk_sets_kernel.h"

#pragma clang fp contract(off)

namespace blp {

constexpr int kTopkSetsScanThreads = 1024;

// S_max, the partial lists per query: topk_sets_slabs_rule (topk_sets_kernel.h) for chunks of topk_chunk(k) queries
static int64_t topk_sets_slabs(int64_t Q, int64_t nnz, int k) { return topk_sets_slabs_rule(Q, nnz, topk_chunk(k)); }

__global__ __launch_bounds__(kTopkSetsScanThreads) void topk_sets_unit_prefix_kernel(const int64_t* __restrict__ set_ptr,
                                                                                     const int64_t* __restrict__ qptr_head,
                                                                                     const int64_t* __restrict__ qptr_tail,
                                                                                     int64_t G, int q_chunk, int s_max,
                                                                                     int64_t* __restrict__ prefix) {
    __shared__ int64_t wave_sum[kTopkSetsScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = 0;
    for (int64_t g0 = 0; g0 < G; g0 += kTopkSetsScanThreads) {  // workgroup-uniform
        const int64_t g = g0 + tid;
        int64_t units = 0;
        if (g < G) {
            const int64_t n = set_ptr[g + 1] - set_ptr[g];
            if (n > 0)
                units = topk_sets_slabs_of(n, s_max) * (topk_sets_chunks(qptr_head[g + 1] - qptr_head[g], q_chunk) +
                                                        topk_sets_chunks(qptr_tail[g + 1] - qptr_tail[g], q_chunk));
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
        for (int w = 0; w < kTopkSetsScanThreads / 64; ++w) {
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
hipError_t launch_topk_sets_unit_prefix(const SetLookup& sets, int q_chunk, int s_max, int64_t* prefix, hipStream_t stream) {
    topk_sets_unit_prefix_kernel<<<1, kTopkSetsScanThreads, 0, stream>>>(sets.set_ptr, sets.qptr_head, sets.qptr_tail, sets.G, q_chunk,
                                                                         s_max, prefix);
    return hipGetLastError();
}

bool topk_sets_supported(int model, int D, int k) { return topk_supported(model, D, k); }
bool topk_sets_typed_supported(int model, int dtype, int D, int k) {
    return (dtype == kTableF32 || dtype == kTableF16 || dtype == kTableBF16) && topk_sets_supported(model, D, k);
}

static TopkSetsWorkspace carve_topk_sets(void* base, int D, int64_t q_head, int64_t q_tail, int64_t G, int64_t nnz, int k) {
    TopkSetsWorkspace w;
    char* p = static_cast<char*>(base);
    const int64_t Q = q_head + q_tail;
    size_t off = 0;
    w.coef_head = reinterpret_cast<float*>(p + off); off = align_up(off + (size_t)q_head * max_coef(D) * 4, 256);
    w.coef_tail = reinterpret_cast<float*>(p + off); off = align_up(off + (size_t)q_tail * max_coef(D) * 4, 256);
    w.prefix = reinterpret_cast<int64_t*>(p + off);  off = align_up(off + (size_t)(G + 1) * 8, 256);
    w.partial = reinterpret_cast<u64*>(p + off);
    w.partial_bytes = (size_t)Q * topk_sets_slabs(Q, nnz, k) * k * 8;
    // reserved: a bound of it that never shrinks when Q, nnz or k grow (Q x S_max itself does: S_max falls as the chunks
    // multiply) -- Q x S_max <= kTopkTargetGroups x topk_chunk(k) wherever S_max > 1, and S_max <= the cap of topk_sets_slabs
    const size_t cap = (size_t)(((nnz + kTileRows - 1) / kTileRows + kTopkWaves - 1) / kTopkWaves);
    const size_t chunk_keys = (size_t)(kTopkMaxChunk * k < kTopkListBytes / (kTopkWaves * 8) ? kTopkMaxChunk * k : kTopkListBytes / (kTopkWaves * 8));
    size_t keys = (size_t)kTopkTargetGroups * chunk_keys;
    if (keys > (size_t)Q * cap * k) keys = (size_t)Q * cap * k;
    if (keys < (size_t)Q * k) keys = (size_t)Q * k;
    off = align_up(off + keys * 8, 256);
    w.bytes = off;
    return w;
}

size_t topk_sets_workspace_bytes(int model, int D, int64_t q_head, int64_t q_tail, int64_t G, int64_t nnz, int k) {
    if (!topk_sets_supported(model, D, k) || q_head < 0 || q_tail < 0 || G < 0 || nnz < 0) return 0;
    return carve_topk_sets(nullptr, D, q_head, q_tail, G, nnz, k).bytes;
}

hipError_t launch_topk_sets(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, const QRows q_fixed,
                            const QRows q_rel, int64_t q_head, int64_t q_tail, int k, const SetLookup& sets, int64_t nnz,
                            const FilterSpec& filter, int64_t* rows, float* scores, void* workspace, int n_cu, hipStream_t stream) {
    if (!topk_sets_typed_supported(model, dtype, D, k)) return hipErrorInvalidValue;
    const int64_t Q = q_head + q_tail;
    if (Q == 0) return hipSuccess;
    const TopkSetsWorkspace w = carve_topk_sets(workspace, D, q_head, q_tail, sets.G, nnz, k);
    if (N == 0 || nnz == 0 || sets.G == 0)  // every slot empty
        return launch_topk_merge_keys(w.partial, Q, 0, k, rows, scores, stream);
    const int q_chunk = topk_chunk(k);
    const int s_max = (int)topk_sets_slabs(Q, nnz, k);
    hipError_t err = launch_prep_coef(model, D, q_fixed, q_rel, q_head, q_tail, w.coef_head, w.coef_tail, stream);
    if (err != hipSuccess) return err;
    if ((err = hipMemsetAsync(w.partial, 0, w.partial_bytes, stream)) != hipSuccess) return err;
    if ((err = launch_topk_sets_unit_prefix(sets, q_chunk, s_max, w.prefix, stream)) != hipSuccess) return err;
    err = hipErrorInvalidValue;
    if (dtype != kTableF32) {
        err = launch_topk_sets_pass16(model, D, dtype, table, N, ld, w, q_head, sets, q_chunk, s_max, k, filter, n_cu, stream);
    } else {
        const float* table32 = static_cast<const float*>(table);
#define BLP_TOPK_SETS_CASE(M, DD) \
    if (model == M && D == DD) err = topk_sets_pass<M, DD>(table32, N, ld, w, q_head, sets, q_chunk, s_max, k, filter, n_cu, stream);
#define BLP_TOPK_SETS_MODEL(M) BLP_TOPK_SETS_CASE(M, 64) BLP_TOPK_SETS_CASE(M, 128) BLP_TOPK_SETS_CASE(M, 256)
        BLP_TOPK_SETS_MODEL(TRANSE) BLP_TOPK_SETS_MODEL(DISTMULT) BLP_TOPK_SETS_MODEL(COMPLEX) BLP_TOPK_SETS_MODEL(SIMPLE)
#undef BLP_TOPK_SETS_MODEL
#undef BLP_TOPK_SETS_CASE
    }
    if (err != hipSuccess) return err;
    if ((err = launch_topk_merge_keys(w.partial, Q, (int64_t)s_max * k, k, rows, scores, stream)) != hipSuccess) return err;
    return launch_topk_rescore_typed(model, D, dtype, table, ld, sets.row_base, q_fixed, q_rel, q_head, Q, k, rows, scores, stream);
}

}  // namespace blp
