// topk_sets_wide.hip -- filtered, deterministic top-k prediction inside candidate sets SHARED between queries for TransE at
// ANY width (include/blp_hip.h: blp_topk_sets_wide): D % 4 == 0, 4 <= D <= 1024 -- the BOW / DKRL encoders' 300 and 768, where
// topk_sets_kernel.h's layout (a lane holds a whole set row in D VGPRs, one code object per width) does not fit.  The contract
// is blp_topk_sets_typed's word for word: the sets CSR of strictly ascending global rows, row_base shards, the query grouping,
// the filter rules, the (Q, k) rows and scores -- descending score, ties by ascending row, NaN last, -1 / quiet NaN beyond the
// entries left; scores are the reference's f32 score_fn bit for bit (on a 16-bit table: of the table widened to f32).
//
// The kernel joins two halves the tree already has.  The arithmetic is rank_sets_wide.hip's (sets_wide_sums.h): for a wave's 64
// gathered set rows and a chunk of up to 16 queries of one side the reference's running sums at run-time width, in 64-column
// slabs with pieces of 32 / 16 / 8 / 4 at the end of a row, 16-bit rows through tile16.h.  The selection is topk_sets.hip's
// (topk_lists.h, topk_sets_kernel.h): 64-bit keys, per-(wave, query) sorted lists in LDS, unfiltered_rows on the lanes above a
// list's threshold, the fold of the four waves' lists, the (Q, S_max, k) partial buffer.  topk_rels_wide_kernel
// (rank_rels_wide.hip) is the precedent for the join: -acc[j] goes straight into topk_key.
//
// Kernels of one call (one code object for every width: D is a kernel argument; nothing about set or group sizes is known on
// the host):
//   1. topk_sets_wide_coef    the coefficient rows, rank_sets_wide's: head-replacing [r | t] (2 D floats), tail-replacing h + r
//                             (D floats, rounded once as the reference's first operation).  There is no true row in this call:
//                             no true keys, no accumulators.
//   2. the partial buffer cleared: (Q, S_max, k) keys, 0 = an empty slot
//   3. topk_sets_unit_prefix  (topk_sets.hip) the exclusive prefix over the sets of chunks_g x slabs_g with
//                             q_chunk = min(topk_chunk(k), 16): 16 for k <= 48, 12 at k = 64, 4 at k = 192, 3 at k = 256.
//                             S_max is topk_sets_slabs_rule's with that q_chunk: from Q, k and nnz alone.
//   4. topk_sets_wide         a fixed grid of persistent workgroups (knob topk_sets_grid: any other number); workgroup b takes
//                             units b, b + gridDim.x, ... and finds (set, slab, chunk) by a binary search in the prefix.  Wave w
//                             takes tiles slab x 4 + w, + slabs_g x 4, ... of the set.  Entries past the end of the set or
//                             outside [row_base, row_base + N) are masked (key 0) and read a valid lane's row; set_row is
//                             range-checked before anything is addressed through it; a tile without a valid entry is skipped.
//                             The chunk loop is fully unrolled: the sums are never dynamically indexed.  The workgroup folds its
//                             four waves' lists and writes the k keys to slot (query, slab) of the partial buffer.
//   5. topk_merge<keys>       (topk.hip) per query the k best of its S_max lists -> rows / scores
// There is NO re-scoring kernel and none is needed: every chain starts from a literal 0.0f and adds in ascending d, so -acc IS
// score_fn's value, and the key carries it exactly -- sign of zero included (the key's low bit), NaN as 0x7fc00000.  The
// device tests hold it to that on the bits.  A query's top k are its k largest keys, a set that does not depend on the order
// the keys are seen in: the result does not depend on the grid.  No kernel of this file uses scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knobs.h"
#include "launch.h"
#include "rank_common.h"
#include "score_core.h"
#include "sets_wide_sums.h"
#include "table_elem.h"
#include "tile.h"
#include "tile16.h"
#include "topk_lists.h"
#include "topk_sets_kernel.h"

#pragma clang fp contract(off)

namespace blp {

static_assert(kTopkWaves == kWaves, "one LDS transpose slab per wave of the workgroup");

// ------------------------------------------------------------------------------------------------ 1. coefficient rows
__global__ __launch_bounds__(256) void topk_sets_wide_coef_kernel(const QRows q_fixed, const QRows q_rel, int D, int64_t q_head,
                                                                  int64_t Q, float* __restrict__ coef_head,
                                                                  float* __restrict__ coef_tail) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
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

// ------------------------------------------------------------------------------------------------ 4. the selection kernel
template <class TE>  // TE: the candidate table's storage type (table_elem.h); ld in elements
__global__ __launch_bounds__(kTopkWaves * 64, 2) void topk_sets_wide_kernel(
    const TE* __restrict__ table, int64_t N, int64_t ld, int D, const float* __restrict__ coef_head,
    const float* __restrict__ coef_tail, int64_t q_head, const SetLookup sets, const int64_t* __restrict__ prefix, int q_chunk,
    int s_max, int k, const FilterSpec filter, u64* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    float* slab = smem + wave * kSlabFloats;
    u64* lists_all = reinterpret_cast<u64*>(smem + kTopkWaves * kSlabFloats);
    u64* lists = lists_all + (size_t)wave * q_chunk * k;

    const int64_t G = sets.G, n_units = prefix[G];
    for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {  // workgroup-uniform
        int64_t g_lo = 0, g_hi = G;  // prefix[g_lo] <= unit < prefix[g_hi]: the last set that starts at or before the unit
        while (g_hi - g_lo > 1) {
            const int64_t mid = (g_lo + g_hi) >> 1;
            if (prefix[mid] <= unit) g_lo = mid; else g_hi = mid;
        }
        const int64_t g = wide_uniform64(g_lo);
        const int64_t p0 = sets.set_ptr[g], p1 = sets.set_ptr[g + 1];
        const int64_t h0 = sets.qptr_head[g], h1 = sets.qptr_head[g + 1], t0 = sets.qptr_tail[g], t1 = sets.qptr_tail[g + 1];
        const int64_t ch_head = topk_sets_chunks(h1 - h0, q_chunk), chunks = ch_head + topk_sets_chunks(t1 - t0, q_chunk);
        const int64_t n_tiles = (p1 - p0 + kTileRows - 1) / kTileRows;
        const int64_t n_slabs = topk_sets_slabs_of(p1 - p0, s_max);
        const int64_t local = unit - prefix[g], s = local / chunks, chunk = local - s * chunks;
        const bool head = chunk < ch_head;
        // the chunk's queries: [q0, q0 + nq) of the call, side query number s0 (its coefficient row)
        const int64_t s0 = wide_uniform64(head ? h0 + chunk * q_chunk : t0 + (chunk - ch_head) * q_chunk);
        const int64_t left = (head ? h1 : t1) - s0;
        const int nq = __builtin_amdgcn_readfirstlane((int)(left < q_chunk ? left : q_chunk));
        const int64_t q0 = wide_uniform64(head ? s0 : q_head + s0);

        for (int i = lane; i < nq * k; i += 64) lists[i] = 0ull;
        wave_lds_sync();

        for (int64_t t = s * kTopkWaves + wave; t < n_tiles; t += n_slabs * kTopkWaves) {
            // the wave's 64 entries of the set -> rows of this shard
            const int64_t p = wide_uniform64(p0 + t * kTileRows) + lane;
            const int64_t row = p < p1 ? sets.set_row[p] - sets.row_base : -1;
            const bool valid = (uint64_t)row < (uint64_t)N;
            const u64 vmask = __ballot(valid);
            if (!vmask) continue;  // (wave-uniform; the workgroup barriers are outside this loop)
            int lrow = (int)row;  // N < 2^31
            const int first_valid = __shfl(lrow, __builtin_ctzll(vmask));  // (every lane takes part in the shuffle)
            if (!valid) lrow = first_valid;

            float acc[kSetsWideChunk];
            if (head) sets_wide_sums<HEAD, TE>(acc, table, ld, lrow, coef_head + s0 * 2 * D, nq, D, slab, lane);
            else sets_wide_sums<TAIL, TE>(acc, table, ld, lrow, coef_tail + s0 * D, nq, D, slab, lane);

            static_for<kSetsWideChunk>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                if (j < nq) {
                    const u64 key = valid ? topk_key(-acc[j], sets.row_base + lrow) : 0ull;
                    list_offer(lists + j * k, k, key, lane,
                               [&](u64 m) { return filter.on() ? unfiltered_rows(filter, q0 + j, N, lrow, m, lane) : m; });
                }
            });
        }

        __syncthreads();
        // fold the other waves' lists into wave 0's, query j by wave j % kTopkWaves; write the unit's list
        for (int j = wave; j < nq; j += kTopkWaves) {
            u64* L = lists_all + (size_t)j * k;
            for (int w = 1; w < kTopkWaves; ++w) {
                const u64* src = lists_all + ((size_t)w * q_chunk + j) * k;
                for (int c = 0; c < k; c += 64)
                    list_offer(L, k, c + lane < k ? src[c + lane] : 0ull, lane, [](u64 m) { return m; });
            }
            u64* out = partial + ((size_t)(q0 + j) * s_max + s) * k;
            for (int i = lane; i < k; i += 64) out[i] = L[i];
        }
        __syncthreads();  // the lists are zeroed again by their own waves only after every fold has read them
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool topk_sets_wide_supported(int model, int dtype, int D, int k) {
    return model == TRANSE && (dtype == kTableF32 || dtype == kTableF16 || dtype == kTableBF16) && D >= 4 && D <= kSetsWideMaxD &&
           D % 4 == 0 && k >= 1 && k <= kTopkMaxK;
}

namespace {
// queries per work unit: what the lists' LDS holds at this k (topk_lists.h: topk_chunk), at most one running sum per lane each
int topk_sets_wide_chunk(int k) {
    const int c = topk_chunk(k);
    return c < kSetsWideChunk ? c : kSetsWideChunk;
}

struct TopkSetsWideWorkspace {
    float* coef_head;
    float* coef_tail;
    int64_t* prefix;
    u64* partial;
    size_t partial_bytes;
    size_t bytes;
};

TopkSetsWideWorkspace carve_topk_sets_wide(void* base, int D, int64_t q_head, int64_t q_tail, int64_t G, int64_t nnz, int k) {
    TopkSetsWideWorkspace w;
    char* p = static_cast<char*>(base);
    const int64_t Q = q_head + q_tail;
    size_t off = 0;
    w.coef_head = reinterpret_cast<float*>(p + off); off = align_up(off + (size_t)q_head * 2 * D * 4, 256);
    w.coef_tail = reinterpret_cast<float*>(p + off); off = align_up(off + (size_t)q_tail * D * 4, 256);
    w.prefix = reinterpret_cast<int64_t*>(p + off);  off = align_up(off + (size_t)(G + 1) * 8, 256);
    w.partial = reinterpret_cast<u64*>(p + off);
    w.partial_bytes = (size_t)Q * topk_sets_slabs_rule(Q, nnz, topk_sets_wide_chunk(k)) * k * 8;
    // reserved: a bound of it that never shrinks when Q, nnz or k grow (Q x S_max itself does: S_max falls as the chunks
    // multiply) -- Q x S_max <= kTopkTargetGroups x q_chunk wherever S_max > 1, q_chunk x k <= min(16 k, the lists' LDS in
    // keys per wave), and S_max <= the cap of topk_sets_slabs_rule
    const size_t cap = (size_t)(((nnz + kTileRows - 1) / kTileRows + kTopkWaves - 1) / kTopkWaves);
    const size_t chunk_keys = (size_t)(kSetsWideChunk * k < kTopkListBytes / (kTopkWaves * 8) ? kSetsWideChunk * k : kTopkListBytes / (kTopkWaves * 8));
    size_t keys = (size_t)kTopkTargetGroups * chunk_keys;
    if (keys > (size_t)Q * cap * k) keys = (size_t)Q * cap * k;
    if (keys < (size_t)Q * k) keys = (size_t)Q * k;
    off = align_up(off + keys * 8, 256);
    w.bytes = off;
    return w;
}

template <class TE>
hipError_t topk_sets_wide_pass(const TE* table, int64_t N, int64_t ld, int D, const TopkSetsWideWorkspace& w, int64_t q_head,
                               const SetLookup& sets, int q_chunk, int s_max, int k, const FilterSpec& filter, int n_cu,
                               hipStream_t stream) {
    // persistent workgroups, two per compute unit: what the kernel's LDS lets reside (knob topk_sets_grid: any other number --
    // a query's keys are a set, the result does not depend on it)
    int64_t grid = (int64_t)(n_cu > 0 ? n_cu : 1) * 2;
    if (const long long forced = knob(KNOB_TOPK_SETS_GRID); forced > 0 && forced < (1ll << 20)) grid = forced;
    const size_t lds = (size_t)kTopkWaves * kSlabFloats * 4 + (size_t)kTopkWaves * q_chunk * k * 8;
    topk_sets_wide_kernel<TE><<<dim3((unsigned)grid), kTopkWaves * 64, lds, stream>>>(table, N, ld, D, w.coef_head, w.coef_tail, q_head, sets,
                                                                                   w.prefix, q_chunk, s_max, k, filter, w.partial);
    return hipGetLastError();
}
}  // namespace

size_t topk_sets_wide_workspace_bytes(int D, int64_t q_head, int64_t q_tail, int64_t G, int64_t nnz, int k) {
    return carve_topk_sets_wide(nullptr, D, q_head, q_tail, G, nnz, k).bytes;
}

hipError_t launch_topk_sets_wide(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, const QRows q_fixed,
                                 const QRows q_rel, int64_t q_head, int64_t q_tail, int k, const SetLookup& sets, int64_t nnz,
                                 const FilterSpec& filter, int64_t* rows, float* scores, void* workspace, int n_cu, hipStream_t stream) {
    if (!topk_sets_wide_supported(model, dtype, D, k)) return hipErrorInvalidValue;
    const int64_t Q = q_head + q_tail;
    if (Q == 0) return hipSuccess;
    const TopkSetsWideWorkspace w = carve_topk_sets_wide(workspace, D, q_head, q_tail, sets.G, nnz, k);
    if (N == 0 || nnz == 0 || sets.G == 0)  // every slot empty
        return launch_topk_merge_keys(w.partial, Q, 0, k, rows, scores, stream);
    const int q_chunk = topk_sets_wide_chunk(k);
    const int s_max = (int)topk_sets_slabs_rule(Q, nnz, q_chunk);
    const int64_t prep_items = Q * (D / 4);
    const unsigned prep_grid = (unsigned)((prep_items + 255) / 256 < 65536 ? (prep_items + 255) / 256 : 65536);
    topk_sets_wide_coef_kernel<<<prep_grid, 256, 0, stream>>>(q_fixed, q_rel, D, q_head, Q, w.coef_head, w.coef_tail);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    if ((err = hipMemsetAsync(w.partial, 0, w.partial_bytes, stream)) != hipSuccess) return err;
    if ((err = launch_topk_sets_unit_prefix(sets, q_chunk, s_max, w.prefix, stream)) != hipSuccess) return err;
    if (dtype == kTableF32)
        err = topk_sets_wide_pass(static_cast<const float*>(table), N, ld, D, w, q_head, sets, q_chunk, s_max, k, filter, n_cu, stream);
    else if (dtype == kTableF16)
        err = topk_sets_wide_pass(static_cast<const _Float16*>(table), N, ld, D, w, q_head, sets, q_chunk, s_max, k, filter, n_cu, stream);
    else
        err = topk_sets_wide_pass(static_cast<const __bf16*>(table), N, ld, D, w, q_head, sets, q_chunk, s_max, k, filter, n_cu, stream);
    if (err != hipSuccess) return err;
    return launch_topk_merge_keys(w.partial, Q, (int64_t)s_max * k, k, rows, scores, stream);
}

}  // namespace blp
