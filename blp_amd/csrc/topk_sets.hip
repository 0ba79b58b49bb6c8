// topk_sets.hip -- filtered, deterministic top-k prediction INSIDE candidate sets that queries share (include/blp_hip.h:
// blp_topk_sets): blp_topk's selection (topk.hip: 64-bit keys, per-(wave, query) sorted LDS lists; topk_lists.h) over
// blp_rank_sets' sets, grouping and gathered tiles (rank_sets.hip).  "The 10 best tails of (h, r, ?) among the entities that
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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knobs.h"
#include "launch.h"
#include "rank_common.h"
#include "score_core.h"
#include "tile.h"
#include "topk_lists.h"

#pragma clang fp contract(off)

namespace blp {

constexpr int kTopkSetsScanThreads = 1024;

__device__ __forceinline__ int64_t topk_sets_uniform(int64_t v) {  // a wave-uniform value, into scalar registers
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((u64)v & 0xffffffffull));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((u64)v >> 32));
    return (int64_t)(((u64)hi << 32) | lo);
}

__host__ __device__ inline int64_t topk_sets_chunks(int64_t n_queries, int q_chunk) {
    return n_queries > 0 ? (n_queries + q_chunk - 1) / q_chunk : 0;
}
// slabs of a set of n > 0 entries
__host__ __device__ inline int64_t topk_sets_slabs_of(int64_t n, int s_max) {
    const int64_t tiles = (n + kTileRows - 1) / kTileRows;
    const int64_t s = (tiles + kTopkWaves - 1) / kTopkWaves;
    return s < 1 ? 1 : (s > s_max ? s_max : s);
}

// S_max, the partial lists per query: n_slabs x (a lower bound of the chunks) <= max(chunks, kTopkTargetGroups), and at
// most one per kTopkWaves tiles of all the sets' entries together -- topk_slabs' rule (topk.hip) with nnz in N's place.
static int64_t topk_sets_slabs(int64_t Q, int64_t nnz, int k) {
    const int64_t chunks = (Q + topk_chunk(k) - 1) / topk_chunk(k);
    const int64_t tiles = (nnz + kTileRows - 1) / kTileRows;
    int64_t s = chunks > 0 ? kTopkTargetGroups / chunks : 1;
    const int64_t cap = (tiles + kTopkWaves - 1) / kTopkWaves;
    if (s > cap) s = cap;
    return s < 1 ? 1 : s;
}

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

// nq queries of one side, q0 .. (the call's numbering), against the wave's gathered tile; coef = the coefficient row of q0
template <int MODEL, int SIDE, int D>
__device__ __forceinline__ void topk_sets_side(const float (&e)[D], bool valid, int lrow, int64_t row_base, int64_t N,
                                               const float* __restrict__ coef, int64_t q0, int nq, u64* lists, int k,
                                               const FilterSpec& f, int lane) {
    using S = Scorer<MODEL, SIDE, D>;
    for (int j = 0; j < nq; ++j) {
        const float s = S::template score<false>(e, PtrCoef{coef + (int64_t)j * S::C});
        const u64 key = valid ? topk_key(s, row_base + lrow) : 0ull;
        list_offer(lists + j * k, k, key, lane, [&](u64 m) { return f.on() ? unfiltered_rows(f, q0 + j, N, lrow, m, lane) : m; });
    }
}

template <int MODEL, int D>
__global__ __launch_bounds__(kTopkWaves * 64, (D == 256 ? 1 : 2)) void topk_sets_kernel(
    const float* __restrict__ table, int64_t N, int64_t ld, const float* __restrict__ coef_head,
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
        const int64_t g = topk_sets_uniform(g_lo);
        const int64_t p0 = sets.set_ptr[g], p1 = sets.set_ptr[g + 1];
        const int64_t h0 = sets.qptr_head[g], h1 = sets.qptr_head[g + 1], t0 = sets.qptr_tail[g], t1 = sets.qptr_tail[g + 1];
        const int64_t ch_head = topk_sets_chunks(h1 - h0, q_chunk), chunks = ch_head + topk_sets_chunks(t1 - t0, q_chunk);
        const int64_t n_tiles = (p1 - p0 + kTileRows - 1) / kTileRows;
        const int64_t n_slabs = topk_sets_slabs_of(p1 - p0, s_max);
        const int64_t local = unit - prefix[g], s = local / chunks, chunk = local - s * chunks;
        const bool head = chunk < ch_head;
        // the chunk's queries: [q0, q0 + nq) of the call, side query number s0 (its coefficient row)
        const int64_t s0 = topk_sets_uniform(head ? h0 + chunk * q_chunk : t0 + (chunk - ch_head) * q_chunk);
        const int64_t left = (head ? h1 : t1) - s0;
        const int nq = __builtin_amdgcn_readfirstlane((int)(left < q_chunk ? left : q_chunk));
        const int64_t q0 = head ? s0 : q_head + s0;

        for (int i = lane; i < nq * k; i += 64) lists[i] = 0ull;
        wave_lds_sync();

        for (int64_t t = s * kTopkWaves + wave; t < n_tiles; t += n_slabs * kTopkWaves) {
            // the wave's 64 entries of the set -> rows of this shard
            const int64_t p = topk_sets_uniform(p0 + t * kTileRows) + lane;
            const int64_t row = p < p1 ? sets.set_row[p] - sets.row_base : -1;
            const bool valid = (uint64_t)row < (uint64_t)N;
            const u64 vmask = __ballot(valid);
            if (!vmask) continue;
            int lrow = (int)row;  // N < 2^31
            if (!valid) lrow = __shfl(lrow, __builtin_ctzll(vmask));
            float e[D];
            const int sub_row = lane >> 3, sub_col = (lane & 7) * 4;
            tile_fetch_from<D, false>(e, [&](auto ii) {
                constexpr int i = decltype(ii)::value;
                return table + (int64_t)__shfl(lrow, 8 * i + sub_row) * ld + sub_col;
            });
            tile_transpose<D>(e, slab, lane);
            if (head)
                topk_sets_side<MODEL, HEAD, D>(e, valid, lrow, sets.row_base, N, coef_head + s0 * Scorer<MODEL, HEAD, D>::C, q0, nq,
                                               lists, k, filter, lane);
            else
                topk_sets_side<MODEL, TAIL, D>(e, valid, lrow, sets.row_base, N, coef_tail + s0 * Scorer<MODEL, TAIL, D>::C, q0, nq,
                                               lists, k, filter, lane);
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
bool topk_sets_supported(int model, int D, int k) { return topk_supported(model, D, k); }

struct TopkSetsWorkspace {
    float* coef_head;
    float* coef_tail;
    int64_t* prefix;
    u64* partial;
    size_t partial_bytes;
    size_t bytes;
};

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

template <int MODEL, int D>
static hipError_t topk_sets_pass(const float* table, int64_t N, int64_t ld, const TopkSetsWorkspace& w, int64_t q_head,
                                 const SetLookup& sets, int q_chunk, int s_max, int k, const FilterSpec& filter, int n_cu,
                                 hipStream_t stream) {
    // persistent workgroups, as many per compute unit as the kernel's registers and LDS let reside (knob topk_sets_grid: any
    // other number -- a query's keys are a set, the result does not depend on it)
    int64_t grid = (int64_t)(n_cu > 0 ? n_cu : 1) * (D == 256 ? 1 : 2);
    if (const long long forced = knob(KNOB_TOPK_SETS_GRID); forced > 0 && forced < (1ll << 20)) grid = forced;
    const size_t lds = (size_t)kTopkWaves * kSlabFloats * 4 + (size_t)kTopkWaves * q_chunk * k * 8;
    topk_sets_kernel<MODEL, D><<<dim3((unsigned)grid), kTopkWaves * 64, lds, stream>>>(
        table, N, ld, w.coef_head, w.coef_tail, q_head, sets, w.prefix, q_chunk, s_max, k, filter, w.partial);
    return hipGetLastError();
}

hipError_t launch_topk_sets(int model, int D, const float* table, int64_t N, int64_t ld, const QRows q_fixed, const QRows q_rel,
                            int64_t q_head, int64_t q_tail, int k, const SetLookup& sets, int64_t nnz, const FilterSpec& filter,
                            int64_t* rows, float* scores, void* workspace, int n_cu, hipStream_t stream) {
    if (!topk_sets_supported(model, D, k)) return hipErrorInvalidValue;
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
    topk_sets_unit_prefix_kernel<<<1, kTopkSetsScanThreads, 0, stream>>>(sets.set_ptr, sets.qptr_head, sets.qptr_tail, sets.G, q_chunk,
                                                                         s_max, w.prefix);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    err = hipErrorInvalidValue;
#define BLP_TOPK_SETS_CASE(M, DD) \
    if (model == M && D == DD) err = topk_sets_pass<M, DD>(table, N, ld, w, q_head, sets, q_chunk, s_max, k, filter, n_cu, stream);
#define BLP_TOPK_SETS_MODEL(M) BLP_TOPK_SETS_CASE(M, 64) BLP_TOPK_SETS_CASE(M, 128) BLP_TOPK_SETS_CASE(M, 256)
    BLP_TOPK_SETS_MODEL(TRANSE) BLP_TOPK_SETS_MODEL(DISTMULT) BLP_TOPK_SETS_MODEL(COMPLEX) BLP_TOPK_SETS_MODEL(SIMPLE)
#undef BLP_TOPK_SETS_MODEL
#undef BLP_TOPK_SETS_CASE
    if (err != hipSuccess) return err;
    if ((err = launch_topk_merge_keys(w.partial, Q, (int64_t)s_max * k, k, rows, scores, stream)) != hipSuccess) return err;
    return launch_topk_rescore(model, D, table, ld, sets.row_base, q_fixed, q_rel, q_head, Q, k, rows, scores, stream);
}

}  // namespace blp
