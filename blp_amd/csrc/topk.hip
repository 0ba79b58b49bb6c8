// topk.hip -- filtered, deterministic top-k entity prediction over the whole candidate table (include/blp_hip.h:
// blp_topk, blp_topk_merge): for a query (h, r, ?) / (?, r, t) the k rows with the highest score_fn value
// (models.py:222-248), without materialising the (Q, N) score matrix.
//
// Order.  Every (candidate, query) pair becomes one 64-bit KEY, larger = better:
//   high word  the score made orderable as an unsigned integer (IEEE order; -0 and +0 equal; every NaN = 1, below -inf);
//   low word   (0x7fffffff - row) << 1 | (score is -0): among equal scores the smaller row wins; the bit only carries
//              the sign of zero (rows are distinct, so it never decides);
//   key 0      an empty slot (row -1, score NaN): it sorts after everything.
// The top k of a query are the k largest keys -- a set that does not depend on the order the keys are seen in, so the
// result is deterministic whatever the grid.
//
// Kernels of one blp_topk call (all on the caller's stream):
//   1. prep_coef    (rank_all.hip) the queries' coefficient rows, as for the exact ranking kernels
//   2. topk_tiles   rank_tiles' layout: a wave owns a tile of 64 table rows, one row per lane in D VGPRs, and applies every
//                   query of its workgroup's chunk to it (Scorer<> arithmetic, coefficients as SGPR operands).  Per (wave,
//                   query) an LDS list holds the best k keys seen so far, sorted; its last entry is the admission threshold.
//                   A tile costs a query two compares and a ballot once the list is warm: only lanes above the threshold are
//                   checked against the query's filter segment (filter_row, as filter_finalize walks it) and inserted, one
//                   key at a time (each lane moves its slots of the list by one).  At the end the workgroup folds its four
//                   waves' lists into one and writes it to the workspace: (Q, n_slabs, k) keys.
//   3. topk_merge   one workgroup per query selects the k best of its n_slabs lists the same way and writes rows / scores.
//                   blp_topk_merge is this kernel on caller-given (rows, scores) lists.
//   4. topk_rescore the k rows of every query re-scored with the reference's literal "0 + first term" additions
//                   (Scorer<>::score<true>, = blp_score_fwd's arithmetic): the keys compare -0 and +0 as equal, the output
//                   carries the reference's sign of zero.
// Grid of topk_tiles: (query chunk x candidate slab), bounded: few queries against a long table -> one chunk, up to
// kTopkTargetGroups slabs grid-striding over the tiles (HBM-bound); many queries -> one slab per chunk, the table re-read from
// L2 by every chunk (VALU-bound).  Nothing is dynamically indexed in registers: lists live in LDS.
//
// A 16-BIT TABLE (blp_topk_typed; table_elem.h): topk_tiles16 is topk_tiles with another row loader, Rows16.  A row-piece is
// 64 columns per 128-byte line (rank_stream16.hip's layout): the loads and the transposing LDS slab carry the 16-bit words,
// and a lane widens its row (exactly) only after the transpose, into the same e[D] the f32 kernel scores.  The loads of a
// tile are issued when the tile is taken, as load_tile issues the f32 kernel's (loads issued one tile ahead kept
// their buffer in scratch).  topk_rescore reads the winners from the 16-bit table, widened.  The result is blp_topk's on the
// table widened to f32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "launch.h"
#include "rank_common.h"
#include "score_core.h"
#include "table_elem.h"
#include "tile.h"
#include "topk_lists.h"

#pragma clang fp contract(off)

namespace blp {

// candidate slabs per query chunk: n_slabs x n_chunks <= max(n_chunks, kTopkTargetGroups), and at most one per kTopkWaves tiles
static int64_t topk_slabs(int64_t N, int64_t Q, int k) {
    const int64_t chunks = (Q + topk_chunk(k) - 1) / topk_chunk(k);
    const int64_t tiles = (N + kTileRows - 1) / kTileRows;
    int64_t s = chunks > 0 ? kTopkTargetGroups / chunks : 1;
    const int64_t cap = (tiles + kTopkWaves - 1) / kTopkWaves;
    if (s > cap) s = cap;
    return s < 1 ? 1 : s;
}

// The lanes of `mask` whose candidate (table row row0 + lane) query q's filter segment does NOT remove: the segment is
// read 64 entries at a time (filter_row: exclude, ent2idx, row_base as filter_finalize applies them), every candidate of
// the mask looked up with one compare + ballot per chunk.
__device__ __forceinline__ u64 unfiltered(const FilterSpec& f, int64_t q, int64_t N, int64_t row0, u64 mask, int lane) {
    const int64_t lo = f.lo[q], hi = f.hi[q];
    for (int64_t c = lo; c < hi && mask; c += 64) {
        const int64_t v = c + lane < hi ? filter_row(f, q, c + lane, N) : -1;
        u64 m = mask;
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            if (__ballot(v == row0 + b)) mask &= ~(1ull << b);
        }
    }
    return mask;
}

// queries [q_lo, q_hi) of one side against the wave's tile; coef = the coefficient row of q_lo
template <int MODEL, int SIDE, int D>
__device__ __forceinline__ void topk_side(const float (&e)[D], bool valid, int64_t row0, int64_t row_base, int64_t N,
                                          const float* __restrict__ coef, int64_t q_lo, int64_t q_hi, int64_t qa, u64* lists,
                                          int k, const FilterSpec& f, int lane) {
    using S = Scorer<MODEL, SIDE, D>;
    for (int64_t q = q_lo; q < q_hi; ++q) {
        const float s = S::template score<false>(e, PtrCoef{coef + (q - q_lo) * S::C});
        const u64 key = valid ? topk_key(s, row_base + row0 + lane) : 0ull;
        list_offer(lists + (q - qa) * k, k, key, lane,
                   [&](u64 m) { return f.on() ? unfiltered(f, q, N, row0, m, lane) : m; });
    }
}

// Row loaders of the tile loop: take(e, t) puts tile t's rows in e[] (lane l <- row 64 t + l; rows past the end clamped to
// the last row, the caller masks them).
template <int D>
struct RowsF32 {  // load_tile: every load of the tile, then the transpose
    const float* __restrict__ table;
    int64_t N, ld;
    float* slab;
    int lane;
    __device__ __forceinline__ void take(float (&e)[D], int64_t t) {
        load_tile<D, false>(e, table, N, ld, t * kTileRows, slab, lane);
    }
};

// A 16-bit table (T = _Float16 / __bf16, row stride ld elements, rows 16-byte aligned): w[s][i] = this lane's 16 bytes of
// piece s (columns 64 s ..) of row 8 i + lane / 8 -- 8 rows x 128 B per instruction, as rank_stream16.hip loads them.
// (tile16.h holds the same body with the row source taken out, for rank_sets_kernel.h: a fix here belongs there too.)
template <int D, class T>
struct Rows16 {
    static constexpr int NP = D / 64;
    const char* __restrict__ table;
    int64_t N, ld;
    float* slab;
    int lane;
    uint4 w[NP][8];
    __device__ __forceinline__ void fetch(int64_t t) {
        static_for<8>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            int64_t row = t * kTileRows + 8 * i + (lane >> 3);
            row = row < N ? row : N - 1;
            const char* src = table + row * ld * 2 + (lane & 7) * 16;
            static_for<NP>([&](auto ss) {
                constexpr int s = decltype(ss)::value;
                w[s][i] = *reinterpret_cast<const uint4*>(src + s * 128);
            });
        });
    }
    __device__ __forceinline__ void take(float (&e)[D], int64_t t) {
        fetch(t);
        float* wr = slab + (lane >> 3) * kLdsStride + (lane & 7) * 4;
        const float* rd = slab + lane * kLdsStride;
        static_for<NP>([&](auto ss) {
            constexpr int s = decltype(ss)::value;
            if (s > 0) wave_lds_sync();  // the previous piece's reads are done before the slab is rewritten
            static_for<8>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                *reinterpret_cast<uint4*>(wr + 8 * i * kLdsStride) = w[s][i];
            });
            wave_lds_sync();
            static_for<8>([&](auto jj) {  // the lane's row, columns 64 s + 8 j .. + 7 (element 2 m in word m's low half)
                constexpr int j = decltype(jj)::value, c = 64 * s + 8 * j;
                const uint4 v = *reinterpret_cast<const uint4*>(rd + 4 * j);
                widen_pair<T>(v.x, e[c], e[c + 1]);
                widen_pair<T>(v.y, e[c + 2], e[c + 3]);
                widen_pair<T>(v.z, e[c + 4], e[c + 5]);
                widen_pair<T>(v.w, e[c + 6], e[c + 7]);
            });
        });
    }
};

// The body of topk_tiles over either loader.
template <int MODEL, int D, class Rows>
__device__ __forceinline__ void topk_tiles_run(Rows& rows, int64_t N, int64_t row_base, const float* __restrict__ coef_head,
                                               const float* __restrict__ coef_tail, int64_t q_head, int64_t q_tail, int q_chunk,
                                               int n_slabs, int k, const FilterSpec& filter, u64* __restrict__ partial,
                                               u64* lists_all, int wave, int lane) {
    u64* lists = lists_all + (size_t)wave * q_chunk * k;

    const int64_t chunk = blockIdx.x / n_slabs;
    const int s = blockIdx.x % n_slabs;
    const int64_t Q = q_head + q_tail;
    const int64_t qa = chunk * q_chunk, qb = qa + q_chunk < Q ? qa + q_chunk : Q;
    const int nq = (int)(qb - qa);
    const int64_t h_lo = qa < q_head ? qa : q_head, h_hi = qb < q_head ? qb : q_head;
    const int64_t t_lo = qa > q_head ? qa : q_head, t_hi = qb > q_head ? qb : q_head;
    const float* ch = coef_head + h_lo * Scorer<MODEL, HEAD, D>::C;
    const float* ct = coef_tail + (t_lo - q_head) * Scorer<MODEL, TAIL, D>::C;

    for (int i = lane; i < nq * k; i += 64) lists[i] = 0ull;
    wave_lds_sync();

    const int64_t n_tiles = (N + kTileRows - 1) / kTileRows;
    for (int64_t t = (int64_t)s * kTopkWaves + wave; t < n_tiles; t += (int64_t)n_slabs * kTopkWaves) {
        float e[D];
        const int64_t row0 = t * kTileRows;
        rows.take(e, t);
        const bool valid = row0 + lane < N;
        topk_side<MODEL, HEAD, D>(e, valid, row0, row_base, N, ch, h_lo, h_hi, qa, lists, k, filter, lane);
        topk_side<MODEL, TAIL, D>(e, valid, row0, row_base, N, ct, t_lo, t_hi, qa, lists, k, filter, lane);
    }

    __syncthreads();
    // fold the other waves' lists into wave 0's, query j by wave j % kTopkWaves; write the workgroup's list
    for (int j = wave; j < nq; j += kTopkWaves) {
        u64* L = lists_all + (size_t)j * k;
        for (int w = 1; w < kTopkWaves; ++w) {
            const u64* src = lists_all + ((size_t)w * q_chunk + j) * k;
            for (int c = 0; c < k; c += 64)
                list_offer(L, k, c + lane < k ? src[c + lane] : 0ull, lane, [](u64 m) { return m; });
        }
        u64* out = partial + ((size_t)(qa + j) * n_slabs + s) * k;
        for (int i = lane; i < k; i += 64) out[i] = L[i];
    }
}

template <int MODEL, int D>
__global__ __launch_bounds__(kTopkWaves * 64, (D == 256 ? 1 : 2)) void topk_tiles_kernel(
    const float* __restrict__ table, int64_t N, int64_t ld, int64_t row_base, const float* __restrict__ coef_head,
    const float* __restrict__ coef_tail, int64_t q_head, int64_t q_tail, int q_chunk, int n_slabs, int k,
    const FilterSpec filter, u64* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    RowsF32<D> rows{table, N, ld, smem + wave * kSlabFloats, lane};
    topk_tiles_run<MODEL, D>(rows, N, row_base, coef_head, coef_tail, q_head, q_tail, q_chunk, n_slabs, k, filter, partial,
                             reinterpret_cast<u64*>(smem + kTopkWaves * kSlabFloats), wave, lane);
}

// the same over a 16-bit table (T = _Float16 / __bf16; ld in elements)
template <int MODEL, int D, class T>
__global__ __launch_bounds__(kTopkWaves * 64, (D == 256 ? 1 : 2)) void topk_tiles16_kernel(
    const T* __restrict__ table, int64_t N, int64_t ld, int64_t row_base, const float* __restrict__ coef_head,
    const float* __restrict__ coef_tail, int64_t q_head, int64_t q_tail, int q_chunk, int n_slabs, int k,
    const FilterSpec filter, u64* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    Rows16<D, T> rows{reinterpret_cast<const char*>(table), N, ld, smem + wave * kSlabFloats, lane};
    topk_tiles_run<MODEL, D>(rows, N, row_base, coef_head, coef_tail, q_head, q_tail, q_chunk, n_slabs, k, filter, partial,
                             reinterpret_cast<u64*>(smem + kTopkWaves * kSlabFloats), wave, lane);
}

// One workgroup (blockDim.x / 64 waves) per query: the k best of its n_in keys -- `keys` (Q, n_in), or made from
// (rows, scores) (Q, n_in), a row < 0 being an empty slot.  Wave w takes entries w x 64 ..., the next chunk's load
// issued before the current one is offered; wave 0 folds the others' lists into its own and writes the result.
template <bool FROM_KEYS>
__global__ __launch_bounds__(kTopkMergeMaxWaves * 64) void topk_merge_kernel(const u64* __restrict__ keys,
                                                                             const int64_t* __restrict__ rows_in,
                                                                             const float* __restrict__ scores_in, int64_t n_in,
                                                                             int k, int64_t* __restrict__ rows_out,
                                                                             float* __restrict__ scores_out) {
    extern __shared__ u64 mlists[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int waves = blockDim.x / 64;
    const int64_t q = blockIdx.x;
    u64* L = mlists + (size_t)wave * k;
    for (int i = lane; i < k; i += 64) L[i] = 0ull;
    wave_lds_sync();

    auto fetch = [&](int64_t i) -> u64 {
        if (i >= n_in) return 0ull;
        if constexpr (FROM_KEYS) {
            return keys[q * n_in + i];
        } else {
            const int64_t r = rows_in[q * n_in + i];
            return r < 0 ? 0ull : topk_key(scores_in[q * n_in + i], r);
        }
    };
    const int64_t stride = (int64_t)waves * 64;
    u64 cur = fetch((int64_t)wave * 64 + lane);
    for (int64_t c = (int64_t)wave * 64; c < n_in; c += stride) {
        const u64 nxt = fetch(c + stride + lane);
        list_offer(L, k, cur, lane, [](u64 m) { return m; });
        cur = nxt;
    }
    __syncthreads();
    if (wave == 0) {
        for (int w = 1; w < waves; ++w)
            for (int c = 0; c < k; c += 64)
                list_offer(L, k, c + lane < k ? mlists[(size_t)w * k + c + lane] : 0ull, lane, [](u64 m) { return m; });
        for (int i = lane; i < k; i += 64) {
            const u64 key = L[i];
            rows_out[q * k + i] = key_row(key);
            scores_out[q * k + i] = key_score(key);
        }
    }
}

// One lane per output slot: the score of the selected row by Scorer<>::score<true> from the query's own vectors
// (LazyCoef) -- blp_score_fwd's arithmetic, bit for bit, sign of zero included.  Empty slots keep NaN.  T: the table's
// storage type (a 16-bit row is widened as it is read).
template <int MODEL, int D, class T>
__global__ __launch_bounds__(64) void topk_rescore_kernel(const T* __restrict__ table, int64_t ld, int64_t row_base,
                                                          const QRows q_fixed, const QRows q_rel, int64_t q_head, int64_t Q,
                                                          int k, const int64_t* __restrict__ rows, float* __restrict__ scores) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= Q * k) return;
    const int64_t r = rows[i];
    if (r < 0) return;
    const int64_t q = i / k;
    float e[D];
    const T* row = table + (r - row_base) * ld;
#pragma unroll
    for (int d = 0; d < D; d += 4) {
        const float4 v = load4<T>(row + d);
        e[d] = v.x; e[d + 1] = v.y; e[d + 2] = v.z; e[d + 3] = v.w;
    }
    const float* f = q_fixed.row(q);
    const float* rel = q_rel.row(q);
    float s;
    if (q < q_head)
        s = Scorer<MODEL, HEAD, D>::template score<true>(e, LazyCoef<MODEL, HEAD, D>{f, rel});
    else
        s = Scorer<MODEL, TAIL, D>::template score<true>(e, LazyCoef<MODEL, TAIL, D>{f, rel});
    scores[i] = s;
}

// ------------------------------------------------------------------------------------------------ host side
bool topk_supported(int model, int D, int k) {
    return model >= TRANSE && model <= SIMPLE && (D == 64 || D == 128 || D == 256) && k >= 1 && k <= kTopkMaxK;
}
bool topk_typed_supported(int model, int dtype, int D, int k) {
    return (dtype == kTableF32 || dtype == kTableF16 || dtype == kTableBF16) && topk_supported(model, D, k);
}

struct TopkWorkspace {
    float* coef_head;
    float* coef_tail;
    u64* partial;
    size_t bytes;
};

static TopkWorkspace carve_topk(void* base, int D, int64_t N, int64_t q_head, int64_t q_tail, int k) {
    const int64_t Q = q_head + q_tail;
    const size_t coef_h = align_up((size_t)q_head * max_coef(D) * 4, 256), coef_t = align_up((size_t)q_tail * max_coef(D) * 4, 256);
    const size_t part = align_up((size_t)Q * topk_slabs(N, Q, k) * k * 8, 256);
    char* p = static_cast<char*>(base);
    TopkWorkspace w;
    w.coef_head = reinterpret_cast<float*>(p);
    w.coef_tail = reinterpret_cast<float*>(p + coef_h);
    w.partial = reinterpret_cast<u64*>(p + coef_h + coef_t);
    w.bytes = coef_h + coef_t + part;
    return w;
}

size_t topk_workspace_bytes(int model, int D, int64_t N, int64_t q_head, int64_t q_tail, int k) {
    if (!topk_supported(model, D, k) || N < 0 || q_head < 0 || q_tail < 0) return 0;
    return carve_topk(nullptr, D, N, q_head, q_tail, k).bytes;
}

static hipError_t launch_merge(const u64* keys, const int64_t* rows_in, const float* scores_in, int64_t Q, int64_t n_in, int k,
                               int64_t* rows_out, float* scores_out, hipStream_t stream) {
    if (Q == 0) return hipSuccess;
    int64_t waves = n_in / 256;  // a wave per >= 4 chunks of 64 entries
    waves = waves < 1 ? 1 : (waves > kTopkMergeMaxWaves ? kTopkMergeMaxWaves : waves);
    const size_t lds = (size_t)waves * k * 8;
    if (keys)
        topk_merge_kernel<true><<<dim3((unsigned)Q), (unsigned)(waves * 64), lds, stream>>>(keys, nullptr, nullptr, n_in, k,
                                                                                           rows_out, scores_out);
    else
        topk_merge_kernel<false><<<dim3((unsigned)Q), (unsigned)(waves * 64), lds, stream>>>(nullptr, rows_in, scores_in, n_in,
                                                                                            k, rows_out, scores_out);
    return hipGetLastError();
}

hipError_t launch_topk_merge(const int64_t* rows, const float* scores, int64_t Q, int64_t n_in, int k, int64_t* rows_out,
                             float* scores_out, hipStream_t stream) {
    return launch_merge(nullptr, rows, scores, Q, n_in, k, rows_out, scores_out, stream);
}

// topk_sets.hip: the second and third stage of a call on its own partial lists -- keys (Q, n_in), 0 = an empty slot
hipError_t launch_topk_merge_keys(const unsigned long long* keys, int64_t Q, int64_t n_in, int k, int64_t* rows_out, float* scores_out,
                                  hipStream_t stream) {
    return launch_merge(keys, nullptr, nullptr, Q, n_in, k, rows_out, scores_out, stream);
}

hipError_t launch_topk_rescore(int model, int D, const float* table, int64_t ld, int64_t row_base, const QRows q_fixed, const QRows q_rel,
                               int64_t q_head, int64_t Q, int k, const int64_t* rows, float* scores, hipStream_t stream) {
    const int64_t slots = Q * k;
    if (slots == 0) return hipSuccess;
#define BLP_RESCORE_CASE(M, DD)                                                                                                   \
    if (model == M && D == DD) {                                                                                                  \
        topk_rescore_kernel<M, DD, float><<<dim3((unsigned)((slots + 63) / 64)), 64, 0, stream>>>(table, ld, row_base, q_fixed, q_rel, \
                                                                                                  q_head, Q, k, rows, scores);   \
        return hipGetLastError();                                                                                                 \
    }
#define BLP_RESCORE_MODEL(M) BLP_RESCORE_CASE(M, 64) BLP_RESCORE_CASE(M, 128) BLP_RESCORE_CASE(M, 256)
    BLP_RESCORE_MODEL(TRANSE) BLP_RESCORE_MODEL(DISTMULT) BLP_RESCORE_MODEL(COMPLEX) BLP_RESCORE_MODEL(SIMPLE)
#undef BLP_RESCORE_MODEL
#undef BLP_RESCORE_CASE
    return hipErrorInvalidValue;
}

// launch_topk_rescore for a table of any storage type (dtype: table_elem.h; ld in elements): the winners re-scored on the
// rows widened to f32 -- the instantiations of topk_rescore_kernel that topk_impl launches, no kernel of its own
template <int MODEL, int D, class T>
static hipError_t rescore_impl(const T* table, int64_t ld, int64_t row_base, const QRows& q_fixed, const QRows& q_rel, int64_t q_head,
                               int64_t Q, int k, const int64_t* rows, float* scores, hipStream_t stream) {
    const int64_t slots = Q * k;
    topk_rescore_kernel<MODEL, D, T><<<dim3((unsigned)((slots + 63) / 64)), 64, 0, stream>>>(table, ld, row_base, q_fixed, q_rel,
                                                                                             q_head, Q, k, rows, scores);
    return hipGetLastError();
}

hipError_t launch_topk_rescore_typed(int model, int D, int dtype, const void* table, int64_t ld, int64_t row_base, const QRows q_fixed,
                                     const QRows q_rel, int64_t q_head, int64_t Q, int k, const int64_t* rows, float* scores,
                                     hipStream_t stream) {
    if (dtype == kTableF32)
        return launch_topk_rescore(model, D, static_cast<const float*>(table), ld, row_base, q_fixed, q_rel, q_head, Q, k, rows, scores,
                                   stream);
    if (Q * k == 0) return hipSuccess;
#define BLP_RESCORE16_CASE(M, DD)                                                                                                  \
    if (model == M && D == DD) {                                                                                                   \
        if (dtype == kTableF16)                                                                                                    \
            return rescore_impl<M, DD>(static_cast<const _Float16*>(table), ld, row_base, q_fixed, q_rel, q_head, Q, k, rows, scores, \
                                       stream);                                                                                    \
        if (dtype == kTableBF16)                                                                                                   \
            return rescore_impl<M, DD>(static_cast<const __bf16*>(table), ld, row_base, q_fixed, q_rel, q_head, Q, k, rows, scores,   \
                                       stream);                                                                                    \
        return hipErrorInvalidValue;                                                                                               \
    }
#define BLP_RESCORE16_MODEL(M) BLP_RESCORE16_CASE(M, 64) BLP_RESCORE16_CASE(M, 128) BLP_RESCORE16_CASE(M, 256)
    BLP_RESCORE16_MODEL(TRANSE) BLP_RESCORE16_MODEL(DISTMULT) BLP_RESCORE16_MODEL(COMPLEX) BLP_RESCORE16_MODEL(SIMPLE)
#undef BLP_RESCORE16_MODEL
#undef BLP_RESCORE16_CASE
    return hipErrorInvalidValue;
}

template <int MODEL, int D, class T>
static hipError_t topk_impl(const T* table, int64_t N, int64_t ld, int64_t row_base, const QRows& q_fixed, const QRows& q_rel,
                            int64_t q_head, int64_t q_tail, int k, const FilterSpec& filter, int64_t* rows, float* scores,
                            void* workspace, hipStream_t stream) {
    const int64_t Q = q_head + q_tail;
    if (Q == 0) return hipSuccess;
    if (N == 0) return launch_merge(nullptr, rows, scores, Q, 0, k, rows, scores, stream);  // every slot empty
    const TopkWorkspace w = carve_topk(workspace, D, N, q_head, q_tail, k);
    hipError_t err = launch_prep_coef(MODEL, D, q_fixed, q_rel, q_head, q_tail, w.coef_head, w.coef_tail, stream);
    if (err != hipSuccess) return err;
    const int q_chunk = topk_chunk(k);
    const int64_t n_slabs = topk_slabs(N, Q, k), n_chunks = (Q + q_chunk - 1) / q_chunk;
    const size_t lds = (size_t)kTopkWaves * kSlabFloats * 4 + (size_t)kTopkWaves * q_chunk * k * 8;
    const dim3 grid((unsigned)(n_chunks * n_slabs));
    if constexpr (std::is_same<T, float>::value) {
        topk_tiles_kernel<MODEL, D><<<grid, kTopkWaves * 64, lds, stream>>>(
            table, N, ld, row_base, w.coef_head, w.coef_tail, q_head, q_tail, q_chunk, (int)n_slabs, k, filter, w.partial);
    } else {
        topk_tiles16_kernel<MODEL, D, T><<<grid, kTopkWaves * 64, lds, stream>>>(
            table, N, ld, row_base, w.coef_head, w.coef_tail, q_head, q_tail, q_chunk, (int)n_slabs, k, filter, w.partial);
    }
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if ((err = launch_merge(w.partial, nullptr, nullptr, Q, n_slabs * k, k, rows, scores, stream)) != hipSuccess) return err;
    const int64_t slots = Q * k;
    topk_rescore_kernel<MODEL, D, T><<<dim3((unsigned)((slots + 63) / 64)), 64, 0, stream>>>(table, ld, row_base, q_fixed, q_rel,
                                                                                             q_head, Q, k, rows, scores);
    return hipGetLastError();
}

hipError_t launch_topk(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, int64_t row_base, const QRows q_fixed,
                       const QRows q_rel, int64_t q_head, int64_t q_tail, int k, const FilterSpec& filter, int64_t* rows,
                       float* scores, void* workspace, hipStream_t stream) {
#define BLP_TOPK_TYPED(M, DD, TT)                                                                                           \
    return topk_impl<M, DD>(static_cast<const TT*>(table), N, ld, row_base, q_fixed, q_rel, q_head, q_tail, k, filter, rows, \
                            scores, workspace, stream);
#define BLP_TOPK_CASE(M, DD)                                                                                              \
    if (model == M && D == DD) {                                                                                          \
        if (dtype == kTableF32) BLP_TOPK_TYPED(M, DD, float)                                                              \
        if (dtype == kTableF16) BLP_TOPK_TYPED(M, DD, _Float16)                                                           \
        if (dtype == kTableBF16) BLP_TOPK_TYPED(M, DD, __bf16)                                                            \
        return hipErrorInvalidValue;                                                                                      \
    }
#define BLP_TOPK_MODEL(M) BLP_TOPK_CASE(M, 64) BLP_TOPK_CASE(M, 128) BLP_TOPK_CASE(M, 256)
    BLP_TOPK_MODEL(TRANSE) BLP_TOPK_MODEL(DISTMULT) BLP_TOPK_MODEL(COMPLEX) BLP_TOPK_MODEL(SIMPLE)
#undef BLP_TOPK_MODEL
#undef BLP_TOPK_CASE
#undef BLP_TOPK_TYPED
    return hipErrorInvalidValue;
}

}  // namespace blp
