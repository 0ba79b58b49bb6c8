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
// The table pass.  The reference sums the n terms of a score (n = D for DistMult, D / 2 for ComplEx and SimplE) in torch's
// sum(dim=-1) order (score_direct.h: torch_inner_sum_any): 32 accumulators, accumulator a takes term 32 i + a of every
// whole 32-term row i; for n >= 512 the accumulators are added into a second set and zeroed after rows 16 and 32; the
// (n / 8) % 4 leftover vectors of 8 go to accumulators 0 .. 7; fold A[l] + A[8 + l] + A[16 + l] + A[24 + l]; the n % 8
// tail terms first, then the eight folded values left to right.  That order is mapped onto EIGHT LANES PER CANDIDATE ROW:
// lane `sub` of the eight owns accumulators 4 sub .. 4 sub + 3, so a 32-term row of a candidate is one 16-byte load per
// lane -- the eight lanes read one 128-B line -- and the leftover vectors belong to lanes 0 and 1.  A wave is 8 candidate
// groups; each group holds kAwRows candidate rows against the kAwQueries queries of the workgroup's chunk, i.e.
// kAwRows x kAwQueries x 4 accumulators per lane (twice that for n >= 512: CASCADE), all in registers.  The queries'
// coefficients -- what Scorer<MODEL, SIDE, D>::coef hoists (score_core.h), computed by the workgroup when it takes the
// chunk -- sit in LDS as K arrays of n floats per query; a lane reads the 16 bytes of its four columns, the eight groups
// the same addresses (broadcast).  The fold is three v_add with a DPP row shift (lanes 0 and 1 get accumulators 0 .. 7
// folded), the last eight additions take the values by DPP quad broadcasts from lanes 0 and 1; lane 0 of a group
// compares with the true key and the wave counts by ballot into scalar counters, flushed once per (chunk, slab) with a
// 64-bit atomic (gt low word, ge high word).  Additions of all-zero upper cascade levels are dropped: they can turn -0
// into +0 only, which no > / >= sees.
//
// Grid: x = query chunks (at most kAwMaxGridX, the workgroup strides), y = candidate slabs of about kAwSlabBytes (one
// slab stays in an XCD's L2 while the chunks that run together stream it), fewer rows per slab when there are few chunks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "rank_common.h"
#include "score_core.h"

#pragma clang fp contract(off)

namespace blp {

namespace {

constexpr int kAwQueries = 8;                          // queries of a chunk
constexpr int kAwRows = 2;                             // candidate rows of an eight-lane group
constexpr int kAwWaves = 4;
constexpr int kAwBlockRows = kAwWaves * 8 * kAwRows;   // rows a workgroup takes per trip
constexpr int kAwMaxD = 1024;
constexpr int64_t kAwSlabBytes = 2 << 20;
constexpr int64_t kAwMaxGridX = 32768, kAwMaxGridY = 32768;

// One summand of the score with the candidate's elements ea = e[j] and (two-halves models) eb = e[H + j], and the query's K
// coefficients at j: the operations of Scorer<MODEL, SIDE, D>::score / coef (score_core.h), i.e. of score_direct<MODEL>.
template <int MODEL, int SIDE>
struct WideTerm;

template <>
struct WideTerm<DISTMULT, TAIL> {  // (h * r) * e
    static constexpr int K = 1;
    static constexpr bool kHalves = false;
    __device__ __forceinline__ static float coef(const float* f, const float* r, int j, int H, int k) { return f[j] * r[j]; }
    __device__ __forceinline__ static float term(float ea, float eb, const float (&c)[K]) { return c[0] * ea; }
};
template <>
struct WideTerm<DISTMULT, HEAD> {  // (e * r) * t
    static constexpr int K = 2;
    static constexpr bool kHalves = false;
    __device__ __forceinline__ static float coef(const float* f, const float* r, int j, int H, int k) { return k == 0 ? r[j] : f[j]; }
    __device__ __forceinline__ static float term(float ea, float eb, const float (&c)[K]) {
        const float x = ea * c[0];
        return x * c[1];
    }
};
template <>
struct WideTerm<COMPLEX, TAIL> {  // f = head: the four r * h products are hoisted
    static constexpr int K = 4;
    static constexpr bool kHalves = true;
    __device__ __forceinline__ static float coef(const float* f, const float* r, int j, int H, int k) {
        switch (k) {
        case 0: return r[j] * f[j];
        case 1: return r[j] * f[H + j];
        case 2: return r[H + j] * f[j];
        default: return r[H + j] * f[H + j];
        }
    }
    __device__ __forceinline__ static float term(float ea, float eb, const float (&c)[K]) {
        const float a = c[0] * ea;
        const float b = c[1] * eb;
        const float cc = c[2] * eb;
        const float d = c[3] * ea;
        float s = a + b;
        s = s + cc;
        return s - d;
    }
};
template <>
struct WideTerm<COMPLEX, HEAD> {  // f = tail: rr, ri, tr, ti as they are
    static constexpr int K = 4;
    static constexpr bool kHalves = true;
    __device__ __forceinline__ static float coef(const float* f, const float* r, int j, int H, int k) {
        switch (k) {
        case 0: return r[j];
        case 1: return r[H + j];
        case 2: return f[j];
        default: return f[H + j];
        }
    }
    __device__ __forceinline__ static float term(float ea, float eb, const float (&c)[K]) {
        float a = c[0] * ea;   a = a * c[2];    // (rr*hr)*tr
        float b = c[0] * eb;   b = b * c[3];    // (rr*hi)*ti
        float cc = c[1] * ea;  cc = cc * c[3];  // (ri*hr)*ti
        float d = c[1] * eb;   d = d * c[2];    // (ri*hi)*tr
        float s = a + b;
        s = s + cc;
        return s - d;
    }
};
template <>
struct WideTerm<SIMPLE, TAIL> {  // f = head = [hh | ht], e = tail = [th | tt]: (hh*ra)*tt + (th*rb)*ht
    static constexpr int K = 3;
    static constexpr bool kHalves = true;
    __device__ __forceinline__ static float coef(const float* f, const float* r, int j, int H, int k) {
        return k == 0 ? f[j] * r[j] : (k == 1 ? r[H + j] : f[H + j]);
    }
    __device__ __forceinline__ static float term(float ea, float eb, const float (&c)[K]) {
        const float a = c[0] * eb;
        float b = ea * c[1];
        b = b * c[2];
        return a + b;
    }
};
template <>
struct WideTerm<SIMPLE, HEAD> {  // f = tail = [th | tt], e = head = [hh | ht]
    static constexpr int K = 3;
    static constexpr bool kHalves = true;
    __device__ __forceinline__ static float coef(const float* f, const float* r, int j, int H, int k) {
        return k == 0 ? r[j] : (k == 1 ? f[H + j] : f[j] * r[H + j]);
    }
    __device__ __forceinline__ static float term(float ea, float eb, const float (&c)[K]) {
        float a = ea * c[0];
        a = a * c[1];
        const float b = c[2] * eb;
        return a + b;
    }
};

template <int S>
__device__ __forceinline__ float row_shl(float x) {  // lane l <- lane l + S of its row of 16
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x100 + S, 0xf, 0xf, true));
}

// four columns of kAwRows candidate rows
template <bool HALVES>
struct WideCols {
    float a[kAwRows][4];
    float b[HALVES ? kAwRows : 1][4];
};

template <bool HALVES>
__device__ __forceinline__ void wide_load(WideCols<HALVES>& e, const float* const (&ptr)[kAwRows], int col, int H) {
#pragma unroll
    for (int r = 0; r < kAwRows; ++r) {
        const float4 v = *reinterpret_cast<const float4*>(ptr[r] + col);
        e.a[r][0] = v.x; e.a[r][1] = v.y; e.a[r][2] = v.z; e.a[r][3] = v.w;
        if constexpr (HALVES) {  // H is even, not always a multiple of 4: two 8-byte loads
            const float2 lo = *reinterpret_cast<const float2*>(ptr[r] + H + col);
            const float2 hi = *reinterpret_cast<const float2*>(ptr[r] + H + col + 2);
            e.b[r][0] = lo.x; e.b[r][1] = lo.y; e.b[r][2] = hi.x; e.b[r][3] = hi.y;
        } else {
            e.b[0][0] = e.b[0][1] = e.b[0][2] = e.b[0][3] = 0.0f;  // never used
        }
    }
}

// acc[q][r][c] += term of column col + c (col: the lane's first of four) for every query of the chunk
template <int MODEL, int SIDE>
__device__ __forceinline__ void wide_step(float (&acc)[kAwQueries][kAwRows][4], const WideCols<WideTerm<MODEL, SIDE>::kHalves>& e,
                                          const float* coef, int n4, int col) {
    using T = WideTerm<MODEL, SIDE>;
#pragma unroll
    for (int q = 0; q < kAwQueries; ++q) {
        float c4[T::K][4];
#pragma unroll
        for (int k = 0; k < T::K; ++k) {
            const float4 v = *reinterpret_cast<const float4*>(coef + (q * T::K + k) * n4 + col);
            c4[k][0] = v.x; c4[k][1] = v.y; c4[k][2] = v.z; c4[k][3] = v.w;
        }
#pragma unroll
        for (int r = 0; r < kAwRows; ++r) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float ck[T::K];
#pragma unroll
                for (int k = 0; k < T::K; ++k) ck[k] = c4[k][c];
                acc[q][r][c] = acc[q][r][c] + T::term(e.a[r][c], e.b[T::kHalves ? r : 0][c], ck);
            }
        }
    }
}

template <int MODEL, int SIDE, bool CASCADE>
__global__ __launch_bounds__(kAwWaves * 64) void rank_all_wide_kernel(const float* __restrict__ table, int64_t N, int64_t ld, int D,
                                                                      const QRows q_fixed, const QRows q_rel,
                                                                      const float* __restrict__ key_true, int64_t q_off, int64_t nq,
                                                                      int64_t slab_rows, unsigned long long* __restrict__ acc_out) {
    using T = WideTerm<MODEL, SIDE>;
    constexpr int K = T::K, QC = kAwQueries, R = kAwRows;
    extern __shared__ __attribute__((aligned(16))) float aw_coef[];  // [query of the chunk][K][n4]
    const int H = D / 2, n = MODEL == DISTMULT ? D : H, n4 = (n + 3) & ~3;
    const int size_ilp = n / 32, vec_size = n / 8, n_left = vec_size - 4 * size_ilp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 3, sub = lane & 7;
    const int64_t row_lo = (int64_t)blockIdx.y * slab_rows, row_hi = row_lo + slab_rows < N ? row_lo + slab_rows : N;
    const int64_t n_chunks = (nq + QC - 1) / QC;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t q0 = q_off + chunk * QC;
        const int live_q = (int)(q_off + nq - q0 < QC ? q_off + nq - q0 : QC);
        __syncthreads();  // the previous chunk's coefficients have been read
        for (int x = threadIdx.x; x < QC * K * n4; x += kAwWaves * 64) {
            const int q = x / (K * n4), rem = x - q * (K * n4), k = rem / n4, j = rem - k * n4;
            float v = 0.0f;
            if (q < live_q && j < n) v = T::coef(q_fixed.row(q0 + q), q_rel.row(q0 + q), j, H, k);
            aw_coef[x] = v;
        }
        __syncthreads();
        float kt[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) kt[q] = key_true[q0 + (q < live_q ? q : 0)];
        unsigned cgt[QC], cge[QC];
#pragma unroll
        for (int q = 0; q < QC; ++q) cgt[q] = cge[q] = 0;

        for (int64_t rb = row_lo + wave * (8 * R); rb < row_hi; rb += kAwBlockRows) {  // wave-uniform
            const float* base[R];  // the group's rows (past the slab: its last row, not counted)
            const float* ptr[R];   // ... at the lane's four columns
            bool live[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t row = rb + grp + 8 * r;
                live[r] = row < row_hi;
                base[r] = table + (live[r] ? row : row_hi - 1) * ld;
                ptr[r] = base[r] + 4 * sub;
            }
            float acc[QC][R][4];
            float up[CASCADE ? QC : 1][R][4];
#pragma unroll
            for (int q = 0; q < QC; ++q)
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        acc[q][r][c] = 0.0f;
                        if (CASCADE) up[CASCADE ? q : 0][r][c] = 0.0f;
                    }
            // whole rows of 32 terms, the next row's loads in flight behind the current row's arithmetic
            WideCols<T::kHalves> cur;
            if (size_ilp > 0) wide_load<T::kHalves>(cur, ptr, 0, H);
#pragma unroll 1
            for (int i = 0; i < size_ilp; ++i) {
                WideCols<T::kHalves> nxt;
                wide_load<T::kHalves>(nxt, ptr, i + 1 < size_ilp ? 32 * (i + 1) : 32 * i, H);
                wide_step<MODEL, SIDE>(acc, cur, aw_coef, n4, 32 * i + 4 * sub);
                cur = nxt;
                if constexpr (CASCADE) {
                    if (((i + 1) & 15) == 0) {  // after rows 16 and 32: one level up
#pragma unroll
                        for (int q = 0; q < QC; ++q)
#pragma unroll
                            for (int r = 0; r < R; ++r)
#pragma unroll
                                for (int c = 0; c < 4; ++c) {
                                    up[CASCADE ? q : 0][r][c] = up[CASCADE ? q : 0][r][c] + acc[q][r][c];
                                    acc[q][r][c] = 0.0f;
                                }
                    }
                }
            }
            if constexpr (CASCADE) {
#pragma unroll
                for (int q = 0; q < QC; ++q)
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[q][r][c] = acc[q][r][c] + up[CASCADE ? q : 0][r][c];
            }
            // the leftover vectors of 8: accumulators 0 .. 7, i.e. lanes 0 and 1 of the group
            for (int v = 0; v < n_left; ++v) {
                if (sub < 2) {
                    const int col = 32 * size_ilp + 8 * v;
                    WideCols<T::kHalves> e;
                    wide_load<T::kHalves>(e, ptr, col, H);
                    wide_step<MODEL, SIDE>(acc, e, aw_coef, n4, col + 4 * sub);
                }
            }
            // the n % 8 tail terms, one after the other (every lane of the group the same)
            float tail[QC][R];
#pragma unroll
            for (int q = 0; q < QC; ++q)
#pragma unroll
                for (int r = 0; r < R; ++r) tail[q][r] = 0.0f;
            for (int j = 8 * vec_size; j < n; ++j) {
                float ea[R], eb[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    ea[r] = base[r][j];
                    eb[r] = T::kHalves ? base[r][H + j] : 0.0f;
                }
#pragma unroll
                for (int q = 0; q < QC; ++q) {
                    float ck[K];
#pragma unroll
                    for (int k = 0; k < K; ++k) ck[k] = aw_coef[(q * K + k) * n4 + j];
#pragma unroll
                    for (int r = 0; r < R; ++r) tail[q][r] = tail[q][r] + T::term(ea[r], eb[r], ck);
                }
            }
            // fold, the last eight additions, the comparison
#pragma unroll
            for (int q = 0; q < QC; ++q) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    float V[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {  // lanes 0, 1: A[l] + A[8 + l] + A[16 + l] + A[24 + l], l = 4 sub + c
                        const float a = acc[q][r][c];
                        float v = a + row_shl<2>(a);
                        v = v + row_shl<4>(a);
                        V[c] = v + row_shl<6>(a);
                    }
                    float s = tail[q][r];
#pragma unroll
                    for (int c = 0; c < 4; ++c) s = s + quad_bcast<0>(V[c]);
#pragma unroll
                    for (int c = 0; c < 4; ++c) s = s + quad_bcast<1>(V[c]);
                    const float key = MODEL == SIMPLE ? s / 2.0f : s;
                    const bool mine = live[r] && sub == 0;
                    cgt[q] += (unsigned)__popcll(__ballot(mine && key > kt[q]));
                    cge[q] += (unsigned)__popcll(__ballot(mine && key >= kt[q]));
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

// One (candidate, query) pair by eight lanes, straight from the three vectors: the table pass's mapping and operations (lane
// `sub` owns accumulators 4 sub .. 4 sub + 3, the same fold and last additions), the coefficients computed in place by the
// expressions the pass stages in LDS -- so a pair gets the number the pass gives it, bit for bit.  Every lane of the wave must
// call (the fold reads neighbouring lanes); the result is valid in lanes 0 .. 3 of the eight.
template <int MODEL, int SIDE>
__device__ __forceinline__ float wide_pair_score(const float* __restrict__ e, const float* __restrict__ f, const float* __restrict__ r,
                                                 int D, int sub) {
    using T = WideTerm<MODEL, SIDE>;
    constexpr int K = T::K;
    const int H = D / 2, n = MODEL == DISTMULT ? D : H;
    const int size_ilp = n / 32, vec_size = n / 8, n_left = vec_size - 4 * size_ilp;
    auto term_at = [&](int j) {
        float ck[K];
#pragma unroll
        for (int k = 0; k < K; ++k) ck[k] = T::coef(f, r, j, H, k);
        return T::term(e[j], T::kHalves ? e[H + j] : 0.0f, ck);
    };
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, up[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < size_ilp; ++i) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = acc[c] + term_at(32 * i + 4 * sub + c);
        if (((i + 1) & 15) == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                up[c] = up[c] + acc[c];
                acc[c] = 0.0f;
            }
        }
    }
    if (n >= 512) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = acc[c] + up[c];
    }
    for (int v = 0; v < n_left; ++v) {
        if (sub < 2) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = acc[c] + term_at(32 * size_ilp + 8 * v + 4 * sub + c);
        }
    }
    float s = 0.0f;
    for (int j = 8 * vec_size; j < n; ++j) s = s + term_at(j);
    float V[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float v = acc[c] + row_shl<2>(acc[c]);
        v = v + row_shl<4>(acc[c]);
        V[c] = v + row_shl<6>(acc[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) s = s + quad_bcast<0>(V[c]);
#pragma unroll
    for (int c = 0; c < 4; ++c) s = s + quad_bcast<1>(V[c]);
    return MODEL == SIMPLE ? s / 2.0f : s;
}

// True-entity keys, eight lanes per query (wide_pair_score); the queries' accumulators start at zero.
template <int MODEL>
__global__ __launch_bounds__(256) void wide_bilinear_true_key_kernel(int D, const QRows q_fixed, const QRows q_rel, const QRows q_true,
                                                                     int64_t q_head, int64_t Q, float* __restrict__ key_true,
                                                                     unsigned long long* __restrict__ acc) {
    const int sub = threadIdx.x & 7;
    for (int64_t q0 = blockIdx.x * 32ll; q0 < Q; q0 += gridDim.x * 32ll) {  // workgroup-uniform
        const int64_t qq = q0 + (threadIdx.x >> 3), q = qq < Q ? qq : Q - 1;
        const float* e = q_true.row(q);
        const float* f = q_fixed.row(q);
        const float* r = q_rel.row(q);
        const bool head = q0 + 31 < q_head ? true : (q0 >= q_head ? false : q < q_head);
        float key;
        if (q0 + 31 < q_head || q0 >= q_head) {  // wave-uniform side (all but the one group that straddles q_head)
            key = head ? wide_pair_score<MODEL, HEAD>(e, f, r, D, sub) : wide_pair_score<MODEL, TAIL>(e, f, r, D, sub);
        } else {  // both sides by every lane, each lane keeps its own
            const float kh = wide_pair_score<MODEL, HEAD>(e, f, r, D, sub);
            const float kt = wide_pair_score<MODEL, TAIL>(e, f, r, D, sub);
            key = head ? kh : kt;
        }
        if (sub == 0 && qq < Q) {
            key_true[qq] = key;
            acc[qq] = 0;
        }
    }
}

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
