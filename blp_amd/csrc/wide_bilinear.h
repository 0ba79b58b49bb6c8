// wide_bilinear.h -- the arithmetic of the exact table pass for DistMult / ComplEx / SimplE at run-time width (D % 4 == 0,
// 4 <= D <= 1024), shared by rank_all_wide.hip (counts against the true key) and topk_wide.hip (selection): one definition
// of the sum order, as sets_wide_sums.h is for TransE.
//
// The reference sums the n terms of a score (n = D for DistMult, D / 2 for ComplEx and SimplE) in torch's sum(dim=-1) order
// (score_direct.h: torch_inner_sum_any): 32 accumulators, accumulator a takes term 32 i + a of every whole 32-term row i; for
// n >= 512 the accumulators are added into a second set and zeroed after rows 16 and 32; the (n / 8) % 4 leftover vectors of
// 8 go to accumulators 0 .. 7; fold A[l] + A[8 + l] + A[16 + l] + A[24 + l]; the n % 8 tail terms first, then the eight
// folded values left to right.  That order is mapped onto EIGHT LANES PER CANDIDATE ROW: lane `sub` of the eight owns
// accumulators 4 sub .. 4 sub + 3, so a 32-term row of a candidate is one 16-byte load per lane -- the eight lanes read one
// 128-B line -- and the leftover vectors belong to lanes 0 and 1.  A wave is 8 candidate groups; each group holds kAwRows
// candidate rows against the kAwQueries queries of the workgroup's chunk, i.e. kAwRows x kAwQueries x 4 accumulators per lane
// (twice that for n >= 512: CASCADE), all in registers.  The queries' coefficients -- what Scorer<MODEL, SIDE, D>::coef hoists
// (score_core.h), computed by the workgroup when it takes the chunk (wide_stage_coef) -- sit in LDS as K arrays of n floats
// per query; a lane reads the 16 bytes of its four columns, the eight groups the same addresses (broadcast).  The fold is
// three v_add with a DPP row shift (lanes 0 and 1 get accumulators 0 .. 7 folded), the last eight additions take the values
// by DPP quad broadcasts from lanes 0 and 1 (wide_fold).  Additions of all-zero upper cascade levels are dropped.  They change
// nothing: every chain starts from +0, and x + y is -0 only when both are, so no accumulator and no partial sum is ever -0,
// and z + (+0) == z bit for bit for every other z.  The sum is torch's bit for bit, sign of zero included (SimplE's final
// s / 2 is the reference's own operation on the same s).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rank_common.h"
#include "score_core.h"
#include "table_elem.h"

#pragma clang fp contract(off)

namespace blp {

constexpr int kAwQueries = 8;                          // queries of a chunk
constexpr int kAwRows = 2;                             // candidate rows of an eight-lane group
constexpr int kAwWaves = 4;
constexpr int kAwBlockRows = kAwWaves * 8 * kAwRows;   // rows a workgroup takes per trip
constexpr int kAwMaxD = 1024;

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

// A third side next to HEAD / TAIL (score_core.h): the candidates are RELATION rows (rank_rels_wide_bilinear.hip), f = the
// pair's head vector, r = its tail vector.  The candidate sits in the middle of the reference's expressions, so nothing is
// hoisted: the coefficients are the two vectors as they are, the operations those of rel_scorer.h / score_direct.h.
constexpr int REL = 2;

template <>
struct WideTerm<DISTMULT, REL> {  // (h * e) * t
    static constexpr int K = 2;
    static constexpr bool kHalves = false;
    __device__ __forceinline__ static float coef(const float* f, const float* r, int j, int H, int k) { return k == 0 ? f[j] : r[j]; }
    __device__ __forceinline__ static float term(float ea, float eb, const float (&c)[K]) {
        const float x = c[0] * ea;
        return x * c[1];
    }
};
template <>
struct WideTerm<COMPLEX, REL> {  // e = [rr | ri]; hr, hi, tr, ti as they are
    static constexpr int K = 4;
    static constexpr bool kHalves = true;
    __device__ __forceinline__ static float coef(const float* f, const float* r, int j, int H, int k) {
        switch (k) {
        case 0: return f[j];
        case 1: return f[H + j];
        case 2: return r[j];
        default: return r[H + j];
        }
    }
    __device__ __forceinline__ static float term(float ea, float eb, const float (&c)[K]) {
        float a = ea * c[0];   a = a * c[2];    // (rr*hr)*tr
        float b = ea * c[1];   b = b * c[3];    // (rr*hi)*ti
        float cc = eb * c[0];  cc = cc * c[3];  // (ri*hr)*ti
        float d = eb * c[1];   d = d * c[2];    // (ri*hi)*tr
        float s = a + b;
        s = s + cc;
        return s - d;
    }
};
template <>
struct WideTerm<SIMPLE, REL> {  // f = head = [hh | ht], r = tail = [th | tt], e = [ra | rb]: (hh*ra)*tt + (th*rb)*ht
    static constexpr int K = 4;
    static constexpr bool kHalves = true;
    __device__ __forceinline__ static float coef(const float* f, const float* r, int j, int H, int k) {
        switch (k) {
        case 0: return f[j];
        case 1: return r[H + j];
        case 2: return r[j];
        default: return f[H + j];
        }
    }
    __device__ __forceinline__ static float term(float ea, float eb, const float (&c)[K]) {
        float a = c[0] * ea;  a = a * c[1];
        float b = c[2] * eb;  b = b * c[3];
        return a + b;
    }
};

// terms of a score, and the floats of a coefficient array in LDS (n rounded up to whole 16-byte reads)
__host__ __device__ inline int wide_terms(int model, int D) { return model == DISTMULT ? D : D / 2; }
__host__ __device__ inline int wide_n4(int model, int D) { return (wide_terms(model, D) + 3) & ~3; }

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

// The fold of a lane's four accumulators with those of lanes + 2, + 4, + 6 of its eight (lanes 0, 1: A[l] + A[8 + l] +
// A[16 + l] + A[24 + l], l = 4 sub + c), then the last eight additions onto the tail sum s, left to right.  Every lane of the
// wave must call; the result is valid in lanes 0 .. 3 of the eight.
template <int MODEL>
__device__ __forceinline__ float wide_fold(const float (&acc)[4], float s) {
    float V[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float a = acc[c];
        float v = a + row_shl<2>(a);
        v = v + row_shl<4>(a);
        V[c] = v + row_shl<6>(a);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) s = s + quad_bcast<0>(V[c]);
#pragma unroll
    for (int c = 0; c < 4; ++c) s = s + quad_bcast<1>(V[c]);
    return MODEL == SIMPLE ? s / 2.0f : s;
}

// The workgroup (kAwWaves x 64 threads) stages the coefficients of queries q0 .. q0 + live_q - 1 in LDS: coef[query of the
// chunk][K][n4], zero beyond live_q and beyond n.  The caller puts the barriers around it.
template <int MODEL, int SIDE>
__device__ __forceinline__ void wide_stage_coef(float* coef, const QRows& q_fixed, const QRows& q_rel, int64_t q0, int live_q, int D) {
    using T = WideTerm<MODEL, SIDE>;
    constexpr int K = T::K;
    const int H = D / 2, n = MODEL == DISTMULT ? D : H, n4 = (n + 3) & ~3;
    for (int x = threadIdx.x; x < kAwQueries * K * n4; x += kAwWaves * 64) {
        const int q = x / (K * n4), rem = x - q * (K * n4), k = rem / n4, j = rem - k * n4;
        float v = 0.0f;
        if (q < live_q && j < n) v = T::coef(q_fixed.row(q0 + q), q_rel.row(q0 + q), j, H, k);
        coef[x] = v;
    }
}

// One trip of the table pass: the scores s[q][r] of the group's kAwRows candidate rows (base[r]: the row's first element)
// against the kAwQueries queries whose coefficients wide_stage_coef put in `coef`.  Every lane of the wave must call; the
// scores are valid in lanes 0 .. 3 of the eight.
template <int MODEL, int SIDE, bool CASCADE>
__device__ __forceinline__ void wide_trip(float (&s)[kAwQueries][kAwRows], const float* const (&base)[kAwRows], const float* coef,
                                          int D, int sub) {
    using T = WideTerm<MODEL, SIDE>;
    constexpr int K = T::K, QC = kAwQueries, R = kAwRows;
    const int H = D / 2, n = MODEL == DISTMULT ? D : H, n4 = (n + 3) & ~3;
    const int size_ilp = n / 32, vec_size = n / 8, n_left = vec_size - 4 * size_ilp;
    const float* ptr[R];  // the group's rows at the lane's four columns
#pragma unroll
    for (int r = 0; r < R; ++r) ptr[r] = base[r] + 4 * sub;
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
        wide_step<MODEL, SIDE>(acc, cur, coef, n4, 32 * i + 4 * sub);
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
            wide_step<MODEL, SIDE>(acc, e, coef, n4, col + 4 * sub);
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
            for (int k = 0; k < K; ++k) ck[k] = coef[(q * K + k) * n4 + j];
#pragma unroll
            for (int r = 0; r < R; ++r) tail[q][r] = tail[q][r] + T::term(ea[r], eb[r], ck);
        }
    }
#pragma unroll
    for (int q = 0; q < QC; ++q)
#pragma unroll
        for (int r = 0; r < R; ++r) s[q][r] = wide_fold<MODEL>(acc[q][r], tail[q][r]);
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
    return wide_fold<MODEL>(acc, s);
}

// ---- one candidate row against ONE query whose coefficients are staged (rank_lists_wide.hip): wide_trip at one query and
// one row, templated on the table's element type (table_elem.h: a 16-bit element is widened exactly as it is read).

// A wave stages one query's coefficients: coef[K][n4] as wide_stage_coef lays them out, zero beyond n.  The caller puts the
// wave_lds_sync()s around it.
template <int MODEL, int SIDE>
__device__ __forceinline__ void wide_stage_coef_wave(float* coef, const float* __restrict__ f, const float* __restrict__ r, int D,
                                                     int lane) {
    using T = WideTerm<MODEL, SIDE>;
    const int H = D / 2, n = MODEL == DISTMULT ? D : H, n4 = (n + 3) & ~3;
#pragma unroll
    for (int k = 0; k < T::K; ++k)
        for (int j = lane; j < n4; j += 64) coef[k * n4 + j] = j < n ? T::coef(f, r, j, H, k) : 0.0f;
}

// one element, and four consecutive elements at an address aligned to two of them (the second half of a row: H is even,
// not always a multiple of 4), widened
template <class TE>
__device__ __forceinline__ float wide_elem(const TE* p);
template <>
__device__ __forceinline__ float wide_elem<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float wide_elem<_Float16>(const _Float16* p) { return (float)*p; }
template <>
__device__ __forceinline__ float wide_elem<__bf16>(const __bf16* p) {
    return __builtin_bit_cast(float, (unsigned)*reinterpret_cast<const unsigned short*>(p) << 16);
}

template <class TE>
__device__ __forceinline__ float4 wide_load4_halves(const TE* p) {
    const unsigned lo = *reinterpret_cast<const unsigned*>(p), hi = *reinterpret_cast<const unsigned*>(p + 2);
    float4 v;
    widen_pair<TE>(lo, v.x, v.y);
    widen_pair<TE>(hi, v.z, v.w);
    return v;
}
template <>
__device__ __forceinline__ float4 wide_load4_halves<float>(const float* p) {
    const float2 lo = *reinterpret_cast<const float2*>(p), hi = *reinterpret_cast<const float2*>(p + 2);
    return make_float4(lo.x, lo.y, hi.x, hi.y);
}

// four columns of one candidate row
struct WidePairCols {
    float4 a, b;
};

template <bool HALVES, class TE>
__device__ __forceinline__ WidePairCols wide_pair_load(const TE* p, int col, int H) {
    WidePairCols e;
    e.a = load4<TE>(p + col);
    e.b = HALVES ? wide_load4_halves<TE>(p + H + col) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (else never used)
    return e;
}

// acc[c] += term of column col + c (col: the lane's first of four): one 16-byte coefficient read per array
template <int MODEL, int SIDE>
__device__ __forceinline__ void wide_pair_step(float (&acc)[4], const WidePairCols& e, const float* coef, int n4, int col) {
    using T = WideTerm<MODEL, SIDE>;
    float c4[T::K][4];
#pragma unroll
    for (int k = 0; k < T::K; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(coef + k * n4 + col);
        c4[k][0] = v.x; c4[k][1] = v.y; c4[k][2] = v.z; c4[k][3] = v.w;
    }
    const float ea[4] = {e.a.x, e.a.y, e.a.z, e.a.w}, eb[4] = {e.b.x, e.b.y, e.b.z, e.b.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float ck[T::K];
#pragma unroll
        for (int k = 0; k < T::K; ++k) ck[k] = c4[k][c];
        acc[c] = acc[c] + T::term(ea[c], eb[c], ck);
    }
}

// The score of candidate row e (its first element) against the query whose coefficients wide_stage_coef_wave put in `coef`:
// wide_trip's order at one query and one row -- the next 32-term row's load in flight behind the current row's arithmetic,
// the cascade after rows 16 and 32 (CASCADE == (n >= 512)), the leftover vectors in lanes 0 and 1, the tail terms first, the
// fold.  Every lane of the wave must call; the result is valid in lanes 0 .. 3 of the eight.
template <int MODEL, int SIDE, bool CASCADE, class TE>
__device__ __forceinline__ float wide_pair_staged(const TE* __restrict__ e, const float* coef, int D, int sub) {
    using T = WideTerm<MODEL, SIDE>;
    constexpr int K = T::K;
    const int H = D / 2, n = MODEL == DISTMULT ? D : H, n4 = (n + 3) & ~3;
    const int size_ilp = n / 32, vec_size = n / 8, n_left = vec_size - 4 * size_ilp;
    const TE* p = e + 4 * sub;  // the row at the lane's four columns
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float up[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    WidePairCols cur;
    if (size_ilp > 0) cur = wide_pair_load<T::kHalves, TE>(p, 0, H);
#pragma unroll 1
    for (int i = 0; i < size_ilp; ++i) {
        const WidePairCols nxt = wide_pair_load<T::kHalves, TE>(p, i + 1 < size_ilp ? 32 * (i + 1) : 32 * i, H);
        wide_pair_step<MODEL, SIDE>(acc, cur, coef, n4, 32 * i + 4 * sub);
        cur = nxt;
        if constexpr (CASCADE) {
            if (((i + 1) & 15) == 0) {  // after rows 16 and 32: one level up
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    up[c] = up[c] + acc[c];
                    acc[c] = 0.0f;
                }
            }
        }
    }
    if constexpr (CASCADE) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = acc[c] + up[c];
    }
    // the leftover vectors of 8: accumulators 0 .. 7, i.e. lanes 0 and 1 of the group
    for (int v = 0; v < n_left; ++v) {
        if (sub < 2) {
            const int col = 32 * size_ilp + 8 * v;
            const WidePairCols x = wide_pair_load<T::kHalves, TE>(p, col, H);
            wide_pair_step<MODEL, SIDE>(acc, x, coef, n4, col + 4 * sub);
        }
    }
    // the n % 8 tail terms, one after the other (every lane of the group the same)
    float s = 0.0f;
    for (int j = 8 * vec_size; j < n; ++j) {
        float ck[K];
#pragma unroll
        for (int k = 0; k < K; ++k) ck[k] = coef[k * n4 + j];
        s = s + T::term(wide_elem<TE>(e + j), T::kHalves ? wide_elem<TE>(e + H + j) : 0.0f, ck);
    }
    return wide_fold<MODEL>(acc, s);
}

}  // namespace blp
