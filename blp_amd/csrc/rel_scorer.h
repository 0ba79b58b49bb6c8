// rel_scorer.h -- the four score functions with the RELATION row as the lane-resident operand (rank_rels.hip): lane l holds
// row r of rel_emb in e[D], the query's head and tail vectors h, t are wave-uniform accessors (h(ic<i>), t(ic<i>): scalar
// loads -> SGPR operands, at most one per VALU instruction, which every expression below respects).
//
// The operation order is score_direct<MODEL>'s (score_direct.h), term by term: the candidate sits in the MIDDLE of the
// reference's expressions -- (h + r) - t, (h * r) * t, the ComplEx / SimplE products --, so none of them is Scorer<>'s
// "coefficient row against candidate row" form without changing a rounding.  Sums in score_core.h's orders: TransE strictly
// left to right, the bilinear models by torch_inner_sum.  score<true> is score_direct's value bit for bit (the literal
// "0 + first term" additions: the reference's sign of an all-zero sum); score<false> leaves them out and is the selection key
// (it compares equal under IEEE, -0 == +0).  Compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "score_core.h"

#pragma clang fp contract(off)

namespace blp {

template <int MODEL, int D>
struct RelScorer;

template <int D>
struct RelScorer<TRANSE, D> {  // -sum |(h + r) - t|; the differences kPipe ahead of the dependent adds (Scorer<TRANSE, HEAD>)
    template <bool LZ, class PH, class PT>
    __device__ __forceinline__ static float score(const float (&e)[D], const PH& h, const PT& t) {
        float x[kPipe];
        static_for<kPipe>([&](auto k) {
            constexpr int d = decltype(k)::value;
            const float y = h(ic<d>{}) + e[d];
            x[d] = y - t(ic<d>{});
        });
        float acc = 0.0f;
        static_for<D>([&](auto k) {
            constexpr int d = decltype(k)::value;
            const float cur = fabsf(x[d % kPipe]);
            if constexpr (d + kPipe < D) {
                const float y = h(ic<d + kPipe>{}) + e[d + kPipe];
                x[d % kPipe] = y - t(ic<d + kPipe>{});
            }
            acc = (d == 0 && !LZ) ? cur : acc + cur;
        });
        return -acc;
    }
};

template <int D>
struct RelScorer<DISTMULT, D> {  // sum (h * r) * t
    template <bool LZ, class PH, class PT>
    __device__ __forceinline__ static float score(const float (&e)[D], const PH& h, const PT& t) {
        return torch_inner_sum<D, LZ>([&](auto i) {
            const float x = h(i) * e[i];
            return x * t(i);
        });
    }
};

template <int D>
struct RelScorer<COMPLEX, D> {  // halves re = [0, H), im = [H, D): ((rr*hr)*tr + (rr*hi)*ti + (ri*hr)*ti) - (ri*hi)*tr
    static constexpr int H = D / 2;
    template <bool LZ, class PH, class PT>
    __device__ __forceinline__ static float score(const float (&e)[D], const PH& h, const PT& t) {
        return torch_inner_sum<H, LZ>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const float hr = h(ic<j>{}), hi = h(ic<H + j>{}), tr = t(ic<j>{}), ti = t(ic<H + j>{});  // (each read once)
            float a = e[j] * hr;       a = a * tr;
            float b = e[j] * hi;       b = b * ti;
            float c = e[H + j] * hr;   c = c * ti;
            float d = e[H + j] * hi;   d = d * tr;
            float s = a + b;
            s = s + c;
            return s - d;
        });
    }
};

template <int D>
struct RelScorer<SIMPLE, D> {  // h = [hh | ht], t = [th | tt], r = [ra | rb]: (sum (hh*ra)*tt + (th*rb)*ht) / 2
    static constexpr int H = D / 2;
    template <bool LZ, class PH, class PT>
    __device__ __forceinline__ static float score(const float (&e)[D], const PH& h, const PT& t) {
        const float s = torch_inner_sum<H, LZ>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            float a = h(ic<j>{}) * e[j];
            a = a * t(ic<H + j>{});
            float b = t(ic<j>{}) * e[H + j];
            b = b * h(ic<H + j>{});
            return a + b;
        });
        return s / 2.0f;
    }
};

}  // namespace blp
