// rerank.hip -- re-ranking a first-stage retrieval run with entity embeddings (include/blp_hip.h: blp_rerank_cosine,
// blp_rerank_ndcg; reference retrieval.py:139-258).
//
// rerank_cosine  s1[c] = F.normalize(table[row[c]]) . F.normalize(query[q])  for every candidate c of query q's segment.
//   One wave per candidate.  SUMMATION ORDER (every sum of the kernel -- the two squared norms and the dot product -- is
//   taken this way, and blp_amd.retrieval.cosine_restated restates it): lane l (0..63) accumulates the terms of elements
//   l, l + 64, l + 128, ... in that order into a partial that starts at +0.0f; the 64 partials are then folded as a tree,
//   p[l] = p[l] + p[l + h] for h = 32, 16, 8, 4, 2, 1, and the sum is p[0].  A term of the norms is x * x, of the dot
//   product (x_i / max(n_x, 1e-12f)) * (y_i / max(n_y, 1e-12f)) (max as torch's clamp_min: a NaN norm stays NaN);
//   n = sqrtf(sum); the division and the square root are the correctly rounded f32 operations.  Row -1 (no description)
//   gives exactly 0.0f; a row outside [-1, E) gives NaN (never read).
//
// rerank_ndcg    nDCG@k of every (alpha, query) as trec_eval's ndcg_cut computes it:
//   c = alpha * s1 + (1 - alpha) * s2 in f64 (two roundings, no FMA); candidates ordered by (float)c descending, equal
//   floats (-0 == +0) by the lower segment index (the host sorts a segment by docno descending), NaN last.  Each workgroup
//   holds one query's segment in registers (s1, s2: at most 8 per thread) and loops over a block of alphas: one unique
//   64-bit key per candidate, orderable(f32) << 32 | (0xFFFFFFFF - index), sorted descending by a bitonic sort in LDS; the
//   DCG terms gain / log2(i + 2) of the positions below the largest cutoff are computed in parallel (into the same LDS),
//   then wave 0 adds the non-zero ones in rank order (f64) and records the sum at each cutoff.
// Both kernels are deterministic (nothing depends on the grid or on timing) and use no scratch memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"

#pragma clang fp contract(off)

namespace blp {

typedef unsigned long long u64;

constexpr int kRerankCosineWaves = 4;  // waves (= candidates in flight) per workgroup of rerank_cosine

__device__ __forceinline__ float wave_tree_sum(float p) {
    // p[l] + p[l ^ h] is p[l] + p[l + h] for the lanes that go on (l < h): the tree of the header comment
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) p = p + __shfl_xor(p, h, 64);
    return __shfl(p, 0, 64);
}

__device__ __forceinline__ float clamp_norm(float n) { return n < 1e-12f ? 1e-12f : n; }

// Correctly rounded f32 square root of a non-negative sum (v_sqrt_f32 alone is within 1 ulp): the hardware estimate s, then
// the exact residuals x - s_down * s and x - s_up * s of its two neighbours pick the correctly rounded one of the three
// (the refinement LLVM emits for a correctly rounded sqrt).  Tiny arguments are scaled by 2^32 first.
__device__ __forceinline__ float sqrt_rn(float x) {
    if (!(x > 0.0f) || __builtin_isinf(x)) return x == 0.0f ? x : __builtin_amdgcn_sqrtf(x);
    const bool tiny = x < 0x1p-96f;
    const float xs = tiny ? x * 0x1p+32f : x;
    const float s = __builtin_amdgcn_sqrtf(xs);
    const float down = __uint_as_float(__float_as_uint(s) - 1u);
    const float up = __uint_as_float(__float_as_uint(s) + 1u);
    const float r_down = __builtin_fmaf(-down, s, xs), r_up = __builtin_fmaf(-up, s, xs);
    const float r = r_up > 0.0f ? up : (r_down <= 0.0f ? down : s);
    return tiny ? r * 0x1p-16f : r;
}

__global__ __launch_bounds__(64 * kRerankCosineWaves) void rerank_cosine_kernel(
    const float* __restrict__ table, int64_t E, int D, int64_t ld, const float* __restrict__ query, int64_t Q, int64_t ldq,
    const int64_t* __restrict__ cand_ptr, const int32_t* __restrict__ cand_row, int64_t C, float* __restrict__ s1) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kRerankCosineWaves + (threadIdx.x >> 6);
    if (c >= C) return;
    const int64_t row = cand_row[c];
    if (row == -1) {
        if (lane == 0) s1[c] = 0.0f;
        return;
    }
    // the query of candidate c: the last q with cand_ptr[q] <= c (empty segments are skipped over)
    int64_t lo = 0, hi = Q;  // cand_ptr[lo] <= c < cand_ptr[hi] for a well-formed CSR (checked below)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (cand_ptr[mid] <= c) lo = mid; else hi = mid;
    }
    if (row < -1 || row >= E || c < cand_ptr[lo] || c >= cand_ptr[hi]) {
        if (lane == 0) s1[c] = __int_as_float(0x7fc00000);
        return;
    }
    const float* x = table + row * ld;
    const float* y = query + lo * ldq;
    float px = 0.0f, py = 0.0f;
    for (int i = lane; i < D; i += 64) {
        const float a = x[i], b = y[i];
        px = px + a * a;
        py = py + b * b;
    }
    const float nx = clamp_norm(sqrt_rn(wave_tree_sum(px)));
    const float ny = clamp_norm(sqrt_rn(wave_tree_sum(py)));
    float p = 0.0f;
    for (int i = lane; i < D; i += 64) p = p + __fdiv_rn(x[i], nx) * __fdiv_rn(y[i], ny);
    const float s = wave_tree_sum(p);
    if (lane == 0) s1[c] = s;
}

__device__ __forceinline__ u64 rerank_key(double c, int index) {
    const float f = (float)c;
    unsigned hi;
    if (__builtin_isnan(f)) {
        hi = 0u;  // below every number; still above the padding key 0 (the low word is never 0 for index < 2^32 - 1)
    } else {
        unsigned b = __float_as_uint(f);
        if (b == 0x80000000u) b = 0u;  // -0 == +0
        hi = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    return ((u64)hi << 32) | (u64)(0xFFFFFFFFu - (unsigned)index);
}

// One workgroup = one query x one block of alphas.  T threads, n_pad = T * PER keys (a power of two >= the segment).
template <int PER>
__global__ __launch_bounds__(1024) void rerank_ndcg_kernel(
    const float* __restrict__ s1, const double* __restrict__ s2, const int32_t* __restrict__ gain,
    const int64_t* __restrict__ cand_ptr, int64_t Q, int64_t C, const double* __restrict__ alphas, int A,
    int alphas_per_block, RerankCutoffs cuts, const double* __restrict__ log2_table, const double* __restrict__ idcg,
    int64_t max_segment, double* __restrict__ ndcg) {
    extern __shared__ u64 keys[];  // n_pad keys; after the sort, the DCG terms (as doubles) in rank order
    const int T = blockDim.x;
    const int n_pad = T * PER;
    const int t = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int a0 = blockIdx.y * alphas_per_block;
    const int a1 = min(A, a0 + alphas_per_block);
    const int64_t base = cand_ptr[q];
    const int64_t n64 = cand_ptr[q + 1] - base;
    const int n_cut = cuts.n;
    if (base < 0 || n64 < 0 || n64 > max_segment || n64 > n_pad || base + n64 > C) {
        // a segment longer than the caller's max_segment (or a malformed CSR): NaN, nothing of it read
        if (t < n_cut)
            for (int a = a0; a < a1; ++a) ndcg[((int64_t)a * Q + q) * n_cut + t] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const int n = (int)n64;
    float r1[PER];
    double r2[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int i = t + e * T;
        r1[e] = i < n ? s1[base + i] : 0.0f;
        r2[e] = i < n ? s2[base + i] : 0.0;
    }
    const int kmax = cuts.k[n_cut - 1];
    const int m = n < kmax ? n : kmax;  // the positions that can count
    for (int a = a0; a < a1; ++a) {
        const double al = alphas[a];
        const double bl = 1.0 - al;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int i = t + e * T;
            keys[i] = i < n ? rerank_key(al * (double)r1[e] + bl * r2[e], i) : 0ull;
        }
        __syncthreads();
        // bitonic sort, descending (padding keys 0 end up last)
        for (int k = 2; k <= n_pad; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int p = t; p < (n_pad >> 1); p += T) {
                    const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                    const int l = i | j;
                    const u64 ki = keys[i], kl = keys[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? (ki < kl) : (ki > kl)) {
                        keys[i] = kl;
                        keys[l] = ki;
                    }
                }
                __syncthreads();
            }
        }
        // DCG terms of the positions below m, in parallel (0 for an unjudged or non-positive gain)
        double term[PER];
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int i = t + e * T;
            term[e] = 0.0;
            if (i < m) {
                const int idx = (int)(0xFFFFFFFFu - (unsigned)keys[i]);
                const int g = gain[base + idx];
                if (g > 0) term[e] = (double)g / log2_table[i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int i = t + e * T;
            if (i < m) reinterpret_cast<double*>(keys)[i] = term[e];
        }
        __syncthreads();
        // the additions, one at a time in rank order (wave 0; loop bounds and sum are wave-uniform); lane j keeps DCG@k_j
        if (t < 64) {
            double acc = 0.0, mine = 0.0;
            int next_cut = 0;
            for (int c0 = 0; c0 < m; c0 += 64) {
                const int i = c0 + t;
                const double v = i < m ? reinterpret_cast<const double*>(keys)[i] : 0.0;
                u64 mask = __ballot(v > 0.0);
                while (mask) {
                    const int b = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    while (next_cut < n_cut && cuts.k[next_cut] <= c0 + b) {
                        if (t == next_cut) mine = acc;
                        ++next_cut;
                    }
                    acc = acc + __shfl(v, b, 64);
                }
            }
            for (; next_cut < n_cut; ++next_cut)
                if (t == next_cut) mine = acc;
            if (t < n_cut) {
                const double id = idcg[q * n_cut + t];
                ndcg[((int64_t)a * Q + q) * n_cut + t] = id > 0.0 ? mine / id : 0.0;
            }
        }
        __syncthreads();  // the next alpha overwrites the keys
    }
}

hipError_t launch_rerank_cosine(const float* table, int64_t E, int D, int64_t ld, const float* query, int64_t Q, int64_t ldq,
                                const int64_t* cand_ptr, const int32_t* cand_row, int64_t C, float* s1, hipStream_t stream) {
    if (C == 0) return hipSuccess;
    const int64_t groups = (C + kRerankCosineWaves - 1) / kRerankCosineWaves;
    hipLaunchKernelGGL(rerank_cosine_kernel, dim3((unsigned)groups), dim3(64 * kRerankCosineWaves), 0, stream, table, E, D, ld,
                       query, Q, ldq, cand_ptr, cand_row, C, s1);
    return hipGetLastError();
}

hipError_t launch_rerank_ndcg(const float* s1, const double* s2, const int32_t* gain, const int64_t* cand_ptr, int64_t Q,
                              int64_t C, const double* alphas, int A, const RerankCutoffs& cuts, const double* log2_table,
                              const double* idcg, int64_t max_segment, double* ndcg, hipStream_t stream) {
    if (Q == 0 || A == 0) return hipSuccess;
    int n_pad = 64;
    while (n_pad < max_segment) n_pad <<= 1;
    int T = n_pad >> 1;
    T = T < 64 ? 64 : (T > 1024 ? 1024 : T);
    const int per = n_pad / T;  // 1, 2, 4 or 8
    // alphas per workgroup: enough workgroups to fill the device several times over; a segment is read once per block
    int apb = (int)(((int64_t)A * Q + 2047) / 2048);
    apb = apb < 1 ? 1 : (apb > A ? A : apb);
    const dim3 grid((unsigned)Q, (unsigned)((A + apb - 1) / apb));
    const size_t lds = (size_t)n_pad * sizeof(u64);
    switch (per) {
#define BLP_RERANK_NDCG(P)                                                                                                   \
    case P:                                                                                                                  \
        hipLaunchKernelGGL(rerank_ndcg_kernel<P>, grid, dim3(T), lds, stream, s1, s2, gain, cand_ptr, Q, C, alphas, A, apb,  \
                           cuts, log2_table, idcg, max_segment, ndcg);                                                       \
        break;
        BLP_RERANK_NDCG(1)
        BLP_RERANK_NDCG(2)
        BLP_RERANK_NDCG(4)
        BLP_RERANK_NDCG(8)
#undef BLP_RERANK_NDCG
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace blp
