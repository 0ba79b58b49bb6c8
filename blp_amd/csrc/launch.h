// launch.h -- host-side launchers implemented in the .hip files, called by the C-ABI in api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace blp {

// The filtered setting (train.py:159-171) for a block of Q queries: query q loses the candidates listed in
// val[lo[q] .. hi[q]).  Two layouts share these fields (include/blp_hip.h: blp_filter):
//   CSR       lo = rowptr, hi = rowptr + 1, val = table rows, nothing else set;
//   segments  [lo[q], hi[q]) is a slice of a sorted index of the filtering graph (blp_amd.utils.FilterIndex),
//             val = entity ids, exclude[q] = the triple's own entity (never filtered, utils.py:71,78), ent2idx maps
//             ids to table rows (-1 or beyond its length: not a candidate, utils.py:72,79).
// row_base is subtracted from every row and rows outside [0, N) are skipped (candidate shards).
// The query vectors of a block, q_fixed / q_rel, are (Q, D) row arrays -- either DENSE (row q = base + q * D) or INDEXED
// (row q = base + idx[q] * ld: the fixed-entity vector is a row of the entity table, the relation vector a row of
// rel_emb).  Indexed queries cost no gather and no 2 x Q x D x 4 bytes that every prep / true-key / refinement /
// filter kernel would stream again; their rows come out of L2 instead.  Kernels address both forms through row(q)
// (and flat(offset, D) for the few element-wise sweeps, D the caller's -- usually compile-time -- width).
struct QRows {
    const float* base = nullptr;
    const int64_t* idx = nullptr;  // NULL: dense
    int64_t ld = 0;                // row stride in floats (dense: D)
    __host__ __device__ const float* row(int64_t q) const { return base + (idx ? idx[q] : q) * ld; }
    __host__ __device__ const float* flat(int64_t off, int D) const {
        const int64_t q = off / D;
        return row(q) + (off - q * D);
    }
    static QRows dense(const float* p, int D) { return make(p, nullptr, D); }
    static QRows rows_of(const float* table, const int64_t* idx, int64_t ld) { return make(table, idx, ld); }
    static QRows make(const float* p, const int64_t* idx, int64_t ld) {
        QRows r;
        r.base = p; r.idx = idx; r.ld = ld;
        return r;
    }
};

struct FilterSpec {
    const int64_t* lo = nullptr;
    const int64_t* hi = nullptr;
    const int64_t* val = nullptr;
    const int64_t* exclude = nullptr;
    const int64_t* ent2idx = nullptr;
    int64_t ent2idx_len = 0;
    int64_t row_base = 0;
    __host__ __device__ bool on() const { return lo != nullptr; }
};

bool rank_sad_wide_applicable(int model, int D, int64_t q_head, int64_t q_tail);
size_t rank_all_workspace_bytes(int model, int D, int64_t N, int64_t q_head, int64_t q_tail);

hipError_t launch_rank_all(int model, int D, const float* table, int64_t N, int64_t ld,
                           const QRows q_fixed, const QRows q_rel,
                           const QRows q_true, int64_t q_head, int64_t q_tail,
                           const FilterSpec& filter, int32_t* counts,
                           void* workspace, int n_cu, hipStream_t stream, hipEvent_t ev_start = nullptr,
                           hipEvent_t ev_stop = nullptr);

// rank_all_wide.hip: the exact table pass for DistMult / ComplEx / SimplE at any width (D % 4 == 0, 4 <= D <= 1024;
// include/blp_hip.h: blp_rank_all_wide): launch_rank_all's arguments; the workspace holds the true keys and the accumulators
bool rank_all_wide_supported(int model, int D);
size_t rank_all_wide_workspace_bytes(int64_t q_head, int64_t q_tail);
hipError_t launch_rank_all_wide(int model, int D, const float* table, int64_t N, int64_t ld, const QRows q_fixed, const QRows q_rel,
                                const QRows q_true, int64_t q_head, int64_t q_tail, const FilterSpec& filter, int32_t* counts,
                                void* workspace, int n_cu, hipStream_t stream, hipEvent_t ev_start = nullptr,
                                hipEvent_t ev_stop = nullptr);

// rank_sets_wide_bilinear.hip: the same arithmetic inside candidate sets shared between queries (include/blp_hip.h:
// blp_rank_sets_wide_bilinear).  Its launcher takes a SetLookup and is declared beside it and launch_rank_sets_wide, in
// rank_common.h: rank_sets_wide_bilinear_supported, rank_sets_wide_bilinear_workspace_bytes, launch_rank_sets_wide_bilinear.

// rank_all.hip: many passes of <= 4 + 4 queries back to back (one preparation and one finalisation launch for all of them)
bool rank_static_passes_applicable(int model, int D, int64_t N, int64_t batch);
size_t rank_static_passes_workspace_bytes(int D, int64_t n, int64_t batch);
// (table: f32, or a 16-bit table -- dtype: table_elem.h -- when rank_stream16_takes_passes says so)
hipError_t launch_rank_static_passes(int model, int D, const void* table, int dtype, int64_t N, int64_t ld, const QRows q_fixed,
                                     const QRows q_rel, const QRows q_true, int64_t n, int64_t batch, const FilterSpec& filter,
                                     int32_t* counts, void* workspace, int n_cu, hipStream_t stream, hipEvent_t ev_start,
                                     hipEvent_t ev_stop);

// queries.hip: every batch of the reference's evaluation loop in one call (include/blp_hip.h: blp_rank_all_batches)
size_t rank_all_batches_workspace_bytes(int model, int D, int64_t N, int64_t n, int64_t batch, int64_t block_triples);
int64_t rank_all_batches_passes_per_launch(int model, int D, int64_t N, int64_t ld, int64_t n, int64_t batch, int64_t block_triples);
hipError_t launch_rank_all_batches(int model, int D, const float* table, int64_t N, int64_t ld, const float* source, int64_t ld_src,
                                   const int64_t* fixed_row, const float* rel_emb, const int64_t* rel_id, const int64_t* true_row,
                                   int64_t n, int64_t batch, int64_t block_triples, const FilterSpec& filter, int32_t* counts,
                                   void* workspace, int n_cu, hipStream_t stream, hipEvent_t ev_start = nullptr,
                                   hipEvent_t ev_stop = nullptr);

// ... with the candidate table in a 16-bit storage type (include/blp_hip.h: blp_rank_all_batches)
bool rank_all_batches_native16(int model, int D, int64_t N, int64_t ld, int64_t n, int64_t batch, int64_t block_triples);
size_t rank_all_batches16_workspace_bytes(int model, int D, int64_t N, int64_t ld, int64_t n, int64_t batch, int64_t block_triples);
hipError_t launch_rank_all_batches16(int model, int D, const void* table, int dtype, int64_t N, int64_t ld, const float* source,
                                     int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, const int64_t* rel_id,
                                     const int64_t* true_row, int64_t n, int64_t batch, int64_t block_triples, const FilterSpec& filter,
                                     int32_t* counts, void* workspace, int n_cu, hipStream_t stream, hipEvent_t ev_start = nullptr,
                                     hipEvent_t ev_stop = nullptr);

// rank_all.hip: prep_coef_kernel's coefficient rows alone (C floats per query, Scorer<MODEL, SIDE, D>::C)
hipError_t launch_prep_coef(int model, int D, const QRows q_fixed, const QRows q_rel, int64_t q_head, int64_t q_tail,
                            float* coef_head, float* coef_tail, hipStream_t stream);

// topk.hip: filtered top-k over the candidate table (include/blp_hip.h: blp_topk, blp_topk_typed, blp_topk_merge); the
// table f32 or 16-bit (dtype: table_elem.h; the workspace does not depend on it)
bool topk_supported(int model, int D, int k);
bool topk_typed_supported(int model, int dtype, int D, int k);
size_t topk_workspace_bytes(int model, int D, int64_t N, int64_t q_head, int64_t q_tail, int k);
hipError_t launch_topk(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, int64_t row_base, const QRows q_fixed,
                       const QRows q_rel, int64_t q_head, int64_t q_tail, int k, const FilterSpec& filter, int64_t* rows,
                       float* scores, void* workspace, hipStream_t stream);
hipError_t launch_topk_merge(const int64_t* rows, const float* scores, int64_t Q, int64_t n_in, int k, int64_t* rows_out,
                             float* scores_out, hipStream_t stream);

// topk_wide.hip: launch_topk for DistMult / ComplEx / SimplE at any width (D % 4 == 0, 4 <= D <= 1024; include/blp_hip.h:
// blp_topk_wide), an f32 table; the workspace holds the partial key lists only.  topk_wide_lds_bytes: the dynamic LDS the
// table pass of one side (HEAD / TAIL) is launched with.
bool topk_wide_supported(int model, int D, int k);
size_t topk_wide_workspace_bytes(int64_t N, int64_t q_head, int64_t q_tail, int k);
size_t topk_wide_lds_bytes(int model, int side, int D, int k);
hipError_t launch_topk_wide(int model, int D, const float* table, int64_t N, int64_t ld, int64_t row_base, const QRows q_fixed,
                            const QRows q_rel, int64_t q_head, int64_t q_tail, int k, const FilterSpec& filter, int64_t* rows,
                            float* scores, void* workspace, hipStream_t stream);

// topk.hip's second and third stage for topk_sets.hip: the k best of (Q, n_in) keys (topk_lists.h; 0 = an empty slot) ->
// rows / scores, and the winners of an f32 table re-scored by Scorer<>::score<true>
hipError_t launch_topk_merge_keys(const unsigned long long* keys, int64_t Q, int64_t n_in, int k, int64_t* rows_out, float* scores_out,
                                  hipStream_t stream);
hipError_t launch_topk_rescore(int model, int D, const float* table, int64_t ld, int64_t row_base, const QRows q_fixed, const QRows q_rel,
                               int64_t q_head, int64_t Q, int k, const int64_t* rows, float* scores, hipStream_t stream);
// ... of a table of any storage type (dtype: table_elem.h; ld in elements), re-scored on the rows widened to f32
hipError_t launch_topk_rescore_typed(int model, int D, int dtype, const void* table, int64_t ld, int64_t row_base, const QRows q_fixed,
                                     const QRows q_rel, int64_t q_head, int64_t Q, int k, const int64_t* rows, float* scores,
                                     hipStream_t stream);

// rank_lists.hip: counts and scores of per-query candidate lists (include/blp_hip.h: blp_rank_lists); q_true.base == nullptr
// with counts == nullptr: scores only.  The workspace holds the true keys (needed with counts only).
bool rank_lists_supported(int model, int dtype, int D);
size_t rank_lists_workspace_bytes(int64_t q_head, int64_t q_tail);
hipError_t launch_rank_lists(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, int64_t row_base,
                             const QRows q_fixed, const QRows q_rel, const QRows q_true, int64_t q_head, int64_t q_tail,
                             const int64_t* list_ptr, const int64_t* list_row, int64_t nnz, const FilterSpec& filter, int32_t* counts,
                             float* scores, void* workspace, hipStream_t stream);

// rank_lists_wide.hip: the same contract for DistMult / ComplEx / SimplE at any D % 4 == 0, 4 <= D <= 1024 (include/blp_hip.h:
// blp_rank_lists_wide), by wide_bilinear.h's arithmetic; launch_rank_lists' argument list.
bool rank_lists_wide_supported(int model, int dtype, int D);
size_t rank_lists_wide_workspace_bytes(int64_t q_head, int64_t q_tail);
hipError_t launch_rank_lists_wide(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, int64_t row_base,
                                  const QRows q_fixed, const QRows q_rel, const QRows q_true, int64_t q_head, int64_t q_tail,
                                  const int64_t* list_ptr, const int64_t* list_row, int64_t nnz, const FilterSpec& filter,
                                  int32_t* counts, float* scores, void* workspace, hipStream_t stream);

// lists_topk.hip: filtered top-k inside per-query candidate lists (include/blp_hip.h: blp_topk_lists): rank_lists' queries,
// table and lists, topk's output.  The workspace holds the (Q, S, k) partial key lists when a query's list is cut into S > 1
// slabs (S from Q and nnz alone), else nothing.
bool topk_lists_supported(int model, int dtype, int D, int k);
size_t topk_lists_workspace_bytes(int64_t q_head, int64_t q_tail, int64_t nnz, int k);
hipError_t launch_topk_lists(int model, int D, int dtype, const void* table, int64_t N, int64_t ld, int64_t row_base,
                             const QRows q_fixed, const QRows q_rel, int64_t q_head, int64_t q_tail, const int64_t* list_ptr,
                             const int64_t* list_row, int64_t nnz, int k, const FilterSpec& filter, int64_t* rows, float* scores,
                             void* workspace, hipStream_t stream);

// rank_rels.hip: relation prediction (include/blp_hip.h: blp_rank_relations, blp_topk_relations): query q = rows head_row[q],
// tail_row[q] of `source`; the candidates are all R rows of rel_emb (contiguous); the filter's values are relation ids.
// counts and / or scores (Q, R; row stride ld_scores); the workspace holds the true keys (needed with counts only).  The top-k
// call needs no workspace.
bool rank_relations_supported(int model, int D);
size_t rank_relations_workspace_bytes(int64_t Q);
hipError_t launch_rank_relations(int model, int D, const float* source, int64_t ld_src, const int64_t* head_row, const int64_t* tail_row,
                                 int64_t Q, const float* rel_emb, int64_t R, const int64_t* true_rel, const FilterSpec& filter,
                                 int32_t* counts, float* scores, int64_t ld_scores, void* workspace, hipStream_t stream);
bool topk_relations_supported(int model, int D, int k);
hipError_t launch_topk_relations(int model, int D, const float* source, int64_t ld_src, const int64_t* head_row, const int64_t* tail_row,
                                 int64_t Q, const float* rel_emb, int64_t R, int k, const FilterSpec& filter, int64_t* rels, float* scores,
                                 hipStream_t stream);

// rank_rels_wide.hip: the same two calls for TransE at any width (D % 4 == 0, 4 <= D <= 1024; include/blp_hip.h:
// blp_rank_relations_wide, blp_topk_relations_wide): same arguments, same workspace (rank_relations_workspace_bytes; top-k none)
bool rank_relations_wide_supported(int model, int D);
hipError_t launch_rank_relations_wide(int model, int D, const float* source, int64_t ld_src, const int64_t* head_row,
                                      const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R, const int64_t* true_rel,
                                      const FilterSpec& filter, int32_t* counts, float* scores, int64_t ld_scores, void* workspace,
                                      hipStream_t stream);
bool topk_relations_wide_supported(int model, int D, int k);
hipError_t launch_topk_relations_wide(int model, int D, const float* source, int64_t ld_src, const int64_t* head_row,
                                      const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R, int k, const FilterSpec& filter,
                                      int64_t* rels, float* scores, hipStream_t stream);

// rank_rels_wide_bilinear.hip: the same two calls for DistMult / ComplEx / SimplE at any width (D % 4 == 0, 4 <= D <= 1024;
// include/blp_hip.h: blp_rank_relations_wide_bilinear, blp_topk_relations_wide_bilinear): same arguments, same workspace
// (rank_relations_workspace_bytes; top-k none)
bool rank_relations_wide_bilinear_supported(int model, int D);
hipError_t launch_rank_relations_wide_bilinear(int model, int D, const float* source, int64_t ld_src, const int64_t* head_row,
                                               const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R,
                                               const int64_t* true_rel, const FilterSpec& filter, int32_t* counts, float* scores,
                                               int64_t ld_scores, void* workspace, hipStream_t stream);
bool topk_relations_wide_bilinear_supported(int model, int D, int k);
hipError_t launch_topk_relations_wide_bilinear(int model, int D, const float* source, int64_t ld_src, const int64_t* head_row,
                                               const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R, int k,
                                               const FilterSpec& filter, int64_t* rels, float* scores, hipStream_t stream);

// rerank.hip: re-ranking a retrieval run (include/blp_hip.h: blp_rerank_cosine, blp_rerank_ndcg)
constexpr int kRerankMaxSegment = 8192;  // candidates per query: 8 192 keys of 8 bytes = 64 KiB of LDS
constexpr int kRerankMaxCutoffs = 8;
struct RerankCutoffs {  // ascending cutoffs, passed by value as a kernel argument
    int n;
    int k[kRerankMaxCutoffs];
};
hipError_t launch_rerank_cosine(const float* table, int64_t E, int D, int64_t ld, const float* query, int64_t Q, int64_t ldq,
                                const int64_t* cand_ptr, const int32_t* cand_row, int64_t C, float* s1, hipStream_t stream);
hipError_t launch_rerank_ndcg(const float* s1, const double* s2, const int32_t* gain, const int64_t* cand_ptr, int64_t Q,
                              int64_t C, const double* alphas, int A, const RerankCutoffs& cuts, const double* log2_table,
                              const double* idcg, int64_t max_segment, double* ndcg, hipStream_t stream);

hipError_t launch_rank_metrics(const int32_t* counts, int64_t Q, const int32_t* k, float* rr,
                               uint8_t* hits, hipStream_t stream);

hipError_t launch_rank_from_scores(const float* scores, int64_t Q, int64_t N, int64_t ld, const int64_t* true_idx,
                                   const float* true_score, const int64_t* rowptr, const int64_t* col,
                                   int32_t* counts, hipStream_t stream);

// queries.hip: blp_build_queries (include/blp_hip.h: blp_queries, same fields)
struct QueryBuild {
    const int64_t* triples; int64_t n, block;
    const int64_t* ent2idx; int64_t ent2idx_len;
    const float* source; int64_t src_rows, ld; int D;
    const float* rel_emb; int64_t R;
    const int64_t* heads_key; int64_t n_heads;
    const int64_t* tails_key; int64_t n_tails;
    int64_t index_R;
    float* q_fixed; float* q_rel; int64_t* true_row; int64_t* rel_ids; int* ids_min;
    int64_t* seg_lo; int64_t* seg_hi; int64_t* exclude;
    int64_t* fixed_row;
    int64_t by_position;  // source = [head vectors of the n triples | tail vectors] (launch_gather_triple_vectors)
};
hipError_t launch_build_queries(const QueryBuild& a, hipStream_t stream);
hipError_t launch_gather_triple_vectors(const int64_t* triples, int64_t n, const int64_t* ent2idx, int64_t ent2idx_len,
                                        const void* table, int dtype, int64_t N, int D, int64_t ld, int64_t row_base, float* out,
                                        hipStream_t stream);

bool project_rows_supported(int E, int D);
hipError_t launch_project_rows(const float* x, int64_t n, int64_t ldx, const float* w, int E, int D, int normalize,
                               float* out, int64_t ldo, hipStream_t stream);

bool bow_rows_supported(int E);
hipError_t launch_bow_rows(const int64_t* tok, const float* mask, int64_t n, int L, const float* emb, int64_t V, int E,
                           int normalize, float* out, int64_t ldo, int* bad_tok, hipStream_t stream);

bool dkrl_rows_supported(int E, int D, int L);
hipError_t launch_dkrl_rows(const int64_t* tok, const float* mask, int64_t n, int L, const float* emb, int64_t V, int E,
                            const float* w1, const float* b1, const float* w2, const float* b2, int normalize, float* out,
                            int64_t ldo, int* bad_tok, int n_cu, hipStream_t stream);

struct StridedRows {  // row(i0, i1) = base + i0 * s0 + i1 * s1   (strides in floats)
    const float* base;
    int64_t s0, s1;
};

hipError_t launch_rank_metric_sums(const int32_t* counts, int64_t Q, const int32_t* k, double* sums,
                                   hipStream_t stream);

hipError_t launch_score_fwd(int model, int D, int64_t M0, int64_t M1, StridedRows h, StridedRows t,
                            StridedRows r, float* out, hipStream_t stream);
hipError_t launch_score_bwd(int model, int D, int64_t M0, int64_t M1, StridedRows h, StridedRows t,
                            StridedRows r, const float* grad_out, float* grad_h, float* grad_t,
                            float* grad_r, hipStream_t stream);

hipError_t launch_inbatch_loss_fwd(int model, int loss, int ent_dtype, int rel_dtype, const void* ent, const void* rel,
                                   const int64_t* neg_idx, int B, int K, int D, float regularizer,
                                   float* out_loss, float* save_pos, float* save_neg, unsigned* ticket, hipStream_t stream);
size_t inbatch_loss_save_floats(int model, int B, int K, int D);
int inbatch_loss_fwd_launches(int model, int B, int K, int D, bool regularised);
hipError_t launch_inbatch_loss_bwd(int model, int loss, int ent_dtype, int rel_dtype, const void* ent, const void* rel,
                                   const int64_t* neg_idx, int B, int K, int D, float regularizer,
                                   const float* grad_loss, const float* save_pos, const float* save_neg,
                                   void* grad_ent, void* grad_rel, hipStream_t stream);

}  // namespace blp
