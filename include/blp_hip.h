/*
 * blp_hip.h -- C-ABI of libblp_hip.so: MI355X (gfx950) kernels for the link-prediction
 * scoring / ranking hot path of dfdazac/blp.
 *
 * The reference is Python/PyTorch and has no FFI of its own; this is the boundary a maintainer
 * binds with ctypes (INTEGRATION.md shows the stub).  Each entry point names the reference
 * expression it replaces (file:line under the reference checkout).
 *
 * Conventions (every call):
 *   - plain C types; every pointer except `workspace`-free host outputs is a DEVICE pointer owned
 *     by the caller (torch: tensor.data_ptr()); nothing is allocated or freed inside a call;
 *   - `device` is the HIP device ordinal the pointers live on, `stream` a hipStream_t (torch:
 *     torch.cuda.current_stream().cuda_stream; NULL = the legacy default stream).  Calls only
 *     enqueue work on `stream`: no host synchronisation, safe to capture in a hipGraph (one exception, once per device:
 *     blp_selftest below);
 *   - re-entrant: no process-wide mutable state except the per-device verdict of the matrix-pipe self-test (blp_selftest:
 *     written once, under a mutex; the test knobs exist only in the -DBLP_TEST_HOOKS build, see the end of this file); one thread per device (nn.DataParallel replicas) may call concurrently.  ctypes releases
 *     the GIL for the duration of the call;
 *   - return 0 (BLP_OK) or a negative blp_status; blp_last_error() gives the thread-local message;
 *   - f32 tensors, int64 indices exactly as the reference produces them (neg_idx, true_idx);
 *   - arithmetic follows the torch-CPU evaluation order of the reference expressions (see
 *     oracle/blp_oracle.c), so scores are bit-identical and rank counts are exact.
 */
#ifndef BLP_HIP_H
#define BLP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLP_HIP_VERSION 60000 /* major*10000 + minor*100 + patch; 6.0.0: the in-batch loss in two launches (fwd takes a ticket
                                 counter, save_pos sized by blp_inbatch_loss_save_floats); entry points pruned: ONE form per
                                 operation (storage-typed, filter as blp_filter), q_rel_id gone */

typedef enum blp_status {
    BLP_OK = 0,
    BLP_ERR_BAD_ARG = -1,         /* null / misaligned pointer, negative size, bad enum     */
    BLP_ERR_UNSUPPORTED_DIM = -2, /* D not in the compiled set (see blp_dim_supported)      */
    BLP_ERR_HIP = -3,             /* a HIP runtime call failed; message has hipGetErrorString */
    BLP_ERR_WORKSPACE = -4        /* workspace NULL / too small / misaligned                */
} blp_status;

/* rel_model of models.py:16-26 */
typedef enum blp_model { BLP_TRANSE = 0, BLP_DISTMULT = 1, BLP_COMPLEX = 2, BLP_SIMPLE = 3 } blp_model;
/* loss_fn of models.py:31-36 */
typedef enum blp_loss { BLP_LOSS_MARGIN = 0, BLP_LOSS_NLL = 1 } blp_loss;

typedef struct blp_caps {
    int compute_units;        /* 256 on MI355X                      */
    int wavefront_size;       /* 64                                 */
    int lds_bytes_per_cu;     /* 163840                             */
    int clock_mhz;            /* max engine clock                   */
    int64_t hbm_bytes;        /* total device memory                */
    char arch[32];            /* "gfx950..."                        */
    int mfma_bf16_accum;      /* verdict of the matrix-pipe self-test on this device (blp_selftest): 0 = not run yet,
                                 1 = passed (bilinear blocks use the bf16 x 3 MFMA pre-pass), 2 = FAILED (they use the
                                 f32-chain pre-pass, ~3.5 x slower, same results)                              */
    float mfma_bf16_accum_worst; /* the largest |S~ - S3| / (262 u T) the self-test measured; it fails at 0.5 */
} blp_caps;

int blp_version(void);
const char *blp_last_error(void);
int blp_device_caps(int device, blp_caps *out);

/* The matrix-pipe self-test behind the bilinear pre-pass (DistMult / ComplEx / SimplE blocks of >= 32 queries).  That
 * pre-pass decides most (query, candidate) pairs from a bf16 x 3 MFMA product inside an error band; every term of the
 * band is arithmetic except one: how v_mfma_f32_32x32x16_bf16 rounds its 16-term accumulation, which the ISA does not
 * document.  Once per device this library therefore pushes adversarial operand sets (same-sign runs, one huge term among
 * tiny ones, exact cancellation, 2^-60 / 2^50 scales, all-ones significands) through the pre-pass's own MFMA sequence
 * and compares every accumulator with the exactly evaluated split sum against HALF of what the band allows.  A device
 * that fails is served by the f32-chain pre-pass (exact fused multiply-adds; its band needs no assumption) -- the results
 * are the same either way, only the speed differs.
 *   blp_selftest(device, stream)  runs it now if it has not run on `device` (allocates and frees 4 096 bytes, enqueues on
 *        `stream` and WAITS for it -- a set-up call, not to be captured into a graph); returns the verdict (1 / 2) or a
 *        negative status.  CALL IT AT SET-UP (blp_amd.ops does, before the first bilinear ranking call of a device): a
 *        caller that does not leaves it to the first bilinear blp_rank_all* call on the device, which then runs it by
 *        itself with its workspace as scratch -- that ONE call holds a process-wide mutex and synchronises `stream`
 *        (several threads making their first calls together are serialised by it); if `stream` is being captured the
 *        verdict stays open and that call takes the f32-chain pre-pass.
 * This per-device verdict (an int, written once under a mutex) is the library's only process-wide state. */
int blp_selftest(int device, void *stream);
/* storage types of the arrays that may come in 16 bits (the in-batch loss' embeddings; the candidate table of
 * blp_rank_all_batches) */
enum { BLP_DTYPE_F32 = 0, BLP_DTYPE_F16 = 1, BLP_DTYPE_BF16 = 2 };

/* 1 if kernels are compiled for embedding width D of `model` (D % 32 == 0, D <= 256; the
 * half-width models complex / simple additionally need D % 64 == 0). */
int blp_dim_supported(int model, int D);

/* --------------------------------------------------------------------------------------------
 * All-entities ranking  (replaces train.py:146-171 + utils.py:103-105 for one block of queries)
 *
 *   heads_predictions = score_fn(ent_emb, tail_embs, rel_embs)      train.py:146
 *   tails_predictions = score_fn(head_embs, ent_emb, rel_embs)      train.py:147
 *   pred_ents = cat(heads_predictions, tails_predictions)           train.py:149
 *   best = (pred > true).sum + 1 ; worst = (pred >= true).sum       utils.py:103-105
 *   pred_ents[filter_mask] = pred_ents.min() - 1.0 ; get_metrics    train.py:165-167
 *
 * One call streams the (N, D) candidate table once and serves Q = q_head + q_tail queries:
 * queries [0, q_head) replace the HEAD (q_fixed = tail embedding), queries [q_head, Q) replace
 * the TAIL (q_fixed = head embedding) -- the same "head queries first" order as train.py:149.
 * The (Q, N) score matrix is never materialised.  Results are the reference's, bit for bit, whichever
 * kernel serves the block: exact f32 kernels for small blocks; for blocks of many
 * queries a cheap pre-pass (16-bit fixed-point v_sad_u16 for TransE, bf16 x 3 MFMA GEMM for the
 * bilinear models) with a rigorous error band, then exact re-scoring of the undecided pairs -- and when a pre-pass leaves
 * more undecided than its lists hold (exact ties with the true entity on whole percents of the table), a device-side counter
 * makes the exact kernels re-rank the block instead: a block never costs more than pre-pass + exact kernel.
 *
 *   table      (N, D) f32, row stride ld floats (ld % 4 == 0, 16-byte aligned base)
 *   q_fixed    (Q, D) f32  the entity kept fixed (tail_embs for head queries, head_embs for tail)
 *   q_rel      (Q, D) f32  rel_emb(rels)
 *   true_row   (Q) int64   row of the true entity in `table` (true_ents, train.py:150), or NULL
 *   q_true     (Q, D) f32  the true entity's vector, used when true_row == NULL (candidate-axis
 *                          sharding: the true row may live in another shard).  Exactly one of
 *                          true_row / q_true is non-NULL.
 *   filter     a blp_filter (below): the table rows the filtered setting removes for each query (the True entries of
 *                          utils.get_triple_filters' mask, utils.py:46-83) as segments of a sorted index of the filtering
 *                          graph -- or as a plain CSR (seg_lo = rowptr, seg_hi = rowptr + 1, values = col, the rest
 *                          NULL / 0); NULL = no filtering (filtered == raw).  Each row at most once per query (a mask
 *                          bit is set once however many parallel edges the graph has), never the true entity
 *                          (utils.py:71,78); blp_amd.utils.FilterIndex produces exactly that.  Rows outside [0, N) are
 *                          ignored, so a candidate shard holding global rows [lo, lo + N) takes the global filter
 *                          with row_base = lo.
 *   counts     (Q, 4) int32 OUT: {#(pred > true), #(pred >= true), same two over the
 *                          non-filtered candidates}.  Overwritten.  With the candidate axis
 *                          sharded, per-shard counts add up to the unsharded ones.
 *   workspace  caller-owned scratch of >= blp_rank_all_workspace_bytes(model, N, D, q_head, q_tail)
 *              bytes, 256-B aligned.
 * Limits: Q <= 2^30, N < 2^31 per call (int32 counts); q_fixed / q_rel / q_true 16-byte aligned.
 * -------------------------------------------------------------------------------------------- */
size_t blp_rank_all_workspace_bytes(int model, int64_t N, int D, int64_t q_head, int64_t q_tail);

/* 1 if blp_rank_all takes a block of this shape: D in {64, 128, 256} (what blp_dim_supported reports), or
 * TransE at any D % 4 == 0, D <= 1024 (the 300 / 768-wide bag-of-words and DKRL encoders, models.py:118-135,
 * 165-172).  Otherwise callers use blp_score_fwd + blp_rank_from_scores. */
int blp_rank_all_supported(int model, int D, int64_t q_head, int64_t q_tail);
/* The filter of a ranking call: SEGMENTS of a sorted index of the filtering graph, so that
 * utils.get_triple_filters (utils.py:46-83: a Python walk over a networkx graph per batch, then a dense
 * (2B, N) mask copied to the device) needs no per-batch list at all:
 *   the graph's edges are sorted once by key (head, rel) with value tail -- and by (tail, rel) with value
 *   head -- into one `values` array of ENTITY IDS (blp_amd.utils.FilterIndex); for query q the caller
 *   binary-searches the key of its triple and passes the slice [seg_lo[q], seg_hi[q]) of `values` (empty when
 *   seg_hi[q] <= seg_lo[q]; `values` is then never read);
 *   exclude[q] is the triple's own entity at the replaced position, which is never filtered (utils.py:71,78);
 *   ent2idx (utils.make_ent2idx, utils.py:31-43) maps an entity id to its table row, -1 (or an id beyond
 *   ent2idx_len) = not a candidate (utils.py:72,79); NULL = the values are table rows already;
 *   row_base is subtracted from every row and rows outside [0, N) are skipped (a candidate shard).
 * A value may occur once per segment (parallel edges collapsed when the index is built).
 * A CSR (rowptr (Q + 1), col (nnz) of table rows) is the special case seg_lo = rowptr, seg_hi = rowptr + 1, values = col,
 * exclude = ent2idx = NULL, row_base = 0.
 * filter == NULL: no filtering. */
typedef struct blp_filter {
    const int64_t *seg_lo;   /* (Q) */
    const int64_t *seg_hi;   /* (Q) */
    const int64_t *values;
    const int64_t *exclude;  /* (Q) or NULL */
    const int64_t *ent2idx;  /* (ent2idx_len) or NULL */
    int64_t ent2idx_len;
    int64_t row_base;
} blp_filter;
int blp_rank_all(int model, const float *table, int64_t N, int D, int64_t ld,
                 const float *q_fixed, const float *q_rel, const int64_t *true_row, const float *q_true,
                 int64_t q_head, int64_t q_tail, const blp_filter *filter, int32_t *counts,
                 void *workspace, size_t workspace_bytes, int device, void *stream);

/* ---- the same call for DistMult / ComplEx / SimplE AT ANY WIDTH: D % 4 == 0, 4 <= D <= 1024 (the 300 / 768-wide bag-of-words and
 * DKRL encoders, models.py:118-135, 165-172, which blp_rank_all takes for TransE only).  The exact f32 pass over the table and
 * nothing in front of it: eight lanes per candidate row restate torch's sum(dim=-1) order at run-time width from registers
 * (rank_all_wide.hip), so the counts are the reference's bit for bit; no (Q, N) array exists anywhere.  The
 * contract is blp_rank_all's, word for word: head queries first; exactly one of true_row / q_true; the blp_filter as segments or
 * a CSR, with row_base, rows outside [0, N) ignored; counts (Q, 4) int32 {gt, ge, gt_filt, ge_filt}, overwritten; per-shard
 * counts add up to the unsharded ones; asynchronous on `stream`, no allocation, no host sync; the same status codes, messages
 * (under this entry's name) and order of checks, every check before the device is touched; Q == 0 returns BLP_OK, N == 0 gives
 * zero counts.
 *   blp_rank_all_wide_supported        1 for BLP_DISTMULT / BLP_COMPLEX / BLP_SIMPLE at D % 4 == 0, 4 <= D <= 1024 -- 64 / 128 /
 *                                      256 included, where this is a second implementation of the same bits and blp_rank_all the
 *                                      faster one --; 0 for BLP_TRANSE (blp_rank_all takes it at these widths) and anything else.
 *                                      blp_rank_all_supported does not change.
 *   blp_rank_all_wide_workspace_bytes  the true keys and the packed accumulators: 4 Q + 8 Q bytes, each rounded up to 256, so
 *                                      <= 12 Q + 510 bytes (Q = q_head + q_tail), independent of N and D; 0 where the call is
 *                                      unsupported or a size is negative.
 *   blp_rank_all_wide                  BLP_ERR_UNSUPPORTED_DIM where blp_rank_all_wide_supported is 0.
 * The launch chain is bounded whatever the sizes: one true-key launch, one table pass per side with a grid of at most
 * 32 768 query chunks x 32 768 candidate slabs (workgroups stride over the chunks), one filter + finalize launch. */
int blp_rank_all_wide_supported(int model, int D);
size_t blp_rank_all_wide_workspace_bytes(int model, int64_t N, int D, int64_t q_head, int64_t q_tail);
int blp_rank_all_wide(int model, const float *table, int64_t N, int D, int64_t ld,
                      const float *q_fixed, const float *q_rel, const int64_t *true_row, const float *q_true,
                      int64_t q_head, int64_t q_tail, const blp_filter *filter, int32_t *counts,
                      void *workspace, size_t workspace_bytes, int device, void *stream);

/* The same with the queries given as INDICES instead of vectors, for ONE SHARD OF THE CANDIDATE AXIS (the north_star's
 * multi-GPU layout: the entity table partitioned by rows over the ranks, every rank ranking every query against its own
 * rows) -- or, with source == table, for the whole table: query q's fixed-entity vector is row fixed_row[q] of `source`, its
 * relation vector row rel_id[q] of rel_emb (R, D) f32 contiguous -- exactly what the reference gathers into ent_emb[tails] /
 * rel_emb(rels) (train.py:141-145), un-gathered: no (Q, D) arrays are built or streamed.  `table` is this rank's shard -- global rows
 * [row_base, row_base + N), the CANDIDATES -- while the queries' own vectors, the fixed entity and the true entity of every
 * triple, are rows of a second array `source` (S, D), row stride ld_src, that every rank holds in full: either the whole
 * table (small tables: one all-gather per evaluation) or the vectors of the entities that occur in the triples
 * (blp_gather_triple_vectors + one all-reduce).  fixed_row / true_row (Q,) index `source`; nothing else changes: the
 * reference's `ent_emb[tails]`, `ent_emb[heads]`, `rel_emb(rels)` (train.py:141-145) stay un-gathered, `true_ents`
 * (train.py:150) becomes the true entity's score from its vector, and the filter's row_base keeps the rows of other shards
 * out (blp_filter).  Per-shard counts add up exactly to the unsharded counts: one all-gather of (Q, 4) int32 + a sum is
 * the only exchange after the ranking.  The unsharded case: source == table, S == N, ld_src == ld.
 * Workspace: blp_rank_all_workspace_bytes(model, N, D, q_head, q_tail). */
int blp_rank_all_shard(int model, const float *table, int64_t N, int D, int64_t ld, const float *source, int64_t S,
                       int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R, const int64_t *rel_id,
                       const int64_t *true_row, int64_t q_head, int64_t q_tail, const blp_filter *filter, int32_t *counts,
                       void *workspace, size_t workspace_bytes, int device, void *stream);

/* EVERY BATCH OF THE REFERENCE'S EVALUATION LOOP IN ONE CALL.  train.py:128-157 hands the ranking eval_batch_size triples at
 * a time (64 in the FB15k-237 scripts, 2 for Wikidata5M: scripts/blp-*.sh:18); a query's counts do not depend on the batch
 * it came in, so a caller that keeps the loop's layout passes all of it at once: the 2 n_triples queries batch after batch
 * of `batch` triples (the last may be short), each batch as [its head-replacing queries | its tail-replacing queries] --
 * exactly what blp_build_queries writes with block = batch.  fixed_row / rel_id / true_row / the filter's seg_lo, seg_hi,
 * exclude and `counts` (2 n_triples, 4) all use that layout; source / S / ld_src as in blp_rank_all_shard (source = table
 * for an unsharded table).  Inside, the queries are ranked as ONE block per block_triples triples (0 = the default, 65 536;
 * whole batches; [all heads | all tails]: the throughput-bound kernels) and the counts scattered back: 3.1 ms instead of
 * 827 calls x 29 us for the FB15k-237 test set.  block_triples <= batch keeps one ranking pass per batch -- the reference's
 * own pass structure (one read of the table per eval_batch_size triples), issued back to back without a host round trip.
 *
 * THE CANDIDATE TABLE MAY COME IN A 16-BIT STORAGE TYPE.  The table build can emit a half-precision copy of the entity table
 * next to the f32 one (train.py:96-121 builds `ent_emb` once per evaluation); `table` (N, D) is f32 (BLP_DTYPE_F32, row
 * stride ld floats, ld % 4 == 0), IEEE half (BLP_DTYPE_F16) or bfloat16 (BLP_DTYPE_BF16; row stride ld ELEMENTS, ld % 8 ==
 * 0), 16-byte aligned.  A 16-bit element widens to f32 exactly: every kernel widens first and then runs the f32 arithmetic
 * of the reference in the reference's order, so the counts are those of the table widened to f32, bit for bit.  `source`
 * stays f32 -- the queries' own vectors, which the caller widens along with gathering them (blp_gather_triple_vectors; they
 * are a few thousand rows) -- as does everything else.  What the 16-bit copy buys: the reference's Wikidata5M batching
 * (eval_batch_size = 2: 4 queries per pass over 4.6 M rows, scripts/blp-*-wikidata5m.sh:18) is one read of the table per
 * batch, HBM-bound; with block_triples <= batch <= 4 and D = 128 or 256 the passes read the 16-bit table AS IT IS (half the
 * bytes per pass; all passes in one launch: blp_rank_all_batches_native16 says whether a call is such a one).  Any other
 * shape of call -- bound by arithmetic, not by the table read -- ranks a widened f32 copy made inside the call (the workspace
 * holds it: N x D x 4 bytes more; a caller that has the f32 table should rank that one instead; blp_amd.ranking does).
 * Workspace: blp_rank_all_batches_workspace_bytes(...), 256-B aligned. */
size_t blp_rank_all_batches_workspace_bytes(int model, int table_dtype, int64_t N, int D, int64_t ld, int64_t n_triples,
                                            int64_t batch, int64_t block_triples);
int blp_rank_all_batches(int model, const void *table, int table_dtype, int64_t N, int D, int64_t ld, const float *source,
                         int64_t S, int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R,
                         const int64_t *rel_id, const int64_t *true_row, int64_t n_triples, int64_t batch,
                         int64_t block_triples, const blp_filter *filter, int32_t *counts, void *workspace,
                         size_t workspace_bytes, int device, void *stream);
int blp_rank_all_batches_native16(int model, int table_dtype, int64_t N, int D, int64_t ld, int64_t n_triples, int64_t batch,
                                  int64_t block_triples);

/* Producer of `source` for big tables: out (2n, D) f32 contiguous, out[t] = the vector of triple t's head, out[n + t] = of
 * its tail (train.py:141-142's `ent_emb[heads]` / `ent_emb[tails]` for the whole set of triples), filled only for the
 * entities whose global row ent2idx[id] (NULL: the id itself) lies in this shard's [row_base, row_base + N) and ZERO
 * otherwise -- so that one all-reduce (sum) over the ranks replicates all 2n vectors exactly (x + 0 = x).  With
 * blp_queries.by_position the queries then index this array.  `table` in any storage type (table_dtype: BLP_DTYPE_*; a 16-bit
 * table: ld % 8 == 0); out stays f32: the vectors are widened exactly. */
int blp_gather_triple_vectors(const int64_t *triples, int64_t n, const int64_t *ent2idx, int64_t ent2idx_len,
                              const void *table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base, float *out,
                              int device, void *stream);

/* Measurement aid (bench.py): the NEXT blp_rank_all issued by the calling thread records the two
 * hipEvent_t (created by the caller with timing enabled) on its stream immediately before and after
 * the rank pass (rank_tiles, or pre-pass + refinement), so its duration can be read without a profiler.  One-shot;
 * NULL, NULL cancels.  Has no effect on results. */
int blp_profile_next_rank_kernel(void *start_event, void *stop_event);

/* Measurement aid (bench.py): the number of table passes the first ranking launch of a blp_rank_all_batches call with these
 * sizes covers -- every pass of the call when the streaming kernels take the passes of a reference-batched evaluation
 * (train.py:128-171 with eval_batch_size <= 4) in one launch, else 1 (0: nothing to rank).  What the events of
 * blp_profile_next_rank_kernel bracket divides by it. */
int64_t blp_rank_all_batches_passes_per_launch(int model, int table_dtype, int64_t N, int D, int64_t ld, int64_t n_triples,
                                               int64_t batch, int64_t block_triples);

/* Measurement aid (bench.py's `decided_frac`): what the pre-pass of the LAST blp_rank_all / blp_rank_all_shard call that ran on
 * `workspace` (same model, N, D, q_head, q_tail) left to the exact path.  out[0] = (query, candidate) pairs of the block,
 * out[1] = undecided pairs it listed one by one, out[2] = candidates inside the segments it flagged for wholesale exact
 * re-scoring (a workgroup's list was full), out[3] = the path: 0 = no pre-pass (exact kernels took the block), 1 = TransE
 * v_sad_u16, 2 = bf16 x 3 MFMA, 3 = f32-chain MFMA and 4 = any-width TransE (these two are not counted: out[1] = out[2] = -1).
 * Blocks ranked in several candidate slabs report their last slab.  Waits for `stream`, allocates 32 bytes for the call. */
int blp_rank_all_prepass_stats(int model, int64_t N, int D, int64_t q_head, int64_t q_tail, const void *workspace,
                               size_t workspace_bytes, int64_t out[4], int device, void *stream);

/* The same counts from a DENSE score matrix already in HBM: scores (Q, N) f32 with row stride ld, the
 * true entity given per query as a column index (true_idx, the reference's `true_ents`,
 * utils.py:102) or as a score (true_score); exactly one of the two.  Replaces utils.py:103-105 and the
 * filtered overwrite train.py:159-167 for callers that materialise pred_ents, and serves embedding
 * widths the fused kernels are not compiled for (the matrix then comes from blp_score_fwd).  filt_rowptr (Q + 1) / filt_col:
 * the CSR of the columns the filtered setting removes (both NULL: none); a column outside [0, N) is ignored. */
int blp_rank_from_scores(const float *scores, int64_t Q, int64_t N, int64_t ld, const int64_t *true_idx,
                         const float *true_score, const int64_t *filt_rowptr, const int64_t *filt_col,
                         int32_t *counts, int device, void *stream);

/* utils.py:104-109 on the counts of blp_rank_all: realistic rank = ((gt + 1) + ge) / 2,
 * rr = 1 / rank (f32), hits = rank <= k.   rr (Q, 2) f32 {raw, filtered};
 * hits (Q, 2, 3) uint8 for k = k_values[0..2] (train.py:72: 1, 3, 10). */
int blp_rank_metrics(const int32_t *counts, int64_t Q, const int32_t k_values[3], float *rr,
                     uint8_t *hits, int device, void *stream);

/* The accumulation of train.py:152-157 on the device: sums[0..1] = sum over queries of the reciprocal
 * rank (raw, filtered), sums[2 + 3 v + j] = number of queries with avg rank <= k_values[j] (v = 0 raw,
 * 1 filtered), all f64, summed in a fixed order (reproducible).  Divide by Q for MRR / Hits@k.
 * `sums` must have room for BLP_METRIC_SUMS_DOUBLES doubles: the 8 results come first, the rest is
 * scratch for the per-block partial sums of large Q. */
#define BLP_METRIC_SUMS_DOUBLES 520
int blp_rank_metric_sums(const int32_t *counts, int64_t Q, const int32_t k_values[3], double *sums,
                         int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * score_fn(heads, tails, rels)   models.py:222-248, any broadcast the reference uses.
 *
 * Output is an (M0, M1) f32 matrix; each operand row is addressed as
 *     base + i0 * stride0 + i1 * stride1      (strides in floats; 0 broadcasts that axis)
 * which covers the eval shapes (1,N,D)x(B,1,D) -> (B,N) of train.py:146-147, the training shapes
 * (B,K,D)x(B,1,D) -> (B,K) of models.py:67 and plain aligned rows (M0 = 1 or M1 = 1).
 * Scores are bit-identical to the reference's torch-CPU result.
 * -------------------------------------------------------------------------------------------- */
int blp_score_fwd(int model, int D, int64_t M0, int64_t M1,
                  const float *heads, int64_t h_s0, int64_t h_s1,
                  const float *tails, int64_t t_s0, int64_t t_s1,
                  const float *rels, int64_t r_s0, int64_t r_s1,
                  float *out, int device, void *stream);
/* d score / d operand for every (i0, i1): grad_* are (M0, M1, D) f32 dense (NULL = skip); the
 * caller reduces over broadcast axes.  grad_out is (M0, M1). */
int blp_score_bwd(int model, int D, int64_t M0, int64_t M1,
                  const float *heads, int64_t h_s0, int64_t h_s1,
                  const float *tails, int64_t t_s0, int64_t t_s1,
                  const float *rels, int64_t r_s0, int64_t r_s1,
                  const float *grad_out, float *grad_heads, float *grad_tails, float *grad_rels,
                  int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * In-batch negatives loss   LinkPrediction.compute_loss, models.py:51-70 (+ :251-266)
 *
 *   ent_embs  (B, 2, D) contiguous == (2B, D): row 2b = head of b, 2b+1 = tail of b
 *   rel_vecs  (B, D)    rel_emb(rels) already gathered (its backward stays in torch)
 *   neg_idx   (B, K, 2) int64, values in [0, 2B): rows of ent_embs.view(2B, D)  (data.py:35-81)
 *   regularizer: models.py:59-60, applied iff > 0
 * Storage types: ent_embs and grad_ent are ent_dtype, rel_vecs and grad_rel are rel_dtype (= ent_dtype, or f32: nn.Embedding
 *      rows stay f32 under autocast -- BASELINE config 5: half-precision embeddings).  Half operands are widened exactly and
 *      every operation is the f32 one of the reference (f32 accumulate); the loss and the saved scores stay f32; gradients
 *      are rounded once on store.  The reference has no half path: parity there is a tolerance against the f32 oracle on the
 *      widened inputs (tests/test_gpu_parity.py::test_inbatch_loss_half_*).
 * fwd: loss (1) f32; save_pos (blp_inbatch_loss_save_floats(model, B, K, D) floats) -- the B positive scores, the
 *      workgroups' partial loss sums, and an INDEX of neg_idx (per chunk of consecutive entries: the entries grouped by
 *      the row they name, in entry order) -- and save_neg (B, K) f32 scores are kept for bwd.  Scores: the bilinear models
 *      32 lanes per pair = torch.sum's 32 running sums, folded by wavefront shuffles; TransE four lanes per pair, the
 *      running L1 sum walking through them -- bit-identical to the reference at the scripts' widths.  Loss: every
 *      workgroup adds its slots' terms in f64 (slot order); the partial sums are then added in workgroup order -- by the
 *      workgroup that takes the last ticket when there are at most 96 of them (ONE launch: the TransE step at the scripts'
 *      batch sizes), else by a second, one-workgroup launch (cheaper than that many tickets).  A fixed order either way.
 *      ticket: BLP_INBATCH_TICKET_INTS int32 the caller keeps PER STREAM, ZERO on entry; the kernel leaves them zero when it
 *      completes (calls on one stream are ordered and may share them; concurrent streams need their own).
 * bwd: ONE launch.  grad_ent (2B, D), grad_rel (B, D), both overwritten, scaled by *grad_loss (device scalar).  O(B K) work:
 *      a row's negatives come from the forward's index, in entry order.  Deterministic (no float atomics).  margin_loss
 *      passes gradient where the hinge is exactly 0 (models.py:252-253 masks in place).
 * Floating point: the scores are the reference's elementwise terms summed in tree order, so the loss agrees with the
 * reference to ~1e-6 relative and the gradients to ~1e-5 (the bit-exact score_fn is blp_score_fwd).
 * -------------------------------------------------------------------------------------------- */
#define BLP_INBATCH_TICKET_INTS 4
size_t blp_inbatch_loss_save_floats(int model, int B, int K, int D);
/* kernel launches of blp_inbatch_loss_fwd at these sizes: 1 (at most 96 scoring workgroups: the last one finishes the loss) or 2 */
int blp_inbatch_loss_fwd_launches(int model, int B, int K, int D, float regularizer);
int blp_inbatch_loss_fwd(int model, int loss, int ent_dtype, int rel_dtype, const void *ent_embs,
                           const void *rel_vecs, const int64_t *neg_idx, int B, int K, int D,
                           float regularizer, float *out_loss, float *save_pos, float *save_neg,
                           int32_t *ticket, int device, void *stream);
int blp_inbatch_loss_bwd(int model, int loss, int ent_dtype, int rel_dtype, const void *ent_embs,
                           const void *rel_vecs, const int64_t *neg_idx, int B, int K, int D,
                           float regularizer, const float *grad_loss, const float *save_pos,
                           const float *save_neg, void *grad_ent, void *grad_rel, int device,
                           void *stream);

/* --------------------------------------------------------------------------------------------
 * The evaluation loop's per-batch prelude for a whole set of n triples, in one kernel (the producer of blp_rank_all's
 * query arguments and of blp_rank_all_ex's filter segments):
 *
 *   heads = [ent2idx[ent] for ent in triples[:, 0]], tails likewise, assert min >= 0        train.py:134-138
 *   head_embs = ent_emb[heads], tail_embs = ent_emb[tails], rel_embs = rel_emb(rels)       train.py:141-145
 *   utils.get_triple_filters(triples, graph, ...)                                           utils.py:46-83
 *
 * Query order: blocks of `block` triples, each block as [its head-replacing queries | its tail-replacing queries]
 * (train.py:149), so that block b is rows [2 b block, ...) of every output and can be handed to blp_rank_all(_ex) as is.
 *   triples      (n, 3) int64 rows (head id, tail id, relation id) -- data.py:128 column order
 *   ent2idx      id -> row of `source`, -1 = not a candidate (utils.make_ent2idx); NULL: ids are rows
 *   source       (src_rows, D) f32, row stride ld: the entity table;  rel_emb (R, D) f32 contiguous
 *   heads_key / tails_key  sorted keys entity * index_R + relation of the filtering graph's (tail, rel) -> heads and
 *                (head, rel) -> tails indices (blp_amd.utils.FilterIndex); both NULL: no filter outputs
 * Outputs (2n rows each): q_fixed, q_rel (2n, D) f32 (both NULL: no vectors are gathered -- blp_rank_all_idx takes
 * fixed_row / rel_ids instead); fixed_row, true_row, rel_ids int64 (fixed_row may be NULL); seg_lo / seg_hi: the
 * query's slice of the caller's value array [heads' values | tails' values] (tail-side slices are offset by n_heads);
 * exclude: the triple's own entity id; *ids_min: 0, or -1 if any id has no row / any relation is outside [0, R) (such
 * queries get zero vectors and rows / relation 0: the caller must check before trusting the counts, as
 * train.py:137-138 asserts).
 * D % 4 == 0; 16-byte aligned source / rel_emb / q_fixed / q_rel; ld % 4 == 0.
 * -------------------------------------------------------------------------------------------- */
typedef struct blp_queries {
    const int64_t *triples; int64_t n, block;
    const int64_t *ent2idx; int64_t ent2idx_len;
    const float *source; int64_t src_rows, ld; int D;
    const float *rel_emb; int64_t R;
    const int64_t *heads_key; int64_t n_heads;
    const int64_t *tails_key; int64_t n_tails;
    int64_t index_R;
    float *q_fixed; float *q_rel; int64_t *true_row; int64_t *rel_ids; int32_t *ids_min;
    int64_t *seg_lo; int64_t *seg_hi; int64_t *exclude;
    int64_t *fixed_row;
    int64_t by_position;     /* 0: fixed_row / true_row are rows of `source` (= ent2idx[id]).  1: `source` is the (2n, D) array
                              * of blp_gather_triple_vectors and fixed_row / true_row are POSITIONS in it (head of triple t = t,
                              * tail = n + t); ent2idx and src_rows (= rows of the whole table) then only serve the id check. */
} blp_queries;
int blp_build_queries(const blp_queries *q, int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * Entity-table build, last step (the producer of blp_rank_all's `table`), for the BERT encoders:
 *
 *   embs = self.enc_linear(embs)              models.py:110-111 (nn.Linear(hidden, dim, bias=False), :104)
 *   ent_emb = F.normalize(ent_emb, dim=-1)    models.py:40-41   (iff normalize != 0: TransE)
 *   ent_emb[idx:idx + batch] = batch_emb      train.py:109-113
 *
 *   out[i, :] = x[i, :] . w^T  [ / max(||.||_2, 1e-12) ]      i < n
 *
 *   x    (n, E) f32, row stride ldx floats (the [CLS] rows of the encoder output are strided: pass the view);
 *   w    (D, E) f32 row-major (enc_linear.weight);  out  (n, D) f32, row stride ldo: rows of the table shard.
 * f32 operands and accumulation on the matrix cores (v_mfma_f32_32x32x2_f32); a floating-point GEMM: results agree
 * with the torch expression to ~1e-6 relative, not bit for bit (the K-reduction order is the kernel's own).
 * blp_project_rows_supported: E % 4 == 0 and D in {64, 128, 256}; x, w, out 16-byte aligned, ldx % 4 == 0.
 * -------------------------------------------------------------------------------------------- */
int blp_project_rows_supported(int E, int D);
int blp_project_rows(const float *x, int64_t n, int64_t ldx, const float *w, int E, int D, int normalize,
                     float *out, int64_t ldo, int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * Entity-table build for the bag-of-words encoder (models.py:143-155; the glove-bow / bert-bow scripts), with the steps
 * that follow it:
 *
 *   embs = self.embeddings(text_tok); lengths = torch.sum(text_mask, dim=-1, keepdim=True)      models.py:150-151
 *   embs = torch.sum(text_mask.unsqueeze(dim=-1) * embs, dim=1) / lengths                       models.py:152-153
 *   ent_emb = F.normalize(ent_emb, dim=-1)    models.py:40-41 (iff normalize != 0)
 *   ent_emb[idx:idx + batch] = batch_emb      train.py:109-113
 *
 *   out[i, :] = (sum_l mask[i, l] * emb[tok[i, l], :]) / (sum_l mask[i, l])  [ / max(||.||_2, 1e-12) ]      i < n
 *
 *   tok   (n, L) int64 token ids, row-major;  mask (n, L) f32 or NULL (all ones: models.py:147-148);
 *   emb   (V, E) f32 row-major (embeddings.weight);  out (n, E) f32, row stride ldo: rows of the table shard;
 *   bad_tok  int32 on the device, set to -1 if a token id was outside [0, V) (row 0 is read for it; nn.Embedding would
 *            raise) and left alone otherwise: the caller initialises it to 0 and reads it when convenient.
 * No (n, L, E) temporary: every gathered row is read once.  Floating point (tokens summed in order, product and sum rounded
 * separately): agrees with the torch expression to ~1e-6 relative, not bit for bit.
 * blp_bow_rows_supported: E % 4 == 0, E <= 1024; emb, out 16-byte aligned, ldo % 4 == 0, ldo >= E.
 * -------------------------------------------------------------------------------------------- */
int blp_bow_rows_supported(int E);
int blp_bow_rows(const int64_t *tok, const float *mask, int64_t n, int L, const float *emb, int64_t V, int E,
                 int normalize, float *out, int64_t ldo, int32_t *bad_tok, int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * Entity-table build for the DKRL encoder (models.py:158-204; the bert-dkrl / glove-dkrl scripts), with the steps that
 * follow it:
 *
 *   embs = self.embeddings(text_tok) * text_mask.unsqueeze(-1)                                    models.py:177
 *   embs = self.conv1(F.pad(embs.transpose(1, 2), [0, 1])) * text_mask          Conv1d(E, dim, 2)  models.py:180-187
 *   embs = F.max_pool1d(embs, 4); text_mask = F.max_pool1d(text_mask, 4)        (L >= 4)           models.py:188-195
 *   embs = self.conv2(F.pad(torch.tanh(embs), [0, 1]))                          Conv1d(dim, dim, 2) models.py:196-198
 *   embs = torch.tanh(torch.sum(embs * text_mask, dim=-1) / lengths)                               models.py:199-202
 *   ent_emb = F.normalize(ent_emb, dim=-1)    models.py:40-41 (iff normalize != 0)
 *   ent_emb[idx:idx + batch] = batch_emb      train.py:109-113
 *
 *   tok (n, L) int64, mask (n, L) f32 or NULL (all ones), emb (V, E) f32 as for blp_bow_rows;
 *   w1 (dim, E, 2), b1 (dim): conv1.weight / .bias;  w2 (dim, dim, 2), b2 (dim): conv2.weight / .bias, contiguous f32;
 *   out (n, dim) f32, row stride ldo: rows of the table shard;  bad_tok as for blp_bow_rows.
 * One kernel, nothing materialised: conv1 on the matrix cores with f32 operands (v_mfma_f32_32x32x2_f32), bias / mask /
 * max-pool / tanh in the accumulator registers, conv2 + masked mean folded into two 128-vectors per entity (they are linear
 * in the pooled activations).  A masked position contributes exact zeros (the stock expression multiplies the gathered
 * row by 0: the same unless the embedding row holds Inf / NaN).  Floating point: agrees with the stock modules to ~1e-6,
 * not bit for bit (the reduction orders differ from the convolution library's).
 * blp_dkrl_rows_supported: E % 4 == 0, dim == 128 (every DKRL script's), 4 <= L <= 64 (max_len 32 / 64; shorter chunks
 * change the pooling window, models.py:188-193, and stay with the stock modules); emb, w1, w2 16-byte aligned, ldo >= dim.
 * -------------------------------------------------------------------------------------------- */
int blp_dkrl_rows_supported(int E, int D, int L);
int blp_dkrl_rows(const int64_t *tok, const float *mask, int64_t n, int L, const float *emb, int64_t V, int E,
                  const float *w1, const float *b1, const float *w2, const float *b2, int D, int normalize, float *out,
                  int64_t ldo, int32_t *bad_tok, int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * Filtered top-k entity prediction: ANSWER a query (h, r, ?) / (?, r, t) with the k table rows the model scores highest,
 * the known edges left out -- what a trained link predictor is used for (inductive BLP: the table holds the encoded new
 * entities).  The (Q, N) score matrix of score_fn(ent_emb, ...) (models.py:222-248; train.py:146-147) is never built.
 *
 * Queries as in blp_rank_all_shard: Q = q_head + q_tail, head-replacing first; query q's fixed-entity vector is row
 * fixed_row[q] of source (S, D) (row stride ld_src), its relation vector row rel_id[q] of rel_emb (R, D) contiguous.  A caller
 * with loose query vectors (an entity that is not in the table) passes them as `source` with fixed_row = 0, 1, ...
 * Candidates: the rows of table (N, D) f32, row stride ld -- GLOBAL rows [row_base, row_base + N) (a candidate shard).
 * Output per query, k slots: rows (Q, k) int64 global rows, scores (Q, k) f32:
 *   scores are score_fn's values bit for bit (the torch-CPU order of oracle/blp_oracle.c, sign of zero included);
 *   order: descending score by IEEE comparison, equal scores (-0 == +0) by ascending row, NaN after every number (by row)
 *          -- i.e. numpy's argsort(-score_row, kind="stable")[:k];
 *   filter (optional): a blp_filter with blp_rank_all's semantics (segments of entity ids through ent2idx and row_base;
 *          exclude[q] is never filtered) whose row_base MUST equal this call's (else BLP_ERR_BAD_ARG); filtered rows are
 *          REMOVED, not demoted;
 *   slots left over (k > N, or the filter leaves fewer than k rows): row -1, score NaN.
 * Limits: 1 <= k <= 256 and D in {64, 128, 256} (blp_topk_supported); row_base + N <= 2^31; Q x k < 2^31; table / source /
 * rel_emb 16-byte aligned, ld % 4 == 0, ld_src % 4 == 0.
 * Workspace: blp_topk_workspace_bytes(...) bytes, 256-B aligned.  It does not grow with N beyond N = 2^17 rows and is bounded
 * by 8 (D + k) Q + 4 MiB bytes (the queries' coefficient rows and at most Q + 16 384 partial lists of k 8-byte keys).
 * Deterministic: the result does not depend on the grid, the device or the order of the candidates' evaluation.
 * -------------------------------------------------------------------------------------------- */
int blp_topk_supported(int model, int D, int k);
size_t blp_topk_workspace_bytes(int model, int64_t N, int D, int64_t q_head, int64_t q_tail, int k);
int blp_topk(int model, const float *table, int64_t N, int D, int64_t ld, int64_t row_base, const float *source, int64_t S,
             int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R, const int64_t *rel_id, int64_t q_head,
             int64_t q_tail, int k, const blp_filter *filter, int64_t *rows, float *scores, void *workspace,
             size_t workspace_bytes, int device, void *stream);
/* Merge `lists` per-query lists -- e.g. the blp_topk results of several candidate shards, gathered side by side: rows / scores
 * (Q, lists x k_in), each list of k_in slots in blp_topk's order -- into the k best per query (rows_out, scores_out (Q, k)),
 * by the same order; a row < 0 is an empty slot and sorts last.  Rows must be below 2^31.  The non-empty rows of one query
 * are distinct (the order breaks ties by row; what a row given twice gives is not specified).  Scores are copied (a NaN
 * comes out as the quiet NaN 0x7fc00000).  The second stage of blp_topk, on caller-given lists; no workspace. */
int blp_topk_merge(const int64_t *rows, const float *scores, int64_t Q, int lists, int k_in, int k, int64_t *rows_out,
                   float *scores_out, int device, void *stream);
/* blp_topk over a candidate table in any storage type (table_dtype: BLP_DTYPE_*; see "THE CANDIDATE TABLE MAY COME IN A 16-BIT
 * STORAGE TYPE" above): the same contract on the table WIDENED to f32 exactly -- the same rows in the same order, the
 * reference's f32 scores of the widened rows bit for bit (sign of zero included), filtered rows removed, -1 / NaN slots, the
 * same workspace (it does not depend on the storage type), independent of the grid.  A 16-bit table's row stride ld is in
 * ELEMENTS, ld % 8 == 0, 16-byte aligned base; source and rel_emb stay f32 (the queries' vectors: gather and widen the
 * fixed entities' rows, blp_gather_triple_vectors).  BLP_DTYPE_F32 is blp_topk itself.  An unknown table_dtype is
 * BLP_ERR_BAD_ARG (the _supported / _workspace_bytes calls answer 0).  The 16-bit rows are read as they are: half the bytes of
 * the f32 table per pass. */
int blp_topk_typed_supported(int model, int table_dtype, int D, int k);
size_t blp_topk_typed_workspace_bytes(int model, int table_dtype, int64_t N, int D, int64_t q_head, int64_t q_tail, int k);
int blp_topk_typed(int model, const void *table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                   const float *source, int64_t S, int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R,
                   const int64_t *rel_id, int64_t q_head, int64_t q_tail, int k, const blp_filter *filter, int64_t *rows,
                   float *scores, void *workspace, size_t workspace_bytes, int device, void *stream);
/* blp_topk for DistMult / ComplEx / SimplE at ANY width D % 4 == 0, 4 <= D <= 1024 (the bag-of-words / DKRL encoders' 300 and
 * 768), 1 <= k <= 256, an f32 table (blp_topk_wide_supported; 0 for TransE -- blp_topk_sets_wide with one set serves it -- and
 * for anything else).  The contract is blp_topk's word for word: the same arguments in the same order, the queries as rows of
 * source / rel_emb, global rows [row_base, row_base + N), the same order of the k slots, filtered rows removed, -1 / NaN
 * slots, score_fn's values bit for bit (sign of zero included), the same limits, alignment rules, checks and status codes
 * (BLP_ERR_UNSUPPORTED_DIM where blp_topk_wide_supported says 0), deterministic whatever the grid, asynchronous on `stream`,
 * no allocation, no host synchronisation.  At D in {64, 128, 256} it is a second implementation of blp_topk's bits.
 * One code object for every width: eight lanes per candidate row sum in the reference's order from registers, the queries'
 * coefficients live in LDS, and the winners' scores come straight from the selection keys (at most three launches).
 * Workspace: blp_topk_wide_workspace_bytes(...) bytes, 256-B aligned: only the partial lists, exactly
 *   round_up_256(8 k Q S),  S = max(1, min(2048 / (ceil(q_head / 8) + ceil(q_tail / 8)), ceil(N / 64)))  (integer division)
 * -- independent of D, constant in N from N = 2^17 rows on, at most 8 k (Q + 16 384) + 256 bytes; 0 where unsupported, for a
 * negative size and where Q x k >= 2^31.
 * (Added after 6.0.0 without a version change: no existing entry point changed.) */
int blp_topk_wide_supported(int model, int D, int k);
size_t blp_topk_wide_workspace_bytes(int model, int64_t N, int D, int64_t q_head, int64_t q_tail, int k);
int blp_topk_wide(int model, const float *table, int64_t N, int D, int64_t ld, int64_t row_base, const float *source, int64_t S,
                  int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R, const int64_t *rel_id, int64_t q_head,
                  int64_t q_tail, int k, const blp_filter *filter, int64_t *rows, float *scores, void *workspace,
                  size_t workspace_bytes, int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * Per-query candidate lists: RANK and SCORE a query (h, r, ?) / (?, r, t) against a list of table rows that belongs to that
 * query -- the sampled negatives of an evaluation on a table of millions of rows, the candidates a first stage (BM25, a type
 * index) hands over for re-ranking, or any sparse set of (query, entity) pairs.  Only the listed rows are read.
 *
 * Queries as in blp_rank_all_shard: Q = q_head + q_tail, head-replacing first; fixed_row / true_row index source (S, D) f32
 * (row stride ld_src), rel_id indexes rel_emb (R, D) contiguous.  Candidates: the rows of table (N, D) in table_dtype
 * (BLP_DTYPE_*, widened exactly), row stride ld -- GLOBAL rows [row_base, row_base + N).
 * Lists: a CSR over the queries -- query q owns entries [list_ptr[q], list_ptr[q + 1]) of list_row (nnz) int64 GLOBAL rows;
 * list_ptr (Q + 1) int64 is trusted to be non-decreasing with list_ptr[0] = 0 and list_ptr[Q] = nnz.  A list is a multiset:
 * every entry counts, duplicates included.  There is no limit on a list's length; an empty list gives zero counts.
 * An entry outside [row_base, row_base + N) -- the -1 of a padded rectangular (Q, C) list, a row of another candidate shard --
 * is SKIPPED: it counts nowhere and its score slot is the quiet NaN 0x7fc00000, so per-shard counts add up to the
 * unsharded ones.
 * Outputs (either may be NULL, not both):
 *   counts (Q, 4) int32 {gt, ge, gt_filt, ge_filt}: the entries of the list that score above / at least the true entity
 *          (row true_row[q] of source; its key as blp_rank_all_shard computes it; IEEE comparisons, so a NaN counts nowhere,
 *          as in blp_rank_from_scores); the _filt columns count only entries whose row the filter does not remove (without a
 *          filter they repeat the first two).  The true row, if listed, is an entry like any other (it adds to ge).
 *          counts needs true_row and the workspace; true_row == NULL goes with counts == NULL (scores only).
 *   scores (nnz) f32, aligned with list_row: score_fn's value of every entry bit for bit (the torch-CPU order of
 *          oracle/blp_oracle.c, sign of zero included).
 *   filter (optional): a blp_filter with blp_rank_all's semantics (segments of entity ids through ent2idx and row_base;
 *          exclude[q] is never removed) whose row_base MUST equal this call's (else BLP_ERR_BAD_ARG).
 * Limits (blp_rank_lists_supported): TransE at any D % 4 == 0, D <= 1024; DistMult / ComplEx / SimplE at D in {64, 128, 256};
 * nnz < 2^31; row_base + N <= 2^31; Q <= 2^30; table rows / source / rel_emb / counts 16-byte aligned (ld % 4 == 0, a
 * 16-bit table: ld % 8 == 0, in elements; ld_src % 4 == 0).
 * Workspace: blp_rank_lists_workspace_bytes(...) bytes, 256-B aligned, needed with counts only: 4 Q bytes rounded up to 256
 * (the true keys) -- independent of N and nnz.
 * Asynchronous on `stream`, no allocation; deterministic: long lists are split over workgroups whose partial counts are
 * combined by integer adds, so nothing depends on the grid.
 * (Added after 6.0.0 without a version change: no existing entry point changed.)
 * -------------------------------------------------------------------------------------------- */
int blp_rank_lists_supported(int model, int table_dtype, int D);
size_t blp_rank_lists_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail);
int blp_rank_lists(int model, const void *table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                   const float *source, int64_t S, int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R,
                   const int64_t *rel_id, const int64_t *true_row, int64_t q_head, int64_t q_tail, const int64_t *list_ptr,
                   const int64_t *list_row, int64_t nnz, const blp_filter *filter, int32_t *counts, float *scores,
                   void *workspace, size_t workspace_bytes, int device, void *stream);

/* Per-query candidate lists for DistMult / ComplEx / SimplE at ANY width (the BOW / DKRL encoders' 300 and 768).  The
 * contract is blp_rank_lists' word for word -- queries, table (f32 / f16 / bf16, widened exactly), row_base shards, the lists
 * CSR, skipped entries (score slot 0x7fc00000), counts and / or scores (score_fn's value bit for bit, sign of zero included),
 * the filter, the argument checks with their status codes, deterministic whatever the grid, asynchronous on `stream`, no
 * allocation -- and so is the argument list.
 * Limits (blp_rank_lists_wide_supported): model DistMult / ComplEx / SimplE (TransE: BLP_ERR_UNSUPPORTED_DIM -- blp_rank_lists
 * takes it at these widths); table_dtype BLP_DTYPE_F32 / F16 / BF16; D % 4 == 0, 4 <= D <= 1024; everything else 0.  The
 * other limits (nnz, rows, Q, alignment) are blp_rank_lists'.
 * At D in {64, 128, 256} it is a second implementation of blp_rank_lists' bits; blp_rank_lists is the call
 * ranking.rank_candidates routes there.
 * One code object per (model, table dtype) for every width: eight lanes per (entry, query) pair sum in the reference's order,
 * the query's coefficients staged once per (wave, query) in LDS.
 * Workspace: blp_rank_lists_wide_workspace_bytes(...) bytes, 256-B aligned, needed with counts only: 4 Q bytes rounded up to
 * 256 (the true keys) -- independent of N, D and nnz; 0 where unsupported and for a negative size.
 * (Added after 6.0.0 without a version change: no existing entry point changed.) */
int blp_rank_lists_wide_supported(int model, int table_dtype, int D);
size_t blp_rank_lists_wide_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail);
int blp_rank_lists_wide(int model, const void *table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                        const float *source, int64_t S, int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R,
                        const int64_t *rel_id, const int64_t *true_row, int64_t q_head, int64_t q_tail, const int64_t *list_ptr,
                        const int64_t *list_row, int64_t nnz, const blp_filter *filter, int32_t *counts, float *scores,
                        void *workspace, size_t workspace_bytes, int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * Candidate sets SHARED between queries: rank a query against the rows of a set that a whole group of queries ranks against --
 * type-constrained evaluation (a head query of relation r against the entities seen as heads of r, a tail query against
 * those seen as its tails), per-relation / per-type / per-language pools, one first-stage pool for a group of queries.
 * A row of a set is fetched once per (set, chunk of 128 queries of its group), not once per query as a per-query list of
 * blp_rank_lists would be.
 *
 * Table: (N, D) f32, row stride ld -- GLOBAL rows [row_base, row_base + N).  Queries as in blp_rank_all_shard: Q = q_head +
 * q_tail, head-replacing first; fixed_row / true_row index source (S, D) f32 (row stride ld_src), rel_id indexes rel_emb
 * (R, D) contiguous.
 * Sets: a CSR over G sets -- set g owns entries [set_ptr[g], set_ptr[g + 1]) of set_row (nnz) int64 GLOBAL rows, STRICTLY
 * ASCENDING within a set (a set is a set; the filter's membership test is a binary search); set_ptr (G + 1) int64 is trusted
 * to be non-decreasing with set_ptr[0] = 0 and set_ptr[G] = nnz.  An entry outside [row_base, row_base + N) is SKIPPED, so
 * per-shard counts add up to the unsharded ones.
 * Which set a query ranks against: within each side the queries are ordered by non-decreasing set.  Set g serves the
 * head-replacing queries [qset_ptr_head[g], qset_ptr_head[g + 1]) and the tail-replacing queries q_head + [qset_ptr_tail[g],
 * qset_ptr_tail[g + 1]) -- both (G + 1) int64, non-decreasing, qset_ptr_head from 0 to q_head, qset_ptr_tail (counted from
 * q_head) from 0 to q_tail.  A set may serve both sides, one side or no query; a query of an empty set gets zero counts.
 * counts (Q, 4) int32 {gt, ge, gt_filt, ge_filt}, overwritten, in the caller's (grouped) query order: blp_rank_all's counts
 *   taken over the entries of the query's set only -- the true entity's key as blp_rank_all_shard computes it, every entry
 *   by the exact f32 kernel's arithmetic (the reference's counts bit for bit).  The true entity adds to ge if and only if
 *   its row is in the set.
 * filter (optional): a blp_filter with blp_rank_all's semantics whose row_base MUST equal this call's (else
 *   BLP_ERR_BAD_ARG).  An entry removes its row from the _filt columns only if that row is in the query's set.
 * Limits (blp_rank_sets_supported): the four models at D in {64, 128, 256}; Q <= 2^30; nnz < 2^31; row_base + N <= 2^31;
 * table / source / rel_emb / counts 16-byte aligned, ld % 4 == 0, ld_src % 4 == 0.
 * Workspace: blp_rank_sets_workspace_bytes(model, D, q_head, q_tail, G) bytes, 256-B aligned: true keys, accumulators,
 * coefficient rows (2 D floats per query) and G + 1 int64 of work-unit offsets -- independent of N and nnz.
 * Asynchronous on `stream`, no host synchronisation, no allocation; nothing about set or group sizes is read on the host.
 * Deterministic: partial counts are combined by integer adds, so nothing depends on the grid.
 * (Added after 6.0.0 without a version change: no existing entry point changed.)
 * -------------------------------------------------------------------------------------------- */
int blp_rank_sets_supported(int model, int D);
size_t blp_rank_sets_workspace_bytes(int model, int D, int64_t q_head, int64_t q_tail, int64_t G);
int blp_rank_sets(int model, const float *table, int64_t N, int D, int64_t ld, int64_t row_base, const float *source, int64_t S,
                  int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R, const int64_t *rel_id,
                  const int64_t *true_row, int64_t q_head, int64_t q_tail, const int64_t *set_ptr, const int64_t *set_row,
                  int64_t nnz, int64_t G, const int64_t *qset_ptr_head, const int64_t *qset_ptr_tail, const blp_filter *filter,
                  int32_t *counts, void *workspace, size_t workspace_bytes, int device, void *stream);
/* blp_rank_sets over a candidate table in any storage type (table_dtype: BLP_DTYPE_*; see "THE CANDIDATE TABLE MAY COME IN A
 * 16-BIT STORAGE TYPE" above): the same contract on the table WIDENED to f32 exactly -- the (Q, 4) counts are blp_rank_sets'
 * on the widened table bit for bit, with the same set, shard (row_base), filter and true-entity semantics, the same limits and
 * the same workspace (it does not depend on the storage type), independent of the grid.  A 16-bit table's row stride ld is in
 * ELEMENTS, ld % 8 == 0, 16-byte aligned base; source and rel_emb stay f32 (the queries' vectors: gather and widen the Q
 * fixed and the Q true rows, blp_gather_triple_vectors).  BLP_DTYPE_F32 is blp_rank_sets itself.  An unknown table_dtype is
 * BLP_ERR_BAD_ARG (the _supported / _workspace_bytes calls answer 0).  The 16-bit rows are gathered as they are: half the
 * cache lines of the f32 table per set entry.
 * (Added after 6.0.0 without a version change: no existing entry point changed.) */
int blp_rank_sets_typed_supported(int model, int table_dtype, int D);
size_t blp_rank_sets_typed_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail, int64_t G);
int blp_rank_sets_typed(int model, const void *table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                        const float *source, int64_t S, int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R,
                        const int64_t *rel_id, const int64_t *true_row, int64_t q_head, int64_t q_tail, const int64_t *set_ptr,
                        const int64_t *set_row, int64_t nnz, int64_t G, const int64_t *qset_ptr_head,
                        const int64_t *qset_ptr_tail, const blp_filter *filter, int32_t *counts, void *workspace,
                        size_t workspace_bytes, int device, void *stream);
/* Candidate sets shared between queries for TransE at ANY width: blp_rank_sets_wide is blp_rank_sets_typed -- the contract
 * above word for word: the sets CSR of strictly ascending global rows, row_base shards with entries outside [row_base,
 * row_base + N) skipped, the grouping by qset_ptr_head / qset_ptr_tail, the filter (an entry is subtracted only if its row is
 * in the query's set; the triple's own entity is never removed), the true entity (adds to ge iff its row is in the set), the
 * (Q, 4) int32 counts in grouped order, the reference's bit for bit (a 16-bit table: of the table widened to f32) -- at the
 * widths blp_rank_sets_supported refuses: the BOW / DKRL encoders' 300 and 768.  A lane holds 64 columns of its set row at a
 * time and the running sums of a chunk of 16 queries of the set's group (rank_sets_wide.hip): a row of a set is fetched once
 * per (set, chunk of 16 queries of its group).
 * Limits (blp_rank_sets_wide_supported): BLP_MODEL_TRANSE only, table_dtype a BLP_DTYPE_*, D % 4 == 0 and 4 <= D <= 1024 --
 * 64 / 128 / 256 included, where it is a second implementation of the same bits (blp_rank_sets is the faster one); the other
 * models, other widths and unknown dtypes answer 0.  Q <= 2^30; nnz < 2^31; row_base + N <= 2^31; table / source / rel_emb /
 * counts 16-byte aligned, ld % 4 == 0 (f32) or ld % 8 == 0 (a 16-bit table, in elements), ld_src % 4 == 0.  Status codes and
 * messages as blp_rank_sets_typed.
 * Workspace: blp_rank_sets_wide_workspace_bytes(model, table_dtype, D, q_head, q_tail, G) bytes (0 where unsupported or a
 * size is negative), 256-B aligned: true keys (4 Q bytes), accumulators (8 Q), per-query coefficient rows (2 D floats per
 * head-replacing query, D per tail-replacing one) and G + 1 int64 of work-unit offsets -- independent of N and nnz.
 * Asynchronous on `stream`, no host synchronisation, no allocation; nothing about set or group sizes is read on the host.
 * Deterministic: partial counts are combined by integer adds, so nothing depends on the grid.
 * (Added after 6.0.0 without a version change: no existing entry point changed.) */
int blp_rank_sets_wide_supported(int model, int table_dtype, int D);
size_t blp_rank_sets_wide_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail, int64_t G);
int blp_rank_sets_wide(int model, const void *table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                       const float *source, int64_t S, int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R,
                       const int64_t *rel_id, const int64_t *true_row, int64_t q_head, int64_t q_tail, const int64_t *set_ptr,
                       const int64_t *set_row, int64_t nnz, int64_t G, const int64_t *qset_ptr_head,
                       const int64_t *qset_ptr_tail, const blp_filter *filter, int32_t *counts, void *workspace,
                       size_t workspace_bytes, int device, void *stream);
/* Candidate sets shared between queries for DistMult / ComplEx / SimplE at ANY width: blp_rank_sets_wide_bilinear is
 * blp_rank_sets_wide -- the same argument list in the same order and the contract above word for word (the sets CSR, row_base
 * shards, the grouping, the filter and true-entity rules, the (Q, 4) int32 counts, the reference's bit for bit) -- for the three
 * bilinear models at the widths blp_rank_sets_supported refuses.  The sum order is blp_rank_all_wide's (eight lanes per set
 * row, the coefficients of a chunk of 8 queries of the set's group in LDS: rank_sets_wide_bilinear.hip): a row of a set is
 * fetched once per (set, chunk of 8 queries of one side of its group).
 * Limits (blp_rank_sets_wide_bilinear_supported): BLP_MODEL_DISTMULT / COMPLEX / SIMPLE, table_dtype BLP_DTYPE_F32 only (the
 * argument is there for 16-bit tables to follow), D % 4 == 0 and 4 <= D <= 1024 -- 64 / 128 / 256 included, where it is a
 * second implementation of the same bits (blp_rank_sets is the faster one); everything else answers 0.  The other limits, the
 * alignment rules, the status codes and the messages are blp_rank_sets_wide's (one argument-checking path).
 * Workspace: blp_rank_sets_wide_bilinear_workspace_bytes(model, table_dtype, D, q_head, q_tail, G) bytes (0 where unsupported
 * or a size is negative), 256-B aligned: true keys (4 Q bytes), accumulators (8 Q) and two unit prefixes of G + 1 int64, one
 * per side -- independent of N, nnz and D.
 * Asynchronous on `stream`, no host synchronisation, no allocation.  Deterministic: integer adds only, nothing depends on the
 * grid.  (Added after 6.0.0 without a version change: no existing entry point changed.) */
int blp_rank_sets_wide_bilinear_supported(int model, int table_dtype, int D);
size_t blp_rank_sets_wide_bilinear_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail, int64_t G);
int blp_rank_sets_wide_bilinear(int model, const void *table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                                const float *source, int64_t S, int64_t ld_src, const int64_t *fixed_row, const float *rel_emb,
                                int64_t R, const int64_t *rel_id, const int64_t *true_row, int64_t q_head, int64_t q_tail,
                                const int64_t *set_ptr, const int64_t *set_row, int64_t nnz, int64_t G,
                                const int64_t *qset_ptr_head, const int64_t *qset_ptr_tail, const blp_filter *filter,
                                int32_t *counts, void *workspace, size_t workspace_bytes, int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * Filtered top-k INSIDE candidate sets shared between queries: ANSWER a query (h, r, ?) / (?, r, t) with the k rows of ITS SET
 * the model scores highest -- "the 10 best tails of (h, r, ?) among the entities that can be a tail of r", a first-stage
 * pool re-ranked for a group of queries, per-language pools.  The contract is the union of blp_rank_sets' (queries, sets,
 * grouping) and blp_topk's (output).  A row of a set is fetched once per (set, chunk of <= 32 queries of its group); no
 * score is written out and nothing is sorted.
 *
 * Table: (N, D) f32, row stride ld -- GLOBAL rows [row_base, row_base + N).  Queries as in blp_rank_all_shard: Q = q_head +
 * q_tail, head-replacing first; fixed_row indexes source (S, D) f32 (row stride ld_src), rel_id indexes rel_emb (R, D)
 * contiguous.
 * Sets and grouping exactly as in blp_rank_sets: set g owns entries [set_ptr[g], set_ptr[g + 1]) of set_row (nnz) int64
 * GLOBAL rows, STRICTLY ASCENDING within a set; set_ptr (G + 1) int64 is trusted to be non-decreasing from 0 to nnz.  Within
 * each side the queries are ordered by non-decreasing set: set g serves the head-replacing queries [qset_ptr_head[g],
 * qset_ptr_head[g + 1]) and the tail-replacing queries q_head + [qset_ptr_tail[g], qset_ptr_tail[g + 1]) -- both (G + 1)
 * int64, non-decreasing, from 0 to q_head / to q_tail.  A set may serve both sides, one side or no query.
 * Output per query, k slots, in the caller's (grouped) query order: rows (Q, k) int64 global rows, scores (Q, k) f32 --
 * blp_topk's output taken over the entries of the query's set that lie in [row_base, row_base + N):
 *   scores are score_fn's values bit for bit (the torch-CPU order of oracle/blp_oracle.c, sign of zero included);
 *   order: descending score by IEEE comparison, equal scores (-0 == +0) by ascending row, NaN after every number (by row);
 *   filter (optional): a blp_filter with blp_rank_all's semantics whose row_base MUST equal this call's (else
 *          BLP_ERR_BAD_ARG); filtered rows are REMOVED, not demoted; exclude[q] is never removed;
 *   slots left over (an empty set, a set smaller than k, a filter that leaves fewer than k rows, a shard that holds fewer
 *          than k of the set's rows): row -1, score NaN (the quiet NaN 0x7fc00000).
 * Shards: an entry outside [row_base, row_base + N) is SKIPPED, so the per-shard results of several row_base shards, merged
 * by blp_topk_merge, equal the unsharded call.
 * Limits (blp_topk_sets_supported): the four models at D in {64, 128, 256}; 1 <= k <= 256; Q x k < 2^31; nnz < 2^31;
 * row_base + N <= 2^31; table / source / rel_emb 16-byte aligned, ld % 4 == 0, ld_src % 4 == 0.
 * Workspace: blp_topk_sets_workspace_bytes(model, D, q_head, q_tail, G, nnz, k) bytes, 256-B aligned: the queries'
 * coefficient rows (2 D floats per query), G + 1 int64 of work-unit offsets and the partial lists of k 8-byte keys -- at most
 * Q + 16 384 of them whatever nnz (long sets are cut into slabs only while the queries alone do not fill the device).  It
 * does not depend on N and is <= 8 (D + k) Q + 8 (G + 1) + 4 MiB bytes.
 * Asynchronous on `stream`, no host synchronisation, no allocation; nothing about set or group sizes is read on the host.
 * Deterministic: a query's result is the set of its k largest keys, so nothing depends on the grid.
 * (Added after 6.0.0 without a version change: no existing entry point changed.)
 * -------------------------------------------------------------------------------------------- */
int blp_topk_sets_supported(int model, int D, int k);
size_t blp_topk_sets_workspace_bytes(int model, int D, int64_t q_head, int64_t q_tail, int64_t G, int64_t nnz, int k);
int blp_topk_sets(int model, const float *table, int64_t N, int D, int64_t ld, int64_t row_base, const float *source, int64_t S,
                  int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R, const int64_t *rel_id, int64_t q_head,
                  int64_t q_tail, int k, const int64_t *set_ptr, const int64_t *set_row, int64_t nnz, int64_t G,
                  const int64_t *qset_ptr_head, const int64_t *qset_ptr_tail, const blp_filter *filter, int64_t *rows,
                  float *scores, void *workspace, size_t workspace_bytes, int device, void *stream);
/* blp_topk_sets over a candidate table in any storage type (table_dtype: BLP_DTYPE_*; see "THE CANDIDATE TABLE MAY COME IN A
 * 16-BIT STORAGE TYPE" above): the same contract on the table WIDENED to f32 exactly -- the same rows in the same order and
 * the reference's f32 scores of the widened rows bit for bit (sign of zero included), with the same set, shard (row_base),
 * filter / exclude semantics, the same -1 / quiet-NaN slots, the same limits and the same workspace (it does not depend on the
 * storage type), independent of the grid.  A 16-bit table's row stride ld is in ELEMENTS, ld % 8 == 0, 16-byte aligned base;
 * source and rel_emb stay f32 (the queries' vectors: gather and widen the Q fixed rows, blp_gather_triple_vectors).
 * BLP_DTYPE_F32 is blp_topk_sets itself.  An unknown table_dtype is BLP_ERR_BAD_ARG (the _supported / _workspace_bytes calls
 * answer 0).  The 16-bit rows are gathered as they are: half the cache lines of the f32 table per set entry.
 * (Added after 6.0.0 without a version change: no existing entry point changed.) */
int blp_topk_sets_typed_supported(int model, int table_dtype, int D, int k);
size_t blp_topk_sets_typed_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail, int64_t G,
                                           int64_t nnz, int k);
int blp_topk_sets_typed(int model, const void *table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                        const float *source, int64_t S, int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R,
                        const int64_t *rel_id, int64_t q_head, int64_t q_tail, int k, const int64_t *set_ptr,
                        const int64_t *set_row, int64_t nnz, int64_t G, const int64_t *qset_ptr_head,
                        const int64_t *qset_ptr_tail, const blp_filter *filter, int64_t *rows, float *scores, void *workspace,
                        size_t workspace_bytes, int device, void *stream);
/* Filtered top-k inside candidate sets shared between queries for TransE at ANY width: blp_topk_sets_wide is
 * blp_topk_sets_typed -- the contract above word for word: the sets CSR of strictly ascending global rows, row_base shards with
 * entries outside [row_base, row_base + N) skipped (shards merged by blp_topk_merge equal the unsharded call), the grouping by
 * qset_ptr_head / qset_ptr_tail, the filter (rows removed, exclude[q] never), the (Q, k) rows and scores in grouped order:
 * descending score, ties by ascending row, NaN last, left-over slots -1 / quiet NaN; scores are the reference's f32 score_fn
 * bit for bit, sign of zero included (a 16-bit table: of the table widened to f32) -- at the widths blp_topk_sets_supported
 * refuses: the BOW / DKRL encoders' 300 and 768.  A lane holds 64 columns of its set row at a time and the running sums of a
 * chunk of min(16, what the lists' LDS holds at this k) queries of the set's group (topk_sets_wide.hip): 16 for k <= 48, 12 at
 * k = 64, 4 at k = 192, 3 at k = 256.  The winners' scores come straight from the selection keys: there is no re-scoring pass.
 * Limits (blp_topk_sets_wide_supported): BLP_MODEL_TRANSE only, table_dtype a BLP_DTYPE_*, D % 4 == 0 and 4 <= D <= 1024 --
 * 64 / 128 / 256 included, where it is a second implementation of the same bits (blp_topk_sets is the faster one: chunks of up
 * to 32 queries); 1 <= k <= 256; the other models, other widths and unknown dtypes answer 0.  Q x k < 2^31; nnz < 2^31;
 * row_base + N <= 2^31; table / source / rel_emb 16-byte aligned, ld % 4 == 0 (f32) or ld % 8 == 0 (a 16-bit table, in
 * elements), ld_src % 4 == 0.  Status codes, messages and the order of the checks as blp_topk_sets_typed; every check runs
 * before a device is touched.
 * Workspace: blp_topk_sets_wide_workspace_bytes(model, table_dtype, D, q_head, q_tail, G, nnz, k) bytes (0 where unsupported
 * or a size is negative), 256-B aligned: per-query coefficient rows (2 D floats per head-replacing query, D per tail-replacing
 * one), G + 1 int64 of work-unit offsets and the partial lists of k 8-byte keys -- at most Q + 8 192 of them whatever nnz --,
 * each part rounded up to 256 bytes.  It does not depend on N or on the table's type, never shrinks when Q, G, k or nnz grow,
 * and is <= 8 (D + k) Q + 8 (G + 1) + 4 MiB bytes.
 * Asynchronous on `stream`, no host synchronisation, no allocation; nothing about set or group sizes is read on the host.
 * Deterministic: a query's result is the set of its k largest keys, so nothing depends on the grid.
 * (Added after 6.0.0 without a version change: no existing entry point changed.) */
int blp_topk_sets_wide_supported(int model, int table_dtype, int D, int k);
size_t blp_topk_sets_wide_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail, int64_t G,
                                          int64_t nnz, int k);
int blp_topk_sets_wide(int model, const void *table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                       const float *source, int64_t S, int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R,
                       const int64_t *rel_id, int64_t q_head, int64_t q_tail, int k, const int64_t *set_ptr,
                       const int64_t *set_row, int64_t nnz, int64_t G, const int64_t *qset_ptr_head,
                       const int64_t *qset_ptr_tail, const blp_filter *filter, int64_t *rows, float *scores, void *workspace,
                       size_t workspace_bytes, int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * Filtered top-k INSIDE per-query candidate lists: ANSWER a query (h, r, ?) / (?, r, t) with the k entries of ITS OWN LIST
 * the model scores highest -- the candidates a first stage (BM25, a type index, an ANN probe) hands over, re-ranked, known
 * edges removed.  The contract is the union of blp_rank_lists' (queries, table, lists) and blp_topk's (output).  Only the
 * listed rows are read; no score is written out and nothing is sorted.
 *
 * Queries, table and lists exactly as in blp_rank_lists (there is no true_row): Q = q_head + q_tail, head-replacing first;
 * fixed_row indexes source (S, D) f32 (row stride ld_src), rel_id indexes rel_emb (R, D) contiguous; table (N, D) in
 * table_dtype (BLP_DTYPE_*, widened exactly), row stride ld in elements -- GLOBAL rows [row_base, row_base + N); query q owns
 * entries [list_ptr[q], list_ptr[q + 1]) of list_row (nnz) int64 GLOBAL rows, list_ptr (Q + 1) int64 trusted to be
 * non-decreasing from 0 to nnz.  An entry outside [row_base, row_base + N) (-1 padding, another shard's row) is SKIPPED.
 * A list is a MULTISET: every valid entry competes, so a row listed twice may come back twice -- in adjacent slots, with the
 * same row and the same score.
 * Output per query, k slots: rows (Q, k) int64 global rows, scores (Q, k) f32:
 *   scores are score_fn's values bit for bit (the torch-CPU order of oracle/blp_oracle.c, sign of zero included; for a 16-bit
 *          table: of the table widened to f32);
 *   order: descending score by IEEE comparison, equal scores (-0 == +0) by ascending row, entries whose score is NaN after
 *          every number (by row); a NaN score comes out as the quiet NaN 0x7fc00000, its row >= 0;
 *   filter (optional): a blp_filter with blp_rank_lists' semantics whose row_base MUST equal this call's (else
 *          BLP_ERR_BAD_ARG); filtered rows are REMOVED, a filter entry removes every copy of its row; exclude[q] is never
 *          removed;
 *   slots left over (an empty list, a list with fewer than k valid entries, a filter that leaves fewer): row -1, score
 *          0x7fc00000.
 * Shards: the per-shard results of several row_base shards, side by side, merged by blp_topk_merge equal the unsharded call.
 * Limits: blp_topk_lists_supported(model, table_dtype, D, k) = blp_rank_lists_supported(model, table_dtype, D) and
 * 1 <= k <= 256; nnz < 2^31; row_base + N <= 2^31; Q <= 2^30; Q x k < 2^31; table rows / source / rel_emb 16-byte aligned
 * (ld % 4 == 0, a 16-bit table: ld % 8 == 0, in elements; ld_src % 4 == 0).  An unknown table_dtype is BLP_ERR_BAD_ARG (the
 * _supported / _workspace_bytes calls answer 0).  Every check runs before a device is touched.
 * Workspace: blp_topk_lists_workspace_bytes(...) bytes, 256-B aligned.  A query's list is cut into S slabs, S computed from Q
 * and nnz alone: S = 1 when Q >= 2048, else min(ceil(2048 / Q), max(1, ceil(ceil(nnz / (64 Q)) / 4)), 256).  S = 1 needs no
 * workspace (0 bytes, workspace may be NULL); S > 1 needs Q x S x k 8-byte keys rounded up to 256 bytes -- fewer than 4 096 lists
 * of k keys whatever nnz, independent of N and the storage type.
 * Asynchronous on `stream`, no host synchronisation, no allocation.  Deterministic: a query's result is the multiset of its k
 * largest keys, so nothing depends on the grid or the slabs.
 * (Added after 6.0.0 without a version change: no existing entry point changed.)
 * -------------------------------------------------------------------------------------------- */
int blp_topk_lists_supported(int model, int table_dtype, int D, int k);
size_t blp_topk_lists_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail, int64_t nnz, int k);
int blp_topk_lists(int model, const void *table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                   const float *source, int64_t S, int64_t ld_src, const int64_t *fixed_row, const float *rel_emb, int64_t R,
                   const int64_t *rel_id, int64_t q_head, int64_t q_tail, const int64_t *list_ptr, const int64_t *list_row,
                   int64_t nnz, int k, const blp_filter *filter, int64_t *rows, float *scores, void *workspace,
                   size_t workspace_bytes, int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * RELATION prediction: the third question of knowledge-graph completion, (h, ?, t) -- which relation holds between two
 * entities.  The candidates are the rows of rel_emb; the (Q, R) score matrix is never needed to rank or to predict.
 *
 * Queries: query q is the pair (row head_row[q], row tail_row[q]) of source (S, D) f32, row stride ld_src (rows trusted to lie
 * in [0, S)).  As everywhere in this ABI the queries' vectors are f32: a caller with a 16-bit table gathers and widens them
 * with blp_gather_triple_vectors.  head_row[q] == tail_row[q] is legal.
 * Candidates: all R rows of rel_emb (R, D) f32, contiguous.
 * blp_rank_relations:
 *   counts (Q, 4) int32 = {gt, ge, gt_filt, ge_filt}: the relations that score above / at least relation true_rel[q] (Q int64,
 *          trusted to lie in [0, R)) by IEEE comparison.  The true relation is a candidate like any other, so it adds to ge
 *          (unless its score is NaN); blp_rank_metrics applies unchanged.  counts needs true_rel.
 *   scores (Q, R) f32, row stride ld_scores >= R: score_fn's value of every (pair, relation) bit for bit (the torch-CPU order
 *          of oracle/blp_oracle.c, sign of zero included); floats [R, ld_scores) of a row are not touched.
 *   Either output may be NULL, not both.
 * blp_topk_relations: rels (Q, k) int64 relation ids, scores (Q, k) f32, in blp_topk's order and padding exactly: descending
 *   score, equal scores (-0 == +0) by ascending relation id, NaN scores after every number (by id) and written as 0x7fc00000;
 *   filtered relations are REMOVED; slots left over are -1 / 0x7fc00000; k > R is legal.
 * Filter (optional): a blp_filter whose `values` are RELATION ids -- ent2idx must be NULL and row_base 0, else
 *   BLP_ERR_BAD_ARG.  Query q loses the relations values[seg_lo[q] .. seg_hi[q]); an id outside [0, R) is ignored; exclude[q]
 *   is never removed; a segment's entries are trusted to be distinct.  Filtered relations leave gt_filt / ge_filt.  Segments are
 *   walked entry by entry per query: they are meant to be the handful of known relations of one pair.
 * Limits: the four models at D in {64, 128, 256} (blp_rank_relations_supported; the top-k call also 1 <= k <= 256);
 *   1 <= R < 2^31; Q <= 2^30; Q x k < 2^31; source / rel_emb / outputs 16-byte aligned, ld_src % 4 == 0, ld_src >= D.
 *   Q = 0 succeeds and touches nothing.  Every check runs before a device is touched.
 * Workspace, 256-B aligned: blp_rank_relations_workspace_bytes = 4 Q bytes rounded up to 256 (the true relations' scores;
 *   used with counts only: a scores-only call accepts NULL), whatever R; blp_topk_relations_workspace_bytes = 0 for every Q,
 *   R, k (the k-lists live in on-chip memory and every query has one owning workgroup: there is nothing to merge), workspace
 *   may be NULL.
 * Asynchronous on `stream`, no host synchronisation, no allocation.  Deterministic: counts are integer sums, a top-k result
 * is the set of the k largest keys; nothing depends on the grid.
 * (Added after 6.0.0 without a version change: no existing entry point changed.)
 * -------------------------------------------------------------------------------------------- */
int blp_rank_relations_supported(int model, int D);
size_t blp_rank_relations_workspace_bytes(int model, int D, int64_t Q, int64_t R);
int blp_rank_relations(int model, const float *source, int64_t S, int D, int64_t ld_src, const int64_t *head_row,
                       const int64_t *tail_row, int64_t Q, const float *rel_emb, int64_t R, const int64_t *true_rel,
                       const blp_filter *filter, int32_t *counts, float *scores, int64_t ld_scores, void *workspace,
                       size_t workspace_bytes, int device, void *stream);
int blp_topk_relations_supported(int model, int D, int k);
size_t blp_topk_relations_workspace_bytes(int model, int D, int64_t Q, int64_t R, int k);
int blp_topk_relations(int model, const float *source, int64_t S, int D, int64_t ld_src, const int64_t *head_row,
                       const int64_t *tail_row, int64_t Q, const float *rel_emb, int64_t R, int k, const blp_filter *filter,
                       int64_t *rels, float *scores, void *workspace, size_t workspace_bytes, int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * Relation prediction for TransE at ANY width: blp_rank_relations_wide and blp_topk_relations_wide are blp_rank_relations and
 * blp_topk_relations -- the same argument lists, the same outputs bit for bit (counts; scores with the reference's sign of
 * zero; top-k order, padding, NaN as 0x7fc00000), the same filter rules, argument checks, error codes and order of checks --
 * at the widths the BOW / DKRL encoders train TransE at (300: GloVe, 768: BERT embeddings), where a relation row no longer
 * fits a lane's registers.  A caller switches by name.
 * Limits: model BLP_MODEL_TRANSE only, D % 4 == 0 and 4 <= D <= 1024 (blp_rank_relations_wide_supported; the top-k call also
 *   1 <= k <= 256); any other model or width: BLP_ERR_UNSUPPORTED_DIM.  64 / 128 / 256 are inside the rule: there the two
 *   pairs of calls give identical results.  Everything else as above: 1 <= R < 2^31; Q <= 2^30; Q x k < 2^31; source /
 *   rel_emb / outputs 16-byte aligned, ld_src % 4 == 0, ld_src >= D; Q = 0 succeeds and touches nothing; every check runs
 *   before a device is touched.
 * Workspace, 256-B aligned: blp_rank_relations_wide_workspace_bytes = 4 Q bytes rounded up to 256 (the true relations'
 *   scores; used with counts only), whatever R and D; blp_topk_relations_wide_workspace_bytes = 0 (one owning workgroup per
 *   query, its k-lists in on-chip memory; the winners' scores are written from the selection keys, which carry them exactly).
 * TransE's sum runs strictly left to right, so the kernels carry one running sum per (relation, query) across 64-column slabs
 * of the relation row: the value after the last column is score_fn's, bit for bit, at every width.
 * Asynchronous on `stream`, no host synchronisation, no allocation.  Deterministic; nothing depends on the grid.
 * (Added after 6.0.0 without a version change: no existing entry point changed.)
 * -------------------------------------------------------------------------------------------- */
int blp_rank_relations_wide_supported(int model, int D);
size_t blp_rank_relations_wide_workspace_bytes(int model, int D, int64_t Q, int64_t R);
int blp_rank_relations_wide(int model, const float *source, int64_t S, int D, int64_t ld_src, const int64_t *head_row,
                            const int64_t *tail_row, int64_t Q, const float *rel_emb, int64_t R, const int64_t *true_rel,
                            const blp_filter *filter, int32_t *counts, float *scores, int64_t ld_scores, void *workspace,
                            size_t workspace_bytes, int device, void *stream);
int blp_topk_relations_wide_supported(int model, int D, int k);
size_t blp_topk_relations_wide_workspace_bytes(int model, int D, int64_t Q, int64_t R, int k);
int blp_topk_relations_wide(int model, const float *source, int64_t S, int D, int64_t ld_src, const int64_t *head_row,
                            const int64_t *tail_row, int64_t Q, const float *rel_emb, int64_t R, int k,
                            const blp_filter *filter, int64_t *rels, float *scores, void *workspace, size_t workspace_bytes,
                            int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * Relation prediction for DistMult / ComplEx / SimplE at ANY width: blp_rank_relations_wide_bilinear and
 * blp_topk_relations_wide_bilinear are blp_rank_relations and blp_topk_relations -- the same argument lists, the same outputs
 * bit for bit (counts {gt, ge, gt_filt, ge_filt}; scores (Q, R) with ld_scores, the torch-CPU order of oracle/blp_oracle.c,
 * sign of zero included; counts only, scores only or both; top-k order, padding, NaN as 0x7fc00000, removed relations
 * removed, k > R legal), the same filter rules (values are relation ids, ent2idx NULL, row_base 0, exclude[q] never
 * removed), argument checks, error codes, messages and order of checks -- at the widths the BOW / DKRL encoders train the
 * bilinear models at (300, 768).  A caller switches by name.
 * Limits: BLP_MODEL_DISTMULT / BLP_MODEL_COMPLEX / BLP_MODEL_SIMPLE, D % 4 == 0 and 4 <= D <= 1024
 *   (blp_rank_relations_wide_bilinear_supported; the top-k call also 1 <= k <= 256); TransE and any other width:
 *   BLP_ERR_UNSUPPORTED_DIM.  64 / 128 / 256 are inside the rule, as a second implementation of the same bits.  Everything
 *   else as above: 1 <= R < 2^31; Q <= 2^30; Q x k < 2^31; source / rel_emb / outputs 16-byte aligned, ld_src % 4 == 0,
 *   ld_src >= D; Q = 0 succeeds and touches nothing; every check runs before a device is touched.
 * Workspace, 256-B aligned: blp_rank_relations_wide_bilinear_workspace_bytes = 4 Q bytes rounded up to 256 (the true
 *   relations' keys; used with counts only: a scores-only call accepts NULL), whatever R and D;
 *   blp_topk_relations_wide_bilinear_workspace_bytes = 0, NULL accepted (one owning workgroup per query, its k-lists in
 *   on-chip memory; the winners' scores are written from the selection keys, which carry them exactly).  Both answer 0 where
 *   unsupported or a size is negative.
 * The sum of a score is torch's sum(dim=-1) order restated by eight lanes per relation row (the arithmetic of
 * blp_rank_all_wide, the relation row in the candidate's place).
 * Asynchronous on `stream`, no host synchronisation, no allocation, no global atomics.  Deterministic; nothing depends on the
 * grid.
 * (Added after 6.0.0 without a version change: no existing entry point changed.)
 * -------------------------------------------------------------------------------------------- */
int blp_rank_relations_wide_bilinear_supported(int model, int D);
size_t blp_rank_relations_wide_bilinear_workspace_bytes(int model, int D, int64_t Q, int64_t R);
int blp_rank_relations_wide_bilinear(int model, const float *source, int64_t S, int D, int64_t ld_src, const int64_t *head_row,
                                     const int64_t *tail_row, int64_t Q, const float *rel_emb, int64_t R, const int64_t *true_rel,
                                     const blp_filter *filter, int32_t *counts, float *scores, int64_t ld_scores, void *workspace,
                                     size_t workspace_bytes, int device, void *stream);
int blp_topk_relations_wide_bilinear_supported(int model, int D, int k);
size_t blp_topk_relations_wide_bilinear_workspace_bytes(int model, int D, int64_t Q, int64_t R, int k);
int blp_topk_relations_wide_bilinear(int model, const float *source, int64_t S, int D, int64_t ld_src, const int64_t *head_row,
                                     const int64_t *tail_row, int64_t Q, const float *rel_emb, int64_t R, int k,
                                     const blp_filter *filter, int64_t *rels, float *scores, void *workspace,
                                     size_t workspace_bytes, int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * Re-ranking a first-stage retrieval run (reference retrieval.py rerank: BM25F candidates of DBpedia-Entity v2 re-scored
 * with entity embeddings, the mixing weight alpha chosen per fold by nDCG@100).  Candidates are a CSR over Q queries:
 * query q owns candidates [cand_ptr[q], cand_ptr[q + 1]) (cand_ptr (Q + 1) int64, cand_ptr[0] = 0, cand_ptr[Q] = C).
 *
 * blp_rerank_supported(max_segment, D): 1 if both kernels take segments of up to max_segment candidates and embeddings of
 *   width D (any D >= 1; max_segment <= BLP_RERANK_MAX_SEGMENT).
 *
 * blp_rerank_cosine: s1 (C) f32 = F.normalize(table[cand_row[c]]) . F.normalize(query[q]) (retrieval.py:170-175) -- table
 *   (E, D) f32, row stride ld; query (Q, D) f32, row stride ldq; cand_row (C) int32, -1 = the entity has no description:
 *   s1 = 0.0f exactly (the reference's literal 0).  Norms n = sqrtf(sum x^2), x_i / max(n, 1e-12f), division and square
 *   root correctly rounded; every sum in one fixed order (stated in blp_amd/csrc/rerank.hip; blp_amd.retrieval.
 *   cosine_restated restates it bit for bit).  A row outside [-1, E) gives NaN.
 *
 * blp_rerank_ndcg: ndcg (A, Q, n_cut) f64 = trec_eval's ndcg_cut of every (alphas[a], query):
 *   c = alpha * s1 + (1 - alpha) * s2 in f64 (s2 (C) f64: the first-stage scores); candidates ranked by (float)c descending,
 *   ties (-0 == +0) by the LOWER index within the segment -- the caller orders each segment by docno descending, trec_eval's
 *   tie-break --, NaN last; DCG@k = sum over the first min(k, n) ranks i with gain > 0 of gain / log2_table[i], added in rank
 *   order in f64 (gain (C) int32: the qrels relevance, 0 if unjudged); nDCG = DCG / idcg[q, j] if idcg > 0, else 0.
 *   cutoffs: a HOST array of n_cut (1..BLP_RERANK_MAX_CUTOFFS) ascending cutoffs >= 1; log2_table (n_log2 >= the last cutoff)
 *   f64 = log2(i + 2); idcg (Q, n_cut) f64; alphas (A) f64.  max_segment: the caller's bound on cand_ptr[q + 1] - cand_ptr[q]
 *   (it sizes the launch); above BLP_RERANK_MAX_SEGMENT the call is refused (BLP_ERR_BAD_ARG); a segment longer than the
 *   given bound gets NaN results.
 * Both: no workspace, asynchronous, deterministic.
 * -------------------------------------------------------------------------------------------- */
#define BLP_RERANK_MAX_SEGMENT 8192
#define BLP_RERANK_MAX_CUTOFFS 8
int blp_rerank_supported(int64_t max_segment, int D);
int blp_rerank_cosine(const float *table, int64_t E, int D, int64_t ld, const float *query, int64_t Q, int64_t ldq,
                      const int64_t *cand_ptr, const int32_t *cand_row, int64_t C, float *s1, int device, void *stream);
int blp_rerank_ndcg(const float *s1, const double *s2, const int32_t *gain, const int64_t *cand_ptr, int64_t Q, int64_t C,
                    int64_t max_segment, const double *alphas, int A, const int32_t *cutoffs, int n_cut,
                    const double *log2_table, int64_t n_log2, const double *idcg, double *ndcg, int device, void *stream);

/* --------------------------------------------------------------------------------------------
 * Test / A-B hooks -- NOT part of the production library.  They are compiled only with -DBLP_TEST_HOOKS, into a second
 * library (blp_amd/libblp_hip.hooks.so) that tests/ and tools/ load; libblp_hip.so exports neither symbol and has no
 * mutable process-wide state.  The library never reads the environment; the kernel-selection and slab-size overrides the
 * parity tests need (force the exact f32 kernels, the f32-chain GEMM, tiny candidate slabs, ...) are process-wide integer
 * knobs of the hooks build, 0 = automatic (names: blp_amd/csrc/knobs.h).  Results never depend on a knob.
 * -------------------------------------------------------------------------------------------- */
#ifdef BLP_TEST_HOOKS
int blp_debug_set_knob(const char *name, long long value);

/* Test hook for the error band of the bilinear pre-pass: the NEXT blp_rank_all of the calling thread on a DistMult /
 * ComplEx / SimplE block (D = 128, >= 64 queries, one candidate slab) runs the SAME bf16 x 3 MFMA sequence and band
 * arithmetic as always but, instead of deciding, stores the approximate score S~ and the band half-width eps of every
 * (query, candidate) pair into two dense (Q, N) f32 matrices; `counts` of that call are meaningless.  One-shot (the
 * pointers are dropped when that call returns); NULL, NULL cancels. */
int blp_debug_gemm_dump(float *scores, float *eps);

/* Forget `device`'s self-test verdict: the next blp_selftest / bilinear block tests again (with knob "mfma_selftest" = 1 it
 * then reports a violation whatever it measures -- how tests reach the f32-chain route). */
int blp_debug_reset_selftest(int device);

/* The dynamic LDS bytes blp_topk_wide's table pass is launched with at (model, D, k): the larger of its two sides; 0 where
 * blp_topk_wide_supported says 0.  Host arithmetic only (the launch code's own function). */
size_t blp_debug_topk_wide_lds_bytes(int model, int D, int k);
#endif

#ifdef __cplusplus
}
#endif
#endif /* BLP_HIP_H */
