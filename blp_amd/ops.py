"""Torch-facing operators over the C-ABI (libblp_hip.so).  PyTorch is plumbing here: it owns the
device memory and the stream; every arithmetic step of the hot path runs in the HIP kernels.

    rank_all(...)       all-entities ranking counts        (train.py:146-171, utils.py:103-105)
    rank_metrics(...)   counts -> reciprocal ranks, hits   (utils.py:104-109)
    topk(...)           filtered top-k prediction per query (no score matrix)
    rank_lists(...)     counts / scores of per-query candidate lists (only the listed rows are read)
    rank_lists_wide(...) the same for DistMult / ComplEx / SimplE at any width D % 4 == 0, 4 <= D <= 1024
    rank_sets(...)      counts against candidate sets shared by groups of queries (type-constrained evaluation)
    rank_sets_wide(...) the same for TransE at any width D % 4 == 0, 4 <= D <= 1024 (the BOW / DKRL 300 and 768)
    rank_sets_wide_bilinear(...) the same for DistMult / ComplEx / SimplE at those widths, a float32 table
    topk_sets(...)      filtered top-k prediction inside candidate sets shared by groups of queries
    topk_sets_wide(...) the same for TransE at any width D % 4 == 0, 4 <= D <= 1024 (the BOW / DKRL 300 and 768)
    rerank_cosine(...)  cosine of every retrieval candidate with its query (retrieval.py:170-175)
    rerank_ndcg(...)    trec_eval ndcg_cut of every (alpha, query) of a re-ranked run (retrieval.py:139-258)
    score(...)          score_fn(heads, tails, rels)       (models.py:222-248), differentiable
    inbatch_loss(...)   compute_loss on in-batch negatives (models.py:51-70), differentiable

Tensors must live on a HIP device; there is no CPU implementation behind these functions (CPU
tensors are handled one level up, in blp_amd.models, with plain torch expressions).
"""
import collections
import ctypes

import torch

from . import _lib

_K_VALUES = (ctypes.c_int32 * 3)


def _stream(device):
    # (the raw hipStream_t of torch's current stream on `device`; the public torch.cuda.current_stream() builds a Stream
    # object around the same handle at ~2 us per call)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(device.index))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _addr(t):
    """The device address as a plain int (what a c_void_p argument takes without building a ctypes object), None = NULL."""
    return None if t is None else t.data_ptr()


def _filter_spec(filter, Q, dev):
    """SegmentFilter -> byref(blp_filter) (the tensors stay referenced by the caller's ``filter`` for the duration of the call)."""
    seg = [None if x is None else (x if x.dtype is torch.int64 and x.device == dev and x.is_contiguous()
                                   else x.to(device=dev, dtype=torch.int64).contiguous())
           for x in (filter.seg_lo, filter.seg_hi, filter.values, filter.exclude, filter.ent2idx)]
    if seg[0].shape[0] != Q or seg[1].shape[0] != Q or (seg[3] is not None and seg[3].shape[0] != Q):
        raise ValueError("SegmentFilter: seg_lo, seg_hi and exclude need one entry per query")
    spec = _lib.BlpFilter(seg[0].data_ptr(), seg[1].data_ptr(), seg[2].data_ptr() if seg[2].numel() else seg[0].data_ptr(),
                          None if seg[3] is None else seg[3].data_ptr(), None if seg[4] is None else seg[4].data_ptr(),
                          0 if seg[4] is None else seg[4].shape[0], int(filter.row_base))
    spec._keep = seg  # converted copies must outlive the (asynchronous) call's argument marshalling
    return ctypes.byref(spec)


# Ranking workspaces, one per (device, stream), grown on demand and kept: every kernel of a call runs on the caller's stream,
# so the next call on that stream is ordered behind it and may reuse the buffer (a torch.empty + a size query per call were
# ~4 us of a 20 us small call).  The sizes come from the library (blp_rank_all*_workspace_bytes), memoised per shape.
_workspaces = {}
_ws_bytes_memo = {}
# The cache is bounded two ways (round 4 kept the largest workspace per stream for the life of the process, so an evaluation's
# scratch -- hundreds of MB of operand images and pair lists -- stayed pinned through the training steps that followed it and a
# configuration that fitted before could run out of memory): (a) ranking.eval_link_prediction calls release_workspaces() when
# it is done, so nothing of an evaluation outlives it; (b) a workspace above WORKSPACE_CACHE_MAX_BYTES (the Wikidata5M-scale
# blocks: GBs) is never kept at all -- a per-call torch.empty that goes back to the caching allocator when the call returns
# (stream-ordered: the allocator hands the block to later work on the same stream only).  Everything below the cap is kept
# WITHIN an evaluation: allocating the FB15k-237 block's 250 MB per call cost the evaluation step 40 us and, when the allocator
# had split the block in between, a hipMalloc of ~9 ms now and then (profiles/r05/clustered_sweep.log, first version).
WORKSPACE_CACHE_MAX_BYTES = 1 << 30


def _workspace(dev, stream, nbytes):
    if nbytes > WORKSPACE_CACHE_MAX_BYTES:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    key = (dev.index, stream)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _workspaces[key] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    return buf


def release_workspaces():
    """Drop the cached ranking workspaces (they hold the largest requirement seen per stream)."""
    _workspaces.clear()


def _rank_ws_bytes(L, model, N, D, q_head, q_tail):
    if L is not _lib._product:  # the hooks build (tests, tools): its routing -- hence the size -- moves with the knobs
        return L.blp_rank_all_workspace_bytes(model, N, D, q_head, q_tail)
    key = (model, N, D, q_head, q_tail)
    n = _ws_bytes_memo.get(key)
    if n is None:
        if len(_ws_bytes_memo) > 4096:
            _ws_bytes_memo.clear()
        n = _ws_bytes_memo[key] = L.blp_rank_all_workspace_bytes(model, N, D, q_head, q_tail)
    return n


def _i64_vector(t):
    """(Q,) int64, contiguous -- as given when it already is."""
    if t.dtype is torch.int64 and t.dim() == 1 and t.is_contiguous():
        return t
    return t.reshape(-1).to(torch.int64).contiguous()


def _f32_matrix(t, D, name):
    """(Q, D) float32, contiguous -- as given when it already is."""
    if t.dtype is torch.float32 and t.dim() == 2 and t.shape[1] == D and t.is_contiguous():
        return t
    return _f32_rows(t, name).reshape(-1, D).contiguous()


def _require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("blp_amd.ops works on HIP device tensors only (got a CPU tensor); "
                               "there is no CPU fallback in the product path")


def _f32_rows(t, name):
    """float32, unit stride along the last dim (rows may be strided)."""
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if t.stride(-1) != 1 and t.shape[-1] != 1:
        t = t.contiguous()
    return t


TABLE_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}  # BLP_DTYPE_* of include/blp_hip.h


def _table_rows(t, name):
    """A candidate table: float32, or the 16-bit copy the table build can emit next to it (float16 / bfloat16: rows start on
    16-byte boundaries); unit stride along the last dim."""
    if t.dtype not in TABLE_DTYPES:
        raise TypeError(f"{name} must be float32, float16 or bfloat16, got {t.dtype}")
    if t.stride(-1) != 1 and t.shape[-1] != 1:
        t = t.contiguous()
    if t.dtype != torch.float32 and t.dim() == 2 and (t.stride(0) % 8 or t.data_ptr() % 16):
        # (a width that is not a multiple of 8 -- the bag-of-words 300 --: rows padded to the next multiple, a copy)
        wide = torch.zeros((t.shape[0], (t.shape[1] + 7) // 8 * 8), dtype=t.dtype, device=t.device)
        wide[:, :t.shape[1]] = t
        t = wide[:, :t.shape[1]]
    return t


# The filtered setting as segments of a sorted index of the filtering graph (include/blp_hip.h: blp_filter;
# built by blp_amd.utils.FilterIndex.segments): seg_lo, seg_hi (Q,) int64 slices of `values` (entity ids),
# exclude (Q,) the triple's own entity, ent2idx the id -> table row map (None: values are rows), row_base the
# first global row of a candidate shard.  Everything stays on the device; nothing is materialised per batch.
SegmentFilter = collections.namedtuple("SegmentFilter", "seg_lo seg_hi values exclude ent2idx row_base")


_selftested = set()


def ensure_selftest(device, rel_model=None):
    """The matrix-pipe self-test of ``device`` (include/blp_hip.h: blp_selftest), once per process and device, from HERE -- a
    set-up step that waits for the stream -- so that no ranking call ever synchronises inside the C-ABI (which it would, under a
    process-wide mutex, if the first bilinear block of a device found the verdict open).  TransE never needs it."""
    if rel_model == "transe":
        return
    index = device.index if isinstance(device, torch.device) else int(device)
    if index not in _selftested:
        if torch.cuda.is_current_stream_capturing():  # (the test has to be waited for: the library then takes its provable pre-pass)
            return
        _lib.selftest(index, torch._C._cuda_getCurrentRawStream(index))
        _selftested.add(index)


def dim_supported(rel_model, dim):
    """True if the fused ranking kernels are compiled for this embedding width."""
    return bool(_lib.lib().blp_dim_supported(_lib.MODEL_IDS[rel_model], int(dim)))


def rank_all_supported(rel_model, dim, q_head, q_tail):
    """True if rank_all takes a block of this shape (fused kernels at 64 / 128 / 256, or the any-width
    TransE pre-pass at any D % 4 == 0 up to 1024); otherwise use score + rank_from_scores."""
    return bool(_lib.lib().blp_rank_all_supported(_lib.MODEL_IDS[rel_model], int(dim), int(q_head), int(q_tail)))


def rank_all(rel_model, table, q_fixed, q_rel, q_head, true_row=None, q_true=None,
             filt_rowptr=None, filt_col=None, out=None, rel_ids=None, filter=None, workspace=None):
    """Rank-count every query against every row of ``table`` in one pass over the table.

    table (N, D) f32; q_fixed, q_rel (Q, D) f32; queries [0, q_head) replace the head (q_fixed is the
    tail embedding), queries [q_head, Q) replace the tail (q_fixed is the head embedding).
    true_row (Q,) int64 rows of the true entities in ``table``  -- or -- q_true (Q, D) their vectors
    (sharded ranking).  filt_rowptr (Q+1,), filt_col (nnz,) int64: CSR of filtered rows per query -- or --
    filter: a SegmentFilter (slices of a FilterIndex on the device; no per-batch list).
    rel_ids: accepted for compatibility and ignored (it was an optimisation hint of the C-ABI before 6.0.0).
    workspace: optional uint8 device tensor of >= rank_all_workspace_bytes(...) bytes to use as the call's scratch (a caller
    that wants to look at it afterwards: prepass_stats); default: this module's own.
    Returns counts (Q, 4) int32: gt, ge, gt_filtered, ge_filtered.
    """
    return _rank_all_call(False, rel_model, table, q_fixed, q_rel, q_head, true_row, q_true, filt_rowptr, filt_col, out, rel_ids,
                          filter, workspace)


def _rank_all_call(wide, rel_model, table, q_fixed, q_rel, q_head, true_row, q_true, filt_rowptr, filt_col, out, rel_ids, filter,
                   workspace):
    """rank_all (blp_rank_all) and rank_all_wide (blp_rank_all_wide): the same arguments, checks and workspace cache."""
    _require_device(table, q_fixed, q_rel, true_row, q_true, filt_rowptr, filt_col, rel_ids)
    table = _f32_rows(table, "table")
    if table.dim() != 2:
        raise ValueError(f"table must be (N, D), got {tuple(table.shape)}")
    N, D = table.shape
    q_fixed = _f32_matrix(q_fixed, D, "q_fixed")
    q_rel = _f32_matrix(q_rel, D, "q_rel")
    Q = q_fixed.shape[0]
    if q_rel.shape[0] != Q:
        raise ValueError("q_fixed and q_rel must have the same number of rows")
    if not 0 <= q_head <= Q:
        raise ValueError(f"q_head = {q_head} outside [0, {Q}]")
    if (true_row is None) == (q_true is None):
        raise ValueError("give exactly one of true_row / q_true")
    if true_row is not None:
        true_row = _i64_vector(true_row)
        if true_row.shape[0] != Q:
            raise ValueError("true_row must have one entry per query")
    else:
        q_true = _f32_matrix(q_true, D, "q_true")
        if q_true.shape[0] != Q:
            raise ValueError("q_true must have one row per query")
    if rel_ids is not None:
        rel_ids = _i64_vector(rel_ids)
        if rel_ids.shape[0] != Q:
            raise ValueError("rel_ids must have one entry per query")
    if (filt_rowptr is None) != (filt_col is None):
        raise ValueError("filt_rowptr and filt_col go together")
    if filter is not None and filt_rowptr is not None:
        raise ValueError("give the filter as a CSR or as a SegmentFilter, not both")
    if filt_rowptr is not None:
        filt_rowptr = filt_rowptr.to(torch.int64).contiguous()
        filt_col = filt_col.to(torch.int64).contiguous()
        if filt_rowptr.shape[0] != Q + 1:
            raise ValueError("filt_rowptr must have Q + 1 entries")
        if filt_col.numel() == 0:  # empty CSR: keep a non-NULL pointer for the C-ABI
            filt_col = torch.zeros(1, dtype=torch.int64, device=filt_col.device)
    dev = table.device
    counts = out if out is not None else torch.empty((Q, 4), dtype=torch.int32, device=dev)
    if counts.shape != (Q, 4) or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError("out must be a contiguous (Q, 4) int32 tensor")
    if Q == 0:
        return counts
    if not wide:
        ensure_selftest(dev, rel_model)
    L = _lib.lib()
    model = _lib.MODEL_IDS[rel_model]
    ws_bytes = (L.blp_rank_all_wide_workspace_bytes(model, N, D, q_head, Q - q_head) if wide
                else _rank_ws_bytes(L, model, N, D, q_head, Q - q_head))
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    if workspace is None:
        workspace = _workspace(dev, stream, ws_bytes)
    elif not workspace.is_cuda or workspace.dtype != torch.uint8 or workspace.numel() < ws_bytes or workspace.data_ptr() % 256:
        raise ValueError(f"workspace must be a 256-byte aligned uint8 device tensor of >= {ws_bytes} bytes")
    if filter is not None:
        spec = _filter_spec(filter, Q, dev)
    elif filt_rowptr is not None:  # a CSR is the segment form with seg_lo = rowptr, seg_hi = rowptr + 1, values = col
        csr = _lib.BlpFilter(filt_rowptr.data_ptr(), filt_rowptr.data_ptr() + 8, filt_col.data_ptr(), None, None, 0, 0)
        spec = ctypes.byref(csr)
    else:
        spec = None
    call = L.blp_rank_all_wide if wide else L.blp_rank_all
    status = call(model, table.data_ptr(), N, D, table.stride(0) if N > 0 else D, q_fixed.data_ptr(), q_rel.data_ptr(),
                  _addr(true_row), _addr(q_true), q_head, Q - q_head, spec, counts.data_ptr(), workspace.data_ptr(),
                  ws_bytes, dev.index, stream)
    if status:
        _lib.check(status, "blp_rank_all_wide" if wide else "blp_rank_all")
    return counts


def rank_all_wide_supported(rel_model, dim):
    """True if rank_all_wide takes this model and width: DistMult / ComplEx / SimplE at any D % 4 == 0, 4 <= D <= 1024
    (include/blp_hip.h: blp_rank_all_wide_supported)."""
    return bool(_lib.lib().blp_rank_all_wide_supported(_lib.MODEL_IDS[rel_model], int(dim)))


def rank_all_wide(rel_model, table, q_fixed, q_rel, q_head, true_row=None, q_true=None, filt_rowptr=None, filt_col=None,
                  filter=None, out=None, workspace=None):
    """rank_all for DistMult / ComplEx / SimplE at any width D % 4 == 0, 4 <= D <= 1024 (the 300 / 768-wide bag-of-words and
    DKRL tables): the exact table pass of blp_rank_all_wide, no (Q, N) score matrix.  Arguments, filter forms (CSR or
    SegmentFilter), workspace and result as rank_all; workspace: >= rank_all_wide_workspace_bytes(...) bytes."""
    return _rank_all_call(True, rel_model, table, q_fixed, q_rel, q_head, true_row, q_true, filt_rowptr, filt_col, out, None,
                          filter, workspace)


def rank_all_wide_workspace_bytes(rel_model, N, D, q_head, q_tail):
    return int(_lib.lib().blp_rank_all_wide_workspace_bytes(_lib.MODEL_IDS[rel_model], int(N), int(D), int(q_head), int(q_tail)))


def table16_is_read_directly(rel_model, dtype, N, D, n_triples, batch, block_triples=None, ld=None):
    """include/blp_hip.h: blp_rank_all_batches_native16 -- True if rank_all_batches over a float16 / bfloat16 table of these sizes
    streams the 16-bit rows themselves (half the bytes per pass); False if the library would widen the table to f32 first.
    ``ld``: the row stride (elements) the call will be made with; default = what rank_all_batches passes for a contiguous
    ``table.to(dtype)`` copy (D, or D padded to a multiple of 8 by _table_rows when D % 8 != 0)."""
    if dtype not in TABLE_DTYPES or dtype == torch.float32:
        return False
    if ld is None:
        ld = (D + 7) // 8 * 8
    return bool(_lib.lib().blp_rank_all_batches_native16(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(N), int(D), ld, int(n_triples),
                                                         int(batch), int(batch if block_triples is None else block_triples)))


def rank_all_workspace_bytes(rel_model, N, D, q_head, q_tail):
    return int(_lib.lib().blp_rank_all_workspace_bytes(_lib.MODEL_IDS[rel_model], int(N), int(D), int(q_head), int(q_tail)))


PREPASS_PATHS = {0: "exact kernels (no pre-pass)", 1: "v_sad_u16 pre-pass", 2: "bf16 x 3 MFMA pre-pass", 3: "f32-chain MFMA pre-pass",
                 4: "any-width v_sad_u16 pre-pass"}


def prepass_stats(rel_model, N, D, q_head, q_tail, workspace):
    """include/blp_hip.h: blp_rank_all_prepass_stats -- what the pre-pass of the last rank_all(..., workspace=workspace) of this
    shape left to the exact path.  Waits for the stream.  {"pairs", "listed", "flagged_rows", "path", "decided_frac"};
    decided_frac is None on the paths that are not counted."""
    out = (ctypes.c_int64 * 4)()
    dev = workspace.device
    L = _lib.lib()
    _lib.check(L.blp_rank_all_prepass_stats(_lib.MODEL_IDS[rel_model], int(N), int(D), int(q_head), int(q_tail), workspace.data_ptr(),
                                            workspace.numel(), out, dev.index, torch._C._cuda_getCurrentRawStream(dev.index)),
               "blp_rank_all_prepass_stats")
    pairs, listed, flagged, path = (int(x) for x in out)
    undecided = None if listed < 0 else listed + flagged
    return {"pairs": pairs, "listed": listed, "flagged_rows": flagged, "path": PREPASS_PATHS[path],
            "decided_frac": None if undecided is None or pairs == 0 else 1.0 - undecided / pairs}


def rank_all_idx(rel_model, table, fixed_row, rel_emb, rel_ids, q_head, true_row, filter=None, out=None):
    """rank_all with the queries left as INDICES (blp_rank_all_shard with source == table): query q's fixed-entity vector is row
    ``fixed_row[q]`` of ``table``, its relation vector row ``rel_ids[q]`` of ``rel_emb`` (R, D) -- what the reference
    gathers into ``ent_emb[tails]`` / ``rel_emb(rels)`` (train.py:141-145), un-gathered: no (Q, D) arrays are built or
    streamed.  All indices must be in range (build_queries clamps and flags bad ids).  Same counts as rank_all."""
    return rank_all_shard(rel_model, table, table, fixed_row, rel_emb, rel_ids, q_head, true_row, filter=filter, out=out)


def rank_all_shard(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, true_row, filter=None, out=None):
    """One shard of the candidate axis (blp_rank_all_shard): ``table`` (N, D) holds this rank's rows of the entity table --
    the candidates --, ``source`` (S, D) the vectors the queries themselves are made of (the whole table, or the vectors
    of the entities in the triples: gather_triple_vectors), replicated on every rank; fixed_row / true_row (Q,) index
    ``source``, rel_ids (Q,) index ``rel_emb`` (R, D).  A SegmentFilter's row_base = this shard's first global row.
    Counts (Q, 4) int32 of this shard; the shards' counts add up to the unsharded ones.  ``source is table``: the
    unsharded index form (rank_all_idx)."""
    _require_device(table, source, fixed_row, rel_emb, rel_ids, true_row)
    table = _f32_rows(table, "table")
    source = table if source is table else _f32_rows(source, "source")
    rel_emb = _f32_rows(rel_emb, "rel_emb").contiguous()
    N, D = table.shape
    if source.dim() != 2 or source.shape[1] != D:
        raise ValueError(f"source must be (S, {D}), got {tuple(source.shape)}")
    fixed_row, rel_ids, true_row = _i64_vector(fixed_row), _i64_vector(rel_ids), _i64_vector(true_row)
    Q = fixed_row.shape[0]
    if rel_ids.shape[0] != Q or true_row.shape[0] != Q or rel_emb.shape[1] != D:
        raise ValueError("fixed_row, rel_ids and true_row need one entry per query; rel_emb must be (R, D)")
    if not 0 <= q_head <= Q:
        raise ValueError(f"q_head = {q_head} outside [0, {Q}]")
    dev = table.device
    counts = out if out is not None else torch.empty((Q, 4), dtype=torch.int32, device=dev)
    if counts.shape != (Q, 4) or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError("out must be a contiguous (Q, 4) int32 tensor")
    if Q == 0:
        return counts
    ensure_selftest(dev, rel_model)
    L = _lib.lib()
    model = _lib.MODEL_IDS[rel_model]
    ws_bytes = _rank_ws_bytes(L, model, N, D, q_head, Q - q_head)
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    workspace = _workspace(dev, stream, ws_bytes)
    spec = None if filter is None else _filter_spec(filter, Q, dev)
    status = L.blp_rank_all_shard(model, table.data_ptr(), N, D, table.stride(0) if N > 1 else D, source.data_ptr(), source.shape[0],
                                  source.stride(0) if source.shape[0] > 1 else D, fixed_row.data_ptr(), rel_emb.data_ptr(),
                                  rel_emb.shape[0], rel_ids.data_ptr(), true_row.data_ptr(), q_head, Q - q_head, spec, counts.data_ptr(),
                                  workspace.data_ptr(), ws_bytes, dev.index, stream)
    if status:
        _lib.check(status, "blp_rank_all_shard")
    return counts


def topk_supported(rel_model, dim, k, dtype=torch.float32):
    """True if topk takes this width, k and table dtype (include/blp_hip.h: blp_topk_typed_supported -- D in {64, 128, 256},
    1 <= k <= 256, a float32, float16 or bfloat16 table)."""
    if dtype not in TABLE_DTYPES:
        return False
    return bool(_lib.lib().blp_topk_typed_supported(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(dim), int(k)))


def topk_workspace_bytes(rel_model, N, D, q_head, q_tail, k, dtype=torch.float32):
    return int(_lib.lib().blp_topk_typed_workspace_bytes(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(N), int(D), int(q_head),
                                                         int(q_tail), int(k)))


def topk(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, k, filter=None, row_base=0, out=None):
    """Filtered top-k prediction (blp_topk): for each query -- head-replacing [0, q_head), then tail-replacing; fixed entity
    row fixed_row[q] of ``source`` (S, D), relation row rel_ids[q] of ``rel_emb`` (R, D) -- the k rows of ``table`` (N, D),
    global rows [row_base, row_base + N), with the highest score_fn value, as blp_topk orders them (descending score, ties by
    ascending row, NaN last; numpy's argsort(-scores, kind="stable")[:k]).  ``filter``: a SegmentFilter whose row_base is
    ``row_base``; the rows it names are removed.  Slots beyond the candidates left: row -1, score NaN.
    ``table`` may be float16 / bfloat16 (blp_topk_typed: the result is the float32 table's, widened exactly, read at half the
    bytes); ``source`` and ``rel_emb`` are float32.
    Returns (rows (Q, k) int64, scores (Q, k) float32); ``out`` may give both."""
    return _topk(False, rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, k, filter, row_base, out)


def topk_wide_supported(rel_model, dim, k, dtype=torch.float32):
    """True if topk_wide takes this model, width, k and table dtype (blp_topk_wide_supported: distmult / complex / simple,
    D % 4 == 0, 4 <= D <= 1024 -- the BOW / DKRL encoders' 300 and 768 --, 1 <= k <= 256; a float32 table only)."""
    if dtype != torch.float32:
        return False
    return bool(_lib.lib().blp_topk_wide_supported(_lib.MODEL_IDS[rel_model], int(dim), int(k)))


def topk_wide_workspace_bytes(rel_model, N, D, q_head, q_tail, k):
    """Bytes of topk_wide's workspace: the partial key lists only -- never a function of D, constant in N from 2^17 rows on
    (0: not supported, a negative size, or Q x k >= 2^31)."""
    return int(_lib.lib().blp_topk_wide_workspace_bytes(_lib.MODEL_IDS[rel_model], int(N), int(D), int(q_head), int(q_tail), int(k)))


def topk_wide(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, k, filter=None, row_base=0, out=None):
    """topk for DistMult / ComplEx / SimplE at any width D % 4 == 0, 4 <= D <= 1024 on a float32 table (blp_topk_wide: eight
    lanes per candidate row sum in the reference's order, the winners' scores come straight from the selection keys): same
    arguments, same rows and scores -- score_fn's bit for bit."""
    return _topk(True, rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, k, filter, row_base, out)


def _topk(wide, rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, k, filter, row_base, out):
    """topk (blp_topk_typed) and topk_wide (blp_topk_wide): one argument handling, two entries."""
    who = "topk_wide" if wide else "topk"
    _require_device(table, source, fixed_row, rel_emb, rel_ids)
    if source is table and table.dtype != torch.float32:
        raise TypeError("a 16-bit table needs a float32 `source` for the queries' vectors (ops.gather_triple_vectors + build_queries(by_position=True))")
    same = source is table
    table = _table_rows(table, "table")
    source = table if same else _f32_rows(source, "source")
    rel_emb = _f32_rows(rel_emb, "rel_emb").contiguous()
    N, D = table.shape
    if source.dim() != 2 or source.shape[1] != D:
        raise ValueError(f"source must be (S, {D}), got {tuple(source.shape)}")
    fixed_row, rel_ids = _i64_vector(fixed_row), _i64_vector(rel_ids)
    Q = fixed_row.shape[0]
    k = int(k)
    if rel_ids.shape[0] != Q or rel_emb.dim() != 2 or rel_emb.shape[1] != D:
        raise ValueError("fixed_row and rel_ids need one entry per query; rel_emb must be (R, D)")
    if not 0 <= q_head <= Q:
        raise ValueError(f"q_head = {q_head} outside [0, {Q}]")
    if wide and not topk_wide_supported(rel_model, D, k, table.dtype):
        raise ValueError(f"topk_wide: {rel_model} at D = {D}, k = {k} not supported (distmult / complex / simple, D % 4 == 0, "
                         "4 <= D <= 1024, 1 <= k <= 256, a float32 table): see topk_wide_supported")
    if not wide and not topk_supported(rel_model, D, k, table.dtype):
        raise ValueError(f"topk: D = {D}, k = {k} not supported (D in 64 / 128 / 256, 1 <= k <= 256): see topk_supported")
    if filter is not None and int(filter.row_base) != int(row_base):
        raise ValueError(f"{who}: the filter's row_base {filter.row_base} differs from row_base {row_base}")
    dev = table.device
    if out is None:
        out = (torch.empty((Q, k), dtype=torch.int64, device=dev), torch.empty((Q, k), dtype=torch.float32, device=dev))
    rows, scores = out
    if rows.shape != (Q, k) or rows.dtype != torch.int64 or not rows.is_contiguous() or scores.shape != (Q, k) or \
            scores.dtype != torch.float32 or not scores.is_contiguous():
        raise ValueError("out must be contiguous (Q, k) int64 rows and (Q, k) float32 scores")
    if Q == 0:
        return rows, scores
    L = _lib.lib()
    model = _lib.MODEL_IDS[rel_model]
    tdt = TABLE_DTYPES[table.dtype]
    if wide:  # (a float32 table: blp_topk's argument list, without the storage type)
        ws_bytes = L.blp_topk_wide_workspace_bytes(model, N, D, q_head, Q - q_head, k)
        entry, dtype_arg = L.blp_topk_wide, ()
    else:
        ws_bytes = L.blp_topk_typed_workspace_bytes(model, tdt, N, D, q_head, Q - q_head, k)
        entry, dtype_arg = L.blp_topk_typed, (tdt,)
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    workspace = _workspace(dev, stream, ws_bytes)
    spec = None if filter is None else _filter_spec(filter, Q, dev)
    status = entry(model, table.data_ptr(), *dtype_arg, N, D, table.stride(0) if tdt or N > 1 else D, int(row_base),
                   source.data_ptr(), source.shape[0], source.stride(0) if source.shape[0] > 1 else D, fixed_row.data_ptr(),
                   rel_emb.data_ptr(), rel_emb.shape[0], rel_ids.data_ptr(), q_head, Q - q_head, k, spec, rows.data_ptr(),
                   scores.data_ptr(), workspace.data_ptr(), ws_bytes, dev.index, stream)
    if status:
        _lib.check(status, "blp_topk_wide" if wide else "blp_topk_typed" if tdt else "blp_topk")
    return rows, scores


def rank_lists_supported(rel_model, dim, dtype=torch.float32):
    """True if rank_lists takes this width and table dtype (include/blp_hip.h: blp_rank_lists_supported -- TransE at any
    D % 4 == 0 up to 1024, the other models at 64 / 128 / 256; a float32, float16 or bfloat16 table)."""
    if dtype not in TABLE_DTYPES:
        return False
    return bool(_lib.lib().blp_rank_lists_supported(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(dim)))


def rank_lists(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, list_ptr, list_row, true_row=None, filter=None,
               row_base=0, want_scores=False, out=None):
    """Counts and / or scores of per-query candidate lists (blp_rank_lists).  Queries as in rank_all_shard -- head-replacing
    [0, q_head), then tail-replacing; fixed_row / true_row (Q,) index ``source`` (S, D) float32, rel_ids (Q,) index ``rel_emb``
    (R, D).  Query q owns entries [list_ptr[q], list_ptr[q + 1]) of ``list_row`` (nnz,) int64 GLOBAL rows of ``table`` (N, D)
    (float32 / float16 / bfloat16), which holds global rows [row_base, row_base + N); entries outside (-1 padding, another
    shard's rows) are skipped: counted nowhere, score NaN.  list_ptr (Q + 1,) must be non-decreasing from 0 to nnz.
    ``true_row`` given: counts (Q, 4) int32 {gt, ge, gt_filtered, ge_filtered} of the list's entries against the true entity's
    score (a multiset: duplicates count; ``filter``: a SegmentFilter whose row_base is ``row_base``).  ``want_scores`` (or no
    true_row): scores (nnz,) float32, score_fn's values bit for bit.  Returns (counts or None, scores or None); ``out`` may
    give both (None for the one not wanted)."""
    return _rank_lists(False, rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, list_ptr, list_row, true_row, filter,
                       row_base, want_scores, out)


def rank_lists_wide_supported(rel_model, dim, dtype=torch.float32):
    """True if rank_lists_wide takes this model, width and table dtype (blp_rank_lists_wide_supported: distmult, complex or
    simple, D % 4 == 0, 4 <= D <= 1024 -- the BOW / DKRL encoders' 300 and 768; a float32, float16 or bfloat16 table)."""
    if dtype not in TABLE_DTYPES:
        return False
    return bool(_lib.lib().blp_rank_lists_wide_supported(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(dim)))


def rank_lists_wide(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, list_ptr, list_row, true_row=None, filter=None,
                    row_base=0, want_scores=False, out=None):
    """rank_lists for DistMult / ComplEx / SimplE at any width D % 4 == 0, 4 <= D <= 1024 (blp_rank_lists_wide: eight lanes per
    (entry, query) pair in rank_all_wide's sum order, the query's coefficients staged per wave in LDS): same arguments, same
    counts and scores -- the reference's bit for bit, on a 16-bit table those of the table widened to float32.  At 64 / 128 /
    256 it gives rank_lists' bits by a second implementation."""
    return _rank_lists(True, rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, list_ptr, list_row, true_row, filter,
                       row_base, want_scores, out)


def _rank_lists(wide, rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, list_ptr, list_row, true_row, filter, row_base,
                want_scores, out):
    """rank_lists (blp_rank_lists) and rank_lists_wide (blp_rank_lists_wide): one argument handling, two entries."""
    who = "rank_lists_wide" if wide else "rank_lists"
    _require_device(table, source, fixed_row, rel_emb, rel_ids, list_ptr, list_row, true_row)
    if source is table and table.dtype != torch.float32:
        raise TypeError("a 16-bit table needs a float32 `source` for the queries' vectors")
    same = source is table
    table = _table_rows(table, "table")
    source = table if same else _f32_rows(source, "source")
    rel_emb = _f32_rows(rel_emb, "rel_emb").contiguous()
    N, D = table.shape
    if source.dim() != 2 or source.shape[1] != D:
        raise ValueError(f"source must be (S, {D}), got {tuple(source.shape)}")
    fixed_row, rel_ids, list_ptr, list_row = _i64_vector(fixed_row), _i64_vector(rel_ids), _i64_vector(list_ptr), _i64_vector(list_row)
    Q, nnz = fixed_row.shape[0], list_row.shape[0]
    if rel_ids.shape[0] != Q or list_ptr.shape[0] != Q + 1 or rel_emb.dim() != 2 or rel_emb.shape[1] != D:
        raise ValueError("fixed_row and rel_ids need one entry per query, list_ptr Q + 1; rel_emb must be (R, D)")
    if not 0 <= q_head <= Q:
        raise ValueError(f"q_head = {q_head} outside [0, {Q}]")
    if wide and not rank_lists_wide_supported(rel_model, D, table.dtype):
        raise ValueError(f"rank_lists_wide: {rel_model} at D = {D} not supported (distmult / complex / simple, D % 4 == 0, "
                         "4 <= D <= 1024: see rank_lists_wide_supported)")
    if not wide and not rank_lists_supported(rel_model, D, table.dtype):
        raise ValueError(f"rank_lists: D = {D} not supported for {rel_model} (see rank_lists_supported)")
    if filter is not None and int(filter.row_base) != int(row_base):
        raise ValueError(f"{who}: the filter's row_base {filter.row_base} differs from row_base {row_base}")
    want_scores = bool(want_scores) or true_row is None
    dev = table.device
    counts, scores = out if out is not None else (None, None)
    if true_row is not None:
        true_row = _i64_vector(true_row)
        if true_row.shape[0] != Q:
            raise ValueError("true_row needs one entry per query")
        if counts is None:
            counts = torch.empty((Q, 4), dtype=torch.int32, device=dev)
        if counts.shape != (Q, 4) or counts.dtype != torch.int32 or not counts.is_contiguous():
            raise ValueError("out[0] must be a contiguous (Q, 4) int32 tensor")
    else:
        counts = None
    if want_scores:
        if scores is None:
            scores = torch.empty((nnz,), dtype=torch.float32, device=dev)
        if scores.shape != (nnz,) or scores.dtype != torch.float32 or not scores.is_contiguous():
            raise ValueError("out[1] must be a contiguous (nnz,) float32 tensor")
    else:
        scores = None
    if Q == 0:
        return counts, scores
    L = _lib.lib()
    model = _lib.MODEL_IDS[rel_model]
    tdt = TABLE_DTYPES[table.dtype]
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    entry = "blp_rank_lists_wide" if wide else "blp_rank_lists"
    ws_bytes = getattr(L, entry + "_workspace_bytes")(model, tdt, D, q_head, Q - q_head) if counts is not None else 0
    workspace = _workspace(dev, stream, ws_bytes) if ws_bytes else None
    spec = None if filter is None else _filter_spec(filter, Q, dev)
    status = getattr(L, entry)(model, table.data_ptr(), tdt, N, D, table.stride(0) if tdt or N > 1 else D, int(row_base),
                               source.data_ptr(), source.shape[0], source.stride(0) if source.shape[0] > 1 else D, fixed_row.data_ptr(),
                               rel_emb.data_ptr(), rel_emb.shape[0], rel_ids.data_ptr(), _addr(true_row), q_head, Q - q_head,
                               list_ptr.data_ptr(), list_row.data_ptr(), nnz, spec, _addr(counts), _addr(scores), _addr(workspace),
                               ws_bytes, dev.index, stream)
    if status:
        _lib.check(status, entry)
    return counts, scores


def rank_sets_supported(rel_model, dim, dtype=torch.float32):
    """True if rank_sets takes this width and table dtype (include/blp_hip.h: blp_rank_sets_typed_supported -- the four models at
    64 / 128 / 256; a float32, float16 or bfloat16 table)."""
    if dtype not in TABLE_DTYPES:
        return False
    return bool(_lib.lib().blp_rank_sets_typed_supported(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(dim)))


def rank_sets_workspace_bytes(rel_model, D, q_head, q_tail, num_sets):
    return int(_lib.lib().blp_rank_sets_workspace_bytes(_lib.MODEL_IDS[rel_model], int(D), int(q_head), int(q_tail), int(num_sets)))


def rank_sets(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, true_row, set_ptr, set_row, qset_ptr_head,
              qset_ptr_tail, filter=None, row_base=0, out=None):
    """Counts of queries against candidate sets that queries SHARE (blp_rank_sets, blp_rank_sets_typed).  Queries as in rank_all_shard -- head-replacing
    [0, q_head), then tail-replacing; fixed_row / true_row (Q,) index ``source`` (S, D) float32, rel_ids (Q,) index ``rel_emb``
    (R, D) -- and, within each side, GROUPED by set: set g serves head queries [qset_ptr_head[g], qset_ptr_head[g + 1]) and
    tail queries q_head + [qset_ptr_tail[g], qset_ptr_tail[g + 1]) (both (G + 1,), from 0 to q_head / to Q - q_head).
    Set g is entries [set_ptr[g], set_ptr[g + 1]) of ``set_row`` (nnz,): GLOBAL rows of ``table`` (N, D) (float32 / float16 /
    bfloat16; a 16-bit table needs a float32 ``source``: the counts are those of the table widened to float32) -- which holds
    global rows [row_base, row_base + N) --, strictly ascending within a set; entries outside the shard are skipped.
    Returns counts (Q, 4) int32 {gt, ge, gt_filtered, ge_filtered} over the entries of each query's set (``filter``: a
    SegmentFilter whose row_base is ``row_base``; an entry of it counts only if its row is in the set)."""
    return _rank_sets(False, rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, true_row, set_ptr, set_row, qset_ptr_head,
                      qset_ptr_tail, filter, row_base, out)


def rank_sets_wide_supported(rel_model, dim, dtype=torch.float32):
    """True if rank_sets_wide takes this width and table dtype (blp_rank_sets_wide_supported: transe, D % 4 == 0, 4 <= D <= 1024 --
    the BOW / DKRL encoders' 300 and 768; a float32, float16 or bfloat16 table)."""
    if dtype not in TABLE_DTYPES:
        return False
    return bool(_lib.lib().blp_rank_sets_wide_supported(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(dim)))


def rank_sets_wide_workspace_bytes(rel_model, D, q_head, q_tail, num_sets, dtype=torch.float32):
    """Bytes of rank_sets_wide's workspace: true keys, accumulators, coefficient rows and num_sets + 1 unit offsets, whatever
    the table's length and the sets' sizes (0: not supported, or a negative size)."""
    if dtype not in TABLE_DTYPES:
        return 0
    return int(_lib.lib().blp_rank_sets_wide_workspace_bytes(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(D), int(q_head),
                                                            int(q_tail), int(num_sets)))


def rank_sets_wide(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, true_row, set_ptr, set_row, qset_ptr_head,
                   qset_ptr_tail, filter=None, row_base=0, out=None):
    """rank_sets for TransE at any width D % 4 == 0, 4 <= D <= 1024 (blp_rank_sets_wide: a lane holds 64 columns of its set row at
    a time and the running sums of a chunk of 16 queries of the set's group): same arguments, same counts -- the reference's bit
    for bit, on a 16-bit table those of the table widened to float32."""
    return _rank_sets(True, rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, true_row, set_ptr, set_row, qset_ptr_head,
                      qset_ptr_tail, filter, row_base, out)


def rank_sets_wide_bilinear_supported(rel_model, dim, dtype=torch.float32):
    """True if rank_sets_wide_bilinear takes this model, width and table dtype (blp_rank_sets_wide_bilinear_supported: distmult,
    complex or simple, D % 4 == 0, 4 <= D <= 1024, a float32 table)."""
    if dtype not in TABLE_DTYPES:
        return False
    return bool(_lib.lib().blp_rank_sets_wide_bilinear_supported(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(dim)))


def rank_sets_wide_bilinear_workspace_bytes(rel_model, D, q_head, q_tail, num_sets, dtype=torch.float32):
    """Bytes of rank_sets_wide_bilinear's workspace: true keys, accumulators and two unit prefixes of num_sets + 1 offsets,
    whatever the width, the table's length and the sets' sizes (0: not supported, or a negative size)."""
    if dtype not in TABLE_DTYPES:
        return 0
    return int(_lib.lib().blp_rank_sets_wide_bilinear_workspace_bytes(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(D), int(q_head),
                                                                     int(q_tail), int(num_sets)))


def rank_sets_wide_bilinear(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, true_row, set_ptr, set_row, qset_ptr_head,
                            qset_ptr_tail, filter=None, row_base=0, out=None):
    """rank_sets for DistMult / ComplEx / SimplE at any width D % 4 == 0, 4 <= D <= 1024 on a float32 table
    (blp_rank_sets_wide_bilinear: eight lanes per set row, the coefficients of a chunk of 8 queries of the set's group in LDS --
    rank_all_wide's sum order on gathered rows): same arguments, same counts -- the reference's bit for bit."""
    return _rank_sets("bilinear", rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, true_row, set_ptr, set_row, qset_ptr_head,
                      qset_ptr_tail, filter, row_base, out)


def _rank_sets(wide, rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, true_row, set_ptr, set_row, qset_ptr_head,
               qset_ptr_tail, filter, row_base, out):
    """rank_sets (blp_rank_sets_typed), rank_sets_wide (blp_rank_sets_wide) and rank_sets_wide_bilinear
    (blp_rank_sets_wide_bilinear; ``wide`` == "bilinear"): one argument handling, three entries."""
    bilinear = wide == "bilinear"
    who = "rank_sets_wide_bilinear" if bilinear else "rank_sets_wide" if wide else "rank_sets"
    _require_device(table, source, fixed_row, rel_emb, rel_ids, true_row, set_ptr, set_row, qset_ptr_head, qset_ptr_tail)
    if table.dtype not in TABLE_DTYPES:
        raise TypeError(f"{who} reads a float32, float16 or bfloat16 table, got {table.dtype}")
    if source is table and table.dtype != torch.float32:
        raise TypeError("a 16-bit table needs a float32 `source` for the queries' vectors")
    same = source is table
    table = _table_rows(table, "table")
    source = table if same else _f32_rows(source, "source")
    rel_emb = _f32_rows(rel_emb, "rel_emb").contiguous()
    N, D = table.shape
    if source.dim() != 2 or source.shape[1] != D:
        raise ValueError(f"source must be (S, {D}), got {tuple(source.shape)}")
    fixed_row, rel_ids, true_row = _i64_vector(fixed_row), _i64_vector(rel_ids), _i64_vector(true_row)
    set_ptr, set_row = _i64_vector(set_ptr), _i64_vector(set_row)
    qset_ptr_head, qset_ptr_tail = _i64_vector(qset_ptr_head), _i64_vector(qset_ptr_tail)
    Q, nnz, G = fixed_row.shape[0], set_row.shape[0], set_ptr.shape[0] - 1
    if rel_ids.shape[0] != Q or true_row.shape[0] != Q or rel_emb.dim() != 2 or rel_emb.shape[1] != D:
        raise ValueError("fixed_row, rel_ids and true_row need one entry per query; rel_emb must be (R, D)")
    if G < 0 or qset_ptr_head.shape[0] != G + 1 or qset_ptr_tail.shape[0] != G + 1:
        raise ValueError("set_ptr, qset_ptr_head and qset_ptr_tail need G + 1 entries each")
    if not 0 <= q_head <= Q:
        raise ValueError(f"q_head = {q_head} outside [0, {Q}]")
    if bilinear and not rank_sets_wide_bilinear_supported(rel_model, D, table.dtype):
        raise ValueError(f"rank_sets_wide_bilinear: {rel_model} with a {table.dtype} table at D = {D} not supported (distmult / complex / "
                         "simple, a float32 table, D % 4 == 0, 4 <= D <= 1024: see rank_sets_wide_bilinear_supported)")
    if wide and not bilinear and not rank_sets_wide_supported(rel_model, D, table.dtype):
        raise ValueError(f"rank_sets_wide: {rel_model} at D = {D} not supported (transe, D % 4 == 0, 4 <= D <= 1024: see rank_sets_wide_supported)")
    if not wide and not rank_sets_supported(rel_model, D, table.dtype):
        raise ValueError(f"rank_sets: D = {D} not supported (64 / 128 / 256: see rank_sets_supported)")
    if filter is not None and int(filter.row_base) != int(row_base):
        raise ValueError(f"{who}: the filter's row_base {filter.row_base} differs from row_base {row_base}")
    dev = table.device
    counts = torch.empty((Q, 4), dtype=torch.int32, device=dev) if out is None else out
    if counts.shape != (Q, 4) or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError("out must be a contiguous (Q, 4) int32 tensor")
    if Q == 0:
        return counts
    L = _lib.lib()
    model = _lib.MODEL_IDS[rel_model]
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    tdt = TABLE_DTYPES[table.dtype]
    entry = "blp_rank_sets_wide_bilinear" if bilinear else "blp_rank_sets_wide" if wide else "blp_rank_sets_typed"
    ws_bytes = getattr(L, entry + "_workspace_bytes")(model, tdt, D, q_head, Q - q_head, G)
    workspace = _workspace(dev, stream, ws_bytes)
    spec = None if filter is None else _filter_spec(filter, Q, dev)
    status = getattr(L, entry)(model, table.data_ptr(), tdt, N, D, table.stride(0) if tdt or N > 1 else D, int(row_base),
                                   source.data_ptr(), source.shape[0], source.stride(0) if source.shape[0] > 1 else D,
                                   fixed_row.data_ptr(), rel_emb.data_ptr(), rel_emb.shape[0], rel_ids.data_ptr(), true_row.data_ptr(),
                                   q_head, Q - q_head, set_ptr.data_ptr(), _addr(set_row) if nnz else None, nnz, G,
                                   qset_ptr_head.data_ptr(), qset_ptr_tail.data_ptr(), spec, counts.data_ptr(), workspace.data_ptr(),
                                   ws_bytes, dev.index, stream)
    if status:
        _lib.check(status, entry if wide or tdt else "blp_rank_sets")
    return counts


def topk_sets_supported(rel_model, dim, k, dtype=torch.float32):
    """True if topk_sets takes this width, k and table dtype (include/blp_hip.h: blp_topk_sets_typed_supported -- the four
    models at 64 / 128 / 256, 1 <= k <= 256; a float32, float16 or bfloat16 table)."""
    if dtype not in TABLE_DTYPES:
        return False
    return bool(_lib.lib().blp_topk_sets_typed_supported(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(dim), int(k)))


def topk_sets_workspace_bytes(rel_model, D, q_head, q_tail, num_sets, nnz, k):
    """Bytes of topk_sets' workspace: it depends on the queries, the number of sets, k and (boundedly) the number of set
    entries -- never on the table's length or its storage type."""
    return int(_lib.lib().blp_topk_sets_workspace_bytes(_lib.MODEL_IDS[rel_model], int(D), int(q_head), int(q_tail), int(num_sets),
                                                        int(nnz), int(k)))


def topk_sets(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, k, set_ptr, set_rows, qset_ptr_head, qset_ptr_tail,
              filter=None, row_base=0, out=None):
    """Filtered top-k prediction inside candidate sets that queries SHARE (blp_topk_sets, blp_topk_sets_typed).  Queries, sets and grouping as in
    rank_sets -- head-replacing [0, q_head), then tail-replacing; fixed_row (Q,) indexes ``source`` (S, D) float32, rel_ids
    (Q,) index ``rel_emb`` (R, D); within each side GROUPED by set: set g serves head queries [qset_ptr_head[g],
    qset_ptr_head[g + 1]) and tail queries q_head + [qset_ptr_tail[g], qset_ptr_tail[g + 1]); set g is entries [set_ptr[g],
    set_ptr[g + 1]) of ``set_rows`` (nnz,): GLOBAL rows of ``table`` (N, D) (float32 / float16 / bfloat16; a 16-bit table needs
    a float32 ``source``: the result is that of the table widened to float32) -- which holds global rows [row_base,
    row_base + N) --, strictly ascending within a set; entries outside the shard are skipped.  The output is topk's, taken over
    the query's set: the k entries with the highest score_fn value (descending score, ties by ascending row, NaN last), the
    rows ``filter`` (a SegmentFilter whose row_base is ``row_base``) names removed; slots beyond the entries left: row -1,
    score NaN.  Returns (rows (Q, k) int64, scores (Q, k) float32) in the caller's (grouped) order; ``out`` may give both."""
    return _topk_sets(False, rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, k, set_ptr, set_rows, qset_ptr_head,
                      qset_ptr_tail, filter, row_base, out)


def topk_sets_wide_supported(rel_model, dim, k, dtype=torch.float32):
    """True if topk_sets_wide takes this width, k and table dtype (blp_topk_sets_wide_supported: transe, D % 4 == 0,
    4 <= D <= 1024 -- the BOW / DKRL encoders' 300 and 768 --, 1 <= k <= 256; a float32, float16 or bfloat16 table)."""
    if dtype not in TABLE_DTYPES:
        return False
    return bool(_lib.lib().blp_topk_sets_wide_supported(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(dim), int(k)))


def topk_sets_wide_workspace_bytes(rel_model, D, q_head, q_tail, num_sets, nnz, k, dtype=torch.float32):
    """Bytes of topk_sets_wide's workspace: coefficient rows, num_sets + 1 unit offsets and the partial lists -- never a function
    of the table's length or its storage type (0: not supported, or a negative size)."""
    if dtype not in TABLE_DTYPES:
        return 0
    return int(_lib.lib().blp_topk_sets_wide_workspace_bytes(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(D), int(q_head),
                                                            int(q_tail), int(num_sets), int(nnz), int(k)))


def topk_sets_wide(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, k, set_ptr, set_rows, qset_ptr_head, qset_ptr_tail,
                   filter=None, row_base=0, out=None):
    """topk_sets for TransE at any width D % 4 == 0, 4 <= D <= 1024 (blp_topk_sets_wide: a lane holds 64 columns of its set row at
    a time and the running sums of a chunk of up to 16 queries of the set's group; the winners' scores come straight from the
    selection keys): same arguments, same rows and scores -- the reference's bit for bit, on a 16-bit table those of the table
    widened to float32."""
    return _topk_sets(True, rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, k, set_ptr, set_rows, qset_ptr_head,
                      qset_ptr_tail, filter, row_base, out)


def _topk_sets(wide, rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, k, set_ptr, set_rows, qset_ptr_head, qset_ptr_tail,
               filter, row_base, out):
    """topk_sets (blp_topk_sets_typed) and topk_sets_wide (blp_topk_sets_wide): one argument handling, two entries."""
    who = "topk_sets_wide" if wide else "topk_sets"
    _require_device(table, source, fixed_row, rel_emb, rel_ids, set_ptr, set_rows, qset_ptr_head, qset_ptr_tail)
    if table.dtype not in TABLE_DTYPES:
        raise TypeError(f"{who} reads a float32, float16 or bfloat16 table, got {table.dtype}")
    if source.dtype != torch.float32:
        raise TypeError(f"{who} needs a float32 `source` for the queries' vectors, got {source.dtype}")
    same = source is table
    table = _table_rows(table, "table")
    source = table if same else _f32_rows(source, "source")
    rel_emb = _f32_rows(rel_emb, "rel_emb").contiguous()
    N, D = table.shape
    if source.dim() != 2 or source.shape[1] != D:
        raise ValueError(f"source must be (S, {D}), got {tuple(source.shape)}")
    fixed_row, rel_ids = _i64_vector(fixed_row), _i64_vector(rel_ids)
    set_ptr, set_rows = _i64_vector(set_ptr), _i64_vector(set_rows)
    qset_ptr_head, qset_ptr_tail = _i64_vector(qset_ptr_head), _i64_vector(qset_ptr_tail)
    Q, nnz, G = fixed_row.shape[0], set_rows.shape[0], set_ptr.shape[0] - 1
    k = int(k)
    if rel_ids.shape[0] != Q or rel_emb.dim() != 2 or rel_emb.shape[1] != D:
        raise ValueError("fixed_row and rel_ids need one entry per query; rel_emb must be (R, D)")
    if G < 0 or qset_ptr_head.shape[0] != G + 1 or qset_ptr_tail.shape[0] != G + 1:
        raise ValueError("set_ptr, qset_ptr_head and qset_ptr_tail need G + 1 entries each")
    if not 0 <= q_head <= Q:
        raise ValueError(f"q_head = {q_head} outside [0, {Q}]")
    if wide and not topk_sets_wide_supported(rel_model, D, k, table.dtype):
        raise ValueError(f"topk_sets_wide: {rel_model} at D = {D}, k = {k} not supported (transe, D % 4 == 0, 4 <= D <= 1024, "
                         "1 <= k <= 256): see topk_sets_wide_supported")
    if not wide and not topk_sets_supported(rel_model, D, k, table.dtype):
        raise ValueError(f"topk_sets: D = {D}, k = {k} not supported (D in 64 / 128 / 256, 1 <= k <= 256): see topk_sets_supported")
    if filter is not None and int(filter.row_base) != int(row_base):
        raise ValueError(f"{who}: the filter's row_base {filter.row_base} differs from row_base {row_base}")
    dev = table.device
    if out is None:
        out = (torch.empty((Q, k), dtype=torch.int64, device=dev), torch.empty((Q, k), dtype=torch.float32, device=dev))
    rows, scores = out
    if rows.shape != (Q, k) or rows.dtype != torch.int64 or not rows.is_contiguous() or scores.shape != (Q, k) or \
            scores.dtype != torch.float32 or not scores.is_contiguous():
        raise ValueError("out must be contiguous (Q, k) int64 rows and (Q, k) float32 scores")
    if Q == 0:
        return rows, scores
    L = _lib.lib()
    model = _lib.MODEL_IDS[rel_model]
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    tdt = TABLE_DTYPES[table.dtype]
    ws_bytes = (L.blp_topk_sets_wide_workspace_bytes if wide else L.blp_topk_sets_typed_workspace_bytes)(model, tdt, D, q_head, Q - q_head, G, nnz, k)
    workspace = _workspace(dev, stream, ws_bytes)
    spec = None if filter is None else _filter_spec(filter, Q, dev)
    status = (L.blp_topk_sets_wide if wide else L.blp_topk_sets_typed)(model, table.data_ptr(), tdt, N, D, table.stride(0) if tdt or N > 1 else D, int(row_base),
                                   source.data_ptr(), source.shape[0], source.stride(0) if source.shape[0] > 1 else D,
                                   fixed_row.data_ptr(), rel_emb.data_ptr(), rel_emb.shape[0], rel_ids.data_ptr(), q_head, Q - q_head, k,
                                   set_ptr.data_ptr(), _addr(set_rows) if nnz else None, nnz, G, qset_ptr_head.data_ptr(),
                                   qset_ptr_tail.data_ptr(), spec, rows.data_ptr(), scores.data_ptr(), workspace.data_ptr(), ws_bytes,
                                   dev.index, stream)
    if status:
        _lib.check(status, "blp_topk_sets_wide" if wide else "blp_topk_sets_typed" if tdt else "blp_topk_sets")
    return rows, scores


def topk_lists_supported(rel_model, dim, k, dtype=torch.float32):
    """True if topk_lists takes this width, k and table dtype (include/blp_hip.h: blp_topk_lists_supported -- rank_lists'
    widths: TransE at any D % 4 == 0 up to 1024, the other models at 64 / 128 / 256; 1 <= k <= 256; a float32, float16 or
    bfloat16 table)."""
    if dtype not in TABLE_DTYPES:
        return False
    return bool(_lib.lib().blp_topk_lists_supported(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(dim), int(k)))


def topk_lists_workspace_bytes(rel_model, D, q_head, q_tail, nnz, k, dtype=torch.float32):
    """Bytes of topk_lists' workspace: 0 while every list is one slab (2 048 queries or more, or short lists), else the
    (Q, S, k) partial key lists -- never a function of the table's length or storage type."""
    if dtype not in TABLE_DTYPES:
        return 0
    return int(_lib.lib().blp_topk_lists_workspace_bytes(_lib.MODEL_IDS[rel_model], TABLE_DTYPES[dtype], int(D), int(q_head),
                                                         int(q_tail), int(nnz), int(k)))


def topk_lists(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, list_ptr, list_row, k, filter=None, row_base=0,
               out=None):
    """Filtered top-k prediction inside per-query candidate lists (blp_topk_lists).  Queries, table and lists as in rank_lists
    -- head-replacing [0, q_head), then tail-replacing; fixed_row (Q,) indexes ``source`` (S, D) float32, rel_ids (Q,) index
    ``rel_emb`` (R, D); query q owns entries [list_ptr[q], list_ptr[q + 1]) of ``list_row`` (nnz,) int64 GLOBAL rows of
    ``table`` (N, D) (float32 / float16 / bfloat16; a 16-bit table needs a float32 ``source``: the result is that of the table
    widened to float32), which holds global rows [row_base, row_base + N); entries outside are skipped.  The output is topk's,
    taken over the query's list: the k entries with the highest score_fn value (descending score, ties by ascending row, NaN
    last), the rows ``filter`` (a SegmentFilter whose row_base is ``row_base``) names removed; a list is a multiset: a row
    listed twice may come back twice; slots beyond the entries left: row -1, score NaN.
    Returns (rows (Q, k) int64, scores (Q, k) float32); ``out`` may give both."""
    _require_device(table, source, fixed_row, rel_emb, rel_ids, list_ptr, list_row)
    if table.dtype not in TABLE_DTYPES:
        raise TypeError(f"topk_lists reads a float32, float16 or bfloat16 table, got {table.dtype}")
    if source.dtype != torch.float32:
        raise TypeError(f"topk_lists needs a float32 `source` for the queries' vectors, got {source.dtype}")
    same = source is table
    table = _table_rows(table, "table")
    source = table if same else _f32_rows(source, "source")
    rel_emb = _f32_rows(rel_emb, "rel_emb").contiguous()
    N, D = table.shape
    if source.dim() != 2 or source.shape[1] != D:
        raise ValueError(f"source must be (S, {D}), got {tuple(source.shape)}")
    fixed_row, rel_ids, list_ptr, list_row = _i64_vector(fixed_row), _i64_vector(rel_ids), _i64_vector(list_ptr), _i64_vector(list_row)
    Q, nnz = fixed_row.shape[0], list_row.shape[0]
    k = int(k)
    if rel_ids.shape[0] != Q or list_ptr.shape[0] != Q + 1 or rel_emb.dim() != 2 or rel_emb.shape[1] != D:
        raise ValueError("fixed_row and rel_ids need one entry per query, list_ptr Q + 1; rel_emb must be (R, D)")
    if not 0 <= q_head <= Q:
        raise ValueError(f"q_head = {q_head} outside [0, {Q}]")
    if not topk_lists_supported(rel_model, D, k, table.dtype):
        raise ValueError(f"topk_lists: D = {D}, k = {k} not supported for {rel_model} (1 <= k <= 256: see topk_lists_supported)")
    if filter is not None and int(filter.row_base) != int(row_base):
        raise ValueError(f"topk_lists: the filter's row_base {filter.row_base} differs from row_base {row_base}")
    dev = table.device
    if out is None:
        out = (torch.empty((Q, k), dtype=torch.int64, device=dev), torch.empty((Q, k), dtype=torch.float32, device=dev))
    rows, scores = out
    if rows.shape != (Q, k) or rows.dtype != torch.int64 or not rows.is_contiguous() or scores.shape != (Q, k) or \
            scores.dtype != torch.float32 or not scores.is_contiguous():
        raise ValueError("out must be contiguous (Q, k) int64 rows and (Q, k) float32 scores")
    if Q == 0:
        return rows, scores
    L = _lib.lib()
    model = _lib.MODEL_IDS[rel_model]
    tdt = TABLE_DTYPES[table.dtype]
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    ws_bytes = L.blp_topk_lists_workspace_bytes(model, tdt, D, q_head, Q - q_head, nnz, k)
    workspace = _workspace(dev, stream, ws_bytes) if ws_bytes else None
    spec = None if filter is None else _filter_spec(filter, Q, dev)
    status = L.blp_topk_lists(model, table.data_ptr(), tdt, N, D, table.stride(0) if tdt or N > 1 else D, int(row_base),
                              source.data_ptr(), source.shape[0], source.stride(0) if source.shape[0] > 1 else D, fixed_row.data_ptr(),
                              rel_emb.data_ptr(), rel_emb.shape[0], rel_ids.data_ptr(), q_head, Q - q_head, list_ptr.data_ptr(),
                              _addr(list_row) if nnz else None, nnz, k, spec, rows.data_ptr(), scores.data_ptr(), _addr(workspace),
                              ws_bytes, dev.index, stream)
    if status:
        _lib.check(status, "blp_topk_lists")
    return rows, scores


def rank_relations_supported(rel_model, dim):
    """True if rank_relations takes this width (include/blp_hip.h: blp_rank_relations_supported -- the four models at 64 / 128 /
    256)."""
    return bool(_lib.lib().blp_rank_relations_supported(_lib.MODEL_IDS[rel_model], int(dim)))


def rank_relations_workspace_bytes(rel_model, D, Q, R):
    """Bytes of rank_relations' workspace: the Q true-relation scores (4 Q rounded up to 256), whatever R."""
    return int(_lib.lib().blp_rank_relations_workspace_bytes(_lib.MODEL_IDS[rel_model], int(D), int(Q), int(R)))


def topk_relations_supported(rel_model, dim, k):
    """True if topk_relations takes this width and k (rank_relations' widths, 1 <= k <= 256)."""
    return bool(_lib.lib().blp_topk_relations_supported(_lib.MODEL_IDS[rel_model], int(dim), int(k)))


def topk_relations_workspace_bytes(rel_model, D, Q, R, k):
    """Bytes of topk_relations' workspace: 0 (the lists live on chip, every query has one owner)."""
    return int(_lib.lib().blp_topk_relations_workspace_bytes(_lib.MODEL_IDS[rel_model], int(D), int(Q), int(R), int(k)))


def _relation_queries(source, head_row, tail_row, rel_emb, who):
    _require_device(source, head_row, tail_row, rel_emb)
    if source.dtype != torch.float32:
        raise TypeError(f"{who} needs a float32 `source` for the queries' vectors, got {source.dtype} (gather and widen a 16-bit "
                        "table's rows with gather_triple_vectors)")
    source = _f32_rows(source, "source")
    rel_emb = _f32_rows(rel_emb, "rel_emb").contiguous()
    if source.dim() != 2 or rel_emb.dim() != 2 or rel_emb.shape[1] != source.shape[1] or rel_emb.shape[0] < 1:
        raise ValueError(f"source must be (S, D) and rel_emb (R >= 1, D), got {tuple(source.shape)} and {tuple(rel_emb.shape)}")
    head_row, tail_row = _i64_vector(head_row), _i64_vector(tail_row)
    if head_row.shape[0] != tail_row.shape[0]:
        raise ValueError("head_row and tail_row need one entry per query")
    return source, head_row, tail_row, rel_emb


_RELATION_ROUTES = {"": "64 / 128 / 256", "_wide": "transe, D % 4 == 0, 4 <= D <= 1024",
                    "_wide_bilinear": "distmult / complex / simple, D % 4 == 0, 4 <= D <= 1024"}  # entry suffix -> what it takes


def _rank_relations(route, rel_model, source, head_row, tail_row, rel_emb, true_rel, filter, return_scores, out):
    """rank_relations (blp_rank_relations), rank_relations_wide (blp_rank_relations_wide) and rank_relations_wide_bilinear
    (blp_rank_relations_wide_bilinear): one argument handling, three entries (``route``: the entry's suffix)."""
    who = "rank_relations" + route
    source, head_row, tail_row, rel_emb = _relation_queries(source, head_row, tail_row, rel_emb, who)
    _require_device(true_rel)
    Q, (R, D) = head_row.shape[0], rel_emb.shape
    if true_rel is None and not return_scores:
        raise ValueError(f"{who}: give true_rel (counts), return_scores=True, or both")
    if not getattr(_lib.lib(), f"blp_{who}_supported")(_lib.MODEL_IDS[rel_model], int(D)):
        raise ValueError(f"{who}: D = {D} not supported for {rel_model} ({_RELATION_ROUTES[route]}: see {who}_supported)")
    if filter is not None and (filter.ent2idx is not None or int(filter.row_base) != 0):
        raise ValueError(f"{who}: the filter's values are relation ids (ent2idx None, row_base 0)")
    dev = source.device
    counts = scores = None
    if true_rel is not None:
        true_rel = _i64_vector(true_rel)
        if true_rel.shape[0] != Q:
            raise ValueError("true_rel needs one entry per query")
        counts = torch.empty((Q, 4), dtype=torch.int32, device=dev) if out is None else out
        if counts.shape != (Q, 4) or counts.dtype != torch.int32 or not counts.is_contiguous():
            raise ValueError("out must be a contiguous (Q, 4) int32 tensor")
    if return_scores:
        scores = torch.empty((Q, R), dtype=torch.float32, device=dev)
    if Q:
        L = _lib.lib()
        entry = "blp_" + who
        model = _lib.MODEL_IDS[rel_model]
        stream = torch._C._cuda_getCurrentRawStream(dev.index)
        ws_bytes = getattr(L, entry + "_workspace_bytes")(model, D, Q, R) if counts is not None else 0
        workspace = _workspace(dev, stream, ws_bytes) if ws_bytes else None
        spec = None if filter is None else _filter_spec(filter, Q, dev)
        status = getattr(L, entry)(model, source.data_ptr(), source.shape[0], D, source.stride(0) if source.shape[0] > 1 else D,
                                   head_row.data_ptr(), tail_row.data_ptr(), Q, rel_emb.data_ptr(), R, _addr(true_rel), spec,
                                   _addr(counts), _addr(scores), R, _addr(workspace), ws_bytes, dev.index, stream)
        if status:
            _lib.check(status, entry)
    if counts is None:
        return scores
    return (counts, scores) if return_scores else counts


def _topk_relations(route, rel_model, source, head_row, tail_row, rel_emb, k, filter, out):
    """topk_relations (blp_topk_relations), topk_relations_wide (blp_topk_relations_wide) and topk_relations_wide_bilinear
    (blp_topk_relations_wide_bilinear)."""
    who = "topk_relations" + route
    source, head_row, tail_row, rel_emb = _relation_queries(source, head_row, tail_row, rel_emb, who)
    Q, (R, D) = head_row.shape[0], rel_emb.shape
    k = int(k)
    if not getattr(_lib.lib(), f"blp_{who}_supported")(_lib.MODEL_IDS[rel_model], int(D), k):
        raise ValueError(f"{who}: D = {D}, k = {k} not supported for {rel_model} ({_RELATION_ROUTES[route]}, 1 <= k <= 256)")
    if filter is not None and (filter.ent2idx is not None or int(filter.row_base) != 0):
        raise ValueError(f"{who}: the filter's values are relation ids (ent2idx None, row_base 0)")
    dev = source.device
    if out is None:
        out = (torch.empty((Q, k), dtype=torch.int64, device=dev), torch.empty((Q, k), dtype=torch.float32, device=dev))
    rels, scores = out
    if rels.shape != (Q, k) or rels.dtype != torch.int64 or not rels.is_contiguous() or scores.shape != (Q, k) or \
            scores.dtype != torch.float32 or not scores.is_contiguous():
        raise ValueError("out must be contiguous (Q, k) int64 relation ids and (Q, k) float32 scores")
    if Q == 0:
        return rels, scores
    L = _lib.lib()
    entry = "blp_" + who
    model = _lib.MODEL_IDS[rel_model]
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    ws_bytes = getattr(L, entry + "_workspace_bytes")(model, D, Q, R, k)
    workspace = _workspace(dev, stream, ws_bytes) if ws_bytes else None
    spec = None if filter is None else _filter_spec(filter, Q, dev)
    status = getattr(L, entry)(model, source.data_ptr(), source.shape[0], D, source.stride(0) if source.shape[0] > 1 else D,
                               head_row.data_ptr(), tail_row.data_ptr(), Q, rel_emb.data_ptr(), R, k, spec, rels.data_ptr(),
                               scores.data_ptr(), _addr(workspace), ws_bytes, dev.index, stream)
    if status:
        _lib.check(status, entry)
    return rels, scores


def rank_relations(rel_model, source, head_row, tail_row, rel_emb, true_rel=None, filter=None, return_scores=False, out=None):
    """Relation prediction, ranking form (blp_rank_relations): query q is the pair (row head_row[q], row tail_row[q]) of ``source``
    (S, D) float32; the candidates are all R rows of ``rel_emb``.  With ``true_rel`` (Q,): counts (Q, 4) int32 = {gt, ge, gt_filt,
    ge_filt}, the relations that score above / at least the true one, the last two without those ``filter`` (a SegmentFilter
    whose values are RELATION ids: no ent2idx, row_base 0; ``exclude`` is never removed) names.  ``return_scores``: the (Q, R)
    score matrix, score_fn's values bit for bit.  Returns counts, scores, or (counts, scores); ``out`` may give counts."""
    return _rank_relations("", rel_model, source, head_row, tail_row, rel_emb, true_rel, filter, return_scores, out)


def topk_relations(rel_model, source, head_row, tail_row, rel_emb, k, filter=None, out=None):
    """Relation prediction, answer form (blp_topk_relations): per pair (row head_row[q], row tail_row[q]) of ``source`` the k
    relations with the highest score_fn value in topk's order (descending score, ties by ascending relation id, NaN last), the
    relations ``filter`` names removed (a SegmentFilter of relation ids, as in rank_relations); slots beyond the relations left
    (k > R, a filter that leaves fewer): -1, score NaN.  Returns (rels (Q, k) int64, scores (Q, k) float32); ``out`` may give
    both."""
    return _topk_relations("", rel_model, source, head_row, tail_row, rel_emb, k, filter, out)


def rank_relations_wide_supported(rel_model, dim):
    """True if rank_relations_wide takes this width (blp_rank_relations_wide_supported: transe, D % 4 == 0, 4 <= D <= 1024 -- the
    BOW / DKRL encoders' 300 and 768 among them)."""
    return bool(_lib.lib().blp_rank_relations_wide_supported(_lib.MODEL_IDS[rel_model], int(dim)))


def rank_relations_wide_workspace_bytes(rel_model, D, Q, R):
    """Bytes of rank_relations_wide's workspace: the Q true-relation scores (4 Q rounded up to 256), whatever R and D."""
    return int(_lib.lib().blp_rank_relations_wide_workspace_bytes(_lib.MODEL_IDS[rel_model], int(D), int(Q), int(R)))


def topk_relations_wide_supported(rel_model, dim, k):
    """True if topk_relations_wide takes this width and k (rank_relations_wide's widths, 1 <= k <= 256)."""
    return bool(_lib.lib().blp_topk_relations_wide_supported(_lib.MODEL_IDS[rel_model], int(dim), int(k)))


def topk_relations_wide_workspace_bytes(rel_model, D, Q, R, k):
    """Bytes of topk_relations_wide's workspace: 0 (the lists live on chip, every query has one owner)."""
    return int(_lib.lib().blp_topk_relations_wide_workspace_bytes(_lib.MODEL_IDS[rel_model], int(D), int(Q), int(R), int(k)))


def rank_relations_wide(rel_model, source, head_row, tail_row, rel_emb, true_rel=None, filter=None, return_scores=False, out=None):
    """rank_relations for TransE at any width D % 4 == 0, 4 <= D <= 1024 (blp_rank_relations_wide: a lane holds 64 columns of
    its relation row at a time and carries the running sums): the same arguments, the same counts and score bits."""
    return _rank_relations("_wide", rel_model, source, head_row, tail_row, rel_emb, true_rel, filter, return_scores, out)


def topk_relations_wide(rel_model, source, head_row, tail_row, rel_emb, k, filter=None, out=None):
    """topk_relations for TransE at any width D % 4 == 0, 4 <= D <= 1024 (blp_topk_relations_wide): the same arguments, order,
    padding and score bits."""
    return _topk_relations("_wide", rel_model, source, head_row, tail_row, rel_emb, k, filter, out)


def rank_relations_wide_bilinear_supported(rel_model, dim):
    """True if rank_relations_wide_bilinear takes this width (blp_rank_relations_wide_bilinear_supported: distmult / complex /
    simple, D % 4 == 0, 4 <= D <= 1024 -- the BOW / DKRL encoders' 300 and 768 among them)."""
    return bool(_lib.lib().blp_rank_relations_wide_bilinear_supported(_lib.MODEL_IDS[rel_model], int(dim)))


def rank_relations_wide_bilinear_workspace_bytes(rel_model, D, Q, R):
    """Bytes of rank_relations_wide_bilinear's workspace: the Q true-relation keys (4 Q rounded up to 256), whatever R and D."""
    return int(_lib.lib().blp_rank_relations_wide_bilinear_workspace_bytes(_lib.MODEL_IDS[rel_model], int(D), int(Q), int(R)))


def topk_relations_wide_bilinear_supported(rel_model, dim, k):
    """True if topk_relations_wide_bilinear takes this width and k (rank_relations_wide_bilinear's widths, 1 <= k <= 256)."""
    return bool(_lib.lib().blp_topk_relations_wide_bilinear_supported(_lib.MODEL_IDS[rel_model], int(dim), int(k)))


def topk_relations_wide_bilinear_workspace_bytes(rel_model, D, Q, R, k):
    """Bytes of topk_relations_wide_bilinear's workspace: 0 (the lists live on chip, every query has one owner)."""
    return int(_lib.lib().blp_topk_relations_wide_bilinear_workspace_bytes(_lib.MODEL_IDS[rel_model], int(D), int(Q), int(R), int(k)))


def rank_relations_wide_bilinear(rel_model, source, head_row, tail_row, rel_emb, true_rel=None, filter=None, return_scores=False,
                                 out=None):
    """rank_relations for DistMult / ComplEx / SimplE at any width D % 4 == 0, 4 <= D <= 1024 (blp_rank_relations_wide_bilinear:
    eight lanes per relation row restate torch's sum order, eight pairs per workgroup pass): the same arguments, the same counts
    and score bits."""
    return _rank_relations("_wide_bilinear", rel_model, source, head_row, tail_row, rel_emb, true_rel, filter, return_scores, out)


def topk_relations_wide_bilinear(rel_model, source, head_row, tail_row, rel_emb, k, filter=None, out=None):
    """topk_relations for DistMult / ComplEx / SimplE at any width D % 4 == 0, 4 <= D <= 1024 (blp_topk_relations_wide_bilinear):
    the same arguments, order, padding and score bits."""
    return _topk_relations("_wide_bilinear", rel_model, source, head_row, tail_row, rel_emb, k, filter, out)


def topk_merge(rows, scores, k):
    """The k best of per-query candidate lists (blp_topk_merge): rows (Q, n) int64 global rows (< 0: an empty slot) and
    scores (Q, n) float32 -- e.g. the topk results of several candidate shards side by side -- in topk's order.
    Returns (rows (Q, k), scores (Q, k))."""
    _require_device(rows, scores)
    if rows.dim() != 2 or scores.shape != rows.shape:
        raise ValueError("rows and scores must be (Q, n) of the same shape")
    rows = rows.to(torch.int64).contiguous()
    scores = _f32_rows(scores, "scores").contiguous()
    Q, n = rows.shape
    k = int(k)
    if not 1 <= k <= 256 or n < 1:
        raise ValueError(f"topk_merge: k = {k} outside [1, 256] or empty lists")
    dev = rows.device
    rows_out = torch.empty((Q, k), dtype=torch.int64, device=dev)
    scores_out = torch.empty((Q, k), dtype=torch.float32, device=dev)
    if Q == 0:
        return rows_out, scores_out
    status = _lib.lib().blp_topk_merge(rows.data_ptr(), scores.data_ptr(), Q, 1, n, k, rows_out.data_ptr(), scores_out.data_ptr(),
                                       dev.index, torch._C._cuda_getCurrentRawStream(dev.index))
    if status:
        _lib.check(status, "blp_topk_merge")
    return rows_out, scores_out


def rerank_supported(max_segment, dim):
    """True if rerank_cosine / rerank_ndcg take segments of ``max_segment`` candidates and width ``dim``
    (include/blp_hip.h: blp_rerank_supported)."""
    return bool(_lib.lib().blp_rerank_supported(int(max_segment), int(dim)))


def _i64_flat(t):
    return t.reshape(-1).to(torch.int64).contiguous()


def rerank_cosine(table, queries, cand_ptr, cand_row, out=None):
    """blp_rerank_cosine: s1 (C,) float32 = F.normalize(table[cand_row[c]]) . F.normalize(queries[q]) for the candidates c of
    query q ([cand_ptr[q], cand_ptr[q + 1])), 0.0 where cand_row is -1 (retrieval.py:170-175; the summation order is
    blp_amd.retrieval.cosine_restated's)."""
    _require_device(table, queries, cand_ptr, cand_row, out)
    table = _f32_rows(table, "table")
    queries = _f32_rows(queries, "queries")
    if table.dim() != 2 or queries.dim() != 2 or queries.shape[1] != table.shape[1]:
        raise ValueError(f"table (E, D) and queries (Q, D) of the same width, got {tuple(table.shape)} / {tuple(queries.shape)}")
    E, D = table.shape
    Q = queries.shape[0]
    cand_ptr = _i64_flat(cand_ptr)
    cand_row = cand_row.reshape(-1).to(torch.int32).contiguous()
    C = cand_row.shape[0]
    if cand_ptr.shape[0] != Q + 1:
        raise ValueError(f"cand_ptr must hold Q + 1 = {Q + 1} offsets, got {cand_ptr.shape[0]}")
    dev = table.device
    if out is None:
        out = torch.empty(C, dtype=torch.float32, device=dev)
    if out.shape != (C,) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous (C,) float32 tensor")
    status = _lib.lib().blp_rerank_cosine(_addr(table), E, D, table.stride(0) if E > 1 else D, _addr(queries), Q,
                                          queries.stride(0) if Q > 1 else D, _addr(cand_ptr), _addr(cand_row), C, _addr(out),
                                          dev.index, _stream(dev))
    _lib.check(status, "blp_rerank_cosine")
    return out


def rerank_ndcg(s1, s2, gain, cand_ptr, alphas, cutoffs, log2_table, idcg, max_segment=None, out=None):
    """blp_rerank_ndcg: (A, Q, len(cutoffs)) float64, trec_eval's ndcg_cut of the run alpha * s1 + (1 - alpha) * s2 for every
    alpha and query (each segment ordered by docno descending).  ``cutoffs`` is a host sequence; ``max_segment``
    bounds the segment lengths (None: read from cand_ptr, one host synchronisation)."""
    _require_device(s1, s2, gain, cand_ptr, alphas, log2_table, idcg, out)
    dev = s1.device
    s1 = s1.reshape(-1).to(torch.float32).contiguous()
    s2 = s2.reshape(-1).to(torch.float64).contiguous()
    gain = gain.reshape(-1).to(torch.int32).contiguous()
    cand_ptr = _i64_flat(cand_ptr)
    alphas = alphas.reshape(-1).to(torch.float64).contiguous()
    log2_table = log2_table.reshape(-1).to(torch.float64).contiguous()
    cutoffs = [int(k) for k in cutoffs]
    Q, C, A, n_cut = cand_ptr.shape[0] - 1, s1.shape[0], alphas.shape[0], len(cutoffs)
    if Q < 0 or s2.shape[0] != C or gain.shape[0] != C:
        raise ValueError("s1, s2 and gain need one entry per candidate; cand_ptr Q + 1 offsets")
    idcg = idcg.to(torch.float64).contiguous()
    if idcg.shape != (Q, n_cut):
        raise ValueError(f"idcg must be (Q, n_cut) = ({Q}, {n_cut}), got {tuple(idcg.shape)}")
    if max_segment is None:
        max_segment = int((cand_ptr[1:] - cand_ptr[:-1]).max()) if Q > 0 else 0
    if out is None:
        out = torch.empty((A, Q, n_cut), dtype=torch.float64, device=dev)
    if out.shape != (A, Q, n_cut) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError("out must be a contiguous (A, Q, n_cut) float64 tensor")
    k = (ctypes.c_int32 * max(1, n_cut))(*cutoffs)
    status = _lib.lib().blp_rerank_ndcg(_addr(s1), _addr(s2), _addr(gain), _addr(cand_ptr), Q, C, int(max_segment), _addr(alphas),
                                        A, k, n_cut, _addr(log2_table), log2_table.shape[0], _addr(idcg), _addr(out), dev.index,
                                        _stream(dev))
    _lib.check(status, "blp_rerank_ndcg")
    return out


def rank_all_batches(rel_model, table, fixed_row, rel_emb, rel_ids, true_row, num_triples, batch, filter=None, out=None, source=None,
                     block_triples=0):
    """Every batch of the reference's evaluation loop in ONE call (blp_rank_all_batches): fixed_row / rel_ids / true_row
    (2 num_triples,), a SegmentFilter's seg_lo / seg_hi / exclude and the returned counts (2 num_triples, 4) are laid out
    batch after batch of ``batch`` triples, each batch as [its head queries | its tail queries] -- build_queries'
    layout with block_size = batch, i.e. what a loop over the reference's DataLoader sees.  Same counts as one
    rank_all_idx call per batch; the library ranks ``block_triples`` triples at a time (0: 65 536; <= batch: one pass per
    batch, the reference's own pass structure, issued back to back by the library)."""
    source = table if source is None else source
    _require_device(table, source, fixed_row, rel_emb, rel_ids, true_row)
    # (a 16-bit table -- float16 / bfloat16 --: the candidates only; `source`, the queries' own
    #  vectors, is float32: gather_triple_vectors widens them)
    table, rel_emb = _table_rows(table, "table"), _f32_rows(rel_emb, "rel_emb").contiguous()
    if source is table and table.dtype != torch.float32:
        raise TypeError("a 16-bit table needs a float32 `source` for the queries' vectors (ops.gather_triple_vectors + build_queries(by_position=True))")
    source = table if source is table else _f32_rows(source, "source")
    N, D = table.shape
    tdt = TABLE_DTYPES[table.dtype]
    ld = table.stride(0) if tdt or N > 1 else D
    n, Q = int(num_triples), 2 * int(num_triples)
    fixed_row, rel_ids, true_row = _i64_vector(fixed_row), _i64_vector(rel_ids), _i64_vector(true_row)
    if fixed_row.shape[0] != Q or rel_ids.shape[0] != Q or true_row.shape[0] != Q or rel_emb.shape[1] != D or source.shape[1] != D:
        raise ValueError("fixed_row, rel_ids, true_row need 2 * num_triples entries; rel_emb / source must be (., D)")
    dev = table.device
    counts = out if out is not None else torch.empty((Q, 4), dtype=torch.int32, device=dev)
    if counts.shape != (Q, 4) or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError("out must be a contiguous (2 * num_triples, 4) int32 tensor")
    if Q == 0:
        return counts
    ensure_selftest(dev, rel_model)
    L = _lib.lib()
    model = _lib.MODEL_IDS[rel_model]
    ws_bytes = L.blp_rank_all_batches_workspace_bytes(model, tdt, N, D, ld, n, int(batch), int(block_triples))
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    workspace = _workspace(dev, stream, ws_bytes)
    spec = None if filter is None else _filter_spec(filter, Q, dev)
    status = L.blp_rank_all_batches(model, table.data_ptr(), tdt, N, D, ld, source.data_ptr(), source.shape[0],
                                      source.stride(0) if source.shape[0] > 1 else D, fixed_row.data_ptr(), rel_emb.data_ptr(), rel_emb.shape[0],
                                      rel_ids.data_ptr(), true_row.data_ptr(), n, int(batch), int(block_triples), spec, counts.data_ptr(),
                                      workspace.data_ptr(), ws_bytes, dev.index, stream)
    if status:
        _lib.check(status, "blp_rank_all_batches")
    return counts


def gather_triple_vectors(triples, ent2idx, table, row_base=0):
    """(2n, D) f32: row t = the vector of triple t's head, row n + t = of its tail (train.py:141-142 for the whole set),
    for the entities whose global row ent2idx[id] lies in [row_base, row_base + len(table)); zeros for the others, so
    that ONE all-reduce over the ranks of a candidate-axis shard replicates every vector (blp_gather_triple_vectors)."""
    _require_device(triples, ent2idx, table)
    table = _table_rows(table, "table")  # (float16 / bfloat16 rows come out widened, exactly: the result is float32 always)
    triples = triples.to(torch.int64).contiguous()
    n, (N, D) = triples.shape[0], table.shape
    tdt = TABLE_DTYPES[table.dtype]
    out = torch.empty((2 * n, D), dtype=torch.float32, device=table.device)
    if ent2idx is not None:
        ent2idx = ent2idx.to(torch.int64).contiguous()
    ld = table.stride(0) if tdt or N > 1 else D
    status = _lib.lib().blp_gather_triple_vectors(_ptr(triples), n, _ptr(ent2idx), 0 if ent2idx is None else ent2idx.shape[0],
                                                    _ptr(table), tdt, N, D, ld, int(row_base), _ptr(out),
                                                    table.device.index, _stream(table.device))
    _lib.check(status, "blp_gather_triple_vectors")
    return out


def rank_from_scores(scores, true_idx=None, true_score=None, filt_rowptr=None, filt_col=None):
    """Counts (Q, 4) int32 from a dense (Q, N) score matrix on the device (utils.py:103-105 +
    train.py:159-167): the true entity as column index ``true_idx`` (Q,) or as score ``true_score`` (Q,)."""
    _require_device(scores, true_idx, true_score, filt_rowptr, filt_col)
    if scores.dtype != torch.float32 or scores.dim() != 2:
        raise TypeError("scores must be a 2-D float32 tensor")
    if scores.stride(1) != 1:
        scores = scores.contiguous()
    if (true_idx is None) == (true_score is None):
        raise ValueError("give exactly one of true_idx / true_score")
    Q, N = scores.shape
    dev = scores.device
    if true_idx is not None:
        true_idx = true_idx.reshape(-1).to(torch.int64).contiguous()
    else:
        true_score = true_score.reshape(-1).to(torch.float32).contiguous()
    if filt_rowptr is not None:
        filt_rowptr = filt_rowptr.to(torch.int64).contiguous()
        filt_col = filt_col.to(torch.int64).contiguous()
        if filt_col.numel() == 0:
            filt_col = torch.zeros(1, dtype=torch.int64, device=dev)
    counts = torch.empty((Q, 4), dtype=torch.int32, device=dev)
    status = _lib.lib().blp_rank_from_scores(_ptr(scores), Q, N, scores.stride(0) if Q else N, _ptr(true_idx),
                                             _ptr(true_score), _ptr(filt_rowptr), _ptr(filt_col), _ptr(counts),
                                             dev.index, _stream(dev))
    _lib.check(status, "blp_rank_from_scores")
    return counts


def rank_metrics(counts, k_values=(1, 3, 10)):
    """counts (Q, 4) int32 -> rr (Q, 2) f32 [raw, filtered], hits (Q, 2, 3) bool."""
    _require_device(counts)
    Q = counts.shape[0]
    dev = counts.device
    rr = torch.empty((Q, 2), dtype=torch.float32, device=dev)
    hits = torch.empty((Q, 2, 3), dtype=torch.uint8, device=dev)
    if Q:
        status = _lib.lib().blp_rank_metrics(_ptr(counts.contiguous()), Q, _K_VALUES(*k_values), _ptr(rr),
                                             _ptr(hits), dev.index, _stream(dev))
        _lib.check(status, "blp_rank_metrics")
    return rr, hits.bool()


def rank_metric_sums(counts, k_values=(1, 3, 10)):
    """counts (Q, 4) int32 -> (8,) f64: [sum rr raw, sum rr filtered, hits@k raw x 3, hits@k filtered x 3]
    (train.py:152-157 accumulated on the device, fixed summation order)."""
    _require_device(counts)
    sums = torch.empty(_lib.METRIC_SUMS_DOUBLES, dtype=torch.float64, device=counts.device)  # 8 results + scratch
    status = _lib.lib().blp_rank_metric_sums(_ptr(counts.contiguous()), counts.shape[0], _K_VALUES(*k_values),
                                             _ptr(sums), counts.device.index, _stream(counts.device))
    _lib.check(status, "blp_rank_metric_sums")
    return sums[:8]


# ------------------------------------------------------------------------------- evaluation prelude
QueryBlock = collections.namedtuple("QueryBlock", "q_fixed q_rel fixed_row true_row rel_ids ids_min filter")


def build_queries(triples, ent2idx, table, rel_emb, block_size, index=None, row_base=0, gather=True, by_position=False,
                  num_rows=None):
    """train.py:132-145 (+ utils.py:46-83 with ``index``) for a whole set of triples in one kernel (blp_build_queries).

    triples (n, 3) int64 rows (head id, tail id, relation id) on the table's device; ent2idx: id -> table row (-1: not a
    candidate) or None (ids are rows); table (N, D) f32; rel_emb (R, D) f32 (model.rel_emb.weight); queries come out
    block after block of ``block_size`` triples, each block as [head-replacing | tail-replacing] queries.
    index: a utils.FilterIndex -> ``filter`` is the SegmentFilter of all 2n queries (slice it per block).
    gather=False: no vectors are built (q_fixed = q_rel = None); rank_all_idx takes fixed_row / rel_ids instead.
    by_position: ``table`` is the (2n, D) array of gather_triple_vectors and fixed_row / true_row come out as positions in
    it (head of triple t = t, tail = n + t); ``num_rows`` = rows of the whole entity table (the id check's bound).
    Returns QueryBlock(q_fixed (2n, D), q_rel (2n, D), fixed_row (2n,), true_row (2n,), rel_ids (2n,), ids_min (0-dim
    int32: -1 if any id had no row -- the reference's assertion train.py:137-138, left on the device), filter or
    None)."""
    _require_device(triples, ent2idx, table, rel_emb)
    dev = table.device
    table = _f32_rows(table, "table")
    rel_emb = _f32_rows(rel_emb, "rel_emb").contiguous()
    triples = triples.to(torch.int64).contiguous()
    n, D = triples.shape[0], table.shape[1]
    q_fixed = torch.empty((2 * n, D), dtype=torch.float32, device=dev) if gather else None
    q_rel = torch.empty((2 * n, D), dtype=torch.float32, device=dev) if gather else None
    fixed_row = torch.empty(2 * n, dtype=torch.int64, device=dev)
    true_row = torch.empty(2 * n, dtype=torch.int64, device=dev)
    rel_ids = torch.empty(2 * n, dtype=torch.int64, device=dev)
    ids_min = torch.empty((), dtype=torch.int32, device=dev)
    a = _lib.BlpQueries()
    a.triples, a.n, a.block = triples.data_ptr(), n, int(block_size)
    if ent2idx is not None:
        ent2idx = ent2idx.to(torch.int64).contiguous()
        a.ent2idx, a.ent2idx_len = ent2idx.data_ptr(), ent2idx.shape[0]
    a.source, a.src_rows, a.ld, a.D = table.data_ptr(), table.shape[0], table.stride(0) if table.shape[0] > 1 else D, D
    if by_position:
        if table.shape[0] != 2 * n or num_rows is None:
            raise ValueError("by_position: the source is the (2n, D) array of gather_triple_vectors; give num_rows")
        a.by_position, a.src_rows = 1, int(num_rows)
    a.rel_emb, a.R = rel_emb.data_ptr(), rel_emb.shape[0]
    if gather:
        a.q_fixed, a.q_rel = q_fixed.data_ptr(), q_rel.data_ptr()
    a.fixed_row, a.true_row, a.rel_ids, a.ids_min = fixed_row.data_ptr(), true_row.data_ptr(), rel_ids.data_ptr(), ids_min.data_ptr()
    filt = None
    if index is not None:
        heads_key, tails_key, values, n_head_vals = index.device_arrays(dev)
        seg_lo = torch.empty(2 * n, dtype=torch.int64, device=dev)
        seg_hi = torch.empty_like(seg_lo)
        exclude = torch.empty_like(seg_lo)
        a.heads_key, a.n_heads, a.tails_key, a.n_tails, a.index_R = (heads_key.data_ptr(), heads_key.shape[0],
                                                                     tails_key.data_ptr(), tails_key.shape[0], index.R)
        a.seg_lo, a.seg_hi, a.exclude = seg_lo.data_ptr(), seg_hi.data_ptr(), exclude.data_ptr()
        assert n_head_vals == heads_key.shape[0]
        filt = SegmentFilter(seg_lo, seg_hi, values, exclude, ent2idx, row_base)
    status = _lib.lib().blp_build_queries(ctypes.byref(a), dev.index, _stream(dev))
    _lib.check(status, "blp_build_queries")
    return QueryBlock(q_fixed, q_rel, fixed_row, true_row, rel_ids, ids_min, filt)


# ------------------------------------------------------------------------------- table build epilogue
def project_rows_supported(hidden_size, dim):
    """True if blp_project_rows takes an (n, hidden_size) -> (n, dim) projection."""
    return bool(_lib.lib().blp_project_rows_supported(int(hidden_size), int(dim)))


def project_rows(x, weight, out, normalize):
    """out[i] = x[i] @ weight.T, L2-normalised if ``normalize`` -- enc_linear (models.py:110-111) + F.normalize
    (models.py:40-41) + the row assignment into the entity table (train.py:109-113) in one kernel.  ``x`` (n, E) f32
    may be a strided view (the [CLS] rows of an encoder output), ``out`` (n, D) f32 rows of the table (shard).
    Inference only (no autograd)."""
    _require_device(x, weight, out)
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or out.dtype != torch.float32:
        raise TypeError("project_rows works on float32 tensors")
    if x.dim() != 2 or weight.dim() != 2 or out.dim() != 2 or x.shape[1] != weight.shape[1] or \
            out.shape != (x.shape[0], weight.shape[0]):
        raise ValueError(f"shapes do not match: x {tuple(x.shape)}, weight {tuple(weight.shape)}, out {tuple(out.shape)}")
    if x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16:
        x = x.contiguous()
    if out.stride(1) != 1:
        raise ValueError("out must have contiguous rows")
    weight = weight.contiguous()
    status = _lib.lib().blp_project_rows(_ptr(x), x.shape[0], x.stride(0) if x.shape[0] > 1 else x.shape[1], _ptr(weight),
                                         x.shape[1], weight.shape[0], int(bool(normalize)), _ptr(out),
                                         out.stride(0) if out.shape[0] > 1 else out.shape[1], out.device.index,
                                         _stream(out.device))
    _lib.check(status, "blp_project_rows")
    return out


def bow_rows_supported(embedding_dim):
    """True if blp_bow_rows takes word vectors of this width."""
    return bool(_lib.lib().blp_bow_rows_supported(int(embedding_dim)))


def bow_rows(text_tok, text_mask, weight, out, normalize, bad_flag=None):
    """out[i] = sum_l mask[i, l] * weight[tok[i, l]] / sum_l mask[i, l], L2-normalised if ``normalize`` -- the bag-of-words
    encoder (models.py:143-155) + F.normalize (models.py:40-41) + the row assignment into the entity table
    (train.py:109-113) in one kernel that reads every gathered word vector once (blp_bow_rows).  text_tok (n, L) int64,
    text_mask (n, L) float or None (all ones), weight (V, E) f32 (embeddings.weight), out (n, E) f32 rows of the table.
    Inference only (no autograd).  Token ids outside [0, V) raise IndexError, as nn.Embedding does -- checked after the
    launch with one host read of a flag, or, with ``bad_flag`` (a 0-dim int32 device tensor the caller zeroed once), left to
    the caller: the kernel sets it to -1 and nothing synchronises here (models.BOW.check_tokens reads it after a table build)."""
    _require_device(text_tok, text_mask, weight, out)
    if weight.dtype != torch.float32 or out.dtype != torch.float32:
        raise TypeError("bow_rows works on float32 tables")
    if text_tok.dim() != 2 or weight.dim() != 2 or out.dim() != 2 or out.shape != (text_tok.shape[0], weight.shape[1]):
        raise ValueError(f"shapes do not match: tok {tuple(text_tok.shape)}, weight {tuple(weight.shape)}, out {tuple(out.shape)}")
    if out.stride(1) != 1:
        raise ValueError("out must have contiguous rows")
    tok = text_tok if text_tok.dtype is torch.int64 and text_tok.is_contiguous() else text_tok.to(torch.int64).contiguous()
    mask = None
    if text_mask is not None:
        if text_mask.shape != text_tok.shape:
            raise ValueError("text_mask must have text_tok's shape")
        mask = text_mask if text_mask.dtype is torch.float32 and text_mask.is_contiguous() else text_mask.to(torch.float32).contiguous()
    weight = weight.contiguous()
    n, L = tok.shape
    dev = out.device
    bad = bad_flag if bad_flag is not None else torch.zeros((), dtype=torch.int32, device=dev)
    status = _lib.lib().blp_bow_rows(tok.data_ptr(), _addr(mask), n, L, weight.data_ptr(), weight.shape[0], weight.shape[1],
                                     int(bool(normalize)), out.data_ptr(), out.stride(0) if n > 1 else weight.shape[1],
                                     bad.data_ptr(), dev.index, torch._C._cuda_getCurrentRawStream(dev.index))
    _lib.check(status, "blp_bow_rows")
    if bad_flag is None and bad.item() < 0:
        raise IndexError("bow_rows: a token id is outside the embedding table")
    return out


def dkrl_rows_supported(embedding_dim, dim, num_tokens):
    """True if blp_dkrl_rows takes word vectors of this width, this output width and descriptions of this many tokens."""
    return bool(_lib.lib().blp_dkrl_rows_supported(int(embedding_dim), int(dim), int(num_tokens)))


def dkrl_rows(text_tok, text_mask, weight, conv1, conv2, out, normalize, bad_flag=None):
    """The DKRL encoder (models.py:158-204: lookup, Conv1d(E, dim, 2), mask, max-pool 4, tanh, Conv1d(dim, dim, 2), masked
    mean, tanh) + F.normalize (models.py:40-41) + the row assignment into the entity table (train.py:109-113) in one kernel
    (blp_dkrl_rows).  text_tok (n, L) int64, text_mask (n, L) float or None, weight (V, E) f32 (embeddings.weight), conv1 /
    conv2 the two nn.Conv1d modules (f32), out (n, dim) f32 rows of the table.  Inference only.  bad_flag as for bow_rows."""
    _require_device(text_tok, text_mask, weight, out)
    w1, b1, w2, b2 = conv1.weight, conv1.bias, conv2.weight, conv2.bias
    if any(t.dtype != torch.float32 for t in (weight, w1, b1, w2, b2, out)):
        raise TypeError("dkrl_rows works on float32 tables and weights")
    n, L = text_tok.shape
    dim, E = w1.shape[0], weight.shape[1]
    if w1.shape != (dim, E, 2) or w2.shape != (dim, dim, 2) or out.shape != (n, dim) or out.stride(1) != 1:
        raise ValueError(f"shapes do not match: conv1 {tuple(w1.shape)}, conv2 {tuple(w2.shape)}, weight {tuple(weight.shape)}, out {tuple(out.shape)}")
    tok = text_tok if text_tok.dtype is torch.int64 and text_tok.is_contiguous() else text_tok.to(torch.int64).contiguous()
    mask = None
    if text_mask is not None:
        if text_mask.shape != text_tok.shape:
            raise ValueError("text_mask must have text_tok's shape")
        mask = text_mask if text_mask.dtype is torch.float32 and text_mask.is_contiguous() else text_mask.to(torch.float32).contiguous()
    weight, w1, b1, w2, b2 = weight.contiguous(), w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous()
    dev = out.device
    bad = bad_flag if bad_flag is not None else torch.zeros((), dtype=torch.int32, device=dev)
    status = _lib.lib().blp_dkrl_rows(tok.data_ptr(), _addr(mask), n, L, weight.data_ptr(), weight.shape[0], E, w1.data_ptr(),
                                      b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), dim, int(bool(normalize)), out.data_ptr(),
                                      out.stride(0) if n > 1 else dim, bad.data_ptr(), dev.index,
                                      torch._C._cuda_getCurrentRawStream(dev.index))
    _lib.check(status, "blp_dkrl_rows")
    if bad_flag is None and bad.item() < 0:
        raise IndexError("dkrl_rows: a token id is outside the embedding table")
    return out


# ------------------------------------------------------------------------------------- score_fn
def _collapse(sizes, strides):
    """Collapse a group of dims into (size, stride) or None if not expressible with one stride."""
    size, stride = 1, 0
    for n, st in zip(sizes, strides):
        if n == 1:
            continue
        if size == 1:
            size, stride = n, st
        elif stride == st * n:   # outer stride == inner stride * inner size
            size, stride = size * n, st
        else:
            return None
    return size, stride


def _two_level(shape, operands):
    """Find a split of the broadcast leading shape into (M0, M1) such that every operand's rows are
    base + i0*s0 + i1*s1.  Returns (M0, M1, [(tensor, s0, s1), ...]); copies an operand only if
    its layout cannot be expressed that way."""
    nd = len(shape)
    expanded = [op.expand(*shape, op.shape[-1]) for op in operands]
    for split in range(nd + 1):
        plan = []
        for op in expanded:
            outer = _collapse(shape[:split], op.stride()[:split])
            inner = _collapse(shape[split:], op.stride()[split:nd])
            if outer is None or inner is None:
                plan = None
                break
            plan.append((op, outer[1], inner[1]))
        if plan is not None:
            m0 = 1
            for n in shape[:split]:
                m0 *= n
            m1 = 1
            for n in shape[split:]:
                m1 *= n
            return m0, m1, plan
    total = 1
    for n in shape:
        total *= n
    D = operands[0].shape[-1]
    return total, 1, [(op.contiguous(), D, 0) for op in expanded]


class _ScoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rel_model, heads, tails, rels):
        _require_device(heads, tails, rels)
        D = heads.shape[-1]
        if tails.shape[-1] != D or rels.shape[-1] != D:
            raise ValueError("heads, tails, rels must share the last dimension")
        ops = [_f32_rows(x, n) for x, n in ((heads, "heads"), (tails, "tails"), (rels, "rels"))]
        shape = torch.broadcast_shapes(*(x.shape[:-1] for x in ops))
        m0, m1, plan = _two_level(tuple(shape), ops)
        dev = heads.device
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        (h, hs0, hs1), (t, ts0, ts1), (r, rs0, rs1) = plan
        status = _lib.lib().blp_score_fwd(_lib.MODEL_IDS[rel_model], D, m0, m1, _ptr(h), hs0, hs1,
                                          _ptr(t), ts0, ts1, _ptr(r), rs0, rs1, _ptr(out), dev.index,
                                          _stream(dev))
        _lib.check(status, "blp_score_fwd")
        ctx.rel_model = rel_model
        ctx.shapes = (heads.shape, tails.shape, rels.shape)
        ctx.geometry = (m0, m1, D, tuple(shape))
        ctx.strides = ((hs0, hs1), (ts0, ts1), (rs0, rs1))
        ctx.save_for_backward(h, t, r)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, t, r = ctx.saved_tensors
        m0, m1, D, shape = ctx.geometry
        dev = grad_out.device
        grad_out = grad_out.contiguous()
        need = ctx.needs_input_grad[1:4]
        grads = [torch.empty((*shape, D), dtype=torch.float32, device=dev) if n else None for n in need]
        (hs0, hs1), (ts0, ts1), (rs0, rs1) = ctx.strides
        status = _lib.lib().blp_score_bwd(_lib.MODEL_IDS[ctx.rel_model], D, m0, m1, _ptr(h), hs0, hs1,
                                          _ptr(t), ts0, ts1, _ptr(r), rs0, rs1, _ptr(grad_out),
                                          _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), dev.index,
                                          _stream(dev))
        _lib.check(status, "blp_score_bwd")
        outs = [g.sum_to_size(s) if g is not None else None for g, s in zip(grads, ctx.shapes)]
        return (None, *outs)


def score(rel_model, heads, tails, rels):
    """score_fn(heads, tails, rels) with the reference's broadcasting; bit-identical forward."""
    return _ScoreFn.apply(rel_model, heads, tails, rels)


# --------------------------------------------------------------------------------- in-batch loss
_tickets = {}


def inbatch_ticket(dev, stream):
    """The forward's ticket counter (include/blp_hip.h: BLP_INBATCH_TICKET_INTS int32, zero on entry, left zero by the kernel):
    one per (device, stream), zeroed once -- calls on one stream are ordered and share it."""
    key = (dev.index, stream)
    t = _tickets.get(key)
    if t is None:
        t = _tickets[key] = torch.zeros(_lib.INBATCH_TICKET_INTS, dtype=torch.int32, device=dev)
    return t


class _InBatchLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rel_model, loss_fn, regularizer, ent_embs, rel_vecs, neg_idx):
        _require_device(ent_embs, rel_vecs, neg_idx)
        if ent_embs.dim() != 3 or ent_embs.shape[1] != 2:
            raise ValueError(f"ent_embs must be (B, 2, D), got {tuple(ent_embs.shape)}")
        B, _, D = ent_embs.shape
        if neg_idx.dim() != 3 or neg_idx.shape[0] != B or neg_idx.shape[2] != 2:
            raise ValueError(f"neg_idx must be (B, K, 2), got {tuple(neg_idx.shape)}")
        K = neg_idx.shape[1]
        names = {getattr(torch, n): i for i, n in enumerate(_lib.DTYPE_NAMES)}
        if ent_embs.dtype not in names or rel_vecs.dtype not in (ent_embs.dtype, torch.float32):
            raise TypeError("ent_embs must be float32 / float16 / bfloat16 and rel_vecs of the same dtype or float32 "
                            f"(got {ent_embs.dtype}, {rel_vecs.dtype})")
        dtypes = (names[ent_embs.dtype], names[rel_vecs.dtype])
        ent = ent_embs.contiguous()
        rel = rel_vecs.reshape(B, D).contiguous()
        idx = neg_idx.to(torch.int64).contiguous()
        dev = ent.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        # blp_inbatch_loss_save_floats: positives' scores, the workgroups' partial loss sums, the index of neg_idx for the backward
        pos = torch.empty(_lib.inbatch_save_floats(_lib.MODEL_IDS[rel_model], B, K, D), dtype=torch.float32, device=dev)
        neg = torch.empty((B, K), dtype=torch.float32, device=dev)
        stream = torch._C._cuda_getCurrentRawStream(dev.index)
        status = _lib.lib().blp_inbatch_loss_fwd(_lib.MODEL_IDS[rel_model], _lib.LOSS_IDS[loss_fn], *dtypes,
                                                   _ptr(ent), _ptr(rel), _ptr(idx), B, K, D, float(regularizer),
                                                   _ptr(loss), _ptr(pos), _ptr(neg), _ptr(inbatch_ticket(dev, stream)), dev.index, stream)
        _lib.check(status, "blp_inbatch_loss_fwd")
        ctx.meta = (rel_model, loss_fn, float(regularizer), B, K, D, rel_vecs.shape, dtypes)
        ctx.save_for_backward(ent, rel, idx, pos, neg)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        ent, rel, idx, pos, neg = ctx.saved_tensors
        rel_model, loss_fn, regularizer, B, K, D, rel_shape, dtypes = ctx.meta
        dev = ent.device
        grad_loss = grad_loss.to(torch.float32).contiguous()
        grad_ent = torch.empty((B, 2, D), dtype=ent.dtype, device=dev)
        grad_rel = torch.empty((B, D), dtype=rel.dtype, device=dev)
        status = _lib.lib().blp_inbatch_loss_bwd(_lib.MODEL_IDS[rel_model], _lib.LOSS_IDS[loss_fn], *dtypes,
                                                   _ptr(ent), _ptr(rel), _ptr(idx), B, K, D, regularizer,
                                                   _ptr(grad_loss), _ptr(pos), _ptr(neg), _ptr(grad_ent),
                                                   _ptr(grad_rel), dev.index, _stream(dev))
        _lib.check(status, "blp_inbatch_loss_bwd")
        return None, None, None, grad_ent, grad_rel.reshape(rel_shape), None


_glue_module = False  # False: not looked for yet; None: not available (the Python autograd.Function serves)


def torch_glue():
    """blp_amd/_torch_glue.so (csrc/torch_glue.cpp: the in-batch loss's autograd plumbing as a torch::autograd::Function, no
    kernels) bound to the product library's entry points -- or None when it is not built / not loadable with this torch,
    in which case _InBatchLoss above does the same job from Python (same C-ABI calls, ~100 us more host time per step)."""
    global _glue_module
    if _glue_module is False:
        try:
            from . import _torch_glue as g
            L = _lib.lib()
            if getattr(g, "abi_version", 0) // 10000 != L.blp_version() // 10000:  # a stale build against an older header
                raise ImportError(f"blp_amd/_torch_glue.so was built for include/blp_hip.h {getattr(g, 'abi_version', '< 6.0.0')}, the library is "
                                  f"{L.blp_version()}; rebuild with python -m blp_amd.build")
            g.bind(*(ctypes.cast(fn, ctypes.c_void_p).value for fn in (L.blp_inbatch_loss_fwd, L.blp_inbatch_loss_bwd, L.blp_last_error,
                                                                       L.blp_inbatch_loss_save_floats)))
            _glue_module = g
        except Exception as exc:  # not built, another torch, a stale build, a failed bind: the Python autograd.Function serves
            import warnings
            if not isinstance(exc, ModuleNotFoundError):
                warnings.warn(f"blp_amd: C++ autograd glue not used ({exc}); falling back to the Python autograd.Function")
            _glue_module = None
    return _glue_module


def inbatch_loss(rel_model, loss_fn, ent_embs, rel_vecs, neg_idx, regularizer=0.0):
    """compute_loss on in-batch negatives (fused forward + deterministic backward)."""
    glue = torch_glue()
    if glue is None:
        return _InBatchLoss.apply(rel_model, loss_fn, regularizer, ent_embs, rel_vecs, neg_idx)
    _require_device(ent_embs, rel_vecs, neg_idx)
    return glue.inbatch_loss(ent_embs, rel_vecs, neg_idx, _lib.MODEL_IDS[rel_model], _lib.LOSS_IDS[loss_fn], float(regularizer),
                             torch._C._cuda_getCurrentRawStream(ent_embs.device.index))
