"""All-entities ranking evaluation: the reference's eval_link_prediction (/root/reference/train.py:57-243)
restated around the fused HIP ranking, plus candidate-axis sharding across GPUs (new capability).

What changes relative to the reference, and what does not:
  * same inputs, same metric names, same numbers: raw and filtered MRR / Hits@{1,3,10}, the by-new-
    position split, the relation-category split, ``(mrr, ent_emb)`` return value;
  * the (2B, N) score matrix, the dense (2B, N) filter mask and the per-batch ``.item()`` syncs are
    gone: a block of triples becomes a (2B, 4) int32 count tensor on the device (blp_amd.ops.rank_all
    with a CSR filter from utils.FilterIndex), metrics are reduced once at the end;
  * with a process group, every rank encodes only rows [lo, hi) of the entity table; the ranking is
    then sharded along one of two axes (choose_shard_axis):
      - "candidate" (big tables, e.g. Wikidata5M): every rank keeps its rows, query / true-entity
        vectors are replicated by one exchange, and the per-shard counts of the whole evaluation
        are combined by ONE all-gather + sum;
      - "query" (small tables, many test triples, e.g. FB15k-237): the table shards are all-gathered
        once, every rank ranks its slice of the test triples against the full table, and the
        per-triple counts are all-gathered (no sum).  Per-query costs shrink with the world size too.
    RCCL over xGMI on GPUs; gloo in the CPU tests.

CPU tensors (the reference's CPU-runnable smoke configuration) take the reference's own dense route
through score_fn + get_metrics.
"""
import copy
import math

import torch
import torch.distributed as dist

from . import models, multidevice, ops, utils

HIT_POSITIONS = (1, 3, 10)


# ----------------------------------------------------------------------------------- one block
def _rank_block_dense(score_fn, table, q_fixed, q_rel, q_head, true_scores_from, filt_rowptr, filt_col):
    """Reference route (train.py:146-171) for CPU tensors: dense scores, then counts.
    ``true_scores_from`` is either ('row', true_row) or ('vec', q_true)."""
    ent = table.unsqueeze(0)
    fixed, rel = q_fixed.unsqueeze(1), q_rel.unsqueeze(1)
    pred = torch.cat((score_fn(ent, fixed[:q_head], rel[:q_head]), score_fn(fixed[q_head:], ent, rel[q_head:])))
    kind, value = true_scores_from
    if kind == "row":
        true = pred.gather(1, value.reshape(-1, 1))
    else:
        tv = value.unsqueeze(1)
        true = torch.cat((score_fn(tv[:q_head], fixed[:q_head], rel[:q_head]),
                          score_fn(fixed[q_head:], tv[q_head:], rel[q_head:])))
    gt_mask, ge_mask = pred > true, pred >= true
    counts = torch.empty((pred.shape[0], 4), dtype=torch.int32)
    counts[:, 0] = gt_mask.sum(1)
    counts[:, 1] = ge_mask.sum(1)
    if filt_rowptr is not None:
        keep = torch.ones_like(gt_mask)
        rows = torch.repeat_interleave(torch.arange(pred.shape[0]), filt_rowptr[1:] - filt_rowptr[:-1])
        keep[rows, filt_col] = False
        counts[:, 2] = (gt_mask & keep).sum(1)
        counts[:, 3] = (ge_mask & keep).sum(1)
    else:
        counts[:, 2:] = counts[:, :2]
    return counts


def fused_ranking_takes(model, table, num_queries):
    """True if a block of ``num_queries`` (half per side) against ``table`` goes through blp_rank_all (which takes
    the filter as device-side segments); otherwise the block takes a dense route that wants a CSR."""
    half = num_queries // 2
    return table.is_cuda and ops.rank_all_supported(model.rel_model, table.shape[1], half, num_queries - half)


def rank_block(model, table, q_fixed, q_rel, q_head, true_row=None, q_true=None, filt_rowptr=None, filt_col=None,
               rel_ids=None, filter=None, out=None):
    """Counts (Q, 4) int32 {gt, ge, gt_filtered, ge_filtered} for a block of queries against ``table``.
    Queries [0, q_head) replace the head, the rest replace the tail (train.py:149 order).  The filter is a CSR
    (filt_rowptr, filt_col) or, on a HIP device, an ops.SegmentFilter (``filter``)."""
    if table.is_cuda and not ops.rank_all_supported(model.rel_model, table.shape[1], q_head, q_fixed.shape[0] - q_head):
        if table.dtype is torch.float32 and ops.rank_all_wide_supported(model.rel_model, table.shape[1]):
            # the bilinear models at any width D % 4 == 0 up to 1024: the exact table pass, either filter form
            dev = table.device
            return ops.rank_all_wide(model.rel_model, table, q_fixed, q_rel, q_head,
                                     true_row=None if true_row is None else true_row.to(dev), q_true=q_true,
                                     filt_rowptr=None if filt_rowptr is None else filt_rowptr.to(dev),
                                     filt_col=None if filt_col is None else filt_col.to(dev), filter=filter, out=out)
        if filter is not None:
            raise ValueError("the dense any-width route takes the filter as a CSR (utils.FilterIndex.csr)")
        counts = _rank_block_generic_width(model, table, q_fixed, q_rel, q_head, true_row, q_true, filt_rowptr, filt_col)
        return counts if out is None else out.copy_(counts)
    if table.is_cuda:
        dev = table.device
        return ops.rank_all(model.rel_model, table, q_fixed, q_rel, q_head,
                            true_row=None if true_row is None else true_row.to(dev),
                            q_true=q_true,
                            filt_rowptr=None if filt_rowptr is None else filt_rowptr.to(dev),
                            filt_col=None if filt_col is None else filt_col.to(dev),
                            rel_ids=None if rel_ids is None else rel_ids.to(dev), filter=filter, out=out)
    if filter is not None:
        raise ValueError("SegmentFilter is the HIP path's filter form; CPU tensors take a CSR")
    source = ("row", true_row) if true_row is not None else ("vec", q_true)
    counts = _rank_block_dense(model.score_fn, table, q_fixed, q_rel, q_head, source, filt_rowptr, filt_col)
    return counts if out is None else out.copy_(counts)


def _rank_block_generic_width(model, table, q_fixed, q_rel, q_head, true_row, q_true, filt_rowptr, filt_col,
                              max_matrix_bytes=1 << 30):
    """HIP route for embedding widths the fused ranking kernels are not compiled for (300 / 768-wide
    bag-of-words encoders): order-exact dense scores from blp_score_fwd in query slabs of bounded size,
    then blp_rank_from_scores.  Same counts; the (Q, N) slab does go through HBM here."""
    dev = table.device
    n = table.shape[0]
    q_total = q_fixed.shape[0]
    slab = max(1, min(q_total, max_matrix_bytes // max(4 * n, 1)))
    ent = table.unsqueeze(0)
    out = torch.empty((q_total, 4), dtype=torch.int32, device=dev)
    if filt_rowptr is not None:
        filt_rowptr, filt_col = filt_rowptr.to(dev), filt_col.to(dev)
    for lo in range(0, q_total, slab):
        hi = min(lo + slab, q_total)
        parts = []
        for a, b, head in ((lo, min(hi, q_head), True), (max(lo, q_head), hi, False)):
            if a < b:
                fixed, rel = q_fixed[a:b].unsqueeze(1), q_rel[a:b].unsqueeze(1)
                parts.append(model.score_fn(ent, fixed, rel) if head else model.score_fn(fixed, ent, rel))
        scores = torch.cat(parts) if len(parts) > 1 else parts[0]
        kw = {}
        if true_row is not None:
            kw["true_idx"] = true_row[lo:hi].to(dev)
        else:
            tv = q_true[lo:hi]
            h_end = max(min(hi, q_head) - lo, 0)
            kw["true_score"] = torch.cat((model.score_fn(tv[:h_end], q_fixed[lo:lo + h_end], q_rel[lo:lo + h_end]),
                                          model.score_fn(q_fixed[lo + h_end:hi], tv[h_end:], q_rel[lo + h_end:hi])))
        if filt_rowptr is not None:
            kw["filt_rowptr"] = filt_rowptr[lo:hi + 1] - filt_rowptr[lo]
            kw["filt_col"] = filt_col[filt_rowptr[lo]:filt_rowptr[hi]]
        out[lo:hi] = ops.rank_from_scores(scores, **kw)
    return out


def metrics_from_counts(counts, k_values=HIT_POSITIONS):
    """utils.py:104-109 from counts: rr (Q, 2) f32 [raw, filtered], hits (Q, 2, 3) bool."""
    if counts.is_cuda:
        return ops.rank_metrics(counts, k_values)
    c = counts.to(torch.int64)
    avg = torch.stack((c[:, 0] + 1 + c[:, 1], c[:, 2] + 1 + c[:, 3]), dim=1).float() * 0.5
    k = torch.tensor(k_values, dtype=torch.float32).view(1, 1, -1)
    return avg.reciprocal(), avg.unsqueeze(-1) <= k


# ----------------------------------------------------------------------------------- sharding
def shard_bounds(num_rows, world_size, rank):
    per = (num_rows + world_size - 1) // world_size
    return min(rank * per, num_rows), min((rank + 1) * per, num_rows)


QUERY_AXIS_MAX_TABLE_BYTES = 256 << 20   # replicate the table only if it is this small ...
QUERY_AXIS_MIN_QUERIES = 256             # ... and every rank still gets a many-query block


def choose_shard_axis(num_rows, dim, num_queries, world_size):
    """"query" when replicating the table is cheap and each rank keeps >= 256 queries (the regime
    where per-query costs, not the table pass, dominate a candidate shard); else "candidate"."""
    if world_size <= 1:
        return "candidate"
    small_table = num_rows * dim * 4 <= QUERY_AXIS_MAX_TABLE_BYTES
    return "query" if small_table and num_queries // world_size >= QUERY_AXIS_MIN_QUERIES else "candidate"


def replicates_whole_table(num_entities, num_triples, half_table=False):
    """Candidate-axis shards need the vectors the queries are made of on every rank: the whole table by ONE all-gather when it is
    smaller than the 2T vectors of the triples, else those 2T vectors by ONE all-reduce of an owner-filled array."""
    return num_entities <= 2 * num_triples and not half_table


def exchange_plan(num_entities, dim, num_triples, world, axis, half_table=False):
    """The collectives ONE evaluation of num_triples triples (2 * num_triples queries) issues on `world` ranks, as
    rank_triples below issues them (its fused path; same conditions): a list of {"op", "what", "bytes_per_rank",
    "bytes_total"} -- bytes_per_rank = what one rank contributes, bytes_total = what every rank holds afterwards.  SURVEY
    8e: the candidate axis ends in ONE all-gather of the int32 counts, G x Q x 16 bytes in all.  No GPU needed (tests, bench's
    plan of an N-GPU run)."""
    if world <= 1:
        return []
    Q = 2 * num_triples
    plan = []
    if axis == "candidate":
        if replicates_whole_table(num_entities, num_triples, half_table):
            per = (num_entities + world - 1) // world  # all_gather_rows pads every shard to the longest
            plan.append({"op": "all_gather", "what": "table rows (the queries' vectors: the table is smaller than they are)",
                         "bytes_per_rank": per * dim * 4, "bytes_total": world * per * dim * 4})
        else:
            plan.append({"op": "all_reduce", "what": "(2T, D) f32 vectors of the triples' entities, each filled by the shard that owns the row",
                         "bytes_per_rank": Q * dim * 4, "bytes_total": Q * dim * 4})
        plan.append({"op": "all_gather", "what": "(2T, 4) int32 rank counts of every shard, then a sum",
                     "bytes_per_rank": Q * 16, "bytes_total": world * Q * 16})
    elif axis == "query":
        per = (num_triples + world - 1) // world
        plan.append({"op": "all_gather", "what": "(T / G, 8) int32 counts of each rank's triples (head and tail query side by side)",
                     "bytes_per_rank": per * 32, "bytes_total": world * per * 32})
    else:
        raise ValueError(f"unknown shard axis {axis!r}")
    return plan


def _via_host(tensor, group):
    """gloo carries host memory only: device tensors go through a host copy there (functional runs of the N > 1
    path on fewer GPUs than ranks, tests); RCCL takes them as they are."""
    return tensor.is_cuda and dist.get_backend(group) == "gloo"


def _threads(group):
    """True if ``group`` is a member of a one-process / one-thread-per-device group (multidevice.DeviceGroup) rather than
    a torch.distributed process group: the same two collectives, issued for all devices from one thread."""
    return isinstance(group, multidevice.Member)


def _all_reduce(tensor, group=None):
    if _threads(group):
        group.all_reduce(tensor)
    elif _via_host(tensor, group):
        host = tensor.cpu()
        dist.all_reduce(host, group=group)
        tensor.copy_(host)
    else:
        dist.all_reduce(tensor, group=group)


def _all_gather_into(full, part, group=None):
    if _threads(group):
        group.all_gather_into(full, part)
    elif _via_host(part, group):
        host = torch.empty(full.shape, dtype=full.dtype)
        dist.all_gather_into_tensor(host, part.cpu(), group=group)
        full.copy_(host)
    else:
        dist.all_gather_into_tensor(full, part, group=group)


def all_gather_rows(local, num_rows, world_size, group=None):
    """Row shards (shard_bounds layout) -> the full (num_rows, ...) tensor on every rank: ONE all-gather."""
    if world_size == 1:
        return local
    per = (num_rows + world_size - 1) // world_size
    padded = torch.zeros((per,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    padded[: local.shape[0]] = local
    full = torch.empty((world_size * per,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    _all_gather_into(full, padded, group)
    return full[:num_rows]


class ShardedRanker:
    """Candidate-axis sharded ranking.  Rank r owns table rows [lo, hi); the per-shard
    count tensors add up exactly to the unsharded counts, so one all-gather of int32 counts per
    evaluation is the only data-path collective."""

    def __init__(self, model, local_table, num_rows, group=None):
        self.model = model
        self.table = local_table
        self.num_rows = int(num_rows)
        self.group = group
        if _threads(group):
            self.world, self.rank = group.world, group.rank
        else:
            self.world = dist.get_world_size(group) if self._distributed() else 1
            self.rank = dist.get_rank(group) if self._distributed() else 0
        self.lo, self.hi = shard_bounds(self.num_rows, self.world, self.rank)
        if local_table.shape[0] != self.hi - self.lo:
            raise ValueError(f"rank {self.rank} must hold rows [{self.lo}, {self.hi}) of the table, "
                             f"got {local_table.shape[0]} rows")
        self._blocks = []

    def _distributed(self):
        return dist.is_available() and dist.is_initialized()

    def gather_rows(self, rows):
        """Vectors of the given global table rows on every rank: owners fill, one all-reduce (adding
        exact zeros) replicates.  Called once per evaluation for the entities of the test triples."""
        rows = rows.to(device=self.table.device, dtype=torch.long)
        out = torch.zeros((rows.shape[0], self.table.shape[1]), dtype=self.table.dtype, device=self.table.device)
        if self.hi > self.lo:  # no host decision on the data: rows of other shards read row 0 and are zeroed
            mine = (rows >= self.lo) & (rows < self.hi)
            local = torch.where(mine, rows - self.lo, torch.zeros_like(rows))
            out = torch.where(mine.unsqueeze(1), self.table[local], out)
        if self.world > 1:
            _all_reduce(out, self.group)
        return out

    def rank_block(self, q_fixed, q_rel, q_true, q_head, filt_rowptr=None, filt_col=None, rel_ids=None, filter=None):
        """Local counts of one query block against this rank's shard (queued for the final exchange).
        filt_col are GLOBAL table rows; only the ones this shard owns are kept (a SegmentFilter carries this
        shard's first row as row_base and the kernel skips the rows of other shards)."""
        if filter is not None:
            filter = filter._replace(row_base=self.lo)
        if filt_rowptr is not None and self.table.is_cuda:  # global rows minus this shard's first row; others are skipped
            filt_col = filt_col.to(self.table.device) - self.lo
        elif filt_rowptr is not None:
            owned = (filt_col >= self.lo) & (filt_col < self.hi)
            per_row = torch.zeros(filt_rowptr.shape[0] - 1, dtype=torch.long)
            rows = torch.repeat_interleave(torch.arange(per_row.shape[0]), filt_rowptr[1:] - filt_rowptr[:-1])
            per_row.index_add_(0, rows[owned], torch.ones(int(owned.sum()), dtype=torch.long))
            filt_rowptr = torch.cat((torch.zeros(1, dtype=torch.long), torch.cumsum(per_row, 0)))
            filt_col = filt_col[owned] - self.lo
        counts = rank_block(self.model, self.table, q_fixed, q_rel, q_head, q_true=q_true,
                            filt_rowptr=filt_rowptr, filt_col=filt_col, rel_ids=rel_ids, filter=filter)
        self._blocks.append(counts)
        return counts

    def finish(self):
        """Global counts of every queued block: ONE all-gather of the (Q, 4) int32 tensor, then a sum."""
        local = torch.cat(self._blocks) if self._blocks else torch.zeros((0, 4), dtype=torch.int32, device=self.table.device)
        self._blocks = []
        if self.world == 1:
            return local
        gathered = torch.empty((self.world,) + tuple(local.shape), dtype=local.dtype, device=local.device)
        _all_gather_into(gathered.view(-1), local.contiguous().view(-1), self.group)
        return gathered.sum(dim=0, dtype=torch.int32)


# ----------------------------------------------------------------------------------- a set of triples
class _Stopwatch:
    """Device-side timing of the collectives of one evaluation (bench.py's ``exchange_ms``): events around each exchange
    on the current stream, read after the caller's synchronisation.  ``timing`` = None: nothing is recorded."""

    def __init__(self, timing, device):
        self.timing = timing if (timing is not None and device.type == "cuda") else None

    def __enter__(self):
        if self.timing is not None:
            self.start = torch.cuda.Event(enable_timing=True)
            self.stop = torch.cuda.Event(enable_timing=True)
            self.start.record()
        return self

    def __exit__(self, *exc):
        if self.timing is not None:
            self.stop.record()
            self.timing.setdefault("exchange_events", []).append((self.start, self.stop))
        return False


def exchange_ms(timing):
    """Milliseconds the recorded exchanges of ``timing`` took (call after a device synchronisation)."""
    return sum(a.elapsed_time(b) for a, b in timing.get("exchange_events", []))


def rank_triples(model, table, triples, ent2idx, index=None, *, num_entities=None, group=None, world=1, rank=0,
                 axis="candidate", block_size=65536, timing=None):
    """The reference's evaluation loop body (train.py:128-171) for a whole set of triples at once: rank counts of
    every triple's head and tail query against all ``num_entities`` candidates, raw and filtered.

    triples   (T, 3) int64 on the table's device, rows (head, tail, rel) entity / relation ids, any order
    ent2idx   utils.make_ent2idx map (entity id -> table row) on the same device
    index     utils.FilterIndex of the filtering graph, or None (filtered counts = raw counts)
    table     world == 1 or axis == "query": the full (num_entities, D) table; axis == "candidate": this rank's
              rows shard_bounds(num_entities, world, rank) of it
    timing    optional dict: the collectives are bracketed by device events (exchange_ms(timing) after a synchronise)
    Returns (triples in evaluation order -- as given --, counts (2T, 4) int32 in that order with every head query first,
    ids_ok: 0-dim bool tensor or None -- the reference's assertion train.py:137-138, left on the device).

    Everything runs on the table's device without a host round trip: the id lookups (train.py:134-135), the layout of
    the queries -- left as (vector row, relation) index pairs -- and the filter segments are one kernel
    (ops.build_queries); the blocks are then ONE library call (blp_rank_all_batches: per block <= 8 launches, none of them
    torch's).
    Collectives: candidate axis -- the vectors the queries are made of are replicated ONCE (the whole table by one
    all-gather when it is smaller than the 2T vectors of the triples, else those vectors by one all-reduce of an
    owner-filled array) and the (2T, 4) counts of every shard are combined by ONE all-gather + sum; query axis -- ONE
    all-gather of the per-triple counts.  No size is decided on the device (no torch.unique, no .item())."""
    device = table.device
    num_entities = table.shape[0] if num_entities is None else num_entities
    num_triples = triples.shape[0]
    by_query = world > 1 and axis == "query"
    by_candidate = world > 1 and not by_query
    t_lo, t_hi = shard_bounds(num_triples, world, rank) if by_query else (0, num_triples)
    n = t_hi - t_lo
    mine = slice(t_lo, t_hi)
    # (whether the fused path takes a block depends on the model and the width only; WHICH kernels rank it is decided per
    # block inside blp_rank_all_batches -- the short last block of a call may well take another route than the full ones)
    fused = n > 0 and model.rel_emb.weight.dtype == torch.float32 and fused_ranking_takes(model, table, 2 * min(block_size, n))
    row_lo = shard_bounds(num_entities, world, rank)[0] if by_candidate else 0
    head_pos = tail_pos = None

    def block_positions():
        idx = torch.arange(n, device=device)
        first = torch.div(idx, block_size, rounding_mode="floor") * block_size       # first triple of the block
        hp = first + idx                                                                # = 2 * first + (idx - first)
        return idx, hp, hp + torch.clamp(n - first, max=block_size)

    if fused:
        # The queries stay INDICES: (row of `source`, row of rel_emb) -- no (2n, D) arrays at all.  `source` holds the
        # vectors the queries are made of: the table itself, or on a candidate shard a replicated copy of what the
        # triples need from the other shards.
        rel_w = model.rel_emb.weight
        source, by_position = table, False
        half_table = table.dtype != torch.float32  # the 16-bit copy of the table (ops.rank_all_batches): candidates only
        if by_candidate and replicates_whole_table(num_entities, num_triples, half_table):  # small table: all of it, one all-gather
            with _Stopwatch(timing, device):
                source = all_gather_rows(table, num_entities, world, group)
        elif by_candidate or half_table:                          # big table: the 2T vectors of the triples, one all-reduce
            # (a 16-bit table on any axis: the queries' own vectors are its rows WIDENED to float32 -- exactly --, which this
            #  gather does on the way; nothing to exchange unless the candidate axis is sharded)
            source = ops.gather_triple_vectors(triples[mine], ent2idx, table, row_base=row_lo)
            if by_candidate:
                with _Stopwatch(timing, device):
                    _all_reduce(source, group)
            by_position = True
        # one kernel (blp_build_queries) instead of ~35 small torch kernels: lookups, layout, binary searches
        qb = ops.build_queries(triples[mine], ent2idx, source, rel_w, block_size, index=index, gather=False, row_base=row_lo,
                               by_position=by_position, num_rows=num_entities)
        ids_ok = qb.ids_min >= 0
        # every block in ONE library call (blp_rank_all_batches with a ranking pass per block: the blocks are issued back to
        # back by the library -- at the reference's Wikidata5M batching, 2 triples per table pass, a Python-level loop over
        # the blocks costs as much host time per pass as the pass takes on a 1/8 shard)
        counts = ops.rank_all_batches(model.rel_model, table, qb.fixed_row, rel_w, qb.rel_ids, qb.true_row, n, block_size,
                                      filter=qb.filter, source=source, block_triples=block_size)
        if by_candidate:  # ONE all-gather for the whole set; the shards' counts add up exactly
            with _Stopwatch(timing, device):
                gathered = torch.empty((world,) + tuple(counts.shape), dtype=counts.dtype, device=device)
                _all_gather_into(gathered.view(-1), counts.view(-1), group)
                counts = gathered.sum(dim=0, dtype=torch.int32)
    else:
        # CPU tensors, half-precision relation tables, widths the fused kernels do not take: the torch prelude and
        # gathered query vectors (dense routes; a CSR filter per block).
        if table.dtype != torch.float32:
            table = table.float()  # (a 16-bit table on a dense route: widened once, exactly)
        ranker = ShardedRanker(model, table, num_entities, group) if by_candidate else None
        heads = ent2idx[triples[:, 0]]
        tails = ent2idx[triples[:, 1]]
        ids_ok = torch.minimum(heads.min(), tails.min()) >= 0 if num_triples else None
        heads, tails = heads.clamp_min(0), tails.clamp_min(0)  # a bad id reads row 0 instead of out of bounds; ids_ok tells
        if by_candidate:  # replicate the vectors of the entities in the triples: one exchange
            with _Stopwatch(timing, device):
                source = ranker.gather_rows(torch.cat((heads, tails)))
            head_ref = torch.arange(num_triples, device=device)
            tail_ref = head_ref + num_triples
        else:
            source, head_ref, tail_ref = table, heads[mine], tails[mine]
        idx, head_pos, tail_pos = block_positions()
        fixed_src = torch.empty(2 * n, dtype=torch.long, device=device)
        true_src = torch.empty_like(fixed_src)
        rel_ids = torch.empty_like(fixed_src)
        order_src = torch.empty_like(fixed_src)  # position in the [all heads | all tails] order of utils.FilterIndex
        fixed_src[head_pos], fixed_src[tail_pos] = tail_ref, head_ref
        true_src[head_pos], true_src[tail_pos] = head_ref, tail_ref
        rel_ids[head_pos] = rel_ids[tail_pos] = triples[mine, 2]
        order_src[head_pos], order_src[tail_pos] = idx, idx + n
        q_fixed = source[fixed_src]
        q_rel = model.rel_emb(rel_ids)
        q_true = source[true_src] if by_candidate else None
        seg = None
        if index is not None and n > 0 and fused_ranking_takes(model, table, 2 * min(block_size, n)):  # slices of the sorted index: nothing is listed per batch
            seg = index.segments(triples[mine], ent2idx, device)
            seg = seg._replace(seg_lo=seg.seg_lo[order_src], seg_hi=seg.seg_hi[order_src], exclude=seg.exclude[order_src])
        counts = torch.empty((2 * n, 4), dtype=torch.int32, device=device)
        for start in range(0, n, block_size):
            b = min(start + block_size, n) - start
            sl = slice(2 * start, 2 * (start + b))
            filt = {}
            if seg is not None:
                filt = dict(filter=seg._replace(seg_lo=seg.seg_lo[sl], seg_hi=seg.seg_hi[sl], exclude=seg.exclude[sl]))
            elif index is not None:  # dense any-width routes take a CSR
                rowptr, col = index.csr(triples[t_lo + start: t_lo + start + b], ent2idx, device)
                filt = dict(filt_rowptr=rowptr, filt_col=col)
            if by_candidate:
                ranker.rank_block(q_fixed[sl], q_rel[sl], q_true[sl], b, rel_ids=rel_ids[sl], **filt)
            else:
                rank_block(model, table, q_fixed[sl], q_rel[sl], b, true_row=true_src[sl], rel_ids=rel_ids[sl], out=counts[sl],
                           **filt)
        if by_candidate:
            with _Stopwatch(timing, device):
                counts = ranker.finish()  # ONE all-gather for the whole set; blocks in the order they were queued
    if n > block_size:  # every head query first, like one big batch
        if head_pos is None:
            _, head_pos, tail_pos = block_positions()
        counts = counts[torch.cat((head_pos, tail_pos))]
    if by_query:  # per-triple counts of every rank's slice: ONE all-gather for the whole set
        with _Stopwatch(timing, device):
            both = all_gather_rows(torch.cat((counts[:n], counts[n:]), dim=1), num_triples, world, group)
        counts = torch.cat((both[:, :4], both[:, 4:])).contiguous()
    return triples, counts, ids_ok


# ----------------------------------------------------------------------------------- evaluation
# ----------------------------------------------------------------------------------- link prediction (top-k)
def _stable_topk(scores, rows, removed, k):
    """Order of blp_topk on dense candidate lists: (Q, n) scores, global rows, removed flags -> the first k (rows, scores) by
    descending score (-0 == +0), ties by ascending row, NaN after every number, removed entries and rows < 0 dropped; slots
    beyond the candidates left: -1 / NaN.  numpy's argsort(-scores, kind="stable") for rows in ascending order."""
    gone = removed | (rows < 0)
    order = torch.argsort(torch.where(gone, torch.iinfo(torch.int64).max, rows), dim=1, stable=True)
    neg = -scores.gather(1, order)
    order = order.gather(1, torch.sort(neg, dim=1, stable=True).indices)
    order = order.gather(1, torch.sort(gone.gather(1, order).to(torch.uint8), dim=1, stable=True).indices)
    n = scores.shape[1]
    take = order[:, :min(k, n)]
    out_rows = torch.where(gone.gather(1, take), -1, rows.gather(1, take))
    out_scores = torch.where(out_rows < 0, float("nan"), scores.gather(1, take))
    if k > n:
        pad = k - n
        out_rows = torch.cat((out_rows, out_rows.new_full((out_rows.shape[0], pad), -1)), 1)
        out_scores = torch.cat((out_scores, out_scores.new_full((out_scores.shape[0], pad), float("nan"))), 1)
    return out_rows, out_scores


def _filtered_pairs(filt, lo, hi, row_base, N, dev):
    """What the filter removes for queries [lo, hi): (owner, local) -- query lo + owner loses table row local -- from the
    segments (seg_lo, seg_hi, values, exclude, ent2idx) as SegmentFilter holds them (None: nothing), with blp_filter's
    semantics: exclude[q] is never removed, ids without a row and rows outside [row_base, row_base + N) remove nothing."""
    none = torch.empty(0, dtype=torch.int64, device=dev)
    if filt is None:
        return none, none
    seg_lo, seg_hi, values, exclude, e2i = filt
    n_per = (seg_hi[lo:hi] - seg_lo[lo:hi]).clamp(min=0)
    total = int(n_per.sum())
    if not total:
        return none, none
    owner = torch.repeat_interleave(torch.arange(hi - lo, device=dev), n_per, output_size=total)
    first = torch.cumsum(n_per, 0) - n_per
    vals = values[seg_lo[lo:hi][owner] + torch.arange(total, device=dev) - first[owner]]
    keep = torch.ones_like(vals, dtype=torch.bool) if exclude is None else vals != exclude[lo:hi][owner]
    if e2i is not None:
        ok = (vals >= 0) & (vals < e2i.shape[0])
        vals = torch.where(ok, e2i[torch.where(ok, vals, torch.zeros_like(vals))], torch.full_like(vals, -1))
    local = vals - row_base
    keep &= (local >= 0) & (local < N)
    return owner[keep], local[keep]


def _topk_dense(score_fn, table, fixed, rel, q_head, k, row_base, filt, max_matrix_bytes=1 << 28):
    """The reference's route (score_fn over the whole table, train.py:146-147) + the stable order, in query chunks of a
    bounded (chunk, N) matrix: CPU tensors, and widths blp_topk is not compiled for.  filt: (seg_lo, seg_hi, values,
    exclude, ent2idx) as SegmentFilter holds them, or None."""
    Q, N = fixed.shape[0], table.shape[0]
    dev = table.device
    chunk = max(1, min(max(Q, 1), max_matrix_bytes // max(4 * N, 1)))
    ent = table.unsqueeze(0)
    grows = torch.arange(row_base, row_base + N, device=dev, dtype=torch.int64)
    rows_out = torch.empty((Q, k), dtype=torch.int64, device=dev)
    scores_out = torch.empty((Q, k), dtype=torch.float32, device=dev)
    for lo in range(0, Q, chunk):
        hi = min(lo + chunk, Q)
        parts = []
        for a, b, head in ((lo, min(hi, q_head), True), (max(lo, q_head), hi, False)):
            if a < b:
                f, r = fixed[a:b].unsqueeze(1), rel[a:b].unsqueeze(1)
                parts.append(score_fn(ent, f, r) if head else score_fn(f, ent, r))
        pred = torch.cat(parts) if len(parts) > 1 else parts[0]
        removed = torch.zeros(pred.shape, dtype=torch.bool, device=dev)
        owner, local = _filtered_pairs(filt, lo, hi, row_base, N, dev)
        removed[owner, local] = True
        rows_out[lo:hi], scores_out[lo:hi] = _stable_topk(pred, grows.expand(hi - lo, N), removed, k)
    return rows_out, scores_out


def _topk_one_set(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, k, filter=None, row_base=0):
    """ops.topk's call served by ops.topk_sets_wide (TransE at the widths blp_topk is not compiled for): ONE candidate set
    that is the local table, every query in its group -- the same contract, the same bits."""
    dev, N, Q = table.device, table.shape[0], fixed_row.shape[0]
    # the three two-entry offset arrays in ONE host-to-device copy; the set's rows are made on the device
    ptr = torch.tensor([0, N, 0, q_head, 0, Q - q_head], dtype=torch.int64, device=dev)
    return ops.topk_sets_wide(rel_model, table, source, fixed_row, rel_emb, rel_ids, q_head, k, ptr[0:2],
                              torch.arange(row_base, row_base + N, dtype=torch.int64, device=dev), ptr[2:4], ptr[4:6],
                              filter=filter, row_base=row_base)


def predict_links(model, table, triples, k, ent2idx, *, side="both", filter_index=None, entities=None, group=None, world=1,
                  rank=0, num_entities=None):
    """Answer link-prediction queries: for every triple (head, tail, rel) of ``triples`` (T, 3) the k table rows the model
    scores highest as the replaced entity -- ``side`` "head": (?, r, t); "tail": (h, r, ?); "both": [heads | tails], the
    evaluation's order (train.py:149).  The entity at the replaced position is not used, except that a known edge never
    filters the triple's own entity (utils.py:71,78): pass -1 there to have every known edge filtered.
    table        (N, D) entity table (build_entity_table); with world > 1 this rank's rows shard_bounds(num_entities, world,
                 rank) of it, and every rank calls with the same triples
    ent2idx      utils.make_ent2idx map (entity id -> table row); the fixed entity of every query must have a row
    filter_index utils.FilterIndex of the known edges (the training graph): the rows it names are removed, not demoted
    entities     optional (num_entities,) entity id of every table row: ids instead of rows are returned
    Returns (rows or ids (Q, k) int64, scores (Q, k) float32): descending score, ties by ascending row, NaN last; -1 / NaN
    beyond the candidates left.  Scores are score_fn's values bit for bit.  HIP tensors at a width blp_topk takes: blp_topk
    (one call per rank; shards merged by one all-gather of the (Q, k) lists + blp_topk_merge).  A float16 / bfloat16 HIP
    table takes blp_topk_typed, which reads the 16-bit rows as they are: rows and scores are those of the same table widened
    to float32, bit for bit.  HIP tensors at the other widths D % 4 == 0, 4 <= D <= 1024 (the BOW / DKRL encoders' 300 and
    768), k <= 256: DistMult / ComplEx / SimplE on a float32 table take blp_topk_wide; TransE (float32, float16 or bfloat16
    table) takes blp_topk_sets_wide with ONE candidate set that is the local table -- the same contract, the same bits, the
    same merge of shards.  Everything else (CPU tensors, k > 256, other widths, the bilinear models on a 16-bit table at
    those widths) takes the reference's dense route (score_fn + a stable sort) in query chunks."""
    model = _module(model)
    if side not in ("head", "tail", "both"):
        raise ValueError(f"side must be 'head', 'tail' or 'both', got {side!r}")
    k = int(k)
    if k < 1:
        raise ValueError(f"k = {k} must be >= 1")
    device = table.device
    n_local, D = table.shape
    num_entities = n_local if num_entities is None else int(num_entities)
    row_lo = shard_bounds(num_entities, world, rank)[0] if world > 1 else 0
    triples = triples.to(device=device, dtype=torch.long).reshape(-1, 3)
    ent2idx = ent2idx.to(device=device, dtype=torch.long)
    T = triples.shape[0]
    h, t, r = triples[:, 0], triples[:, 1], triples[:, 2]
    heads, tails = side in ("head", "both"), side in ("tail", "both")
    q_head = T if heads else 0
    fixed_ids = torch.cat([x for x, on in ((t, heads), (h, tails)) if on])
    rel_ids = torch.cat([r] * (int(heads) + int(tails)))
    Q = fixed_ids.shape[0]
    known = (fixed_ids >= 0) & (fixed_ids < ent2idx.shape[0])
    fixed_rows = torch.where(known, ent2idx[torch.where(known, fixed_ids, torch.zeros_like(fixed_ids))], torch.full_like(fixed_ids, -1))
    rel_w = model.rel_emb.weight.detach()
    if Q and bool(((fixed_rows < 0) | (fixed_rows >= num_entities) | (rel_ids < 0) | (rel_ids >= rel_w.shape[0])).any()):
        raise ValueError("predict_links: a query's fixed entity has no table row, or its relation is out of range")
    # the vectors the queries are made of, on every rank: owner-filled, then summed over the ranks
    if world > 1:
        local = fixed_rows - row_lo
        mine = (local >= 0) & (local < n_local)
        fixed_vecs = torch.zeros((Q, D), dtype=table.dtype, device=device)
        fixed_vecs[mine] = table[local[mine]]
        _all_reduce(fixed_vecs, group)
        source, src_rows = fixed_vecs, torch.arange(Q, device=device)
    else:
        source, src_rows = table, fixed_rows
    # the fused call this table takes, if any: blp_topk at its widths; at the others blp_topk_wide (the bilinear models, a
    # float32 table) or blp_topk_sets_wide with the local table as the one candidate set (TransE)
    route = None
    if table.is_cuda:
        if ops.topk_supported(model.rel_model, D, k, table.dtype):
            route = ops.topk
        elif ops.topk_wide_supported(model.rel_model, D, k, table.dtype):
            route = ops.topk_wide
        elif ops.topk_sets_wide_supported(model.rel_model, D, k, table.dtype):
            route = _topk_one_set
    fused = route is not None
    if fused and table.dtype != torch.float32:
        # the kernels take float32 query vectors: the Q fixed rows, widened (exact; after the sum on several ranks -- x + 0
        # is exact in 16 bits too)
        source, src_rows = (source if world > 1 else table[fixed_rows]).float(), torch.arange(Q, device=device)
    filt = None
    if filter_index is not None and Q:
        seg = filter_index.segments(triples, ent2idx, device, row_base=row_lo)
        sel = torch.cat([x for x, on in ((torch.arange(T, device=device), heads), (torch.arange(T, 2 * T, device=device), tails)) if on])
        filt = ops.SegmentFilter(seg.seg_lo[sel].contiguous(), seg.seg_hi[sel].contiguous(), seg.values,
                                 seg.exclude[sel].contiguous(), seg.ent2idx, row_lo)
    if fused:
        rows, scores = route(model.rel_model, table, source, src_rows, rel_w, rel_ids, q_head, k, filter=filt, row_base=row_lo)
    else:
        dense_filt = None if filt is None else (filt.seg_lo, filt.seg_hi, filt.values, filt.exclude, filt.ent2idx)
        rows, scores = _topk_dense(model.score_fn, table, source[src_rows], rel_w[rel_ids], q_head, k, row_lo, dense_filt)
    if world > 1:
        # ONE all-gather of every rank's (Q, k) list, rows and score bits packed together, then the merge
        packed = torch.stack((rows, scores.view(torch.int32).to(torch.int64)), dim=-1)
        full = torch.empty((world * Q, k, 2), dtype=packed.dtype, device=device)
        _all_gather_into(full, packed, group)
        full = full.view(world, Q, k, 2)
        all_rows = full[..., 0].permute(1, 0, 2).reshape(Q, world * k)
        all_scores = full[..., 1].to(torch.int32).view(torch.float32).permute(1, 0, 2).reshape(Q, world * k)
        if fused:
            rows, scores = ops.topk_merge(all_rows, all_scores, k)
        else:
            rows, scores = _stable_topk(all_scores, all_rows, torch.zeros_like(all_rows, dtype=torch.bool), k)
    if entities is not None:
        entities = entities.to(device=device, dtype=torch.long)
        rows = torch.where(rows >= 0, entities[rows.clamp(min=0)], rows)
    return rows, scores


# ----------------------------------------------------------------------------------- per-query candidate lists
def sample_candidates(num_queries, num_rows, c, generator=None, device=None):
    """(num_queries, c) int64 table rows drawn uniformly (with replacement) from [0, num_rows) by a torch generator: the
    deterministic helper of a sampled-candidate evaluation (rank_candidates(..., include_true=False)).  The reference has no
    such protocol; this only fixes how the negatives are drawn."""
    where = generator.device if generator is not None else "cpu"
    rows = torch.randint(0, int(num_rows), (int(num_queries), int(c)), generator=generator, device=where, dtype=torch.int64)
    return rows if device is None else rows.to(device)


def _rank_lists_dense(score_fn, table, fixed, rel, true_vec, q_head, ptr, rows, row_base, filt, want_scores,
                      max_bytes=1 << 28):
    """The dense route of rank_candidates: score_fn on the gathered rows of the lists, in query chunks of bounded bytes, the
    comparisons against the true score, the filter through _filtered_pairs.  CPU tensors and the widths neither blp_rank_lists
    nor blp_rank_lists_wide takes; on CPU tensors it is the oracle of the fused routes.  fixed / rel / true_vec: (Q, D) float32 (true_vec None: scores
    only); ptr (Q + 1,), rows (nnz,) global rows.  Returns (counts (Q, 4) int32 or None, scores (nnz,) or None)."""
    Q, (N, D) = fixed.shape[0], table.shape
    dev = table.device
    nnz = rows.shape[0]
    counts = torch.zeros((Q, 4), dtype=torch.int32, device=dev) if true_vec is not None else None
    scores = torch.full((nnz,), float("nan"), dtype=torch.float32, device=dev) if want_scores else None
    budget = max(1, max_bytes // (12 * D))  # entries per chunk: three gathered (n, D) float32 operands
    ptr_host = ptr.tolist()
    lo = 0
    while lo < Q:
        hi = lo + 1
        while hi < Q and ptr_host[hi + 1] - ptr_host[lo] <= budget:
            hi += 1
        p0, p1 = ptr_host[lo], ptr_host[hi]
        n_per = ptr[lo + 1:hi + 1] - ptr[lo:hi]
        owner = torch.repeat_interleave(torch.arange(hi - lo, device=dev), n_per, output_size=p1 - p0)
        local = rows[p0:p1] - row_base
        valid = (local >= 0) & (local < N)
        e = table[torch.where(valid, local, torch.zeros_like(local))].float() if N else table.new_zeros((p1 - p0, D)).float()
        f, r = fixed[lo:hi][owner], rel[lo:hi][owner]
        is_head = owner < q_head - lo
        s = torch.empty((p1 - p0,), dtype=torch.float32, device=dev)
        if bool(is_head.any()):
            s[is_head] = score_fn(e[is_head], f[is_head], r[is_head])
        if bool((~is_head).any()):
            s[~is_head] = score_fn(f[~is_head], e[~is_head], r[~is_head])
        if scores is not None:
            scores[p0:p1] = torch.where(valid, s, torch.full_like(s, float("nan")))
        if counts is not None:
            h_end = max(min(hi, q_head) - lo, 0)
            tv, fq, rq = true_vec[lo:hi], fixed[lo:hi], rel[lo:hi]
            true = torch.cat((score_fn(tv[:h_end], fq[:h_end], rq[:h_end]), score_fn(fq[h_end:], tv[h_end:], rq[h_end:])))
            kt = true[owner]
            gt, ge = valid & (s > kt), valid & (s >= kt)
            f_owner, f_local = _filtered_pairs(filt, lo, hi, row_base, N, dev)
            span = max(N, 1)
            kept = ~torch.isin(owner * span + torch.where(valid, local, torch.zeros_like(local)), f_owner * span + f_local)
            for col, mask in enumerate((gt, ge, gt & kept, ge & kept)):
                counts[lo:hi, col] = torch.zeros(hi - lo, dtype=torch.int64, device=dev).index_add_(0, owner, mask.to(torch.int64)).to(torch.int32)
        lo = hi
    return counts, scores


def rank_candidates(model, table, triples, candidates, ent2idx, *, side="both", filter_index=None, candidates_are="rows",
                    include_true=True, return_scores=False):
    """Rank every triple's true entity against a candidate list of its own -- sampled negatives, the candidates of a first
    stage to re-rank -- instead of the whole table: only the listed rows are read.
    triples      (T, 3) (head, tail, rel); ``side`` "head": (?, r, t); "tail": (h, r, ?); "both": Q = 2 T queries in
                 predict_links' order [heads | tails]
    candidates   (Q, C) int64, padded with -1, or a CSR pair (ptr (Q + 1,), rows (nnz,)); table rows, or entity ids mapped
                 through ``ent2idx`` with candidates_are="ids" (an id without a row is skipped).  A list is a multiset
    ent2idx      utils.make_ent2idx map (entity id -> table row); the fixed and the true entity of a query must have a row
    filter_index utils.FilterIndex of the known edges: the filtered columns count only entries it does not remove (the
                 triple's own entity is never removed)
    include_true False: the lists hold negatives only and 1 is added to both ``ge`` columns, so that the counts mean what
                 rank_all's mean (the true entity ties with itself) and metrics_from_counts applies unchanged
    Returns counts (Q, 4) int32 {gt, ge, gt_filtered, ge_filtered}; with return_scores also the candidates' scores in the
    caller's layout ((Q, C), or (nnz,); NaN at padding and skipped entries), score_fn's values bit for bit.
    A HIP table at a width blp_rank_lists takes goes through it, a DistMult / ComplEx / SimplE model at any other width
    D % 4 == 0, 4 <= D <= 1024 (the BOW / DKRL encoders' 300 and 768) through blp_rank_lists_wide (a float16 / bfloat16 table
    is read as it is; only the Q fixed and true rows are widened); CPU tensors and everything else take the dense route:
    score_fn on gathered rows."""
    model = _module(model)
    if side not in ("head", "tail", "both"):
        raise ValueError(f"side must be 'head', 'tail' or 'both', got {side!r}")
    if candidates_are not in ("rows", "ids"):
        raise ValueError(f"candidates_are must be 'rows' or 'ids', got {candidates_are!r}")
    device = table.device
    N, D = table.shape
    triples = triples.to(device=device, dtype=torch.long).reshape(-1, 3)
    ent2idx = ent2idx.to(device=device, dtype=torch.long)
    T = triples.shape[0]
    h, t, r = triples[:, 0], triples[:, 1], triples[:, 2]
    heads, tails = side in ("head", "both"), side in ("tail", "both")
    q_head = T if heads else 0
    fixed_ids = torch.cat([x for x, on in ((t, heads), (h, tails)) if on])
    true_ids = torch.cat([x for x, on in ((h, heads), (t, tails)) if on])
    rel_ids = torch.cat([r] * (int(heads) + int(tails)))
    Q = fixed_ids.shape[0]

    def to_rows(ids):
        known = (ids >= 0) & (ids < ent2idx.shape[0])
        return torch.where(known, ent2idx[torch.where(known, ids, torch.zeros_like(ids))], torch.full_like(ids, -1))

    fixed_rows, true_rows = to_rows(fixed_ids), to_rows(true_ids)
    rel_w = model.rel_emb.weight.detach()
    if Q and bool(((fixed_rows < 0) | (fixed_rows >= N) | (true_rows < 0) | (true_rows >= N) | (rel_ids < 0) |
                   (rel_ids >= rel_w.shape[0])).any()):
        raise ValueError("rank_candidates: a query's fixed or true entity has no table row, or its relation is out of range")
    rect = None
    if isinstance(candidates, (tuple, list)):
        ptr, rows = (x.to(device=device, dtype=torch.long).reshape(-1) for x in candidates)
        if ptr.shape[0] != Q + 1:
            raise ValueError(f"candidates: ptr must have Q + 1 = {Q + 1} entries, got {ptr.shape[0]}")
    else:
        rect = candidates.to(device=device, dtype=torch.long)
        if rect.dim() != 2 or rect.shape[0] != Q:
            raise ValueError(f"candidates must be (Q, C) with Q = {Q}, got {tuple(rect.shape)}")
        ptr = torch.arange(Q + 1, device=device, dtype=torch.long) * rect.shape[1]
        rows = rect.reshape(-1)
    if candidates_are == "ids":
        rows = to_rows(rows)
    filt = None
    if filter_index is not None and Q:
        seg = filter_index.segments(triples, ent2idx, device)
        sel = torch.cat([x for x, on in ((torch.arange(T, device=device), heads), (torch.arange(T, 2 * T, device=device), tails)) if on])
        filt = ops.SegmentFilter(seg.seg_lo[sel].contiguous(), seg.seg_hi[sel].contiguous(), seg.values,
                                 seg.exclude[sel].contiguous(), seg.ent2idx, 0)
    fused = None
    if table.is_cuda and ops.rank_lists_supported(model.rel_model, D, table.dtype):
        fused = ops.rank_lists
    elif table.is_cuda and ops.rank_lists_wide_supported(model.rel_model, D, table.dtype):
        fused = ops.rank_lists_wide  # DistMult / ComplEx / SimplE off 64 / 128 / 256: the BOW / DKRL widths
    if fused is not None:
        if table.dtype != torch.float32:  # float32 query vectors: the Q fixed and the Q true rows, widened (exact)
            source = table[torch.cat((fixed_rows, true_rows))].float()
            src_fixed, src_true = torch.arange(Q, device=device), torch.arange(Q, 2 * Q, device=device)
        else:
            source, src_fixed, src_true = table, fixed_rows, true_rows
        counts, scores = fused(model.rel_model, table, source, src_fixed, rel_w, rel_ids, q_head, ptr, rows,
                               true_row=src_true, filter=filt, want_scores=return_scores)
    else:
        dense_filt = None if filt is None else (filt.seg_lo, filt.seg_hi, filt.values, filt.exclude, filt.ent2idx)
        counts, scores = _rank_lists_dense(model.score_fn, table, table[fixed_rows].float(), rel_w[rel_ids],
                                           table[true_rows].float(), q_head, ptr, rows, 0, dense_filt, return_scores)
    if not include_true:
        counts[:, 1] += 1
        counts[:, 3] += 1
    if not return_scores:
        return counts
    return counts, (scores if rect is None else scores.reshape(rect.shape))


def _topk_lists_dense(score_fn, table, fixed, rel, q_head, k, ptr, rows, row_base, filt, max_bytes=1 << 28):
    """The dense route of predict_from_candidates: score_fn on the gathered rows of the lists, in query chunks of bounded
    bytes, the filter through _filtered_pairs, the order by _stable_topk on the chunk's lists padded to a rectangle.  CPU
    tensors, and the widths and k blp_topk_lists does not take; on CPU tensors it is the oracle of the fused route.
    fixed / rel: (Q, D) float32; ptr (Q + 1,), rows (nnz,) global rows (a multiset; entries outside [row_base, row_base + N)
    are skipped).  Returns (rows (Q, k) int64 global rows, scores (Q, k) float32)."""
    Q, (N, D) = fixed.shape[0], table.shape
    dev = table.device
    rows_out = torch.full((Q, k), -1, dtype=torch.int64, device=dev)
    scores_out = torch.full((Q, k), float("nan"), dtype=torch.float32, device=dev)
    budget = max(1, max_bytes // (12 * D))  # slots of the chunk's rectangle: three gathered (n, D) float32 operands at most
    ptr_host = ptr.tolist()
    lo = 0
    while lo < Q:
        hi, width = lo + 1, ptr_host[lo + 1] - ptr_host[lo]
        while hi < Q and (hi + 1 - lo) * max(width, ptr_host[hi + 1] - ptr_host[hi]) <= budget:
            width = max(width, ptr_host[hi + 1] - ptr_host[hi])
            hi += 1
        p0, p1 = ptr_host[lo], ptr_host[hi]
        if p1 > p0:
            n_per = ptr[lo + 1:hi + 1] - ptr[lo:hi]
            owner = torch.repeat_interleave(torch.arange(hi - lo, device=dev), n_per, output_size=p1 - p0)
            local = rows[p0:p1] - row_base
            valid = (local >= 0) & (local < N)
            safe = torch.where(valid, local, torch.zeros_like(local))
            e = table[safe].float() if N else table.new_zeros((p1 - p0, D)).float()
            f, r = fixed[lo:hi][owner], rel[lo:hi][owner]
            is_head = owner < q_head - lo
            s = torch.empty((p1 - p0,), dtype=torch.float32, device=dev)
            if bool(is_head.any()):
                s[is_head] = score_fn(e[is_head], f[is_head], r[is_head])
            if bool((~is_head).any()):
                s[~is_head] = score_fn(f[~is_head], e[~is_head], r[~is_head])
            f_owner, f_local = _filtered_pairs(filt, lo, hi, row_base, N, dev)
            span = max(N, 1)
            gone = torch.isin(owner * span + safe, f_owner * span + f_local)
            col = torch.arange(p1 - p0, device=dev) - (ptr[lo:hi] - p0)[owner]
            shape = (hi - lo, width)
            r_rect = torch.full(shape, -1, dtype=torch.int64, device=dev)
            s_rect = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
            g_rect = torch.zeros(shape, dtype=torch.bool, device=dev)
            r_rect[owner, col] = torch.where(valid, local + row_base, torch.full_like(local, -1))
            s_rect[owner, col] = s
            g_rect[owner, col] = gone
            rows_out[lo:hi], scores_out[lo:hi] = _stable_topk(s_rect, r_rect, g_rect, k)
        lo = hi
    return rows_out, scores_out


def predict_from_candidates(model, table, triples, k, candidates, ent2idx, *, side="both", filter_index=None,
                            candidates_are="rows", entities=None, unique=False):
    """predict_links over a candidate list of each query's own -- what a first stage (BM25, a type index, an ANN probe) hands
    over for re-ranking: for every triple (head, tail, rel) of ``triples`` (T, 3) the k entries of the query's list the model
    scores highest as the replaced entity, known edges removed.  Only the listed rows are read.
    triples      ``side`` "head": (?, r, t); "tail": (h, r, ?); "both": Q = 2 T queries in predict_links' order [heads | tails]
    candidates   (Q, C) int64, padded with -1, or a CSR pair (ptr (Q + 1,), rows (nnz,)); table rows, or entity ids mapped
                 through ``ent2idx`` with candidates_are="ids" (an id without a row is skipped) -- rank_candidates' forms.  A
                 list is a multiset: a row listed twice may come back twice (adjacent, same score) unless ``unique``
    ent2idx      utils.make_ent2idx map (entity id -> table row); the fixed entity of every query must have a row
    filter_index utils.FilterIndex of the known edges: the rows it names are removed, every copy, not demoted (the entity at
                 the replaced position is never removed: pass -1 there to have every known edge filtered)
    entities     optional (num_entities,) entity id of every table row: ids instead of rows are returned
    unique       True: duplicate rows within a list are dropped (torch ops) before the call
    Returns predict_links' result, (rows or ids (Q, k) int64, scores (Q, k) float32): descending score, ties by ascending row,
    NaN last; -1 / NaN beyond the entries of the list that are left.  Scores are score_fn's values bit for bit (of the table
    widened to float32).  A float32, float16 or bfloat16 HIP table at a width blp_topk_lists takes and k <= 256 goes through
    it (a 16-bit table is read as it is, only the Q fixed rows are gathered and widened); CPU tensors, other widths and
    k > 256 take the dense route: score_fn on gathered rows and a stable sort."""
    model = _module(model)
    if side not in ("head", "tail", "both"):
        raise ValueError(f"side must be 'head', 'tail' or 'both', got {side!r}")
    if candidates_are not in ("rows", "ids"):
        raise ValueError(f"candidates_are must be 'rows' or 'ids', got {candidates_are!r}")
    k = int(k)
    if k < 1:
        raise ValueError(f"k = {k} must be >= 1")
    device = table.device
    N, D = table.shape
    triples = triples.to(device=device, dtype=torch.long).reshape(-1, 3)
    ent2idx = ent2idx.to(device=device, dtype=torch.long)
    T = triples.shape[0]
    h, t, r = triples[:, 0], triples[:, 1], triples[:, 2]
    heads, tails = side in ("head", "both"), side in ("tail", "both")
    q_head = T if heads else 0
    fixed_ids = torch.cat([x for x, on in ((t, heads), (h, tails)) if on])
    rel_ids = torch.cat([r] * (int(heads) + int(tails)))
    Q = fixed_ids.shape[0]

    def to_rows(ids):
        known = (ids >= 0) & (ids < ent2idx.shape[0])
        return torch.where(known, ent2idx[torch.where(known, ids, torch.zeros_like(ids))], torch.full_like(ids, -1))

    fixed_rows = to_rows(fixed_ids)
    rel_w = model.rel_emb.weight.detach()
    if Q and bool(((fixed_rows < 0) | (fixed_rows >= N) | (rel_ids < 0) | (rel_ids >= rel_w.shape[0])).any()):
        raise ValueError("predict_from_candidates: a query's fixed entity has no table row, or its relation is out of range")
    if isinstance(candidates, (tuple, list)):
        ptr, rows = (x.to(device=device, dtype=torch.long).reshape(-1) for x in candidates)
        if ptr.shape[0] != Q + 1:
            raise ValueError(f"candidates: ptr must have Q + 1 = {Q + 1} entries, got {ptr.shape[0]}")
    else:
        rect = candidates.to(device=device, dtype=torch.long)
        if rect.dim() != 2 or rect.shape[0] != Q:
            raise ValueError(f"candidates must be (Q, C) with Q = {Q}, got {tuple(rect.shape)}")
        ptr = torch.arange(Q + 1, device=device, dtype=torch.long) * rect.shape[1]
        rows = rect.reshape(-1)
    if candidates_are == "ids":
        rows = to_rows(rows)
    if Q == 0:
        return torch.empty((0, k), dtype=torch.int64, device=device), torch.empty((0, k), dtype=torch.float32, device=device)
    if unique and rows.numel():
        # one entry per (query, row): the pairs as single integers, sorted and de-duplicated; entries without a row of the
        # table would be skipped anyway and are dropped here
        owner = torch.repeat_interleave(torch.arange(Q, device=device), ptr[1:] - ptr[:-1], output_size=rows.shape[0])
        ok = (rows >= 0) & (rows < N)
        pairs = torch.unique(owner[ok] * max(N, 1) + rows[ok])
        rows = pairs % max(N, 1)
        ptr = torch.cat((ptr.new_zeros(1), torch.cumsum(torch.bincount(pairs // max(N, 1), minlength=Q), 0)))
    filt = None
    if filter_index is not None:
        seg = filter_index.segments(triples, ent2idx, device)
        sel = torch.cat([x for x, on in ((torch.arange(T, device=device), heads), (torch.arange(T, 2 * T, device=device), tails)) if on])
        filt = ops.SegmentFilter(seg.seg_lo[sel].contiguous(), seg.seg_hi[sel].contiguous(), seg.values,
                                 seg.exclude[sel].contiguous(), seg.ent2idx, 0)
    if table.is_cuda and k <= 256 and ops.topk_lists_supported(model.rel_model, D, k, table.dtype):
        if table.dtype != torch.float32:  # float32 query vectors: the Q fixed rows, gathered and widened (exact)
            source, src_fixed = table[fixed_rows].float(), torch.arange(Q, device=device)
        else:
            source, src_fixed = table, fixed_rows
        out_rows, scores = ops.topk_lists(model.rel_model, table, source, src_fixed, rel_w, rel_ids, q_head, ptr, rows, k,
                                          filter=filt)
    else:
        dense_filt = None if filt is None else (filt.seg_lo, filt.seg_hi, filt.values, filt.exclude, filt.ent2idx)
        out_rows, scores = _topk_lists_dense(model.score_fn, table, table[fixed_rows].float(), rel_w[rel_ids], q_head, k, ptr,
                                             rows, 0, dense_filt)
    if entities is not None:
        entities = entities.to(device=device, dtype=torch.long)
        out_rows = torch.where(out_rows >= 0, entities[out_rows.clamp(min=0)], out_rows)
    return out_rows, scores


# ----------------------------------------------------------------------------------- relation prediction: (h, ?, t)
def _relation_scores_dense(score_fn, head_vecs, tail_vecs, rel_w, max_bytes=1 << 28):
    """The reference's route for (h, ?, t): score_fn broadcast over every relation, in query pieces whose (piece, R, D)
    intermediate stays within ``max_bytes``.  Yields (lo, hi, (hi - lo, R) scores)."""
    Q, (R, D) = head_vecs.shape[0], rel_w.shape
    piece = max(1, min(max(Q, 1), max_bytes // max(4 * R * D, 1)))
    rels = rel_w.unsqueeze(0)
    for lo in range(0, Q, piece):
        hi = min(lo + piece, Q)
        yield lo, hi, score_fn(head_vecs[lo:hi].unsqueeze(1), tail_vecs[lo:hi].unsqueeze(1), rels)


def _relation_queries(model, table, triples, ent2idx, who, min_cols):
    """(triples on the table's device, head rows, tail rows, rel_emb weight) of a relation-prediction call."""
    device = table.device
    triples = triples.to(device=device, dtype=torch.long)
    if triples.dim() != 2 or not min_cols <= triples.shape[1] <= 3:
        raise ValueError(f"{who}: rows of {'(head, tail, rel)' if min_cols == 3 else '(head, tail) or (head, tail, rel)'} "
                         f"entity ids expected, got shape {tuple(triples.shape)}")
    ent2idx = ent2idx.to(device=device, dtype=torch.long)
    ids = triples[:, :2]
    known = (ids >= 0) & (ids < ent2idx.shape[0])
    rows = torch.where(known, ent2idx[torch.where(known, ids, torch.zeros_like(ids))], torch.full_like(ids, -1))
    rel_w = model.rel_emb.weight.detach()
    if triples.shape[0] and bool(((rows < 0) | (rows >= table.shape[0])).any()):
        raise ValueError(f"{who}: an entity of a pair has no table row")
    if triples.shape[1] == 3 and triples.shape[0]:
        r = triples[:, 2]
        if bool((r >= rel_w.shape[0]).any()) or (min_cols == 3 and bool((r < 0).any())):
            raise ValueError(f"{who}: a relation id is out of range")
    return triples, rows[:, 0].contiguous(), rows[:, 1].contiguous(), rel_w


def _relation_source(table, triples, ent2idx, head_rows, tail_rows):
    """The f32 source of the fused route: the table itself, or -- a 16-bit table -- its 2 T query rows gathered and widened."""
    if table.dtype == torch.float32:
        return table, head_rows, tail_rows
    T = triples.shape[0]
    if triples.shape[1] == 2:  # (the gather reads (head, tail, rel) rows)
        triples = torch.cat((triples, torch.zeros_like(triples[:, :1])), 1)
    both = ops.gather_triple_vectors(triples, ent2idx.to(device=table.device, dtype=torch.long), table)
    at = torch.arange(T, device=table.device)
    return both, at, at + T


def rank_relations(model, table, triples, ent2idx, *, filter_index=None, return_scores=False):
    """Rank the true relation of every triple (head, tail, rel) of ``triples`` (T, 3) entity / relation ids among ALL relations
    of the model, for the pair (head, ?, tail).
    table        (N, D) entity table (build_entity_table), float32 / float16 / bfloat16 (16-bit rows are widened exactly)
    ent2idx      utils.make_ent2idx map; both entities of every triple must have a row
    filter_index utils.RelationFilterIndex of the known edges: the other known relations of the pair leave the filtered counts
    Returns counts (T, 4) int32 = {gt, ge, gt_filt, ge_filt} -- relations scoring above / at least the true one, IEEE
    comparison, the true relation itself included in ge; metrics_from_counts applies unchanged -- and, with ``return_scores``,
    the (T, R) score_fn values bit for bit.  HIP tensors at a width blp_rank_relations takes (64 / 128 / 256), or at any other
    width D % 4 == 0, 4 <= D <= 1024 (the BOW / DKRL 300 and 768) -- blp_rank_relations_wide for a TransE model,
    blp_rank_relations_wide_bilinear for DistMult / ComplEx / SimplE: the fused kernel (no (T, R) matrix unless asked for); CPU
    tensors and everything else: score_fn broadcast over the relations in bounded pieces.  The fused kernels give the C
    oracle's bits (torch's sum(dim=-1) order of a single score); the routes give the same bits wherever the CPU dense route
    equals the oracle.  One exception is known: ComplEx / SimplE at D = 12, where torch's broadcast reduction adds the 6 terms
    in another order than its reduction of one row (tests/test_rank_relations_wide_bilinear_host.py pins it)."""
    model = _module(model)
    triples, head_rows, tail_rows, rel_w = _relation_queries(model, table, triples, ent2idx, "rank_relations", 3)
    device, T, R = table.device, triples.shape[0], rel_w.shape[0]
    filt = filter_index.segments(triples, device) if filter_index is not None and T else None
    fused = None
    if table.is_cuda and ops.rank_relations_supported(model.rel_model, table.shape[1]):
        fused = ops.rank_relations
    elif table.is_cuda and ops.rank_relations_wide_supported(model.rel_model, table.shape[1]):
        fused = ops.rank_relations_wide
    elif table.is_cuda and ops.rank_relations_wide_bilinear_supported(model.rel_model, table.shape[1]):
        fused = ops.rank_relations_wide_bilinear
    if fused is not None:
        source, hr, tr = _relation_source(table, triples, ent2idx, head_rows, tail_rows)
        return fused(model.rel_model, source, hr, tr, rel_w, triples[:, 2].contiguous(), filter=filt, return_scores=return_scores)
    counts = torch.empty((T, 4), dtype=torch.int32, device=device)
    scores = torch.empty((T, R), dtype=torch.float32, device=device) if return_scores else None
    dense_filt = None if filt is None else (filt.seg_lo, filt.seg_hi, filt.values, filt.exclude, None)
    for lo, hi, s in _relation_scores_dense(model.score_fn, table[head_rows].float(), table[tail_rows].float(), rel_w):
        kt = s.gather(1, triples[lo:hi, 2:3])
        kept = torch.ones(s.shape, dtype=torch.bool, device=device)
        owner, local = _filtered_pairs(dense_filt, lo, hi, 0, R, device)
        kept[owner, local] = False
        gt, ge = s > kt, s >= kt
        counts[lo:hi] = torch.stack((gt.sum(1), ge.sum(1), (gt & kept).sum(1), (ge & kept).sum(1)), 1).to(torch.int32)
        if return_scores:
            scores[lo:hi] = s
    return (counts, scores) if return_scores else counts


def predict_relations(model, table, pairs, k, ent2idx, *, filter_index=None):
    """Answer (head, ?, tail): for every row of ``pairs`` -- (head, tail) or (head, tail, rel) entity ids -- the k relations
    the model scores highest.  ``filter_index`` (utils.RelationFilterIndex of the known edges): the known relations of the pair
    are REMOVED, except the row's third column when there is one (-1 there removes every known relation, as two columns do).
    Returns (rels (T, k) int64, scores (T, k) float32): descending score, ties by ascending relation id, NaN last; -1 / NaN
    beyond the relations left (k may exceed R).  Scores are score_fn's values bit for bit.  HIP tensors at a width
    blp_topk_relations takes -- or at any other D % 4 == 0, 4 <= D <= 1024: blp_topk_relations_wide for a TransE model,
    blp_topk_relations_wide_bilinear for DistMult / ComplEx / SimplE -- and k <= 256: the fused kernel; otherwise (CPU tensors,
    k > 256) score_fn broadcast in bounded pieces + the stable order.  The routes give the same bits wherever the CPU dense
    route equals the C oracle (rank_relations names the one known exception, ComplEx / SimplE at D = 12)."""
    model = _module(model)
    k = int(k)
    if k < 1:
        raise ValueError(f"k = {k} must be >= 1")
    pairs, head_rows, tail_rows, rel_w = _relation_queries(model, table, pairs, ent2idx, "predict_relations", 2)
    device, T, R = table.device, pairs.shape[0], rel_w.shape[0]
    filt = filter_index.segments(pairs, device) if filter_index is not None and T else None
    fused = None
    if table.is_cuda and ops.topk_relations_supported(model.rel_model, table.shape[1], k):
        fused = ops.topk_relations
    elif table.is_cuda and ops.topk_relations_wide_supported(model.rel_model, table.shape[1], k):
        fused = ops.topk_relations_wide
    elif table.is_cuda and ops.topk_relations_wide_bilinear_supported(model.rel_model, table.shape[1], k):
        fused = ops.topk_relations_wide_bilinear
    if fused is not None:
        source, hr, tr = _relation_source(table, pairs, ent2idx, head_rows, tail_rows)
        return fused(model.rel_model, source, hr, tr, rel_w, k, filter=filt)
    rels_out = torch.empty((T, k), dtype=torch.int64, device=device)
    scores_out = torch.empty((T, k), dtype=torch.float32, device=device)
    dense_filt = None if filt is None else (filt.seg_lo, filt.seg_hi, filt.values, filt.exclude, None)
    ids = torch.arange(R, device=device, dtype=torch.int64)
    for lo, hi, s in _relation_scores_dense(model.score_fn, table[head_rows].float(), table[tail_rows].float(), rel_w):
        removed = torch.zeros(s.shape, dtype=torch.bool, device=device)
        owner, local = _filtered_pairs(dense_filt, lo, hi, 0, R, device)
        removed[owner, local] = True
        rels_out[lo:hi], scores_out[lo:hi] = _stable_topk(s, ids.expand(hi - lo, R), removed, k)
    return rels_out, scores_out


# ----------------------------------------------------------------------------------- candidate sets shared between queries
def _sets_from_pairs(owner, rows, num_sets):
    """(ptr (G + 1,), rows (nnz,)) of the sets {rows[i] : owner[i] == g}: each set sorted ascending, duplicates dropped."""
    span = int(rows.max()) + 1 if rows.numel() else 1
    keys = torch.unique(owner * span + rows)  # sorted: by set, then by row
    counts = torch.bincount(torch.div(keys, span, rounding_mode="floor"), minlength=num_sets)
    ptr = torch.zeros(num_sets + 1, dtype=torch.long, device=rows.device)
    ptr[1:] = torch.cumsum(counts, 0)
    return ptr, keys % span


class CandidateSets:
    """G candidate sets of table rows that queries share (rank_in_sets), held as a CSR: ``ptr`` (G + 1,) and ``rows`` (nnz,)
    int64, the rows of a set ascending and without duplicates -- a set is a set.  Built from
      * a sequence of G sets, each a Python list or a 1-D tensor of rows, in any order, duplicates allowed;
      * a padded rectangle: a (G, C) tensor, negative entries are padding;
      * a CSR: CandidateSets(ptr=..., rows=...) (sorted and de-duplicated per set like the others).
    Sorted, de-duplicated and validated once, here: a negative row (outside a rectangle's padding), a row >= ``num_rows`` (if
    given) or a ptr that is not a non-decreasing run from 0 to len(rows) raises ValueError."""

    def __init__(self, sets=None, *, ptr=None, rows=None, num_rows=None, device=None):
        if (sets is None) == (ptr is None) or (ptr is None) != (rows is None):
            raise ValueError("CandidateSets: give either the sets (a sequence of sets or a padded (G, C) tensor) or ptr and rows")
        if sets is not None and isinstance(sets, torch.Tensor):
            if sets.dim() != 2 or sets.dtype.is_floating_point or sets.dtype is torch.bool:
                raise ValueError("CandidateSets: a tensor must be a padded (G, C) rectangle of integer rows")
            rect = sets.to(torch.long)
            G = rect.shape[0]
            owner = torch.arange(G, device=rect.device).unsqueeze(1).expand_as(rect)[rect >= 0]
            flat = rect[rect >= 0]
        elif sets is not None:
            parts = [torch.as_tensor(s, dtype=torch.long).reshape(-1) for s in sets]
            G = len(parts)
            dev0 = parts[0].device if parts else torch.device("cpu")
            flat = torch.cat(parts) if parts else torch.empty(0, dtype=torch.long)
            owner = torch.repeat_interleave(torch.arange(G, device=dev0), torch.tensor([p.numel() for p in parts], dtype=torch.long, device=dev0)) \
                if parts else flat
        else:
            ptr = torch.as_tensor(ptr).reshape(-1)
            flat = torch.as_tensor(rows).reshape(-1)
            if ptr.dtype.is_floating_point or flat.dtype.is_floating_point:
                raise ValueError("CandidateSets: ptr and rows must be integer tensors")
            ptr, flat = ptr.to(torch.long), flat.to(device=ptr.device, dtype=torch.long)
            G = ptr.shape[0] - 1
            if G < 0 or int(ptr[0]) != 0 or int(ptr[-1]) != flat.shape[0] or bool((ptr[1:] < ptr[:-1]).any()):
                raise ValueError("CandidateSets: ptr must run from 0 to len(rows) without decreasing")
            owner = torch.repeat_interleave(torch.arange(G, device=ptr.device), ptr[1:] - ptr[:-1], output_size=flat.shape[0])
        if flat.numel() and int(flat.min()) < 0:
            raise ValueError("CandidateSets: negative row")
        if num_rows is not None and flat.numel() and int(flat.max()) >= int(num_rows):
            raise ValueError(f"CandidateSets: row {int(flat.max())} outside the table of {int(num_rows)} rows")
        self.ptr, self.rows = _sets_from_pairs(owner, flat, G)
        if device is not None:
            self.ptr, self.rows = self.ptr.to(device), self.rows.to(device)

    @property
    def num_sets(self):
        return self.ptr.shape[0] - 1

    def to(self, device):
        return _SetsView(self.ptr.to(device), self.rows.to(device))

    def tolist(self):
        p, r = self.ptr.tolist(), self.rows.tolist()
        return [r[p[g]:p[g + 1]] for g in range(len(p) - 1)]

    def contains(self, set_ids, rows):
        """(n,) bool: is rows[i] in set set_ids[i]?  (searchsorted over the CSR, whose (set, row) keys ascend)"""
        if not self.rows.numel():
            return torch.zeros(rows.shape, dtype=torch.bool, device=rows.device)
        span = max(int(self.rows.max()), int(rows.max()) if rows.numel() else 0) + 1
        owner = torch.repeat_interleave(torch.arange(self.num_sets, device=self.rows.device), self.ptr[1:] - self.ptr[:-1],
                                        output_size=self.rows.shape[0])
        keys, want = owner * span + self.rows, set_ids * span + rows
        pos = torch.searchsorted(keys, want).clamp(max=keys.shape[0] - 1)
        return (keys[pos] == want) & (rows >= 0)


class _SetsView(CandidateSets):
    """A CandidateSets over tensors that are already a valid CSR (no second normalisation)."""

    def __init__(self, ptr, rows):
        self.ptr, self.rows = ptr, rows


def relation_candidate_sets(graph_triples, num_relations, ent2idx):
    """The candidate sets of type-constrained evaluation, 2 R of them: set r = the table rows of the entities seen as HEAD of
    relation r in ``graph_triples`` ((T, 3): head, tail, rel) -- the relation's domain --, set R + r = those seen as its TAIL
    (its range).  Ids without a row in ``ent2idx`` are dropped.  Torch ops only: CPU or device, wherever the triples are."""
    R = int(num_relations)
    triples = graph_triples.to(torch.long).reshape(-1, 3)
    ent2idx = ent2idx.to(device=triples.device, dtype=torch.long)
    ids = torch.cat((triples[:, 0], triples[:, 1]))
    owner = torch.cat((triples[:, 2], triples[:, 2] + R))
    if owner.numel() and (int(triples[:, 2].min()) < 0 or int(triples[:, 2].max()) >= R):
        raise ValueError(f"relation_candidate_sets: a relation outside [0, {R})")
    known = (ids >= 0) & (ids < ent2idx.shape[0])
    rows = torch.where(known, ent2idx[torch.where(known, ids, torch.zeros_like(ids))], torch.full_like(ids, -1))
    return _SetsView(*_sets_from_pairs(owner[rows >= 0], rows[rows >= 0], 2 * R))


def _rank_sets_dense(score_fn, table, fixed, rel, true_vec, q_head, set_ptr, set_rows, qptr_head, qptr_tail, row_base, filt,
                     max_bytes=1 << 28):
    """The dense route of rank_in_sets: score_fn of each set's gathered rows against its group's queries, in (row slab, query
    chunk) pieces of bounded bytes, the comparisons against the true score, the filter through _filtered_pairs (an entry counts
    only if its row is in the set).  Queries grouped by set within each side, as blp_rank_sets takes them; fixed / rel /
    true_vec (Q, D) float32.  CPU tensors and the widths and table dtypes blp_rank_sets_typed does not take; on CPU tensors it is the oracle
    of the fused route.  Returns counts (Q, 4) int32."""
    Q, (N, D) = fixed.shape[0], table.shape
    dev = table.device
    acc = torch.zeros((Q, 4), dtype=torch.int64, device=dev)
    true = torch.cat((score_fn(true_vec[:q_head], fixed[:q_head], rel[:q_head]), score_fn(fixed[q_head:], true_vec[q_head:], rel[q_head:])))
    budget = max(1, max_bytes // (12 * D))  # (row, query) pairs per piece: three (pairs, D) float32 operands
    sp, qh, qt = set_ptr.tolist(), qptr_head.tolist(), qptr_tail.tolist()
    for g in range(len(sp) - 1):
        local = set_rows[sp[g]:sp[g + 1]] - row_base
        local = local[(local >= 0) & (local < N)]
        runs = [(head, a, b) for head, a, b in ((True, qh[g], qh[g + 1]), (False, q_head + qt[g], q_head + qt[g + 1])) if a < b]
        if not local.numel() or not runs:
            continue
        for r0 in range(0, local.shape[0], budget):
            rows = local[r0:r0 + budget]
            n = rows.shape[0]
            e = table[rows].float()
            step = max(1, budget // n)
            for head, a, b in runs:
                for lo in range(a, b, step):
                    hi = min(lo + step, b)
                    c = hi - lo
                    ee = e.unsqueeze(0).expand(c, n, D).reshape(c * n, D)
                    ff = fixed[lo:hi].unsqueeze(1).expand(c, n, D).reshape(c * n, D)
                    rr = rel[lo:hi].unsqueeze(1).expand(c, n, D).reshape(c * n, D)
                    s = (score_fn(ee, ff, rr) if head else score_fn(ff, ee, rr)).reshape(c, n)
                    kt = true[lo:hi].unsqueeze(1)
                    gt, ge = s > kt, s >= kt
                    keep = torch.ones_like(gt)
                    f_owner, f_local = _filtered_pairs(filt, lo, hi, row_base, N, dev)
                    if f_owner.numel():
                        pos = torch.searchsorted(rows, f_local).clamp(max=n - 1)
                        hit = rows[pos] == f_local
                        keep[f_owner[hit], pos[hit]] = False
                    for col, mask in enumerate((gt, ge, gt & keep, ge & keep)):
                        acc[lo:hi, col] += mask.sum(1)
    return acc.to(torch.int32)


def _group_by_set(set_ids, q_head, num_sets):
    """The queries of each side grouped by set (stable: a group keeps the caller's order): (perm (Q,), qptr_head (G + 1,),
    qptr_tail (G + 1,)) -- grouped query i is the caller's query perm[i]; the runs as blp_rank_sets takes them."""
    device = set_ids.device
    order_h = torch.sort(set_ids[:q_head], stable=True).indices
    order_t = torch.sort(set_ids[q_head:], stable=True).indices + q_head
    qptr_head = torch.zeros(num_sets + 1, dtype=torch.long, device=device)
    qptr_tail = torch.zeros(num_sets + 1, dtype=torch.long, device=device)
    qptr_head[1:] = torch.cumsum(torch.bincount(set_ids[:q_head], minlength=num_sets), 0)
    qptr_tail[1:] = torch.cumsum(torch.bincount(set_ids[q_head:], minlength=num_sets), 0)
    return torch.cat((order_h, order_t)), qptr_head, qptr_tail


def rank_in_sets(model, table, triples, sets, ent2idx, *, set_ids=None, side="both", filter_index=None, add_true=True):
    """Rank every triple's true entity against a candidate SET that it shares with other queries -- type-constrained
    evaluation (the default: a head query of relation r against set r, a tail query against set R + r of
    relation_candidate_sets), per-type or per-language pools, one first-stage pool per group of queries.
    triples      (T, 3) (head, tail, rel); ``side`` "head": (?, r, t); "tail": (h, r, ?); "both": Q = 2 T queries in
                 predict_links' order [heads | tails]
    sets         CandidateSets of table rows
    set_ids      (Q,) the set of every query, in that order; an id outside [0, G) raises ValueError
    ent2idx      utils.make_ent2idx map (entity id -> table row); the fixed and the true entity of a query must have a row
    filter_index utils.FilterIndex of the known edges: the filtered columns leave out the entries of the set it removes (the
                 triple's own entity is never removed)
    add_true     True: a query whose true entity is not in its set gets 1 added to both ``ge`` columns -- the true entity always
                 competes and ties with itself, so metrics_from_counts applies unchanged; False: the counts over the set as it is
    Returns counts (Q, 4) int32 {gt, ge, gt_filtered, ge_filtered} in the caller's order.
    A float32, float16 or bfloat16 HIP table at 64 / 128 / 256 goes through blp_rank_sets / blp_rank_sets_typed (every row of a
    set is fetched once per chunk of 128 queries of its group; a 16-bit table is read as it is, only the Q fixed and the Q true
    rows are gathered and widened).  A HIP table at any other width blp_rank_sets_wide takes -- TransE, D % 4 == 0, 4 <= D <= 1024:
    the BOW / DKRL 300 and 768 -- goes through blp_rank_sets_wide (a row of a set fetched once per chunk of 16 queries of its
    group; the same counts, a 16-bit table handled the same way).  A float32 HIP table of DistMult / ComplEx / SimplE at those
    widths goes through blp_rank_sets_wide_bilinear (a row of a set fetched once per chunk of 8 queries of one side of its
    group; the same counts).  CPU tensors, and 16-bit tables of the bilinear models at other widths than 64 / 128 / 256, take
    the dense route: score_fn on gathered rows."""
    model = _module(model)
    if side not in ("head", "tail", "both"):
        raise ValueError(f"side must be 'head', 'tail' or 'both', got {side!r}")
    device = table.device
    N, D = table.shape
    triples = triples.to(device=device, dtype=torch.long).reshape(-1, 3)
    ent2idx = ent2idx.to(device=device, dtype=torch.long)
    T = triples.shape[0]
    h, t, r = triples[:, 0], triples[:, 1], triples[:, 2]
    heads, tails = side in ("head", "both"), side in ("tail", "both")
    q_head = T if heads else 0
    fixed_ids = torch.cat([x for x, on in ((t, heads), (h, tails)) if on])
    true_ids = torch.cat([x for x, on in ((h, heads), (t, tails)) if on])
    rel_ids = torch.cat([r] * (int(heads) + int(tails)))
    Q = fixed_ids.shape[0]

    def to_rows(ids):
        known = (ids >= 0) & (ids < ent2idx.shape[0])
        return torch.where(known, ent2idx[torch.where(known, ids, torch.zeros_like(ids))], torch.full_like(ids, -1))

    fixed_rows, true_rows = to_rows(fixed_ids), to_rows(true_ids)
    rel_w = model.rel_emb.weight.detach()
    R = rel_w.shape[0]
    if Q and bool(((fixed_rows < 0) | (fixed_rows >= N) | (true_rows < 0) | (true_rows >= N) | (rel_ids < 0) | (rel_ids >= R)).any()):
        raise ValueError("rank_in_sets: a query's fixed or true entity has no table row, or its relation is out of range")
    set_ptr, set_rows = sets.ptr.to(device), sets.rows.to(device)
    G = set_ptr.shape[0] - 1
    if set_rows.numel() and int(set_rows.max()) >= N:
        raise ValueError(f"rank_in_sets: the sets name row {int(set_rows.max())}, the table has {N} rows")
    if set_ids is None:
        set_ids = torch.cat([x for x, on in ((r, heads), (r + R, tails)) if on])
    set_ids = set_ids.to(device=device, dtype=torch.long).reshape(-1)
    if set_ids.shape[0] != Q:
        raise ValueError(f"set_ids needs one entry per query ({Q}), got {set_ids.shape[0]}")
    if Q and (int(set_ids.min()) < 0 or int(set_ids.max()) >= G):
        raise ValueError(f"rank_in_sets: a set id outside [0, {G})")
    perm, qptr_head, qptr_tail = _group_by_set(set_ids, q_head, G)
    g_fixed, g_true, g_rel = fixed_rows[perm], true_rows[perm], rel_ids[perm]
    filt = None
    if filter_index is not None and Q:
        seg = filter_index.segments(triples, ent2idx, device)
        sel = torch.cat([x for x, on in ((torch.arange(T, device=device), heads), (torch.arange(T, 2 * T, device=device), tails)) if on])[perm]
        filt = ops.SegmentFilter(seg.seg_lo[sel].contiguous(), seg.seg_hi[sel].contiguous(), seg.values,
                                 seg.exclude[sel].contiguous(), seg.ent2idx, 0)
    if Q == 0:
        return torch.empty((0, 4), dtype=torch.int32, device=device)
    fused = None
    if table.is_cuda and ops.rank_sets_supported(model.rel_model, D, table.dtype):
        fused = ops.rank_sets
    elif table.is_cuda and ops.rank_sets_wide_supported(model.rel_model, D, table.dtype):
        fused = ops.rank_sets_wide
    elif table.is_cuda and ops.rank_sets_wide_bilinear_supported(model.rel_model, D, table.dtype):
        fused = ops.rank_sets_wide_bilinear
    if fused is not None:
        if table.dtype != torch.float32:
            # float32 query vectors: the Q fixed rows, then the Q true rows, gathered and widened (exact) by the library's own
            # kernel (blp_gather_triple_vectors: 64-bit offsets, a table of more than 2^31 bytes included)
            pairs = torch.stack((g_fixed, g_true, torch.zeros_like(g_fixed)), dim=1)
            source = ops.gather_triple_vectors(pairs, None, table)
            src_fixed, src_true = torch.arange(Q, device=device), torch.arange(Q, 2 * Q, device=device)
        else:
            source, src_fixed, src_true = table, g_fixed, g_true
        grouped = fused(model.rel_model, table, source, src_fixed, rel_w, g_rel, q_head, src_true, set_ptr, set_rows, qptr_head, qptr_tail,
                        filter=filt)
    else:
        dense_filt = None if filt is None else (filt.seg_lo, filt.seg_hi, filt.values, filt.exclude, filt.ent2idx)
        grouped = _rank_sets_dense(model.score_fn, table, table[g_fixed].float(), rel_w[g_rel], table[g_true].float(), q_head,
                                   set_ptr, set_rows, qptr_head, qptr_tail, 0, dense_filt)
    counts = torch.empty_like(grouped)
    counts[perm] = grouped
    if add_true:
        absent = ~_SetsView(set_ptr, set_rows).contains(set_ids, true_rows)
        counts[:, 1] += absent.to(torch.int32)
        counts[:, 3] += absent.to(torch.int32)
    return counts


# ----------------------------------------------------------------------------------- link prediction inside candidate sets
def _topk_sets_dense(score_fn, table, fixed, rel, q_head, k, set_ptr, set_rows, qptr_head, qptr_tail, row_base, filt,
                     max_bytes=1 << 28):
    """The dense route of predict_links_in_sets: score_fn of each set's gathered rows against its group's queries, in (query
    chunk, row slab) pieces of bounded bytes, the filter through _filtered_pairs, the order by _stable_topk.  Queries grouped by
    set within each side, as blp_topk_sets takes them; fixed / rel (Q, D) float32.  CPU tensors and the widths and k that
    neither blp_topk_sets / blp_topk_sets_typed nor blp_topk_sets_wide take (the bilinear models off 64 / 128 / 256, k > 256); on
    CPU tensors it is the oracle of the fused routes.  Returns (rows (Q, k) int64 global rows,
    scores (Q, k) float32)."""
    Q, (N, D) = fixed.shape[0], table.shape
    dev = table.device
    rows_out = torch.full((Q, k), -1, dtype=torch.int64, device=dev)
    scores_out = torch.full((Q, k), float("nan"), dtype=torch.float32, device=dev)
    budget = max(1, max_bytes // (12 * D))  # (row, query) pairs per piece: three (pairs, D) float32 operands
    sp, qh, qt = set_ptr.tolist(), qptr_head.tolist(), qptr_tail.tolist()
    for g in range(len(sp) - 1):
        local = set_rows[sp[g]:sp[g + 1]] - row_base
        local = local[(local >= 0) & (local < N)]
        n = local.shape[0]
        runs = [(head, a, b) for head, a, b in ((True, qh[g], qh[g + 1]), (False, q_head + qt[g], q_head + qt[g + 1])) if a < b]
        if not n or not runs:
            continue
        step = max(1, budget // n)  # queries per piece; a set longer than the budget goes through in row slabs
        slab = max(1, budget // step)
        for head, a, b in runs:
            for lo in range(a, b, step):
                hi = min(lo + step, b)
                c = hi - lo
                s = torch.empty((c, n), dtype=torch.float32, device=dev)
                for r0 in range(0, n, slab):
                    e = table[local[r0:r0 + slab]].float()
                    m = e.shape[0]
                    ee = e.unsqueeze(0).expand(c, m, D).reshape(c * m, D)
                    ff = fixed[lo:hi].unsqueeze(1).expand(c, m, D).reshape(c * m, D)
                    rr = rel[lo:hi].unsqueeze(1).expand(c, m, D).reshape(c * m, D)
                    s[:, r0:r0 + m] = (score_fn(ee, ff, rr) if head else score_fn(ff, ee, rr)).reshape(c, m)
                removed = torch.zeros((c, n), dtype=torch.bool, device=dev)
                f_owner, f_local = _filtered_pairs(filt, lo, hi, row_base, N, dev)
                if f_owner.numel():
                    pos = torch.searchsorted(local, f_local).clamp(max=n - 1)
                    hit = local[pos] == f_local
                    removed[f_owner[hit], pos[hit]] = True
                rows_out[lo:hi], scores_out[lo:hi] = _stable_topk(s, (local + row_base).expand(c, n), removed, k)
    return rows_out, scores_out


def predict_links_in_sets(model, table, triples, k, sets, ent2idx, *, set_ids=None, side="both", filter_index=None,
                          entities=None):
    """predict_links inside candidate SETS that queries share: for every triple (head, tail, rel) of ``triples`` (T, 3) the k
    rows of the query's set the model scores highest as the replaced entity -- "the 10 best tails of (h, r, ?) among the
    entities that can be a tail of r" (the default: a head query of relation r answers from set r, a tail query from set
    R + r of relation_candidate_sets), a first-stage pool re-ranked for a group of queries, per-language pools.
    triples      ``side`` "head": (?, r, t); "tail": (h, r, ?); "both": Q = 2 T queries in predict_links' order [heads | tails]
    sets         CandidateSets of table rows; set_ids (Q,) the set of every query, in that order (rank_in_sets' arguments)
    ent2idx      utils.make_ent2idx map (entity id -> table row); the fixed entity of every query must have a row
    filter_index utils.FilterIndex of the known edges: the rows it names are removed, not demoted (the entity at the replaced
                 position is never removed: pass -1 there to have every known edge filtered)
    entities     optional (num_entities,) entity id of every table row: ids instead of rows are returned
    Returns predict_links' result, (rows or ids (Q, k) int64, scores (Q, k) float32) in the caller's order: descending score,
    ties by ascending row, NaN last; -1 / NaN beyond the entries of the set that are left.  Scores are score_fn's values bit
    for bit (of the table widened to float32).  A float32, float16 or bfloat16 HIP table at 64 / 128 / 256 and k <= 256 goes
    through blp_topk_sets / blp_topk_sets_typed (a row of a set is fetched once per chunk of its group's queries; a 16-bit
    table is read as it is, only the Q fixed rows are gathered and widened).  A HIP table at any other width blp_topk_sets_wide
    takes -- TransE, D % 4 == 0, 4 <= D <= 1024: the BOW / DKRL 300 and 768 -- and k <= 256 goes through blp_topk_sets_wide (a row
    of a set fetched once per chunk of up to 16 queries of its group).  CPU tensors, the bilinear models at other widths and
    k > 256 take the dense route: score_fn on gathered rows and a stable sort."""
    model = _module(model)
    if side not in ("head", "tail", "both"):
        raise ValueError(f"side must be 'head', 'tail' or 'both', got {side!r}")
    k = int(k)
    if k < 1:
        raise ValueError(f"k = {k} must be >= 1")
    device = table.device
    N, D = table.shape
    triples = triples.to(device=device, dtype=torch.long).reshape(-1, 3)
    ent2idx = ent2idx.to(device=device, dtype=torch.long)
    T = triples.shape[0]
    h, t, r = triples[:, 0], triples[:, 1], triples[:, 2]
    heads, tails = side in ("head", "both"), side in ("tail", "both")
    q_head = T if heads else 0
    fixed_ids = torch.cat([x for x, on in ((t, heads), (h, tails)) if on])
    rel_ids = torch.cat([r] * (int(heads) + int(tails)))
    Q = fixed_ids.shape[0]
    known = (fixed_ids >= 0) & (fixed_ids < ent2idx.shape[0])
    fixed_rows = torch.where(known, ent2idx[torch.where(known, fixed_ids, torch.zeros_like(fixed_ids))], torch.full_like(fixed_ids, -1))
    rel_w = model.rel_emb.weight.detach()
    R = rel_w.shape[0]
    if Q and bool(((fixed_rows < 0) | (fixed_rows >= N) | (rel_ids < 0) | (rel_ids >= R)).any()):
        raise ValueError("predict_links_in_sets: a query's fixed entity has no table row, or its relation is out of range")
    set_ptr, set_rows = sets.ptr.to(device), sets.rows.to(device)
    G = set_ptr.shape[0] - 1
    if set_rows.numel() and int(set_rows.max()) >= N:
        raise ValueError(f"predict_links_in_sets: the sets name row {int(set_rows.max())}, the table has {N} rows")
    if set_ids is None:
        set_ids = torch.cat([x for x, on in ((r, heads), (r + R, tails)) if on])
    set_ids = set_ids.to(device=device, dtype=torch.long).reshape(-1)
    if set_ids.shape[0] != Q:
        raise ValueError(f"set_ids needs one entry per query ({Q}), got {set_ids.shape[0]}")
    if Q and (int(set_ids.min()) < 0 or int(set_ids.max()) >= G):
        raise ValueError(f"predict_links_in_sets: a set id outside [0, {G})")
    if Q == 0:
        return torch.empty((0, k), dtype=torch.int64, device=device), torch.empty((0, k), dtype=torch.float32, device=device)
    perm, qptr_head, qptr_tail = _group_by_set(set_ids, q_head, G)
    g_fixed, g_rel = fixed_rows[perm], rel_ids[perm]
    filt = None
    if filter_index is not None:
        seg = filter_index.segments(triples, ent2idx, device)
        sel = torch.cat([x for x, on in ((torch.arange(T, device=device), heads), (torch.arange(T, 2 * T, device=device), tails)) if on])[perm]
        filt = ops.SegmentFilter(seg.seg_lo[sel].contiguous(), seg.seg_hi[sel].contiguous(), seg.values,
                                 seg.exclude[sel].contiguous(), seg.ent2idx, 0)
    fused = None
    if table.is_cuda and k <= 256 and ops.topk_sets_supported(model.rel_model, D, k, table.dtype):
        fused = ops.topk_sets
    elif table.is_cuda and k <= 256 and ops.topk_sets_wide_supported(model.rel_model, D, k, table.dtype):
        fused = ops.topk_sets_wide
    if fused is not None:
        if table.dtype != torch.float32:
            # float32 query vectors: the Q fixed rows gathered and widened (exact) by the library's own kernel
            # (blp_gather_triple_vectors: 64-bit offsets, a table of more than 2^31 bytes included)
            pairs = torch.stack((g_fixed, g_fixed, torch.zeros_like(g_fixed)), dim=1)
            source, src_fixed = ops.gather_triple_vectors(pairs, None, table)[:Q], torch.arange(Q, device=device)
        else:
            source, src_fixed = table, g_fixed
        g_rows, g_scores = fused(model.rel_model, table, source, src_fixed, rel_w, g_rel, q_head, k, set_ptr, set_rows, qptr_head,
                                 qptr_tail, filter=filt)
    else:
        dense_filt = None if filt is None else (filt.seg_lo, filt.seg_hi, filt.values, filt.exclude, filt.ent2idx)
        g_rows, g_scores = _topk_sets_dense(model.score_fn, table, table[g_fixed].float(), rel_w[g_rel], q_head, k, set_ptr,
                                            set_rows, qptr_head, qptr_tail, 0, dense_filt)
    rows, scores = torch.empty_like(g_rows), torch.empty_like(g_scores)
    rows[perm], scores[perm] = g_rows, g_scores
    if entities is not None:
        entities = entities.to(device=device, dtype=torch.long)
        rows = torch.where(rows >= 0, entities[rows.clamp(min=0)], rows)
    return rows, scores


def _module(model):
    wrappers =(torch.nn.DataParallel, torch.nn.parallel.DistributedDataParallel)
    return model.module if isinstance(model, wrappers) else model


def _loader_triples(loader, max_num_batches):
    """Every triple the reference's loop ``for i, triples in enumerate(loader)`` would see before
    ``i == max_num_batches``.  A sequential default-collate DataLoader over a dataset that holds its
    triples as one tensor (data.GraphDataset and subclasses: the reference's eval loaders,
    train.py:124-128) is read as a slice instead of 800+ Python-level batches."""
    from torch.utils.data import SequentialSampler
    from torch.utils.data.dataloader import default_collate
    dataset = getattr(loader, "dataset", None)
    stored = getattr(dataset, "triples", None)
    batch_size = getattr(loader, "batch_size", None)
    if (isinstance(stored, torch.Tensor) and stored.dim() == 2 and batch_size
            and isinstance(getattr(loader, "sampler", None), SequentialSampler)
            and getattr(loader, "collate_fn", None) is default_collate and len(dataset) == stored.shape[0]):
        n = stored.shape[0]
        if getattr(loader, "drop_last", False):
            n = n // batch_size * batch_size
        if max_num_batches is not None:
            n = min(n, max_num_batches * batch_size)
        return stored[:n]
    batches = []
    for i, triples in enumerate(loader):
        if max_num_batches is not None and i == max_num_batches:
            break
        batches.append(triples)
    return torch.cat(batches) if batches else torch.zeros((0, 3), dtype=torch.long)


@torch.no_grad()
def build_entity_table(model, text_dataset, entities, emb_batch_size, device, log=None, rows=None):
    """train.py:96-121: encode ``entities`` (or the slice ``rows`` = (lo, hi) of them) in chunks of
    emb_batch_size into an (n, dim) f32 table, in the order of ``entities``."""
    lo, hi = rows if rows is not None else (0, entities.shape[0])
    n = hi - lo
    table = torch.zeros((n, model.dim), dtype=torch.float, device=device)
    num_iters = math.ceil(n / emb_batch_size) if n else 0
    report = max(1, math.ceil(0.2 * num_iters))
    for it, idx in enumerate(range(0, n, emb_batch_size)):
        batch_ents = entities[lo + idx: lo + min(idx + emb_batch_size, n)]
        if isinstance(model, models.InductiveLinkPrediction):
            text_tok, text_mask, _ = text_dataset.get_entity_description(batch_ents)
            # the model writes its rows itself: the BERT encoders fuse enc_linear + normalise + this assignment
            # (models.BertEmbeddingsLP.encode_into -> blp_project_rows); same values as model(tok, mask), train.py:109
            rows, tok, mask = table[idx: idx + batch_ents.shape[0]], text_tok.to(device), text_mask.to(device)
            if hasattr(model, "check_tokens"):  # (the fused bag-of-words / DKRL builds: their token-id check once per table, below)
                model.encode_into(rows, tok, mask, defer_check=True)
            else:
                model.encode_into(rows, tok, mask)
        else:
            table[idx: idx + batch_ents.shape[0]] = model(batch_ents.to(device))
        if log is not None and (it + 1) % report == 0:
            log.info(f"[{idx + batch_ents.shape[0]:,}/{n:,}]")
    if hasattr(model, "check_tokens"):  # the fused bag-of-words build leaves its token-id check on the device until here
        model.check_tokens()
    return table


def table16_everywhere(rel_model, dtype, num_entities, dim, num_triples, block_size, world, axis):
    """Whether EVERY rank's shard of an evaluation would stream a 16-bit copy of the table itself (ops.table16_is_read_directly),
    evaluated for all ranks' (rows, triples) from the shard layout alone -- so that every rank takes the same decision
    without an exchange.  A per-rank decision can differ between ranks (the last candidate shard is shorter and the
    library's routing has a row threshold): some ranks would then rank the rounded copy and others the float32 table,
    the summed counts would mix two inputs, and -- the copy deciding which collective replicates the queries' vectors
    (replicates_whole_table) -- the ranks could issue mismatched collectives and hang."""
    by_query = world > 1 and axis == "query"
    for r in range(max(world, 1)):
        lo, hi = (0, num_entities) if (world <= 1 or by_query) else shard_bounds(num_entities, world, r)
        t_lo, t_hi = shard_bounds(num_triples, world, r) if by_query else (0, num_triples)
        if not ops.table16_is_read_directly(rel_model, dtype, hi - lo, dim, t_hi - t_lo, block_size):
            return False
    return True


def _shard_of_evaluation(model, text_dataset, entities, emb_batch_size, device, _log, triples, ent2idx, index, *, group, world, rank,
                         shard_axis, block_size, rank_table_dtype):
    """What ONE rank (a process of a torch.distributed group, or a device thread of a multidevice.DeviceGroup) does of an
    evaluation: encode its rows of the entity table (train.py:96-121), rank the triples against them (rank_triples; the
    collectives of SURVEY.md 8e inside).  Returns (table -- this rank's rows, or all rows on the query axis --, axis,
    triples, counts (2T, 4) int32 of the WHOLE evaluation, ids_ok)."""
    num_entities, num_triples = entities.shape[0], triples.shape[0]
    lo, hi = shard_bounds(num_entities, world, rank)
    table = build_entity_table(model, text_dataset, entities, emb_batch_size, device, _log if rank == 0 else None, rows=(lo, hi))
    triples = triples.to(device)  # in loader order (train.py:128-131)
    axis = shard_axis if shard_axis != "auto" else choose_shard_axis(num_entities, table.shape[1], 2 * num_triples, world)
    if world > 1 and axis == "query":  # full table everywhere, each rank takes a slice of the triples
        table = all_gather_rows(table, num_entities, world, group)
    rank_table = table
    if rank_table_dtype not in (None, torch.float32) and table.is_cuda:
        if table16_everywhere(model.rel_model, rank_table_dtype, num_entities, table.shape[1], num_triples, block_size, world, axis):
            rank_table = table.to(rank_table_dtype)
        else:
            # (the library would widen a 16-bit copy back to float32: more memory and time than the float32 table and other
            #  metrics for nothing; and the reference's pass structure -- a table pass per eval batch -- only pays with it)
            block_size = max(block_size, 65536)
            if rank == 0:
                _log.info(f"rank_table_dtype={rank_table_dtype}: not used for this evaluation (dim {table.shape[1]}, {num_entities:,} rows "
                          f"on {world} rank(s): the library would widen a 16-bit copy back to float32); ranking the float32 table "
                          f"in blocks of {block_size:,} triples")
    triples, counts, ids_ok = rank_triples(model, rank_table, triples, ent2idx.to(device), index, num_entities=num_entities,
                                           group=group, world=world, rank=rank, axis=axis, block_size=block_size)
    return table, axis, triples, counts, ids_ok


@torch.no_grad()
def eval_link_prediction(model, triples_loader, text_dataset, entities, epoch, emb_batch_size, _run, _log,
                         prefix="", max_num_batches=None, filtering_graph=None, new_entities=None,
                         return_embeddings=False, device=None, group=None, block_size=65536, shard_axis="auto",
                         eval_mode=False, rank_table_dtype=None, devices=None):
    """Drop-in for train.eval_link_prediction (same positional arguments, metric names and return
    value).  ``device`` defaults to the model's device.  Several GPUs, two ways (both: SURVEY.md 8e -- every shard encodes
    and keeps its own rows, ONE all-gather of the int32 counts; ``shard_axis`` = "candidate" | "query" | "auto"):

      * ``devices`` = [device, ...]: THIS process, one Python thread per device -- the reference's own process model
        (nn.DataParallel, train.py:329-330,344).  Every thread gets a replica of the model, builds its row shard, ranks on its
        own stream; the counts are combined by RCCL calls issued for all devices from one thread (multidevice.DeviceGroup).
        A device may repeat (two shards on one GPU).  The metrics, and the returned table, live on devices[0].
      * ``group`` (or an initialised default process group): one PROCESS per device under torch.distributed.run.

    ``eval_mode``: the reference never leaves train mode (train.py:57-121 has no model.eval()), so its entity table is
    built with BERT's dropout active and its metrics differ run to run.  The default (False) keeps whatever mode the
    model is in -- the reference's behaviour, so that this function drops in without changing a result's law;
    ``eval_mode=True`` puts the encoder in eval mode for the table build and restores it afterwards (deterministic
    tables; train.py's config key ``eval_dropout=False``).

    ``rank_table_dtype`` (torch.float16 / torch.bfloat16; default None = the reference's float32): rank against a 16-bit COPY of
    the table ("emit fp16 copy").  A deliberate change of the INPUT, not of the arithmetic: the candidates are
    the rounded rows, scored in f32 in the reference's order (counts = the reference's on the rounded table, bit for bit).
    Honoured ONLY where it pays: at the reference's Wikidata5M batching (``block_size`` <= 4 triples per table pass, dim 128 /
    256, a table long enough for the streaming kernels ON EVERY RANK) the passes read the 16-bit rows themselves, half the
    bytes; for any other shape the float32 table is ranked in the default 65 536-triple blocks and a log line says so
    (train.py: ``rank_table_dtype=float16``).  The returned embeddings stay float32."""
    model = _module(model)
    if device is None:
        device = next(model.parameters()).device
    compute_filtered = filtering_graph is not None
    dataset = triples_loader.dataset
    if devices is not None and group is not None:
        raise ValueError("give `devices` (threads of this process) or `group` (a process group), not both")
    if devices is not None:
        threads = multidevice.DeviceGroup(devices)
        device = threads.devices[0]
    else:
        threads = None

    if isinstance(model, models.InductiveLinkPrediction):
        if compute_filtered:
            index = filtering_graph if isinstance(filtering_graph, utils.FilterIndex) else utils.FilterIndex(filtering_graph, device=device)
            max_ent_id = max(index.max_node, int(entities.max()))
        else:
            index, max_ent_id = None, int(entities.max())
        ent2idx = utils.make_ent2idx(entities, max_ent_id)
    else:
        entities = torch.arange(model.ent_emb.num_embeddings)
        ent2idx = entities
        index = None
        if compute_filtered:
            index = filtering_graph if isinstance(filtering_graph, utils.FilterIndex) else utils.FilterIndex(filtering_graph, device=device)
    num_entities = entities.shape[0]

    was_training = model.training
    if eval_mode:
        model.eval()
    triples = _loader_triples(triples_loader, max_num_batches)
    num_triples = triples.shape[0]
    common = dict(shard_axis=shard_axis, block_size=block_size, rank_table_dtype=rank_table_dtype)
    if threads is not None:
        # one replica per device thread, made here on the calling thread (a module is not copied while another thread runs it);
        # the model itself serves the first thread on its own device
        home = next(model.parameters()).device
        replicas, used_home = [], False
        for d in threads.devices:
            if d == home and not used_home:
                replicas.append(model)
                used_home = True
            else:
                replicas.append(copy.deepcopy(model).to(d))
        for d in set(threads.devices):
            if d.type == "cuda":
                ops.ensure_selftest(d, model.rel_model)  # (a set-up step that waits: here, not in whichever thread ranks first)
                if index is not None:
                    index.device_arrays(d)  # moved once, here, not by whichever thread asks first
        world = threads.world
        _log.info(f"Evaluating on {world} device thread(s): {', '.join(str(d) for d in threads.devices)} ({threads.exchange} exchange)")
        shards = threads.run(lambda m: _shard_of_evaluation(replicas[m.rank], text_dataset, entities, emb_batch_size, m.device, _log, triples,
                                                            ent2idx, index, group=m, world=world, rank=m.rank, **common))
        del replicas
        table, axis, triples, counts, ids_ok = shards[0]
        sharded = world > 1
    else:
        sharded = group is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
        world = dist.get_world_size(group) if sharded else 1
        rank = dist.get_rank(group) if sharded else 0
        shards = None
        table, axis, triples, counts, ids_ok = _shard_of_evaluation(model, text_dataset, entities, emb_batch_size, device, _log, triples,
                                                                    ent2idx, index, group=group, world=world, rank=rank, **common)
    _log.info("Computing metrics on set of triples")
    if table.is_cuda:
        ops.release_workspaces()  # the evaluation's scratch does not stay pinned through the training steps that follow
    rr, hits = metrics_from_counts(counts)
    num_predictions = 2 * num_triples
    _log.info(f"The total number of predictions is {num_predictions:,}")
    denom = max(num_predictions, 1)
    sums = rr.double().sum(dim=0).tolist() if num_predictions else [0.0, 0.0]
    hit_sums = hits.double().sum(dim=0).tolist() if num_predictions else [[0.0] * 3, [0.0] * 3]
    assert ids_ok is None or bool(ids_ok), "a test triple names an entity that is not among the candidates"
    mrr, mrr_filt = sums[0] / denom, (sums[1] / denom if compute_filtered else 0.0)

    log_str = f"{prefix} mrr: {mrr:.4f}  "
    _run.log_scalar(f"{prefix}_mrr", mrr, epoch)
    for j, k in enumerate(HIT_POSITIONS):
        value = hit_sums[0][j] / denom
        log_str += f"hits@{k}: {value:.4f}  "
        _run.log_scalar(f"{prefix}_hits@{k}", value, epoch)
    if compute_filtered:
        log_str += f"mrr_filt: {mrr_filt:.4f}  "
        _run.log_scalar(f"{prefix}_mrr_filt", mrr_filt, epoch)
        for j, k in enumerate(HIT_POSITIONS):
            value = hit_sums[1][j] / denom
            log_str += f"hits@{k}_filt: {value:.4f}  "
            _run.log_scalar(f"{prefix}_hits@{k}_filt", value, epoch)
    _log.info(log_str)

    if compute_filtered and new_entities is not None:
        by_pos, pos_counts = utils.split_by_new_position(triples, rr[:, 1], new_entities)
        pos_counts[pos_counts < 1.0] = 1.0
        by_pos = by_pos / pos_counts
        log_str = ""
        for i, name in enumerate((f"{prefix}_mrr_filt_both_new", f"{prefix}_mrr_filt_head_new",
                                  f"{prefix}_mrr_filt_tail_new")):
            value = by_pos[i].item()
            log_str += f"{name}: {value:.4f}  "
            _run.log_scalar(name, value, epoch)
        _log.info(log_str)

    if compute_filtered and getattr(dataset, "has_rel_categories", False):
        from .data import CATEGORY_IDS
        by_cat, cat_count = utils.split_by_category(triples, rr[:, 1], dataset.rel_categories)
        cat_count[cat_count < 1.0] = 1.0
        by_cat = by_cat / cat_count
        for i, case in enumerate(["pred_head", "pred_tail"]):
            log_str = f"{case} "
            for cat, cat_id in CATEGORY_IDS.items():
                log_str += f"{cat}_mrr: {by_cat[i, cat_id]:.4f}  "
            _log.info(log_str)

    if was_training and eval_mode:
        model.train()
    if return_embeddings:
        if sharded and world > 1 and axis != "query":  # the full table only on request
            if shards is not None:  # device threads: the shards come to devices[0] by peer copies
                table = torch.cat([s[0].to(device) for s in shards])
            else:                   # processes: all-gather of the shards
                table = all_gather_rows(table, num_entities, world, group)
        return mrr, table.unsqueeze(0)
    return mrr, None
