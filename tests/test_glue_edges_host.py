"""The glue kernels' contracts, without a GPU: plain numpy restatements of what include/blp_hip.h promises for blp_topk_merge,
blp_rank_from_scores, blp_rank_metrics / blp_rank_metric_sums, blp_build_queries and blp_gather_triple_vectors, the case
builders that tests/test_gpu_glue_edges.py runs on the device, and a self-check of every builder.

* ``merge_expected``: per query the slots with row >= 0, sorted by ascending row and then by numpy's stable argsort of the
  negated scores (the header's own definition of the order), NaN last by row, padded with row -1; scores as uint32 with every
  NaN written 0x7fc00000.  Pinned to ``merge_brute``, a Python sort whose comparison is written out by hand.
* ``dense_counts_expected``: (row > t).sum(), (row >= t).sum() and the same minus the listed in-range columns.  Pinned to the C
  oracle (oracle.rank_counts on a one-hot DistMult problem whose scores ARE the matrix; finite cases) and to
  ranking._rank_block_dense, the CPU sibling of the dense route (all cases).
* ``metrics_expected``: avg = float32(int64(gt) + 1 + int64(ge)) * 0.5f, rr = 1f / avg, hits = avg <= float32(k) in numpy
  float32.  Pinned to ranking.metrics_from_counts' CPU branch, to the C oracle's metrics and, on dense score matrices that
  have the same counts, to oracle.ref_port.rank_metrics (the port of the reference's get_metrics, utils.py:103-109).
* ``prelude_expected``: the layout, the row_of rule, by_position, the substitutes of a bad id, the segment bounds by
  np.searchsorted.  Pinned to torch indexing + utils.FilterIndex.segments at a valid-ids shape.
* ``gather_expected``: ent2idx, row - row_base, zeros unless the row is in [0, N); 16-bit rows widened by Tensor.float().

Every builder asserts that its case reaches the edge it exists for; those assertions run here, on the CPU.

One thing the issue's list asks for cannot be built: a rank_metric_sums launch whose last block holds a single query.  The
launch takes b = clamp(ceil(Q / 8192), 1, 64) blocks of p = ceil(Q / b) queries, so the last block holds p - (b p - Q) >
p - b >= 4097 - 64 queries (``sums_partition`` restates it; test_sums_partition_has_no_tiny_last_block walks every Q up to
64 x 8192 + 8192).  SUMS_Q holds the shortest last blocks there are instead: Q = b (p - 1) + 1 for b = 2 and b = 64.
"""
import collections
import functools
import math
import struct

import numpy as np
import pytest
import torch

from blp_amd import ranking, utils
from oracle import oracle as orc
from oracle import ref_port

QNAN = 0x7FC00000
ROW_MAX = (1 << 31) - 1
FLT_MAX = float(np.finfo(np.float32).max)


def f32_from_bits(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def seed_of(*parts):
    return abs(hash(tuple(int(p) for p in parts))) % (1 << 31)


# ================================================================================================ merge
def merge_expected(rows, scores, k):
    """blp_topk_merge's words: (rows (Q, k) int64, score bits (Q, k) uint32)."""
    rows, scores = np.asarray(rows, np.int64), np.asarray(scores, np.float32)
    Q = rows.shape[0]
    out_rows, out_bits = np.full((Q, k), -1, np.int64), np.full((Q, k), QNAN, np.uint32)
    for q in range(Q):
        keep = rows[q] >= 0
        r, s = rows[q][keep], scores[q][keep]
        by_row = np.argsort(r, kind="stable")
        r, s = r[by_row], s[by_row]
        order = np.argsort(-s, kind="stable")[:k]          # numpy sorts every NaN last; stable: by row among equals
        b = s[order].view(np.uint32).copy()
        b[np.isnan(s[order])] = QNAN
        out_rows[q, :len(order)], out_bits[q, :len(order)] = r[order], b
    return out_rows, out_bits


def merge_brute(rows, scores, k):
    """The same by a Python sort with the comparison written out."""
    def compare(a, b):
        (ra, sa), (rb, sb) = a, b
        nan_a, nan_b = sa != sa, sb != sb
        if nan_a != nan_b:
            return 1 if nan_a else -1          # a number before any NaN
        if not nan_a:
            if sa > sb:
                return -1
            if sa < sb:
                return 1                        # (-0.0 == 0.0 falls through)
        return -1 if ra < rb else 1             # equal scores, or two NaN: the smaller row first

    out_rows, out_bits = [], []
    for row_q, score_q in zip(np.asarray(rows).tolist(), np.asarray(scores, np.float32).tolist()):
        items = sorted(((r, s) for r, s in zip(row_q, score_q) if r >= 0), key=functools.cmp_to_key(compare))[:k]
        out_rows.append([r for r, _ in items] + [-1] * (k - len(items)))
        out_bits.append([QNAN if s != s else struct.unpack("<I", struct.pack("<f", s))[0] for _, s in items]
                        + [QNAN] * (k - len(items)))
    return np.asarray(out_rows, np.int64).reshape(-1, k), np.asarray(out_bits, np.uint32).reshape(-1, k)


MERGE_K = (1, 2, 63, 64, 65, 128, 255, 256)           # list_insert's 64-slot boundaries
MERGE_N_IN = (1, 63, 64, 65, 255, 256, 257, 511, 512, 1025, 4095, 4096, 4097, 12289)
MERGE_Q = (1, 5)


def merge_waves(n_in):
    """launch_merge's geometry (topk.hip): a wave per 256 entries, 1 .. 16."""
    return min(max(n_in // 256, 1), 16)


def merge_split(n_in):
    """n_in = lists x k_in for the raw C call: the largest divisor up to sqrt(n_in) as `lists` (1 for a prime)."""
    lists = max(d for d in range(1, int(math.isqrt(n_in)) + 1) if n_in % d == 0)
    if lists == 1 and n_in > 1:
        lists = n_in                                    # a prime: n_in lists of one slot
    return lists, n_in // lists


def merge_geometry_case(n_in, Q):
    """Scores from a 40-value grid (ties in every chunk: the row decides), distinct shuffled rows, one slot in eight empty."""
    rng = np.random.default_rng(seed_of(n_in, Q))
    rows = np.stack([rng.permutation(4 * n_in + 8)[:n_in] for _ in range(Q)]).astype(np.int64)
    scores = (rng.integers(-20, 20, (Q, n_in)) / 4).astype(np.float32)
    rows[rng.random((Q, n_in)) < 0.125] = -1
    if n_in > 1:
        rows[:, 0] = np.where(rows[:, 0] < 0, 4 * n_in + 9, rows[:, 0])   # never all empty here
    return rows, scores


MERGE_ORDER_CASES = ("ties", "zeros", "specials", "empty", "extremes")
MERGE_ORDER_N = 1025   # 4 waves, 17 chunks of 64 entries: wave 0 makes five trips, the others four


def merge_order_case(name, k):
    """(rows (Q, n), scores (Q, n)) of a named order case; asserts that the case reaches its edge."""
    n = MERGE_ORDER_N
    rng = np.random.default_rng(seed_of(len(name), k))
    pos = np.arange(n)
    if name == "ties":
        # 661 equal scores over entries 40 .. 700 (eleven chunks, all four waves), three better entries in three different
        # waves, the rest worse; the tie block's rows in descending, ascending and shuffled input order
        scores = np.where((pos >= 40) & (pos <= 700), 2.0, 1.0).astype(np.float32)
        scores[[5, 330, 1000]] = 3.0
        rows = np.stack((n - 1 - pos, pos, rng.permutation(n))).astype(np.int64) * 3 + 1
        scores = np.stack((scores,) * 3)
        block = pos[(pos >= 40) & (pos <= 700)]
        assert len(set(block // 64 % merge_waves(n))) == merge_waves(n) == 4 and len(block) > 256 + 3   # the row cuts the block
        assert {5 // 64 % 4, 330 // 64 % 4, 1000 // 64 % 4} == {0, 1, 3}
    elif name == "zeros":
        # +0 / -0 with interleaved rows, a few numbers above and below; the zero's sign must come out with its row
        scores = np.where(pos % 3 == 0, -0.0, 0.0).astype(np.float32)
        scores[[7, 500]] = 1.0
        scores[[9, 800]] = -1.0
        rows = np.stack((pos, rng.permutation(n), n - 1 - pos)).astype(np.int64)
        scores = np.stack((scores,) * 3)
        want = merge_expected(rows, scores, max(k, 8))[1]
        assert all({0x80000000, 0}.issubset(set(w[:max(k, 8)].tolist())) for w in want)
    elif name == "specials":
        bits = [0x7F800000, 0xFF800000, 0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FA5A5A5,   # inf, NaN
                0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,                          # subnormals
                0x7F7FFFFF, 0xFF7FFFFF, 0x00000000, 0x80000000, 0x3F800000, 0xBF800000]                          # FLT_MAX, 0, 1
        base = f32_from_bits(bits)
        scores = np.stack([base[rng.integers(0, len(bits), n)] for _ in range(3)])
        scores[:, :len(bits)] = base                      # every pattern at least once
        rows = np.stack([rng.permutation(2 * n)[:n] for _ in range(3)]).astype(np.int64)
        nan_bits = {int(b) for b in scores.view(np.uint32).ravel() if (b & 0x7FFFFFFF) > 0x7F800000}
        assert len(nan_bits) >= 6 and any(b >> 31 for b in nan_bits)
        want_rows, want = merge_expected(rows, scores, n)
        first_nan = int(np.argmax(want[0] == QNAN))
        assert (want[0][first_nan:] == QNAN).all() and (np.diff(want_rows[0][first_nan:]) > 0).all()   # NaN last, by row
    elif name == "empty":
        rows = np.stack([rng.permutation(2 * n)[:n] for _ in range(6)]).astype(np.int64)
        scores = (rng.integers(-20, 20, (6, n)) / 4).astype(np.float32)
        rows[0] = -1                                       # every slot empty
        keep = rng.permutation(n)[:k]
        rows[1, np.setdiff1d(pos, keep)] = -1              # exactly k non-empty
        rows[2, :-1] = -1                                  # one non-empty, in the last slot
        rows[3, ::2] = -1                                  # empty slots interleaved with real ones
        rows[4, 1::3] = -1
        scores[4, 1::3] = 1.0e30                           # ... carrying a finite score above every real one
        rows[5, ::5] = -7                                  # ... carrying row -7
        scores[5, ::5] = np.inf
        want_rows = merge_expected(rows, scores, k)[0]
        assert (want_rows[0] == -1).all() and (want_rows[1] >= 0).all() and (want_rows[2] >= 0).sum() == 1
        assert (want_rows[2][1:] == -1).all() and (scores[4][rows[4] >= 0] < 1.0e30).all()
    elif name == "extremes":
        # rows 0 and 2^31 - 1 as the best, as a tie with others, and with NaN scores (the two ends of the key's row field)
        rows = np.stack([rng.permutation(2 * n)[:n] + 1 for _ in range(4)]).astype(np.int64)
        scores = (rng.integers(-20, 20, (4, n)) / 4).astype(np.float32)
        rows[:, 100], rows[:, 900] = ROW_MAX, 0
        scores[0, [100, 900]] = 9.0
        scores[1, [100, 900, 333, 334]] = 9.0
        scores[2, [100, 900]] = np.nan
        scores[2, 2:] = np.where(pos[2:] % 7 == 0, np.nan, scores[2, 2:])
        rows[3, :] = -1                                    # nothing but the two extremes, both NaN: they take slots 0 and 1
        rows[3, [100, 900]] = ROW_MAX, 0
        scores[3, [100, 900]] = np.nan
        want_rows, want = merge_expected(rows, scores, 2)
        assert want_rows[3].tolist() == [0, ROW_MAX] and (want[3] == QNAN).all()
        assert want_rows[0].tolist() == [0, ROW_MAX]
    else:
        raise KeyError(name)
    for q in range(rows.shape[0]):                         # non-empty rows of one query are distinct
        live = rows[q][rows[q] >= 0]
        assert len(np.unique(live)) == len(live) and (live <= ROW_MAX).all()
    return rows, scores


# ================================================================================================ dense counts
def dense_counts_expected(scores, true, rowptr=None, col=None):
    """blp_rank_from_scores' words: counts (Q, 4) int32 {gt, ge, gt_filt, ge_filt}; ``true`` (Q,) the true SCORES."""
    scores, true = np.asarray(scores, np.float32), np.asarray(true, np.float32)
    Q, N = scores.shape
    out = np.zeros((Q, 4), np.int32)
    for q in range(Q):
        row, t = scores[q], true[q]
        gt, ge = int((row > t).sum()), int((row >= t).sum())
        fgt = fge = 0
        if rowptr is not None:
            c = np.asarray(col[int(rowptr[q]):int(rowptr[q + 1])], np.int64)
            c = c[(c >= 0) & (c < N)]                      # "a column outside [0, N) is ignored"
            fgt, fge = int((row[c] > t).sum()), int((row[c] >= t).sum())
        out[q] = gt, ge, gt - fgt, ge - fge
    return out


DENSE_Q = (1, 3, 4, 5, 9)          # four queries per workgroup
DENSE_N = (1, 63, 64, 65, 129)     # 64 columns per trip of a wave
DENSE_KINDS = ("ties", "zeros", "nonfinite", "true_nan", "true_pinf", "true_ninf")
DENSE_FINITE = ("ties", "zeros")
DenseCase = collections.namedtuple("DenseCase", "scores true_idx rowptr col")


def dense_case(kind, Q, N):
    """A (Q, N) score matrix, true columns (0 for even queries, N - 1 for odd ones) and a CSR filter whose rows are empty
    (q % 3 == 0), list the true column and every fourth one (q % 3 == 1) or list every column (q % 3 == 2)."""
    rng = np.random.default_rng(seed_of(len(kind), DENSE_KINDS.index(kind), Q, N))
    true_idx = np.where(np.arange(Q) % 2 == 0, 0, N - 1).astype(np.int64)
    qs = np.arange(Q)
    if kind == "zeros":
        scores = f32_from_bits(rng.choice(np.asarray([0, 0x80000000, 1, 0x80000001], np.uint32), (Q, N))).copy()
        scores[qs, true_idx] = np.where(qs % 2 == 0, 0.0, -0.0)
    else:
        scores = (rng.integers(-2, 3, (Q, N)) / 2).astype(np.float32)
        scores[qs, true_idx] = 0.0
    if kind != "ties" and kind != "zeros":
        special = rng.random((Q, N))
        scores[special < 0.10] = np.inf
        scores[(special >= 0.10) & (special < 0.20)] = -np.inf
        scores[(special >= 0.20) & (special < 0.30)] = np.nan
        scores[qs, true_idx] = {"nonfinite": 0.0, "true_nan": np.nan, "true_pinf": np.inf, "true_ninf": -np.inf}[kind]
    rowptr, col = [0], []
    for q in range(Q):
        if q % 3 == 1:
            col += sorted({int(true_idx[q]), *range(0, N, 4)})
        elif q % 3 == 2:
            col += list(range(N))
        rowptr.append(len(col))
    case = DenseCase(scores, true_idx, np.asarray(rowptr, np.int64), np.asarray(col, np.int64))
    want = dense_counts_expected(scores, scores[qs, true_idx], case.rowptr, case.col)
    if kind == "true_nan":
        assert not want.any()                              # every comparison with NaN is false: worst rank 0
    elif kind == "true_pinf":
        assert (want[:, 0] == 0).all() and (want[:, 1] >= 1).all()
    elif kind == "true_ninf":
        assert (want[:, 1] == (~np.isnan(scores)).sum(1)).all()
    else:
        assert (want[:, 1] >= want[:, 0] + 1).all()        # the true column itself
        if N >= 63:
            assert (want[:, 1] >= want[:, 0] + 2).any(), "no tie with the true score"
            if kind == "nonfinite":
                assert np.isnan(scores).any() and np.isposinf(scores).any() and np.isneginf(scores).any()
            if kind == "zeros":
                signs = scores.view(np.uint32)
                assert (signs == 0x80000000).any() and (signs == 0).any() and (want[:, 0] > 0).any()
    if kind != "true_nan":
        assert (want[qs % 3 == 2, 2:] == 0).all()          # every column listed
        if kind in ("ties", "zeros", "nonfinite"):
            assert (want[qs % 3 == 1, 3] < want[qs % 3 == 1, 1]).all()   # the true column is listed
    assert (want[qs % 3 == 0, 2:] == want[qs % 3 == 0, :2]).all()
    return case


# ================================================================================================ metrics
K_VALUE_SETS = ((1, 3, 10), (10, 3, 1), (2, 2, 5))
METRICS_Q = (1, 255, 256, 257)                                       # rank_metrics_kernel's 256-thread blocks
SUMS_Q = (1, 1023, 1024, 1025, 8191, 8192, 8193, 16385, 64 * 8192, 64 * 8192 + 1)
SUMS_MIN_PER_BLOCK, SUMS_MAX_BLOCKS = 8192, 64


def sums_partition(Q):
    """launch_rank_metric_sums' partition (rank_all.hip): (blocks, queries per block, queries of the last block)."""
    blocks = min(max(-(-Q // SUMS_MIN_PER_BLOCK), 1), SUMS_MAX_BLOCKS)
    per_block = -(-Q // blocks) if blocks > 1 else max(Q, 1)
    return blocks, per_block, Q - (blocks - 1) * per_block


def metrics_expected(counts, k_values):
    """blp_rank_metrics' words: rr (Q, 2) float32, hits (Q, 2, 3) bool."""
    c = np.asarray(counts).astype(np.int64)
    total = np.stack((c[:, 0] + 1 + c[:, 1], c[:, 2] + 1 + c[:, 3]), axis=1)
    avg = total.astype(np.float32) * np.float32(0.5)
    with np.errstate(divide="ignore"):
        rr = np.float32(1) / avg
    return rr, avg[:, :, None] <= np.asarray(k_values, np.float32)


def metric_sums_expected(counts, k_values):
    """blp_rank_metric_sums' words: [exact sum of rr raw, filtered] (math.fsum of the float32 values) and the six hit
    counts as integers, raw x 3 then filtered x 3."""
    rr, hits = metrics_expected(counts, k_values)
    return [math.fsum(rr[:, v].astype(np.float64).tolist()) for v in (0, 1)], hits.sum(0).reshape(-1).astype(np.int64)


def metric_edge_pairs(k_values):
    """(gt, ge) pairs at the edges: avg exactly k, k + 1/2, k - 1/2 for each k; gt == ge (worst below best: the NaN true
    score's 0, 0); 0, 1; and counts around 2^24 and at 2^31 - 1, where float32(best + worst) rounds."""
    pairs = [(0, 0), (0, 1), (5, 5)]
    for k in sorted(set(k_values)):
        pairs += [(k - 1, k), (k - 1, k + 1), (k - 1, k - 1)]       # 2 avg = 2k, 2k + 1, 2k - 1
    top = (1 << 31) - 1
    for c in ((1 << 24) - 1, 1 << 24, (1 << 24) + 1, top):
        pairs += [(c, c), (c - 1, c), (c, min(c + 1, top)), (c - 2, min(c + 1, top))]
    return pairs


def metric_counts(Q, k_values):
    """(Q, 4) int32: the edge pairs tiled, the filtered columns a rotation of the raw ones (so that they differ from them at
    every edge); the last 64 queries rank first (a sum that drops the tail of the queries loses hits)."""
    pairs = np.asarray(metric_edge_pairs(k_values), np.int64)
    raw = pairs[np.arange(Q) % len(pairs)]
    filt = pairs[(np.arange(Q) + 7) % len(pairs)]
    counts = np.concatenate((raw, filt), axis=1)
    counts[max(Q - 64, 0):] = (0, 1, 0, 1)
    assert counts.max() <= (1 << 31) - 1 and counts.min() >= 0
    return counts.astype(np.int32)


# ================================================================================================ prelude and gather
def row_of(ident, ent2idx, src_rows):
    """id -> row of the source, -1 if it has none (include/blp_hip.h: blp_queries)."""
    if ent2idx is None:
        return ident if 0 <= ident < src_rows else -1
    r = int(ent2idx[ident]) if 0 <= ident < len(ent2idx) else -1
    return r if 0 <= r < src_rows else -1


def layout(n, block):
    """[(head side?, triple)] per query position: block after block, each [heads | tails], the last block short."""
    out = []
    for first in range(0, n, block):
        nb = min(block, n - first)
        out += [(True, first + j) for j in range(nb)] + [(False, first + j) for j in range(nb)]
    return out


Prelude = collections.namedtuple("Prelude", "fixed_row true_row rel_ids ids_min q_fixed q_rel seg_lo seg_hi exclude")


def prelude_expected(triples, ent2idx, src_rows, R, block, by_position=False, source=None, rel_emb=None, index=None):
    """blp_build_queries' words.  triples (n, 3) numpy; ent2idx numpy or None; source / rel_emb: float32 numpy, given when the
    vectors are wanted (by_position: the (2n, D) array); index: (heads_key, tails_key, index_R) numpy, or None."""
    n = triples.shape[0]
    fixed_row, true_row, rel_ids = (np.zeros(2 * n, np.int64) for _ in range(3))
    seg_lo, seg_hi, exclude = (np.zeros(2 * n, np.int64) for _ in range(3))
    q_fixed = q_rel = None
    if source is not None:
        q_fixed, q_rel = np.zeros((2 * n, source.shape[1]), np.float32), np.zeros((2 * n, source.shape[1]), np.float32)
    ids_min = 0
    for p, (head_side, t) in enumerate(layout(n, block)):
        h_id, t_id, r_id = (int(x) for x in triples[t])
        h_row, t_row = row_of(h_id, ent2idx, src_rows), row_of(t_id, ent2idx, src_rows)
        fixed, true = (t_row, h_row) if head_side else (h_row, t_row)
        if by_position:
            fixed = -1 if fixed < 0 else (n + t if head_side else t)
            true = -1 if true < 0 else (t if head_side else n + t)
        rel_ok = 0 <= r_id < R
        if h_row < 0 or t_row < 0 or not rel_ok:
            ids_min = -1
        fixed_row[p], true_row[p], rel_ids[p] = max(fixed, 0), max(true, 0), r_id if rel_ok else 0
        if source is not None:
            if fixed >= 0:
                q_fixed[p] = source[fixed]
            if rel_ok:
                q_rel[p] = rel_emb[r_id]
        if index is not None:
            heads_key, tails_key, index_R = index
            keys, base = (heads_key, 0) if head_side else (tails_key, len(heads_key))
            key = (t_id if head_side else h_id) * index_R + r_id if 0 <= r_id < index_R else -1
            seg_lo[p] = base + np.searchsorted(keys, key, side="left")
            seg_hi[p] = base + np.searchsorted(keys, key, side="right")
            exclude[p] = h_id if head_side else t_id
    if index is None:
        seg_lo = seg_hi = exclude = None
    return Prelude(fixed_row, true_row, rel_ids, ids_min, q_fixed, q_rel, seg_lo, seg_hi, exclude)


def gather_expected(triples, ent2idx, table, row_base=0):
    """blp_gather_triple_vectors' words: (2n, D) float32; ``table`` a torch CPU tensor of any storage type."""
    n, (N, D) = triples.shape[0], table.shape
    wide = table.float().numpy()
    out = np.zeros((2 * n, D), np.float32)
    for p in range(2 * n):
        ident = int(triples[p, 0]) if p < n else int(triples[p - n, 1])
        row = ident
        if ent2idx is not None:
            row = int(ent2idx[ident]) if 0 <= ident < len(ent2idx) else -1
        if row >= 0 and 0 <= row - row_base < N:
            out[p] = wide[row - row_base]
    return out


PRELUDE_N = (0, 1, 7, 8, 9, 64, 65)       # eight queries per workgroup of the gather half
PRELUDE_D = (4, 124, 128, 132, 300, 1024)  # 128 floats per sweep
NUM_IDS, NUM_ROWS, NUM_RELS, INDEX_RELS = 40, 23, 6, 4
PAD = 4                                    # the source is a column slice of a tensor PAD floats wider


def prelude_blocks(n):
    return sorted({b for b in (1, 3, n - 1, n, n + 1, 1 << 20) if b > 0})


World = collections.namedtuple("World", "entities ent2idx table rel_emb edges index")


@functools.lru_cache(maxsize=None)
def world(D, dtype=torch.float32):
    """NUM_ROWS entities out of NUM_IDS ids, a strided (NUM_ROWS, D) table, NUM_RELS relation rows and a filter index that
    knows INDEX_RELS of the relations and none of the two largest entity ids."""
    g = torch.Generator().manual_seed(D)
    entities = torch.randperm(NUM_IDS - 2, generator=g)[:NUM_ROWS - 2]
    entities = torch.cat((entities, torch.tensor([NUM_IDS - 2, NUM_IDS - 1])))      # the largest ids are candidates too
    ent2idx = utils.make_ent2idx(entities, NUM_IDS - 1)
    pad = PAD if dtype == torch.float32 else 8
    table = torch.randn(NUM_ROWS, D + pad, generator=g).to(dtype)[:, :D]
    rel_emb = torch.randn(NUM_RELS, D, generator=g)
    known = entities[:-2]
    pick = lambda m: known[torch.randint(0, len(known), (m,), generator=g)]
    edges = torch.stack((pick(150), pick(150), torch.randint(0, INDEX_RELS, (150,), generator=g)), dim=1)
    index = utils.FilterIndex(edges)
    assert index.R == INDEX_RELS < NUM_RELS and index.max_node < NUM_IDS - 2 and table.stride(0) > D
    return World(entities, ent2idx, table, rel_emb, edges, index)


def prelude_triples(w, n, mapped):
    """n triples of valid ids (mapped: entity ids; else table rows); the first uses the first and the last table row."""
    g = torch.Generator().manual_seed(1000 + n)
    rows = torch.randint(0, NUM_ROWS, (n, 2), generator=g)
    if n:
        rows[0, 0], rows[0, 1] = 0, NUM_ROWS - 1
    ids = w.entities[rows] if mapped else rows
    return torch.cat((ids.reshape(n, 2), torch.randint(0, NUM_RELS, (n, 1), generator=g)), dim=1)


def index_arrays(index):
    heads_key, tails_key, _, n_head_vals = index.device_arrays("cpu")
    assert n_head_vals == heads_key.shape[0]
    return heads_key.numpy(), tails_key.numpy(), index.R


BAD_IDS = ("unmapped", "minus_one", "past_map", "row_past_source", "rel_minus_one", "rel_R")


def bad_id_case(w, kind, where, n=9, t_bad=4):
    """Valid triples with ONE bad id at triple t_bad: ``where`` = 0 (head), 1 (tail) or 2 (relation).  Returns (triples,
    ent2idx): `row_past_source` needs a map of its own, with an id whose row lies past the table."""
    triples = prelude_triples(w, n, True).clone()
    ent2idx = w.ent2idx.clone()
    free = int((ent2idx < 0).nonzero()[0])
    if kind == "unmapped":
        triples[t_bad, where] = free
    elif kind == "minus_one":
        triples[t_bad, where] = -1
    elif kind == "past_map":
        triples[t_bad, where] = NUM_IDS
    elif kind == "row_past_source":
        ent2idx[free] = NUM_ROWS + 3
        triples[t_bad, where] = free
    elif kind == "rel_minus_one":
        triples[t_bad, 2] = -1
    elif kind == "rel_R":
        triples[t_bad, 2] = NUM_RELS
    assert (where == 2) == kind.startswith("rel_")
    return triples, ent2idx


def bad_id_cases():
    return [(kind, where) for kind in BAD_IDS for where in ((2,) if kind.startswith("rel_") else (0, 1))]


def segment_case(w):
    """Triples whose keys sit at the edges of the index: the first and the last key of each side, a key with one value and
    one with many, an absent key, a relation the index never saw (INDEX_RELS <= r < NUM_RELS), an entity id above every
    indexed node.  Asserts on the expectation that each is reached."""
    heads_key, tails_key, R = index_arrays(w.index)
    known = w.entities[:-2].tolist()

    def by_count(keys, many):
        uniq, cnt = np.unique(keys, return_counts=True)
        return int(uniq[cnt > 1][0]) if many else int(uniq[cnt == 1][0])

    other = known[0]
    triples = []
    for key in (heads_key[0], heads_key[-1], by_count(heads_key, False), by_count(heads_key, True)):   # (tail, rel) -> heads
        triples.append((other, int(key) // R, int(key) % R))
    for key in (tails_key[0], tails_key[-1], by_count(tails_key, False), by_count(tails_key, True)):   # (head, rel) -> tails
        triples.append((int(key) // R, other, int(key) % R))
    absent = next((e, r) for e in known for r in range(R) if e * R + r not in set(heads_key.tolist()) | set(tails_key.tolist()))
    triples.append((absent[0], absent[0], absent[1]))
    triples.append((known[1], known[2], NUM_RELS - 1))            # a relation of the embedding, not of the index
    triples.append((NUM_IDS - 1, NUM_IDS - 2, 0))                 # entity ids above every indexed node
    triples = torch.tensor(triples, dtype=torch.long)
    n = triples.shape[0]
    want = prelude_expected(triples.numpy(), w.ent2idx.numpy(), NUM_ROWS, NUM_RELS, n, index=(heads_key, tails_key, R))
    assert want.ids_min == 0
    length = want.seg_hi - want.seg_lo
    nh, nt = len(heads_key), len(tails_key)
    head, tail = slice(0, n), slice(n, 2 * n)
    assert want.seg_lo[head][0] == 0 and want.seg_hi[head][1] == nh                      # first / last key, head side
    assert want.seg_lo[tail][4] == nh and want.seg_hi[tail][5] == nh + nt                # ... tail side, offset by n_heads
    assert length[head][2] == 1 and length[head][3] > 1 and length[tail][6] == 1 and length[tail][7] > 1
    assert length[head][8] == 0 and length[tail][8] == 0                                 # absent key
    assert length[head][9] == 0 and length[tail][9] == 0 and want.seg_lo[head][9] == 0 and want.seg_lo[tail][9] == nh
    assert want.seg_lo[head][10] == want.seg_hi[head][10] == nh and want.seg_lo[tail][10] == nh + nt   # past every key
    assert (want.seg_lo[tail] >= nh).all() and (want.seg_hi[head] <= nh).all()
    assert (want.exclude[head] == triples[:, 0].numpy()).all() and (want.exclude[tail] == triples[:, 1].numpy()).all()
    return triples, want


GATHER_D = (8, 128, 136, 768)
GATHER_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
# A signalling half NaN is left out: the half -> float conversion instruction quiets it, on the host as on the device, so
# what `.float()` gives for it depends on whether the host converts in hardware.  Quiet payloads widen bit for bit.
SPECIAL_BITS = {
    torch.float32: [0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0, 0x80000000, 1,
                    0x80000001, 0x007FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000],
    torch.float16: [0x7E00, 0x7E01, 0xFE00, 0xFFFF, 0x7F55, 0x7C00, 0xFC00, 0, 0x8000, 1, 0x8001, 0x03FF, 0x83FF, 0x7BFF, 0xFBFF,
                    0x3C00],
    torch.bfloat16: [0x7FC0, 0x7FC1, 0xFFC0, 0x7F81, 0xFFFF, 0x7F80, 0xFF80, 0, 0x8000, 1, 0x8001, 0x007F, 0x807F, 0x7F7F, 0xFF7F,
                     0x3F80],
}


def special_table(dtype, N, D):
    """(N, D) of ``dtype``, a column slice of a wider tensor (row stride D + 8), every element one of the special patterns."""
    bits = SPECIAL_BITS[dtype]
    g = torch.Generator().manual_seed(N * 1000 + D)
    pick = torch.randint(0, len(bits), (N, D + 8), generator=g)
    pick[0, :len(bits)] = torch.arange(len(bits))[:D + 8]
    if dtype == torch.float32:
        raw = torch.tensor(bits, dtype=torch.int64)[pick].to(torch.int64)
        table = torch.from_numpy(raw.numpy().astype(np.uint32).view(np.float32).copy())
    else:
        raw = torch.tensor(bits, dtype=torch.int64)[pick]
        table = torch.from_numpy(raw.numpy().astype(np.uint16).view(np.int16).copy()).view(dtype)
    table = table[:, :D]
    assert table.stride(0) % 8 == 0 and table.stride(0) > D and table.dtype == dtype
    return table


def as_bits(x):
    """float32 numpy / torch -> int32 numpy of the same bits."""
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.int32)


# ================================================================================================ the self-checks
@pytest.mark.parametrize("n_in", [1, 63, 65, 257, 1025])
def test_merge_expected_is_the_handwritten_sort(n_in):
    for Q in MERGE_Q:
        rows, scores = merge_geometry_case(n_in, Q)
        for k in (1, 2, 64, 65, 256):
            want_rows, want_bits = merge_expected(rows, scores, k)
            brute_rows, brute_bits = merge_brute(rows, scores, k)
            assert np.array_equal(want_rows, brute_rows) and np.array_equal(want_bits, brute_bits), (n_in, Q, k)


@pytest.mark.parametrize("name", MERGE_ORDER_CASES)
def test_merge_order_cases_reach_their_edges(name):
    for k in (1, 65, 256):
        rows, scores = merge_order_case(name, k)
        assert rows.shape == scores.shape == (rows.shape[0], MERGE_ORDER_N)
        want_rows, want_bits = merge_expected(rows, scores, k)
        brute_rows, brute_bits = merge_brute(rows, scores, k)
        assert np.array_equal(want_rows, brute_rows) and np.array_equal(want_bits, brute_bits), (name, k)


def test_merge_geometry_reaches_every_wave_count_and_the_padding():
    waves = {merge_waves(n) for n in MERGE_N_IN}
    assert {1, 2, 4, 15, 16} <= waves and merge_waves(12289) == 16 and 12289 == 16 * 64 * 12 + 1   # 3 x 4 chunks per wave + 1
    assert any(n < k for n in MERGE_N_IN for k in MERGE_K)
    for n in MERGE_N_IN:
        lists, k_in = merge_split(n)
        assert lists * k_in == n and (n == 1 or lists > 1)
        rows, _ = merge_geometry_case(n, 5)
        assert ((rows >= 0).sum(1) >= min(n, 1)).all() and (n < 64 or (rows < 0).any())


@pytest.mark.parametrize("kind", DENSE_KINDS)
def test_dense_counts_expected_is_the_oracle_and_the_cpu_route(kind):
    for Q in DENSE_Q:
        for N in DENSE_N:
            c = dense_case(kind, Q, N)
            true = c.scores[np.arange(Q), c.true_idx]
            want = dense_counts_expected(c.scores, true, c.rowptr, c.col)
            m = torch.from_numpy(c.scores)
            cpu = ranking._rank_block_dense(lambda h, t, r: m if r.shape[0] else m[:0], torch.zeros(N, 1), torch.zeros(Q, 1),
                                            torch.zeros(Q, 1), Q, ("row", torch.from_numpy(c.true_idx)),
                                            torch.from_numpy(c.rowptr), torch.from_numpy(c.col))
            assert np.array_equal(cpu.numpy(), want), (kind, Q, N)
            if kind in DENSE_FINITE:
                # DistMult on one-hot queries: score(row n, query q) = sum_d table[n, d] * 1 * [d == q] = scores[q, n] exactly
                got = orc.rank_counts("distmult", orc.SIDE_HEAD, np.ascontiguousarray(c.scores.T), np.eye(Q, dtype=np.float32),
                                      np.ones((Q, Q), np.float32), true_row=c.true_idx, filt_rowptr=c.rowptr, filt_col=c.col)
                assert np.array_equal(got, want), (kind, Q, N)


def dense_matrix_with_counts(gt, ge):
    """A score row and its true column with exactly these raw counts (ge == 0: a NaN true score)."""
    row = [0.0 if ge else float("nan")] + [1.0] * gt + [0.0] * max(ge - gt - 1, 0) + [-1.0, -1.0]
    return row


@pytest.mark.parametrize("k_values", K_VALUE_SETS)
def test_metrics_expected_is_the_cpu_branch_the_oracle_and_the_port(k_values):
    counts = metric_counts(257, k_values)
    rr, hits = metrics_expected(counts, k_values)
    t_rr, t_hits = ranking.metrics_from_counts(torch.from_numpy(counts), k_values)
    assert np.array_equal(as_bits(t_rr), as_bits(rr)) and np.array_equal(t_hits.numpy(), hits)
    for v in (0, 1):
        o_rr, o_hits = orc.metrics_from_counts(counts[:, 2 * v], counts[:, 2 * v + 1], k_values)
        assert np.array_equal(as_bits(o_rr), as_bits(rr[:, v])) and np.array_equal(o_hits, hits[:, v])
    # the port of the reference's get_metrics on dense matrices with the same counts (the small pairs: a row per count)
    small = [(gt, ge) for gt, ge in metric_edge_pairs(k_values) if ge < 64 and (ge > gt or gt == ge == 0)]
    assert len(small) >= 6 and (0, 0) in small and (0, 1) in small
    width = max(len(dense_matrix_with_counts(*p)) for p in small)
    pred = torch.tensor([dense_matrix_with_counts(*p) + [-1.0] * (width - len(dense_matrix_with_counts(*p))) for p in small])
    gt, ge, p_rr, p_hits = ref_port.rank_metrics(pred, torch.zeros(len(small), 1, dtype=torch.long), k_values)
    assert [tuple(x) for x in torch.stack((gt, ge), 1).tolist()] == small
    c4 = np.asarray([(a, b, a, b) for a, b in small], np.int32)
    rr, hits = metrics_expected(c4, k_values)
    assert np.array_equal(as_bits(p_rr), as_bits(rr[:, 0])) and np.array_equal(p_hits.numpy(), hits[:, 0])


@pytest.mark.parametrize("k_values", K_VALUE_SETS)
def test_metric_counts_reach_their_edges(k_values):
    counts = metric_counts(257, k_values).astype(np.int64)
    for v in (0, 1):
        total = counts[:, 2 * v] + 1 + counts[:, 2 * v + 1]
        for k in k_values:
            assert {2 * k - 1, 2 * k, 2 * k + 1} <= set(total.tolist())
        assert (counts[:, 2 * v] == counts[:, 2 * v + 1]).any() and (total == 1).any() and (total == 2).any()
        inexact = total.astype(np.float32).astype(np.int64) != total               # the conversion of best + worst rounds
        assert inexact.any() and (total > (1 << 31)).any()                         # ... and the sum needs 64 bits
        separately = (counts[:, 2 * v] + 1).astype(np.float32) + counts[:, 2 * v + 1].astype(np.float32)
        assert (separately != total.astype(np.float32)).any()                      # adding two rounded floats is not the same
    assert (counts[:-64, :2] != counts[:-64, 2:]).any(1).all()
    rr, hits = metrics_expected(counts, k_values)
    assert np.isfinite(rr).all() and (rr > 0).all() and hits.any() and not hits.all()
    sums, hit_sums = metric_sums_expected(counts, k_values)
    assert hit_sums.shape == (6,) and sums[0] != sums[1]


def test_sums_partition_has_no_tiny_last_block():
    assert [sums_partition(Q)[0] for Q in SUMS_Q] == [1, 1, 1, 1, 1, 1, 2, 3, 64, 64]
    assert sums_partition(64 * 8192 + 1) == (64, 8193, 8193 - 63) and sums_partition(8193)[2] == 4096
    assert sums_partition(16385) == (3, 5462, 5461)
    shortest = min(sums_partition(Q)[2] for Q in range(8193, 64 * 8192 + 8193))
    assert shortest == 4096                                  # Q = 8193: no launch leaves one query to its last block
    for Q in (8193, 64 * 8192 + 1):                          # ... and these are the shortest last blocks of 2 and of 64 blocks
        b, p, last = sums_partition(Q)
        assert last == p - (b - 1) and Q == b * (p - 1) + 1


@pytest.mark.parametrize("mapped", [True, False])
def test_prelude_expected_is_the_torch_prelude(mapped):
    """At valid ids: torch indexing for rows and vectors, FilterIndex.segments for the filter, block by block."""
    D, n, block = 132, 65, 9
    w = world(D)
    triples = prelude_triples(w, n, mapped)
    ent2idx = w.ent2idx if mapped else None
    table = w.table.contiguous()
    want = prelude_expected(triples.numpy(), None if ent2idx is None else ent2idx.numpy(), NUM_ROWS, NUM_RELS, block,
                            source=table.numpy(), rel_emb=w.rel_emb.numpy(), index=index_arrays(w.index))
    assert want.ids_min == 0
    heads = ent2idx[triples[:, 0]] if mapped else triples[:, 0]
    tails = ent2idx[triples[:, 1]] if mapped else triples[:, 1]
    assert int(heads[0]) == 0 and int(tails[0]) == NUM_ROWS - 1
    seg = w.index.segments(triples, w.ent2idx, "cpu")
    pos = 0
    for first in range(0, n, block):
        nb = min(block, n - first)
        t, hs, ts = slice(first, first + nb), slice(pos, pos + nb), slice(pos + nb, pos + 2 * nb)
        assert np.array_equal(want.q_fixed[hs], table[tails[t]].numpy()) and np.array_equal(want.q_fixed[ts], table[heads[t]].numpy())
        rel = w.rel_emb[triples[t, 2]].numpy()
        assert np.array_equal(want.q_rel[hs], rel) and np.array_equal(want.q_rel[ts], rel)
        assert np.array_equal(want.true_row[hs], heads[t].numpy()) and np.array_equal(want.true_row[ts], tails[t].numpy())
        assert np.array_equal(want.fixed_row[hs], tails[t].numpy()) and np.array_equal(want.fixed_row[ts], heads[t].numpy())
        assert np.array_equal(want.rel_ids[hs], triples[t, 2].numpy()) and np.array_equal(want.rel_ids[ts], triples[t, 2].numpy())
        for name in ("seg_lo", "seg_hi", "exclude"):
            ref = getattr(seg, name).numpy()
            got = getattr(want, name)
            assert np.array_equal(got[hs], ref[first:first + nb]) and np.array_equal(got[ts], ref[n + first:n + first + nb]), name
        pos += 2 * nb
    assert pos == 2 * n and n % block != 0


def test_prelude_layout_and_by_position():
    assert layout(0, 3) == [] and layout(2, 1) == [(True, 0), (False, 0), (True, 1), (False, 1)]
    assert layout(3, 2) == [(True, 0), (True, 1), (False, 0), (False, 1), (True, 2), (False, 2)]
    assert layout(3, 1 << 20) == layout(3, 3) == layout(3, 4)
    w = world(4)
    triples = prelude_triples(w, 7, True)
    want = prelude_expected(triples.numpy(), w.ent2idx.numpy(), NUM_ROWS, NUM_RELS, 3, by_position=True)
    for p, (head_side, t) in enumerate(layout(7, 3)):
        assert (want.fixed_row[p], want.true_row[p]) == ((7 + t, t) if head_side else (t, 7 + t))
    for n in PRELUDE_N:
        assert all(b >= 1 for b in prelude_blocks(n)) and (n < 2 or {n - 1, n, n + 1} <= set(prelude_blocks(n)))


def test_segment_case_reaches_its_edges():
    triples, want = segment_case(world(4))
    assert triples.shape == (11, 3) and want.seg_lo.shape == (22,)


@pytest.mark.parametrize("kind,where", bad_id_cases())
def test_bad_id_cases_substitute_only_the_bad_operand(kind, where):
    w = world(8)
    n, t_bad = 9, 4
    good = prelude_triples(w, n, True)
    triples, ent2idx = bad_id_case(w, kind, where, n, t_bad)
    assert (triples != good).sum() == 1
    table = w.table.contiguous().numpy()
    for by_position in (False, True):
        source = gather_expected(triples.numpy(), ent2idx.numpy(), w.table) if by_position else table
        good_source = gather_expected(good.numpy(), w.ent2idx.numpy(), w.table) if by_position else table
        want = prelude_expected(triples.numpy(), ent2idx.numpy(), NUM_ROWS, NUM_RELS, 3, by_position, source, w.rel_emb.numpy())
        ref = prelude_expected(good.numpy(), w.ent2idx.numpy(), NUM_ROWS, NUM_RELS, 3, by_position, good_source, w.rel_emb.numpy())
        assert want.ids_min == -1 and ref.ids_min == 0
        for p, (head_side, t) in enumerate(layout(n, 3)):
            if t != t_bad:                                     # every other query of the call is untouched
                assert all(np.array_equal(getattr(want, f)[p], getattr(ref, f)[p]) for f in Prelude._fields[:3] + Prelude._fields[4:6])
                continue
            bad_is_fixed = where == (1 if head_side else 0)
            bad_is_true = where == (0 if head_side else 1)
            assert (not want.q_fixed[p].any()) == bad_is_fixed and (not want.q_rel[p].any()) == (where == 2)
            assert want.fixed_row[p] == (0 if bad_is_fixed else ref.fixed_row[p])
            assert want.true_row[p] == (0 if bad_is_true else ref.true_row[p])
            assert want.rel_ids[p] == (0 if where == 2 else ref.rel_ids[p])
            assert ref.q_fixed[p].any() and ref.q_rel[p].any() and ref.true_row[p] > 0 and ref.fixed_row[p] > 0 and ref.rel_ids[p] > 0


@pytest.mark.parametrize("dtype", GATHER_DTYPES)
def test_special_tables_hold_every_pattern_and_widen_exactly(dtype):
    table = special_table(dtype, 11, 136)
    wide = table.float()
    bits = as_bits(wide)
    assert np.isnan(wide.numpy()).any() and np.isinf(wide.numpy()).any() and (bits == np.int32(-(1 << 31))).any() and (bits == 0).any()
    finfo = torch.finfo(dtype)
    assert (wide == finfo.max).any() and (wide == -finfo.max).any()
    tiny = wide.abs()[(wide != 0) & ~wide.isnan()].min().item()
    assert tiny == finfo.smallest_normal * finfo.eps                # the smallest subnormal of the storage type
    nan_patterns = {int(b) for b in bits[np.isnan(wide.numpy())].ravel()}
    assert len(nan_patterns) >= 4 and any(b < 0 for b in nan_patterns)
    if dtype != torch.float32:                                      # widening is exact: narrowing again gives the table's bits
        number = ~wide.isnan()
        assert torch.equal(wide.to(dtype).view(torch.int16)[number], table.contiguous().view(torch.int16)[number])
        shift = 13 if dtype == torch.float16 else 16               # a NaN keeps its sign and its payload, moved up
        src = table.contiguous().view(torch.int16).to(torch.int32)[~number] & 0xFFFF
        mant = 0x3FF if dtype == torch.float16 else 0x7F
        assert np.array_equal(bits[~number.numpy()] & 0x7FFFFF, ((src & mant) << shift).numpy())
        assert np.array_equal(bits[~number.numpy()] < 0, (src >= 0x8000).numpy())


def test_gather_expected_shards_and_bad_ids():
    w = world(8)
    triples = prelude_triples(w, 9, True).clone()
    triples[3, 0], triples[5, 1] = -1, NUM_IDS + 1                  # an id of -1, an id past the map
    full = gather_expected(triples.numpy(), w.ent2idx.numpy(), w.table)
    assert not full[3].any() and not full[9 + 5].any() and full[0].any()
    assert np.array_equal(full[0], w.table[0].numpy()) and np.array_equal(full[9], w.table[NUM_ROWS - 1].numpy())
    lo, hi = 5, 14
    triples_np = triples.numpy()
    parts = [gather_expected(triples_np, w.ent2idx.numpy(), w.table[a:b], a) for a, b in ((0, lo), (lo, hi), (hi, NUM_ROWS))]
    assert np.array_equal(as_bits(sum(parts)), as_bits(full))
    assert all(((p != 0).any(1)).sum() < ((full != 0).any(1)).sum() for p in parts)
    none = gather_expected(np.asarray([[0, NUM_ROWS - 1, 0], [NUM_ROWS, -1, 0]]), None, w.table)
    assert np.array_equal(none[0], w.table[0].numpy()) and np.array_equal(none[2], w.table[NUM_ROWS - 1].numpy())
    assert not none[1].any() and not none[3].any()
