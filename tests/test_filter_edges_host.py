"""The filter step of the ranking paths at its edges, without a GPU: a plain restatement of the blp_filter contract
(include/blp_hip.h), float64 expectations, and the case builders that tests/test_gpu_filter_edges.py runs on the device.

* ``removed_rows`` restates which table rows a query loses, from the header's words alone (segment, exclude, ent2idx,
  row_base, the [0, N) test).  It is pinned against a brute-force scan of a toy graph and against FilterIndex.csr.
* "grid" problems hold table, relation and query values on a coarse binary grid (multiples of 1/8 of bounded magnitude):
  every score is exact in float32 and in float64 whatever the summation order, which ``problem`` asserts pair by pair
  (oracle.ref_port in float32 == numpy in float64).  The expected counts are then four numpy expressions; the C oracle
  (oracle.rank_counts with the CSR of removed_rows) is pinned to them on every grid case.
* "real" problems (a normalised random table, as test_gpu_parity.random_problem) and "nonfinite" ones (the same with a NaN
  row, +Inf / -Inf rows and a query whose true key is NaN) take the oracle with that CSR as their expectation.
* every case builder asserts that its filter reaches the edge it exists for; those assertions run here, on the CPU.

Queries: a problem has QMAX queries given by (fixed_row, rel_id, true_row); a Variant takes the first Q of them, with a flag
per query saying which side it replaces: plain blocks (the first q_head replace the head) or the evaluation loop's layout
(batch after batch of `batch` triples, each as [its head queries | its tail queries]).  The scores of both sides are kept.
"""
import collections
import functools

import numpy as np
import pytest
import torch

from conftest import REL_MODELS
from blp_amd import utils
from blp_amd.ops import SegmentFilter
from oracle import oracle as orc
from oracle import ref_port

STEP = 0.125          # the grid
TIES = 128            # queries 0 .. TIES - 1 of a grid problem own three rows: a copy of their true row, one step up, one down
N_ROWS = 777          # 13 tiles, the last of 9 rows
N_SLOTS = 2050        # 33 tiles = 33 partial slots of the small-block kernel (sum_partials' eight-load trip starts at 29)
N_TILES = 256 * 64 + 65  # more tiles than the small-block kernel has slots (kSmallMaxSlots = 256, rank_common.h)
QMAX = 383
CASES = ("long", "last_slot", "idmap", "exclude", "ties", "empty")

Variant = collections.namedtuple("Variant", "name Q head filter")
Layout = collections.namedtuple("Layout", "batch q_head Qs")  # Qs: (Q % 64 == 63 or 62, Q % 64 == 1 or 2)
PLAIN = Layout(0, 150, (383, 321))
HALF = Layout(0, 75, (191, 129))       # blocks the shipped dispatch still gives to the small-block kernel at N_SLOTS rows
TINY = Layout(0, 10, (24, None))       # ... and, the bilinear models, at N_TILES rows (below 400 000 pairs); no full workgroup


def loop_layout(batch):
    """2 n queries in the loop's layout cannot be odd: Q % 64 is 62 and 2; n = 191 and 161 are no multiples of 2 or 3."""
    return Layout(batch, None, (382, 322))


def head_flags(Q, layout):
    """Which queries replace the head: include/blp_hip.h, blp_rank_all (plain) and blp_rank_all_batches (the loop's layout)."""
    if layout.batch == 0:
        return np.arange(Q) < layout.q_head
    n, flags = Q // 2, []
    for first in range(0, n, layout.batch):
        nb = min(layout.batch, n - first)
        flags += [True] * nb + [False] * nb
    return np.asarray(flags)


# ------------------------------------------------------------------------------------------------ the contract, restated
def removed_rows(f, q, N):
    """The table rows query q loses (include/blp_hip.h, blp_filter)."""
    rows = set()
    for k in range(int(f.seg_lo[q]), int(f.seg_hi[q])):      # empty when hi <= lo
        v = int(f.values[k])
        if f.exclude is not None and v == int(f.exclude[q]):
            continue
        if f.ent2idx is not None:
            if not 0 <= v < len(f.ent2idx):
                continue
            v = int(f.ent2idx[v])
            if v < 0:
                continue
        row = v - int(f.row_base)
        if 0 <= row < N:
            rows.add(row)
    return rows


def removed_mask(f, Q, N):
    mask = np.zeros((Q, N), bool)
    for q in range(Q):
        mask[q, sorted(removed_rows(f, q, N))] = True
    return mask


def mask_csr(mask, extra=()):
    """CSR of a removal mask; ``extra`` columns are appended to every row's list."""
    rowptr, col = [0], []
    for q in range(mask.shape[0]):
        col += [int(c) for c in np.nonzero(mask[q])[0]] + list(extra)
        rowptr.append(len(col))
    return np.asarray(rowptr, np.int64), np.asarray(col, np.int64)


# ------------------------------------------------------------------------------------------------ scores
def score64(model, h, t, r):
    """models.py:222-248 in float64 numpy."""
    if model == "transe":
        return -np.abs(h + r - t).sum(-1)
    if model == "distmult":
        return (h * r * t).sum(-1)
    half = h.shape[-1] // 2
    h1, h2, t1, t2, r1, r2 = h[..., :half], h[..., half:], t[..., :half], t[..., half:], r[..., :half], r[..., half:]
    if model == "complex":
        return (r1 * h1 * t1 + r1 * h2 * t2 + r2 * h1 * t2 - r2 * h2 * t1).sum(-1)
    return (h1 * r1 * t2 + t1 * r2 * h2).sum(-1) / 2


def _all_pairs(fn, table, fixed, rel, head, chunk):
    out = []
    for q0 in range(0, fixed.shape[0], chunk):
        f, r, e = fixed[q0:q0 + chunk, None], rel[q0:q0 + chunk, None], table[None]
        out.append(fn(e, f, r) if head else fn(f, e, r))
    return out


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def problem(model, D, N, family, qmax=QMAX):
    p = Problem()
    p.model, p.D, p.N, p.family, p.qmax = model, D, N, family, qmax
    g = torch.Generator().manual_seed(1000 * D + N + 7 * REL_MODELS.index(model) + len(family))
    R = 11
    if family == "grid":
        table = torch.randint(-8, 9, (N, D), generator=g).float() * STEP
        rel = torch.randint(-4, 5, (R, D), generator=g).float() * STEP
    else:
        table = torch.randn(N, D, generator=g)
        table = torch.nn.functional.normalize(table, dim=-1) if model == "transe" else table * 0.1
        rel = (torch.rand(R, D, generator=g) - 0.5) * 0.25
    p.fixed_row = torch.randint(8, N, (qmax,), generator=g)
    p.rel_id = torch.randint(0, R, (qmax,), generator=g)
    p.true_row = torch.randint(8, N - 3 * TIES, (qmax,), generator=g)
    if family == "grid":
        for q in range(min(TIES, qmax)):
            base = N - 3 * TIES + 3 * q
            table[base:base + 3] = table[p.true_row[q]]
            table[base + 1, q % D] += STEP
            table[base + 2, q % D] -= STEP
    if family == "nonfinite":
        table[5, 3 % D] = float("nan")
        table[6, 2 % D] = float("inf")
        table[7] = float("-inf")
        p.true_row[3] = 5            # a true key that is NaN
        p.true_row[70] = 6
    p.table, p.rel = table, rel
    p.q_fixed, p.q_rel = table[p.fixed_row].clone(), rel[p.rel_id].clone()
    if family == "grid":
        t64, f64, r64 = table.double().numpy(), p.q_fixed.double().numpy(), p.q_rel.double().numpy()
        chunk = max(1, (1 << 21) // (N * D))
        for head in (True, False):
            s64 = np.concatenate(_all_pairs(functools.partial(score64, model), t64, f64, r64, head, chunk))
            s32 = torch.cat(_all_pairs(ref_port.SCORE_FNS[model], table, p.q_fixed, p.q_rel, head, chunk)).numpy()
            assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), s64)  # exact: the order cannot matter
            setattr(p, "S_h" if head else "S_t", s64)
    else:
        p.S_h = orc.score_all(model, orc.SIDE_HEAD, table.numpy(), p.q_fixed.numpy(), p.q_rel.numpy()).astype(np.float64)
        p.S_t = orc.score_all(model, orc.SIDE_TAIL, table.numpy(), p.q_fixed.numpy(), p.q_rel.numpy()).astype(np.float64)
    return p


def scores(p, v):
    """(S, s_true) of a variant's queries: (Q, N) and (Q,) float64."""
    S = np.where(v.head[:, None], p.S_h[:v.Q], p.S_t[:v.Q])
    return S, S[np.arange(v.Q), p.true_row[:v.Q].numpy()]


def numpy_counts(S, s_true, mask):
    gt, ge = S > s_true[:, None], S >= s_true[:, None]
    return np.stack([gt.sum(1), ge.sum(1), (gt & ~mask).sum(1), (ge & ~mask).sum(1)], 1).astype(np.int32)


def oracle_counts(p, v, mask, rows=None, table=None):
    """The C oracle on the candidate rows [rows[0], rows[1]) of ``table`` (default: the problem's own, all of it)."""
    table = (p.table if table is None else table).numpy()
    lo, hi = rows or (0, table.shape[0])
    out = np.zeros((v.Q, 4), np.int32)
    for side, idx in ((orc.SIDE_HEAD, np.nonzero(v.head)[0]), (orc.SIDE_TAIL, np.nonzero(~v.head)[0])):
        if len(idx):
            rowptr, col = mask_csr(mask[idx])
            out[idx] = orc.rank_counts(p.model, side, table[lo:hi], p.q_fixed.numpy()[idx], p.q_rel.numpy()[idx],
                                       q_true=p.table.numpy()[p.true_row.numpy()[idx]], filt_rowptr=rowptr, filt_col=col)
    return out


def expected(p, v, rows=None, table=None):
    """(Q, 4) int32 expectation of a variant, on the whole table or on the candidate shard ``rows`` = (lo, hi) -- whose
    filter then carries row_base = lo.  Grid problems: numpy on the float64 scores; the others: the oracle."""
    lo, hi = rows or (0, p.N)
    assert int(v.filter.row_base) == lo
    mask = removed_mask(v.filter, v.Q, hi - lo)
    if p.family != "grid":
        return oracle_counts(p, v, mask, rows, table)
    S, s_true = scores(p, v)
    return numpy_counts(S[:, lo:hi], s_true, mask)


# ------------------------------------------------------------------------------------------------ case builders
def _t(x):
    return torch.as_tensor(np.asarray(x, np.int64))


def assemble(p, Q, lists, rng, exclude=None, ent2idx=None, row_base=0):
    """A SegmentFilter over per-query value lists: the segments lie in `values` in a shuffled order, with live row numbers
    in the gaps between them (an entry read outside its segment changes a count)."""
    values, lo, hi = [], np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    for q in rng.permutation(Q):
        values += [int(x) for x in rng.integers(0, p.N, int(rng.integers(0, 3)))]
        lo[q] = len(values)
        values += [int(x) for x in lists[q]]
        hi[q] = len(values)
    values += [int(x) for x in rng.integers(0, p.N, 2)]
    return SegmentFilter(_t(lo), _t(hi), _t(values), None if exclude is None else _t(exclude),
                         None if ent2idx is None else _t(ent2idx), row_base)


def pick(p, S, s_true, q, k, rng):
    """k distinct rows, none the true one: those at or above the true score first (a miss then moves a filtered count)."""
    true = int(p.true_row[q])
    strong = [int(r) for r in np.nonzero(S[q] >= s_true[q])[0] if r != true]
    rng.shuffle(strong)
    rows = strong[:(k + 1) // 2]
    while len(rows) < k:
        r = int(rng.integers(0, p.N))
        if r != true and r not in rows:
            rows.append(r)
    return rows


def _variant(p, name, Q, layout, make):
    head = head_flags(Q, layout)
    v0 = Variant(name, Q, head, None)
    S, s_true = scores(p, v0)
    return v0._replace(filter=make(S, s_true))


def case_long(p, layout, rng):
    Q, N, true = layout.Qs[0], p.N, p.true_row.numpy()

    def make(S, s_true):
        lists = [[] for _ in range(Q)]
        lists[7] = [int(r) for r in rng.permutation(N) if r != true[7]]       # workgroup 0: one query holds it all
        for q in range(64, 128):                                                # workgroup 1: 64 x 5 entries
            lists[q] = pick(p, S, s_true, q, 5, rng)
        lists[130] = [int(r) for r in rng.permutation(N)]                        # workgroup 2: every row, the true one protected
        return assemble(p, Q, lists, rng, exclude=true[:Q])
    v = _variant(p, "long", Q, layout, make)
    n = (v.filter.seg_hi - v.filter.seg_lo).numpy()
    assert n[7] >= 700 and n[:64].sum() == n[7] and n[64:128].sum() == 320 > 256 and (n[64:128] == 5).all()
    assert n[130] == N and int(true[130]) in v.filter.values[int(v.filter.seg_lo[130]):int(v.filter.seg_hi[130])].tolist()
    if p.family == "grid":
        assert expected(p, v)[130, 2:].tolist() == [0, 1]
    return [v]


def case_last_slot(p, layout, rng):
    out = []
    for Q in layout.Qs:
        assert Q % 64 in ((1, 63) if layout.batch == 0 else (2, 62)) and Q > 128

        def make(S, s_true):
            lists = [[] for _ in range(Q)]
            for q in (127, Q - 1):
                lists[q] = pick(p, S, s_true, q, 6, rng)
            return assemble(p, Q, lists, rng, exclude=p.true_row.numpy()[:Q])
        v = _variant(p, "last_slot-Q%d" % Q, Q, layout, make)
        n = (v.filter.seg_hi - v.filter.seg_lo).numpy()
        assert n[127] == 6 and n[Q - 1] == 6 and n.sum() == 12 and (Q - 1) // 64 == Q // 64 and (Q - 1) % 64 in (0, 1, 61, 62)
        out.append(v)
    return out


def case_idmap(p, layout, rng):
    Q, N, true = layout.Qs[0], p.N, p.true_row.numpy()
    n_ids = N + 200
    ids = rng.permutation(n_ids)
    ent2idx = np.full(n_ids, -1, np.int64)
    ent2idx[ids[:N]] = np.arange(N)                     # injective on the N live ids; 200 holes
    id_of = np.empty(N, np.int64)
    id_of[np.arange(N)] = ids[:N]
    holes = ids[N:]
    dropped = collections.Counter()

    def make_map(S, s_true):
        lists = []
        for q in range(Q):
            rows = pick(p, S, s_true, q, 5, rng)
            vals = [int(id_of[rows[0]]), int(holes[q % 200]), int(id_of[rows[1]]), n_ids + q, int(id_of[rows[2]]),
                    -1 - (q % 5), int(id_of[rows[3]]), (1 << 40) + int(id_of[rows[4]])]
            if q % 4 == 0:
                vals.insert(3, int(id_of[true[q]]))      # the triple's own entity: exclude is an id, compared before the map
            lists.append(vals)
        return assemble(p, Q, lists, rng, exclude=id_of[true[:Q]], ent2idx=ent2idx)

    def make_rows(S, s_true):
        lists = []
        for q in range(Q):
            rows = pick(p, S, s_true, q, 5, rng)          # (2^33 + a live row: its low 32 bits alone would be a row)
            lists.append([rows[0], N, rows[1], -1, rows[2], N + 5 + q, rows[3], -3 - q, rows[4], (1 << 33) + rows[0]])
        return assemble(p, Q, lists, rng)               # no ent2idx: values are rows already; no exclude
    a, b = _variant(p, "idmap-ent2idx", Q, layout, make_map), _variant(p, "idmap-rows", Q, layout, make_rows)
    for v in (a, b):
        f = v.filter
        for q in range(Q):
            kept = removed_rows(f, q, N)
            seg = f.values[int(f.seg_lo[q]):int(f.seg_hi[q])].tolist()
            for i, val in enumerate(seg):
                if f.ent2idx is not None:
                    why = "negative" if val < 0 else "beyond" if val >= n_ids else "hole" if ent2idx[val] < 0 else None
                    row = None if why else int(ent2idx[val])
                else:
                    why = "negative" if val < 0 else "beyond" if val >= N else None
                    row = None if why else val
                if why:                                   # dropped for this reason, and a neighbour in the segment survives
                    near = [seg[j] for j in (i - 1, i + 1) if 0 <= j < len(seg)]
                    near_rows = [int(ent2idx[x]) if f.ent2idx is not None and 0 <= x < n_ids else x for x in near]
                    assert any(r in kept for r in near_rows)
                    dropped[(v.name, why)] += 1
                elif row is not None and row != int(true[q]):
                    assert row in kept
            assert int(true[q]) not in kept
    assert all(dropped[(a.name, why)] >= 1 for why in ("negative", "beyond", "hole"))
    assert all(dropped[(b.name, why)] >= 1 for why in ("negative", "beyond"))
    return [a, b]


def case_exclude(p, layout, rng):
    Q, true = layout.Qs[0], p.true_row.numpy()
    hits = []

    def make(S, s_true):
        lists, exclude = [], true[:Q].copy()
        for q in range(Q):
            rows = pick(p, S, s_true, q, 6, rng)
            lists.append(rows)
            if q % 3 == 0 and S[q, rows[0]] >= s_true[q]:
                exclude[q] = rows[0]                    # a listed value that is at or above the true entity stays
                hits.append(q)
        return assemble(p, Q, lists, rng, exclude=exclude)
    v = _variant(p, "exclude-hit", Q, layout, make)
    assert len(hits) >= 8
    for q in hits:
        assert int(v.filter.exclude[q]) not in removed_rows(v.filter, q, p.N)
    # the same lists without `exclude`: no list holds the true entity, so the header defines the result -- every listed row goes
    w = v._replace(name="exclude-none", filter=v.filter._replace(exclude=None))
    for q in hits:
        assert int(v.filter.exclude[q]) in removed_rows(w.filter, q, p.N)
    return [v, w]


def case_ties(p, layout, rng):
    assert p.family == "grid"
    Q = layout.Qs[0]

    def make(S, s_true):
        lists = [[] for _ in range(Q)]
        for q in range(TIES):
            base = p.N - 3 * TIES + 3 * q
            lists[q] = [base + 2, base, base + 1] + pick(p, S, s_true, q, 2, rng)
            lists[q] = list(dict.fromkeys(lists[q]))
        return assemble(p, Q, lists, rng, exclude=p.true_row.numpy()[:Q])
    v = _variant(p, "ties", Q, layout, make)
    S, s_true = scores(p, v)
    above = below = 0
    for q in range(TIES):
        base = p.N - 3 * TIES + 3 * q
        assert S[q, base] == s_true[q] and np.array_equal(p.table[base].numpy(), p.table[p.true_row[q]].numpy())
        above += bool((S[q, base + 1:base + 3] > s_true[q]).any())
        below += bool((S[q, base + 1:base + 3] < s_true[q]).any())
    assert above >= TIES // 4 and below >= TIES // 4       # one grid step up and one down, as scores
    c = expected(p, v)
    assert ((c[:, 1] - c[:, 3]) != (c[:, 0] - c[:, 2])).sum() * 4 >= Q
    return [v]


def case_empty(p, layout, rng):
    Q = layout.Qs[0]
    live = _t(rng.integers(0, p.N, 50))
    at = _t(rng.integers(0, 50, Q))
    eq = Variant("empty-hi_eq_lo", Q, head_flags(Q, layout), SegmentFilter(at, at.clone(), live, None, None, 0))

    def make(S, s_true):
        f = assemble(p, Q, [pick(p, S, s_true, q, 3, rng) if q % 2 else [] for q in range(Q)], rng, exclude=p.true_row.numpy()[:Q])
        lo, hi = f.seg_lo.clone(), f.seg_hi.clone()
        for q in range(0, Q, 2):                          # hi < lo, by 1 .. 9, over live values
            lo[q], hi[q] = 10 + q % 9, 9
        return f._replace(seg_lo=lo, seg_hi=hi)
    lt = _variant(p, "empty-hi_lt_lo", Q, layout, make)
    assert (lt.filter.seg_hi < lt.filter.seg_lo).sum() >= Q // 2 and (lt.filter.seg_hi > lt.filter.seg_lo).sum() >= Q // 2 - 1
    zero = Variant("empty-no_values", Q, eq.head, SegmentFilter(_t(np.zeros(Q)), _t(np.zeros(Q)), _t([]), None, None, 0))
    assert zero.filter.values.numel() == 0
    for v in (eq, zero):
        assert not removed_mask(v.filter, Q, p.N).any()
    assert not removed_mask(lt.filter, Q, p.N)[0::2].any() and removed_mask(lt.filter, Q, p.N)[1::2].any(1).all()
    return [eq, lt, zero]


SHARDS = ((0, 100), (100, 101), (101, None))


def case_shards(p, layout, rng):
    """One Variant per candidate shard plus the unsharded one (first): the same global lists, row_base = the shard's first row."""
    Q, N = layout.Qs[0], p.N

    def make(S, s_true):
        lists = []
        for q in range(Q):
            rows = [r for r in pick(p, S, s_true, q, 4, rng) if r > 101]
            extra = [int(rng.integers(0, 100)), 100, N + q] if q % 3 == 0 else [N + q] if q % 3 == 1 else [int(rng.integers(0, 100))]
            lists.append([r for r in dict.fromkeys(rows + extra) if r != int(p.true_row[q])])
        return assemble(p, Q, lists, rng, exclude=p.true_row.numpy()[:Q])
    whole = _variant(p, "shards-whole", Q, layout, make)
    out = [whole]
    for lo, hi in SHARDS:
        hi = N if hi is None else hi
        v = whole._replace(name="shards-%d-%d" % (lo, hi), filter=whole.filter._replace(row_base=lo))
        assert removed_mask(v.filter, Q, hi - lo).any()    # entries fall in every shard
        out.append(v)
    n_in = sum(removed_mask(v.filter, Q, (N if hi is None else hi) - lo).sum() for v, (lo, hi) in zip(out[1:], SHARDS))
    assert n_in == removed_mask(whole.filter, Q, N).sum() < (whole.filter.seg_hi - whole.filter.seg_lo).sum()  # ... and in none
    return out


def shard_rows(p):
    return [(lo, p.N if hi is None else hi) for lo, hi in SHARDS]


def case_nonfinite(p, layout, rng):
    assert p.family == "nonfinite"
    Q = layout.Qs[0]

    def make(S, s_true):
        lists = [[5, 6, 7] + [r for r in pick(p, S, s_true, q, 3, rng) if r > 7] for q in range(Q)]
        for q in range(Q):
            lists[q] = [r for r in lists[q] if r != int(p.true_row[q])]
        return assemble(p, Q, lists, rng, exclude=p.true_row.numpy()[:Q])
    v = _variant(p, "nonfinite", Q, layout, make)
    assert torch.isnan(p.table[5]).any() and torch.isinf(p.table[6]).any() and (p.table[7] == float("-inf")).all()
    S, s_true = scores(p, v)
    assert np.isnan(s_true[3]) and np.isnan(S[:, 5]).all()  # a NaN key: every comparison against it is false
    c = expected(p, v)
    assert (c[3] == 0).all()
    return [v]


BUILDERS = {"long": case_long, "last_slot": case_last_slot, "idmap": case_idmap, "exclude": case_exclude, "ties": case_ties,
            "empty": case_empty, "shards": case_shards, "nonfinite": case_nonfinite}


@functools.lru_cache(maxsize=None)
def build(case, model, D, N, family, layout=PLAIN, qmax=QMAX):
    """The variants of a case with their expectations: [(Variant, counts)] (shards: on the variant's own candidate rows)."""
    p = problem(model, D, N, family, qmax)
    rng = np.random.default_rng(sorted(BUILDERS).index(case) + 31 * D + N)
    variants = BUILDERS[case](p, layout, rng)
    if case == "shards":
        rows = [None] + shard_rows(p)
        return [(v, torch.from_numpy(expected(p, v, r))) for v, r in zip(variants, rows)]
    return [(v, torch.from_numpy(expected(p, v))) for v in variants]


def families(case):
    return {"ties": ("grid",), "nonfinite": ("nonfinite",), "last_slot": ("grid",), "empty": ("grid",)}.get(case, ("grid", "real"))


# ------------------------------------------------------------------------------------------------ host tests
def _toy_graph():
    g = torch.Generator().manual_seed(5)
    edges = torch.stack([torch.randint(0, 30, (400,), generator=g), torch.randint(0, 30, (400,), generator=g),
                         torch.randint(0, 4, (400,), generator=g)], 1)
    ent2idx = torch.full((40,), -1, dtype=torch.long)
    live = torch.randperm(30, generator=g)[:24]
    ent2idx[live] = torch.arange(24)
    return edges, ent2idx, edges[torch.randperm(400, generator=g)[:60]]


def test_restatement_equals_a_scan_of_the_edges_and_filter_index_csr():
    edges, ent2idx, triples = _toy_graph()
    index = utils.FilterIndex(edges)
    B, N = triples.shape[0], 24
    for row_base, n_rows in ((0, N), (10, 9)):
        seg = index.segments(triples, ent2idx, "cpu", row_base=row_base)
        for q in range(2 * B):
            h, t, r = (int(x) for x in triples[q % B])
            if q < B:   # head-replacing: the known heads of (?, r, t), the triple's own head kept (utils.py:46-83)
                ids = {int(e[0]) for e in edges if int(e[1]) == t and int(e[2]) == r and int(e[0]) != h}
            else:
                ids = {int(e[1]) for e in edges if int(e[0]) == h and int(e[2]) == r and int(e[1]) != t}
            want = {int(ent2idx[i]) - row_base for i in ids if ent2idx[i] >= 0 and 0 <= int(ent2idx[i]) - row_base < n_rows}
            assert removed_rows(seg, q, n_rows) == want, (q, row_base)
    rowptr, col = index.csr(triples, ent2idx)
    seg = index.segments(triples, ent2idx, "cpu")
    for q in range(2 * B):
        assert removed_rows(seg, q, N) == set(col[int(rowptr[q]):int(rowptr[q + 1])].tolist())
    assert any(removed_rows(seg, q, N) for q in range(2 * B))


def test_restatement_on_hand_made_entries():
    f = SegmentFilter(_t([0, 6, 4]), _t([6, 6, 2]), _t([3, 9, -1, 7, 100, 5]), _t([9, 0, 0]), None, 2)
    assert removed_rows(f, 0, 5) == {1, 3} and removed_rows(f, 0, 6) == {1, 5, 3}       # 9 excluded; -1, 100 out; 7 - 2 = 5
    assert removed_rows(f, 1, 6) == set() and removed_rows(f, 2, 6) == set()             # hi == lo, hi < lo
    m = SegmentFilter(_t([0]), _t([5]), _t([0, 1, 2, 3, -2]), _t([1]), _t([4, 0, -1]), 0)
    assert removed_rows(m, 0, 5) == {4} and removed_rows(m, 0, 4) == set()               # id 1 excluded, 2 a hole, 3 beyond, -2 negative


@pytest.mark.parametrize("model", REL_MODELS)
def test_head_flags_and_grid_scores(model):
    assert head_flags(7, Layout(0, 3, None)).tolist() == [True] * 3 + [False] * 4
    assert head_flags(10, loop_layout(2)).tolist() == [True, True, False, False, True, True, False, False, True, False]
    assert head_flags(8, loop_layout(3)).tolist() == [True] * 3 + [False] * 3 + [True, False]
    p = problem(model, 64, N_ROWS, "grid")                 # (asserts float32 == float64 for every pair, both sides)
    q, n = 11, 300
    h, t, r = p.table[n].double().numpy(), p.q_fixed[q].double().numpy(), p.q_rel[q].double().numpy()
    assert p.S_h[q, n] == score64(model, h, t, r) and p.S_t[q, n] == score64(model, t, h, r)
    assert p.S_h[q, n] == float(orc.score_pairs(model, p.table[n:n + 1].numpy(), p.q_fixed[q:q + 1].numpy(), p.q_rel[q:q + 1].numpy())[0])


HOST_SHAPES = [("transe", 64, PLAIN), ("distmult", 128, PLAIN), ("complex", 64, loop_layout(3)), ("simple", 128, loop_layout(2)),
               ("transe", 100, PLAIN)]


@pytest.mark.parametrize("case", CASES + ("shards",))
@pytest.mark.parametrize("model,D,layout", HOST_SHAPES, ids=lambda x: str(x) if not isinstance(x, Layout) else "batch%d" % x.batch)
def test_builders_reach_their_edges_and_the_oracle_agrees_on_the_grid(case, model, D, layout):
    """Every builder's own assertions hold, and on the grid the C oracle, given the CSR of removed_rows, returns the numpy counts."""
    p = problem(model, D, N_ROWS, "grid")
    rows = [None] + shard_rows(p) if case == "shards" else None
    for i, (v, want) in enumerate(build(case, model, D, N_ROWS, "grid", layout)):
        r = rows[i] if rows else None
        lo, hi = r or (0, p.N)
        got = oracle_counts(p, v, removed_mask(v.filter, v.Q, hi - lo), r)
        assert np.array_equal(got, want.numpy()), v.name
        assert (want[:, 2] <= want[:, 0]).all() and (want[:, 3] <= want[:, 1]).all()
        if r is None:
            assert (want[:, 1] >= 1).all()                   # the true entity is a row of the table
    if case == "shards":
        parts = build(case, model, D, N_ROWS, "grid", layout)
        assert torch.equal(parts[0][1], sum(c for _, c in parts[1:]))


@pytest.mark.parametrize("model", ["transe", "complex"])
def test_real_and_nonfinite_builders(model):
    for case in ("long", "idmap", "exclude", "shards"):
        assert build(case, model, 64, N_ROWS, "real")
    (v, want), = build("nonfinite", model, 64, N_ROWS, "nonfinite")
    assert want.shape == (v.Q, 4)
    parts = build("shards", model, 64, N_ROWS, "real")
    assert torch.equal(parts[0][1], sum(c for _, c in parts[1:]))
