"""Per-query candidate lists on the MI355X (blp_rank_lists through blp_amd.ops.rank_lists and ranking.rank_candidates): counts
equal and scores bit-identical to the C oracle's (oracle.score_all / score_pairs) and to rank_candidates' CPU route on the same
tensors -- every model and width, list lengths around the 64-entry step and past a workgroup's chunk, skipped entries,
duplicates, ties, NaN / inf / -0, filters, 16-bit tables, candidate shards, two threads on two streams, one larger shape."""
import threading

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden

pytestmark = pytest.mark.gpu

SIDE_HEAD, SIDE_TAIL = 0, 1
LENGTHS = (0, 1, 63, 64, 65, 200, 1500)  # 1 500 > the 1 024 entries a workgroup owns: the split-list path
NAN_BITS = 0x7fc00000


@pytest.fixture(scope="module")
def ops():
    from blp_amd import ops as _ops
    return _ops


def random_problem(model, N, D, Q, R=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(N, D, generator=g)
    table = torch.nn.functional.normalize(table, dim=-1) if model == "transe" else table * 0.1
    rel = (torch.rand(R, D, generator=g) - 0.5) * 0.25
    return (table, rel, torch.randint(0, N, (Q,), generator=g), torch.randint(0, R, (Q,), generator=g),
            torch.randint(0, N, (Q,), generator=g))


def random_lists(Q, N, lengths=LENGTHS, seed=0, specials=True):
    """Lists of the given lengths (cycled over the queries): uniform rows, 30 % of the entries duplicates of earlier ones, and
    -1, N - 1, N, N + 7 planted where a list is long enough."""
    rng = np.random.default_rng(seed)
    lists = []
    for q in range(Q):
        n = lengths[q % len(lengths)]
        rows = rng.integers(0, N, n)
        if n > 1:
            dup = rng.random(n) < 0.3
            rows[dup] = rows[rng.integers(0, n, int(dup.sum()))]
        if specials and n >= 63:
            rows[[0, 7, 31, n - 1]] = (-1, N - 1, N, N + 7)
        lists.append(rows.astype(np.int64))
    ptr = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int64)
    return ptr, np.concatenate(lists) if lists else np.zeros(0, np.int64)


def oracle_pred(oracle, model, table, fixed_vec, rel_vec, q_head):
    parts = []
    if q_head:
        parts.append(oracle.score_all(model, SIDE_HEAD, table, fixed_vec[:q_head], rel_vec[:q_head]))
    if q_head < len(fixed_vec):
        parts.append(oracle.score_all(model, SIDE_TAIL, table, fixed_vec[q_head:], rel_vec[q_head:]))
    return np.concatenate(parts)


def true_scores(oracle, model, true_vec, fixed_vec, rel_vec, q_head):
    return np.concatenate((oracle.score_pairs(model, true_vec[:q_head], fixed_vec[:q_head], rel_vec[:q_head]),
                           oracle.score_pairs(model, fixed_vec[q_head:], true_vec[q_head:], rel_vec[q_head:])))


def expected(pred, true, ptr, rows, row_base=0, removed=None):
    """counts (Q, 4), scores (nnz,) and the mask of skipped entries (nnz,) read off the oracle's (Q, N) matrix of the local
    table: rows outside are skipped."""
    Q, N = pred.shape
    counts = np.zeros((Q, 4), np.int32)
    scores = np.full(len(rows), np.nan, np.float32)
    skipped = np.ones(len(rows), bool)
    for q in range(Q):
        local = rows[ptr[q]:ptr[q + 1]] - row_base
        ok = (local >= 0) & (local < N)
        s = pred[q, local[ok]]
        seg = scores[ptr[q]:ptr[q + 1]]
        seg[ok] = s
        skipped[ptr[q]:ptr[q + 1]] = ~ok
        keep = np.ones(len(s), bool) if removed is None else ~removed[q, local[ok]]
        with np.errstate(invalid="ignore"):
            gt, ge = s > true[q], s >= true[q]
        counts[q] = (gt.sum(), ge.sum(), (gt & keep).sum(), (ge & keep).sum())
    return counts, scores, skipped


def check(got, want, what=""):
    """want: (counts, scores[, skipped]); without the mask every NaN of the expected scores is a skipped entry.  A skipped
    entry's slot holds exactly NAN_BITS.  A score that is NaN by arithmetic (a NaN row, inf - inf) must be a NaN: which NaN
    a processor produces is its own (x86 gives inf - inf the sign bit, the GPU does not), so its bits are not compared."""
    counts, scores = got
    want_counts, want_scores = want[0], want[1]
    if counts is not None:
        assert np.array_equal(counts.cpu().numpy(), want_counts), what
    if scores is not None:
        s = scores.cpu().numpy()
        nan = np.isnan(want_scores)
        skipped = want[2] if len(want) > 2 else nan
        assert np.array_equal(np.isnan(s), nan), what
        assert np.array_equal(s[~nan].view(np.int32), want_scores[~nan].view(np.int32)), what
        assert (s[skipped].view(np.int32) == NAN_BITS).all(), what


def run(ops, model, table, source, fixed, rel, rel_ids, q_head, ptr, rows, true_row, **kw):
    dev = "cuda"
    t = lambda a: None if a is None else torch.as_tensor(a).to(dev)
    tab = table.to(dev)
    src = tab if source is table else source.to(dev)
    return ops.rank_lists(model, tab, src, t(fixed), rel.to(dev), t(rel_ids), q_head, t(ptr), t(rows), true_row=t(true_row),
                          want_scores=True, **kw)


CASES = [(m, D) for m in REL_MODELS for D in (64, 128, 256)] + [("transe", 300), ("transe", 768)]


@pytest.mark.parametrize("model,D", CASES)
def test_counts_and_scores_match_the_oracle(ops, oracle, model, D):
    N, Q = 1000, 12
    table, rel, fixed, rel_ids, true_row = random_problem(model, N, D, Q, seed=D)
    ptr, rows = random_lists(Q, N, seed=D + 1)
    f, r, tv = table[fixed].numpy(), rel[rel_ids].numpy(), table[true_row].numpy()
    for q_head in (0, 5, Q):
        pred = oracle_pred(oracle, model, table.numpy(), f, r, q_head)
        true = true_scores(oracle, model, tv, f, r, q_head)
        assert np.array_equal(true.view(np.int32), pred[np.arange(Q), true_row.numpy()].view(np.int32))
        want = expected(pred, true, ptr, rows)
        check(run(ops, model, table, table, fixed, rel, rel_ids, q_head, ptr, rows, true_row), want, (model, D, q_head))
        if q_head == 5:  # scores alone (no true_row, no workspace); counts alone
            c, s = run(ops, model, table, table, fixed, rel, rel_ids, q_head, ptr, rows, None)
            assert c is None
            check((None, s), want)
            dev = lambda a: torch.as_tensor(a).cuda()
            c, s = ops.rank_lists(model, table.cuda(), table.cuda(), dev(fixed), rel.cuda(), dev(rel_ids), q_head, dev(ptr), dev(rows),
                                  true_row=dev(true_row))
            assert s is None
            check((c, None), want)


@pytest.mark.parametrize("model", ["transe", "complex"])
def test_ties_with_the_true_entity(ops, oracle, model):
    N, D, Q = 1000, 128, 12
    table, rel, fixed, rel_ids, true_row = random_problem(model, N, D, Q, seed=3)
    g = torch.Generator().manual_seed(4)
    dups = torch.randperm(N, generator=g)[:N // 20]  # 5 % of the rows are copies of some query's true entity
    table[dups] = table[true_row[torch.randint(0, Q, (len(dups),), generator=g)]]
    ptr, rows = random_lists(Q, N, seed=5)
    f, r = table[fixed].numpy(), rel[rel_ids].numpy()
    pred = oracle_pred(oracle, model, table.numpy(), f, r, 5)
    true = pred[np.arange(Q), true_row.numpy()]
    want = expected(pred, true, ptr, rows)
    assert (want[0][:, 1] > want[0][:, 0]).sum() >= 3, "ties must occur"
    check(run(ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, true_row), want)


@pytest.mark.parametrize("model", REL_MODELS)
def test_nan_inf_and_signed_zero_rows(ops, oracle, model):
    N, D, Q = 1000, 64, 12
    table, rel, fixed, rel_ids, true_row = random_problem(model, N, D, Q, seed=6)
    table[10] = float("nan")
    table[11, 3] = float("inf")
    table[12, 5] = float("-inf")
    table[13] = 0.0
    table[14] = -0.0
    table[15, ::2] = -0.0
    table[15, 1::2] = 0.0
    true_row[0], true_row[7] = 10, 13  # a NaN true score; a zero one
    rel[0] = -0.0
    ptr, rows = random_lists(Q, N, lengths=(64, 200), seed=7, specials=False)
    rows[ptr[:-1, None] + np.arange(6)] = np.arange(10, 16)  # every list meets the special rows
    f, r = table[fixed].numpy(), rel[rel_ids].numpy()
    pred = oracle_pred(oracle, model, table.numpy(), f, r, 5)
    true = pred[np.arange(Q), true_row.numpy()]
    want = expected(pred, true, ptr, rows)
    if model != "transe":
        assert (want[1].view(np.int32) == np.int32(-2 ** 31)).any() or (want[1] == 0).any()
    check(run(ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, true_row), want, model)


def segment_filter(ops, lists, exclude, ent2idx, row_base, dev="cuda"):
    lo = np.cumsum([0] + [len(x) for x in lists[:-1]]).astype(np.int64)
    hi = lo + np.array([len(x) for x in lists], np.int64)
    values = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(1, np.int64)])
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.int64)).to(dev)
    return ops.SegmentFilter(t(lo), t(hi), t(values), t(exclude), t(ent2idx), row_base)


def removed_mask(lists, exclude, ent2idx, N, row_base=0):
    out = np.zeros((len(lists), N), bool)
    for q, seg in enumerate(lists):
        for v in seg:
            if exclude is not None and v == exclude[q]:
                continue
            row = v if ent2idx is None else (ent2idx[v] if 0 <= v < len(ent2idx) else -1)
            row -= row_base
            if 0 <= row < N:
                out[q, row] = True
    return out


@pytest.mark.parametrize("model", ["transe", "complex"])
def test_filters(ops, oracle, model):
    N, D, Q = 1000, 128, 12
    table, rel, fixed, rel_ids, true_row = random_problem(model, N, D, Q, seed=8)
    ptr, rows = random_lists(Q, N, seed=9)
    f, r = table[fixed].numpy(), rel[rel_ids].numpy()
    pred = oracle_pred(oracle, model, table.numpy(), f, r, 5)
    true = pred[np.arange(Q), true_row.numpy()]
    rng = np.random.default_rng(10)
    members = lambda q, n: rng.choice(rows[ptr[q]:ptr[q + 1]], n) if ptr[q + 1] > ptr[q] else np.zeros(0, np.int64)

    # (a) segments of rows that remove list members (out-of-range values among them), one of them the query's own entity
    segs = [np.concatenate((members(q, 9), rng.integers(0, N, 5), [-1, N + 3])) for q in range(Q)]
    exclude = np.array([segs[q][0] for q in range(Q)], np.int64)
    want = expected(pred, true, ptr, rows, removed=removed_mask(segs, exclude, None, N))
    assert (want[0][:, 3] < want[0][:, 1]).any()
    got = run(ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, true_row, filter=segment_filter(ops, segs, exclude, None, 0))
    check(got, want, "rows")
    no_ex = expected(pred, true, ptr, rows, removed=removed_mask(segs, None, None, N))
    got = run(ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, true_row, filter=segment_filter(ops, segs, None, None, 0))
    check(got, no_ex, "rows, nothing exempt")

    # (b) entity ids through an ent2idx with -1 entries
    ent2idx = rng.permutation(N + 200).astype(np.int64)
    ent2idx[ent2idx >= N] = -1
    row2id = np.full(N, -1, np.int64)
    row2id[ent2idx[ent2idx >= 0]] = np.nonzero(ent2idx >= 0)[0]
    id_segs = [np.concatenate((row2id[np.clip(members(q, 9), 0, N - 1)], rng.integers(0, N + 200, 6), [N + 500, -2])) for q in range(Q)]
    id_ex = np.array([s[0] for s in id_segs], np.int64)
    want = expected(pred, true, ptr, rows, removed=removed_mask(id_segs, id_ex, ent2idx, N))
    got = run(ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, true_row, filter=segment_filter(ops, id_segs, id_ex, ent2idx, 0))
    check(got, want, "ids")

    # (c) a 5 000-entry segment; (d) a query whose whole list is filtered
    big = [np.zeros(0, np.int64) for _ in range(Q)]
    big[6] = rng.integers(0, N, 5000)
    big[5] = rows[ptr[5]:ptr[6]].copy()
    big[4] = np.arange(N)
    rm = removed_mask(big, None, None, N)
    want = expected(pred, true, ptr, rows, removed=rm)
    assert (want[0][[4, 5], 2:] == 0).all() and want[0][5, 1] > 0
    got = run(ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, true_row, filter=segment_filter(ops, big, None, None, 0))
    check(got, want, "long segment")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("model,D", [("transe", 128), ("transe", 300), ("distmult", 64), ("complex", 128), ("simple", 256)])
def test_16_bit_table_equals_the_widened_table(ops, oracle, model, D, dtype):
    N, Q = 1000, 12
    table, rel, fixed, rel_ids, true_row = random_problem(model, N, D, Q, seed=11)
    t16 = table.to(dtype)
    wide = t16.float()
    ptr, rows = random_lists(Q, N, seed=12)
    src = wide[torch.cat((fixed, true_row))]
    idx_f, idx_t = np.arange(Q), np.arange(Q, 2 * Q)
    segs = [rows[ptr[q]:ptr[q + 1]][:7] for q in range(Q)]
    got16 = run(ops, model, t16, src, idx_f, rel, rel_ids, 5, ptr, rows, idx_t, filter=segment_filter(ops, segs, None, None, 0))
    got32 = run(ops, model, wide, src, idx_f, rel, rel_ids, 5, ptr, rows, idx_t, filter=segment_filter(ops, segs, None, None, 0))
    assert torch.equal(got16[0], got32[0])
    assert torch.equal(got16[1].view(torch.int32), got32[1].view(torch.int32))
    f, r = wide[fixed].numpy(), rel[rel_ids].numpy()
    pred = oracle_pred(oracle, model, wide.numpy(), f, r, 5)
    check(got16, expected(pred, pred[np.arange(Q), true_row.numpy()], ptr, rows, removed=removed_mask(segs, None, None, N)))


@pytest.mark.parametrize("model", ["transe", "simple"])
def test_two_candidate_shards_add_up(ops, oracle, model):
    N, D, Q = 1000, 128, 12
    table, rel, fixed, rel_ids, true_row = random_problem(model, N, D, Q, seed=13)
    ptr, rows = random_lists(Q, N, seed=14)
    f, r = table[fixed].numpy(), rel[rel_ids].numpy()
    pred = oracle_pred(oracle, model, table.numpy(), f, r, 5)
    true = pred[np.arange(Q), true_row.numpy()]
    segs = [rows[ptr[q]:ptr[q + 1]][:9] for q in range(Q)]
    whole = expected(pred, true, ptr, rows, removed=removed_mask(segs, None, None, N))
    total = np.zeros((Q, 4), np.int32)
    seen = np.zeros(len(rows), int)
    for lo, hi in ((0, 517), (517, N)):
        got = run(ops, model, table[lo:hi], table, fixed, rel, rel_ids, 5, ptr, rows, true_row, row_base=lo,
                  filter=segment_filter(ops, segs, None, None, lo))
        check(got, expected(pred[:, lo:hi], true, ptr, rows, row_base=lo, removed=removed_mask(segs, None, None, hi - lo, lo)), (lo, hi))
        s = got[1].cpu().numpy()
        assert np.array_equal(np.isnan(s), ~((rows >= lo) & (rows < hi)) | np.isnan(whole[1]))
        seen += ~np.isnan(s)
        total += got[0].cpu().numpy()
    assert np.array_equal(total, whole[0])
    assert (seen <= 1).all()


def test_two_threads_on_two_streams(ops, oracle):
    N, D, Q = 1000, 128, 12
    problems = []
    for i, model in enumerate(("transe", "complex")):
        table, rel, fixed, rel_ids, true_row = random_problem(model, N, D, Q, seed=20 + i)
        ptr, rows = random_lists(Q, N, seed=30 + i)
        dev = [x.cuda() for x in (table, rel, fixed, rel_ids, true_row, torch.from_numpy(ptr), torch.from_numpy(rows))]
        single = ops.rank_lists(model, dev[0], dev[0], dev[2], dev[1], dev[3], 5, dev[5], dev[6], true_row=dev[4], want_scores=True)
        problems.append((model, dev, single))
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def worker(i):
        try:
            model, dev, _ = problems[i]
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for _ in range(5):
                    out = ops.rank_lists(model, dev[0], dev[0], dev[2], dev[1], dev[3], 5, dev[5], dev[6], true_row=dev[4], want_scores=True)
            stream.synchronize()
            results[i] = out
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    for i in range(2):
        assert torch.equal(results[i][0], problems[i][2][0])
        assert torch.equal(results[i][1].view(torch.int32), problems[i][2][1].view(torch.int32))


@pytest.mark.parametrize("model", ["transe", "complex"])
def test_larger_shape_against_gathered_oracle_scores(ops, oracle, model):
    """2 048 queries x 500 candidates against a 300 001-row table: the expected counts are the oracle's scores of the gathered
    (query, candidate) pairs compared with its true scores -- not a ranking of the whole table."""
    N, D, Q, C = 300_001, 128, 2048, 500
    table, rel, fixed, rel_ids, true_row = random_problem(model, N, D, Q, seed=40)
    g = torch.Generator().manual_seed(41)
    cand = torch.randint(0, N, (Q, C), generator=g)
    cand[:, 0] = true_row  # the true entity is listed
    cand[:, 1] = N - 1
    q_head = Q // 2
    tab = table.numpy()
    f, r, tv = tab[fixed.numpy()], rel[rel_ids].numpy(), tab[true_row.numpy()]
    true = true_scores(oracle, model, tv, f, r, q_head)
    want = np.zeros((Q, 4), np.int32)
    ref = np.empty((Q, C), np.float32)
    for lo in range(0, Q, 128):
        hi = lo + 128
        e = tab[cand[lo:hi].numpy().reshape(-1)]
        fq, rq = np.repeat(f[lo:hi], C, axis=0), np.repeat(r[lo:hi], C, axis=0)
        s = oracle.score_pairs(model, e, fq, rq) if hi <= q_head else oracle.score_pairs(model, fq, e, rq)
        ref[lo:hi] = s.reshape(hi - lo, C)
    want[:, 0] = (ref > true[:, None]).sum(1)
    want[:, 1] = (ref >= true[:, None]).sum(1)
    want[:, 2:] = want[:, :2]
    assert (want[:, 1] > want[:, 0]).all()
    ptr = np.arange(Q + 1, dtype=np.int64) * C
    got = run(ops, model, table, table, fixed, rel, rel_ids, q_head, ptr, cand.reshape(-1), true_row)
    check(got, (want, ref.reshape(-1)), model)


# ------------------------------------------------------------------------------------------------ rank_candidates
def _model(rel_model, rel_w):
    from blp_amd import models
    m = models.LinkPrediction(rel_w.shape[1], rel_model, "margin", rel_w.shape[0], 0)
    with torch.no_grad():
        m.rel_emb.weight.copy_(torch.from_numpy(rel_w))
    return m


@pytest.mark.parametrize("rel_model", REL_MODELS)
def test_rank_candidates_on_device_equals_its_cpu_route(rel_model, monkeypatch):
    from blp_amd import ranking, utils
    g, f = golden(f"eval_toy_{rel_model}"), golden("filters_toy")
    table, triples, ent2idx = torch.from_numpy(g["ent_emb"]), torch.from_numpy(f["triples"]), torch.from_numpy(f["ent2idx"])
    index = utils.FilterIndex(torch.from_numpy(f["graph_edges"]))
    model = _model(rel_model, g["rel_w"])
    Q = 2 * triples.shape[0]
    rng = np.random.default_rng(50)
    cand = torch.from_numpy(rng.integers(-1, table.shape[0], (Q, 90)))
    ids = torch.from_numpy(rng.integers(-1, len(ent2idx) + 2, (Q, 90)))
    cpu = {}
    for name, c, kw in (("rows", cand, {}), ("ids", ids, dict(candidates_are="ids")), ("neg", cand, dict(include_true=False)),
                        ("tail", cand[Q // 2:], dict(side="tail"))):
        for dtype in (torch.float32, torch.float16):
            cpu[name, dtype] = ranking.rank_candidates(model, table.to(dtype), triples, c, ent2idx, filter_index=index,
                                                       return_scores=True, **kw)

    def no_dense(*a, **k):
        raise AssertionError("the dense route was taken on a device table")

    monkeypatch.setattr(ranking, "_rank_lists_dense", no_dense)
    dev_model = _model(rel_model, g["rel_w"]).cuda()
    for name, c, kw in (("rows", cand, {}), ("ids", ids, dict(candidates_are="ids")), ("neg", cand, dict(include_true=False)),
                        ("tail", cand[Q // 2:], dict(side="tail"))):
        for dtype in (torch.float32, torch.float16):
            counts, scores = ranking.rank_candidates(dev_model, table.to(dtype).cuda(), triples, c.cuda(), ent2idx, filter_index=index,
                                                     return_scores=True, **kw)
            want_counts, want_scores = cpu[name, dtype]
            assert torch.equal(counts.cpu(), want_counts), (name, dtype)
            assert scores.shape == want_scores.shape
            check((None, scores.reshape(-1)), (None, want_scores.reshape(-1).numpy()), (name, dtype))
    # metrics_from_counts applies unchanged
    rr, hits = ranking.metrics_from_counts(counts)
    assert rr.shape == (Q // 2, 2) and hits.shape == (Q // 2, 2, 3)
