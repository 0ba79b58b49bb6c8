"""Filtered top-k inside per-query candidate lists on the MI355X (blp_topk_lists through blp_amd.ops.topk_lists and
ranking.predict_from_candidates).  Everything is compared bit for bit -- rows, NaN positions, the other scores as int32
patterns, empty slots exactly -1 / 0x7fc00000 -- against the brute-force order (entries sorted by row, a stable
argsort(-score), NaN last, removed and skipped entries dropped) read off the C oracle's (Q, N) score matrix: every model and
width, k around list_insert's 64-slot groups, lists around the 64-entry step, slabs, ties, NaN / inf / -0, filters, 16-bit
tables, candidate shards, a table above 2^31 bytes, two threads on two streams, and the Python route."""
import threading

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden
from test_gpu_rank_lists import CASES, oracle_pred, random_lists, random_problem, removed_mask, segment_filter

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7fc00000
KS = (1, 5, 64, 65, 256)  # lists shorter than k among them; 65: the second 64-slot group of list_insert


@pytest.fixture(scope="module")
def ops():
    from blp_amd import ops as _ops
    return _ops


def expected(pred, ptr, rows, k, row_base=0, removed=None):
    """rows (Q, k) int64 global, scores (Q, k) f32 from the oracle's matrix of the LOCAL table (pred[q, local row])."""
    Q, N = pred.shape
    out_rows = np.full((Q, k), -1, np.int64)
    out_scores = np.full((Q, k), np.nan, np.float32)
    for q in range(Q):
        local = rows[ptr[q]:ptr[q + 1]] - row_base
        local = local[(local >= 0) & (local < N)]
        if removed is not None:
            local = local[~removed[q, local]]
        local = np.sort(local, kind="stable")
        s = pred[q, local]
        order = np.argsort(-s, kind="stable")[:k]
        out_rows[q, :len(order)], out_scores[q, :len(order)] = local[order] + row_base, s[order]
    return out_rows, out_scores


def check(got, want, what=""):
    rows, scores = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert rows.dtype == np.int64 and scores.dtype == np.float32 and rows.shape == want[0].shape == scores.shape, what
    assert np.array_equal(rows, want[0]), what
    nan = np.isnan(want[1])
    assert np.array_equal(np.isnan(scores), nan), what
    assert np.array_equal(scores[~nan].view(np.int32), want[1][~nan].view(np.int32)), what
    assert (scores[nan].view(np.int32) == NAN_BITS).all(), what  # empty slots and NaN scores alike: the quiet NaN


def run(ops, model, table, source, fixed, rel, rel_ids, q_head, ptr, rows, k, **kw):
    dev = "cuda"
    t = lambda a: torch.as_tensor(a).to(dev)
    tab = table.to(dev)
    src = tab if source is table else source.to(dev)
    return ops.topk_lists(model, tab, src, t(fixed), rel.to(dev), t(rel_ids), q_head, t(ptr), t(rows), k, **kw)


@pytest.mark.parametrize("model,D", CASES)
def test_rows_and_scores_match_the_oracle(ops, oracle, model, D):
    N, Q = 1000, 12
    table, rel, fixed, rel_ids, _ = random_problem(model, N, D, Q, seed=D)
    ptr, rows = random_lists(Q, N, seed=D + 1)  # lengths 0, 1, 63, 64, 65, 200, 1 500; 30 % duplicates; -1, N - 1, N, N + 7
    f, r = table[fixed].numpy(), rel[rel_ids].numpy()
    for q_head in (0, 5, Q):
        pred = oracle_pred(oracle, model, table.numpy(), f, r, q_head)
        for k in KS:
            want = expected(pred, ptr, rows, k)
            got = run(ops, model, table, table, fixed, rel, rel_ids, q_head, ptr, rows, k)
            check(got, want, (model, D, q_head, k))
            if k == 256 and q_head == 5:
                assert (want[0][0] == -1).all() and (want[0][1, 1:] == -1).all() and want[0][1, 0] >= 0  # lengths 0 and 1
                r_ = want[0]
                twice = (r_[:, 1:] == r_[:, :-1]) & (r_[:, 1:] >= 0)
                assert twice.any(), "a row listed twice comes back twice, in adjacent slots"
                s_ = got[1].cpu().numpy().view(np.int32)
                assert np.array_equal(s_[:, 1:][twice], s_[:, :-1][twice])


@pytest.mark.parametrize("model,D", [("transe", 128), ("transe", 768), ("complex", 128)])
def test_slabs_equal_the_single_slab_call(ops, oracle, model, D):
    """Q = 3 with lists of 5 000, 0 and 70 entries: S = 7 slabs, most of them empty for the short lists, through the key
    buffer and the merge.  The same three lists as the first queries of a Q = 4 096 call (S = 1: the wave decodes its list
    itself) must give the same rows and scores."""
    N = 1000
    table, rel, fixed, rel_ids, _ = random_problem(model, N, D, 3, seed=60)
    ptr, rows = random_lists(3, N, lengths=(5000, 0, 70), seed=61)
    assert ops.topk_lists_workspace_bytes(model, D, 1, 2, len(rows), 10) == (3 * 7 * 10 * 8 + 255) // 256 * 256
    assert ops.topk_lists_workspace_bytes(model, D, 1, 4095, len(rows), 10) == 0
    f, r = table[fixed].numpy(), rel[rel_ids].numpy()
    pred = oracle_pred(oracle, model, table.numpy(), f, r, 1)
    big_q = 4096
    fixed_big = torch.cat((fixed, fixed[:1].expand(big_q - 3)))
    rel_big = torch.cat((rel_ids, rel_ids[:1].expand(big_q - 3)))
    ptr_big = np.concatenate((ptr, np.full(big_q - 3, ptr[-1], np.int64)))
    segs = [rows[ptr[q]:ptr[q + 1]][:40] for q in range(3)]
    rm = removed_mask(segs, None, None, N)
    for k in (10, 65):
        for filt, removed in ((None, None), (segs, rm)):
            kw = {} if filt is None else dict(filter=segment_filter(ops, filt, None, None, 0))
            want = expected(pred, ptr, rows, k, removed=removed)
            few = run(ops, model, table, table, fixed, rel, rel_ids, 1, ptr, rows, k, **kw)
            check(few, want, (model, k, "S = 7"))
            kw = {} if filt is None else dict(filter=segment_filter(ops, filt + [np.zeros(0, np.int64)] * (big_q - 3), None, None, 0))
            many = run(ops, model, table, table, fixed_big, rel, rel_big, 1, ptr_big, rows, k, **kw)
            check((many[0][:3], many[1][:3]), want, (model, k, "S = 1"))
            assert torch.equal(many[0][:3], few[0]) and torch.equal(many[1][:3].view(torch.int32), few[1].view(torch.int32))
            assert bool((many[0][3:] == -1).all()) and bool((many[1][3:].view(torch.int32) == NAN_BITS).all())


@pytest.mark.parametrize("model", REL_MODELS)
def test_ties_nan_inf_and_signed_zero(ops, oracle, model):
    N, D, Q = 1000, 64, 12
    table, rel, fixed, rel_ids, _ = random_problem(model, N, D, Q, seed=6)
    g = torch.Generator().manual_seed(7)
    copies = torch.randperm(N - 100, generator=g)[:200] + 100  # 20 % of the rows are copies of 20 others: ties between rows
    table[copies] = table[copies[:20]].repeat(10, 1)
    table[10] = float("nan")
    table[11, 3] = float("inf")
    table[12, 5] = float("-inf")
    table[13] = 0.0
    table[14] = -0.0
    table[15, ::2] = -0.0
    table[15, 1::2] = 0.0
    table[16, 7] = float("nan")
    fixed[fixed < 30] += 30  # no query is made of a special row
    rel[0] = 0.0
    rel_ids[0], rel_ids[7] = 0, 1
    # TransE scores of exactly zero: head query 0, (e + r) - t with r = 0 and e = t; tail query 7, (h + r) - e with e = h + r
    table[20] = table[fixed[0]]
    table[21] = table[fixed[7]] + rel[1]
    ptr, rows = random_lists(Q, N, lengths=(64, 200, 70), seed=8, specials=False)
    special = np.arange(10, 22)
    rows[ptr[:-1, None] + np.arange(len(special))] = special  # every list meets the special rows
    rows[ptr[2]:ptr[3]] = np.resize([10, 16], ptr[3] - ptr[2])  # a list whose every entry scores NaN
    f, r = table[fixed].numpy(), rel[rel_ids].numpy()
    pred = oracle_pred(oracle, model, table.numpy(), f, r, 5)
    assert np.isnan(pred[2, [10, 16]]).all() and not np.isfinite(pred[:, 11]).any()
    if model == "transe":  # -(+0): the sign of a zero score travels in the key's low bit
        assert pred[0, 20] == 0 and pred[7, 21] == 0 and np.signbit(pred[0, 20]) and np.signbit(pred[7, 21])
    else:
        assert (pred[:, 13:16] == 0).all()
    for k in (5, 64, 200):
        want = expected(pred, ptr, rows, k)
        check(run(ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, k), want, (model, k))
    assert (want[0][2] >= 0).sum() == 70 and np.isnan(want[1][2]).all()  # NaN scores keep their rows, ordered by row
    assert (np.diff(want[0][2][:70]) >= 0).all()
    ties = (want[1][:, 1:] == want[1][:, :-1]) & (want[0][:, 1:] != want[0][:, :-1])
    assert ties.sum() >= 10 and (want[0][:, 1:][ties] > want[0][:, :-1][ties]).all(), "ties between rows: ascending row"


@pytest.mark.parametrize("model", ["transe", "complex"])
def test_filters(ops, oracle, model):
    N, D, Q = 1000, 128, 12
    table, rel, fixed, rel_ids, _ = random_problem(model, N, D, Q, seed=8)
    ptr, rows = random_lists(Q, N, seed=9)
    f, r = table[fixed].numpy(), rel[rel_ids].numpy()
    pred = oracle_pred(oracle, model, table.numpy(), f, r, 5)
    rng = np.random.default_rng(10)
    members = lambda q, n: rng.choice(rows[ptr[q]:ptr[q + 1]], n) if ptr[q + 1] > ptr[q] else np.zeros(0, np.int64)
    call = lambda k, filt: run(ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, k, filter=filt)

    # (a) segments of rows that remove list members (duplicated ones and out-of-range values among them); exclude exempts one
    best = expected(pred, ptr, rows, 3)[0]
    segs = [np.concatenate((members(q, 9), best[q][best[q] >= 0], rng.integers(0, N, 5), [-1, N + 3])) for q in range(Q)]
    exclude = np.array([segs[q][0] for q in range(Q)], np.int64)
    for k in (5, 65):
        want = expected(pred, ptr, rows, k, removed=removed_mask(segs, exclude, None, N))
        plain = expected(pred, ptr, rows, k)
        assert not np.array_equal(want[0], plain[0]), "the filter must bite"
        check(call(k, segment_filter(ops, segs, exclude, None, 0)), want, ("rows", k))
        check(call(k, segment_filter(ops, segs, None, None, 0)), expected(pred, ptr, rows, k, removed=removed_mask(segs, None, None, N)),
              ("rows, nothing exempt", k))
    dup_removed = [q for q in range(Q) if any((rows[ptr[q]:ptr[q + 1]] == v).sum() > 1 for v in segs[q][1:])]
    assert dup_removed, "a filter entry removes every copy of its row"

    # (b) entity ids through an ent2idx with -1 entries
    ent2idx = rng.permutation(N + 200).astype(np.int64)
    ent2idx[ent2idx >= N] = -1
    row2id = np.full(N, -1, np.int64)
    row2id[ent2idx[ent2idx >= 0]] = np.nonzero(ent2idx >= 0)[0]
    id_segs = [np.concatenate((row2id[np.clip(members(q, 9), 0, N - 1)], rng.integers(0, N + 200, 6), [N + 500, -2])) for q in range(Q)]
    id_ex = np.array([s[0] for s in id_segs], np.int64)
    want = expected(pred, ptr, rows, 10, removed=removed_mask(id_segs, id_ex, ent2idx, N))
    check(call(10, segment_filter(ops, id_segs, id_ex, ent2idx, 0)), want, "ids")

    # (c) a query left with 3 rows at k = 5; a query whose whole list goes; a 5 000-entry segment; a filter with nothing in the list
    big = [np.zeros(0, np.int64) for _ in range(Q)]
    mine, times = np.unique(rows[ptr[5]:ptr[6]], return_counts=True)
    once = mine[(mine >= 0) & (mine < N) & (times == 1)][:3]
    big[5] = np.setdiff1d(mine, once)
    big[4] = np.arange(N)
    big[6] = rng.integers(0, N, 5000)
    big[3] = np.setdiff1d(np.arange(N), rows[ptr[3]:ptr[4]])[:300]
    want = expected(pred, ptr, rows, 5, removed=removed_mask(big, None, None, N))
    assert (want[0][5] >= 0).sum() == 3 and set(want[0][5][:3]) == set(once) and (want[0][4] == -1).all()
    assert np.array_equal(want[0][3], expected(pred, ptr, rows, 5)[0][3])
    check(call(5, segment_filter(ops, big, None, None, 0)), want, "few left")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("model,D", [("transe", 128), ("transe", 300), ("distmult", 64), ("complex", 128), ("simple", 256)])
def test_16_bit_table_equals_the_widened_table(ops, oracle, model, D, dtype):
    N, Q = 1000, 12
    table, rel, fixed, rel_ids, _ = random_problem(model, N, D, Q, seed=11)
    store = torch.zeros((N, D + 8), dtype=dtype)  # row stride D + 8
    store[:, :D] = table.to(dtype)
    t16 = store[:, :D]
    wide = t16.float()
    ptr, rows = random_lists(Q, N, seed=12)
    src = wide[fixed]
    segs = [rows[ptr[q]:ptr[q + 1]][:7] for q in range(Q)]
    f, r = wide[fixed].numpy(), rel[rel_ids].numpy()
    pred = oracle_pred(oracle, model, wide.numpy(), f, r, 5)
    dev16 = store.cuda()[:, :D]
    assert dev16.stride(0) == D + 8
    t = lambda a: torch.as_tensor(a).cuda()
    for k in (5, 65):
        filt = segment_filter(ops, segs, None, None, 0)
        got16 = ops.topk_lists(model, dev16, src.cuda(), t(np.arange(Q)), rel.cuda(), t(rel_ids), 5, t(ptr), t(rows), k, filter=filt)
        got32 = run(ops, model, wide, src, np.arange(Q), rel, rel_ids, 5, ptr, rows, k, filter=filt)
        assert torch.equal(got16[0], got32[0]) and torch.equal(got16[1].view(torch.int32), got32[1].view(torch.int32))
        check(got16, expected(pred, ptr, rows, k, removed=removed_mask(segs, None, None, N)), (model, D, dtype, k))
    with pytest.raises(TypeError):
        ops.topk_lists(model, dev16, dev16, t(fixed), rel.cuda(), t(rel_ids), 5, t(ptr), t(rows), 5)


@pytest.mark.parametrize("model", ["transe", "simple"])
def test_two_candidate_shards_merge_to_the_unsharded_call(ops, oracle, model):
    N, D, Q = 1000, 128, 12
    table, rel, fixed, rel_ids, _ = random_problem(model, N, D, Q, seed=13)
    ptr, rows = random_lists(Q, N, seed=14)  # uniform rows: the split at row 517 falls inside every 64-entry step
    f, r = table[fixed].numpy(), rel[rel_ids].numpy()
    pred = oracle_pred(oracle, model, table.numpy(), f, r, 5)
    segs = [rows[ptr[q]:ptr[q + 1]][:9] for q in range(Q)]
    for k in (5, 65):
        whole = expected(pred, ptr, rows, k, removed=removed_mask(segs, None, None, N))
        check(run(ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, k, filter=segment_filter(ops, segs, None, None, 0)), whole)
        parts = []
        for lo, hi in ((0, 517), (517, N)):
            got = run(ops, model, table[lo:hi], table, fixed, rel, rel_ids, 5, ptr, rows, k, row_base=lo,
                      filter=segment_filter(ops, segs, None, None, lo))
            check(got, expected(pred[:, lo:hi], ptr, rows, k, row_base=lo, removed=removed_mask(segs, None, None, hi - lo, lo)), (lo, hi, k))
            parts.append(got)
        merged = ops.topk_merge(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), k)
        check(merged, whole, ("merged", k))


@pytest.mark.parametrize("model", ["transe", "distmult"])
def test_table_above_two_gib(ops, oracle, model):
    """2 100 000 x 256 f32 = 2.15 GB, filled on the device; short lists drawn from both ends of the table.  Expected: the
    oracle's scores of the gathered (query, entry) pairs."""
    N, D, Q, C, k = 2_100_000, 256, 8, 48, 10
    g = torch.Generator(device="cuda").manual_seed(70)
    table = torch.rand((N, D), generator=g, device="cuda") - 0.5
    assert table.numel() * 4 > 2 ** 31
    rng = np.random.default_rng(71)
    cand = np.concatenate((rng.integers(0, 200, (Q, C // 2)), rng.integers(N - 200, N, (Q, C // 2))), 1).astype(np.int64)
    cand[:, 0], cand[:, 1] = 0, N - 1
    fixed = torch.from_numpy(rng.integers(N - 1000, N, Q))
    rel = (torch.rand(5, D) - 0.5) * 0.25
    rel_ids = torch.from_numpy(rng.integers(0, 5, Q))
    q_head = Q // 2
    e = table[torch.from_numpy(cand.reshape(-1)).cuda()].cpu().numpy()
    fq = np.repeat(table[fixed.cuda()].cpu().numpy(), C, axis=0)
    rq = np.repeat(rel[rel_ids].numpy(), C, axis=0)
    h = q_head * C
    s = np.concatenate((oracle.score_pairs(model, e[:h], fq[:h], rq[:h]), oracle.score_pairs(model, fq[h:], e[h:], rq[h:]))).reshape(Q, C)
    want_rows, want_scores = np.empty((Q, k), np.int64), np.empty((Q, k), np.float32)
    for q in range(Q):
        by_row = np.argsort(cand[q], kind="stable")
        order = by_row[np.argsort(-s[q][by_row], kind="stable")[:k]]
        want_rows[q], want_scores[q] = cand[q][order], s[q][order]
    ptr = torch.arange(Q + 1) * C
    got = ops.topk_lists(model, table, table, fixed.cuda(), rel.cuda(), rel_ids.cuda(), q_head, ptr.cuda(),
                         torch.from_numpy(cand.reshape(-1)).cuda(), k)
    check(got, (want_rows, want_scores), model)
    assert (want_rows < 200).any() and (want_rows >= N - 200).any()


def test_two_threads_on_two_streams(ops):
    N, D, Q = 1000, 128, 12
    problems = []
    for i, model in enumerate(("transe", "complex")):
        table, rel, fixed, rel_ids, _ = random_problem(model, N, D, 3 if i else Q, seed=20 + i)
        ptr, rows = random_lists(3, N, lengths=(5000, 0, 70), seed=30) if i else random_lists(Q, N, seed=31)  # S = 7 and S = 1
        dev = [x.cuda() for x in (table, rel, fixed, rel_ids, torch.from_numpy(ptr), torch.from_numpy(rows))]
        single = ops.topk_lists(model, dev[0], dev[0], dev[2], dev[1], dev[3], 1, dev[4], dev[5], 10)
        problems.append((model, dev, single))
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def worker(i):
        try:
            model, dev, _ = problems[i]
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for _ in range(5):
                    out = ops.topk_lists(model, dev[0], dev[0], dev[2], dev[1], dev[3], 1, dev[4], dev[5], 10)
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


# ------------------------------------------------------------------------------------------------ predict_from_candidates
def _model(rel_model, rel_w):
    from blp_amd import models
    m = models.LinkPrediction(rel_w.shape[1], rel_model, "margin", rel_w.shape[0], 0)
    with torch.no_grad():
        m.rel_emb.weight.copy_(torch.from_numpy(rel_w))
    return m


def _same(got, want, what=""):
    check(got, (want[0].numpy(), want[1].numpy()), what)


@pytest.mark.parametrize("rel_model", REL_MODELS)
def test_predict_from_candidates_on_device_equals_its_cpu_route(rel_model, monkeypatch):
    from blp_amd import ranking, utils
    g, f = golden(f"eval_toy_{rel_model}"), golden("filters_toy")
    table, triples, ent2idx = torch.from_numpy(g["ent_emb"]), torch.from_numpy(f["triples"]), torch.from_numpy(f["ent2idx"])
    index = utils.FilterIndex(torch.from_numpy(f["graph_edges"]))
    model = _model(rel_model, g["rel_w"])
    Q = 2 * triples.shape[0]
    rng = np.random.default_rng(50)
    cand = torch.from_numpy(rng.integers(-1, table.shape[0], (Q, 90)))
    ids = torch.from_numpy(rng.integers(-1, len(ent2idx) + 2, (Q, 90)))
    lens = rng.integers(0, 90, Q)
    csr = (torch.from_numpy(np.concatenate(([0], np.cumsum(lens)))), torch.cat([cand[q, :n] for q, n in enumerate(lens)]))
    entities = torch.arange(table.shape[0]) * 3 + 1
    cases = (("rows", cand, {}), ("ids", ids, dict(candidates_are="ids")), ("csr", csr, {}), ("unique", cand, dict(unique=True)),
             ("tail", cand[Q // 2:], dict(side="tail")), ("entities", cand, dict(entities=entities)))
    dense = ranking._topk_lists_dense
    cpu = {}
    for name, c, kw in cases:
        for dtype in (torch.float32, torch.float16):
            for k in (3, 100):
                cpu[name, dtype, k] = ranking.predict_from_candidates(model, table.to(dtype), triples, k, c, ent2idx, filter_index=index, **kw)

    def no_dense(*a, **kw):
        raise AssertionError("the dense route was taken on a device table")

    monkeypatch.setattr(ranking, "_topk_lists_dense", no_dense)
    dev_model = _model(rel_model, g["rel_w"]).cuda()
    on_dev = lambda c: tuple(x.cuda() for x in c) if isinstance(c, tuple) else c.cuda()
    for name, c, kw in cases:
        for dtype in (torch.float32, torch.float16):
            for k in (3, 100):
                got = ranking.predict_from_candidates(dev_model, table.to(dtype).cuda(), triples, k, on_dev(c), ent2idx,
                                                      filter_index=index, **kw)
                _same(got, cpu[name, dtype, k], (name, dtype, k))

    # k = 300 and DistMult at D = 96 are not the kernel's: they must reach the dense route (here on the device's tensors)
    taken = []

    def recording(*a, **kw):
        taken.append(a[5])
        return dense(*a, **kw)

    monkeypatch.setattr(ranking, "_topk_lists_dense", recording)
    got = ranking.predict_from_candidates(dev_model, table.cuda(), triples, 300, cand.cuda(), ent2idx, filter_index=index)
    assert taken == [300] and got[0].shape == (Q, 300)
    want = ranking.predict_from_candidates(model, table, triples, 300, cand, ent2idx, filter_index=index)
    assert torch.equal(got[0].cpu() < 0, want[0] < 0) and torch.equal(torch.isnan(got[1].cpu()), torch.isnan(want[1]))
    if rel_model == "distmult":
        gen = torch.Generator().manual_seed(3)
        t96, rel96 = torch.randn(table.shape[0], 96, generator=gen) * 0.1, torch.randn(g["rel_w"].shape[0], 96, generator=gen) * 0.1
        m96 = _model("distmult", rel96.numpy())
        taken.clear()
        got = ranking.predict_from_candidates(_model("distmult", rel96.numpy()).cuda(), t96.cuda(), triples, 5, cand.cuda(), ent2idx)
        assert taken == [5]
        want = ranking.predict_from_candidates(m96, t96, triples, 5, cand, ent2idx)
        assert got[0].shape == want[0].shape and torch.equal(torch.isnan(got[1].cpu()), torch.isnan(want[1]))
