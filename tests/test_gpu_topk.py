"""Filtered top-k prediction on the MI355X (blp_topk / blp_topk_merge through blp_amd.ops and ranking.predict_links):
rows exact and scores bit-identical to the reference's scores in numpy's stable order -- the score goldens, random
problems against the C oracle, adversarial tables (duplicates, NaN / inf / -0), filters, candidate shards, a
Wikidata5M-sized table and two threads on two streams."""
import threading

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden, golden_names

pytestmark = pytest.mark.gpu

SIDE_HEAD, SIDE_TAIL = 0, 1


@pytest.fixture(scope="module")
def ops():
    from blp_amd import ops as _ops
    return _ops


def expected(pred, k, removed=None):
    """np.argsort(-pred, kind="stable") per query, removed entries dropped, -1 / NaN beyond what is left."""
    Q, N = pred.shape
    order = np.argsort(-pred, axis=1, kind="stable")
    rows = np.full((Q, k), -1, np.int64)
    scores = np.full((Q, k), np.nan, np.float32)
    for q in range(Q):
        o = order[q] if removed is None else order[q][~removed[q, order[q]]]
        o = o[:k]
        rows[q, :len(o)] = o
        scores[q, :len(o)] = pred[q, o]
    return rows, scores


def check(got, want, what=""):
    rows, scores = got[0].cpu().numpy(), got[1].cpu().numpy()
    want_rows, want_scores = want
    assert np.array_equal(rows, want_rows), what
    nan = np.isnan(want_scores)
    assert np.array_equal(np.isnan(scores), nan), what
    assert np.array_equal(scores[~nan].view(np.int32), want_scores[~nan].view(np.int32)), what


def oracle_pred(oracle, model, table, source, fixed_row, rel_emb, rel_ids, q_head):
    f, r = source[fixed_row], rel_emb[rel_ids]
    parts = []
    if q_head:
        parts.append(oracle.score_all(model, SIDE_HEAD, table, f[:q_head], r[:q_head]))
    if q_head < len(fixed_row):
        parts.append(oracle.score_all(model, SIDE_TAIL, table, f[q_head:], r[q_head:]))
    return np.concatenate(parts)


def random_problem(model, N, D, Q, R=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(N, D, generator=g)
    table = torch.nn.functional.normalize(table, dim=-1) if model == "transe" else table * 0.1
    rel = (torch.rand(R, D, generator=g) - 0.5) * 0.25
    return table, rel, torch.randint(0, N, (Q,), generator=g), torch.randint(0, R, (Q,), generator=g)


def segment_filter(ops, lists, exclude, ent2idx, row_base, dev):
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


# ------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", golden_names("scores_"))
def test_topk_matches_reference_score_goldens(ops, name):
    g = golden(name)
    model = name.split("_")[1]
    table = torch.from_numpy(g["table"]).cuda()
    rel = torch.from_numpy(g["rel_w"]).cuda()
    heads, tails, rels = (torch.from_numpy(g[x].reshape(-1)).cuda() for x in ("heads", "tails", "rels"))
    T = heads.shape[0]
    pred = np.concatenate((g["head_pred"], g["tail_pred"]))
    for k in (1, 5, 64, 192, 256):
        got = ops.topk(model, table, table, torch.cat((tails, heads)), rel, torch.cat((rels, rels)), T, k)
        check(got, expected(pred, k), (name, k))
        head_only = ops.topk(model, table, table, tails, rel, rels, T, k)
        tail_only = ops.topk(model, table, table, heads, rel, rels, 0, k)
        check(head_only, expected(g["head_pred"], k), (name, "head", k))
        check(tail_only, expected(g["tail_pred"], k), (name, "tail", k))


def test_topk_scratch_free_kernels_are_built():
    """The new kernels are in the object directory the scratch-memory test of test_abi.py reads."""
    import os
    import sys
    from blp_amd import build
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources
    kernels = kernel_resources.kernels_of(build.OBJ)
    names = [k for k in kernels if "topk" in k]
    assert len(names) >= 2 * 12 + 2
    assert all(kernels[k]["private_segment_fixed_size"] == 0 for k in names)


# ------------------------------------------------------------------------------------------------ random problems
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("model", REL_MODELS)
def test_topk_random_problems_against_oracle(ops, oracle, model, D):
    cases = [(300_001, 2, 2, (1, 10, 100, 256)),  # a few queries over a long table (the HBM-bound grid)
             (5_003, 150, 150, (10, 256)),         # N not a multiple of 64
             (5_003, 0, 97, (10,)),                # q_head = 0
             (1_000, 64, 0, (1, 100))]             # q_head = Q
    if D == 128:
        cases.append((14_541, 1024, 1024, (10,)))  # many queries (the VALU-bound grid)
    for i, (N, qh, qt, ks) in enumerate(cases):
        table, rel, fixed_row, rel_ids = random_problem(model, N, D, qh + qt, seed=100 + 7 * i + D)
        pred = oracle_pred(oracle, model, table.numpy(), table.numpy(), fixed_row.numpy(), rel.numpy(), rel_ids.numpy(), qh)
        dev = [x.cuda() for x in (table, rel, fixed_row, rel_ids)]
        for k in ks:
            got = ops.topk(model, dev[0], dev[0], dev[2], dev[1], dev[3], qh, k)
            check(got, expected(pred, k), (model, D, N, qh, qt, k))


# ------------------------------------------------------------------------------------------------ adversarial
@pytest.mark.parametrize("model", REL_MODELS)
def test_topk_duplicates_straddle_workgroups(ops, oracle, model):
    """5 % of the table exact copies of a few rows: equal scores everywhere, across slabs and workgroups, many more than k."""
    N, D, qh, qt = 40_000, 128, 40, 40
    table, rel, fixed_row, rel_ids = random_problem(model, N, D, qh + qt, seed=3)
    g = torch.Generator().manual_seed(4)
    dup = torch.randperm(N, generator=g)[: N // 20]
    table[dup] = table[dup % 5]
    fixed_row[:8] = dup[:8]
    pred = oracle_pred(oracle, model, table.numpy(), table.numpy(), fixed_row.numpy(), rel.numpy(), rel_ids.numpy(), qh)
    dev = [x.cuda() for x in (table, rel, fixed_row, rel_ids)]
    for k in (10, 256):
        check(ops.topk(model, dev[0], dev[0], dev[2], dev[1], dev[3], qh, k), expected(pred, k), (model, k))


@pytest.mark.parametrize("model", REL_MODELS)
def test_topk_nan_inf_and_signed_zero(ops, oracle, model):
    N, D, qh, qt = 3_000, 64, 6, 6
    table, rel, fixed_row, rel_ids = random_problem(model, N, D, qh + qt, seed=5)
    table[5, 3] = float("nan")
    table[7, 0] = float("inf")
    table[9, 1] = float("-inf")
    table[11:40] = -0.0
    table[40:60, ::2] = -0.0
    table[60:80] = table[fixed_row[0]]  # TransE with a zero relation: scores of -0.0
    rel[0] = 0.0
    rel_ids[0] = rel_ids[qh] = 0
    fixed_row[1] = 11
    pred = oracle_pred(oracle, model, table.numpy(), table.numpy(), fixed_row.numpy(), rel.numpy(), rel_ids.numpy(), qh)
    assert np.isnan(pred).any()
    dev = [x.cuda() for x in (table, rel, fixed_row, rel_ids)]
    for k in (1, 10, 100, 256):
        check(ops.topk(model, dev[0], dev[0], dev[2], dev[1], dev[3], qh, k), expected(pred, k), (model, k))


@pytest.mark.parametrize("model", ["transe", "distmult"])
def test_topk_filters(ops, oracle, model):
    """Filters with blp_rank_all's semantics: entity ids through ent2idx (-1 entries), exclude never filtered, rows removed;
    one query keeps 3 of 50 rows (padding), one has a 5 000-entry segment."""
    D = 128
    for N, qh, qt in ((50, 2, 2), (20_000, 3, 3)):
        table, rel, fixed_row, rel_ids = random_problem(model, N, D, qh + qt, seed=N)
        rng = np.random.default_rng(N)
        n_ids = N + 40
        ent2idx = np.full(n_ids, -1, np.int64)  # entity id -> row; 40 ids have no row
        ids = rng.permutation(n_ids)[:N]
        ent2idx[ids] = np.arange(N)
        row2id = np.empty(N, np.int64)
        row2id[ent2idx[ids]] = ids
        lists, exclude = [], []
        for q in range(qh + qt):
            if N == 50 and q == 0:
                seg = row2id[3:]                           # leaves rows 0, 1, 2
            elif N == 20_000 and q == 1:
                seg = rng.choice(n_ids, 5_000, replace=False)
            else:
                seg = rng.choice(n_ids, min(N // 3, 40), replace=False)
            lists.append(seg)
            exclude.append(int(seg[len(seg) // 2]) if q % 2 else int(row2id[0 if N == 50 else fixed_row[q]]))
        pred = oracle_pred(oracle, model, table.numpy(), table.numpy(), fixed_row.numpy(), rel.numpy(), rel_ids.numpy(), qh)
        removed = removed_mask(lists, exclude, ent2idx, N)
        dev = [x.cuda() for x in (table, rel, fixed_row, rel_ids)]
        filt = segment_filter(ops, lists, exclude, ent2idx, 0, dev[0].device)
        for k in (1, 10, 256):
            got = ops.topk(model, dev[0], dev[0], dev[2], dev[1], dev[3], qh, k, filter=filt)
            want = expected(pred, k, removed)
            check(got, want, (model, N, k))
        if N == 50:  # k = 256: three rows, then padding
            assert (got[0][0, :3] >= 0).all() and (got[0][0, 3:] == -1).all()


@pytest.mark.parametrize("model", ["transe", "complex"])
def test_topk_shards_merge_to_unsharded(ops, model):
    """The table in three candidate shards (row_base), each ranked with the global filter, lists merged by blp_topk_merge."""
    N, D, qh, qt = 30_011, 128, 5, 7
    table, rel, fixed_row, rel_ids = random_problem(model, N, D, qh + qt, seed=9)
    table[1000:2500] = table[7]  # ties across the shard boundaries
    rng = np.random.default_rng(9)
    lists = [rng.choice(N, 30, replace=False) for _ in range(qh + qt)]
    exclude = [int(x[0]) for x in lists]
    table, rel, fixed_row, rel_ids = (x.cuda() for x in (table, rel, fixed_row, rel_ids))
    for k in (10, 256):
        whole = ops.topk(model, table, table, fixed_row, rel, rel_ids, qh, k,
                         filter=segment_filter(ops, lists, exclude, None, 0, table.device))
        parts = []
        for lo, hi in ((0, 9_000), (9_000, 21_000), (21_000, N)):
            f = segment_filter(ops, lists, exclude, None, lo, table.device)
            parts.append(ops.topk(model, table[lo:hi], table, fixed_row, rel, rel_ids, qh, k, filter=f, row_base=lo))
        rows, scores = ops.topk_merge(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), k)
        assert torch.equal(rows, whole[0])
        assert torch.equal(scores.view(torch.int32), whole[1].view(torch.int32))


def test_topk_full_size_table(ops, oracle):
    """Wikidata5M's size: 4.6 M x 128, 4 queries (2 + 2), k = 10, filtered."""
    model, N, D, qh, qt = "transe", 4_600_000, 128, 2, 2
    g = torch.Generator(device="cuda").manual_seed(11)
    table = torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=g), dim=-1)
    rel = (torch.rand(5, D, device="cuda", generator=g) - 0.5) * 0.25
    fixed_row = torch.tensor([5, 4_599_999, 123_456, 2_000_000], device="cuda")
    rel_ids = torch.tensor([0, 1, 2, 3], device="cuda")
    host = table.cpu().numpy()
    pred = oracle_pred(oracle, model, host, host, fixed_row.cpu().numpy(), rel.cpu().numpy(), rel_ids.cpu().numpy(), qh)
    top = np.argsort(-pred, axis=1, kind="stable")[:, :6]
    lists = [np.concatenate((top[q, ::2], [7, 4_599_990])) for q in range(4)]  # three of the best six filtered
    exclude = [int(top[q, 2]) for q in range(4)]                                # ... but one of them excluded
    filt = segment_filter(ops, lists, exclude, None, 0, table.device)
    got = ops.topk(model, table, table, fixed_row, rel, rel_ids, qh, 10, filter=filt)
    check(got, expected(pred, 10, removed_mask(lists, exclude, None, N)))


def test_topk_two_threads_two_streams(ops):
    problems = []
    for i, model in enumerate(("transe", "distmult")):
        table, rel, fixed_row, rel_ids = random_problem(model, 50_000 + 13 * i, 128, 96, seed=20 + i)
        problems.append((model, [x.cuda() for x in (table, rel, fixed_row, rel_ids)]))
    serial = [ops.topk(m, d[0], d[0], d[2], d[1], d[3], 48, 20) for m, d in problems]
    torch.cuda.synchronize()
    failures, start = [], threading.Barrier(2)

    def worker(i):
        try:
            m, d = problems[i]
            stream = torch.cuda.Stream()
            start.wait()
            with torch.cuda.stream(stream):
                for _ in range(6):
                    rows, scores = ops.topk(m, d[0], d[0], d[2], d[1], d[3], 48, 20)
                    stream.synchronize()
                    if not (torch.equal(rows, serial[i][0]) and torch.equal(scores.view(torch.int32), serial[i][1].view(torch.int32))):
                        failures.append(i)
        except Exception as exc:  # noqa: BLE001
            failures.append(repr(exc))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures


def test_predict_links_gpu_equals_cpu_route():
    """ranking.predict_links on the device (blp_topk) == its CPU route (score_fn + stable sort), filtered, ids returned."""
    from blp_amd import models, ranking, utils
    f = golden("filters_toy")
    for model_name in REL_MODELS:
        g = golden(f"eval_toy_{model_name}")
        model = models.LinkPrediction(128, model_name, "margin", g["rel_w"].shape[0], 0)
        with torch.no_grad():
            model.rel_emb.weight.copy_(torch.from_numpy(g["rel_w"]))
        index = utils.FilterIndex(torch.from_numpy(f["graph_edges"]))
        args = (torch.from_numpy(f["triples"]), 10, torch.from_numpy(f["ent2idx"]))
        kw = dict(filter_index=index, entities=torch.from_numpy(f["entities"]))
        cpu = ranking.predict_links(model, torch.from_numpy(g["ent_emb"]), *args, **kw)
        gpu = ranking.predict_links(model.cuda(), torch.from_numpy(g["ent_emb"]).cuda(), *args, **kw)
        assert torch.equal(gpu[0].cpu(), cpu[0])
        assert torch.equal(gpu[1].cpu().view(torch.int32), cpu[1].view(torch.int32))
