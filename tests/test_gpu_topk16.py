"""Filtered top-k prediction over a 16-bit candidate table on the MI355X (blp_topk_typed through ops.topk and
ranking.predict_links): the result must be blp_topk's contract on the table WIDENED to float32 -- rows in numpy's stable order
of the C oracle's scores of the widened table, scores bit for bit.  Score goldens rounded to float16 / bfloat16, random
problems in both regimes, adversarial tables (ties from rounding, duplicates, NaN / inf / -0, subnormals), filters, candidate
shards, a Wikidata5M-sized float16 table, two streams, and predict_links against its CPU route."""
import threading

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden, golden_names
from test_gpu_topk import check, expected, oracle_pred, random_problem, removed_mask, segment_filter

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def ops():
    from blp_amd import ops as _ops
    return _ops


def rounded(table, dtype):
    """(16-bit copy on the device, the same values widened to float32 on the host)"""
    t16 = table.to(dtype)
    return t16.cuda(), t16.float().contiguous()


def oracle_of(oracle, model, wide, fixed_row, rel, rel_ids, qh):
    w = wide.numpy()
    return oracle_pred(oracle, model, w, w, fixed_row.numpy(), rel.numpy(), rel_ids.numpy(), qh)


def run16(ops, model, t16, wide, fixed_row, rel, rel_ids, qh, k, **kw):
    return ops.topk(model, t16, wide.cuda(), fixed_row.cuda(), rel.cuda(), rel_ids.cuda(), qh, k, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", golden_names("scores_"))
def test_topk16_score_goldens(ops, oracle, name, dtype):
    g = golden(name)
    model = name.split("_")[1]
    t16, wide = rounded(torch.from_numpy(g["table"]), dtype)
    rel = torch.from_numpy(g["rel_w"])
    heads, tails, rels = (torch.from_numpy(g[x].reshape(-1)) for x in ("heads", "tails", "rels"))
    T = heads.shape[0]
    fixed, rel_ids = torch.cat((tails, heads)), torch.cat((rels, rels))
    pred = oracle_of(oracle, model, wide, fixed, rel, rel_ids, T)
    for k in (1, 5, 64, 256):
        check(run16(ops, model, t16, wide, fixed, rel, rel_ids, T, k), expected(pred, k), (name, dtype, k))
        check(run16(ops, model, t16, wide, tails, rel, rels, T, k), expected(pred[:T], k), (name, dtype, "head", k))
        check(run16(ops, model, t16, wide, heads, rel, rels, 0, k), expected(pred[T:], k), (name, dtype, "tail", k))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("model", REL_MODELS)
def test_topk16_random_problems_against_oracle(ops, oracle, model, D, dtype):
    cases = [(300_001, 2, 2, (1, 10, 256)),   # 4 queries over a long table (the HBM-bound grid)
             (14_541, 1024, 1024, (10,)),     # 2 048 queries (the VALU-bound grid)
             (5_003, 0, 97, (10,)),           # q_head = 0
             (1_000, 64, 0, (1, 100))]        # q_head = Q
    for i, (N, qh, qt, ks) in enumerate(cases):
        table, rel, fixed_row, rel_ids = random_problem(model, N, D, qh + qt, seed=300 + 7 * i + D)
        t16, wide = rounded(table, dtype)
        pred = oracle_of(oracle, model, wide, fixed_row, rel, rel_ids, qh)
        for k in ks:
            check(run16(ops, model, t16, wide, fixed_row, rel, rel_ids, qh, k), expected(pred, k), (model, D, dtype, N, qh, qt, k))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", REL_MODELS)
def test_topk16_ties_duplicates_nonfinite_subnormals(ops, oracle, model, dtype):
    """5 % duplicate rows straddling workgroups, +-inf / NaN / -0 entries, rows of 16-bit subnormals (widened exactly)."""
    N, D, qh, qt = 40_000, 128, 40, 40
    table, rel, fixed_row, rel_ids = random_problem(model, N, D, qh + qt, seed=31)
    g = torch.Generator().manual_seed(32)
    dup = torch.randperm(N, generator=g)[: N // 20]
    table[dup] = table[dup % 5]
    fixed_row[:8] = dup[:8]
    table[5, 3] = float("nan")
    table[7, 0] = float("inf")
    table[9, 1] = float("-inf")
    table[11:40] = -0.0
    table[40:60, ::2] = -0.0
    tiny = torch.finfo(dtype).tiny  # the smallest normal: below it the 16-bit values are subnormal
    table[100:300] = (torch.rand(200, D, generator=g) - 0.5) * tiny
    table[300:310] = tiny / 8
    rel[0] = 0.0
    rel_ids[0] = rel_ids[qh] = 0
    fixed_row[1], fixed_row[2] = 11, 150
    t16, wide = rounded(table, dtype)
    sub = wide[100:300]
    assert ((sub != 0) & (sub.abs() < tiny)).any()  # real subnormals survived the rounding
    pred = oracle_of(oracle, model, wide, fixed_row, rel, rel_ids, qh)
    assert np.isnan(pred).any()
    for k in (1, 10, 100, 256):
        check(run16(ops, model, t16, wide, fixed_row, rel, rel_ids, qh, k), expected(pred, k), (model, dtype, k))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["transe", "distmult"])
def test_topk16_filters(ops, oracle, model, dtype):
    """blp_rank_all's filter semantics; one query keeps 3 of 50 rows (padding), one has a 5 000-entry segment."""
    D = 128
    for N, qh, qt in ((50, 2, 2), (20_000, 3, 3)):
        table, rel, fixed_row, rel_ids = random_problem(model, N, D, qh + qt, seed=N + 1)
        t16, wide = rounded(table, dtype)
        rng = np.random.default_rng(N)
        n_ids = N + 40
        ent2idx = np.full(n_ids, -1, np.int64)
        ids = rng.permutation(n_ids)[:N]
        ent2idx[ids] = np.arange(N)
        row2id = np.empty(N, np.int64)
        row2id[ent2idx[ids]] = ids
        lists, exclude = [], []
        for q in range(qh + qt):
            if N == 50 and q == 0:
                seg = row2id[3:]
            elif N == 20_000 and q == 1:
                seg = rng.choice(n_ids, 5_000, replace=False)
            else:
                seg = rng.choice(n_ids, min(N // 3, 40), replace=False)
            lists.append(seg)
            exclude.append(int(seg[len(seg) // 2]) if q % 2 else int(row2id[0 if N == 50 else fixed_row[q]]))
        pred = oracle_of(oracle, model, wide, fixed_row, rel, rel_ids, qh)
        removed = removed_mask(lists, exclude, ent2idx, N)
        filt = segment_filter(ops, lists, exclude, ent2idx, 0, t16.device)
        for k in (1, 10, 256):
            got = run16(ops, model, t16, wide, fixed_row, rel, rel_ids, qh, k, filter=filt)
            check(got, expected(pred, k, removed), (model, dtype, N, k))
        if N == 50:
            assert (got[0][0, :3] >= 0).all() and (got[0][0, 3:] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_topk16_shards_merge_to_unsharded(ops, dtype):
    model, N, D, qh, qt = "complex", 30_011, 128, 5, 7
    table, rel, fixed_row, rel_ids = random_problem(model, N, D, qh + qt, seed=39)
    table[1000:2500] = table[7]
    t16, wide = rounded(table, dtype)
    rng = np.random.default_rng(39)
    lists = [rng.choice(N, 30, replace=False) for _ in range(qh + qt)]
    exclude = [int(x[0]) for x in lists]
    src, rel, fixed_row, rel_ids = (x.cuda() for x in (wide, rel, fixed_row, rel_ids))
    for k in (10, 256):
        whole = ops.topk(model, t16, src, fixed_row, rel, rel_ids, qh, k, filter=segment_filter(ops, lists, exclude, None, 0, src.device))
        parts = []
        for lo, hi in ((0, 14_000), (14_000, N)):
            f = segment_filter(ops, lists, exclude, None, lo, src.device)
            parts.append(ops.topk(model, t16[lo:hi], src, fixed_row, rel, rel_ids, qh, k, filter=f, row_base=lo))
        rows, scores = ops.topk_merge(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), k)
        assert torch.equal(rows, whole[0])
        assert torch.equal(scores.view(torch.int32), whole[1].view(torch.int32))


def test_topk16_full_size_float16_table(ops, oracle):
    """Wikidata5M's size: 4.6 M x 128 float16, 4 queries (2 + 2), k = 10, filtered."""
    model, N, D, qh = "transe", 4_600_000, 128, 2
    g = torch.Generator(device="cuda").manual_seed(41)
    t16 = torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=g), dim=-1).half()
    rel = (torch.rand(5, D, device="cuda", generator=g) - 0.5) * 0.25
    fixed_row = torch.tensor([5, 4_599_999, 123_456, 2_000_000], device="cuda")
    rel_ids = torch.tensor([0, 1, 2, 3], device="cuda")
    host = t16.float().cpu().numpy()
    pred = oracle_pred(oracle, model, host, host, fixed_row.cpu().numpy(), rel.cpu().numpy(), rel_ids.cpu().numpy(), qh)
    top = np.argsort(-pred, axis=1, kind="stable")[:, :6]
    lists = [np.concatenate((top[q, ::2], [7, 4_599_990])) for q in range(4)]
    exclude = [int(top[q, 2]) for q in range(4)]
    filt = segment_filter(ops, lists, exclude, None, 0, t16.device)
    got = ops.topk(model, t16, t16[fixed_row].float(), torch.arange(4, device="cuda"), rel, rel_ids, qh, 10, filter=filt)
    check(got, expected(pred, 10, removed_mask(lists, exclude, None, N)))


def test_topk16_two_threads_two_streams(ops):
    problems = []
    for i, (model, dtype) in enumerate((("transe", torch.float16), ("distmult", torch.bfloat16))):
        table, rel, fixed_row, rel_ids = random_problem(model, 50_000 + 13 * i, 128, 96, seed=50 + i)
        t16, wide = rounded(table, dtype)
        problems.append((model, t16, [x.cuda() for x in (wide, rel, fixed_row, rel_ids)]))
    serial = [ops.topk(m, t, d[0], d[2], d[1], d[3], 48, 20) for m, t, d in problems]
    torch.cuda.synchronize()
    failures, start = [], threading.Barrier(2)

    def worker(i):
        try:
            m, t, d = problems[i]
            stream = torch.cuda.Stream()
            start.wait()
            with torch.cuda.stream(stream):
                for _ in range(6):
                    rows, scores = ops.topk(m, t, d[0], d[2], d[1], d[3], 48, 20)
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


def test_topk16_source_must_be_float32(ops):
    table, rel, fixed_row, rel_ids = (x.cuda() for x in random_problem("transe", 100, 64, 4, seed=1))
    t16 = table.half()
    with pytest.raises(TypeError, match="16-bit table needs a float32 `source`"):
        ops.topk("transe", t16, t16, fixed_row, rel, rel_ids, 2, 5)
    with pytest.raises(TypeError, match="source must be float32"):
        ops.topk("transe", t16, t16.clone(), fixed_row, rel, rel_ids, 2, 5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_predict_links_on_16bit_table_is_fused_and_equals_cpu_widened(monkeypatch, dtype):
    """predict_links on a device 16-bit table takes blp_topk_typed (the dense route would raise) and equals predict_links on
    the CPU float32 widened table, filtered, ids returned, bit for bit."""
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
        t16 = torch.from_numpy(g["ent_emb"]).to(dtype)
        cpu = ranking.predict_links(model, t16.float(), *args, **kw)

        def no_dense(*a, **k):
            raise AssertionError("the dense route was taken")

        monkeypatch.setattr(ranking, "_topk_dense", no_dense)
        gpu = ranking.predict_links(model.cuda(), t16.cuda(), *args, **kw)
        monkeypatch.undo()
        assert torch.equal(gpu[0].cpu(), cpu[0])
        assert torch.equal(gpu[1].cpu().view(torch.int32), cpu[1].view(torch.int32))
