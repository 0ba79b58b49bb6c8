"""Relation prediction on the MI355X (blp_rank_relations / blp_topk_relations through blp_amd.ops and ranking).  Everything is
compared bit for bit -- counts, relation ids, scores as int32 patterns, NaN positions, empty slots exactly -1 / 0x7fc00000 --
against the C oracle's score of every expanded (pair, relation) (oracle.score_pairs) and numpy's stable order: every model and
width, R around the 64-row tile and the 256-row workgroup, Q around the query chunks, k around list_insert's 64-slot groups,
ties, NaN / inf / -0, filters, padded score rows, the reference's goldens, a source above 2^31 bytes, two threads on two
streams, the Python route, and the same queries inside a larger call."""
import threading

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden, golden_names
from test_rank_relations_host import (NAN_BITS, make_model, relation_matrix, removed_mask, same_scores, same_topk, want_counts,
                                      want_topk)

pytestmark = pytest.mark.gpu

DEV = "cuda"
RS = (1, 11, 63, 64, 65, 237, 822)  # a lone lane, a partial tile, the tile edge, one workgroup's worth, several tile groups
KS = (1, 5, 64, 65, 256)            # R < k among them; 65: the second 64-slot group of list_insert
CASES = [(m, D) for m in REL_MODELS for D in (64, 128, 256)]


@pytest.fixture(scope="module")
def ops():
    from blp_amd import ops as _ops
    return _ops


def problem(S, D, R, Q, seed):
    g = torch.Generator().manual_seed(seed)
    source = torch.randn((S, D), generator=g)
    rel_w = torch.randn((R, D), generator=g)
    head_row = torch.randint(0, S, (Q,), generator=g)
    tail_row = torch.randint(0, S, (Q,), generator=g)
    true_rel = torch.randint(0, R, (Q,), generator=g)
    true_rel[0], true_rel[-1] = 0, R - 1
    return source, rel_w, head_row, tail_row, true_rel


def matrix(oracle, model, source, rel_w, head_row, tail_row):
    return relation_matrix(oracle, model, source[head_row].numpy(), source[tail_row].numpy(), rel_w.numpy())


def segment_filter(ops, segs, exclude):
    lens = np.array([len(s) for s in segs], np.int64)
    hi = np.cumsum(lens)
    values = np.concatenate([np.asarray(s, np.int64) for s in segs] + [np.zeros(0, np.int64)])
    t = lambda a: torch.as_tensor(np.asarray(a, np.int64)).to(DEV)
    return ops.SegmentFilter(t(hi - lens), t(hi), t(values), None if exclude is None else t(exclude), None, 0)


def check_topk(got, want, what=""):
    same_topk(got, want, what)
    scores = got[1].cpu().numpy()
    assert (scores[np.isnan(want[1])].view(np.int32) == NAN_BITS).all(), what  # empty slots and NaN scores alike: the quiet NaN


def rank(ops, model, source, head_row, tail_row, rel_w, true_rel=None, **kw):
    t = lambda a: None if a is None else a.to(DEV)
    return ops.rank_relations(model, t(source), t(head_row), t(tail_row), t(rel_w), t(true_rel), **kw)


def topk(ops, model, source, head_row, tail_row, rel_w, k, **kw):
    t = lambda a: a.to(DEV)
    return ops.topk_relations(model, t(source), t(head_row), t(tail_row), t(rel_w), k, **kw)


@pytest.mark.parametrize("model,D", CASES)
def test_counts_scores_and_topk_match_the_oracle(ops, oracle, model, D):
    Q = 12
    for R in RS:
        source, rel_w, hr, tr, true_rel = problem(500, D, R, Q, seed=D + R)
        S = matrix(oracle, model, source, rel_w, hr, tr)
        none = np.zeros((Q, R), bool)
        want = want_counts(S, true_rel.numpy(), none)
        counts, scores = rank(ops, model, source, hr, tr, rel_w, true_rel, return_scores=True)
        assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), want), (model, D, R)
        same_scores(scores, S, (model, D, R))
        assert np.array_equal(rank(ops, model, source, hr, tr, rel_w, true_rel).cpu().numpy(), want), (model, D, R, "counts only")
        same_scores(rank(ops, model, source, hr, tr, rel_w, return_scores=True), S, (model, D, R, "scores only"))
        for k in KS if R in (11, 65, 237, 822) else (5,):
            check_topk(topk(ops, model, source, hr, tr, rel_w, k), want_topk(S, none, k), (model, D, R, k))


@pytest.mark.parametrize("model,D", [("transe", 64), ("distmult", 128), ("complex", 256)])
def test_query_counts_around_the_chunks(ops, oracle, model, D):
    """rank_rels takes 64 queries per workgroup pass; topk_rels 24 576 / (32 k) of them, at most 32: k = 5 -> 32, k = 256 -> 3."""
    R = 70
    source, rel_w, hr, tr, true_rel = problem(300, D, R, 129, seed=11)
    S = matrix(oracle, model, source, rel_w, hr, tr)
    none = np.zeros((129, R), bool)
    for Q in (1, 63, 64, 65, 128, 129):
        counts, scores = rank(ops, model, source, hr[:Q], tr[:Q], rel_w, true_rel[:Q], return_scores=True)
        assert np.array_equal(counts.cpu().numpy(), want_counts(S[:Q], true_rel[:Q].numpy(), none[:Q])), Q
        same_scores(scores, S[:Q], Q)
    for k, Qs in ((5, (1, 31, 32, 33, 65)), (256, (1, 2, 3, 4, 7))):
        for Q in Qs:
            check_topk(topk(ops, model, source, hr[:Q], tr[:Q], rel_w, k), want_topk(S[:Q], none[:Q], k), (k, Q))


@pytest.mark.parametrize("model", REL_MODELS)
def test_ties_nan_inf_and_signed_zero(ops, oracle, model):
    D, R, Q = 64, 300, 12
    source, rel_w, hr, tr, true_rel = problem(200, D, R, Q, seed=6)
    g = torch.Generator().manual_seed(7)
    copies = torch.randperm(R - 20, generator=g)[:15] + 20  # 5 % of the relation rows are copies of others: ties by ascending id
    rel_w[copies] = rel_w[torch.randint(0, 20, (15,), generator=g)]
    rel_w[3, 5], rel_w[4, 0], rel_w[5, 63], rel_w[6, 1] = float("nan"), float("inf"), float("-inf"), -0.0
    rel_w[7], rel_w[8] = 0.0, -0.0                           # all-zero rows of either sign: the sign of a zero score
    source[hr[1], 2], source[tr[2], 7], source[hr[3], 9] = float("nan"), float("inf"), float("-inf")
    source[hr[4]] = 0.0
    source[tr[5]] = -0.0
    true_rel[6], true_rel[7], true_rel[8] = 3, 7, int(copies[0])  # a NaN true score, a zero one, a tied one
    S = matrix(oracle, model, source, rel_w, hr, tr)
    assert np.isnan(S).any() and np.isinf(S).any()
    none = np.zeros((Q, R), bool)
    counts, scores = rank(ops, model, source, hr, tr, rel_w, true_rel, return_scores=True)
    assert np.array_equal(counts.cpu().numpy(), want_counts(S, true_rel.numpy(), none))
    same_scores(scores, S)
    for k in (5, 65, 256):
        check_topk(topk(ops, model, source, hr, tr, rel_w, k), want_topk(S, none, k), k)


@pytest.mark.parametrize("model,R", [("transe", 237), ("simple", 822), ("distmult", 11)])
def test_filters(ops, oracle, model, R):
    D, Q = 128, 12
    source, rel_w, hr, tr, true_rel = problem(300, D, R, Q, seed=R)
    S = matrix(oracle, model, source, rel_w, hr, tr)
    true = true_rel.numpy()
    rng = np.random.default_rng(R)
    segs = [rng.choice(R, size=min(R, 4), replace=False) for _ in range(Q)]
    segs[0] = np.zeros(0, np.int64)                                         # an empty segment
    segs[1] = np.array([r for r in range(R) if r != true[1]])               # every relation but the true one
    segs[2] = np.array([R, R + 7, 1 << 40, -1, 2])                          # ids that are no relation are ignored
    segs[3] = np.array([true[3], (true[3] + 1) % R])                        # names the true relation: exclude keeps it
    segs[4] = np.arange(R)                                                  # everything named: only exclude survives
    keep3 = rng.choice(R, size=3, replace=False)
    segs[5] = np.array([r for r in range(R) if r not in keep3])             # a query left with 3 relations
    for exclude in (true, None):
        ex = true if exclude is not None else np.full(Q, -1)
        removed = removed_mask(segs, ex, Q, R)
        filt = segment_filter(ops, segs, exclude)
        counts = rank(ops, model, source, hr, tr, rel_w, true_rel, filter=filt)
        assert np.array_equal(counts.cpu().numpy(), want_counts(S, true, removed)), exclude is None
        for k in (1, 5, 65):
            got = topk(ops, model, source, hr, tr, rel_w, k, filter=filt)
            want = want_topk(S, removed, k)
            check_topk(got, want, (k, exclude is None))
            if k == 5:
                left = 3 + (exclude is not None and true[5] not in keep3)
                assert (want[0][5] >= 0).sum() == min(left, R) and (want[0][4] >= 0).sum() == (exclude is not None)
    # without a filter the last two counts equal the first two
    plain = rank(ops, model, source, hr, tr, rel_w, true_rel).cpu().numpy()
    assert np.array_equal(plain[:, 2:], plain[:, :2])


def test_score_rows_with_padding_are_left_alone(ops, oracle):
    from blp_amd import _lib
    model, D, R, Q, pad = "complex", 64, 70, 9, 6
    source, rel_w, hr, tr, true_rel = problem(100, D, R, Q, seed=2)
    S = matrix(oracle, model, source, rel_w, hr, tr)
    src, rw, h, t, tru = (x.to(DEV) for x in (source, rel_w, hr, tr, true_rel))
    out = torch.full((Q, R + pad), 12345.0, device=DEV)
    counts = torch.empty((Q, 4), dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.rank_relations_workspace_bytes(model, D, Q, R), dtype=torch.uint8, device=DEV)
    status = _lib.lib().blp_rank_relations(_lib.MODEL_IDS[model], src.data_ptr(), 100, D, D, h.data_ptr(), t.data_ptr(), Q, rw.data_ptr(), R,
                                           tru.data_ptr(), None, counts.data_ptr(), out.data_ptr(), R + pad, ws.data_ptr(), ws.numel(), 0,
                                           torch.cuda.current_stream().cuda_stream)
    assert status == 0
    torch.cuda.synchronize()
    same_scores(out[:, :R].contiguous(), S)
    assert bool((out[:, R:] == 12345.0).all())
    assert np.array_equal(counts.cpu().numpy(), want_counts(S, true_rel.numpy(), np.zeros((Q, R), bool)))


@pytest.mark.parametrize("name", golden_names("scores_"))
def test_true_relation_column_equals_the_goldens_true_triple_score(name):
    from blp_amd import ranking
    g = golden(name)
    rel_model = name.split("_")[1]
    heads, tails, rels = g["heads"][:, 0], g["tails"][:, 0], g["rels"][:, 0]
    triples = torch.from_numpy(np.stack((heads, tails, rels), 1).astype(np.int64))
    table = torch.from_numpy(g["table"]).to(DEV)
    assert table.shape[1] in (64, 128, 256)  # a width the fused route takes: this is the kernel, not the dense route
    model = make_model(rel_model, g["rel_w"]).to(DEV)
    counts, scores = ranking.rank_relations(model, table, triples, torch.arange(table.shape[0]), return_scores=True)
    q = np.arange(len(heads))
    same_scores(scores.cpu().numpy()[q, rels], g["head_pred"][q, heads], name)
    assert bool((counts[:, 1] >= 1).all()) or np.isnan(g["head_pred"][q, heads]).any()


@pytest.mark.parametrize("model", ["transe", "simple"])
def test_head_row_equals_tail_row(ops, oracle, model):
    source, rel_w, hr, _, true_rel = problem(50, 128, 40, 12, seed=9)
    S = matrix(oracle, model, source, rel_w, hr, hr)
    none = np.zeros(S.shape, bool)
    counts, scores = rank(ops, model, source, hr, hr, rel_w, true_rel, return_scores=True)
    assert np.array_equal(counts.cpu().numpy(), want_counts(S, true_rel.numpy(), none))
    same_scores(scores, S)
    check_topk(topk(ops, model, source, hr, hr, rel_w, 5), want_topk(S, none, 5))


def test_source_above_two_gib(ops, oracle):
    """Rows whose byte offset needs more than 31 bits: row x ld is 64-bit arithmetic everywhere."""
    model, D, R, Q = "distmult", 64, 70, 8
    S_rows = (1 << 31) // (4 * D) + 1000
    small, rel_w, _, _, true_rel = problem(2 * Q, D, R, Q, seed=4)
    big = torch.zeros((S_rows, D), device=DEV)
    assert big.numel() * 4 > 1 << 31
    hr = torch.arange(S_rows - Q, S_rows)
    tr = torch.cat((torch.arange(Q // 2), torch.arange(S_rows - 2 * Q, S_rows - 2 * Q + Q // 2)))
    big[hr.to(DEV)] = small[:Q].to(DEV)
    big[tr.to(DEV)] = small[Q:].to(DEV)
    S = relation_matrix(oracle, model, small[:Q].numpy(), small[Q:].numpy(), rel_w.numpy())
    none = np.zeros((Q, R), bool)
    counts, scores = ops.rank_relations(model, big, hr.to(DEV), tr.to(DEV), rel_w.to(DEV), true_rel.to(DEV), return_scores=True)
    assert np.array_equal(counts.cpu().numpy(), want_counts(S, true_rel.numpy(), none))
    same_scores(scores, S)
    check_topk(ops.topk_relations(model, big, hr.to(DEV), tr.to(DEV), rel_w.to(DEV), 5), want_topk(S, none, 5))


def test_two_threads_on_two_streams(ops, oracle):
    jobs = []
    for i, (model, R) in enumerate((("transe", 237), ("complex", 822))):
        source, rel_w, hr, tr, true_rel = problem(400, 128, R, 200, seed=20 + i)
        S = matrix(oracle, model, source, rel_w, hr, tr)
        jobs.append(dict(model=model, args=[x.to(DEV) for x in (source, hr, tr, rel_w)], true=true_rel, S=S, out=None))
    torch.cuda.synchronize()

    def work(job):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            for _ in range(3):
                counts = ops.rank_relations(job["model"], *job["args"], job["true"].to(DEV))
                top = ops.topk_relations(job["model"], *job["args"], 10)
            stream.synchronize()
        job["out"] = (counts.cpu(), top[0].cpu(), top[1].cpu())

    threads = [threading.Thread(target=work, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for job in jobs:
        none = np.zeros(job["S"].shape, bool)
        assert np.array_equal(job["out"][0].numpy(), want_counts(job["S"], job["true"].numpy(), none))
        check_topk(job["out"][1:], want_topk(job["S"], none, 10))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("model", ["transe", "complex"])
def test_python_route_on_a_device_table_equals_the_cpu_route(model, dtype):
    from blp_amd import ranking, utils
    N, D, R, T = 120, 128, 30, 40
    g = torch.Generator().manual_seed(12)
    table = torch.randn((N, D), generator=g).to(dtype)
    rel_w = torch.randn((R, D), generator=g)
    entities = torch.randperm(N + 30, generator=g)[:N]
    ent2idx = utils.make_ent2idx(entities, N + 29)
    triples = torch.stack((entities[torch.randint(0, N, (T,), generator=g)], entities[torch.randint(0, N, (T,), generator=g)],
                           torch.randint(0, R, (T,), generator=g)), 1)
    edges = torch.cat((triples, torch.stack((triples[:, 0], triples[:, 1], torch.randint(0, R, (T,), generator=g)), 1)))
    index = utils.RelationFilterIndex(edges)
    cpu, gpu = make_model(model, rel_w.numpy()), make_model(model, rel_w.numpy()).to(DEV)
    for fi in (None, index):
        want = ranking.rank_relations(cpu, table, triples, ent2idx, filter_index=fi, return_scores=True)
        got = ranking.rank_relations(gpu, table.to(DEV), triples, ent2idx, filter_index=fi, return_scores=True)
        assert np.array_equal(got[0].cpu().numpy(), want[0].numpy())
        same_scores(got[1], want[1].numpy())
        if fi is not None:
            assert bool((want[0][:, 2:] != want[0][:, :2]).any()), "the filter must bite somewhere"
        for k, pairs in ((5, triples), (R + 3, triples[:, :2]), (300, triples)):  # 300 > 256: the dense route on the device
            want_k = ranking.predict_relations(cpu, table, pairs, k, ent2idx, filter_index=fi)
            got_k = ranking.predict_relations(gpu, table.to(DEV), pairs, k, ent2idx, filter_index=fi)
            same_topk(got_k, tuple(x.numpy() for x in want_k), (k, fi is not None))


@pytest.mark.parametrize("model,R", [("transe", 237), ("distmult", 822)])
def test_the_same_queries_inside_a_larger_call(ops, oracle, model, R):
    """The kernels have no tiling knob: three queries alone (one workgroup) and leading a Q = 4 096 call (64 / 128 workgroups,
    other chunk neighbours) give the same bits."""
    D, big = 128, 4096
    source, rel_w, hr, tr, true_rel = problem(300, D, R, big, seed=31)
    S = matrix(oracle, model, source, rel_w, hr[:3], tr[:3])
    none = np.zeros((3, R), bool)
    few = rank(ops, model, source, hr[:3], tr[:3], rel_w, true_rel[:3], return_scores=True)
    many = rank(ops, model, source, hr, tr, rel_w, true_rel, return_scores=True)
    assert np.array_equal(few[0].cpu().numpy(), want_counts(S, true_rel[:3].numpy(), none))
    assert torch.equal(many[0][:3], few[0]) and torch.equal(many[1][:3].view(torch.int32), few[1].view(torch.int32))
    same_scores(few[1], S)
    for k in (10, 65):
        few_k = topk(ops, model, source, hr[:3], tr[:3], rel_w, k)
        many_k = topk(ops, model, source, hr, tr, rel_w, k)
        check_topk(few_k, want_topk(S, none, k), k)
        assert torch.equal(many_k[0][:3], few_k[0]) and torch.equal(many_k[1][:3].view(torch.int32), few_k[1].view(torch.int32))
