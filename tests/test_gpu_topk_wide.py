"""blp_topk_wide on the MI355X: filtered top-k over the whole table for DistMult / ComplEx / SimplE at any width, rows exact
and scores bit-identical to the C oracle's scores (oracle.score_all) in numpy's stable order -- the judge of
test_gpu_topk.py, whose helpers are used here.

What the shapes aim at (topk_wide.hip): the sum order has a branch per width (wide_bilinear.h: whole rows of 32 terms, the
cascade at n >= 512, leftover vectors of 8, n % 8 tail terms; n = D for DistMult, D / 2 for the others); a wave's trip is 8
groups x 2 rows = 16 rows, a workgroup's 64, a chunk is 8 queries of one side; the slabs of a call are
min(2048 / chunks, trips), so every small table is cut into one-trip slabs that the merge kernel joins, a table of at most 64
rows is one slab, and 2 050 chunks or more walk the whole table in one slab."""
import numpy as np
import pytest
import torch

from test_gpu_rank_all_wide import SUM_ORDER
from test_gpu_topk import check, expected, oracle_pred, random_problem, removed_mask, segment_filter
from test_gpu_workspace_bounds import guard, three_fills  # noqa: F401  (guard is a fixture)

pytestmark = pytest.mark.gpu

BILINEAR = ("distmult", "complex", "simple")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


def scaled_problem(model, N, D, Q, seed, R=7):
    """random_problem with every entry carrying its own binary exponent over 2^-6 .. 2^6: the terms of a sum differ by up to
    2^36, so any reordering of the additions changes low bits of the score."""
    table, rel, fixed_row, rel_ids = random_problem(model, N, D, Q, R=R, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    scale = lambda t: t * torch.exp2(torch.randint(-6, 7, t.shape, generator=g).float())
    return scale(table), scale(rel), fixed_row, rel_ids


def pred_of(oracle, model, table, rel, fixed_row, rel_ids, q_head, source=None):
    source = table if source is None else source
    return oracle_pred(oracle, model, table.numpy(), source.numpy(), fixed_row.numpy(), rel.numpy(), rel_ids.numpy(), q_head)


def run(ops, model, table, rel, fixed_row, rel_ids, q_head, k, **kw):
    t = table if table.is_cuda else table.cuda()
    return ops.topk_wide(model, t, kw.pop("source", t), fixed_row.cuda(), rel.cuda(), rel_ids.cuda(), q_head, k, **kw)


# ------------------------------------------------------------------------------------------------ the sum order
@pytest.mark.parametrize("model,D", SUM_ORDER)
def test_every_branch_of_the_sum_order(ops, oracle, model, D):
    N, qh, qt = 523, 19, 21
    p = scaled_problem(model, N, D, qh + qt, seed=D)
    pred = pred_of(oracle, model, *p, qh)
    for k in (1, 10):
        check(run(ops, model, *p, qh, k), expected(pred, k), (model, D, k))


# ------------------------------------------------------------------------------------------------ table lengths, k
@pytest.mark.parametrize("model,D", [("distmult", 300), ("complex", 768), ("simple", 300)])
@pytest.mark.parametrize("N,k", [(1, 1), (15, 10), (16, 10), (17, 10), (63, 10), (64, 10), (65, 10), (523, 10), (5, 10)])
def test_table_lengths_and_padding(ops, oracle, model, D, N, k):
    """One group, one wave's trip, one workgroup's trip, each +- 1; k > N: the slots beyond the table are -1 / NaN."""
    qh, qt = 5, 4
    p = scaled_problem(model, N, D, qh + qt, seed=N)
    got = run(ops, model, *p, qh, k)
    check(got, expected(pred_of(oracle, model, *p, qh), k), (model, D, N, k))
    if k > N:
        assert bool((got[0][:, N:] == -1).all()) and bool(torch.isnan(got[1][:, N:]).all())


@pytest.fixture(scope="module")
def k_edges_problem(oracle):
    p = scaled_problem("distmult", 2000, 300, 9, seed=77)
    return p, pred_of(oracle, "distmult", *p, 5)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 192, 256])
def test_k_at_the_list_edges(ops, k_edges_problem, k):
    """A lane moves slots l, l + 64, ... of a list: k at one, two, three and four slots per lane and their edges."""
    p, pred = k_edges_problem
    check(run(ops, "distmult", *p, 5, k), expected(pred, k), k)


def test_lds_corner_complex_1024_k_256(ops, oracle):
    """64 KiB of coefficients + 64 KiB of lists: the launch raises the kernel's dynamic-LDS limit."""
    p = scaled_problem("complex", 2000, 1024, 11, seed=78)
    check(run(ops, "complex", *p, 6, 256), expected(pred_of(oracle, "complex", *p, 6), 256))


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("model,D", [("distmult", 300), ("complex", 768), ("simple", 300)])
def test_duplicate_rows_across_slabs_and_waves(ops, oracle, model, D):
    """5 % of the rows exact copies of five rows, spread over every slab (one trip of 64 rows each) and wave (16 rows): equal
    scores everywhere, more of them than k; the smaller row wins."""
    N, qh, qt = 2000, 10, 10
    table, rel, fixed_row, rel_ids = scaled_problem(model, N, D, qh + qt, seed=3)
    dup = torch.randperm(N, generator=torch.Generator().manual_seed(4))[: N // 20]
    table[dup] = table[dup % 5]
    table[[15, 16, 63, 64, 127, 128]] = table[0].clone()  # ... and on both sides of a wave's and a workgroup's boundary
    fixed_row[:8] = dup[:8]
    pred = pred_of(oracle, model, table, rel, fixed_row, rel_ids, qh)
    for k in (10, 256):
        check(run(ops, model, table, rel, fixed_row, rel_ids, qh, k), expected(pred, k), (model, k))


@pytest.mark.parametrize("model", BILINEAR)
def test_all_zero_table_rows_come_out_in_order(ops, oracle, model):
    N, D, qh, qt = 1000, 300, 5, 6
    _, rel, fixed_row, rel_ids = scaled_problem(model, N, D, qh + qt, seed=8)
    table = torch.zeros(N, D)
    source = torch.randn(N, D, generator=torch.Generator().manual_seed(9))
    pred = pred_of(oracle, model, table, rel, fixed_row, rel_ids, qh, source=source)
    for k in (10, 200):
        got = run(ops, model, table, rel, fixed_row, rel_ids, qh, k, source=source.cuda())
        check(got, expected(pred, k), (model, k))
        assert torch.equal(got[0].cpu(), torch.arange(k).expand(qh + qt, k))


# ------------------------------------------------------------------------------------------------ special values
@pytest.mark.parametrize("model", BILINEAR)
def test_nan_inf_and_signed_zero(ops, oracle, model):
    N, D, qh, qt = 700, 300, 6, 6
    table, rel, fixed_row, rel_ids = scaled_problem(model, N, D, qh + qt, seed=5)
    table[5, 3] = float("nan")
    table[7, 0] = float("inf")
    table[9, 1] = float("-inf")
    table[10, 150] = float("inf")
    table[10, 151] = float("-inf")
    table[11:40] = -0.0
    table[40:60, ::2] = -0.0
    table[60:80] = 0.0
    rel[0] = -0.0
    rel_ids[0] = rel_ids[qh] = 0
    fixed_row[1] = 11
    pred = pred_of(oracle, model, table, rel, fixed_row, rel_ids, qh)
    assert np.isnan(pred).any() and np.isinf(pred).any()
    for k in (1, 10, 100, 256):
        check(run(ops, model, table, rel, fixed_row, rel_ids, qh, k), expected(pred, k), (model, k))


@pytest.mark.parametrize("model,D", [("distmult", 300), ("distmult", 768), ("complex", 300), ("simple", 768), ("simple", 1024)])
def test_zero_scores_carry_the_oracle_s_sign(ops, oracle, model, D):
    """Zero rows (+0 and -0) against negative coefficients: every term is a -0, and the oracle's score is a zero whose sign
    the key must carry (the pass drops the additions of all-zero cascade levels; topk_wide.hip says why that cannot show).
    The other rows score below zero, so the zeros are the winners."""
    N, qh, qt, k = 300, 5, 4, 40
    g = torch.Generator().manual_seed(D)
    table = torch.rand(N, D, generator=g) + 0.5          # positive rows ...
    table[20:40] = 0.0
    table[100:120] = -0.0
    source = torch.rand(N, D, generator=g) + 0.5
    rel = -(torch.rand(7, D, generator=g) + 0.5)         # ... against negative relations
    if model == "complex":
        table[:, D // 2:] = 0.0                          # (real parts only: the score is sum(rr * hr * tr), negative)
        source[:, D // 2:] = 0.0
        rel[:, D // 2:] = 0.0
    fixed_row, rel_ids = torch.randint(0, N, (qh + qt,), generator=g), torch.randint(0, 7, (qh + qt,), generator=g)
    pred = pred_of(oracle, model, table, rel, fixed_row, rel_ids, qh, source=source)
    zero = pred[:, 20:40]
    assert (zero == 0).all() and (pred[:, :20] < 0).all()
    want = expected(pred, k)
    assert (want[1] == 0).all()
    got = run(ops, model, table, rel, fixed_row, rel_ids, qh, k, source=source.cuda())
    check(got, want, (model, D))
    assert np.array_equal(np.signbit(got[1].cpu().numpy()), np.signbit(want[1]))


# ------------------------------------------------------------------------------------------------ filters
@pytest.mark.parametrize("model", ["distmult", "complex"])
def test_filters(ops, oracle, model):
    """blp_rank_all's filter semantics: entity ids through ent2idx (-1 entries, ids beyond it), exclude never filtered, rows
    removed; one query keeps 3 of 50 rows at k = 10 (padding), one has a 5 000-entry segment."""
    D = 300
    for N, qh, qt in ((50, 2, 2), (6_000, 3, 3)):
        table, rel, fixed_row, rel_ids = scaled_problem(model, N, D, qh + qt, seed=N)
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
                seg = row2id[3:]                            # leaves rows 0, 1, 2
            elif N == 6_000 and q == 1:
                seg = rng.choice(n_ids + 50, 5_000, replace=False)  # (ids beyond ent2idx among them)
            else:
                seg = rng.choice(n_ids, min(N // 3, 40), replace=False)
            lists.append(seg)
            exclude.append(int(seg[len(seg) // 2]) if q % 2 else int(row2id[0 if N == 50 else fixed_row[q]]))
        pred = pred_of(oracle, model, table, rel, fixed_row, rel_ids, qh)
        removed = removed_mask(lists, exclude, ent2idx, N)
        filt = segment_filter(ops, lists, exclude, ent2idx, 0, torch.device("cuda"))
        for k in (1, 10, 256):
            got = run(ops, model, table, rel, fixed_row, rel_ids, qh, k, filter=filt)
            check(got, expected(pred, k, removed), (model, N, k))
            if N == 50 and k == 10:  # three rows, then padding
                assert (got[0][0, :3] >= 0).all() and (got[0][0, 3:] == -1).all()


@pytest.mark.parametrize("model", ["distmult", "simple"])
def test_shards_merge_to_unsharded(ops, oracle, model):
    """The table in three candidate shards (row_base), each with the global filter -- most of its entries outside the shard's
    [row_base, row_base + N) --, the lists merged by blp_topk_merge."""
    N, D, qh, qt = 3_011, 300, 5, 7
    table, rel, fixed_row, rel_ids = scaled_problem(model, N, D, qh + qt, seed=9)
    table[100:250] = table[7]  # ties across the shard boundaries
    rng = np.random.default_rng(9)
    lists = [rng.choice(N, 30, replace=False) for _ in range(qh + qt)]
    exclude = [int(x[0]) for x in lists]
    pred = pred_of(oracle, model, table, rel, fixed_row, rel_ids, qh)
    removed = removed_mask(lists, exclude, None, N)
    dev = torch.device("cuda")
    t = table.cuda()
    for k in (10, 256):
        whole = run(ops, model, t, rel, fixed_row, rel_ids, qh, k, filter=segment_filter(ops, lists, exclude, None, 0, dev))
        check(whole, expected(pred, k, removed), (model, k))
        parts = []
        for lo, hi in ((0, 90), (90, 2_100), (2_100, N)):
            f = segment_filter(ops, lists, exclude, None, lo, dev)
            parts.append(run(ops, model, t[lo:hi], rel, fixed_row, rel_ids, qh, k, source=t, filter=f, row_base=lo))
        rows, scores = ops.topk_merge(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), k)
        assert torch.equal(rows, whole[0])
        assert torch.equal(scores.view(torch.int32), whole[1].view(torch.int32))


# ------------------------------------------------------------------------------------------------ queries, strides, grids
@pytest.mark.parametrize("model", BILINEAR)
@pytest.mark.parametrize("qh,qt", [(0, 19), (19, 0), (140, 131)])
def test_query_sides_and_ragged_chunks(ops, oracle, model, qh, qt):
    N, D = 200, 300
    p = scaled_problem(model, N, D, qh + qt, seed=qh + 1)
    check(run(ops, model, *p, qh, 10), expected(pred_of(oracle, model, *p, qh), 10), (model, qh, qt))


def test_empty_block_and_empty_table(ops):
    table = torch.randn(50, 300).cuda()
    rel = torch.randn(3, 300).cuda()
    none = torch.zeros(0, dtype=torch.int64).cuda()
    rows, scores = ops.topk_wide("distmult", table, table, none, rel, none, 0, 10)
    assert tuple(rows.shape) == (0, 10) and tuple(scores.shape) == (0, 10)
    idx = torch.tensor([0, 1, 2, 3, 4]).cuda()
    out = (torch.full((5, 7), 77, dtype=torch.int64).cuda(), torch.zeros(5, 7).cuda())
    rows, scores = ops.topk_wide("complex", torch.zeros(0, 300).cuda(), table, idx, rel, idx % 3, 2, 7, out=out)
    assert rows is out[0] and bool((rows == -1).all()) and bool(torch.isnan(scores).all())


@pytest.mark.parametrize("model", BILINEAR)
def test_row_stride_wider_than_the_rows(ops, oracle, model):
    N, D, qh, qt = 150, 300, 7, 9
    p = scaled_problem(model, N, D, qh + qt, seed=31)
    padded = torch.full((N, D + 20), float("nan")).cuda()
    padded[:, :D] = p[0].cuda()
    view = padded[:, :D]
    assert view.stride(0) == D + 20
    check(run(ops, model, view, *p[1:], qh, 10, source=p[0].cuda()), expected(pred_of(oracle, model, *p, qh), 10), model)


@pytest.fixture(scope="module")
def fb_problem(oracle):
    """14 541 x 300, 1 024 head- and 1 024 tail-replacing queries, their oracle scores and the expected top 10: computed once,
    shared by the three grid regimes below (which take subsets and repetitions of these queries)."""
    table, rel, fixed_row, rel_ids = scaled_problem("distmult", 14_541, 300, 2_048, seed=237)
    want = expected(pred_of(oracle, "distmult", table, rel, fixed_row, rel_ids, 1_024), 10)
    return table.cuda(), rel, fixed_row, rel_ids, want


@pytest.mark.parametrize("n_head,n_tail,slabs", [(4, 4, 228), (1_024, 1_024, 8), (8_200, 8_200, 1)])
def test_fb15k237_sized_table_every_grid_regime(ops, fb_problem, n_head, n_tail, slabs):
    """14 541 x 300 (228 trips).  8 queries: two chunks, 228 slabs of one trip each, joined by the merge kernel.  2 048
    queries: 256 chunks, 8 slabs of 29 trips each.  16 400 queries (the 2 048, repeated): 2 050 chunks reach the target of
    2 048 workgroups alone -- ONE slab per chunk, every workgroup walks the whole table and the merge kernel reads one list
    per query."""
    table, rel, fixed_row, rel_ids, want = fb_problem
    pick = torch.cat((torch.arange(n_head) % 1_024, 1_024 + torch.arange(n_tail) % 1_024))
    need = ops.topk_wide_workspace_bytes("distmult", 14_541, 300, n_head, n_tail, 10)
    assert need == -(-(n_head + n_tail) * slabs * 10 * 8 // 256) * 256
    got = run(ops, "distmult", table, rel, fixed_row[pick], rel_ids[pick], n_head, 10)
    check(got, (want[0][pick.numpy()], want[1][pick.numpy()]), (n_head, n_tail))


def test_one_slab_per_chunk_on_a_short_table(ops, oracle):
    """16 400 distinct queries on 200 rows: one slab of four trips per chunk, the last trip ragged."""
    model, N, D, qh, qt = "simple", 200, 12, 8_200, 8_200
    p = scaled_problem(model, N, D, qh + qt, seed=41)
    assert ops.topk_wide_workspace_bytes(model, N, D, qh, qt, 10) == (qh + qt) * 10 * 8
    check(run(ops, model, *p, qh, 10), expected(pred_of(oracle, model, *p, qh), 10))


def test_the_same_call_twice_gives_the_same_bytes(ops):
    p = scaled_problem("complex", 5_003, 300, 40, seed=55)
    p[0][1000:1200] = p[0][3]
    a = run(ops, "complex", *p, 19, 10)
    b = run(ops, "complex", *p, 19, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ------------------------------------------------------------------------------------------------ workspace
@pytest.mark.parametrize("model,D,N,qh,qt,k", [("distmult", 300, 523, 21, 18, 10), ("complex", 768, 700, 3, 0, 256),
                                              ("simple", 1024, 64, 33, 32, 7), ("distmult", 300, 1, 0, 1, 1)])
def test_exact_workspace_between_guards(ops, oracle, guard, model, D, N, qh, qt, k):  # noqa: F811
    """A workspace of exactly the advertised bytes and the outputs, each between two 64 KiB guards, everything pre-filled with
    0x00 / 0xFF / 0xA5: the guards stay untouched, the three results are bit-identical and equal the oracle's.  The workspace
    is never cleared by the call -- every (chunk, slab) workgroup writes its lists, the empty ones too."""
    Q = qh + qt
    p = scaled_problem(model, N, D, Q, seed=43)
    rng = np.random.default_rng(44)
    lists = [rng.choice(N, min(N, 6), replace=False) for _ in range(Q)]
    filt = segment_filter(ops, lists, None, None, 0, torch.device("cuda"))
    need = ops.topk_wide_workspace_bytes(model, N, D, qh, qt, k)
    dev_p = [x.cuda() for x in p]

    def call(g):
        out = (g.out((Q, k), torch.int64), g.out((Q, k), torch.float32))
        return ops.topk_wide(model, dev_p[0], dev_p[0], dev_p[2], dev_p[1], dev_p[3], qh, k, filter=filt, out=out)

    got, requests = three_fills(guard, call, (model, D, N, k))
    assert requests == [need]
    check(got, expected(pred_of(oracle, model, *p, qh), k, removed_mask(lists, None, None, N)), (model, D, N, k))


# ------------------------------------------------------------------------------------------------ routing
def _toy(model_name, N, D, dtype=torch.float32, seed=61):
    from blp_amd import models, utils
    from test_gpu_shard import _problem
    table, rel_w, ent2idx, triples, edges = _problem(model_name, N, D, 40, 5, seed=seed)
    m = models.LinkPrediction(D, model_name, "margin", 5, 0)
    m.rel_emb.weight.data = rel_w.clone()
    return m, table.to(dtype), ent2idx, triples, utils.FilterIndex(edges, num_relations=5)


def _spy(ops, monkeypatch):
    calls = []
    for name in ("topk", "topk_wide", "topk_sets_wide"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    return calls


def _same(gpu, cpu):
    assert (cpu[0] >= 0).any() and torch.equal(gpu[0].cpu(), cpu[0])
    assert torch.equal(gpu[1].cpu().view(torch.int32), cpu[1].view(torch.int32))


@pytest.mark.parametrize("model_name,D,dtype,route", [("distmult", 300, torch.float32, "topk_wide"), ("complex", 768, torch.float32, "topk_wide"),
                                                       ("distmult", 1100, torch.float32, None), ("distmult", 300, torch.bfloat16, None),
                                                       ("transe", 300, torch.float32, "topk_sets_wide"),
                                                       ("transe", 300, torch.bfloat16, "topk_sets_wide"),
                                                       ("distmult", 128, torch.float32, "topk")])
def test_predict_links_route(ops, monkeypatch, model_name, D, dtype, route):
    """Which fused call ranking.predict_links reaches (none: the dense route), and that the result equals the CPU route's on
    the same table (a 16-bit table widened: the fused calls' contract) bit for bit -- the dense route's too: on the device
    score_fn is blp_score_fwd, the reference's bits."""
    from blp_amd import ranking
    m, table, ent2idx, triples, index = _toy(model_name, 700, D, dtype)
    cpu = ranking.predict_links(m, table.float(), triples, 10, ent2idx, filter_index=index)
    calls = _spy(ops, monkeypatch)
    if route is None and dtype != torch.float32:
        # no fused call is tried; the dense route it is left with does not take a 16-bit device table (score_fn's kernel reads
        # float32 rows) and says so, as before
        with pytest.raises(TypeError, match="must be float32"):
            ranking.predict_links(m.cuda(), table.cuda(), triples.cuda(), 10, ent2idx.cuda(), filter_index=index)
        assert calls == []
        return
    gpu = ranking.predict_links(m.cuda(), table.cuda(), triples.cuda(), 10, ent2idx.cuda(), filter_index=index)
    assert calls == ([route] if route else [])
    _same(gpu, cpu)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("side", ["head", "tail"])
def test_one_set_route_with_one_side_only(ops, monkeypatch, side, dtype):
    """q_head = Q and q_head = 0 through the one-set route: the other side's group of the set is empty ([0, 0])."""
    from blp_amd import ranking
    m, table, ent2idx, triples, index = _toy("transe", 700, 300, dtype, seed=71)
    cpu = ranking.predict_links(m, table.float(), triples, 10, ent2idx, side=side, filter_index=index)
    calls = _spy(ops, monkeypatch)
    gpu = ranking.predict_links(m.cuda(), table.cuda(), triples.cuda(), 10, ent2idx.cuda(), side=side, filter_index=index)
    assert calls == ["topk_sets_wide"] and tuple(gpu[0].shape) == (triples.shape[0], 10)
    _same(gpu, cpu)


def test_one_set_route_in_row_base_shards(ops):
    """What a rank of a sharded predict_links hands the one-set route: a shard of the table with its row_base, the queries'
    vectors in a `source` of their own, the global filter.  Three shards merged by blp_topk_merge equal the unsharded call,
    which equals the dense route on CPU tensors."""
    from blp_amd import models, ranking
    N, D, qh, qt, k = 1_501, 300, 9, 11, 10
    table, rel, fixed_row, rel_ids = random_problem("transe", N, D, qh + qt, seed=81)
    table[200:300] = table[7]  # ties across the shard boundaries
    rng = np.random.default_rng(81)
    lists = [rng.choice(N, 30, replace=False) for _ in range(qh + qt)]
    exclude = [int(x[0]) for x in lists]
    score_fn = models.LinkPrediction(D, "transe", "margin", 7, 0).score_fn
    i64 = lambda a: torch.as_tensor(np.asarray(a, np.int64))
    lo_ = np.cumsum([0] + [len(x) for x in lists[:-1]])
    cpu_filt = (i64(lo_), i64(lo_ + 30), i64(np.concatenate(lists)), i64(exclude), None)
    cpu = ranking._topk_dense(score_fn, table, table[fixed_row], rel[rel_ids], qh, k, 0, cpu_filt)
    dev = torch.device("cuda")
    t, source = table.cuda(), table[fixed_row].cuda()
    src_rows = torch.arange(qh + qt).cuda()
    args = (source, src_rows, rel.cuda(), rel_ids.cuda(), qh, k)
    whole = ranking._topk_one_set("transe", t, *args, filter=segment_filter(ops, lists, exclude, None, 0, dev))
    _same(whole, cpu)
    parts = [ranking._topk_one_set("transe", t[lo:hi], *args, filter=segment_filter(ops, lists, exclude, None, lo, dev), row_base=lo)
             for lo, hi in ((0, 250), (250, 1_000), (1_000, N))]
    rows, scores = ops.topk_merge(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), k)
    assert torch.equal(rows, whole[0]) and torch.equal(scores.view(torch.int32), whole[1].view(torch.int32))

