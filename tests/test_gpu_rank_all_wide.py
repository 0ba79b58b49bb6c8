"""blp_rank_all_wide on the MI355X: DistMult / ComplEx / SimplE ranked against the whole table at any width, counts
bit-equal to the C oracle (oracle.rank_counts through the helpers of test_gpu_parity.py).

What the shapes aim at (rank_all_wide.hip): the sum order has a branch per width -- whole rows of 32 terms, the cascade
after rows 16 and 32 (n >= 512), leftover vectors of 8, n % 8 tail terms; n = D for DistMult, D / 2 for the others --; a
workgroup takes 8 queries and 64 rows per trip (16 per wave), so N = 63 / 64 / 65 / 523 and 21 / 18 queries leave ragged
chunks, trips and waves; a candidate slab is ~2 MB, so 14 541 x 300 makes several."""
import numpy as np
import pytest
import torch

from test_gpu_parity import oracle_counts, random_csr, random_problem

pytestmark = pytest.mark.gpu

BILINEAR = ("distmult", "complex", "simple")
GUARD = 1 << 16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


def run(ops, model, table, q_fixed, q_rel, q_head, true_row=None, q_true=None, csr=None, **kw):
    c = lambda t: None if t is None else t.cuda()
    if csr is not None:
        kw.update(filt_rowptr=torch.from_numpy(csr[0]).cuda(), filt_col=torch.from_numpy(csr[1]).cuda())
    out = ops.rank_all_wide(model, table.cuda() if not table.is_cuda else table, c(q_fixed), c(q_rel), q_head, true_row=c(true_row),
                            q_true=c(q_true), **kw)
    return out.cpu().numpy()


def scaled_problem(model, N, D, q_head, q_tail, seed):
    """random_problem with every entry carrying its own binary exponent over 2^-20 .. 2^20: the terms of a sum differ by
    up to 2^120, so any reordering of the additions changes low bits of the score."""
    table, q_fixed, q_rel, true_row = random_problem(model, N, D, q_head, q_tail, seed)
    g = torch.Generator().manual_seed(seed + 1)
    scale = lambda t: t * torch.exp2(torch.randint(-20, 21, t.shape, generator=g).float())
    return scale(table), scale(q_fixed), scale(q_rel), true_row


SUM_ORDER = [("distmult", D) for D in (4, 8, 12, 32, 36, 100, 300, 508, 512, 516, 768, 1020, 1024)] + \
            [(m, D) for m in ("complex", "simple") for D in (12, 20, 64, 128, 300, 768, 1000, 1024)]


@pytest.mark.parametrize("model,D", SUM_ORDER)
def test_every_branch_of_the_sum_order(ops, oracle, model, D):
    N, q_head, q_tail = 523, 21, 18
    table, q_fixed, q_rel, true_row = scaled_problem(model, N, D, q_head, q_tail, seed=D)
    csr = random_csr(q_head + q_tail, N, true_row.numpy(), seed=D + 3)
    want = oracle_counts(oracle, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr)
    got = run(ops, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr)
    np.testing.assert_array_equal(got, want)
    got = run(ops, model, table, q_fixed, q_rel, q_head, q_true=table[true_row].clone(), csr=csr)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("model", BILINEAR)
@pytest.mark.parametrize("D", [300, 768])
def test_order_matters_copies_of_the_true_row_tie(ops, oracle, model, D):
    """5 % of the rows are bit-identical copies of queries' true rows: the table pass must give such a row the very number
    the true-key routine gives the true row (ge, not gt), on both sides."""
    N, q_head, q_tail = 523, 21, 18
    Q = q_head + q_tail
    table, q_fixed, q_rel, true_row = scaled_problem(model, N, D, q_head, q_tail, seed=7 * D)
    rng = np.random.default_rng(D)
    true_row = torch.from_numpy(rng.choice(N // 2, size=Q, replace=False).astype(np.int64))  # distinct, in the lower half
    spots = rng.choice(np.arange(N // 2, N), size=N // 20, replace=False)
    copies = np.zeros(Q, np.int64)
    for i, s in enumerate(spots):
        q = i % Q
        table[s] = table[true_row[q]]
        copies[q] += 1
    assert copies.sum() == N // 20 and copies.max() >= 1
    want = oracle_counts(oracle, model, table, q_fixed, q_rel, q_head, true_row=true_row)
    got = run(ops, model, table, q_fixed, q_rel, q_head, true_row=true_row)
    np.testing.assert_array_equal(got, want)
    # the true row itself and its copies tie; with exponents spread over 2^40 nothing else does
    np.testing.assert_array_equal(got[:, 1] - got[:, 0], copies + 1)


@pytest.mark.parametrize("model", BILINEAR)
def test_special_values(ops, oracle, model):
    N, D, q_head, q_tail = 200, 300, 9, 11
    table, q_fixed, q_rel, true_row = random_problem(model, N, D, q_head, q_tail, seed=5)
    table[3, 7] = float("nan")
    table[10, 0] = float("inf")
    table[11, 299] = float("-inf")
    table[12, 150] = float("inf")
    table[12, 151] = float("-inf")
    table[20] = -0.0
    table[21] = 0.0
    table[22, ::2] = -0.0
    q_fixed[2, 5] = float("inf")
    q_rel[4, 9] = float("nan")
    q_fixed[13] = -0.0
    true_row[0], true_row[1], true_row[12] = 20, 3, 10
    csr = random_csr(q_head + q_tail, N, true_row.numpy(), seed=6)
    want = oracle_counts(oracle, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr)
    got = run(ops, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("model", BILINEAR)
def test_all_zero_table_every_pair_ties(ops, oracle, model):
    N, D, q_head, q_tail = 131, 300, 5, 6
    _, q_fixed, q_rel, true_row = random_problem(model, N, D, q_head, q_tail, seed=8)
    table = torch.zeros(N, D)
    got = run(ops, model, table, q_fixed, q_rel, q_head, true_row=true_row)
    np.testing.assert_array_equal(got, oracle_counts(oracle, model, table, q_fixed, q_rel, q_head, true_row=true_row))
    np.testing.assert_array_equal(got[:, 0], 0)
    np.testing.assert_array_equal(got[:, 1], N)


@pytest.mark.parametrize("model,D", [("distmult", 300), ("complex", 768), ("simple", 300)])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 523])
def test_table_lengths(ops, oracle, model, D, N):
    q_head, q_tail = 5, 4
    table, q_fixed, q_rel, true_row = random_problem(model, N, D, q_head, q_tail, seed=N)
    csr = random_csr(q_head + q_tail, N, true_row.numpy(), seed=N + 1, max_per_row=min(9, N))
    want = oracle_counts(oracle, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr)
    np.testing.assert_array_equal(run(ops, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr), want)


@pytest.mark.parametrize("model", BILINEAR)
@pytest.mark.parametrize("q_head,q_tail", [(0, 19), (19, 0), (140, 131)])
def test_query_sides_and_chunks(ops, oracle, model, q_head, q_tail):
    N, D = 200, 300
    table, q_fixed, q_rel, true_row = random_problem(model, N, D, q_head, q_tail, seed=q_head + 1)
    csr = random_csr(q_head + q_tail, N, true_row.numpy(), seed=q_tail + 2)
    want = oracle_counts(oracle, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr)
    np.testing.assert_array_equal(run(ops, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr), want)


def test_empty_block_and_empty_table(ops):
    table = torch.randn(50, 300).cuda()
    none = torch.zeros(0, 300).cuda()
    assert tuple(ops.rank_all_wide("distmult", table, none, none, 0, true_row=torch.zeros(0, dtype=torch.int64).cuda()).shape) == (0, 4)
    q = torch.randn(5, 300).cuda()
    out = torch.full((5, 4), 77, dtype=torch.int32).cuda()
    got = ops.rank_all_wide("complex", none, q, q, 2, q_true=q, out=out)
    assert got is out and bool((out == 0).all())


@pytest.mark.parametrize("model", BILINEAR)
def test_row_stride_wider_than_the_rows(ops, oracle, model):
    N, D, q_head, q_tail = 150, 300, 7, 9
    table, q_fixed, q_rel, true_row = random_problem(model, N, D, q_head, q_tail, seed=31)
    padded = torch.full((N, D + 20), float("nan")).cuda()
    padded[:, :D] = table.cuda()
    view = padded[:, :D]
    assert view.stride(0) == D + 20
    want = oracle_counts(oracle, model, table, q_fixed, q_rel, q_head, true_row=true_row)
    np.testing.assert_array_equal(run(ops, model, view, q_fixed, q_rel, q_head, true_row=true_row), want)


def test_fb15k237_sized_table_several_slabs(ops, oracle):
    """14 541 x 300 with 300 queries: several candidate slabs, several workgroups per chunk, atomics from all of them."""
    model, N, D, q_head, q_tail = "distmult", 14541, 300, 150, 150
    table, q_fixed, q_rel, true_row = random_problem(model, N, D, q_head, q_tail, seed=237)
    csr = random_csr(q_head + q_tail, N, true_row.numpy(), seed=238)
    want = oracle_counts(oracle, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr)
    np.testing.assert_array_equal(run(ops, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr), want)


# ---------------------------------------------------------------------------------------------- filters
def segment_problem(model, N, D, q_head, q_tail, seed, n_ids):
    """A segment filter over entity ids: ent2idx with -1 entries and ids beyond its length, exclude = one value of the query's
    own segment, an empty segment, and one segment longer than a 64-entry step.  Returns the SegmentFilter's arrays and the
    equivalent CSR of table rows for the oracle."""
    rng = np.random.default_rng(seed)
    table, q_fixed, q_rel, true_row = random_problem(model, N, D, q_head, q_tail, seed)
    Q = q_head + q_tail
    ent2idx = np.full(n_ids, -1, np.int64)
    ids = rng.choice(n_ids, size=N, replace=False)
    ent2idx[ids] = np.arange(N)
    values, lo, hi, exclude, cols, rowptr = [], [], [], [], [], [0]
    for q in range(Q):
        k = 0 if q % 5 == 0 else (150 if q == 3 else int(rng.integers(1, 12)))
        seg = rng.choice(n_ids + 10, size=k, replace=False)  # ids without a row (-1) and ids beyond ent2idx among them
        ex = int(seg[0]) if k else -7
        lo.append(len(values))
        values.extend(int(v) for v in seg)
        hi.append(len(values))
        exclude.append(ex)
        rows = [int(ent2idx[v]) for v in seg if v != ex and v < n_ids and ent2idx[v] >= 0]
        cols.append(np.sort(np.asarray(rows, np.int64)))
        rowptr.append(rowptr[-1] + len(rows))
    i64 = lambda x: torch.tensor(x, dtype=torch.int64)
    seg = (i64(lo), i64(hi), i64(values), i64(exclude), torch.from_numpy(ent2idx))
    return table, q_fixed, q_rel, true_row, seg, (np.asarray(rowptr, np.int64), np.concatenate(cols).astype(np.int64))


@pytest.mark.parametrize("model", BILINEAR)
def test_segment_filter_with_ent2idx_and_exclude(ops, oracle, model):
    N, D, q_head, q_tail = 400, 300, 11, 13
    table, q_fixed, q_rel, true_row, seg, csr = segment_problem(model, N, D, q_head, q_tail, seed=17, n_ids=600)
    want = oracle_counts(oracle, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr)
    assert (want[:, 0] != want[:, 2]).any()  # the filter removes something that counts
    filt = ops.SegmentFilter(*(t.cuda() for t in seg), 0)
    np.testing.assert_array_equal(run(ops, model, table, q_fixed, q_rel, q_head, true_row=true_row, filter=filt), want)


@pytest.mark.parametrize("model", BILINEAR)
def test_row_base_shards_add_up(ops, oracle, model):
    N, D, q_head, q_tail = 400, 300, 11, 13
    table, q_fixed, q_rel, true_row, seg, csr = segment_problem(model, N, D, q_head, q_tail, seed=19, n_ids=600)
    want = oracle_counts(oracle, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr)
    q_true = table[true_row].clone()
    total = np.zeros_like(want)
    for lo, hi in ((0, 171), (171, N)):
        filt = ops.SegmentFilter(*(t.cuda() for t in seg), lo)
        total += run(ops, model, table[lo:hi].contiguous(), q_fixed, q_rel, q_head, q_true=q_true, filter=filt)
    np.testing.assert_array_equal(total, want)


# ---------------------------------------------------------------------------------------------- workspace
@pytest.mark.parametrize("model,D,q_head,q_tail", [("distmult", 300, 21, 18), ("complex", 768, 64, 0), ("simple", 1024, 33, 32)])
def test_exact_workspace_between_guards(ops, oracle, model, D, q_head, q_tail):
    """A workspace of exactly the advertised bytes and the counts, each between two 64 KiB guards; the scratch pre-filled with
    0x00 / 0xFF / random bytes: the guards stay untouched and the three results equal the oracle's."""
    N, Q = 523, q_head + q_tail
    table, q_fixed, q_rel, true_row = random_problem(model, N, D, q_head, q_tail, seed=41)
    csr = random_csr(Q, N, true_row.numpy(), seed=42)
    want = oracle_counts(oracle, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr)
    need = ops.rank_all_wide_workspace_bytes(model, N, D, q_head, q_tail)
    for fill in (0x00, 0xFF, "random"):
        guard_byte = 0x5A
        bufs = []
        def carve(nbytes):
            buf = torch.full((GUARD + nbytes + GUARD + 256,), guard_byte, dtype=torch.uint8, device="cuda")
            off = GUARD + (-(buf.data_ptr() + GUARD)) % 256
            bufs.append((buf, off, nbytes))
            return buf[off:off + nbytes]
        ws = carve(need)
        if fill == "random":
            ws.copy_(torch.randint(0, 256, (need,), dtype=torch.uint8, generator=torch.Generator().manual_seed(43)).cuda())
        else:
            ws.fill_(fill)
        out = carve(Q * 16)
        out.fill_(0xFF if fill == "random" else fill)
        counts = out.view(torch.int32).view(Q, 4)
        got = run(ops, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr, workspace=ws, out=counts)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got, want)
        for buf, off, nbytes in bufs:
            assert bool((buf[:off] == guard_byte).all()) and bool((buf[off + nbytes:] == guard_byte).all()), (fill, nbytes)


# ---------------------------------------------------------------------------------------------- route
@pytest.mark.parametrize("model,D,wide", [("distmult", 300, True), ("complex", 768, True), ("distmult", 1100, False)])
def test_rank_block_route(ops, oracle, monkeypatch, model, D, wide):
    from blp_amd import models, ranking
    N, q_head, q_tail = 131, 6, 7
    table, q_fixed, q_rel, true_row = random_problem(model, N, D, q_head, q_tail, seed=51)
    csr = random_csr(q_head + q_tail, N, true_row.numpy(), seed=52)
    calls = []
    real = ops.rank_all_wide
    monkeypatch.setattr(ops, "rank_all_wide", lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    got = ranking.rank_block(models.LinkPrediction(D, model, "margin", 3, 0), table.cuda(), q_fixed.cuda(), q_rel.cuda(), q_head, true_row=true_row.cuda(),
                             filt_rowptr=torch.from_numpy(csr[0]).cuda(), filt_col=torch.from_numpy(csr[1]).cuda())
    assert calls == ([model] if wide else [])
    want = oracle_counts(oracle, model, table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_rank_triples_300_wide_distmult_equals_its_cpu_route(ops, monkeypatch):
    """End to end: the dense branch of rank_triples hands its blocks to rank_block, which now takes the new call."""
    from blp_amd import models, ranking, utils
    from test_gpu_shard import _problem
    N, D, T, R = 700, 300, 90, 5
    table, rel_w, ent2idx, triples, edges = _problem("distmult", N, D, T, R, seed=61)
    index = utils.FilterIndex(edges, num_relations=R)
    m = models.LinkPrediction(D, "distmult", "margin", R, 0)
    m.rel_emb.weight.data = rel_w.clone()
    _, want, _ = ranking.rank_triples(m, table, triples, ent2idx, index, block_size=32)
    calls = []
    real = ops.rank_all_wide
    monkeypatch.setattr(ops, "rank_all_wide", lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    _, got, ok = ranking.rank_triples(m.cuda(), table.cuda(), triples.cuda(), ent2idx.cuda(), index, block_size=32)
    assert bool(ok) and len(calls) == 3
    assert (want[:, 0] != want[:, 2]).any()
    np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
