"""Relation prediction for TransE at any width on the MI355X (blp_rank_relations_wide / blp_topk_relations_wide through blp_amd.ops
and ranking).  Everything is compared bit for bit -- counts, relation ids, scores as int32 patterns, NaN positions, empty slots
exactly -1 / 0x7fc00000 -- against the C oracle's score of every expanded (pair, relation) and numpy's stable order (the helpers
of test_rank_relations_host.py / test_gpu_rank_relations.py): widths around the 64-column slab (one partial slab, exactly one, a
slab plus the smallest tail, 300 = 4 slabs + 32 + 8 + 4, 768, 1024), R around the 64-row tile and the 256-row group, Q around the
16-query chunk and beyond 1024 chunks (workgroups stride), the three output forms, filters, -0 / inf / NaN / ties, k around
list_insert's 64-slot groups, the register kernels at 64 / 128 / 256 as a second reference, strided and gathered sources, the
Python route against the dense one, and workspace / output bounds."""
import numpy as np
import pytest
import torch

from test_gpu_rank_relations import check_topk, matrix, problem, segment_filter
from test_gpu_workspace_bounds import guard, three_fills  # noqa: F401  (guard is a fixture)
from test_rank_relations_host import NAN_BITS, make_model, removed_mask, same_scores, same_topk, want_counts, want_topk

pytestmark = pytest.mark.gpu

DEV = "cuda"
M = "transe"
CHUNK = 16            # rank_rels_wide.hip: kWideChunk
MAX_GROUPS = 1024     # rel_common.h: kRelMaxGroups
WIDTHS = (4, 64, 68, 128, 300, 768, 1024)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


def rank(ops, source, head_row, tail_row, rel_w, true_rel=None, **kw):
    t = lambda a: None if a is None else a.to(DEV)
    return ops.rank_relations_wide(M, t(source), t(head_row), t(tail_row), t(rel_w), t(true_rel), **kw)


def topk(ops, source, head_row, tail_row, rel_w, k, **kw):
    t = lambda a: a.to(DEV)
    return ops.topk_relations_wide(M, t(source), t(head_row), t(tail_row), t(rel_w), k, **kw)


def check_all_forms(ops, source, rel_w, hr, tr, true_rel, S, what, ks=(10,)):
    Q, R = S.shape
    none = np.zeros((Q, R), bool)
    want = want_counts(S, true_rel.numpy(), none)
    counts, scores = rank(ops, source, hr, tr, rel_w, true_rel, return_scores=True)
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), want), (what, "both")
    same_scores(scores, S, (what, "both"))
    assert np.array_equal(rank(ops, source, hr, tr, rel_w, true_rel).cpu().numpy(), want), (what, "counts only")
    same_scores(rank(ops, source, hr, tr, rel_w, return_scores=True), S, (what, "scores only"))
    for k in ks:
        check_topk(topk(ops, source, hr, tr, rel_w, k), want_topk(S, none, k), (what, k))


@pytest.mark.parametrize("D", WIDTHS)
def test_widths(ops, oracle, D):
    R, Q = 70, 130
    assert ops.rank_relations_wide_supported(M, D) and ops.topk_relations_wide_supported(M, D, 10)
    source, rel_w, hr, tr, true_rel = problem(200, D, R, Q, seed=D)
    check_all_forms(ops, source, rel_w, hr, tr, true_rel, matrix(oracle, M, source, rel_w, hr, tr), D)


@pytest.mark.parametrize("D", [68, 300])
@pytest.mark.parametrize("R", [1, 11, 64, 65, 237, 257, 822])  # 257: a second group holding one tile
def test_relation_counts(ops, oracle, D, R):
    Q = 20
    source, rel_w, hr, tr, true_rel = problem(100, D, R, Q, seed=D + R)
    check_all_forms(ops, source, rel_w, hr, tr, true_rel, matrix(oracle, M, source, rel_w, hr, tr), (D, R), ks=(5, 65))


def test_query_counts_around_the_chunk(ops, oracle):
    """16 queries per workgroup pass; the top-k kernel min(16, 24 576 / (32 k)): k = 5 -> 16, k = 256 -> 3."""
    D, R = 68, 70
    source, rel_w, hr, tr, true_rel = problem(100, D, R, 2 * CHUNK + 1, seed=5)
    S = matrix(oracle, M, source, rel_w, hr, tr)
    for Q in (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        check_all_forms(ops, source, rel_w, hr[:Q], tr[:Q], true_rel[:Q], S[:Q], Q, ks=(5,))
    for Q in (1, 2, 3, 4, 7):
        check_topk(topk(ops, source, hr[:Q], tr[:Q], rel_w, 256), want_topk(S[:Q], np.zeros((Q, R), bool), 256), (256, Q))


def test_more_chunks_than_workgroups(ops, oracle):
    D, R, Q = 4, 11, MAX_GROUPS * CHUNK + CHUNK + 5
    source, rel_w, hr, tr, true_rel = problem(500, D, R, Q, seed=8)
    S = matrix(oracle, M, source, rel_w, hr, tr)
    check_all_forms(ops, source, rel_w, hr, tr, true_rel, S, Q, ks=(5,))
    few = 3 * MAX_GROUPS + 4  # k = 256: three queries per pass
    check_topk(topk(ops, source, hr[:few], tr[:few], rel_w, 256), want_topk(S[:few], np.zeros((few, R), bool), 256), few)


@pytest.mark.parametrize("D", [68, 300])
def test_score_rows_with_padding_are_left_alone(ops, oracle, D):
    from blp_amd import _lib
    R, Q, pad = 70, 19, 6
    source, rel_w, hr, tr, true_rel = problem(100, D, R, Q, seed=2)
    S = matrix(oracle, M, source, rel_w, hr, tr)
    src, rw, h, t, tru = (x.to(DEV) for x in (source, rel_w, hr, tr, true_rel))
    need = ops.rank_relations_wide_workspace_bytes(M, D, Q, R)
    assert need == 256
    for with_counts in (True, False):
        out = torch.full((Q, R + pad), 12345.0, device=DEV)
        counts = torch.full((Q, 4), -7, dtype=torch.int32, device=DEV)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        status = _lib.lib().blp_rank_relations_wide(0, src.data_ptr(), 100, D, D, h.data_ptr(), t.data_ptr(), Q, rw.data_ptr(), R,
                                                    tru.data_ptr() if with_counts else None, None,
                                                    counts.data_ptr() if with_counts else None, out.data_ptr(), R + pad,
                                                    ws.data_ptr() if with_counts else None, need if with_counts else 0, 0,
                                                    torch.cuda.current_stream().cuda_stream)
        assert status == 0
        torch.cuda.synchronize()
        same_scores(out[:, :R].contiguous(), S)
        assert bool((out[:, R:] == 12345.0).all())
        if with_counts:
            assert np.array_equal(counts.cpu().numpy(), want_counts(S, true_rel.numpy(), np.zeros((Q, R), bool)))
        else:
            assert bool((counts == -7).all())


@pytest.mark.parametrize("D,R", [(300, 237), (68, 11), (768, 300)])
def test_filters(ops, oracle, D, R):
    Q = 20
    source, rel_w, hr, tr, true_rel = problem(300, D, R, Q, seed=R)
    S = matrix(oracle, M, source, rel_w, hr, tr)
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
    segs[17] = np.array([r for r in range(R) if r != true[17]])             # ... in the second chunk too
    for exclude in (true, None):
        ex = true if exclude is not None else np.full(Q, -1)
        removed = removed_mask(segs, ex, Q, R)
        filt = segment_filter(ops, segs, exclude)
        counts = rank(ops, source, hr, tr, rel_w, true_rel, filter=filt)
        assert np.array_equal(counts.cpu().numpy(), want_counts(S, true, removed)), exclude is None
        for k in (1, 5, 65):  # 5, 65 > the relations the filter leaves queries 4 and 5
            check_topk(topk(ops, source, hr, tr, rel_w, k, filter=filt), want_topk(S, removed, k), (k, exclude is None))
    empty = segment_filter(ops, [np.zeros(0, np.int64)] * Q, None)          # empty segments everywhere == no filter
    plain = rank(ops, source, hr, tr, rel_w, true_rel).cpu().numpy()
    assert np.array_equal(rank(ops, source, hr, tr, rel_w, true_rel, filter=empty).cpu().numpy(), plain)
    assert np.array_equal(plain[:, 2:], plain[:, :2])


@pytest.mark.parametrize("D", [68, 300])
def test_ties_nan_inf_and_signed_zero(ops, oracle, D):
    R, Q = 300, 20
    source, rel_w, hr, tr, true_rel = problem(200, D, R, Q, seed=6)
    g = torch.Generator().manual_seed(7)
    copies = torch.randperm(R - 20, generator=g)[:15] + 20  # copies of other relation rows: ties by ascending id
    rel_w[copies] = rel_w[torch.randint(0, 20, (15,), generator=g)]
    rel_w[3, 5], rel_w[4, 0], rel_w[5, D - 1], rel_w[6, 1] = float("nan"), float("inf"), float("-inf"), -0.0
    rel_w[7], rel_w[8] = 0.0, -0.0                           # all-zero rows of either sign
    source[hr[1], 2], source[tr[2], D - 3], source[hr[3], 1] = float("nan"), float("inf"), float("-inf")
    tr[9], tr[18] = hr[9], hr[18]                            # h + 0 - h: every column of relations 7 and 8 is zero
    true_rel[6], true_rel[7], true_rel[8], true_rel[9] = 3, 7, int(copies[0]), 8  # a NaN true score, ..., a tied one, a zero one
    S = matrix(oracle, M, source, rel_w, hr, tr)
    assert np.isnan(S).any() and np.isinf(S).any()
    for q in (9, 18):
        assert (S[q, 7:9].view(np.int32) == np.int32(-2 ** 31)).all()  # the reference's all-zero sum is -0.0
    none = np.zeros((Q, R), bool)
    counts, scores = rank(ops, source, hr, tr, rel_w, true_rel, return_scores=True)
    assert np.array_equal(counts.cpu().numpy(), want_counts(S, true_rel.numpy(), none))
    same_scores(scores, S)
    assert (scores.cpu().numpy()[[9, 18], 7:9].view(np.int32) == np.int32(-2 ** 31)).all()
    for k in (5, 65, 256):
        got = topk(ops, source, hr, tr, rel_w, k)
        check_topk(got, want_topk(S, none, k), k)
    assert got[1][9, 0].cpu().numpy().view(np.int32) == np.int32(-2 ** 31) and int(got[0][9, 0]) == 7  # -0.0 leads, lower id first


@pytest.mark.parametrize("k", [1, 10, 64, 65, 256])
def test_topk_sizes(ops, oracle, k):
    D, Q = 300, 9
    for R in (40, 300):  # k > R among them
        source, rel_w, hr, tr, true_rel = problem(60, D, R, Q, seed=k + R)
        S = matrix(oracle, M, source, rel_w, hr, tr)
        check_topk(topk(ops, source, hr, tr, rel_w, k), want_topk(S, np.zeros((Q, R), bool), k), (k, R))
        rng = np.random.default_rng(k)
        segs = [np.array([r for r in range(R) if r not in rng.choice(R, size=7, replace=False)]) for _ in range(Q)]  # 7 are left
        removed = removed_mask(segs, np.full(Q, -1), Q, R)
        check_topk(topk(ops, source, hr, tr, rel_w, k, filter=segment_filter(ops, segs, None)), want_topk(S, removed, k), (k, R, "filter"))


@pytest.mark.parametrize("D", [64, 128, 256])
def test_wide_kernel_equals_the_register_kernel(ops, D):
    R, Q = 300, 70
    source, rel_w, hr, tr, true_rel = problem(150, D, R, Q, seed=D)
    rel_w[10] = rel_w[2]
    source[hr[4], 3] = float("nan")
    rng = np.random.default_rng(D)
    filt = segment_filter(ops, [rng.choice(R, size=5, replace=False) for _ in range(Q)], true_rel.numpy())
    args = tuple(x.to(DEV) for x in (source, hr, tr, rel_w))
    for f in (None, filt):
        a = ops.rank_relations(M, *args, true_rel.to(DEV), filter=f, return_scores=True)
        b = ops.rank_relations_wide(M, *args, true_rel.to(DEV), filter=f, return_scores=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), (D, f is not None)
        for k in (1, 10, 65):
            a, b = ops.topk_relations(M, *args, k, filter=f), ops.topk_relations_wide(M, *args, k, filter=f)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), (D, k, f is not None)


@pytest.mark.parametrize("D", [68, 300])
def test_strided_source(ops, oracle, D):
    """ld_src > D (a column slice of a wider tensor), and a source that is not a table: the 2 Q query rows gathered."""
    R, Q = 70, 21
    source, rel_w, hr, tr, true_rel = problem(90, D, R, Q, seed=3)
    S = matrix(oracle, M, source, rel_w, hr, tr)
    none = np.zeros((Q, R), bool)
    padded = torch.full((90, D + 12), float("nan"))
    padded[:, :D] = source
    view = padded.to(DEV)[:, :D]
    assert view.stride(0) == D + 12 and not view.is_contiguous()
    gathered = torch.cat((source[hr], source[tr])).to(DEV)
    at = torch.arange(Q)
    for src, h, t in ((view, hr, tr), (gathered, at, at + Q)):
        counts, scores = ops.rank_relations_wide(M, src, h.to(DEV), t.to(DEV), rel_w.to(DEV), true_rel.to(DEV), return_scores=True)
        assert np.array_equal(counts.cpu().numpy(), want_counts(S, true_rel.numpy(), none))
        same_scores(scores, S)
        check_topk(ops.topk_relations_wide(M, src, h.to(DEV), t.to(DEV), rel_w.to(DEV), 10), want_topk(S, none, 10))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("D", [300, 768])
def test_python_route_takes_the_fused_kernel_and_equals_the_dense_route(ops, monkeypatch, D, dtype):
    from blp_amd import ranking, utils
    N, R, T = 120, 30, 40
    g = torch.Generator().manual_seed(12)
    table = torch.randn((N, D), generator=g).to(dtype)
    rel_w = torch.randn((R, D), generator=g)
    entities = torch.randperm(N + 30, generator=g)[:N]
    ent2idx = utils.make_ent2idx(entities, N + 29)
    triples = torch.stack((entities[torch.randint(0, N, (T,), generator=g)], entities[torch.randint(0, N, (T,), generator=g)],
                           torch.randint(0, R, (T,), generator=g)), 1)
    edges = torch.cat((triples, torch.stack((triples[:, 0], triples[:, 1], torch.randint(0, R, (T,), generator=g)), 1)))
    index = utils.RelationFilterIndex(edges)
    cpu, gpu = make_model(M, rel_w.numpy()), make_model(M, rel_w.numpy()).to(DEV)
    assert ops.rank_relations_wide_supported(M, D) and not ops.rank_relations_supported(M, D)
    cases = ((5, triples), (R + 3, triples[:, :2]))
    want = {fi is not None: (ranking.rank_relations(cpu, table, triples, ent2idx, filter_index=fi, return_scores=True),
                             [ranking.predict_relations(cpu, table, pairs, k, ent2idx, filter_index=fi) for k, pairs in cases])
            for fi in (None, index)}
    dense = ranking._relation_scores_dense

    def refuse(*a, **kw):
        raise AssertionError("the dense route was taken")
    monkeypatch.setattr(ranking, "_relation_scores_dense", refuse)
    for fi in (None, index):
        want_rank, want_k = want[fi is not None]
        got = ranking.rank_relations(gpu, table.to(DEV), triples, ent2idx, filter_index=fi, return_scores=True)
        assert np.array_equal(got[0].cpu().numpy(), want_rank[0].numpy())
        same_scores(got[1], want_rank[1].numpy())
        if fi is not None:
            assert bool((want_rank[0][:, 2:] != want_rank[0][:, :2]).any()), "the filter must bite somewhere"
        for (k, pairs), w in zip(cases, want_k):
            same_topk(ranking.predict_relations(gpu, table.to(DEV), pairs, k, ent2idx, filter_index=fi), tuple(x.numpy() for x in w),
                      (k, fi is not None))
    # k > 256 is the dense route's, on the device too
    with pytest.raises(AssertionError, match="dense route"):
        ranking.predict_relations(gpu, table.to(DEV), triples, 300, ent2idx)
    monkeypatch.setattr(ranking, "_relation_scores_dense", dense)
    same_topk(ranking.predict_relations(gpu, table.to(DEV), triples, 300, ent2idx),
              tuple(x.numpy() for x in ranking.predict_relations(cpu, table, triples, 300, ent2idx)))


# ------------------------------------------------------------------------------------------------ workspace and output bounds
@pytest.mark.parametrize("Q", [1, 64, 65])
@pytest.mark.parametrize("D", [68, 300])
def test_workspace_and_output_bounds_rank(ops, oracle, guard, D, Q):
    R = 70
    source, rel_w, hr, tr, true_rel = problem(300, D, R, Q, seed=Q + D)
    S = matrix(oracle, M, source, rel_w, hr, tr)
    rng = np.random.default_rng(Q)
    segs = [rng.choice(R, size=4, replace=False) for _ in range(Q)]
    args = (M, source.cuda(), hr.cuda(), tr.cuda(), rel_w.cuda())
    need = ops.rank_relations_wide_workspace_bytes(M, D, Q, R)
    assert need == (4 * Q + 255) // 256 * 256 == 256 * (1 + (Q > 64))
    for filt, removed in ((None, np.zeros((Q, R), bool)),
                          (segment_filter(ops, segs, true_rel.numpy()), removed_mask(segs, true_rel.numpy(), Q, R))):
        what = (D, Q, filt is not None)
        want = want_counts(S, true_rel.numpy(), removed)
        got, asked = three_fills(guard, lambda g: ops.rank_relations_wide(*args, true_rel.cuda(), filter=filt, return_scores=True,
                                                                          out=g.out((Q, 4), torch.int32)), what)
        assert asked == [need] and np.array_equal(got[0].numpy(), want), what
        same_scores(got[1], S, what)
        got, asked = three_fills(guard, lambda g: ops.rank_relations_wide(*args, true_rel.cuda(), filter=filt,
                                                                          out=g.out((Q, 4), torch.int32)), what)
        assert asked == [need] and np.array_equal(got[0].numpy(), want), what
    got, asked = three_fills(guard, lambda g: ops.rank_relations_wide(*args, return_scores=True), (D, Q, "scores only"))
    assert asked == []  # the scores-only form touches no workspace: none is asked for, NULL is passed
    same_scores(got[0], S, (D, Q, "scores only"))


@pytest.mark.parametrize("D", [68, 300])
def test_workspace_and_output_bounds_topk(ops, oracle, guard, D):
    for Q, R in ((1, 11), (65, 70), (7, 300)):
        source, rel_w, hr, tr, true_rel = problem(300, D, R, Q, seed=Q + R)
        S = matrix(oracle, M, source, rel_w, hr, tr)
        rng = np.random.default_rng(R)
        segs = [rng.choice(R, size=4, replace=False) for _ in range(Q)]
        args = (M, source.cuda(), hr.cuda(), tr.cuda(), rel_w.cuda())
        for k in (1, 10, 256):
            assert ops.topk_relations_wide_workspace_bytes(M, D, Q, R, k) == 0
            for filt, removed in ((None, np.zeros((Q, R), bool)),
                                  (segment_filter(ops, segs, None), removed_mask(segs, np.full(Q, -1), Q, R))):
                what = (D, Q, R, k, filt is not None)
                got, asked = three_fills(guard, lambda g: ops.topk_relations_wide(*args, k, filter=filt,
                                                                                  out=(g.out((Q, k), torch.int64), g.out((Q, k), torch.float32))), what)
                assert all(n == 0 for n in asked), what  # workspace = NULL reaches the library
                same_topk(got, want_topk(S, removed, k), what)
                assert (got[1].numpy().view(np.int32)[got[0].numpy() < 0] == NAN_BITS).all(), what
