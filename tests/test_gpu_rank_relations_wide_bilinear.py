"""Relation prediction for DistMult / ComplEx / SimplE at any width on the MI355X (blp_rank_relations_wide_bilinear /
blp_topk_relations_wide_bilinear through blp_amd.ops and ranking).  Everything is compared bit for bit -- counts, relation ids,
scores as int32 patterns, NaN positions, empty slots exactly -1 / 0x7fc00000 -- against the C oracle's score of every expanded
(pair, relation) and numpy's stable order (the helpers of test_rank_relations_host.py / test_gpu_rank_relations.py): every branch
of the sum order with entries of spread binary exponents, R around a wave's 16 rows and the workgroup's 64-row trip, Q around the
chunk of 8 and beyond the grid cap, the three output forms, k around list_insert's 64-slot groups and beyond R, the LDS extremes
(D = 1024 with k = 256; D = 4), filters, ties / NaN / inf / zeros of either sign, the register kernels at 64 / 128 / 256 as a
second reference, strided and gathered sources, the Python route, workspace / output bounds, and two threads on two streams."""
import threading

import numpy as np
import pytest
import torch

from test_gpu_rank_relations import check_topk, matrix, problem, segment_filter
from test_gpu_workspace_bounds import guard, three_fills  # noqa: F401  (guard is a fixture)
from test_rank_relations_host import NAN_BITS, make_model, removed_mask, same_scores, same_topk, want_counts, want_topk

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODELS = ("distmult", "complex", "simple")
CHUNK = 8             # wide_bilinear.h: kAwQueries
MAX_GROUPS = 1024     # rel_common.h: kRelMaxGroups, the grid cap
NEG0 = np.int32(-2 ** 31)
SUM_ORDER = [("distmult", D) for D in (4, 12, 36, 100, 300, 508, 512, 516, 768, 1024)] + \
            [(m, D) for m in ("complex", "simple") for D in (12, 20, 64, 300, 768, 1000, 1024)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


def spread(x, seed):
    """Every entry gets its own binary exponent over 2^-20 .. 2^20 (spread of test_gpu_rank_sets_wide_bilinear.py): the terms
    of a sum differ by up to 2^120, so any reordering of the additions changes low bits."""
    g = torch.Generator().manual_seed(seed)
    return x * torch.exp2(torch.randint(-20, 21, x.shape, generator=g).float())


def spread_problem(S, D, R, Q, seed):
    source, rel_w, hr, tr, true_rel = problem(S, D, R, Q, seed)
    return spread(source, seed + 1000), spread(rel_w, seed + 2000), hr, tr, true_rel


def rank(ops, model, source, head_row, tail_row, rel_w, true_rel=None, **kw):
    t = lambda a: None if a is None else a.to(DEV)
    return ops.rank_relations_wide_bilinear(model, t(source), t(head_row), t(tail_row), t(rel_w), t(true_rel), **kw)


def topk(ops, model, source, head_row, tail_row, rel_w, k, **kw):
    t = lambda a: a.to(DEV)
    return ops.topk_relations_wide_bilinear(model, t(source), t(head_row), t(tail_row), t(rel_w), k, **kw)


def check_all_forms(ops, model, source, rel_w, hr, tr, true_rel, S, what, ks=(10,)):
    Q, R = S.shape
    none = np.zeros((Q, R), bool)
    want = want_counts(S, true_rel.numpy(), none)
    counts, scores = rank(ops, model, source, hr, tr, rel_w, true_rel, return_scores=True)
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), want), (what, "both")
    same_scores(scores, S, (what, "both"))
    assert np.array_equal(rank(ops, model, source, hr, tr, rel_w, true_rel).cpu().numpy(), want), (what, "counts only")
    same_scores(rank(ops, model, source, hr, tr, rel_w, return_scores=True), S, (what, "scores only"))
    for k in ks:
        check_topk(topk(ops, model, source, hr, tr, rel_w, k), want_topk(S, none, k), (what, k))


@pytest.mark.parametrize("model,D", SUM_ORDER)
def test_every_branch_of_the_sum_order(ops, oracle, model, D):
    """Whole 32-term rows, the cascade from 512 terms on, leftover vectors of 8, the n % 8 tail."""
    R, Q = 70, 19
    assert ops.rank_relations_wide_bilinear_supported(model, D) and ops.topk_relations_wide_bilinear_supported(model, D, 10)
    source, rel_w, hr, tr, true_rel = spread_problem(60, D, R, Q, seed=D)
    check_all_forms(ops, model, source, rel_w, hr, tr, true_rel, matrix(oracle, model, source, rel_w, hr, tr), (model, D))


@pytest.mark.parametrize("R", [1, 11, 15, 16, 17, 63, 64, 65, 237, 257, 822])
@pytest.mark.parametrize("D", [68, 300])
@pytest.mark.parametrize("model", MODELS)
def test_relation_counts_around_the_layout_s_edges(ops, oracle, model, D, R):
    """A wave's 16 rows, the workgroup's 64-row trip, the workloads' own R (237: FB15k-237, 822: Wikidata5M)."""
    Q = 9
    source, rel_w, hr, tr, true_rel = problem(50, D, R, Q, seed=D + R)
    check_all_forms(ops, model, source, rel_w, hr, tr, true_rel, matrix(oracle, model, source, rel_w, hr, tr), (model, D, R), ks=(5, 65))


@pytest.mark.parametrize("model", MODELS)
def test_query_counts_around_the_chunk(ops, oracle, model):
    D, R = 68, 70
    source, rel_w, hr, tr, true_rel = problem(60, D, R, 2 * CHUNK + 1, seed=5)
    S = matrix(oracle, model, source, rel_w, hr, tr)
    for Q in (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        check_all_forms(ops, model, source, rel_w, hr[:Q], tr[:Q], true_rel[:Q], S[:Q], (model, Q), ks=(5, 256))


@pytest.mark.parametrize("model", MODELS)
def test_more_chunks_than_workgroups(ops, oracle, model):
    D, R, Q = 68, 11, CHUNK * MAX_GROUPS + 9
    source, rel_w, hr, tr, true_rel = problem(500, D, R, Q, seed=8)
    check_all_forms(ops, model, source, rel_w, hr, tr, true_rel, matrix(oracle, model, source, rel_w, hr, tr), (model, Q), ks=(5,))


@pytest.mark.parametrize("k", [1, 64, 65, 256])
@pytest.mark.parametrize("model", MODELS)
def test_topk_sizes(ops, oracle, model, k):
    D, Q = 300, 9
    for R in (11, 300):  # k > R among them
        source, rel_w, hr, tr, true_rel = problem(60, D, R, Q, seed=k + R)
        S = matrix(oracle, model, source, rel_w, hr, tr)
        check_topk(topk(ops, model, source, hr, tr, rel_w, k), want_topk(S, np.zeros((Q, R), bool), k), (model, k, R))
        rng = np.random.default_rng(k)
        segs = [np.array([r for r in range(R) if r not in rng.choice(R, size=7, replace=False)]) for _ in range(Q)]  # 7 are left
        removed = removed_mask(segs, np.full(Q, -1), Q, R)
        assert removed.any()
        check_topk(topk(ops, model, source, hr, tr, rel_w, k, filter=segment_filter(ops, segs, None)), want_topk(S, removed, k),
                   (model, k, R, "filter"))


@pytest.mark.parametrize("model,D,k", [(m, 1024, 256) for m in MODELS] + [("distmult", 4, 1)])
def test_lds_extremes(ops, oracle, model, D, k):
    """D = 1024: the coefficients alone are 64 KiB; with k = 256 the lists add 64 KiB.  D = 4, k = 1: the smallest of both (the
    count kernel's 32 counters still fit the coefficient area they reuse)."""
    R, Q = 300, 11
    source, rel_w, hr, tr, true_rel = spread_problem(40, D, R, Q, seed=D + k)
    S = matrix(oracle, model, source, rel_w, hr, tr)
    check_all_forms(ops, model, source, rel_w, hr, tr, true_rel, S, (model, D), ks=(k,))
    rng = np.random.default_rng(D)
    segs = [rng.choice(R, size=4, replace=False) for _ in range(Q)]
    removed = removed_mask(segs, true_rel.numpy(), Q, R)
    filt = segment_filter(ops, segs, true_rel.numpy())
    assert np.array_equal(rank(ops, model, source, hr, tr, rel_w, true_rel, filter=filt).cpu().numpy(), want_counts(S, true_rel.numpy(), removed))
    check_topk(topk(ops, model, source, hr, tr, rel_w, k, filter=filt), want_topk(S, removed, k), (model, D, "filter"))


@pytest.mark.parametrize("D,R", [(300, 237), (68, 11), (768, 300)])
@pytest.mark.parametrize("model", MODELS)
def test_filters(ops, oracle, model, D, R):
    Q = 20
    source, rel_w, hr, tr, true_rel = problem(300, D, R, Q, seed=R)
    S = matrix(oracle, model, source, rel_w, hr, tr)
    true = true_rel.numpy()
    rng = np.random.default_rng(R)
    segs = [rng.choice(R, size=int(rng.integers(1, 5)), replace=False) for _ in range(Q)]  # 1 - 4 relations
    segs[0] = np.zeros(0, np.int64)                                         # an empty segment
    segs[1] = np.array([r for r in range(R) if r != true[1]])               # every relation but the true one
    segs[2] = np.array([R, R + 7, 1 << 40, -1, 2])                          # ids that are no relation are ignored
    segs[3] = np.array([true[3], (true[3] + 1) % R])                        # names the true relation: exclude keeps it
    segs[4] = np.arange(R)                                                  # everything named: only exclude survives
    keep3 = rng.choice(R, size=3, replace=False)
    segs[5] = np.array([r for r in range(R) if r not in keep3])             # a query left with 3 relations: fewer than k
    segs[17] = np.array([r for r in range(R) if r != true[17]])             # ... in the third chunk too
    for exclude in (true, None):
        ex = true if exclude is not None else np.full(Q, -1)
        removed = removed_mask(segs, ex, Q, R)
        filt = segment_filter(ops, segs, exclude)
        want = want_counts(S, true, removed)
        assert (want[:, 2:] != want[:, :2]).any(), "the filter must bite"
        counts = rank(ops, model, source, hr, tr, rel_w, true_rel, filter=filt)
        assert np.array_equal(counts.cpu().numpy(), want), (model, exclude is None)
        both = rank(ops, model, source, hr, tr, rel_w, true_rel, filter=filt, return_scores=True)
        assert np.array_equal(both[0].cpu().numpy(), want), (model, exclude is None, "with scores")
        same_scores(both[1], S)                                             # the filter removes nothing from the score matrix
        for k in (1, 5, 65):  # 5, 65 > the relations the filter leaves queries 4 and 5
            wk = want_topk(S, removed, k)
            assert k == 1 or (wk[0] < 0).any()
            assert not np.array_equal(wk[0], want_topk(S, np.zeros((Q, R), bool), k)[0]), "the filter must bite"
            check_topk(topk(ops, model, source, hr, tr, rel_w, k, filter=filt), wk, (model, k, exclude is None))
    empty = segment_filter(ops, [np.zeros(0, np.int64)] * Q, None)          # empty segments everywhere == no filter
    plain = rank(ops, model, source, hr, tr, rel_w, true_rel).cpu().numpy()
    assert np.array_equal(rank(ops, model, source, hr, tr, rel_w, true_rel, filter=empty).cpu().numpy(), plain)
    assert np.array_equal(plain[:, 2:], plain[:, :2])


@pytest.mark.parametrize("D", [68, 300])
@pytest.mark.parametrize("model", MODELS)
def test_ties_nan_inf_and_zero_rows(ops, oracle, model, D):
    R, Q = 300, 20
    source, rel_w, hr, tr, true_rel = problem(200, D, R, Q, seed=6)
    g = torch.Generator().manual_seed(7)
    copies = torch.randperm(R - 20, generator=g)[:15] + 20  # copies of other relation rows: ties by ascending id
    rel_w[copies] = rel_w[torch.randint(0, 20, (15,), generator=g)]
    # NaN / +inf / -inf in the first and in the last four columns
    rel_w[3, 1], rel_w[4, 0], rel_w[5, 2] = float("nan"), float("inf"), float("-inf")
    rel_w[9, D - 1], rel_w[10, D - 4], rel_w[11, D - 2] = float("nan"), float("inf"), float("-inf")
    rel_w[6, 1] = -0.0
    rel_w[7], rel_w[8] = 0.0, -0.0                          # all-zero rows of either sign
    source[hr[1], 2], source[tr[2], D - 3], source[hr[3], 1] = float("nan"), float("inf"), float("-inf")
    true_rel[6], true_rel[7], true_rel[8], true_rel[9] = 3, 7, int(copies[0]), 8  # a NaN true score, a zero one, a tied one ...
    S = matrix(oracle, model, source, rel_w, hr, tr)
    assert np.isnan(S).any() and np.isinf(S).any()
    finite = [q for q in range(Q) if bool(torch.isfinite(source[hr[q]]).all()) and bool(torch.isfinite(source[tr[q]]).all())]
    assert len(finite) >= 10
    assert (S[finite, 7].view(np.int32) == 0).all()         # an all-zero relation row scores +0: the sum starts from +0
    none = np.zeros((Q, R), bool)
    counts, scores = rank(ops, model, source, hr, tr, rel_w, true_rel, return_scores=True)
    assert np.array_equal(counts.cpu().numpy(), want_counts(S, true_rel.numpy(), none))
    same_scores(scores, S)
    assert (scores.cpu().numpy()[finite][:, 7:9].view(np.int32) == S[finite][:, 7:9].view(np.int32)).all()
    for k in (5, 65, 256):
        check_topk(topk(ops, model, source, hr, tr, rel_w, k), want_topk(S, none, k), (model, k))


@pytest.mark.parametrize("D", [4, 68])
def test_simple_s_halved_underflow_is_minus_zero(ops, oracle, D):
    """SimplE's final s / 2 with s = -2^-149, the smallest negative number: the quotient rounds to -0.  The reference's own
    last operation, done by the kernel on the same s; the key of the top-k lists carries the sign."""
    R, Q, H = 20, 9, D // 2
    source, rel_w, hr, tr, true_rel = problem(40, D, R, Q, seed=3)
    hr[2], tr[2], true_rel[2] = 5, 6, 4
    hr[:2], tr[:2], hr[3:], tr[3:] = hr[:2] % 5, tr[:2] % 5, 7 + hr[3:] % 30, 7 + tr[3:] % 30  # rows 5 and 6: query 2 only
    source[5], source[6], rel_w[4] = 0.0, 0.0, 0.0
    source[5, 0], rel_w[4, 0], source[6, H] = 2.0 ** -50, -(2.0 ** -50), 2.0 ** -49  # (hh * ra) * tt = -2^-149; th, rb, ht = 0
    S = matrix(oracle, "simple", source, rel_w, hr, tr)
    assert S[2, 4].view(np.int32) == NEG0, "the oracle's -0"
    none = np.zeros((Q, R), bool)
    counts, scores = rank(ops, "simple", source, hr, tr, rel_w, true_rel, return_scores=True)
    assert scores.cpu().numpy()[2, 4].view(np.int32) == NEG0
    same_scores(scores, S)
    assert np.array_equal(counts.cpu().numpy(), want_counts(S, true_rel.numpy(), none))
    got = topk(ops, "simple", source, hr, tr, rel_w, R)
    check_topk(got, want_topk(S, none, R))
    at = (got[0][2] == 4).nonzero()[0, 0]
    assert got[1][2, at].cpu().numpy().view(np.int32) == NEG0


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("model", MODELS)
def test_wide_kernel_equals_the_register_kernel(ops, model, D):
    R, Q = 300, 70
    source, rel_w, hr, tr, true_rel = problem(150, D, R, Q, seed=D)
    rel_w[10] = rel_w[2]
    source[hr[4], 3] = float("nan")
    rng = np.random.default_rng(D)
    filt = segment_filter(ops, [rng.choice(R, size=5, replace=False) for _ in range(Q)], true_rel.numpy())
    args = tuple(x.to(DEV) for x in (source, hr, tr, rel_w))
    for f in (None, filt):
        a = ops.rank_relations(model, *args, true_rel.to(DEV), filter=f, return_scores=True)
        b = ops.rank_relations_wide_bilinear(model, *args, true_rel.to(DEV), filter=f, return_scores=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), (model, D, f is not None)
        for k in (1, 10, 65):
            a, b = ops.topk_relations(model, *args, k, filter=f), ops.topk_relations_wide_bilinear(model, *args, k, filter=f)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), (model, D, k, f is not None)


@pytest.mark.parametrize("D", [68, 300])
@pytest.mark.parametrize("model", MODELS)
def test_strided_and_gathered_sources(ops, oracle, model, D):
    """ld_src > D (a column slice of a wider tensor), a source that is not a table (the 2 Q query rows gathered), and pairs
    whose head is their tail."""
    R, Q = 70, 21
    source, rel_w, hr, tr, true_rel = problem(90, D, R, Q, seed=3)
    tr[4], tr[13] = hr[4], hr[13]  # head_row == tail_row
    S = matrix(oracle, model, source, rel_w, hr, tr)
    none = np.zeros((Q, R), bool)
    padded = torch.full((90, D + 12), float("nan"))
    padded[:, :D] = source
    view = padded.to(DEV)[:, :D]
    assert view.stride(0) == D + 12 and not view.is_contiguous()
    gathered = torch.cat((source[hr], source[tr])).to(DEV)
    at = torch.arange(Q)
    for src, h, t in ((view, hr, tr), (gathered, at, at + Q)):
        counts, scores = ops.rank_relations_wide_bilinear(model, src, h.to(DEV), t.to(DEV), rel_w.to(DEV), true_rel.to(DEV), return_scores=True)
        assert np.array_equal(counts.cpu().numpy(), want_counts(S, true_rel.numpy(), none))
        same_scores(scores, S)
        check_topk(ops.topk_relations_wide_bilinear(model, src, h.to(DEV), t.to(DEV), rel_w.to(DEV), 10), want_topk(S, none, 10))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("D", [300, 768])
@pytest.mark.parametrize("model", MODELS)
def test_python_route_takes_the_fused_kernel_and_equals_the_cpu_route(ops, monkeypatch, model, D, dtype):
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
    cpu, gpu = make_model(model, rel_w.numpy()), make_model(model, rel_w.numpy()).to(DEV)
    assert ops.rank_relations_wide_bilinear_supported(model, D) and not ops.rank_relations_supported(model, D)
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
        assert np.array_equal(ranking.rank_relations(gpu, table.to(DEV), triples, ent2idx, filter_index=fi).cpu().numpy(), want_rank[0].numpy())
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
@pytest.mark.parametrize("D", [68, 300])
@pytest.mark.parametrize("model", MODELS)
def test_score_rows_with_padding_are_left_alone(ops, oracle, model, D):
    from blp_amd import _lib
    R, Q, pad = 70, 19, 6
    source, rel_w, hr, tr, true_rel = problem(100, D, R, Q, seed=2)
    S = matrix(oracle, model, source, rel_w, hr, tr)
    src, rw, h, t, tru = (x.to(DEV) for x in (source, rel_w, hr, tr, true_rel))
    need = ops.rank_relations_wide_bilinear_workspace_bytes(model, D, Q, R)
    assert need == 256
    for with_counts in (True, False):
        out = torch.full((Q, R + pad), 12345.0, device=DEV)
        counts = torch.full((Q, 4), -7, dtype=torch.int32, device=DEV)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        status = _lib.lib().blp_rank_relations_wide_bilinear(_lib.MODEL_IDS[model], src.data_ptr(), 100, D, D, h.data_ptr(), t.data_ptr(), Q,
                                                             rw.data_ptr(), R, tru.data_ptr() if with_counts else None, None,
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


@pytest.mark.parametrize("Q", [1, 64, 65])
@pytest.mark.parametrize("model,D", [("distmult", 68), ("complex", 300), ("simple", 68)])
def test_workspace_and_output_bounds_rank(ops, oracle, guard, model, D, Q):
    R = 70
    source, rel_w, hr, tr, true_rel = problem(300, D, R, Q, seed=Q + D)
    S = matrix(oracle, model, source, rel_w, hr, tr)
    rng = np.random.default_rng(Q)
    segs = [rng.choice(R, size=4, replace=False) for _ in range(Q)]
    args = (model, source.cuda(), hr.cuda(), tr.cuda(), rel_w.cuda())
    need = ops.rank_relations_wide_bilinear_workspace_bytes(model, D, Q, R)
    assert need == (4 * Q + 255) // 256 * 256 == 256 * (1 + (Q > 64))
    for filt, removed in ((None, np.zeros((Q, R), bool)),
                          (segment_filter(ops, segs, true_rel.numpy()), removed_mask(segs, true_rel.numpy(), Q, R))):
        what = (model, D, Q, filt is not None)
        want = want_counts(S, true_rel.numpy(), removed)
        got, asked = three_fills(guard, lambda g: ops.rank_relations_wide_bilinear(*args, true_rel.cuda(), filter=filt, return_scores=True,
                                                                                   out=g.out((Q, 4), torch.int32)), what)
        assert asked == [need] and np.array_equal(got[0].numpy(), want), what  # a workspace of exactly the advertised size
        same_scores(got[1], S, what)
        got, asked = three_fills(guard, lambda g: ops.rank_relations_wide_bilinear(*args, true_rel.cuda(), filter=filt,
                                                                                   out=g.out((Q, 4), torch.int32)), what)
        assert asked == [need] and np.array_equal(got[0].numpy(), want), what
    got, asked = three_fills(guard, lambda g: ops.rank_relations_wide_bilinear(*args, return_scores=True), (model, D, Q, "scores only"))
    assert asked == []  # the scores-only form touches no workspace: none is asked for, NULL is passed
    same_scores(got[0], S, (model, D, Q, "scores only"))


@pytest.mark.parametrize("model,D", [("distmult", 300), ("complex", 68), ("simple", 300)])
def test_workspace_and_output_bounds_topk(ops, oracle, guard, model, D):
    for Q, R in ((1, 11), (65, 70), (7, 300)):
        source, rel_w, hr, tr, true_rel = problem(300, D, R, Q, seed=Q + R)
        S = matrix(oracle, model, source, rel_w, hr, tr)
        rng = np.random.default_rng(R)
        segs = [rng.choice(R, size=4, replace=False) for _ in range(Q)]
        args = (model, source.cuda(), hr.cuda(), tr.cuda(), rel_w.cuda())
        for k in (1, 10, 256):
            assert ops.topk_relations_wide_bilinear_workspace_bytes(model, D, Q, R, k) == 0
            for filt, removed in ((None, np.zeros((Q, R), bool)),
                                  (segment_filter(ops, segs, None), removed_mask(segs, np.full(Q, -1), Q, R))):
                what = (model, D, Q, R, k, filt is not None)
                got, asked = three_fills(guard, lambda g: ops.topk_relations_wide_bilinear(
                    *args, k, filter=filt, out=(g.out((Q, k), torch.int64), g.out((Q, k), torch.float32))), what)
                assert all(n == 0 for n in asked), what  # workspace = NULL, 0 bytes, reaches the library
                same_topk(got, want_topk(S, removed, k), what)
                assert (got[1].numpy().view(np.int32)[got[0].numpy() < 0] == NAN_BITS).all(), what


def test_two_threads_on_two_streams(ops, oracle):
    jobs = []
    for i, (model, D, R) in enumerate((("distmult", 300, 237), ("complex", 768, 822))):
        source, rel_w, hr, tr, true_rel = problem(400, D, R, 100, seed=20 + i)
        S = matrix(oracle, model, source, rel_w, hr, tr)
        jobs.append(dict(model=model, args=[x.to(DEV) for x in (source, hr, tr, rel_w)], true=true_rel, S=S, out=None))
    torch.cuda.synchronize()

    def work(job):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            for _ in range(3):
                counts = ops.rank_relations_wide_bilinear(job["model"], *job["args"], job["true"].to(DEV))
                top = ops.topk_relations_wide_bilinear(job["model"], *job["args"], 10)
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
