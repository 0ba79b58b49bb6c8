"""Per-query candidate lists without a GPU (include/blp_hip.h: blp_rank_lists_supported, blp_rank_lists_workspace_bytes,
blp_rank_lists; ranking.rank_candidates): the entry points are exported and bound, which (model, dtype, D) they take, the
workspace bound, the argument refusals (checked before anything touches a device), no scratch memory in the new kernels, and
the CPU route of rank_candidates -- the oracle of the fused one -- against the C oracle on the toy goldens."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden
from blp_amd import _lib, models, ranking, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_rank_lists_supported", "blp_rank_lists_workspace_bytes", "blp_rank_lists")
F32, F16, BF16 = 0, 1, 2
SIDE_HEAD, SIDE_TAIL = 0, 1


def _L():
    return _lib.lib()


def test_new_entry_points_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "blp_hip.h")).read()
    L = _L()
    for name in NEW:
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert getattr(L, name).argtypes is not None
    from blp_amd import ops
    assert callable(ops.rank_lists) and callable(ops.rank_lists_supported)
    assert callable(ranking.rank_candidates) and callable(ranking.sample_candidates)


def test_supported_grid():
    L = _L()
    for dt in (F32, F16, BF16):
        for D in (4, 64, 100, 128, 256, 300, 768, 1024):
            assert L.blp_rank_lists_supported(0, dt, D), (dt, D)
        for D in (0, -4, 2, 126, 1028, 2048):
            assert not L.blp_rank_lists_supported(0, dt, D), (dt, D)
        for m in (1, 2, 3):
            for D in (64, 128, 256):
                assert L.blp_rank_lists_supported(m, dt, D)
            for D in (32, 96, 300, 512, 768):
                assert not L.blp_rank_lists_supported(m, dt, D)
        assert not L.blp_rank_lists_supported(4, dt, 128) and not L.blp_rank_lists_supported(-1, dt, 128)
    for dt in (3, -1):
        assert not L.blp_rank_lists_supported(0, dt, 128)
    from blp_amd import ops
    assert ops.rank_lists_supported("transe", 300, torch.float16) and not ops.rank_lists_supported("complex", 300)
    assert not ops.rank_lists_supported("transe", 128, torch.float64)


def test_workspace_is_a_small_multiple_of_Q():
    """The entry takes neither N nor nnz: the workspace cannot depend on them.  4 bytes per query, rounded up to 256."""
    L = _L()
    for dt in (F32, F16, BF16):
        for m, D in ((0, 128), (0, 768), (2, 256)):
            for qh, qt in ((0, 0), (1, 0), (2, 2), (6894, 6894), (52870, 52870)):
                n = L.blp_rank_lists_workspace_bytes(m, dt, D, qh, qt)
                assert 4 * (qh + qt) <= n <= 4 * (qh + qt) + 256 and n % 256 == 0
    assert L.blp_rank_lists_workspace_bytes(1, F32, 300, 2, 2) == 0
    assert L.blp_rank_lists_workspace_bytes(0, 3, 128, 2, 2) == 0
    assert L.blp_rank_lists_workspace_bytes(0, F32, 128, -1, 2) == 0


def _call(L, **over):
    """blp_rank_lists with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(model=0, table=1 << 20, dtype=F32, N=1000, D=128, ld=128, row_base=0, source=1 << 21, S=1000, ld_src=128,
             fixed_row=1 << 22, rel_emb=1 << 23, R=5, rel_id=1 << 24, true_row=1 << 25, q_head=2, q_tail=2, list_ptr=1 << 26,
             list_row=1 << 27, nnz=100, filter=None, counts=1 << 28, scores=1 << 29, workspace=1 << 30, ws=1 << 20, device=0,
             stream=None)
    a.update(over)
    f = a["filter"]
    return L.blp_rank_lists(a["model"], a["table"], a["dtype"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"],
                            a["ld_src"], a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["true_row"], a["q_head"], a["q_tail"],
                            a["list_ptr"], a["list_row"], a["nnz"], None if f is None else ctypes.byref(f), a["counts"],
                            a["scores"], a["workspace"], a["ws"], a["device"], a["stream"])


def test_bad_arguments():
    L = _L()
    assert _call(L, counts=None, scores=None, true_row=None) == -1 and b"both outputs NULL" in L.blp_last_error()
    assert _call(L, true_row=None) == -1 and b"true_row" in L.blp_last_error()  # counts without true_row
    filt = _lib.BlpFilter(1 << 31, 1 << 32, 1 << 33, None, None, 0, 100)
    assert _call(L, filter=filt) == -1 and b"row_base" in L.blp_last_error()
    assert _call(L, dtype=3) == -1 and b"dtype 3" in L.blp_last_error()
    assert _call(L, dtype=-1) == -1
    assert _call(L, nnz=1 << 31) == -1 and b"nnz" in L.blp_last_error()
    assert _call(L, nnz=-1) == -1
    # the conventions shared with blp_topk_typed
    assert _call(L, model=7) == -1
    assert _call(L, model=1, D=300, ld=300, ld_src=300) == -2
    assert _call(L, D=302, ld=302, ld_src=302) == -2
    assert _call(L, dtype=F16, ld=132) == -1 and b"ld % 8" in L.blp_last_error()
    assert _call(L, table=(1 << 20) + 8) == -1
    assert _call(L, ld=64) == -1
    assert _call(L, source=None) == -1
    assert _call(L, list_ptr=None) == -1
    assert _call(L, list_row=None) == -1
    assert _call(L, row_base=(1 << 31) - 10) == -1
    assert _call(L, workspace=None) == -4
    assert _call(L, ws=1) == -4
    assert _call(L, workspace=(1 << 30) + 64) == -4


def test_rank_lists_kernels_use_no_scratch():
    from blp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = kernel_resources.kernels_of(os.path.join(build.OBJ, "rank_lists.hip.o"))
    # TransE at a run-time width + three models x three widths, each over three storage types; the true keys: 1 + 9
    assert len([k for k in kernels if "rank_lists_kernel" in k]) == 3 * (1 + 9)
    assert len([k for k in kernels if "lists_true_key" in k]) == 1 + 9
    assert len(kernels) == 40
    assert all(v["private_segment_fixed_size"] == 0 for v in kernels.values()), [k for k, v in kernels.items() if v["private_segment_fixed_size"]]


# ------------------------------------------------------------------------------------------- rank_candidates on CPU tensors
def _model(rel_model, rel_w):
    m = models.LinkPrediction(rel_w.shape[1], rel_model, "margin", rel_w.shape[0], 0)
    with torch.no_grad():
        m.rel_emb.weight.copy_(torch.from_numpy(rel_w))
    return m


@pytest.fixture(scope="module", params=REL_MODELS)
def toy(request, oracle):
    """The toy evaluation: table, triples, filter -- and the oracle's (2 T, N) score matrix and true scores, computed once."""
    rel_model = request.param
    g, f = golden(f"eval_toy_{rel_model}"), golden("filters_toy")
    table, rel_w, triples, ent2idx = g["ent_emb"], g["rel_w"], f["triples"], f["ent2idx"]
    h_row, t_row, r = ent2idx[triples[:, 0]], ent2idx[triples[:, 1]], triples[:, 2]
    pred = np.concatenate((oracle.score_all(rel_model, SIDE_HEAD, table, table[t_row], rel_w[r]),
                           oracle.score_all(rel_model, SIDE_TAIL, table, table[h_row], rel_w[r])))
    true_row = np.concatenate((h_row, t_row))
    masks = np.concatenate((f["heads_filter"], f["tails_filter"]))
    return dict(rel_model=rel_model, model=_model(rel_model, rel_w), table=torch.from_numpy(table), triples=torch.from_numpy(triples),
                ent2idx=torch.from_numpy(ent2idx), index=utils.FilterIndex(torch.from_numpy(f["graph_edges"])), pred=pred,
                true=pred[np.arange(len(true_row)), true_row], true_row=true_row, masks=masks, entities=f["entities"],
                t_row=t_row, h_row=h_row, rel=r, rel_w=rel_w)


def counts_of(pred, true, masks, lists):
    """{gt, ge, gt_filt, ge_filt} of each query's list (rows; < 0 or >= N skipped) read off the oracle's score matrix."""
    out = np.zeros((len(lists), 4), np.int32)
    N = pred.shape[1]
    for q, rows in enumerate(lists):
        rows = np.asarray([x for x in rows if 0 <= x < N], np.int64)
        s, keep = pred[q, rows], ~masks[q, rows]
        out[q] = ((s > true[q]).sum(), (s >= true[q]).sum(), ((s > true[q]) & keep).sum(), ((s >= true[q]) & keep).sum())
    return out


def test_full_lists_reproduce_the_oracle_rank_counts(toy, oracle):
    N, Q = toy["table"].shape[0], 2 * toy["triples"].shape[0]
    T = Q // 2
    table, rel_w = toy["table"].numpy(), toy["rel_w"]
    want = []
    for side, fixed, sl in ((SIDE_HEAD, toy["t_row"], slice(0, T)), (SIDE_TAIL, toy["h_row"], slice(T, Q))):
        m = toy["masks"][sl]
        rowptr = np.concatenate(([0], np.cumsum(m.sum(1)))).astype(np.int64)
        want.append(oracle.rank_counts(toy["rel_model"], side, table, table[fixed], rel_w[toy["rel"]], true_row=toy["true_row"][sl],
                                       filt_rowptr=rowptr, filt_col=np.nonzero(m)[1].astype(np.int64)))
    want = np.concatenate(want)
    every = torch.arange(N).expand(Q, N)
    got = ranking.rank_candidates(toy["model"], toy["table"], toy["triples"], every, toy["ent2idx"], filter_index=toy["index"])
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    raw = ranking.rank_candidates(toy["model"], toy["table"], toy["triples"], every, toy["ent2idx"])
    assert np.array_equal(raw.numpy()[:, :2], want[:, :2]) and np.array_equal(raw.numpy()[:, 2:], want[:, :2])
    for side, sl in (("head", slice(0, T)), ("tail", slice(T, Q))):
        one = ranking.rank_candidates(toy["model"], toy["table"], toy["triples"], every[sl], toy["ent2idx"], side=side,
                                      filter_index=toy["index"])
        assert np.array_equal(one.numpy(), want[sl])


def test_sublists_with_duplicates_and_padding(toy):
    N, Q = toy["table"].shape[0], 2 * toy["triples"].shape[0]
    rng = np.random.default_rng(5)
    cand = rng.integers(0, N, (Q, 37))
    cand[:, 20:30] = cand[:, 5:15]               # duplicates
    cand[rng.random((Q, 37)) < 0.2] = -1           # padding anywhere
    cand[3] = -1                                   # an empty list
    want = counts_of(toy["pred"], toy["true"], toy["masks"], cand)
    args = (toy["model"], toy["table"], toy["triples"])
    got, scores = ranking.rank_candidates(*args, torch.from_numpy(cand), toy["ent2idx"], filter_index=toy["index"], return_scores=True)
    assert np.array_equal(got.numpy(), want)
    assert want[:, 1].max() > 0 and (want[:, 3] < want[:, 1]).any(), "the filter must bite somewhere"
    ref = np.where(cand >= 0, np.take_along_axis(toy["pred"], np.maximum(cand, 0), axis=1), np.float32(np.nan))
    assert scores.shape == cand.shape and np.array_equal(np.isnan(scores.numpy()), cand < 0)
    assert np.array_equal(scores.numpy()[cand >= 0].view(np.int32), ref[cand >= 0].view(np.int32))
    # the same lists as a CSR without the padding
    lists = [row[row >= 0] for row in cand]
    ptr = torch.from_numpy(np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int64))
    flat = torch.from_numpy(np.concatenate(lists))
    got2, s2 = ranking.rank_candidates(*args, (ptr, flat), toy["ent2idx"], filter_index=toy["index"], return_scores=True)
    assert np.array_equal(got2.numpy(), want) and s2.shape == flat.shape
    assert np.array_equal(s2.numpy().view(np.int32), ref[cand >= 0].view(np.int32))
    # negatives only: the true entity's tie with itself is added to the two `ge` columns, nothing else moves
    neg = ranking.rank_candidates(*args, torch.from_numpy(cand), toy["ent2idx"], filter_index=toy["index"], include_true=False)
    assert np.array_equal(neg.numpy(), want + np.array([0, 1, 0, 1], np.int32))


def test_candidates_as_entity_ids(toy):
    N, Q = toy["table"].shape[0], 2 * toy["triples"].shape[0]
    ent2idx = toy["ent2idx"].numpy()
    assert (ent2idx < 0).any()
    rng = np.random.default_rng(6)
    ids = rng.integers(-1, len(ent2idx) + 3, (Q, 41))  # ids without a row, out of range and -1 among them
    rows = np.where((ids >= 0) & (ids < len(ent2idx)), ent2idx[np.clip(ids, 0, len(ent2idx) - 1)], -1)
    assert (rows < 0).any() and (rows >= 0).any()
    want = counts_of(toy["pred"], toy["true"], toy["masks"], rows)
    got = ranking.rank_candidates(toy["model"], toy["table"], toy["triples"], torch.from_numpy(ids), toy["ent2idx"],
                                  filter_index=toy["index"], candidates_are="ids")
    assert np.array_equal(got.numpy(), want)


def test_sample_candidates_is_deterministic():
    a = ranking.sample_candidates(7, 1000, 50, generator=torch.Generator().manual_seed(3))
    b = ranking.sample_candidates(7, 1000, 50, generator=torch.Generator().manual_seed(3))
    assert a.shape == (7, 50) and a.dtype == torch.int64 and torch.equal(a, b)
    assert int(a.min()) >= 0 and int(a.max()) < 1000


def test_rank_candidates_argument_errors(toy):
    args = (toy["model"], toy["table"], toy["triples"])
    cand = torch.zeros((2 * toy["triples"].shape[0], 3), dtype=torch.long)
    with pytest.raises(ValueError):
        ranking.rank_candidates(*args, cand, toy["ent2idx"], side="middle")
    with pytest.raises(ValueError):
        ranking.rank_candidates(*args, cand, toy["ent2idx"], candidates_are="names")
    with pytest.raises(ValueError):
        ranking.rank_candidates(*args, cand[:5], toy["ent2idx"])
