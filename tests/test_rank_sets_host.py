"""Candidate sets shared between queries, without a GPU (include/blp_hip.h: blp_rank_sets_supported,
blp_rank_sets_workspace_bytes, blp_rank_sets; ranking.CandidateSets, relation_candidate_sets, rank_in_sets): the entry points
are exported and bound, which (model, D) they take, the workspace bound, the argument refusals (checked before anything
touches a device), no scratch memory in the new kernels, and the CPU route of rank_in_sets -- the oracle of the fused one --
against rank_candidates on the expanded per-query lists and against rank_block on the full table."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden
from blp_amd import _lib, models, ranking, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_rank_sets_supported", "blp_rank_sets_workspace_bytes", "blp_rank_sets")


def _L():
    return _lib.lib()


def test_new_entry_points_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "blp_hip.h")).read()
    L = _L()
    for name in NEW:
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert getattr(L, name).argtypes is not None
    assert L.blp_version() == 60000
    from blp_amd import ops
    assert callable(ops.rank_sets) and callable(ops.rank_sets_supported) and callable(ops.rank_sets_workspace_bytes)
    assert callable(ranking.rank_in_sets) and callable(ranking.relation_candidate_sets)
    assert "rank_sets_grid" in _lib.KNOBS
    assert not hasattr(L, "blp_debug_set_knob")  # the product library exports no hook


def test_supported_grid():
    L = _L()
    for m in range(4):
        for D in (64, 128, 256):
            assert L.blp_rank_sets_supported(m, D), (m, D)
        for D in (0, -64, 4, 32, 96, 100, 300, 512, 768, 1024):
            assert not L.blp_rank_sets_supported(m, D), (m, D)
    assert not L.blp_rank_sets_supported(4, 128) and not L.blp_rank_sets_supported(-1, 128)
    from blp_amd import ops
    assert ops.rank_sets_supported("complex", 256) and not ops.rank_sets_supported("transe", 300)


def test_workspace_is_monotone_and_aligned():
    """True keys, accumulators, coefficient rows (2 D floats per query) and G + 1 unit offsets: grows with Q and with G, never
    with N or nnz (the entry takes neither), 256-byte aligned."""
    L = _L()
    for m, D in ((0, 64), (1, 128), (2, 256), (3, 128)):
        last = 0
        for qh, qt in ((0, 1), (1, 1), (2, 2), (100, 3), (6894, 6894), (52870, 52870)):
            n = L.blp_rank_sets_workspace_bytes(m, D, qh, qt, 474)
            assert n % 256 == 0 and n >= (qh + qt) * (4 + 8 + 8 * D) + 475 * 8 and n > last
            assert n <= (qh + qt) * (4 + 8 + 8 * D) + 475 * 8 + 5 * 256
            last = n
        sizes = [L.blp_rank_sets_workspace_bytes(m, D, 300, 300, G) for G in (1, 12, 474, 1644, 100000)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0] and all(s % 256 == 0 for s in sizes)
    assert L.blp_rank_sets_workspace_bytes(1, 300, 2, 2, 5) == 0
    assert L.blp_rank_sets_workspace_bytes(7, 128, 2, 2, 5) == 0
    assert L.blp_rank_sets_workspace_bytes(0, 128, -1, 2, 5) == 0
    assert L.blp_rank_sets_workspace_bytes(0, 128, 2, 2, -1) == 0


def _call(L, **over):
    """blp_rank_sets with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(model=0, table=1 << 20, N=1000, D=128, ld=128, row_base=0, source=1 << 21, S=1000, ld_src=128, fixed_row=1 << 22,
             rel_emb=1 << 23, R=5, rel_id=1 << 24, true_row=1 << 25, q_head=2, q_tail=2, set_ptr=1 << 26, set_row=1 << 27, nnz=100,
             G=3, qh=1 << 28, qt=1 << 29, filter=None, counts=1 << 30, workspace=1 << 31, ws=1 << 20, device=0, stream=None)
    a.update(over)
    f = a["filter"]
    return L.blp_rank_sets(a["model"], a["table"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"], a["ld_src"],
                           a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["true_row"], a["q_head"], a["q_tail"], a["set_ptr"],
                           a["set_row"], a["nnz"], a["G"], a["qh"], a["qt"], None if f is None else ctypes.byref(f), a["counts"],
                           a["workspace"], a["ws"], a["device"], a["stream"])


def test_bad_arguments():
    L = _L()
    assert _call(L, model=7) == -1 and b"unknown model" in L.blp_last_error()
    assert _call(L, model=-1) == -1
    for D in (300, 100, 32, 0, -128):
        assert _call(L, D=D, ld=max(D, 4), ld_src=max(D, 4)) == -2 and b"not supported" in L.blp_last_error()
    for name in ("N", "q_head", "q_tail", "nnz", "G", "row_base"):
        assert _call(L, **{name: -1}) == -1 and b"negative" in L.blp_last_error(), name
    assert _call(L, ld=64) == -1
    assert _call(L, nnz=1 << 31) == -1 and b"nnz" in L.blp_last_error()
    assert _call(L, q_head=(1 << 30), q_tail=1) == -1 and b"2^30" in L.blp_last_error()
    assert _call(L, row_base=(1 << 31) - 10) == -1
    for name in ("table", "source", "fixed_row", "rel_emb", "rel_id", "true_row", "set_ptr", "set_row", "qh", "qt", "counts"):
        assert _call(L, **{name: None}) == -1 and b"NULL" in L.blp_last_error(), name
    assert _call(L, G=0) == -1
    assert _call(L, R=0) == -1 and _call(L, S=0) == -1
    assert _call(L, table=(1 << 20) + 8) == -1 and b"aligned" in L.blp_last_error()
    assert _call(L, ld=130) == -1 and _call(L, ld_src=130) == -1 and _call(L, ld_src=64) == -1
    filt = _lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 100)
    assert _call(L, filter=filt) == -1 and b"row_base" in L.blp_last_error()
    assert _call(L, filter=_lib.BlpFilter(None, 1 << 33, 1 << 34, None, None, 0, 0)) == -1 and b"filter" in L.blp_last_error()
    assert _call(L, workspace=None) == -4 and b"workspace" in L.blp_last_error()
    assert _call(L, ws=1) == -4
    assert _call(L, ws=L.blp_rank_sets_workspace_bytes(0, 128, 2, 2, 3) - 1) == -4
    assert _call(L, workspace=(1 << 31) + 64) == -4
    assert _call(L, q_head=0, q_tail=0) == 0  # no query: nothing to do, nothing touched


def test_rank_sets_kernels_use_no_scratch():
    from blp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    obj = os.path.join(build.OBJ, "rank_sets.hip.o")
    kernels = kernel_resources.kernels_of(obj)
    assert len([k for k in kernels if "rank_sets_kernel" in k]) == 4 * 3  # four models x three widths
    assert len([k for k in kernels if "sets_unit_prefix" in k]) == 1
    assert all(v["private_segment_fixed_size"] == 0 for v in kernels.values()), [k for k, v in kernels.items() if v["private_segment_fixed_size"]]
    # the filter + finalize kernel with the membership test lives next to the one it extends
    shared = kernel_resources.kernels_of(os.path.join(build.OBJ, "rank_all.hip.o"))
    with_sets = [k for k in shared if "filter_finalize_kernel" in k and "SetLookup" in k]
    assert len(with_sets) == 4 * 3 and all(shared[k]["private_segment_fixed_size"] == 0 for k in with_sets)
    # the hand-issued scalar loads of the reused TransE body: no result touched before its wait, VALU wait states kept
    assert not kernel_resources.early_uses_of_scalar_loads(obj)
    assert not kernel_resources.valu_sgpr_hazards(obj)


# ------------------------------------------------------------------------------------------- CandidateSets
def test_candidate_sets_sort_deduplicate_and_validate():
    s = ranking.CandidateSets([[5, 3, 3, 1], [], torch.tensor([7, 2, 7]), (4,)])
    assert s.num_sets == 4 and s.ptr.tolist() == [0, 3, 3, 5, 6] and s.rows.tolist() == [1, 3, 5, 2, 7, 4]
    assert s.ptr.dtype == torch.int64 and s.rows.dtype == torch.int64
    assert s.tolist() == [[1, 3, 5], [], [2, 7], [4]]
    rect = ranking.CandidateSets(torch.tensor([[5, 3, -1, 3], [-1, -1, -1, -1], [9, 9, 2, 0]]))
    assert rect.tolist() == [[3, 5], [], [0, 2, 9]]
    csr = ranking.CandidateSets(ptr=torch.tensor([0, 3, 3, 5]), rows=torch.tensor([4, 4, 1, 8, 0]), num_rows=9)
    assert csr.tolist() == [[1, 4], [], [0, 8]]
    assert csr.contains(torch.tensor([0, 0, 1, 2, 2]), torch.tensor([4, 2, 4, 0, 8])).tolist() == [True, False, False, True, True]
    assert ranking.CandidateSets([]).num_sets == 0
    rng = np.random.default_rng(0)
    lists = [rng.integers(0, 50, rng.integers(0, 40)).tolist() for _ in range(30)]
    assert ranking.CandidateSets(lists).tolist() == [sorted(set(x)) for x in lists]
    for bad in (dict(ptr=torch.tensor([0, 3, 2, 5]), rows=torch.arange(5)), dict(ptr=torch.tensor([1, 5]), rows=torch.arange(5)),
                dict(ptr=torch.tensor([0, 4]), rows=torch.arange(5)), dict(sets=[[1, -2]]), dict(sets=[[1, 20]], num_rows=10),
                dict(sets=torch.tensor([1, 2, 3])), dict(sets=torch.tensor([[0.5, 1.0]])), dict(sets=[[1]], ptr=torch.tensor([0, 1])),
                dict(ptr=torch.tensor([0, 1])), dict()):
        with pytest.raises(ValueError):
            ranking.CandidateSets(**bad)


def test_relation_candidate_sets_on_a_toy_graph():
    ent2idx = torch.tensor([3, -1, 0, 2, 1, -1, 4])  # ids 1 and 5 have no row
    graph = torch.tensor([[0, 2, 1], [2, 0, 1], [0, 3, 1], [1, 4, 0], [4, 1, 0], [6, 6, 2], [9, 0, 2], [0, 2, 1], [3, 5, 2]])
    R = 4  # relation 3 never occurs
    sets = ranking.relation_candidate_sets(graph, R, ent2idx)
    assert sets.num_sets == 2 * R
    want = [set() for _ in range(2 * R)]
    for h, t, r in graph.tolist():
        for ent, g in ((h, r), (t, R + r)):
            if 0 <= ent < len(ent2idx) and ent2idx[ent] >= 0:
                want[g].add(int(ent2idx[ent]))
    assert sets.tolist() == [sorted(x) for x in want]
    assert sets.tolist()[3] == [] and sets.tolist()[R + 3] == []
    with pytest.raises(ValueError):
        ranking.relation_candidate_sets(graph, 2, ent2idx)


# ------------------------------------------------------------------------------------------- rank_in_sets on CPU tensors
def _model(rel_model, rel_w):
    m = models.LinkPrediction(rel_w.shape[1], rel_model, "margin", rel_w.shape[0], 0)
    with torch.no_grad():
        m.rel_emb.weight.copy_(torch.from_numpy(rel_w))
    return m


@pytest.fixture(scope="module", params=REL_MODELS)
def toy(request):
    rel_model = request.param
    g, f = golden(f"eval_toy_{rel_model}"), golden("filters_toy")
    table, triples, ent2idx = torch.from_numpy(g["ent_emb"]), torch.from_numpy(f["triples"]), torch.from_numpy(f["ent2idx"])
    return dict(rel_model=rel_model, model=_model(rel_model, g["rel_w"]), table=table, triples=triples, ent2idx=ent2idx,
                index=utils.FilterIndex(torch.from_numpy(f["graph_edges"])), graph=torch.from_numpy(f["graph_edges"]), R=g["rel_w"].shape[0])


def _expanded(sets, set_ids):
    """The per-query lists the sets expand to: a CSR (ptr (Q + 1,), rows) for rank_candidates."""
    lists = sets.tolist()
    per_query = [lists[g] for g in set_ids.tolist()]
    ptr = torch.tensor(np.concatenate(([0], np.cumsum([len(x) for x in per_query]))).astype(np.int64))
    return ptr, torch.tensor([x for rows in per_query for x in rows], dtype=torch.long)


def _random_sets(N, G, rng):
    sizes = [0, 1, N] + [int(x) for x in rng.integers(2, N, G - 3)]
    return ranking.CandidateSets([rng.choice(N, n, replace=False) for n in sizes])


@pytest.mark.parametrize("filtered", [False, True])
def test_counts_equal_rank_candidates_on_the_expanded_lists(toy, filtered):
    N, T = toy["table"].shape[0], toy["triples"].shape[0]
    Q = 2 * T
    rng = np.random.default_rng(11)
    G = 9
    sets = _random_sets(N, G, rng)
    set_ids = torch.from_numpy(rng.integers(0, G, Q))
    set_ids[:3] = torch.tensor([0, 1, 2])  # the empty set, a one-row set and the whole table serve queries
    index = toy["index"] if filtered else None
    args = (toy["model"], toy["table"], toy["triples"])
    want = ranking.rank_candidates(*args, _expanded(sets, set_ids), toy["ent2idx"], filter_index=index)
    got = ranking.rank_in_sets(*args, sets, toy["ent2idx"], set_ids=set_ids, filter_index=index, add_true=False)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    assert int(want[:, 1].max()) > 0
    if filtered:
        assert bool((want[:, 3] < want[:, 1]).any()), "the filter must bite somewhere"
    else:
        assert torch.equal(got[:, 2:], got[:, :2])
    # add_true: + 1 on both ge columns exactly where the true row is not in the query's set (a plain loop)
    lists = sets.tolist()
    true_rows = toy["ent2idx"][torch.cat((toy["triples"][:, 0], toy["triples"][:, 1]))].tolist()
    absent = torch.tensor([true_rows[q] not in lists[g] for q, g in enumerate(set_ids.tolist())])
    assert bool(absent.any()) and not bool(absent.all())
    with_true = ranking.rank_in_sets(*args, sets, toy["ent2idx"], set_ids=set_ids, filter_index=index)
    assert torch.equal(with_true, want + absent.to(torch.int32).unsqueeze(1) * torch.tensor([0, 1, 0, 1], dtype=torch.int32))
    # one side at a time
    for side, sl in (("head", slice(0, T)), ("tail", slice(T, Q))):
        one = ranking.rank_in_sets(*args, sets, toy["ent2idx"], set_ids=set_ids[sl], side=side, filter_index=index, add_true=False)
        assert torch.equal(one, want[sl])


def test_default_set_ids_are_the_type_constrained_protocol(toy):
    R, T = toy["R"], toy["triples"].shape[0]
    sets = ranking.relation_candidate_sets(toy["graph"], R, toy["ent2idx"])
    args = (toy["model"], toy["table"], toy["triples"])
    rel = toy["triples"][:, 2]
    explicit = torch.cat((rel, rel + R))
    got = ranking.rank_in_sets(*args, sets, toy["ent2idx"], filter_index=toy["index"], add_true=False)
    want = ranking.rank_candidates(*args, _expanded(sets, explicit), toy["ent2idx"], filter_index=toy["index"])
    assert torch.equal(got, want)
    assert torch.equal(got, ranking.rank_in_sets(*args, sets, toy["ent2idx"], set_ids=explicit, filter_index=toy["index"], add_true=False))
    rr, hits = ranking.metrics_from_counts(ranking.rank_in_sets(*args, sets, toy["ent2idx"], filter_index=toy["index"]))
    assert rr.shape == (2 * T, 2) and hits.shape == (2 * T, 2, 3) and bool((rr > 0).all()) and bool((rr <= 1).all())


def test_every_set_the_full_table_equals_rank_block(toy):
    """The protocol degenerates to the reference's: with every set the whole table, the counts are rank_block's."""
    table, triples, ent2idx = toy["table"], toy["triples"], toy["ent2idx"]
    N, T = table.shape[0], triples.shape[0]
    G = 3
    sets = ranking.CandidateSets([np.arange(N)] * G)
    set_ids = torch.from_numpy(np.random.default_rng(2).integers(0, G, 2 * T))
    got = ranking.rank_in_sets(toy["model"], table, triples, sets, ent2idx, set_ids=set_ids, filter_index=toy["index"])
    h_row, t_row, r = ent2idx[triples[:, 0]], ent2idx[triples[:, 1]], triples[:, 2]
    rel_w = toy["model"].rel_emb.weight.detach()
    rowptr, col = toy["index"].csr(triples, ent2idx)
    want = ranking.rank_block(toy["model"], table, torch.cat((table[t_row], table[h_row])), rel_w[torch.cat((r, r))], T,
                              true_row=torch.cat((h_row, t_row)), filt_rowptr=rowptr, filt_col=col)
    assert torch.equal(got, want)


def test_rank_in_sets_argument_errors(toy):
    args = (toy["model"], toy["table"], toy["triples"])
    Q = 2 * toy["triples"].shape[0]
    sets = ranking.CandidateSets([[0, 1], [2]])
    with pytest.raises(ValueError):
        ranking.rank_in_sets(*args, sets, toy["ent2idx"], set_ids=torch.zeros(Q, dtype=torch.long), side="middle")
    for bad in (torch.full((Q,), 2), torch.full((Q,), -1), torch.zeros(Q - 1, dtype=torch.long)):
        with pytest.raises(ValueError):
            ranking.rank_in_sets(*args, sets, toy["ent2idx"], set_ids=bad)
    with pytest.raises(ValueError):  # the default ids need 2 R sets
        ranking.rank_in_sets(*args, sets, toy["ent2idx"])
    with pytest.raises(ValueError):
        ranking.rank_in_sets(*args, ranking.CandidateSets([[toy["table"].shape[0]]]), toy["ent2idx"], set_ids=torch.zeros(Q, dtype=torch.long))
