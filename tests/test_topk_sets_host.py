"""Filtered top-k inside shared candidate sets, without a GPU (include/blp_hip.h: blp_topk_sets_supported,
blp_topk_sets_workspace_bytes, blp_topk_sets; ranking.predict_links_in_sets): the entry points are exported and bound, which
(model, D, k) they take, the workspace bound, the argument refusals (checked before anything touches a device), no scratch
memory in the new kernels, and the CPU route of predict_links_in_sets -- the oracle of the fused one -- against
rank_candidates' scores on the expanded per-query lists and against predict_links on the full table."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden
from blp_amd import _lib, models, ops, ranking, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_topk_sets_supported", "blp_topk_sets_workspace_bytes", "blp_topk_sets")


def _L():
    return _lib.lib()


def _exported(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines()}


def test_new_entry_points_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "blp_hip.h")).read()
    L = _L()
    for name in NEW:
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert getattr(L, name).argtypes is not None
        assert name in _exported(_lib.LIB_PATH) and name in _exported(_lib.HOOKS_LIB_PATH)
    assert L.blp_version() == 60000
    assert callable(ops.topk_sets) and callable(ops.topk_sets_supported) and callable(ranking.predict_links_in_sets)
    assert _lib.KNOBS[-1] == "topk_sets_grid"
    assert not hasattr(L, "blp_debug_set_knob")  # the product library exports no hook


def test_supported_grid():
    L = _L()
    for m in range(4):
        for D in (64, 128, 256):
            assert L.blp_topk_sets_supported(m, D, 1) and L.blp_topk_sets_supported(m, D, 256), (m, D)
            assert not L.blp_topk_sets_supported(m, D, 0) and not L.blp_topk_sets_supported(m, D, 257), (m, D)
        for D in (100, 300):
            assert not L.blp_topk_sets_supported(m, D, 10), (m, D)
    assert not L.blp_topk_sets_supported(4, 128, 10) and not L.blp_topk_sets_supported(-1, 128, 10)
    assert ops.topk_sets_supported("complex", 256, 256) and not ops.topk_sets_supported("transe", 300, 10)
    assert not ops.topk_sets_supported("transe", 128, 257)


def test_workspace_is_aligned_monotone_bounded_and_free_of_N():
    """Coefficient rows, partial lists, G + 1 unit offsets: 256-byte aligned, monotone in Q, G and k, bounded by the header's
    8 (D + k) Q + 8 (G + 1) + 4 MiB whatever nnz, and N is not even an argument."""
    L = _L()
    bound = lambda D, Q, G, k: 8 * (D + k) * Q + 8 * (G + 1) + (4 << 20)
    for m, D in ((0, 64), (1, 128), (2, 256), (3, 128)):
        for nnz in (0, 1, 10_000, 1_500_000, (1 << 31) - 1):
            for k in (1, 10, 192, 256):
                last = 0
                for qh, qt in ((0, 1), (1, 1), (2, 2), (100, 3), (6894, 6894), (52870, 52870)):
                    n = L.blp_topk_sets_workspace_bytes(m, D, qh, qt, 474, nnz, k)
                    assert n % 256 == 0 and n >= last and n > 0, (m, D, nnz, k, qh, qt)
                    assert n >= (qh + qt) * 8 * (D + k) and n <= bound(D, qh + qt, 474, k), (m, D, nnz, k, qh, qt, n)
                    last = n
            sizes = [L.blp_topk_sets_workspace_bytes(m, D, 300, 300, G, nnz, 10) for G in (1, 12, 474, 1644, 100000)]
            assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
            sizes = [L.blp_topk_sets_workspace_bytes(m, D, 300, 300, 474, nnz, k) for k in (1, 2, 10, 64, 96, 97, 192, 256)]
            assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
        # few queries against long sets: more than one partial list per query, still inside the bound
        assert L.blp_topk_sets_workspace_bytes(m, D, 2, 2, 1, 1_000_000, 256) > L.blp_topk_sets_workspace_bytes(m, D, 2, 2, 1, 64, 256)
    # N is not an argument: ops' sizing takes no table length, so a table of 10^3 and one of 10^9 rows ask for the same bytes
    import inspect
    assert list(inspect.signature(ops.topk_sets_workspace_bytes).parameters) == ["rel_model", "D", "q_head", "q_tail", "num_sets", "nnz", "k"]
    assert ops.topk_sets_workspace_bytes("transe", 128, 300, 300, 474, 1000, 10) == L.blp_topk_sets_workspace_bytes(0, 128, 300, 300, 474, 1000, 10)
    assert L.blp_topk_sets_workspace_bytes(1, 300, 2, 2, 5, 10, 10) == 0
    assert L.blp_topk_sets_workspace_bytes(7, 128, 2, 2, 5, 10, 10) == 0
    assert L.blp_topk_sets_workspace_bytes(0, 128, -1, 2, 5, 10, 10) == 0
    assert L.blp_topk_sets_workspace_bytes(0, 128, 2, 2, -1, 10, 10) == 0
    assert L.blp_topk_sets_workspace_bytes(0, 128, 2, 2, 5, -1, 10) == 0
    assert L.blp_topk_sets_workspace_bytes(0, 128, 2, 2, 5, 10, 0) == 0 and L.blp_topk_sets_workspace_bytes(0, 128, 2, 2, 5, 10, 257) == 0


def _call(L, **over):
    """blp_topk_sets with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(model=0, table=1 << 20, N=1000, D=128, ld=128, row_base=0, source=1 << 21, S=1000, ld_src=128, fixed_row=1 << 22,
             rel_emb=1 << 23, R=5, rel_id=1 << 24, q_head=2, q_tail=2, k=10, set_ptr=1 << 26, set_row=1 << 27, nnz=100, G=3,
             qh=1 << 28, qt=1 << 29, filter=None, rows=1 << 30, scores=1 << 25, workspace=1 << 31, ws=1 << 24, device=0, stream=None)
    a.update(over)
    f = a["filter"]
    return L.blp_topk_sets(a["model"], a["table"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"], a["ld_src"],
                           a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["q_head"], a["q_tail"], a["k"], a["set_ptr"],
                           a["set_row"], a["nnz"], a["G"], a["qh"], a["qt"], None if f is None else ctypes.byref(f), a["rows"],
                           a["scores"], a["workspace"], a["ws"], a["device"], a["stream"])


def test_bad_arguments():
    L = _L()
    assert _call(L, model=7) == -1 and b"unknown model" in L.blp_last_error()
    assert _call(L, k=0) == -1 and b"k = 0" in L.blp_last_error()
    assert _call(L, k=257) == -1 and _call(L, k=-3) == -1
    for D in (300, 100, 32):
        assert _call(L, D=D, ld=D, ld_src=D) == -2 and b"not supported" in L.blp_last_error()
    for name in ("N", "q_head", "q_tail", "nnz", "G", "row_base"):
        assert _call(L, **{name: -1}) == -1 and b"negative" in L.blp_last_error(), name
    filt = _lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 100)
    assert _call(L, filter=filt) == -1 and b"row_base" in L.blp_last_error()
    assert _call(L, row_base=100, filter=filt, workspace=None) == -4  # the same filter on its own shard passes the check
    assert _call(L, filter=_lib.BlpFilter(None, 1 << 33, 1 << 34, None, None, 0, 0)) == -1 and b"filter" in L.blp_last_error()
    assert _call(L, ld=130) == -1 and b"aligned" in L.blp_last_error()  # misaligned rows
    assert _call(L, ld=64) == -1 and _call(L, ld_src=130) == -1 and _call(L, ld_src=64) == -1
    assert _call(L, table=(1 << 20) + 8) == -1 and b"aligned" in L.blp_last_error()
    assert _call(L, rows=None) == -1 and b"NULL" in L.blp_last_error()
    assert _call(L, scores=None) == -1 and b"NULL" in L.blp_last_error()
    for name in ("table", "source", "fixed_row", "rel_emb", "rel_id", "set_ptr", "set_row", "qh", "qt"):
        assert _call(L, **{name: None}) == -1 and b"NULL" in L.blp_last_error(), name
    assert _call(L, G=0) == -1 and _call(L, R=0) == -1 and _call(L, S=0) == -1
    # Q x k must stay below 2^31; so must nnz and the global rows
    assert _call(L, q_head=1 << 23, q_tail=1, k=256) == -1 and b"2^31" in L.blp_last_error()
    assert _call(L, q_head=(1 << 31) // 10, q_tail=1, k=10) == -1
    assert _call(L, nnz=1 << 31) == -1 and b"nnz" in L.blp_last_error()
    assert _call(L, row_base=(1 << 31) - 10) == -1
    assert _call(L, workspace=None) == -4 and b"workspace" in L.blp_last_error()
    assert _call(L, ws=1) == -4
    assert _call(L, ws=L.blp_topk_sets_workspace_bytes(0, 128, 2, 2, 3, 100, 10) - 1) == -4
    assert _call(L, workspace=(1 << 31) + 64) == -4
    assert _call(L, q_head=0, q_tail=0) == 0  # no query: nothing to do, nothing touched
    assert _call(L, q_head=0, q_tail=0, workspace=None, ws=0, G=0, set_ptr=None, qh=None, qt=None) == 0


def test_topk_sets_kernels_use_no_scratch_and_topk_keeps_its_kernels():
    from blp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    for obj_dir in (build.OBJ, os.path.join(build.OBJ, build.HOOKS_VARIANT)):
        kernels = kernel_resources.kernels_of(os.path.join(obj_dir, "topk_sets.hip.o"))
        assert len([k for k in kernels if "topk_sets_kernel" in k]) == 4 * 3  # four models x three widths
        assert len([k for k in kernels if "topk_sets_unit_prefix" in k]) == 1
        assert len(kernels) == 13
        assert all(v["private_segment_fixed_size"] == 0 for v in kernels.values()), [k for k, v in kernels.items() if v["private_segment_fixed_size"]]
    # the list helpers moved into topk_lists.h: topk.hip.o holds exactly the kernels it held (tests/test_topk16_host.py counts
    # the 16-bit ones), the merge and rescore kernels are reached through its host launchers
    shared = kernel_resources.kernels_of(os.path.join(build.OBJ, "topk.hip.o"))
    assert len([k for k in shared if "topk_tiles_kernel" in k]) == 12
    assert len([k for k in shared if "topk_tiles16" in k or ("topk_rescore" in k and "DF16" in k)]) == 2 * 2 * 12
    assert len([k for k in shared if "topk_rescore" in k]) == 3 * 12 and len([k for k in shared if "topk_merge" in k]) == 2
    assert len(shared) == 12 + 24 + 36 + 2
    assert all(v["private_segment_fixed_size"] == 0 for v in shared.values())


# ------------------------------------------------------------------------------------------- predict_links_in_sets on CPU tensors
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


def _random_sets(N, G, rng):
    sizes = [0, 1, N] + [int(x) for x in rng.integers(2, N, G - 3)]
    return ranking.CandidateSets([rng.choice(N, n, replace=False) for n in sizes])


def _rect(sets, set_ids):
    """The per-query lists the sets expand to, as a (Q, C) rectangle padded with -1, for rank_candidates."""
    lists = sets.tolist()
    per_query = [lists[g] for g in set_ids.tolist()]
    C = max(1, max(len(x) for x in per_query))
    return torch.tensor([x + [-1] * (C - len(x)) for x in per_query], dtype=torch.long)


def _removed(toy, rect, side="both"):
    """(Q, C) bool: the known edges of each query among its candidates, the triple's own entity kept (a plain loop)."""
    known_heads, known_tails = {}, {}
    for h, t, r in toy["graph"].tolist():
        known_heads.setdefault((t, r), set()).add(h)
        known_tails.setdefault((h, r), set()).add(t)
    row2ent = {int(row): ent for ent, row in enumerate(toy["ent2idx"].tolist()) if row >= 0}
    queries = []
    if side in ("head", "both"):
        queries += [(known_heads.get((t, r), set()), h) for h, t, r in toy["triples"].tolist()]
    if side in ("tail", "both"):
        queries += [(known_tails.get((h, r), set()), t) for h, t, r in toy["triples"].tolist()]
    out = torch.zeros(rect.shape, dtype=torch.bool)
    for q, (known, own) in enumerate(queries):
        for c, row in enumerate(rect[q].tolist()):
            out[q, c] = row >= 0 and row2ent[row] in known and row2ent[row] != own
    return out


def _same(got, want):
    assert torch.equal(got[0], want[0])
    nan = torch.isnan(want[1])
    assert torch.equal(torch.isnan(got[1]), nan)
    assert torch.equal(got[1][~nan].view(torch.int32), want[1][~nan].view(torch.int32))


@pytest.mark.parametrize("filtered", [False, True])
def test_equals_the_top_k_of_rank_candidates_scores(toy, filtered):
    N, T = toy["table"].shape[0], toy["triples"].shape[0]
    Q = 2 * T
    rng = np.random.default_rng(11)
    G = 9
    sets = _random_sets(N, G, rng)
    set_ids = torch.from_numpy(rng.integers(0, G, Q))
    set_ids[:3] = torch.tensor([0, 1, 2])  # the empty set, a one-row set and the whole table serve queries
    index = toy["index"] if filtered else None
    args = (toy["model"], toy["table"], toy["triples"])
    rect = _rect(sets, set_ids)
    _, scores = ranking.rank_candidates(*args, rect, toy["ent2idx"], return_scores=True)
    removed = _removed(toy, rect) if filtered else torch.zeros(rect.shape, dtype=torch.bool)
    assert not filtered or bool(removed.any()), "the filter must bite somewhere"
    for k in (1, 3, N + 5):
        want = ranking._stable_topk(scores, rect, removed, k)
        got = ranking.predict_links_in_sets(*args, k, sets, toy["ent2idx"], set_ids=set_ids, filter_index=index)
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[0].shape == (Q, k)
        _same(got, want)
        assert bool((got[0][0] == -1).all()) and bool(torch.isnan(got[1][0]).all())  # the empty set
        for side, sl in (("head", slice(0, T)), ("tail", slice(T, Q))):
            one = ranking.predict_links_in_sets(*args, k, sets, toy["ent2idx"], set_ids=set_ids[sl], side=side, filter_index=index)
            _same(one, (want[0][sl], want[1][sl]))
    if filtered:  # known edges never come back
        got = ranking.predict_links_in_sets(*args, N, sets, toy["ent2idx"], set_ids=set_ids, filter_index=index)
        gone = [set(rect[q][removed[q]].tolist()) for q in range(Q)]
        assert all(not (gone[q] & set(got[0][q].tolist())) for q in range(Q))
        plain = ranking.predict_links_in_sets(*args, N, sets, toy["ent2idx"], set_ids=set_ids)
        assert any(gone[q] & set(plain[0][q].tolist()) for q in range(Q))
    # a tiny piece budget takes the row-slab and query-chunk loops of the dense route
    g = ranking._group_by_set(set_ids, T, G)
    fixed_rows = toy["ent2idx"][torch.cat((toy["triples"][:, 1], toy["triples"][:, 0]))][g[0]]
    rel = toy["model"].rel_emb.weight.detach()[torch.cat((toy["triples"][:, 2],) * 2)][g[0]]
    big = ranking._topk_sets_dense(toy["model"].score_fn, toy["table"], toy["table"][fixed_rows], rel, T, 3, sets.ptr, sets.rows, g[1], g[2], 0, None)
    small = ranking._topk_sets_dense(toy["model"].score_fn, toy["table"], toy["table"][fixed_rows], rel, T, 3, sets.ptr, sets.rows, g[1], g[2], 0,
                                     None, max_bytes=12 * toy["table"].shape[1] * 7)
    _same(small, big)


def test_every_set_the_full_table_equals_predict_links(toy):
    table, triples, ent2idx = toy["table"], toy["triples"], toy["ent2idx"]
    N, T = table.shape[0], triples.shape[0]
    G = 3
    sets = ranking.CandidateSets([np.arange(N)] * G)
    set_ids = torch.from_numpy(np.random.default_rng(2).integers(0, G, 2 * T))
    entities = torch.arange(N) * 3 + 1
    for k in (1, 4, N + 2):
        for index in (None, toy["index"]):
            for side, sl in (("both", slice(0, 2 * T)), ("head", slice(0, T)), ("tail", slice(T, 2 * T))):
                want = ranking.predict_links(toy["model"], table, triples, k, ent2idx, side=side, filter_index=index, entities=entities)
                got = ranking.predict_links_in_sets(toy["model"], table, triples, k, sets, ent2idx, set_ids=set_ids[sl], side=side,
                                                    filter_index=index, entities=entities)
                _same(got, want)


def test_default_set_ids_are_the_type_constrained_protocol(toy):
    R = toy["R"]
    sets = ranking.relation_candidate_sets(toy["graph"], R, toy["ent2idx"])
    args = (toy["model"], toy["table"], toy["triples"])
    rel = toy["triples"][:, 2]
    explicit = torch.cat((rel, rel + R))
    got = ranking.predict_links_in_sets(*args, 3, sets, toy["ent2idx"], filter_index=toy["index"])
    _same(got, ranking.predict_links_in_sets(*args, 3, sets, toy["ent2idx"], set_ids=explicit, filter_index=toy["index"]))
    lists = sets.tolist()
    for q, g in enumerate(explicit.tolist()):  # every answer is a member of the query's relation set
        assert set(got[0][q][got[0][q] >= 0].tolist()) <= set(lists[g])
    for side, ids in (("head", rel), ("tail", rel + R)):
        _same(ranking.predict_links_in_sets(*args, 3, sets, toy["ent2idx"], side=side),
              ranking.predict_links_in_sets(*args, 3, sets, toy["ent2idx"], side=side, set_ids=ids))


def test_predict_links_in_sets_argument_errors(toy):
    args = (toy["model"], toy["table"], toy["triples"])
    Q = 2 * toy["triples"].shape[0]
    sets = ranking.CandidateSets([[0, 1], [2]])
    with pytest.raises(ValueError):
        ranking.predict_links_in_sets(*args, 3, sets, toy["ent2idx"], set_ids=torch.zeros(Q, dtype=torch.long), side="middle")
    with pytest.raises(ValueError):
        ranking.predict_links_in_sets(*args, 0, sets, toy["ent2idx"], set_ids=torch.zeros(Q, dtype=torch.long))
    for bad in (torch.full((Q,), 2), torch.full((Q,), -1), torch.zeros(Q - 1, dtype=torch.long)):
        with pytest.raises(ValueError):
            ranking.predict_links_in_sets(*args, 3, sets, toy["ent2idx"], set_ids=bad)
    with pytest.raises(ValueError):  # the default ids need 2 R sets
        ranking.predict_links_in_sets(*args, 3, sets, toy["ent2idx"])
    with pytest.raises(ValueError):
        ranking.predict_links_in_sets(*args, 3, ranking.CandidateSets([[toy["table"].shape[0]]]), toy["ent2idx"],
                                      set_ids=torch.zeros(Q, dtype=torch.long))
