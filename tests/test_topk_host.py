"""Filtered top-k link prediction without a GPU: the CPU route of ranking.predict_links against the reference score goldens
(every candidate's score is in them) and the filter fixtures, the C-ABI's workspace bound and argument refusals (checked
before anything touches a device), and candidate-axis sharding on gloo ranks."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import REL_MODELS, golden, golden_names
from blp_amd import models, ranking, utils

KS = (1, 5, 64, 192, 200)
SCORE_GOLDENS = golden_names("scores_")


def _model(rel_model, rel_w):
    m = models.LinkPrediction(rel_w.shape[1], rel_model, "margin", rel_w.shape[0], 0)
    with torch.no_grad():
        m.rel_emb.weight.copy_(torch.from_numpy(rel_w))
    return m


def _stable(pred, k):
    order = np.argsort(-pred, axis=1, kind="stable")[:, :k]
    return order, np.take_along_axis(pred, order, axis=1)


def test_score_goldens_cover_every_model_width_and_shape():
    assert len(SCORE_GOLDENS) == 32


@pytest.mark.parametrize("name", SCORE_GOLDENS)
def test_predict_links_matches_stable_order_of_reference_scores(name):
    g = golden(name)
    rel_model = name.split("_")[1]
    table, n = torch.from_numpy(g["table"]), g["table"].shape[0]
    triples = torch.from_numpy(np.concatenate((g["heads"], g["tails"], g["rels"]), axis=1))
    model = _model(rel_model, g["rel_w"])
    ent2idx = torch.arange(n)
    for k in KS:
        both_rows, both_scores = ranking.predict_links(model, table, triples, k, ent2idx)
        for side, pred in (("head", g["head_pred"]), ("tail", g["tail_pred"])):
            rows, scores = ranking.predict_links(model, table, triples, k, ent2idx, side=side)
            want_rows, want_scores = _stable(pred, k)
            kk = min(k, n)
            assert np.array_equal(rows[:, :kk].numpy(), want_rows), (name, side, k)
            assert np.array_equal(scores[:, :kk].numpy().view(np.int32), want_scores.view(np.int32)), (name, side, k)
            if k > n:  # fewer candidates than slots: -1 / NaN padding
                assert (rows[:, n:] == -1).all() and torch.isnan(scores[:, n:]).all()
            half = slice(0, len(triples)) if side == "head" else slice(len(triples), 2 * len(triples))
            assert torch.equal(both_rows[half], rows)
            assert np.array_equal(both_scores[half].numpy().view(np.int32), scores.numpy().view(np.int32))


def test_predict_links_ties_order_by_row():
    """The ties fixtures hold exact duplicates: equal scores must come out by ascending row."""
    g = golden("scores_transe_ties_d64")
    pred = g["tail_pred"]
    assert any(len(np.unique(row)) < len(row) for row in pred)
    model = _model("transe", g["rel_w"])
    triples = torch.from_numpy(np.concatenate((g["heads"], g["tails"], g["rels"]), axis=1))
    rows, scores = ranking.predict_links(model, torch.from_numpy(g["table"]), triples, 192, torch.arange(192), side="tail")
    s, r = scores.numpy(), rows.numpy()
    same = s[:, 1:] == s[:, :-1]
    assert same.any() and (r[:, 1:][same] > r[:, :-1][same]).all()


@pytest.mark.parametrize("rel_model", REL_MODELS)
def test_predict_links_filtered_on_toy_graph(rel_model):
    g, f = golden(f"eval_toy_{rel_model}"), golden("filters_toy")
    ent_emb = torch.from_numpy(g["ent_emb"])
    entities = torch.from_numpy(f["entities"])
    ent2idx = torch.from_numpy(f["ent2idx"])
    triples = torch.from_numpy(f["triples"])
    index = utils.FilterIndex(torch.from_numpy(f["graph_edges"]))
    model = _model(rel_model, g["rel_w"])
    n, T = ent_emb.shape[0], triples.shape[0]
    for k in (1, 10, 52, 60):
        rows, scores = ranking.predict_links(model, ent_emb, triples, k, ent2idx, filter_index=index)
        ids, _ = ranking.predict_links(model, ent_emb, triples, k, ent2idx, filter_index=index, entities=entities)
        raw_rows, raw_scores = ranking.predict_links(model, ent_emb, triples, n, ent2idx)
        masks = np.concatenate((f["heads_filter"], f["tails_filter"]))
        exclude = np.concatenate((ent2idx[triples[:, 0]].numpy(), ent2idx[triples[:, 1]].numpy()))
        for q in range(2 * T):
            got = rows[q].numpy()
            kept = got[got >= 0]
            assert not masks[q, kept].any(), "a filtered row came back"
            # the stable order of the unfiltered remainder
            order = [int(x) for x in raw_rows[q].numpy() if not masks[q, x]]
            assert kept.tolist() == order[:k]
            assert (got[len(kept):] == -1).all() and torch.isnan(scores[q, len(kept):]).all()
            assert len(kept) == min(k, n - int(masks[q].sum()))
            if exclude[q] in order[:k]:
                assert exclude[q] in kept  # the triple's own entity survives its filter
            assert np.array_equal(scores[q, :len(kept)].numpy().view(np.int32),
                                  raw_scores[q].numpy()[[raw_rows[q].tolist().index(x) for x in kept]].view(np.int32))
            assert ids[q].tolist() == [int(entities[x]) if x >= 0 else -1 for x in got]
        # the exclude entity is never filtered: with every query's own entity known, it is among the candidates left
        assert all(exclude[q] in [int(x) for x in raw_rows[q]] for q in range(2 * T))


def test_predict_links_replaced_minus_one_filters_everything_known():
    """A -1 at the replaced position exempts nothing: every known edge of (h, r, ?) is removed."""
    g, f = golden("eval_toy_transe"), golden("filters_toy")
    ent_emb, ent2idx = torch.from_numpy(g["ent_emb"]), torch.from_numpy(f["ent2idx"])
    triples = torch.from_numpy(f["triples"]).clone()
    index = utils.FilterIndex(torch.from_numpy(f["graph_edges"]))
    model = _model("transe", g["rel_w"])
    open_q = triples.clone()
    open_q[:, 1] = -1
    rows, _ = ranking.predict_links(model, ent_emb, open_q, 52, ent2idx, side="tail", filter_index=index)
    own, _ = ranking.predict_links(model, ent_emb, triples, 52, ent2idx, side="tail", filter_index=index)
    edges = torch.from_numpy(f["graph_edges"])
    for q, (h, t, r) in enumerate(triples.tolist()):
        known = {int(ent2idx[x]) for x in edges[(edges[:, 0] == h) & (edges[:, 2] == r), 1].tolist() if ent2idx[x] >= 0}
        got = set(int(x) for x in rows[q] if x >= 0)
        assert not (got & known) and len(got) == 52 - len(known)
        if int(ent2idx[t]) in known:
            assert int(ent2idx[t]) in set(int(x) for x in own[q] if x >= 0)


def test_predict_links_argument_errors():
    g = golden("scores_transe_gauss_d64")
    model = _model("transe", g["rel_w"])
    table = torch.from_numpy(g["table"])
    triples = torch.from_numpy(np.concatenate((g["heads"], g["tails"], g["rels"]), axis=1))
    with pytest.raises(ValueError):
        ranking.predict_links(model, table, triples, 5, torch.arange(192), side="middle")
    with pytest.raises(ValueError):
        ranking.predict_links(model, table, triples, 0, torch.arange(192))
    bad = triples.clone()
    bad[0, 1] = -1  # the fixed entity of a head query
    with pytest.raises(ValueError):
        ranking.predict_links(model, table, bad, 5, torch.arange(192), side="head")


# ------------------------------------------------------------------------------------------- C-ABI, no device touched
def _L():
    from blp_amd import _lib
    return _lib.lib()


def test_topk_supported_and_workspace_bound():
    L = _L()
    for m in range(4):
        for D in (64, 128, 256):
            assert L.blp_topk_supported(m, D, 1) and L.blp_topk_supported(m, D, 256)
            assert not L.blp_topk_supported(m, D, 0) and not L.blp_topk_supported(m, D, 257)
        for D in (32, 96, 300):
            assert not L.blp_topk_supported(m, D, 10)
    assert not L.blp_topk_supported(4, 128, 10)
    for m in range(4):
        for D in (64, 128, 256):
            for qh, qt in ((2, 2), (0, 128), (52870, 52870), (1, 0)):
                Q = qh + qt
                for k in (1, 10, 256):
                    sizes = [L.blp_topk_workspace_bytes(m, N, D, qh, qt, k) for N in (1_000_000, 2_000_000, 4_600_000, 1 << 30)]
                    assert len(set(sizes)) == 1, (m, D, Q, k, sizes)  # flat in N from 1 M rows on
                    assert 0 < sizes[0] <= 8 * (D + k) * Q + (4 << 20), (m, D, Q, k, sizes[0])  # the header's bound
    # linear in Q x k once the queries fill the grid: doubling Q doubles the partial lists
    a = L.blp_topk_workspace_bytes(0, 4_600_000, 128, 50_000, 50_000, 10)
    b = L.blp_topk_workspace_bytes(0, 4_600_000, 128, 100_000, 100_000, 10)
    assert abs(b - 2 * a) <= 4096
    assert L.blp_topk_workspace_bytes(0, 1000, 128, 2, 2, 0) == 0 and L.blp_topk_workspace_bytes(0, 1000, 96, 2, 2, 10) == 0


def _call(L, **over):
    """blp_topk with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    from blp_amd import _lib
    a = dict(model=0, table=1 << 20, N=1000, D=128, ld=128, row_base=0, source=1 << 21, S=1000, ld_src=128, fixed_row=1 << 22,
             rel_emb=1 << 23, R=5, rel_id=1 << 24, q_head=2, q_tail=2, k=10, filter=None, rows=1 << 25, scores=1 << 26,
             workspace=1 << 27, ws=1 << 30, device=0, stream=None)
    a.update(over)
    f = a["filter"]
    return L.blp_topk(a["model"], a["table"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"], a["ld_src"],
                      a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["q_head"], a["q_tail"], a["k"],
                      None if f is None else ctypes.byref(f), a["rows"], a["scores"], a["workspace"], a["ws"], a["device"],
                      a["stream"])


def test_topk_refuses_bad_arguments():
    from blp_amd import _lib
    L = _L()
    assert _call(L, k=0) == -1 and b"k = 0" in L.blp_last_error()
    assert _call(L, k=257) == -1
    assert _call(L, D=96, ld=96, ld_src=96) == -2
    assert _call(L, model=7) == -1
    filt = _lib.BlpFilter(1 << 28, 1 << 29, 1 << 30, None, None, 0, 100)
    assert _call(L, filter=filt) == -1 and b"row_base" in L.blp_last_error()
    assert _call(L, rows=None) == -1
    assert _call(L, scores=None) == -1
    assert _call(L, workspace=None) == -4
    assert _call(L, ws=1) == -4
    assert _call(L, row_base=(1 << 31) - 10) == -1  # global rows beyond 2^31
    assert L.blp_topk_merge(1 << 20, 1 << 21, 4, 2, 10, 0, 1 << 22, 1 << 23, 0, None) == -1
    assert L.blp_topk_merge(1 << 20, 1 << 21, 4, 2, 10, 257, 1 << 22, 1 << 23, 0, None) == -1
    assert L.blp_topk_merge(1 << 20, 1 << 21, 4, 0, 10, 5, 1 << 22, 1 << 23, 0, None) == -1
    assert L.blp_topk_merge(1 << 20, 1 << 21, 4, 2, 10, 5, None, 1 << 23, 0, None) == -1


# ------------------------------------------------------------------------------------------- gloo ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("rel_model", ["transe", "complex"])
def test_sharded_predict_links_equals_unsharded(tmp_path, world, rel_model):
    import topk_worker
    mp.spawn(topk_worker.run, args=(world, _free_port(), rel_model, str(tmp_path)), nprocs=world, join=True)
    want_rows, want_scores = topk_worker.unsharded(rel_model)
    for r in range(world):
        rows = np.load(tmp_path / f"rows_{r}.npy")
        scores = np.load(tmp_path / f"scores_{r}.npy")
        assert np.array_equal(rows, want_rows.numpy())
        assert np.array_equal(scores.view(np.int32), want_scores.numpy().view(np.int32))
