"""Relation prediction -- (h, ?, t) against every row of rel_emb -- without a GPU (include/blp_hip.h: blp_rank_relations,
blp_topk_relations; ops.rank_relations / topk_relations; utils.RelationFilterIndex; ranking.rank_relations /
predict_relations): the entry points are exported and bound, which (model, D, k) they take, the workspace formula, the argument
refusals (checked before anything touches a device), no scratch memory in the new kernels and the other objects' kernels as they
were, the pair index against a brute-force dict, and the CPU route -- the oracle of the fused one -- against the C oracle's
score of every expanded (pair, relation) plus numpy's stable order.  The helpers at the top are shared with
tests/test_gpu_rank_relations.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden, golden_names
from blp_amd import _lib, models, ops, ranking, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_rank_relations_supported", "blp_rank_relations_workspace_bytes", "blp_rank_relations",
       "blp_topk_relations_supported", "blp_topk_relations_workspace_bytes", "blp_topk_relations")
NAN_BITS = 0x7fc00000


# ------------------------------------------------------------------------------------------- the contract, spelled out in numpy
def relation_matrix(oracle, rel_model, head_vecs, tail_vecs, rel_w):
    """(Q, R) f32: the C oracle's score of every expanded (pair q, relation r) -- Q x R calls' worth of score_pairs."""
    Q, R = head_vecs.shape[0], rel_w.shape[0]
    h = np.ascontiguousarray(np.repeat(head_vecs, R, axis=0))
    t = np.ascontiguousarray(np.repeat(tail_vecs, R, axis=0))
    r = np.ascontiguousarray(np.tile(rel_w, (Q, 1)))
    return oracle.score_pairs(rel_model, h, t, r).reshape(Q, R)


def removed_mask(segments, exclude, Q, R):
    """segments: per query the relation ids its filter names; exclude: per query the id never removed (or -1)."""
    m = np.zeros((Q, R), bool)
    for q, seg in enumerate(segments):
        for v in seg:
            if 0 <= v < R and v != exclude[q]:
                m[q, v] = True
    return m


def want_counts(S, true_rel, removed):
    with np.errstate(invalid="ignore"):
        kt = S[np.arange(len(S)), true_rel][:, None]
        gt, ge = S > kt, S >= kt
        return np.stack((gt.sum(1), ge.sum(1), (gt & ~removed).sum(1), (ge & ~removed).sum(1)), 1).astype(np.int32)


def want_topk(S, removed, k):
    """Per query the relations the filter leaves, ascending id, a stable argsort(-score) -- numpy puts NaN last --, the first
    k; -1 / NaN beyond."""
    Q, R = S.shape
    rels = np.full((Q, k), -1, np.int64)
    scores = np.full((Q, k), np.nan, np.float32)
    for q in range(Q):
        ids = np.nonzero(~removed[q])[0]
        order = np.argsort(-S[q, ids], kind="stable")[:k]
        rels[q, :len(order)], scores[q, :len(order)] = ids[order], S[q, ids][order]
    return rels, scores


def same_topk(got, want, what=""):
    rels, scores = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in got)
    assert rels.dtype == np.int64 and scores.dtype == np.float32 and rels.shape == want[0].shape, what
    assert np.array_equal(rels, want[0]), what
    nan = np.isnan(want[1])
    assert np.array_equal(np.isnan(scores), nan), what
    assert np.array_equal(scores[~nan].view(np.int32), want[1][~nan].view(np.int32)), what
    assert (np.isnan(scores[rels < 0])).all(), what


def same_scores(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    nan = np.isnan(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32)), what


def make_model(rel_model, rel_w):
    m = models.LinkPrediction(rel_w.shape[1], rel_model, "margin", rel_w.shape[0], 0)
    with torch.no_grad():
        m.rel_emb.weight.copy_(torch.from_numpy(rel_w))
    return m


# ------------------------------------------------------------------------------------------- the C-ABI
def _L():
    return _lib.lib()


def _exported(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines()}


def test_new_entry_points_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "blp_hip.h")).read()
    L = _L()
    product, hooks = _exported(_lib.LIB_PATH), _exported(_lib.HOOKS_LIB_PATH)
    for name in NEW:
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert getattr(L, name).argtypes is not None
        assert name in product and name in hooks
    assert L.blp_version() == 60000
    for f in ("rank_relations", "topk_relations"):
        assert callable(getattr(ops, f)) and callable(getattr(ops, f + "_supported")) and callable(getattr(ops, f + "_workspace_bytes"))
    assert callable(ranking.rank_relations) and callable(ranking.predict_relations) and callable(utils.RelationFilterIndex)


def test_supported_grid():
    L = _L()
    for m in range(-1, 5):
        for D in (32, 64, 96, 128, 256, 300, 512):
            base = 0 <= m <= 3 and D in (64, 128, 256)
            assert bool(L.blp_rank_relations_supported(m, D)) == base, (m, D)
            for k in (0, 1, 256, 257):
                assert bool(L.blp_topk_relations_supported(m, D, k)) == (base and 1 <= k <= 256), (m, D, k)
    assert ops.rank_relations_supported("complex", 128) and not ops.rank_relations_supported("transe", 300)
    assert ops.topk_relations_supported("simple", 64, 256) and not ops.topk_relations_supported("simple", 64, 257)


def test_workspace_formula():
    """rank: the Q true-relation scores, 4 Q bytes rounded up to 256, whatever R; top-k: nothing (the header says why)."""
    L = _L()
    rank = lambda Q, R, m=0, D=128: L.blp_rank_relations_workspace_bytes(m, D, Q, R)
    topk = lambda Q, R, k, m=0, D=128: L.blp_topk_relations_workspace_bytes(m, D, Q, R, k)
    align = lambda n: (n + 255) // 256 * 256
    Qs, Rs, ks = (0, 1, 63, 64, 65, 1000, 310_116, 1_000_000, 1 << 30), (1, 11, 237, 822, (1 << 31) - 1), (1, 10, 64, 256)
    for R in Rs:
        sizes = [rank(Q, R) for Q in Qs]
        assert sizes == [align(4 * Q) for Q in Qs] and sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
        for m, D in ((1, 64), (2, 256), (3, 128)):
            assert [rank(Q, R, m, D) for Q in Qs] == sizes
    for Q in Qs:
        sizes = [rank(Q, R) for R in Rs]
        assert sizes == sorted(sizes)
        for k in ks:
            assert all(topk(Q, R, k) == 0 for R in Rs)
    # refusals answer 0
    assert rank(100, 0) == 0 and rank(100, 1 << 31) == 0 and rank(-1, 5) == 0 and rank((1 << 30) + 1, 5) == 0
    assert rank(100, 5, m=7) == 0 and rank(100, 5, D=300) == 0 and rank(100, 5) == 512
    assert ops.rank_relations_workspace_bytes("transe", 128, 100, 5) == 512 and ops.topk_relations_workspace_bytes("transe", 128, 100, 5, 10) == 0


def _rank(L, **over):
    """blp_rank_relations with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(model=0, source=1 << 21, S=1000, D=128, ld_src=128, head_row=1 << 22, tail_row=1 << 23, Q=3, rel_emb=1 << 24, R=11,
             true_rel=1 << 25, filter=None, counts=1 << 26, scores=1 << 27, ld_scores=11, workspace=1 << 31, ws=1 << 20, device=0,
             stream=None)
    a.update(over)
    f = a["filter"]
    return L.blp_rank_relations(a["model"], a["source"], a["S"], a["D"], a["ld_src"], a["head_row"], a["tail_row"], a["Q"], a["rel_emb"],
                                a["R"], a["true_rel"], None if f is None else ctypes.byref(f), a["counts"], a["scores"], a["ld_scores"],
                                a["workspace"], a["ws"], a["device"], a["stream"])


def _topk(L, **over):
    a = dict(model=0, source=1 << 21, S=1000, D=128, ld_src=128, head_row=1 << 22, tail_row=1 << 23, Q=3, rel_emb=1 << 24, R=11,
             k=10, filter=None, rels=1 << 26, scores=1 << 27, workspace=None, ws=0, device=0, stream=None)
    a.update(over)
    f = a["filter"]
    return L.blp_topk_relations(a["model"], a["source"], a["S"], a["D"], a["ld_src"], a["head_row"], a["tail_row"], a["Q"], a["rel_emb"],
                                a["R"], a["k"], None if f is None else ctypes.byref(f), a["rels"], a["scores"], a["workspace"], a["ws"],
                                a["device"], a["stream"])


def test_bad_arguments_are_refused_before_a_device_is_touched():
    """This machine has no device: a call that got as far as one would answer BLP_ERR_HIP (-3), never one of these."""
    L = _L()
    for call in (_rank, _topk):
        assert call(L, model=7) == -1 and b"unknown model" in L.blp_last_error()
        assert call(L, model=-1) == -1
        for m, D in ((0, 300), (1, 96), (2, 32), (3, 512), (0, 0)):
            assert call(L, model=m, D=D, ld_src=max(D, 8)) == -2 and b"not supported" in L.blp_last_error(), (m, D)
        assert call(L, R=0) == -1 and b"R = 0" in L.blp_last_error()
        assert call(L, R=-5) == -1 and call(L, R=1 << 31, ld_scores=1 << 31) == -1
        assert call(L, Q=-1) == -1 and b"negative" in L.blp_last_error()
        assert call(L, Q=(1 << 30) + 1, k=1) == -1 and b"2^30" in L.blp_last_error()
        assert call(L, ld_src=64) == -1 and call(L, ld_src=130) == -1 and b"aligned" in L.blp_last_error()
        assert call(L, source=(1 << 21) + 4) == -1 and b"aligned" in L.blp_last_error()
        assert call(L, rel_emb=(1 << 24) + 8) == -1
        for name in ("source", "head_row", "tail_row", "rel_emb"):
            assert call(L, **{name: None}) == -1 and b"NULL" in L.blp_last_error(), name
        assert call(L, S=0) == -1
        # the filter's values are relation ids: no ent2idx, no row_base
        assert call(L, filter=_lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, 1 << 35, 10, 0)) == -1 and b"ent2idx" in L.blp_last_error()
        assert call(L, filter=_lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 100)) == -1 and b"row_base" in L.blp_last_error()
        assert call(L, filter=_lib.BlpFilter(None, 1 << 33, 1 << 34, None, None, 0, 0)) == -1 and b"filter" in L.blp_last_error()
        assert call(L, Q=0) == 0                                      # no query: nothing to do, nothing touched
        assert call(L, Q=0, source=None, head_row=None, tail_row=None, workspace=None, ws=0) == 0
    # the ranking entry's own
    assert _rank(L, counts=None, scores=None) == -1 and b"both outputs NULL" in L.blp_last_error()
    assert _rank(L, true_rel=None) == -1 and b"true_rel" in L.blp_last_error()
    assert _rank(L, ld_scores=10) == -1 and b"ld_scores" in L.blp_last_error()
    assert _rank(L, counts=(1 << 26) + 4) == -1 and _rank(L, scores=(1 << 27) + 8) == -1 and b"aligned" in L.blp_last_error()
    need = L.blp_rank_relations_workspace_bytes(0, 128, 3, 11)
    assert need == 256
    assert _rank(L, workspace=None) == -4 and b"workspace" in L.blp_last_error()
    assert _rank(L, ws=need - 1) == -4 and _rank(L, ws=0) == -4 and _rank(L, workspace=(1 << 31) + 64) == -4
    # a good filter, and a scores-only call without a workspace, get past every check (and stop at the missing device)
    good = _lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, 1 << 35, None, 0, 0)
    assert _rank(L, filter=good) == -3 and _rank(L, counts=None, true_rel=None, workspace=None, ws=0) == -3
    # the top-k entry's own
    assert _topk(L, k=0) == -1 and b"k = 0" in L.blp_last_error()
    assert _topk(L, k=257) == -1 and _topk(L, k=-3) == -1
    assert _topk(L, Q=1 << 23, k=256) == -1 and b"2^31" in L.blp_last_error()
    assert _topk(L, rels=None) == -1 and b"NULL" in L.blp_last_error()
    assert _topk(L, scores=None) == -1 and _topk(L, rels=(1 << 26) + 8) == -1
    assert _topk(L, filter=good, k=256, R=3) == -3  # k > R is legal; no workspace is asked for


def test_new_kernels_use_no_scratch_and_the_other_objects_keep_their_kernels():
    from blp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    for obj_dir in (build.OBJ, os.path.join(build.OBJ, build.HOOKS_VARIANT)):
        kernels = kernel_resources.kernels_of(os.path.join(obj_dir, "rank_rels.hip.o"))
        # 4 models x 3 widths of: the true keys, the ranking kernel (counts / scores / both), the top-k kernel, its re-score
        for name, n in (("rel_true_key_kernel", 12), ("rank_rels_kernel", 36), ("topk_rels_kernel", 12), ("topk_rels_rescore_kernel", 12)):
            assert len([k for k in kernels if name in k]) == n, name
        assert len(kernels) == 72
        assert all(v["private_segment_fixed_size"] == 0 for v in kernels.values()), [k for k, v in kernels.items() if v["private_segment_fixed_size"]]
        # up to D = 128 nothing is even parked outside the vector registers (DESIGN 4.12 lists the D = 256 figures)
        narrow = {k: v for k, v in kernels.items() if "Li256E" not in k and ", 256" not in k}
        assert len(narrow) == 48 and all(v["vgpr_spill_count"] == 0 for v in narrow.values())
        # what the neighbouring host tests pin for the objects whose headers this one includes
        assert len(kernel_resources.kernels_of(os.path.join(obj_dir, "lists_topk.hip.o"))) == 30
        assert len(kernel_resources.kernels_of(os.path.join(obj_dir, "rank_lists.hip.o"))) == 40
        assert len(kernel_resources.kernels_of(os.path.join(obj_dir, "topk.hip.o"))) == 12 + 24 + 36 + 2
        assert len(kernel_resources.kernels_of(os.path.join(obj_dir, "topk_sets.hip.o"))) == 13


# ------------------------------------------------------------------------------------------- RelationFilterIndex
def test_relation_filter_index_against_a_dict():
    rng = np.random.default_rng(3)
    edges = np.stack((rng.integers(0, 9, 300), rng.integers(0, 9, 300), rng.integers(0, 7, 300)), 1)
    edges = np.concatenate((edges, edges[:40]))  # parallel edges
    known = {}
    for h, t, r in edges:
        known.setdefault((int(h), int(t)), set()).add(int(r))
    assert max(len(v) for v in known.values()) >= 3
    index = utils.RelationFilterIndex(torch.from_numpy(edges))
    assert index.values.shape[0] == sum(len(v) for v in known.values())
    queries = np.array([(h, t, r) for h in range(-1, 11) for t in range(0, 10) for r in (0, 6)], np.int64)
    for cols in (3, 2):
        seg = index.segments(torch.from_numpy(queries[:, :cols]), "cpu")
        assert seg.ent2idx is None and seg.row_base == 0
        lo, hi, values, exclude = (x.numpy() for x in (seg.seg_lo, seg.seg_hi, seg.values, seg.exclude))
        for q, (h, t, r) in enumerate(queries):
            got = values[lo[q]:hi[q]].tolist()
            assert got == sorted(known.get((int(h), int(t)), ())), (h, t)
            assert exclude[q] == (r if cols == 3 else -1)
    empty = utils.RelationFilterIndex(torch.zeros((0, 3), dtype=torch.long))
    seg = empty.segments(torch.from_numpy(queries), "cpu")
    assert bool((seg.seg_lo == seg.seg_hi).all())


# ------------------------------------------------------------------------------------------- the CPU route against the oracle
@pytest.fixture(scope="module", params=REL_MODELS)
def toy(request, oracle):
    """The toy evaluation's table, triples and graph, and the oracle's (T, R) relation score matrix, computed once."""
    rel_model = request.param
    g, f = golden(f"eval_toy_{rel_model}"), golden("filters_toy")
    table, rel_w, triples, ent2idx, edges = g["ent_emb"], g["rel_w"], f["triples"], f["ent2idx"], f["graph_edges"]
    assert (ent2idx < 0).any()  # entity ids go through a map with holes
    h_row, t_row = ent2idx[triples[:, 0]], ent2idx[triples[:, 1]]
    S = relation_matrix(oracle, rel_model, table[h_row], table[t_row], rel_w)
    known = {}
    for h, t, r in np.concatenate((edges, triples)):  # the evaluated triples are known edges too: every query's filter bites
        known.setdefault((int(h), int(t)), set()).add(int(r))
    segs = [sorted(known[(int(h), int(t))]) for h, t, _ in triples]
    return dict(rel_model=rel_model, model=make_model(rel_model, rel_w), table=torch.from_numpy(table), triples=torch.from_numpy(triples),
                ent2idx=torch.from_numpy(ent2idx), S=S, segs=segs, R=rel_w.shape[0],
                index=utils.RelationFilterIndex(torch.from_numpy(np.concatenate((edges, triples)))))


@pytest.mark.parametrize("filtered", [False, True])
def test_cpu_route_against_the_oracle(toy, filtered):
    T, R, S = toy["triples"].shape[0], toy["R"], toy["S"]
    rel = toy["triples"][:, 2].numpy()
    args = (toy["model"], toy["table"], toy["triples"], toy["ent2idx"])
    index = toy["index"] if filtered else None
    removed = removed_mask(toy["segs"], rel, T, R) if filtered else np.zeros((T, R), bool)
    if filtered:
        assert removed.any(), "the filter must bite somewhere"
    counts, scores = ranking.rank_relations(*args, filter_index=index, return_scores=True)
    assert counts.dtype == torch.int32 and np.array_equal(counts.numpy(), want_counts(S, rel, removed))
    same_scores(scores, S)
    assert np.array_equal(ranking.rank_relations(*args, filter_index=index).numpy(), counts.numpy())
    assert bool((counts[:, 1] >= 1).all())  # the true relation counts itself
    pairs3 = (toy["model"], toy["table"], toy["triples"])
    for k in (1, 3, R, R + 4):
        same_topk(ranking.predict_relations(*pairs3, k, toy["ent2idx"], filter_index=index), want_topk(S, removed, k), k)
    if filtered:  # two columns (or -1 in the third): every known relation of the pair goes
        everything = removed_mask(toy["segs"], np.full(T, -1), T, R)
        assert everything.sum() > removed.sum()
        got = ranking.predict_relations(toy["model"], toy["table"], toy["triples"][:, :2], 3, toy["ent2idx"], filter_index=index)
        same_topk(got, want_topk(S, everything, 3))
        minus = toy["triples"].clone()
        minus[:, 2] = -1
        same_topk(ranking.predict_relations(toy["model"], toy["table"], minus, 3, toy["ent2idx"], filter_index=index), want_topk(S, everything, 3))
    # a tiny byte budget takes the piece loop of the dense route
    hv, tv = toy["table"][toy["ent2idx"][toy["triples"][:, 0]]], toy["table"][toy["ent2idx"][toy["triples"][:, 1]]]
    rel_w = toy["model"].rel_emb.weight.detach()
    pieces = list(ranking._relation_scores_dense(toy["model"].score_fn, hv, tv, rel_w, max_bytes=3 * 4 * R * hv.shape[1]))
    assert len(pieces) == -(-T // 3)
    same_scores(torch.cat([p[2] for p in pieces]), S)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16_bit_cpu_table_equals_its_widened_copy(toy, dtype):
    t16 = toy["table"].to(dtype)
    for index in (None, toy["index"]):
        a = ranking.rank_relations(toy["model"], t16, toy["triples"], toy["ent2idx"], filter_index=index, return_scores=True)
        b = ranking.rank_relations(toy["model"], t16.float(), toy["triples"], toy["ent2idx"], filter_index=index, return_scores=True)
        assert np.array_equal(a[0].numpy(), b[0].numpy()) and a[1].dtype == torch.float32
        same_scores(a[1], b[1].numpy())
        same_topk(ranking.predict_relations(toy["model"], t16, toy["triples"], 4, toy["ent2idx"], filter_index=index),
                  tuple(x.numpy() for x in ranking.predict_relations(toy["model"], t16.float(), toy["triples"], 4, toy["ent2idx"], filter_index=index)))


def test_argument_errors(toy):
    m, table, triples, e2i = toy["model"], toy["table"], toy["triples"], toy["ent2idx"]
    with pytest.raises(ValueError):
        ranking.rank_relations(m, table, triples[:, :2], e2i)          # the true relation is missing
    with pytest.raises(ValueError):
        ranking.predict_relations(m, table, triples[:, :1], 3, e2i)
    with pytest.raises(ValueError):
        ranking.predict_relations(m, table, triples, 0, e2i)
    bad = triples.clone()
    bad[0, 2] = toy["R"]
    with pytest.raises(ValueError):
        ranking.rank_relations(m, table, bad, e2i)
    bad = triples.clone()
    bad[0, 0] = int(np.nonzero(e2i.numpy() < 0)[0][0])                 # an entity without a row
    with pytest.raises(ValueError):
        ranking.rank_relations(m, table, bad, e2i)
    with pytest.raises(ValueError):
        ranking.predict_relations(m, table, bad, 3, e2i)
    with pytest.raises(RuntimeError):                                   # ops is device-only: no quiet CPU fallback
        ops.rank_relations(toy["rel_model"], table, triples[:, 0], triples[:, 1], m.rel_emb.weight.detach(), triples[:, 2])


# ------------------------------------------------------------------------------------------- anchored to the reference's outputs
@pytest.mark.parametrize("name", golden_names("scores_"))
def test_true_relation_column_equals_the_goldens_true_triple_score(name):
    """Column rels[q] of the relation score matrix is the score of the true triple -- which the golden holds as
    head_pred[q, heads[q]], computed by the reference."""
    g = golden(name)
    rel_model = name.split("_")[1]
    heads, tails, rels = g["heads"][:, 0], g["tails"][:, 0], g["rels"][:, 0]
    triples = torch.from_numpy(np.stack((heads, tails, rels), 1).astype(np.int64))
    N = g["table"].shape[0]
    counts, scores = ranking.rank_relations(make_model(rel_model, g["rel_w"]), torch.from_numpy(g["table"]), triples, torch.arange(N),
                                            return_scores=True)
    q = np.arange(len(heads))
    same_scores(scores.numpy()[q, rels], g["head_pred"][q, heads], name)
    same_scores(scores.numpy()[q, rels], g["tail_pred"][q, tails], name)
