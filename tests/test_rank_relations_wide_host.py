"""Relation prediction for TransE at any width -- blp_rank_relations_wide / blp_topk_relations_wide (include/blp_hip.h; ops.
rank_relations_wide / topk_relations_wide; the dispatch of ranking.rank_relations / predict_relations) -- without a GPU: the six
entry points are exported and bound, the narrow pair's support table is as it was, which (model, D, k) the wide pair takes, the
workspace sizes, the argument refusals (the narrow pair's cases, checked before anything touches a device), no scratch memory and
no spills in the new kernels, and the CPU route at D = 300 against the C oracle."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from blp_amd import _lib, ops, ranking, utils
from test_rank_relations_host import (_exported, make_model, relation_matrix, removed_mask, same_scores, same_topk, want_counts,
                                      want_topk)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_rank_relations_wide_supported", "blp_rank_relations_wide_workspace_bytes", "blp_rank_relations_wide",
       "blp_topk_relations_wide_supported", "blp_topk_relations_wide_workspace_bytes", "blp_topk_relations_wide")
WIDE_YES = (4, 64, 68, 128, 300, 768, 1024)
WIDE_NO = (0, 2, 302, 1028)


def _L():
    return _lib.lib()


def test_the_six_entry_points_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "blp_hip.h")).read()
    L = _L()
    product, hooks = _exported(_lib.LIB_PATH), _exported(_lib.HOOKS_LIB_PATH)
    for name in NEW:
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert getattr(L, name).argtypes is not None
        assert name in product and name in hooks
        # a caller switches by name: the narrow entry's signature
        narrow = getattr(L, name.replace("_wide", ""))
        assert getattr(L, name).argtypes == narrow.argtypes and getattr(L, name).restype == narrow.restype
    assert L.blp_version() == 60000
    for f in ("rank_relations_wide", "topk_relations_wide"):
        assert callable(getattr(ops, f)) and callable(getattr(ops, f + "_supported")) and callable(getattr(ops, f + "_workspace_bytes"))


def test_the_narrow_support_table_is_unchanged():
    L = _L()
    for m in range(-1, 5):
        for D in (4, 32, 64, 68, 96, 128, 256, 300, 512, 768, 1024):
            base = 0 <= m <= 3 and D in (64, 128, 256)
            assert bool(L.blp_rank_relations_supported(m, D)) == base, (m, D)
            assert bool(L.blp_topk_relations_supported(m, D, 10)) == base, (m, D)
            assert L.blp_rank_relations_workspace_bytes(m, D, 100, 5) == (512 if base else 0)
    assert not ops.rank_relations_supported("transe", 300) and not ops.topk_relations_supported("transe", 768, 10)


def test_the_wide_support_table():
    L = _L()
    for D in WIDE_YES:
        assert L.blp_rank_relations_wide_supported(0, D) == 1, D
        assert ops.rank_relations_wide_supported("transe", D)
        for k in (1, 10, 256):
            assert L.blp_topk_relations_wide_supported(0, D, k) == 1, (D, k)
        for k in (0, 257, -1):
            assert L.blp_topk_relations_wide_supported(0, D, k) == 0, (D, k)
        assert ops.topk_relations_wide_supported("transe", D, 256) and not ops.topk_relations_wide_supported("transe", D, 257)
    for D in WIDE_NO + (-4, 1, 3, 6, 66, 1023, 2048):
        assert L.blp_rank_relations_wide_supported(0, D) == 0 and L.blp_topk_relations_wide_supported(0, D, 10) == 0, D
    for m in (-1, 1, 2, 3, 4, 7):  # every other model, known or not
        for D in WIDE_YES + WIDE_NO:
            assert L.blp_rank_relations_wide_supported(m, D) == 0 and L.blp_topk_relations_wide_supported(m, D, 10) == 0, (m, D)
    for name in ("distmult", "complex", "simple"):
        assert not ops.rank_relations_wide_supported(name, 300) and not ops.topk_relations_wide_supported(name, 128, 10)


def test_workspace_sizes():
    """rank: the Q true-relation scores, 4 Q bytes rounded up to 256, whatever R and D; top-k: nothing."""
    L = _L()
    rank = lambda Q, R, m=0, D=300: L.blp_rank_relations_wide_workspace_bytes(m, D, Q, R)
    topk = lambda Q, R, k, m=0, D=300: L.blp_topk_relations_wide_workspace_bytes(m, D, Q, R, k)
    align = lambda n: (n + 255) // 256 * 256
    Qs, Rs = (0, 1, 15, 16, 17, 63, 64, 65, 1000, 310_116, 1 << 30), (1, 11, 237, 822, (1 << 31) - 1)
    for D in WIDE_YES:
        for R in Rs:
            assert [rank(Q, R, D=D) for Q in Qs] == [align(4 * Q) for Q in Qs], (D, R)
            for k in (1, 10, 64, 256):
                assert all(topk(Q, R, k, D=D) == 0 for Q in Qs)
    assert rank(100, 5, D=300) == 512 and rank(100, 5, D=768) == 512
    # refusals answer 0
    assert rank(100, 0) == 0 and rank(100, 1 << 31) == 0 and rank(-1, 5) == 0 and rank((1 << 30) + 1, 5) == 0
    assert rank(100, 5, m=7) == 0 and rank(100, 5, m=1) == 0 and rank(100, 5, m=3, D=128) == 0 and rank(100, 5, D=302) == 0
    assert ops.rank_relations_wide_workspace_bytes("transe", 300, 100, 5) == 512
    assert ops.rank_relations_wide_workspace_bytes("distmult", 300, 100, 5) == 0
    assert ops.topk_relations_wide_workspace_bytes("transe", 768, 100, 5, 10) == 0


def _rank(L, **over):
    """blp_rank_relations_wide with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(model=0, source=1 << 21, S=1000, D=300, ld_src=300, head_row=1 << 22, tail_row=1 << 23, Q=3, rel_emb=1 << 24, R=11,
             true_rel=1 << 25, filter=None, counts=1 << 26, scores=1 << 27, ld_scores=11, workspace=1 << 31, ws=1 << 20, device=0,
             stream=None)
    a.update(over)
    f = a["filter"]
    return L.blp_rank_relations_wide(a["model"], a["source"], a["S"], a["D"], a["ld_src"], a["head_row"], a["tail_row"], a["Q"],
                                     a["rel_emb"], a["R"], a["true_rel"], None if f is None else ctypes.byref(f), a["counts"], a["scores"],
                                     a["ld_scores"], a["workspace"], a["ws"], a["device"], a["stream"])


def _topk(L, **over):
    a = dict(model=0, source=1 << 21, S=1000, D=300, ld_src=300, head_row=1 << 22, tail_row=1 << 23, Q=3, rel_emb=1 << 24, R=11,
             k=10, filter=None, rels=1 << 26, scores=1 << 27, workspace=None, ws=0, device=0, stream=None)
    a.update(over)
    f = a["filter"]
    return L.blp_topk_relations_wide(a["model"], a["source"], a["S"], a["D"], a["ld_src"], a["head_row"], a["tail_row"], a["Q"],
                                     a["rel_emb"], a["R"], a["k"], None if f is None else ctypes.byref(f), a["rels"], a["scores"],
                                     a["workspace"], a["ws"], a["device"], a["stream"])


def test_bad_arguments_are_refused_before_a_device_is_touched():
    """This machine has no device: a call that got as far as one would answer BLP_ERR_HIP (-3), never one of these.  The cases
    of test_rank_relations_host.py, at D = 300."""
    L = _L()
    for call in (_rank, _topk):
        assert call(L, model=7) == -1 and b"unknown model" in L.blp_last_error()
        assert call(L, model=-1) == -1
        for m, D in ((0, 302), (0, 2), (0, 0), (0, 1028), (1, 300), (2, 128), (3, 64), (1, 96)):  # the other models: unsupported
            assert call(L, model=m, D=D, ld_src=max(D // 4 * 4 + 4, 8)) == -2 and b"not supported" in L.blp_last_error(), (m, D)
        assert call(L, R=0) == -1 and b"R = 0" in L.blp_last_error()
        assert call(L, R=-5) == -1 and call(L, R=1 << 31, ld_scores=1 << 31) == -1
        assert call(L, Q=-1) == -1 and b"negative" in L.blp_last_error()
        assert call(L, Q=(1 << 30) + 1, k=1) == -1 and b"2^30" in L.blp_last_error()
        assert call(L, ld_src=296) == -1 and call(L, ld_src=302) == -1 and b"aligned" in L.blp_last_error()
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
        for D in (4, 68, 768, 1024):                                  # a supported width gets past every check
            assert call(L, D=D, ld_src=D + 4) == -3, D
    # the ranking entry's own
    assert _rank(L, counts=None, scores=None) == -1 and b"both outputs NULL" in L.blp_last_error()
    assert _rank(L, true_rel=None) == -1 and b"true_rel" in L.blp_last_error()
    assert _rank(L, ld_scores=10) == -1 and b"ld_scores" in L.blp_last_error()
    assert _rank(L, counts=(1 << 26) + 4) == -1 and _rank(L, scores=(1 << 27) + 8) == -1 and b"aligned" in L.blp_last_error()
    need = L.blp_rank_relations_wide_workspace_bytes(0, 300, 3, 11)
    assert need == 256
    assert _rank(L, workspace=None) == -4 and b"workspace" in L.blp_last_error()
    assert _rank(L, ws=need - 1) == -4 and _rank(L, ws=0) == -4 and _rank(L, workspace=(1 << 31) + 64) == -4
    assert b"blp_rank_relations_wide" in L.blp_last_error()  # the messages carry the entry's own name
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


def test_ops_refuse_what_the_library_refuses():
    table = torch.zeros((4, 300))
    with pytest.raises(RuntimeError):                                   # ops is device-only: no quiet CPU fallback
        ops.rank_relations_wide("transe", table, torch.zeros(2, dtype=torch.long), torch.ones(2, dtype=torch.long), torch.zeros((3, 300)),
                                torch.zeros(2, dtype=torch.long))
    with pytest.raises(RuntimeError):
        ops.topk_relations_wide("transe", table, torch.zeros(2, dtype=torch.long), torch.ones(2, dtype=torch.long), torch.zeros((3, 300)), 2)


def test_new_kernels_use_no_scratch_and_spill_nothing():
    """One code object serves every width (D is a run-time argument of the kernels), 300 and 768 included: no scratch memory,
    no vector register parked outside the register file."""
    from blp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    for obj_dir in (build.OBJ, os.path.join(build.OBJ, build.HOOKS_VARIANT)):
        kernels = kernel_resources.kernels_of(os.path.join(obj_dir, "rank_rels_wide.hip.o"))
        # the true keys, the ranking kernel (counts / scores / both), the top-k kernel: none is a template of the width
        for name, n in (("rel_true_key_wide_kernel", 1), ("rank_rels_wide_kernel", 3), ("topk_rels_wide_kernel", 1)):
            assert len([k for k in kernels if name in k]) == n, name
        assert len(kernels) == 5
        for k, v in kernels.items():
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)
            assert v["vgpr_count"] <= 256, (k, v)  # two waves per SIMD at least
        # the register kernels' object is what it was (test_rank_relations_host.py pins its registers)
        assert len(kernel_resources.kernels_of(os.path.join(obj_dir, "rank_rels.hip.o"))) == 72


# ------------------------------------------------------------------------------------------- the CPU route at the new widths
@pytest.mark.parametrize("D", [300, 768])
def test_cpu_route_at_the_wide_widths_is_the_dense_one(oracle, D):
    """ranking.rank_relations / predict_relations on CPU tensors: the dense route, unchanged -- against the C oracle."""
    N, R, T = 40, 9, 14
    g = torch.Generator().manual_seed(D)
    table = torch.randn((N, D), generator=g)
    rel_w = torch.randn((R, D), generator=g)
    ent2idx = utils.make_ent2idx(torch.arange(N), N - 1)
    triples = torch.stack((torch.randint(0, N, (T,), generator=g), torch.randint(0, N, (T,), generator=g),
                           torch.randint(0, R, (T,), generator=g)), 1)
    edges = torch.cat((triples, torch.stack((triples[:, 0], triples[:, 1], torch.randint(0, R, (T,), generator=g)), 1)))
    index = utils.RelationFilterIndex(edges)
    model = make_model("transe", rel_w.numpy())
    S = relation_matrix(oracle, "transe", table[triples[:, 0]].numpy(), table[triples[:, 1]].numpy(), rel_w.numpy())
    known = {}
    for h, t, r in edges.numpy():
        known.setdefault((int(h), int(t)), set()).add(int(r))
    segs = [sorted(known[(int(h), int(t))]) for h, t, _ in triples.numpy()]
    rel = triples[:, 2].numpy()
    for fi, removed in ((None, np.zeros((T, R), bool)), (index, removed_mask(segs, rel, T, R))):
        counts, scores = ranking.rank_relations(model, table, triples, ent2idx, filter_index=fi, return_scores=True)
        assert counts.dtype == torch.int32 and np.array_equal(counts.numpy(), want_counts(S, rel, removed))
        same_scores(scores, S)
        for k in (1, 4, R + 2):
            same_topk(ranking.predict_relations(model, table, triples, k, ent2idx, filter_index=fi), want_topk(S, removed, k), k)
