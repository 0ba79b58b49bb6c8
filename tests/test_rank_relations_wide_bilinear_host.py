"""Relation prediction for DistMult / ComplEx / SimplE at any width -- blp_rank_relations_wide_bilinear /
blp_topk_relations_wide_bilinear (include/blp_hip.h; ops.rank_relations_wide_bilinear / topk_relations_wide_bilinear; the dispatch
of ranking.rank_relations / predict_relations) -- without a GPU: the six entry points are exported and bound with the TransE
wide calls' signatures, which (model, D, k) they take (the existing support tables as they were), the workspace sizes, every
argument refusal of the TransE wide pair case for case (checked before anything touches a device), no scratch memory in the new
kernels, and the CPU route against the C oracle at every branch of the sum order -- with the one known disagreement of the dense
broadcast route (ComplEx / SimplE at D = 12) pinned."""
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
NEW = ("blp_rank_relations_wide_bilinear_supported", "blp_rank_relations_wide_bilinear_workspace_bytes",
       "blp_rank_relations_wide_bilinear", "blp_topk_relations_wide_bilinear_supported",
       "blp_topk_relations_wide_bilinear_workspace_bytes", "blp_topk_relations_wide_bilinear")
BILINEAR = {"distmult": 1, "complex": 2, "simple": 3}
DS = (0, 4, 6, 12, 64, 68, 300, 768, 1024, 1028, -64)
KS = (0, 1, 256, 257)
CPU_WIDTHS = [("distmult", D) for D in (4, 12, 36, 100, 300, 508, 512, 516, 768, 1024)] + \
             [(m, D) for m in ("complex", "simple") for D in (4, 20, 36, 64, 100, 300, 508, 512, 516, 768, 1000, 1024)]


def _L():
    return _lib.lib()


def takes(m, D):
    return m in (1, 2, 3) and 4 <= D <= 1024 and D % 4 == 0


def test_the_six_entry_points_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "blp_hip.h")).read()
    L = _L()
    product, hooks = _exported(_lib.LIB_PATH), _exported(_lib.HOOKS_LIB_PATH)
    for name in NEW:
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert name in product and name in hooks
        wide = getattr(L, name.replace("_wide_bilinear", "_wide"))  # a caller switches by name: the TransE wide entry's signature
        assert getattr(L, name).argtypes is not None
        assert getattr(L, name).argtypes == wide.argtypes and getattr(L, name).restype == wide.restype
    assert L.blp_version() == 60000
    assert _lib.KNOBS[-1] == "topk_sets_grid"
    for f in ("rank_relations_wide_bilinear", "topk_relations_wide_bilinear"):
        assert callable(getattr(ops, f)) and callable(getattr(ops, f + "_supported")) and callable(getattr(ops, f + "_workspace_bytes"))


def test_the_support_tables():
    L = _L()
    for m in (-1, 0, 1, 2, 3, 4, 7):
        for D in DS:
            assert L.blp_rank_relations_wide_bilinear_supported(m, D) == int(takes(m, D)), (m, D)
            for k in KS:
                assert L.blp_topk_relations_wide_bilinear_supported(m, D, k) == int(takes(m, D) and 1 <= k <= 256), (m, D, k)
            # the existing calls answer as before
            fixed, transe = 0 <= m <= 3 and D in (64, 128, 256), m == 0 and 4 <= D <= 1024 and D % 4 == 0
            assert L.blp_rank_relations_supported(m, D) == int(fixed) and L.blp_rank_relations_wide_supported(m, D) == int(transe), (m, D)
            for k in KS:
                assert L.blp_topk_relations_supported(m, D, k) == int(fixed and 1 <= k <= 256), (m, D, k)
                assert L.blp_topk_relations_wide_supported(m, D, k) == int(transe and 1 <= k <= 256), (m, D, k)
    for name in BILINEAR:
        assert ops.rank_relations_wide_bilinear_supported(name, 300) and ops.topk_relations_wide_bilinear_supported(name, 768, 256)
        assert ops.rank_relations_wide_bilinear_supported(name, 128) and not ops.topk_relations_wide_bilinear_supported(name, 768, 257)
        assert not ops.rank_relations_wide_bilinear_supported(name, 302)
    assert not ops.rank_relations_wide_bilinear_supported("transe", 300)
    assert not ops.topk_relations_wide_bilinear_supported("transe", 128, 10)


def test_workspace_sizes():
    """rank: the Q true-relation keys, 4 Q bytes rounded up to 256, whatever R and D; top-k: nothing."""
    L = _L()
    rank = lambda Q, R, m=1, D=300: L.blp_rank_relations_wide_bilinear_workspace_bytes(m, D, Q, R)
    topk = lambda Q, R, k, m=1, D=300: L.blp_topk_relations_wide_bilinear_workspace_bytes(m, D, Q, R, k)
    align = lambda n: (n + 255) // 256 * 256
    Qs, Rs = (0, 1, 7, 8, 9, 63, 64, 65, 1000, 310_116, 1 << 30), (1, 11, 237, 822, (1 << 31) - 1)
    for m in (1, 2, 3):
        for D in (4, 64, 68, 300, 768, 1024):
            for R in Rs:
                assert [rank(Q, R, m, D) for Q in Qs] == [align(4 * Q) for Q in Qs], (m, D, R)
                for k in (1, 10, 64, 256):
                    assert all(topk(Q, R, k, m, D) == 0 for Q in Qs)
    assert rank(100, 5) == 512 and rank(100, 5, D=768) == 512
    # unsupported or negative sizes answer 0
    assert rank(100, 0) == 0 and rank(100, 1 << 31) == 0 and rank(-1, 5) == 0 and rank((1 << 30) + 1, 5) == 0 and rank(100, -3) == 0
    assert rank(100, 5, m=7) == 0 and rank(100, 5, m=0) == 0 and rank(100, 5, m=0, D=128) == 0 and rank(100, 5, D=302) == 0
    assert topk(-1, 5, 10) == 0 and topk(100, -1, 10) == 0 and topk(100, 5, 10, m=0) == 0 and topk(100, 5, 257) == 0
    assert ops.rank_relations_wide_bilinear_workspace_bytes("complex", 300, 100, 5) == 512
    assert ops.rank_relations_wide_bilinear_workspace_bytes("transe", 300, 100, 5) == 0
    assert ops.topk_relations_wide_bilinear_workspace_bytes("simple", 768, 100, 5, 10) == 0


RANK_ARGS = dict(model=1, source=1 << 21, S=1000, D=300, ld_src=300, head_row=1 << 22, tail_row=1 << 23, Q=3, rel_emb=1 << 24, R=11,
                 true_rel=1 << 25, filter=None, counts=1 << 26, scores=1 << 27, ld_scores=11, workspace=1 << 31, ws=1 << 20, device=0,
                 stream=None)
TOPK_ARGS = dict(model=1, source=1 << 21, S=1000, D=300, ld_src=300, head_row=1 << 22, tail_row=1 << 23, Q=3, rel_emb=1 << 24, R=11,
                 k=10, filter=None, rels=1 << 26, scores=1 << 27, workspace=None, ws=0, device=0, stream=None)


def _rank(entry, **over):
    """A ranking entry with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(RANK_ARGS)
    a.update(over)
    f = a["filter"]
    return getattr(_L(), entry)(a["model"], a["source"], a["S"], a["D"], a["ld_src"], a["head_row"], a["tail_row"], a["Q"], a["rel_emb"],
                                a["R"], a["true_rel"], None if f is None else ctypes.byref(f), a["counts"], a["scores"], a["ld_scores"],
                                a["workspace"], a["ws"], a["device"], a["stream"])


def _topk(entry, **over):
    a = dict(TOPK_ARGS)
    a.update(over)
    f = a["filter"]
    return getattr(_L(), entry)(a["model"], a["source"], a["S"], a["D"], a["ld_src"], a["head_row"], a["tail_row"], a["Q"], a["rel_emb"],
                                a["R"], a["k"], None if f is None else ctypes.byref(f), a["rels"], a["scores"], a["workspace"], a["ws"],
                                a["device"], a["stream"])


def _same_refusal(call, new, old, new_model, want, **over):
    """The case through the new entry (its own model) and through the TransE wide entry (model 0): the same status, the same
    message after the entry's own name."""
    L = _L()
    a = call(new, model=new_model, **over)
    msg_new = L.blp_last_error()
    b = call(old, model=0, **over)
    msg_old = L.blp_last_error()
    assert a == b == want, (new, over, a, b)
    assert msg_new.startswith(new.encode() + b":") and msg_old.startswith(old.encode() + b":"), (msg_new, msg_old)
    assert msg_new[len(new):] == msg_old[len(old):], (msg_new, msg_old)
    return msg_new


@pytest.mark.parametrize("model", [1, 2, 3])
def test_bad_arguments_are_refused_as_the_transe_wide_calls_refuse_them(model):
    """This machine has no device: a call that got as far as one would answer BLP_ERR_HIP (-3), never one of these.  The cases
    of test_rank_relations_wide_host.py, each through both entries."""
    L = _L()
    for call, new in ((_rank, "blp_rank_relations_wide_bilinear"), (_topk, "blp_topk_relations_wide_bilinear")):
        old = new.replace("_wide_bilinear", "_wide")
        same = lambda want, **over: _same_refusal(call, new, old, model, want, **over)
        assert call(new, model=7) == -1 and b"unknown model" in L.blp_last_error() and call(new, model=-1) == -1
        for D in (302, 2, 0, 1028, -64, 6):                        # no such width; TransE and everything else: unsupported
            assert call(new, model=model, D=D, ld_src=max(D // 4 * 4 + 4, 8)) == -2 and b"not supported" in L.blp_last_error(), D
            assert L.blp_last_error().startswith(new.encode() + b": D = ")
        for D in (300, 128, 64):
            assert call(new, model=0, D=D) == -2 and b"not supported" in L.blp_last_error(), D
        assert b"R = 0" in same(-1, R=0)
        same(-1, R=-5)
        same(-1, R=1 << 31, ld_scores=1 << 31)
        assert b"negative" in same(-1, Q=-1)
        assert b"2^30" in same(-1, Q=(1 << 30) + 1, k=1)
        same(-1, ld_src=296)
        assert b"aligned" in same(-1, ld_src=302)
        assert b"aligned" in same(-1, source=(1 << 21) + 4)
        same(-1, rel_emb=(1 << 24) + 8)
        for name in ("source", "head_row", "tail_row", "rel_emb"):
            assert b"NULL" in same(-1, **{name: None}), name
        same(-1, S=0)
        # the filter's values are relation ids: no ent2idx, no row_base
        assert b"ent2idx" in same(-1, filter=_lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, 1 << 35, 10, 0))
        assert b"row_base" in same(-1, filter=_lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 100))
        assert b"filter" in same(-1, filter=_lib.BlpFilter(None, 1 << 33, 1 << 34, None, None, 0, 0))
        assert call(new, model=model, Q=0) == 0                      # no query: nothing to do, nothing touched
        assert call(new, model=model, Q=0, source=None, head_row=None, tail_row=None, workspace=None, ws=0) == 0
        for D in (4, 68, 128, 768, 1024):                            # a supported width gets past every check
            assert call(new, model=model, D=D, ld_src=D + 4) == -3, D
    new, old = "blp_rank_relations_wide_bilinear", "blp_rank_relations_wide"
    same = lambda want, **over: _same_refusal(_rank, new, old, model, want, **over)
    assert b"both outputs NULL" in same(-1, counts=None, scores=None)
    assert b"true_rel" in same(-1, true_rel=None)
    assert b"ld_scores" in same(-1, ld_scores=10)
    same(-1, counts=(1 << 26) + 4)
    assert b"aligned" in same(-1, scores=(1 << 27) + 8)
    need = L.blp_rank_relations_wide_bilinear_workspace_bytes(model, 300, 3, 11)
    assert need == 256
    assert b"workspace" in same(-4, workspace=None)
    same(-4, ws=need - 1)
    same(-4, ws=0)
    same(-4, workspace=(1 << 31) + 64)
    # a good filter, and a scores-only call without a workspace, get past every check (and stop at the missing device)
    good = _lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, 1 << 35, None, 0, 0)
    assert _rank(new, model=model, filter=good) == -3
    assert _rank(new, model=model, counts=None, true_rel=None, workspace=None, ws=0) == -3
    new, old = "blp_topk_relations_wide_bilinear", "blp_topk_relations_wide"
    same = lambda want, **over: _same_refusal(_topk, new, old, model, want, **over)
    assert b"k = 0" in same(-1, k=0)
    same(-1, k=257)
    same(-1, k=-3)
    assert b"2^31" in same(-1, Q=1 << 23, k=256)
    assert b"NULL" in same(-1, rels=None)
    same(-1, scores=None)
    same(-1, rels=(1 << 26) + 8)
    assert _topk(new, model=model, filter=good, k=256, R=3) == -3  # k > R is legal; no workspace is asked for


def test_ops_refuse_what_the_library_refuses():
    table = torch.zeros((4, 300))
    z, o = torch.zeros(2, dtype=torch.long), torch.ones(2, dtype=torch.long)
    with pytest.raises(RuntimeError):                                   # ops is device-only: no quiet CPU fallback
        ops.rank_relations_wide_bilinear("distmult", table, z, o, torch.zeros((3, 300)), z)
    with pytest.raises(RuntimeError):
        ops.topk_relations_wide_bilinear("complex", table, z, o, torch.zeros((3, 300)), 2)


def test_new_kernels_use_no_scratch_and_spill_nothing():
    """One code object serves every width (D is a run-time argument of the kernels): no scratch memory, no vector register
    parked outside the register file -- the [query][row] arrays of the pass are never dynamically indexed."""
    from blp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert "rank_rels_wide_bilinear.hip" in build.SOURCES
    for obj_dir in (build.OBJ, os.path.join(build.OBJ, build.HOOKS_VARIANT)):
        kernels = kernel_resources.kernels_of(os.path.join(obj_dir, "rank_rels_wide_bilinear.hip.o"))
        # per model: the true keys; the ranking kernel (counts / scores / both) and the top-k kernel with and without the cascade
        for name, n in (("rel_true_key_wb_kernel", 3), ("rank_rels_wb_kernel", 18), ("topk_rels_wb_kernel", 6)):
            assert len([k for k in kernels if name in k]) == n, name
        assert len(kernels) == 27
        for k, v in kernels.items():
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)
            assert v["vgpr_count"] <= 256, (k, v)  # two waves per SIMD at least
            assert v["group_segment_fixed_size"] == 0, (k, v)  # LDS is dynamic: sized by D (and k) at the launch


# ------------------------------------------------------------------------------------------- the CPU route at the new widths
def spread(x, seed):
    """Every entry gets its own binary exponent over 2^-20 .. 2^20 (spread of test_gpu_rank_sets_wide_bilinear.py): the terms
    of a sum differ by up to 2^120, so any reordering of the additions changes low bits."""
    g = torch.Generator().manual_seed(seed)
    return x * torch.exp2(torch.randint(-20, 21, x.shape, generator=g).float())


def cpu_problem(D, seed):
    N, R, T = 16, 7, 6
    g = torch.Generator().manual_seed(seed)
    table = spread(torch.randn((N, D), generator=g), seed + 1)
    rel_w = spread(torch.randn((R, D), generator=g), seed + 2)
    ent2idx = utils.make_ent2idx(torch.arange(N), N - 1)
    triples = torch.stack((torch.randint(0, N, (T,), generator=g), torch.randint(0, N, (T,), generator=g),
                           torch.randint(0, R, (T,), generator=g)), 1)
    edges = torch.cat((triples, torch.stack((triples[:, 0], triples[:, 1], torch.randint(0, R, (T,), generator=g)), 1)))
    return table, rel_w, ent2idx, triples, edges


@pytest.mark.parametrize("rel_model,D", CPU_WIDTHS)
def test_cpu_route_equals_the_oracle_at_every_branch_of_the_sum_order(oracle, rel_model, D):
    """ranking.rank_relations / predict_relations on CPU tensors (the dense broadcast route, the fused route's yardstick in
    tests/test_gpu_rank_relations_wide_bilinear.py) against the C oracle, bit for bit."""
    table, rel_w, ent2idx, triples, edges = cpu_problem(D, seed=D)
    T, R = triples.shape[0], rel_w.shape[0]
    index = utils.RelationFilterIndex(edges)
    model = make_model(rel_model, rel_w.numpy())
    S = relation_matrix(oracle, rel_model, table[triples[:, 0]].numpy(), table[triples[:, 1]].numpy(), rel_w.numpy())
    known = {}
    for h, t, r in edges.numpy():
        known.setdefault((int(h), int(t)), set()).add(int(r))
    segs = [sorted(known[(int(h), int(t))]) for h, t, _ in triples.numpy()]
    rel = triples[:, 2].numpy()
    for fi, removed in ((None, np.zeros((T, R), bool)), (index, removed_mask(segs, rel, T, R))):
        counts, scores = ranking.rank_relations(model, table, triples, ent2idx, filter_index=fi, return_scores=True)
        assert counts.dtype == torch.int32 and np.array_equal(counts.numpy(), want_counts(S, rel, removed))
        same_scores(scores, S, (rel_model, D))
        for k in (3, R + 2):
            same_topk(ranking.predict_relations(model, table, triples, k, ent2idx, filter_index=fi), want_topk(S, removed, k), k)


@pytest.mark.parametrize("rel_model", ["complex", "simple"])
def test_the_dense_route_disagrees_with_the_oracle_at_d12(oracle, rel_model):
    """The one known exception: at D = 12 (6 terms) torch's broadcast reduction adds the terms in another order than its
    reduction of a single score, which is what the oracle (and the fused kernel) restate.  So D = 12 of these two models is
    tested against the oracle only, never against the dense route; if this assertion starts to fail, torch has changed and the
    exception can leave the docstrings."""
    table, rel_w, ent2idx, triples, _ = cpu_problem(12, seed=12)
    S = relation_matrix(oracle, rel_model, table[triples[:, 0]].numpy(), table[triples[:, 1]].numpy(), rel_w.numpy())
    _, scores = ranking.rank_relations(make_model(rel_model, rel_w.numpy()), table, triples, ent2idx, return_scores=True)
    assert not np.array_equal(scores.numpy().view(np.int32), S.view(np.int32))