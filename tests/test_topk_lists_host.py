"""Filtered top-k inside per-query candidate lists, without a GPU (include/blp_hip.h: blp_topk_lists_supported,
blp_topk_lists_workspace_bytes, blp_topk_lists; ranking.predict_from_candidates): the entry points are exported and bound,
which (model, dtype, D, k) they take, the workspace and the slab rule behind it, the argument refusals (checked before anything
touches a device), no scratch memory in the new kernels, the kernels of the neighbouring objects as they were, and the CPU route
of predict_from_candidates -- the oracle of the fused one -- against a brute-force numpy order on the C oracle's score matrix."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REL_MODELS
from blp_amd import _lib, ops, ranking
from test_rank_lists_host import toy  # noqa: F401  (the toy evaluation with the oracle's (2 T, N) score matrix and filter masks)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_topk_lists_supported", "blp_topk_lists_workspace_bytes", "blp_topk_lists")


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
    assert callable(ops.topk_lists) and callable(ops.topk_lists_supported) and callable(ops.topk_lists_workspace_bytes)
    assert callable(ranking.predict_from_candidates)


def test_supported_grid_is_rank_lists_times_k():
    L = _L()
    for m in range(-1, 5):
        for dt in range(-1, 4):
            for D in (4, 32, 64, 96, 100, 128, 256, 300, 302, 512, 768, 1024, 1028):
                base = bool(L.blp_rank_lists_supported(m, dt, D))
                for k in (1, 2, 64, 65, 255, 256):
                    assert bool(L.blp_topk_lists_supported(m, dt, D, k)) == base, (m, dt, D, k)
                for k in (0, 257, -1, 1 << 20):
                    assert not L.blp_topk_lists_supported(m, dt, D, k), (m, dt, D, k)
    assert ops.topk_lists_supported("transe", 300, 10) and ops.topk_lists_supported("transe", 768, 256, torch.bfloat16)
    assert ops.topk_lists_supported("simple", 256, 1, torch.float16) and not ops.topk_lists_supported("simple", 96, 10)
    assert not ops.topk_lists_supported("transe", 128, 257) and not ops.topk_lists_supported("transe", 128, 10, torch.float64)


def slabs(Q, nnz):
    """The header's rule: 1 once the queries alone give 2 048 waves; else enough slabs to get there, at most one per four
    64-entry steps of the mean list, at most 256."""
    if Q >= 2048:
        return 1
    mean_steps = -(-nnz // (64 * Q))
    return min(-(-2048 // Q), max(1, -(-mean_steps // 4)), 256)


def test_workspace_follows_the_slab_rule():
    L = _L()
    ws = lambda Q, nnz, k, m=0, dt=0, D=128, qh=None: L.blp_topk_lists_workspace_bytes(m, dt, D, Q // 2 if qh is None else qh,
                                                                                      Q - (Q // 2 if qh is None else qh), nnz, k)
    align = lambda n: (n + 255) // 256 * 256
    # the issue's example: Q = 3, nnz = 5 070, k = 10 -> S = 7
    assert slabs(3, 5070) == 7 and ws(3, 5070, 10) == align(3 * 7 * 10 * 8)
    # S = 1: no workspace -- many queries whatever the lists, few queries with short lists
    for Q, nnz in ((2048, (1 << 31) - 1), (4096, 4_096_000), (105_740, 52_870_000), (1, 256), (3, 3 * 256), (12, 3000), (5, 0)):
        assert slabs(Q, nnz) == 1 and ws(Q, nnz, 10) == 0, (Q, nnz)
    # the formula everywhere else, for every model / dtype / width alike, and however the queries split into sides
    for Q in (1, 2, 3, 7, 100, 1000, 2047):
        for nnz in (257 * Q, 1000 * Q, 5070, 1_000_000, (1 << 31) - 1):
            for k in (1, 10, 64, 65, 256):
                S = slabs(Q, nnz)
                want = align(Q * S * k * 8) if S > 1 else 0
                assert ws(Q, nnz, k) == want, (Q, nnz, k, S)
                assert ws(Q, nnz, k, m=2, dt=1, D=256) == want and ws(Q, nnz, k, m=0, dt=2, D=300, qh=0) == want
                assert ws(Q, nnz, k, qh=Q) == want
                assert want % 256 == 0 and want < 4096 * k * 8 + 256  # fewer than 4 096 lists of k keys whatever nnz
    # monotone in nnz and in k at fixed Q (S never shrinks with nnz; the bytes are linear in k)
    for Q in (1, 3, 100, 2047):
        sizes = [ws(Q, nnz, 10) for nnz in (0, 64, 256 * Q, 257 * Q, 1000 * Q, 5000 * Q, 100_000 * Q, (1 << 31) - 1)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0], (Q, sizes)
        sizes = [ws(Q, 5000 * Q, k) for k in (1, 2, 10, 64, 65, 128, 256)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0], (Q, sizes)
    # monotone in Q for lists of one length (more queries of the same kind) while the MEAN LIST decides S (ceil(steps / 4) <=
    # ceil(2048 / Q)): Q x S grows with Q there.  Outside that regime the rule itself is not monotone in Q, and the three
    # ways it is not are pinned here as facts of the contract (the call sizes its workspace per call):
    #   at fixed nnz more queries mean shorter lists and fewer slabs (5 070 entries: Q = 3 -> 21 lists, Q = 4 -> 20);
    #   where Q decides, Q x ceil(2048 / Q) wobbles between 2 048 and 2 048 + Q (Q = 9 -> 2 052 lists, Q = 16 -> 2 048);
    #   from Q = 2 048 on S = 1 and the workspace is 0 again.
    for per_list, q_sweep in ((1000, (1, 2, 3, 8, 50, 128, 400, 512)), (5000, (1, 2, 3, 8, 50, 102)), (100_000, (1, 2, 3, 5, 8))):
        assert all(slabs(Q, per_list * Q) == min(-(-(-(-per_list // 64)) // 4), 256) for Q in q_sweep)
        sizes = [ws(Q, per_list * Q, 10) for Q in q_sweep]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0], (per_list, sizes)
    assert ws(3, 5070, 64) > ws(4, 5070, 64) > 0
    assert ws(9, 9_000_000, 10) > ws(16, 16_000_000, 10) > 0
    assert ws(2047, 2047 * 1000, 10) > 0 and ws(2048, 2048 * 1000, 10) == 0
    # refusals answer 0
    assert ws(3, 5070, 0) == 0 and ws(3, 5070, 257) == 0 and ws(3, -1, 10) == 0 and ws(3, 1 << 31, 10) == 0
    assert ws(3, 5070, 10, m=7) == 0 and ws(3, 5070, 10, dt=3) == 0 and ws(3, 5070, 10, dt=-1) == 0 and ws(3, 5070, 10, m=1, D=300) == 0
    assert L.blp_topk_lists_workspace_bytes(0, 0, 128, -1, 4, 5070, 10) == 0 and L.blp_topk_lists_workspace_bytes(0, 0, 128, 4, -1, 5070, 10) == 0
    assert ops.topk_lists_workspace_bytes("transe", 128, 1, 2, 5070, 10) == ws(3, 5070, 10)
    assert ops.topk_lists_workspace_bytes("transe", 128, 1, 2, 5070, 10, torch.float64) == 0


def _call(L, **over):
    """blp_topk_lists with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(model=0, table=1 << 20, dtype=0, N=1000, D=128, ld=128, row_base=0, source=1 << 21, S=1000, ld_src=128, fixed_row=1 << 22,
             rel_emb=1 << 23, R=5, rel_id=1 << 24, q_head=2, q_tail=1, list_ptr=1 << 26, list_row=1 << 27, nnz=5070, k=10,
             filter=None, rows=1 << 30, scores=1 << 25, workspace=1 << 31, ws=1 << 24, device=0, stream=None)
    a.update(over)
    f = a["filter"]
    return L.blp_topk_lists(a["model"], a["table"], a["dtype"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"], a["ld_src"],
                            a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["q_head"], a["q_tail"], a["list_ptr"], a["list_row"],
                            a["nnz"], a["k"], None if f is None else ctypes.byref(f), a["rows"], a["scores"], a["workspace"], a["ws"],
                            a["device"], a["stream"])


def test_bad_arguments_are_refused_before_a_device_is_touched():
    """This machine has no device: a call that got as far as one would answer BLP_ERR_HIP (-3), never one of these."""
    L = _L()
    assert _call(L, model=7) == -1 and b"unknown model" in L.blp_last_error()
    assert _call(L, model=-1) == -1
    assert _call(L, dtype=3) == -1 and b"dtype" in L.blp_last_error()
    assert _call(L, dtype=-1) == -1
    assert _call(L, k=0) == -1 and b"k = 0" in L.blp_last_error()
    assert _call(L, k=257) == -1 and _call(L, k=-3) == -1
    for m, D in ((1, 300), (2, 96), (3, 32), (0, 302), (0, 1028), (0, 0)):
        assert _call(L, model=m, D=D, ld=max(D, 8), ld_src=max(D, 8)) == -2 and b"not supported" in L.blp_last_error(), (m, D)
    for name in ("N", "q_head", "q_tail", "nnz", "row_base"):
        assert _call(L, **{name: -1}) == -1 and b"negative" in L.blp_last_error(), name
    # Q x k < 2^31, Q <= 2^30, nnz < 2^31, global rows <= 2^31
    assert _call(L, q_head=1 << 23, q_tail=0, k=256) == -1 and b"2^31" in L.blp_last_error()
    assert _call(L, q_head=(1 << 23) - 1, q_tail=0, k=256, workspace=None, ws=0, rows=None) == -1 and b"NULL rows" in L.blp_last_error()
    assert _call(L, q_head=(1 << 31) // 10 + 1, q_tail=0, k=10) == -1 and b"2^31" in L.blp_last_error()
    assert _call(L, q_head=(1 << 30) + 1, q_tail=0, k=1) == -1 and b"2^30" in L.blp_last_error()
    assert _call(L, nnz=1 << 31) == -1 and b"nnz" in L.blp_last_error()
    assert _call(L, row_base=(1 << 31) - 10) == -1 and b"2^31" in L.blp_last_error()
    # alignment: f32 rows ld % 4, 16-bit rows ld % 8 (in elements), 16-byte bases
    assert _call(L, ld=130) == -1 and b"aligned" in L.blp_last_error()
    assert _call(L, ld=64) == -1 and _call(L, ld_src=130) == -1 and _call(L, ld_src=64) == -1
    assert _call(L, table=(1 << 20) + 8) == -1 and b"aligned" in L.blp_last_error()
    assert _call(L, source=(1 << 21) + 4) == -1 and _call(L, rel_emb=(1 << 23) + 8) == -1
    for dt in (1, 2):
        assert _call(L, dtype=dt, ld=132) == -1 and b"ld % 8" in L.blp_last_error(), dt
        assert _call(L, dtype=dt, ld=136, workspace=None) == -4, dt  # D + 8 is a 16-bit table's stride: passes, stops at the workspace
    assert _call(L, rows=None) == -1 and b"NULL" in L.blp_last_error()
    assert _call(L, scores=None) == -1 and b"NULL" in L.blp_last_error()
    for name in ("table", "source", "fixed_row", "rel_emb", "rel_id", "list_ptr", "list_row"):
        assert _call(L, **{name: None}) == -1 and b"NULL" in L.blp_last_error(), name
    assert _call(L, R=0) == -1 and _call(L, S=0) == -1
    assert _call(L, q_head=0, q_tail=0) == -1 and b"no query" in L.blp_last_error()  # entries without a query
    filt = _lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 100)
    assert _call(L, filter=filt) == -1 and b"row_base" in L.blp_last_error()
    assert _call(L, row_base=100, filter=filt, workspace=None) == -4  # the same filter on its own shard passes the check
    assert _call(L, filter=_lib.BlpFilter(None, 1 << 33, 1 << 34, None, None, 0, 0)) == -1 and b"filter" in L.blp_last_error()
    # workspace: Q = 3, nnz = 5 070 needs the (3, 7, 10) keys
    need = L.blp_topk_lists_workspace_bytes(0, 0, 128, 2, 1, 5070, 10)
    assert need == 1792
    assert _call(L, workspace=None) == -4 and b"workspace" in L.blp_last_error()
    assert _call(L, ws=1) == -4 and _call(L, ws=need - 1) == -4
    assert _call(L, workspace=(1 << 31) + 64) == -4
    assert _call(L, q_head=0, q_tail=0, nnz=0) == 0  # no query: nothing to do, nothing touched
    assert _call(L, q_head=0, q_tail=0, nnz=0, workspace=None, ws=0, list_ptr=None, list_row=None, source=None) == 0


def test_new_kernels_use_no_scratch_and_the_other_objects_keep_their_kernels():
    from blp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    for obj_dir in (build.OBJ, os.path.join(build.OBJ, build.HOOKS_VARIANT)):
        kernels = kernel_resources.kernels_of(os.path.join(obj_dir, "lists_topk.hip.o"))
        # TransE at a run-time width + three models x three widths, each over three storage types; nothing else
        assert len([k for k in kernels if "topk_lists_kernel" in k]) == 3 * (1 + 9) and len(kernels) == 30
        assert all(v["private_segment_fixed_size"] == 0 for v in kernels.values()), [k for k, v in kernels.items() if v["private_segment_fixed_size"]]
        # what tests/test_rank_lists_host.py and tests/test_topk_sets_host.py pin for the objects the step and the merge live in
        lists = kernel_resources.kernels_of(os.path.join(obj_dir, "rank_lists.hip.o"))
        assert len([k for k in lists if "rank_lists_kernel" in k]) == 30 and len([k for k in lists if "lists_true_key" in k]) == 10
        assert len(lists) == 40 and all(v["private_segment_fixed_size"] == 0 for v in lists.values())
        shared = kernel_resources.kernels_of(os.path.join(obj_dir, "topk.hip.o"))
        assert len(shared) == 12 + 24 + 36 + 2 and len([k for k in shared if "topk_merge" in k]) == 2
        assert len(kernel_resources.kernels_of(os.path.join(obj_dir, "topk_sets.hip.o"))) == 13


# ------------------------------------------------------------------------------------------- predict_from_candidates on CPU tensors
def brute_force(pred, lists, removed, k, unique=False):
    """The contract, spelled out: per query the valid entries (0 <= row < N; with `unique` one per row) that the filter leaves,
    sorted by row, then a stable argsort(-score) -- numpy puts NaN last --, the first k; -1 / NaN beyond."""
    Q, N = pred.shape
    rows_out = np.full((Q, k), -1, np.int64)
    scores_out = np.full((Q, k), np.nan, np.float32)
    for q in range(Q):
        rows = np.asarray([x for x in lists[q] if 0 <= x < N and not removed[q, x]], np.int64)
        rows = np.unique(rows) if unique else np.sort(rows, kind="stable")
        s = pred[q, rows]
        order = np.argsort(-s, kind="stable")[:k]
        rows_out[q, :len(order)], scores_out[q, :len(order)] = rows[order], s[order]
    return rows_out, scores_out


def same(got, want, what=""):
    rows, scores = (x.numpy() if isinstance(x, torch.Tensor) else x for x in got)
    assert rows.dtype == np.int64 and scores.dtype == np.float32 and rows.shape == want[0].shape, what
    assert np.array_equal(rows, want[0]), what
    nan = np.isnan(want[1])
    assert np.array_equal(np.isnan(scores), nan), what
    assert np.array_equal(scores[~nan].view(np.int32), want[1][~nan].view(np.int32)), what
    assert (np.isnan(scores[rows < 0])).all(), what


def _candidates(toy_, seed, C=37):
    N, Q = toy_["table"].shape[0], 2 * toy_["triples"].shape[0]
    rng = np.random.default_rng(seed)
    cand = rng.integers(0, N, (Q, C))
    cand[:, 20:30] = cand[:, 5:15]                  # duplicates
    cand[rng.random((Q, C)) < 0.2] = -1             # padding anywhere
    cand[3] = -1                                    # an empty list
    cand[4, 2:] = -1                                # a list of at most two entries
    return cand


@pytest.mark.parametrize("filtered", [False, True])
def test_rectangle_and_csr_against_the_brute_force_order(toy, filtered):  # noqa: F811
    N, Q = toy["table"].shape[0], 2 * toy["triples"].shape[0]
    T = Q // 2
    cand = _candidates(toy, 5)
    removed = toy["masks"] if filtered else np.zeros_like(toy["masks"])
    index = toy["index"] if filtered else None
    args = (toy["model"], toy["table"], toy["triples"])
    lists = [row[row >= 0] for row in cand]
    ptr = torch.from_numpy(np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int64))
    flat = torch.from_numpy(np.concatenate(lists))
    if filtered:
        assert any(removed[q, lists[q]].any() for q in range(Q)), "the filter must bite somewhere"
    for k in (1, 3, 10, 37 + 5):  # the last: larger than every list
        for unique in (False, True):
            want = brute_force(toy["pred"], cand, removed, k, unique)
            got = ranking.predict_from_candidates(*args, k, torch.from_numpy(cand), toy["ent2idx"], filter_index=index, unique=unique)
            same(got, want, (k, unique, "rectangle"))
            same(ranking.predict_from_candidates(*args, k, (ptr, flat), toy["ent2idx"], filter_index=index, unique=unique), want,
                 (k, unique, "csr"))
            assert (got[0][3] == -1).all() and (want[0][4] >= 0).sum() <= 2
            for side, sl in (("head", slice(0, T)), ("tail", slice(T, Q))):
                one = ranking.predict_from_candidates(*args, k, torch.from_numpy(cand[sl]), toy["ent2idx"], side=side,
                                                      filter_index=index, unique=unique)
                same(one, (want[0][sl], want[1][sl]), (k, unique, side))
    # duplicates come back adjacent with the same score unless `unique`
    dup = ranking.predict_from_candidates(*args, 37, torch.from_numpy(cand), toy["ent2idx"])
    r, s = dup[0].numpy(), dup[1].numpy()
    twice = (r[:, 1:] == r[:, :-1]) & (r[:, 1:] >= 0)
    assert twice.any() and np.array_equal(s[:, 1:][twice].view(np.int32), s[:, :-1][twice].view(np.int32))
    uni = ranking.predict_from_candidates(*args, 37, torch.from_numpy(cand), toy["ent2idx"], unique=True)[0].numpy()
    assert not ((uni[:, 1:] == uni[:, :-1]) & (uni[:, 1:] >= 0)).any()
    # a tiny byte budget takes the chunk loop of the dense route
    fixed = toy["table"][torch.from_numpy(np.concatenate((toy["t_row"], toy["h_row"])))]
    rel = toy["model"].rel_emb.weight.detach()[torch.from_numpy(np.concatenate((toy["rel"], toy["rel"])))]
    big = ranking._topk_lists_dense(toy["model"].score_fn, toy["table"], fixed, rel, T, 5, ptr, flat, 0, None)
    small = ranking._topk_lists_dense(toy["model"].score_fn, toy["table"], fixed, rel, T, 5, ptr, flat, 0, None,
                                      max_bytes=12 * toy["table"].shape[1] * 50)
    same(small, tuple(x.numpy() for x in big))
    same(big, brute_force(toy["pred"], cand, np.zeros_like(toy["masks"]), 5))


def test_entity_ids_in_and_out(toy):  # noqa: F811
    N, Q = toy["table"].shape[0], 2 * toy["triples"].shape[0]
    ent2idx = toy["ent2idx"].numpy()
    assert (ent2idx < 0).any()
    rng = np.random.default_rng(6)
    ids = rng.integers(-1, len(ent2idx) + 3, (Q, 41))  # ids without a row, out of range and -1 among them
    rows = np.where((ids >= 0) & (ids < len(ent2idx)), ent2idx[np.clip(ids, 0, len(ent2idx) - 1)], -1)
    assert (rows < 0).any() and (rows >= 0).any()
    want = brute_force(toy["pred"], rows, toy["masks"], 7)
    args = (toy["model"], toy["table"], toy["triples"])
    got = ranking.predict_from_candidates(*args, 7, torch.from_numpy(ids), toy["ent2idx"], filter_index=toy["index"], candidates_are="ids")
    same(got, want)
    entities = torch.from_numpy(np.asarray(toy["entities"]).astype(np.int64))
    as_ids = ranking.predict_from_candidates(*args, 7, torch.from_numpy(ids), toy["ent2idx"], filter_index=toy["index"],
                                             candidates_are="ids", entities=entities)
    same(as_ids, (np.where(want[0] >= 0, entities.numpy()[np.maximum(want[0], 0)], -1), want[1]))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16_bit_cpu_table_equals_its_widened_copy(toy, dtype):  # noqa: F811
    cand = torch.from_numpy(_candidates(toy, 7))
    t16 = toy["table"].to(dtype)
    for index in (None, toy["index"]):
        a = ranking.predict_from_candidates(toy["model"], t16, toy["triples"], 6, cand, toy["ent2idx"], filter_index=index)
        b = ranking.predict_from_candidates(toy["model"], t16.float(), toy["triples"], 6, cand, toy["ent2idx"], filter_index=index)
        same(a, tuple(x.numpy() for x in b))
        assert a[1].dtype == torch.float32


def test_predict_from_candidates_argument_errors(toy):  # noqa: F811
    args = (toy["model"], toy["table"], toy["triples"])
    Q = 2 * toy["triples"].shape[0]
    cand = torch.zeros((Q, 4), dtype=torch.long)
    with pytest.raises(ValueError):
        ranking.predict_from_candidates(*args, 3, cand, toy["ent2idx"], side="middle")
    with pytest.raises(ValueError):
        ranking.predict_from_candidates(*args, 3, cand, toy["ent2idx"], candidates_are="names")
    with pytest.raises(ValueError):
        ranking.predict_from_candidates(*args, 0, cand, toy["ent2idx"])
    with pytest.raises(ValueError):
        ranking.predict_from_candidates(*args, 3, cand[:-1], toy["ent2idx"])
    with pytest.raises(ValueError):
        ranking.predict_from_candidates(*args, 3, (torch.zeros(Q, dtype=torch.long), torch.zeros(0, dtype=torch.long)), toy["ent2idx"])
    assert REL_MODELS  # (the fixture runs once per model)
