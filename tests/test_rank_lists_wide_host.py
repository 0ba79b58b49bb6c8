"""Per-query candidate lists for DistMult / ComplEx / SimplE at any width (blp_rank_lists_wide): what can be checked without a
device -- the exports and the binding, the _supported truth table (blp_rank_lists' unchanged), the workspace size, every
refusal of blp_rank_lists reproduced under the new name with the same status and the same text, no scratch memory and only
dynamic LDS in the new kernels (read from the built object), and ranking.rank_candidates on CPU tensors at D = 300."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from blp_amd import _lib, build, ops, ranking
from test_rank_sets_host import _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_rank_lists_wide_supported", "blp_rank_lists_wide_workspace_bytes", "blp_rank_lists_wide")
TRANSE, DISTMULT, COMPLEX, SIMPLE = 0, 1, 2, 3
BILINEAR = {"distmult": DISTMULT, "complex": COMPLEX, "simple": SIMPLE}
F32, F16, BF16 = 0, 1, 2
WIDTHS = (0, 2, 4, 12, 64, 150, 300, 302, 768, 1024, 1028)
SIDE_HEAD, SIDE_TAIL = 0, 1


def _L():
    return _lib.lib()


def test_new_entry_points_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "blp_hip.h")).read()
    L = _L()
    for name in NEW:
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert getattr(L, name).argtypes is not None
    assert L.blp_version() == 60000
    assert list(L.blp_rank_lists_wide.argtypes) == list(L.blp_rank_lists.argtypes)
    assert list(L.blp_rank_lists_wide_workspace_bytes.argtypes) == list(L.blp_rank_lists_workspace_bytes.argtypes)
    assert list(L.blp_rank_lists_wide_supported.argtypes) == list(L.blp_rank_lists_supported.argtypes)
    assert L.blp_rank_lists_wide_workspace_bytes.restype is L.blp_rank_lists_workspace_bytes.restype
    assert callable(ops.rank_lists_wide) and callable(ops.rank_lists_wide_supported)
    for lib in (build.LIB, build.HOOKS_LIB):  # both libraries export the three names
        exported = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout.split()
        assert all(name in exported for name in NEW), lib


def test_supported_grid():
    L = _L()
    for m in (-1, TRANSE, DISTMULT, COMPLEX, SIMPLE, 4):
        for dt in (-1, F32, F16, BF16, 3):
            for D in WIDTHS:
                width = D % 4 == 0 and 4 <= D <= 1024
                want = int(m in (DISTMULT, COMPLEX, SIMPLE) and dt in (F32, F16, BF16) and width)
                assert L.blp_rank_lists_wide_supported(m, dt, D) == want, (m, dt, D)
                # blp_rank_lists answers as before
                old = dt in (F32, F16, BF16) and ((m == TRANSE and width) or (m in (DISTMULT, COMPLEX, SIMPLE) and D in (64, 128, 256)))
                assert L.blp_rank_lists_supported(m, dt, D) == int(old), (m, dt, D)
    for name, m in _lib.MODEL_IDS.items():
        for D in WIDTHS:
            for torch_dt, dt in ((torch.float32, F32), (torch.float16, F16), (torch.bfloat16, BF16)):
                assert ops.rank_lists_wide_supported(name, D, torch_dt) == bool(L.blp_rank_lists_wide_supported(m, dt, D))
    assert not ops.rank_lists_wide_supported("distmult", 300, torch.float64)
    assert not ops.rank_lists_supported("distmult", 300) and ops.rank_lists_supported("distmult", 128)


def test_workspace_bytes():
    """Q floats rounded up to 256 bytes, as blp_rank_lists': independent of the model, the table dtype and D; the entry takes
    neither N nor nnz."""
    L = _L()
    for m in BILINEAR.values():
        for dt in (F32, F16, BF16):
            for D in (4, 64, 300, 768, 1024):
                for qh, qt in ((0, 0), (0, 1), (1, 0), (2, 2), (32, 32), (64, 1), (6894, 6894), (52870, 52870), (1 << 29, 1 << 29)):
                    n = L.blp_rank_lists_wide_workspace_bytes(m, dt, D, qh, qt)
                    assert n == (4 * (qh + qt) + 255) // 256 * 256, (m, dt, D, qh, qt)
    assert len(L.blp_rank_lists_wide_workspace_bytes.argtypes) == 5  # model, dtype, D, q_head, q_tail
    for D in WIDTHS:
        if not (D % 4 == 0 and 4 <= D <= 1024):
            assert L.blp_rank_lists_wide_workspace_bytes(DISTMULT, F32, D, 2, 2) == 0, D
    assert L.blp_rank_lists_wide_workspace_bytes(TRANSE, F32, 300, 2, 2) == 0
    assert L.blp_rank_lists_wide_workspace_bytes(DISTMULT, 3, 300, 2, 2) == 0
    assert L.blp_rank_lists_wide_workspace_bytes(DISTMULT, -1, 300, 2, 2) == 0
    assert L.blp_rank_lists_wide_workspace_bytes(7, F32, 300, 2, 2) == 0
    assert L.blp_rank_lists_wide_workspace_bytes(DISTMULT, F32, 300, -1, 2) == 0
    assert L.blp_rank_lists_wide_workspace_bytes(DISTMULT, F32, 300, 2, -1) == 0


def _call(fn, **over):
    """A list-ranking entry with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(model=DISTMULT, table=1 << 20, dtype=F32, N=1000, D=300, ld=304, row_base=0, source=1 << 21, S=1000, ld_src=300,
             fixed_row=1 << 22, rel_emb=1 << 23, R=5, rel_id=1 << 24, true_row=1 << 25, q_head=2, q_tail=2, list_ptr=1 << 26,
             list_row=1 << 27, nnz=100, filter=None, counts=1 << 28, scores=1 << 29, workspace=1 << 30, ws=1 << 20, device=0,
             stream=None)
    a.update(over)
    f = a["filter"]
    return fn(a["model"], a["table"], a["dtype"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"], a["ld_src"],
              a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["true_row"], a["q_head"], a["q_tail"], a["list_ptr"],
              a["list_row"], a["nnz"], None if f is None else ctypes.byref(f), a["counts"], a["scores"], a["workspace"], a["ws"],
              a["device"], a["stream"])


# every refusal of api.cpp's rank_lists_call, in the order of its checks
REFUSALS = [
    (dict(model=7), -1, b"unknown model"),
    (dict(model=-1), -1, b"unknown model"),
    (dict(dtype=3), -1, b"unknown table dtype"),
    (dict(dtype=-1), -1, b"unknown table dtype"),
    (dict(model=TRANSE), -2, b"not supported"),
    (dict(D=302, ld=304, ld_src=304), -2, b"not supported"),
    (dict(D=1028, ld=1028, ld_src=1028), -2, b"not supported"),
    (dict(D=0, ld=8, ld_src=4), -2, b"not supported"),
    (dict(D=-128, ld=8, ld_src=4), -2, b"not supported"),
    (dict(N=-1), -1, b"negative"),
    (dict(q_head=-1), -1, b"negative"),
    (dict(q_tail=-1), -1, b"negative"),
    (dict(ld=296), -1, b"ld < D"),
    (dict(row_base=-1), -1, b"negative"),
    (dict(nnz=-1), -1, b"negative"),
    (dict(nnz=1 << 31), -1, b"nnz"),
    (dict(row_base=(1 << 31) - 10), -1, b"2^31"),
    (dict(q_head=(1 << 30), q_tail=1), -1, b"2^30"),
    (dict(counts=None, scores=None, true_row=None), -1, b"both outputs NULL"),
    (dict(true_row=None), -1, b"counts and true_row go together"),
    (dict(counts=None), -1, b"counts and true_row go together"),
    (dict(source=None), -1, b"NULL source"),
    (dict(fixed_row=None), -1, b"NULL source"),
    (dict(rel_id=None), -1, b"NULL source"),
    (dict(rel_emb=None), -1, b"NULL source"),
    (dict(list_ptr=None), -1, b"NULL source"),
    (dict(R=0), -1, b"R <= 0"),
    (dict(S=0), -1, b"S <= 0"),
    (dict(list_row=None), -1, b"NULL list_row"),
    (dict(q_head=0, q_tail=0), -1, b"but no query"),
    (dict(table=None), -1, b"NULL table"),
    (dict(table=(1 << 20) + 8), -1, b"aligned"),
    (dict(ld=302), -1, b"ld % 4"),
    (dict(dtype=F16, ld=308), -1, b"ld % 8"),
    (dict(dtype=BF16, ld=308), -1, b"ld % 8"),
    (dict(source=(1 << 21) + 4), -1, b"aligned"),
    (dict(ld_src=302), -1, b"aligned"),
    (dict(ld_src=296), -1, b"ld_src >= D"),
    (dict(rel_emb=(1 << 23) + 4), -1, b"aligned"),
    (dict(counts=(1 << 28) + 4), -1, b"aligned"),
    (dict(filter=_lib.BlpFilter(None, 1 << 33, 1 << 34, None, None, 0, 0)), -1, b"filter needs"),
    (dict(filter=_lib.BlpFilter(1 << 32, None, 1 << 34, None, None, 0, 0)), -1, b"filter needs"),
    (dict(filter=_lib.BlpFilter(1 << 32, 1 << 33, None, None, None, 0, 0)), -1, b"filter needs"),
    (dict(filter=_lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, 1 << 35, -1, 0)), -1, b"ent2idx_len"),
    (dict(filter=_lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 100)), -1, b"row_base"),
    (dict(workspace=None), -4, b"workspace"),
    (dict(ws=1), -4, b"workspace"),
    (dict(workspace=(1 << 30) + 64), -4, b"workspace"),
]


@pytest.mark.parametrize("over,status,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_follow_blp_rank_lists(over, status, message):
    """Reached with no device present: the status and the message, under this entry's name; blp_rank_lists refuses the same
    bad argument, on a TransE call (which it takes at D = 300), with the same status and -- but for the unsupported-width
    message, which names each entry's own limits -- the same text after the name."""
    L = _L()
    assert _call(L.blp_rank_lists_wide, **over) == status, over
    err = L.blp_last_error()
    assert message in err and err.startswith(b"blp_rank_lists_wide: "), err
    if over.get("model") == TRANSE:
        assert b"blp_rank_lists_wide_supported" in err
        return  # (the two entries differ in WHICH models they take, by design)
    narrow = dict(model=TRANSE)
    narrow.update(over)
    assert _call(L.blp_rank_lists, **narrow) == status, over
    old = L.blp_last_error()
    assert old.startswith(b"blp_rank_lists: "), old
    if status == -2:
        assert b"blp_rank_lists_wide_supported" in err and b"blp_rank_lists_supported" in old
    else:
        assert err[len(b"blp_rank_lists_wide"):] == old[len(b"blp_rank_lists"):], (err, old)


def test_blp_rank_lists_keeps_its_refusal_of_these_widths():
    L = _L()
    for m in BILINEAR.values():
        assert _call(L.blp_rank_lists, model=m) == -2
        assert L.blp_last_error().startswith(b"blp_rank_lists: D = 300 not supported (TransE")


def test_exact_workspace_size_and_the_empty_block():
    L = _L()
    for m in BILINEAR.values():
        need = L.blp_rank_lists_wide_workspace_bytes(m, F32, 300, 2, 2)
        assert need == 256
        assert _call(L.blp_rank_lists_wide, model=m, ws=need - 1) == -4
        assert b">= 256 bytes (got 255)" in L.blp_last_error()
        assert _call(L.blp_rank_lists_wide, model=m, q_head=40, q_tail=25, ws=256) == -4  # 65 queries: a second line
    # scores alone need no workspace: the first thing a NULL workspace meets is the device (no refusal to reach here), so only
    # the counts form is probed.  No query and no entry: nothing to do, nothing touched
    assert _call(L.blp_rank_lists_wide, q_head=0, q_tail=0, nnz=0) == 0
    assert _call(L.blp_rank_lists_wide, q_head=0, q_tail=0, nnz=0, workspace=None, ws=0) == 0
    assert _call(L.blp_rank_lists_wide, q_head=0, q_tail=0, nnz=0, model=TRANSE) == -2  # ... after the model / width checks
    assert _call(L.blp_rank_lists_wide, q_head=0, q_tail=0, nnz=0, N=-1) == -1
    assert _call(L.blp_rank_lists, model=TRANSE, q_head=0, q_tail=0, nnz=0) == 0


def test_no_kernel_of_the_new_file_uses_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = kernel_resources.kernels_of(os.path.join(build.OBJ, "rank_lists_wide.hip.o"))
    passes = [k for k in kernels if "rank_lists_wide_kernel" in k]
    assert len(passes) == 3 * 3 * 2  # model x table dtype x (n < 512, n >= 512): both sides and every width in one
    keys = [k for k in kernels if "lists_wide_true_key_kernel" in k]
    assert len(keys) == 3 and len(kernels) == len(passes) + len(keys)
    assert all(k["private_segment_fixed_size"] == 0 for k in kernels.values()), [n for n, k in kernels.items() if k["private_segment_fixed_size"]]
    assert all(kernels[k]["group_segment_fixed_size"] == 0 for k in passes)  # the ranking kernels' LDS is all dynamic
    # rank_lists.hip keeps its kernels
    assert len(kernel_resources.kernels_of(os.path.join(build.OBJ, "rank_lists.hip.o"))) == 40


@pytest.mark.parametrize("rel_model", list(BILINEAR))
def test_rank_candidates_on_cpu_tensors_at_300_takes_the_dense_route(oracle, rel_model, monkeypatch):
    N, D, R, T, C = 150, 300, 5, 20, 40
    g = torch.Generator().manual_seed(300)
    table = torch.randn(N, D, generator=g) * 0.1
    table[7] = table[3]  # a tie
    rel_w = ((torch.rand(R, D, generator=g) - 0.5) * 0.25).numpy()
    model = _model(rel_model, rel_w)
    triples = torch.stack((torch.randint(0, N, (T,), generator=g), torch.randint(0, N, (T,), generator=g),
                           torch.randint(0, R, (T,), generator=g)), dim=1)
    triples[0, 0] = 3
    ent2idx = torch.arange(N)
    cand = torch.randint(-1, N, (2 * T, C), generator=g)
    cand[0, :2] = torch.tensor([7, 3])
    dense, seen = ranking._rank_lists_dense, []

    def spy(*a, **k):
        seen.append(dense(*a, **k))
        return seen[-1]

    def no_fused(*a, **k):
        raise AssertionError("CPU tensors went to a fused call")

    monkeypatch.setattr(ranking, "_rank_lists_dense", spy)
    monkeypatch.setattr(ops, "rank_lists_wide", no_fused)
    monkeypatch.setattr(ops, "rank_lists", no_fused)
    got = ranking.rank_candidates(model, table, triples, cand, ent2idx)
    assert len(seen) == 1 and torch.equal(got, seen[0][0])
    tab, h, t, r = table.numpy(), triples[:, 0].numpy(), triples[:, 1].numpy(), triples[:, 2].numpy()
    pred = np.concatenate((oracle.score_all(rel_model, SIDE_HEAD, tab, tab[t], rel_w[r]),
                           oracle.score_all(rel_model, SIDE_TAIL, tab, tab[h], rel_w[r])))
    true = pred[np.arange(2 * T), np.concatenate((h, t))]
    want = np.zeros((2 * T, 4), np.int32)
    for q in range(2 * T):
        rows = cand[q].numpy()
        s = pred[q, rows[rows >= 0]]
        want[q] = ((s > true[q]).sum(), (s >= true[q]).sum(), (s > true[q]).sum(), (s >= true[q]).sum())
    assert np.array_equal(got.numpy(), want) and want[0, 1] >= 2, "the oracle's counts, the tie with the true entity among them"
