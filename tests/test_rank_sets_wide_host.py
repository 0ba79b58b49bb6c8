"""Candidate sets shared between queries for TransE at any width (blp_rank_sets_wide): what can be checked without a device --
the _supported truth table, the workspace size, the argument errors, the exports, and ranking.rank_in_sets on CPU tensors at
D = 300 against the C oracle's counts on the expanded sets (the yardstick tests/test_gpu_rank_sets_wide.py compares with)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from blp_amd import _lib, ops, ranking
from test_rank_sets_host import _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_rank_sets_wide_supported", "blp_rank_sets_wide_workspace_bytes", "blp_rank_sets_wide")
TRANSE, COMPLEX, DISTMULT, SIMPLE = (_lib.MODEL_IDS[m] for m in ("transe", "complex", "distmult", "simple"))
F32, F16, BF16 = 0, 1, 2
YES = (4, 64, 68, 128, 300, 768, 1024)
NO = (0, 2, 6, 1028, 2048)


def _L():
    return _lib.lib()


def test_new_entry_points_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "blp_hip.h")).read()
    L = _L()
    for name in NEW:
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert getattr(L, name).argtypes is not None
    assert L.blp_version() == 60000
    assert list(L.blp_rank_sets_wide.argtypes) == list(L.blp_rank_sets_typed.argtypes)
    assert callable(ops.rank_sets_wide) and callable(ops.rank_sets_wide_supported) and callable(ops.rank_sets_wide_workspace_bytes)


def test_supported_truth_table():
    L = _L()
    for dt, torch_dt in ((F32, torch.float32), (F16, torch.float16), (BF16, torch.bfloat16)):
        for D in YES:
            assert L.blp_rank_sets_wide_supported(TRANSE, dt, D) == 1, (dt, D)
            assert ops.rank_sets_wide_supported("transe", D, torch_dt), (dt, D)
        for D in NO + (-4, -64):
            assert L.blp_rank_sets_wide_supported(TRANSE, dt, D) == 0, (dt, D)
            assert not ops.rank_sets_wide_supported("transe", D, torch_dt), (dt, D)
        for m, name in ((DISTMULT, "distmult"), (COMPLEX, "complex"), (SIMPLE, "simple")):
            for D in (300, 128):
                assert L.blp_rank_sets_wide_supported(m, dt, D) == 0, (m, D)
                assert not ops.rank_sets_wide_supported(name, D, torch_dt)
    for dt in (-1, 3, 7):
        assert L.blp_rank_sets_wide_supported(TRANSE, dt, 300) == 0, dt
    assert not ops.rank_sets_wide_supported("transe", 300, torch.float64)
    assert L.blp_rank_sets_wide_supported(4, F32, 300) == 0 and L.blp_rank_sets_wide_supported(-1, F32, 300) == 0
    # the fixed-width entry points answer as before
    for D in (64, 128, 256):
        assert L.blp_rank_sets_supported(TRANSE, D) and L.blp_rank_sets_typed_supported(TRANSE, BF16, D)
    assert not L.blp_rank_sets_supported(TRANSE, 300) and not L.blp_rank_sets_typed_supported(TRANSE, F16, 768)


def test_workspace_bytes():
    """True keys, accumulators, coefficient rows (head side 2 D floats per query, tail side D) and G + 1 unit offsets: a multiple
    of 256, the same for every table dtype; the entry takes neither N nor nnz, so it cannot depend on them."""
    L = _L()
    for D in YES:
        last = 0
        for qh, qt in ((0, 1), (1, 0), (1, 1), (100, 3), (6894, 6894), (52870, 52870)):
            n = L.blp_rank_sets_wide_workspace_bytes(TRANSE, F32, D, qh, qt, 474)
            floor = (qh + qt) * 12 + qh * 8 * D + qt * 4 * D + 475 * 8
            assert n % 256 == 0 and floor <= n <= floor + 5 * 256, (D, qh, qt)
            assert n >= last
            last = n
            assert n == L.blp_rank_sets_wide_workspace_bytes(TRANSE, F16, D, qh, qt, 474) == L.blp_rank_sets_wide_workspace_bytes(TRANSE, BF16, D, qh, qt, 474)
            assert n == ops.rank_sets_wide_workspace_bytes("transe", D, qh, qt, 474)
        sizes = [L.blp_rank_sets_wide_workspace_bytes(TRANSE, F32, D, 300, 300, G) for G in (1, 12, 474, 1644, 100000)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0] and all(s % 256 == 0 for s in sizes)
    assert len(L.blp_rank_sets_wide_workspace_bytes.argtypes) == 6  # model, dtype, D, q_head, q_tail, G: no N, no nnz
    for D in NO:
        assert L.blp_rank_sets_wide_workspace_bytes(TRANSE, F32, D, 2, 2, 5) == 0, D
    assert L.blp_rank_sets_wide_workspace_bytes(COMPLEX, F32, 300, 2, 2, 5) == 0
    assert L.blp_rank_sets_wide_workspace_bytes(TRANSE, 5, 300, 2, 2, 5) == 0
    assert L.blp_rank_sets_wide_workspace_bytes(7, F32, 300, 2, 2, 5) == 0
    assert L.blp_rank_sets_wide_workspace_bytes(TRANSE, F32, 300, -1, 2, 5) == 0
    assert L.blp_rank_sets_wide_workspace_bytes(TRANSE, F32, 300, 2, -1, 5) == 0
    assert L.blp_rank_sets_wide_workspace_bytes(TRANSE, F32, 300, 2, 2, -1) == 0
    assert ops.rank_sets_wide_workspace_bytes("complex", 300, 2, 2, 5) == 0 and ops.rank_sets_wide_workspace_bytes("transe", 300, -1, 2, 5) == 0


def _call(L, **over):
    """blp_rank_sets_wide with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(model=TRANSE, table=1 << 20, dtype=F32, N=1000, D=300, ld=304, row_base=0, source=1 << 21, S=1000, ld_src=300,
             fixed_row=1 << 22, rel_emb=1 << 23, R=5, rel_id=1 << 24, true_row=1 << 25, q_head=2, q_tail=2, set_ptr=1 << 26,
             set_row=1 << 27, nnz=100, G=3, qh=1 << 28, qt=1 << 29, filter=None, counts=1 << 30, workspace=1 << 31, ws=1 << 20,
             device=0, stream=None)
    a.update(over)
    f = a["filter"]
    return L.blp_rank_sets_wide(a["model"], a["table"], a["dtype"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"], a["ld_src"],
                                a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["true_row"], a["q_head"], a["q_tail"], a["set_ptr"],
                                a["set_row"], a["nnz"], a["G"], a["qh"], a["qt"], None if f is None else ctypes.byref(f), a["counts"],
                                a["workspace"], a["ws"], a["device"], a["stream"])


def test_bad_arguments_return_their_status_without_a_device():
    L = _L()
    assert _call(L, model=7) == -1 and b"unknown model" in L.blp_last_error()
    assert _call(L, model=-1) == -1
    assert _call(L, dtype=3) == -1 and b"dtype" in L.blp_last_error()
    for D in NO + (-128,):
        assert _call(L, D=D, ld=max(D, 8), ld_src=max(D, 4)) == -2 and b"blp_rank_sets_wide" in L.blp_last_error(), D
    for m in (DISTMULT, COMPLEX, SIMPLE):
        assert _call(L, model=m) == -2 and b"not supported" in L.blp_last_error(), m
    for name in ("N", "q_head", "q_tail", "nnz", "G", "row_base"):
        assert _call(L, **{name: -1}) == -1 and b"negative" in L.blp_last_error(), name
    assert _call(L, ld=296) == -1  # ld < D
    assert _call(L, nnz=1 << 31) == -1 and b"nnz" in L.blp_last_error()
    assert _call(L, q_head=(1 << 30), q_tail=1) == -1 and b"2^30" in L.blp_last_error()
    assert _call(L, row_base=(1 << 31) - 10) == -1
    for name in ("table", "source", "fixed_row", "rel_emb", "rel_id", "true_row", "set_ptr", "set_row", "qh", "qt", "counts"):
        assert _call(L, **{name: None}) == -1 and b"NULL" in L.blp_last_error(), name
    assert _call(L, G=0) == -1
    assert _call(L, R=0) == -1 and _call(L, S=0) == -1
    assert _call(L, table=(1 << 20) + 8) == -1 and b"aligned" in L.blp_last_error()
    assert _call(L, ld=302) == -1 and b"ld % 4" in L.blp_last_error()          # f32: ld % 4
    assert _call(L, dtype=F16, ld=300) == -1 and b"ld % 8" in L.blp_last_error()  # 16-bit: ld % 8 (300 is only a multiple of 4)
    assert _call(L, dtype=BF16, ld=308) == -1
    assert _call(L, ld_src=302) == -1 and _call(L, ld_src=296) == -1
    filt = _lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 100)
    assert _call(L, filter=filt) == -1 and b"row_base" in L.blp_last_error()
    assert _call(L, filter=_lib.BlpFilter(None, 1 << 33, 1 << 34, None, None, 0, 0)) == -1 and b"filter" in L.blp_last_error()
    assert _call(L, workspace=None) == -4 and b"workspace" in L.blp_last_error()
    assert _call(L, ws=1) == -4
    for dt, ld in ((F32, 304), (F16, 304), (BF16, 304)):
        assert _call(L, dtype=dt, ld=ld, ws=L.blp_rank_sets_wide_workspace_bytes(TRANSE, dt, 300, 2, 2, 3) - 1) == -4
    assert _call(L, workspace=(1 << 31) + 64) == -4
    assert _call(L, q_head=0, q_tail=0) == 0  # no query: nothing to do, nothing touched


def test_rank_in_sets_on_cpu_tensors_at_300_equals_the_oracle_on_the_expanded_sets(oracle):
    """The dense route on CPU tensors (what the device route is compared with) against blp_oracle_rank_counts: each query ranked
    against the rows of its set as a table of their own, the true entity's vector given."""
    N, D, R, T, G = 150, 300, 5, 40, 8
    g = torch.Generator().manual_seed(300)
    table = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    table[7] = table[3]  # a tie
    rel_w = ((torch.rand(R, D, generator=g) - 0.5) * 0.25).numpy()
    model = _model("transe", rel_w)
    triples = torch.stack((torch.randint(0, N, (T,), generator=g), torch.randint(0, N, (T,), generator=g),
                           torch.randint(0, R, (T,), generator=g)), dim=1)
    triples[0, 0] = 3
    ent2idx = torch.arange(N)
    rng = np.random.default_rng(301)
    sets = ranking.CandidateSets([rng.choice(N, n, replace=False) for n in (0, 1, N, 64, 65, 20, 100, 7)])
    set_ids = torch.from_numpy(rng.integers(0, G, 2 * T))
    set_ids[:3] = torch.tensor([2, 0, 1])
    got = ranking.rank_in_sets(model, table, triples, sets, ent2idx, set_ids=set_ids, add_true=False).numpy()
    lists, tab = sets.tolist(), table.numpy()
    want = np.zeros((2 * T, 4), np.int32)
    for q in range(2 * T):
        rows = lists[int(set_ids[q])]
        if not rows:
            continue
        tr = triples[q % T]
        head = q < T
        fixed, true = (tab[tr[1]], tab[tr[0]]) if head else (tab[tr[0]], tab[tr[1]])
        want[q] = oracle.rank_counts("transe", 0 if head else 1, tab[rows], fixed[None], rel_w[tr[2]][None], q_true=true[None])[0]
    assert want[0, 1] >= 2, "the tie with the true entity must be counted"
    assert np.array_equal(got, want)
