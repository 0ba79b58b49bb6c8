"""Candidate sets shared between queries for DistMult / ComplEx / SimplE at any width (blp_rank_sets_wide_bilinear): what can
be checked without a device -- the exports, the _supported truth table (the other set entries' unchanged), the workspace size,
every refusal of the shared argument checks with blp_rank_sets_wide's status codes, no scratch memory in the new kernels (read
from the built object), ranking.rank_in_sets on CPU tensors at D = 300, and the yardstick of the device tests: the C oracle's
score_all equals score_fn on CPU torch bit for bit at D = 300 and 768."""
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
NEW = ("blp_rank_sets_wide_bilinear_supported", "blp_rank_sets_wide_bilinear_workspace_bytes", "blp_rank_sets_wide_bilinear")
TRANSE, DISTMULT, COMPLEX, SIMPLE = 0, 1, 2, 3
BILINEAR = {"distmult": DISTMULT, "complex": COMPLEX, "simple": SIMPLE}
F32, F16, BF16 = 0, 1, 2
WIDTHS = (0, 2, 4, 12, 64, 150, 300, 302, 768, 1024, 1028)


def _L():
    return _lib.lib()


def test_new_entry_points_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "blp_hip.h")).read()
    L = _L()
    for name in NEW:
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert getattr(L, name).argtypes is not None
    assert L.blp_version() == 60000
    assert list(L.blp_rank_sets_wide_bilinear.argtypes) == list(L.blp_rank_sets_wide.argtypes)
    assert list(L.blp_rank_sets_wide_bilinear_workspace_bytes.argtypes) == list(L.blp_rank_sets_wide_workspace_bytes.argtypes)
    assert callable(ops.rank_sets_wide_bilinear) and callable(ops.rank_sets_wide_bilinear_supported)
    assert callable(ops.rank_sets_wide_bilinear_workspace_bytes)
    for lib in (build.LIB, build.HOOKS_LIB):  # both libraries export the three names
        exported = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout.split()
        assert all(name in exported for name in NEW), lib


def test_supported_grid():
    L = _L()
    for m in (-1, TRANSE, DISTMULT, COMPLEX, SIMPLE, 4):
        for dt, torch_dt in ((F32, torch.float32), (F16, torch.float16), (BF16, torch.bfloat16)):
            for D in WIDTHS:
                width = D % 4 == 0 and 4 <= D <= 1024
                assert L.blp_rank_sets_wide_bilinear_supported(m, dt, D) == int(m in (DISTMULT, COMPLEX, SIMPLE) and dt == F32 and width), (m, dt, D)
                # the other set entries answer as before
                assert L.blp_rank_sets_wide_supported(m, dt, D) == int(m == TRANSE and width), (m, dt, D)
                assert L.blp_rank_sets_supported(m, D) == int(m in range(4) and D in (64, 128, 256)), (m, D)
                assert L.blp_rank_sets_typed_supported(m, dt, D) == int(m in range(4) and D in (64, 128, 256)), (m, dt, D)
    for dt in (-1, 3, 7):
        assert L.blp_rank_sets_wide_bilinear_supported(DISTMULT, dt, 300) == 0, dt
    for name, m in _lib.MODEL_IDS.items():
        for D in WIDTHS:
            for torch_dt, dt in ((torch.float32, F32), (torch.float16, F16), (torch.bfloat16, BF16)):
                assert ops.rank_sets_wide_bilinear_supported(name, D, torch_dt) == bool(L.blp_rank_sets_wide_bilinear_supported(m, dt, D))
    assert not ops.rank_sets_wide_bilinear_supported("distmult", 300, torch.float64)


def test_workspace_bytes():
    """True keys and accumulators (12 bytes per query) and two unit prefixes of G + 1 int64, each piece rounded up to 256
    bytes: a multiple of 256, monotone in Q and G, independent of D; the entry takes neither N nor nnz."""
    L = _L()
    for m in BILINEAR.values():
        for G in (1, 12, 474, 1644, 100000):
            last = 0
            for qh, qt in ((0, 1), (1, 0), (1, 1), (100, 3), (6894, 6894), (52870, 52870), (1 << 29, 1 << 29)):
                n = L.blp_rank_sets_wide_bilinear_workspace_bytes(m, F32, 300, qh, qt, G)
                floor = 12 * (qh + qt) + 16 * (G + 1)
                assert n % 256 == 0 and floor <= n <= floor + 4 * 256, (m, G, qh, qt)
                assert n >= last
                last = n
                for D in (4, 64, 768, 1024):
                    assert n == L.blp_rank_sets_wide_bilinear_workspace_bytes(m, F32, D, qh, qt, G), D
                assert n == L.blp_rank_sets_wide_bilinear_workspace_bytes(m, F32, 300, qt, qh, G)
        sizes = [L.blp_rank_sets_wide_bilinear_workspace_bytes(m, F32, 300, 300, 300, G) for G in (1, 12, 474, 1644, 100000)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert ops.rank_sets_wide_bilinear_workspace_bytes("complex", 768, 100, 171, 474) == L.blp_rank_sets_wide_bilinear_workspace_bytes(COMPLEX, F32, 768, 100, 171, 474)
    assert len(L.blp_rank_sets_wide_bilinear_workspace_bytes.argtypes) == 6  # model, dtype, D, q_head, q_tail, G: no N, no nnz
    for D in WIDTHS:
        if not (D % 4 == 0 and 4 <= D <= 1024):
            assert L.blp_rank_sets_wide_bilinear_workspace_bytes(DISTMULT, F32, D, 2, 2, 5) == 0, D
    assert L.blp_rank_sets_wide_bilinear_workspace_bytes(TRANSE, F32, 300, 2, 2, 5) == 0
    assert L.blp_rank_sets_wide_bilinear_workspace_bytes(DISTMULT, BF16, 300, 2, 2, 5) == 0
    assert L.blp_rank_sets_wide_bilinear_workspace_bytes(DISTMULT, 5, 300, 2, 2, 5) == 0
    assert L.blp_rank_sets_wide_bilinear_workspace_bytes(7, F32, 300, 2, 2, 5) == 0
    assert L.blp_rank_sets_wide_bilinear_workspace_bytes(DISTMULT, F32, 300, -1, 2, 5) == 0
    assert L.blp_rank_sets_wide_bilinear_workspace_bytes(DISTMULT, F32, 300, 2, -1, 5) == 0
    assert L.blp_rank_sets_wide_bilinear_workspace_bytes(DISTMULT, F32, 300, 2, 2, -1) == 0
    assert ops.rank_sets_wide_bilinear_workspace_bytes("transe", 300, 2, 2, 5) == 0
    assert ops.rank_sets_wide_bilinear_workspace_bytes("simple", 300, -1, 2, 5) == 0


def _call(fn, **over):
    """A set-ranking entry with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(model=DISTMULT, table=1 << 20, dtype=F32, N=1000, D=300, ld=304, row_base=0, source=1 << 21, S=1000, ld_src=300,
             fixed_row=1 << 22, rel_emb=1 << 23, R=5, rel_id=1 << 24, true_row=1 << 25, q_head=2, q_tail=2, set_ptr=1 << 26,
             set_row=1 << 27, nnz=100, G=3, qh=1 << 28, qt=1 << 29, filter=None, counts=1 << 30, workspace=1 << 31, ws=1 << 20,
             device=0, stream=None)
    a.update(over)
    f = a["filter"]
    return fn(a["model"], a["table"], a["dtype"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"], a["ld_src"],
              a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["true_row"], a["q_head"], a["q_tail"], a["set_ptr"],
              a["set_row"], a["nnz"], a["G"], a["qh"], a["qt"], None if f is None else ctypes.byref(f), a["counts"],
              a["workspace"], a["ws"], a["device"], a["stream"])


# every refusal of api.cpp's rank_sets_call, in the order of its checks
REFUSALS = [
    (dict(model=7), -1, b"unknown model"),
    (dict(model=-1), -1, b"unknown model"),
    (dict(dtype=3), -1, b"unknown table dtype"),
    (dict(dtype=-1), -1, b"unknown table dtype"),
    (dict(model=TRANSE), -2, b"not supported"),
    (dict(dtype=F16, ld=304), -2, b"not supported"),
    (dict(dtype=BF16, ld=304), -2, b"not supported"),
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
    (dict(G=-1), -1, b"negative"),
    (dict(nnz=1 << 31), -1, b"nnz"),
    (dict(row_base=(1 << 31) - 10), -1, b"2^31"),
    (dict(q_head=(1 << 30), q_tail=1), -1, b"2^30"),
    (dict(source=None), -1, b"NULL source"),
    (dict(fixed_row=None), -1, b"NULL source"),
    (dict(rel_id=None), -1, b"NULL source"),
    (dict(rel_emb=None), -1, b"NULL source"),
    (dict(true_row=None), -1, b"NULL source"),
    (dict(counts=None), -1, b"NULL source"),
    (dict(R=0), -1, b"R <= 0"),
    (dict(S=0), -1, b"S <= 0"),
    (dict(G=0), -1, b"no set"),
    (dict(set_ptr=None), -1, b"NULL set_ptr"),
    (dict(qh=None), -1, b"NULL set_ptr"),
    (dict(qt=None), -1, b"NULL set_ptr"),
    (dict(set_row=None), -1, b"NULL set_row"),
    (dict(table=None), -1, b"NULL table"),
    (dict(table=(1 << 20) + 8), -1, b"aligned"),
    (dict(ld=302), -1, b"ld % 4"),
    (dict(source=(1 << 21) + 4), -1, b"aligned"),
    (dict(ld_src=302), -1, b"aligned"),
    (dict(ld_src=296), -1, b"ld_src >= D"),
    (dict(rel_emb=(1 << 23) + 4), -1, b"aligned"),
    (dict(counts=(1 << 30) + 4), -1, b"aligned"),
    (dict(filter=_lib.BlpFilter(None, 1 << 33, 1 << 34, None, None, 0, 0)), -1, b"filter needs"),
    (dict(filter=_lib.BlpFilter(1 << 32, None, 1 << 34, None, None, 0, 0)), -1, b"filter needs"),
    (dict(filter=_lib.BlpFilter(1 << 32, 1 << 33, None, None, None, 0, 0)), -1, b"filter needs"),
    (dict(filter=_lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, 1 << 35, -1, 0)), -1, b"ent2idx_len"),
    (dict(filter=_lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 100)), -1, b"row_base"),
    (dict(workspace=None), -4, b"workspace"),
    (dict(ws=1), -4, b"workspace"),
    (dict(workspace=(1 << 31) + 64), -4, b"workspace"),
]


@pytest.mark.parametrize("over,status,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_follow_blp_rank_sets_wide(over, status, message):
    """Reached with no device present: the status and the message, under this entry's name; blp_rank_sets_wide refuses the
    same bad argument, on a TransE call, with the same status."""
    L = _L()
    assert _call(L.blp_rank_sets_wide_bilinear, **over) == status, over
    err = L.blp_last_error()
    assert message in err and err.startswith(b"blp_rank_sets_wide_bilinear:"), err
    if over.get("model") == TRANSE or over.get("dtype") in (F16, BF16):
        return  # (the two entries differ in WHICH models and table dtypes they take, by design)
    wide = dict(model=TRANSE)
    wide.update(over)
    assert _call(L.blp_rank_sets_wide, **wide) == status, over
    assert L.blp_last_error().startswith(b"blp_rank_sets_wide:")


def test_blp_rank_sets_wide_keeps_its_refusal_of_these_models():
    L = _L()
    for m in BILINEAR.values():
        assert _call(L.blp_rank_sets_wide, model=m) == -2
        assert b"blp_rank_sets_wide: model" in L.blp_last_error() and b"transe" in L.blp_last_error()


def test_exact_workspace_size_and_the_empty_block():
    L = _L()
    for m in BILINEAR.values():
        need = L.blp_rank_sets_wide_bilinear_workspace_bytes(m, F32, 300, 2, 2, 3)
        assert need == 4 * 256
        assert _call(L.blp_rank_sets_wide_bilinear, model=m, ws=need - 1) == -4
    assert _call(L.blp_rank_sets_wide_bilinear, q_head=0, q_tail=0) == 0  # no query: nothing to do, nothing touched
    assert _call(L.blp_rank_sets_wide_bilinear, q_head=0, q_tail=0, model=TRANSE) == -2  # ... after the model / width checks
    assert _call(L.blp_rank_sets_wide_bilinear, q_head=0, q_tail=0, N=-1) == -1


def test_no_kernel_of_the_new_file_uses_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = kernel_resources.kernels_of(os.path.join(build.OBJ, "rank_sets_wide_bilinear.hip.o"))
    passes = [k for k in kernels if "rank_sets_wide_bilinear_kernel" in k]
    assert len(passes) == 3 * 2 * 2  # model x side x (n < 512, n >= 512)
    assert len(kernels) == len(passes) + 3 + 3 + 1  # true keys and finalize per model, one unit prefix
    assert all(k["private_segment_fixed_size"] == 0 for k in kernels.values()), [n for n, k in kernels.items() if k["private_segment_fixed_size"]]
    assert all(kernels[k]["group_segment_fixed_size"] == 0 for k in passes)  # the ranking kernel's LDS is all dynamic
    # rank_all_wide.hip's kernels keep their names, the true-key kernel (now in a shared header) included
    table_pass = kernel_resources.kernels_of(os.path.join(build.OBJ, "rank_all_wide.hip.o"))
    for stem, n in (("rank_all_wide_kernel", 12), ("wide_bilinear_true_key_kernel", 3), ("wide_bilinear_filter_finalize_kernel", 3)):
        assert sum(stem in k for k in table_pass) == n, stem
    assert len(table_pass) == 18


@pytest.mark.parametrize("rel_model", list(BILINEAR))
@pytest.mark.parametrize("D", [300, 768])
def test_oracle_score_all_equals_score_fn_bit_for_bit(oracle, rel_model, D):
    """The yardstick of tests/test_gpu_rank_sets_wide_bilinear.py: the C oracle's (Q, N) scores are CPU torch's score_fn on the
    same pairs, bit for bit, on a table whose entries carry their own binary exponent."""
    N, Q, R = 97, 11, 5
    g = torch.Generator().manual_seed(D)
    scale = lambda x: x * torch.exp2(torch.randint(-20, 21, x.shape, generator=g).float())
    table, rel_w = scale(torch.randn(N, D, generator=g) * 0.1), scale((torch.rand(R, D, generator=g) - 0.5) * 0.25)
    fixed, rel = table[torch.randint(0, N, (Q,), generator=g)], rel_w[torch.randint(0, R, (Q,), generator=g)]
    score_fn = _model(rel_model, rel_w.numpy()).score_fn
    ee = table.unsqueeze(0).expand(Q, N, D).reshape(Q * N, D)
    ff = fixed.unsqueeze(1).expand(Q, N, D).reshape(Q * N, D)
    rr = rel.unsqueeze(1).expand(Q, N, D).reshape(Q * N, D)
    with torch.no_grad():
        for side, want in ((0, score_fn(ee, ff, rr)), (1, score_fn(ff, ee, rr))):
            got = oracle.score_all(rel_model, side, table.numpy(), fixed.numpy(), rel.numpy())
            assert np.array_equal(got.view(np.int32), want.reshape(Q, N).numpy().view(np.int32)), (rel_model, D, side)


@pytest.mark.parametrize("rel_model", list(BILINEAR))
def test_rank_in_sets_on_cpu_tensors_at_300_takes_the_dense_route(rel_model, monkeypatch):
    N, D, R, T, G = 150, 300, 5, 40, 8
    g = torch.Generator().manual_seed(300)
    table = torch.randn(N, D, generator=g) * 0.1
    table[7] = table[3]  # a tie
    rel_w = ((torch.rand(R, D, generator=g) - 0.5) * 0.25).numpy()
    model = _model(rel_model, rel_w)
    triples = torch.stack((torch.randint(0, N, (T,), generator=g), torch.randint(0, N, (T,), generator=g),
                           torch.randint(0, R, (T,), generator=g)), dim=1)
    triples[0, 0] = 3
    ent2idx = torch.arange(N)
    rng = np.random.default_rng(301)
    sets = ranking.CandidateSets([rng.choice(N, n, replace=False) for n in (0, 1, N, 64, 65, 20, 100, 7)])
    set_ids = torch.from_numpy(rng.integers(0, G, 2 * T))
    set_ids[:3] = torch.tensor([2, 0, 1])
    dense, seen = ranking._rank_sets_dense, []

    def spy(*a, **k):
        seen.append(dense(*a, **k))
        return seen[-1]

    def no_fused(*a, **k):
        raise AssertionError("CPU tensors went to the fused call")

    monkeypatch.setattr(ranking, "_rank_sets_dense", spy)
    monkeypatch.setattr(ops, "rank_sets_wide_bilinear", no_fused)
    got = ranking.rank_in_sets(model, table, triples, sets, ent2idx, set_ids=set_ids, add_true=False)
    assert len(seen) == 1
    perm, _, _ = ranking._group_by_set(set_ids, T, G)
    want = torch.empty_like(seen[0])
    want[perm] = seen[0]
    assert torch.equal(got, want) and got[0, 1] >= 2, "the dense route's counts, the tie with the true entity among them"
