"""Candidate sets on a 16-bit entity table, without a GPU (include/blp_hip.h: blp_rank_sets_typed_supported,
blp_rank_sets_typed_workspace_bytes, blp_rank_sets_typed): the entry points are exported by both libraries and declared, which
(model, dtype, D) they take, the workspace equals the untyped one, the argument refusals (checked before anything touches a
device), the f32 dtype answers as blp_rank_sets, no scratch memory in the 16-bit kernels, and the CPU route of rank_in_sets on a
16-bit table against the same route on the table widened to f32."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden
from blp_amd import _lib, build, models, ranking, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_rank_sets_typed_supported", "blp_rank_sets_typed_workspace_bytes", "blp_rank_sets_typed")
F32, F16, BF16 = 0, 1, 2


def _L():
    return _lib.lib()


def test_typed_entry_points_are_exported_by_both_libraries_and_declared():
    header = open(os.path.join(ROOT, "include", "blp_hip.h")).read()
    L = _L()
    for name in NEW:
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert getattr(L, name).argtypes is not None
    for lib in (build.LIB, build.HOOKS_LIB):
        exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
        assert set(NEW) <= names, (lib, set(NEW) - names)
    assert L.blp_version() == 60000


def test_support_matrix():
    L = _L()
    from blp_amd import ops
    for m in range(4):
        for dt in (F32, F16, BF16):
            for D in (64, 128, 256):
                assert L.blp_rank_sets_typed_supported(m, dt, D), (m, dt, D)
            for D in (0, -64, 32, 96, 300, 512, 768):
                assert not L.blp_rank_sets_typed_supported(m, dt, D), (m, dt, D)
        for dt in (-1, 3, 7):
            assert not L.blp_rank_sets_typed_supported(m, dt, 128), (m, dt)
    for m in (-1, 4):
        assert not L.blp_rank_sets_typed_supported(m, F16, 128)
    for rel_model in REL_MODELS:
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            assert ops.rank_sets_supported(rel_model, 128, dtype) and not ops.rank_sets_supported(rel_model, 300, dtype)
        assert not ops.rank_sets_supported(rel_model, 128, torch.float64)
    assert ops.rank_sets_supported("complex", 256) and not ops.rank_sets_supported("transe", 300)  # the two-argument form


def test_typed_workspace_equals_the_untyped_one():
    L = _L()
    for m, D in ((0, 64), (1, 128), (2, 256), (3, 128)):
        for qh, qt, G in ((0, 1, 1), (2, 2, 5), (100, 3, 474), (6894, 6894, 1644)):
            want = L.blp_rank_sets_workspace_bytes(m, D, qh, qt, G)
            assert want > 0
            for dt in (F32, F16, BF16):
                assert L.blp_rank_sets_typed_workspace_bytes(m, dt, D, qh, qt, G) == want, (m, D, dt)
    assert L.blp_rank_sets_typed_workspace_bytes(0, 3, 128, 2, 2, 5) == 0
    assert L.blp_rank_sets_typed_workspace_bytes(0, F16, 300, 2, 2, 5) == 0
    assert L.blp_rank_sets_typed_workspace_bytes(4, F16, 128, 2, 2, 5) == 0
    assert L.blp_rank_sets_typed_workspace_bytes(0, F16, 128, -1, 2, 5) == 0
    assert L.blp_rank_sets_typed_workspace_bytes(0, F16, 128, 2, 2, -1) == 0


def _args(**over):
    """Plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(model=0, table=1 << 20, dtype=F16, N=1000, D=128, ld=128, row_base=0, source=1 << 21, S=1000, ld_src=128,
             fixed_row=1 << 22, rel_emb=1 << 23, R=5, rel_id=1 << 24, true_row=1 << 25, q_head=2, q_tail=2, set_ptr=1 << 26,
             set_row=1 << 27, nnz=100, G=3, qh=1 << 28, qt=1 << 29, filter=None, counts=1 << 30, workspace=1 << 31, ws=1 << 20,
             device=0, stream=None)
    a.update(over)
    return a


def _typed(L, **over):
    a = _args(**over)
    f = a["filter"]
    return L.blp_rank_sets_typed(a["model"], a["table"], a["dtype"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"],
                                 a["ld_src"], a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["true_row"], a["q_head"],
                                 a["q_tail"], a["set_ptr"], a["set_row"], a["nnz"], a["G"], a["qh"], a["qt"],
                                 None if f is None else ctypes.byref(f), a["counts"], a["workspace"], a["ws"], a["device"], a["stream"])


def _untyped(L, **over):
    a = _args(**over)
    f = a["filter"]
    return L.blp_rank_sets(a["model"], a["table"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"], a["ld_src"],
                           a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["true_row"], a["q_head"], a["q_tail"], a["set_ptr"],
                           a["set_row"], a["nnz"], a["G"], a["qh"], a["qt"], None if f is None else ctypes.byref(f), a["counts"],
                           a["workspace"], a["ws"], a["device"], a["stream"])


def test_typed_argument_errors():
    L = _L()
    for dt in (F16, BF16):
        for ld in (132, 129, 130, 140):  # ld % 8 != 0 (132 would pass the f32 check)
            assert _typed(L, dtype=dt, ld=ld) == -1 and b"ld % 8 == 0" in L.blp_last_error(), (dt, ld)
            assert L.blp_last_error().startswith(b"blp_rank_sets_typed")
        assert _typed(L, dtype=dt, table=(1 << 20) + 8) == -1 and b"aligned" in L.blp_last_error()
        assert _typed(L, dtype=dt, table=None) == -1 and b"NULL table" in L.blp_last_error()
        assert _typed(L, dtype=dt, D=300, ld=304, ld_src=300) == -2 and b"not supported" in L.blp_last_error()
        filt = _lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 100)
        assert _typed(L, dtype=dt, filter=filt) == -1 and b"row_base" in L.blp_last_error()
        assert _typed(L, dtype=dt, row_base=100, filter=_lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 0)) == -1
        assert b"row_base" in L.blp_last_error()
        assert _typed(L, dtype=dt, ws=L.blp_rank_sets_workspace_bytes(0, 128, 2, 2, 3) - 1) == -4
        assert _typed(L, dtype=dt, q_head=0, q_tail=0) == 0
    for dt in (-1, 3, 99):
        assert _typed(L, dtype=dt) == -1 and b"unknown table dtype" in L.blp_last_error(), dt
    assert _typed(L, model=7) == -1 and b"unknown model" in L.blp_last_error()


def test_f32_dtype_answers_exactly_as_blp_rank_sets():
    """One set of argument checks: same status and same message, under blp_rank_sets' name."""
    L = _L()
    filt = _lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 100)
    cases = [dict(model=7), dict(D=300, ld=300, ld_src=300), dict(N=-1), dict(ld=64), dict(ld=130), dict(nnz=1 << 31),
             dict(q_head=1 << 30, q_tail=1), dict(table=None), dict(set_row=None), dict(G=0), dict(R=0), dict(table=(1 << 20) + 8), dict(ld_src=130), dict(filter=filt), dict(workspace=None), dict(ws=1),
             dict(q_head=0, q_tail=0)]
    for over in cases:  # (each one is refused before a launch)
        want = _untyped(L, **over)
        want_msg = L.blp_last_error() if want else b""
        got = _typed(L, dtype=F32, **over)
        got_msg = L.blp_last_error() if got else b""
        assert (got, got_msg) == (want, want_msg), over
        assert not want or want_msg.startswith(b"blp_rank_sets:"), want_msg
    for m in range(-1, 5):
        for D in (32, 64, 128, 256, 300):
            assert L.blp_rank_sets_typed_supported(m, F32, D) == L.blp_rank_sets_supported(m, D)


def test_rank_sets16_kernels_use_no_scratch():
    """Every 16-bit rank_sets_kernel and set-aware filter_finalize_kernel instantiation is in the built objects of both
    libraries (rank_sets16.hip: the linked library's fat binary holds one bundle per source, which the tool does not walk), with
    a private segment of 0 bytes and no spill in the code object's metadata, as tools/kernel_resources.py reads it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    for obj_dir in (build.OBJ, os.path.join(build.OBJ, build.HOOKS_VARIANT)):
        kernels = kernel_resources.kernels_of(os.path.join(obj_dir, "rank_sets16.hip.o"))
        for tag in ("DF16_", "DF16b"):  # _Float16, __bf16 in the mangled names
            ranking_kernels = [k for k in kernels if "rank_sets_kernel" in k and tag in k]
            finalize = [k for k in kernels if "filter_finalize_kernel" in k and "SetLookup" in k and tag in k]
            assert len(ranking_kernels) == 4 * 3 and len(finalize) == 4 * 3, (obj_dir, tag, len(ranking_kernels), len(finalize))
        assert len(kernels) == 2 * 2 * 12
        for k, v in kernels.items():
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)
    obj = os.path.join(build.OBJ, "rank_sets16.hip.o")
    # the hand-issued scalar loads of the reused TransE body: no result touched before its wait, VALU wait states kept
    assert not kernel_resources.early_uses_of_scalar_loads(obj)
    assert not kernel_resources.valu_sgpr_hazards(obj)


# ------------------------------------------------------------------------------------------- rank_in_sets on CPU tensors
def _model(rel_model, rel_w):
    m = models.LinkPrediction(rel_w.shape[1], rel_model, "margin", rel_w.shape[0], 0)
    with torch.no_grad():
        m.rel_emb.weight.copy_(torch.from_numpy(rel_w))
    return m


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("rel_model", REL_MODELS)
def test_cpu_route_on_a_16_bit_table_equals_the_widened_table(rel_model, dtype):
    g, f = golden(f"eval_toy_{rel_model}"), golden("filters_toy")
    table16 = torch.from_numpy(g["ent_emb"]).to(dtype)
    triples, ent2idx = torch.from_numpy(f["triples"]), torch.from_numpy(f["ent2idx"])
    index = utils.FilterIndex(torch.from_numpy(f["graph_edges"]))
    model = _model(rel_model, g["rel_w"])
    Q, N = 2 * triples.shape[0], table16.shape[0]
    rng = np.random.default_rng(5)
    sets = ranking.CandidateSets([rng.choice(N, n, replace=False) for n in (0, 1, 7, N, 20)])
    set_ids = torch.from_numpy(rng.integers(0, 5, Q))
    for add_true in (True, False):
        got = ranking.rank_in_sets(model, table16, triples, sets, ent2idx, set_ids=set_ids, filter_index=index, add_true=add_true)
        want = ranking.rank_in_sets(model, table16.float(), triples, sets, ent2idx, set_ids=set_ids, filter_index=index, add_true=add_true)
        assert got.dtype == torch.int32 and torch.equal(got, want), (rel_model, dtype, add_true)
    assert int(want[:, 1].max()) > 0 and bool((want[:, 3] < want[:, 1]).any())
