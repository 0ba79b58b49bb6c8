"""Filtered top-k inside shared candidate sets on a 16-bit entity table, without a GPU (include/blp_hip.h:
blp_topk_sets_typed_supported, blp_topk_sets_typed_workspace_bytes, blp_topk_sets_typed): the entry points are exported by both
libraries, declared and bound, which (model, dtype, D, k) they take, the workspace equals the untyped one, blp_topk_sets'
argument refusals through the typed entry (checked before anything touches a device) plus the 16-bit ones, the kernels of the
new object (24, no scratch) next to the pinned counts of topk_sets.hip.o and topk.hip.o, and the CPU route of
predict_links_in_sets on a 16-bit table against the same route on the table widened to f32."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden
from blp_amd import _lib, build, ops, ranking, utils
import test_topk_sets_host as base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_topk_sets_typed_supported", "blp_topk_sets_typed_workspace_bytes", "blp_topk_sets_typed")
F32, F16, BF16 = 0, 1, 2


def _L():
    return _lib.lib()


def test_typed_entry_points_are_exported_by_both_libraries_declared_and_bound():
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
    assert _lib.KNOBS[-1] == "topk_sets_grid"  # no new knob: topk_sets_grid forces the 16-bit kernel's grid too


def test_supported_grid():
    L = _L()
    for m in range(4):
        for dt in (F32, F16, BF16):
            for D in (64, 128, 256):
                assert L.blp_topk_sets_typed_supported(m, dt, D, 1) and L.blp_topk_sets_typed_supported(m, dt, D, 256), (m, dt, D)
                assert not L.blp_topk_sets_typed_supported(m, dt, D, 0) and not L.blp_topk_sets_typed_supported(m, dt, D, 257), (m, dt, D)
            for D in (100, 300):
                assert not L.blp_topk_sets_typed_supported(m, dt, D, 10), (m, dt, D)
        for dt in (3, -1):
            assert not L.blp_topk_sets_typed_supported(m, dt, 128, 10), (m, dt)
    for dt in (F32, F16, BF16):
        assert not L.blp_topk_sets_typed_supported(4, dt, 128, 10) and not L.blp_topk_sets_typed_supported(-1, dt, 128, 10)
    for rel_model in REL_MODELS:
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            assert ops.topk_sets_supported(rel_model, 128, 10, dtype) and ops.topk_sets_supported(rel_model, 256, 256, dtype=dtype)
            assert not ops.topk_sets_supported(rel_model, 300, 10, dtype) and not ops.topk_sets_supported(rel_model, 128, 257, dtype)
        assert not ops.topk_sets_supported(rel_model, 128, 10, torch.float64)
    assert ops.topk_sets_supported("complex", 256, 256) and not ops.topk_sets_supported("transe", 300, 10)  # the three-argument form


def test_typed_workspace_equals_the_untyped_one():
    """Every tuple tests/test_topk_sets_host.py sweeps: the workspace does not depend on the storage type."""
    L = _L()
    tuples = []
    for m, D in ((0, 64), (1, 128), (2, 256), (3, 128)):
        for nnz in (0, 1, 10_000, 1_500_000, (1 << 31) - 1):
            for k in (1, 10, 192, 256):
                tuples += [(m, D, qh, qt, 474, nnz, k) for qh, qt in ((0, 1), (1, 1), (2, 2), (100, 3), (6894, 6894), (52870, 52870))]
            tuples += [(m, D, 300, 300, G, nnz, 10) for G in (1, 12, 474, 1644, 100000)]
            tuples += [(m, D, 300, 300, 474, nnz, k) for k in (1, 2, 10, 64, 96, 97, 192, 256)]
        tuples += [(m, D, 2, 2, 1, 1_000_000, 256), (m, D, 2, 2, 1, 64, 256)]
    tuples += [(0, 128, 300, 300, 474, 1000, 10)]
    for m, D, qh, qt, G, nnz, k in tuples:
        want = L.blp_topk_sets_workspace_bytes(m, D, qh, qt, G, nnz, k)
        assert want > 0
        for dt in (F32, F16, BF16):
            assert L.blp_topk_sets_typed_workspace_bytes(m, dt, D, qh, qt, G, nnz, k) == want, (m, dt, D, qh, qt, G, nnz, k)
    for dt in (F16, BF16):  # the untyped call's zeros
        assert L.blp_topk_sets_typed_workspace_bytes(1, dt, 300, 2, 2, 5, 10, 10) == 0
        assert L.blp_topk_sets_typed_workspace_bytes(7, dt, 128, 2, 2, 5, 10, 10) == 0
        assert L.blp_topk_sets_typed_workspace_bytes(0, dt, 128, -1, 2, 5, 10, 10) == 0
        assert L.blp_topk_sets_typed_workspace_bytes(0, dt, 128, 2, 2, -1, 10, 10) == 0
        assert L.blp_topk_sets_typed_workspace_bytes(0, dt, 128, 2, 2, 5, -1, 10) == 0
        assert L.blp_topk_sets_typed_workspace_bytes(0, dt, 128, 2, 2, 5, 10, 0) == 0
        assert L.blp_topk_sets_typed_workspace_bytes(0, dt, 128, 2, 2, 5, 10, 257) == 0
    for dt in (3, -1, 99):  # an unknown dtype
        assert L.blp_topk_sets_typed_workspace_bytes(0, dt, 128, 2, 2, 5, 10, 10) == 0
    # ops' sizing keeps its parameter list: no dtype
    assert ops.topk_sets_workspace_bytes("transe", 128, 300, 300, 474, 1000, 10) == L.blp_topk_sets_typed_workspace_bytes(0, F16, 128, 300, 300, 474, 1000, 10)


def _typed(L, **over):
    """blp_topk_sets_typed with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(model=0, table=1 << 20, dtype=F16, N=1000, D=128, ld=128, row_base=0, source=1 << 21, S=1000, ld_src=128,
             fixed_row=1 << 22, rel_emb=1 << 23, R=5, rel_id=1 << 24, q_head=2, q_tail=2, k=10, set_ptr=1 << 26, set_row=1 << 27, nnz=100,
             G=3, qh=1 << 28, qt=1 << 29, filter=None, rows=1 << 30, scores=1 << 25, workspace=1 << 31, ws=1 << 24, device=0, stream=None)
    a.update(over)
    f = a["filter"]
    return L.blp_topk_sets_typed(a["model"], a["table"], a["dtype"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"],
                                 a["ld_src"], a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["q_head"], a["q_tail"], a["k"],
                                 a["set_ptr"], a["set_row"], a["nnz"], a["G"], a["qh"], a["qt"], None if f is None else ctypes.byref(f),
                                 a["rows"], a["scores"], a["workspace"], a["ws"], a["device"], a["stream"])


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_blp_topk_sets_refusals_through_the_typed_entry(dt):
    """tests/test_topk_sets_host.py::test_bad_arguments, case for case, on a 16-bit table."""
    L = _L()
    call = lambda **over: _typed(L, dtype=dt, **over)
    assert call(model=7) == -1 and b"unknown model" in L.blp_last_error()
    assert call(k=0) == -1 and b"k = 0" in L.blp_last_error() and L.blp_last_error().startswith(b"blp_topk_sets_typed")
    assert call(k=257) == -1 and call(k=-3) == -1
    for D in (300, 100, 32):
        assert call(D=D, ld=(D + 7) // 8 * 8, ld_src=D) == -2 and b"not supported" in L.blp_last_error()
    for name in ("N", "q_head", "q_tail", "nnz", "G", "row_base"):
        assert call(**{name: -1}) == -1 and b"negative" in L.blp_last_error(), name
    filt = _lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 100)
    assert call(filter=filt) == -1 and b"row_base" in L.blp_last_error()
    assert call(row_base=100, filter=filt, workspace=None) == -4  # the same filter on its own shard passes the check
    assert call(filter=_lib.BlpFilter(None, 1 << 33, 1 << 34, None, None, 0, 0)) == -1 and b"filter" in L.blp_last_error()
    assert call(ld=130) == -1 and b"aligned" in L.blp_last_error()  # misaligned rows
    assert call(ld=64) == -1 and call(ld_src=130) == -1 and call(ld_src=64) == -1
    assert call(table=(1 << 20) + 8) == -1 and b"aligned" in L.blp_last_error()
    assert call(rows=None) == -1 and b"NULL" in L.blp_last_error()
    assert call(scores=None) == -1 and b"NULL" in L.blp_last_error()
    for name in ("table", "source", "fixed_row", "rel_emb", "rel_id", "set_ptr", "set_row", "qh", "qt"):
        assert call(**{name: None}) == -1 and b"NULL" in L.blp_last_error(), name
    assert call(G=0) == -1 and call(R=0) == -1 and call(S=0) == -1
    assert call(q_head=1 << 23, q_tail=1, k=256) == -1 and b"2^31" in L.blp_last_error()
    assert call(q_head=(1 << 31) // 10, q_tail=1, k=10) == -1
    assert call(nnz=1 << 31) == -1 and b"nnz" in L.blp_last_error()
    assert call(row_base=(1 << 31) - 10) == -1
    assert call(workspace=None) == -4 and b"workspace" in L.blp_last_error()
    assert call(ws=1) == -4
    assert call(ws=L.blp_topk_sets_workspace_bytes(0, 128, 2, 2, 3, 100, 10) - 1) == -4
    assert call(workspace=(1 << 31) + 64) == -4
    assert call(q_head=0, q_tail=0) == 0  # no query: nothing to do, nothing touched
    assert call(q_head=0, q_tail=0, workspace=None, ws=0, G=0, set_ptr=None, qh=None, qt=None) == 0


def test_the_refusals_of_the_typed_entry_alone():
    L = _L()
    for dt in (-1, 3, 99):
        assert _typed(L, dtype=dt) == -1 and b"unknown table dtype" in L.blp_last_error(), dt
    for dt in (F16, BF16):
        for ld in (132, 129, 130, 140):  # ld % 8 != 0 (132 and 140 would pass the f32 check)
            assert _typed(L, dtype=dt, ld=ld) == -1 and b"aligned" in L.blp_last_error() and b"ld % 8 == 0" in L.blp_last_error(), (dt, ld)
        assert _typed(L, dtype=dt, ld=136, workspace=None) == -4
        assert _typed(L, dtype=dt, table=(1 << 20) + 8) == -1 and b"aligned" in L.blp_last_error()  # 8-byte, not 16-byte aligned
    # BLP_DTYPE_F32 is blp_topk_sets itself: ld % 4 == 0 is accepted up to the workspace check, under blp_topk_sets' name
    assert _typed(L, dtype=F32, ld=132, workspace=None) == -4 and L.blp_last_error().startswith(b"blp_topk_sets:")
    assert _typed(L, dtype=F32, ld=130) == -1 and b"ld % 4 == 0" in L.blp_last_error()
    for over in (dict(model=7), dict(k=0), dict(D=300, ld=300, ld_src=300), dict(N=-1), dict(ld=64), dict(nnz=1 << 31), dict(table=None),
                 dict(table=(1 << 20) + 8), dict(rows=None), dict(G=0), dict(workspace=None), dict(ws=1), dict(q_head=0, q_tail=0)):
        want = base._call(L, **over)
        want_msg = L.blp_last_error() if want else b""
        got = _typed(L, dtype=F32, **over)
        got_msg = L.blp_last_error() if got else b""
        assert (got, got_msg) == (want, want_msg), over


def test_topk_sets16_kernels_use_no_scratch_and_the_pinned_objects_keep_their_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    for obj_dir in (build.OBJ, os.path.join(build.OBJ, build.HOOKS_VARIANT)):
        kernels = kernel_resources.kernels_of(os.path.join(obj_dir, "topk_sets16.hip.o"))
        assert len(kernels) == 24 and all("topk_sets_kernel" in k for k in kernels), (obj_dir, sorted(kernels))
        for tag in ("DF16_", "DF16b"):  # _Float16, __bf16 in the mangled names
            assert len([k for k in kernels if tag in k]) == 4 * 3, (obj_dir, tag)
        for k, v in kernels.items():
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)
        f32 = kernel_resources.kernels_of(os.path.join(obj_dir, "topk_sets.hip.o"))
        assert len(f32) == 13 and len([k for k in f32 if "topk_sets_kernel" in k]) == 12
        assert all(v["private_segment_fixed_size"] == 0 for v in f32.values())
        assert len(kernel_resources.kernels_of(os.path.join(obj_dir, "topk.hip.o"))) == 74


# ------------------------------------------------------------------------------------------- predict_links_in_sets on CPU tensors
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("rel_model", REL_MODELS)
def test_cpu_route_on_a_16_bit_table_equals_the_widened_table(rel_model, dtype):
    g, f = golden(f"eval_toy_{rel_model}"), golden("filters_toy")
    table16 = torch.from_numpy(g["ent_emb"]).to(dtype)
    triples, ent2idx = torch.from_numpy(f["triples"]), torch.from_numpy(f["ent2idx"])
    index = utils.FilterIndex(torch.from_numpy(f["graph_edges"]))
    model = base._model(rel_model, g["rel_w"])
    Q, N = 2 * triples.shape[0], table16.shape[0]
    rng = np.random.default_rng(5)
    sets = ranking.CandidateSets([rng.choice(N, n, replace=False) for n in (0, 1, 7, N, 20)])
    set_ids = torch.from_numpy(rng.integers(0, 5, Q))
    for k in (1, 4, N + 2):
        for filt in (None, index):
            got = ranking.predict_links_in_sets(model, table16, triples, k, sets, ent2idx, set_ids=set_ids, filter_index=filt)
            want = ranking.predict_links_in_sets(model, table16.float(), triples, k, sets, ent2idx, set_ids=set_ids, filter_index=filt)
            assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[0].shape == (Q, k)
            base._same(got, want)
    assert bool((want[0] >= 0).any()) and bool((want[0] == -1).any())
