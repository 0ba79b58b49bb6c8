"""Top-k prediction over a 16-bit candidate table without a GPU (include/blp_hip.h: blp_topk_typed_supported,
blp_topk_typed_workspace_bytes, blp_topk_typed): the new entry points are exported and bound, which (model, dtype, D, k) they
take, the workspace bound, the argument refusals (checked before anything touches a device), the f32 entry behaving as
blp_topk, and no scratch memory in the new kernels (read from the built objects)."""
import ctypes
import os

import pytest
import torch

from blp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_topk_typed_supported", "blp_topk_typed_workspace_bytes", "blp_topk_typed")
F32, F16, BF16 = 0, 1, 2


def _L():
    return _lib.lib()


def test_new_entry_points_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "blp_hip.h")).read()
    L = _L()
    for name in NEW:
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert getattr(L, name).argtypes is not None
    assert L.blp_version() == 60000


def test_supported_grid():
    L = _L()
    for dt in (F32, F16, BF16):
        for m in range(4):
            for D in (64, 128, 256):
                assert L.blp_topk_typed_supported(m, dt, D, 1) and L.blp_topk_typed_supported(m, dt, D, 256)
                assert not L.blp_topk_typed_supported(m, dt, D, 0) and not L.blp_topk_typed_supported(m, dt, D, 257)
            for D in (32, 96, 300):
                assert not L.blp_topk_typed_supported(m, dt, D, 10)
        assert not L.blp_topk_typed_supported(4, dt, 128, 10)
    for dt in (3, -1):
        assert not L.blp_topk_typed_supported(0, dt, 128, 10)
    for m in range(5):
        for D in (64, 96, 128):
            for k in (0, 10, 257):
                assert L.blp_topk_typed_supported(m, F32, D, k) == L.blp_topk_supported(m, D, k)


def test_workspace_bound_flat_in_N_and_as_f32():
    L = _L()
    for dt in (F16, BF16):
        for m in range(4):
            for D in (64, 128, 256):
                for qh, qt in ((2, 2), (0, 128), (52870, 52870), (1, 0)):
                    Q = qh + qt
                    for k in (1, 10, 256):
                        sizes = [L.blp_topk_typed_workspace_bytes(m, dt, N, D, qh, qt, k) for N in (1_000_000, 4_600_000, 1 << 30)]
                        assert len(set(sizes)) == 1, (dt, m, D, Q, k, sizes)
                        assert 0 < sizes[0] <= 8 * (D + k) * Q + (4 << 20)
                        assert sizes[0] == L.blp_topk_workspace_bytes(m, 4_600_000, D, qh, qt, k)
    assert L.blp_topk_typed_workspace_bytes(0, 3, 1000, 128, 2, 2, 10) == 0
    assert L.blp_topk_typed_workspace_bytes(0, F16, 1000, 96, 2, 2, 10) == 0
    assert L.blp_topk_typed_workspace_bytes(0, F16, 1000, 128, 2, 2, 0) == 0


def _args(**over):
    """Plausible (never dereferenced: every case below fails its argument check) 256-byte aligned addresses."""
    a = dict(model=0, table=1 << 20, dtype=F16, N=1000, D=128, ld=128, row_base=0, source=1 << 21, S=1000, ld_src=128,
             fixed_row=1 << 22, rel_emb=1 << 23, R=5, rel_id=1 << 24, q_head=2, q_tail=2, k=10, filter=None, rows=1 << 25,
             scores=1 << 26, workspace=1 << 27, ws=1 << 30, device=0, stream=None)
    a.update(over)
    return a


def _typed(L, **over):
    a = _args(**over)
    f = a["filter"]
    return L.blp_topk_typed(a["model"], a["table"], a["dtype"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"],
                            a["ld_src"], a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["q_head"], a["q_tail"], a["k"],
                            None if f is None else ctypes.byref(f), a["rows"], a["scores"], a["workspace"], a["ws"],
                            a["device"], a["stream"])


def _plain(L, **over):
    a = _args(**over)
    f = a["filter"]
    return L.blp_topk(a["model"], a["table"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"], a["ld_src"],
                      a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["q_head"], a["q_tail"], a["k"],
                      None if f is None else ctypes.byref(f), a["rows"], a["scores"], a["workspace"], a["ws"], a["device"],
                      a["stream"])


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_bad_arguments(dtype):
    L = _L()
    assert _typed(L, dtype=3) == -1 and b"dtype 3" in L.blp_last_error()
    assert _typed(L, dtype=-1) == -1
    # a 16-bit table's row stride is in elements, a multiple of 8 (16-byte rows); for an f32 table ld % 4 == 0 suffices
    assert _typed(L, dtype=dtype, ld=132, workspace=None) == -1 and b"ld % 8" in L.blp_last_error()
    assert _typed(L, dtype=F32, ld=132, workspace=None) == -4
    assert _typed(L, dtype=dtype, table=(1 << 20) + 8) == -1  # base not 16-byte aligned
    assert _typed(L, dtype=dtype, k=0) == -1 and b"k = 0" in L.blp_last_error()
    assert _typed(L, dtype=dtype, k=257) == -1
    assert _typed(L, dtype=dtype, D=96, ld=96, ld_src=96) == -2
    assert _typed(L, dtype=dtype, model=7) == -1
    filt = _lib.BlpFilter(1 << 28, 1 << 29, 1 << 30, None, None, 0, 100)
    assert _typed(L, dtype=dtype, filter=filt) == -1 and b"row_base" in L.blp_last_error()
    assert _typed(L, dtype=dtype, rows=None) == -1
    assert _typed(L, dtype=dtype, scores=None) == -1
    assert _typed(L, dtype=dtype, source=None) == -1
    assert _typed(L, dtype=dtype, workspace=None) == -4
    assert _typed(L, dtype=dtype, ws=1) == -4
    assert _typed(L, dtype=dtype, workspace=(1 << 27) + 64) == -4  # not 256-byte aligned
    assert _typed(L, dtype=dtype, row_base=(1 << 31) - 10) == -1


def test_f32_entry_is_blp_topk():
    L = _L()
    filt = _lib.BlpFilter(1 << 28, 1 << 29, 1 << 30, None, None, 0, 100)
    cases = [dict(k=0), dict(k=257), dict(D=96, ld=96, ld_src=96), dict(model=7), dict(filter=filt), dict(rows=None),
             dict(scores=None), dict(workspace=None), dict(ws=1), dict(row_base=(1 << 31) - 10), dict(ld=130),
             dict(table=(1 << 20) + 8), dict(N=-1), dict(ld=64)]
    for over in cases:
        want = _plain(L, **over)
        want_msg = L.blp_last_error()
        assert want != 0, over
        assert _typed(L, dtype=F32, **over) == want, over
        assert L.blp_last_error() == want_msg, over
    for m in range(4):
        for D in (64, 128, 256):
            for qh, qt, k in ((2, 2, 10), (0, 97, 256), (52870, 52870, 10)):
                for N in (0, 50, 300_001, 4_600_000):
                    assert L.blp_topk_typed_workspace_bytes(m, F32, N, D, qh, qt, k) == L.blp_topk_workspace_bytes(m, N, D, qh, qt, k)


def test_ops_wrappers_take_a_dtype():
    from blp_amd import ops
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        assert ops.topk_supported("complex", 128, 10, dt)
        assert not ops.topk_supported("complex", 96, 10, dt)
        assert ops.topk_workspace_bytes("transe", 4_600_000, 128, 2, 2, 10, dt) == ops.topk_workspace_bytes("transe", 4_600_000, 128, 2, 2, 10)
    assert not ops.topk_supported("transe", 128, 10, torch.float64)
    assert ops.topk_supported("transe", 128, 10)  # the old signature


def test_topk16_kernels_use_no_scratch():
    import os
    import sys
    from blp_amd import build
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources
    kernels = kernel_resources.kernels_of(os.path.join(build.OBJ, "topk.hip.o"))
    new = [k for k in kernels if "topk_tiles16" in k or ("topk_rescore" in k and "DF16" in k)]
    assert len(new) == 2 * 2 * 12
    assert all(kernels[k]["private_segment_fixed_size"] == 0 for k in new), [k for k in new if kernels[k]["private_segment_fixed_size"]]
