"""Filtered top-k inside shared candidate sets for TransE at any width (blp_topk_sets_wide): what can be checked without a device
-- the exports of both libraries, the _supported truth table, the workspace size and its stated bound, blp_topk_sets_typed's
argument refusals case for case through the new entry, the kernels of the new object (none with scratch) next to the pinned
counts of the objects it shares code with, and ranking.predict_links_in_sets on CPU tensors at D = 300 against the C oracle's
scores in numpy's stable order on the expanded sets (the yardstick tests/test_gpu_topk_sets_wide.py compares with)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from blp_amd import _lib, build, ops, ranking
from test_topk_sets_host import _model, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_topk_sets_wide_supported", "blp_topk_sets_wide_workspace_bytes", "blp_topk_sets_wide")
TRANSE, COMPLEX, DISTMULT, SIMPLE = (_lib.MODEL_IDS[m] for m in ("transe", "complex", "distmult", "simple"))
F32, F16, BF16 = 0, 1, 2
TORCH_DT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
WIDTHS = (0, 4, 6, 64, 68, 300, 768, 1024, 1028)
KS = (0, 1, 256, 257)


def _L():
    return _lib.lib()


def test_new_entry_points_are_exported_by_both_libraries_declared_and_bound():
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
    assert "Added after 6.0.0 without a version change" in header[header.index("blp_topk_sets_wide is"):header.index("int blp_topk_sets_wide_supported(")]
    assert list(L.blp_topk_sets_wide.argtypes) == list(L.blp_topk_sets_typed.argtypes)
    assert list(L.blp_topk_sets_wide_workspace_bytes.argtypes) == list(L.blp_topk_sets_typed_workspace_bytes.argtypes)
    assert callable(ops.topk_sets_wide) and callable(ops.topk_sets_wide_supported) and callable(ops.topk_sets_wide_workspace_bytes)
    assert _lib.KNOBS[-1] == "topk_sets_grid"  # no new knob: topk_sets_grid forces the wide kernel's grid too


def test_supported_grid():
    L = _L()
    for m, name in ((TRANSE, "transe"), (DISTMULT, "distmult"), (COMPLEX, "complex"), (SIMPLE, "simple"), (4, None), (-1, None)):
        for dt in (F32, F16, BF16, 3, -1):
            for D in WIDTHS:
                for k in KS:
                    want = int(m == TRANSE and dt in (F32, F16, BF16) and D % 4 == 0 and 4 <= D <= 1024 and 1 <= k <= 256)
                    assert L.blp_topk_sets_wide_supported(m, dt, D, k) == want, (m, dt, D, k)
                    if name is not None and dt in TORCH_DT:
                        assert ops.topk_sets_wide_supported(name, D, k, TORCH_DT[dt]) == bool(want), (name, dt, D, k)
    assert not ops.topk_sets_wide_supported("transe", 300, 10, torch.float64)
    assert ops.topk_sets_wide_supported("transe", 300, 10)  # the three-argument form
    assert not L.blp_topk_sets_wide_supported(TRANSE, F32, -64, 10)
    # the fixed-width entry points answer as before
    for D in (64, 128, 256):
        assert L.blp_topk_sets_supported(TRANSE, D, 10) and L.blp_topk_sets_typed_supported(COMPLEX, BF16, D, 10)
    assert not L.blp_topk_sets_supported(TRANSE, 300, 10) and not L.blp_topk_sets_typed_supported(TRANSE, F16, 768, 10)


def _chunk(k):
    return min(max(1, min(32, 24576 // (32 * k))), 16)


def _s_max(Q, nnz, k):
    """topk_sets_slabs_rule (blp_amd/csrc/topk_sets_kernel.h) with the wide chunk, restated."""
    chunks = -(-Q // _chunk(k))
    cap = -(-(-(-nnz // 64)) // 4)
    return max(1, min(512 // chunks if chunks else 1, cap))


def test_workspace_is_aligned_monotone_bounded_and_free_of_N_and_dtype():
    """Coefficient rows (head side 2 D floats per query, tail side D), G + 1 unit offsets, the partial lists, each part rounded
    up to 256 bytes: a multiple of 256, monotone in Q, G, k and nnz, the same for every table dtype, never below what one
    call uses, within the header's 8 (D + k) Q + 8 (G + 1) + 4 MiB; N is not an argument."""
    L = _L()
    up = lambda n: -(-n // 256) * 256
    bound = lambda D, Q, G, k: 8 * (D + k) * Q + 8 * (G + 1) + (4 << 20)
    ws = lambda D, qh, qt, G, nnz, k, dt=F32: L.blp_topk_sets_wide_workspace_bytes(TRANSE, dt, D, qh, qt, G, nnz, k)
    for D in (4, 68, 300, 768, 1024):
        for nnz in (0, 1, 10_000, 1_500_000, (1 << 31) - 1):
            for k in (1, 10, 64, 192, 256):
                last = 0
                for qh, qt in ((0, 1), (1, 0), (1, 1), (2, 2), (100, 3), (6894, 6894), (52870, 52870)):
                    n, Q = ws(D, qh, qt, 474, nnz, k), qh + qt
                    used = up(qh * 8 * D) + up(qt * 4 * D) + up(475 * 8) + up(Q * _s_max(Q, nnz, k) * k * 8)
                    assert n % 256 == 0 and n >= last and n > 0, (D, nnz, k, qh, qt)
                    assert used <= n <= bound(D, Q, 474, k), (D, nnz, k, qh, qt, n, used)
                    assert n == ws(D, qh, qt, 474, nnz, k, F16) == ws(D, qh, qt, 474, nnz, k, BF16)
                    assert n == ops.topk_sets_wide_workspace_bytes("transe", D, qh, qt, 474, nnz, k, torch.bfloat16)
                    last = n
            sizes = [ws(D, 300, 300, G, nnz, 10) for G in (1, 12, 474, 1644, 100000)]
            assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
            sizes = [ws(D, 300, 300, 474, nnz, k) for k in (1, 2, 10, 48, 49, 64, 96, 97, 192, 256)]
            assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
        for k in (1, 10, 256):
            for qh, qt in ((2, 2), (300, 300), (6894, 6894)):
                sizes = [ws(D, qh, qt, 474, nnz, k) for nnz in (0, 1, 64, 257, 10_000, 200_000, 1_500_000, (1 << 31) - 1)]
                assert sizes == sorted(sizes), (D, k, qh, qt)
        # few queries against long sets: more than one partial list per query, still inside the bound
        assert ws(D, 2, 2, 1, 1_000_000, 256) > ws(D, 2, 2, 1, 64, 256)
    assert len(L.blp_topk_sets_wide_workspace_bytes.argtypes) == 8  # model, dtype, D, q_head, q_tail, G, nnz, k: no N
    for D in (0, 6, 1028, -4):
        assert ws(D, 2, 2, 5, 10, 10) == 0, D
    for m in (COMPLEX, DISTMULT, SIMPLE, 7, -1):
        assert L.blp_topk_sets_wide_workspace_bytes(m, F32, 300, 2, 2, 5, 10, 10) == 0, m
    for dt in (3, -1, 99):
        assert ws(300, 2, 2, 5, 10, 10, dt) == 0, dt
    assert ws(300, -1, 2, 5, 10, 10) == 0 and ws(300, 2, -1, 5, 10, 10) == 0 and ws(300, 2, 2, -1, 10, 10) == 0
    assert ws(300, 2, 2, 5, -1, 10) == 0 and ws(300, 2, 2, 5, 10, 0) == 0 and ws(300, 2, 2, 5, 10, 257) == 0
    assert ops.topk_sets_wide_workspace_bytes("complex", 300, 2, 2, 5, 10, 10) == 0
    assert ops.topk_sets_wide_workspace_bytes("transe", 300, 2, 2, 5, 10, 10, torch.float64) == 0


def _wide(L, **over):
    """blp_topk_sets_wide with plausible (never dereferenced: every case fails its argument check) 256-byte aligned addresses."""
    a = dict(model=TRANSE, table=1 << 20, dtype=F32, N=1000, D=300, ld=304, row_base=0, source=1 << 21, S=1000, ld_src=300,
             fixed_row=1 << 22, rel_emb=1 << 23, R=5, rel_id=1 << 24, q_head=2, q_tail=2, k=10, set_ptr=1 << 26, set_row=1 << 27, nnz=100,
             G=3, qh=1 << 28, qt=1 << 29, filter=None, rows=1 << 30, scores=1 << 25, workspace=1 << 31, ws=1 << 24, device=0, stream=None)
    a.update(over)
    f = a["filter"]
    return L.blp_topk_sets_wide(a["model"], a["table"], a["dtype"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"],
                                a["ld_src"], a["fixed_row"], a["rel_emb"], a["R"], a["rel_id"], a["q_head"], a["q_tail"], a["k"],
                                a["set_ptr"], a["set_row"], a["nnz"], a["G"], a["qh"], a["qt"], None if f is None else ctypes.byref(f),
                                a["rows"], a["scores"], a["workspace"], a["ws"], a["device"], a["stream"])


@pytest.mark.parametrize("dt", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
def test_blp_topk_sets_typed_refusals_through_the_wide_entry(dt):
    """tests/test_topk_sets16_host.py's refusals of blp_topk_sets_typed, case for case, at D = 300 (ld = 304: % 8 == 0)."""
    L = _L()
    call = lambda **over: _wide(L, dtype=dt, **over)
    assert call(model=7) == -1 and b"unknown model" in L.blp_last_error()
    assert call(k=0) == -1 and b"k = 0" in L.blp_last_error() and L.blp_last_error().startswith(b"blp_topk_sets_wide")
    assert call(k=257) == -1 and call(k=-3) == -1
    for D in (0, 6, 1028, 2048, -128):
        assert call(D=D, ld=max((D + 7) // 8 * 8, 8), ld_src=max(D, 4)) == -2 and b"not supported" in L.blp_last_error(), D
        assert b"blp_topk_sets_wide_supported" in L.blp_last_error()
    for m in (DISTMULT, COMPLEX, SIMPLE):  # a bilinear model
        assert call(model=m) == -2 and b"not supported" in L.blp_last_error(), m
        assert call(model=m, D=128, ld=128, ld_src=128) == -2
    for name in ("N", "q_head", "q_tail", "nnz", "G", "row_base"):
        assert call(**{name: -1}) == -1 and b"negative" in L.blp_last_error(), name
    filt = _lib.BlpFilter(1 << 32, 1 << 33, 1 << 34, None, None, 0, 100)
    assert call(filter=filt) == -1 and b"row_base" in L.blp_last_error()
    assert call(row_base=100, filter=filt, workspace=None) == -4  # the same filter on its own shard passes the check
    assert call(filter=_lib.BlpFilter(None, 1 << 33, 1 << 34, None, None, 0, 0)) == -1 and b"filter" in L.blp_last_error()
    assert call(ld=302) == -1 and b"aligned" in L.blp_last_error()  # misaligned rows
    assert call(ld=296) == -1 and call(ld_src=302) == -1 and call(ld_src=296) == -1
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
    assert call(ws=L.blp_topk_sets_wide_workspace_bytes(TRANSE, dt, 300, 2, 2, 3, 100, 10) - 1) == -4
    assert call(workspace=(1 << 31) + 64) == -4
    assert call(q_head=0, q_tail=0) == 0  # no query: nothing to do, nothing touched
    assert call(q_head=0, q_tail=0, workspace=None, ws=0, G=0, set_ptr=None, qh=None, qt=None) == 0


def test_the_dtype_refusals():
    L = _L()
    for dt in (-1, 3, 99):
        assert _wide(L, dtype=dt) == -1 and b"unknown table dtype" in L.blp_last_error(), dt
    for dt in (F16, BF16):
        for ld in (300, 308, 301, 316):  # ld % 8 != 0 (300, 308 and 316 would pass the f32 check)
            assert _wide(L, dtype=dt, ld=ld) == -1 and b"aligned" in L.blp_last_error() and b"ld % 8 == 0" in L.blp_last_error(), (dt, ld)
        assert _wide(L, dtype=dt, ld=312, workspace=None) == -4
    assert _wide(L, dtype=F32, ld=300, workspace=None) == -4 and L.blp_last_error().startswith(b"blp_topk_sets_wide:")
    assert _wide(L, dtype=F32, ld=302) == -1 and b"ld % 4 == 0" in L.blp_last_error()
    # at a width both entries take, the wide entry's status is blp_topk_sets_typed's for every refusal, and so is the message
    # behind the entry's name
    import test_topk_sets16_host as typed
    for over in (dict(model=7), dict(k=0), dict(N=-1), dict(ld=64), dict(ld=132), dict(nnz=1 << 31), dict(table=None), dict(rows=None),
                 dict(table=(1 << 20) + 8), dict(G=0), dict(workspace=None), dict(ws=1), dict(q_head=1 << 23, k=256), dict(q_head=0, q_tail=0)):
        for dt in (F16, F32):
            want = typed._typed(L, dtype=dt, **over)
            want_msg = L.blp_last_error().split(b":", 1)[1] if want else b""
            got = _wide(L, **dict(dict(dtype=dt, D=128, ld=128, ld_src=128), **over))
            got_msg = L.blp_last_error().split(b":", 1)[1] if got else b""
            if want == -4:  # (the message names the entry's own workspace size)
                assert got == -4 and b"workspace must be 256-byte aligned" in got_msg and b"workspace must be 256-byte aligned" in want_msg
            else:
                assert (got, got_msg) == (want, want_msg), (over, dt)


def test_topk_sets_wide_kernels_use_no_scratch_and_the_pinned_objects_keep_their_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    for obj_dir in (build.OBJ, os.path.join(build.OBJ, build.HOOKS_VARIANT)):
        kernels = kernel_resources.kernels_of(os.path.join(obj_dir, "topk_sets_wide.hip.o"))
        assert len(kernels) == 4, (obj_dir, sorted(kernels))
        wide = [k for k in kernels if "topk_sets_wide_kernel" in k]
        assert len(wide) == 3 and len([k for k in kernels if "topk_sets_wide_coef" in k]) == 1
        for tag in ("IfE", "DF16_", "DF16b"):  # float, _Float16, __bf16 in the mangled names
            assert len([k for k in wide if tag in k]) == 1, (obj_dir, tag, wide)
        for k, v in kernels.items():
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)
        for k in wide:  # 4 x 9 KiB of transpose slabs + 24 KiB of lists are asked for at the launch: two workgroups per compute unit
            assert kernels[k]["vgpr_count"] <= 256, (k, kernels[k])
        # the objects the new one shares code with hold the kernels they held
        f32 = kernel_resources.kernels_of(os.path.join(obj_dir, "topk_sets.hip.o"))
        assert len(f32) == 13 and len([k for k in f32 if "topk_sets_kernel" in k]) == 12 and len([k for k in f32 if "topk_sets_unit_prefix" in k]) == 1
        assert len(kernel_resources.kernels_of(os.path.join(obj_dir, "topk_sets16.hip.o"))) == 24
        assert len(kernel_resources.kernels_of(os.path.join(obj_dir, "topk.hip.o"))) == 74
        rank = kernel_resources.kernels_of(os.path.join(obj_dir, "rank_sets_wide.hip.o"))
        assert len(rank) == 8 and len([k for k in rank if "rank_sets_wide_kernel" in k]) == 3, sorted(rank)
        assert all(v["private_segment_fixed_size"] == 0 for v in list(f32.values()) + list(rank.values()))


# ------------------------------------------------------------------------------------------- predict_links_in_sets on CPU tensors
def test_predict_links_in_sets_on_cpu_tensors_at_300_equals_the_oracle_on_the_expanded_sets(oracle):
    """The dense route on CPU tensors (what the device route is compared with) against blp_oracle's scores of the whole table,
    taken inside each query's set in numpy's stable order."""
    N, D, R, T, G = 150, 300, 5, 40, 8
    g = torch.Generator().manual_seed(300)
    table = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    table[7] = table[3]  # a tie
    rel_w = ((torch.rand(R, D, generator=g) - 0.5) * 0.25).numpy()
    model = _model("transe", rel_w)
    triples = torch.stack((torch.randint(0, N, (T,), generator=g), torch.randint(0, N, (T,), generator=g),
                           torch.randint(0, R, (T,), generator=g)), dim=1)
    ent2idx = torch.arange(N)
    rng = np.random.default_rng(301)
    sets = ranking.CandidateSets([rng.choice(N, n, replace=False) for n in (0, 1, N, 64, 65, 20, 100, 7)])
    set_ids = torch.from_numpy(rng.integers(0, G, 2 * T))
    set_ids[:3] = torch.tensor([2, 0, 1])
    tab, lists = table.numpy(), [np.sort(np.asarray(x, np.int64)) for x in sets.tolist()]
    h, t, r = triples[:, 0].numpy(), triples[:, 1].numpy(), triples[:, 2].numpy()
    pred = np.concatenate((oracle.score_all("transe", 0, tab, tab[t], rel_w[r]), oracle.score_all("transe", 1, tab, tab[h], rel_w[r])))
    for k in (1, 10, 70, N + 5):
        rows = np.full((2 * T, k), -1, np.int64)
        scores = np.full((2 * T, k), np.nan, np.float32)
        for q in range(2 * T):
            s = lists[int(set_ids[q])]
            o = s[np.argsort(-pred[q, s], kind="stable")][:k]
            rows[q, :len(o)], scores[q, :len(o)] = o, pred[q, o]
        got = ranking.predict_links_in_sets(model, table, triples, k, sets, ent2idx, set_ids=set_ids)
        _same(got, (torch.from_numpy(rows), torch.from_numpy(scores)))
    both = [q for q in range(2 * T) if 3 in lists[int(set_ids[q])] and 7 in lists[int(set_ids[q])]]
    assert both, "the tied rows must share a set somewhere"
    assert (rows[1] == -1).all() and (rows[:, -1] == -1).any() and (rows[:, 0] >= 0).sum() == 2 * T - int((set_ids == 0).sum())
