"""Top-k link prediction for DistMult / ComplEx / SimplE at any width without a GPU (include/blp_hip.h:
blp_topk_wide_supported, blp_topk_wide_workspace_bytes, blp_topk_wide): the entry points are exported and bound with
blp_topk's signatures, which (model, D, k) they take -- and blp_topk_supported unchanged --, the workspace rule, every
argument refusal of blp_topk with the same status and message (checked before anything touches a device), the LDS the
launch code asks for at every corner, and no scratch memory or spilled vector register in the kernels (read from the
built object)."""
import ctypes
import os
import sys

import pytest

from blp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blp_topk_wide_supported", "blp_topk_wide_workspace_bytes", "blp_topk_wide")
TRANSE, DISTMULT, COMPLEX, SIMPLE = 0, 1, 2, 3
WIDTHS = (0, 4, 6, 64, 128, 300, 768, 1024, 1028, -64)
KS = (0, 1, 256, 257)


def _L():
    return _lib.lib()


def test_new_entry_points_are_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "blp_hip.h")).read()
    L = _L()
    for name in NEW:
        assert name in _lib.SYMBOLS and f"{name}(" in header
    assert L.blp_topk_wide.argtypes == L.blp_topk.argtypes and L.blp_topk_wide.restype == L.blp_topk.restype
    assert L.blp_topk_wide_workspace_bytes.argtypes == L.blp_topk_workspace_bytes.argtypes
    assert L.blp_topk_wide_workspace_bytes.restype == L.blp_topk_workspace_bytes.restype
    assert L.blp_topk_wide_supported.argtypes == L.blp_topk_supported.argtypes
    assert L.blp_version() == 60000
    # the header's note on the three entries
    doc = header[header.index("blp_topk for DistMult / ComplEx / SimplE at ANY width"):header.index("int blp_topk_wide_supported(")]
    assert "Added after 6.0.0 without a version change" in doc
    assert not hasattr(L, "blp_debug_topk_wide_lds_bytes")  # the product library gets the three entries and nothing else


def test_supported_grid():
    L = _L()
    for m in (TRANSE, DISTMULT, COMPLEX, SIMPLE, 4, -1):
        for D in WIDTHS:
            for k in KS:
                want = m in (DISTMULT, COMPLEX, SIMPLE) and D % 4 == 0 and 4 <= D <= 1024 and 1 <= k <= 256
                assert L.blp_topk_wide_supported(m, D, k) == int(want), (m, D, k)
                # blp_topk_supported is what it was
                assert L.blp_topk_supported(m, D, k) == int(m in range(4) and D in (64, 128, 256) and 1 <= k <= 256), (m, D, k)


def test_workspace_rule():
    L = _L()
    ws = L.blp_topk_wide_workspace_bytes
    for m in (DISTMULT, COMPLEX, SIMPLE):
        for k in (1, 10, 256):
            for qh, qt in ((1, 0), (0, 1), (4, 4), (19, 21), (140, 131), (1024, 1024), (52870, 52870), (1 << 20, 0)):
                Q = qh + qt
                last = 0
                for N in (0, 1, 63, 64, 65, 523, 14541, 1 << 17, (1 << 17) + 1, 4_600_000, 1 << 30):
                    n = ws(m, N, 300, qh, qt, k)
                    assert n == ws(m, N, 768, qh, qt, k) == ws(m, N, 4, qh, qt, k) == ws(DISTMULT, N, 1024, qh, qt, k), (m, N, qh, qt, k)
                    assert n % 256 == 0 and n >= last, (m, N, qh, qt, k)      # non-decreasing in N
                    assert Q * k * 8 <= n <= 8 * k * (Q + 16384) + 4096, (m, N, qh, qt, k, n)
                    # the header's formula: only the partial lists, (Q, S, k) 8-byte keys
                    chunks = -(-qh // 8) + -(-qt // 8)
                    S = max(1, min(2048 // chunks, -(-N // 64)))
                    assert n == -(-8 * k * Q * S // 256) * 256, (m, N, qh, qt, k)
                    last = n
                assert ws(m, 1 << 17, 300, qh, qt, k) == ws(m, 1 << 30, 300, qh, qt, k)  # constant from 2^17 rows on
    # 0: TransE, an unsupported width or k, negative sizes, Q x k >= 2^31
    assert ws(TRANSE, 1000, 300, 2, 2, 10) == 0 and ws(DISTMULT, 1000, 302, 2, 2, 10) == 0 and ws(DISTMULT, 1000, 300, 2, 2, 257) == 0
    assert ws(7, 1000, 300, 2, 2, 10) == 0
    assert ws(DISTMULT, -1, 300, 2, 2, 10) == 0 and ws(DISTMULT, 1000, 300, -1, 2, 10) == 0 and ws(DISTMULT, 1000, 300, 2, -1, 10) == 0
    assert ws(DISTMULT, 1000, 300, 1 << 30, 1 << 30, 1) == 0 and ws(DISTMULT, 1000, 300, 1 << 23, 0, 256) == 0
    assert ws(DISTMULT, 1000, 300, (1 << 23) - 1, 0, 256) > 0 and ws(DISTMULT, 1000, 300, (1 << 31) - 1, 0, 1) > 0


def _args(**over):
    """Plausible (never dereferenced: every case below fails its argument check) 256-byte aligned addresses."""
    a = dict(model=DISTMULT, table=1 << 20, N=1000, D=300, ld=300, row_base=0, source=1 << 21, S=1000, ld_src=300,
             fixed_row=1 << 22, rel_emb=1 << 23, R=5, rel_id=1 << 24, q_head=2, q_tail=2, k=10, filter=None, rows=1 << 25,
             scores=1 << 26, workspace=1 << 27, ws=1 << 30, device=0, stream=None)
    a.update(over)
    return a


def _call(fn, **over):
    a = _args(**over)
    f = a["filter"]
    return fn(a["model"], a["table"], a["N"], a["D"], a["ld"], a["row_base"], a["source"], a["S"], a["ld_src"], a["fixed_row"],
              a["rel_emb"], a["R"], a["rel_id"], a["q_head"], a["q_tail"], a["k"], None if f is None else ctypes.byref(f),
              a["rows"], a["scores"], a["workspace"], a["ws"], a["device"], a["stream"])


def _filter(seg_lo=1 << 28, seg_hi=1 << 29, values=1 << 30, ent2idx=None, ent2idx_len=0, row_base=0):
    return _lib.BlpFilter(seg_lo, seg_hi, values, None, ent2idx, ent2idx_len, row_base)


# every argument refusal of blp_topk (api.cpp: topk_call), in the order of its checks
REFUSALS = [
    (dict(model=7), -1, b"unknown model 7"),
    (dict(model=-1), -1, b"unknown model -1"),
    (dict(k=0), -1, b"k = 0 outside [1, 256]"),
    (dict(k=257), -1, b"k = 257 outside [1, 256]"),
    (dict(model=TRANSE), -2, b"not supported"),
    (dict(D=302, ld=304, ld_src=304), -2, b"not supported"),
    (dict(D=1028, ld=1028, ld_src=1028), -2, b"not supported"),
    (dict(D=0, ld=0, ld_src=0), -2, b"not supported"),
    (dict(N=-1), -1, b"negative size / row_base or ld < D"),
    (dict(q_head=-1), -1, b"negative size / row_base or ld < D"),
    (dict(q_tail=-1), -1, b"negative size / row_base or ld < D"),
    (dict(row_base=-1), -1, b"negative size / row_base or ld < D"),
    (dict(ld=296), -1, b"negative size / row_base or ld < D"),
    (dict(row_base=(1 << 31) - 10), -1, b"global rows must stay below 2^31 and Q x k below 2^31"),
    (dict(q_head=1 << 28), -1, b"global rows must stay below 2^31 and Q x k below 2^31"),
    (dict(rows=None), -1, b"NULL rows / scores"),
    (dict(scores=None), -1, b"NULL rows / scores"),
    (dict(source=None), -1, b"NULL source / fixed_row / rel_id / rel_emb, or R <= 0 / S <= 0"),
    (dict(fixed_row=None), -1, b"NULL source / fixed_row / rel_id / rel_emb, or R <= 0 / S <= 0"),
    (dict(rel_id=None), -1, b"NULL source / fixed_row / rel_id / rel_emb, or R <= 0 / S <= 0"),
    (dict(rel_emb=None), -1, b"NULL source / fixed_row / rel_id / rel_emb, or R <= 0 / S <= 0"),
    (dict(R=0), -1, b"NULL source / fixed_row / rel_id / rel_emb, or R <= 0 / S <= 0"),
    (dict(S=0), -1, b"NULL source / fixed_row / rel_id / rel_emb, or R <= 0 / S <= 0"),
    (dict(table=None), -1, b"NULL table"),
    (dict(table=(1 << 20) + 8), -1, b"must be 16-byte aligned, ld % 4 == 0, ld_src % 4 == 0, ld_src >= D"),
    (dict(ld=302), -1, b"must be 16-byte aligned, ld % 4 == 0, ld_src % 4 == 0, ld_src >= D"),
    (dict(source=(1 << 21) + 4), -1, b"must be 16-byte aligned, ld % 4 == 0, ld_src % 4 == 0, ld_src >= D"),
    (dict(ld_src=302), -1, b"must be 16-byte aligned, ld % 4 == 0, ld_src % 4 == 0, ld_src >= D"),
    (dict(ld_src=296), -1, b"must be 16-byte aligned, ld % 4 == 0, ld_src % 4 == 0, ld_src >= D"),
    (dict(rel_emb=(1 << 23) + 4), -1, b"must be 16-byte aligned, ld % 4 == 0, ld_src % 4 == 0, ld_src >= D"),
    (dict(filter=_filter(seg_lo=None)), -1, b"filter needs seg_lo, seg_hi and values (ent2idx_len >= 0)"),
    (dict(filter=_filter(seg_hi=None)), -1, b"filter needs seg_lo, seg_hi and values (ent2idx_len >= 0)"),
    (dict(filter=_filter(values=None)), -1, b"filter needs seg_lo, seg_hi and values (ent2idx_len >= 0)"),
    (dict(filter=_filter(ent2idx=1 << 31, ent2idx_len=-1)), -1, b"filter needs seg_lo, seg_hi and values (ent2idx_len >= 0)"),
    (dict(filter=_filter(row_base=100)), -1, b"filter row_base 100 differs from the call's row_base 0"),
    (dict(workspace=None), -4, b"workspace must be 256-byte aligned and >= "),
    (dict(ws=255), -4, b"workspace must be 256-byte aligned and >= "),
    (dict(workspace=(1 << 27) + 64), -4, b"workspace must be 256-byte aligned and >= "),
]


@pytest.mark.parametrize("over,status,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_are_blp_topk_s(over, status, message):
    """Reached with no device present: the status and the message, under this entry's name; blp_topk refuses the same
    arguments, at a width it takes, with the same status and the same text under its own name."""
    L = _L()
    assert _call(L.blp_topk_wide, **over) == status, over
    err = L.blp_last_error()
    assert err.startswith(b"blp_topk_wide: ") and message in err, err
    if over.get("model", DISTMULT) == TRANSE or "D" in over:
        return  # (the two entries differ in WHICH models and widths they refuse, by design -- and say so)
    narrow = dict(D=128, ld=128, ld_src=128)
    narrow.update({k: (v - 172 if k in ("ld", "ld_src") else v) for k, v in over.items()})
    assert _call(L.blp_topk, **narrow) == status, over
    theirs = L.blp_last_error()
    assert theirs.startswith(b"blp_topk: ")
    if status == -4:  # (the number of bytes wanted differs)
        assert message in theirs
    else:
        assert theirs[len(b"blp_topk: "):] == err[len(b"blp_topk_wide: "):].replace(b"ld=300", b"ld=128").replace(b"ld=296", b"ld=124")


def test_unsupported_message_names_what_is_taken():
    L = _L()
    assert _call(L.blp_topk_wide, model=TRANSE) == -2
    assert b"distmult / complex / simple" in L.blp_last_error() and b"blp_topk_wide_supported" in L.blp_last_error()


def test_empty_block_is_ok_without_a_device():
    L = _L()
    assert _call(L.blp_topk_wide, q_head=0, q_tail=0, workspace=None, source=None, fixed_row=None, rel_id=None) == 0
    # ... but only after the model / width / size / output checks, as blp_topk
    assert _call(L.blp_topk_wide, q_head=0, q_tail=0, model=TRANSE) == -2
    assert _call(L.blp_topk_wide, q_head=0, q_tail=0, N=-1) == -1
    assert _call(L.blp_topk_wide, q_head=0, q_tail=0, rows=None) == -1
    assert _call(L.blp_topk, q_head=0, q_tail=0, rows=None, D=128, ld=128, ld_src=128) == -1


def test_workspace_one_byte_short_is_refused():
    L = _L()
    for m, D, N, qh, qt, k in ((DISTMULT, 300, 1000, 2, 2, 10), (COMPLEX, 768, 14541, 100, 171, 256), (SIMPLE, 1024, 70, 9, 0, 1)):
        need = L.blp_topk_wide_workspace_bytes(m, N, D, qh, qt, k)
        assert need > 0
        assert _call(L.blp_topk_wide, model=m, D=D, ld=D, ld_src=D, N=N, q_head=qh, q_tail=qt, k=k, ws=need - 1) == -4
        assert f">= {need} bytes (got {need - 1})".encode() in L.blp_last_error()
    assert L.blp_topk_wide_workspace_bytes(DISTMULT, 1000, 300, 2, 2, 10) == 8 * 10 * 4 * 16 + 0  # 4 queries x 16 slabs of 10 keys


def test_ops_supported_mirrors_the_c_call():
    import torch
    from blp_amd import ops
    L = _L()
    for name, m in _lib.MODEL_IDS.items():
        for D in WIDTHS:
            for k in KS:
                assert ops.topk_wide_supported(name, D, k) == bool(L.blp_topk_wide_supported(m, D, k))
                assert not ops.topk_wide_supported(name, D, k, torch.bfloat16) and not ops.topk_wide_supported(name, D, k, torch.float16)
    assert ops.topk_wide_workspace_bytes("complex", 14541, 768, 100, 171, 10) == L.blp_topk_wide_workspace_bytes(2, 14541, 768, 100, 171, 10)
    assert not ops.topk_supported("distmult", 300, 10)  # (unchanged: predict_links routes on the pair)


def test_lds_of_every_corner_fits_the_cu():
    """The launch code's own LDS computation (hooks build: blp_debug_topk_wide_lds_bytes, the larger of the two sides): the
    coefficients of 8 queries plus the lists of 4 waves x 8 queries x k keys, within the CU's 160 KiB at every supported
    (model, D, k) -- the corners, and every width at the largest k."""
    H = _lib.hooks_lib()
    K_of = {DISTMULT: 2, COMPLEX: 4, SIMPLE: 3}  # coefficient arrays per query, the larger of the two sides
    worst = 0
    for m in (DISTMULT, COMPLEX, SIMPLE):
        for D in list(range(4, 1025, 4)):
            for k in (1, 10, 64, 255, 256):
                n = H.blp_debug_topk_wide_lds_bytes(m, D, k)
                terms = D if m == DISTMULT else D // 2
                n4 = (terms + 3) // 4 * 4
                coef = 8 * K_of[m] * n4 * 4
                assert n == coef + 4 * 8 * k * 8, (m, D, k, n)
                assert 0 < n <= 160 * 1024, (m, D, k, n)
                worst = max(worst, n)
    assert worst == H.blp_debug_topk_wide_lds_bytes(COMPLEX, 1024, 256) == 128 * 1024  # 64 KiB of coefficients + 64 KiB of lists
    assert H.blp_debug_topk_wide_lds_bytes(TRANSE, 300, 10) == 0 and H.blp_debug_topk_wide_lds_bytes(DISTMULT, 302, 10) == 0
    assert H.blp_debug_topk_wide_lds_bytes(DISTMULT, 300, 257) == 0


def test_kernels_use_no_scratch_and_spill_no_vector_register():
    from blp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = kernel_resources.kernels_of(os.path.join(build.OBJ, "topk_wide.hip.o"))
    passes = [k for k in kernels if "topk_wide" in k]
    assert len(passes) == 3 * 2 * 2 == len(kernels)  # model x side x (n < 512, n >= 512), and nothing else in the object
    assert not [k for k in kernels if "rank_all_wide_kernel" in k]
    for k in passes:
        assert kernels[k]["private_segment_fixed_size"] == 0, k
        assert kernels[k].get("vgpr_spill_count", 0) == 0, k
