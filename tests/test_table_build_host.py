"""The entity-table build without a GPU: plain float64 restatements of the three operations the table-build kernels fuse
(blp_project_rows, blp_bow_rows, blp_dkrl_rows), written from the reference's expressions line by line with basic torch
operations only -- BOW models.py:146-155, DKRL models.py:174-204, enc_linear models.py:110-111, F.normalize models.py:38-43 --
plus the float32 sequential restatement of BOW in the order bow.hip's header documents.  They are pinned here, where they can
run: against the reference's own outputs (tests/golden/encoders_*.npz, within 2e-6) and against the stock modules in float64 on
every edge input of tests/test_gpu_table_build_edges.py (within 1e-12, NaN rows by position).  The edge inputs are built here;
every builder asserts on the host that its input reaches the case it is for."""
import functools
import zlib

import numpy as np
import pytest
import torch

from conftest import golden, golden_names

F64, F32 = torch.float64, torch.float32
V = 60            # rows of the word table of every case
DIM = 128         # DKRL output width (the only one blp_dkrl_rows takes)
NORM_FLOOR = 0.05  # normalised cases: the float64 norm before F.normalize stays above this (no amplified rounding error)


class Case:
    """One edge input: raw float32 / int64 CPU tensors as the kernels take them, the rows whose result is NaN by expectation."""

    def __init__(self, **fields):
        self.nan_rows = ()
        self.__dict__.update(fields)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------------------------ the restatements
def normalize_restated(x):
    """F.normalize(x, dim=-1) (models.py:38-43): x / max(||x||_2, 1e-12)."""
    return x / torch.sqrt(torch.sum(x * x, dim=-1, keepdim=True)).clamp(min=1e-12)


def linear_restated(x, w, normalize, dtype=F64):
    """enc_linear (models.py:110-111; nn.Linear without bias), then F.normalize if ``normalize``."""
    out = x.to(dtype) @ w.to(dtype).t()
    return normalize_restated(out) if normalize else out


def bow_restated(tok, mask, word, normalize, dtype=F64):
    """models.py:146-155, then F.normalize if ``normalize``."""
    if mask is None:
        mask = torch.ones(tok.shape, dtype=dtype)                     # :147-148
    mask = mask.to(dtype)
    embs = word.to(dtype)[tok]                                        # :150   (B, L, E)
    lengths = torch.sum(mask, dim=-1, keepdim=True)                   # :151
    embs = torch.sum(mask.unsqueeze(-1) * embs, dim=1)                # :152
    embs = embs / lengths                                             # :153
    return normalize_restated(embs) if normalize else embs


def bow_sequential_f32(tok, mask, word):
    """BOW without normalisation in float32, in the order bow.hip's header states: the tokens walked in order, the product
    mask * vector and the sum rounded separately, the length summed in order, one IEEE division.  numpy's float32 arithmetic
    rounds every operation on its own."""
    tok, word = tok.numpy(), word.numpy()
    assert word.dtype == np.float32
    mask = None if mask is None else mask.numpy()
    n, L = tok.shape
    out = np.empty((n, word.shape[1]), np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            acc, length = np.zeros(word.shape[1], np.float32), np.float32(0)
            for l in range(L):
                m = np.float32(1) if mask is None else mask[i, l]
                assert m.dtype == np.float32
                prod = m * word[tok[i, l]]
                acc = acc + prod
                length = length + m
            out[i] = acc / length
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def _conv_k2(x, w, b):
    """nn.Conv1d(kernel_size=2) over F.pad(x, [0, 1]) with positions on dim 1: out[:, l] = b + x[:, l] W[..., 0]^T + x[:, l + 1] W[..., 1]^T."""
    x = torch.cat((x, torch.zeros(x.shape[0], 1, x.shape[2], dtype=x.dtype)), dim=1)
    return b + x[:, :-1] @ w[:, :, 0].t() + x[:, 1:] @ w[:, :, 1].t()


def dkrl_preact(tok, mask, word, w1, b1, dtype=F64):
    """models.py:175-188: the masked output of conv1, (B, L, C), and the mask it was multiplied by."""
    if mask is None:
        mask = torch.ones(tok.shape, dtype=dtype)                     # :175-176
    mask = mask.to(dtype)
    embs = word.to(dtype)[tok] * mask.unsqueeze(-1)                   # :178
    embs = _conv_k2(embs, w1.to(dtype), b1.to(dtype))                 # :186-187
    return embs * mask.unsqueeze(-1), mask                            # :188


def dkrl_restated(tok, mask, word, w1, b1, w2, b2, normalize, dtype=F64, pool=None):
    """models.py:174-204, then F.normalize if ``normalize``.  (``pool``: another max-pool of the (B, J, k, C) windows, for
    the builders that show what a wrong pool would give.)"""
    embs, mask = dkrl_preact(tok, mask, word, w1, b1, dtype)
    B, L, C = embs.shape
    k = 4 if L >= 4 else (1 if L == 1 else 2)                         # :189-194
    J = L // k                                                        # (F.max_pool1d floors)
    windows, mwin = embs[:, :J * k].reshape(B, J, k, C), mask[:, :J * k].reshape(B, J, k)
    embs = windows.max(dim=2).values if pool is None else pool(windows, mwin)   # :195
    mask = mwin.max(dim=2).values                                     # :196
    embs = torch.tanh(embs)                                           # :197
    embs = _conv_k2(embs, w2.to(dtype), b2.to(dtype))                 # :198-199
    lengths = torch.sum(mask, dim=-1, keepdim=True)                   # :200
    embs = torch.sum(embs * mask.unsqueeze(-1), dim=1) / lengths      # :201
    embs = torch.tanh(embs)                                           # :202
    return normalize_restated(embs) if normalize else embs


def errors(got, want64, want32):
    """(err_fused, err32) of the tolerance rule: the largest absolute difference from the float64 restatement of the kernel's
    output and of the same restatement evaluated in float32, over the rows that are numbers.  NaN rows are compared by
    position: the output is NaN exactly where the float64 restatement is, and those are whole rows."""
    nan = torch.isnan(want64)
    assert torch.equal(torch.isnan(got), nan), torch.nonzero(torch.isnan(got) != nan)[:5]
    assert torch.equal(nan.all(dim=-1), nan.any(dim=-1))
    assert not torch.isnan(want32[~nan]).any()
    if nan.all():
        return 0.0, 0.0
    return (got.double() - want64)[~nan].abs().max().item(), (want32.double() - want64)[~nan].abs().max().item()


def assert_within_rule(got, want64, want32):
    """err_fused <= max(4 err32, 2e-6): the rule of test_dkrl_table_build_is_one_kernel."""
    err_fused, err32 = errors(got, want64, want32)
    assert err_fused <= max(4 * err32, 2e-6), f"err_fused={err_fused:.3e} err32={err32:.3e}"


# ------------------------------------------------------------------------------------------------ masks
def make_mask(kind, n, L, g, masked_rows=(), window=None):
    """(n, L) float32 mask of one kind, or None; every kind asserts what it is for."""
    if kind == "none":
        assert not masked_rows
        return None
    live = torch.randint(1, L + 1, (n,), generator=g) if L else torch.zeros(n, dtype=torch.int64)
    if L:
        live[0] = L
    if kind == "every_prefix":
        assert n == L
        live = torch.arange(1, L + 1)
    prefix = (torch.arange(L).unsqueeze(0) < live.unsqueeze(1)).float()
    if kind in ("prefix", "every_prefix"):
        mask = prefix
    elif kind == "fractional":  # values in (0, 2] on a prefix
        mask = prefix * (2.0 - 2.0 * torch.rand(n, L, generator=g))
        on = mask[prefix > 0]
        assert (on > 0).all() and (on <= 2).all() and ((on != 1) & (on != 0)).any()
    elif kind == "holes":  # zeros strictly inside the live span
        assert L >= 3
        mask = torch.ones(n, L)
        for i in range(n):
            holes = torch.randperm(L - 2, generator=g)[:max(1, (L - 2) // 3)] + 1
            mask[i, holes] = 0.0
        for row in mask:
            on = torch.nonzero(row).flatten()
            assert (row[on[0]:on[-1] + 1] == 0).any()
    elif kind == "masked_window":  # a fully masked pooling window between live ones
        assert L >= 12 and 1 <= window < L // 4 - 1
        mask = 2.0 - 2.0 * torch.rand(n, L, generator=g)
        mask[:, 4 * window:4 * window + 4] = 0.0
        pooled = mask[:, :L // 4 * 4].reshape(n, L // 4, 4).max(dim=2).values
        assert (pooled[:, window] == 0).all() and (pooled[:, window - 1] > 0).all() and (pooled[:, window + 1] > 0).all()
    else:
        raise ValueError(kind)
    for r in masked_rows:
        mask[r] = 0.0
    dead = torch.nonzero(mask.sum(-1) == 0).flatten().tolist() if L else list(range(n))
    assert dead == sorted(masked_rows) or L == 0, (dead, masked_rows)
    return mask


# ------------------------------------------------------------------------------------------------ projection inputs
PROJECT_E = (72, 96, 160, 200, 36)   # 3, 3, 5, 7 and 2 staging steps; 72, 200 and 36 with a partial last step
PROJECT_D = (64, 128, 256)
PROJECT_N = (1, 63, 64, 65, 70)      # around the workgroup's 64 rows
PROJECT_SHAPES = tuple((E, D, PROJECT_N[i % 5]) for i, (E, D) in enumerate((E, D) for E in PROJECT_E for D in PROJECT_D))
assert {s[2] for s in PROJECT_SHAPES} == set(PROJECT_N)
assert [(E + 31) // 32 for E in PROJECT_E] == [3, 3, 5, 7, 2] and [E % 32 != 0 for E in PROJECT_E] == [True, False, False, True, True]


@functools.lru_cache(maxsize=None)
def project_case(E, D, n, special=None):
    """x as a strided view ((n, 3, E)[:, 0], as the [CLS] rows are), weights divided by sqrt(E): outputs of magnitude ~ 1.
    ``special`` "nonfinite": one row holding a NaN and one holding an Inf among finite ones; "zero": one all-zero row."""
    g = _gen(f"project {E} {D} {n} {special}")
    seq = torch.randn(n, 3, E, generator=g)
    w = torch.randn(D, E, generator=g) / E ** 0.5
    case = Case(seq=seq, x=seq[:, 0], w=w, E=E, D=D, n=n, nonfinite_rows=(), zero_rows=())
    if special == "nonfinite":
        assert n >= 4
        seq[1, 0, E - 3] = float("nan")
        seq[n - 2, 0, 5] = float("inf")
        case.nonfinite_rows = (1, n - 2)
        want = linear_restated(case.x, w, False)
        assert torch.isnan(want[1]).all() and torch.isinf(want[n - 2]).all()
        rest = [r for r in range(n) if r not in case.nonfinite_rows]
        assert torch.isfinite(want[rest]).all()
    elif special == "zero":
        seq[n // 2, 0] = 0.0
        case.zero_rows = (n // 2,)
    else:
        assert special is None
    rest = [r for r in range(n) if r not in case.nonfinite_rows + case.zero_rows]
    assert (linear_restated(case.x, w, False)[rest].norm(dim=-1) > 1.0).all()   # ~ sqrt(D): well away from 0
    assert case.x.stride(0) == 3 * E and not case.x.is_contiguous() or n == 1
    return case


PROJECT_SPECIALS = ((72, 64, 65, "nonfinite"), (200, 128, 70, "nonfinite"), (96, 256, 5, "nonfinite"),
                    (72, 128, 65, "zero"), (36, 64, 4, "zero"))


# ------------------------------------------------------------------------------------------------ BOW inputs
BOW_E = (4, 256, 260, 512, 516, 1020, 1024)   # one live lane; the sweeps' boundaries from both sides
BOW_L = (0, 1, 2, 3, 5, 8, 33)                # tokens are walked four at a time
BOW_N = (1, 2, 3, 5)                          # four entities per workgroup
BOW_CASES = {}
for _i, _E in enumerate(BOW_E):
    BOW_CASES[f"E{_E}-L5-n{BOW_N[_i % 4]}-{('fractional', 'prefix', 'holes', 'none')[_i % 4]}"] = \
        (_E, 5, BOW_N[_i % 4], ("fractional", "prefix", "holes", "none")[_i % 4], ())
_i = 0
for _L in BOW_L:
    for _kind in ("none", "prefix", "fractional", "holes"):
        if (_kind == "holes" and _L < 3) or (_kind == "fractional" and _L == 0):
            continue
        BOW_CASES[f"E260-L{_L}-n{BOW_N[_i % 4]}-{_kind}"] = (260, _L, BOW_N[_i % 4], _kind, ())
        _i += 1
BOW_CASES["E260-L8-n5-fractional-rows1,3-fully-masked"] = (260, 8, 5, "fractional", (1, 3))
BOW_CASES["E1024-L3-n3-prefix-row0-fully-masked"] = (1024, 3, 3, "prefix", (0,))
BOW_CASES["E4-L33-n2-holes-row1-fully-masked"] = (4, 33, 2, "holes", (1,))
assert {c[1] for c in BOW_CASES.values()} == set(BOW_L) and {c[2] for c in BOW_CASES.values()} == set(BOW_N)


@functools.lru_cache(maxsize=None)
def bow_case(name):
    E, L, n, kind, masked_rows = BOW_CASES[name]
    g = _gen("bow " + name)
    word = torch.randn(V, E, generator=g) * 0.3 + 0.1    # (a common offset: the mean of many rows stays away from 0)
    tok = torch.randint(0, V, (n, L), generator=g)      # (masked positions keep random ids: the mask alone decides)
    mask = make_mask(kind, n, L, g, masked_rows)
    case = Case(name=name, tok=tok, mask=mask, word=word, E=E, L=L, n=n, nan_rows=tuple(range(n)) if L == 0 else masked_rows)
    want = bow_restated(tok, mask, word, False)
    nan = torch.isnan(want)
    assert sorted(torch.nonzero(nan.any(-1)).flatten().tolist()) == sorted(case.nan_rows) and torch.equal(nan.any(-1), nan.all(-1))
    assert (want[~nan.any(-1)].norm(dim=-1) > NORM_FLOOR).all()
    return case


BOW_BAD_ID_CASES = ("E260-L5-n3-fractional", "E1024-L5-n3-holes")
BAD_ID_PLACES = ("live", "masked")


@functools.lru_cache(maxsize=None)
def bow_bad_id_case(name, where):
    """The clean input of a bad-token test: position (row, at) -- the last token of a row in the middle -- is live or masked
    (padding) and the rest of the row is not all padding; the test puts the bad id there."""
    base = bow_case(name)
    mask = torch.ones(base.tok.shape) if base.mask is None else base.mask.clone()
    row, at = base.n // 2, base.L - 1
    mask[row, at] = 0.0 if where == "masked" else 1.0
    assert (mask[row, :at] > 0).any() and not torch.isnan(bow_restated(base.tok, mask, base.word, False)).any()
    return Case(**{**base.__dict__, "mask": mask, "row": row, "at": at})


def all_bow_cases():
    cases = {name: functools.partial(bow_case, name) for name in BOW_CASES}
    for name in BOW_BAD_ID_CASES:
        for where in BAD_ID_PLACES:
            cases[f"{name}-bad-id-place-{where}"] = functools.partial(bow_bad_id_case, name, where)
    return cases


# ------------------------------------------------------------------------------------------------ DKRL inputs
DKRL_E = (72, 96, 160, 200, 8)       # 3, 3, 5, 7 and 1 staging steps; 72, 200 and 8 with a partial last step
DKRL_L = (4, 5, 6, 8, 31, 32, 33, 36, 60, 63, 64)
DKRL_SPLITS = (0, 1, 2, 4)           # the dkrl_split knob: 0 = the launcher's own choice
DKRL_N = (1, 2, 3, 5)
# (L, split, n): every L at every split (so every (split, L > 32) pair), n walking 1, 2, 3, 5 against both
DKRL_SPLIT_SHAPES = tuple((L, split, DKRL_N[(i + j) % 4]) for i, L in enumerate(DKRL_L) for j, split in enumerate(DKRL_SPLITS))
assert {(s, L) for L, s, _ in DKRL_SPLIT_SHAPES} >= {(s, L) for s in DKRL_SPLITS for L in DKRL_L if L > 32}
assert all({n for L, s, n in DKRL_SPLIT_SHAPES if s == split} == set(DKRL_N) for split in DKRL_SPLITS)


def dkrl_weights(E, g, bias1=(-0.2, 0.2), scale1=1.0):
    """Word table, conv1 and conv2 as nn.Conv1d initialises them (uniform in +- 1 / sqrt(fan_in)), biases that matter."""
    word = torch.randn(V, E, generator=g) * 0.3
    u = lambda *shape: 2.0 * torch.rand(*shape, generator=g) - 1.0
    w1 = u(DIM, E, 2) * scale1 / (2 * E) ** 0.5
    b1 = bias1[0] + (bias1[1] - bias1[0]) * torch.rand(DIM, generator=g)
    w2 = u(DIM, DIM, 2) / (2 * DIM) ** 0.5
    b2 = u(DIM) * 0.2
    return dict(word=word, w1=w1, b1=b1, w2=w2, b2=b2)


def dkrl_args(case):
    return case.tok, case.mask, case.word, case.w1, case.b1, case.w2, case.b2


def _finish_dkrl(case):
    """The checks every DKRL case shares: NaN exactly in the fully masked rows, the other rows' norm well away from 0."""
    want = dkrl_restated(*dkrl_args(case), False)
    nan = torch.isnan(want)
    assert sorted(torch.nonzero(nan.any(-1)).flatten().tolist()) == sorted(case.nan_rows) and torch.equal(nan.any(-1), nan.all(-1))
    assert (want[~nan.any(-1)].norm(dim=-1) > NORM_FLOOR).all()
    assert case.tok.shape[0] <= 70 and case.tok.shape[1] <= 64 and case.word.shape[0] <= 200
    return case


@functools.lru_cache(maxsize=None)
def dkrl_case(E, L, n, kind, masked_rows=(), window=None):
    g = _gen(f"dkrl {E} {L} {n} {kind} {masked_rows} {window}")
    tok = torch.randint(0, V, (n, L), generator=g)      # (masked positions keep random ids: the mask alone decides)
    mask = make_mask(kind, n, L, g, masked_rows, window)
    return _finish_dkrl(Case(tok=tok, mask=mask, E=E, L=L, n=n, nan_rows=tuple(masked_rows), **dkrl_weights(E, g)))


def _max_over_live(windows, mwin):
    """A WRONG pool: the maximum over the live positions of a window only (a masked position's 0 never wins)."""
    live = (mwin > 0).unsqueeze(-1)
    best = torch.where(live, windows, torch.full_like(windows, -float("inf"))).max(dim=2).values
    return torch.where(live.any(dim=2), best, torch.zeros_like(best))


@functools.lru_cache(maxsize=None)
def dkrl_all_negative_window_case(E=72):
    """Biases near -1 and small conv1 weights: every live pre-activation is negative.  Row 0 has a hole in window 0, row 1 is
    a prefix that ends inside window 1, row 2 is fractional with one zero in window 1, row 3 has no masked position at all
    (its pooled values are the negative maxima themselves).  The masked position's exact 0 must win its window."""
    g = _gen(f"dkrl all negative {E}")
    L, n = 8, 4
    tok = torch.randint(0, V, (n, L), generator=g)
    mask = torch.ones(n, L)
    mask[0, 2] = 0.0
    mask[1, 6:] = 0.0
    mask[2] = 2.0 - 2.0 * torch.rand(L, generator=g)
    mask[2, 5] = 0.0
    case = Case(tok=tok, mask=mask, E=E, L=L, n=n, windows=((0, 0), (1, 1), (2, 1)),
                **dkrl_weights(E, g, bias1=(-1.2, -0.8), scale1=0.25))
    h, m = dkrl_preact(tok, mask, case.word, case.w1, case.b1)
    for row, window in case.windows:
        hw, mw = h[row, 4 * window:4 * window + 4], m[row, 4 * window:4 * window + 4]
        assert (mw == 0).any() and (mw > 0).any()           # the window has a masked position beside live ones ...
        assert (hw[mw > 0] < 0).all()                       # ... whose pre-activations are all below 0, in every channel
    assert (h[3] < 0).all() and (m[3] > 0).all()
    wrong = dkrl_restated(*dkrl_args(case), False, pool=_max_over_live)
    right = dkrl_restated(*dkrl_args(case), False)
    assert ((wrong - right)[:3].abs().max(dim=-1).values > 1e-3).all() and torch.equal(wrong[3], right[3])
    return _finish_dkrl(case)


@functools.lru_cache(maxsize=None)
def dkrl_position32_case(L, E=72):
    """L >= 33: a distinctive word vector at position 32, the 33rd gathered row.  The first M-tile reads it for the second
    conv tap of position 31 (lanes 0..7 only); at L = 33 that is its ONLY way into the output, since the pool's floor drops
    position 32 itself.  Changing the token there must change the float64 output by more than 1e-3, in every row."""
    assert 33 <= L <= 64
    g = _gen(f"dkrl position 32 {L} {E}")
    n, hot, plain = 3, V - 1, 7
    weights = dkrl_weights(E, g)
    weights["word"][hot] = 3.0 * torch.sign(torch.randn(E, generator=g))
    tok = torch.randint(0, V - 1, (n, L), generator=g)
    tok[:, 32] = hot
    mask = torch.ones(n, L)
    mask[1] = 2.0 - 2.0 * torch.rand(L, generator=g)
    case = Case(tok=tok, mask=mask, E=E, L=L, n=n, hot=hot, **weights)
    other = tok.clone()
    other[:, 32] = plain
    moved = (dkrl_restated(*dkrl_args(case), False) - dkrl_restated(other, *dkrl_args(case)[1:], False)).abs().max(dim=-1).values
    assert (moved > 1e-3).all(), moved
    gone = mask.clone()
    gone[:, 32] = 0.0   # (... and so must a 33rd row that reads as zeros: at L = 33 this changes nothing else, J = 8 either way)
    moved = (dkrl_restated(*dkrl_args(case), False) - dkrl_restated(tok, gone, *dkrl_args(case)[2:], False)).abs().max(dim=-1).values
    assert (moved > 1e-3).all(), moved
    return _finish_dkrl(case)


@functools.lru_cache(maxsize=None)
def dkrl_length36_case(E=72):
    """L = 36: pooled position 8, the first one the second M-tile owns, is live and carries weight in the output."""
    g = _gen(f"dkrl length 36 {E}")
    L, n = 36, 3
    tok = torch.randint(0, V, (n, L), generator=g)
    mask = torch.ones(n, L)
    mask[1, 34:] = 0.0
    mask[2] = 2.0 - 2.0 * torch.rand(L, generator=g)
    case = Case(tok=tok, mask=mask, E=E, L=L, n=n, **dkrl_weights(E, g))
    pooled = mask.reshape(n, 9, 4).max(dim=2).values
    assert pooled.shape[1] == 9 and (pooled[:, 8] > 0).all()
    cut = mask.clone()
    cut[:, 32:] = 0.0   # (without pooled position 8 the rows would be other rows)
    moved = (dkrl_restated(*dkrl_args(case), False) - dkrl_restated(tok, cut, *dkrl_args(case)[2:], False)).abs().max(dim=-1).values
    assert (moved > 1e-3).all(), moved
    return _finish_dkrl(case)


# name -> a builder without arguments: every DKRL input the GPU file runs, beside the (L, split, n) shapes above
DKRL_CASES = {}
for _E in DKRL_E:
    DKRL_CASES[f"E{_E}-L12-n3-holes"] = functools.partial(dkrl_case, _E, 12, 3, "holes")
    DKRL_CASES[f"E{_E}-L37-n5-fractional"] = functools.partial(dkrl_case, _E, 37, 5, "fractional")
for _L in (12, 40):
    for _kind in ("none", "prefix", "fractional", "holes"):
        DKRL_CASES[f"E96-L{_L}-n5-{_kind}"] = functools.partial(dkrl_case, 96, _L, 5, _kind)
for _L, _w in ((12, 1), (40, 3), (40, 8), (64, 7)):   # (40, 8): the second M-tile's first window; (64, 7): the first tile's last
    DKRL_CASES[f"E96-L{_L}-n3-window{_w}-fully-masked"] = functools.partial(dkrl_case, 96, _L, 3, "masked_window", (), _w)
for _L in (8, 33, 64):
    DKRL_CASES[f"E40-L{_L}-every-prefix-1..{_L}"] = functools.partial(dkrl_case, 40, _L, _L, "every_prefix")
DKRL_CASES["all-negative-window"] = dkrl_all_negative_window_case
DKRL_CASES["position32-L33"] = functools.partial(dkrl_position32_case, 33)
DKRL_CASES["position32-L36"] = functools.partial(dkrl_position32_case, 36)
DKRL_CASES["position32-L64"] = functools.partial(dkrl_position32_case, 64)
DKRL_CASES["length36-pooled-position-8"] = dkrl_length36_case
# a fully masked description among live ones, at the splits that put it in one workgroup with them (entities per workgroup:
# 4 / 2 at split 1 / 2 for L <= 32, 2 at split 1 for L > 32)
DKRL_MASKED_ROWS = (("E72-L12-n5-rows1,2-fully-masked", (72, 12, 5, "fractional", (1, 2))),
                    ("E72-L40-n5-rows0,3-fully-masked", (72, 40, 5, "prefix", (0, 3))),
                    ("E8-L4-n3-row2-fully-masked", (8, 4, 3, "prefix", (2,))))
for _name, _args in DKRL_MASKED_ROWS:
    DKRL_CASES[_name] = functools.partial(dkrl_case, *_args)


def dkrl_split_case(L, n):
    """The input of one (L, split, n) shape: prefixes (row 0 whole), E = 72 (three staging steps, the last one partial)."""
    return dkrl_case(72, L, n, "prefix")


DKRL_BAD_ID_PLACES = BAD_ID_PLACES + ("position32",)


@functools.lru_cache(maxsize=None)
def dkrl_bad_id_case(where):
    """The clean input of a bad-token test, as bow_bad_id_case; "position32": (row 1, l = 32) of the L = 33 case, the 33rd
    gathered row."""
    if where == "position32":
        base, row, at = dkrl_position32_case(33), 1, 32
        mask = base.mask.clone()
        assert mask[row, at] > 0
    else:
        base, row, at = dkrl_case(72, 12, 5, "prefix"), 2, 11
        mask = base.mask.clone()
        mask[row, at] = 0.0 if where == "masked" else 1.0
        assert mask[row, 0] > 0
    return _finish_dkrl(Case(**{**base.__dict__, "mask": mask, "row": row, "at": at}))


def all_dkrl_cases():
    seen = dict(DKRL_CASES)
    for L, _, n in DKRL_SPLIT_SHAPES:
        seen[f"E72-L{L}-n{n}-prefix"] = functools.partial(dkrl_split_case, L, n)
    for where in DKRL_BAD_ID_PLACES:
        seen[f"bad-id-place-{where}"] = functools.partial(dkrl_bad_id_case, where)
    return seen


# ------------------------------------------------------------------------------------------------ the restatements, pinned
@pytest.mark.parametrize("name", golden_names("encoders_"))
def test_restatements_reproduce_the_reference_encoders(name):
    """The float64 restatements against the reference's own outputs (tests/golden/encoders_L9.npz, encoders_L37.npz): within
    2e-6 absolute, the bound test_fused_table_builds_reproduce_the_reference_encoders uses."""
    g = {k: torch.from_numpy(v) for k, v in golden(name).items() if v.dtype.kind in "fi"}
    assert name in ("encoders_L9", "encoders_L37")
    for rel_model, normalize in (("transe", True), ("distmult", False)):
        got = bow_restated(g["tok"], g["mask"], g["word_emb"], normalize)
        assert (got - g[f"bow_{rel_model}"].double()).abs().max().item() <= 2e-6
        got = dkrl_restated(g["tok"], g["mask"], g["word_emb"], g["conv1_w"], g["conv1_b"], g["conv2_w"], g["conv2_b"], normalize)
        assert (got - g[f"dkrl_{rel_model}"].double()).abs().max().item() <= 2e-6


def _stock(cls, case, normalize):
    """The stock module (blp_amd.models: the reference's expressions on nn.Embedding / nn.Conv1d / F.max_pool1d) in float64."""
    from blp_amd import models
    rel_model = "transe" if normalize else "distmult"
    if cls == "bow":
        model = models.BOW(rel_model, "margin", 3, 0.0, embeddings=case.word.clone())
    else:
        model = models.DKRL(DIM, rel_model, "margin", 3, 0.0, embeddings=case.word.clone())
        with torch.no_grad():
            model.conv1.weight.copy_(case.w1); model.conv1.bias.copy_(case.b1)
            model.conv2.weight.copy_(case.w2); model.conv2.bias.copy_(case.b2)
    model = model.double().eval()
    assert model.normalize_embs == normalize
    with torch.no_grad():
        return model.encode(case.tok, None if case.mask is None else case.mask.double())


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("name", list(all_bow_cases()))
def test_bow_restatement_equals_the_stock_module_in_float64(name, normalize):
    case = all_bow_cases()[name]()
    want = _stock("bow", case, normalize)
    got = bow_restated(case.tok, case.mask, case.word, normalize)
    assert want.dtype == F64 and got.dtype == F64
    assert torch.allclose(got, want, rtol=0, atol=1e-12, equal_nan=True)
    assert torch.equal(torch.isnan(got).all(-1), torch.tensor([r in case.nan_rows for r in range(case.n)]))


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("name", list(all_dkrl_cases()))
def test_dkrl_restatement_equals_the_stock_module_in_float64(name, normalize):
    case = all_dkrl_cases()[name]()
    want = _stock("dkrl", case, normalize)
    got = dkrl_restated(*dkrl_args(case), normalize)
    assert want.dtype == F64 and got.dtype == F64
    assert torch.allclose(got, want, rtol=0, atol=1e-12, equal_nan=True)
    assert torch.equal(torch.isnan(got).all(-1), torch.tensor([r in case.nan_rows for r in range(case.n)]))


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shape", PROJECT_SHAPES + PROJECT_SPECIALS, ids=lambda s: "-".join(map(str, s)))
def test_linear_restatement_equals_the_stock_module_in_float64(shape, normalize):
    case = project_case(*shape)
    linear = torch.nn.Linear(case.E, case.D, bias=False).double()
    with torch.no_grad():
        linear.weight.copy_(case.w)
        want = linear(case.x.double())
        if normalize:
            want = torch.nn.functional.normalize(want, dim=-1)
    got = linear_restated(case.x, case.w, normalize)
    assert torch.allclose(got, want, rtol=0, atol=1e-12, equal_nan=True)
    for r in case.nonfinite_rows:
        assert not torch.isfinite(got[r]).any()
    for r in case.zero_rows:
        assert (got[r] == 0).all()


@pytest.mark.parametrize("name", list(all_bow_cases()))
def test_bow_sequential_restatement(name):
    """The float32 sequential restatement is BOW: NaN rows where the float64 one has them, elsewhere within float32 rounding of
    it (L additions and one division of values of magnitude <= 2: 1e-5 is generous); and exact where float32 is exact."""
    case = all_bow_cases()[name]()
    got, want = bow_sequential_f32(case.tok, case.mask, case.word), bow_restated(case.tok, case.mask, case.word, False)
    assert got.dtype == F32
    err, _ = errors(got, want, bow_restated(case.tok, case.mask, case.word, False, dtype=F32))
    assert err <= 1e-5, err
    if case.L and case.mask is None:   # small integers: every operation exact but the division, which is correctly rounded
        word = torch.randint(-8, 9, case.word.shape, generator=_gen(name)).float()
        exact = (word.double()[case.tok].sum(1) / case.L).float()
        assert torch.equal(bow_sequential_f32(case.tok, None, word), exact)


def test_tolerance_rule_compares_nan_rows_by_position():
    want = torch.tensor([[1.0, 2.0], [float("nan")] * 2, [0.5, 0.25]], dtype=F64)
    got = want.float()
    assert errors(got, want, want.float()) == (0.0, 0.0)
    assert_within_rule(got + torch.tensor([[1e-6], [0.0], [0.0]]), want, want.float())
    with pytest.raises(AssertionError, match="err_fused"):
        assert_within_rule(got + torch.tensor([[3e-6], [0.0], [0.0]]), want, want.float())
    with pytest.raises(AssertionError):                      # a number where NaN is expected
        errors(torch.ones(3, 2), want, want.float())
    with pytest.raises(AssertionError):                      # NaN where a number is expected
        errors(torch.full((3, 2), float("nan")), want, want.float())


def test_every_listed_size_is_reached():
    """The sizes the GPU file must cover are all in the case tables (a reviewer's checklist, kept honest by an assertion)."""
    cases = [build() for build in all_dkrl_cases().values()]
    assert {c.L for c in cases} >= set(DKRL_L) and {c.E for c in cases} >= set(DKRL_E) and {c.n for c in cases} >= set(DKRL_N)
    assert {c.mask is None for c in cases} == {True, False}
    bow = [bow_case(name) for name in BOW_CASES]
    assert {c.E for c in bow} == set(BOW_E) and {c.L for c in bow} == set(BOW_L) and {c.n for c in bow} == set(BOW_N)
    assert any(c.mask is None for c in bow) and any(c.nan_rows and c.L for c in bow)
    assert {s[0] for s in PROJECT_SHAPES} == set(PROJECT_E) and {s[1] for s in PROJECT_SHAPES} == set(PROJECT_D)
