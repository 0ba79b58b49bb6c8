"""The three table-build kernels at their mask, width and launch edges, on the device: ops.project_rows (project.hip),
ops.bow_rows (bow.hip) and ops.dkrl_rows (dkrl.hip) called directly, the C entry points' refusals through _lib.lib().

What each group is for (the paths the model-level tests of tests/test_gpu_eval.py never reach):
* odd staging-step counts of the double-buffered K / E loop (3, 5 and 7 steps, with and without a partial last step) in
  project.hip and dkrl.hip;
* a row stride wider than the row: every call writes into ``big[r0:r0 + n, :width]`` of a wider, taller matrix filled with
  a sentinel, and every element outside the written block must keep its bits -- columns past the row, neighbouring rows;
* masks that are not 0/1 prefixes: fractional values in (0, 2], interior zeros (dkrl.hip's ``xm[j] != 0`` load skip and its
  smask), a fully masked pooling window between live ones, a fully masked description (lengths == 0: NaN in the reference
  and in the kernel) sharing a workgroup and its LDS stages with live descriptions, mask None;
* the DKRL max-pool sign case: a masked position's exact 0 wins a window whose live pre-activations are all negative;
* DKRL lengths around its tiling (L = 4, 5, 6, 8, 31, 32, 33, 36, 60, 63, 64), the 33rd gathered row (position 32: a
  distinctive word vector there, a bad token id there), every wave split (the dkrl_split knob: default, 1, 2, 4) at n = 1, 2,
  3, 5 -- each held against the float64 restatement, never against another split -- and a forced split of 4 at L > 32, which
  the launcher must ignore;
* BOW column sweeps (E = 4, 256, 260, 512, 516, 1020, 1024), its token walk (L = 0, 1, 2, 3, 5, 8, 33) and n = 1, 2, 3, 5;
  without normalisation the output is bit-equal to the float32 restatement of the order bow.hip's header documents;
* bad token ids: negative, and out of range at a masked position (nn.Embedding raises whatever the mask says);
* projection: n = 64 and 65 (the workgroup's 64 rows), D = 64 with an E tail, a NaN row and an Inf row among finite ones;
* every argument refusal of the three entry points: a negative status, its message, nothing launched.

The float comparisons follow one rule, the one test_dkrl_table_build_is_one_kernel applies: err_fused <= max(4 err32, 2e-6),
err_fused the kernel's largest absolute distance from the float64 restatement and err32 that of the same restatement
evaluated in float32 on the CPU.  NaN rows are compared by position; nothing is skipped or filtered.  The inputs and the
restatements come from tests/test_table_build_host.py, which pins them on the host and asserts that every input reaches the
case it is for.

What a subtly wrong kernel would trip, argued from the code (nothing here breaks a kernel on purpose):
1. The staging loop's lone last step.  With an odd step count the last trip runs compute(0) alone; `if (k + 1 < n_steps)
   compute(1)` is then false.  Dropping that guard is harmless by construction -- LDS stage 1 then holds step n_steps, which
   fetch() zero-fills -- so no test can or should see it.  What the odd counts do catch is the trip itself going wrong: a loop
   bound of `k + 1 < n_steps`, a guard one trip too strict (`k + 3 < n_steps`), or a ring slot put into the wrong stage lose
   or repeat 32 columns of E, an error of order 0.1: test_project_rows_odd_step_counts_...[E72-*|E96-*|E160-*|E200-*] and
   test_dkrl_rows_widths_masks_and_tile_edges[E72-*|E96-*|E160-*|E200-*] (3, 3, 5, 7 steps) fail the rule.
2. The row-32 fetch (lanes 0..7, j = 4).  Without it position 32 reads as zeros in the first M-tile's second tap.
   test_dkrl_rows_widths_masks_and_tile_edges[position32-L33-*]: at L = 33 that tap is the token's only way into the output,
   and the builder asserts that a zero row there (and another token there) moves the float64 output by more than 1e-3.
3. The `jp + 1 < J` guard of u1.  Without it u1 adds pm[J - 1] * ts[J], a row of the epilogue's LDS no thread wrote: what is
   left of the staged W1 slice and word vectors (for J = 16, the next entity's first row).  Every DKRL case whose last window
   is live fails the rule, first test_dkrl_rows_every_split_against_float64[4-*] (J = 1).
4. The `ie < n` store guard.  Without it the waves of a partly empty last workgroup write rows n .. of the frame with the
   clamped entity's values: Frame.result() fails in every test_dkrl_rows_every_split_against_float64 case with n % epw != 0,
   e.g. [4-1-2] (split 1, four entities per workgroup, n = 2).
5. The `c < E` guards of bow.hip's sweeps.  Without the store's guard every row is written out to column 1023: the sentinel
   columns E .. E + 7 and the rows below change, Frame.result() fails in every BOW case with E < 1024.  The guard of the
   sum of squares only skips exact zeros, and the load's guard only keeps reads inside the table: neither changes a result.

A chosen limit of these tests, not an oversight: the weights and the word tables are finite.  dkrl.hip's max-pool never lets
a NaN pre-activation win (F.max_pool1d propagates it), and it never loads the word vector of a fully masked position (the
reference multiplies it by 0), so a non-finite word vector behind a zero mask gives a finite row where the reference gives NaN.
"""
import ctypes
import types

import pytest
import torch

import test_table_build_host as host
from test_table_build_host import DIM, F32, V

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 7.25


@pytest.fixture(scope="module")
def ops():
    from blp_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def _lib():
    from blp_amd import _lib as lib_module
    return lib_module


class Frame:
    """``out`` as rows r0 .. r0 + n - 1, columns 0 .. width - 1 of a wider, taller sentinel-filled matrix."""

    def __init__(self, n, width, ld, r0):
        self.n, self.width, self.r0 = n, width, r0
        self.big = torch.full((r0 + n + 4, ld), SENTINEL, device=DEV)  # (four rows below: a workgroup's worth of entities)
        self.out = self.big[r0:r0 + n, :width]
        assert self.out.shape == (n, width) and (n <= 1 or self.out.stride(0) == ld) and ld > width

    def result(self):
        """The written block, after checking that every element outside it is bit-unchanged."""
        torch.cuda.synchronize()
        big = self.big.cpu()
        outside = torch.ones(big.shape, dtype=torch.bool)
        outside[self.r0:self.r0 + self.n, :self.width] = False
        want = torch.full((), SENTINEL).view(torch.int32)
        touched = outside & (big.view(torch.int32) != want)
        assert not touched.any(), torch.nonzero(touched)[:5]
        return big[self.r0:self.r0 + self.n, :self.width].clone()


def assert_f32_bits(got, want):
    """Bit-equal where the expectation is a number; NaN where it is NaN."""
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), torch.nonzero(torch.isnan(got) != nan)[:5]
    differ = ~nan & (got.view(torch.int32) != want.view(torch.int32))
    assert not differ.any(), torch.nonzero(differ)[:5]


# ------------------------------------------------------------------------------------------------ project_rows
def run_project(ops, case, normalize):
    x = case.seq.to(DEV)[:, 0]                                   # a strided view: row stride 3 E
    assert case.n == 1 or x.stride(0) == 3 * case.E
    frame = Frame(case.n, case.D, case.D + 3, 4)                  # (rows start at 16 (D + 3) bytes: aligned, odd stride)
    assert ops.project_rows(x, case.w.to(DEV), frame.out, normalize) is frame.out
    return frame.result()


def check_project(case, got, normalize):
    want64 = host.linear_restated(case.x, case.w, normalize)
    want32 = host.linear_restated(case.x, case.w, normalize, dtype=F32)
    rest = [r for r in range(case.n) if r not in case.nonfinite_rows]
    assert torch.isfinite(got[rest]).all()                         # only the rows that hold a NaN / an Inf may be non-finite
    host.assert_within_rule(got[rest], want64[rest], want32[rest])
    for r in case.nonfinite_rows:
        assert not torch.isfinite(got[r]).any()
        assert torch.equal(torch.isnan(got[r]), torch.isnan(want64[r]))
        inf = torch.isinf(want64[r])
        assert torch.equal(got[r][inf].double(), want64[r][inf])   # (the sign of every infinity)
    for r in case.zero_rows:
        if normalize:
            assert (got[r] == 0).all()                             # F.normalize's eps: a zero row stays zero, no NaN


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("shape", host.PROJECT_SHAPES, ids=lambda s: "E%d-D%d-n%d" % s)
def test_project_rows_odd_step_counts_workgroup_boundary_and_row_stride(ops, shape, normalize):
    """E = 72 / 96 (3 steps), 160 (5), 200 (7), 36 (2); 72, 200 and 36 with a partial last step; D = 64, 128, 256 (D = 64 with an
    E tail among them); n = 1, 63, 64, 65, 70; x a strided view; ldo = D + 3 inside a sentinel frame."""
    case = host.project_case(*shape)
    check_project(case, run_project(ops, case, normalize), normalize)


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("shape", host.PROJECT_SPECIALS, ids=lambda s: "E%d-D%d-n%d-%s" % s)
def test_project_rows_nan_inf_and_zero_rows_stay_in_their_rows(ops, shape, normalize):
    """One row holding a NaN and one holding an Inf among finite ones: only those output rows are non-finite, the others stay
    within the rule.  An all-zero row normalises to exact zeros."""
    case = host.project_case(*shape)
    check_project(case, run_project(ops, case, normalize), normalize)


@pytest.mark.parametrize("D", host.PROJECT_D)
def test_project_rows_of_no_rows_touches_nothing(ops, D):
    frame = Frame(0, D, D + 3, 4)
    x, w = torch.empty(0, 72, device=DEV), torch.randn(D, 72, device=DEV)
    assert ops.project_rows(x, w, frame.out, True) is frame.out
    assert frame.result().shape == (0, D)


# ------------------------------------------------------------------------------------------------ bow_rows
def run_bow(ops, case, normalize, tok=None, bad_flag=None):
    tok, mask = case.tok if tok is None else tok, case.mask
    frame = Frame(case.n, case.E, case.E + 8, 2)                  # (float4 stores: ldo % 4 == 0)
    out = ops.bow_rows(tok.to(DEV), None if mask is None else mask.to(DEV), case.word.to(DEV), frame.out, normalize,
                       bad_flag=bad_flag)
    assert out is frame.out
    return frame.result()


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("name", list(host.BOW_CASES))
def test_bow_rows_column_sweeps_token_walk_and_masks(ops, name, normalize):
    """E = 4 (one lane live), 256 | 260, 512 | 516, 1020 | 1024; L = 0 (NaN rows: 0 / 0), 1, 2, 3, 5, 8, 33; n = 1, 2, 3, 5; mask
    None, a prefix, fractional in (0, 2], interior zeros; a fully masked row among live ones (NaN in that row only); sentinel
    columns and rows.  Without normalisation: bit-equal to the float32 sequential restatement (bow.hip's documented order)."""
    case = host.bow_case(name)
    got = run_bow(ops, case, normalize)
    if not normalize:
        assert_f32_bits(got, host.bow_sequential_f32(case.tok, case.mask, case.word))
    host.assert_within_rule(got, host.bow_restated(case.tok, case.mask, case.word, normalize),
                            host.bow_restated(case.tok, case.mask, case.word, normalize, dtype=F32))
    assert torch.equal(torch.isnan(got).all(-1), torch.tensor([r in case.nan_rows for r in range(case.n)]))


@pytest.mark.parametrize("bad", [-1, V, -2 ** 63, 2 ** 40], ids=["minus1", "V", "int64min", "2^40"])
@pytest.mark.parametrize("where", host.BAD_ID_PLACES)
@pytest.mark.parametrize("name", host.BOW_BAD_ID_CASES)
def test_bow_rows_bad_token_ids(ops, name, where, bad):
    """A negative id, an id == V (and two far ones), at a live and at a masked position: IndexError when no bad_flag is passed,
    the caller's flag at -1 when one is; the other rows are the clean rows; a clean call leaves a zeroed flag at zero."""
    case = host.bow_bad_id_case(name, where)
    tok = case.tok.clone()
    tok[case.row, case.at] = bad
    with pytest.raises(IndexError):
        run_bow(ops, case, False, tok)
    flag = torch.zeros((), dtype=torch.int32, device=DEV)
    clean = run_bow(ops, case, False, bad_flag=flag)
    assert flag.item() == 0
    assert_f32_bits(clean, host.bow_sequential_f32(case.tok, case.mask, case.word))
    got = run_bow(ops, case, False, tok, bad_flag=flag)
    assert flag.item() == -1
    rest = [r for r in range(case.n) if r != case.row]
    assert_f32_bits(got[rest], clean[rest])
    if where == "masked":                                            # (row 0 is read instead, and multiplied by the zero mask)
        assert_f32_bits(got, clean)


# ------------------------------------------------------------------------------------------------ dkrl_rows
def conv(weight, bias):
    return types.SimpleNamespace(weight=weight.to(DEV), bias=bias.to(DEV))


def run_dkrl(ops, _lib, case, normalize, split=0, tok=None, bad_flag=None):
    tok = case.tok if tok is None else tok
    frame = Frame(case.n, DIM, DIM + 3, 1)
    try:
        if split:
            _lib.set_knob("dkrl_split", split)
        out = ops.dkrl_rows(tok.to(DEV), None if case.mask is None else case.mask.to(DEV), case.word.to(DEV),
                            conv(case.w1, case.b1), conv(case.w2, case.b2), frame.out, normalize, bad_flag=bad_flag)
        assert out is frame.out
        return frame.result()
    finally:
        _lib.reset_knobs()


def check_dkrl(case, got, normalize):
    host.assert_within_rule(got, host.dkrl_restated(*host.dkrl_args(case), normalize),
                            host.dkrl_restated(*host.dkrl_args(case), normalize, dtype=F32))
    assert torch.equal(torch.isnan(got).all(-1), torch.tensor([r in case.nan_rows for r in range(case.n)]))


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("name", [n for n in host.DKRL_CASES if n not in dict(host.DKRL_MASKED_ROWS)])
def test_dkrl_rows_widths_masks_and_tile_edges(ops, _lib, name, normalize):
    """E = 72 / 96 (3 staging steps), 160 (5), 200 (7), 8 (1); masks None, prefixes of every length 1 .. L, fractional, interior
    zeros, a fully masked pooling window between live ones; the all-negative window (the masked position's 0 wins); the
    distinctive word vector at position 32 (L = 33: the row-32 fetch is its only way into the output); L = 36 with pooled
    position 8 live; sentinel columns and rows (ldo = 131)."""
    case = host.DKRL_CASES[name]()
    check_dkrl(case, run_dkrl(ops, _lib, case, normalize), normalize)


@pytest.mark.parametrize("L,split,n", host.DKRL_SPLIT_SHAPES, ids=lambda v: str(v))
def test_dkrl_rows_every_split_against_float64(ops, _lib, L, split, n):
    """L = 4, 5, 6, 8, 31, 32, 33, 36, 60, 63, 64 x dkrl_split = default (0), 1, 2, 4 x n = 1, 2, 3, 5 (the last workgroup partly
    empty): every split against the float64 restatement.  A forced split of 4 at L > 32 is ignored by the launcher (an entity of
    two M-tiles would not fit a workgroup): bit-equal to the default."""
    case = host.dkrl_split_case(L, n)
    normalize = (L + n) % 2 == 0
    got = run_dkrl(ops, _lib, case, normalize, split)
    check_dkrl(case, got, normalize)
    if split == 4 and L > 32:
        assert_f32_bits(got, run_dkrl(ops, _lib, case, normalize, 0))


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("split", host.DKRL_SPLITS)
@pytest.mark.parametrize("name", [name for name, _ in host.DKRL_MASKED_ROWS])
def test_dkrl_rows_fully_masked_description_among_live_ones(ops, _lib, name, split, normalize):
    """lengths == 0: NaN in that row only, at every split -- at split 1 (and 2 for L <= 32) the row shares a workgroup and its
    LDS stages with live descriptions, whose rows must be unaffected."""
    case = host.DKRL_CASES[name]()
    assert case.nan_rows
    check_dkrl(case, run_dkrl(ops, _lib, case, normalize, split), normalize)


@pytest.mark.parametrize("bad", [-1, V], ids=["minus1", "V"])
@pytest.mark.parametrize("where", host.DKRL_BAD_ID_PLACES)
@pytest.mark.parametrize("split", [0, 1])
def test_dkrl_rows_bad_token_ids(ops, _lib, split, where, bad):
    """As for BOW; and a bad id at exactly l = 32, the 33rd gathered row."""
    case = host.dkrl_bad_id_case(where)
    tok, row = case.tok.clone(), case.row
    tok[row, case.at] = bad
    with pytest.raises(IndexError):
        run_dkrl(ops, _lib, case, True, split, tok)
    flag = torch.zeros((), dtype=torch.int32, device=DEV)
    clean = run_dkrl(ops, _lib, case, True, split, bad_flag=flag)
    assert flag.item() == 0
    check_dkrl(case, clean, True)
    got = run_dkrl(ops, _lib, case, True, split, tok, bad_flag=flag)
    assert flag.item() == -1
    rest = [r for r in range(case.n) if r != row]
    assert_f32_bits(got[rest], clean[rest])
    if where == "masked":                                            # (a masked position's word vector is never used)
        assert_f32_bits(got, clean)


# ------------------------------------------------------------------------------------------------ refusals
BAD_ARG, UNSUPPORTED = -1, -2


class Refusal:
    """Valid arguments of one entry point over sentinel-filled outputs; call(**overrides) replaces some by name."""

    def __init__(self, lib, entry):
        self.lib, self.entry = lib, entry
        g = torch.Generator().manual_seed(5)
        self.frame = Frame(3, 264 if entry == "blp_bow_rows" else DIM, 272 if entry == "blp_bow_rows" else DIM + 4, 4)
        self.flag = torch.zeros((), dtype=torch.int32, device=DEV)
        self.t = dict(x=torch.randn(3, 72, generator=g), w=torch.randn(DIM, 72, generator=g) / 8,
                      tok=torch.randint(0, V, (3, 8), generator=g), mask=torch.ones(3, 8),
                      emb=torch.randn(V, 264 if entry == "blp_bow_rows" else 72, generator=g),
                      w1=torch.randn(DIM, 72, 2, generator=g) / 12, b1=torch.zeros(DIM),
                      w2=torch.randn(DIM, DIM, 2, generator=g) / 16, b2=torch.zeros(DIM))
        self.t = {k: v.to(DEV) for k, v in self.t.items()}
        p = {k: v.data_ptr() for k, v in self.t.items()}
        out, bad = self.frame.out.data_ptr(), self.flag.data_ptr()
        assert all(v % 16 == 0 for v in p.values()) and out % 16 == 0
        if entry == "blp_project_rows":
            self.args = dict(x=p["x"], n=3, ldx=72, w=p["w"], E=72, D=DIM, normalize=1, out=out, ldo=DIM + 4)
        elif entry == "blp_bow_rows":
            self.args = dict(tok=p["tok"], mask=p["mask"], n=3, L=8, emb=p["emb"], V=V, E=264, normalize=1, out=out, ldo=272, bad_tok=bad)
        else:
            self.args = dict(tok=p["tok"], mask=p["mask"], n=3, L=8, emb=p["emb"], V=V, E=72, w1=p["w1"], b1=p["b1"], w2=p["w2"],
                             b2=p["b2"], D=DIM, normalize=1, out=out, ldo=DIM + 4, bad_tok=bad)

    def call(self, **overrides):
        assert set(overrides) <= set(self.args)
        args = {**self.args, **overrides}
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        return getattr(self.lib, self.entry)(*args.values(), torch.cuda.current_device(), stream)


PTR = 4  # bytes: a pointer that is float-aligned but not 16-byte aligned
REFUSALS = {
    "blp_project_rows": [
        (dict(E=70, ldx=72), UNSUPPORTED, "needs E % 4 == 0"), (dict(E=0), UNSUPPORTED, "needs E % 4 == 0"),
        (dict(D=100), UNSUPPORTED, "needs 64 / 128 / 256"), (dict(D=32), UNSUPPORTED, "needs 64 / 128 / 256"),
        (dict(n=-1), BAD_ARG, "negative row count"),
        (dict(x=None), BAD_ARG, "NULL pointer"), (dict(w=None), BAD_ARG, "NULL pointer"), (dict(out=None), BAD_ARG, "NULL pointer"),
        (dict(x=PTR), BAD_ARG, "16-byte aligned"), (dict(w=PTR), BAD_ARG, "16-byte aligned"), (dict(out=PTR), BAD_ARG, "16-byte aligned"),
        (dict(ldx=74), BAD_ARG, "ldx % 4 == 0"), (dict(ldx=68), BAD_ARG, "ldx >= E"), (dict(ldo=DIM - 1), BAD_ARG, "ldo >= D"),
    ],
    "blp_bow_rows": [
        (dict(E=262), UNSUPPORTED, "needs E % 4 == 0"), (dict(E=1028, ldo=1028), UNSUPPORTED, "E <= 1024"), (dict(E=0), UNSUPPORTED, "E = 0"),
        (dict(n=-1), BAD_ARG, "negative size"), (dict(L=-1), BAD_ARG, "negative size"), (dict(V=-1), BAD_ARG, "negative size"),
        (dict(out=None), BAD_ARG, "NULL pointer"), (dict(bad_tok=None), BAD_ARG, "NULL pointer"), (dict(tok=None), BAD_ARG, "NULL pointer"),
        (dict(emb=None), BAD_ARG, "NULL pointer"), (dict(V=0), BAD_ARG, "empty embedding table"),
        (dict(emb=PTR), BAD_ARG, "16-byte aligned"), (dict(out=PTR), BAD_ARG, "16-byte aligned"),
        (dict(ldo=270), BAD_ARG, "ldo % 4 == 0"), (dict(ldo=260), BAD_ARG, "ldo >= E"),
    ],
    "blp_dkrl_rows": [
        (dict(E=70), UNSUPPORTED, "needs E % 4 == 0"), (dict(E=0), UNSUPPORTED, "E = 0"),
        (dict(D=64), UNSUPPORTED, "needs 128"), (dict(D=256), UNSUPPORTED, "needs 128"),
        (dict(L=3), UNSUPPORTED, "needs 4 .. 64"), (dict(L=65), UNSUPPORTED, "needs 4 .. 64"),
        (dict(n=-1), BAD_ARG, "negative size"), (dict(V=-1), BAD_ARG, "negative size"),
        (dict(tok=None), BAD_ARG, "NULL pointer"), (dict(emb=None), BAD_ARG, "NULL pointer"), (dict(w1=None), BAD_ARG, "NULL pointer"),
        (dict(b1=None), BAD_ARG, "NULL pointer"), (dict(w2=None), BAD_ARG, "NULL pointer"), (dict(b2=None), BAD_ARG, "NULL pointer"),
        (dict(out=None), BAD_ARG, "NULL pointer"), (dict(bad_tok=None), BAD_ARG, "NULL pointer"), (dict(V=0), BAD_ARG, "empty embedding table"),
        (dict(emb=PTR), BAD_ARG, "16-byte aligned"), (dict(w1=PTR), BAD_ARG, "16-byte aligned"), (dict(w2=PTR), BAD_ARG, "16-byte aligned"),
        (dict(ldo=DIM - 1), BAD_ARG, "ldo >= dim"),
    ],
}


@pytest.mark.parametrize("entry", list(REFUSALS))
def test_entry_points_refuse_bad_arguments_without_launching(_lib, entry):
    """E % 4 != 0, BOW E > 1024, DKRL D != 128, L = 3 and L = 65, misaligned pointers, ldo < D (BOW: ldo < E, ldo % 4), projection
    ldx % 4 and ldx < E, NULL pointers, V == 0, negative sizes: each returns its negative status with the message _lib reports
    and leaves the sentinel-filled out (and the bad-token flag) unchanged.  The valid call itself is accepted."""
    lib = _lib.lib()
    r = Refusal(lib, entry)
    for overrides, status, text in REFUSALS[entry]:
        for name, value in list(overrides.items()):
            if value == PTR:                                         # the valid pointer, moved off its 16-byte boundary
                overrides = {**overrides, name: r.args[name] + PTR}
        got = r.call(**overrides)
        assert got == status, (overrides, got)
        message = lib.blp_last_error().decode()
        assert message.startswith(entry + ":") and text in message, (overrides, message)
        with pytest.raises(RuntimeError, match=_lib.STATUS_NAMES[status]) as raised:
            _lib.check(got, entry)
        assert message in str(raised.value)
        block = r.frame.result()                                     # (synchronises; checks the frame around the block)
        assert (block == SENTINEL).all() and r.flag.item() == 0, overrides
    assert r.call() == 0
    assert not (r.frame.result() == SENTINEL).any() and r.flag.item() == 0


def test_supported_functions_agree_with_the_entry_points(_lib, ops):
    """blp_*_supported at the boundary values, both sides: exactly what the entry points accept (BLP_ERR_UNSUPPORTED_DIM
    otherwise), and what the ops wrappers report."""
    lib = _lib.lib()
    p = Refusal(lib, "blp_project_rows")
    for E, D, ok in ((72, 64, 1), (72, 128, 1), (72, 256, 1), (4, 64, 1), (0, 64, 0), (-4, 64, 0), (70, 64, 0), (71, 64, 0), (72, 63, 0),
                     (72, 65, 0), (72, 32, 0), (72, 0, 0), (72, 512, 0), (72, 127, 0), (72, 129, 0), (72, 255, 0)):
        assert lib.blp_project_rows_supported(E, D) == ok == int(ops.project_rows_supported(E, D)), (E, D)
        if D <= DIM:                                                 # (w and out hold 128 columns)
            assert p.call(E=E, D=D) == (0 if ok else UNSUPPORTED), (E, D)
    b = Refusal(lib, "blp_bow_rows")
    for E, ok in ((4, 1), (8, 1), (260, 1), (264, 1), (0, 0), (-4, 0), (2, 0), (5, 0), (262, 0), (1020, 1), (1022, 0), (1024, 1), (1025, 0),
                  (1028, 0), (2048, 0)):
        assert lib.blp_bow_rows_supported(E) == ok == int(ops.bow_rows_supported(E)), E
        if E <= 264:                                                 # (emb and out hold 264 columns)
            assert b.call(E=E) == (0 if ok else UNSUPPORTED), E
        elif not ok:
            assert b.call(E=E, ldo=4096) == UNSUPPORTED, E
    d = Refusal(lib, "blp_dkrl_rows")
    for E, D, L, ok in ((72, 128, 8, 1), (4, 128, 8, 1), (0, 128, 8, 0), (70, 128, 8, 0), (73, 128, 8, 0), (72, 127, 8, 0), (72, 129, 8, 0),
                        (72, 64, 8, 0), (72, 256, 8, 0), (72, 128, 3, 0), (72, 128, 4, 1), (72, 128, 5, 1), (72, 128, 0, 0), (72, 128, -4, 0)):
        assert lib.blp_dkrl_rows_supported(E, D, L) == ok == int(ops.dkrl_rows_supported(E, D, L)), (E, D, L)
        assert d.call(E=E, D=D, L=L) == (0 if ok else UNSUPPORTED), (E, D, L)
    wide = torch.randint(0, V, (3, 65), device=DEV)                  # L = 63, 64 | 65 on tokens that are there
    ones = torch.ones(3, 65, device=DEV)
    for L, ok in ((63, 1), (64, 1), (65, 0), (66, 0)):
        assert lib.blp_dkrl_rows_supported(72, DIM, L) == ok == int(ops.dkrl_rows_supported(72, DIM, L)), L
        assert d.call(L=L, tok=wide.data_ptr(), mask=ones.data_ptr()) == (0 if ok else UNSUPPORTED), L
    torch.cuda.synchronize()
    assert d.flag.item() == 0 and b.flag.item() == 0
    for r in (p, b, d):
        r.frame.result()                                             # the accepted calls stayed inside their block too
