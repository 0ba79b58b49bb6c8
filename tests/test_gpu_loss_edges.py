"""The training side on the MI355X, adversarially (inbatch_loss.hip, score.hip, the autograd glue of ops.py / csrc/torch_glue.cpp).

1. Bit-exact: margin loss, regularizer 0, B and K powers of two, embeddings from a small integer grid -- every score, hinge,
   loss and gradient is then exactly representable and the same number in any summation order, so the kernels' loss and both
   gradients must be torch.equal to the torch port's (oracle/ref_port.compute_loss), at one shape per forward / backward path.
   Every case holds hinges that are exactly 0 (gradient passes), negative (masked) and positive, and for TransE many
   coordinates of h + r - t that are exactly 0 (sign(0) = 0).
2. NLL where tolerance tests never went: the multi-workgroup reduce, odd widths, 16-bit storage, one row named by every
   negative, and scores around and far past softplus' threshold of 20 -- against the port in float64.
3. Non-finite inputs propagate to the loss and leave the ticket counters zero for the next step.
4. ops.score forward and backward on the integer grids, bit-equal to CPU autograd of the port, for the eval broadcast, the
   training broadcast, the copy fallback of ops._two_level and NULL gradient pointers.

Problems and references are built on the CPU, once per case (cached), before the device is touched."""
import functools

import pytest
import torch

from conftest import REL_MODELS

pytestmark = pytest.mark.gpu

MARGIN, NLL = "margin", "nll"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    assert _ops.torch_glue() is not None, "blp_amd/_torch_glue.so is not loaded: the product's autograd path would go untested"
    return _ops


# ---------------------------------------------------------------------------------------------- helpers
def grid(shape, step, density, gen):
    """Entries in {-step, 0, step}; `density` (a number, or a tensor broadcastable to `shape`) is the share of non-zeros."""
    nonzero = torch.rand(shape, generator=gen) < density
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (nonzero * sign).float() * step


def port(model, loss_fn, ent, rel, neg_idx, reg, dtype):
    """oracle/ref_port.compute_loss and its autograd gradients in `dtype`: (loss, grad_ent, grad_rel), detached."""
    from oracle import ref_port
    e, r = ent.to(dtype, copy=True).requires_grad_(True), rel.to(dtype, copy=True).requires_grad_(True)
    loss = ref_port.compute_loss(model, loss_fn, e, r, neg_idx, reg)
    loss.backward()
    return loss.detach(), e.grad, r.grad


def port_scores(model, ent, rel, neg_idx):
    """The port's f32 scores: positives (B, 1), negatives (B, K), and the negatives' gathered rows (B, K, 2, D)."""
    from oracle import ref_port
    score = ref_port.SCORE_FNS[model]
    gathered = ent.reshape(-1, ent.shape[-1])[neg_idx]
    return score(ent[:, 0:1], ent[:, 1:2], rel), score(gathered[:, :, 0], gathered[:, :, 1], rel), gathered


def run(ops, model, loss_fn, ent, rel, neg_idx, reg, upstream=1.0, python_glue=False):
    """One step on the device: (loss, grad_ent, grad_rel) on the CPU.  python_glue: through ops._InBatchLoss (the Python
    autograd.Function, whose ticket counter ops.inbatch_ticket exposes) instead of the C++ glue ops.inbatch_loss uses."""
    e, r, idx = ent.cuda().requires_grad_(True), rel.cuda().requires_grad_(True), neg_idx.cuda()
    if python_glue:
        loss = ops._InBatchLoss.apply(model, loss_fn, reg, e, r, idx)
    else:
        loss = ops.inbatch_loss(model, loss_fn, e, r, idx, reg)
    (loss * upstream).backward()
    return loss.detach().cpu(), e.grad.cpu(), r.grad.cpu()


def ticket_ints(ops):
    dev = torch.device("cuda", torch.cuda.current_device())
    ticket = ops.inbatch_ticket(dev, torch._C._cuda_getCurrentRawStream(dev.index))
    torch.cuda.synchronize()
    return ticket.tolist()


def lanes_per_pair(model, D):
    """inbatch_loss.hip: TransE's sum walks through four lanes at widths % 16 == 0 up to 256, else one lane per pair; the
    bilinear models take 32 lanes where torch.sum keeps 32 running sums (reduction width % 32 == 0, < 512), else a 16-lane tree."""
    if model == "transe":
        return 4 if D % 16 == 0 and D <= 256 else 1
    n = D if model == "distmult" else D // 2
    return 32 if n % 32 == 0 and 32 <= n < 512 else 16


def forward_launches(model, B, K, D, reg):
    """launches_match of test_gpu_parity.py at any width and with or without the regulariser's workgroups: one launch iff at
    most 96 scoring + regulariser workgroups, slots packed or -- when a row's K + 1 pairs fit a workgroup -- a workgroup per row."""
    lanes = lanes_per_pair(model, D)
    reg_blocks = (B + 3) // 4 if reg > 0 else 0
    packed = -(-B * (K + 1) // (256 // lanes)) + reg_blocks
    per_row = B + reg_blocks if (K + 1 <= 256 and (K + 1) * lanes <= 1024) else packed
    return 1 if min(packed, per_row) <= 96 else 2


def worst(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): numpy.testing.assert_allclose's criterion as a number (passes at <= 1)."""
    got, want = got.double(), want.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - want).abs() / (atol + rtol * want.abs())).max())


RTOL = {torch.float32: 2e-5, torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}


def assert_matches_port64(label, got, ref, K, loss_rel=2e-6):
    """test_gpu_parity.py's tolerances against the float64 port: loss rel 2e-6 (abs 1e-7); gradients rtol 2e-5 (f32) / 2^-10
    (f16) / 2^-7 (bf16) with the absolute term of test_inbatch_loss_backward_row_ownership_and_rounds -- a few ulps of the
    largest partial sum of a row.  A float16 gradient below 2^-14 is stored subnormal, in steps of 2^-24: half a step more.
    (On the CPU the f32 port itself sits within 0.25 of every band used here, 0.85 once rounded to f16: no case needed a
    measured band.)"""
    (loss, ge, gr), (ref_loss, ref_ge, ref_gr) = got, ref
    scale = float(ref_ge.abs().max())
    atol = 2e-6 * max(scale, 1e-3) * max(1.0, K / 250.0)
    loss_err = abs(float(loss) - float(ref_loss)) / (1e-7 + loss_rel * abs(float(ref_loss)))
    errs = [worst(g, want, RTOL[g.dtype], atol + (2.0 ** -25 if g.dtype == torch.float16 else 0.0))
            for g, want in ((ge, ref_ge), (gr, ref_gr))]
    print(f"{label}: loss {float(loss):.9g} (port {float(ref_loss):.9g}) at {loss_err:.3f} of its band; "
          f"grad_ent at {errs[0]:.3f}, grad_rel at {errs[1]:.3f} of theirs")
    assert bool(torch.isfinite(loss)) and loss_err <= 1.0
    assert errs[0] <= 1.0 and errs[1] <= 1.0


# ---------------------------------------------------------------------------------------------- 1. bit-exact, margin, reg = 0
# (B, K, D) -> forward launches (TransE, bilinear); the path each shape is there for:
EXACT_SHAPES = {
    (16, 8, 64): (1, 1),      # a workgroup per batch row, one launch; grad4 below D = 128; TransE quad at 64; ComplEx / SimplE at reduction width 32
    (8, 64, 128): (1, 1),     # TransE: a row workgroup of 65 x 4 threads; bilinear: packed slots, 65 workgroups, still one launch
    (128, 2, 128): (1, 1),    # B > 96: packed slots, one launch
    (64, 64, 128): (1, 2),    # bilinear: two launches, one reduce workgroup
    (256, 64, 128): (2, 2),   # reduce G = 2; 2 B K = 32 768, the last speculating size of grad4
    (256, 128, 64): (2, 2),   # 2 B K = 65 536: grad4 without speculation; reduce G = 4
    (512, 1, 36): (1, 1),     # K = 1; 2 B = 1 024 rows = one histogram pass exactly; TransE one lane per pair; bilinear 16-lane tree;
                              # grad4 at D = 36 (TransE, DistMult), the sweep kernel for ComplEx / SimplE (D % 8 != 0)
    (32, 16, 300): (1, 1),    # the sweep kernel; no register-order sum
    (16, 32, 256): (1, 1),    # TransE quad at its upper bound; DistMult 32 lanes at n = 256 (33 x 32 threads do not fit: packed); sweep kernel
    (2048, 2, 8): (1, 2),     # 4 096 rows: four histogram passes; two live lanes per half-wave in grad4; reduction width 4
}
HALF_SHAPES = ((16, 8, 64), (512, 1, 36), (32, 16, 300))


def exact_densities(model, D):
    """Shares of non-zero entries (entities, relations), per width, chosen on the CPU so that every case has hinges on both
    sides of 0 and exactly 0 (narrow rows need denser ones for scores to differ at all)."""
    if model == "transe":
        return (0.3, 0.3) if D <= 8 else (0.15, 0.15)
    if D <= 8:
        return (0.7, 0.9)
    return (0.35, 0.6) if D <= 64 else (0.2, 0.5)


@functools.lru_cache(maxsize=None)
def exact_case(model, B, K, D):
    """Inputs on the grid, the f32 port's loss and gradients, and the preconditions that make the case worth running."""
    gen = torch.Generator().manual_seed(1000 * B + 10 * K + D + REL_MODELS.index(model))
    step = 0.25 if model == "transe" else 1.0
    p_ent, p_rel = exact_densities(model, D)
    ent = grid((B, 2, D), step, p_ent, gen)
    rel = grid((B, 1, D), step, p_rel, gen)
    neg_idx = torch.randint(0, 2 * B, (B, K, 2), generator=gen)
    neg_idx[0, 0] = torch.tensor([0, 1])   # the positive's own pair: a hinge of exactly 1
    neg_idx[B - 1, K - 1] = 5              # both slots name one row: the index's partner row is the row itself
    pos, neg, gathered = port_scores(model, ent, rel, neg_idx)
    hinge = 1 - pos + neg
    assert hinge[0, 0] == 1.0
    counts = int((hinge == 0).sum()), int((hinge < 0).sum()), int((hinge > 0).sum())
    assert min(counts) >= 1, f"hinges == 0, < 0, > 0: {counts}"
    if model == "transe":
        zero = (gathered[:, :, 0] + rel - gathered[:, :, 1] == 0).float().mean()
        assert zero >= 0.25, f"only {float(zero):.2f} of the negatives' h + r - t coordinates are exactly 0"
    loss, ge, gr = port(model, MARGIN, ent, rel, neg_idx, 0.0, torch.float32)
    loss64, ge64, gr64 = port(model, MARGIN, ent, rel, neg_idx, 0.0, torch.float64)
    assert torch.equal(loss.double(), loss64) and torch.equal(ge.double(), ge64) and torch.equal(gr.double(), gr64), \
        "the case is not exact: the f32 port and the float64 port differ"
    return ent, rel, neg_idx, loss, ge, gr


@pytest.mark.parametrize("model", REL_MODELS)
@pytest.mark.parametrize("B,K,D", list(EXACT_SHAPES))
def test_exact_margin_loss_and_gradients(ops, model, B, K, D):
    """Loss and both gradients bit-equal to the port's, with upstream gradient 1 and 0.5, through the C++ glue and the Python
    autograd.Function; the launch count the shape is there for; ticket counters left zero; a repeat gives the same bits."""
    from blp_amd import _lib
    ent, rel, neg_idx, loss, ge, gr = exact_case(model, B, K, D)
    launches = forward_launches(model, B, K, D, 0.0)
    assert launches == EXACT_SHAPES[(B, K, D)][0 if model == "transe" else 1]
    assert _lib.lib().blp_inbatch_loss_fwd_launches(_lib.MODEL_IDS[model], B, K, D, 0.0) == launches
    first = run(ops, model, MARGIN, ent, rel, neg_idx, 0.0)
    assert torch.equal(first[0], loss), (float(first[0]), float(loss))
    assert torch.equal(first[1], ge), f"grad_ent: {int((first[1] != ge).sum())} elements differ"
    assert torch.equal(first[2], gr), f"grad_rel: {int((first[2] != gr).sum())} elements differ"
    halved = run(ops, model, MARGIN, ent, rel, neg_idx, 0.0, upstream=0.5)
    assert torch.equal(halved[0], loss) and torch.equal(halved[1], ge * 0.5) and torch.equal(halved[2], gr * 0.5)
    again = run(ops, model, MARGIN, ent, rel, neg_idx, 0.0, python_glue=True)
    assert ticket_ints(ops) == [0] * _lib.INBATCH_TICKET_INTS
    assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("model", REL_MODELS)
@pytest.mark.parametrize("dtype,rel_f32", [(torch.float16, False), (torch.float16, True), (torch.bfloat16, False),
                                            (torch.bfloat16, True)])
@pytest.mark.parametrize("B,K,D", HALF_SHAPES)
def test_exact_margin_half_storage(ops, model, dtype, rel_f32, B, K, D):
    """The grid is exact in f16 / bf16 and the kernels round once on store: gradients bit-equal to the port's f32 gradients cast
    once to the storage type (relation rows in the entities' type or in f32, the autocast mix).  D = 36 and 300: 16-bit rows
    whose byte length is no multiple of 16 under the four-element loads, and the sweep kernel on 16-bit operands."""
    ent, rel, neg_idx, loss, ge, gr = exact_case(model, B, K, D)
    rel_dtype = torch.float32 if rel_f32 else dtype
    e, r = ent.to(dtype), rel.to(rel_dtype)
    assert torch.equal(e.float(), ent) and torch.equal(r.float(), rel)
    for upstream in (1.0, 0.5):
        got = run(ops, model, MARGIN, e, r, neg_idx, 0.0, upstream=upstream)
        assert got[0].dtype == torch.float32 and got[1].dtype == dtype and got[2].dtype == rel_dtype
        assert torch.equal(got[0], loss), (float(got[0]), float(loss))
        assert torch.equal(got[1], (ge * upstream).to(dtype)), f"grad_ent: {int((got[1] != (ge * upstream).to(dtype)).sum())} elements differ"
        assert torch.equal(got[2], (gr * upstream).to(rel_dtype)), f"grad_rel: {int((got[2] != (gr * upstream).to(rel_dtype)).sum())} elements differ"


# ---------------------------------------------------------------------------------------------- 2. NLL against the float64 port
def gaussian_problem(model, B, K, D, skew=None):
    """The inputs of test_inbatch_loss_training_shape_vs_port."""
    gen = torch.Generator().manual_seed(7 * B + 3 * K + D)
    ent = torch.randn(B, 2, D, generator=gen) * (1.0 if model == "transe" else 0.4)
    if model == "transe":
        ent = torch.nn.functional.normalize(ent, dim=-1)
    rel = torch.randn(B, 1, D, generator=gen) * 0.3
    neg_idx = torch.randint(0, 2 * B, (B, K, 2), generator=gen)
    if skew == "one_row":
        neg_idx[..., 0] = 5
    return ent, rel, neg_idx


@functools.lru_cache(maxsize=None)
def nll_case(model, B, K, D, skew, reg, dtype, rel_dtype):
    ent, rel, neg_idx = gaussian_problem(model, B, K, D, skew)
    ent, rel = ent.to(dtype), rel.to(rel_dtype)
    return ent, rel, neg_idx, port(model, NLL, ent, rel, neg_idx, reg, torch.float64)


# (256, 64, 128): reduce G = 2, the ticket hand-over of three partial sums, the positives' terms from block 0 only
NLL_SHAPES = [(256, 64, 128, None), (3, 2, 128, None), (300, 1, 64, None), (32, 16, 300, None), (96, 64, 36, "one_row")]


@pytest.mark.parametrize("model", REL_MODELS)
@pytest.mark.parametrize("reg", [0.0, 1e-3])
@pytest.mark.parametrize("B,K,D,skew", NLL_SHAPES)
def test_nll_vs_float64_port(ops, model, reg, B, K, D, skew):
    from blp_amd import _lib
    ent, rel, neg_idx, ref = nll_case(model, B, K, D, skew, reg, torch.float32, torch.float32)
    assert _lib.lib().blp_inbatch_loss_fwd_launches(_lib.MODEL_IDS[model], B, K, D, reg) == forward_launches(model, B, K, D, reg)
    if (B, K, D) == (256, 64, 128):
        assert forward_launches(model, B, K, D, reg) == 2 and B * K > 8192
    got = run(ops, model, NLL, ent, rel, neg_idx, reg, python_glue=True)
    assert ticket_ints(ops) == [0] * _lib.INBATCH_TICKET_INTS
    assert_matches_port64(f"nll {model} {B}x{K}x{D} reg {reg}", got, ref, K)
    again = run(ops, model, NLL, ent, rel, neg_idx, reg)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("model", REL_MODELS)
@pytest.mark.parametrize("dtype,rel_f32", [(torch.float16, False), (torch.float16, True), (torch.bfloat16, False),
                                            (torch.bfloat16, True)])
@pytest.mark.parametrize("B,K,D", [(32, 16, 300), (64, 8, 64)])
def test_nll_half_storage_vs_float64_port(ops, model, dtype, rel_f32, B, K, D):
    rel_dtype = torch.float32 if rel_f32 else dtype
    ent, rel, neg_idx, ref = nll_case(model, B, K, D, None, 1e-3, dtype, rel_dtype)
    got = run(ops, model, NLL, ent, rel, neg_idx, 1e-3)
    assert got[1].dtype == dtype and got[2].dtype == rel_dtype
    assert_matches_port64(f"nll {model} {B}x{K}x{D} {dtype} rel {rel_dtype}", got, ref, K)


SATURATION_SHAPE = (64, 16, 128)


@functools.lru_cache(maxsize=None)
def saturation_case(model):
    """A grid-valued problem scaled until the scores leave expf's range on both sides (expf overflows past 88.7 and is 0 below
    -103.9), with scores of exactly 20 -- softplus' threshold -- and the f32 neighbours of 20 planted as one-hot rows (a
    single non-zero term: the same bits in any summation order).  The bilinear models' negatives carry them; TransE's
    scores are never positive, so there the positives do (softplus(-pos))."""
    B, K, D = SATURATION_SHAPE
    gen = torch.Generator().manual_seed(20 + REL_MODELS.index(model))
    above, below = 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24   # 20 x these round to the f32 numbers next to 20 (40 x: next to 40)
    neg_idx = torch.randint(0, 2 * B, (B, K, 2), generator=gen)
    if model == "transe":
        # rows of differing density: scores from about -10 to about -140
        ent = grid((B, 2, D), 1.0, torch.rand((B, 2, 1), generator=gen) * 0.7, gen)
        rel = grid((B, 1, D), 1.0, 0.15, gen)
        for b, v in ((1, 1.0), (2, above), (3, below)):  # positive b: h = t = 0, r = 20 v e_7: score -20 v
            ent[b] = 0.0
            rel[b] = 0.0
            rel[b, 0, 7] = 20.0 * v
        want = torch.tensor([-20.0, -20.0 * above, -20.0 * below])
    else:
        scale = 40.0 if model == "simple" else 20.0   # (SimplE halves its sum)
        ent = grid((B, 2, D), 1.0, 0.22 if model == "complex" else 0.3, gen)
        rel = grid((B, 1, D), scale, 0.5, gen)
        # negatives (0, 0..2) pair row 2 = e_7 with rows 3, 4, 5 = v e_7 (SimplE: in the tail half), relation 0 has `scale` at 7
        ent.view(2 * B, D)[2:6] = 0.0
        ent.view(2 * B, D)[2, 7] = 1.0
        for row, v in ((3, 1.0), (4, above), (5, below)):
            ent.view(2 * B, D)[row, 7 + (D // 2 if model == "simple" else 0)] = v
        rel[0, 0, 7] = scale
        neg_idx[0, 0:3, 0] = 2
        neg_idx[0, 0:3, 1] = torch.tensor([3, 4, 5])
        want = torch.tensor([20.0, 20.0 * above, 20.0 * below])
    pos, neg, _ = port_scores(model, ent, rel, neg_idx)
    planted = pos[1:4, 0] if model == "transe" else neg[0, 0:3]
    assert torch.equal(planted, want) and planted.abs().tolist() == [20.0, 20.0 + 2.0 ** -19, 20.0 - 2.0 ** -19]
    if model == "transe":
        assert pos.min() < -104 and neg.min() < -104 and neg.max() > -20
    else:
        assert neg.max() > 89 and neg.min() < -104 and pos.max() > 89 and pos.min() < -89
    assert max(float(pos.abs().max()), float(neg.abs().max())) < 250
    return ent, rel, neg_idx, port(model, NLL, ent, rel, neg_idx, 0.0, torch.float64)


@pytest.mark.parametrize("model", REL_MODELS)
def test_nll_saturated_scores(ops, model):
    """softplus' `> 20` branch and its guards in the backward, expf's overflow and underflow: finite, and the float64 port's."""
    B, K, D = SATURATION_SHAPE
    ent, rel, neg_idx, ref = saturation_case(model)
    got = run(ops, model, NLL, ent, rel, neg_idx, 0.0)
    assert bool(torch.isfinite(got[1]).all()) and bool(torch.isfinite(got[2]).all())
    assert_matches_port64(f"nll saturated {model}", got, ref, K)


# ---------------------------------------------------------------------------------------------- 3. non-finite inputs
@functools.lru_cache(maxsize=None)
def nonfinite_case(model, loss_fn, B, K, D, kind):
    ent, rel, neg_idx = gaussian_problem(model, B, K, D)
    clean = port(model, loss_fn, ent, rel, neg_idx, 0.0, torch.float32)[0]
    bad = ent.clone()
    bad.view(2 * B, D)[9, 3] = {"inf": float("inf"), "nan": float("nan")}[kind]
    idx = neg_idx.clone()
    idx[1, 0, 0] = idx[2, K - 1, 1] = idx[B - 1, 0, 1] = 9   # a few negatives name the row
    from oracle import ref_port
    with torch.no_grad():
        want = ref_port.compute_loss(model, loss_fn, bad, rel, idx, 0.0)
    assert not bool(torch.isfinite(want))
    return ent, bad, rel, neg_idx, idx, clean, want


@pytest.mark.parametrize("model", REL_MODELS)
@pytest.mark.parametrize("loss_fn", [MARGIN, NLL])
@pytest.mark.parametrize("kind", ["inf", "nan"])
@pytest.mark.parametrize("B,K,D", [(16, 8, 64), (128, 64, 64)])
def test_nonfinite_inputs_propagate_and_the_next_step_is_clean(ops, model, loss_fn, kind, B, K, D):
    """One +inf or NaN element in an entity row that its own positive and a few negatives read: the loss is NaN / inf exactly
    where the f32 port's is, the ticket counters are zero afterwards and the next call on the stream gives the clean loss --
    at a one-launch shape and a two-launch shape, through the Python autograd.Function and the C++ glue."""
    from blp_amd import _lib
    assert forward_launches(model, B, K, D, 0.0) == (1 if B == 16 else 2)
    ent, bad, rel, neg_idx, idx, clean, want = nonfinite_case(model, loss_fn, B, K, D, kind)
    for python_glue in (True, False):
        with torch.no_grad():
            if python_glue:
                got = ops._InBatchLoss.apply(model, loss_fn, 0.0, bad.cuda(), rel.cuda(), idx.cuda()).cpu()
                assert ticket_ints(ops) == [0] * _lib.INBATCH_TICKET_INTS
                after = ops._InBatchLoss.apply(model, loss_fn, 0.0, ent.cuda(), rel.cuda(), neg_idx.cuda()).cpu()
            else:
                got = ops.inbatch_loss(model, loss_fn, bad.cuda(), rel.cuda(), idx.cuda(), 0.0).cpu()
                after = ops.inbatch_loss(model, loss_fn, ent.cuda(), rel.cuda(), neg_idx.cuda(), 0.0).cpu()
        assert bool(torch.isnan(got)) == bool(torch.isnan(want)) and bool(torch.isinf(got)) == bool(torch.isinf(want)), (float(got), float(want))
        assert float(after) == pytest.approx(float(clean), rel=2e-6, abs=1e-7)


# ---------------------------------------------------------------------------------------------- 4. ops.score, forward and backward
def score_operands(layout, model, D, gen):
    """(heads, tails, rels) on the grid, CPU, in the layout's shapes and strides; and whether ops._two_level has to copy."""
    step = 0.25 if model == "transe" else 1.0
    p_ent, p_rel = (0.3, 0.3) if model == "transe" else (0.4, 0.6)
    if layout == "eval":        # train.py:146: every entity against each query's tail and relation
        return grid((1, 70, D), step, p_ent, gen), grid((5, 1, D), step, p_ent, gen), grid((5, 1, D), step, p_rel, gen), False
    if layout == "training":    # models.py:67
        return grid((6, 9, D), step, p_ent, gen), grid((6, 9, D), step, p_ent, gen), grid((6, 1, D), step, p_rel, gen), False
    # three leading dims none of which merges with its neighbour: no (outer, inner) pair of strides addresses the heads' rows
    heads = grid((4, 3, 2, D), step, p_ent, gen).permute(2, 1, 0, 3)
    return heads, grid((2, 3, 4, D), step, p_ent, gen), grid((2, 1, 1, D), step, p_rel, gen), True


@pytest.mark.parametrize("model", REL_MODELS)
@pytest.mark.parametrize("D", [36, 128, 300])
@pytest.mark.parametrize("layout", ["eval", "training", "permuted"])
def test_score_forward_and_backward_exact(ops, model, D, layout):
    """Scores and the gradients of all three operands bit-equal to CPU autograd of the port, upstream gradients from
    {-1, 0, 0.5, 2}; then with only `tails` requiring a gradient (NULL pointers for the two others)."""
    from oracle import ref_port
    gen = torch.Generator().manual_seed(D + 7 * REL_MODELS.index(model))
    h, t, r, copies = score_operands(layout, model, D, gen)
    want_out = ref_port.SCORE_FNS[model](h, t, r)
    w = torch.tensor([-1.0, 0.0, 0.5, 2.0])[torch.randint(0, 4, want_out.shape, generator=gen)]
    cpu = [x.clone().requires_grad_(True) for x in (h, t, r)]   # (clone keeps the strides)
    (ref_port.SCORE_FNS[model](*cpu) * w).sum().backward()

    def on_device(x):
        out = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device="cuda")
        return out.copy_(x)
    dev = [on_device(x) for x in (h, t, r)]
    assert [x.stride() for x in dev] == [x.stride() for x in (h, t, r)]
    shape = tuple(torch.broadcast_shapes(*(x.shape[:-1] for x in dev)))
    m0, m1, plan = ops._two_level(shape, dev)
    copied = [p[0].data_ptr() != x.data_ptr() for p, x in zip(plan, dev)]   # (the fallback's .contiguous() leaves the contiguous tails alone)
    assert copied == [copies, False, copies], "the layout does not take the path it is here for"
    assert ((m1 == 1 and all(p[1:] == (D, 0) for p in plan)) if copies else m1 > 1) and m0 * m1 == want_out.numel()
    for x in dev:
        x.requires_grad_(True)
    out = ops.score(model, *dev)
    assert torch.equal(out.detach().cpu(), want_out)
    (out * w.cuda()).sum().backward()
    for name, got, want in zip(("heads", "tails", "rels"), dev, cpu):
        assert got.grad.shape == want.grad.shape
        assert torch.equal(got.grad.cpu(), want.grad), f"grad of {name}: {int((got.grad.cpu() != want.grad).sum())} elements differ"
    # only tails
    dev = [on_device(x) for x in (h, t, r)]
    dev[1].requires_grad_(True)
    (ops.score(model, *dev) * w.cuda()).sum().backward()
    assert dev[0].grad is None and dev[2].grad is None
    assert torch.equal(dev[1].grad.cpu(), cpu[1].grad)
