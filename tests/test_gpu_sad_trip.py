"""The query loop of the TransE pre-pass (rank_sad.hip: rank_sad_kernel) takes four consecutive queries per trip: their
thresholds come from one LDS address, their certainly-above counts are packed a byte each into one scalar and added to one lane
of the count register (query j -> byte j % 4 of lane j / 4), and the chunk's last nq % 4 queries go one at a time.

Every case compares all four counts (gt, ge, raw and filtered) of ops.rank_all with the CPU oracle for exact equality, on the
hooks library with the knobs that send a small block to the pre-pass (sad_min_queries = 1, small_kernel = 2; the route is asserted
through ops.prepass_stats).  N = 321 rows: six tiles of 64, the last one holds ONE row; at D = 128 / 256 (one tile per wave) two
candidate groups, the second of two tiles; at D = 64 (two tiles per wave) one group of which the last wave has no tile.
"""
import numpy as np
import pytest
import torch

from test_gpu_parity import dev, oracle_counts, random_csr, random_problem

pytestmark = pytest.mark.gpu
N = 321
DIMS = [64, 128, 256]
SLICE = 256        # sad_common.h: kSQuota / kSW, a wave's slice of the pair list


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def prepass_routing():
    from blp_amd import _lib
    _lib.reset_knobs()
    _lib.set_knob("sad_min_queries", 1)
    _lib.set_knob("small_kernel", 2)
    yield
    _lib.reset_knobs()


def problem(D, Q, seed):
    """q_head = Q // 2 + 1: head and tail sides of uneven length (65 -> 33 + 32, 67 -> 34 + 33)"""
    q_head = Q // 2 + 1
    return (q_head,) + random_problem("transe", N, D, q_head, Q - q_head, seed=seed)


def coefficients(q_fixed, q_rel, q_head):
    """the vector a query's candidates are compared with: t - r for head queries, h + r for tail queries (f32, as the kernels)"""
    c = q_fixed + q_rel
    c[:q_head] = q_fixed[:q_head] - q_rel[:q_head]
    return c


def run(ops, oracle, D, table, q_fixed, q_rel, q_head, true_row=None, q_true=None, per_group=0, pass_groups=0, csr=None):
    """counts == oracle; returns (counts, the pre-pass's statistics of the call)"""
    from blp_amd import _lib
    _lib.set_knob("sad_queries_per_group", per_group)
    _lib.set_knob("sad_pass_groups", pass_groups)
    Q, n = q_fixed.shape[0], table.shape[0]
    want = oracle_counts(oracle, "transe", table, q_fixed, q_rel, q_head, true_row=true_row, q_true=q_true, csr=csr)
    ws = torch.empty(ops.rank_all_workspace_bytes("transe", n, D, q_head, Q - q_head), dtype=torch.uint8, device="cuda")
    kw = dict(true_row=true_row.cuda()) if q_true is None else dict(q_true=q_true.cuda())
    if csr is not None:
        kw.update(filt_rowptr=dev(csr[0]), filt_col=dev(csr[1]))
    got = ops.rank_all("transe", table.cuda(), q_fixed.cuda(), q_rel.cuda(), q_head, workspace=ws, **kw).cpu().numpy()
    st = ops.prepass_stats("transe", n, D, q_head, Q - q_head, ws)
    assert st["path"] == "v_sad_u16 pre-pass", st
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.nonzero((got != want).any(1))[0][:8].tolist()
    return got, st


# 256: the longest chunk (64 .. 67: one chunk of 16 trips and 0 .. 3 single queries; 257: a second chunk of ONE query);
# 16: 16 k + {0, 1, 2, 3} queries as four (257: sixteen) chunks of four whole trips and a last chunk of 0 .. 3 single queries
@pytest.mark.parametrize("per_group", [256, 16])
@pytest.mark.parametrize("Q", [64, 65, 66, 67, 257])
@pytest.mark.parametrize("D", DIMS)
def test_every_remainder(ops, oracle, D, Q, per_group):
    q_head, table, q_fixed, q_rel, true_row = problem(D, Q, seed=D + Q)
    csr = random_csr(Q, N, true_row.numpy(), seed=Q)
    got, st = run(ops, oracle, D, table, q_fixed, q_rel, q_head, true_row=true_row, per_group=per_group, csr=csr)
    assert (got[:, 0] > 0).any() and (got[:, :2] != got[:, 2:]).any()
    assert st["listed"] >= Q  # a query's own true entity is always undecided


@pytest.mark.parametrize("Q", [64, 67])
@pytest.mark.parametrize("D", DIMS)
def test_bytes_at_their_limits(ops, oracle, D, Q):
    """The true entity as a vector (q_true).  Worst: 0.9 in every element, farther from every query than any normalised row
    (0.9 D - |c|_1 against |c|_1 + sqrt(D), |c|_1 <= sqrt(D) + D / 8): every candidate is certainly above, 64 in each byte of
    each lane (128 at D = 64: two tiles per wave), so a carry into the neighbouring byte would show.  Best: the query's own
    coefficients, distance 0: every count 0, nothing to flush.  Then the two alternating inside every trip."""
    q_head, table, q_fixed, q_rel, _ = problem(D, Q, seed=7 * D + Q)
    worst = torch.full((Q, D), 0.9)
    best = coefficients(q_fixed, q_rel, q_head)
    got, _ = run(ops, oracle, D, table, q_fixed, q_rel, q_head, q_true=worst, per_group=256)
    assert (got == N).all()
    got, _ = run(ops, oracle, D, table, q_fixed, q_rel, q_head, q_true=best, per_group=256)
    assert (got[:, 0] == 0).all()
    mixed = torch.where((torch.arange(Q) % 2 == 0)[:, None], worst, best)
    got, _ = run(ops, oracle, D, table, q_fixed, q_rel, q_head, q_true=mixed, per_group=256)
    assert (got[0::2, 0] == N).all() and (got[1::2, 0] == 0).all()


@pytest.mark.parametrize("D", DIMS)
def test_equal_rows_overflow_in_every_slot(ops, oracle, D):
    """321 equal rows: every pair is undecided.  A wave's slice of the list (256 pairs) is full after its tile's first four
    queries -- the first trip --, so from the second trip on every slot of a trip takes the overflow branch (the segment's
    flag, n_t = 0), and so do the three single queries at the end."""
    Q = 67
    q_head, table, q_fixed, q_rel, true_row = problem(D, Q, seed=3 * D)
    table[:] = table[0]
    q_fixed[:] = table[0]
    got, st = run(ops, oracle, D, table, q_fixed, q_rel, q_head, true_row=true_row, per_group=256)
    assert (got[:, 0] == 0).all() and (got[:, 1] == N).all()
    full_tiles = N // 64  # (at D = 64 a wave's two tiles share its slice: at least two slices run full, at D >= 128 five)
    assert st["listed"] >= (2 if D == 64 else full_tiles) * SLICE and st["flagged_rows"] >= (Q - 5) * full_tiles * 64, st


@pytest.mark.parametrize("D", DIMS)
def test_duplicate_of_the_true_entity_in_every_slot(ops, oracle, D):
    """Row 300 is a bitwise copy of row 7, the true entity of the queries at positions 8, 9, 10, 11 (slots 0 .. 3 of a trip),
    33 (the tail side's first query, slot 1) and 64 (the single query after the trips): ge counts the copy, gt does not."""
    Q = 65
    q_head, table, q_fixed, q_rel, true_row = problem(D, Q, seed=5 * D)
    table[300] = table[7]
    hit = [8, 9, 10, 11, 33, 64]
    true_row[hit] = 7
    got, _ = run(ops, oracle, D, table, q_fixed, q_rel, q_head, true_row=true_row, per_group=256)
    assert (got[hit, 1] == got[hit, 0] + 2).all()  # the entity itself and its copy


@pytest.mark.parametrize("D", DIMS)
def test_queries_past_the_chunk_list_nothing(ops, oracle, D):
    """65 queries as one chunk: 16 trips and ONE single query; thr_s and the query image behind it hold padding that would read
    as undecided against every row.  The expected number of listed pairs comes from the same block cut into chunks of 16 and
    of 32 queries: there every chunk but the last is whole trips, and the last is the one query alone, so no trip of those
    runs reaches past a chunk's end whatever the loop does with a partial trip; a pair's being undecided depends on its query's
    thresholds and its candidate group's largest residual, not on the chunk length, and no list comes near the quota."""
    q_head, table, q_fixed, q_rel, true_row = problem(D, 65, seed=11 * D)
    listed = [run(ops, oracle, D, table, q_fixed, q_rel, q_head, true_row=true_row, per_group=pg)[1]["listed"] for pg in (16, 32, 256)]
    assert listed[0] == listed[1] and 65 <= listed[0] < SLICE
    assert listed[2] == listed[0], listed


@pytest.mark.parametrize("D", [64, 128])
def test_multi_slab_with_filter(ops, oracle, D):
    """sad_pass_groups = 1 on 1 000 rows: two (D = 64) or four slabs, each slab's launch walks the trips again; only the first
    carries the filter role, whose `removed` is applied once."""
    Q, n = 67, 1000
    q_head = Q // 2 + 1
    table, q_fixed, q_rel, true_row = random_problem("transe", n, D, q_head, Q - q_head, seed=13 * D)
    csr = random_csr(Q, n, true_row.numpy(), seed=D)
    got, _ = run(ops, oracle, D, table, q_fixed, q_rel, q_head, true_row=true_row, per_group=256, pass_groups=1, csr=csr)
    assert (got[:, 1] > got[:, 3]).any()
