"""The launch chain in front of and behind the TransE pre-pass (rank_sad.hip): one prelude launch for the true keys and the
range of what is quantised (sad_prelude_kernel), the range finished by the quantising workgroups themselves at every size,
the query image written eight coefficients per thread, and one refinement launch with a pair role and a flag-sweep role
(sad_refine_kernel).  Every case compares the counts of the pre-pass path, bit for bit, with those of the exact f32 kernels
(knob rank_kernel = 1) on the same device inputs; cases of at most 64 queries with the CPU oracle as well.  The knobs are
those of test_gpu_sad_inline_refine.py: sad_min_queries = 1 and the small-block kernel off, so that any block takes the
pre-pass.  The quantise kernel keeps no size threshold (every workgroup reduces the prelude's partial results), so there is
no block "on each side" of one; what the shapes do cross is the prelude's own edges: one wave of queries (<= 64), one
workgroup (<= 256), several, and a table of less than one workgroup's loads up to several workgroups'."""
import numpy as np
import pytest
import torch

from test_gpu_parity import dev, oracle_counts, random_csr, random_problem

pytestmark = pytest.mark.gpu

ORACLE_MAX_QUERIES = 64


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def clean_knobs():
    from blp_amd import _lib
    _lib.reset_knobs()
    yield
    _lib.reset_knobs()


def route(exact, pass_groups=0):
    from blp_amd import _lib
    _lib.reset_knobs()
    _lib.set_knob("small_kernel", 2)
    if exact:
        _lib.set_knob("rank_kernel", 1)
    else:
        _lib.set_knob("sad_min_queries", 1)
        _lib.set_knob("sad_pass_groups", pass_groups)


def check(ops, oracle, table, q_fixed, q_rel, true_row, q_head, pass_groups=0, filtered=True, dev_table=None):
    """counts of the pre-pass path == counts of the exact kernels (== the oracle up to ORACLE_MAX_QUERIES queries), raw and
    filtered; returns the pre-pass's statistics.  dev_table: the table as the device sees it (a strided view), if not
    table.cuda()."""
    Q, (N, D) = q_fixed.shape[0], table.shape
    q_tail = Q - q_head
    csr = random_csr(Q, N, true_row.numpy(), seed=Q + N + D) if filtered else None
    kw = {} if csr is None else {"filt_rowptr": dev(csr[0]), "filt_col": dev(csr[1])}
    t = table.cuda() if dev_table is None else dev_table
    args = (t, q_fixed.cuda(), q_rel.cuda(), q_head)
    route(exact=True)
    want = ops.rank_all("transe", *args, true_row=true_row.cuda(), **kw).cpu().numpy()
    route(exact=False, pass_groups=pass_groups)
    ws = torch.empty(ops.rank_all_workspace_bytes("transe", N, D, q_head, q_tail), dtype=torch.uint8, device="cuda")
    got = ops.rank_all("transe", *args, true_row=true_row.cuda(), workspace=ws, **kw).cpu().numpy()
    st = ops.prepass_stats("transe", N, D, q_head, q_tail, ws)
    assert st["path"] == "v_sad_u16 pre-pass"
    assert np.array_equal(got, want)
    if Q <= ORACLE_MAX_QUERIES:
        assert np.array_equal(got, oracle_counts(oracle, "transe", table, q_fixed, q_rel, q_head, true_row=true_row, csr=csr))
    return st


def sides(Q, side):
    return Q if side == "head" else 0  # q_head: every query replaces the head (q_tail = 0) or the tail (q_head = 0)


@pytest.mark.parametrize("side", ["head", "tail"])
@pytest.mark.parametrize("Q", [1, 65, 320])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_shapes(ops, oracle, D, N, Q, side):
    """Tables of one row, one tile less a row, one tile, one tile and a row, 16 tiles; one query, two waves of the prelude
    with one live lane in the second, two workgroups of it; all queries on one side."""
    q_head = sides(Q, side)
    table, q_fixed, q_rel, true_row = random_problem("transe", N, D, q_head, Q - q_head, seed=D + N + Q)
    st = check(ops, oracle, table, q_fixed, q_rel, true_row, q_head)
    assert st["listed"] + st["flagged_rows"] >= Q  # a query's own true entity is always undecided


@pytest.mark.parametrize("D", [64, 128, 256])
def test_several_slabs(ops, oracle, D):
    """sad_pass_groups = 1: a candidate group per slab, the refinement launch once per slab with slab-relative rows."""
    table, q_fixed, q_rel, true_row = random_problem("transe", 1000, D, 150, 170, seed=10 + D)
    check(ops, oracle, table, q_fixed, q_rel, true_row, 150, pass_groups=1)
    table, q_fixed, q_rel, true_row = random_problem("transe", 1000, D, 30, 34, seed=20 + D)
    check(ops, oracle, table, q_fixed, q_rel, true_row, 30, pass_groups=1)


@pytest.mark.parametrize("Q", [64, 320])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_row_stride_larger_than_width(ops, oracle, D, Q):
    """The table as a view of a wider array: the prelude's table workgroups and the quantiser step by the stride."""
    q_head = Q // 2 - 3
    table, q_fixed, q_rel, true_row = random_problem("transe", 1000, D, q_head, Q - q_head, seed=30 + D + Q)
    wide = torch.full((1000, D + 8), float("nan"))  # what lies between the rows must never be read as data
    wide[:, :D] = table
    view = wide.cuda()[:, :D]
    assert view.stride(0) == D + 8
    check(ops, oracle, table, q_fixed, q_rel, true_row, q_head, dev_table=view)


@pytest.mark.parametrize("Q", [64, 320])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_gathered_rows_equal_dense_rows(ops, oracle, D, Q):
    """The queries as indices into the table and the relation matrix (rank_all_idx: QRows with an index) and as dense
    (Q, D) arrays: the prelude and the quantiser address both through QRows::row."""
    N, nrel, q_head = 1000, 11, Q // 2 + 1
    g = torch.Generator().manual_seed(40 + D + Q)
    table = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    rel_w = (torch.rand(nrel, D, generator=g) - 0.5) * 0.25
    fixed_row, true_row = torch.randint(0, N, (Q,), generator=g), torch.randint(0, N, (Q,), generator=g)
    rel_ids = torch.randint(0, nrel, (Q,), generator=g)
    q_fixed, q_rel = table[fixed_row].clone(), rel_w[rel_ids].clone()
    check(ops, oracle, table, q_fixed, q_rel, true_row, q_head, filtered=False)  # dense rows; leaves the pre-pass routing set
    want = ops.rank_all("transe", table.cuda(), q_fixed.cuda(), q_rel.cuda(), q_head, true_row=true_row.cuda()).cpu().numpy()
    got = ops.rank_all_idx("transe", table.cuda(), fixed_row.cuda(), rel_w.cuda(), rel_ids.cuda(), q_head, true_row.cuda()).cpu().numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("Q", [64, 320])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_constant_table(ops, oracle, D, Q):
    """Every table element the same value: with constant queries as well the range is degenerate (hi == lo) and the pre-pass
    stands down -- every tile is swept; with random relations the range is that of the coefficients alone."""
    N, q_head = 1000, Q // 2
    _, q_fixed, q_rel, true_row = random_problem("transe", N, D, q_head, Q - q_head, seed=50 + D + Q)
    table = torch.full((N, D), 0.25)
    q_fixed = torch.full((Q, D), 0.25)
    check(ops, oracle, table, q_fixed, q_rel, true_row, q_head)
    st = check(ops, oracle, table, q_fixed, torch.zeros(Q, D), true_row, q_head)
    assert st["listed"] == 0  # degenerate: the pre-pass kernel returned at once, the sweep took all tiles


@pytest.mark.parametrize("where", ["table", "query"])
@pytest.mark.parametrize("Q", [64, 320])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_nan_and_inf(ops, oracle, D, Q, where):
    """One NaN and one Inf, in table rows or in queries (a fixed-entity row, a relation row): those rows / queries are left
    to the exact path (SadRange::see skips the values, the quantiser marks the row or the query) and the counts stay exact."""
    N, q_head = 1000, Q // 2
    table, q_fixed, q_rel, true_row = random_problem("transe", N, D, q_head, Q - q_head, seed=60 + D + Q)
    if where == "table":
        table[7, 3] = float("nan")
        table[N - 2, D - 1] = float("inf")
        floor = 2 * Q  # the two rows against every query
    else:
        q_fixed[1, D - 1] = float("nan")
        q_rel[Q - 2, 0] = float("-inf")
        floor = 2 * N  # the two queries against every row
    st = check(ops, oracle, table, q_fixed, q_rel, true_row, q_head)
    assert st["listed"] + st["flagged_rows"] >= floor


@pytest.mark.parametrize("Q", [64, 320])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_exact_duplicates_of_the_true_entity(ops, oracle, D, Q):
    """Every 16th row an exact copy of some query's true row: ties, which only the exact arithmetic of the true key decides
    (ge counts them, gt does not)."""
    N, q_head = 1000, Q // 2
    table, q_fixed, q_rel, true_row = random_problem("transe", N, D, q_head, Q - q_head, seed=70 + D + Q)
    for k, row in enumerate(range(0, N, 16)):
        table[row] = table[int(true_row[(5 * k) % Q])]
    st = check(ops, oracle, table, q_fixed, q_rel, true_row, q_head)
    assert st["listed"] + st["flagged_rows"] >= Q + N // 16 // 2


# listed + flagged_rows of the 150 + 170 queries x 1 000 rows x 128 block below (random_problem seed 4128, no filter) with the
# library of the parent commit 9a19f58 (true_key_kernel + sad_range_kernel + the two-elements-per-thread quantiser):
PARENT_UNDECIDED_320x1000 = 568  # listed 568, flagged_rows 0


def test_undecided_pairs_as_the_parent(ops, oracle):
    """The quantisation map is the parent's bit for bit (the same values reduced by min and max); the thresholds may move by
    an LSB, since the residuals are summed in another order.  So the pairs left to the exact path stay within 1 % of the
    parent's number."""
    table, q_fixed, q_rel, true_row = random_problem("transe", 1000, 128, 150, 170, seed=4128)
    st = check(ops, oracle, table, q_fixed, q_rel, true_row, 150, filtered=False)
    undecided = st["listed"] + st["flagged_rows"]
    print(f"listed {st['listed']} flagged_rows {st['flagged_rows']} parent {PARENT_UNDECIDED_320x1000}")
    assert abs(undecided - PARENT_UNDECIDED_320x1000) <= 0.01 * PARENT_UNDECIDED_320x1000
