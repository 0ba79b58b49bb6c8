"""The TransE pre-pass's own refinement (rank_sad.hip): a workgroup whose list of undecided pairs holds at most
kSInlineCap entries re-scores them itself before it exits; longer lists go through the global list as before.  Every
case compares the raw and filtered counts of ops.rank_all with the CPU oracle for exact equality, on the hooks library
with the knobs that send a 320-query block against a 1 000-row table to the pre-pass (sad_min_queries = 1, and the
small-block kernel off, which would otherwise take so small a block first)."""
import numpy as np
import pytest
import torch

from test_gpu_parity import dev, oracle_counts, random_csr, random_problem

pytestmark = pytest.mark.gpu

INLINE_CAP = 256   # rank_sad.hip: kSInlineCap
QUOTA = 1024       # sad_common.h: kSQuota
N, Q_HEAD, Q_TAIL = 1000, 150, 170  # 16 tiles (the last one partial): four candidate groups, two at D = 64
Q = Q_HEAD + Q_TAIL
# queries per workgroup: 16 and the library's own choice (0), which for so small a grid is 16 as well
# (rank_sad.hip: sad_queries_per_group -- one round of workgroups whatever the length, so the shortest wins): 20 full chunks.
# 256, beyond what the shapes above need, gives the partial last chunk (256 + 64 queries) and workgroups to which a random
# table alone leaves a few dozen pairs; test_listed_is_exactly_the_undecided_pairs has a partial chunk at 16 too.
PER_GROUP = [16, 0, 256]
DEFAULT_PER_GROUP = 16


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


def run(ops, oracle, table, q_fixed, q_rel, true_row, D, per_group, pass_groups=0, seed=0):
    """counts == oracle (raw and filtered); returns the pre-pass's own statistics of the call"""
    from blp_amd import _lib
    _lib.set_knob("sad_queries_per_group", per_group)
    _lib.set_knob("sad_pass_groups", pass_groups)
    rowptr, col = random_csr(Q, N, true_row.numpy(), seed=seed + D)
    want = oracle_counts(oracle, "transe", table, q_fixed, q_rel, Q_HEAD, true_row=true_row, csr=(rowptr, col))
    ws = torch.empty(ops.rank_all_workspace_bytes("transe", N, D, Q_HEAD, Q_TAIL), dtype=torch.uint8, device="cuda")
    got = ops.rank_all("transe", table.cuda(), q_fixed.cuda(), q_rel.cuda(), Q_HEAD, true_row=true_row.cuda(),
                       filt_rowptr=dev(rowptr), filt_col=dev(col), workspace=ws).cpu().numpy()
    st = ops.prepass_stats("transe", N, D, Q_HEAD, Q_TAIL, ws)
    assert st["path"] == "v_sad_u16 pre-pass"
    assert np.array_equal(got, want)
    return st


def ties_per_workgroup(table, true_row, D, per_group):
    """exact (query, row) ties -- the row's vector is the query's true entity's, bit for bit: undecided whatever the band --
    counted per pre-pass workgroup (candidate group of 4 x TPW tiles, chunk of per_group queries)"""
    _, ident = np.unique(table.numpy().view(np.uint32), axis=0, return_inverse=True)
    ident = ident.reshape(-1)
    tie = ident[None, :] == ident[true_row.numpy()][:, None]  # (Q, N)
    rows_per_group = 64 * 4 * (2 if D == 64 else 1)
    n_groups, n_chunks = -(-N // rows_per_group), -(-Q // per_group)
    out = np.zeros((n_chunks, n_groups), np.int64)
    qs, rs = np.nonzero(tie)
    np.add.at(out, (qs // per_group, rs // rows_per_group), 1)
    return out


@pytest.mark.parametrize("per_group", PER_GROUP)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_random_table(ops, oracle, D, per_group):
    """Normalised random rows: few undecided pairs, most workgroups refine nothing or a handful."""
    table, q_fixed, q_rel, true_row = random_problem("transe", N, D, Q_HEAD, Q_TAIL, seed=D + per_group)
    st = run(ops, oracle, table, q_fixed, q_rel, true_row, D, per_group)
    assert st["listed"] >= Q  # a query's own true entity is always undecided


def partly_filled_problem(D, seed):
    table, q_fixed, q_rel, true_row = random_problem("transe", N, D, Q_HEAD, Q_TAIL, seed=seed)
    for k, row in enumerate(range(0, N, 16)):  # every 16th row: an exact duplicate of some query's true row
        table[row] = table[int(true_row[(5 * k) % Q])]
    return table, q_fixed, q_rel, true_row


@pytest.mark.parametrize("per_group", [16, 0])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_partly_filled_lists(ops, oracle, D, per_group):
    """Exact duplicates of true rows on every 16th row: lists of 1 .. kSInlineCap pairs, refined in the kernel with partly
    filled waves.  What the CPU bounds here is the exact ties, a LOWER bound of a list's length: the list also holds the
    pairs the band leaves undecided on random rows (test_random_table: a handful per 16 x 256 pairs), which is why the ties
    are held to half the cap.  test_listed_is_exactly_the_undecided_pairs has lists whose lengths the CPU knows exactly."""
    table, q_fixed, q_rel, true_row = partly_filled_problem(D, seed=100 + D + per_group)
    ties = ties_per_workgroup(table, true_row, D, per_group or DEFAULT_PER_GROUP)
    assert ties.max() >= 1 and (ties >= 1).sum() > ties.size // 2 and ties.max() <= INLINE_CAP // 2
    st = run(ops, oracle, table, q_fixed, q_rel, true_row, D, per_group)
    assert st["listed"] >= ties.sum()


@pytest.mark.parametrize("per_group", PER_GROUP)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_overflowing_lists(ops, oracle, D, per_group):
    """8 distinct rows repeated, except in the last candidate group, whose rows stay random: the workgroups of the other
    groups tie beyond the cap (at 256 queries per workgroup beyond the quota as well: flagged segments), those of the last
    group have short lists (two duplicates there) -- the global list, the flag sweep and the in-kernel path in one launch, nothing counted twice."""
    table, q_fixed, q_rel, true_row = random_problem("transe", N, D, Q_HEAD, Q_TAIL, seed=200 + D + per_group)
    rows_per_group = 64 * 4 * (2 if D == 64 else 1)
    last_group = (N - 1) // rows_per_group * rows_per_group  # first row of the last candidate group
    table[:last_group] = table[:8].repeat(last_group // 8, 1)
    table[last_group + 3], table[N - 1] = table[0], table[1]  # two of the eight once more: a quarter of the queries tie there
    true_row = true_row % last_group  # every query ties with an eighth of the repeated rows
    ties = ties_per_workgroup(table, true_row, D, per_group or DEFAULT_PER_GROUP)
    assert ties[:, :-1].min() > INLINE_CAP  # (also the partial last chunk: 64 queries x 32 ties and more)
    assert 1 <= ties[:, -1].max() <= INLINE_CAP // 2  # (a lower bound of those lists, as in test_partly_filled_lists)
    st = run(ops, oracle, table, q_fixed, q_rel, true_row, D, per_group)
    if per_group == 256:
        assert ties[:-1, :-1].min() > QUOTA and st["flagged_rows"] > 0
    else:
        assert st["listed"] + st["flagged_rows"] >= ties.sum()  # (a wave's slice that ran full flags the segment instead)


@pytest.mark.parametrize("per_group", PER_GROUP)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_exact_only_rows_and_queries(ops, oracle, D, per_group):
    """A row with a NaN, a row with an Inf (kSRowExact: undecided against every query) and a query whose relation row has
    an Inf (thresholds that decide nothing)."""
    table, q_fixed, q_rel, true_row = partly_filled_problem(D, seed=300 + D + per_group)
    table[7, 3] = float("nan")
    table[N - 2, D - 1] = float("inf")
    q_rel[Q_HEAD + 5, 1] = float("inf")
    st = run(ops, oracle, table, q_fixed, q_rel, true_row, D, per_group)
    assert st["listed"] + st["flagged_rows"] >= 2 * Q + N - 2  # the two rows against every query, the query against every row


@pytest.mark.parametrize("D", [64, 128, 256])
def test_several_slabs(ops, oracle, D):
    """One candidate group per pass: several slabs, so the in-kernel path reads slab-relative rows."""
    table, q_fixed, q_rel, true_row = partly_filled_problem(D, seed=400 + D)
    table[N - 5, 0] = float("nan")  # an exact-only row in the last slab
    st = run(ops, oracle, table, q_fixed, q_rel, true_row, D, 16, pass_groups=1)
    rows_per_group = 64 * 4 * (2 if D == 64 else 1)
    last = ties_per_workgroup(table, true_row, D, 16)[:, -1]  # the statistics are the last slab's
    assert st["listed"] >= last.sum()
    assert N > rows_per_group  # more than one slab


def lattice_problem(D, q_head, q_tail, seed):
    """Every row a constant vector, row i = (i, i, ..., i), relations constant vectors of small integers: every distance is
    D x an integer, exact in f32, and two candidates of a query either tie exactly or differ by at least D -- thirty times
    the widest band the pre-pass can have here (quantisation 2 x 0.51 D steps of 1 / 65.6, rounding terms below 5).  So the
    undecided pairs are exactly the ties, and the CPU counts them in integers."""
    g = torch.Generator().manual_seed(seed)
    Qn = q_head + q_tail
    fixed = torch.randint(0, N, (Qn,), generator=g)
    true_row = torch.randint(0, N, (Qn,), generator=g)
    rel = torch.randint(0, 6, (Qn,), generator=g)
    table = torch.arange(N, dtype=torch.float32)[:, None].repeat(1, D).contiguous()
    ones = torch.ones(1, D)
    cand = torch.arange(N)[None, :]
    head = (torch.arange(Qn) < q_head)[:, None]
    # head-replacing (e + r) - f, tail-replacing (f + r) - e, per coordinate
    dist = torch.where(head, cand + rel[:, None] - fixed[:, None], fixed[:, None] + rel[:, None] - cand).abs()
    undecided = dist == dist[torch.arange(Qn), true_row][:, None]  # (Q, N)
    return table, fixed[:, None] * ones, rel[:, None] * ones, true_row, undecided.numpy()


@pytest.mark.parametrize("pass_groups", [0, 1])
@pytest.mark.parametrize("per_group", [16, 256])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_listed_is_exactly_the_undecided_pairs(ops, oracle, D, per_group, pass_groups):
    """prepass_stats().listed == the CPU's count, to the pair: a pair counted twice, a list left out or a counter not cleared
    between slabs (pass_groups = 1: the statistics are the last slab's) would show.  150 + 173 queries: a partial last chunk
    at 16 as well.  Every workgroup's list is within the cap, most of them non-empty: all of it is refined in the kernel."""
    q_head, q_tail = 150, 173
    table, q_fixed, q_rel, true_row, undecided = lattice_problem(D, q_head, q_tail, seed=500 + D + per_group)
    from blp_amd import _lib
    _lib.set_knob("sad_queries_per_group", per_group)
    _lib.set_knob("sad_pass_groups", pass_groups)
    rows_per_group = 64 * 4 * (2 if D == 64 else 1)
    n_groups, n_chunks = -(-N // rows_per_group), -(-(q_head + q_tail) // per_group)
    lists = np.zeros((n_chunks, n_groups), np.int64)  # the workgroups' lists
    qs, rs = np.nonzero(undecided)
    np.add.at(lists, (qs // per_group, rs // rows_per_group), 1)
    assert lists.max() <= INLINE_CAP and (lists >= 1).sum() > lists.size // 2
    want = oracle_counts(oracle, "transe", table, q_fixed, q_rel, q_head, true_row=true_row)
    ws = torch.empty(ops.rank_all_workspace_bytes("transe", N, D, q_head, q_tail), dtype=torch.uint8, device="cuda")
    got = ops.rank_all("transe", table.cuda(), q_fixed.cuda(), q_rel.cuda(), q_head, true_row=true_row.cuda(), workspace=ws).cpu().numpy()
    st = ops.prepass_stats("transe", N, D, q_head, q_tail, ws)
    assert st["path"] == "v_sad_u16 pre-pass"
    assert np.array_equal(got, want)
    assert st["flagged_rows"] == 0
    assert st["listed"] == (lists[:, -1].sum() if pass_groups else lists.sum())
