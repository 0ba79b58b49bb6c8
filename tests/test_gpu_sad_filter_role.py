"""The filter role of the TransE pre-pass launch (rank_sad.hip: sad_filter_role, sad_finalize_kernel) on the device.

In the filtered setting the rows a query's filter removes are re-scored by extra workgroups at the end of the first
rank_sad_kernel launch, counted per query in the workspace's `removed` array and subtracted by a one-thread-per-query
finalize.  Every test here runs ops.rank_all on the hooks library with sad_min_queries = 64 and small_kernel = 2 (the pre-pass
on small blocks; the route is asserted through ops.prepass_stats) and requires all four counts of EVERY query to equal the CPU
oracle's (oracle.rank_counts) given the CSR of the rows the filter removes -- that CSR is built here by a restatement of the
blp_filter contract (include/blp_hip.h): an entry equal to the query's `exclude` id removes nothing; with ent2idx an id
outside the map or mapped to -1 removes nothing; row_base is subtracted and a row outside [0, N) removes nothing; hi <= lo is
an empty segment.

Shapes: 320 .. 1 000 rows, 130 .. 600 queries, D = 64 / 128 / 256 -- a role workgroup owns runs of 64 queries and takes 256
entries per trip, a pre-pass workgroup 4 (D = 64: 8) tiles of 64 rows and 16 .. 256 queries.  The one exception is the heavy
gate, which the library arms from 2^27 (query, row) pairs on (rank_common.h: kFallbackMinPairs): 52 900 queries x 2 540 rows at
D = 64, the smallest block of whole pre-pass groups that reaches it.
"""
import numpy as np
import pytest
import torch

from test_gpu_parity import oracle_counts

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 1 << 16
SAD_PATH = "v_sad_u16 pre-pass"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _prepass_route():
    from blp_amd import _lib
    _lib.reset_knobs()
    _lib.set_knob("sad_min_queries", 64)
    _lib.set_knob("small_kernel", 2)
    yield _lib.set_knob
    _lib.reset_knobs()


class Problem:
    def __init__(self, D, N, q_head, q_tail, seed=0):
        gen = torch.Generator().manual_seed(seed)
        self.D, self.N, self.q_head, self.Q = D, N, q_head, q_head + q_tail
        self.table = torch.nn.functional.normalize(torch.randn(N, D, generator=gen), dim=-1)
        rel_w = (torch.rand(7, D, generator=gen) - 0.5) * 0.25
        self.q_fixed = self.table[torch.randint(0, N, (self.Q,), generator=gen)].clone()
        self.q_rel = rel_w[torch.randint(0, 7, (self.Q,), generator=gen)].clone()
        self.true_row = torch.randint(0, N, (self.Q,), generator=gen)


def removed_rows(f, Q, N):
    """The blp_filter contract restated: per query the table rows its segment removes, one per entry that removes something."""
    lo, hi, val = (np.asarray(x, np.int64) for x in (f.seg_lo, f.seg_hi, f.values))
    rowptr, col = [0], []
    for q in range(Q):
        for k in range(int(lo[q]), max(int(hi[q]), int(lo[q]))):
            v = int(val[k])
            if f.exclude is not None and v == int(f.exclude[q]):
                continue
            if f.ent2idx is not None:
                v = int(f.ent2idx[v]) if 0 <= v < len(f.ent2idx) else -1
            v -= int(f.row_base)
            if 0 <= v < N:
                col.append(v)
        rowptr.append(len(col))
    return np.asarray(rowptr, np.int64), np.asarray(col, np.int64)


def segments(ops, lists, exclude=None, ent2idx=None, row_base=0, gap=3):
    """A SegmentFilter whose query q lists ``lists[q]``; ``gap`` live-looking values (row 1) lie between the segments, so an
    entry read from a neighbour's range would remove something."""
    values, lo, hi = [], [], []
    for entries in lists:
        values += [1] * gap
        lo.append(len(values))
        values += [int(e) for e in entries]
        hi.append(len(values))
    t = lambda x: None if x is None else torch.as_tensor(np.asarray(x, np.int64))
    return ops.SegmentFilter(t(lo), t(hi), t(values + [1] * gap), t(exclude), t(ent2idx), row_base)


def random_lists(p, seed, max_len=9, every=3):
    rng = np.random.default_rng(seed)
    out = []
    for q in range(p.Q):
        n = 0 if q % every == 0 else int(rng.integers(0, max_len + 1))
        c = rng.choice(p.N, size=n, replace=False)
        out.append(c[c != int(p.true_row[q])])
    return out


def to_dev(f):
    return f._replace(**{k: getattr(f, k).to(DEV) for k in ("seg_lo", "seg_hi", "values", "exclude", "ent2idx") if getattr(f, k) is not None})


def rank(ops, p, f, table=None, q_true=None, ws=None, path=SAD_PATH):
    table = p.table if table is None else table
    N = table.shape[0]
    nbytes = ops.rank_all_workspace_bytes("transe", N, p.D, p.q_head, p.Q - p.q_head)
    if ws is None:
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
    kw = dict(true_row=p.true_row.to(DEV)) if q_true is None else dict(q_true=q_true.to(DEV))
    got = ops.rank_all("transe", table.to(DEV), p.q_fixed.to(DEV), p.q_rel.to(DEV), p.q_head, workspace=ws,
                       filter=None if f is None else to_dev(f), **kw)
    if path is not None:
        stats = ops.prepass_stats("transe", N, p.D, p.q_head, p.Q - p.q_head, ws)
        assert stats["path"] == path, stats
    return got.cpu().numpy()


def want(oracle, p, f, table=None, q_true=None):
    table = p.table if table is None else table
    csr = None if f is None else removed_rows(f, p.Q, table.shape[0])
    kw = dict(true_row=p.true_row) if q_true is None else dict(q_true=q_true)
    return oracle_counts(oracle, "transe", table, p.q_fixed, p.q_rel, p.q_head, csr=csr, **kw)


def check(got, exp, what=""):
    assert got.dtype == np.int32 and got.shape == exp.shape
    assert np.array_equal(got, exp), (what, np.nonzero((got != exp).any(1))[0][:8].tolist())


SHAPES = [(64, 1000, 77, 120), (128, 333, 70, 61), (128, 650, 300, 299), (256, 330, 1, 130)]   # D, N, q_head, q_tail


@pytest.mark.parametrize("D,N,q_head,q_tail", SHAPES)
def test_random_filter_odd_sizes_and_no_filter(ops, oracle, D, N, q_head, q_tail):
    """q_head != q_tail, Q no multiple of 64 nor of the queries per group, N no multiple of 64 (1 000 also no multiple of the
    pre-pass group's 512 rows at D = 64).  With filter=None the same block is unchanged: no role workgroups, the old finalize."""
    p = Problem(D, N, q_head, q_tail, seed=D + N)
    assert p.Q % 64 and N % 64 and q_head != q_tail
    f = segments(ops, random_lists(p, 1))
    exp = want(oracle, p, f)
    assert (exp[:, :2] != exp[:, 2:]).any()
    check(rank(ops, p, f), exp)
    raw = rank(ops, p, None)
    check(raw, want(oracle, p, None))
    assert np.array_equal(raw[:, :2], exp[:, :2]) and np.array_equal(raw[:, 2:], raw[:, :2])


@pytest.mark.parametrize("per_group", [16, 256])
def test_forced_queries_per_group(ops, oracle, _prepass_route, per_group):
    _prepass_route("sad_queries_per_group", per_group)
    p = Problem(128, 650, 300, 299, seed=5)
    assert p.Q % per_group
    f = segments(ops, random_lists(p, 2))
    check(rank(ops, p, f), want(oracle, p, f))


@pytest.mark.parametrize("D", [64, 128, 256])
def test_empty_filter(ops, oracle, D):
    """Every segment empty (lo == hi, and hi < lo on every other query): filtered counts equal raw counts."""
    p = Problem(D, 400, 100, 93, seed=D)
    f = segments(ops, [[] for _ in range(p.Q)])
    f = f._replace(seg_hi=f.seg_hi - (torch.arange(p.Q) % 2) * 2)
    got = rank(ops, p, f)
    check(got, want(oracle, p, None))
    assert np.array_equal(got[:, :2], got[:, 2:])


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("where", [0, 63, 64, 129])
def test_one_long_segment(ops, oracle, D, where):
    """One query lists 300 rows -- more than a trip's 256, the second trip partial -- and no other query of its run of 64 lists
    anything: the numbering across the run, the search at the prefix's flat stretches (first slot, last slot of a run, first of
    the next, the ragged last run) and the idle lanes of the last trip."""
    p = Problem(D, 500, 70, 62, seed=where)
    assert p.Q == 132 and where < p.Q
    rng = np.random.default_rng(where)
    long = rng.choice(p.N, size=300, replace=False)
    lists = [long[long != int(p.true_row[q])] if q == where else [] for q in range(p.Q)]
    other = (where + 64) % 128    # a query of another run keeps a short list
    lists[other] = [r for r in (3, 5) if r != int(p.true_row[other])]
    f = segments(ops, lists)
    exp = want(oracle, p, f)
    assert len(lists[where]) > 256 + 32 and exp[where, 1] > exp[where, 3]
    check(rank(ops, p, f), exp)


@pytest.mark.parametrize("D", [64, 128])
def test_entries_that_remove_nothing(ops, oracle, D):
    """exclude (an id, compared before the map), ent2idx holes (-1), ids outside the map (beyond it, negative, 2^33 + a live id)
    and, on a candidate shard with row_base = 100, rows before and behind the shard."""
    p = Problem(D, 700, 80, 75, seed=11)
    rng = np.random.default_rng(3)
    n_ids = p.N + 50
    perm = rng.permutation(p.N)
    ent2idx = np.full(n_ids, -1, np.int64)
    ids = np.sort(rng.choice(n_ids, size=p.N, replace=False))
    ent2idx[ids] = perm                                   # id -> row, 50 holes
    row2id = np.empty(p.N, np.int64)
    row2id[perm] = ids
    holes = np.setdiff1d(np.arange(n_ids), ids)
    exclude = row2id[p.true_row.numpy()]                  # the triple's own entity, as an id
    lists = []
    for q in range(p.Q):
        live = row2id[rng.choice(p.N, size=6, replace=False)]
        live = live[live != exclude[q]]
        lists.append(list(live[:3]) + [exclude[q], holes[q % len(holes)], n_ids, n_ids + 12345, -1, (1 << 33) + int(live[0])] + list(live[3:]))
    f = segments(ops, lists, exclude=exclude, ent2idx=ent2idx)
    exp = want(oracle, p, f)
    rowptr, _ = removed_rows(f, p.Q, p.N)
    assert (np.diff(rowptr) <= 6).all() and (np.diff(rowptr) >= 5).all() and (exp[:, 1] - exp[:, 3]).max() > 0
    check(rank(ops, p, f), exp, "whole table")
    # the shard [100, 550): the same ids, rows outside the shard remove nothing; the true entities come as vectors
    shard, q_true = p.table[100:550], p.table[p.true_row]
    fs = f._replace(row_base=100)
    exp_s = want(oracle, p, fs, table=shard, q_true=q_true)
    assert removed_rows(fs, p.Q, 450)[0][-1] < rowptr[-1]
    check(rank(ops, p, fs, table=shard, q_true=q_true), exp_s, "shard")


@pytest.mark.parametrize("D", [64, 128, 256])
def test_exact_tie_lowers_ge_only(ops, oracle, D):
    """Every query lists a row that is a bitwise copy of its true entity's row: ge_filtered drops by one, gt_filtered does not."""
    p = Problem(D, 640 + 37, 90, 81, seed=21)
    half = p.N // 2
    p.table[half:2 * half] = p.table[:half]               # row r + half duplicates row r
    p.true_row = p.true_row % half
    f = segments(ops, [[int(p.true_row[q]) + half] for q in range(p.Q)])
    exp = want(oracle, p, f)
    assert np.array_equal(exp[:, 2], exp[:, 0]) and np.array_equal(exp[:, 3], exp[:, 1] - 1)
    check(rank(ops, p, f), exp)


@pytest.mark.parametrize("D", [64, 128])
def test_multi_slab_removes_once(ops, oracle, _prepass_route, D):
    """sad_pass_groups = 1: the table goes through several candidate slabs, only the first slab's launch carries the role."""
    _prepass_route("sad_pass_groups", 1)
    p = Problem(D, 1000, 150, 131, seed=31)
    assert p.N > (512 if D == 64 else 256)               # more than one slab (D = 64: two, D = 128: four)
    f = segments(ops, random_lists(p, 4))
    check(rank(ops, p, f), want(oracle, p, f))


@pytest.mark.parametrize("D", [64, 128, 256])
def test_nan_in_an_unused_row_keeps_the_filter(ops, oracle, D):
    """A NaN in a table row no query uses as its fixed or true entity (it stays a candidate, and one list names it).  Whatever
    the pre-pass kernels make of the block -- down to standing aside for the exact sweep of every tile --, the role's
    workgroups must do their work: their branch comes before the pre-pass's off-switch."""
    p = Problem(D, 450, 100, 95, seed=41)
    p.table[449, 5] = float("nan")
    p.true_row = p.true_row % 449
    assert not torch.isnan(p.q_fixed).any()
    lists = random_lists(p, 5)
    lists[1] = list(lists[1]) + [449]
    f = segments(ops, [[r for r in l if r != int(p.true_row[q])] for q, l in enumerate(lists)])
    exp = want(oracle, p, f)
    assert (exp[:, :2] != exp[:, 2:]).any()
    check(rank(ops, p, f), exp)
    # and a table whose every value is non-finite-free but whose range is degenerate for the map: all rows one constant
    flat = Problem(D, 450, 100, 95, seed=42)
    flat.table[:] = 0.25
    flat.q_fixed[:] = 0.25
    flat.q_rel[:] = 0.0
    g = segments(ops, random_lists(flat, 6))
    exp = want(oracle, flat, g)
    assert (exp[:, 1] == flat.N).all() and (exp[:, 3] < exp[:, 1]).any()
    check(rank(ops, flat, g), exp, "degenerate range")


def test_workspace_reuse_with_another_filter(ops, oracle):
    """Two calls, one after the other, on the same workspace: the second's filter leaves empty what the first's filled."""
    p = Problem(128, 600, 140, 133, seed=51)
    nbytes = ops.rank_all_workspace_bytes("transe", p.N, p.D, p.q_head, p.Q - p.q_head)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    first = segments(ops, random_lists(p, 7, max_len=20, every=1000))
    lists = random_lists(p, 8)
    second = segments(ops, [l if q % 2 else [] for q, l in enumerate(lists)])
    check(rank(ops, p, first, ws=ws), want(oracle, p, first), "first")
    exp = want(oracle, p, second)
    assert np.array_equal(exp[::2, :2], exp[::2, 2:])
    check(rank(ops, p, second, ws=ws), exp, "second")
    check(rank(ops, p, None, ws=ws), want(oracle, p, None), "third, unfiltered")


@pytest.mark.parametrize("D,N,q_head,q_tail", SHAPES)
@pytest.mark.parametrize("fill", [0x00, 0xFF, 0xA5])
def test_workspace_bounds(ops, oracle, D, N, q_head, q_tail, fill):
    """The workspace at exactly rank_all_workspace_bytes(...) between two guards, everything pre-filled with one byte: the
    guards are intact after the call and the counts right whatever the workspace held."""
    p = Problem(D, N, q_head, q_tail, seed=61)
    nbytes = ops.rank_all_workspace_bytes("transe", N, D, q_head, q_tail)
    buf = torch.full((GUARD + nbytes + GUARD + 256,), fill, dtype=torch.uint8, device=DEV)
    off = GUARD + (-(buf.data_ptr() + GUARD)) % 256
    ws = buf[off:off + nbytes]
    f = segments(ops, random_lists(p, 9))
    got = rank(ops, p, f, ws=ws)
    torch.cuda.synchronize()
    assert bool((buf[:off] == fill).all()) and bool((buf[off + nbytes:] == fill).all())
    check(got, want(oracle, p, f))


def test_heavy_gate_keeps_removed(ops, oracle, _prepass_route):
    """Two clusters of near-duplicates (rows alternate between a vector and a copy moved by 1e-6: the fixed-point pre-pass can
    decide no pair) on the smallest block that arms the gate: Q N >= 2^27 pairs, five whole pre-pass groups of 512 rows at
    D = 64, 256 queries per workgroup.  Every workgroup's list runs full, the gate trips, fallback_prep zeroes the accumulators
    and the exact kernel re-ranks the block -- and what the role counted in `removed` must still be subtracted."""
    _prepass_route("sad_queries_per_group", 256)
    D, N, q_head, q_tail = 64, 2540, 26500, 26400
    assert (q_head + q_tail) * N >= 1 << 27 and (N + 63) // 64 % 8 == 0
    p = Problem(D, N, q_head, q_tail, seed=71)
    a = p.table[0].clone()
    b = a + 1e-6 * torch.sign(torch.randn(D, generator=torch.Generator().manual_seed(1)))
    p.table[0::2] = a
    p.table[1::2] = b
    p.q_fixed = p.table[torch.randint(0, N, (p.Q,), generator=torch.Generator().manual_seed(2))].clone()
    rng = np.random.default_rng(10)
    lists = [[] if q % 3 == 0 else [r for r in rng.integers(0, N, size=3).tolist() if r != int(p.true_row[q])] for q in range(p.Q)]
    lists = [sorted(set(l)) for l in lists]
    f = segments(ops, lists)
    ws = torch.empty(ops.rank_all_workspace_bytes("transe", N, D, q_head, q_tail), dtype=torch.uint8, device=DEV)
    got = rank(ops, p, f, ws=ws)
    stats = ops.prepass_stats("transe", N, D, q_head, q_tail, ws)
    n_blocks = ((N + 63) // 64 // 8) * ((p.Q + 255) // 256)
    assert stats["listed"] >= n_blocks * 1024 * 9 // 10, stats     # the gate's condition (rank_sad.hip: Gate)
    exp = want(oracle, p, f)
    assert (exp[:, 3] < exp[:, 1]).any() and len(np.unique(exp[:, 0])) > 1
    check(got, exp)
