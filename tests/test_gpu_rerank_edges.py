"""The re-ranking kernels at their numeric, tie and launch edges, on the device.  rerank_cosine: the correctly rounded square
root over 5 000 exact sums, degenerate rows (NaN, inf, overflow, the 1e-12f clamp from both sides, denormal products), the
row and CSR guards, empty segments, strided operands, the output's bounds.  rerank_ndcg: NaN / +-0 / denormal / infinite /
overflowing keys, segments that tie throughout, partial and clamped alpha blocks, every launch shape down to all padding,
the max_segment early exit beside valid segments, eight cutoffs, zero idcg, the output's bounds, and both calls replayed
from a captured graph.  The inputs are built by tests/test_rerank_host.py, which pins the restatements to plain references
on the host; every test first asserts there that its input reaches the case it is for."""
import numpy as np
import pytest
import torch

import test_rerank_host as host
from blp_amd import retrieval as R
from test_gpu_rerank import DEV, check_ndcg, cosine_problem, dev, ndcg_problem

pytestmark = pytest.mark.gpu
INT32_MIN = -2 ** 31


@pytest.fixture(scope="module")
def ops():
    from blp_amd import ops as _ops
    return _ops


def assert_f32_bits(got, want):
    """Bit-equal where the expectation is a number; NaN where it is NaN (sign and payload are not part of the contract)."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), np.argwhere(np.isnan(got) != nan)[:5]
    assert np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32)), np.argwhere(~nan & (got != want))[:5]


def assert_f64_bits(got, want):
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), np.argwhere(got != want)[:5]


def cosine(ops, table, queries, ptr, rows):
    return ops.rerank_cosine(dev(table), dev(queries), dev(ptr), dev(rows)).cpu().numpy()


# ------------------------------------------------------------------------------------------------ rerank_cosine
@pytest.mark.parametrize("scale", host.SWEEP_SCALES)
def test_cosine_square_root_sweep(ops, scale):
    table, queries, ptr, rows, sums, want = host.sqrt_sweep(scale)
    assert len(np.unique(sums)) >= 4000 and table.shape == (20000, 6)
    got = cosine(ops, table, queries, ptr, rows)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.argwhere(got != want)[:5]  # numpy f32 alone
    assert_f32_bits(got, R.cosine_restated(table, queries, ptr, rows))


@pytest.mark.parametrize("D", host.DEGENERATE_DIMS)
def test_cosine_degenerate_rows(ops, D):
    table, queries, ptr, rows, names = host.degenerate_cosine_problem(D)
    named, at, n = host.degenerate_rows(D), names.index, len(names)
    # the sides of the clamp, and the denormal products, as the host sees them
    v = {k: named[k][0] for k in ("hot_below", "hot_above")}
    assert np.sqrt(v["hot_below"] * v["hot_below"]) < host.CLAMP < np.sqrt(v["hot_above"] * v["hot_above"])
    assert np.linalg.norm(named["below"].astype(np.float64)) < 0.9995e-12
    assert np.linalg.norm(named["above"].astype(np.float64)) > 1.0005e-12
    prod = (named["u1e-32"] / host.CLAMP) * (named["w1e-32"] / host.CLAMP)
    assert prod.dtype == np.float32 and ((prod != 0) & (np.abs(prod) < host.F32_TINY)).any()
    want = R.cosine_restated(table, queries, ptr, rows)
    assert want.reshape(n, n + 1)[at("u1e-32"), at("w1e-32")] != 0
    got = cosine(ops, table, queries, ptr, rows)
    assert_f32_bits(got, want)
    got = got.reshape(n, n + 1)
    assert np.isnan(got[at("nan"), :n]).all() and np.isnan(got[:n, at("inf")]).all()
    r = v["hot_below"] / host.CLAMP  # by hand: a norm below 1e-12f divides by exactly 1e-12f
    assert got[at("hot"), at("hot_below")] == r == got[at("hot_below"), at("hot")] and got[at("hot_below"), at("hot_below")] == r * r
    assert got[at("hot"), at("hot_above")] == 1.0 == got[at("hot_at"), at("hot")]


def test_cosine_row_guards(ops):
    E = 50
    table, queries, ptr, rows = cosine_problem(E, 70, [9, 0, 14], seed=3, missing=0.0)
    bad = {2: E, 5: E + 5, 8: -2, 9: INT32_MIN, 22: 2 ** 31 - 1}
    want = R.cosine_restated(table, queries, ptr, rows)
    for c, row in bad.items():
        rows[c] = row
        want[c] = np.nan
    assert (np.delete(rows, list(bad)) >= 0).all() and not np.isnan(np.delete(want, list(bad))).any()
    got = cosine(ops, table, queries, ptr, rows)
    assert_f32_bits(got, want)  # the neighbours of a refused row are untouched


def test_cosine_csr_guards(ops):
    table, queries, ptr, rows = cosine_problem(50, 13, [6, 0, 7, 4], seed=4, missing=0.0)
    want = R.cosine_restated(table, queries, ptr, rows)
    C = len(rows)
    late = ptr.copy()
    late[0] = 2  # candidates 0 and 1 belong to no query
    assert (np.diff(late) >= 0).all()
    got = cosine(ops, table, queries, late, rows)
    assert_f32_bits(got, np.concatenate(([np.nan] * 2, want[2:])).astype(np.float32))
    short = ptr.copy()
    short[-1] = C - 3  # the last three candidates belong to no query
    assert (np.diff(short) >= 0).all() and short[-1] == 14
    got = cosine(ops, table, queries, short, rows)
    assert_f32_bits(got, np.concatenate((want[:C - 3], [np.nan] * 3)).astype(np.float32))
    rows[[0, C - 1]] = -1  # "no description" is decided before the CSR is looked at: 0.0
    both = late.copy()
    both[-1] = C - 3
    got = cosine(ops, table, queries, both, rows)
    assert got[0] == 0 and got[C - 1] == 0 and np.isnan(got[[1, C - 3, C - 2]]).all()
    assert_f32_bits(got[2:C - 3], want[2:C - 3])


@pytest.mark.parametrize("lengths", [[0, 0, 5, 0, 0, 1, 0], [9], [1], [0, 1], [1, 0], [0, 0, 0, 3]])
def test_cosine_empty_segments_and_single_candidates(ops, lengths):
    table, queries, ptr, rows = cosine_problem(20, 70, lengths, seed=len(lengths), missing=0.0)
    got = cosine(ops, table, queries, ptr, rows)
    assert_f32_bits(got, R.cosine_restated(table, queries, ptr, rows))
    # the binary search found the right query: each candidate against its own query in float64
    assert np.abs(got - host.plain_cosine_f64(table, queries, ptr, rows)).max() <= 1e-6


@pytest.mark.parametrize("D", [1, 65])
def test_cosine_strided_queries_and_table(ops, D):
    table, queries, ptr, rows = cosine_problem(30, D, [5, 0, 11, 3], seed=D)
    wide_t = torch.full((30, D + 3), 7.0, device=DEV)
    wide_q = torch.full((4, D + 28), -3.0, device=DEV)
    wide_t[:, :D] = dev(table)
    wide_q[:, :D] = dev(queries)
    t, q = wide_t[:, :D], wide_q[:, :D]
    assert q.stride(0) == D + 28 and t.stride(0) == D + 3 and (D <= 64 or D % 64 == 1)
    got = ops.rerank_cosine(t, q, dev(ptr), dev(rows)).cpu().numpy()
    assert_f32_bits(got, R.cosine_restated(table, queries, ptr, rows))


def test_cosine_output_bounds(ops):
    C, guard, sentinel = 101, 64, -7.0
    table, queries, ptr, rows = cosine_problem(40, 70, [50, 0, 51], seed=8)
    rows[[3, 77]], rows[10] = 40, -1  # a refused row and row -1 are written too
    assert C % 4 == 1 and len(rows) == C and (rows == -1).any()
    buf = torch.full((guard + C + guard,), sentinel, device=DEV)
    out = buf[guard:guard + C]
    assert ops.rerank_cosine(dev(table), dev(queries), dev(ptr), dev(rows), out=out) is out
    got = buf.cpu().numpy()
    assert (got[:guard] == sentinel).all() and (got[guard + C:] == sentinel).all()
    assert not (got[guard:guard + C] == sentinel).any()
    assert_f32_bits(got[guard:guard + C], R.cosine_restated(table, queries, ptr, rows))


# ------------------------------------------------------------------------------------------------ rerank_ndcg
def ndcg(ops, ptr, s1, s2, gain, alphas, cutoffs, idcg, max_segment=None, out=None):
    return ops.rerank_ndcg(dev(s1), dev(s2), dev(gain), dev(ptr), dev(alphas, torch.float64), cutoffs,
                           dev(R.log2_table(max(cutoffs))), dev(idcg, torch.float64), max_segment=max_segment, out=out)


def gains_idcg(ptr, gain, cutoffs):
    return np.array([host.plain_idcg(gain[ptr[q]:ptr[q + 1]], cutoffs) for q in range(len(ptr) - 1)]).reshape(len(ptr) - 1,
                                                                                                            len(cutoffs))


def run_ndcg(ops, ptr, s1, s2, gain, alphas, cutoffs, idcg=None, max_segment=None):
    """The device against the restatement, bit for bit, with ``max_segment`` passed as given; returns the device's result."""
    idcg = gains_idcg(ptr, gain, cutoffs) if idcg is None else idcg
    got = ndcg(ops, ptr, s1, s2, gain, alphas, cutoffs, idcg, max_segment).cpu().numpy()
    assert_f64_bits(got, R.trec_ndcg_cut(s1, s2, gain, ptr, alphas, cutoffs, R.log2_table(max(cutoffs)), idcg))
    return got


def test_ndcg_key_edges_alone_and_embedded(ops):
    f = host.edge_floats(0.5)
    s1, s2, gain = host.edge_segment()
    assert f[8] == f[9] and gain[8] != gain[9]                                       # the f32 tie
    assert f[1] == f[2] == 0 and np.signbit(f[1]) and not np.signbit(f[2])           # -0 before +0
    assert 0 < f[3] < f[4] < host.F32_TINY and gain[3] != gain[4]                    # denormal keys, the smaller first
    assert np.isnan(f[0]) and f[5] == f[11] == np.inf and f[6] == -np.inf and s2[11] > np.finfo(np.float32).max
    ptr = np.array([0, 12], np.int64)
    idcg = gains_idcg(ptr, gain, host.EDGE_CUTOFFS)
    got = run_ndcg(ops, ptr, s1, s2, gain, host.EDGE_ALPHAS, host.EDGE_CUTOFFS, idcg)
    assert_f64_bits(got, host.plain_ndcg_cut(s1, s2, gain, ptr, host.EDGE_ALPHAS, host.EDGE_CUTOFFS, idcg))
    assert not np.isnan(got).any()
    ptr, s1, s2, gain, q = host.embed_edge_segment()
    idcg = gains_idcg(ptr, gain, host.EDGE_CUTOFFS)
    both = run_ndcg(ops, ptr, s1, s2, gain, host.EDGE_ALPHAS, host.EDGE_CUTOFFS, idcg)
    assert_f64_bits(both, host.plain_ndcg_cut(s1, s2, gain, ptr, host.EDGE_ALPHAS, host.EDGE_CUTOFFS, idcg))
    assert_f64_bits(both[:, q], got[:, 0])


def test_ndcg_segments_that_tie_throughout(ops):
    ptr, s1, s2, gain = host.tie_segments()
    alphas = np.array([0.25, 0.5])
    for a in alphas:  # every key of a segment is the same float (or NaN)
        with np.errstate(invalid="ignore"):
            c = (a * s1.astype(np.float64) + (1 - a) * s2).astype(np.float32)
        assert np.isnan(c[ptr[0]:ptr[1]]).all() and (c[ptr[1]:ptr[2]] == np.inf).all()
        z = c[ptr[2]:ptr[3]]
        assert (z == 0).all() and 0 < np.signbit(z).sum() < len(z) and (c[ptr[3]:] == 0.5).all()
    assert ptr[4] - ptr[3] == 8192 and (gain[ptr[3] + 3:ptr[4] - 10] == 0).all()
    idcg = gains_idcg(ptr, gain, host.TIE_CUTOFFS)
    got = run_ndcg(ops, ptr, s1, s2, gain, alphas, host.TIE_CUTOFFS, idcg)
    assert_f64_bits(got, host.plain_ndcg_cut(s1, s2, gain, ptr, alphas, host.TIE_CUTOFFS, idcg))


def small_problem(Q, seed, longest=6):
    g = np.random.default_rng(seed)
    return ndcg_problem(g.integers(1, longest + 1, Q), seed=seed, quantum=0.5, n_rel=0.6)


@pytest.mark.parametrize("Q, A, apb, blocks, last", [(300, 7, 2, 4, 1), (2100, 3, 3, 1, 3), (40, 1, 1, 1, 1), (1, 101, 1, 101, 1),
                                                     (1100, 5, 3, 2, 2)])
def test_ndcg_alpha_blocks(ops, Q, A, apb, blocks, last):
    ptr, s1, s2, gain = small_problem(Q, seed=Q)
    shape = host.ndcg_launch_shape(A, Q, int(np.diff(ptr).max()))
    assert shape[3:] == (apb, blocks) and A - (blocks - 1) * apb == last
    if Q == 2100:
        assert (A * Q + 2047) // 2048 > A  # the clamp to A
    got = check_ndcg(ops, ptr, s1, s2, gain, np.linspace(0, 1, A), (1, 3, 10))
    assert got.shape == (A, Q, 3) and got.max() > 0


@pytest.mark.parametrize("longest, n_pad, per", [(100, 128, 2), (300, 512, 2), (64, 64, 1), (65, 128, 2)])
def test_ndcg_launch_shapes_never_launched_before(ops, longest, n_pad, per):
    ptr, s1, s2, gain = ndcg_problem([longest, 1, longest - 1, 0, longest // 2], seed=longest, quantum=0.5)
    assert np.diff(ptr).max() == longest and host.ndcg_launch_shape(4, 5, longest)[:3] == (n_pad, max(64, n_pad // 2), per)
    alphas = np.array([0.0, 0.3, 0.5, 1.0])
    check_ndcg(ops, ptr, s1, s2, gain, alphas, (1, 5, 10, 100, 1000))                 # max_segment read from cand_ptr
    run_ndcg(ops, ptr, s1, s2, gain, alphas, (1, 5, 10, 100, 1000), max_segment=longest)  # ... and passed explicitly


@pytest.mark.parametrize("max_segment, n_pad, T, per", [(8192, 8192, 1024, 8), (4096, 4096, 1024, 4), (1000, 1024, 512, 2),
                                                        (64, 64, 64, 1), (10, 64, 64, 1)])
def test_ndcg_almost_all_padding(ops, max_segment, n_pad, T, per):
    ptr, s1, s2, gain = ndcg_problem([10, 0, 3, 1, 7, 10, 2], seed=2, quantum=0.5, n_rel=0.6)
    assert np.diff(ptr).max() == 10 and host.ndcg_launch_shape(3, 7, max_segment)[:3] == (n_pad, T, per)
    got = run_ndcg(ops, ptr, s1, s2, gain, np.array([0.0, 0.5, 1.0]), (1, 3, 10, 20), max_segment=max_segment)
    assert got.max() > 0


def test_ndcg_all_segments_empty(ops):
    ptr = np.zeros(6, np.int64)
    empty = np.zeros(0)
    assert host.ndcg_launch_shape(3, 5, 0)[:3] == (64, 64, 1)
    got = ndcg(ops, ptr, empty.astype(np.float32), empty, empty.astype(np.int32), np.array([0.0, 0.5, 1.0]), (10, 100),
               np.ones((5, 2)), max_segment=0).cpu().numpy()
    assert got.shape == (3, 5, 2) and (got == 0).all() and not np.signbit(got).any()


def test_ndcg_segment_longer_than_max_segment(ops):
    lengths = [10, 65, 64, 200, 0]
    ptr, s1, s2, gain = ndcg_problem(lengths, seed=6, quantum=0.5, n_rel=0.5)
    alphas, cutoffs = np.array([0.0, 0.4, 1.0]), (5, 64, 100)
    idcg = gains_idcg(ptr, gain, cutoffs)
    assert host.ndcg_launch_shape(3, 5, 64)[0] == 64 and [n > 64 for n in lengths] == [False, True, False, True, False]
    got = ndcg(ops, ptr, s1, s2, gain, alphas, cutoffs, idcg, max_segment=64).cpu().numpy()
    assert np.isnan(got[:, [1, 3]]).all()
    keep = [0, 2, 4]  # ... and the restatement of those segments alone
    pieces = [np.arange(ptr[q], ptr[q + 1]) for q in keep]
    sel = np.concatenate(pieces)
    alone = np.concatenate(([0], np.cumsum([len(p) for p in pieces]))).astype(np.int64)
    want = R.trec_ndcg_cut(s1[sel], s2[sel], gain[sel], alone, alphas, cutoffs, R.log2_table(100), idcg[keep])
    assert_f64_bits(got[:, keep], want)
    assert want[:, :2].max() > 0


def test_ndcg_segment_past_the_end_of_the_candidates(ops):
    ptr, s1, s2, gain = ndcg_problem([10, 30, 0, 20], seed=7, quantum=0.5, n_rel=0.5)
    alphas, cutoffs = np.array([0.0, 0.4, 1.0]), (5, 100)
    idcg = gains_idcg(ptr, gain, cutoffs)
    want = R.trec_ndcg_cut(s1, s2, gain, ptr, alphas, cutoffs, R.log2_table(100), idcg)
    C = len(s1)
    over = ptr.copy()
    over[-1] = C + 4  # monotone, within max_segment, but 4 past s1 / s2 / gain: nothing of the segment is read
    assert over[-1] - over[-2] == 24 and (np.diff(over) >= 0).all()
    got = ndcg(ops, over, s1, s2, gain, alphas, cutoffs, idcg, max_segment=30).cpu().numpy()
    assert np.isnan(got[:, 3]).all()
    assert_f64_bits(got[:, :3], want[:, :3])


def test_ndcg_eight_cutoffs_at_and_around_the_segment_lengths(ops):
    cutoffs = (1, 2, 3, 5, 64, 65, 1000, 8192)
    assert len(cutoffs) == 8  # BLP_RERANK_MAX_CUTOFFS
    ptr, s1, s2, gain = ndcg_problem([64, 65, 3, 1], seed=9, quantum=0.5, n_rel=0.7)
    gain[:] = 1 + np.arange(len(gain)) % 3  # every rank counts, the last one of each segment too
    assert np.diff(ptr).tolist() == [64, 65, 3, 1]  # cutoffs equal to n (64, 65, 3, 1), to n + 1 (65, 2) and above n
    alphas = np.array([0.0, 0.5, 1.0])
    check_ndcg(ops, ptr, s1, s2, gain, alphas, cutoffs)
    idcg = gains_idcg(ptr, gain, cutoffs)
    got = run_ndcg(ops, ptr, s1, s2, gain, alphas, cutoffs, idcg)
    assert_f64_bits(got, host.plain_ndcg_cut(s1, s2, gain, ptr, alphas, cutoffs, idcg))
    assert (got[:, 0, 4] == got[:, 0, 7]).all() and (got[:, :, 7] == got[:, :, 6]).all()


@pytest.mark.parametrize("cutoffs", [(10,), (1,), (500, 1000), (8192,)])
def test_ndcg_single_cutoff_and_cutoffs_above_every_segment(ops, cutoffs):
    ptr, s1, s2, gain = ndcg_problem([64, 65, 3, 1, 0, 130], seed=10, quantum=0.5, n_rel=0.5)
    assert cutoffs[0] in (1, 10) or cutoffs[0] > np.diff(ptr).max()
    check_ndcg(ops, ptr, s1, s2, gain, np.array([0.0, 0.5, 1.0]), cutoffs)


def test_ndcg_zero_idcg_and_no_positive_gain(ops):
    ptr, s1, s2, gain = ndcg_problem([20, 20, 20], seed=12, quantum=0.5, n_rel=0.5)
    gain[ptr[1]:ptr[2]] = -np.abs(gain[ptr[1]:ptr[2]])  # segment 1: every gain <= 0
    cutoffs = (5, 100)
    idcg = gains_idcg(ptr, gain, cutoffs)
    idcg[0] = 0.0  # segment 0: positive gains retrieved, the qrels' ideal is 0
    assert (gain[ptr[0]:ptr[1]] > 0).any() and (gain[ptr[1]:ptr[2]] <= 0).all() and (gain[ptr[1]:ptr[2]] < 0).any()
    assert (idcg[1] == 0).all() and (idcg[2] > 0).all()
    got = run_ndcg(ops, ptr, s1, s2, gain, np.array([0.0, 0.5, 1.0]), cutoffs, idcg)
    assert (got[:, :2] == 0).all() and not np.signbit(got[:, :2]).any() and (got[:, 2, 1] > 0).all()
    idcg[1] = 1.0  # a positive ideal: the DCG itself is 0
    got = run_ndcg(ops, ptr, s1, s2, gain, np.array([0.0, 0.5, 1.0]), cutoffs, idcg)
    assert (got[:, 1] == 0).all()


@pytest.mark.parametrize("max_segment", [64, 8])
def test_ndcg_output_bounds(ops, max_segment):
    """out between two guards of 64 doubles.  The last alpha block is partial (one alpha of two), and one alpha's rows,
    Q * n_cut = 63 doubles, fit in a guard: an alpha written past A lands in it."""
    Q, A, cutoffs, guard, sentinel = 21, 101, (1, 5, 10), 64, -7.0
    ptr, s1, s2, gain = small_problem(Q, seed=13, longest=12)
    n_pad, T, per, apb, blocks = host.ndcg_launch_shape(A, Q, max_segment)
    assert (T, apb, blocks) == (64, 2, 51) and A - (blocks - 1) * apb == 1 and Q * len(cutoffs) <= guard
    long = np.diff(ptr) > max_segment
    assert long.any() == (max_segment == 8) and not long.all()
    alphas = np.linspace(0, 1, A)
    idcg = gains_idcg(ptr, gain, cutoffs)
    n = A * Q * len(cutoffs)
    buf = torch.full((guard + n + guard,), sentinel, dtype=torch.float64, device=DEV)
    out = buf[guard:guard + n].view(A, Q, len(cutoffs))
    assert ndcg(ops, ptr, s1, s2, gain, alphas, cutoffs, idcg, max_segment=max_segment, out=out) is out
    got = buf.cpu().numpy()
    assert (got[:guard] == sentinel).all() and (got[guard + n:] == sentinel).all()
    mid = got[guard:guard + n].reshape(A, Q, len(cutoffs))
    assert not (mid == sentinel).any()
    assert np.isnan(mid[:, long]).all()
    want = R.trec_ndcg_cut(s1, s2, gain, ptr, alphas, cutoffs, R.log2_table(10), idcg)
    assert_f64_bits(mid[:, ~long], want[:, ~long])


def test_both_calls_replay_from_a_captured_graph(ops):
    """Asynchronous on the caller's stream, no host read (max_segment is given), no allocation: rerank_cosine followed by
    rerank_ndcg, captured once as one chain, gives the results of the buffers' new contents on each replay."""
    E, D, lengths, cutoffs = 200, 70, [40, 0, 64, 7], (5, 100)
    alphas = np.linspace(0, 1, 5)

    def make(seed):
        table, queries, ptr, rows = cosine_problem(E, D, lengths, seed=seed)
        _, _, s2, gain = ndcg_problem(lengths, seed=seed, quantum=0.5, n_rel=0.5)
        return dict(table=table, queries=queries, rows=rows, s2=s2, gain=gain, idcg=gains_idcg(ptr, gain, cutoffs)), ptr

    first, ptr = make(20)
    bufs = {k: dev(v) for k, v in first.items()}
    ptr_d, alphas_d, log2_d = dev(ptr), dev(alphas, torch.float64), dev(R.log2_table(100))
    s1 = torch.empty(len(first["rows"]), dtype=torch.float32, device=DEV)
    out = torch.empty((5, 4, 2), dtype=torch.float64, device=DEV)

    def call():
        ops.rerank_cosine(bufs["table"], bufs["queries"], ptr_d, bufs["rows"], out=s1)
        ops.rerank_ndcg(s1, bufs["s2"], bufs["gain"], ptr_d, alphas_d, cutoffs, log2_d, bufs["idcg"], max_segment=64, out=out)

    call()  # lazy initialisation outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for seed in (21, 22):
        new, _ = make(seed)
        for k, v in new.items():
            bufs[k].copy_(dev(v))
        s1.fill_(-5.0)
        out.fill_(-5.0)
        graph.replay()
        torch.cuda.synchronize()
        want_s1 = R.cosine_restated(new["table"], new["queries"], ptr, new["rows"])
        assert_f32_bits(s1.cpu().numpy(), want_s1)
        assert_f64_bits(out.cpu().numpy(),
                        R.trec_ndcg_cut(want_s1, new["s2"], new["gain"], ptr, alphas, cutoffs, R.log2_table(100), new["idcg"]))
