"""The glue kernels on the device, each against the restatement of its contract in tests/test_glue_edges_host.py (which builds the
cases, asserts that each reaches its edge, and pins every restatement to an independent source): topk_merge_kernel (topk.hip,
topk_lists.h), rank_from_scores_kernel (rank_dense.hip), rank_metrics_kernel / rank_metric_sums_kernel (rank_all.hip),
build_queries_kernel and gather_triple_vectors_kernel (queries.hip).  The shipped dispatch, the product library, no knobs.
Integers are compared with torch.equal / array_equal, floats as their bit patterns; the one tolerance -- the f64 sum of Q
non-negative reciprocal ranks -- is the bound of recursive summation in any order, Q x 2^-53 x the exact sum (math.fsum).

What a subtly wrong kernel would trip, argued from the code (nothing here breaks a kernel on purpose):
1. topk_key / key_row dropping the key's low bit: the `zeros` case wants the sign of every zero back with its row.
2. a NaN key whose high word is 0: NaN at row 2^31 - 1 becomes key 0, an empty slot (`extremes`, queries 2 and 3).
3. a slip of list_insert at a 64-slot boundary, or in the tie-break: every geometry case has ties in every chunk and k on both
   sides of 64, 128 and 256; `ties` cuts a 661-entry tie block by row in three input orders.  (`prev > x` written `prev >= x`
   is no slip: the two differ only where prev == x, and there both pick the same key.)
4. the merge's strided loop: n_in on both sides of every wave count (1, 2, 4, 15, 16 waves), a last trip of one entry
   (12 289), n_in < k (padding), the fetch past n_in.  The RESULT does not depend on the number of waves -- that is the
   kernel's contract -- so a launch with another wave count is not a wrong result and no test here can tell it.
5. `s >= t` as `s > t`, signed zeros, NaN on either side, +-Inf, a filter that lists the true column or every column.
6. best + worst in 32 bits or rounded separately; `avg <= k` as `avg < k`; a sum that drops the queries after
   blocks x floor(Q / blocks) (the last 64 queries rank first, so the hit counts move).
7. query_at's short last block, by_position positions, a bad id's substitutes, the 128-float sweep at D = 124 / 132 / 300 /
   1024, `row - row_base` at both ends of a shard, 16-bit rows with every special pattern.
"""
import numpy as np
import pytest
import torch

import test_glue_edges_host as host

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _no_knob_left():
    from blp_amd import _lib
    _lib.reset_knobs()
    yield
    _lib.reset_knobs()


def dev(x):
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(DEV)


def bits_of(t):
    """A float32 device tensor's bit patterns as uint32 numpy."""
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def strided(t, pad, poison=1.0):
    """``t`` (CPU, 2-D) on the device as a column slice of a tensor ``pad`` elements wider, moved as integers (every bit
    pattern survives); the columns past the slice hold ``poison``."""
    ints = {4: torch.int32, 2: torch.int16}[t.element_size()]
    buf = torch.full((t.shape[0], t.shape[1] + pad), poison, dtype=t.dtype).view(ints).to(DEV)
    buf[:, :t.shape[1]].copy_(t.contiguous().view(ints).to(DEV))
    view = buf.view(t.dtype)[:, :t.shape[1]]
    assert view.stride(0) == t.shape[1] + pad
    return view


# ================================================================================================ merge
def raw_merge(rows, scores, k):
    """blp_topk_merge itself with lists x k_in = n_in (lists > 1 wherever n_in > 1)."""
    from blp_amd import _lib
    Q, n = rows.shape
    lists, k_in = host.merge_split(n)
    rows_out = torch.full((Q, k), 5, dtype=torch.int64, device=DEV)
    scores_out = torch.full((Q, k), 1.0, dtype=torch.float32, device=DEV)
    status = _lib.lib().blp_topk_merge(rows.data_ptr(), scores.data_ptr(), Q, lists, k_in, k, rows_out.data_ptr(), scores_out.data_ptr(),
                                       rows.device.index, torch.cuda.current_stream().cuda_stream)
    _lib.check(status, "blp_topk_merge")
    return rows_out, scores_out


def check_merge(ops, rows, scores, k, what):
    want_rows, want_bits = host.merge_expected(rows, scores, k)
    r, s = dev(rows), dev(scores)
    assert np.array_equal(bits_of(s), np.ascontiguousarray(scores).view(np.uint32))      # the inputs arrived bit for bit
    first = None
    for name, call in (("ops", lambda: ops.topk_merge(r, s, k)), ("raw", lambda: raw_merge(r, s, k)), ("again", lambda: ops.topk_merge(r, s, k))):
        got_rows, got_scores = call()
        got_rows, got_bits = got_rows.cpu().numpy(), bits_of(got_scores)
        assert got_rows.dtype == np.int64 and got_rows.shape == want_rows.shape
        bad = np.nonzero((got_rows != want_rows) | (got_bits != want_bits))
        assert bad[0].size == 0, (what, name, k, [(int(q), int(i), int(got_rows[q, i]), int(want_rows[q, i]), hex(got_bits[q, i]),
                                                   hex(want_bits[q, i])) for q, i in zip(bad[0][:4], bad[1][:4])])
        first = first or (got_rows, got_bits)
    assert np.array_equal(first[0], got_rows) and np.array_equal(first[1], got_bits)     # the same call twice: bit-equal


@pytest.mark.parametrize("n_in", host.MERGE_N_IN)
def test_merge_geometry(ops, n_in):
    """k across list_insert's 64-slot boundaries x n_in across the wave counts of launch_merge, Q = 1 and 5; n_in < k pads."""
    for Q in host.MERGE_Q:
        rows, scores = host.merge_geometry_case(n_in, Q)
        for k in host.MERGE_K:
            check_merge(ops, rows, scores, k, ("geometry", n_in, Q))


@pytest.mark.parametrize("k", [1, 3, 64, 65, 256])
@pytest.mark.parametrize("name", host.MERGE_ORDER_CASES)
def test_merge_order(ops, name, k):
    """The order contract of the header: ties by row, the sign of zero, NaN payloads, +-Inf, subnormals, empty slots, rows 0 and
    2^31 - 1 (test_glue_edges_host.merge_order_case)."""
    rows, scores = host.merge_order_case(name, k)
    check_merge(ops, rows, scores, k, name)
    if name == "specials":                    # fewer entries than slots: the whole order is visible, then the padding
        check_merge(ops, rows[:, :100], scores[:, :100], 256, name)


@pytest.mark.parametrize("k", [1, 65, 256])
def test_merge_aliased_on_an_empty_table(ops, k):
    """blp_topk on an empty table slice runs the merge kernel with rows_out == rows and no entries: every slot -1 / NaN."""
    g = torch.Generator().manual_seed(k)
    table = torch.randn(8, 64, generator=g).to(DEV)
    rel_emb = torch.randn(3, 64, generator=g).to(DEV)
    fixed_row, rel_ids = torch.tensor([0, 7, 3, 1, 2], device=DEV), torch.tensor([0, 2, 1, 1, 0], device=DEV)
    out = (torch.full((5, k), 5, dtype=torch.int64, device=DEV), torch.full((5, k), 1.0, dtype=torch.float32, device=DEV))
    rows, scores = ops.topk("distmult", table[:0], table, fixed_row, rel_emb, rel_ids, 2, k, out=out)
    assert (rows.cpu() == -1).all() and (bits_of(scores) == host.QNAN).all()


# ================================================================================================ dense counts
def check_counts(got, want, what):
    got = got.cpu()
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.numpy(), want), (what, got.numpy()[(got.numpy() != want).any(1)][:4], want[(got.numpy() != want).any(1)][:4])


@pytest.mark.parametrize("kind", host.DENSE_KINDS)
def test_dense_counts(ops, kind):
    """rank_from_scores_kernel at Q around its four queries per workgroup and N around its 64 columns per trip: true_idx and
    true_score, a packed matrix, a column slice of a wider one (ld > N) and a transposed one, the CSR of the case.  (Columns
    outside [0, N): test_gpu_filter_edges.py, route g.)"""
    nan_counts = []
    for Q in host.DENSE_Q:
        for N in host.DENSE_N:
            c = host.dense_case(kind, Q, N)
            true = c.scores[np.arange(Q), c.true_idx]
            want_raw = host.dense_counts_expected(c.scores, true)
            want = host.dense_counts_expected(c.scores, true, c.rowptr, c.col)
            assert np.array_equal(want_raw[:, :2], want[:, :2]) and np.array_equal(want_raw[:, 2:], want_raw[:, :2])
            packed = dev(c.scores)
            sliced = strided(torch.from_numpy(c.scores), 5, poison=float("inf"))
            transposed = dev(np.ascontiguousarray(c.scores.T)).T
            assert transposed.stride(1) != 1 or Q == 1 or N == 1
            idx, score, rowptr, col = dev(c.true_idx), dev(true), dev(c.rowptr), dev(c.col)
            for name, m in (("packed", packed), ("sliced", sliced), ("transposed", transposed)):
                assert np.array_equal(bits_of(m), c.scores.view(np.uint32))
                check_counts(ops.rank_from_scores(m, true_idx=idx), want_raw, (kind, Q, N, name, "idx"))
                check_counts(ops.rank_from_scores(m, true_score=score), want_raw, (kind, Q, N, name, "score"))
                check_counts(ops.rank_from_scores(m, true_idx=idx, filt_rowptr=rowptr, filt_col=col), want, (kind, Q, N, name, "idx+csr"))
                got = ops.rank_from_scores(m, true_score=score, filt_rowptr=rowptr, filt_col=col)
                check_counts(got, want, (kind, Q, N, name, "score+csr"))
            nan_counts.append(got)
    if kind == "true_nan":                    # the worst rank below the best one, on to the metrics
        counts = torch.cat(nan_counts)
        assert not counts.any()
        for k_values in host.K_VALUE_SETS:
            rr, hits = ops.rank_metrics(counts, k_values)
            want_rr, want_hits = host.metrics_expected(counts.cpu().numpy(), k_values)
            assert (bits_of(rr) == np.float32(2.0).view(np.uint32)).all() and hits.all()
            assert np.array_equal(bits_of(rr), want_rr.view(np.uint32)) and np.array_equal(hits.cpu().numpy(), want_hits)


def test_dense_counts_no_queries(ops):
    got = ops.rank_from_scores(torch.empty((0, 65), device=DEV), true_idx=torch.empty(0, dtype=torch.int64, device=DEV))
    assert got.shape == (0, 4) and got.dtype == torch.int32


# ================================================================================================ metrics
@pytest.mark.parametrize("Q", sorted(set(host.METRICS_Q + host.SUMS_Q)))
def test_metrics_and_sums(ops, Q):
    """rank_metrics_kernel bit for bit and rank_metric_sums_kernel -- hit counts exactly, reciprocal-rank sums within the
    summation bound -- on counts at every edge of metric_edge_pairs, at Q around both kernels' partitions."""
    for k_values in host.K_VALUE_SETS:
        counts_np = host.metric_counts(Q, k_values)
        counts = dev(counts_np)
        want_rr, want_hits = host.metrics_expected(counts_np, k_values)
        rr, hits = ops.rank_metrics(counts, k_values)
        assert rr.shape == (Q, 2) and hits.shape == (Q, 2, 3) and hits.dtype == torch.bool
        bad = np.nonzero(bits_of(rr) != want_rr.view(np.uint32))[0]
        assert bad.size == 0, (Q, k_values, counts_np[bad[:4]], rr.cpu().numpy()[bad[:4]], want_rr[bad[:4]])
        assert np.array_equal(hits.cpu().numpy(), want_hits), (Q, k_values)
        rr2, hits2 = ops.rank_metrics(counts, k_values)
        assert torch.equal(rr2.view(torch.int32), rr.view(torch.int32)) and torch.equal(hits2, hits)

        exact, hit_sums = host.metric_sums_expected(counts_np, k_values)
        sums = ops.rank_metric_sums(counts, k_values)
        assert sums.dtype == torch.float64 and sums.shape == (8,)
        got = sums.cpu().tolist()
        assert got[2:] == [float(h) for h in hit_sums.tolist()], (Q, k_values, got[2:], hit_sums.tolist())
        for v in (0, 1):
            bound = Q * 2.0 ** -53 * exact[v]
            print(f"Q={Q} k={k_values} v={v}: sum {got[v]!r} exact {exact[v]!r} |diff| {abs(got[v] - exact[v]):.3e} bound {bound:.3e}")
            assert abs(got[v] - exact[v]) <= bound, (Q, k_values, v, got[v], exact[v], bound)
        assert torch.equal(ops.rank_metric_sums(counts, k_values).view(torch.int64), sums.view(torch.int64))


# ================================================================================================ prelude
def check_prelude(qb, want, what, vectors, with_index):
    assert int(qb.ids_min) == want.ids_min, what
    for name in ("fixed_row", "true_row", "rel_ids"):
        got = getattr(qb, name).cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, getattr(want, name)), (what, name, got, getattr(want, name))
    if vectors:
        for name in ("q_fixed", "q_rel"):
            got = getattr(qb, name)
            assert got.shape == getattr(want, name).shape and got.is_contiguous()
            bad = np.nonzero((bits_of(got) != getattr(want, name).view(np.uint32)).any(1))[0] if got.numel() else np.empty(0)
            assert bad.size == 0, (what, name, bad[:8])
    else:
        assert qb.q_fixed is None and qb.q_rel is None
    if with_index:
        for name in ("seg_lo", "seg_hi", "exclude"):
            got = getattr(qb.filter, name).cpu().numpy()
            assert np.array_equal(got, getattr(want, name)), (what, name, got, getattr(want, name))
    else:
        assert qb.filter is None


@pytest.mark.parametrize("D", host.PRELUDE_D)
def test_prelude_shapes(ops, D):
    """build_queries_kernel at n around its eight queries per workgroup, every block size that moves the short last block, D
    around the 128-float sweep: the vector form, the index form and by_position, ent2idx given and None, a strided source."""
    w = host.world(D)
    index = host.index_arrays(w.index)
    table_np = w.table.contiguous().numpy()
    table, rel_emb = strided(w.table.contiguous(), host.PAD), dev(w.rel_emb)
    for n in host.PRELUDE_N:
        for mapped in (True, False):
            triples = host.prelude_triples(w, n, mapped)
            e_np, e_dev = (w.ent2idx.numpy(), dev(w.ent2idx)) if mapped else (None, None)
            source_np = host.gather_expected(triples.numpy(), e_np, w.table)
            source = strided(torch.from_numpy(source_np), host.PAD)
            for block in host.prelude_blocks(n):
                what = (D, n, mapped, block)
                want = host.prelude_expected(triples.numpy(), e_np, host.NUM_ROWS, host.NUM_RELS, block, False, table_np, w.rel_emb.numpy(), index)
                assert want.ids_min == 0
                qb = ops.build_queries(dev(triples), e_dev, table, rel_emb, block, index=w.index)
                check_prelude(qb, want, what + ("vectors",), True, True)
                qb = ops.build_queries(dev(triples), e_dev, table, rel_emb, block, index=w.index, gather=False)
                check_prelude(qb, want, what + ("index form",), False, True)
                qb = ops.build_queries(dev(triples), e_dev, table, rel_emb, block)
                check_prelude(qb, want._replace(seg_lo=None), what + ("no index",), True, False)
                want = host.prelude_expected(triples.numpy(), e_np, host.NUM_ROWS, host.NUM_RELS, block, True, source_np, w.rel_emb.numpy(), index)
                qb = ops.build_queries(dev(triples), e_dev, source, rel_emb, block, index=w.index, by_position=True, num_rows=host.NUM_ROWS)
                check_prelude(qb, want, what + ("by_position",), True, True)
                qb = ops.build_queries(dev(triples), e_dev, source, rel_emb, block, gather=False, by_position=True, num_rows=host.NUM_ROWS)
                check_prelude(qb, want._replace(seg_lo=None), what + ("by_position, index form",), False, False)


@pytest.mark.parametrize("kind,where", host.bad_id_cases())
def test_prelude_bad_ids(ops, kind, where):
    """One bad id on the head, the tail or the relation of one triple: ids_min = -1, row / relation 0 and a zero vector for
    the bad operand only, every other query as the restatement has it; the next call with good ids reports 0 again."""
    D, n, block = 132, 9, 3
    w = host.world(D)
    triples, ent2idx = host.bad_id_case(w, kind, where, n)
    good = host.prelude_triples(w, n, True)
    table_np = w.table.contiguous().numpy()
    table, rel_emb = strided(w.table.contiguous(), host.PAD), dev(w.rel_emb)
    index = host.index_arrays(w.index)
    for by_position in (False, True):
        source_np = host.gather_expected(triples.numpy(), ent2idx.numpy(), w.table) if by_position else table_np
        source = strided(torch.from_numpy(source_np), host.PAD) if by_position else table
        want = host.prelude_expected(triples.numpy(), ent2idx.numpy(), host.NUM_ROWS, host.NUM_RELS, block, by_position, source_np,
                                     w.rel_emb.numpy(), index)
        assert want.ids_min == -1
        kw = dict(by_position=True, num_rows=host.NUM_ROWS) if by_position else {}
        qb = ops.build_queries(dev(triples), dev(ent2idx), source, rel_emb, block, index=w.index, **kw)
        check_prelude(qb, want, (kind, where, by_position), True, True)
        qb = ops.build_queries(dev(triples), dev(ent2idx), source, rel_emb, block, gather=False, **kw)
        check_prelude(qb, want._replace(seg_lo=None), (kind, where, by_position, "index form"), False, False)
        good_np = host.gather_expected(good.numpy(), w.ent2idx.numpy(), w.table) if by_position else table_np
        good_source = strided(torch.from_numpy(good_np), host.PAD) if by_position else table
        ref = host.prelude_expected(good.numpy(), w.ent2idx.numpy(), host.NUM_ROWS, host.NUM_RELS, block, by_position, good_np,
                                    w.rel_emb.numpy(), index)
        qb = ops.build_queries(dev(good), dev(w.ent2idx), good_source, rel_emb, block, index=w.index, **kw)
        assert int(qb.ids_min) == 0
        check_prelude(qb, ref, (kind, where, by_position, "good again"), True, True)


def test_prelude_segments(ops):
    """The filter segments at the edges of the index (test_glue_edges_host.segment_case)."""
    w = host.world(4)
    triples, _ = host.segment_case(w)
    table, rel_emb = strided(w.table.contiguous(), host.PAD), dev(w.rel_emb)
    for block in (1, 3, triples.shape[0], 1 << 20):
        want = host.prelude_expected(triples.numpy(), w.ent2idx.numpy(), host.NUM_ROWS, host.NUM_RELS, block, False,
                                     w.table.contiguous().numpy(), w.rel_emb.numpy(), host.index_arrays(w.index))
        qb = ops.build_queries(dev(triples), dev(w.ent2idx), table, rel_emb, block, index=w.index)
        check_prelude(qb, want, ("segments", block), True, True)
        assert torch.equal(qb.filter.values.cpu(), w.index.device_arrays("cpu")[2])


# ================================================================================================ gather
GATHER_ROWS = 11
SHARDS = ((0, 4), (4, 9), (9, GATHER_ROWS))


def gather_ids():
    """ids 1 .. 11 map to rows 10 .. 0; triples name every row as a head and as a tail, an unmapped id, -1 and an id past
    the map: every shard sees rows below it, its first and last row and the row one past it."""
    ent2idx = torch.full((16,), -1, dtype=torch.long)
    ent2idx[1:GATHER_ROWS + 1] = torch.arange(GATHER_ROWS - 1, -1, -1)
    heads = torch.tensor(list(range(1, GATHER_ROWS + 1)) + [0, -1, 16])
    triples = torch.stack((heads, heads.flip(0), torch.zeros_like(heads)), dim=1)
    return ent2idx, triples


def check_gather(ops, triples, ent2idx, table_cpu, table_dev, what):
    full = None
    for lo, hi in ((0, table_cpu.shape[0]),) + SHARDS:
        want = host.gather_expected(triples.numpy(), None if ent2idx is None else ent2idx.numpy(), table_cpu[lo:hi], lo)
        got = ops.gather_triple_vectors(dev(triples), dev(ent2idx), table_dev[lo:hi], row_base=lo)
        assert got.dtype == torch.float32 and got.shape == want.shape and got.is_contiguous()
        bad = np.nonzero((bits_of(got) != want.view(np.uint32)).any(1))[0]
        assert bad.size == 0, (what, lo, hi, bad[:8])
        if full is None:
            full = want
            assert (np.isnan(want).any() or (want != 0).any()) and not want[len(triples) - 2].any()
        else:
            assert 0 < (want.view(np.uint32) != 0).any(1).sum() < (full.view(np.uint32) != 0).any(1).sum()


@pytest.mark.parametrize("D", host.GATHER_D)
@pytest.mark.parametrize("dtype", host.GATHER_DTYPES, ids=str)
def test_gather_special_patterns(ops, dtype, D):
    """Rows of NaN payloads, +-Inf, +-0, subnormals and the largest finite value, strided, whole and in three shards, through
    ent2idx and with ids as rows: bit-equal to Tensor.float() of the row, zeros outside the shard."""
    table = host.special_table(dtype, GATHER_ROWS, D)
    table_dev = strided(table, 8)
    assert table_dev.stride(0) % 8 == 0
    ent2idx, triples = gather_ids()
    check_gather(ops, triples, ent2idx, table, table_dev, (dtype, D, "ent2idx"))
    rows = torch.tensor(list(range(GATHER_ROWS)) + [GATHER_ROWS, -1, 1 << 40])          # ids are rows: one past the table, -1
    as_rows = torch.stack((rows, rows.flip(0), torch.zeros_like(rows)), dim=1)
    check_gather(ops, as_rows, None, table, table_dev, (dtype, D, "ids are rows"))


@pytest.mark.parametrize("dtype", host.GATHER_DTYPES, ids=str)
def test_gather_shards_sum_to_the_whole(ops, dtype):
    """The candidate shards' outputs add up to the unsharded gather bit for bit (x + 0 = x; on a table of finite non-zero
    values: -0 + 0 is +0 and a sum quiets a signalling NaN, which is why the special patterns are checked shard by shard)."""
    for D in host.GATHER_D:
        w = host.world(D, dtype)
        table_dev = strided(w.table, 8)
        g = torch.Generator().manual_seed(D)
        triples = torch.cat((w.entities[torch.randint(0, host.NUM_ROWS, (33, 2), generator=g)], torch.zeros(33, 1, dtype=torch.long)), dim=1)
        triples[0, 0], triples[0, 1] = w.entities[0], w.entities[host.NUM_ROWS - 1]
        want = host.gather_expected(triples.numpy(), w.ent2idx.numpy(), w.table)
        assert (want != 0).all()
        full = ops.gather_triple_vectors(dev(triples), dev(w.ent2idx), table_dev)
        assert np.array_equal(bits_of(full), want.view(np.uint32))
        parts = [ops.gather_triple_vectors(dev(triples), dev(w.ent2idx), table_dev[lo:hi], row_base=lo)
                 for lo, hi in ((0, 7), (7, 8), (8, host.NUM_ROWS))]
        assert all((p == 0).all(1).any() for p in parts)
        assert torch.equal(torch.stack(parts).sum(0).view(torch.int32), full.view(torch.int32))


def test_gather_no_triples(ops):
    table = torch.randn(5, 8).to(DEV)
    got = ops.gather_triple_vectors(torch.empty((0, 3), dtype=torch.long, device=DEV), None, table)
    assert got.shape == (0, 8) and got.dtype == torch.float32
