"""Per-query candidate lists for DistMult / ComplEx / SimplE at any width on the MI355X (blp_rank_lists_wide through
blp_amd.ops.rank_lists_wide and ranking.rank_candidates): counts EQUAL and scores bit-identical (int32 patterns, sign of zero
included; a skipped slot exactly 0x7fc00000) to the C oracle's score_all / score_pairs -- every branch of the sum order on
tables whose entries carry their own binary exponent; list lengths around the 8-pair sub-step, the 64-entry step and one and two
chunk boundaries; skipped entries, steps and sub-steps; NaN / inf / -0, ties, an all-zero table; filters; three candidate
shards; 16-bit tables; the fixed-width kernel as a second reference at 64 / 128 / 256; workspace and output bounds; two threads
on two streams; one larger shape; the Python route."""
import threading

import numpy as np
import pytest
import torch

from test_gpu_rank_lists import (check, expected, oracle_pred, random_lists, random_problem, removed_mask, segment_filter,
                                 true_scores)
from test_gpu_rank_sets16 import padded
from test_gpu_workspace_bounds import guard, three_fills  # noqa: F401  (guard: a fixture)

pytestmark = pytest.mark.gpu

BILINEAR = ("distmult", "complex", "simple")
NAN_BITS = 0x7fc00000
SUM_ORDER = [("distmult", D) for D in (4, 12, 36, 100, 300, 508, 512, 516, 768, 1024)] + \
            [(m, D) for m in ("complex", "simple") for D in (12, 20, 64, 300, 768, 1000, 1024)]
# around the 8-pair sub-step, the 64-entry step, and one and two boundaries of a workgroup's 1 024-entry chunk
LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 200, 1500, 2500)
N_SMALL, Q_SMALL = 301, 12


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


def dev(a):
    return None if a is None else torch.as_tensor(a).cuda()


def spread(table, rel, seed):
    """Every entry of the table and of the relations gets its own binary exponent over 2^-20 .. 2^20 (spread of
    test_gpu_rank_sets_wide_bilinear.py): the terms of a sum differ by up to 2^120, so any reordering of the additions
    changes low bits."""
    g = torch.Generator().manual_seed(seed)
    return tuple(x * torch.exp2(torch.randint(-20, 21, x.shape, generator=g).float()) for x in (table, rel))


def problem(model, N, D, Q, seed, scaled=False, ties=True):
    """random_problem of test_gpu_rank_lists.py; ``ties``: a tenth of the rows are copies of some query's true entity."""
    table, rel, fixed, rel_ids, true_row = random_problem(model, N, D, Q, seed=seed)
    if scaled:
        table, rel = spread(table, rel, seed + 1000)
    if ties:
        g = torch.Generator().manual_seed(seed + 2000)
        dups = torch.randperm(N, generator=g)[:max(N // 10, 1)]
        dups = dups[~torch.isin(dups, true_row)]
        table[dups] = table[true_row[torch.randint(0, Q, (len(dups),), generator=g)]]
    return table, rel, fixed, rel_ids, true_row


def run(ops, model, table, source, fixed, rel, rel_ids, q_head, ptr, rows, true_row, want_scores=True, fn=None, **kw):
    """ops.rank_lists_wide; ``table`` / ``source``: host or device tensors, one tensor for both when they are the same."""
    tab = table if table.is_cuda else table.cuda()
    src = tab if source is table else (source if source.is_cuda else source.cuda())
    return (fn or ops.rank_lists_wide)(model, tab, src, dev(fixed), rel.cuda(), dev(rel_ids), q_head, dev(ptr), dev(rows),
                                       true_row=dev(true_row), want_scores=want_scores, **kw)


def oracle_of(oracle, model, table, rel, fixed, rel_ids, true_row, q_head):
    """The oracle's (Q, N) scores and the true scores read off them (checked against score_pairs on the true pairs)."""
    f, r, tv = table[fixed].numpy(), rel[rel_ids].numpy(), table[true_row].numpy()
    pred = oracle_pred(oracle, model, table.numpy(), f, r, q_head)
    true = pred[np.arange(len(f)), np.asarray(true_row)]
    pairs = true_scores(oracle, model, tv, f, r, q_head)
    both = ~np.isnan(true)
    assert np.array_equal(np.isnan(pairs), ~both) and np.array_equal(pairs[both].view(np.int32), true[both].view(np.int32))
    return pred, true


# ------------------------------------------------------------------------------------------------ 1. the sum order
@pytest.mark.parametrize("model,D", SUM_ORDER)
def test_every_branch_of_the_sum_order(ops, oracle, model, D):
    N, Q = N_SMALL, Q_SMALL
    table, rel, fixed, rel_ids, true_row = problem(model, N, D, Q, seed=D, scaled=True)
    ptr, rows = random_lists(Q, N, lengths=LENGTHS, seed=D + 1)
    seen_ties = seen_long = False
    for q_head in (0, 5, Q):
        pred, true = oracle_of(oracle, model, table, rel, fixed, rel_ids, true_row, q_head)
        want = expected(pred, true, ptr, rows)
        seen_ties |= bool((want[0][:, 1] > want[0][:, 0]).any())
        seen_long |= bool(want[0][:, 0].max() > 64)
        check(run(ops, model, table, table, fixed, rel, rel_ids, q_head, ptr, rows, true_row), want, (model, D, q_head))
        if q_head == 5:  # scores alone (no true_row, no workspace); counts alone
            c, s = run(ops, model, table, table, fixed, rel, rel_ids, q_head, ptr, rows, None)
            assert c is None
            check((None, s), want, (model, D, "scores alone"))
            c, s = run(ops, model, table, table, fixed, rel, rel_ids, q_head, ptr, rows, true_row, want_scores=False)
            assert s is None
            check((c, None), want, (model, D, "counts alone"))
    assert seen_ties and seen_long, "ties with the true entity and more than 64 entries above it must occur"


# ------------------------------------------------------------------------------------------------ 2. skipped entries
@pytest.mark.parametrize("model,D", [("distmult", 300), ("complex", 20), ("simple", 768)])
def test_skipped_entries_steps_and_substeps(ops, oracle, model, D):
    N, Q = N_SMALL, 8
    table, rel, fixed, rel_ids, true_row = problem(model, N, D, Q, seed=D + 7, scaled=True)
    rng = np.random.default_rng(D)
    lens = (200, 70, 100, 5, 64, 0, 130, 9)
    lists = [rng.integers(0, N, n).astype(np.int64) for n in lens]
    lists[0][64:128] = rng.choice([-1, N, N + 7, -5], 64)      # the list starts the chunk: entries 64 .. 127 are its second step
    lists[0][[0, 7, 31, 199]] = (-1, N - 1, N, N + 7)
    lists[1][:] = N + rng.integers(0, 50, 70)                  # a list that is entirely skipped (two steps)
    lists[2][8:16] = -1                                        # a sub-step of eight invalid entries
    lists[2][40:48] = N
    lists[3][:] = -1                                           # a short list entirely skipped
    lists[4][:63] = -1                                         # one valid entry, the step's last: every other lane reads its row
    lists[6][0:64] = N + 3                                     # a first step with no valid entry
    lists[7][[0, 8]] = (N, -1)
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    rows = np.concatenate(lists)
    for q_head in (0, 4):
        pred, true = oracle_of(oracle, model, table, rel, fixed, rel_ids, true_row, q_head)
        want = expected(pred, true, ptr, rows)
        assert (want[0][[1, 3, 5]] == 0).all() and want[2][ptr[1]:ptr[2]].all() and want[2][64:128].all()
        got = run(ops, model, table, table, fixed, rel, rel_ids, q_head, ptr, rows, true_row)
        check(got, want, (model, D, q_head))
        assert (got[1].cpu().numpy()[want[2]].view(np.int32) == NAN_BITS).all()


# ------------------------------------------------------------------------------------------------ 3. special values, ties
def special_columns(model, D):
    """A column of the first 32-term row, of a leftover vector of 8 and of the n % 8 tail (None where the width has none)."""
    n = D if model == "distmult" else D // 2
    whole, vecs = n // 32, n // 8
    return (3 if whole else None, 32 * whole + 9 if vecs - 4 * whole >= 2 else (32 * whole + 1 if vecs - 4 * whole else None),
            n - 1 if n % 8 else None)


@pytest.mark.parametrize("D", [300, 20])
@pytest.mark.parametrize("model", BILINEAR)
def test_nan_inf_signed_zero_and_duplicates(ops, oracle, model, D):
    N, Q = N_SMALL, Q_SMALL
    table, rel, fixed, rel_ids, true_row = problem(model, N, D, Q, seed=D + 11)
    H = D // 2
    row = 10
    for col in special_columns(model, D):
        for value in (float("nan"), float("inf"), float("-inf")):
            if col is not None:
                table[row, col] = value
                if model != "distmult":
                    table[row + 1, H + col] = value
            row += 2
    first_plain = row
    table[row] = 0.0
    table[row + 1] = -0.0
    table[row + 2, ::2] = -0.0
    table[row + 2, 1::2] = 0.0
    table[row + 3] = -table[row + 4].abs()  # negative products against a positive query
    true_row[0], true_row[7] = 10, first_plain  # a true score that is NaN where the width has whole rows; a zero one
    rel[0] = -0.0
    special = np.arange(10, row + 5)
    ptr, rows = random_lists(Q, N, lengths=(64, 200, 40), seed=D + 12, specials=False)
    rows[ptr[:-1, None] + np.arange(len(special))] = special  # every list meets the special rows
    rows[ptr[:-1] + 39] = rows[ptr[:-1] + 38]                 # a duplicate list entry next to its twin
    pred, true = oracle_of(oracle, model, table, rel, fixed, rel_ids, true_row, 5)
    want = expected(pred, true, ptr, rows)
    assert np.isnan(want[1][~want[2]]).any() and np.isinf(want[1]).any()
    assert (want[1] == 0).any(), "zero scores must occur (their sign bit is compared)"
    check(run(ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, true_row), want, (model, D))


@pytest.mark.parametrize("model,D", [("distmult", 300), ("complex", 20), ("simple", 300)])
def test_all_zero_table_every_entry_ties(ops, oracle, model, D):
    N, Q = N_SMALL, Q_SMALL
    table, rel, fixed, rel_ids, true_row = problem(model, N, D, Q, seed=D + 13, ties=False)
    table.zero_()
    ptr, rows = random_lists(Q, N, lengths=LENGTHS, seed=D + 14)
    pred, true = oracle_of(oracle, model, table, rel, fixed, rel_ids, true_row, 5)
    want = expected(pred, true, ptr, rows)
    valid = np.array([(~want[2][ptr[q]:ptr[q + 1]]).sum() for q in range(Q)])
    assert (want[0][:, 0] == 0).all() and np.array_equal(want[0][:, 1], valid) and valid.max() > 2000
    assert (want[1][~want[2]].view(np.int32) == 0).all()  # +0, the oracle's
    check(run(ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, true_row), want, (model, D))


# ------------------------------------------------------------------------------------------------ 4. filters
@pytest.mark.parametrize("model,D", [("distmult", 300), ("complex", 68), ("simple", 300), ("distmult", 68)])
def test_filters(ops, oracle, model, D):
    N, Q = N_SMALL, Q_SMALL
    table, rel, fixed, rel_ids, true_row = problem(model, N, D, Q, seed=D + 17, scaled=True)
    ptr, rows = random_lists(Q, N, lengths=LENGTHS, seed=D + 18)
    pred, true = oracle_of(oracle, model, table, rel, fixed, rel_ids, true_row, 5)
    rng = np.random.default_rng(D + 19)
    args = (ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, true_row)
    # the three best entries of the longest lists are one row: a filtered row that occurs three times, all three removed
    for q in range(Q):
        if ptr[q + 1] - ptr[q] >= 200:
            seg = rows[ptr[q]:ptr[q + 1]]
            ok = np.nonzero((seg >= 0) & (seg < N))[0]
            best = seg[ok[np.argmax(pred[q, seg[ok]])]]
            seg[ok[[3, 50, 150]]] = best
    plain = expected(pred, true, ptr, rows)

    def members(q, n):
        seg = rows[ptr[q]:ptr[q + 1]]
        seg = seg[(seg >= 0) & (seg < N)]
        top = seg[np.argsort(-pred[q, seg], kind="stable")[:3]] if len(seg) else seg
        return np.concatenate((top, rng.choice(seg, n))) if len(seg) else np.zeros(0, np.int64)

    # (a) rows (out-of-range values among them); the segment's first value is the query's own entity: never removed
    segs = [np.unique(np.concatenate((members(q, 9), rng.integers(0, N, 5), [-1, N + 3]))) for q in range(Q)]
    exclude = np.array([s[2] for s in segs], np.int64)
    want = expected(pred, true, ptr, rows, removed=removed_mask(segs, exclude, None, N))
    no_ex = expected(pred, true, ptr, rows, removed=removed_mask(segs, None, None, N))
    assert (want[0][:, 3] < plain[0][:, 1]).any() and (want[0][:, 2] < plain[0][:, 0]).any(), "the filter must change the counts"
    assert not np.array_equal(want[0], no_ex[0]), "exclude must change the counts"
    q_long = int(np.argmax(np.diff(ptr)))
    assert plain[0][q_long, 1] - no_ex[0][q_long, 3] >= 3, "the three copies of the best row are all removed"
    check(run(*args, filter=segment_filter(ops, segs, exclude, None, 0)), want, (model, D, "rows"))
    check(run(*args, filter=segment_filter(ops, segs, None, None, 0)), no_ex, (model, D, "rows, nothing exempt"))

    # (b) entity ids through an ent2idx with -1 entries
    ent2idx = rng.permutation(N + 200).astype(np.int64)
    ent2idx[ent2idx >= N] = -1
    row2id = np.full(N, -1, np.int64)
    row2id[ent2idx[ent2idx >= 0]] = np.nonzero(ent2idx >= 0)[0]
    id_segs = [np.unique(np.concatenate((row2id[members(q, 9)], rng.integers(0, N + 200, 6), [N + 500, -2]))) for q in range(Q)]
    id_ex = np.array([s[3] for s in id_segs], np.int64)
    want = expected(pred, true, ptr, rows, removed=removed_mask(id_segs, id_ex, ent2idx, N))
    assert not np.array_equal(want[0], plain[0])
    check(run(*args, filter=segment_filter(ops, id_segs, id_ex, ent2idx, 0)), want, (model, D, "ids"))

    # (c) segments of more than 64 entries; (d) a query whose whole list is filtered
    big = [np.zeros(0, np.int64) for _ in range(Q)]
    big[9] = rng.permutation(N)[:200]
    big[10] = np.unique(rows[ptr[10]:ptr[11]])
    big[8] = np.arange(N)
    want = expected(pred, true, ptr, rows, removed=removed_mask(big, None, None, N))
    assert (want[0][[8, 10], 2:] == 0).all() and want[0][10, 1] > 0 and not np.array_equal(want[0][9], plain[0][9])
    check(run(*args, filter=segment_filter(ops, big, None, None, 0)), want, (model, D, "long segments"))


# ------------------------------------------------------------------------------------------------ 5. candidate shards
@pytest.mark.parametrize("model,D", [("distmult", 300), ("complex", 300), ("simple", 68)])
def test_three_candidate_shards_add_up(ops, oracle, model, D):
    N, Q = N_SMALL, Q_SMALL
    table, rel, fixed, rel_ids, true_row = problem(model, N, D, Q, seed=D + 23, scaled=True)
    ptr, rows = random_lists(Q, N, lengths=LENGTHS, seed=D + 24)
    pred, true = oracle_of(oracle, model, table, rel, fixed, rel_ids, true_row, 5)
    segs = [np.unique(rows[ptr[q]:ptr[q + 1]][:9]) for q in range(Q)]
    whole = expected(pred, true, ptr, rows, removed=removed_mask(segs, None, None, N))
    check(run(ops, model, table, table, fixed, rel, rel_ids, 5, ptr, rows, true_row, filter=segment_filter(ops, segs, None, None, 0)), whole)
    total = np.zeros((Q, 4), np.int32)
    seen = np.zeros(len(rows), int)
    for lo, hi in ((0, 97), (97, 230), (230, N)):
        got = run(ops, model, table[lo:hi], table, fixed, rel, rel_ids, 5, ptr, rows, true_row, row_base=lo,
                  filter=segment_filter(ops, segs, None, None, lo))
        check(got, expected(pred[:, lo:hi], true, ptr, rows, row_base=lo, removed=removed_mask(segs, None, None, hi - lo, lo)), (lo, hi))
        s = got[1].cpu().numpy()
        assert np.array_equal(np.isnan(s), ~((rows >= lo) & (rows < hi)))
        seen += ~np.isnan(s)
        total += got[0].cpu().numpy()
    assert np.array_equal(total, whole[0])
    assert np.array_equal(seen == 1, (rows >= 0) & (rows < N)) and (seen <= 1).all()


# ------------------------------------------------------------------------------------------------ 6. 16-bit tables
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("D", [20, 300, 768])
@pytest.mark.parametrize("model", BILINEAR)
def test_16_bit_table_equals_the_widened_table(ops, oracle, model, D, dtype):
    N, Q = N_SMALL, Q_SMALL
    table, rel, fixed, rel_ids, true_row = problem(model, N, D, Q, seed=D + 29)
    t16 = padded(table.to(dtype).cuda())
    if D % 8 == 0:
        assert t16.stride(0) == D + 8
    wide = table.to(dtype).float()
    assert torch.equal(t16.float().cpu(), wide)
    ptr, rows = random_lists(Q, N, lengths=LENGTHS, seed=D + 30)
    src = wide[torch.cat((fixed, true_row))]
    idx_f, idx_t = np.arange(Q), np.arange(Q, 2 * Q)
    segs = [np.unique(rows[ptr[q]:ptr[q + 1]][:7]) for q in range(Q)]
    filt = segment_filter(ops, segs, None, None, 0)
    got16 = run(ops, model, t16, src, idx_f, rel, rel_ids, 5, ptr, rows, idx_t, filter=filt)
    got32 = run(ops, model, wide, src, idx_f, rel, rel_ids, 5, ptr, rows, idx_t, filter=filt)
    assert torch.equal(got16[0], got32[0])
    assert torch.equal(got16[1].view(torch.int32), got32[1].view(torch.int32))
    pred, true = oracle_of(oracle, model, wide, rel, fixed, rel_ids, true_row, 5)
    check(got16, expected(pred, true, ptr, rows, removed=removed_mask(segs, None, None, N)), (model, D, dtype))
    with pytest.raises(TypeError):  # a 16-bit source, as ops.rank_lists refuses it
        ops.rank_lists_wide(model, t16, t16, dev(fixed), rel.cuda(), dev(rel_ids), 5, dev(ptr), dev(rows), true_row=dev(true_row))
    with pytest.raises(TypeError):
        ops.rank_lists_wide(model, t16, src.to(dtype).cuda(), dev(idx_f), rel.cuda(), dev(rel_ids), 5, dev(ptr), dev(rows), true_row=dev(idx_t))


# ------------------------------------------------------------------------------------------------ 7. the fixed-width kernel
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("model", BILINEAR)
def test_the_fixed_width_kernel_agrees(ops, model, D):
    N, Q = N_SMALL, Q_SMALL
    table, rel, fixed, rel_ids, true_row = problem(model, N, D, Q, seed=D + 31, scaled=True)
    ptr, rows = random_lists(Q, N, lengths=LENGTHS, seed=D + 32)
    segs = [np.unique(rows[ptr[q]:ptr[q + 1]][:9]) for q in range(Q)]
    filt = segment_filter(ops, segs, None, None, 0)
    plain, _, _, _, _ = problem(model, N, D, Q, seed=D + 31)  # (bf16 holds the unscaled values' range as well; f16 would not)
    for tab, src in ((table, table), (table.to(torch.bfloat16), table.to(torch.bfloat16).float()), (plain.to(torch.bfloat16), plain)):
        for f in (None, filt):
            new = run(ops, model, tab.cuda(), src.cuda(), fixed, rel, rel_ids, 5, ptr, rows, true_row, filter=f)
            old = run(ops, model, tab.cuda(), src.cuda(), fixed, rel, rel_ids, 5, ptr, rows, true_row, filter=f, fn=ops.rank_lists)
            assert torch.equal(new[0], old[0]), (model, D, tab.dtype)
            assert torch.equal(new[1].view(torch.int32), old[1].view(torch.int32)), (model, D, tab.dtype)
            if f is not None:
                assert not torch.equal(new[0][:, 2:], new[0][:, :2]), "the filter must change the counts"


# ------------------------------------------------------------------------------------------------ 8. workspace and outputs
@pytest.mark.parametrize("case", ["both sides", "heads only", "tails only", "every list empty", "one list of 2500"])
@pytest.mark.parametrize("model,D,dtype", [("distmult", 300, torch.float32), ("complex", 68, torch.float16), ("simple", 768, torch.bfloat16)])
def test_workspace_and_output_bounds(ops, oracle, guard, model, D, dtype, case):
    N = N_SMALL
    Q = 1 if case == "one list of 2500" else 65  # 65 queries: 260 bytes of true keys, a second 256-byte line
    table, rel, fixed, rel_ids, true_row = problem(model, N, D, Q, seed=D + 37)
    host = table.to(dtype).float()
    tab = table.cuda() if dtype is torch.float32 else table.to(dtype).cuda()
    src = tab if dtype is torch.float32 else host.cuda()
    lengths = {"every list empty": (0,), "one list of 2500": (2500,)}.get(case, (0, 1, 7, 9, 64, 65, 130))
    ptr, rows = random_lists(Q, N, lengths=lengths, seed=D + 38)
    nnz = len(rows)
    q_head = {"heads only": Q, "tails only": 0, "one list of 2500": 1}.get(case, Q // 2)
    need = (4 * Q + 255) // 256 * 256
    assert need == 256 * (1 + (Q > 64))
    pred, true = oracle_of(oracle, model, host, rel, fixed, rel_ids, true_row, q_head)
    segs = [np.unique(rows[ptr[q]:ptr[q + 1]][:9]) for q in range(Q)]
    args = (model, tab, src, fixed.cuda(), rel.cuda(), rel_ids.cuda(), q_head, dev(ptr), dev(rows))
    for filt, rm in ((None, None), (segment_filter(ops, segs, None, None, 0), removed_mask(segs, None, None, N))):
        what = (model, D, dtype, case, filt is not None)
        want = expected(pred, true, ptr, rows, removed=rm)
        both, asked = three_fills(guard, lambda g: ops.rank_lists_wide(*args, true_row=true_row.cuda(), filter=filt, want_scores=True,
                                                                       out=(g.out((Q, 4), torch.int32), g.out((nnz,), torch.float32))), what)
        assert asked == [need]
        check(both, want, what)
        counts, asked = three_fills(guard, lambda g: ops.rank_lists_wide(*args, true_row=true_row.cuda(), filter=filt,
                                                                         out=(g.out((Q, 4), torch.int32), None)), what)
        assert asked == [need] and counts[1] is None
        check(counts, want, what)
    if nnz == 0:  # no entry, no score slot: the scores-only form has no output to give an address (blp_rank_lists' refusal)
        with pytest.raises(RuntimeError, match="both outputs NULL"):
            ops.rank_lists_wide(*args)
        return
    scores, asked = three_fills(guard, lambda g: ops.rank_lists_wide(*args, out=(None, g.out((nnz,), torch.float32))), (model, D, case, "scores only"))
    assert asked == [] and scores[0] is None  # the scores-only form touches no workspace: none is asked for, NULL is passed
    check(scores, expected(pred, true, ptr, rows), (model, D, case, "scores only"))


# ------------------------------------------------------------------------------------------------ 9. two streams
def test_two_threads_on_two_streams(ops):
    N, Q = 1000, 12
    problems = []
    for i, (model, D) in enumerate((("distmult", 300), ("complex", 768))):
        table, rel, fixed, rel_ids, true_row = problem(model, N, D, Q, seed=50 + i)
        ptr, rows = random_lists(Q, N, lengths=LENGTHS, seed=60 + i)
        d = [x.cuda() for x in (table, rel, fixed, rel_ids, true_row, torch.from_numpy(ptr), torch.from_numpy(rows))]
        single = ops.rank_lists_wide(model, d[0], d[0], d[2], d[1], d[3], 5, d[5], d[6], true_row=d[4], want_scores=True)
        problems.append((model, d, single))
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def worker(i):
        try:
            model, d, _ = problems[i]
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for _ in range(5):
                    out = ops.rank_lists_wide(model, d[0], d[0], d[2], d[1], d[3], 5, d[5], d[6], true_row=d[4], want_scores=True)
            stream.synchronize()
            results[i] = out
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    for i in range(2):
        assert torch.equal(results[i][0], problems[i][2][0])
        assert torch.equal(results[i][1].view(torch.int32), problems[i][2][1].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 10. one larger shape
@pytest.mark.parametrize("model", ["distmult", "complex"])
def test_larger_shape_against_gathered_oracle_scores(ops, oracle, model):
    """512 queries x 500 candidates against a 50 001-row table at D = 300: the expected counts are the oracle's scores of the
    gathered (query, candidate) pairs compared with its true scores -- not a ranking of the whole table."""
    N, D, Q, C = 50_001, 300, 512, 500
    table, rel, fixed, rel_ids, true_row = problem(model, N, D, Q, seed=40, ties=False)
    g = torch.Generator().manual_seed(41)
    cand = torch.randint(0, N, (Q, C), generator=g)
    cand[:, 0] = true_row  # the true entity is listed
    cand[:, 1] = N - 1
    q_head = Q // 2
    tab = table.numpy()
    f, r, tv = tab[fixed.numpy()], rel[rel_ids].numpy(), tab[true_row.numpy()]
    true = true_scores(oracle, model, tv, f, r, q_head)
    ref = np.empty((Q, C), np.float32)
    for lo in range(0, Q, 128):
        hi = lo + 128
        e = tab[cand[lo:hi].numpy().reshape(-1)]
        fq, rq = np.repeat(f[lo:hi], C, axis=0), np.repeat(r[lo:hi], C, axis=0)
        s = oracle.score_pairs(model, e, fq, rq) if hi <= q_head else oracle.score_pairs(model, fq, e, rq)
        ref[lo:hi] = s.reshape(hi - lo, C)
    want = np.zeros((Q, 4), np.int32)
    want[:, 0] = (ref > true[:, None]).sum(1)
    want[:, 1] = (ref >= true[:, None]).sum(1)
    want[:, 2:] = want[:, :2]
    assert (want[:, 1] > want[:, 0]).all()
    ptr = np.arange(Q + 1, dtype=np.int64) * C
    got = run(ops, model, table, table, fixed, rel, rel_ids, q_head, ptr, cand.reshape(-1).numpy(), true_row)
    check(got, (want, ref.reshape(-1)), model)


# ------------------------------------------------------------------------------------------------ 11. rank_candidates
def _model(rel_model, rel_w):
    from blp_amd import models
    m = models.LinkPrediction(rel_w.shape[1], rel_model, "margin", rel_w.shape[0], 0)
    with torch.no_grad():
        m.rel_emb.weight.copy_(rel_w)
    return m


def candidates_problem(D, seed):
    """A table of 200 entities with ids scattered over [0, 260), 30 triples among them, a filtering graph that holds them and
    edges that share their (entity, relation) keys."""
    from blp_amd import utils
    N, T, R = 200, 30, 5
    g = torch.Generator().manual_seed(seed)
    entities = torch.randperm(260, generator=g)[:N]
    ent2idx = utils.make_ent2idx(entities, 259)
    table = torch.randn(N, D, generator=g) * 0.1
    rel_w = (torch.rand(R, D, generator=g) - 0.5) * 0.25
    pick = lambda n: entities[torch.randint(0, N, (n,), generator=g)]
    triples = torch.stack((pick(T), pick(T), torch.randint(0, R, (T,), generator=g)), dim=1)
    more = torch.stack((triples[:, 0].repeat(6), pick(6 * T), triples[:, 2].repeat(6)), dim=1)      # known tails of (h, r)
    more2 = torch.stack((pick(6 * T), triples[:, 1].repeat(6), triples[:, 2].repeat(6)), dim=1)     # known heads of (t, r)
    index = utils.FilterIndex(torch.cat((triples, more, more2)))
    return table, rel_w, triples, ent2idx, index


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [300, 768])
@pytest.mark.parametrize("rel_model", BILINEAR)
def test_rank_candidates_on_device_equals_its_cpu_route(ops, rel_model, D, dtype, monkeypatch):
    from blp_amd import ranking
    table, rel_w, triples, ent2idx, index = candidates_problem(D, seed=D + 70)
    table = table.to(dtype)
    N, Q = table.shape[0], 2 * triples.shape[0]
    rng = np.random.default_rng(D + 71)
    cand = torch.from_numpy(rng.integers(-1, N, (Q, 90)))
    ids = torch.from_numpy(rng.integers(-1, len(ent2idx) + 2, (Q, 90)))
    lens = rng.integers(0, 150, Q)
    lens[:3] = (0, 70, 149)
    csr = (torch.from_numpy(np.concatenate(([0], np.cumsum(lens)))), torch.from_numpy(rng.integers(-1, N + 3, int(lens.sum()))))
    cases = (("rows", cand, {}), ("ids", ids, dict(candidates_are="ids")), ("neg", cand, dict(include_true=False)),
             ("tail", cand[Q // 2:], dict(side="tail")), ("csr", csr, {}))
    model = _model(rel_model, rel_w)
    cpu = {name: ranking.rank_candidates(model, table, triples, c, ent2idx, filter_index=index, return_scores=True, **kw)
           for name, c, kw in cases}
    assert not torch.equal(cpu["rows"][0][:, 2:], cpu["rows"][0][:, :2]), "the filter must change the counts"

    def no_dense(*a, **k):
        raise AssertionError("the dense route was taken on a device table")

    assert not ops.rank_lists_supported(rel_model, D, dtype) and ops.rank_lists_wide_supported(rel_model, D, dtype)
    monkeypatch.setattr(ranking, "_rank_lists_dense", no_dense)
    dev_model = _model(rel_model, rel_w).cuda()
    for name, c, kw in cases:
        c = tuple(x.cuda() for x in c) if isinstance(c, tuple) else c.cuda()
        counts, scores = ranking.rank_candidates(dev_model, table.cuda(), triples, c, ent2idx, filter_index=index, return_scores=True, **kw)
        want_counts, want_scores = cpu[name]
        assert torch.equal(counts.cpu(), want_counts), (name, dtype)
        assert scores.shape == want_scores.shape
        check((None, scores.reshape(-1)), (None, want_scores.reshape(-1).numpy()), (name, dtype))


def test_rank_candidates_keeps_blp_rank_lists_at_128(ops, monkeypatch):
    from blp_amd import ranking
    table, rel_w, triples, ent2idx, index = candidates_problem(128, seed=90)
    Q = 2 * triples.shape[0]
    cand = torch.from_numpy(np.random.default_rng(91).integers(-1, table.shape[0], (Q, 90)))
    model = _model("distmult", rel_w)
    want = ranking.rank_candidates(model, table, triples, cand, ent2idx, filter_index=index)
    narrow, calls = ops.rank_lists, []

    def spy(*a, **k):
        calls.append("rank_lists")
        return narrow(*a, **k)

    def no_wide(*a, **k):
        raise AssertionError("a width blp_rank_lists takes went to blp_rank_lists_wide")

    monkeypatch.setattr(ops, "rank_lists", spy)
    monkeypatch.setattr(ops, "rank_lists_wide", no_wide)
    got = ranking.rank_candidates(_model("distmult", rel_w).cuda(), table.cuda(), triples, cand.cuda(), ent2idx, filter_index=index)
    assert calls == ["rank_lists"] and torch.equal(got.cpu(), want)
