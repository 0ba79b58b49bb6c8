"""Filtered top-k inside shared candidate sets for TransE at any width on the MI355X (blp_topk_sets_wide through
blp_amd.ops.topk_sets_wide and ranking.predict_links_in_sets).  Every comparison is bit-exact: rows equal, NaN positions equal,
the other scores equal as int32 patterns -- against the C oracle's scores of each query's set in numpy's stable order.  Widths
with a partial slab only (4), exactly one slab (64), a slab plus the smallest piece (68), several slabs (128, 768, 1024) and
300 = 4 slabs + 32 + 8 + 4; set sizes around the 64-row wave tile and the 256-row workgroup slab; query runs around every chunk
size (16 / 12 / 4 / 3 at k = 5 / 64 / 192 / 256); ties, NaN / inf / -0; filters; candidate shards merged by blp_topk_merge; the
forced grid; one long set in slabs; f16 / bf16 tables; the fixed-width kernel as a second reference at 64 / 128 / 256;
workspace and output bounds; two threads on two streams; the Python route."""
import threading

import numpy as np
import pytest
import torch

import test_gpu_topk_sets as base
from test_gpu_rank_sets16 import padded
from test_gpu_topk_sets import (HEAD_RUNS, N_ROWS, SET_SIZES, TAIL_RUNS, check, expected, make_problem, make_sets, oracle_pred,
                                removed_mask, segment_filter, unique_values)
from test_gpu_workspace_bounds import NAN_BITS, guard, three_fills  # noqa: F401  (guard: a fixture)

pytestmark = pytest.mark.gpu

WIDTHS = (4, 64, 68, 128, 300, 768, 1024)
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
CHUNKS = ((16, 5), (12, 64), (4, 192), (3, 256))  # (q_chunk, k): min(topk_chunk(k), 16) of blp_amd/csrc/topk_sets_wide.hip


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


def t(a):
    return torch.as_tensor(a).cuda()


def run(ops, p, k, ptr, rows, table=None, source=None, row_base=0, filter=None, queries=None, fn=None):
    """ops.topk_sets_wide on the problem; queries = (lo, hi, q_head, qh, qt): a slice of the queries as a call of its own."""
    lo, hi, q_head, qh, qt = queries if queries is not None else (0, p["Q"], p["q_head"], p["qh"], p["qt"])
    src = p["table"].cuda() if source is None else source
    tab = src if table is None else table
    return (fn or ops.topk_sets_wide)("transe", tab, src, t(p["fixed"][lo:hi]), p["rel"].cuda(), t(p["rel_ids"][lo:hi]), q_head, k,
                                      t(ptr), t(rows), t(qh), t(qt), filter=filter, row_base=row_base)


def same(got, want, what=""):
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), what


# ------------------------------------------------------------------------------------------------ 1. widths
@pytest.mark.parametrize("D", WIDTHS)
def test_widths(ops, oracle, D):
    sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=D)
    p = make_problem("transe", N_ROWS, D, HEAD_RUNS, TAIL_RUNS, seed=D + 1)
    pred = oracle_pred(oracle, p)
    h, Q, zeros = p["q_head"], p["Q"], np.zeros(len(SET_SIZES) + 1, np.int64)
    sizes = np.array(SET_SIZES)[p["set_of"]]
    for k in ((1, 5, 64, 192, 256) if D in (68, 300) else (1, 10, 256)):
        want = expected(pred, k, sets, p["set_of"])
        # the inputs exercise k > |set| (-1 slots present, the empty set's queries entirely) and k < |set|
        assert (want[0][sizes < k, -1] == -1).all() and (sizes < k).any() and (want[0][sizes == 0] == -1).all()
        assert (want[0][sizes >= k] >= 0).all() and (sizes > k).any()
        got = run(ops, p, k, ptr, rows)
        check(got, want, (D, k))
        assert (got[1].cpu().numpy().view(np.int32)[want[0] < 0] == NAN_BITS).all(), (D, k)  # an empty slot: the quiet NaN
        check(run(ops, p, k, ptr, rows, queries=(0, h, h, p["qh"], zeros)), (want[0][:h], want[1][:h]), (D, k, "heads only"))
        check(run(ops, p, k, ptr, rows, queries=(h, Q, 0, zeros, p["qt"])), (want[0][h:], want[1][h:]), (D, k, "tails only"))


# ------------------------------------------------------------------------------------------------ 2. query runs around the chunks
@pytest.mark.parametrize("c,k", CHUNKS)
@pytest.mark.parametrize("D", [68, 300])
def test_query_runs_around_every_chunk(ops, oracle, D, c, k):
    heads = (1, c - 1, c, c + 1, 2 * c + 1, 0, 0, 0, 0, 0, c)
    tails = (0, 0, 0, 0, 0, 1, c - 1, c, c + 1, 2 * c + 1, c + 1)
    sizes = (65, 300, 64, 257, 130, 65, 300, 64, 257, 130, 70)
    N = 301
    sets, ptr, rows = make_sets(N, sizes, seed=200 + D + k)
    p = make_problem("transe", N, D, heads, tails, seed=201 + D + k)
    check(run(ops, p, k, ptr, rows), expected(oracle_pred(oracle, p), k, sets, p["set_of"]), (D, c, k))


# ------------------------------------------------------------------------------------------------ 3. ties, special values
@pytest.mark.parametrize("D", [68, 300])
def test_ties_and_special_values(ops, oracle, D):
    sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=21 + D)
    p = make_problem("transe", N_ROWS, D, HEAD_RUNS, TAIL_RUNS, seed=22 + D)
    table, g = p["table"], torch.Generator().manual_seed(24)
    dups = torch.randperm(N_ROWS, generator=g)[:N_ROWS // 20]            # 5 % of the rows are copies of other rows ...
    table[dups] = table[torch.randint(0, N_ROWS, (dups.shape[0],), generator=g)]
    in_small = np.zeros(N_ROWS, bool)  # (set 9 is the whole table: "outside" means outside the sets below 1000 rows)
    in_small[np.concatenate([sets[g] for g in (1, 2, 3, 4, 5, 6, 7, 10, 11)])] = True
    outside = np.nonzero(~in_small)[0]
    # NaN / +inf / -inf in rows of the 63-, 64- and 255-row sets (they reach the tail of a k = 64 / 256 answer), of the
    # 1000-row set, and in rows outside every set but the whole table; the columns: the first slab, and the LAST 4-column
    # piece of the row (300: columns 296 .. 299; 68: 64 .. 67)
    specials = ((float("nan"), (sets[2][10], sets[3][11], sets[5][7], sets[8][3], outside[1])),
                (float("inf"), (sets[2][20], sets[3][21], sets[8][40], outside[5])),
                (float("-inf"), (sets[2][30], sets[5][31], sets[8][77], outside[9])))
    for value, rows_at in specials:
        for i, r in enumerate(rows_at):
            table[r, 5 if i % 2 else D - 2] = value
    table[sets[8][100]] = 0.0
    table[sets[8][101]] = -0.0
    table[sets[3][40], ::2] = -0.0
    table[sets[3][41], D - 4:] = -0.0
    # a zero relation against copies of the query's own fixed row: scores of exactly -0.0
    q0 = int(np.nonzero(p["set_of"] == 8)[0][0])
    p["rel"][0] = 0.0
    p["rel_ids"][q0] = 0
    table[sets[8][200:204]] = table[p["fixed"][q0]].clone()
    pred = oracle_pred(oracle, p)
    assert np.isnan(pred).any() and np.isinf(pred).any()
    for k in (5, 64, 256):
        check(run(ops, p, k, ptr, rows), expected(pred, k, sets, p["set_of"]), (D, k))
    want = expected(pred, 256, sets, p["set_of"])
    assert np.isnan(want[1][want[0] >= 0]).any() and np.isinf(want[1]).any()
    q8 = np.nonzero(p["set_of"] == 8)[0]
    assert any(len(np.unique(pred[q, sets[8]])) < len(sets[8]) - 3 for q in q8), "duplicate rows must tie inside the set"
    # the sign of zero comes back as the oracle's: checked on the bits (the key carries it; there is no re-scoring pass)
    neg0 = want[1].view(np.int32) == np.int32(-2 ** 31)
    assert neg0[q0, :4].all() and set(sets[8][200:204]) <= set(want[0][q0, :5]), "no -0 score among the expected ones"
    got = run(ops, p, 256, ptr, rows)[1].cpu().numpy()
    assert np.array_equal(got.view(np.int32) == np.int32(-2 ** 31), neg0)


# ------------------------------------------------------------------------------------------------ 4. filters
@pytest.mark.parametrize("D", [68, 300])
def test_filters(ops, oracle, D):
    N = N_ROWS
    sets, ptr, rows = make_sets(N, SET_SIZES, seed=31 + D)
    p = make_problem("transe", N, D, HEAD_RUNS, TAIL_RUNS, seed=32 + D)
    pred = oracle_pred(oracle, p)
    Q, set_of = p["Q"], p["set_of"]
    rng = np.random.default_rng(34)
    k = 10

    def best_inside(q, n):  # the best rows of the query's set: a filter that removes them changes the answer
        s = sets[set_of[q]]
        return s[np.argsort(-pred[q, s], kind="stable")][:n]

    def outside(q, n):
        cand = np.setdiff1d(np.arange(N), sets[set_of[q]])
        return rng.choice(cand, min(n, len(cand)), replace=False)

    # (a) rows: the best members of the set, non-members, values outside the table; the best member exempt (exclude)
    segs = [unique_values(best_inside(q, 6), outside(q, 6), [-1, N + 3]) for q in range(Q)]
    exclude = np.array([s[0] for s in segs], np.int64)
    want = expected(pred, k, sets, set_of, removed=removed_mask(segs, exclude, None, N))
    plain = expected(pred, k, sets, set_of)
    no_ex = expected(pred, k, sets, set_of, removed=removed_mask(segs, None, None, N))
    assert not np.array_equal(want[0], plain[0]) and not np.array_equal(want[0], no_ex[0])
    has = np.array(SET_SIZES)[set_of] > 0
    assert (want[0][has, 0] == exclude[has]).all(), "exclude[q] in its own segment survives (it is the best member)"
    check(run(ops, p, k, ptr, rows, filter=segment_filter(ops, segs, exclude, None, 0)), want, "rows")
    check(run(ops, p, k, ptr, rows, filter=segment_filter(ops, segs, None, None, 0)), no_ex, "rows, nothing exempt")

    # (b) entity ids through an ent2idx with -1 entries
    ent2idx = rng.permutation(N + 200).astype(np.int64)
    ent2idx[ent2idx >= N] = -1
    row2id = np.full(N, -1, np.int64)
    row2id[ent2idx[ent2idx >= 0]] = np.nonzero(ent2idx >= 0)[0]
    no_row = np.nonzero(ent2idx < 0)[0]
    id_segs = [unique_values(row2id[best_inside(q, 6)], row2id[outside(q, 4)], no_row[:3], [N + 500, -2]) for q in range(Q)]
    id_ex = np.array([s[0] for s in id_segs], np.int64)
    want = expected(pred, k, sets, set_of, removed=removed_mask(id_segs, id_ex, ent2idx, N))
    assert not np.array_equal(want[0], plain[0])
    check(run(ops, p, k, ptr, rows, filter=segment_filter(ops, id_segs, id_ex, ent2idx, 0)), want, "ids")

    # (c) a 5 000-entry segment; (d) a query whose filter leaves 3 rows of a 300-row set
    big = [np.zeros(0, np.int64) for _ in range(Q)]
    q_whole = int(np.nonzero(set_of == 9)[0][2])
    q_300 = int(np.nonzero(set_of == 10)[0][0])
    big[q_whole] = rng.permutation(6000)[:5000]     # 5 000 distinct values, those >= N name no row
    big[q_300] = sets[10][3:]
    assert len(big[q_300]) > 64
    for kk in (10, 256):
        want = expected(pred, kk, sets, set_of, removed=removed_mask(big, None, None, N))
        assert (want[0][q_300, :3] >= 0).all() and (want[0][q_300, 3:] == -1).all()
        assert (want[0][q_whole] != plain[0][q_whole]).any() if kk == 10 else True
        check(run(ops, p, kk, ptr, rows, filter=segment_filter(ops, big, None, None, 0)), want, ("long segment", kk))


# ------------------------------------------------------------------------------------------------ 5. shards
def test_two_candidate_shards_merge_to_the_unsharded_call(ops, oracle):
    N, D = N_ROWS, 300
    sets, ptr, rows = make_sets(N, SET_SIZES, seed=41)
    p = make_problem("transe", N, D, HEAD_RUNS, TAIL_RUNS, seed=42)
    pred = oracle_pred(oracle, p)
    segs = [unique_values(sets[g][np.argsort(-pred[q, sets[g]], kind="stable")][:4], [3, N - 2]) if len(sets[g]) else np.zeros(0, np.int64)
            for q, g in enumerate(p["set_of"])]
    cut = 517
    assert all((s < cut).any() and (s >= cut).any() for s in sets if len(s) > 60), "the shard boundary falls inside the sets"
    assert sum((s < cut).sum() % 64 != 0 for s in sets) >= 8 and (sets[9] < cut).sum() % 64 == 5, "... and inside a 64-row tile"
    for k in (10, 192):
        whole = expected(pred, k, sets, p["set_of"], removed=removed_mask(segs, None, None, N))
        check(run(ops, p, k, ptr, rows, filter=segment_filter(ops, segs, None, None, 0)), whole, k)
        parts = []
        for lo, hi in ((0, cut), (cut, N)):
            got = run(ops, p, k, ptr, rows, table=p["table"][lo:hi].cuda(), source=p["table"].cuda(), row_base=lo,
                      filter=segment_filter(ops, segs, None, None, lo))
            check(got, expected(pred[:, lo:hi], k, sets, p["set_of"], row_base=lo, removed=removed_mask(segs, None, None, hi - lo, lo)), (lo, hi, k))
            parts.append(got)
        assert (parts[0][0] == -1).any() and (parts[0][0][:, -1] >= 0).any()  # shards that hold fewer than k of a set's rows
        merged = ops.topk_merge(torch.cat((parts[0][0], parts[1][0]), 1), torch.cat((parts[0][1], parts[1][1]), 1), k)
        check(merged, whole, (k, "merged"))


# ------------------------------------------------------------------------------------------------ 6. the grid
def test_more_work_units_than_resident_workgroups_and_the_forced_grid(ops, oracle, knobs):
    """D = 4, 2 400 tiny sets with one or two queries each: about 3 000 units, far above two workgroups per compute unit; the
    same result with the grid forced to 1 and to 7 workgroups (knob topk_sets_grid of the hooks build)."""
    N, D, G, k = 64, 4, 2400, 5
    rng = np.random.default_rng(7)
    sizes = rng.integers(1, 9, G)
    heads, tails = (np.arange(G) % 2 == 0).astype(np.int64), (np.arange(G) % 4 != 0).astype(np.int64)
    sets, ptr, rows = make_sets(N, sizes, seed=8)
    p = make_problem("transe", N, D, heads, tails, seed=9)
    want = expected(oracle_pred(oracle, p), k, sets, p["set_of"])
    assert int(heads.sum() + tails.sum()) > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    default = run(ops, p, k, ptr, rows)
    check(default, want)
    for grid in (1, 7):
        knobs("topk_sets_grid", grid)
        same(run(ops, p, k, ptr, rows), default, grid)
    knobs("topk_sets_grid", 0)


# ------------------------------------------------------------------------------------------------ 7. one long set
def test_one_long_set_takes_the_slab_path(ops, oracle):
    """300 001 rows x 68, one set of 200 000 rows, 3 + 1 queries: few queries against a long set are cut into slabs (S_max > 1
    partial lists per query, merged)."""
    N, D, n_set = 300_001, 68, 200_000
    sets, ptr, rows = make_sets(N, (n_set,), seed=90)
    p = make_problem("transe", N, D, (3,), (1,), seed=91)
    # the host-side rule (topk_sets_slabs_rule with q_chunk = min(topk_chunk(k), 16)): S_max = min(512 / chunks, tiles / 4)
    for k, chunk in ((256, 3), (10, 16)):
        s_max = min(512 // -(-4 // chunk), -(-(-(-n_set // 64)) // 4))
        assert s_max > 1
        one_list = ops.topk_sets_wide_workspace_bytes("transe", D, 3, 1, 1, 64, k)
        assert ops.topk_sets_wide_workspace_bytes("transe", D, 3, 1, 1, n_set, k) >= one_list + 4 * (s_max - 1) * k * 8
    pred = oracle_pred(oracle, p)
    segs = [sets[0][np.argsort(-pred[q, sets[0]], kind="stable")][1:200:2] for q in range(4)]
    want = expected(pred, 256, sets, p["set_of"], removed=removed_mask(segs, None, None, N))
    check(run(ops, p, 256, ptr, rows, filter=segment_filter(ops, segs, None, None, 0)), want)
    check(run(ops, p, 10, ptr, rows), expected(pred, 10, sets, p["set_of"]))


# ------------------------------------------------------------------------------------------------ 8. 16-bit tables
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("D", [68, 300, 768])
def test_16_bit_tables_equal_the_f32_call_on_the_widened_table_and_the_oracle(ops, oracle, D, dtype):
    dt = DTYPES[dtype]
    sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=600 + D)
    p = make_problem("transe", N_ROWS, D, HEAD_RUNS, TAIL_RUNS, seed=601 + D)
    p["table"] = p["table"].to(dt).float()
    segs = [sets[g][:4] for g in p["set_of"]]
    filt = segment_filter(ops, segs, None, None, 0)
    t32 = p["table"].cuda()
    t16 = padded(p["table"].to(dt).cuda())  # ld = D + 8 > D, ld % 8 == 0
    assert t16.stride(0) == D + 8 and torch.equal(t16.float(), t32)
    pred = oracle_pred(oracle, p)
    for k in (10, 256):
        want32 = run(ops, p, k, ptr, rows, filter=filt)
        got = run(ops, p, k, ptr, rows, table=t16, source=t32, filter=filt)
        same(got, want32, (D, dtype, k))
        check(got, expected(pred, k, sets, p["set_of"], removed=removed_mask(segs, None, None, N_ROWS)), (D, dtype, k))
    with pytest.raises(TypeError):  # a 16-bit `source`
        run(ops, p, 10, ptr, rows, table=t16, source=t16)


# ------------------------------------------------------------------------------------------------ 9. the fixed-width kernel
@pytest.mark.parametrize("D", [64, 128, 256])
def test_fixed_width_kernel_agrees(ops, D):
    sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=700 + D)
    p = make_problem("transe", N_ROWS, D, HEAD_RUNS, TAIL_RUNS, seed=701 + D)
    filt = segment_filter(ops, [sets[g][:5] for g in p["set_of"]], None, None, 0)
    t16 = padded(p["table"].to(torch.bfloat16).cuda())
    src = t16.float().contiguous()
    for k in (10, 256):
        want = run(ops, p, k, ptr, rows, filter=filt, fn=ops.topk_sets)
        assert bool((want[0] >= 0).any()) and bool((want[0] == -1).any())
        same(run(ops, p, k, ptr, rows, filter=filt), want, (D, k))
        same(run(ops, p, k, ptr, rows, table=t16, source=src, filter=filt),
             run(ops, p, k, ptr, rows, table=t16, source=src, filter=filt, fn=ops.topk_sets), (D, k, "bf16"))


# ------------------------------------------------------------------------------------------------ 10. bounds
@pytest.mark.parametrize("D,dtype", [(68, "f32"), (300, "f32"), (300, "f16"), (768, "bf16")])
def test_workspace_and_output_bounds(ops, oracle, guard, D, dtype):
    """A workspace of exactly the advertised size and outputs between 64 KiB guards, under the three fill patterns."""
    sizes = (0, 1, 63, 64, 65, 257, 300, 301, 40, 40)
    heads = (1, 16, 0, 17, 2, 0, 5, 0, 0, 0)
    tails = (0, 1, 17, 0, 16, 3, 0, 0, 0, 0)
    cases = [("both", 301, sizes, heads, tails), ("heads only", 301, sizes, heads, (0,) * 10), ("tails only", 301, sizes, (0,) * 10, tails),
             ("every set empty", 301, (0,) * 10, heads, tails), ("long", 6007, (5000,), (3,), (1,))]
    for name, N, sz, hr, tr in cases:
        sets, ptr, rows = make_sets(N, sz, seed=900 + D)
        p = make_problem("transe", N, D, hr, tr, seed=901 + D)
        if dtype == "f32":
            tab = src = p["table"].cuda()
        else:
            p["table"] = p["table"].to(DTYPES[dtype]).float()
            tab, src = padded(p["table"].to(DTYPES[dtype]).cuda()), p["table"].cuda()
        Q, qh = p["Q"], p["q_head"]
        pred = oracle_pred(oracle, p)
        args = ("transe", tab, src, t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), qh)
        sets_args = (t(ptr), t(rows), t(p["qh"]), t(p["qt"]))
        for k in (10, 256):
            what = (D, dtype, name, k)
            need = ops.topk_sets_wide_workspace_bytes("transe", D, qh, Q - qh, len(sz), len(rows), k, tab.dtype)
            assert need > 0 and need % 256 == 0
            got, asked = three_fills(guard, lambda g: ops.topk_sets_wide(*args, k, *sets_args, out=(g.out((Q, k), torch.int64), g.out((Q, k), torch.float32))),
                                     what)
            assert asked == [need], what
            want = expected(pred, k, sets, p["set_of"])
            check(got, want, what)
            empty = got[0].numpy() < 0
            assert (got[1].numpy().view(np.int32)[empty] == NAN_BITS).all(), what
            if name == "every set empty":
                assert len(rows) == 0 and empty.all()
            if name == "long":
                assert (want[0] >= 0).all() and need > 4 * k * 8 * 8  # several key lists per query


# ------------------------------------------------------------------------------------------------ 11. threads
def test_two_threads_on_two_streams(ops, oracle):
    problems = []
    for i, (D, k) in enumerate(((300, 10), (68, 192))):
        sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=70 + i)
        p = make_problem("transe", N_ROWS, D, HEAD_RUNS, TAIL_RUNS, seed=72 + i)
        args = ("transe", p["table"].cuda(), p["table"].cuda(), t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), p["q_head"], k,
                t(ptr), t(rows), t(p["qh"]), t(p["qt"]))
        single = ops.topk_sets_wide(*args)
        check(single, expected(oracle_pred(oracle, p), k, sets, p["set_of"]), D)
        problems.append((args, single))
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def worker(i):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for _ in range(5):
                    out = ops.topk_sets_wide(*problems[i][0])
            stream.synchronize()
            results[i] = (out[0].cpu(), out[1].cpu())
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    [th.start() for th in threads]
    [th.join() for th in threads]
    assert not errors, errors
    for i in range(2):
        same(results[i], (problems[i][1][0].cpu(), problems[i][1][1].cpu()), i)


# ------------------------------------------------------------------------------------------------ 12. predict_links_in_sets
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", [300, 768])
def test_predict_links_in_sets_on_device_equals_its_cpu_route(D, dtype, monkeypatch):
    from blp_amd import ranking, utils
    N, R, T = 200, 6, 60
    g = torch.Generator().manual_seed(800 + D)
    table = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    if dtype == "bf16":
        table = table.to(torch.bfloat16)
    rel_w = ((torch.rand(R, D, generator=g) - 0.5) * 0.25).numpy()
    ent2idx = torch.randperm(N + 20, generator=g)
    ent2idx[ent2idx >= N] = -1
    ids = torch.nonzero(ent2idx >= 0).reshape(-1)
    pick = lambda n: ids[torch.randint(0, N, (n,), generator=g)]
    graph = torch.stack((pick(400), pick(400), torch.randint(0, R, (400,), generator=g)), dim=1)
    triples = graph[:T]
    index = utils.FilterIndex(graph)
    typed = ranking.relation_candidate_sets(graph, R, ent2idx)
    rng = np.random.default_rng(801)
    pools = ranking.CandidateSets([rng.choice(N, n, replace=False) for n in (0, 1, 65, N, 20)])
    pool_ids = torch.from_numpy(rng.integers(0, 5, 2 * T))
    entities = torch.arange(N) * 2 + 5
    cases = [("typed", typed, 3, {}), ("pools", pools, 5, dict(set_ids=pool_ids)), ("ids", pools, 64, dict(set_ids=pool_ids, entities=entities)),
             ("tail", pools, 256, dict(set_ids=pool_ids[T:], side="tail")), ("head", typed, 2, dict(side="head"))]
    cpu_model = base._model("transe", rel_w)
    cpu = {name: ranking.predict_links_in_sets(cpu_model, table, triples, k, sets, ent2idx, filter_index=index, **kw)
           for name, sets, k, kw in cases}
    plain = ranking.predict_links_in_sets(cpu_model, table, triples, 64, pools, ent2idx, set_ids=pool_ids, entities=entities)
    assert not torch.equal(plain[0], cpu["ids"][0]), "the filter must bite somewhere"
    dense = ranking._topk_sets_dense
    taken = []

    def no_dense(*a, **k):
        raise AssertionError("the dense route was taken on a device table")

    def counted(*a, **k):
        taken.append(1)
        return dense(*a, **k)

    def check_case(model, name, sets, k, kw):
        if "set_ids" in kw:
            kw = dict(kw, set_ids=kw["set_ids"].cuda())
        got = ranking.predict_links_in_sets(model, table.cuda(), triples, k, sets, ent2idx, filter_index=index, **kw)
        assert got[0].is_cuda and got[1].is_cuda
        base.check(got, (cpu[name][0].numpy(), cpu[name][1].numpy()), (name, D, dtype))

    dev_model = base._model("transe", rel_w).cuda()
    monkeypatch.setattr(ranking, "_topk_sets_dense", no_dense)
    for name, sets, k, kw in cases:
        check_case(dev_model, name, sets, k, kw)
    # k = 300 is beyond blp_topk_sets_wide's k, a bilinear model at 300 is not its model: the dense route by design.  (Its
    # scores are torch's on the device, whose reductions need not round as the CPU's do: with k above every set's size the
    # answer is the whole filtered set, compared as a set.)
    monkeypatch.setattr(ranking, "_topk_sets_dense", counted)
    for model, cpu_m, k in ((dev_model, cpu_model, 300), (base._model("distmult", rel_w).cuda(), base._model("distmult", rel_w), 210)):
        want = ranking.predict_links_in_sets(cpu_m, table, triples, k, pools, ent2idx, set_ids=pool_ids, filter_index=index)
        n = len(taken)  # (the CPU call is the dense route too)
        got = ranking.predict_links_in_sets(model, table.cuda(), triples, k, pools, ent2idx, set_ids=pool_ids.cuda(), filter_index=index)
        assert len(taken) == n + 1, "the dense route must be taken"
        assert got[0].is_cuda and got[0].shape == (2 * T, k)
        assert torch.equal(torch.sort(got[0].cpu(), 1)[0], torch.sort(want[0], 1)[0]) and bool((want[0] >= 0).any())
