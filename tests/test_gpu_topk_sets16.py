"""Filtered top-k inside shared candidate sets on a 16-BIT entity table on the MI355X (blp_topk_sets_typed through
blp_amd.ops.topk_sets and ranking.predict_links_in_sets).  Every comparison is bit-exact -- rows equal, NaN positions equal, the
remaining scores equal as int32 bit patterns -- against two yardsticks: blp_topk_sets on the table widened to f32 (it shares
everything after the tile with the kernel under test) and the C oracle's scores of the widened table in numpy's stable order.
Shapes are the f32 sibling's (1 031 rows, set sizes around the 64-row tile, query runs around the 32 / 4 / 3-query chunks, an
empty set with queries) with a row stride of D + 8 elements; one long set in slabs, one table of more than 2^31 bytes."""
import threading

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden
import test_gpu_topk_sets as base
from test_gpu_topk_sets import HEAD_RUNS, KS, N_ROWS, SET_SIZES, TAIL_RUNS

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
both_dtypes = pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))


@pytest.fixture(scope="module")
def ops():
    from blp_amd import ops as _ops
    return _ops


def padded(table16):
    """The same rows with a row stride of D + 8 elements (ld > D, ld % 8 == 0)."""
    wide = torch.zeros((table16.shape[0], table16.shape[1] + 8), dtype=table16.dtype, device=table16.device)
    wide[:, :table16.shape[1]] = table16
    return wide[:, :table16.shape[1]]


def make(model, D, dtype, seed, N=N_ROWS, sizes=SET_SIZES, head_runs=HEAD_RUNS, tail_runs=TAIL_RUNS):
    """A problem whose f32 table IS the 16-bit table widened: p["table"] (f32, host); dev16(p, dtype) is the 16-bit one."""
    sets, ptr, rows = base.make_sets(N, sizes, seed=seed)
    p = base.make_problem(model, N, D, head_runs, tail_runs, seed=seed + 1)
    p["table"] = p["table"].to(dtype).float()
    return p, sets, ptr, rows


def dev16(p, dtype):
    t16 = padded(p["table"].to(dtype).cuda())
    assert t16.stride(0) == p["table"].shape[1] + 8
    assert torch.equal(t16.float().cpu().view(torch.int32), p["table"].view(torch.int32))  # (bit patterns: NaN, -0)
    return t16


def same(got, want, what=""):
    """Two device results, bit for bit."""
    base.check(got, (want[0].cpu().numpy(), want[1].cpu().numpy()), what)


# ------------------------------------------------------------------------------------------------ 1. two yardsticks
@both_dtypes
@pytest.mark.parametrize("model,D", [(m, D) for m in REL_MODELS for D in (64, 128, 256)])
def test_rows_and_scores_match_the_f32_call_and_the_oracle(ops, oracle, model, D, dtype):
    p, sets, ptr, rows = make(model, D, DTYPES[dtype], seed=D)
    t16 = dev16(p, DTYPES[dtype])
    pred = base.oracle_pred(oracle, p)
    h, Q, zeros = p["q_head"], p["Q"], np.zeros(len(SET_SIZES) + 1, np.int64)
    sizes = np.array(SET_SIZES)[p["set_of"]]
    for k in KS:
        want = base.expected(pred, k, sets, p["set_of"])
        assert (want[0][sizes < k, -1] == -1).all() and (sizes < k).any() and (want[0][sizes == 0] == -1).all()
        assert (want[0][sizes >= k] >= 0).all() and (sizes > k).any()
        for what, queries, sl in (("both sides", None, slice(0, Q)), ("heads only", (0, h, h, p["qh"], zeros), slice(0, h)),
                                  ("tails only", (h, Q, 0, zeros, p["qt"]), slice(h, Q))):
            got = base.run(ops, p, k, ptr, rows, table=t16, queries=queries)
            base.check(got, (want[0][sl], want[1][sl]), (model, D, dtype, k, what, "oracle"))
            same(got, base.run(ops, p, k, ptr, rows, queries=queries), (model, D, dtype, k, what, "f32 call"))


# ------------------------------------------------------------------------------------------------ 2. special values
@both_dtypes
@pytest.mark.parametrize("model", ["transe", "complex"])
def test_ties_and_special_values(ops, oracle, model, dtype):
    D, dt = 128, DTYPES[dtype]
    p, sets, ptr, rows = make(model, D, dt, seed=21)
    table, g = p["table"], torch.Generator().manual_seed(24)
    dups = torch.randperm(N_ROWS, generator=g)[:N_ROWS // 20]            # 5 % of the rows are copies of other rows ...
    table[dups] = table[torch.randint(0, N_ROWS, (dups.shape[0],), generator=g)]
    in_small = np.zeros(N_ROWS, bool)  # (set 9 is the whole table: "outside" means outside the sets below 1000 rows)
    in_small[np.concatenate([sets[s] for s in (1, 2, 3, 4, 5, 6, 7, 10, 11)])] = True
    outside = np.nonzero(~in_small)[0]
    specials = ((float("nan"), (sets[2][10], sets[3][11], sets[5][7], sets[8][3], outside[1])),
                (float("inf"), (sets[2][20], sets[3][21], sets[8][40], outside[5])),
                (float("-inf"), (sets[2][30], sets[5][31], sets[8][77], outside[9])))
    for value, rows_at in specials:
        for r in rows_at:
            table[r, 5] = value
    tiny = torch.finfo(dt).smallest_normal / 4                           # a 16-bit subnormal (exact in f32)
    table[sets[8][100]] = 0.0
    table[sets[8][101]] = -0.0
    table[sets[3][40], ::2] = -0.0
    table[sets[8][102], ::3] = tiny
    table[sets[8][102], 1::3] = -tiny
    table[sets[3][41]] = tiny
    # TransE with a zero relation against copies of the query's own fixed row: scores of exactly -0.0
    q0 = int(np.nonzero(p["set_of"] == 8)[0][0])
    p["rel"][0] = 0.0
    p["rel_ids"][q0] = 0
    table[sets[8][200:204]] = table[p["fixed"][q0]].clone()
    # every planted value is a value of the 16-bit type (a NaN may change its payload on the way): the f32 table is made the
    # 16-bit table widened again
    assert torch.equal(table.to(dt).float().nan_to_num(7.0), table.nan_to_num(7.0)) and float(torch.tensor(tiny).to(dt)) == tiny
    assert torch.equal(torch.signbit(table.to(dt).float()) | table.isnan(), torch.signbit(table) | table.isnan())  # (-0 stays -0)
    p["table"] = table = table.to(dt).float()
    t16 = dev16(p, dt)
    pred = base.oracle_pred(oracle, p)
    assert np.isnan(pred).any() and np.isinf(pred).any()
    for k in (5, 64, 256):
        want = base.expected(pred, k, sets, p["set_of"])
        got = base.run(ops, p, k, ptr, rows, table=t16)
        base.check(got, want, (model, dtype, k))
        same(got, base.run(ops, p, k, ptr, rows), (model, dtype, k, "f32 call"))
    want = base.expected(pred, 256, sets, p["set_of"])
    assert np.isnan(want[1][want[0] >= 0]).any() and np.isinf(want[1]).any()
    # NaN comes last, by row; equal scores in ascending row order
    for q in range(p["Q"]):
        nan_q = np.isnan(want[1][q][want[0][q] >= 0])
        assert (np.diff(nan_q.astype(np.int8)) >= 0).all(), "no number after a NaN"
    q8 = np.nonzero(p["set_of"] == 8)[0]
    assert any(len(np.unique(pred[q, sets[8]])) < len(sets[8]) - 3 for q in q8), "duplicate rows must tie inside the set"
    tied = want[1][:, 1:].view(np.int32) == want[1][:, :-1].view(np.int32)
    tied &= (want[0][:, 1:] >= 0) & ~np.isnan(want[1][:, 1:])
    assert tied.any() and (want[0][:, 1:][tied] > want[0][:, :-1][tied]).all()
    if model == "transe":  # the sign of zero comes back as the oracle's (blp_score_fwd's arithmetic on the widened rows)
        neg0 = want[1].view(np.int32) == np.int32(-2 ** 31)
        assert neg0[q0, :4].all() and set(sets[8][200:204]) <= set(want[0][q0, :5]), "no -0 score among the expected ones"
        got = base.run(ops, p, 256, ptr, rows, table=t16)[1].cpu().numpy()
        assert np.array_equal(got.view(np.int32) == np.int32(-2 ** 31), neg0)


# ------------------------------------------------------------------------------------------------ 3. filters
@both_dtypes
@pytest.mark.parametrize("model", ["transe", "complex"])
def test_filters(ops, oracle, model, dtype):
    N, D = N_ROWS, 128
    p, sets, ptr, rows = make(model, D, DTYPES[dtype], seed=31)
    t16 = dev16(p, DTYPES[dtype])
    pred = base.oracle_pred(oracle, p)
    Q, set_of = p["Q"], p["set_of"]
    rng = np.random.default_rng(34)
    k = 10

    def best_inside(q, n):  # the best rows of the query's set: a filter that removes them changes the answer
        s = sets[set_of[q]]
        return s[np.argsort(-pred[q, s], kind="stable")][:n]

    def outside(q, n):
        cand = np.setdiff1d(np.arange(N), sets[set_of[q]])
        return rng.choice(cand, min(n, len(cand)), replace=False)

    def both(filt_args, want, what, kk=k):
        got = base.run(ops, p, kk, ptr, rows, table=t16, filter=base.segment_filter(ops, *filt_args))
        base.check(got, want, (what, "oracle"))
        same(got, base.run(ops, p, kk, ptr, rows, filter=base.segment_filter(ops, *filt_args)), (what, "f32 call"))

    # (a) rows: the best members of the set, non-members, values outside the table; the best member exempt (exclude)
    segs = [base.unique_values(best_inside(q, 6), outside(q, 6), [-1, N + 3]) for q in range(Q)]
    exclude = np.array([s[0] for s in segs], np.int64)
    want = base.expected(pred, k, sets, set_of, removed=base.removed_mask(segs, exclude, None, N))
    plain = base.expected(pred, k, sets, set_of)
    no_ex = base.expected(pred, k, sets, set_of, removed=base.removed_mask(segs, None, None, N))
    assert not np.array_equal(want[0], plain[0]) and not np.array_equal(want[0], no_ex[0])
    has = np.array(SET_SIZES)[set_of] > 0
    assert (want[0][has, 0] == exclude[has]).all(), "exclude[q] in its own segment survives (it is the best member)"
    both((segs, exclude, None, 0), want, "rows")
    both((segs, None, None, 0), no_ex, "rows, nothing exempt")

    # (b) entity ids through an ent2idx with -1 entries
    ent2idx = rng.permutation(N + 200).astype(np.int64)
    ent2idx[ent2idx >= N] = -1
    row2id = np.full(N, -1, np.int64)
    row2id[ent2idx[ent2idx >= 0]] = np.nonzero(ent2idx >= 0)[0]
    no_row = np.nonzero(ent2idx < 0)[0]
    id_segs = [base.unique_values(row2id[best_inside(q, 6)], row2id[outside(q, 4)], no_row[:3], [N + 500, -2]) for q in range(Q)]
    id_ex = np.array([s[0] for s in id_segs], np.int64)
    want = base.expected(pred, k, sets, set_of, removed=base.removed_mask(id_segs, id_ex, ent2idx, N))
    assert not np.array_equal(want[0], plain[0])
    both((id_segs, id_ex, ent2idx, 0), want, "ids")

    # (c) a 5 000-entry segment; (d) a query whose filter leaves 3 rows of a 300-row set: -1 / NaN slots
    big = [np.zeros(0, np.int64) for _ in range(Q)]
    q_whole = int(np.nonzero(set_of == 9)[0][2])
    q_300 = int(np.nonzero(set_of == 10)[0][0])
    big[q_whole] = rng.permutation(6000)[:5000]     # 5 000 distinct values, those >= N name no row
    big[q_300] = sets[10][3:]
    for kk in (10, 256):
        want = base.expected(pred, kk, sets, set_of, removed=base.removed_mask(big, None, None, N))
        assert (want[0][q_300, :3] >= 0).all() and (want[0][q_300, 3:] == -1).all() and np.isnan(want[1][q_300, 3:]).all()
        assert (want[0][q_whole] != base.expected(pred, kk, sets, set_of)[0][q_whole]).any()
        both((big, None, None, 0), want, ("long segment", kk), kk)


# ------------------------------------------------------------------------------------------------ 4. shards
@both_dtypes
@pytest.mark.parametrize("model", ["transe", "simple"])
def test_two_candidate_shards_merge_to_the_unsharded_call(ops, oracle, model, dtype):
    N, D = N_ROWS, 128
    p, sets, ptr, rows = make(model, D, DTYPES[dtype], seed=41)
    t16 = dev16(p, DTYPES[dtype])
    pred = base.oracle_pred(oracle, p)
    segs = [base.unique_values(sets[g][np.argsort(-pred[q, sets[g]], kind="stable")][:4], [3, N - 2]) if len(sets[g]) else np.zeros(0, np.int64)
            for q, g in enumerate(p["set_of"])]
    assert 517 % 64 and any(s[0] < 517 <= s[-1] for s in sets if len(s)), "an unequal split inside a tile, a set across it"
    for k in (10, 192):
        whole = base.expected(pred, k, sets, p["set_of"], removed=base.removed_mask(segs, None, None, N))
        base.check(base.run(ops, p, k, ptr, rows, table=t16, filter=base.segment_filter(ops, segs, None, None, 0)), whole, (model, k))
        parts = []
        for lo, hi in ((0, 517), (517, N)):
            got = base.run(ops, p, k, ptr, rows, table=t16[lo:hi], row_base=lo, filter=base.segment_filter(ops, segs, None, None, lo))
            base.check(got, base.expected(pred[:, lo:hi], k, sets, p["set_of"], row_base=lo,
                                          removed=base.removed_mask(segs, None, None, hi - lo, lo)), (lo, hi, k))
            same(got, base.run(ops, p, k, ptr, rows, table=p["table"][lo:hi], row_base=lo,
                               filter=base.segment_filter(ops, segs, None, None, lo)), (lo, hi, k, "f32 call"))
            parts.append(got)
        assert (parts[0][0] == -1).any() and (parts[0][0][:, -1] >= 0).any()  # shards that hold fewer than k of a set's rows
        merged = ops.topk_merge(torch.cat((parts[0][0], parts[1][0]), 1), torch.cat((parts[0][1], parts[1][1]), 1), k)
        base.check(merged, whole, (model, k, "merged"))


# ------------------------------------------------------------------------------------------------ 5. the grid
@both_dtypes
@pytest.mark.parametrize("model", ["transe", "distmult"])
def test_result_does_not_depend_on_the_grid(ops, knobs, model, dtype):
    """The persistent grid forced to ONE workgroup (knob topk_sets_grid of the hooks build), to 7 and left at its default."""
    p, sets, ptr, rows = make(model, 64, DTYPES[dtype], seed=80)
    t16 = dev16(p, DTYPES[dtype])
    segs = [sets[g][:4] for g in p["set_of"]]
    filt = lambda: base.segment_filter(ops, segs, None, None, 0)
    try:
        for k in (5, 256):
            default = base.run(ops, p, k, ptr, rows, table=t16, filter=filt())
            same(default, base.run(ops, p, k, ptr, rows, filter=filt()), (model, dtype, k, "f32 call"))
            assert not torch.equal(default[0], base.run(ops, p, k, ptr, rows, table=t16)[0]), "the filter must bite"
            for grid in (1, 7):
                knobs("topk_sets_grid", grid)
                same(base.run(ops, p, k, ptr, rows, table=t16, filter=filt()), default, (model, dtype, k, grid))
            knobs("topk_sets_grid", 0)
    finally:
        knobs("topk_sets_grid", 0)


# ------------------------------------------------------------------------------------------------ 6. one long set
@both_dtypes
def test_one_long_set_takes_the_slab_path(ops, dtype):
    """300 001 rows x 128, one set of 200 000 rows, 4 queries: few queries against a long set are cut into slabs (S_max > 1
    partial lists per query, merged).  The yardstick is the f32 call on the widened table."""
    N, D, n_set = 300_001, 128, 200_000
    p, sets, ptr, rows = make("transe", D, DTYPES[dtype], seed=90, N=N, sizes=(n_set,), head_runs=(3,), tail_runs=(1,))
    t16 = dev16(p, DTYPES[dtype])
    one_list = ops.topk_sets_workspace_bytes("transe", D, 3, 1, 1, 64, 256)
    assert ops.topk_sets_workspace_bytes("transe", D, 3, 1, 1, n_set, 256) >= one_list + 4 * 256 * 8 * 100
    plain = base.run(ops, p, 256, ptr, rows)
    segs = [plain[0][q, 1:200:2].cpu().numpy() for q in range(4)]  # every second one of the 200 best rows
    want = base.run(ops, p, 256, ptr, rows, filter=base.segment_filter(ops, segs, None, None, 0))
    assert (want[0] >= 0).all() and not torch.equal(want[0], plain[0])
    same(base.run(ops, p, 256, ptr, rows, table=t16, filter=base.segment_filter(ops, segs, None, None, 0)), want, (dtype, 256))
    same(base.run(ops, p, 10, ptr, rows, table=t16), base.run(ops, p, 10, ptr, rows), (dtype, 10))


# ------------------------------------------------------------------------------------------------ 7. more than 2^31 bytes
def test_a_table_of_more_than_2_31_bytes(ops):
    """4 194 400 x 256 IEEE half = 2 147 532 800 bytes: the last rows start beyond 2^31 bytes.  Sets of <= 300 rows from the last
    1 000 rows and from the first; the yardstick is blp_topk_sets on those 2 000 rows, re-indexed as a small f32 table."""
    N, D, model = 4_194_400, 256, "transe"
    assert N * D * 2 > 2 ** 31
    table = torch.empty((N, D), dtype=torch.float16, device="cuda").normal_(0.0, 0.1)
    rng = np.random.default_rng(90)
    sets = [np.sort(rng.choice(1000, n, replace=False) + off).astype(np.int64)
            for n, off in ((300, N - 1000), (257, 0), (64, N - 1000), (1, N - 1), (300, 0))]
    sets[1] = np.sort(np.concatenate((sets[1][:128], rng.choice(1000, 129, replace=False) + N - 1000)))  # both ends in one set
    # the two ends as a small f32 table, by slices (torch's own index gather is not used on a tensor of this size)
    small = torch.cat((table[:1000], table[N - 1000:])).float()    # row i = table row i, or N - 2000 + i from 1 000 on
    re_index = lambda r: np.where(r < 1000, r, r - (N - 2000))      # ascending stays ascending: ties keep their order
    re_sets = [re_index(s) for s in sets]
    head_runs, tail_runs = (3, 0, 33, 1, 2), (2, 34, 0, 1, 4)
    p = base.make_problem(model, 2000, D, head_runs, tail_runs, seed=91)   # fixed rows index `small`
    p["table"] = small.cpu()
    ptr = np.concatenate(([0], np.cumsum([len(s) for s in sets]))).astype(np.int64)
    segs = [s[::9] for s in (sets[g] for g in p["set_of"])]
    re_segs = [re_index(s) for s in segs]
    for k, filtered in ((10, False), (256, False), (10, True)):
        want = base.run(ops, p, k, ptr, np.concatenate(re_sets), filter=base.segment_filter(ops, re_segs, None, None, 0) if filtered else None)
        got = base.run(ops, p, k, ptr, np.concatenate(sets), table=table, filter=base.segment_filter(ops, segs, None, None, 0) if filtered else None)
        got_rows = got[0].cpu().numpy()
        assert (got_rows >= N - 1000).any() and (got_rows[got_rows >= 0] < 1000).any(), "winners from both ends of the table"
        back = np.where(got_rows < 0, -1, re_index(got_rows))
        base.check((torch.from_numpy(back), got[1]), (want[0].cpu().numpy(), want[1].cpu().numpy()), (k, filtered))
        if k == 256:
            assert (got_rows == -1).any()
    assert not torch.equal(base.run(ops, p, 10, ptr, np.concatenate(re_sets))[0], want[0]), "the filter must bite"


# ------------------------------------------------------------------------------------------------ 8. a one-row table
@both_dtypes
def test_a_table_of_one_row(ops, dtype):
    for model in REL_MODELS:
        g = torch.Generator().manual_seed(3)
        table = (torch.randn(1, 64, generator=g) * 0.1).to(DTYPES[dtype]).float()
        p = dict(model=model, table=table, rel=torch.randn(2, 64, generator=g) * 0.1, fixed=np.zeros(3, np.int64),
                 rel_ids=np.array([0, 1, 1]), q_head=1, Q=3, qh=np.array([0, 1, 1]), qt=np.array([0, 1, 2]))
        ptr, rows = np.array([0, 1, 1]), np.array([0])   # set 0 = {row 0}, set 1 is empty and serves the last query
        for k in (1, 3):
            want = base.run(ops, p, k, ptr, rows)
            assert want[0][:2, 0].tolist() == [0, 0] and (want[0][:, 1:] == -1).all() and (want[0][2] == -1).all()
            t16 = table.to(DTYPES[dtype]).cuda()
            for tab in (t16, padded(t16)):   # row stride D (contiguous) and D + 8
                same(base.run(ops, p, k, ptr, rows, table=tab), want, (model, dtype, k, tab.stride(0)))


def test_a_16_bit_source_is_refused(ops):
    p, sets, ptr, rows = make("transe", 64, torch.float16, seed=5)
    t = lambda a: torch.as_tensor(a).cuda()
    t16 = dev16(p, torch.float16)
    args = (t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), p["q_head"], 5, t(ptr), t(rows), t(p["qh"]), t(p["qt"]))
    for source in (t16, p["table"].cuda().bfloat16()):
        with pytest.raises(TypeError):
            ops.topk_sets("transe", t16, source, *args)
    with pytest.raises(TypeError):
        ops.topk_sets("transe", p["table"].cuda().double(), p["table"].cuda(), *args)


# ------------------------------------------------------------------------------------------------ 9. threads
def test_two_threads_on_two_streams(ops):
    problems = []
    for i, (model, dtype) in enumerate((("transe", torch.float16), ("complex", torch.bfloat16))):
        p, sets, ptr, rows = make(model, 128, dtype, seed=70 + i)
        t = lambda a: torch.as_tensor(a).cuda()
        k = (10, 192)[i]
        args = (model, dev16(p, dtype), p["table"].cuda(), t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), p["q_head"], k,
                t(ptr), t(rows), t(p["qh"]), t(p["qt"]))
        single = ops.topk_sets(*args)
        same(single, ops.topk_sets(model, args[2], *args[2:]), model)
        problems.append((args, single))
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def worker(i):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for _ in range(5):
                    out = ops.topk_sets(*problems[i][0])
            stream.synchronize()
            results[i] = (out[0].cpu(), out[1].cpu())
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    for i in range(2):
        single = problems[i][1]
        assert torch.equal(results[i][0], single[0].cpu())
        assert torch.equal(results[i][1].view(torch.int32), single[1].cpu().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 10. predict_links_in_sets
@both_dtypes
@pytest.mark.parametrize("rel_model", REL_MODELS)
def test_predict_links_in_sets_on_a_16_bit_device_table_takes_the_fused_route(rel_model, dtype, monkeypatch):
    from blp_amd import ranking, utils
    g, f = golden(f"eval_toy_{rel_model}"), golden("filters_toy")
    table16 = torch.from_numpy(g["ent_emb"]).to(DTYPES[dtype])
    triples, ent2idx = torch.from_numpy(f["triples"]), torch.from_numpy(f["ent2idx"])
    graph = torch.from_numpy(f["graph_edges"])
    index = utils.FilterIndex(graph)
    model = base._model(rel_model, g["rel_w"])
    R, Q = g["rel_w"].shape[0], 2 * triples.shape[0]
    typed = ranking.relation_candidate_sets(graph, R, ent2idx)
    rng = np.random.default_rng(60)
    pools = ranking.CandidateSets([rng.choice(table16.shape[0], n, replace=False) for n in (0, 1, 7, table16.shape[0], 20)])
    pool_ids = torch.from_numpy(rng.integers(0, 5, Q))
    entities = torch.arange(table16.shape[0]) * 2 + 5
    cases = [("typed", typed, 3, {}), ("pools", pools, 5, dict(set_ids=pool_ids)), ("ids", pools, 4, dict(set_ids=pool_ids, entities=entities)),
             ("tail", pools, 300, dict(set_ids=pool_ids[Q // 2:], side="tail")), ("head", typed, 2, dict(side="head"))]
    cpu = {name: ranking.predict_links_in_sets(model, table16.float(), triples, k, sets, ent2idx, filter_index=index, **kw)
           for name, sets, k, kw in cases}
    dense, dense_calls = ranking._topk_sets_dense, []

    def no_dense(*a, **k):
        raise AssertionError("the dense route was taken on a 16-bit device table")

    def counted_dense(*a, **k):
        dense_calls.append(1)
        return dense(*a, **k)

    dev_model = base._model(rel_model, g["rel_w"]).cuda()
    for name, sets, k, kw in cases:
        if "set_ids" in kw:
            kw = dict(kw, set_ids=kw["set_ids"].cuda())
        # k = 300 is beyond blp_topk_sets_typed's k: the dense route by design
        monkeypatch.setattr(ranking, "_topk_sets_dense", counted_dense if k > 256 else no_dense)
        got = ranking.predict_links_in_sets(dev_model, table16.cuda(), triples, k, sets, ent2idx, filter_index=index, **kw)
        want = cpu[name]
        assert got[0].is_cuda and got[1].is_cuda and torch.equal(got[0].cpu(), want[0]), (name, dtype)
        nan = torch.isnan(want[1])
        assert torch.equal(torch.isnan(got[1].cpu()), nan), (name, dtype)
        assert torch.equal(got[1].cpu()[~nan].view(torch.int32), want[1][~nan].view(torch.int32)), (name, dtype)
    assert len(dense_calls) == 1
