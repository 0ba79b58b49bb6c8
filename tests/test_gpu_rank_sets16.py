"""Candidate sets on a 16-BIT entity table on the MI355X (blp_rank_sets_typed through blp_amd.ops.rank_sets and
ranking.rank_in_sets).  Every comparison is integer equality of counts, against two oracles: blp_rank_sets on the table widened
to f32 (every case; it shares everything after the tile with the kernel under test) and the C oracle's scores of the widened
table counted inside the sets on the host (one case per model and dtype, the filter, the shards, the special values).
Shapes: 1 031 rows (not a multiple of 64), row stride D + 8, set sizes around the 8-lane group, the 64-row wave tile and the
256-row workgroup tile, query runs around the 128-query chunk; one table of more than 2^31 bytes."""
import threading

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden
import test_gpu_rank_sets as base

pytestmark = pytest.mark.gpu

N_ROWS = 1031
SET_SIZES = (0, 1, 7, 63, 64, 65, 255, 256, 257, 1000, 300)   # set 0 is empty and has queries, set 10 has none
HEAD_RUNS = (1, 1, 127, 0, 128, 0, 1, 4, 0, 5, 0)
TAIL_RUNS = (2, 0, 0, 129, 0, 128, 0, 1, 3, 5, 0)
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def ops():
    from blp_amd import ops as _ops
    return _ops


def padded(table16):
    """The same rows with a row stride of D + 8 elements (ld > D, ld % 8 == 0)."""
    wide = torch.zeros((table16.shape[0], table16.shape[1] + 8), dtype=table16.dtype, device=table16.device)
    wide[:, :table16.shape[1]] = table16
    return wide[:, :table16.shape[1]]


def make(model, D, dtype, seed, N=N_ROWS):
    """A problem whose f32 table IS the 16-bit table widened: p["table"] (f32, host) and table16 (device, padded rows)."""
    sets, ptr, rows = base.make_sets(N, SET_SIZES, seed=seed)
    p = base.make_problem(model, N, D, HEAD_RUNS, TAIL_RUNS, seed=seed + 1)
    base.plant_true_rows(p, sets, seed=seed + 2)   # every third query's true entity in its set, the others anywhere
    p["table"] = p["table"].to(dtype).float()
    return p, sets, ptr, rows


def run(ops, p, ptr, rows, table, row_base=0, filter=None, queries=None):
    """ops.rank_sets with `table` (16-bit or f32, device; a shard if row_base > 0) and the widened f32 table as the source."""
    t = lambda a: torch.as_tensor(a).cuda()
    lo, hi, q_head, qh, qt = queries if queries is not None else (0, p["Q"], p["q_head"], p["qh"], p["qt"])
    return ops.rank_sets(p["model"], table, p["table"].cuda(), t(p["fixed"][lo:hi]), p["rel"].cuda(), t(p["rel_ids"][lo:hi]), q_head,
                         t(p["true_row"][lo:hi]), t(ptr), t(rows), t(qh), t(qt), filter=filter, row_base=row_base).cpu().numpy()


def dev16(p, dtype):
    t16 = padded(p["table"].to(dtype).cuda())
    assert t16.stride(0) == p["table"].shape[1] + 8 and torch.equal(t16.float().cpu(), p["table"])
    return t16


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("model,D", [(m, D) for m in REL_MODELS for D in (64, 128, 256)])
def test_counts_equal_the_f32_call_on_the_widened_table(ops, oracle, model, D, dtype):
    p, sets, ptr, rows = make(model, D, DTYPES[dtype], seed=D + 7)
    t16, t32 = dev16(p, DTYPES[dtype]), p["table"].cuda()
    want = run(ops, p, ptr, rows, t32)
    assert (want[:, 1] > want[:, 0]).any() and (want[p["set_of"] == 0] == 0).all() and want[:, 0].max() > 100
    if D == 128:  # the second oracle: the C reference's scores of the widened table, counted on the host
        pred, true = base.oracle_pred(oracle, p)
        assert np.array_equal(want, base.expected(pred, true, sets, p["set_of"])), (model, dtype)
    assert np.array_equal(run(ops, p, ptr, rows, t16), want), (model, D, dtype)
    h, Q, zeros = p["q_head"], p["Q"], np.zeros(len(SET_SIZES) + 1, np.int64)
    assert np.array_equal(run(ops, p, ptr, rows, t16, queries=(0, h, h, p["qh"], zeros)), want[:h]), (model, D, dtype, "heads only")
    assert np.array_equal(run(ops, p, ptr, rows, t16, queries=(h, Q, 0, zeros, p["qt"])), want[h:]), (model, D, dtype, "tails only")


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
def test_a_table_of_one_row(ops, dtype):
    for model in REL_MODELS:
        g = torch.Generator().manual_seed(3)
        table = (torch.randn(1, 64, generator=g) * 0.1).to(DTYPES[dtype]).float()
        p = dict(model=model, table=table, rel=torch.randn(2, 64, generator=g) * 0.1, fixed=np.zeros(3, np.int64),
                 rel_ids=np.array([0, 1, 1]), true_row=np.zeros(3, np.int64), q_head=1, Q=3, qh=np.array([0, 1, 1]), qt=np.array([0, 1, 2]))
        ptr, rows = np.array([0, 1, 1]), np.array([0])
        want = run(ops, p, ptr, rows, table.cuda())
        assert want[:2].tolist() == [[0, 1, 0, 1], [0, 1, 0, 1]] and (want[2] == 0).all()
        assert np.array_equal(run(ops, p, ptr, rows, padded(table.to(DTYPES[dtype]).cuda())), want), model


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("model", ["transe", "simple"])
def test_candidate_shards_add_up(ops, oracle, model, dtype):
    N, D = N_ROWS, 128
    p, sets, ptr, rows = make(model, D, DTYPES[dtype], seed=41)
    sets[10] = np.sort(np.random.default_rng(40).choice(300, 120, replace=False)).astype(np.int64)  # wholly outside the later shards
    ptr = np.concatenate(([0], np.cumsum([len(s) for s in sets]))).astype(np.int64)
    rows = np.concatenate(sets)
    p["qt"] = p["qt"].copy()
    p["qt"][10] -= 3   # set 10 serves no query of TAIL_RUNS: the last three tail queries of set 9 now belong to it
    p["set_of"] = np.concatenate((np.repeat(np.arange(11), np.diff(p["qh"])), np.repeat(np.arange(11), np.diff(p["qt"]))))
    pred, true = base.oracle_pred(oracle, p)
    rng = np.random.default_rng(44)
    segs = [base.unique_values(rng.choice(sets[g], min(9, len(sets[g])), replace=False), rng.integers(0, N, 3)) if len(sets[g])
            else np.zeros(0, np.int64) for g in p["set_of"]]
    whole = base.expected(pred, true, sets, p["set_of"], removed=base.removed_mask(segs, None, None, N))
    t16 = dev16(p, DTYPES[dtype])
    assert np.array_equal(run(ops, p, ptr, rows, t16, filter=base.segment_filter(ops, segs, None, None, 0)), whole)
    assert any(s[0] < 517 <= s[-1] for s in sets if len(s)), "a set must straddle a boundary"
    for cuts in ((0, 517, N), (0, 304, 776, N)):
        total = np.zeros_like(whole)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            filt = base.segment_filter(ops, segs, None, None, lo)
            got = run(ops, p, ptr, rows, t16[lo:hi], row_base=lo, filter=filt)
            assert np.array_equal(got, run(ops, p, ptr, rows, p["table"][lo:hi].cuda(), row_base=lo, filter=filt)), (lo, hi)
            assert np.array_equal(got, base.expected(pred[:, lo:hi], true, sets, p["set_of"], row_base=lo,
                                                     removed=base.removed_mask(segs, None, None, hi - lo, lo))), (lo, hi)
            if lo >= 304:
                assert (got[p["set_of"] == 10] == 0).all()
            total += got
        assert np.array_equal(total, whole), cuts


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("model", ["transe", "complex"])
def test_filters(ops, oracle, model, dtype):
    """Entries in the set, entries not in the set that beat the true entity (they must not subtract), the true entity excluded,
    an ent2idx with -1, a query left with 3 unfiltered rows, no filter."""
    N, D = N_ROWS, 128
    p, sets, ptr, rows = make(model, D, DTYPES[dtype], seed=31)
    pred, true = base.oracle_pred(oracle, p)
    t16, t32 = dev16(p, DTYPES[dtype]), p["table"].cuda()
    Q, set_of = p["Q"], p["set_of"]
    rng = np.random.default_rng(34)
    member = np.zeros((len(sets), N), bool)
    for g, s in enumerate(sets):
        member[g, s] = True

    def inside(q, n):
        s = sets[set_of[q]]
        return rng.choice(s, min(n, len(s)), replace=False) if len(s) else np.zeros(0, np.int64)

    def outside_above(q, n):
        return np.nonzero(~member[set_of[q]] & (pred[q] > true[q]))[0][:n]

    def check(filt_args, removed, what):
        want = base.expected(pred, true, sets, set_of, removed=removed)
        filt = None if filt_args is None else base.segment_filter(ops, *filt_args)
        got = run(ops, p, ptr, rows, t16, filter=filt)
        assert np.array_equal(got, want), what
        assert np.array_equal(got, run(ops, p, ptr, rows, t32, filter=filt)), what
        return want

    none = check(None, None, "no filter")
    assert np.array_equal(none[:, 2:], none[:, :2])
    # the true entity leads its segment and is excluded; members, non-members above the true key, values that name no row
    true_rows = p["true_row"]
    segs = [base.unique_values([true_rows[q]], inside(q, 9), outside_above(q, 6), rng.integers(0, N, 4), [-1, N + 3]) for q in range(Q)]
    exclude = np.array([s[0] for s in segs], np.int64)
    assert sum(len(outside_above(q, 6)) for q in range(Q)) > Q
    mask = base.removed_mask(segs, exclude, None, N)
    want = check((segs, exclude, None, 0), mask, "rows")
    assert (want[:, 3] < want[:, 1]).any() and (want[:, 2] < want[:, 0]).any()
    wrong = want[:, :2] - (mask & (pred > true[:, None])).sum(1)[:, None]
    assert (wrong[:, 0] != want[:, 2]).any(), "subtracting entries outside the set must change the result"
    kept = check((segs, None, None, 0), base.removed_mask(segs, None, None, N), "rows, the true entity not exempt")
    assert not np.array_equal(kept, want)
    # entity ids through an ent2idx with -1 entries
    ent2idx = rng.permutation(N + 200).astype(np.int64)
    ent2idx[ent2idx >= N] = -1
    row2id = np.full(N, -1, np.int64)
    row2id[ent2idx[ent2idx >= 0]] = np.nonzero(ent2idx >= 0)[0]
    id_segs = [base.unique_values(row2id[inside(q, 9)], row2id[outside_above(q, 4)], rng.integers(0, N + 200, 6), [N + 500, -2]) for q in range(Q)]
    id_ex = np.array([s[0] for s in id_segs], np.int64)
    check((id_segs, id_ex, ent2idx, 0), base.removed_mask(id_segs, id_ex, ent2idx, N), "ids")
    # a query of the 1 000-row set whose filter leaves 3 rows of it
    big = [np.zeros(0, np.int64) for _ in range(Q)]
    q3 = int(np.nonzero(set_of == 9)[0][0])
    big[q3] = sets[9][3:]
    mask = base.removed_mask(big, None, None, N)
    assert base.expected(np.ones_like(pred), np.zeros_like(true), sets, set_of, removed=mask)[q3, 3] == 3
    check((big, None, None, 0), mask, "three rows left")


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("model", ["transe", "complex"])
def test_special_values_and_duplicates(ops, oracle, model, dtype):
    D, dt = 128, DTYPES[dtype]
    p, sets, ptr, rows = make(model, D, dt, seed=21)
    table, g = p["table"], torch.Generator().manual_seed(24)
    dups = torch.randperm(N_ROWS, generator=g)[:N_ROWS // 20]            # 5 % of the rows are copies of other rows ...
    table[dups] = table[torch.randint(0, N_ROWS, (len(dups),), generator=g)]
    twins = torch.randperm(N_ROWS, generator=g)[:40]                     # ... and 40 are bit-identical to some query's true entity
    table[twins] = table[torch.from_numpy(p["true_row"])[torch.randint(0, p["Q"], (40,), generator=g)]]
    special = sets[9][100:107]                                           # rows every query of the 1 000-row set meets
    tiny = torch.finfo(dt).smallest_normal / 4                           # a 16-bit subnormal (exact in f32)
    table[special[0]] = float("nan")
    table[special[1], 3] = float("inf")
    table[special[2], 5] = float("-inf")
    table[special[3]] = 0.0
    table[special[4]] = -0.0
    table[special[5], ::2] = -0.0
    table[special[6], ::3] = tiny
    table[special[6], 1::3] = -tiny
    assert torch.equal(table.to(dt).float().nan_to_num(7.0), table.nan_to_num(7.0)) and float(torch.tensor(tiny).to(dt)) == tiny
    first_of_9 = int(np.nonzero(p["set_of"] == 9)[0][0])
    p["true_row"][first_of_9], p["true_row"][first_of_9 + 1] = special[0], special[6]  # a NaN true score; a subnormal row's
    in_set = np.array([p["true_row"][q] in set(sets[p["set_of"][q]].tolist()) for q in range(p["Q"])])
    assert in_set.any() and not in_set.all()
    pred, true = base.oracle_pred(oracle, p)
    want = base.expected(pred, true, sets, p["set_of"])
    assert (want[:, 1] > want[:, 0] + 1).sum() >= 3, "ties beyond the true entity itself must occur"
    assert (want[first_of_9] == 0).all()
    t16 = padded(table.to(dt).cuda())
    assert np.array_equal(run(ops, p, ptr, rows, t16), want), (model, dtype)
    assert np.array_equal(run(ops, p, ptr, rows, table.cuda()), want), (model, dtype, "f32")


@pytest.mark.parametrize("model", ["transe", "distmult"])
def test_counts_do_not_depend_on_the_grid(ops, knobs, model):
    p, sets, ptr, rows = make(model, 64, torch.float16, seed=80)
    segs = [sets[g][:4] for g in p["set_of"]]
    filt = lambda: base.segment_filter(ops, segs, None, None, 0)
    t16 = dev16(p, torch.float16)
    want = run(ops, p, ptr, rows, p["table"].cuda(), filter=filt())
    assert np.array_equal(run(ops, p, ptr, rows, t16, filter=filt()), want)
    for grid in (1, 7):
        knobs("rank_sets_grid", grid)
        assert np.array_equal(run(ops, p, ptr, rows, t16, filter=filt()), want), grid


def test_two_threads_on_two_streams(ops):
    problems = []
    for i, (model, dtype) in enumerate((("transe", torch.float16), ("complex", torch.bfloat16))):
        p, sets, ptr, rows = make(model, 128, dtype, seed=70 + i)
        t = lambda a: torch.as_tensor(a).cuda()
        src = p["table"].cuda()
        args = (t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), p["q_head"], t(p["true_row"]), t(ptr), t(rows), t(p["qh"]), t(p["qt"]))
        problems.append((model, dev16(p, dtype), src, args, ops.rank_sets(model, src, src, *args).cpu().numpy()))
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def worker(i):
        try:
            model, t16, src, args, _ = problems[i]
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for _ in range(5):
                    out = ops.rank_sets(model, t16, src, *args)
            stream.synchronize()
            results[i] = out.cpu().numpy()
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    for i in range(2):
        assert np.array_equal(results[i], problems[i][4])


def test_a_table_of_more_than_2_31_bytes(ops):
    """4 194 400 x 256 IEEE half = 2 147 532 800 bytes: the last rows start beyond 2^31 bytes.  Sets of <= 300 rows from the last
    1 000 rows and from the first; the oracle is blp_rank_sets on those 2 000 rows, re-indexed as a small f32 table."""
    N, D, model = 4_194_400, 256, "transe"
    assert N * D * 2 > 2 ** 31
    table = torch.empty((N, D), dtype=torch.float16, device="cuda").normal_(0.0, 0.1)
    rng = np.random.default_rng(90)
    sets = [np.sort(rng.choice(1000, n, replace=False) + off).astype(np.int64)
            for n, off in ((300, N - 1000), (257, 0), (64, N - 1000), (1, N - 1), (300, 0))]
    sets[1] = np.sort(np.concatenate((sets[1][:128], rng.choice(1000, 129, replace=False) + N - 1000)))  # both ends in one set
    # the two ends as a small f32 table, by slices (torch's own index gather is not used on a tensor of this size)
    small = torch.cat((table[:1000], table[N - 1000:])).float()    # row i = table row i, or N - 2000 + i from 1 000 on
    re_index = lambda rows: np.where(rows < 1000, rows, rows - (N - 2000))  # ascending stays ascending
    re_sets = [re_index(s) for s in sets]
    head_runs, tail_runs = (3, 0, 130, 1, 2), (2, 129, 0, 1, 4)
    p = base.make_problem(model, 2000, D, head_runs, tail_runs, seed=91)   # fixed / true rows index `small`
    p["table"] = small.cpu()
    ptr = np.concatenate(([0], np.cumsum([len(s) for s in sets]))).astype(np.int64)
    want = run(ops, p, ptr, np.concatenate(re_sets), small)
    assert want[:, 0].max() > 50
    got = run(ops, p, ptr, np.concatenate(sets), table)
    assert np.array_equal(got, want)
    segs = [s[:5] for s in (sets[g] for g in p["set_of"])]
    re_segs = [re_index(s) for s in segs]
    want = run(ops, p, ptr, np.concatenate(re_sets), small, filter=base.segment_filter(ops, re_segs, None, None, 0))
    assert (want[:, 3] < want[:, 1]).any()
    assert np.array_equal(run(ops, p, ptr, np.concatenate(sets), table, filter=base.segment_filter(ops, segs, None, None, 0)), want)


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("rel_model", REL_MODELS)
def test_rank_in_sets_on_a_16_bit_device_table_takes_the_fused_route(rel_model, dtype, monkeypatch):
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
    cases = [("typed", typed, {}), ("typed raw", typed, dict(add_true=False)), ("pools", pools, dict(set_ids=pool_ids)),
             ("pools raw", pools, dict(set_ids=pool_ids, add_true=False))]
    cpu = {name: ranking.rank_in_sets(model, table16.float(), triples, sets, ent2idx, filter_index=index, **kw) for name, sets, kw in cases}

    def no_dense(*a, **k):
        raise AssertionError("the dense route was taken on a 16-bit device table")

    monkeypatch.setattr(ranking, "_rank_sets_dense", no_dense)
    dev_model = base._model(rel_model, g["rel_w"]).cuda()
    for name, sets, kw in cases:
        got = ranking.rank_in_sets(dev_model, table16.cuda(), triples, sets, ent2idx, filter_index=index, **kw)
        assert got.is_cuda and torch.equal(got.cpu(), cpu[name]), (name, dtype)
