"""Candidate sets shared between queries for TransE at any width on the MI355X (blp_rank_sets_wide through
blp_amd.ops.rank_sets_wide and ranking.rank_in_sets): counts EQUAL (int32, no tolerance) to the C oracle's scores counted inside
each query's set -- widths with a partial slab only (4), exactly one slab (64), a slab plus the smallest tail (68), several slabs
(128, 768, 1024) and 300 = 4 slabs + 32 + 8 + 4; set sizes around the 64-row wave tile and the 256-row workgroup tile; query
groups around the chunk of 16; more work units than persistent workgroups; filters inside and outside the set; ties, NaN / inf /
-0; candidate shards; f16 / bf16 tables; the fixed-width kernel as a second reference at 64 / 128 / 256; one larger shape
against blp_rank_lists; the Python route; workspace and output bounds; two threads on two streams."""
import threading

import numpy as np
import pytest
import torch

import test_gpu_rank_sets as base
from test_gpu_rank_sets import expected, make_problem, make_sets, oracle_pred, plant_true_rows, removed_mask, segment_filter, unique_values
from test_gpu_rank_sets16 import padded
from test_gpu_workspace_bounds import guard, three_fills  # noqa: F401  (guard: a fixture)

pytestmark = pytest.mark.gpu

C = 16  # kSetsWideChunk (blp_amd/csrc/rank_sets_wide.hip): queries per work unit
WIDTHS = (4, 64, 68, 128, 300, 768, 1024)
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}

N_SMALL = 301
SIZES_SMALL = (0, 1, 63, 64, 65, 257, 300, 301, 40, 40)      # about 10 sets over about 300 rows
HEADS_SMALL = (1, 3, 0, 5, 17, 0, 16, 1, 33, 0)              # 76 + 60 queries; set 0 is empty and has a query
TAILS_SMALL = (0, 5, 1, 0, 4, 0, 15, 17, 16, 2)

N_TILES = 700
SIZES_TILES = (0, 1, 63, 64, 65, 255, 256, 257, 600, 100, 100, 100)
HEADS_TILES = (1, 2, 1, 3, 0, 4, 17, 1, 18, 5, 0, 0)         # set 9: heads only, set 10: tails only, set 11: no query
TAILS_TILES = (1, 0, 2, 1, 3, 1, 2, 16, 5, 0, 5, 0)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


def t(a):
    return torch.as_tensor(a).cuda()


def run(ops, p, ptr, rows, table=None, source=None, row_base=0, filter=None, queries=None, fn=None):
    """ops.rank_sets_wide on the problem; queries = (lo, hi, q_head, qh, qt): a slice of the queries as a call of its own."""
    lo, hi, q_head, qh, qt = queries if queries is not None else (0, p["Q"], p["q_head"], p["qh"], p["qt"])
    src = p["table"].cuda() if source is None else source
    tab = src if table is None else table
    return (fn or ops.rank_sets_wide)("transe", tab, src, t(p["fixed"][lo:hi]), p["rel"].cuda(), t(p["rel_ids"][lo:hi]), q_head,
                                      t(p["true_row"][lo:hi]), t(ptr), t(rows), t(qh), t(qt), filter=filter, row_base=row_base).cpu().numpy()


def problem(N, D, sizes, heads, tails, seed):
    sets, ptr, rows = make_sets(N, sizes, seed=seed)
    p = make_problem("transe", N, D, heads, tails, seed=seed + 1)
    plant_true_rows(p, sets, seed=seed + 2)
    return p, sets, ptr, rows


@pytest.mark.parametrize("D", WIDTHS)
def test_widths(ops, oracle, D):
    p, sets, ptr, rows = problem(N_SMALL, D, SIZES_SMALL, HEADS_SMALL, TAILS_SMALL, seed=D)
    pred, true = oracle_pred(oracle, p)
    want = expected(pred, true, sets, p["set_of"])
    assert (want[:, 1] > want[:, 0]).any() and (want[p["set_of"] == 0] == 0).all() and want[:, 0].max() > 50
    assert np.array_equal(run(ops, p, ptr, rows), want), D
    h, Q, zeros = p["q_head"], p["Q"], np.zeros(len(SIZES_SMALL) + 1, np.int64)
    assert np.array_equal(run(ops, p, ptr, rows, queries=(0, h, h, p["qh"], zeros)), want[:h]), (D, "heads only")
    assert np.array_equal(run(ops, p, ptr, rows, queries=(h, Q, 0, zeros, p["qt"])), want[h:]), (D, "tails only")


@pytest.mark.parametrize("D", [68, 300])
def test_set_sizes_around_the_tiles(ops, oracle, D):
    p, sets, ptr, rows = problem(N_TILES, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=100 + D)
    pred, true = oracle_pred(oracle, p)
    want = expected(pred, true, sets, p["set_of"])
    assert (want[p["set_of"] == 0] == 0).all() and want[:, 0].max() > 256
    assert np.array_equal(run(ops, p, ptr, rows), want), D


@pytest.mark.parametrize("D", [68, 300])
def test_group_sizes_around_the_chunk(ops, oracle, D):
    heads = (1, C - 1, C, C + 1, 2 * C + 1, 0, 0, 0, 0, 0, C)
    tails = (0, 0, 0, 0, 0, 1, C - 1, C, C + 1, 2 * C + 1, C + 1)
    sizes = (65, 300, 64, 257, 130, 65, 300, 64, 257, 130, 70)
    p, sets, ptr, rows = problem(N_SMALL, D, sizes, heads, tails, seed=200 + D)
    pred, true = oracle_pred(oracle, p)
    assert np.array_equal(run(ops, p, ptr, rows), expected(pred, true, sets, p["set_of"])), D


def test_more_work_units_than_persistent_workgroups(ops, oracle, knobs):
    """D = 4, 2 400 small sets with one or two queries each: about 3 000 units, far above three workgroups per compute unit; the
    same counts with the grid forced to 1 and to 7 workgroups (knob rank_sets_grid of the hooks build)."""
    N, D, G = 64, 4, 2400
    rng = np.random.default_rng(7)
    sizes = rng.integers(1, 9, G)
    heads, tails = (np.arange(G) % 2 == 0).astype(np.int64), (np.arange(G) % 4 != 0).astype(np.int64)
    p, sets, ptr, rows = problem(N, D, sizes, heads, tails, seed=8)
    pred, true = oracle_pred(oracle, p)
    want = expected(pred, true, sets, p["set_of"])
    units = int((heads > 0).sum() + (tails > 0).sum())
    assert units > 3 * torch.cuda.get_device_properties(0).multi_processor_count
    assert np.array_equal(run(ops, p, ptr, rows), want)
    for grid in (1, 7):
        knobs("rank_sets_grid", grid)
        assert np.array_equal(run(ops, p, ptr, rows), want), grid


@pytest.mark.parametrize("D", [68, 300])
def test_filters(ops, oracle, D):
    """Entries inside the set (subtracted), entries outside the set that score ABOVE the true key (a kernel that subtracted them
    would show), the true entity among the entries (exclude: never removed), out-of-range values, empty segments."""
    N = N_TILES
    p, sets, ptr, rows = problem(N, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=300 + D)
    pred, true = oracle_pred(oracle, p)
    Q, set_of = p["Q"], p["set_of"]
    rng = np.random.default_rng(301 + D)
    member = np.zeros((len(sets), N), bool)
    for g, s in enumerate(sets):
        member[g, s] = True

    def inside(q, n):
        s = sets[set_of[q]]
        return rng.choice(s, min(n, len(s)), replace=False) if len(s) else np.zeros(0, np.int64)

    def outside_above(q, n):
        return np.nonzero(~member[set_of[q]] & (pred[q] > true[q]))[0][:n]

    segs = [np.zeros(0, np.int64) if q % 4 == 0 else
            unique_values([p["true_row"][q]], inside(q, 9), outside_above(q, 6), rng.integers(0, N, 4), [-1, N + 3]) for q in range(Q)]
    exclude = p["true_row"].astype(np.int64)
    removed = removed_mask(segs, exclude, None, N)
    want = expected(pred, true, sets, set_of, removed=removed)
    assert (want[:, 3] < want[:, 1]).any() and (want[:, 2] < want[:, 0]).any()
    assert (want[::4, 2:] == want[::4, :2]).all()
    wrong = want[:, 0] - (removed & (pred > true[:, None])).sum(1)
    assert (wrong != want[:, 2]).any(), "subtracting entries outside the set must change the result"
    in_set = np.array([member[set_of[q], p["true_row"][q]] for q in range(Q)])
    assert in_set[np.arange(Q) % 4 != 0].any(), "a true entity inside its set must be among the filter entries somewhere"
    assert np.array_equal(run(ops, p, ptr, rows, filter=segment_filter(ops, segs, exclude, None, 0)), want), "rows"
    no_ex = expected(pred, true, sets, set_of, removed=removed_mask(segs, None, None, N))
    assert not np.array_equal(no_ex, want)
    assert np.array_equal(run(ops, p, ptr, rows, filter=segment_filter(ops, segs, None, None, 0)), no_ex), "rows, nothing exempt"
    # entity ids through an ent2idx with -1 entries
    ent2idx = rng.permutation(N + 200).astype(np.int64)
    ent2idx[ent2idx >= N] = -1
    row2id = np.full(N, -1, np.int64)
    row2id[ent2idx[ent2idx >= 0]] = np.nonzero(ent2idx >= 0)[0]
    id_segs = [unique_values(row2id[[p["true_row"][q]]], row2id[inside(q, 9)], row2id[outside_above(q, 4)], rng.integers(0, N + 200, 6),
                             [N + 500, -2]) for q in range(Q)]
    id_ex = row2id[p["true_row"]]
    want = expected(pred, true, sets, set_of, removed=removed_mask(id_segs, id_ex, ent2idx, N))
    assert np.array_equal(run(ops, p, ptr, rows, filter=segment_filter(ops, id_segs, id_ex, ent2idx, 0)), want), "ids"


@pytest.mark.parametrize("D", [68, 300])
def test_ties_and_special_values(ops, oracle, D):
    N = N_TILES
    p, sets, ptr, rows = problem(N, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=400 + D)
    table, g = p["table"], torch.Generator().manual_seed(401)
    dups = torch.randperm(N, generator=g)[:N // 20]                        # 5 % of the rows are copies of other rows ...
    table[dups] = table[torch.randint(0, N, (len(dups),), generator=g)]
    twins = torch.randperm(N, generator=g)[:40]                            # ... and 40 are bit-identical to some query's true entity
    table[twins] = table[torch.from_numpy(p["true_row"])[torch.randint(0, p["Q"], (40,), generator=g)]]
    special = sets[8][100:106]                                             # rows every query of the 600-row set meets
    table[special[0]] = float("nan")
    table[special[1], 3] = float("inf")
    table[special[2], 5] = float("-inf")
    table[special[3]] = 0.0
    table[special[4]] = -0.0
    table[special[5], ::2] = -0.0
    of_8 = np.nonzero(p["set_of"] == 8)[0]
    p["true_row"][of_8[0]], p["true_row"][of_8[1]] = special[0], special[3]  # a NaN true score; a zero row as the true entity
    p["fixed"][of_8[2]], p["fixed"][of_8[-1]] = special[0], special[1]       # NaN and inf in query rows, one on each side
    pred, true = oracle_pred(oracle, p)
    want = expected(pred, true, sets, p["set_of"])
    assert (want[:, 1] > want[:, 0] + 1).sum() >= 3, "ties beyond the true entity itself must occur"
    assert (want[of_8[0]] == 0).all() and (want[of_8[2]] == 0).all()
    assert np.array_equal(run(ops, p, ptr, rows), want), D


def test_two_candidate_shards_add_up(ops, oracle):
    N, D = N_TILES, 300
    p, sets, ptr, rows = problem(N, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=500)
    pred, true = oracle_pred(oracle, p)
    rng = np.random.default_rng(501)
    segs = [unique_values(rng.choice(sets[g], min(9, len(sets[g])), replace=False), rng.integers(0, N, 3)) if len(sets[g])
            else np.zeros(0, np.int64) for g in p["set_of"]]
    whole = expected(pred, true, sets, p["set_of"], removed=removed_mask(segs, None, None, N))
    assert np.array_equal(run(ops, p, ptr, rows, filter=segment_filter(ops, segs, None, None, 0)), whole)
    total = np.zeros_like(whole)
    cut = 333
    assert all((s < cut).any() and (s >= cut).any() for s in sets if len(s) > 60), "the shard boundary falls inside the sets"
    for lo, hi in ((0, cut), (cut, N)):
        got = run(ops, p, ptr, rows, table=p["table"][lo:hi].cuda(), row_base=lo, filter=segment_filter(ops, segs, None, None, lo))
        assert np.array_equal(got, expected(pred[:, lo:hi], true, sets, p["set_of"], row_base=lo,
                                            removed=removed_mask(segs, None, None, hi - lo, lo))), (lo, hi)
        total += got
    assert np.array_equal(total, whole)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("D", [68, 300, 768])
def test_16_bit_tables_equal_the_f32_call_on_the_widened_table(ops, oracle, D, dtype):
    dt = DTYPES[dtype]
    p, sets, ptr, rows = problem(N_TILES, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=600 + D)
    p["table"] = p["table"].to(dt).float()
    rng = np.random.default_rng(601)
    segs = [sets[g][:4] for g in p["set_of"]]
    filt = segment_filter(ops, segs, None, None, 0)
    t32 = p["table"].cuda()
    want = run(ops, p, ptr, rows, filter=filt)
    assert want[:, 0].max() > 100 and (want[:, 3] < want[:, 1]).any()
    if D == 300:  # the second reference: the C oracle on the widened table
        pred, true = oracle_pred(oracle, p)
        assert np.array_equal(want, expected(pred, true, sets, p["set_of"], removed=removed_mask(segs, None, None, N_TILES)))
    t16 = padded(p["table"].to(dt).cuda())  # ld = D + 8 > D, ld % 8 == 0
    assert t16.stride(0) == D + 8 and torch.equal(t16.float(), t32)
    assert np.array_equal(run(ops, p, ptr, rows, table=t16, source=t32, filter=filt), want), "padded rows"
    # a strided source (row stride D + 4), and a gathered one: the queries' fixed and true rows alone, in another order
    strided = torch.zeros((N_TILES, D + 4), device="cuda")[:, :D]
    strided.copy_(t32)
    assert strided.stride(0) == D + 4
    assert np.array_equal(run(ops, p, ptr, rows, table=t16, source=strided, filter=filt), want), "strided source"
    Q = p["Q"]
    order = rng.permutation(2 * Q)
    where = np.empty(2 * Q, np.int64)
    where[order] = np.arange(2 * Q)
    gathered = t32[t(np.concatenate((p["fixed"], p["true_row"]))[order])]
    q = dict(p, fixed=where[:Q], true_row=where[Q:])
    assert np.array_equal(run(ops, q, ptr, rows, table=t16, source=gathered, filter=filt), want), "gathered source"


@pytest.mark.parametrize("D", [64, 128, 256])
def test_fixed_width_kernel_agrees(ops, D):
    p, sets, ptr, rows = problem(N_TILES, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=700 + D)
    filt = segment_filter(ops, [sets[g][:5] for g in p["set_of"]], None, None, 0)
    want = run(ops, p, ptr, rows, filter=filt, fn=ops.rank_sets)
    assert want[:, 0].max() > 100 and (want[:, 3] < want[:, 1]).any()
    assert np.array_equal(run(ops, p, ptr, rows, filter=filt), want), D
    t16 = padded(p["table"].to(torch.bfloat16).cuda())
    src = t16.float().contiguous()
    assert np.array_equal(run(ops, p, ptr, rows, table=t16, source=src, filter=filt),
                          run(ops, p, ptr, rows, table=t16, source=src, filter=filt, fn=ops.rank_sets)), (D, "bf16")


def test_larger_shape_against_rank_lists(ops):
    """40 sets of 50 .. 2 000 rows (log-uniform) over a 5 000-row table at D = 300, 4 000 queries: the counts of blp_rank_lists
    on the expanded per-query lists -- two independent fused kernels that must agree."""
    N, D, G, Q = 5000, 300, 40, 4000
    rng = np.random.default_rng(50)
    sizes = np.exp(rng.uniform(np.log(50), np.log(2000), G)).astype(np.int64)
    sets, ptr, rows = make_sets(N, sizes, seed=51)
    q_head = Q // 2
    ids_h, ids_t = np.sort(rng.integers(0, G, q_head)), np.sort(rng.integers(0, G, Q - q_head))
    p = make_problem("transe", N, D, np.bincount(ids_h, minlength=G), np.bincount(ids_t, minlength=G), seed=52)
    plant_true_rows(p, sets, seed=53)
    filt = segment_filter(ops, [sets[g][:5] for g in p["set_of"]], None, None, 0)
    got = run(ops, p, ptr, rows, filter=filt)
    set_of, dev_ptr, dev_rows = t(p["set_of"]), t(ptr), t(rows)
    n_per = (dev_ptr[1:] - dev_ptr[:-1])[set_of]
    list_ptr = torch.zeros(Q + 1, dtype=torch.long, device="cuda")
    list_ptr[1:] = torch.cumsum(n_per, 0)
    owner = torch.repeat_interleave(torch.arange(Q, device="cuda"), n_per)
    list_row = dev_rows[dev_ptr[set_of][owner] + torch.arange(owner.shape[0], device="cuda") - list_ptr[owner]]
    table = p["table"].cuda()
    want, _ = ops.rank_lists("transe", table, table, t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), q_head, list_ptr, list_row,
                             true_row=t(p["true_row"]), filter=filt)
    want = want.cpu().numpy()
    assert (want[:, 3] < want[:, 1]).any() and want[:, 0].max() > 500
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", [300, 768])
def test_rank_in_sets_on_device_equals_its_cpu_route(D, dtype, monkeypatch):
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
    cases = [("typed", typed, {}), ("typed raw", typed, dict(add_true=False)), ("pools", pools, dict(set_ids=pool_ids)),
             ("pools raw", pools, dict(set_ids=pool_ids, add_true=False)), ("tail", pools, dict(set_ids=pool_ids[T:], side="tail"))]
    cpu_model = base._model("transe", rel_w)
    cpu = {name: ranking.rank_in_sets(cpu_model, table, triples, sets, ent2idx, filter_index=index, **kw) for name, sets, kw in cases}
    assert bool((cpu["typed raw"][:, 3] < cpu["typed raw"][:, 1]).any()), "the filter must bite somewhere"

    def no_dense(*a, **k):
        raise AssertionError("the dense route was taken on a device table")

    monkeypatch.setattr(ranking, "_rank_sets_dense", no_dense)
    dev_model = base._model("transe", rel_w).cuda()
    for name, sets, kw in cases:
        if "set_ids" in kw:
            kw = dict(kw, set_ids=kw["set_ids"].cuda())
        got = ranking.rank_in_sets(dev_model, table.cuda(), triples, sets, ent2idx, filter_index=index, **kw)
        assert got.is_cuda and torch.equal(got.cpu(), cpu[name]), (name, D, dtype)


@pytest.mark.parametrize("D,dtype", [(68, "f32"), (300, "f32"), (300, "f16"), (768, "bf16")])
def test_workspace_and_output_bounds(ops, oracle, guard, D, dtype):
    """A workspace of exactly the advertised size and outputs between guards, under the three fill patterns."""
    N = N_SMALL
    heads = (1, C, 0, C + 1, 2, 0, 5, 0, 0, 0)
    tails = (0, 1, C + 1, 0, C, 3, 0, 0, 0, 0)
    for name, hr, tr, sizes in (("both", heads, tails, SIZES_SMALL), ("heads only", heads, (0,) * 10, SIZES_SMALL),
                                ("tails only", (0,) * 10, tails, SIZES_SMALL), ("every set empty", heads, tails, (0,) * 10)):
        p, sets, ptr, rows = problem(N, D, sizes, hr, tr, seed=900 + D)
        if dtype == "f32":
            tab = src = p["table"].cuda()
        else:
            p["table"] = p["table"].to(DTYPES[dtype]).float()
            tab, src = padded(p["table"].to(DTYPES[dtype]).cuda()), p["table"].cuda()
        Q, qh = p["Q"], p["q_head"]
        pred, true = oracle_pred(oracle, p)
        segs = [sets[g][:4] for g in p["set_of"]]
        args = ("transe", tab, src, t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), qh, t(p["true_row"]), t(ptr), t(rows), t(p["qh"]), t(p["qt"]))
        need = ops.rank_sets_wide_workspace_bytes("transe", D, qh, Q - qh, len(sizes), tab.dtype)
        assert need > 0 and need % 256 == 0
        for filt, removed in ((None, None), (segment_filter(ops, segs, None, None, 0), removed_mask(segs, None, None, N))):
            what = (D, dtype, name, filt is not None)
            got, asked = three_fills(guard, lambda g: ops.rank_sets_wide(*args, filter=filt, out=g.out((Q, 4), torch.int32)), what)
            assert asked == [need], what
            assert np.array_equal(got[0].numpy(), expected(pred, true, sets, p["set_of"], removed=removed)), what


def test_two_threads_on_two_streams(ops, oracle):
    problems = []
    for i, D in enumerate((300, 68)):
        p, sets, ptr, rows = problem(N_TILES, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=950 + i)
        pred, true = oracle_pred(oracle, p)
        args = ("transe", p["table"].cuda(), p["table"].cuda(), t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), p["q_head"],
                t(p["true_row"]), t(ptr), t(rows), t(p["qh"]), t(p["qt"]))
        problems.append((args, expected(pred, true, sets, p["set_of"])))
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def worker(i):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                out = ops.rank_sets_wide(*problems[i][0])
            stream.synchronize()
            results[i] = out.cpu().numpy()
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    [th.start() for th in threads]
    [th.join() for th in threads]
    assert not errors, errors
    for i in range(2):
        assert np.array_equal(results[i], problems[i][1])
