"""Candidate sets shared between queries for DistMult / ComplEx / SimplE at any width on the MI355X
(blp_rank_sets_wide_bilinear through blp_amd.ops.rank_sets_wide_bilinear and ranking.rank_in_sets): counts EQUAL (int32, no
tolerance) to the C oracle's score_all counted inside each query's set on the host (the oracle equals score_fn on CPU torch
bit for bit at these widths: tests/test_rank_sets_wide_bilinear_host.py) -- every branch of the sum order on tables whose
entries carry their own binary exponent; set sizes around the 64-entry trip and the 256-entry tile; query groups around the
chunk of 8; more work units than persistent workgroups; filters inside and outside the set; ties, NaN / inf / -0, an all-zero
table; three candidate shards; the fixed-width kernel as a second reference at 64 / 128 / 256; one larger shape against
blp_rank_all_wide on the gathered sets (300) and blp_rank_lists on the expanded lists (128); the Python route; workspace and output bounds; two threads on two streams."""
import threading

import numpy as np
import pytest
import torch

import test_gpu_rank_sets as base
from test_gpu_rank_sets import expected, make_problem, make_sets, oracle_pred, plant_true_rows, removed_mask, segment_filter, unique_values
from test_gpu_workspace_bounds import guard, three_fills  # noqa: F401  (guard: a fixture)

pytestmark = pytest.mark.gpu

BILINEAR = ("distmult", "complex", "simple")
C = 8       # kAwQueries (blp_amd/csrc/wide_bilinear.h): queries per work unit
TILE = 256  # kSetsWbTile (blp_amd/csrc/rank_sets_wide_bilinear.hip): entries of a set per work unit, 4 trips of 64

SUM_ORDER = [("distmult", D) for D in (4, 12, 36, 100, 300, 508, 512, 516, 768, 1024)] + \
            [(m, D) for m in ("complex", "simple") for D in (12, 20, 64, 300, 768, 1000, 1024)]
N_SMALL = 301
SIZES_SMALL = (0, 1, 15, 16, 17, 63, 64, 65, 257, 301)
HEADS_SMALL = (1, 3, 0, 5, 17, 0, 8, 1, 9, 0)               # set 0 is empty and has a query
TAILS_SMALL = (0, 5, 1, 0, 4, 0, 7, 9, 8, 2)

N_TILES = 700
SIZES_TILES = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600)   # around the trip (64) and the tile (256)
HEADS_TILES = (1, 2, 1, 3, 0, 4, 9, 1, 2, 5, 0, 3, 1, 10, 18)
TAILS_TILES = (1, 0, 2, 1, 3, 1, 2, 8, 5, 0, 5, 1, 3, 2, 11)
BIG = len(SIZES_TILES) - 1  # the 600-row set


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


def t(a):
    return torch.as_tensor(a).cuda()


def run(ops, p, ptr, rows, table=None, row_base=0, filter=None, queries=None, fn=None):
    """ops.rank_sets_wide_bilinear on the problem; queries = (lo, hi, q_head, qh, qt): a slice of the queries as a call of its own."""
    lo, hi, q_head, qh, qt = queries if queries is not None else (0, p["Q"], p["q_head"], p["qh"], p["qt"])
    src = p["table"].cuda()
    tab = src if table is None else table
    return (fn or ops.rank_sets_wide_bilinear)(p["model"], tab, src, t(p["fixed"][lo:hi]), p["rel"].cuda(), t(p["rel_ids"][lo:hi]), q_head,
                                               t(p["true_row"][lo:hi]), t(ptr), t(rows), t(qh), t(qt), filter=filter,
                                               row_base=row_base).cpu().numpy()


def spread(p, seed):
    """Every entry of the table and of the relations gets its own binary exponent over 2^-20 .. 2^20 (as scaled_problem of
    test_gpu_rank_all_wide.py): the terms of a sum differ by up to 2^120, so any reordering of the additions changes low bits."""
    g = torch.Generator().manual_seed(seed)
    for name in ("table", "rel"):
        p[name] = p[name] * torch.exp2(torch.randint(-20, 21, p[name].shape, generator=g).float())


def problem(model, N, D, sizes, heads, tails, seed, scaled=False):
    sets, ptr, rows = make_sets(N, sizes, seed=seed)
    p = make_problem(model, N, D, heads, tails, seed=seed + 1)
    if scaled:
        spread(p, seed + 3)
    plant_true_rows(p, sets, seed=seed + 2)
    return p, sets, ptr, rows


@pytest.mark.parametrize("model,D", SUM_ORDER)
def test_every_branch_of_the_sum_order(ops, oracle, model, D):
    p, sets, ptr, rows = problem(model, N_SMALL, D, SIZES_SMALL, HEADS_SMALL, TAILS_SMALL, seed=D, scaled=True)
    pred, true = oracle_pred(oracle, p)
    want = expected(pred, true, sets, p["set_of"])
    assert (want[:, 1] > want[:, 0]).any() and (want[p["set_of"] == 0] == 0).all() and want[:, 0].max() > 64
    assert np.array_equal(run(ops, p, ptr, rows), want), (model, D)
    h, Q, zeros = p["q_head"], p["Q"], np.zeros(len(SIZES_SMALL) + 1, np.int64)
    assert np.array_equal(run(ops, p, ptr, rows, queries=(0, h, h, p["qh"], zeros)), want[:h]), (model, D, "heads only")
    assert np.array_equal(run(ops, p, ptr, rows, queries=(h, Q, 0, zeros, p["qt"])), want[h:]), (model, D, "tails only")


@pytest.mark.parametrize("model", BILINEAR)
def test_set_sizes_around_the_trip_and_the_tile(ops, oracle, model):
    p, sets, ptr, rows = problem(model, N_TILES, 300, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=100)
    pred, true = oracle_pred(oracle, p)
    want = expected(pred, true, sets, p["set_of"])
    assert (want[p["set_of"] == 0] == 0).all() and want[:, 0].max() > TILE
    assert np.array_equal(run(ops, p, ptr, rows), want), model


@pytest.mark.parametrize("model", BILINEAR)
def test_group_sizes_around_the_chunk(ops, oracle, model):
    heads = (1, C - 1, C, C + 1, 2 * C + 1, 3, 0, 0)  # set 5: heads only, set 6: tails only, set 7: no query
    tails = (2 * C + 1, C + 1, C, C - 1, 1, 0, 3, 0)
    sizes = (65, 300, 64, 257, 130, 70, 70, 70)
    p, sets, ptr, rows = problem(model, N_SMALL, 300, sizes, heads, tails, seed=200)
    pred, true = oracle_pred(oracle, p)
    assert np.array_equal(run(ops, p, ptr, rows), expected(pred, true, sets, p["set_of"])), model


@pytest.mark.parametrize("model", BILINEAR)
def test_more_work_units_than_persistent_workgroups(ops, oracle, knobs, model):
    """D = 4, 2 400 small sets with one or two queries each: 3 000 units, far above two workgroups per compute unit; the same
    counts with the grid forced to 1 and to 7 workgroups (knob rank_sets_grid of the hooks build)."""
    N, D, G = 64, 4, 2400
    rng = np.random.default_rng(7)
    sizes = rng.integers(1, 9, G)
    heads, tails = (np.arange(G) % 2 == 0).astype(np.int64), (np.arange(G) % 4 != 0).astype(np.int64)
    p, sets, ptr, rows = problem(model, N, D, sizes, heads, tails, seed=8)
    pred, true = oracle_pred(oracle, p)
    want = expected(pred, true, sets, p["set_of"])
    units = int((heads > 0).sum() + (tails > 0).sum())
    assert units > 4 * torch.cuda.get_device_properties(0).multi_processor_count
    assert np.array_equal(run(ops, p, ptr, rows), want)
    for grid in (1, 7):
        knobs("rank_sets_grid", grid)
        assert np.array_equal(run(ops, p, ptr, rows), want), grid


@pytest.mark.parametrize("D", [68, 300])
@pytest.mark.parametrize("model", BILINEAR)
def test_filters(ops, oracle, model, D):
    """Entries inside the set (subtracted), entries outside the set that score ABOVE the true key (a kernel that subtracted them
    would show), the true entity among the entries (exclude: never removed), out-of-range values, empty segments; the filter's
    values as table rows and as entity ids through an ent2idx."""
    N = N_TILES
    p, sets, ptr, rows = problem(model, N, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=300 + D)
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


@pytest.mark.parametrize("D", [300, 768])
@pytest.mark.parametrize("model", BILINEAR)
def test_copies_of_the_true_row_inside_the_set_tie(ops, oracle, model, D):
    """Every query's true row is a row of its set, distinct from every other query's, and up to two more rows of the set are
    bit-identical copies of it: the pass must give a copy the very number the true-key routine gives the true row (ge, not gt),
    on both sides.  With the exponents spread over 2^40 nothing else ties."""
    p, sets, ptr, rows = problem(model, N_TILES, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=400 + D, scaled=True)
    rng = np.random.default_rng(401 + D)
    table, set_of = p["table"], p["set_of"]
    used = set(int(x) for x in p["fixed"])  # rows that stay as they are: the queries' own vectors, the true rows, the copies
    copies = np.zeros(p["Q"], np.int64)
    for q in np.argsort([len(sets[g]) for g in set_of], kind="stable"):  # the small sets choose first
        free = [int(r) for r in sets[set_of[q]] if int(r) not in used]
        if not free:
            p["true_row"][q] = p["fixed"][q]  # (a row of the table, most likely outside the set)
            continue
        picks = rng.permutation(free)[:3]
        p["true_row"][q] = picks[0]
        used.update(int(x) for x in picks)
        for r in picks[1:]:
            table[r] = table[picks[0]]
            copies[q] += 1
    in_set = np.array([p["true_row"][q] in sets[set_of[q]] for q in range(p["Q"])])
    assert copies.sum() > p["Q"] and in_set.sum() > p["Q"] // 2
    pred, true = oracle_pred(oracle, p)
    want = expected(pred, true, sets, set_of)
    assert np.array_equal(want[:, 1] - want[:, 0], copies + in_set)
    assert np.array_equal(run(ops, p, ptr, rows), want), (model, D)


@pytest.mark.parametrize("model", BILINEAR)
def test_special_values(ops, oracle, model):
    """NaN, +-inf and -0.0 in the table, in the queries' fixed rows and in the relations."""
    N, D = N_TILES, 300
    p, sets, ptr, rows = problem(model, N, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=450)
    table = p["table"]
    special = sets[BIG][100:106]                                             # rows every query of the 600-row set meets
    table[special[0]] = float("nan")
    table[special[1], 3] = float("inf")
    table[special[2], 5] = float("-inf")
    table[special[3]] = 0.0
    table[special[4]] = -0.0
    table[special[5], ::2] = -0.0
    p["rel"][0, 7] = float("inf")
    p["rel"][1, ::3] = -0.0
    p["rel"][2, D - 1] = float("nan")
    p["rel"][3, 1] = float("-inf")
    of_big = np.nonzero(p["set_of"] == BIG)[0]
    p["true_row"][of_big[0]], p["true_row"][of_big[1]] = special[0], special[3]  # a NaN true score; a zero row as the true entity
    p["fixed"][of_big[2]], p["fixed"][of_big[-1]] = special[0], special[1]       # NaN and inf in query rows, one on each side
    p["rel_ids"][of_big[3]] = 4                                                  # (a relation without special values)
    pred, true = oracle_pred(oracle, p)
    want = expected(pred, true, sets, p["set_of"])
    assert (want[of_big[0]] == 0).all() and (want[of_big[2]] == 0).all() and want[of_big[3], 0] > 0
    assert np.isnan(true).any() and np.isinf(pred).any()
    assert np.array_equal(run(ops, p, ptr, rows), want), model


@pytest.mark.parametrize("model", BILINEAR)
def test_all_zero_table_every_entry_ties(ops, model):
    p, sets, ptr, rows = problem(model, N_TILES, 300, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=470)
    p["table"] = torch.zeros_like(p["table"])
    got = run(ops, p, ptr, rows)
    sizes = np.array(SIZES_TILES)[p["set_of"]]
    assert np.array_equal(got, np.stack((0 * sizes, sizes, 0 * sizes, sizes), axis=1))


@pytest.mark.parametrize("model", BILINEAR)
def test_three_candidate_shards_add_up(ops, oracle, model):
    N, D = N_TILES, 300
    p, sets, ptr, rows = problem(model, N, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=500)
    cuts = (0, 233, 466, N)
    low = 9  # this set's rows all lie in the first shard: the other two hold no row of it
    sets[low] = np.sort(np.random.default_rng(502).choice(cuts[1], len(sets[low]), replace=False)).astype(np.int64)
    rows = np.concatenate(sets)
    plant_true_rows(p, sets, seed=503)
    assert HEADS_TILES[low] > 0 and (sets[low] < cuts[1]).all()
    pred, true = oracle_pred(oracle, p)
    rng = np.random.default_rng(501)
    segs = [unique_values(rng.choice(sets[g], min(9, len(sets[g])), replace=False), rng.integers(0, N, 3)) if len(sets[g])
            else np.zeros(0, np.int64) for g in p["set_of"]]
    whole = expected(pred, true, sets, p["set_of"], removed=removed_mask(segs, None, None, N))
    assert np.array_equal(run(ops, p, ptr, rows, filter=segment_filter(ops, segs, None, None, 0)), whole)
    total = np.zeros_like(whole)
    assert all(((s >= a) & (s < b)).any() for g, s in enumerate(sets) if g != low and len(s) > 120
               for a, b in zip(cuts, cuts[1:])), "the cuts fall inside the other sets"
    for lo, hi in zip(cuts, cuts[1:]):
        got = run(ops, p, ptr, rows, table=p["table"][lo:hi].cuda(), row_base=lo, filter=segment_filter(ops, segs, None, None, lo))
        assert np.array_equal(got, expected(pred[:, lo:hi], true, sets, p["set_of"], row_base=lo,
                                            removed=removed_mask(segs, None, None, hi - lo, lo))), (lo, hi)
        if lo:
            assert (got[p["set_of"] == low] == 0).all()
        total += got
    assert np.array_equal(total, whole)


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("model", BILINEAR)
def test_fixed_width_kernel_agrees(ops, model, D):
    p, sets, ptr, rows = problem(model, N_TILES, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=700 + D)
    filt = segment_filter(ops, [sets[g][:5] for g in p["set_of"]], None, None, 0)
    want = run(ops, p, ptr, rows, filter=filt, fn=ops.rank_sets)
    assert want[:, 0].max() > 100 and (want[:, 3] < want[:, 1]).any()
    assert np.array_equal(run(ops, p, ptr, rows, filter=filt), want), (model, D)


def _larger_shape(ops, model, D):
    """40 sets of 50 .. 8 000 rows (log-uniform) over a 14 541-row table, 2 000 queries, five members of its set in every
    query's filter."""
    N, G, Q = 14541, 40, 2000
    rng = np.random.default_rng(50)
    sizes = np.exp(rng.uniform(np.log(50), np.log(8000), G)).astype(np.int64)
    sets, ptr, rows = make_sets(N, sizes, seed=51)
    q_head = Q // 2
    ids_h, ids_t = np.sort(rng.integers(0, G, q_head)), np.sort(rng.integers(0, G, Q - q_head))
    p = make_problem(model, N, D, np.bincount(ids_h, minlength=G), np.bincount(ids_t, minlength=G), seed=52)
    plant_true_rows(p, sets, seed=53)
    filt = segment_filter(ops, [sets[g][:5] for g in p["set_of"]], None, None, 0)
    return p, sets, ptr, rows, filt


@pytest.mark.parametrize("model", BILINEAR)
def test_larger_shape_against_the_table_pass_on_gathered_sets(ops, model):
    """The larger shape at D = 300.  blp_rank_lists does not take these models at this width (rank_lists_supported: 64 / 128 /
    256), so the second fused kernel here is the whole-table pass: blp_rank_all_wide on each set's rows gathered into a table of
    their own, its group's queries with their true entities' vectors, the filter as a CSR of positions in that table.  The
    comparison with blp_rank_lists on the expanded lists is the next test, at a width it takes."""
    p, sets, ptr, rows, filt = _larger_shape(ops, model, 300)
    got = run(ops, p, ptr, rows, filter=filt)
    table, want, h = p["table"].cuda(), np.zeros_like(got), p["q_head"]
    for g, s in enumerate(sets):
        q = np.concatenate((np.arange(p["qh"][g], p["qh"][g + 1]), h + np.arange(p["qt"][g], p["qt"][g + 1])))
        if not len(q):
            continue
        n_f = min(5, len(s))  # the set is sorted: its first five rows are positions 0 .. 4 of the gathered table
        want[q] = ops.rank_all_wide(model, table[t(s)].contiguous(), table[t(p["fixed"][q])], p["rel"].cuda()[t(p["rel_ids"][q])],
                                    int(p["qh"][g + 1] - p["qh"][g]), q_true=table[t(p["true_row"][q])],
                                    filt_rowptr=t(np.arange(len(q) + 1, dtype=np.int64) * n_f),
                                    filt_col=t(np.tile(np.arange(n_f, dtype=np.int64), len(q)))).cpu().numpy()
    assert (want[:, 3] < want[:, 1]).any() and want[:, 0].max() > 500
    assert np.array_equal(got, want)


@pytest.mark.parametrize("model", BILINEAR)
def test_larger_shape_against_rank_lists(ops, model):
    """The same shape at D = 128, where blp_rank_lists takes these models: its counts on the expanded per-query lists -- two
    independent fused kernels that must agree."""
    p, sets, ptr, rows, filt = _larger_shape(ops, model, 128)
    Q, q_head = p["Q"], p["q_head"]
    got = run(ops, p, ptr, rows, filter=filt)
    set_of, dev_ptr, dev_rows = t(p["set_of"]), t(ptr), t(rows)
    n_per = (dev_ptr[1:] - dev_ptr[:-1])[set_of]
    list_ptr = torch.zeros(Q + 1, dtype=torch.long, device="cuda")
    list_ptr[1:] = torch.cumsum(n_per, 0)
    owner = torch.repeat_interleave(torch.arange(Q, device="cuda"), n_per)
    list_row = dev_rows[dev_ptr[set_of][owner] + torch.arange(owner.shape[0], device="cuda") - list_ptr[owner]]
    table = p["table"].cuda()
    want, _ = ops.rank_lists(model, table, table, t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), q_head, list_ptr, list_row,
                             true_row=t(p["true_row"]), filter=filt)
    want = want.cpu().numpy()
    assert (want[:, 3] < want[:, 1]).any() and want[:, 0].max() > 500
    assert np.array_equal(got, want)


def _evaluation(D, seed):
    from blp_amd import ranking, utils
    N, R, T = 200, 6, 60
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(N, D, generator=g) * 0.1
    rel_w = ((torch.rand(R, D, generator=g) - 0.5) * 0.25).numpy()
    ent2idx = torch.randperm(N + 20, generator=g)
    ent2idx[ent2idx >= N] = -1
    ids = torch.nonzero(ent2idx >= 0).reshape(-1)
    pick = lambda n: ids[torch.randint(0, N, (n,), generator=g)]
    graph = torch.stack((pick(400), pick(400), torch.randint(0, R, (400,), generator=g)), dim=1)
    triples = graph[:T]
    index = utils.FilterIndex(graph)
    typed = ranking.relation_candidate_sets(graph, R, ent2idx)
    rng = np.random.default_rng(seed + 1)
    pools = ranking.CandidateSets([rng.choice(N, n, replace=False) for n in (0, 1, 65, N, 20)])
    pool_ids = torch.from_numpy(rng.integers(0, 5, 2 * T))
    cases = [("typed", typed, {}), ("typed raw", typed, dict(add_true=False)), ("pools", pools, dict(set_ids=pool_ids)),
             ("pools raw", pools, dict(set_ids=pool_ids, add_true=False)), ("tail", pools, dict(set_ids=pool_ids[T:], side="tail"))]
    return table, rel_w, ent2idx, triples, index, cases


@pytest.mark.parametrize("model", BILINEAR)
def test_rank_in_sets_on_device_equals_its_cpu_route(model, monkeypatch):
    from blp_amd import ranking
    table, rel_w, ent2idx, triples, index, cases = _evaluation(300, 800)
    cpu_model = base._model(model, rel_w)
    cpu = {(name, filtered): ranking.rank_in_sets(cpu_model, table, triples, sets, ent2idx, filter_index=index if filtered else None, **kw)
           for name, sets, kw in cases for filtered in (True, False)}
    assert bool((cpu["typed raw", True][:, 3] < cpu["typed raw", True][:, 1]).any()), "the filter must bite somewhere"
    assert torch.equal(cpu["typed raw", False][:, 2:], cpu["typed raw", False][:, :2])

    def no_dense(*a, **k):
        raise AssertionError("the dense route was taken on a device table")

    monkeypatch.setattr(ranking, "_rank_sets_dense", no_dense)
    dev_model = base._model(model, rel_w).cuda()
    for name, sets, kw in cases:
        if "set_ids" in kw:
            kw = dict(kw, set_ids=kw["set_ids"].cuda())
        for filtered in (True, False):
            got = ranking.rank_in_sets(dev_model, table.cuda(), triples, sets, ent2idx, filter_index=index if filtered else None, **kw)
            assert got.is_cuda and torch.equal(got.cpu(), cpu[name, filtered]), (name, filtered, model)


def test_a_bf16_table_of_distmult_at_300_keeps_the_dense_route(ops, monkeypatch):
    from blp_amd import ranking
    table, rel_w, ent2idx, triples, index, cases = _evaluation(300, 820)
    dense, calls = ranking._rank_sets_dense, []

    def spy(*a, **k):
        calls.append(a[1].dtype)
        return dense(*a, **k)

    def no_fused(*a, **k):
        raise AssertionError("a 16-bit table went to the fused call")

    monkeypatch.setattr(ranking, "_rank_sets_dense", spy)
    monkeypatch.setattr(ops, "rank_sets_wide_bilinear", no_fused)
    name, sets, kw = cases[0]
    got = ranking.rank_in_sets(base._model("distmult", rel_w).cuda(), table.to(torch.bfloat16).cuda(), triples, sets, ent2idx,
                               filter_index=index, **kw)
    assert calls == [torch.bfloat16] and got.is_cuda and got.shape == (2 * triples.shape[0], 4) and got.dtype == torch.int32
    assert not ops.rank_sets_wide_bilinear_supported("distmult", 300, torch.bfloat16)


@pytest.mark.parametrize("model,D", [("distmult", 68), ("distmult", 300), ("complex", 300), ("simple", 768)])
def test_workspace_and_output_bounds(ops, oracle, guard, model, D):
    """A workspace of exactly the advertised size and outputs between guards, under the three fill patterns."""
    N = N_SMALL
    heads = (1, C, 0, C + 1, 2, 0, 5, 0, 0, 0)
    tails = (0, 1, C + 1, 0, C, 3, 0, 0, 0, 0)
    for name, hr, tr, sizes in (("both", heads, tails, SIZES_SMALL), ("heads only", heads, (0,) * 10, SIZES_SMALL),
                                ("tails only", (0,) * 10, tails, SIZES_SMALL), ("every set empty", heads, tails, (0,) * 10)):
        p, sets, ptr, rows = problem(model, N, D, sizes, hr, tr, seed=900 + D)
        tab = p["table"].cuda()
        Q, qh = p["Q"], p["q_head"]
        pred, true = oracle_pred(oracle, p)
        segs = [sets[g][:4] for g in p["set_of"]]
        args = (model, tab, tab, t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), qh, t(p["true_row"]), t(ptr), t(rows), t(p["qh"]), t(p["qt"]))
        need = ops.rank_sets_wide_bilinear_workspace_bytes(model, D, qh, Q - qh, len(sizes))
        assert need > 0 and need % 256 == 0
        for filt, removed in ((None, None), (segment_filter(ops, segs, None, None, 0), removed_mask(segs, None, None, N))):
            what = (model, D, name, filt is not None)
            got, asked = three_fills(guard, lambda g: ops.rank_sets_wide_bilinear(*args, filter=filt, out=g.out((Q, 4), torch.int32)), what)
            assert asked == [need], what
            assert np.array_equal(got[0].numpy(), expected(pred, true, sets, p["set_of"], removed=removed)), what


def test_two_threads_on_two_streams(ops, oracle):
    problems = []
    for i, (model, D) in enumerate((("complex", 300), ("distmult", 68))):
        p, sets, ptr, rows = problem(model, N_TILES, D, SIZES_TILES, HEADS_TILES, TAILS_TILES, seed=950 + i)
        pred, true = oracle_pred(oracle, p)
        args = (model, p["table"].cuda(), p["table"].cuda(), t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), p["q_head"],
                t(p["true_row"]), t(ptr), t(rows), t(p["qh"]), t(p["qt"]))
        problems.append((args, expected(pred, true, sets, p["set_of"])))
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def worker(i):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                out = ops.rank_sets_wide_bilinear(*problems[i][0])
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
