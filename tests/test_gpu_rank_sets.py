"""Candidate sets shared between queries on the MI355X (blp_rank_sets through blp_amd.ops.rank_sets and ranking.rank_in_sets):
counts EQUAL to the C oracle's scores counted inside the sets -- every model and width, set sizes around the 64-row wave tile
and the 256-row workgroup tile, query runs around kQB = 4 and the 128-query chunk, sets without queries and queries of the
empty set, ties, NaN / inf / -0, filters inside and outside the set, candidate shards, two threads on two streams, the
persistent grid forced to one workgroup, one larger shape against blp_rank_lists on the expanded lists."""
import threading

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden

pytestmark = pytest.mark.gpu

SIDE_HEAD, SIDE_TAIL = 0, 1
N_ROWS = 1031                                                          # not a multiple of 64
SET_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 1031, 300, 300)    # 1 031: the whole table
HEAD_RUNS = (1, 4, 0, 5, 128, 0, 129, 1, 300, 4, 0, 0)                 # queries per set: set 0 is empty and has queries, set 2 has
TAIL_RUNS = (0, 5, 1, 0, 4, 0, 1, 129, 128, 300, 5, 0)                 # tail queries only, 3 head only, 1 both, 5 and 11 none


@pytest.fixture(scope="module")
def ops():
    from blp_amd import ops as _ops
    return _ops


def make_sets(N, sizes, seed):
    rng = np.random.default_rng(seed)
    sets = [np.sort(rng.choice(N, n, replace=False)).astype(np.int64) for n in sizes]
    ptr = np.concatenate(([0], np.cumsum([len(s) for s in sets]))).astype(np.int64)
    return sets, ptr, np.concatenate(sets)


def make_problem(model, N, D, head_runs, tail_runs, seed, R=7):
    """Queries already grouped by set within each side; every third query's true entity is a row of its set (if it has one)."""
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(N, D, generator=g)
    table = torch.nn.functional.normalize(table, dim=-1) if model == "transe" else table * 0.1
    rel = (torch.rand(R, D, generator=g) - 0.5) * 0.25
    q_head, q_tail = sum(head_runs), sum(tail_runs)
    Q = q_head + q_tail
    qh = np.concatenate(([0], np.cumsum(head_runs))).astype(np.int64)
    qt = np.concatenate(([0], np.cumsum(tail_runs))).astype(np.int64)
    set_of = np.concatenate((np.repeat(np.arange(len(head_runs)), head_runs), np.repeat(np.arange(len(tail_runs)), tail_runs)))
    return dict(model=model, table=table, rel=rel, fixed=torch.randint(0, N, (Q,), generator=g).numpy(),
                rel_ids=torch.randint(0, R, (Q,), generator=g).numpy(), true_row=torch.randint(0, N, (Q,), generator=g).numpy(),
                q_head=q_head, Q=Q, qh=qh, qt=qt, set_of=set_of)


def plant_true_rows(p, sets, seed):
    rng = np.random.default_rng(seed)
    for q in range(0, p["Q"], 3):
        s = sets[p["set_of"][q]]
        if len(s):
            p["true_row"][q] = s[rng.integers(0, len(s))]


def oracle_pred(oracle, p):
    table = p["table"].numpy()
    f, r, h = table[p["fixed"]], p["rel"].numpy()[p["rel_ids"]], p["q_head"]
    parts = []
    if h:
        parts.append(oracle.score_all(p["model"], SIDE_HEAD, table, f[:h], r[:h]))
    if h < p["Q"]:
        parts.append(oracle.score_all(p["model"], SIDE_TAIL, table, f[h:], r[h:]))
    pred = np.concatenate(parts)
    return pred, pred[np.arange(p["Q"]), p["true_row"]]


def expected(pred, true, sets, set_of, row_base=0, removed=None):
    """Every (query, row) scored once by the oracle (pred, over the LOCAL table), counted inside the query's set on the host."""
    Q, N = pred.shape
    counts = np.zeros((Q, 4), np.int32)
    for q in range(Q):
        local = sets[set_of[q]] - row_base
        local = local[(local >= 0) & (local < N)]
        s = pred[q, local]
        keep = np.ones(len(s), bool) if removed is None else ~removed[q, local]
        with np.errstate(invalid="ignore"):
            gt, ge = s > true[q], s >= true[q]
        counts[q] = (gt.sum(), ge.sum(), (gt & keep).sum(), (ge & keep).sum())
    return counts


def run(ops, p, ptr, rows, table=None, row_base=0, filter=None, queries=None):
    """ops.rank_sets on the problem; queries = (lo, hi, q_head, qh, qt): a slice of the queries as a call of its own."""
    t = lambda a: torch.as_tensor(a).cuda()
    lo, hi, q_head, qh, qt = queries if queries is not None else (0, p["Q"], p["q_head"], p["qh"], p["qt"])
    source = p["table"].cuda()
    tab = source if table is None else table.cuda()
    return ops.rank_sets(p["model"], tab, source, t(p["fixed"][lo:hi]), p["rel"].cuda(), t(p["rel_ids"][lo:hi]), q_head,
                         t(p["true_row"][lo:hi]), t(ptr), t(rows), t(qh), t(qt), filter=filter, row_base=row_base).cpu().numpy()


@pytest.mark.parametrize("model,D", [(m, D) for m in REL_MODELS for D in (64, 128, 256)])
def test_counts_match_the_oracle(ops, oracle, model, D):
    sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=D)
    p = make_problem(model, N_ROWS, D, HEAD_RUNS, TAIL_RUNS, seed=D + 1)
    plant_true_rows(p, sets, seed=D + 2)
    pred, true = oracle_pred(oracle, p)
    want = expected(pred, true, sets, p["set_of"])
    assert (want[:, 1] > want[:, 0]).any() and (want[p["set_of"] == 0] == 0).all()
    assert np.array_equal(run(ops, p, ptr, rows), want), (model, D)
    # one side alone: q_head = Q (no tail query: every tail run empty) and q_head = 0
    h, Q, zeros = p["q_head"], p["Q"], np.zeros(len(SET_SIZES) + 1, np.int64)
    assert np.array_equal(run(ops, p, ptr, rows, queries=(0, h, h, p["qh"], zeros)), want[:h]), (model, D, "heads only")
    assert np.array_equal(run(ops, p, ptr, rows, queries=(h, Q, 0, zeros, p["qt"])), want[h:]), (model, D, "tails only")


@pytest.mark.parametrize("model", ["transe", "complex"])
def test_ties_and_special_values(ops, oracle, model):
    D = 128
    sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=21)
    p = make_problem(model, N_ROWS, D, HEAD_RUNS, TAIL_RUNS, seed=22)
    plant_true_rows(p, sets, seed=23)
    table, g = p["table"], torch.Generator().manual_seed(24)
    dups = torch.randperm(N_ROWS, generator=g)[:N_ROWS // 20]            # 5 % of the rows are copies of other rows ...
    table[dups] = table[torch.randint(0, N_ROWS, (len(dups),), generator=g)]
    twins = torch.randperm(N_ROWS, generator=g)[:40]                     # ... and 40 are bit-identical to some query's true entity
    table[twins] = table[torch.from_numpy(p["true_row"])[torch.randint(0, p["Q"], (40,), generator=g)]]
    special = sets[9][100:106]                                           # rows every query of the whole-table set meets
    table[special[0]] = float("nan")
    table[special[1], 3] = float("inf")
    table[special[2], 5] = float("-inf")
    table[special[3]] = 0.0
    table[special[4]] = -0.0
    table[special[5], ::2] = -0.0
    first_of_9 = int(np.nonzero(p["set_of"] == 9)[0][0])
    p["true_row"][first_of_9], p["true_row"][first_of_9 + 1] = special[0], special[3]  # a NaN true score; a zero one
    pred, true = oracle_pred(oracle, p)
    want = expected(pred, true, sets, p["set_of"])
    assert (want[:, 1] > want[:, 0] + 1).sum() >= 3, "ties beyond the true entity itself must occur"
    assert (want[first_of_9] == 0).all()
    assert np.array_equal(run(ops, p, ptr, rows), want), model


def segment_filter(ops, lists, exclude, ent2idx, row_base):
    lo = np.cumsum([0] + [len(x) for x in lists[:-1]]).astype(np.int64)
    hi = lo + np.array([len(x) for x in lists], np.int64)
    values = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(1, np.int64)])
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.int64)).cuda()
    return ops.SegmentFilter(t(lo), t(hi), t(values), t(exclude), t(ent2idx), row_base)


def unique_values(*parts):
    """One filter segment: a value occurs once per segment (blp_filter's contract), the first part's first value stays first."""
    v = np.concatenate([np.asarray(x, np.int64) for x in parts])
    return v[np.sort(np.unique(v, return_index=True)[1])]


def removed_mask(lists, exclude, ent2idx, N, row_base=0):
    out = np.zeros((len(lists), N), bool)
    for q, seg in enumerate(lists):
        for v in seg:
            if exclude is not None and v == exclude[q]:
                continue
            row = v if ent2idx is None else (ent2idx[v] if 0 <= v < len(ent2idx) else -1)
            row -= row_base
            if 0 <= row < N:
                out[q, row] = True
    return out


@pytest.mark.parametrize("model", ["transe", "complex"])
def test_filters(ops, oracle, model):
    """All four columns.  The expected counts remove a filter entry's row only inside the query's set (expected() looks the
    mask up at the set's rows only); entries outside the set that score ABOVE the true key are planted so that a kernel that
    subtracted them would show."""
    N, D = N_ROWS, 128
    sets, ptr, rows = make_sets(N, SET_SIZES, seed=31)
    p = make_problem(model, N, D, HEAD_RUNS, TAIL_RUNS, seed=32)
    plant_true_rows(p, sets, seed=33)
    pred, true = oracle_pred(oracle, p)
    Q, set_of = p["Q"], p["set_of"]
    rng = np.random.default_rng(34)
    member = np.zeros((len(sets), N), bool)
    for g, s in enumerate(sets):
        member[g, s] = True

    def inside(q, n):
        s = sets[set_of[q]]
        return rng.choice(s, min(n, len(s)), replace=False) if len(s) else np.zeros(0, np.int64)

    def outside_above(q, n):  # rows NOT in the set that beat the true entity
        cand = np.nonzero(~member[set_of[q]] & (pred[q] > true[q]))[0]
        return cand[:n]

    # (a) rows: members of the set, non-members above the true key, out-of-range values; one member exempt (exclude)
    segs = [unique_values(inside(q, 9), outside_above(q, 6), rng.integers(0, N, 4), [-1, N + 3]) for q in range(Q)]
    assert sum(len(outside_above(q, 6)) for q in range(Q)) > Q
    exclude = np.array([s[0] for s in segs], np.int64)
    want = expected(pred, true, sets, set_of, removed=removed_mask(segs, exclude, None, N))
    assert (want[:, 3] < want[:, 1]).any() and (want[:, 2] < want[:, 0]).any()
    wrong = want[:, :2] - removed_mask(segs, exclude, None, N).__and__(pred > true[:, None]).sum(1)[:, None]
    assert (wrong[:, 0] != want[:, 2]).any(), "subtracting entries outside the set must change the result"
    assert np.array_equal(run(ops, p, ptr, rows, filter=segment_filter(ops, segs, exclude, None, 0)), want), "rows"
    no_ex = expected(pred, true, sets, set_of, removed=removed_mask(segs, None, None, N))
    assert not np.array_equal(no_ex, want)
    assert np.array_equal(run(ops, p, ptr, rows, filter=segment_filter(ops, segs, None, None, 0)), no_ex), "rows, nothing exempt"

    # (b) entity ids through an ent2idx with -1 entries
    ent2idx = rng.permutation(N + 200).astype(np.int64)
    ent2idx[ent2idx >= N] = -1
    row2id = np.full(N, -1, np.int64)
    row2id[ent2idx[ent2idx >= 0]] = np.nonzero(ent2idx >= 0)[0]
    id_segs = [unique_values(row2id[inside(q, 9)], row2id[outside_above(q, 4)], rng.integers(0, N + 200, 6), [N + 500, -2]) for q in range(Q)]
    id_ex = np.array([s[0] for s in id_segs], np.int64)
    want = expected(pred, true, sets, set_of, removed=removed_mask(id_segs, id_ex, ent2idx, N))
    assert np.array_equal(run(ops, p, ptr, rows, filter=segment_filter(ops, id_segs, id_ex, ent2idx, 0)), want), "ids"

    # (c) a 5 000-entry segment; (d) a query whose filtered set keeps 3 rows; (e) a query that filters the whole table
    big = [np.zeros(0, np.int64) for _ in range(Q)]
    q_whole = int(np.nonzero(set_of == 9)[0][2])   # queries of the whole-table set and of a 300-row set
    q_300 = int(np.nonzero(set_of == 10)[0][0])
    q_1000 = int(np.nonzero(set_of == 8)[0][5])
    big[q_whole] = rng.permutation(6000)[:5000]     # 5 000 distinct values, those >= N name no row
    big[q_300] = sets[10][3:]
    big[q_1000] = np.arange(N)
    want = expected(pred, true, sets, set_of, removed=removed_mask(big, None, None, N))
    assert (want[q_1000, 2:] == 0).all() and want[q_1000, 1] > 0
    keeps3 = expected(np.ones_like(pred), np.zeros_like(true), sets, set_of, removed=removed_mask(big, None, None, N))
    assert keeps3[q_300, 3] == 3
    assert np.array_equal(run(ops, p, ptr, rows, filter=segment_filter(ops, big, None, None, 0)), want), "long segment"


@pytest.mark.parametrize("model", ["transe", "simple"])
def test_two_candidate_shards_add_up(ops, oracle, model):
    N, D = N_ROWS, 128
    sets, ptr, rows = make_sets(N, SET_SIZES, seed=41)
    p = make_problem(model, N, D, HEAD_RUNS, TAIL_RUNS, seed=42)
    plant_true_rows(p, sets, seed=43)
    pred, true = oracle_pred(oracle, p)
    rng = np.random.default_rng(44)
    segs = [unique_values(rng.choice(sets[g], min(9, len(sets[g])), replace=False), rng.integers(0, N, 3)) if len(sets[g])
            else np.zeros(0, np.int64) for g in p["set_of"]]
    whole = expected(pred, true, sets, p["set_of"], removed=removed_mask(segs, None, None, N))
    assert np.array_equal(run(ops, p, ptr, rows, filter=segment_filter(ops, segs, None, None, 0)), whole)
    total = np.zeros_like(whole)
    for lo, hi in ((0, 517), (517, N)):
        got = run(ops, p, ptr, rows, table=p["table"][lo:hi], row_base=lo, filter=segment_filter(ops, segs, None, None, lo))
        assert np.array_equal(got, expected(pred[:, lo:hi], true, sets, p["set_of"], row_base=lo,
                                            removed=removed_mask(segs, None, None, hi - lo, lo))), (lo, hi)
        total += got
    assert np.array_equal(total, whole)


@pytest.mark.parametrize("model", ["transe", "distmult"])
def test_larger_shape_against_rank_lists(ops, model):
    """474 sets of 50 .. 8 000 rows (log-uniform) over a 14 541-row table, 4 096 queries: the counts of blp_rank_lists on the
    expanded per-query lists -- two independent fused kernels that must agree."""
    N, D, G, Q = 14_541, 128, 474, 4096
    rng = np.random.default_rng(50)
    sizes = np.exp(rng.uniform(np.log(50), np.log(8000), G)).astype(np.int64)
    sets, ptr, rows = make_sets(N, sizes, seed=51)
    q_head = Q // 2
    ids_h, ids_t = np.sort(rng.integers(0, G, q_head)), np.sort(rng.integers(0, G, Q - q_head))
    p = make_problem(model, N, D, np.bincount(ids_h, minlength=G), np.bincount(ids_t, minlength=G), seed=52)
    plant_true_rows(p, sets, seed=53)
    assert np.array_equal(p["set_of"], np.concatenate((ids_h, ids_t)))
    segs = [sets[g][:5] for g in p["set_of"]]
    filt = segment_filter(ops, segs, None, None, 0)
    got = run(ops, p, ptr, rows, filter=filt)
    t = lambda a: torch.as_tensor(a).cuda()
    set_of = t(p["set_of"])
    dev_ptr, dev_rows = t(ptr), t(rows)
    n_per = (dev_ptr[1:] - dev_ptr[:-1])[set_of]
    list_ptr = torch.zeros(Q + 1, dtype=torch.long, device="cuda")
    list_ptr[1:] = torch.cumsum(n_per, 0)
    owner = torch.repeat_interleave(torch.arange(Q, device="cuda"), n_per)
    list_row = dev_rows[dev_ptr[set_of][owner] + torch.arange(owner.shape[0], device="cuda") - list_ptr[owner]]
    table = p["table"].cuda()
    want, _ = ops.rank_lists(model, table, table, t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), q_head, list_ptr, list_row,
                             true_row=t(p["true_row"]), filter=filt)
    want = want.cpu().numpy()
    assert (want[:, 3] < want[:, 1]).any() and want[:, 0].max() > 1000
    assert np.array_equal(got, want), model


def _model(rel_model, rel_w):
    from blp_amd import models
    m = models.LinkPrediction(rel_w.shape[1], rel_model, "margin", rel_w.shape[0], 0)
    with torch.no_grad():
        m.rel_emb.weight.copy_(torch.from_numpy(rel_w))
    return m


@pytest.mark.parametrize("rel_model", REL_MODELS)
def test_rank_in_sets_on_device_equals_its_cpu_route(rel_model, monkeypatch):
    from blp_amd import ranking, utils
    g, f = golden(f"eval_toy_{rel_model}"), golden("filters_toy")
    table, triples, ent2idx = torch.from_numpy(g["ent_emb"]), torch.from_numpy(f["triples"]), torch.from_numpy(f["ent2idx"])
    graph = torch.from_numpy(f["graph_edges"])
    index = utils.FilterIndex(graph)
    model = _model(rel_model, g["rel_w"])
    R, Q = g["rel_w"].shape[0], 2 * triples.shape[0]
    typed = ranking.relation_candidate_sets(graph, R, ent2idx)
    rng = np.random.default_rng(60)
    pools = ranking.CandidateSets([rng.choice(table.shape[0], n, replace=False) for n in (0, 1, 7, table.shape[0], 20)])
    pool_ids = torch.from_numpy(rng.integers(0, 5, Q))
    cases = [("typed", typed, {}), ("typed raw", typed, dict(add_true=False)), ("pools", pools, dict(set_ids=pool_ids)),
             ("pools raw", pools, dict(set_ids=pool_ids, add_true=False)), ("tail", pools, dict(set_ids=pool_ids[Q // 2:], side="tail"))]
    cpu = {name: ranking.rank_in_sets(model, table, triples, sets, ent2idx, filter_index=index, **kw) for name, sets, kw in cases}

    def no_dense(*a, **k):
        raise AssertionError("the dense route was taken on a device table")

    monkeypatch.setattr(ranking, "_rank_sets_dense", no_dense)
    dev_model = _model(rel_model, g["rel_w"]).cuda()
    for name, sets, kw in cases:
        if "set_ids" in kw:
            kw = dict(kw, set_ids=kw["set_ids"].cuda())
        for where in (sets, sets.to("cuda")):
            got = ranking.rank_in_sets(dev_model, table.cuda(), triples, where, ent2idx, filter_index=index, **kw)
            assert got.is_cuda and torch.equal(got.cpu(), cpu[name]), name
    dev_typed = ranking.relation_candidate_sets(graph.cuda(), R, ent2idx.cuda())
    assert dev_typed.rows.is_cuda and torch.equal(dev_typed.ptr.cpu(), typed.ptr) and torch.equal(dev_typed.rows.cpu(), typed.rows)


def test_two_threads_on_two_streams(ops, oracle):
    problems = []
    for i, model in enumerate(("transe", "complex")):
        sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=70 + i)
        p = make_problem(model, N_ROWS, 128, HEAD_RUNS, TAIL_RUNS, seed=72 + i)
        plant_true_rows(p, sets, seed=74 + i)
        pred, true = oracle_pred(oracle, p)
        t = lambda a: torch.as_tensor(a).cuda()
        args = (model, p["table"].cuda(), p["table"].cuda(), t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), p["q_head"],
                t(p["true_row"]), t(ptr), t(rows), t(p["qh"]), t(p["qt"]))
        problems.append((args, expected(pred, true, sets, p["set_of"])))
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def worker(i):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for _ in range(5):
                    out = ops.rank_sets(*problems[i][0])
            stream.synchronize()
            results[i] = out.cpu().numpy()
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    for i in range(2):
        assert np.array_equal(results[i], problems[i][1])


@pytest.mark.parametrize("model", ["transe", "distmult"])
def test_counts_do_not_depend_on_the_grid(ops, oracle, knobs, model):
    """The persistent grid forced to ONE workgroup (knob rank_sets_grid of the hooks build), to 7 and left at its default."""
    sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=80)
    p = make_problem(model, N_ROWS, 64, HEAD_RUNS, TAIL_RUNS, seed=81)
    plant_true_rows(p, sets, seed=82)
    pred, true = oracle_pred(oracle, p)
    segs = [sets[g][:4] for g in p["set_of"]]
    want = expected(pred, true, sets, p["set_of"], removed=removed_mask(segs, None, None, N_ROWS))
    default = run(ops, p, ptr, rows, filter=segment_filter(ops, segs, None, None, 0))
    assert np.array_equal(default, want)
    for grid in (1, 7):
        knobs("rank_sets_grid", grid)
        assert np.array_equal(run(ops, p, ptr, rows, filter=segment_filter(ops, segs, None, None, 0)), default), grid
