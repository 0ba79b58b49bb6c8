"""Filtered top-k inside shared candidate sets on the MI355X (blp_topk_sets through blp_amd.ops and
ranking.predict_links_in_sets): rows exact and scores bit-identical to the C oracle's scores of each query's set in numpy's
stable order -- set sizes and query runs around every tile and chunk boundary, ties and special values, filters, candidate
shards merged by blp_topk_merge, grid independence, a larger shape against blp_rank_lists, one long set in slabs, two threads
on two streams, and the device route of predict_links_in_sets against its CPU route."""
import threading

import numpy as np
import pytest
import torch

from conftest import REL_MODELS, golden

pytestmark = pytest.mark.gpu

SIDE_HEAD, SIDE_TAIL = 0, 1
N_ROWS = 1031
SET_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 1031, 300, 300)
# query runs around the chunk sizes topk_chunk(k) = 32 (k <= 96), 4 (k = 192) and 3 (k = 256); set 0 is empty and has queries
HEAD_RUNS = (1, 4, 0, 5, 32, 0, 33, 1, 97, 3, 0, 0)   # 2 and 10: tail queries only, 5 and 11: none
TAIL_RUNS = (2, 0, 3, 0, 7, 0, 1, 65, 31, 4, 6, 0)    # 1 and 3: head queries only
KS = (1, 5, 64, 192, 256)


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
    """Queries already grouped by set within each side."""
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(N, D, generator=g)
    table = torch.nn.functional.normalize(table, dim=-1) if model == "transe" else table * 0.1
    rel = (torch.rand(R, D, generator=g) - 0.5) * 0.25
    q_head, q_tail = int(sum(head_runs)), int(sum(tail_runs))
    Q = q_head + q_tail
    qh = np.concatenate(([0], np.cumsum(head_runs))).astype(np.int64)
    qt = np.concatenate(([0], np.cumsum(tail_runs))).astype(np.int64)
    set_of = np.concatenate((np.repeat(np.arange(len(head_runs)), head_runs), np.repeat(np.arange(len(tail_runs)), tail_runs)))
    return dict(model=model, table=table, rel=rel, fixed=torch.randint(0, N, (Q,), generator=g).numpy(),
                rel_ids=torch.randint(0, R, (Q,), generator=g).numpy(), q_head=q_head, Q=Q, qh=qh, qt=qt, set_of=set_of)


def oracle_pred(oracle, p):
    table = p["table"].numpy()
    f, r, h = table[p["fixed"]], p["rel"].numpy()[p["rel_ids"]], p["q_head"]
    parts = []
    if h:
        parts.append(oracle.score_all(p["model"], SIDE_HEAD, table, f[:h], r[:h]))
    if h < p["Q"]:
        parts.append(oracle.score_all(p["model"], SIDE_TAIL, table, f[h:], r[h:]))
    return np.concatenate(parts)


def expected(pred, k, sets, set_of, row_base=0, removed=None):
    """pred (Q, N) over the LOCAL table: for query q with set rows r (ascending) inside the shard the order is
    r[np.argsort(-pred[q, r], kind="stable")], removed entries dropped, -1 / NaN beyond what is left; rows come out global."""
    Q, N = pred.shape
    rows = np.full((Q, k), -1, np.int64)
    scores = np.full((Q, k), np.nan, np.float32)
    for q in range(Q):
        r = sets[set_of[q]] - row_base
        r = r[(r >= 0) & (r < N)]
        o = r[np.argsort(-pred[q, r], kind="stable")]
        if removed is not None:
            o = o[~removed[q, o]]
        o = o[:k]
        rows[q, :len(o)] = o + row_base
        scores[q, :len(o)] = pred[q, o]
    return rows, scores


def check(got, want, what=""):
    rows, scores = got[0].cpu().numpy(), got[1].cpu().numpy()
    want_rows, want_scores = want
    assert np.array_equal(rows, want_rows), what
    nan = np.isnan(want_scores)
    assert np.array_equal(np.isnan(scores), nan), what
    assert np.array_equal(scores[~nan].view(np.int32), want_scores[~nan].view(np.int32)), what


def run(ops, p, k, ptr, rows, table=None, row_base=0, filter=None, queries=None):
    """ops.topk_sets on the problem; queries = (lo, hi, q_head, qh, qt): a slice of the queries as a call of its own."""
    t = lambda a: torch.as_tensor(a).cuda()
    lo, hi, q_head, qh, qt = queries if queries is not None else (0, p["Q"], p["q_head"], p["qh"], p["qt"])
    source = p["table"].cuda()
    tab = source if table is None else table.cuda()
    return ops.topk_sets(p["model"], tab, source, t(p["fixed"][lo:hi]), p["rel"].cuda(), t(p["rel_ids"][lo:hi]), q_head, k, t(ptr),
                         t(rows), t(qh), t(qt), filter=filter, row_base=row_base)


def segment_filter(ops, lists, exclude, ent2idx, row_base):
    lo = np.cumsum([0] + [len(x) for x in lists[:-1]]).astype(np.int64)
    hi = lo + np.array([len(x) for x in lists], np.int64)
    values = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(1, np.int64)])
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.int64)).cuda()
    return ops.SegmentFilter(t(lo), t(hi), t(values), t(exclude), t(ent2idx), row_base)


def unique_values(*parts):
    """A filter segment: every value once (blp_filter's contract), first occurrence kept."""
    v = np.concatenate([np.asarray(p, np.int64).reshape(-1) for p in parts])
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


# ------------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("model,D", [(m, D) for m in REL_MODELS for D in (64, 128, 256)])
def test_rows_and_scores_match_the_oracle(ops, oracle, model, D):
    sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=D)
    p = make_problem(model, N_ROWS, D, HEAD_RUNS, TAIL_RUNS, seed=D + 1)
    pred = oracle_pred(oracle, p)
    h, Q, zeros = p["q_head"], p["Q"], np.zeros(len(SET_SIZES) + 1, np.int64)
    sizes = np.array(SET_SIZES)[p["set_of"]]
    for k in KS:
        want = expected(pred, k, sets, p["set_of"])
        # the inputs exercise k > |set| (-1 slots present, the empty set's queries entirely) and k < |set|
        assert (want[0][sizes < k, -1] == -1).all() and (sizes < k).any() and (want[0][sizes == 0] == -1).all()
        assert (want[0][sizes >= k] >= 0).all() and (sizes > k).any()
        check(run(ops, p, k, ptr, rows), want, (model, D, k))
        check(run(ops, p, k, ptr, rows, queries=(0, h, h, p["qh"], zeros)), (want[0][:h], want[1][:h]), (model, D, k, "heads only"))
        check(run(ops, p, k, ptr, rows, queries=(h, Q, 0, zeros, p["qt"])), (want[0][h:], want[1][h:]), (model, D, k, "tails only"))


# ------------------------------------------------------------------------------------------------ 2. ties, special values
@pytest.mark.parametrize("model", ["transe", "complex"])
def test_ties_and_special_values(ops, oracle, model):
    D = 128
    sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=21)
    p = make_problem(model, N_ROWS, D, HEAD_RUNS, TAIL_RUNS, seed=22)
    table, g = p["table"], torch.Generator().manual_seed(24)
    dups = torch.randperm(N_ROWS, generator=g)[:N_ROWS // 20]            # 5 % of the rows are copies of other rows ...
    table[dups] = table[torch.randint(0, N_ROWS, (dups.shape[0],), generator=g)]
    in_small = np.zeros(N_ROWS, bool)  # (set 9 is the whole table: "outside" means outside the sets below 1000 rows)
    in_small[np.concatenate([sets[g] for g in (1, 2, 3, 4, 5, 6, 7, 10, 11)])] = True
    outside = np.nonzero(~in_small)[0]
    # NaN / +inf / -inf in rows of the 63-, 64- and 255-row sets (they reach the tail of a k = 64 / 256 answer), of the
    # 1000-row set, and in rows outside every set but the whole table
    specials = ((float("nan"), (sets[2][10], sets[3][11], sets[5][7], sets[8][3], outside[1])),
                (float("inf"), (sets[2][20], sets[3][21], sets[8][40], outside[5])),
                (float("-inf"), (sets[2][30], sets[5][31], sets[8][77], outside[9])))
    for value, rows_at in specials:
        for r in rows_at:
            table[r, 5] = value
    table[sets[8][100]] = 0.0
    table[sets[8][101]] = -0.0
    table[sets[3][40], ::2] = -0.0
    # TransE with a zero relation against copies of the query's own fixed row: scores of exactly -0.0
    q0 = int(np.nonzero(p["set_of"] == 8)[0][0])
    p["rel"][0] = 0.0
    p["rel_ids"][q0] = 0
    table[sets[8][200:204]] = table[p["fixed"][q0]].clone()
    pred = oracle_pred(oracle, p)
    assert np.isnan(pred).any() and np.isinf(pred).any()
    for k in (5, 64, 256):
        want = expected(pred, k, sets, p["set_of"])
        check(run(ops, p, k, ptr, rows), want, (model, k))
    want = expected(pred, 256, sets, p["set_of"])
    assert np.isnan(want[1][want[0] >= 0]).any() and np.isinf(want[1]).any()
    q8 = np.nonzero(p["set_of"] == 8)[0]
    assert any(len(np.unique(pred[q, sets[8]])) < len(sets[8]) - 3 for q in q8), "duplicate rows must tie inside the set"
    if model == "transe":  # the sign of zero comes back as the oracle's
        neg0 = want[1].view(np.int32) == np.int32(-2 ** 31)
        # (the fixed row itself may be a member of the set: then it ties at -0 too, by its row)
        assert neg0[q0, :4].all() and set(sets[8][200:204]) <= set(want[0][q0, :5]), "no -0 score among the expected ones"
        got = run(ops, p, 256, ptr, rows)[1].cpu().numpy()
        assert np.array_equal(got.view(np.int32) == np.int32(-2 ** 31), neg0)


# ------------------------------------------------------------------------------------------------ 3. filters
@pytest.mark.parametrize("model", REL_MODELS)
def test_filters(ops, oracle, model):
    N, D = N_ROWS, 128
    sets, ptr, rows = make_sets(N, SET_SIZES, seed=31)
    p = make_problem(model, N, D, HEAD_RUNS, TAIL_RUNS, seed=32)
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
    for kk in (10, 256):
        want = expected(pred, kk, sets, set_of, removed=removed_mask(big, None, None, N))
        assert (want[0][q_300, :3] >= 0).all() and (want[0][q_300, 3:] == -1).all()
        assert (want[0][q_whole] != plain[0][q_whole]).any() if kk == 10 else True
        check(run(ops, p, kk, ptr, rows, filter=segment_filter(ops, big, None, None, 0)), want, ("long segment", kk))


# ------------------------------------------------------------------------------------------------ 4. shards
@pytest.mark.parametrize("model", ["transe", "simple"])
def test_two_candidate_shards_merge_to_the_unsharded_call(ops, oracle, model):
    N, D = N_ROWS, 128
    sets, ptr, rows = make_sets(N, SET_SIZES, seed=41)
    p = make_problem(model, N, D, HEAD_RUNS, TAIL_RUNS, seed=42)
    pred = oracle_pred(oracle, p)
    segs = [unique_values(sets[g][np.argsort(-pred[q, sets[g]], kind="stable")][:4], [3, N - 2]) if len(sets[g]) else np.zeros(0, np.int64)
            for q, g in enumerate(p["set_of"])]
    for k in (10, 192):
        whole = expected(pred, k, sets, p["set_of"], removed=removed_mask(segs, None, None, N))
        got_whole = run(ops, p, k, ptr, rows, filter=segment_filter(ops, segs, None, None, 0))
        check(got_whole, whole, (model, k))
        parts = []
        for lo, hi in ((0, 517), (517, N)):
            got = run(ops, p, k, ptr, rows, table=p["table"][lo:hi], row_base=lo, filter=segment_filter(ops, segs, None, None, lo))
            check(got, expected(pred[:, lo:hi], k, sets, p["set_of"], row_base=lo, removed=removed_mask(segs, None, None, hi - lo, lo)), (lo, hi, k))
            parts.append(got)
        assert (parts[0][0] == -1).any() and (parts[0][0][:, -1] >= 0).any()  # shards that hold fewer than k of a set's rows
        merged = ops.topk_merge(torch.cat((parts[0][0], parts[1][0]), 1), torch.cat((parts[0][1], parts[1][1]), 1), k)
        check(merged, whole, (model, k, "merged"))


# ------------------------------------------------------------------------------------------------ 5. the grid
@pytest.mark.parametrize("model", ["transe", "distmult"])
def test_result_does_not_depend_on_the_grid(ops, oracle, knobs, model):
    """The persistent grid forced to ONE workgroup (knob topk_sets_grid of the hooks build), to 7 and left at its default."""
    sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=80)
    p = make_problem(model, N_ROWS, 64, HEAD_RUNS, TAIL_RUNS, seed=81)
    pred = oracle_pred(oracle, p)
    segs = [sets[g][:4] for g in p["set_of"]]
    for k in (5, 256):
        want = expected(pred, k, sets, p["set_of"], removed=removed_mask(segs, None, None, N_ROWS))
        default = run(ops, p, k, ptr, rows, filter=segment_filter(ops, segs, None, None, 0))
        check(default, want, (model, k))
        for grid in (1, 7):
            knobs("topk_sets_grid", grid)
            got = run(ops, p, k, ptr, rows, filter=segment_filter(ops, segs, None, None, 0))
            assert torch.equal(got[0], default[0]) and torch.equal(got[1].view(torch.int32), default[1].view(torch.int32)), (grid, k)
        knobs("topk_sets_grid", 0)


# ------------------------------------------------------------------------------------------------ 6. a larger shape
def host_stable_topk(scores, list_ptr, list_row, removed, k):
    Q = len(list_ptr) - 1
    rows = np.full((Q, k), -1, np.int64)
    out = np.full((Q, k), np.nan, np.float32)
    for q in range(Q):
        a, b = list_ptr[q], list_ptr[q + 1]
        r, s = list_row[a:b], scores[a:b]
        o = np.argsort(-s, kind="stable")
        o = o[~removed[a:b][o]][:k]
        rows[q, :len(o)] = r[o]
        out[q, :len(o)] = s[o]
    return rows, out


@pytest.mark.parametrize("model", ["transe", "distmult"])
def test_larger_shape_against_rank_lists(ops, model):
    """64 sets of 50 .. 8 000 rows (log-uniform) over a 14 541-row table, 2 048 queries, k = 10, filtered: blp_rank_lists'
    scores of the expanded per-query lists in the host's stable order -- two independent fused kernels that must agree."""
    N, D, G, Q, k = 14_541, 128, 64, 2048, 10
    rng = np.random.default_rng(50)
    sizes = np.exp(rng.uniform(np.log(50), np.log(8000), G)).astype(np.int64)
    sets, ptr, rows = make_sets(N, sizes, seed=51)
    q_head = Q // 2
    ids_h, ids_t = np.sort(rng.integers(0, G, q_head)), np.sort(rng.integers(0, G, Q - q_head))
    p = make_problem(model, N, D, np.bincount(ids_h, minlength=G), np.bincount(ids_t, minlength=G), seed=52)
    assert np.array_equal(p["set_of"], np.concatenate((ids_h, ids_t)))
    segs = [sets[g][::7][:40] for g in p["set_of"]]
    filt = segment_filter(ops, segs, None, None, 0)
    got = run(ops, p, k, ptr, rows, filter=filt)
    t = lambda a: torch.as_tensor(a).cuda()
    set_of = t(p["set_of"])
    dev_ptr, dev_rows = t(ptr), t(rows)
    n_per = (dev_ptr[1:] - dev_ptr[:-1])[set_of]
    list_ptr = torch.zeros(Q + 1, dtype=torch.long, device="cuda")
    list_ptr[1:] = torch.cumsum(n_per, 0)
    owner = torch.repeat_interleave(torch.arange(Q, device="cuda"), n_per)
    list_row = dev_rows[dev_ptr[set_of][owner] + torch.arange(owner.shape[0], device="cuda") - list_ptr[owner]]
    table = p["table"].cuda()
    _, scores = ops.rank_lists(model, table, table, t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), q_head, list_ptr, list_row,
                               want_scores=True)
    list_ptr, list_row, scores = list_ptr.cpu().numpy(), list_row.cpu().numpy(), scores.cpu().numpy()
    removed = np.zeros(len(list_row), bool)
    for q in range(Q):
        a, b = list_ptr[q], list_ptr[q + 1]
        removed[a:b] = np.isin(list_row[a:b], segs[q])
    want = host_stable_topk(scores, list_ptr, list_row, removed, k)
    plain = host_stable_topk(scores, list_ptr, list_row, np.zeros_like(removed), k)
    assert not np.array_equal(want[0], plain[0]) and (want[0] >= 0).all()
    check(got, want, model)


# ------------------------------------------------------------------------------------------------ 7. one long set
def test_one_long_set_takes_the_slab_path(ops, oracle):
    """300 001 rows x 128, one set of 200 000 rows, 4 queries, k = 256: few queries against a long set are cut into slabs
    (S_max > 1 partial lists per query, merged)."""
    N, D, n_set, k = 300_001, 128, 200_000, 256
    sets, ptr, rows = make_sets(N, (n_set,), seed=90)
    p = make_problem("transe", N, D, (3,), (1,), seed=91)
    # the sizing: more than one partial list per query -- the workspace holds more than Q lists of k keys
    one_list = ops.topk_sets_workspace_bytes("transe", D, 3, 1, 1, 64, k)
    assert ops.topk_sets_workspace_bytes("transe", D, 3, 1, 1, n_set, k) >= one_list + 4 * k * 8 * 100
    pred = oracle_pred(oracle, p)
    segs = [sets[0][np.argsort(-pred[q, sets[0]], kind="stable")][1:200:2] for q in range(4)]
    want = expected(pred, k, sets, p["set_of"], removed=removed_mask(segs, None, None, N))
    check(run(ops, p, k, ptr, rows, filter=segment_filter(ops, segs, None, None, 0)), want)
    check(run(ops, p, 10, ptr, rows), expected(pred, 10, sets, p["set_of"]))


# ------------------------------------------------------------------------------------------------ 8. threads
def test_two_threads_on_two_streams(ops, oracle):
    problems = []
    for i, model in enumerate(("transe", "complex")):
        sets, ptr, rows = make_sets(N_ROWS, SET_SIZES, seed=70 + i)
        p = make_problem(model, N_ROWS, 128, HEAD_RUNS, TAIL_RUNS, seed=72 + i)
        pred = oracle_pred(oracle, p)
        t = lambda a: torch.as_tensor(a).cuda()
        k = (10, 192)[i]
        args = (model, p["table"].cuda(), p["table"].cuda(), t(p["fixed"]), p["rel"].cuda(), t(p["rel_ids"]), p["q_head"], k,
                t(ptr), t(rows), t(p["qh"]), t(p["qt"]))
        single = ops.topk_sets(*args)
        check(single, expected(pred, k, sets, p["set_of"]), model)
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


# ------------------------------------------------------------------------------------------------ 9. predict_links_in_sets
def _model(rel_model, rel_w):
    from blp_amd import models
    m = models.LinkPrediction(rel_w.shape[1], rel_model, "margin", rel_w.shape[0], 0)
    with torch.no_grad():
        m.rel_emb.weight.copy_(torch.from_numpy(rel_w))
    return m


@pytest.mark.parametrize("rel_model", REL_MODELS)
def test_predict_links_in_sets_on_device_equals_its_cpu_route(rel_model, monkeypatch):
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
    entities = torch.arange(table.shape[0]) * 2 + 5
    cases = [("typed", typed, 3, {}), ("pools", pools, 5, dict(set_ids=pool_ids)), ("ids", pools, 4, dict(set_ids=pool_ids, entities=entities)),
             ("tail", pools, 300, dict(set_ids=pool_ids[Q // 2:], side="tail")), ("head", typed, 2, dict(side="head"))]
    cpu = {name: ranking.predict_links_in_sets(model, table, triples, k, sets, ent2idx, filter_index=index, **kw)
           for name, sets, k, kw in cases}
    dense = ranking._topk_sets_dense
    dev_model = _model(rel_model, g["rel_w"]).cuda()

    def same(got, want, name):
        assert got[0].is_cuda and got[1].is_cuda and torch.equal(got[0].cpu(), want[0]), name
        nan = torch.isnan(want[1])
        assert torch.equal(torch.isnan(got[1].cpu()), nan) and torch.equal(got[1].cpu()[~nan].view(torch.int32), want[1][~nan].view(torch.int32)), name

    def no_dense(*a, **k):
        raise AssertionError("the dense route was taken on a device table")

    for fused in (True, False):
        if fused:
            monkeypatch.setattr(ranking, "_topk_sets_dense", no_dense)
        else:  # the fused route disabled: the dense route on device tensors
            monkeypatch.setattr(ranking, "_topk_sets_dense", dense)
            monkeypatch.setattr(ranking.ops, "topk_sets_supported", lambda *a, **k: False)
        for name, sets, k, kw in cases:
            if "set_ids" in kw:
                kw = dict(kw, set_ids=kw["set_ids"].cuda())
            if k > 256 and fused:
                continue  # beyond blp_topk_sets' k: the dense route by design
            for where in (sets, sets.to("cuda")):
                same(ranking.predict_links_in_sets(dev_model, table.cuda(), triples, k, where, ent2idx, filter_index=index, **kw), cpu[name], name)
