"""retrieval.py rerank without a GPU: the parsers, trec_eval's ndcg_cut as blp_amd.retrieval restates it (the worked example
and the edge cases of the contract), both restatements against plain references at the numeric and tie edges (the inputs
tests/test_gpu_rerank_edges.py runs on the device), the alpha selection rules, the C entry points' argument refusals (before any device is
touched), and the CLI end to end on a synthetic corpus against an independent restatement of the reference's loop."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from blp_amd import retrieval as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ndcg(run, qrels, cutoffs=(2, 100), alphas=(0.0,), s1=None):
    p = R.pack(run, {e: i for i, e in enumerate(sorted({e for r in run.values() for e in r}))}, qrels, cutoffs=cutoffs)
    s1 = np.zeros(len(p.cand_row), np.float32) if s1 is None else s1
    return p, R.trec_ndcg_cut(s1, p.s2, p.gain, p.cand_ptr, np.asarray(alphas), p.cutoffs, p.log2_table, p.idcg)


# ------------------------------------------------------------------------------------------------ an independent evaluator
def plain_ndcg(scores, rels, k):
    """nDCG@k of one query straight from the contract: {doc: score}, {doc: rel}."""
    docs = sorted(scores, key=lambda d: d.encode(), reverse=True)                 # docno descending ...
    docs = sorted(docs, key=lambda d: -float(np.float32(scores[d])))              # ... then score as a C float, stable
    dcg = 0.0
    for i, d in enumerate(docs[:k]):
        if rels.get(d, 0) > 0:
            dcg += rels[d] / math.log2(i + 2)
    ideal = sorted((r for r in rels.values() if r > 0), reverse=True)[:k]
    idcg = 0.0
    for i, r in enumerate(ideal):
        idcg += r / math.log2(i + 2)
    return dcg / idcg if idcg > 0 else 0.0


# ------------------------------------------------------------------------------------------------ parsers
def test_parsers(tmp_path):
    (tmp_path / "run").write_text("q1 Q0 <dbpedia:A> 1 3.5 bm25\nq1 Q0 <dbpedia:B> 2 2.25 bm25 extra\nq2 Q0 <dbpedia:C> 1 -1e-3 x\n")
    (tmp_path / "qrels").write_text("q1 0 <dbpedia:A> 2\nq1 0 <dbpedia:Z> 1\nq2 0 <dbpedia:C> -1\n")
    (tmp_path / "queries").write_text("q1\tfirst query\nq2\tsecond\tpart\n")
    (tmp_path / "folds").write_text(json.dumps({"0": {"training": ["q2"], "testing": ["q1"]},
                                                "1": {"training": ["q1"], "testing": ["q2"]}}))
    (tmp_path / "desc").write_text("<dbpedia:A>\tan entity\twith tabs\n<dbpedia:B>\tanother\n")
    run = R.read_run(tmp_path / "run")
    assert run == {"q1": {"<dbpedia:A>": 3.5, "<dbpedia:B>": 2.25}, "q2": {"<dbpedia:C>": -1e-3}}
    assert isinstance(run["q1"]["<dbpedia:A>"], float)
    qrels = R.read_qrels(tmp_path / "qrels")
    assert qrels == {"q1": {"<dbpedia:A>": 2, "<dbpedia:Z>": 1}, "q2": {"<dbpedia:C>": -1}}
    assert isinstance(qrels["q1"]["<dbpedia:A>"], int)
    assert R.read_queries(tmp_path / "queries") == {"q1": "first query", "q2": "second part"}
    assert list(R.read_folds(tmp_path / "folds")) == ["0", "1"]
    e2i, texts = R.read_descriptions(tmp_path / "desc")
    assert e2i == {"<dbpedia:A>": 0, "<dbpedia:B>": 1} and texts == ["an entity with tabs", "another"]


def test_pack_orders_segments_by_docno_and_keeps_insertion_order():
    run = {"q": {"b": 1.0, "zz": 2.0, "a": 3.0, "c": 0.5}}
    p = R.pack(run, {"a": 7, "b": 3}, {"q": {"zz": 1}})
    assert p.entities == [["zz", "c", "b", "a"]]
    assert p.cand_row.tolist() == [-1, -1, 3, 7]
    # the reference's insertion order: described entities first (b, a), then the others (zz, c)
    assert [p.entities[0][i] for i in p.order[0]] == ["b", "a", "zz", "c"]
    assert p.gain.tolist() == [1, 0, 0, 0] and p.s2.tolist() == [2.0, 0.5, 1.0, 3.0]


# ------------------------------------------------------------------------------------------------ the contract
def test_worked_example():
    run = {"q": {"A": 3.0, "B": 2.0, "C": 2.0, "D": 1.0}}
    qrels = {"q": {"A": 0, "B": 2, "C": 1, "E": 1}}
    _, nd = _ndcg(run, qrels)
    assert nd[0, 0, 0] == 0.23981246656813146
    assert nd[0, 0, 1] == 0.5209090851403014
    assert plain_ndcg(run["q"], qrels["q"], 2) == nd[0, 0, 0] and plain_ndcg(run["q"], qrels["q"], 100) == nd[0, 0, 1]


def test_f32_tie_breaks_by_docno():
    # 0.1 + 1e-9 and 0.1 differ as doubles but are the same C float: the docno decides ("y" before "x")
    assert np.float32(0.1 + 1e-9) == np.float32(0.1)
    run = {"q": {"x": 0.1 + 1e-9, "y": 0.1}}
    _, nd = _ndcg(run, {"q": {"x": 1}}, cutoffs=(1, 2))
    assert nd[0, 0, 0] == 0.0  # y ranks first
    _, nd = _ndcg(run, {"q": {"y": 1}}, cutoffs=(1, 2))
    assert nd[0, 0, 0] == 1.0
    # and a difference that survives the rounding is kept
    _, nd = _ndcg({"q": {"x": 0.1 + 1e-7, "y": 0.1}}, {"q": {"x": 1}}, cutoffs=(1, 2))
    assert nd[0, 0, 0] == 1.0


def test_unjudged_negative_unretrieved_and_short_lists():
    run = {"q": {"a": 5.0, "b": 4.0, "c": 3.0}}
    qrels = {"q": {"a": -1, "c": 2, "gone": 3}}  # a: negative (not relevant), b: unjudged, gone: relevant, never retrieved
    _, nd = _ndcg(run, qrels, cutoffs=(2, 1000))
    assert nd[0, 0, 0] == 0.0
    want = (2 / math.log2(4)) / (3 / math.log2(2) + 2 / math.log2(3))
    assert nd[0, 0, 1] == want == plain_ndcg(run["q"], qrels["q"], 1000)


def test_no_relevant_entity_and_empty_segment():
    run = {"q1": {"a": 1.0}, "q2": {}, "q3": {"b": 2.0}}
    qrels = {"q1": {"a": 0}, "q2": {"z": 1}, "q3": {"b": 1}}
    p, nd = _ndcg(run, qrels, cutoffs=(10,))
    assert nd[0, :, 0].tolist() == [0.0, 0.0, 1.0]
    assert p.evaluated.tolist() == [True, False, True]  # q2: no run entries -> not in the means


def test_alpha_mixes_cosine_and_run_scores():
    run = {"q": {"a": 1.0, "b": 0.0}}
    p = R.pack(run, {"a": 0, "b": 1}, {"q": {"b": 1}}, cutoffs=(1,))
    assert p.entities[0] == ["b", "a"]
    s1 = np.array([1.0, 0.0], np.float32)  # the cosine prefers b, the run prefers a
    nd = R.trec_ndcg_cut(s1, p.s2, p.gain, p.cand_ptr, np.array([0.0, 0.4, 0.6, 1.0]), p.cutoffs, p.log2_table, p.idcg)
    assert nd[:, 0, 0].tolist() == [0.0, 0.0, 1.0, 1.0]


def _toy_problem():
    run = {f"q{i}": {"a": 1.0, "b": 0.5} for i in range(4)}
    qrels = {f"q{i}": {"b": 1} for i in range(4)}
    p = R.pack(run, {"a": 0, "b": 1}, qrels, cutoffs=(10, 100))
    s1 = np.tile(np.array([1.0, -1.0], np.float32), 4)  # segment order (b, a): b is the cosine's favourite
    return p, s1


def test_alpha_selection_rules():
    p, s1 = _toy_problem()
    folds = {"f0": {"training": ["q0", "q1"], "testing": ["q2"]}, "f1": {"training": ["q2", "q3"], "testing": ["q0", "q1"]}}
    alphas = np.linspace(0, 1, 20)
    res = R.alpha_search(p, s1, alphas, folds)
    # ndcg is 1/log2(3) up to the first alpha that puts b first, 1 from there on: strict '>' keeps the FIRST best alpha
    first = next(i for i, a in enumerate(alphas) if np.float32(a * 1.0 + (1 - a) * 0.5) > np.float32(a * -1.0 + (1 - a) * 1.0))
    assert [f["alpha_index"] for f in res["folds"]] == [first, first]
    assert res["folds"][0]["train"] == 1.0 and res["folds"][0]["test"] == 1.0
    assert list(res["query_alpha"]) == ["q2", "q0", "q1"]


def test_all_zero_results_keep_the_first_alpha():
    run = {"q0": {"a": 1.0}, "q1": {"a": 2.0}}
    qrels = {"q0": {"z": 1}, "q1": {"z": 1}}  # relevant entities never retrieved: every result is 0
    p = R.pack(run, {"a": 0}, qrels)
    res = R.alpha_search(p, np.zeros(2, np.float32), np.array([0.3, 0.5, 0.9]), {"f": {"training": ["q0"], "testing": ["q1"]}})
    assert res["folds"][0]["alpha"] == 0.3 and res["folds"][0]["train"] == 0.0


def test_fold_mean_sums_in_strcmp_order():
    vals = [0.1, 0.7, 0.2, 1e-17, 0.3, 0.9, 1e16, 3.3, 0.25, 0.125]
    ids = [f"q{i}" for i in (3, 10, 1, 7, 22, 2, 5, 11, 4, 9)]
    order = sorted(range(len(ids)), key=lambda i: ids[i].encode())
    assert R.fold_mean(vals, ids) == np.mean([vals[i] for i in order])


def test_cosine_restated_rules():
    g = np.random.default_rng(0)
    table = g.standard_normal((5, 13)).astype(np.float32)
    table[3] = 0.0  # a zero row: the norm clamps to 1e-12, the cosine is 0
    queries = g.standard_normal((2, 13)).astype(np.float32)
    ptr = np.array([0, 3, 6])
    rows = np.array([0, -1, 3, 4, 2, 1], np.int32)
    s1 = R.cosine_restated(table, queries, ptr, rows)
    assert s1[1] == 0.0 and s1[2] == 0.0
    ref = torch.nn.functional.normalize(torch.from_numpy(table), dim=-1)[[0, 4, 2, 1]] @ \
        torch.nn.functional.normalize(torch.from_numpy(queries), dim=-1).T
    assert np.allclose(s1[[0, 3, 4, 5]], ref.numpy()[[0, 1, 2, 3], [0, 1, 1, 1]], atol=1e-6)
    assert np.isnan(R.cosine_restated(table, queries, ptr, np.array([0, 0, 0, 5, 0, 0], np.int32))[3])


@pytest.mark.skipif(not __import__("importlib").util.find_spec("pytrec_eval"), reason="pytrec_eval is not installed")
def test_trec_ndcg_cut_matches_pytrec_eval():
    import pytrec_eval
    g = np.random.default_rng(3)
    run = {f"q{q}": {f"d{i}": float(np.round(g.standard_normal(), 1)) for i in range(60)} for q in range(20)}
    qrels = {q: {f"d{i}": int(g.integers(-1, 3)) for i in g.choice(80, 15, replace=False)} for q in run}
    p, nd = _ndcg(run, qrels, cutoffs=(10, 100))
    got = pytrec_eval.RelevanceEvaluator(qrels, {"ndcg_cut_10", "ndcg_cut_100"}).evaluate(run)
    for i, q in enumerate(p.query_ids):
        assert abs(got[q]["ndcg_cut_10"] - nd[0, i, 0]) < 1e-12 and abs(got[q]["ndcg_cut_100"] - nd[0, i, 1]) < 1e-12


# ------------------------------------------------------------------------------------------------ plain references and edges
# The inputs below are built here, on the host, and tests/test_gpu_rerank_edges.py runs the kernels on exactly these.  The
# references use neither blp_amd.retrieval nor the device: Python floats and numpy float32 scalars, one candidate at a time.
F32_TINY = np.finfo(np.float32).tiny  # the smallest normal float32
CLAMP = np.float32(1e-12)             # F.normalize's eps as the kernel holds it


def ndcg_launch_shape(A, Q, max_segment):
    """(n_pad, T, PER, alphas per block, alpha blocks) of a rerank_ndcg launch, by launch_rerank_ndcg's formulas
    (blp_amd/csrc/rerank.hip)."""
    n_pad = 64
    while n_pad < max_segment:
        n_pad <<= 1
    T = min(max(n_pad >> 1, 64), 1024)
    apb = min(max((A * Q + 2047) // 2048, 1), A)
    return n_pad, T, n_pad // T, apb, -(-A // apb)


def plain_ndcg_cut(s1, s2, gain, cand_ptr, alphas, cutoffs, idcg):
    """blp_rerank_ndcg's contract as a loop per (alpha, query): (A, Q, n_cut) float64."""
    out = np.zeros((len(alphas), len(cand_ptr) - 1, len(cutoffs)))
    for a, alpha in enumerate(alphas):
        alpha = float(alpha)
        for q in range(len(cand_ptr) - 1):
            lo, hi = int(cand_ptr[q]), int(cand_ptr[q + 1])
            with np.errstate(over="ignore", invalid="ignore"):
                f = [float(np.float32(alpha * float(s1[i]) + (1.0 - alpha) * float(s2[i]))) for i in range(lo, hi)]
            # NaN last, then the C float descending (-0.0 == 0.0 as Python floats), then the lower index
            order = sorted(range(hi - lo), key=lambda i: (1, 0.0, i) if math.isnan(f[i]) else (0, -f[i], i))
            for j, k in enumerate(cutoffs):
                dcg = 0.0
                for r, i in enumerate(order[:k]):
                    if gain[lo + i] > 0:
                        dcg += int(gain[lo + i]) / math.log2(r + 2)
                out[a, q, j] = dcg / idcg[q][j] if idcg[q][j] > 0 else 0.0
    return out


def plain_idcg(rels, cutoffs):
    levels = sorted((int(r) for r in rels if r > 0), reverse=True)
    out = []
    for k in cutoffs:
        acc = 0.0
        for i, r in enumerate(levels[:k]):
            acc += r / math.log2(i + 2)
        out.append(acc)
    return out


def edge_segment():
    """(s1 f32, s2 f64, gain) of one 12-candidate segment: NaN, -0 before +0, two f32 denormals (the smaller first), +inf
    (NaN at alpha 0 and 1), -inf (NaN at alpha 1), 3e38 in both scores, an f32-only tie whose f64 order is the reverse of
    the index order, -1e-45, and an f64 score that overflows f32.  The gains are distinct, so every change of order
    changes the DCG at a cutoff past it."""
    inf, nan = np.inf, np.nan
    s1 = np.array([nan, -0.0, 0.0, 1e-42, 2e-42, inf, 0.0, 3e38, 1.0, 1.0, -1e-45, 0.0], np.float32)
    s2 = np.array([1.0, -0.0, 0.0, 1e-42, 2e-42, inf, -inf, 3e38, 1.0, 1.0 + 1e-9, -1e-45, 1e39], np.float64)
    gain = np.array([12, 2, 7, 3, 9, 4, 1, 6, 5, 11, 8, 10], np.int32)
    return s1, s2, gain


EDGE_ALPHAS = np.array([0.0, 0.25, 0.5, 1.0])
EDGE_CUTOFFS = (1, 2, 3, 5, 8, 12, 100)


def edge_floats(alpha):
    """The C floats the edge segment is ranked by at ``alpha`` (numpy float32 scalars)."""
    s1, s2, _ = edge_segment()
    with np.errstate(over="ignore", invalid="ignore"):
        return np.array([np.float32(alpha * float(a) + (1.0 - alpha) * float(b)) for a, b in zip(s1, s2)], np.float32)


def embed_edge_segment(seed=11):
    """The edge segment between ordinary ones (and an empty one): ptr, s1, s2, gain, the edge segment's query index."""
    g = np.random.default_rng(seed)
    lengths = [7, 0, 12, 70, 1]
    ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    s1 = g.uniform(-1, 1, ptr[-1]).astype(np.float32)
    s2 = g.uniform(5, 30, ptr[-1])
    gain = g.integers(-1, 4, ptr[-1]).astype(np.int32)
    s1[ptr[2]:ptr[3]], s2[ptr[2]:ptr[3]], gain[ptr[2]:ptr[3]] = edge_segment()
    return ptr, s1, s2, gain, 2


TIE_CUTOFFS = (3, 8192)


def tie_segments():
    """Segments whose keys all tie, so the index alone orders them: all NaN (100), all +inf at 0 < alpha < 1 (70), -0.0 and
    +0.0 mixed (130), all equal at the full length (8192).  Gains: distinct ones on the first 3 indices (DCG@3 is theirs
    alone only in index order) and on the last 10 (they take the last 10 ranks of DCG@8192 only in index order)."""
    g = np.random.default_rng(5)
    lengths = [100, 70, 130, 8192]
    ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    s1, s2 = np.zeros(ptr[-1], np.float32), np.zeros(ptr[-1], np.float64)
    s1[ptr[0]:ptr[1]], s2[ptr[0]:ptr[1]] = np.nan, 1.0
    s1[ptr[1]:ptr[2]], s2[ptr[1]:ptr[2]] = np.inf, np.inf
    signs = np.where(g.random(130) < 0.5, -0.0, 0.0)
    s1[ptr[2]:ptr[3]], s2[ptr[2]:ptr[3]] = signs, signs
    s1[ptr[3]:ptr[4]], s2[ptr[3]:ptr[4]] = 0.5, 0.5
    gain = np.zeros(ptr[-1], np.int32)
    for q in range(4):
        gain[ptr[q]:ptr[q] + 3] = (3, 1, 2)
        gain[ptr[q + 1] - 10:ptr[q + 1]] = g.permutation(10) + 1
    return ptr, s1, s2, gain


def plain_cosine_f64(table, queries, cand_ptr, cand_row):
    """x . y / (max(|x|, 1e-12) max(|y|, 1e-12)) in float64, one candidate at a time (rows >= 0 only)."""
    out = np.zeros(len(cand_row))
    for q in range(len(cand_ptr) - 1):
        y = queries[q].astype(np.float64)
        for c in range(int(cand_ptr[q]), int(cand_ptr[q + 1])):
            x = table[cand_row[c]].astype(np.float64)
            out[c] = float(x @ y) / (max(math.sqrt(float(x @ x)), 1e-12) * max(math.sqrt(float(y @ y)), 1e-12))
    return out


SWEEP_SCALES = (1.0, 2.0 ** -20, 2.0 ** 30)
SWEEP_LENGTHS = (3333, 1, 6000, 4000, 3000, 3666)


def sqrt_sweep(scale):
    """20 000 rows of six small integers times ``scale`` (a power of two) against one-hot queries: table, queries, ptr, rows,
    the integer sums of squares, and the expected cosines from numpy float32 scalar operations alone.  The squares and
    every partial sum of them are exact in f32 in any order, so the norm is the correctly rounded sqrt of a known float and
    the cosine is fl(x_j / n) * 1.0 plus zeros.  The first rows are perfect squares (k, 0, ...) and Pythagorean pairs."""
    g = np.random.default_rng(4)
    ints = g.integers(-40, 41, (20000, 6))
    squares = [[k, 0, 0, 0, 0, 0] for k in range(41)] + [[0, 3, 4, 0, 0, 0], [5, 0, -12, 0, 0, 0], [0, 0, 0, 8, 15, 0],
                                                          [7, 24, 0, 0, 0, 0], [20, 0, 0, 0, 0, -21], [2, 4, 4, 0, 0, 0]]
    ints[:len(squares)] = squares
    s = np.float32(scale)
    table = ints.astype(np.float32) * s
    queries = np.eye(6, dtype=np.float32)
    ptr = np.concatenate(([0], np.cumsum(SWEEP_LENGTHS))).astype(np.int64)
    rows = np.arange(20000, dtype=np.int32)
    sums = (ints * ints).sum(1)
    norm = np.sqrt(sums.astype(np.float32) * s * s)   # exact product, then numpy's correctly rounded f32 square root
    assert norm.dtype == np.float32
    norm = np.where(norm < CLAMP, CLAMP, norm)
    j = np.repeat(np.arange(6), SWEEP_LENGTHS)
    want = (table[rows, j] / norm) * np.float32(1.0) + np.float32(0.0)
    assert want.dtype == np.float32
    return table, queries, ptr, rows, sums, want


DEGENERATE_DIMS = (1, 13, 64, 70, 300)


def degenerate_rows(D):
    """{name: (D,) f32 row}: the rows at which a normalised dot product leaves ordinary arithmetic."""
    g = np.random.default_rng(100 + D)
    u, w = g.standard_normal(D), g.standard_normal(D)
    u, w = u / np.linalg.norm(u), w / np.linalg.norm(w)
    hot = np.zeros(D)
    hot[0] = 1.0
    below, above = np.nextafter(CLAMP, np.float32(0)), np.nextafter(CLAMP, np.float32(1))
    rows = {
        "u": u, "w": w, "hot": hot, "zero": np.zeros(D), "big": u * 1e18,
        "nan": np.where(np.arange(D) == D // 2, np.nan, u), "inf": np.where(np.arange(D) == D // 2, np.inf, w),
        "overflow": np.where(u < 0, -2e19, 2e19),  # every square overflows
        "u1e20": u * 1e20,                          # the sum of squares overflows
        "u1e-22": u * 1e-22,                        # denormal squares
        "u1e-30": u * 1e-30,                        # squares underflow to 0: the norm is 0, clamped
        "u1e-32": u * 1e-32, "w1e-32": w * 1e-32,   # clamped norms; the products of the normalised elements are denormal
        "below": u * 0.999e-12, "above": w * 1.001e-12,  # general rows on either side of the clamp
        "hot_below": hot * float(below), "hot_at": hot * float(CLAMP), "hot_above": hot * float(above),
    }
    with np.errstate(over="ignore"):
        return {k: v.astype(np.float32) for k, v in rows.items()}


def degenerate_cosine_problem(D):
    """Every degenerate row as a table row and as a query row, every pair a candidate (plus one row -1 per query):
    table, queries, ptr, rows, the row names."""
    named = degenerate_rows(D)
    names = list(named)
    table = np.stack([named[k] for k in names])
    n = len(names)
    ptr = np.arange(n + 1, dtype=np.int64) * (n + 1)
    rows = np.tile(np.concatenate((np.arange(n), [-1])), n).astype(np.int32)
    return table, table.copy(), ptr, rows, names


def test_plain_ndcg_reference_agrees_on_the_edge_segment():
    s1, s2, gain = edge_segment()
    f = edge_floats(0.5)
    # the segment reaches what it is for: the C floats tie where the doubles do not, -0 and +0, denormals, the overflow
    assert f[8] == f[9] and 0.5 * 1.0 + 0.5 * s2[8] < 0.5 * 1.0 + 0.5 * s2[9] and gain[8] != gain[9]
    assert np.signbit(f[1]) and f[1] == 0 and not np.signbit(f[2]) and f[2] == 0 and gain[1] != gain[2]
    assert 0 < f[3] < f[4] < F32_TINY and gain[3] != gain[4]
    assert np.isnan(f[0]) and f[5] == np.inf and f[6] == -np.inf and f[11] == np.inf and s2[11] > np.finfo(np.float32).max
    assert f[10] == -np.float32(1.4e-45) and np.isfinite(f[7]) and f[7] > 2.9e38
    assert np.isnan(edge_floats(0.0)[5]) and np.isnan(edge_floats(1.0)[6]) and edge_floats(1.0)[11] == 0
    ptr = np.array([0, 12])
    idcg = [plain_idcg(list(gain) + [3], EDGE_CUTOFFS)]
    want = plain_ndcg_cut(s1, s2, gain, ptr, EDGE_ALPHAS, EDGE_CUTOFFS, idcg)
    got = R.trec_ndcg_cut(s1, s2, gain, ptr, EDGE_ALPHAS, EDGE_CUTOFFS, R.log2_table(100), np.array(idcg))
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert idcg[0] == R.ideal_dcg(list(gain) + [3], EDGE_CUTOFFS, R.log2_table(100))
    # at alpha 0.5 the order is known by hand: +inf (5, 11 by index), 3e38, the f32 tie (8, 9 by index), the denormals
    # (the larger first), -0 == +0 by index, -1e-45, -inf, NaN
    order = [5, 11, 7, 8, 9, 4, 3, 1, 2, 10, 6, 0]
    dcg = 0.0
    for r, i in enumerate(order):
        dcg += int(gain[i]) / math.log2(r + 2)
    assert want[2, 0, 5] == dcg / idcg[0][5]


def test_plain_ndcg_reference_agrees_embedded_and_on_tie_segments():
    ptr, s1, s2, gain, _ = embed_edge_segment()
    idcg = np.array([plain_idcg(gain[ptr[q]:ptr[q + 1]], EDGE_CUTOFFS) for q in range(len(ptr) - 1)])
    want = plain_ndcg_cut(s1, s2, gain, ptr, EDGE_ALPHAS, EDGE_CUTOFFS, idcg)
    got = R.trec_ndcg_cut(s1, s2, gain, ptr, EDGE_ALPHAS, EDGE_CUTOFFS, R.log2_table(100), idcg)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    ptr, s1, s2, gain = tie_segments()
    alphas = np.array([0.25, 0.5])
    idcg = np.array([plain_idcg(gain[ptr[q]:ptr[q + 1]], TIE_CUTOFFS) for q in range(4)])
    want = plain_ndcg_cut(s1, s2, gain, ptr, alphas, TIE_CUTOFFS, idcg)
    got = R.trec_ndcg_cut(s1, s2, gain, ptr, alphas, TIE_CUTOFFS, R.log2_table(8192), idcg)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    for q in range(4):  # index order: DCG@3 holds the first three gains alone, in their order
        assert want[0, q, 0] == (3 / math.log2(2) + 1 / math.log2(3) + 2 / math.log2(4)) / idcg[q, 0]


@pytest.mark.parametrize("D", [1, 13, 64, 65, 70, 128, 300, 768])
def test_cosine_restated_close_to_plain_f64(D):
    g = np.random.default_rng(D)
    table = g.standard_normal((40, D)).astype(np.float32)
    table *= np.array([1.0, 1e-10, 1e15, 3.0], np.float32)[np.arange(40) % 4, None]  # no square under- or overflows
    queries = g.standard_normal((3, D)).astype(np.float32) * np.array([[1.0], [1e-8], [1e12]], np.float32)
    ptr = np.array([0, 40, 40, 120])
    rows = g.integers(0, 40, 120).astype(np.int32)
    got = R.cosine_restated(table, queries, ptr, rows)
    assert np.abs(got - plain_cosine_f64(table, queries, ptr, rows)).max() <= 1e-6


@pytest.mark.parametrize("D", DEGENERATE_DIMS)
def test_cosine_restated_rules_for_degenerate_rows(D):
    table, queries, ptr, rows, names = degenerate_cosine_problem(D)
    named = degenerate_rows(D)
    n = len(names)
    s = R.cosine_restated(table, queries, ptr, rows).reshape(n, n + 1)  # [query row, table row]
    assert (s[:, n] == 0).all() and not np.signbit(s[:, n]).any()      # row -1
    s = s[:, :n]
    at = names.index
    poisoned = [at("nan"), at("inf")]
    assert np.isnan(s[poisoned]).all() and np.isnan(s[:, poisoned]).all()  # a NaN element, one inf element: NaN
    clean = [i for i in range(n) if i not in poisoned]
    assert np.isfinite(s[np.ix_(clean, clean)]).all()
    for k in ("overflow", "u1e20"):  # the norm is inf, every element divides to 0: exactly +0.0 against a finite row
        with np.errstate(over="ignore"):
            assert np.isinf((named[k] * named[k]).sum())
        for v in (s[at(k), clean], s[clean, at(k)]):
            assert (v == 0).all() and not np.signbit(v).any()
    # the clamp: a norm below 1e-12f divides by exactly 1e-12f, one at or above it by itself
    v = {k: named[k][0] for k in ("hot_below", "hot_at", "hot_above")}
    norm = {k: np.sqrt(v[k] * v[k]) for k in v}
    assert norm["hot_below"] < CLAMP and norm["hot_at"] == CLAMP and norm["hot_above"] > CLAMP
    assert all(type(x) is np.float32 for x in norm.values())
    r = v["hot_below"] / CLAMP
    assert r < 1 and s[at("hot"), at("hot_below")] == r == s[at("hot_below"), at("hot")]
    assert s[at("hot_below"), at("hot_below")] == r * r
    assert s[at("hot"), at("hot_at")] == 1.0 == s[at("hot"), at("hot_above")] == s[at("hot_above"), at("hot_at")]
    assert np.linalg.norm(named["below"].astype(np.float64)) < 0.9995e-12
    assert np.linalg.norm(named["above"].astype(np.float64)) > 1.0005e-12
    assert abs(s[at("u"), at("below")] - 0.999) <= 1e-6  # 0.999e-12 u / 1e-12f against u
    assert abs(s[at("w"), at("above")] - 1.0) <= 1e-6    # above the clamp: divided by its own norm
    # denormal products: both norms clamp, (x_i / 1e-12f) * (y_i / 1e-12f) = 1e-40 u_i w_i
    x, y = named["u1e-32"] / CLAMP, named["w1e-32"] / CLAMP
    for k in ("u1e-32", "w1e-32", "u1e-30", "u1e-22"):
        assert np.linalg.norm(named[k].astype(np.float64)) < 1e-13
    prod = x * y
    assert prod.dtype == np.float32 and ((prod != 0) & (np.abs(prod) < F32_TINY)).any()
    got = s[at("u1e-32"), at("w1e-32")]  # [query, table row]: the sum of those products
    assert got != 0 and abs(got) < F32_TINY


@pytest.mark.parametrize("scale", SWEEP_SCALES)
def test_cosine_restated_square_root_sweep(scale):
    table, queries, ptr, rows, sums, want = sqrt_sweep(scale)
    assert sums.max() >= 7000 and len(np.unique(sums)) >= 4000  # of at most 6 * 40 * 40 = 9600
    roots = np.sqrt(sums.astype(np.float64))
    assert (roots == np.round(roots)).sum() >= 47  # perfect squares among the sums
    s = np.float32(scale)
    norms = np.sqrt(R._tree_sum(table * table))
    assert np.array_equal(norms, np.sqrt(sums.astype(np.float32) * s * s))
    got = R.cosine_restated(table, queries, ptr, rows)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------------------------------------ the C entry points
@pytest.fixture(scope="module")
def lib():
    from blp_amd import _lib, build
    build.build()
    return _lib.lib()


def test_rerank_entry_points_refuse_bad_arguments(lib):
    one = ctypes.c_void_p(16)  # non-NULL placeholders: validation fails before anything is dereferenced
    cuts = (ctypes.c_int32 * 2)(10, 100)
    assert lib.blp_rerank_supported(8192, 128) == 1 and lib.blp_rerank_supported(8193, 128) == 0
    assert lib.blp_rerank_supported(1000, 0) == 0 and lib.blp_rerank_supported(1000, 13) == 1
    rc = lib.blp_rerank_ndcg(one, one, one, one, 4, 9000, 8193, one, 20, cuts, 2, one, 100, one, one, 0, None)
    assert rc == -1 and b"8192" in lib.blp_last_error()
    bad = (ctypes.c_int32 * 2)(100, 10)
    rc = lib.blp_rerank_ndcg(one, one, one, one, 4, 90, 30, one, 20, bad, 2, one, 100, one, one, 0, None)
    assert rc == -1 and b"ascending" in lib.blp_last_error()
    rc = lib.blp_rerank_ndcg(one, one, one, one, 4, 90, 30, one, 20, cuts, 2, one, 99, one, one, 0, None)
    assert rc == -1 and b"log2_table" in lib.blp_last_error()
    rc = lib.blp_rerank_ndcg(one, one, one, one, 4, 90, 30, one, 20, cuts, 9, one, 100, one, one, 0, None)
    assert rc == -1 and b"cutoffs" in lib.blp_last_error()
    rc = lib.blp_rerank_ndcg(one, one, one, None, 4, 90, 30, one, 20, cuts, 2, one, 100, one, one, 0, None)
    assert rc == -1 and b"NULL" in lib.blp_last_error()
    rc = lib.blp_rerank_cosine(one, 10, 128, 64, one, 2, 128, one, one, 5, one, 0, None)
    assert rc == -1 and b"stride" in lib.blp_last_error()
    rc = lib.blp_rerank_cosine(one, 10, 128, 128, one, 0, 128, one, one, 5, one, 0, None)
    assert rc == -1 and b"no query" in lib.blp_last_error()
    rc = lib.blp_rerank_cosine(None, 10, 128, 128, one, 2, 128, one, one, 5, one, 0, None)
    assert rc == -1 and b"NULL" in lib.blp_last_error()


def test_rerank_kernels_use_no_scratch(lib):
    """Both kernels (the cosine and the four ndcg launch shapes) keep everything in registers / LDS: no scratch, no spills, in
    the gfx950 code object's notes (tools/kernel_resources.py)."""
    from blp_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    kernels = kernel_resources.kernels_of(os.path.join(build.OBJ, "rerank.hip.o"))
    names = [k for k in kernels if "rerank" in k]
    assert len(names) == 5
    for n in names:
        assert kernels[n]["private_segment_fixed_size"] == 0 and kernels[n].get("vgpr_spill_count", 0) == 0, (n, kernels[n])


def test_ops_refuse_cpu_tensors():
    from blp_amd import ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.rerank_cosine(torch.zeros(3, 4), torch.zeros(1, 4), torch.tensor([0, 3]), torch.tensor([0, 1, 2]))


# ------------------------------------------------------------------------------------------------ the CLI
def write_corpus(root, n_ent=60, n_q=8, seed=0):
    """A synthetic DBpedia-Entity-shaped corpus over write_synthetic_dataset's vocabulary; returns the config updates."""
    from blp_amd.data import write_synthetic_dataset
    write_synthetic_dataset(str(root / "data"), "kg", num_entities=10, num_relations=2, num_train=20, num_valid=4, num_test=4,
                            vocab_size=300, emb_dim=32, seed=seed)
    g = np.random.default_rng(seed)
    words = lambda n: " ".join(f"w{int(i)}" for i in g.integers(0, 300, n))
    ents = [f"<dbpedia:E{i}>" for i in range(n_ent)]
    described = ents[: n_ent - 10]  # the last ten have no description
    with open(root / "desc.txt", "w") as f:
        for e in described:
            f.write(f"{e}\t{words(int(g.integers(3, 12)))}\n")
    qids = [f"Q-{i}" for i in range(n_q)]
    with open(root / "queries.txt", "w") as f:
        for q in qids:
            f.write(f"{q}\t{words(4)} the of\n")
    with open(root / "run.run", "w") as f:
        for q in qids:
            cands = g.choice(n_ent, 25, replace=False)
            scores = np.round(g.uniform(5, 15, 25), 1)  # one decimal: ties in the first-stage scores
            for rank, (c, s) in enumerate(sorted(zip(cands, scores), key=lambda x: -x[1])):
                f.write(f"{q} Q0 {ents[c]} {rank + 1} {s} bm25f\n")
    with open(root / "qrels.txt", "w") as f:
        for q in qids:
            for c in g.choice(n_ent, 12, replace=False):
                f.write(f"{q} 0 {ents[c]} {int(g.integers(0, 3))}\n")
    folds = {"0": {"training": qids[:4], "testing": qids[4:]}, "1": {"training": qids[4:], "testing": qids[:4]}}
    (root / "folds.json").write_text(json.dumps(folds))
    from blp_amd import models
    torch.manual_seed(seed)
    net = models.BOW("transe", "margin", 2, 0.0, embeddings=str(root / "data" / "glove" / "glove.6B.300d.pt"))
    with torch.no_grad():
        net.embeddings.weight.mul_(2.0)  # differs from the file: the checkpoint must really load
    torch.save({"module." + k: v for k, v in net.state_dict().items()}, root / "model-1.pt")
    return dict(model="glove-bow", rel_model="transe", checkpoint=str(root / "model-1.pt"), run_file=str(root / "run.run"),
                queries_file=str(root / "queries.txt"), descriptions_file=str(root / "desc.txt"),
                qrels_file=str(root / "qrels.txt"), folds_file=str(root / "folds.json"), data_root=str(root / "data"))


def run_cli(root, cfg, gpu=False):
    env = dict(os.environ, PYTHONPATH=ROOT)
    if not gpu:
        env.update(CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, os.path.join(ROOT, "retrieval.py"), "with", *[f"{k}={v}" for k, v in cfg.items()]]
    proc = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    return proc.stderr + proc.stdout


def reference_loop(root, cfg):
    """The reference's rerank (retrieval.py:139-284) as dicts and loops, with plain_ndcg for pytrec_eval and the embeddings
    of a torch-CPU encode; returns (run file text, log lines)."""
    from blp_amd import models
    from blp_amd.data import DROPPED, GloVeTokenizer, _word_tokenize
    emb = torch.load(os.path.join(cfg["data_root"], "glove", "glove.6B.300d.pt"))
    net = models.BOW("transe", "margin", 1, 0.0, embeddings=emb)
    state = {k[len("module."):]: v for k, v in torch.load(cfg["checkpoint"]).items() if k != "module.rel_emb.weight"}
    net.load_state_dict(state, strict=False)
    tok = GloVeTokenizer(os.path.join(cfg["data_root"], "glove", "glove.6B.300d-maps.pt"))
    stop = lambda t: " ".join(w for w in _word_tokenize(t) if w.lower() not in DROPPED)
    e2i, texts = R.read_descriptions(cfg["descriptions_file"])
    with torch.no_grad():
        enc = tok.batch_encode_plus([stop(t) for t in texts], max_length=64)
        ent = net.encode(enc["input_ids"], enc["attention_mask"].float())
    id2q = R.read_queries(cfg["queries_file"])
    run, qrels = R.read_run(cfg["run_file"]), R.read_qrels(cfg["qrels_file"])
    folds = R.read_folds(cfg["folds_file"])
    run, qrels = R.restrict_to_folds(folds, run, qrels)
    qemb = {}
    with torch.no_grad():
        for q in run:
            qemb[q] = net.encode(tok.encode(stop(id2q[q]), max_length=64, return_tensors="pt"), text_mask=None).numpy()

    def rerank_on_fold(fold, alpha):
        out = {}
        for q in fold:
            sel = [e for e in run[q] if e in e2i]
            mis = [e for e in run[q] if e not in e2i]
            ptr = np.array([0, len(sel)])
            s1 = R.cosine_restated(ent.numpy(), qemb[q].reshape(1, -1), ptr, np.array([e2i[e] for e in sel], np.int32))
            scores = [float(x) for x in s1] + [0] * len(mis)
            out[q] = {e: alpha * a + (1 - alpha) * run[q][e] for e, a in zip(sel + mis, scores)}
        res = {q: plain_ndcg(out[q], qrels[q], 100) for q in sorted(out, key=str.encode) if out[q] and qrels[q]}
        return np.mean(list(res.values())), out

    logs, test_run = [], {}
    alphas = np.linspace(0, 1, 20)
    for i, (name, fold) in enumerate(folds.items()):
        best, best_alpha = 0.0, alphas[0]
        for a in alphas:
            r, _ = rerank_on_fold(fold["training"], a)
            if r > best:
                best, best_alpha = r, a
        logs.append(f"[Fold {i + 1}/{len(folds)}] Best training result: {best:.3f} with alpha={best_alpha:.3}")
        m, fr = rerank_on_fold(fold["testing"], best_alpha)
        logs.append(f"Test fold result: {m:.3f}")
        test_run.update(fr)
    lines = []
    for q, res in test_run.items():
        for i, (e, s) in enumerate(sorted(res.items(), key=lambda x: x[1], reverse=True)):
            lines.append(f"{q} Q0 {e} {i + 1} {s} glove-bow-transe\n")
    for metric, k in (("ndcg_cut_10", 10), ("ndcg_cut_100", 100)):
        qs = sorted((q for q in run if run[q] and qrels[q]), key=str.encode)
        logs.append(f"Metric: {metric}")
        logs.append(f"Baseline result: {np.mean([plain_ndcg(run[q], qrels[q], k) for q in qs]):.3f}")
        logs.append(f"Test result: {np.mean([plain_ndcg(test_run[q], qrels[q], k) for q in qs]):.3f}")
    return "".join(lines), logs


def test_rerank_cli_end_to_end_on_cpu(tmp_path):
    cfg = write_corpus(tmp_path)
    log = run_cli(tmp_path, cfg)
    assert "Saved entity embeddings to" in log and "No parameter" not in log
    text = (tmp_path / "output" / "None.run").read_text()
    want_text, want_logs = reference_loop(tmp_path, cfg)
    assert text == want_text
    for line in want_logs:
        assert line in log, (line, log[-2000:])
    assert "Finished hyperparameter search" in log and "Saving run file" in log
    # the entity-embedding cache is the reference's file name and format, and it is used on the next run
    cache = tmp_path / "run-qent-model-1.pt"
    assert torch.load(cache).shape == (50, 32)
    log = run_cli(tmp_path, cfg)
    assert f"Loading entity embeddings from {cache}" in log
    assert (tmp_path / "output" / "None.run").read_text() == want_text
