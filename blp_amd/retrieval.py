"""Re-ranking a first-stage retrieval run with entity embeddings: the host side of the reference's `retrieval.py rerank`
(retrieval.py:139-284) -- parsers, the CSR the kernels take, trec_eval's ndcg_cut restated in numpy, the alpha search, the run
file.  The device path is two launches (ops.rerank_cosine, ops.rerank_ndcg); the CPU path restates both bit for
bit (cosine_restated, trec_ndcg_cut), so a run on either writes the same run file.

Evaluation contract (trec_eval's ndcg_cut as pytrec_eval runs it):
  * the combined score c = alpha * s1 + (1 - alpha) * s2 in f64 (retrieval.py:181-182) is stored as a C float;
  * candidates rank by that float descending, ties by docno descending (strcmp on the UTF-8 bytes), NaN last;
  * DCG@k = sum over the first k ranks with relevance > 0 of rel / log2(rank + 1), added in rank order in f64; IDCG@k the same
    over the query's positive qrels levels sorted descending (retrieved or not); nDCG = DCG / IDCG, 0 if IDCG is 0;
  * a query counts towards a mean if the run and the qrels both hold entries for it; means are np.mean over the queries in
    strcmp order of their ids (trec_eval's topic order).
"""
import json
import math
from collections import defaultdict

import numpy as np

MAX_SEGMENT = 8192          # candidates per query the device path takes (include/blp_hip.h: BLP_RERANK_MAX_SEGMENT)
SELECT_METRIC = "ndcg_cut_100"
METRICS = ("ndcg_cut_10", "ndcg_cut_100")
CUTOFFS = (10, 100)


# ------------------------------------------------------------------------------------------------ parsers
def read_scores(path):
    """TREC run (>= 6 columns: query Q0 doc rank score tag; float score) or qrels (4 columns: query 0 doc rel; int relevance)
    -> {query: {doc: score}}, one loop for both as in retrieval.py:224-234 (a repeated (query, doc) keeps its first position
    and its last score)."""
    out = defaultdict(dict)
    with open(path) as f:
        for line in f:
            values = line.strip().split()
            if len(values) >= 6:
                query_id, _q0, entity, _rank, score, *_ = values
                score = float(score)
            else:
                query_id, _q0, entity, score = values
                score = int(score)
            out[query_id][entity] = score
    return out


read_run = read_qrels = read_scores


def read_queries(path):
    """`id<TAB>text...` -> {id: text} (retrieval.py:207-213)."""
    id2query = {}
    with open(path) as f:
        for line in f:
            values = line.strip().split('\t')
            id2query[values[0]] = ' '.join(values[1:])
    return id2query


def read_folds(path):
    """The folds JSON: {name: {"training": [ids], "testing": [ids]}} in file order."""
    with open(path) as f:
        return json.load(f)


def read_descriptions(path):
    """`entity<TAB>text...` -> (entity2idx, texts): entity2idx maps an entity to its LINE number (the row of the entity table;
    a repeated entity keeps its last line), texts holds every line's text (retrieval.py:105-113)."""
    entity2idx, texts = {}, []
    with open(path) as f:
        for i, line in enumerate(f):
            values = line.strip().split('\t')
            entity2idx[values[0]] = i
            texts.append(' '.join(values[1:]))
    return entity2idx, texts


def restrict_to_folds(folds, baseline_run, qrels):
    """Keep the queries some fold tests, in fold order (retrieval.py:239-249)."""
    new_run, new_qrels = {}, {}
    for f in folds.values():
        for query_id in f['testing']:
            new_run[query_id] = baseline_run[query_id]
            new_qrels[query_id] = qrels[query_id]
    return new_run, new_qrels


def _utf8(s):
    return s.encode('utf-8')


# ------------------------------------------------------------------------------------------------ packing
def log2_table(n):
    """log2_table[i] = math.log2(i + 2), i < n: the DCG discount of rank i + 1."""
    return np.array([math.log2(i + 2) for i in range(n)], dtype=np.float64)


def ideal_dcg(rels, cutoffs, table):
    """IDCG@k for each cutoff: the positive relevance levels sorted descending, rel / log2(i + 2) added in order (f64)."""
    levels = sorted((r for r in rels if r > 0), reverse=True)
    out, acc, i = [], 0.0, 0
    for k in cutoffs:
        while i < min(k, len(levels)):
            acc = acc + levels[i] / table[i]
            i += 1
        out.append(acc)
    return out


class Problem:
    """A run packed for the kernels.  Query q (query_ids[q]) owns candidates [cand_ptr[q], cand_ptr[q + 1]), ordered by
    docno descending (entities[q]); cand_row = the entity-table row (-1: no description), s2 the run's score, gain the qrels
    relevance (0: unjudged).  order[q] lists the segment positions in the reference's insertion order -- the candidates that
    have a description first, then the others, each in run order (retrieval.py:158-167): the run file's stable sort follows
    it.  evaluated[q]: the query has run and qrels entries (it counts towards the means)."""

    def __init__(self, query_ids, entities, order, cand_ptr, cand_row, s2, gain, idcg, log2, cutoffs, evaluated):
        self.query_ids, self.entities, self.order = query_ids, entities, order
        self.cand_ptr, self.cand_row, self.s2, self.gain = cand_ptr, cand_row, s2, gain
        self.idcg, self.log2_table, self.cutoffs, self.evaluated = idcg, log2, tuple(cutoffs), evaluated

    @property
    def max_segment(self):
        return int(np.diff(self.cand_ptr).max()) if len(self.query_ids) else 0


def pack(baseline_run, entity2idx, qrels, query_ids=None, cutoffs=CUTOFFS):
    """{query: {entity: score}} run + entity2idx + {query: {entity: rel}} qrels -> Problem (queries in ``query_ids`` order,
    default: the run's)."""
    query_ids = list(baseline_run) if query_ids is None else list(query_ids)
    table = log2_table(max(cutoffs))
    entities, order, ptr, rows, s2, gain, idcg, evaluated = [], [], [0], [], [], [], [], []
    for q in query_ids:
        results = baseline_run.get(q, {})
        judged = qrels.get(q, {})
        inserted = [e for e in results if e in entity2idx] + [e for e in results if e not in entity2idx]
        seg = sorted(inserted, key=_utf8, reverse=True)
        pos = {e: i for i, e in enumerate(seg)}
        entities.append(seg)
        order.append(np.array([pos[e] for e in inserted], dtype=np.int64))
        rows.extend(entity2idx.get(e, -1) for e in seg)
        s2.extend(float(results[e]) for e in seg)
        gain.extend(int(judged.get(e, 0)) for e in seg)
        ptr.append(ptr[-1] + len(seg))
        idcg.append(ideal_dcg(judged.values(), cutoffs, table))
        evaluated.append(bool(results) and bool(judged))
    return Problem(query_ids, entities, order, np.array(ptr, np.int64), np.array(rows, np.int32), np.array(s2, np.float64),
                   np.array(gain, np.int32), np.array(idcg, np.float64).reshape(len(query_ids), len(cutoffs)), table,
                   cutoffs, np.array(evaluated, bool))


# ------------------------------------------------------------------------------------------------ CPU restatements
def _tree_sum(terms):
    """(N, D) f32 terms -> (N,) f32 in rerank_cosine's order: lane l = 0..63 adds elements l, l + 64, ... to +0; the 64 lane
    partials fold as p[l] + p[l + h], h = 32 ... 1."""
    n, d = terms.shape
    p = np.zeros((n, 64), np.float32)
    for k0 in range(0, d, 64):
        w = min(64, d - k0)
        p[:, :w] = p[:, :w] + terms[:, k0:k0 + w]
    h = 32
    while h >= 1:
        p[:, :h] = p[:, :h] + p[:, h:2 * h]
        h //= 2
    return p[:, 0].copy()


def _normalised(x):
    n = np.sqrt(_tree_sum(x * x))
    n = np.where(n < np.float32(1e-12), np.float32(1e-12), n).astype(np.float32)
    return x / n[:, None]


def cosine_restated(table, queries, cand_ptr, cand_row, chunk=65536):
    """numpy f32 restatement of rerank_cosine, bit for bit: s1 (C,) float32 (0.0 for row -1, NaN for a row outside the
    table)."""
    table = np.asarray(table, np.float32)
    queries = np.asarray(queries, np.float32)
    cand_ptr = np.asarray(cand_ptr, np.int64)
    cand_row = np.asarray(cand_row, np.int64)
    C = cand_row.shape[0]
    qidx = np.repeat(np.arange(len(cand_ptr) - 1), np.diff(cand_ptr))
    s1 = np.zeros(C, np.float32)
    bad = (cand_row < -1) | (cand_row >= table.shape[0])
    s1[bad] = np.nan
    live = np.nonzero((cand_row >= 0) & ~bad)[0]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for lo in range(0, live.shape[0], chunk):
            idx = live[lo:lo + chunk]
            x = _normalised(table[cand_row[idx]])
            y = _normalised(queries[qidx[idx]])
            s1[idx] = _tree_sum(x * y)
    return s1


def _keys(c):
    """Unique descending-order keys of one segment: orderable((float)c) << 32 | (0xFFFFFFFF - index), NaN -> 0 high word."""
    f = c.astype(np.float32)
    b = f.view(np.uint32).astype(np.uint64)
    b = np.where(b == 0x80000000, 0, b)
    hi = np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)
    hi = np.where(np.isnan(f), 0, hi).astype(np.uint64)
    idx = np.arange(c.shape[-1], dtype=np.uint64)
    return (hi << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)


def trec_ndcg_cut(s1, s2, gain, cand_ptr, alphas, cutoffs, log2, idcg):
    """The evaluation contract in numpy: (A, Q, n_cut) float64, equal bit for bit to rerank_ndcg."""
    s1 = np.asarray(s1, np.float32).astype(np.float64)
    s2 = np.asarray(s2, np.float64)
    gain = np.asarray(gain, np.int64)
    alphas = np.asarray(alphas, np.float64)
    cand_ptr = np.asarray(cand_ptr, np.int64)
    idcg = np.asarray(idcg, np.float64)
    A, Q, n_cut = alphas.shape[0], len(cand_ptr) - 1, len(cutoffs)
    out = np.zeros((A, Q, n_cut), np.float64)
    kmax = int(cutoffs[-1])
    with np.errstate(invalid='ignore', over='ignore'):
        for q in range(Q):
            lo, hi = int(cand_ptr[q]), int(cand_ptr[q + 1])
            n = hi - lo
            m = min(n, kmax)
            if m == 0:
                continue
            c = alphas[:, None] * s1[None, lo:hi] + (1.0 - alphas)[:, None] * s2[None, lo:hi]
            keys = _keys(c)
            ranked = np.argsort(keys, axis=1)[:, ::-1][:, :m]         # keys are unique: descending order
            g = gain[lo:hi][ranked]
            terms = np.where(g > 0, g / log2[:m], 0.0)
            dcg = np.cumsum(terms, axis=1)                            # sequential, in rank order
            for j, k in enumerate(cutoffs):
                d = dcg[:, min(int(k), m) - 1]
                out[:, q, j] = d / idcg[q, j] if idcg[q, j] > 0 else 0.0
    return out


# ------------------------------------------------------------------------------------------------ the search
def fold_mean(values, query_ids):
    """np.mean of the per-query values in strcmp order of the query ids (trec_eval's topic order)."""
    order = sorted(range(len(query_ids)), key=lambda i: _utf8(query_ids[i]))
    return np.mean([values[i] for i in order])


def device_ndcg(problem, s1, alphas, device):
    """ndcg (A, Q, n_cut) from the device kernel; s1 a device tensor or an array."""
    import torch

    from . import ops
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(device)
    s1 = s1 if isinstance(s1, torch.Tensor) else t(s1, torch.float32)
    out = ops.rerank_ndcg(s1.to(device), t(problem.s2, torch.float64), t(problem.gain, torch.int32),
                          t(problem.cand_ptr, torch.int64), t(alphas, torch.float64), problem.cutoffs,
                          t(problem.log2_table, torch.float64), t(problem.idcg, torch.float64), max_segment=problem.max_segment)
    return out.cpu().numpy()


def alpha_search(problem, s1, alphas, folds, device=None):
    """The reference's per-fold choice of alpha (retrieval.py:251-270) on precomputed nDCGs: every (alpha, query) at once on
    ``device`` (rerank_ndcg; None = CPU: trec_ndcg_cut), then numpy means per fold.  alpha is chosen by strict '>' starting
    from best = 0.0 and alphas[0].  Returns a dict: per fold its name, alpha, training and test result; ``query_alpha`` (the
    alpha each test query's final scores use: the last fold that tests it) and the final per-query ndcg_cut_10 / 100 of the
    re-ranked run and of the baseline."""
    s1_host = s1.cpu().numpy() if hasattr(s1, 'cpu') else np.asarray(s1, np.float32)
    alphas = np.asarray(alphas, np.float64)
    if problem.max_segment > MAX_SEGMENT and device is not None:
        raise ValueError(f"a query has {problem.max_segment} candidates; the device path takes at most {MAX_SEGMENT}")
    if device is None:
        ndcg = trec_ndcg_cut(s1_host, problem.s2, problem.gain, problem.cand_ptr, alphas, problem.cutoffs, problem.log2_table,
                             problem.idcg)
    else:
        ndcg = device_ndcg(problem, s1, alphas, device)
    pos = {q: i for i, q in enumerate(problem.query_ids)}
    j_sel = problem.cutoffs.index(int(SELECT_METRIC.rsplit('_', 1)[1]))

    def mean_over(queries, a_idx):
        idx = sorted({pos[q] for q in queries if problem.evaluated[pos[q]]}, key=lambda i: _utf8(problem.query_ids[i]))
        return np.mean([ndcg[a_idx, i, j_sel] for i in idx])

    result = {'folds': [], 'query_alpha': {}}
    for name, fold in folds.items():
        best_result, best_a = 0.0, 0
        for a in range(len(alphas)):
            r = mean_over(fold['training'], a)
            if r > best_result:
                best_result, best_a = r, a
        test_mean = mean_over(fold['testing'], best_a)
        result['folds'].append({'name': name, 'alpha': alphas[best_a], 'alpha_index': best_a, 'train': best_result,
                                'test': test_mean})
        for q in fold['testing']:  # test_run.update(fold_run): a query keeps its first position and takes its last alpha
            result['query_alpha'][q] = best_a
    # final evaluation: the re-ranked test run and the baseline (the run's own scores: alpha = 0 on s1 = 0)
    test_q = [q for q in dict.fromkeys(problem.query_ids) if q in result['query_alpha']]
    base = trec_ndcg_cut(np.zeros_like(s1_host), problem.s2, problem.gain, problem.cand_ptr, np.zeros(1), problem.cutoffs,
                         problem.log2_table, problem.idcg)[0]
    evaluated = sorted((q for q in test_q if problem.evaluated[pos[q]]), key=_utf8)
    result['evaluated_queries'] = evaluated
    result['baseline'] = {m: np.array([base[pos[q], j] for q in evaluated]) for j, m in enumerate(METRICS)}
    result['test'] = {m: np.array([ndcg[result['query_alpha'][q], pos[q], j] for q in evaluated]) for j, m in enumerate(METRICS)}
    result['ndcg'] = ndcg
    return result


def rerank_run(problem, s1, query_alpha, alphas):
    """The re-ranked run as the reference builds it: {query: {entity: np.float64 score}}, queries in the order a fold first
    tests them, entities in insertion order (retrieval.py:158-186)."""
    s1 = np.asarray(s1, np.float32).astype(np.float64)
    pos = {q: i for i, q in enumerate(problem.query_ids)}
    run = {}
    for q, a in query_alpha.items():
        i = pos[q]
        lo = int(problem.cand_ptr[i])
        alpha = np.float64(alphas[a])
        seg = problem.order[i]
        scores = alpha * s1[lo + seg] + (1 - alpha) * problem.s2[lo + seg]
        run[q] = {problem.entities[i][p]: sc for p, sc in zip(seg.tolist(), scores)}
    return run


def write_run(path, run, model, rel_model):
    """retrieval.py:276-284: per query, a stable sort by score descending; `{query} Q0 {entity} {rank} {score} {tag}`."""
    with open(path, 'w') as f:
        for query, results in run.items():
            ranking = sorted(results.items(), key=lambda x: x[1], reverse=True)
            for i, (entity, score) in enumerate(ranking):
                f.write(f'{query} Q0 {entity} {i + 1} {score} {model}-{rel_model}\n')
