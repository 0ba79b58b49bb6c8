"""Time the device alpha search of `retrieval.py rerank` on a DBpedia-Entity-shaped synthetic problem and compare it with the
numpy restatement on the host.

    python tools/rerank_bench.py [--steps 20] [--warmup 3] [--no-host]

Problem: 467 queries x 1 000 first-stage candidates (5 % without a description), an entity table of 400 000 x 128 f32, 20
alphas, 5 folds, cutoffs 10 / 100.  Each step is the two launches -- blp_rerank_cosine (every candidate's cosine with its
query) and blp_rerank_ndcg (nDCG of every (alpha, query)) -- each bracketed by device events.  One JSON line: medians and p90
of both launches, the gathered bytes of the cosine launch and their rate, the host restatement's time, and whether device
and host agree bit for bit.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blp_amd import ops, retrieval as R  # noqa: E402

Q, PER_QUERY, E, D, N_ALPHAS, N_FOLDS = 467, 1000, 400_000, 128, 20, 5


def make_problem(seed=0, device=torch.device("cuda", 0)):
    g = np.random.default_rng(seed)
    C = Q * PER_QUERY
    ptr = np.arange(Q + 1, dtype=np.int64) * PER_QUERY
    rows = g.integers(0, E, C).astype(np.int32)
    rows[g.random(C) < 0.05] = -1
    s2 = np.round(g.gamma(4.0, 4.0, C), 4)                     # BM25-like scores, 4 decimals: ties among them
    gain = np.where(g.random(C) < 0.03, g.integers(1, 3, C), 0).astype(np.int32)
    table_log2 = R.log2_table(100)
    idcg = np.array([R.ideal_dcg(list(gain[ptr[q]:ptr[q + 1]]) + list(g.integers(1, 3, 5)), R.CUTOFFS, table_log2)
                     for q in range(Q)])
    ids = [f"Q{q:03d}" for q in range(Q)]
    problem = R.Problem(ids, None, None, ptr, rows, s2, gain, idcg, table_log2, R.CUTOFFS, np.ones(Q, bool))
    perm = g.permutation(Q)
    folds = {}
    for f in range(N_FOLDS):
        test = [ids[i] for i in perm[f::N_FOLDS]]
        folds[str(f)] = {"training": [q for q in ids if q not in set(test)], "testing": test}
    table = torch.randn(E, D, generator=torch.Generator().manual_seed(seed)).to(device)
    queries = torch.randn(Q, D, generator=torch.Generator().manual_seed(seed + 1)).to(device)
    return dict(problem=problem, folds=folds, alphas=np.linspace(0, 1, N_ALPHAS), table=table, queries=queries,
                cand_ptr=torch.from_numpy(ptr).to(device), cand_row=torch.from_numpy(rows).to(device))


def stats(ms):
    a = np.asarray(ms)
    return {"median": round(float(np.median(a)), 4), "p90": round(float(np.percentile(a, 90)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement (timing and comparison)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    p = make_problem(device=dev)
    pr = p["problem"]
    t = lambda x, dt: torch.as_tensor(x, dtype=dt).to(dev)
    s2, gain, alphas = t(pr.s2, torch.float64), t(pr.gain, torch.int32), t(p["alphas"], torch.float64)
    log2, idcg = t(pr.log2_table, torch.float64), t(pr.idcg, torch.float64)
    s1 = torch.empty(pr.cand_row.shape[0], dtype=torch.float32, device=dev)
    nd = torch.empty((N_ALPHAS, Q, len(R.CUTOFFS)), dtype=torch.float64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    cos_ms, ndcg_ms = [], []
    for i in range(a.warmup + a.steps):
        ev[0].record()
        ops.rerank_cosine(p["table"], p["queries"], p["cand_ptr"], p["cand_row"], out=s1)
        ev[1].record()
        ops.rerank_ndcg(s1, s2, gain, p["cand_ptr"], alphas, R.CUTOFFS, log2, idcg, max_segment=PER_QUERY, out=nd)
        ev[2].record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            cos_ms.append(ev[0].elapsed_time(ev[1]))
            ndcg_ms.append(ev[1].elapsed_time(ev[2]))
    live = int((pr.cand_row >= 0).sum())
    gathered = live * D * 4 * 2  # candidate row + query row per candidate, each read twice (norm pass, dot pass)
    res = {"workload": "dbpedia-shaped", "Q": Q, "candidates": int(pr.cand_row.shape[0]), "E": E, "D": D, "alphas": N_ALPHAS,
           "folds": N_FOLDS, "cutoffs": list(R.CUTOFFS), "steps": a.steps, "warmup": a.warmup,
           "cosine_ms": stats(cos_ms), "ndcg_ms": stats(ndcg_ms),
           "total_ms_median": round(float(np.median(np.asarray(cos_ms) + np.asarray(ndcg_ms))), 4),
           "sorts": N_ALPHAS * Q, "candidate_row_bytes": live * D * 4,
           "candidate_row_tbs": round(live * D * 4 / (np.median(cos_ms) * 1e-3) / 1e12, 3),
           "estimate_ms": 1.0, "gathered_bytes_upper": gathered}
    t0 = time.perf_counter()
    search = R.alpha_search(pr, s1, p["alphas"], p["folds"], device=dev)
    res["device_search_host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    res["alpha_per_fold"] = [round(float(f["alpha"]), 4) for f in search["folds"]]
    if not a.no_host:
        t0 = time.perf_counter()
        s1_host = R.cosine_restated(p["table"].cpu().numpy(), p["queries"].cpu().numpy(), pr.cand_ptr, pr.cand_row)
        t1 = time.perf_counter()
        host = R.trec_ndcg_cut(s1_host, pr.s2, pr.gain, pr.cand_ptr, p["alphas"], pr.cutoffs, pr.log2_table, pr.idcg)
        t2 = time.perf_counter()
        res["host_cosine_ms"] = round((t1 - t0) * 1e3, 1)
        res["host_ndcg_ms"] = round((t2 - t1) * 1e3, 1)
        res["s1_bit_equal"] = bool(np.array_equal(s1.cpu().numpy().view(np.int32), s1_host.view(np.int32)))
        res["ndcg_bit_equal"] = bool(np.array_equal(nd.cpu().numpy().view(np.int64), host.view(np.int64)))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
