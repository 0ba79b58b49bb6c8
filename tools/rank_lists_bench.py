"""Time blp_rank_lists (counts of per-query candidate lists, filtered) next to the dense route ranking.rank_candidates falls
back to -- ops.score on gathered rows with the comparisons -- and against the bytes it must gather.

For each workload: the same queries, lists and filter; the two calls alternate step by step in one process, each bracketed by
device events; warm-up, then --steps steps; one JSON line with the median and p90 of both, their ratio and the achieved gather
bandwidth nnz x D x sizeof(elem) / median.

    python tools/rank_lists_bench.py [--steps 30] [--warmup 3] [--only NAME ...] [--out FILE.jsonl]

  wikidata5m-{transe,complex}        13 788 queries x 1 000 candidates, 4.6 M x 128 table (sampled Wikidata5M-scale evaluation)
  wikidata5m-{transe,complex}-f16    the same against a float16 table
  fb15k237-{transe,distmult}         105 740 queries x 500 candidates, 14 541 x 128
  bow768-transe                      2 048 x 1 000, 300 000 x 768
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blp_amd import models, ops, ranking  # noqa: E402

WORKLOADS = {
    "wikidata5m-transe": dict(model="transe", N=4_600_000, D=128, Q=13_788, C=1000, dtype="float32"),
    "wikidata5m-complex": dict(model="complex", N=4_600_000, D=128, Q=13_788, C=1000, dtype="float32"),
    "wikidata5m-transe-f16": dict(model="transe", N=4_600_000, D=128, Q=13_788, C=1000, dtype="float16"),
    "wikidata5m-complex-f16": dict(model="complex", N=4_600_000, D=128, Q=13_788, C=1000, dtype="float16"),
    "fb15k237-transe": dict(model="transe", N=14_541, D=128, Q=105_740, C=500, dtype="float32"),
    "fb15k237-distmult": dict(model="distmult", N=14_541, D=128, Q=105_740, C=500, dtype="float32"),
    "bow768-transe": dict(model="transe", N=300_000, D=768, Q=2048, C=1000, dtype="float32"),
}
FILTER_PER_QUERY = 8  # entries of a query's filter segment, half of them members of its list


def measure(calls, steps, warmup):
    ev = {n: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for n in calls}
    out = {n: [] for n in calls}
    for i in range(warmup + steps):
        for n, fn in calls.items():
            ev[n][0].record()
            fn()
            ev[n][1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            for n in calls:
                out[n].append(ev[n][0].elapsed_time(ev[n][1]))
    return out


def stats(ms):
    a = np.asarray(ms)
    return {"median": round(float(np.median(a)), 4), "p90": round(float(np.percentile(a, 90)), 4)}


def run(name, cfg, steps, warmup):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    N, D, Q, C = cfg["N"], cfg["D"], cfg["Q"], cfg["C"]
    table = torch.randn((N, D), generator=g, device=dev)
    table = torch.nn.functional.normalize(table, dim=-1) if cfg["model"] == "transe" else table * 0.1
    table = table.to(getattr(torch, cfg["dtype"]))
    R = 200
    model = models.LinkPrediction(D, cfg["model"], "margin", R, 0).to(dev)
    rel_w = model.rel_emb.weight.detach()
    fixed = torch.randint(0, N, (Q,), generator=g, device=dev)
    true = torch.randint(0, N, (Q,), generator=g, device=dev)
    rel_ids = torch.randint(0, R, (Q,), generator=g, device=dev)
    cand = ranking.sample_candidates(Q, N, C, generator=g)
    ptr = torch.arange(Q + 1, device=dev) * C
    rows = cand.reshape(-1)
    seg = torch.cat((cand[:, :FILTER_PER_QUERY // 2], torch.randint(0, N, (Q, FILTER_PER_QUERY // 2), generator=g, device=dev)), 1)
    lo = torch.arange(Q, device=dev) * FILTER_PER_QUERY
    filt = ops.SegmentFilter(lo, lo + FILTER_PER_QUERY, seg.reshape(-1).contiguous(), None, None, 0)
    q_head = Q // 2
    if table.dtype != torch.float32:
        source, src_fixed, src_true = table[torch.cat((fixed, true))].float(), torch.arange(Q, device=dev), torch.arange(Q, 2 * Q, device=dev)
    else:
        source, src_fixed, src_true = table, fixed, true
    counts = torch.empty((Q, 4), dtype=torch.int32, device=dev)
    fixed_vec, true_vec, rel_vec = source[src_fixed], source[src_true], rel_w[rel_ids]
    dense_filt = (filt.seg_lo, filt.seg_hi, filt.values, None, None)

    def fused():
        ops.rank_lists(cfg["model"], table, source, src_fixed, rel_w, rel_ids, q_head, ptr, rows, true_row=src_true, filter=filt,
                       out=(counts, None))

    dense_out = []

    def dense():
        dense_out[:] = ranking._rank_lists_dense(model.score_fn, table, fixed_vec, rel_vec, true_vec, q_head, ptr, rows, 0, dense_filt,
                                                 False)

    fused()
    dense()
    same = bool(torch.equal(counts, dense_out[0]))
    ms = measure({"fused": fused, "dense": dense}, steps, warmup)
    f, d = stats(ms["fused"]), stats(ms["dense"])
    gathered = rows.numel() * D * table.element_size()
    return {"workload": name, **cfg, "nnz": rows.numel(), "filter_entries_per_query": FILTER_PER_QUERY, "counts_equal_dense": same,
            "fused_ms": f, "dense_ms": d, "dense_over_fused": round(d["median"] / f["median"], 2),
            "gathered_bytes": gathered, "gather_TBps": round(gathered / (f["median"] * 1e-3) / 1e12, 3), "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--out")
    args = ap.parse_args()
    for name, cfg in WORKLOADS.items():
        if args.only and name not in args.only:
            continue
        line = json.dumps(run(name, cfg, args.steps, args.warmup))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        ops.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
