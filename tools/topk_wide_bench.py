"""Time blp_topk_wide (filtered top-k over the whole table for DistMult / ComplEx / SimplE at any width) and the TransE
one-set route (blp_topk_sets_wide with the table as the single candidate set, ranking._topk_one_set) next to the route
ranking.predict_links took for these shapes before: ranking._topk_dense, i.e. score_fn into a (chunk, N) matrix of at most
256 MiB + three stable sorts per chunk.

Workload: the FB15k-237-shaped prediction -- 105 740 queries (half per side) x 14 541 rows, a segment filter of four rows per
query, k = 10 -- at D = 300 and 768 for DistMult, ComplEx and TransE.  Rows and score bits of the two routes must be equal
before anything is timed.  The two routes alternate step by step in one process, each bracketed by device events; --repeats
measurements of --steps steps each (fewer steps where one step of the dense route alone takes longer than --budget seconds
allow -- at the default budget the dense route's seconds cut a repeat to ONE step without a warm-up of its own, so each of
the five "medians" is a single sample taken after the two calls of the equality check); one JSON line per shape with the median of the medians of both routes, their ratio and the spread of the repeated
medians ((max - min) / median).  ``route_it``: the new call is faster than the dense route by more than both spreads
together -- the condition predict_links' routing of a shape rests on.

Side figures, reported and not gated: blp_rank_all_wide on the same shape (the table pass without the selection; it
alternates with the new call for --steps steps after --warmup, one median each, not repeated), and
--narrow: the new call next to blp_topk at D = 128.

    python tools/topk_wide_bench.py [--steps 5] [--warmup 1] [--repeats 5] [--budget 8] [--only MODEL:D ...] [--narrow]
                                    [--queries Q] [--out FILE.jsonl]
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

N_ROWS, N_QUERIES, FILTER_PER_QUERY, K = 14_541, 105_740, 4, 10
SHAPES = [("distmult", 300), ("distmult", 768), ("complex", 300), ("complex", 768), ("transe", 300), ("transe", 768)]


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
    return {n: float(np.median(v)) for n, v in out.items()}


def repeated(calls, args, first):
    """--repeats medians of the alternating routes; the steps of a repeat cut down to the budget by the slowest route's first step"""
    steps = max(1, min(args.steps, int(args.budget * 1000.0 / max(first.values()) / args.repeats)))
    runs = [measure(calls, steps, args.warmup if steps > 1 else 0) for _ in range(args.repeats)]
    out = {"steps": steps, "repeats": args.repeats}
    for n in calls:
        meds = np.asarray([r[n] for r in runs])
        out[n + "_ms"] = round(float(np.median(meds)), 4)
        out[n + "_spread"] = round(float((meds.max() - meds.min()) / np.median(meds)), 4)
    return out


def make_problem(model, D, Q):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn((N_ROWS, D), generator=g, device=dev)
    table = torch.nn.functional.normalize(table, dim=-1) if model == "transe" else table * 0.1
    rel_w = (torch.rand((237, D), generator=g, device=dev) - 0.5) * 0.25
    fixed = torch.randint(0, N_ROWS, (Q,), generator=g, device=dev)
    rels = torch.randint(0, 237, (Q,), generator=g, device=dev)
    base = torch.randint(0, N_ROWS, (Q, 1), generator=g, device=dev)
    values = ((base + torch.arange(FILTER_PER_QUERY, device=dev) * 977) % N_ROWS).reshape(-1).contiguous()  # distinct rows per query
    seg_lo = torch.arange(Q, device=dev) * FILTER_PER_QUERY
    return table, rel_w, fixed, rels, (seg_lo, seg_lo + FILTER_PER_QUERY, values, None, None)


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def new_vs_dense(model, D, args):
    Q = args.queries
    q_head = Q // 2
    table, rel_w, fixed, rels, seg = make_problem(model, D, Q)
    filt = ops.SegmentFilter(*seg, 0)
    score_fn = models.LinkPrediction(D, model, "margin", 3, 0).score_fn
    fused = ranking._topk_one_set if model == "transe" else ops.topk_wide
    calls = {
        "new": lambda: fused(model, table, table, fixed, rel_w, rels, q_head, K, filter=filt),
        "dense": lambda: ranking._topk_dense(score_fn, table, table[fixed], rel_w[rels], q_head, K, 0, seg),
    }
    got, want = calls["new"](), calls["dense"]()
    # on the device score_fn is blp_score_fwd, the reference's bits: the two routes must give the same rows and score bits
    assert same(got, want), "the two routes disagree"
    rec = {"bench": "topk_wide", "model": model, "D": D, "Q": Q, "N": N_ROWS, "k": K, "filter_per_query": FILTER_PER_QUERY,
           "call": "topk_sets_wide_one_set" if model == "transe" else "topk_wide", "results_equal": True}
    first = measure(calls, 1, 0)
    rec.update(repeated(calls, args, first))
    rec["dense_over_new"] = round(rec["dense_ms"] / rec["new_ms"], 3)
    rec["route_it"] = bool(rec["dense_ms"] * (1 - rec["dense_spread"]) > rec["new_ms"] * (1 + rec["new_spread"]))
    if model != "transe":  # the parent commit's code on the same shape: the table pass with counting in place of selection
        q_fixed, q_rel = table[fixed].contiguous(), rel_w[rels].contiguous()
        # (alternating with the new call, --steps steps after --warmup: one median each, no repeats)
        side = measure({"new": calls["new"], "rank_all_wide": lambda: ops.rank_all_wide(model, table, q_fixed, q_rel, q_head, true_row=fixed)},
                       args.steps, args.warmup)
        rec["rank_all_wide_ms"] = round(side["rank_all_wide"], 4)
        rec["new_over_rank_all_wide"] = round(side["new"] / side["rank_all_wide"], 3)
    return rec


def narrow(model, args):
    """D = 128: the new call next to blp_topk, results equal first"""
    D, Q = 128, args.queries
    q_head = Q // 2
    table, rel_w, fixed, rels, seg = make_problem(model, D, Q)
    filt = ops.SegmentFilter(*seg, 0)
    calls = {"new": lambda: ops.topk_wide(model, table, table, fixed, rel_w, rels, q_head, K, filter=filt),
             "topk": lambda: ops.topk(model, table, table, fixed, rel_w, rels, q_head, K, filter=filt)}
    assert same(calls["new"](), calls["topk"]()), "blp_topk_wide and blp_topk disagree"
    first = measure(calls, 1, 0)
    rec = {"bench": "topk_wide_narrow", "model": model, "D": D, "Q": Q, "N": N_ROWS, "k": K}
    rec.update(repeated(calls, args, first))
    rec["new_over_topk"] = round(rec["new_ms"] / rec["topk_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--budget", type=float, default=8.0, help="seconds of the slowest route per shape")
    ap.add_argument("--queries", type=int, default=N_QUERIES)
    ap.add_argument("--only", nargs="*", default=None, help="MODEL:D")
    ap.add_argument("--narrow", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = SHAPES if not args.only else [(s.split(":")[0], int(s.split(":")[1])) for s in args.only]
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)
        if args.out:  # (written as it goes: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                for r in records:
                    f.write(json.dumps(r) + "\n")

    for model, D in shapes:
        emit(new_vs_dense(model, D, args))
        ops.release_workspaces()
        torch.cuda.empty_cache()
    if args.narrow:
        for model in ("distmult", "complex"):
            emit(narrow(model, args))


if __name__ == "__main__":
    main()
