"""Time blp_rank_all_wide (DistMult / ComplEx / SimplE ranked against the whole table at any width, one exact f32 pass) next
to the route rank_block took for these shapes before it: ranking._rank_block_generic_width, i.e. blp_score_fwd into a
(queries, N) slab of at most 1 GiB + blp_rank_from_scores.

Workload: the FB15k-237-shaped filtered evaluation -- 105 740 queries (half per side) x 14 541 rows, a CSR filter of four rows
per query -- at D = 300 and 768 for DistMult and ComplEx.  The counts of the two routes must be equal before anything is
timed.  The two routes alternate step by step in one process, each bracketed by device events; --repeats measurements of
--steps steps each (fewer steps where one step of the dense route alone takes longer than --budget seconds allow); one JSON
line per shape with the median of the medians of both routes, their ratio, the spread of the repeated medians
((max - min) / median) and the new pass's share of the f32 VALU roof in lane-operations (157.3 TFLOPS counts an FMA as two:
78.65 T operations a second for code that may not fuse), counting the multiplies and adds of the terms only.

--narrow: the same call at D = 128 next to blp_rank_all's exact kernel (rank_kernel=1 in the hooks build) and its default
dispatch, counts equal first.

    python tools/rank_all_wide_bench.py [--steps 5] [--warmup 1] [--repeats 5] [--budget 8] [--only MODEL:D ...] [--narrow]
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
from blp_amd import _lib, models, ops, ranking  # noqa: E402

N_ROWS, N_QUERIES, FILTER_PER_QUERY = 14_541, 105_740, 4
SHAPES = [("distmult", 300), ("distmult", 768), ("complex", 300), ("complex", 768)]
VALU_ROOF_OPS = 157.3e12 / 2
# multiplies and adds per term of the table pass, (head side, tail side): rank_all_wide.hip, WideTerm<>::term + the accumulation
TERM_OPS = {"distmult": (3, 2), "complex": (12, 8), "simple": (5, 5)}


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


def make_problem(model, D, Q):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn((N_ROWS, D), generator=g, device=dev) * 0.1
    rel_w = (torch.rand((237, D), generator=g, device=dev) - 0.5) * 0.25
    fixed = torch.randint(0, N_ROWS, (Q,), generator=g, device=dev)
    true_row = torch.randint(0, N_ROWS, (Q,), generator=g, device=dev)
    rels = torch.randint(0, 237, (Q,), generator=g, device=dev)
    base = torch.randint(0, N_ROWS, (Q, 1), generator=g, device=dev)
    col = (base + torch.arange(FILTER_PER_QUERY, device=dev) * 977) % N_ROWS  # distinct rows per query
    col = torch.where(col == true_row[:, None], (col + 1) % N_ROWS, col)      # never the true entity
    rowptr = torch.arange(Q + 1, device=dev) * FILTER_PER_QUERY
    return table, table[fixed].contiguous(), rel_w[rels].contiguous(), true_row, rowptr, col.reshape(-1).contiguous()


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


def wide_vs_dense(model, D, args):
    Q = args.queries
    q_head = Q // 2
    table, q_fixed, q_rel, true_row, rowptr, col = make_problem(model, D, Q)
    m = models.LinkPrediction(D, model, "margin", 3, 0)
    calls = {
        "wide": lambda: ops.rank_all_wide(model, table, q_fixed, q_rel, q_head, true_row=true_row, filt_rowptr=rowptr, filt_col=col),
        "dense": lambda: ranking._rank_block_generic_width(m, table, q_fixed, q_rel, q_head, true_row, None, rowptr, col),
    }
    assert torch.equal(calls["wide"](), calls["dense"]()), "the two routes disagree"
    first = measure(calls, 1, 0)
    rec = {"bench": "rank_all_wide", "model": model, "D": D, "Q": Q, "N": N_ROWS, "filter_per_query": FILTER_PER_QUERY}
    rec.update(repeated(calls, args, first))
    rec["dense_over_wide"] = round(rec["dense_ms"] / rec["wide_ms"], 3)
    rec["faster_by_more_than_spread"] = bool(rec["dense_ms"] * (1 - rec["dense_spread"]) > rec["wide_ms"] * (1 + rec["wide_spread"]))
    n = D if model == "distmult" else D // 2
    lane_ops = N_ROWS * n * (q_head * TERM_OPS[model][0] + (Q - q_head) * TERM_OPS[model][1])
    rec["wide_valu_roof_fraction"] = round(lane_ops / (rec["wide_ms"] * 1e-3) / VALU_ROOF_OPS, 4)
    return rec


def narrow(model, args):
    """D = 128: the new call, blp_rank_all's exact kernel (rank_kernel=1, hooks build) and blp_rank_all's own dispatch"""
    D, Q = 128, args.queries
    q_head = Q // 2
    table, q_fixed, q_rel, true_row, rowptr, col = make_problem(model, D, Q)
    kw = dict(true_row=true_row, filt_rowptr=rowptr, filt_col=col)
    ops.ensure_selftest(table.device, model)
    shipped = ops.rank_all(model, table, q_fixed, q_rel, q_head, **kw).clone()
    shipped_ms = measure({"rank_all": lambda: ops.rank_all(model, table, q_fixed, q_rel, q_head, **kw)}, args.steps, args.warmup)
    _lib.set_knob("rank_kernel", 1)
    try:
        calls = {"wide": lambda: ops.rank_all_wide(model, table, q_fixed, q_rel, q_head, **kw),
                 "exact": lambda: ops.rank_all(model, table, q_fixed, q_rel, q_head, **kw)}
        got = calls["wide"]()
        assert torch.equal(got, calls["exact"]()) and torch.equal(got, shipped), "the routes disagree"
        first = measure(calls, 1, 0)
        rec = {"bench": "rank_all_wide_narrow", "model": model, "D": D, "Q": Q, "N": N_ROWS}
        rec.update(repeated(calls, args, first))
    finally:
        _lib.reset_knobs()
    rec["rank_all_default_ms"] = round(shipped_ms["rank_all"], 4)
    rec["wide_over_exact"] = round(rec["wide_ms"] / rec["exact_ms"], 3)
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
    for model, D in shapes:
        records.append(wide_vs_dense(model, D, args))
        print(json.dumps(records[-1]), flush=True)
        ops.release_workspaces()
        torch.cuda.empty_cache()
    if args.narrow:
        for model in ("distmult", "complex"):
            records.append(narrow(model, args))
            print(json.dumps(records[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in records:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
