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

    python tools/rank_lists_bench.py --wide 300 768 128 [--model distmult complex simple] [--shape fb15k237 bow]
                                     [--dtype float32] [--repeats 5] [--steps 10] [--out profiles/ranklists/FILE.jsonl]

blp_rank_lists_wide (DistMult / ComplEx / SimplE at any width) on the fb15k237 shape (105 740 x 500 over 14 541 rows) or the bow
shape (2 048 x 1 000 over 300 000 rows): off 64 / 128 / 256 next to _rank_lists_dense on the same device tensors -- the route
ranking.rank_candidates took there before the call existed --, at 64 / 128 / 256 next to blp_rank_lists, which stays the routed
call there.  Counts required equal first; the two alternate step by step; one JSON line has the median of the repeated medians
of each with its spread ((max - min) / median), the ratio, whether the new call is faster by more than both spreads together,
the gather bandwidth and the share of the f32 lane-op roof.
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


WIDE_SHAPES = {  # the shapes of WORKLOADS that fit a 300 / 768-wide table next to the dense route's 256 MiB chunks
    "fb15k237": dict(N=14_541, Q=105_740, C=500),
    "bow": dict(N=300_000, Q=2048, C=1000),
}
LANE_OP_ROOF = 78.6e12  # f32 lane-ops per second
# f32 operations per term of a score, head side / tail side (wide_bilinear.h: WideTerm<>::term and the accumulator's add)
OPS_PER_TERM = {"distmult": (3, 2), "complex": (12, 8), "simple": (5, 5)}


def repeated(runs, name):
    a = np.asarray([float(np.median(r[name])) for r in runs])
    mid = float(np.median(a))
    return {"median_ms": round(mid, 4), "spread": round(float((a.max() - a.min()) / mid), 4), "medians_ms": [round(float(x), 4) for x in a]}


def run_wide(model_name, D, shape, steps, warmup, repeats, dtype="float32"):
    """ranking.rank_candidates' fused call for a DistMult / ComplEx / SimplE model at width D -- blp_rank_lists_wide off 64 / 128 /
    256 -- next to _rank_lists_dense on the same device tensors (what the route was before the call existed); at 64 / 128 / 256
    blp_rank_lists_wide next to blp_rank_lists, the call routed there.  Counts required equal first; then the two alternate
    step by step, --repeats measurements of --steps steps each; one JSON line with the median of the repeated medians of each,
    their spread ((max - min) / median), the ratio, the gather bandwidth and the share of the f32 lane-op roof."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    N, Q, C = (WIDE_SHAPES[shape][k] for k in ("N", "Q", "C"))
    table = (torch.randn((N, D), generator=g, device=dev) * 0.1).to(getattr(torch, dtype))
    R = 200
    model = models.LinkPrediction(D, model_name, "margin", R, 0).to(dev)
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
    counts, other_counts = (torch.empty((Q, 4), dtype=torch.int32, device=dev) for _ in range(2))
    fixed_vec, true_vec, rel_vec = source[src_fixed], source[src_true], rel_w[rel_ids]
    dense_filt = (filt.seg_lo, filt.seg_hi, filt.values, None, None)
    fixed_width = ops.rank_lists_supported(model_name, D, table.dtype)

    def wide():
        ops.rank_lists_wide(model_name, table, source, src_fixed, rel_w, rel_ids, q_head, ptr, rows, true_row=src_true, filter=filt,
                            out=(counts, None))

    def fixed_call():
        ops.rank_lists(model_name, table, source, src_fixed, rel_w, rel_ids, q_head, ptr, rows, true_row=src_true, filter=filt,
                       out=(other_counts, None))

    dense_out = []

    def dense():
        dense_out[:] = ranking._rank_lists_dense(model.score_fn, table, fixed_vec, rel_vec, true_vec, q_head, ptr, rows, 0, dense_filt,
                                                 False)

    other_name, other = ("blp_rank_lists", fixed_call) if fixed_width else ("dense", dense)
    wide()
    other()
    same = bool(torch.equal(counts, other_counts if fixed_width else dense_out[0]))
    runs = [measure({"wide": wide, "other": other}, steps, warmup) for _ in range(repeats)]
    a, b = repeated(runs, "wide"), repeated(runs, "other")
    n = D if model_name == "distmult" else D // 2
    lane_ops = rows.numel() * n * sum(OPS_PER_TERM[model_name]) / 2  # q_head = Q / 2
    gathered = rows.numel() * D * table.element_size()
    faster = bool(b["median_ms"] * (1 - b["spread"]) > a["median_ms"] * (1 + a["spread"]))
    return {"workload": f"{shape}-{model_name}-{D}" + ("" if dtype == "float32" else f"-{dtype}"), "model": model_name, "N": N, "D": D,
            "Q": Q, "C": C, "dtype": dtype, "nnz": rows.numel(), "filter_entries_per_query": FILTER_PER_QUERY, "yardstick": other_name,
            "routed": "blp_rank_lists" if fixed_width else "blp_rank_lists_wide", "counts_equal": same, "blp_rank_lists_wide_ms": a,
            f"{other_name}_ms": b, "yardstick_over_wide": round(b["median_ms"] / a["median_ms"], 2),
            "wide_faster_by_more_than_both_spreads": faster, "gathered_bytes": gathered,
            "gather_TBps": round(gathered / (a["median_ms"] * 1e-3) / 1e12, 3),
            "lane_op_roof_share": round(lane_ops / (a["median_ms"] * 1e-3) / LANE_OP_ROOF, 3), "steps": steps, "warmup": warmup,
            "repeats": repeats}


def emit(line, out):
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--out")
    ap.add_argument("--wide", type=int, nargs="+", metavar="D",
                    help="time blp_rank_lists_wide at these widths instead of the workloads: next to the dense route (off 64 / 128 / "
                         "256) or to blp_rank_lists (at them)")
    ap.add_argument("--model", nargs="+", default=["distmult", "complex", "simple"], choices=["distmult", "complex", "simple"])
    ap.add_argument("--shape", nargs="+", default=["fb15k237"], choices=sorted(WIDE_SHAPES))
    ap.add_argument("--dtype", default="float32", choices=["float32", "float16", "bfloat16"])
    ap.add_argument("--repeats", type=int, default=5, help="with --wide: measurements whose medians' spread is reported")
    args = ap.parse_args()
    if args.wide:
        for shape in args.shape:
            for model_name in args.model:
                for D in args.wide:
                    emit(json.dumps(run_wide(model_name, D, shape, args.steps, args.warmup, args.repeats, args.dtype)), args.out)
                    ops.release_workspaces()
                    torch.cuda.empty_cache()
        return
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
