"""Time blp_topk_lists (filtered top-k inside per-query candidate lists) next to what the library offered for the same job
before it: blp_rank_lists with scores, followed by a device-side per-query stable top-k of those scores with the filtered
entries dropped (tools/topk_sets_bench.py: stable_topk_of_lists -- three stable sorts over the nnz entries).

For each workload: Q queries with C candidates each (uniform rows, ascending within a list, so that position order is row
order for the yardstick's ties), k = 10, a filter of 8 entries per query (4 of them members of the list); what the filter
removes is marked per entry once, outside the timing.  Rows and scores of the two routes must be equal before anything is
timed.  The routes alternate step by step in one process, each bracketed by device events; the alternation is repeated
--repeats times; one JSON line with the median of every repeat for both routes and for the yardstick's scoring call alone,
the yardstick's own spread over its medians, and the ratio.

    python tools/topk_lists_bench.py [--steps 20] [--warmup 3] [--repeats 3] [--only NAME ...]
                                     [--out profiles/topklists/topk_lists_bench.jsonl]

  longtable-transe[-f16]   13 788 x 1 000 on a 4.6 M x 128 table (f32 / IEEE half)
  fb15k237-transe          105 740 x 500 on 14 541 x 128
  wide-transe              2 048 x 1 000 on 300 000 x 768
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from blp_amd import ops  # noqa: E402
from rank_sets_bench import measure, stats  # noqa: E402
from topk_sets_bench import spread, stable_topk_of_lists  # noqa: E402

K = 10
FILTER_PER_QUERY = 8
DEFAULT_OUT = os.path.join(ROOT, "profiles", "topklists", "topk_lists_bench.jsonl")
WORKLOADS = {
    "longtable-transe": dict(model="transe", N=4_600_000, D=128, Q=13_788, C=1000, dtype="f32"),
    "longtable-transe-f16": dict(model="transe", N=4_600_000, D=128, Q=13_788, C=1000, dtype="f16"),
    "fb15k237-transe": dict(model="transe", N=14_541, D=128, Q=105_740, C=500, dtype="f32"),
    "wide-transe": dict(model="transe", N=300_000, D=768, Q=2048, C=1000, dtype="f32"),
}


def run(name, cfg, steps, warmup, repeats):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    N, D, Q, C = cfg["N"], cfg["D"], cfg["Q"], cfg["C"]
    table = torch.nn.functional.normalize(torch.randn((N, D), generator=g, device=dev), dim=-1)
    rel_w = (torch.rand((237, D), generator=g, device=dev) - 0.5) * 0.25
    fixed = torch.randint(0, N, (Q,), generator=g, device=dev)
    rel_ids = torch.randint(0, 237, (Q,), generator=g, device=dev)
    q_head = Q // 2
    cand = torch.randint(0, N, (Q, C), generator=g, device=dev).sort(dim=1).values
    ptr = torch.arange(Q + 1, device=dev) * C
    rows = cand.reshape(-1).contiguous()
    half = FILTER_PER_QUERY // 2
    inside = cand[:, torch.randint(0, C, (half,), generator=g, device=dev)]
    seg = torch.cat((inside, torch.randint(0, N, (Q, FILTER_PER_QUERY - half), generator=g, device=dev)), 1)
    lo = torch.arange(Q, device=dev) * FILTER_PER_QUERY
    filt = ops.SegmentFilter(lo, lo + FILTER_PER_QUERY, seg.reshape(-1).contiguous(), None, None, 0)
    removed = (cand.unsqueeze(2) == seg.unsqueeze(1)).any(2).reshape(-1)
    owner = torch.arange(Q, device=dev).repeat_interleave(C)
    if cfg["dtype"] == "f16":  # the queries' f32 vectors: the Q fixed rows widened, the same source for both routes
        table = table.to(torch.float16)
        source, src_fixed = table[fixed].float(), torch.arange(Q, device=dev)
    else:
        source, src_fixed = table, fixed
    out = (torch.empty((Q, K), dtype=torch.int64, device=dev), torch.empty((Q, K), dtype=torch.float32, device=dev))
    scores = torch.empty(Q * C, dtype=torch.float32, device=dev)
    yard = [None, None]

    def fused():
        ops.topk_lists(cfg["model"], table, source, src_fixed, rel_w, rel_ids, q_head, ptr, rows, K, filter=filt, out=out)

    def yard_scores():
        ops.rank_lists(cfg["model"], table, source, src_fixed, rel_w, rel_ids, q_head, ptr, rows, out=(None, scores))

    def yardstick():
        yard_scores()
        yard[0], yard[1] = stable_topk_of_lists(scores, rows, removed, owner, ptr, Q, K)

    fused()
    yardstick()
    torch.cuda.synchronize()
    nan = torch.isnan(yard[1])
    same = bool(torch.equal(out[0], yard[0])) and bool(torch.equal(torch.isnan(out[1]), nan)) and \
        bool(torch.equal(out[1][~nan].view(torch.int32), yard[1][~nan].view(torch.int32)))
    base = {"workload": name, **cfg, "k": K, "entries": Q * C, "filter_entries_per_query": FILTER_PER_QUERY, "results_equal": same}
    if not same:
        return base
    a, b, c = [], [], []
    for _ in range(repeats):
        ms = measure({"topk_lists": fused, "rank_lists_plus_sorts": yardstick, "rank_lists_scores_only": yard_scores}, steps, warmup)
        a.append(stats(ms["topk_lists"])["median"])
        b.append(stats(ms["rank_lists_plus_sorts"])["median"])
        c.append(stats(ms["rank_lists_scores_only"])["median"])
    ma, mb, mc = float(np.median(a)), float(np.median(b)), float(np.median(c))
    elem = 2 if cfg["dtype"] == "f16" else 4
    return {**base, "topk_lists_ms_medians": a, "yardstick_ms_medians": b, "yardstick_scores_only_ms_medians": c,
            "topk_lists_ms": round(ma, 4), "yardstick_ms": round(mb, 4), "yardstick_scores_only_ms": round(mc, 4),
            "topk_lists_spread": spread(a), "yardstick_spread": spread(b), "yardstick_over_topk_lists": round(mb / ma, 2),
            "gather_TBps": round(Q * C * D * elem / (ma * 1e-3) / 1e12, 3),
            "workspace_bytes": ops.topk_lists_workspace_bytes(cfg["model"], D, q_head, Q - q_head, Q * C, K), "steps": steps,
            "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()
    for name, cfg in WORKLOADS.items():
        if args.only and name not in args.only:
            continue
        line = json.dumps(run(name, cfg, args.steps, args.warmup, args.repeats))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        ops.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
