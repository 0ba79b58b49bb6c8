"""Time relation prediction -- blp_rank_relations (filtered counts) and blp_topk_relations (filtered top-k) -- next to the
route the library offered before them: ops.score broadcast to a (Q, R) matrix in query pieces of at most 256 MiB, then
ops.rank_from_scores for the counts or a stable torch sort for the predictions.

For each workload: the same pairs, relations and filter (2 entries per query, never the true relation); the results of the two
routes are compared before anything is timed; the two calls then alternate step by step in one process, each bracketed by device
events: --warmup steps, then --steps steps, the median taken; that five times over.  One JSON line per workload: the median of
the five medians of both routes, their ratio, the spread of the five medians ((max - min) / median) and the fraction of the f32
lane-op roof (78.6 T lane-ops/s) at 3 lane-ops per (pair, column) -- TransE: add, subtract, add |x|; DistMult: multiply,
multiply, add; SimplE: four multiplies and two adds per pair of columns -- and 6 for ComplEx (eight multiplies and four adds per
pair of columns).

    python tools/rank_relations_bench.py [--steps 30] [--warmup 3] [--repeats 5] [--only NAME ...] [--out FILE.jsonl]
                                         [--width D ...] [--model M ...]

  fb15k237-{transe,distmult}     310 116 pairs over a 14 541 x 128 table, R = 237
  wikidata5m-{transe,distmult}   1 000 000 pairs over 100 000 x 128 gathered rows, R = 822

--width D ... : instead of the four workloads above, fb15k237-transe at each width D through the any-width calls
(blp_rank_relations_wide / blp_topk_relations_wide; the BOW / DKRL encoders train TransE at 300 and 768), as workload
fb15k237-transe-wide<D>, against the same yardstick.  At a width the register kernels take as well (64 / 128 / 256) they join the
alternation (register_counts / register_topk) and the line carries the wide call's time over theirs: the cost of the slab form.
--model M ... (with --width; default transe): the same shape for these models, distmult / complex / simple through
blp_rank_relations_wide_bilinear / blp_topk_relations_wide_bilinear, as workload fb15k237-<model>-wide<D>.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blp_amd import ops  # noqa: E402

WORKLOADS = {
    "fb15k237-transe": dict(model="transe", S=14_541, D=128, Q=310_116, R=237),
    "fb15k237-distmult": dict(model="distmult", S=14_541, D=128, Q=310_116, R=237),
    "wikidata5m-transe": dict(model="transe", S=100_000, D=128, Q=1_000_000, R=822),
    "wikidata5m-distmult": dict(model="distmult", S=100_000, D=128, Q=1_000_000, R=822),
}
K = 10
PIECE_BYTES = 1 << 28
ROOF_LANE_OPS = 78.6e12
OPS_PER_COLUMN = {"transe": 3, "distmult": 3, "complex": 6, "simple": 3}


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


def summary(medians):
    a = np.asarray(medians)
    mid = float(np.median(a))
    return {"median_ms": round(mid, 4), "spread": round(float((a.max() - a.min()) / mid), 4), "medians_ms": [round(float(x), 4) for x in a]}


def run(name, cfg, steps, warmup, repeats, wide=False):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    S, D, Q, R, model = cfg["S"], cfg["D"], cfg["Q"], cfg["R"], cfg["model"]
    source = torch.randn((S, D), generator=g, device=dev)
    source = torch.nn.functional.normalize(source, dim=-1) if model == "transe" else source * 0.1
    rel_w = torch.randn((R, D), generator=g, device=dev) * 0.1
    hr = torch.randint(0, S, (Q,), generator=g, device=dev)
    tr = torch.randint(0, S, (Q,), generator=g, device=dev)
    true = torch.randint(0, R, (Q,), generator=g, device=dev)
    u = torch.randint(0, R - 2, (Q,), generator=g, device=dev)
    cols = torch.stack(((true + 1 + u) % R, (true + 1 + (u + 1) % (R - 1)) % R), 1).reshape(-1).contiguous()  # two others, distinct
    lo = torch.arange(Q, device=dev) * 2
    rowptr = torch.arange(Q + 1, device=dev) * 2
    filt = ops.SegmentFilter(lo, lo + 2, cols, None, None, 0)
    piece = max(1, PIECE_BYTES // (4 * R))
    rels = rel_w.unsqueeze(0)
    owner = torch.arange(Q, device=dev).repeat_interleave(2)
    res = {}
    rank_fn, topk_fn = (ops.rank_relations, ops.topk_relations)
    if wide:
        rank_fn, topk_fn = (ops.rank_relations_wide, ops.topk_relations_wide) if model == "transe" else \
            (ops.rank_relations_wide_bilinear, ops.topk_relations_wide_bilinear)

    def matrix(a, b):
        return ops.score(model, source[hr[a:b]].unsqueeze(1), source[tr[a:b]].unsqueeze(1), rels)

    def fused_counts():
        res["fc"] = rank_fn(model, source, hr, tr, rel_w, true, filter=filt)

    def yard_counts():
        out = torch.empty((Q, 4), dtype=torch.int32, device=dev)
        for a in range(0, Q, piece):
            b = min(a + piece, Q)
            out[a:b] = ops.rank_from_scores(matrix(a, b), true_idx=true[a:b], filt_rowptr=rowptr[a:b + 1] - 2 * a, filt_col=cols[2 * a:2 * b])
        res["yc"] = out

    def fused_topk():
        res["ft"] = topk_fn(model, source, hr, tr, rel_w, K, filter=filt)

    def yard_topk():
        ids = torch.empty((Q, K), dtype=torch.int64, device=dev)
        val = torch.empty((Q, K), dtype=torch.float32, device=dev)
        for a in range(0, Q, piece):
            b = min(a + piece, Q)
            s = matrix(a, b)
            s[owner[2 * a:2 * b] - a, cols[2 * a:2 * b]] = float("-inf")  # removed: behind every number (K << R - 2)
            v, i = torch.sort(s, dim=1, descending=True, stable=True)
            ids[a:b], val[a:b] = i[:, :K], v[:, :K]
        res["yt"] = (ids, val)

    for fn in (fused_counts, yard_counts, fused_topk, yard_topk):
        fn()
    torch.cuda.synchronize()
    counts_equal = bool(torch.equal(res["fc"], res["yc"]))
    topk_equal = bool(torch.equal(res["ft"][0], res["yt"][0]) and torch.equal(res["ft"][1].view(torch.int32), res["yt"][1].view(torch.int32)))
    calls = {"fused_counts": fused_counts, "yard_counts": yard_counts, "fused_topk": fused_topk, "yard_topk": yard_topk}
    extra = {}
    if wide and ops.rank_relations_supported(model, D):  # the register kernels on the same inputs, in the same alternation
        def register_counts():
            res["rc"] = ops.rank_relations(model, source, hr, tr, rel_w, true, filter=filt)

        def register_topk():
            res["rt"] = ops.topk_relations(model, source, hr, tr, rel_w, K, filter=filt)
        register_counts(), register_topk()
        torch.cuda.synchronize()
        extra["counts_equal_register"] = bool(torch.equal(res["fc"], res["rc"]))
        extra["topk_equal_register"] = bool(torch.equal(res["ft"][0], res["rt"][0]) and
                                            torch.equal(res["ft"][1].view(torch.int32), res["rt"][1].view(torch.int32)))
        calls.update(register_counts=register_counts, register_topk=register_topk)
    runs = [measure(calls, steps, warmup) for _ in range(repeats)]
    s = {n: summary([r[n] for r in runs]) for n in runs[0]}
    lane_ops = Q * R * D * OPS_PER_COLUMN[model]
    roof = lambda n: round(lane_ops / (s[n]["median_ms"] * 1e-3) / ROOF_LANE_OPS, 4)
    if "register_counts" in s:
        extra["counts_wide_over_register"] = round(s["fused_counts"]["median_ms"] / s["register_counts"]["median_ms"], 2)
        extra["topk_wide_over_register"] = round(s["fused_topk"]["median_ms"] / s["register_topk"]["median_ms"], 2)
    return {"workload": name, **cfg, "k": K, "filter_entries_per_query": 2, "steps": steps, "warmup": warmup, "repeats": repeats,
            "counts_equal_yardstick": counts_equal, "topk_equal_yardstick": topk_equal, **s,
            "counts_yardstick_over_fused": round(s["yard_counts"]["median_ms"] / s["fused_counts"]["median_ms"], 2),
            "topk_yardstick_over_fused": round(s["yard_topk"]["median_ms"] / s["fused_topk"]["median_ms"], 2),
            "counts_roof_fraction": roof("fused_counts"), "topk_roof_fraction": roof("fused_topk"), **extra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--out")
    ap.add_argument("--width", type=int, nargs="*", help="the fb15k237 shape at these widths through the any-width calls")
    ap.add_argument("--model", nargs="*", default=["transe"], choices=sorted(OPS_PER_COLUMN), help="with --width: these models")
    args = ap.parse_args()
    workloads = WORKLOADS
    if args.width:
        workloads = {f"fb15k237-{m}-wide{D}": dict(WORKLOADS["fb15k237-transe"], model=m, D=D) for m in args.model for D in args.width}
    for name, cfg in workloads.items():
        if args.only and name not in args.only:
            continue
        line = json.dumps(run(name, cfg, args.steps, args.warmup, args.repeats, wide=bool(args.width)))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        ops.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
