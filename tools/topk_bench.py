"""Time blp_topk (filtered top-k prediction) next to the ranking call it is compared with, on bench.py's shapes.

For each workload: the same queries, the same filter; the two calls alternate step by step in one process, each bracketed by
device events; warm-up, then --steps steps; one JSON line with the median and p90 of both and their ratio.

    python tools/topk_bench.py [--steps 30] [--warmup 5] [--only NAME ...]

  wikidata5m-{transe,complex}   4.6 M x 128, 4 queries (2 triples), k = 10, filtered  vs blp_rank_all_shard (default route)
  fb15k237-{transe,distmult}    14 541 x 128, 105 740 queries, k = 10, filtered    vs the exact ranking kernels (hooks
                                build, rank_kernel = 1; both calls on the hooks build)
  fb15k237-transe-128q          128 queries of the same table, k = 10                vs blp_rank_all_shard (default route)
  fb15k237-transe-ties5pct      the ties5pct table (5 % of the rows per cluster centre), k = 10 vs the random table's top-k

    python tools/topk_bench.py --table16 {float16,bfloat16} [...]

  the same workloads with the table rounded to the 16-bit type: blp_topk_typed on the 16-bit copy, timed alternately against
  blp_topk on the same values widened to float32 (the queries' vectors are the widened rows in both calls); the ties5pct
  workload is not run.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from blp_amd import _lib, ops  # noqa: E402

HBM_TBS = 8.0          # MI355X peak HBM bandwidth
F32_LANE_OPS = 78.6e12  # f32 lane-ops / s (non-packed VALU)


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()


def measure(calls, steps, warmup):
    """calls: {name: fn}; the functions alternate every step.  Returns {name: [ms, ...]}."""
    ev = {n: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for n in calls}
    out = {n: [] for n in calls}
    for i in range(warmup + steps):
        for n, fn in calls.items():
            timed(fn, *ev[n])
        torch.cuda.synchronize()
        if i >= warmup:
            for n in calls:
                out[n].append(ev[n][0].elapsed_time(ev[n][1]))
    return out


def stats(ms):
    a = np.asarray(ms)
    return {"median": round(float(np.median(a)), 4), "p90": round(float(np.percentile(a, 90)), 4)}


def problem(name, triples=None):
    cfg = dict(bench.WORKLOADS[name])
    dev = torch.device("cuda", 0)
    table, rel_w, heads, tails, rels = bench.make_data(cfg, dev, sort=False)
    if triples is not None:
        heads, tails, rels = heads[:triples], tails[:triples], rels[:triples]
    T = heads.shape[0]
    index = bench.make_filter_index(cfg, heads, tails, rels)
    trip = torch.stack((heads, tails, rels), dim=1)
    filt = index.segments(trip, torch.arange(cfg["N"], device=dev), dev)
    return dict(cfg=cfg, table=table, rel=rel_w, fixed=torch.cat((tails, heads)), rel_ids=torch.cat((rels, rels)),
                true=torch.cat((heads, tails)), q_head=T, filter=filt)


def run(name, label, p, k, steps, warmup, against="rank", hooks_exact=False, other=None):
    model = p["cfg"]["model"]
    t = p["table"]
    N, D = t.shape
    Q = p["fixed"].shape[0]
    topk = lambda: ops.topk(model, t, t, p["fixed"], p["rel"], p["rel_ids"], p["q_head"], k, filter=p["filter"])
    calls = {"topk": topk}
    if against == "rank":
        calls["rank"] = lambda: ops.rank_all_shard(model, t, t, p["fixed"], p["rel"], p["rel_ids"], p["q_head"], p["true"],
                                                   filter=p["filter"])
    else:  # the random-table twin's top-k
        o = other
        calls["twin_topk"] = lambda: ops.topk(model, o["table"], o["table"], o["fixed"], o["rel"], o["rel_ids"], o["q_head"], k,
                                              filter=o["filter"])
    if hooks_exact:
        _lib.set_knob("rank_kernel", 1)
    try:
        ms = measure(calls, steps, warmup)
    finally:
        _lib.reset_knobs()
    res = {"workload": label, "model": model, "N": N, "D": D, "Q": Q, "k": k, "filtered": True,
           "steps": steps, "warmup": warmup}
    for n, v in ms.items():
        res[f"{n}_ms"] = stats(v)
    base = "rank_ms" if against == "rank" else "twin_topk_ms"
    res["ratio_median"] = round(res["topk_ms"]["median"] / res[base]["median"], 3)
    if hooks_exact:
        res["rank_route"] = "exact f32 kernels (hooks build, rank_kernel = 1)"
    tk = res["topk_ms"]["median"] * 1e-3
    res["hbm_tbs"] = round(N * D * 4 / tk / 1e12, 3)
    res["hbm_frac"] = round(res["hbm_tbs"] / HBM_TBS, 3)
    res["f32_roof_frac"] = round(2.0 * Q * N * D / F32_LANE_OPS / tk, 3)
    print(json.dumps(res), flush=True)
    return res


def run16(label, p, k, steps, warmup, dtype):
    model = p["cfg"]["model"]
    t16 = p["table"].to(dtype)
    wide = t16.float()
    del p["table"]
    torch.cuda.empty_cache()
    N, D = t16.shape
    Q = p["fixed"].shape[0]
    args = (p["fixed"], p["rel"], p["rel_ids"], p["q_head"], k)
    calls = {"topk16": lambda: ops.topk(model, t16, wide, *args, filter=p["filter"]),
             "topk": lambda: ops.topk(model, wide, wide, *args, filter=p["filter"])}
    a, b = calls["topk16"](), calls["topk"]()
    same = torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    ms = measure(calls, steps, warmup)
    res = {"workload": label, "table": str(dtype).replace("torch.", ""), "model": model, "N": N, "D": D, "Q": Q, "k": k,
           "filtered": True, "steps": steps, "warmup": warmup, "same_as_f32": same}
    for n, v in ms.items():
        res[f"{n}_ms"] = stats(v)
    res["ratio_median"] = round(res["topk16_ms"]["median"] / res["topk_ms"]["median"], 3)
    tk = res["topk16_ms"]["median"] * 1e-3
    res["hbm_tbs"] = round(N * D * 2 / tk / 1e12, 3)
    res["hbm_frac"] = round(res["hbm_tbs"] / HBM_TBS, 3)
    print(json.dumps(res), flush=True)
    return res


def main16(a):
    dtype = getattr(torch, a.table16)
    want = lambda n: a.only is None or n in a.only
    for model in ("transe", "complex"):
        label = f"wikidata5m-{model}"
        if want(label):
            run16(label, problem(label, triples=2), a.k, a.steps, a.warmup, dtype)
            torch.cuda.empty_cache()
    for model in ("transe", "distmult"):
        label = f"fb15k237-{model}"
        if want(label):
            run16(label, problem(label), a.k, a.steps, a.warmup, dtype)
    if want("fb15k237-transe-128q"):
        run16("fb15k237-transe-128q", problem("fb15k237-transe", triples=64), a.k, a.steps, a.warmup, dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--table16", choices=("float16", "bfloat16"), default=None)
    a = ap.parse_args()
    if a.table16:
        return main16(a)
    want = lambda n: a.only is None or n in a.only
    for model in ("transe", "complex"):
        label = f"wikidata5m-{model}"
        if want(label):
            p = problem(label, triples=2)
            run(label, label, p, a.k, a.steps, a.warmup)
            del p
            torch.cuda.empty_cache()
    for model in ("transe", "distmult"):
        label = f"fb15k237-{model}"
        if want(label):
            run(label, label, problem(label), a.k, a.steps, a.warmup, hooks_exact=True)
    if want("fb15k237-transe-128q"):
        run("fb15k237-transe", "fb15k237-transe-128q", problem("fb15k237-transe", triples=64), a.k, a.steps, a.warmup)
    if want("fb15k237-transe-ties5pct"):
        run("fb15k237-transe-ties5pct", "fb15k237-transe-ties5pct", problem("fb15k237-transe-ties5pct"), a.k, a.steps, a.warmup,
            against="twin", other=problem("fb15k237-transe"))


if __name__ == "__main__":
    main()
