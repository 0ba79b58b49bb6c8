"""Time blp_rank_sets (counts against candidate sets shared by groups of queries, filtered) next to the route the library
offered for the same job before it: blp_rank_lists on the sets expanded into one list per query.

For each workload: the same queries, sets and filter; the expansion is done once, outside the timing (the lists of the expanded
route are cut into calls of < 2^30 entries, blp_rank_lists' limit being 2^31 - 1); the counts of the two routes must be equal
before anything is timed.  The two routes alternate step by step in one process, each bracketed by device events; warm-up,
then --steps steps; one JSON line with the median and p90 of both, their ratio and the achieved gather bandwidth of the new
call (rows fetched: one per set entry and chunk of 128 queries of its group, D x 4 bytes each).

    python tools/rank_sets_bench.py [--steps 30] [--warmup 3] [--only NAME ...] [--out FILE.jsonl] [--table16 {f16,bf16}]
                                    [--width D [D ...]] [--repeats 5] [--model {distmult,complex,simple}]

--table16: the table rounded to IEEE half / bfloat16 instead; blp_rank_sets_typed on the 16-bit table alternates with
blp_rank_sets on that table widened to f32 (the yardstick), counts required equal first; one JSON line with both medians,
their ratio (16-bit over f32) and the gather bandwidth of the 16-bit call (D x 2 bytes per fetched row).

--width D [D ...] (combinable with --table16): blp_rank_sets_wide -- TransE at any width -- on the fb15k237-transe shape at
width D (105 740 queries, 474 sets, 14 541 rows).  At the widths blp_rank_sets takes (64 / 128 / 256) it alternates with
blp_rank_sets, elsewhere (300, 768) with blp_rank_lists on the expanded lists; counts required equal first; --repeats
measurements of --steps steps each, one JSON line with the median of the medians of both routes, their ratio and the spread of
the repeated medians ((max - min) / median).

--model {distmult,complex,simple} (with --width): blp_rank_sets_wide_bilinear -- these models at any width, an f32 table -- on the
same shape.  Its counts must equal those of the dense route (ranking._rank_sets_dense: score_fn on gathered rows, what
rank_in_sets took for these shapes before) and, at the widths blp_rank_lists takes these models (64 / 128 / 256), those of
blp_rank_lists on the expanded lists; then the routes alternate step by step, and one JSON line has the median of the repeated
medians of each with its spread, the ratios to the new call, and whether the new call is faster than the dense route by more
than both spreads together.  At 64 / 128 / 256 blp_rank_sets is timed as well (for the record: it keeps those widths).

  fb15k237-{transe,distmult}   105 740 queries, 14 541 x 128 table, 474 sets of 50 .. 8 000 rows (log-uniform)
  longtable-transe             13 788 queries, 4.6 M x 128 table, 1 644 sets of 10^3 .. 10^6 rows (log-uniform)
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
    "fb15k237-transe": dict(model="transe", N=14_541, D=128, Q=105_740, G=474, set_min=50, set_max=8000),
    "fb15k237-distmult": dict(model="distmult", N=14_541, D=128, Q=105_740, G=474, set_min=50, set_max=8000),
    "longtable-transe": dict(model="transe", N=4_600_000, D=128, Q=13_788, G=1644, set_min=1000, set_max=1_000_000),
}
FILTER_PER_QUERY = 8  # entries of a query's filter segment, half of them members of its set
MAX_LIST_ENTRIES = 1 << 30
QUERY_CHUNK = 128


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


def make_workload(cfg):
    """The table, relations, sets, grouped queries and filter of a workload, on the device."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    N, D, Q, G = cfg["N"], cfg["D"], cfg["Q"], cfg["G"]
    table = torch.randn((N, D), generator=g, device=dev)
    table = torch.nn.functional.normalize(table, dim=-1) if cfg["model"] == "transe" else table * 0.1
    R = 237
    rel_w = (torch.rand((R, D), generator=g, device=dev) - 0.5) * 0.25
    sizes = np.exp(rng.uniform(np.log(cfg["set_min"]), np.log(cfg["set_max"]), G)).astype(np.int64)
    set_ptr = torch.zeros(G + 1, dtype=torch.long, device=dev)
    set_ptr[1:] = torch.cumsum(torch.from_numpy(sizes).to(dev), 0)
    set_row = torch.cat([torch.randperm(N, generator=g, device=dev)[:int(n)].sort().values for n in sizes])
    q_head = Q // 2
    ids = torch.cat((torch.randint(0, G, (q_head,), generator=g, device=dev).sort().values,
                     torch.randint(0, G, (Q - q_head,), generator=g, device=dev).sort().values))
    qh = torch.zeros(G + 1, dtype=torch.long, device=dev)
    qt = torch.zeros(G + 1, dtype=torch.long, device=dev)
    qh[1:] = torch.cumsum(torch.bincount(ids[:q_head], minlength=G), 0)
    qt[1:] = torch.cumsum(torch.bincount(ids[q_head:], minlength=G), 0)
    fixed = torch.randint(0, N, (Q,), generator=g, device=dev)
    true = torch.randint(0, N, (Q,), generator=g, device=dev)
    rel_ids = torch.randint(0, R, (Q,), generator=g, device=dev)
    n_per = (set_ptr[1:] - set_ptr[:-1])[ids]
    first = set_ptr[ids]
    # a value occurs once per filter segment (blp_filter's contract): consecutive members of the set, distinct other rows, and
    # -1 (removes nothing) where one of those is a listed member already
    half = FILTER_PER_QUERY // 2
    k = torch.arange(half, device=dev).unsqueeze(0)
    inside = set_row[first.unsqueeze(1) + (torch.randint(0, 1 << 30, (Q, 1), generator=g, device=dev) + k) % n_per.unsqueeze(1)]
    other = (torch.randint(0, N, (Q, 1), generator=g, device=dev) + k * 3571) % N
    other = torch.where((other.unsqueeze(2) == inside.unsqueeze(1)).any(2), torch.full_like(other, -1), other)
    seg = torch.cat((inside, other), 1)
    lo = torch.arange(Q, device=dev) * FILTER_PER_QUERY
    filt = ops.SegmentFilter(lo, lo + FILTER_PER_QUERY, seg.reshape(-1).contiguous(), None, None, 0)
    counts = torch.empty((Q, 4), dtype=torch.int32, device=dev)
    return dict(table=table, rel_w=rel_w, set_ptr=set_ptr, set_row=set_row, q_head=q_head, qh=qh, qt=qt, fixed=fixed, true=true,
                rel_ids=rel_ids, n_per=n_per, first=first, filt=filt, counts=counts)


def expanded_calls(w, Q):
    """The sets expanded into per-query lists, in calls of at most MAX_LIST_ENTRIES entries, each of one side:
    [(a, b, list_ptr, list_row, filter)] and the number of (query, row) pairs."""
    dev, n_per, q_head, filt = w["table"].device, w["n_per"], w["q_head"], w["filt"]
    list_ptr_all = torch.zeros(Q + 1, dtype=torch.long, device=dev)
    list_ptr_all[1:] = torch.cumsum(n_per, 0)
    host_ptr = list_ptr_all.tolist()
    calls, a = [], 0
    while a < Q:
        end = q_head if a < q_head else Q
        b = a + 1
        while b < end and host_ptr[b + 1] - host_ptr[a] <= MAX_LIST_ENTRIES:
            b += 1
        n = host_ptr[b] - host_ptr[a]
        owner = torch.repeat_interleave(torch.arange(a, b, device=dev), n_per[a:b], output_size=n)
        rows = w["set_row"][w["first"][owner] + torch.arange(host_ptr[a], host_ptr[b], device=dev) - list_ptr_all[owner]]
        del owner
        part = ops.SegmentFilter(filt.seg_lo[a:b].contiguous(), filt.seg_hi[a:b].contiguous(), filt.values, None, None, 0)
        calls.append((a, b, (list_ptr_all[a:b + 1] - host_ptr[a]).contiguous(), rows, part))
        a = b
    return calls, host_ptr[Q]


def run(name, cfg, steps, warmup, table16=None):
    w = make_workload(cfg)
    N, D, Q, G = cfg["N"], cfg["D"], cfg["Q"], cfg["G"]
    table, rel_w, set_ptr, set_row, q_head, qh, qt = (w[k] for k in ("table", "rel_w", "set_ptr", "set_row", "q_head", "qh", "qt"))
    fixed, true, rel_ids, n_per, filt, counts = (w[k] for k in ("fixed", "true", "rel_ids", "n_per", "filt", "counts"))
    dev = table.device
    if table16:  # (the f32 original is not kept: the 16-bit copy and its widened image replace it)
        small = table.to({"f16": torch.float16, "bf16": torch.bfloat16}[table16])
        del table
        w.clear()
        return run16(name, cfg, steps, warmup, table16, small, rel_w, fixed, true, rel_ids, q_head, set_ptr, set_row, qh, qt, filt, counts)

    def fused():
        ops.rank_sets(cfg["model"], table, table, fixed, rel_w, rel_ids, q_head, true, set_ptr, set_row, qh, qt, filter=filt, out=counts)

    calls, _ = expanded_calls(w, Q)  # outside the timing
    expanded_counts = torch.empty((Q, 4), dtype=torch.int32, device=dev)

    def expanded():
        for a, b, ptr, rows, part in calls:
            ops.rank_lists(cfg["model"], table, table, fixed[a:b], rel_w, rel_ids[a:b], min(max(q_head - a, 0), b - a), ptr, rows,
                           true_row=true[a:b], filter=part, out=(expanded_counts[a:b], None))

    fused()
    expanded()
    same = bool(torch.equal(counts, expanded_counts))
    if not same:
        return {"workload": name, **cfg, "counts_equal": False}
    ms = measure({"sets": fused, "expanded_lists": expanded}, steps, warmup)
    s, e = stats(ms["sets"]), stats(ms["expanded_lists"])
    chunks = (torch.div(qh[1:] - qh[:-1] + QUERY_CHUNK - 1, QUERY_CHUNK, rounding_mode="floor") +
              torch.div(qt[1:] - qt[:-1] + QUERY_CHUNK - 1, QUERY_CHUNK, rounding_mode="floor"))
    fetched = int(((set_ptr[1:] - set_ptr[:-1]) * chunks).sum()) * D * 4
    pairs = int(n_per.sum())
    return {"workload": name, **cfg, "set_entries": int(set_row.numel()), "pairs": pairs, "expanded_calls": len(calls),
            "expanded_index_bytes": pairs * 8, "filter_entries_per_query": FILTER_PER_QUERY, "counts_equal": same, "sets_ms": s,
            "expanded_lists_ms": e, "expanded_over_sets": round(e["median"] / s["median"], 2), "fetched_bytes": fetched,
            "gather_TBps": round(fetched / (s["median"] * 1e-3) / 1e12, 3),
            "pairs_per_s": round(pairs / (s["median"] * 1e-3), 0), "steps": steps}


def run16(name, cfg, steps, warmup, table16, small, rel_w, fixed, true, rel_ids, q_head, set_ptr, set_row, qh, qt, filt, counts):
    """blp_rank_sets_typed on the 16-bit table next to blp_rank_sets on that table widened to f32."""
    D, Q = cfg["D"], cfg["Q"]
    wide = small.float()
    counts16 = torch.empty_like(counts)
    # the queries' f32 vectors: the Q fixed rows, then the Q true rows, widened (blp_gather_triple_vectors, as
    # ranking.rank_in_sets gathers them) -- the same source for both calls
    source = ops.gather_triple_vectors(torch.stack((fixed, true, torch.zeros_like(fixed)), dim=1), None, small)
    src_fixed, src_true = torch.arange(Q, device=wide.device), torch.arange(Q, 2 * Q, device=wide.device)

    def f32():
        ops.rank_sets(cfg["model"], wide, source, src_fixed, rel_w, rel_ids, q_head, src_true, set_ptr, set_row, qh, qt, filter=filt, out=counts)

    def t16():
        ops.rank_sets(cfg["model"], small, source, src_fixed, rel_w, rel_ids, q_head, src_true, set_ptr, set_row, qh, qt, filter=filt, out=counts16)

    f32()
    t16()
    same = bool(torch.equal(counts, counts16))
    if not same:
        return {"workload": name, **cfg, "table16": table16, "counts_equal": False}
    ms = measure({"f32": f32, "table16": t16}, steps, warmup)
    a, b = stats(ms["f32"]), stats(ms["table16"])
    chunks = (torch.div(qh[1:] - qh[:-1] + QUERY_CHUNK - 1, QUERY_CHUNK, rounding_mode="floor") +
              torch.div(qt[1:] - qt[:-1] + QUERY_CHUNK - 1, QUERY_CHUNK, rounding_mode="floor"))
    fetched_rows = int(((set_ptr[1:] - set_ptr[:-1]) * chunks).sum())
    return {"workload": name, **cfg, "table16": table16, "set_entries": int(set_row.numel()), "filter_entries_per_query": FILTER_PER_QUERY,
            "counts_equal": same, "f32_ms": a, "table16_ms": b, "table16_over_f32": round(b["median"] / a["median"], 3),
            "fetched_bytes_table16": fetched_rows * D * 2, "gather_TBps_table16": round(fetched_rows * D * 2 / (b["median"] * 1e-3) / 1e12, 3),
            "gather_TBps_f32": round(fetched_rows * D * 4 / (a["median"] * 1e-3) / 1e12, 3), "steps": steps}


def repeated(runs, name):
    a = np.asarray([float(np.median(r[name])) for r in runs])
    mid = float(np.median(a))
    return {"median_ms": round(mid, 4), "spread": round(float((a.max() - a.min()) / mid), 4), "medians_ms": [round(float(x), 4) for x in a]}


def run_wide(D, steps, warmup, repeats, table16=None):
    """blp_rank_sets_wide at width D on the fb15k237-transe shape, next to blp_rank_sets (64 / 128 / 256) or to blp_rank_lists
    on the expanded lists (any other width)."""
    cfg = dict(WORKLOADS["fb15k237-transe"], D=int(D))
    w = make_workload(cfg)
    Q = cfg["Q"]
    table, source, fixed, true = w["table"], w["table"], w["fixed"], w["true"]
    if table16:  # the 16-bit table as it is; the queries' f32 vectors gathered and widened, as ranking.rank_in_sets does
        table = table.to({"f16": torch.float16, "bf16": torch.bfloat16}[table16])
        source = ops.gather_triple_vectors(torch.stack((fixed, true, torch.zeros_like(fixed)), dim=1), None, table)
        fixed, true = torch.arange(Q, device=table.device), torch.arange(Q, 2 * Q, device=table.device)
    sets_args = (w["rel_w"], w["rel_ids"], w["q_head"], true, w["set_ptr"], w["set_row"], w["qh"], w["qt"])
    counts, other_counts = w["counts"], torch.empty_like(w["counts"])

    def wide():
        ops.rank_sets_wide("transe", table, source, fixed, *sets_args, filter=w["filt"], out=counts)

    pairs = int(w["n_per"].sum())
    if ops.rank_sets_supported("transe", D, table.dtype):
        other_name = "rank_sets"

        def other():
            ops.rank_sets("transe", table, source, fixed, *sets_args, filter=w["filt"], out=other_counts)
    else:
        other_name = "expanded_lists"
        calls, _ = expanded_calls(w, Q)  # outside the timing

        def other():
            for a, b, ptr, rows, part in calls:
                ops.rank_lists("transe", table, source, fixed[a:b], w["rel_w"], w["rel_ids"][a:b], min(max(w["q_head"] - a, 0), b - a), ptr,
                               rows, true_row=true[a:b], filter=part, out=(other_counts[a:b], None))

    wide()
    other()
    same = bool(torch.equal(counts, other_counts))
    head = {"workload": f"fb15k237-transe-wide-{D}", **cfg, "table16": table16, "against": other_name, "counts_equal": same}
    if not same:
        return head
    runs = [measure({"wide": wide, "other": other}, steps, warmup) for _ in range(repeats)]
    a, b = repeated(runs, "wide"), repeated(runs, "other")
    return {**head, "set_entries": int(w["set_row"].numel()), "pairs": pairs, "filter_entries_per_query": FILTER_PER_QUERY,
            "sets_wide_ms": a, f"{other_name}_ms": b, f"{other_name}_over_sets_wide": round(b["median_ms"] / a["median_ms"], 3),
            "pairs_per_s": round(pairs / (a["median_ms"] * 1e-3), 0), "steps": steps, "warmup": warmup, "repeats": repeats}


def run_wide_bilinear(model, D, steps, warmup, repeats):
    """blp_rank_sets_wide_bilinear at width D on the fb15k237 shape, next to the dense route and, where they take the shape, to
    blp_rank_lists on the expanded lists and to blp_rank_sets."""
    from blp_amd import models, ranking
    cfg = dict(WORKLOADS["fb15k237-distmult"], model=model, D=int(D))
    w = make_workload(cfg)
    Q, table, filt = cfg["Q"], w["table"], w["filt"]
    sets_args = (w["rel_w"], w["rel_ids"], w["q_head"], w["true"], w["set_ptr"], w["set_row"], w["qh"], w["qt"])
    got = {name: torch.empty_like(w["counts"]) for name in ("wide_bilinear", "dense", "expanded_lists", "rank_sets")}
    module = models.LinkPrediction(int(D), model, "margin", w["rel_w"].shape[0], 0)
    dense_filt = (filt.seg_lo, filt.seg_hi, filt.values, filt.exclude, filt.ent2idx)

    def wide_bilinear():
        ops.rank_sets_wide_bilinear(model, table, table, w["fixed"], *sets_args, filter=filt, out=got["wide_bilinear"])

    def dense():  # the gathers of the query vectors are part of the route, as in ranking.rank_in_sets
        got["dense"] = ranking._rank_sets_dense(module.score_fn, table, table[w["fixed"]].float(), w["rel_w"][w["rel_ids"]],
                                                table[w["true"]].float(), w["q_head"], w["set_ptr"], w["set_row"], w["qh"], w["qt"], 0,
                                                dense_filt)

    calls = {"wide_bilinear": wide_bilinear, "dense": dense}
    if ops.rank_lists_supported(model, D, table.dtype):
        lists, _ = expanded_calls(w, Q)  # outside the timing

        def expanded_lists():
            for a, b, ptr, rows, part in lists:
                ops.rank_lists(model, table, table, w["fixed"][a:b], w["rel_w"], w["rel_ids"][a:b], min(max(w["q_head"] - a, 0), b - a), ptr,
                               rows, true_row=w["true"][a:b], filter=part, out=(got["expanded_lists"][a:b], None))

        calls["expanded_lists"] = expanded_lists
    if ops.rank_sets_supported(model, D, table.dtype):
        calls["rank_sets"] = lambda: ops.rank_sets(model, table, table, w["fixed"], *sets_args, filter=filt, out=got["rank_sets"])
    with torch.no_grad():
        for fn in calls.values():
            fn()
        equal = {name: bool(torch.equal(got["wide_bilinear"], got[name])) for name in calls if name != "wide_bilinear"}
        head = {"workload": f"fb15k237-{model}-wide-{D}", **cfg, "counts_equal": equal,
                "not_timed": [n for n in ("expanded_lists", "rank_sets") if n not in calls]}
        assert all(equal.values()), head
        runs = [measure(calls, steps, warmup) for _ in range(repeats)]
    rec = {name: repeated(runs, name) for name in calls}
    new = rec["wide_bilinear"]
    ratios = {f"{name}_over_wide_bilinear": round(rec[name]["median_ms"] / new["median_ms"], 3) for name in calls if name != "wide_bilinear"}
    faster = bool(rec["dense"]["median_ms"] * (1 - rec["dense"]["spread"]) > new["median_ms"] * (1 + new["spread"]))
    pairs = int(w["n_per"].sum())
    return {**head, "set_entries": int(w["set_row"].numel()), "pairs": pairs, "filter_entries_per_query": FILTER_PER_QUERY,
            **{f"{name}_ms": r for name, r in rec.items()}, **ratios, "faster_than_dense_by_more_than_both_spreads": faster,
            "pairs_per_s": round(pairs / (new["median_ms"] * 1e-3), 0), "steps": steps, "warmup": warmup, "repeats": repeats}


def emit(line, out):
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as fh:
            fh.write(line + "\n")
    ops.release_workspaces()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--out")
    ap.add_argument("--table16", choices=("f16", "bf16"))
    ap.add_argument("--width", type=int, nargs="+", help="blp_rank_sets_wide at these widths on the fb15k237-transe shape")
    ap.add_argument("--repeats", type=int, default=5, help="with --width: measurements whose medians' spread is reported")
    ap.add_argument("--model", choices=("distmult", "complex", "simple"),
                    help="with --width: blp_rank_sets_wide_bilinear for this model instead of blp_rank_sets_wide for TransE")
    args = ap.parse_args()
    if args.model and (not args.width or args.table16):
        ap.error("--model goes with --width and an f32 table")
    if args.model:
        for D in args.width:
            emit(json.dumps(run_wide_bilinear(args.model, D, args.steps, args.warmup, args.repeats)), args.out)
        return
    for D in args.width or ():
        emit(json.dumps(run_wide(D, args.steps, args.warmup, args.repeats, args.table16)), args.out)
    if args.width:
        return
    for name, cfg in WORKLOADS.items():
        if args.only and name not in args.only:
            continue
        emit(json.dumps(run(name, cfg, args.steps, args.warmup, args.table16)), args.out)


if __name__ == "__main__":
    main()
