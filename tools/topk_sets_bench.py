"""Time blp_topk_sets (filtered top-k inside candidate sets shared by groups of queries) next to what the library offered for
the same job before it: blp_rank_lists with scores on the sets expanded into one list per query, followed by a device-side
per-query stable top-k of those scores.

For each workload: the same queries, sets and filter (tools/rank_sets_bench.py's workloads), k = 10; the expansion is done
once, outside the timing (the lists of the expanded route are cut into calls of < 2^30 entries); rows and scores of the two
routes must be equal before anything is timed.  The two routes alternate step by step in one process, each bracketed by
device events; warm-up, then --steps steps; one JSON line with the median and p90 of both, their ratio, the share of the
expanded route spent in blp_rank_lists, and the gather bandwidth of the new call (rows fetched: one per set entry and chunk of
topk_chunk(k) = 32 queries of its group, D x 4 bytes each).

    python tools/topk_sets_bench.py [--steps 30] [--warmup 3] [--only NAME ...] [--out profiles/topksets/topk_sets_bench.jsonl]
                                    [--table16 {f16,bf16}] [--no-expanded] [--repeats 3] [--width D [D ...]]

--table16: the table rounded to IEEE half / bfloat16 instead; blp_topk_sets_typed on the 16-bit table alternates with
blp_topk_sets on that table widened to f32 (the yardstick), rows and scores required equal first; the alternation is repeated
--repeats times, one JSON line with the median of every repeat for both calls, the f32 call's own spread over those medians,
the ratio (16-bit over f32) and the gather bandwidth of both calls.  The expanded route is not run.
--no-expanded: blp_topk_sets alone (the long table: the expanded route's flat sorts of 2 x 10^9 entries are not run), repeated
--repeats times.
--once NAME: one call of the workload after one of warm-up, nothing timed -- the program to put under a kernel trace for the
split of the call by kernel (with --table16: the 16-bit call).

--width D [D ...] (combinable with --table16): blp_topk_sets_wide -- TransE at any width -- on the fb15k237-transe shape at
width D (105 740 queries, 474 sets, 14 541 rows), k = 10, the same filter.  At the widths blp_topk_sets takes (64 / 128 / 256)
it alternates with blp_topk_sets, elsewhere (300, 768) with the expanded route above; rows and scores required equal first; the
alternation is repeated --repeats times: medians of the repeats' medians with their spread.  Off 64 / 128 / 256 it also times
ranking.predict_links_in_sets end to end (host clock around a synchronised call: grouping, filter segments, the call, the
scatter back) next to the same call with the fused branch disabled -- the dense route.

  fb15k237-{transe,distmult}   105 740 queries, 14 541 x 128 table, 474 sets of 50 .. 8 000 rows (log-uniform)
  longtable-transe             13 788 queries, 4.6 M x 128 table, 1 644 sets of 10^3 .. 10^6 rows (log-uniform)
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from blp_amd import ops  # noqa: E402
from rank_sets_bench import FILTER_PER_QUERY, MAX_LIST_ENTRIES, WORKLOADS, measure, stats  # noqa: E402

K = 10
QUERY_CHUNK = 32  # topk_chunk(10)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "topksets", "topk_sets_bench.jsonl")


def stable_topk_of_lists(scores, rows, removed, owner_local, ptr_local, n_queries, k):
    """Per query the k best of its list by (score descending, -0 == +0, NaN last; ties by ascending row -- the lists are
    ascending), removed entries dropped: three stable device sorts over the flat entries, then the first k of every segment."""
    order = torch.sort(-scores, stable=True).indices                                     # descending; torch sorts NaN last
    order = order[torch.sort(removed[order].to(torch.uint8), stable=True).indices]       # removed entries after everything
    order = order[torch.sort(owner_local[order], stable=True).indices]                   # grouped by query, order kept
    n_per = ptr_local[1:] - ptr_local[:-1]
    left = n_per - torch.zeros_like(n_per).index_add_(0, owner_local, removed.to(n_per.dtype))
    slot = torch.arange(k, device=scores.device).unsqueeze(0)
    take = (ptr_local[:-1].unsqueeze(1) + slot).clamp(max=max(scores.shape[0] - 1, 0))
    ok = slot < left.unsqueeze(1)
    picked = order[take]
    out_rows = torch.where(ok, rows[picked], torch.full_like(picked, -1))
    out_scores = torch.where(ok, scores[picked], torch.full((n_queries, k), float("nan"), device=scores.device))
    return out_rows, out_scores


def spread(medians):
    """The spread of repeated medians, relative to their mean: (max - min) / mean."""
    return round((max(medians) - min(medians)) / (sum(medians) / len(medians)), 4)


def fetched_rows(set_ptr, qh, qt):
    chunks = (torch.div(qh[1:] - qh[:-1] + QUERY_CHUNK - 1, QUERY_CHUNK, rounding_mode="floor") +
              torch.div(qt[1:] - qt[:-1] + QUERY_CHUNK - 1, QUERY_CHUNK, rounding_mode="floor"))
    return int(((set_ptr[1:] - set_ptr[:-1]) * chunks).sum())


def run16(name, cfg, steps, warmup, table16, repeats, once, small, rel_w, fixed, rel_ids, q_head, set_ptr, set_row, qh, qt, filt, out):
    """blp_topk_sets_typed on the 16-bit table next to blp_topk_sets on that table widened to f32."""
    D, Q = cfg["D"], cfg["Q"]
    wide = small.float()
    out16 = (torch.empty_like(out[0]), torch.empty_like(out[1]))
    # the queries' f32 vectors: the Q fixed rows widened (blp_gather_triple_vectors, as ranking.predict_links_in_sets gathers
    # them) -- the same source for both calls
    source = ops.gather_triple_vectors(torch.stack((fixed, fixed, torch.zeros_like(fixed)), dim=1), None, small)[:Q]
    src_fixed = torch.arange(Q, device=wide.device)

    def f32():
        ops.topk_sets(cfg["model"], wide, source, src_fixed, rel_w, rel_ids, q_head, K, set_ptr, set_row, qh, qt, filter=filt, out=out)

    def t16():
        ops.topk_sets(cfg["model"], small, source, src_fixed, rel_w, rel_ids, q_head, K, set_ptr, set_row, qh, qt, filter=filt, out=out16)

    f32()
    t16()
    torch.cuda.synchronize()
    if once:
        return None
    nan = torch.isnan(out[1])
    same = bool(torch.equal(out16[0], out[0])) and bool(torch.equal(torch.isnan(out16[1]), nan)) and \
        bool(torch.equal(out16[1][~nan].view(torch.int32), out[1][~nan].view(torch.int32)))
    if not same:
        return {"workload": name, **cfg, "k": K, "table16": table16, "results_equal": False}
    a, b = [], []
    for _ in range(repeats):
        ms = measure({"f32": f32, "table16": t16}, steps, warmup)
        a.append(stats(ms["f32"])["median"])
        b.append(stats(ms["table16"])["median"])
    ma, mb = float(np.median(a)), float(np.median(b))
    rows = fetched_rows(set_ptr, qh, qt)
    return {"workload": name, **cfg, "k": K, "table16": table16, "set_entries": int(set_row.numel()),
            "filter_entries_per_query": FILTER_PER_QUERY, "results_equal": same, "f32_ms_medians": a, "table16_ms_medians": b,
            "f32_ms": round(ma, 4), "table16_ms": round(mb, 4), "f32_spread": spread(a), "table16_spread": spread(b),
            "table16_over_f32": round(mb / ma, 3), "fetched_bytes_table16": rows * D * 2,
            "gather_TBps_table16": round(rows * D * 2 / (mb * 1e-3) / 1e12, 3), "gather_TBps_f32": round(rows * D * 4 / (ma * 1e-3) / 1e12, 3),
            "steps": steps, "repeats": repeats}


def expanded_route(model, table, source, fixed, rel_w, rel_ids, q_head, Q, set_row, n_per, first, seg):
    """The expanded route: per-query lists in calls of at most MAX_LIST_ENTRIES entries, each of one side; what the filter
    removes is marked per entry once, outside the timing (blp_rank_lists' scores are unfiltered).  Returns (the route, its
    blp_rank_lists part alone, its rows, its scores, the calls)."""
    dev = table.device
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
        rows = set_row[first[owner] + torch.arange(host_ptr[a], host_ptr[b], device=dev) - list_ptr_all[owner]]
        removed = torch.zeros(n, dtype=torch.bool, device=dev)
        for j in range(FILTER_PER_QUERY):
            removed |= rows == seg[owner, j]
        calls.append((a, b, (list_ptr_all[a:b + 1] - host_ptr[a]).contiguous(), rows, removed, (owner - a).contiguous(),
                      torch.empty(n, dtype=torch.float32, device=dev)))
        del owner
        a = b
    exp_rows = torch.empty((Q, K), dtype=torch.int64, device=dev)
    exp_scores = torch.empty((Q, K), dtype=torch.float32, device=dev)

    def expanded_scores():
        for a, b, ptr, rows, removed, owner, scores in calls:
            ops.rank_lists(model, table, source, fixed[a:b], rel_w, rel_ids[a:b], min(max(q_head - a, 0), b - a), ptr, rows,
                           out=(None, scores))

    def expanded():
        expanded_scores()
        for a, b, ptr, rows, removed, owner, scores in calls:
            exp_rows[a:b], exp_scores[a:b] = stable_topk_of_lists(scores, rows, removed, owner, ptr, b - a, K)

    return expanded, expanded_scores, exp_rows, exp_scores, calls


def make_workload(cfg):
    """The workload of tools/rank_sets_bench.py's shapes for k = 10: table, relations, sets, grouped queries, the filter."""
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
    rel_ids = torch.randint(0, R, (Q,), generator=g, device=dev)
    n_per = (set_ptr[1:] - set_ptr[:-1])[ids]
    first = set_ptr[ids]
    # a value occurs once per filter segment: consecutive members of the set, distinct other rows, -1 where one of those is a
    # listed member already (tools/rank_sets_bench.py's filter)
    half = FILTER_PER_QUERY // 2
    kk = torch.arange(half, device=dev).unsqueeze(0)
    inside = set_row[first.unsqueeze(1) + (torch.randint(0, 1 << 30, (Q, 1), generator=g, device=dev) + kk) % n_per.unsqueeze(1)]
    other = (torch.randint(0, N, (Q, 1), generator=g, device=dev) + kk * 3571) % N
    other = torch.where((other.unsqueeze(2) == inside.unsqueeze(1)).any(2), torch.full_like(other, -1), other)
    seg = torch.cat((inside, other), 1)
    lo = torch.arange(Q, device=dev) * FILTER_PER_QUERY
    filt = ops.SegmentFilter(lo, lo + FILTER_PER_QUERY, seg.reshape(-1).contiguous(), None, None, 0)
    out = (torch.empty((Q, K), dtype=torch.int64, device=dev), torch.empty((Q, K), dtype=torch.float32, device=dev))
    return dict(table=table, rel_w=rel_w, set_ptr=set_ptr, set_row=set_row, q_head=q_head, ids=ids, qh=qh, qt=qt, fixed=fixed,
                rel_ids=rel_ids, n_per=n_per, first=first, seg=seg, filt=filt, out=out)


def run(name, cfg, steps, warmup, table16=None, with_expanded=True, repeats=3, once=False):
    D, Q, G = cfg["D"], cfg["Q"], cfg["G"]
    w = make_workload(cfg)
    table, rel_w, set_ptr, set_row, q_head, qh, qt = w["table"], w["rel_w"], w["set_ptr"], w["set_row"], w["q_head"], w["qh"], w["qt"]
    fixed, rel_ids, n_per, first, seg, filt, out = w["fixed"], w["rel_ids"], w["n_per"], w["first"], w["seg"], w["filt"], w["out"]
    del w

    if table16:  # (the f32 original is not kept: the 16-bit copy and its widened image replace it)
        small = table.to({"f16": torch.float16, "bf16": torch.bfloat16}[table16])
        del table
        return run16(name, cfg, steps, warmup, table16, repeats, once, small, rel_w, fixed, rel_ids, q_head, set_ptr, set_row, qh, qt, filt, out)

    def fused():
        ops.topk_sets(cfg["model"], table, table, fixed, rel_w, rel_ids, q_head, K, set_ptr, set_row, qh, qt, filter=filt, out=out)

    if once:
        fused()
        fused()
        torch.cuda.synchronize()
        return None
    if not with_expanded:
        fused()
        medians = [stats(measure({"topk_sets": fused}, steps, warmup)["topk_sets"])["median"] for _ in range(repeats)]
        m = float(np.median(medians))
        rows, pairs = fetched_rows(set_ptr, qh, qt), int(n_per.sum())
        return {"workload": name, **cfg, "k": K, "set_entries": int(set_row.numel()), "pairs": pairs,
                "filter_entries_per_query": FILTER_PER_QUERY, "topk_sets_ms_medians": medians, "topk_sets_ms": round(m, 4),
                "topk_sets_spread": spread(medians), "fetched_bytes": rows * D * 4, "gather_TBps": round(rows * D * 4 / (m * 1e-3) / 1e12, 3),
                "pairs_per_s": round(pairs / (m * 1e-3), 0), "valid_slots": int((out[0] >= 0).sum()),
                "workspace_bytes": ops.topk_sets_workspace_bytes(cfg["model"], D, q_head, Q - q_head, G, int(set_row.numel()), K),
                "steps": steps, "repeats": repeats}

    expanded, expanded_scores, exp_rows, exp_scores, calls = expanded_route(cfg["model"], table, table, fixed, rel_w, rel_ids, q_head, Q,
                                                                            set_row, n_per, first, seg)
    fused()
    expanded()
    nan = torch.isnan(exp_scores)
    same = bool(torch.equal(out[0], exp_rows)) and bool(torch.equal(torch.isnan(out[1]), nan)) and \
        bool(torch.equal(out[1][~nan].view(torch.int32), exp_scores[~nan].view(torch.int32)))
    if not same:
        return {"workload": name, **cfg, "k": K, "results_equal": False}
    ms = measure({"topk_sets": fused, "expanded_lists_topk": expanded, "expanded_lists_scores_only": expanded_scores}, steps, warmup)
    s, e, sc = stats(ms["topk_sets"]), stats(ms["expanded_lists_topk"]), stats(ms["expanded_lists_scores_only"])
    fetched = fetched_rows(set_ptr, qh, qt) * D * 4
    pairs = int(n_per.sum())
    return {"workload": name, **cfg, "k": K, "set_entries": int(set_row.numel()), "pairs": pairs, "expanded_calls": len(calls),
            "expanded_index_bytes": pairs * 8, "filter_entries_per_query": FILTER_PER_QUERY, "results_equal": same,
            "topk_sets_ms": s, "expanded_lists_topk_ms": e, "expanded_lists_scores_only_ms": sc,
            "expanded_over_topk_sets": round(e["median"] / s["median"], 2), "fetched_bytes": fetched,
            "gather_TBps": round(fetched / (s["median"] * 1e-3) / 1e12, 3), "pairs_per_s": round(pairs / (s["median"] * 1e-3), 0),
            "workspace_bytes": ops.topk_sets_workspace_bytes(cfg["model"], D, q_head, Q - q_head, G, int(set_row.numel()), K),
            "steps": steps}


def repeated(runs, name):
    a = np.asarray([float(np.median(r[name])) for r in runs])
    mid = float(np.median(a))
    return {"median_ms": round(mid, 4), "spread": round(float((a.max() - a.min()) / mid), 4), "medians_ms": [round(float(x), 4) for x in a]}


def python_route(w, cfg, table, steps, warmup, repeats):
    """ranking.predict_links_in_sets end to end on the workload's sets -- Q / 2 triples, both sides, a FilterIndex over a graph
    of 310 116 edges that holds them -- with the fused branch and with it disabled (the dense route), alternating; host clock
    around a synchronised call.  The two results must be equal first."""
    from blp_amd import models, ranking, utils
    dev = table.device
    N, D, Q, G = cfg["N"], cfg["D"], cfg["Q"], cfg["G"]
    T = Q // 2
    g = torch.Generator(device=dev).manual_seed(1)
    model = models.LinkPrediction(D, "transe", "margin", w["rel_w"].shape[0], 0).to(dev)
    with torch.no_grad():
        model.rel_emb.weight.copy_(w["rel_w"])
    triples = torch.stack((torch.randint(0, N, (T,), generator=g, device=dev), w["fixed"][:T], w["rel_ids"][:T]), dim=1)
    extra = torch.stack((torch.randint(0, N, (310_116 - T,), generator=g, device=dev), torch.randint(0, N, (310_116 - T,), generator=g, device=dev),
                         torch.randint(0, w["rel_w"].shape[0], (310_116 - T,), generator=g, device=dev)), dim=1)
    index = utils.FilterIndex(torch.cat((triples, extra)).cpu())
    ent2idx = torch.arange(N, device=dev)
    sets = ranking.CandidateSets(ptr=w["set_ptr"], rows=w["set_row"]).to(dev)
    set_ids = w["ids"]

    def call():
        out = ranking.predict_links_in_sets(model, table, triples, K, sets, ent2idx, set_ids=set_ids, filter_index=index)
        torch.cuda.synchronize()
        return out

    supported = ranking.ops.topk_sets_wide_supported

    def dense():
        ranking.ops.topk_sets_wide_supported = lambda *a, **k: False
        try:
            return call()
        finally:
            ranking.ops.topk_sets_wide_supported = supported

    a, b = call(), dense()
    nan = torch.isnan(b[1])
    # (the dense route's scores are torch's on the device: rows and NaN slots must agree, the scores to rounding)
    same = bool(torch.equal(a[0], b[0])) and bool(torch.equal(torch.isnan(a[1]), nan))
    close = bool(torch.allclose(a[1][~nan], b[1][~nan], rtol=1e-5, atol=1e-6))
    runs = []
    for _ in range(repeats):
        ms = {"fused": [], "dense": []}
        for i in range(warmup + steps):
            for n, fn in (("fused", call), ("dense", dense)):
                t0 = time.perf_counter()
                fn()
                if i >= warmup:
                    ms[n].append((time.perf_counter() - t0) * 1e3)
        runs.append(ms)
    f, d = repeated(runs, "fused"), repeated(runs, "dense")
    return {"rows_equal": same, "scores_close": close, "fused_ms": f, "dense_ms": d, "dense_over_fused": round(d["median_ms"] / f["median_ms"], 2),
            "steps": steps, "warmup": warmup, "repeats": repeats}


def run_wide(D, steps, warmup, repeats, table16=None, python_steps=3):
    """blp_topk_sets_wide at width D on the fb15k237-transe shape, next to blp_topk_sets (64 / 128 / 256) or to the expanded
    route (any other width: blp_rank_lists' scores + the device-side stable top-k), and -- off 64 / 128 / 256 --
    ranking.predict_links_in_sets with and without the fused branch."""
    cfg = dict(WORKLOADS["fb15k237-transe"], D=int(D))
    w = make_workload(cfg)
    Q, G = cfg["Q"], cfg["G"]
    table, source, fixed = w["table"], w["table"], w["fixed"]
    if table16:  # the 16-bit table as it is; the queries' f32 vectors gathered and widened, as ranking.predict_links_in_sets does
        table = table.to({"f16": torch.float16, "bf16": torch.bfloat16}[table16])
        source = ops.gather_triple_vectors(torch.stack((fixed, fixed, torch.zeros_like(fixed)), dim=1), None, table)[:Q]
        fixed = torch.arange(Q, device=table.device)
        w["table"] = None
    sets_args = (w["set_ptr"], w["set_row"], w["qh"], w["qt"])
    out, other_out = w["out"], (torch.empty_like(w["out"][0]), torch.empty_like(w["out"][1]))

    def wide():
        ops.topk_sets_wide("transe", table, source, fixed, w["rel_w"], w["rel_ids"], w["q_head"], K, *sets_args, filter=w["filt"], out=out)

    if ops.topk_sets_supported("transe", D, K, table.dtype):
        other_name = "topk_sets"

        def other():
            ops.topk_sets("transe", table, source, fixed, w["rel_w"], w["rel_ids"], w["q_head"], K, *sets_args, filter=w["filt"], out=other_out)
    else:
        other_name = "expanded_lists_topk"
        other, _, exp_rows, exp_scores, _ = expanded_route("transe", table, source, fixed, w["rel_w"], w["rel_ids"], w["q_head"], Q,
                                                           w["set_row"], w["n_per"], w["first"], w["seg"])
        other_out = (exp_rows, exp_scores)

    wide()
    other()
    nan = torch.isnan(other_out[1])
    same = bool(torch.equal(out[0], other_out[0])) and bool(torch.equal(torch.isnan(out[1]), nan)) and \
        bool(torch.equal(out[1][~nan].view(torch.int32), other_out[1][~nan].view(torch.int32)))
    head = {"workload": f"fb15k237-transe-wide-{D}", **cfg, "k": K, "table16": table16, "against": other_name, "results_equal": same}
    if not same:
        return head
    runs = [measure({"wide": wide, "other": other}, steps, warmup) for _ in range(repeats)]
    a, b = repeated(runs, "wide"), repeated(runs, "other")
    pairs = int(w["n_per"].sum())
    line = {**head, "set_entries": int(w["set_row"].numel()), "pairs": pairs, "filter_entries_per_query": FILTER_PER_QUERY,
            "topk_sets_wide_ms": a, f"{other_name}_ms": b, f"{other_name}_over_topk_sets_wide": round(b["median_ms"] / a["median_ms"], 3),
            "pairs_per_s": round(pairs / (a["median_ms"] * 1e-3), 0),
            "workspace_bytes": ops.topk_sets_wide_workspace_bytes("transe", D, w["q_head"], Q - w["q_head"], G, int(w["set_row"].numel()), K),
            "steps": steps, "warmup": warmup, "repeats": repeats}
    if other_name != "topk_sets":
        del other, other_out, runs
        torch.cuda.empty_cache()
        line["predict_links_in_sets"] = python_route(w, cfg, table, python_steps, 1, repeats)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--table16", choices=("f16", "bf16"))
    ap.add_argument("--no-expanded", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--once", metavar="NAME")
    ap.add_argument("--width", type=int, nargs="+", help="blp_topk_sets_wide at these widths on the fb15k237-transe shape")
    args = ap.parse_args()
    for D in args.width or ():
        line = json.dumps(run_wide(D, args.steps, args.warmup, args.repeats, args.table16))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        ops.release_workspaces()
        torch.cuda.empty_cache()
    if args.width:
        return
    if args.once:
        run(args.once, WORKLOADS[args.once], 0, 0, args.table16, once=True)
        return
    for name, cfg in WORKLOADS.items():
        if args.only and name not in args.only:
            continue
        line = json.dumps(run(name, cfg, args.steps, args.warmup, args.table16, not args.no_expanded, args.repeats))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        ops.release_workspaces()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
