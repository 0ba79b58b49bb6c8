"""The filter step of every ranking route at its edges, on the device: filter_finalize_kernel (filter_finalize.h),
wide_filter_finalize_kernel (rank_sad_wide.hip) and rank_from_scores_kernel (rank_dense.hip), each given the filters of
tests/test_filter_edges_host.py -- which builds them, asserts that each reaches its edge, and derives the expected counts from
a restatement of the blp_filter contract and float64 scores (grid problems) or the C oracle (real-valued / non-finite ones).
Every test requires torch.equal on all four count columns of every query.

Routes (forced with the README's knobs; asserted where the library can tell: ops.prepass_stats,
blp_rank_all_batches_passes_per_launch, ops.table16_is_read_directly):
a. the shipped dispatch on a small block (rank_small.hip), four models, D = 64 / 128; at D = 64 also a 2 050-row table
   (33 tiles = 33 partial slots: sum_partials' eight-load trip, which starts at 29) and one of 16 449 rows (more tiles than
   the 256 slots: n_partials at its largest).  The shipped dispatch takes 191 TransE queries there (rank_small_sgpr_kernel,
   tiles sharing slots) but a bilinear block only below 400 000 pairs: 24 queries, on which `idmap`, `exclude` and `empty`
   run (the other cases need queries 127 and 130 or 128 tie rows); small_kernel = 1 ("the small-block kernels wherever they
   can run") then puts 191 queries of every model, full workgroups, through every case on rank_small_kernel<.., MULTI>;
b. exact tiles (rank_kernel = 1, small_kernel = 2), four models, D = 64 / 128 / 256;
c. the pre-pass (sad_min_queries = 64, small_kernel = 2): rank_sad.hip for TransE at 64 / 128 / 256, rank_gemm.hip for the
   bilinear models at 64 / 128;
d. TransE at D = 300, 100 and 4: wide_filter_finalize_kernel;
e. ops.rank_all_batches with block_triples = batch in {2, 3}, n % batch != 0, small_kernel = 2 and stream_kernel = 3 and 4:
   the static passes, whose finalisation runs replaces_head(batch > 0); f32 tables at 64 / 128 / 256 and f16 / bf16 tables at
   D = 128 / 256, read as they are (the _Float16 / __bf16 instantiations).  The 16-bit tables run with stream_kernel = 4
   only: rank_stream16.hip has ring kernels alone and blp_rank_all_batches_native16 asks no more than stream_kernel != 2,
   so 3 would run the same code again;
f. ops.rank_all_batches with block_triples = 96 > batch = 3 and n = 191 (two super-blocks, the second short): the filter
   arrays go through permute_batches_kernel, the counts back through unpermute_counts_kernel;
g. ops.rank_from_scores on the grid problem's float32 score matrix: true_idx and true_score, a row-strided view, the case's
   CSR with columns outside [0, N) added to every list;
h. the `shards` case on b, c and d at every width of those routes: every shard against its own expectation, and the shards'
   sum against the unsharded counts.

Not covered: 16-bit tables at D = 64 as such -- rank_stream16_applicable takes D = 128 and 256 only (rank_stream16.hip), so
the call widens the table to f32 and finalises with route e's f32 instantiation: there is no 16-bit instantiation at 64
to reach.  The `last_slot` case in the loop's layout has Q % 64 in {2, 62}, since 2 n is even.

What a subtly wrong kernel would trip, argued from the code (nothing here breaks a kernel on purpose):
1. `locate`'s six-step search must return the LARGEST slot with prefix[slot] <= x.  In `long` 63 of 64 queries are empty, so
   prefix is constant on both sides of query 7; a search that stops at the first such slot, or one step short, lands on an
   empty neighbour and reads filter.lo of the wrong query: the assembled `values` hold live rows between the segments, so
   the filtered columns of queries 0 .. 63 move.  `last_slot` does the same at slot 63 and in the ragged workgroup.
2. The TransE loop's stride of 4 x 64 entries (bilinear: 4 x 2).  With a stride of 64 wave w starts at entry 64 w and then
   walks every later block of 64, so the entries of the 776-entry and 320-entry workgroups are scored up to four times
   (block j by min(j, 3) + 1 waves) and removed[] comes out too large ([*-long]).  The all-rows query checks the other end:
   its filtered counts must come out as 0 / 1 exactly.
3. `exclude` is an id, compared before ent2idx.  Compared after the map, the triple's own id in `idmap-ent2idx` is no
   longer recognised (its row differs from its id under the shuffled map) and ge_filt drops by one on every fourth query.
4. ent2idx holes, ids beyond the map, negative ids and rows outside [0, N) compare as unsigned 64-bit values.  A signed test,
   a 32-bit cast (2^33 + a live row) or a missing length test removes a live row or reads past the map: [*-idmap].
5. row_base is subtracted.  Added instead, shard (100, 101) finds no entry and shard (101, N) the wrong ones: [*-shards],
   which also holds a one-row table and q_true vectors.
6. `>=` for `>` (or the reverse) in either accumulator: `ties` lists bit-identical copies of the true row, so fge counts them
   and fgt must not; ge - ge_filt != gt - gt_filt for at least a quarter of the queries (asserted by the builder).
7. replaces_head in the short last batch: with n % batch != 0 the last batch holds nb < batch triples and its tail
   queries start at 2 first + nb.  Using `batch` there scores the last batch's tail queries as head queries; `last_slot`,
   `idmap`, `exclude`, `empty-hi_lt_lo` and `nonfinite` give those queries entries at or above the true score, so their
   filtered counts move (route e; `long` and `ties` leave the last batch without entries).
8. hi < lo must be an empty segment (`n > 0 ? n : 0`; `k < hi`): a length taken as unsigned, or an absolute value, walks live
   values ([*-empty]); a zero-length `values` must not be dereferenced.
9. NaN: every comparison is false, so a NaN row is never subtracted and a NaN true key gives four zeros ([*-nonfinite]).
10. rank_from_scores must skip columns outside [0, N) and read true_idx through the row stride (route g).
"""
import numpy as np
import pytest
import torch

import test_filter_edges_host as host
from conftest import REL_MODELS
from test_filter_edges_host import CASES, HALF, N_ROWS, N_SLOTS, N_TILES, PLAIN, TINY, loop_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"
BILINEAR = REL_MODELS[1:]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _no_knob_left():
    from blp_amd import _lib
    _lib.reset_knobs()
    yield
    _lib.reset_knobs()


def to_dev(f):
    return f._replace(**{k: getattr(f, k).to(DEV) for k in ("seg_lo", "seg_hi", "values", "exclude", "ent2idx")
                         if getattr(f, k) is not None})


def check(got, want, what):
    got = got.cpu()
    assert got.dtype == torch.int32 and got.shape == want.shape
    assert torch.equal(got, want), (what, torch.nonzero((got != want).any(1)).flatten()[:8].tolist())


def rank_plain(ops, p, v, path, rows=None):
    """ops.rank_all on the variant's queries (vectors, plain layout), the whole table or the candidate shard ``rows``."""
    lo, hi = rows or (0, p.N)
    table = p.table[lo:hi].to(DEV)
    q_head = int(v.head.sum())
    assert v.head[:q_head].all()
    args = (p.model, table, p.q_fixed[:v.Q].to(DEV), p.q_rel[:v.Q].to(DEV), q_head)
    ws = torch.empty(max(ops.rank_all_workspace_bytes(p.model, hi - lo, p.D, q_head, v.Q - q_head), 256), dtype=torch.uint8, device=DEV)
    if rows is None:
        got = ops.rank_all(*args, true_row=p.true_row[:v.Q].to(DEV), filter=to_dev(v.filter), workspace=ws)
    else:
        got = ops.rank_all(*args, q_true=p.table[p.true_row[:v.Q]].to(DEV), filter=to_dev(v.filter), workspace=ws)
    stats = ops.prepass_stats(p.model, hi - lo, p.D, q_head, v.Q - q_head, ws)
    assert stats["path"] in path, (stats, path)
    return got


def paths(ops, *ids):
    return [ops.PREPASS_PATHS[i] for i in ids]


def set_route(route):
    from blp_amd import _lib
    if route == "tiles":
        _lib.set_knob("rank_kernel", 1)
        _lib.set_knob("small_kernel", 2)
    elif route == "prepass":
        _lib.set_knob("sad_min_queries", 64)
        _lib.set_knob("small_kernel", 2)


def route_path(ops, route, model):
    if route in ("shipped", "tiles"):
        return paths(ops, 0)
    if route == "wide":
        return paths(ops, 4)
    return paths(ops, 1) if model == "transe" else paths(ops, 2, 3)


def run_cases(ops, route, model, D, N, case, layout=PLAIN, qmax=host.QMAX):
    for family in host.families(case):
        p = host.problem(model, D, N, family, qmax)
        for v, want in host.build(case, model, D, N, family, layout, qmax):
            check(rank_plain(ops, p, v, route_path(ops, route, model)), want, (family, v.name))


# ------------------------------------------------------------------------------------------------ a: the shipped dispatch
@pytest.mark.parametrize("case", CASES + ("nonfinite",))
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("model", REL_MODELS)
def test_small_block_route(ops, model, D, case):
    # what makes the shipped dispatch choose rank_small.hip here and not the pre-passes (rank_common.h: kSmallMaxPairsBilinear,
    # kSmallMaxPairsTransESgpr, kSmallMaxQueries); the path assertion alone cannot tell it from the exact tiles
    assert PLAIN.Qs[0] * N_ROWS < (6000000 if model == "transe" else 400000) and PLAIN.Qs[0] <= 4096
    run_cases(ops, "shipped", model, D, N_ROWS, case)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("model", REL_MODELS)
def test_small_block_route_33_partial_slots(ops, model, case):
    assert (N_SLOTS + 63) // 64 == 33 > 28 and HALF.Qs[0] * N_SLOTS < 400000   # kSmallMaxPairsBilinear (rank_common.h)
    run_cases(ops, "shipped", model, 64, N_SLOTS, case, HALF, HALF.Qs[0])


@pytest.mark.parametrize("case", CASES + ("nonfinite",))
@pytest.mark.parametrize("model", REL_MODELS)
def test_small_block_route_more_tiles_than_slots(ops, knobs, model, case):
    """256 partial slots.  TransE: the shipped dispatch.  The bilinear models: small_kernel = 1, the README's knob for "the
    small-block kernels wherever they can run" (the shipped dispatch: the test below)."""
    assert (N_TILES + 63) // 64 > 256                                          # kSmallMaxSlots
    if model == "transe":
        assert HALF.Qs[0] * N_TILES < 6000000 and (N_TILES + 63) // 64 <= 1024  # kSmallMaxPairsTransESgpr, kSmallSgprMaxTiles
    else:
        knobs("small_kernel", 1)
    run_cases(ops, "shipped", model, 64, N_TILES, case, HALF, HALF.Qs[0])


@pytest.mark.parametrize("case", ["idmap", "exclude", "empty"])
@pytest.mark.parametrize("model", BILINEAR)
def test_small_block_route_more_tiles_than_slots_bilinear_shipped(ops, model, case):
    assert (N_TILES + 63) // 64 > 256 and TINY.Qs[0] * N_TILES < 400000 <= (TINY.Qs[0] + 1) * N_TILES  # kSmallMaxPairsBilinear
    run_cases(ops, "shipped", model, 64, N_TILES, case, TINY, TINY.Qs[0])


# ------------------------------------------------------------------------------------------------ b, c, d
@pytest.mark.parametrize("case", CASES + ("nonfinite",))
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("model", REL_MODELS)
def test_exact_tiles_route(ops, model, D, case):
    set_route("tiles")
    run_cases(ops, "tiles", model, D, N_ROWS, case)


PREPASS_SHAPES = [("transe", 64), ("transe", 128), ("transe", 256)] + [(m, D) for m in BILINEAR for D in (64, 128)]


@pytest.mark.parametrize("case", CASES + ("nonfinite",))
@pytest.mark.parametrize("model,D", PREPASS_SHAPES)
def test_prepass_route(ops, model, D, case):
    set_route("prepass")
    run_cases(ops, "prepass", model, D, N_ROWS, case)


@pytest.mark.parametrize("case", CASES + ("nonfinite",))
@pytest.mark.parametrize("D", [300, 100, 4])
def test_wide_route(ops, D, case):
    run_cases(ops, "wide", "transe", D, N_ROWS, case)


# ------------------------------------------------------------------------------------------------ h: candidate shards
SHARD_ROUTES = [("tiles", m, D) for m in REL_MODELS for D in (64, 128, 256)] + [("prepass", m, D) for m, D in PREPASS_SHAPES] + \
               [("wide", "transe", D) for D in (300, 100, 4)]


@pytest.mark.parametrize("route,model,D", SHARD_ROUTES)
def test_shards_add_up_and_match_their_own_expectation(ops, route, model, D):
    set_route(route)
    for family in ("grid", "real"):
        p = host.problem(model, D, N_ROWS, family)
        parts = host.build("shards", model, D, N_ROWS, family)
        rows = [None] + host.shard_rows(p)
        got = []
        for (v, want), r in zip(parts, rows):
            # (a shard of 100 rows or of one row is ranked by whatever the forced route leaves it: only the whole table's path is pinned)
            path = route_path(ops, route, model) if r is None or route != "prepass" or model == "transe" else paths(ops, 0, 2, 3)
            got.append(rank_plain(ops, p, v, path, r))
            check(got[-1], want, (family, v.name))
        assert torch.equal(got[0], sum(got[1:]))


# ------------------------------------------------------------------------------------------------ e, f: the loop's layout
def rank_batches(ops, p, v, batch, block_triples, table):
    n = v.Q // 2
    return ops.rank_all_batches(p.model, table, p.fixed_row[:v.Q].to(DEV), p.rel.to(DEV), p.rel_id[:v.Q].to(DEV),
                                p.true_row[:v.Q].to(DEV), n, batch, filter=to_dev(v.filter), source=p.table.to(DEV),
                                block_triples=block_triples)


BATCH_SHAPES = [(m, D, torch.float32) for m in REL_MODELS for D in (64, 128, 256)] + \
               [(m, D, dt) for m in REL_MODELS for D in (128, 256) for dt in (torch.float16, torch.bfloat16)]


@pytest.mark.parametrize("case", CASES + ("nonfinite",))
@pytest.mark.parametrize("model,D,dtype", BATCH_SHAPES, ids=lambda x: str(x).replace("torch.", ""))
def test_static_passes_route(ops, knobs, model, D, dtype, case):
    from blp_amd import _lib
    N = N_ROWS
    for batch in (2, 3):
        layout = loop_layout(batch)
        for family in host.families(case):
            p = host.problem(model, D, N, family)
            table = p.table.to(DEV).to(dtype)
            wide = table.float().cpu()                      # the expectation is that of the widened table
            variants = host.build(case, model, D, N, family, layout)
            for stream_kernel in ((3, 4) if dtype == torch.float32 else (4,)):  # (16-bit: ring kernels only, see route e above)
                knobs("small_kernel", 2)
                knobs("stream_kernel", stream_kernel)
                for v, want in variants:
                    n = v.Q // 2
                    assert n % batch != 0
                    if dtype != torch.float32:
                        assert ops.table16_is_read_directly(model, dtype, N, D, n, batch, batch)
                        if family != "grid":
                            want = torch.from_numpy(host.expected(p, v, table=wide))
                        else:
                            assert torch.equal(wide, p.table)   # the grid is exact in 16 bits
                    else:
                        passes = _lib.lib().blp_rank_all_batches_passes_per_launch(_lib.MODEL_IDS[model], 0, N, D, D, n, batch, batch)
                        ring = stream_kernel == 4 or (model == "transe" and D == 256)
                        assert passes == ((n + batch - 1) // batch if ring else 1)
                    check(rank_batches(ops, p, v, batch, batch, table), want, (family, v.name, batch, stream_kernel))


@pytest.mark.parametrize("case", CASES + ("nonfinite",))
@pytest.mark.parametrize("model,D", [("transe", 128), ("distmult", 64), ("complex", 128), ("simple", 256), ("transe", 300)])
def test_permuted_super_blocks_route(ops, model, D, case):
    layout = loop_layout(3)
    for family in host.families(case):
        p = host.problem(model, D, N_ROWS, family)
        for v, want in host.build(case, model, D, N_ROWS, family, layout):
            n = v.Q // 2
            assert 96 < n < 2 * 96 and n % 3 != 0          # two super-blocks of whole batches, the second short, the last batch short
            check(rank_batches(ops, p, v, 3, 96, p.table.to(DEV)), want, (family, v.name))


# ------------------------------------------------------------------------------------------------ g: the dense route
@pytest.mark.parametrize("case", CASES + ("nonfinite",))
@pytest.mark.parametrize("model", ["transe", "complex"])
def test_rank_from_scores_route(ops, model, case):
    D, N = 64, N_ROWS
    for family in host.families(case):
        p = host.problem(model, D, N, family)
        for v, want in host.build(case, model, D, N, family):
            S, s_true = host.scores(p, v)
            S32 = torch.from_numpy(S.astype(np.float32))
            if family == "grid":
                assert np.array_equal(S32.double().numpy(), S)
            rowptr, col = host.mask_csr(host.removed_mask(v.filter, v.Q, N), extra=(N, -1, N + 7, 1 << 40, -(1 << 33)))
            rowptr, col = torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV)
            big = torch.full((v.Q, N + 5), 1e30, device=DEV)
            big[:, :N] = S32.to(DEV)
            view = big[:, :N]
            assert view.stride(0) == N + 5
            true_idx = p.true_row[:v.Q].to(DEV)
            true_score = torch.from_numpy(s_true.astype(np.float32)).to(DEV)
            for scores in (S32.to(DEV), view):
                check(ops.rank_from_scores(scores, true_idx=true_idx, filt_rowptr=rowptr, filt_col=col), want, (family, v.name, "true_idx"))
                check(ops.rank_from_scores(scores, true_score=true_score, filt_rowptr=rowptr, filt_col=col), want, (family, v.name, "true_score"))
