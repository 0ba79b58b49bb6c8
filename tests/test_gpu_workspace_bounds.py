"""Workspace and output bounds of every workspace-taking entry point on the MI355X (through blp_amd.ops).

The contract (include/blp_hip.h): a call is given `workspace_bytes` bytes of scratch, the number its `*_workspace_bytes`
function returned, and may write those bytes and its outputs -- nothing before, nothing behind -- and what it returns may not
depend on what the scratch held when the call began.  Everywhere else in the suite ops._workspace hands every call the
largest buffer a stream has ever asked for, with the last call's contents in it: an overrun lands in slack and a region a
launch path forgot to clear usually holds the same entry point's own zeros.  Here ops._workspace is replaced for the duration
of a test by an allocator that returns a 256-byte aligned slice of EXACTLY the bytes asked for, between two 64 KiB guards,
everything filled with one byte; the outputs a wrapper takes through ``out=`` are views between guards of their own.  After
the call both guards of every buffer must still hold the fill byte.  Each case runs with the fills 0x00, 0xFF (every stale
u64 key the largest there is, every stale float a NaN) and 0xA5 (a negative float, a plausible row id): the three results are
bit-identical (scores as int32 patterns), and the 0x00 run equals the reference its entry point's own module uses -- the C
oracle's counts, the numpy stable orders of the top-k / sets / lists modules, want_counts / want_topk of
test_rank_relations_host.py -- never another GPU route.

Layout facts the cases aim at (topk.hip: carve_topk; topk_sets.hip: carve_topk_sets; lists_topk.hip; rank_sets.hip:
carve_sets; rank_lists.hip; rank_rels.hip; rank_all.hip / queries.hip):
  topk            [coef_head | coef_tail | (Q, S, k) keys], each rounded to 256.  N = 700 -> S = 3, N = 5 000 -> S = 20, N = 1
                  -> S = 1; a side without queries is an EMPTY coefficient region (the next one starts at the same address);
                  k = 256: chunks of 3 queries, key lists of 2 048 bytes (no slack behind the last); k = 10, Q = 3: 240 S bytes
                  (ragged); Q = 32 at k = 10 fills one chunk of 32 queries exactly.
  topk_sets       [coef_head | coef_tail | (G + 1) prefix | reserved keys]: (G + 1) x 8 = 256 at G = 31 (the keys follow the
                  prefix directly), 16 at G = 1, 264 at G = 32; only partial_bytes of the reserved keys are cleared; a call whose
                  sets are all empty clears nothing and merges zero keys: every slot -1 / the quiet NaN whatever the fill.
  topk_lists      (Q, S, k) keys and nothing else: Q = 3, nnz = 5 070, k = 10 -> S = 7, 1 680 bytes rounded to 1 792; 2 048
                  queries or more: no workspace at all (ops passes NULL).
  rank_lists,     the Q true scores, 4 Q bytes rounded to 256: Q = 64 leaves no slack, 65 starts a second line; the
  rank_relations  scores-only form takes no workspace.  topk_relations: 0 bytes for every Q, R, k.
  rank_sets       [Q true keys | Q accumulators | coef_head | coef_tail | (G + 1) prefix]: groups of 1, 128 and 129 queries (the
                  128-query reuse unit), G + 1 = 32 exact, 2, 33 and 34 ragged; the accumulators are added to, not stored.
  rank_all(_shard) the route's own carve (exact tiles, small slots, the SAD / MFMA pre-pass with their pair lists): block
                  shapes whose tile and chunk counts do not divide evenly, at the shipped dispatch and with the knobs that keep
                  the pre-pass kernels in play on small tables.
  rank_all_batches [the passes' workspace | permuted queries and counts | a widened f32 copy of a 16-bit table the ring
                  kernels do not read directly]; the native 16-bit form carves the static passes only.
"""
import numpy as np
import pytest
import torch

import test_gpu_rank_lists as lists_base
import test_gpu_rank_sets as sets_base
import test_gpu_rank_sets16 as sets16_base
import test_gpu_topk as topk_base
import test_gpu_topk_lists as topk_lists_base
import test_gpu_topk_sets as topk_sets_base
import test_gpu_topk_sets16 as topk_sets16_base
from conftest import golden
from test_gpu_parity import oracle_counts, random_csr
from test_gpu_rank_relations import matrix as relation_matrix_of, problem as relation_problem, segment_filter as relation_filter
from test_gpu_shard import _oracle_counts as triples_oracle_counts, _problem as triples_problem
from test_gpu_table16 import _loop_positions
from test_rank_relations_host import removed_mask as relation_removed_mask, same_scores, same_topk, want_counts, want_topk

pytestmark = pytest.mark.gpu

GUARD = 1 << 16  # the canary test_gpu_parity.py::test_workspace_is_never_overrun puts behind its workspace
FILLS = (0x00, 0xFF, 0xA5)
NAN_BITS = 0x7fc00000
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from blp_amd import ops as _ops
    return _ops


class Guarded:
    """The stand-in for ops._workspace and the maker of guarded outputs of one run: every buffer is guard + bytes + guard,
    filled with ``fill``, and recorded as (buffer, offset, nbytes, fill)."""

    def __init__(self, fill):
        self.fill = fill
        self.records = []
        self.requests = []  # the byte counts ops._workspace was asked for, in order

    def _carve(self, nbytes, align, device):
        buf = torch.full((GUARD + nbytes + GUARD + align,), self.fill, dtype=torch.uint8, device=device)
        off = GUARD + (-(buf.data_ptr() + GUARD)) % align
        self.records.append((buf, off, nbytes, self.fill))
        return buf, off

    def __call__(self, dev, stream, nbytes):
        nbytes = int(nbytes)
        self.requests.append(nbytes)
        buf, off = self._carve(nbytes, 256, dev)
        # (a zero-byte request still gets an address, as the cached buffer has one; the byte it names belongs to the guard)
        ws = buf[off:off + max(nbytes, 1)]
        assert ws.data_ptr() % 256 == 0
        return ws

    def out(self, shape, dtype):
        """A contiguous ``shape`` tensor of ``dtype`` between two guards, pre-filled like them."""
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf, off = self._carve(nbytes, 256, "cuda")
        return buf[off:off + nbytes].view(dtype).view(shape)

    def check(self, what=""):
        torch.cuda.synchronize()
        for i, (buf, off, nbytes, fill) in enumerate(self.records):
            assert bool((buf[:off] == fill).all()), ("a write BEFORE buffer", i, nbytes, hex(fill), what)
            assert bool((buf[off + nbytes:] == fill).all()), ("a write BEHIND buffer", i, nbytes, hex(fill), what)


@pytest.fixture
def guard(ops, monkeypatch):
    """guard(fill) -> a fresh Guarded serving as ops._workspace until the next guard(...) or the end of the test."""
    def make(fill):
        g = Guarded(fill)
        monkeypatch.setattr(ops, "_workspace", g)
        return g
    return make


def bits(t):
    if t is None:
        return None
    a = t.detach().cpu().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


def three_fills(guard, call, what=""):
    """call(g) under each fill: the guards hold, the three results are bit-identical.  Returns (the 0x00 run's result as CPU
    tensors, the workspace requests of that run)."""
    first = requests = None
    for fill in FILLS:
        g = guard(fill)
        got = call(g)
        g.check((what, hex(fill)))
        got = tuple(got) if isinstance(got, (tuple, list)) else (got,)
        got = tuple(None if x is None else x.cpu() for x in got)
        if first is None:
            first, requests = got, list(g.requests)
            continue
        assert g.requests == requests, (what, hex(fill))
        for a, b in zip(first, got):
            assert (a is None) == (b is None), (what, hex(fill))
            assert a is None or np.array_equal(bits(a), bits(b)), ("the result depends on the workspace's contents", what, hex(fill))
    return first, requests


def dev(a):
    return None if a is None else torch.as_tensor(a).cuda()


def table_pair(table, dtype):
    """(the table on the device in ``dtype``, the float32 source of the queries' vectors on the device, the same values on the
    host in float32): one tensor serves as both for float32, a 16-bit table goes with its exactly widened copy."""
    if dtype is torch.float32:
        t = table.cuda()
        return t, t, table
    t16 = table.to(dtype)
    wide = t16.float().contiguous()
    return t16.cuda(), wide.cuda(), wide


# ------------------------------------------------------------------------------------------------ topk / topk_typed
TOPK_SHAPES = ((700, 1, 2), (700, 0, 3), (700, 32, 0), (1, 2, 2), (5000, 3, 4))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("model", ["transe", "complex"])
def test_topk(ops, oracle, guard, model, dtype):
    D, dt = 64, DTYPES[dtype]
    for i, (N, qh, qt) in enumerate(TOPK_SHAPES):
        Q = qh + qt
        table, rel, fixed, rel_ids = topk_base.random_problem(model, N, D, Q, seed=40 + i)
        tab, src, host = table_pair(table, dt)
        pred = topk_base.oracle_pred(oracle, model, host.numpy(), host.numpy(), fixed.numpy(), rel.numpy(), rel_ids.numpy(), qh)
        args = (model, tab, src, fixed.cuda(), rel.cuda(), rel_ids.cuda(), qh)
        for k in (1, 10, 256):
            need = ops.topk_workspace_bytes(model, N, D, qh, qt, k, dt)
            assert need > 0 and need % 256 == 0
            got, asked = three_fills(guard, lambda g: ops.topk(*args, k, out=(g.out((Q, k), torch.int64), g.out((Q, k), torch.float32))),
                                     (model, dtype, N, qh, qt, k))
            assert asked == [need]
            topk_base.check(got, topk_base.expected(pred, k), (model, dtype, N, qh, qt, k))
    # the sizes the shapes were chosen for: one more slab is Q x k more keys; k = 256 leaves no slack behind the keys
    one = lambda N, qh, qt, k: ops.topk_workspace_bytes(model, N, D, qh, qt, k, dt)
    assert one(5000, 3, 4, 256) - one(1, 3, 4, 256) == 7 * 19 * 256 * 8 and one(700, 3, 4, 256) - one(1, 3, 4, 256) == 7 * 2 * 256 * 8
    assert one(700, 32, 0, 10) - one(1, 32, 0, 10) == 32 * 2 * 10 * 8  # 30 lines of 256 bytes exactly, 10 for one slab


# ------------------------------------------------------------------------------------------------ topk_sets / topk_sets_typed
SIZE_CYCLE = (0, 1, 63, 64, 65, 257, 300)
TOPK_HEAD_CYCLE = (1, 0, 3, 32, 0, 33, 2)  # runs around the chunk of 32 (k = 10) / 3 (k = 256) queries; set 0 is empty and has a query
TOPK_TAIL_CYCLE = (0, 2, 1, 0, 4, 0, 3)


def cycled(cycle, G):
    return tuple(cycle[i % len(cycle)] for i in range(G))


def topk_sets_cases(G):
    """(name, N, sizes, head_runs, tail_runs)"""
    if G == 1:  # one long set shared by 3 + 1 queries: many slabs per query
        return [("long", 6007, (5000,), (3,), (1,))]
    sizes, hr, tr, none = cycled(SIZE_CYCLE, G), cycled(TOPK_HEAD_CYCLE, G), cycled(TOPK_TAIL_CYCLE, G), (0,) * G
    return [("both", 1031, sizes, hr, tr), ("heads only", 1031, sizes, hr, none), ("tails only", 1031, sizes, none, tr),
            ("every set empty", 1031, none, hr, tr)]


@pytest.mark.parametrize("G", [1, 31, 32])
@pytest.mark.parametrize("model,D,dtype", [("transe", 64, "f32"), ("distmult", 128, "f32"), ("transe", 64, "f16"), ("complex", 64, "bf16")])
def test_topk_sets(ops, oracle, guard, model, D, dtype, G):
    dt = DTYPES[dtype]
    for name, N, sizes, hr, tr in topk_sets_cases(G):
        if dt is torch.float32:
            sets, ptr, rows = topk_sets_base.make_sets(N, sizes, seed=G)
            p = topk_sets_base.make_problem(model, N, D, hr, tr, seed=G + 1)
            tab = src = p["table"].cuda()
        else:
            p, sets, ptr, rows = topk_sets16_base.make(model, D, dt, G, N=N, sizes=sizes, head_runs=hr, tail_runs=tr)
            tab, src = topk_sets16_base.dev16(p, dt), p["table"].cuda()
        Q, qh = p["Q"], p["q_head"]
        pred = topk_sets_base.oracle_pred(oracle, p)
        args = (model, tab, src, dev(p["fixed"]), p["rel"].cuda(), dev(p["rel_ids"]), qh)
        sets_args = (dev(ptr), dev(rows), dev(p["qh"]), dev(p["qt"]))
        for k in (10, 256):
            what = (model, D, dtype, G, name, k)
            need = ops.topk_sets_workspace_bytes(model, D, qh, Q - qh, G, len(rows), k)
            got, asked = three_fills(guard, lambda g: ops.topk_sets(*args, k, *sets_args, out=(g.out((Q, k), torch.int64), g.out((Q, k), torch.float32))),
                                     what)
            assert asked == [need]
            want = topk_sets_base.expected(pred, k, sets, p["set_of"])
            topk_sets_base.check(got, want, what)
            empty = got[0].numpy() < 0
            assert (got[1].numpy().view(np.int32)[empty] == NAN_BITS).all(), what  # an empty slot: -1 and the quiet NaN
            if name == "every set empty":
                assert len(rows) == 0 and empty.all()
            if name == "long":
                assert (want[0] >= 0).all() and need > 4 * k * 8 * 8  # several key lists per query


# ------------------------------------------------------------------------------------------------ topk_lists
@pytest.mark.parametrize("model,D,dtype", [("transe", 300, "f32"), ("complex", 128, "f32"), ("transe", 300, "f16"), ("complex", 128, "bf16")])
def test_topk_lists(ops, oracle, guard, model, D, dtype):
    dt, N, k = DTYPES[dtype], 1000, 10
    # (a) Q = 3 with lists of 5 000, 0 and 70 entries: S = 7, (3, 7, 10) keys = 1 680 bytes in a workspace of 1 792
    table, rel, fixed, rel_ids, _ = lists_base.random_problem(model, N, D, 3, seed=60)
    tab, src, host = table_pair(table, dt)
    ptr, rows = lists_base.random_lists(3, N, lengths=(5000, 0, 70), seed=61)
    f, r = host[fixed].numpy(), rel[rel_ids].numpy()
    segs = [rows[ptr[q]:ptr[q + 1]][:40] for q in range(3)]
    removed = lists_base.removed_mask(segs, None, None, N)
    for q_head in (0, 1, 3):
        pred = lists_base.oracle_pred(oracle, model, host.numpy(), f, r, q_head)
        need = ops.topk_lists_workspace_bytes(model, D, q_head, 3 - q_head, len(rows), k, dt)
        assert need == (3 * 7 * k * 8 + 255) // 256 * 256 == 1792
        for filt, rm in ((None, None), (lists_base.segment_filter(ops, segs, None, None, 0), removed)):
            what = (model, D, dtype, q_head, filt is not None)
            got, asked = three_fills(guard, lambda g: ops.topk_lists(model, tab, src, fixed.cuda(), rel.cuda(), rel_ids.cuda(), q_head, dev(ptr),
                                                                     dev(rows), k, filter=filt,
                                                                     out=(g.out((3, k), torch.int64), g.out((3, k), torch.float32))), what)
            assert asked == [need]
            topk_lists_base.check(got, topk_lists_base.expected(pred, ptr, rows, k, removed=rm), what)
    # (b) 4 096 queries with short lists: one slab each, no workspace -- ops asks for none and passes NULL
    Q = 4096
    table, rel, fixed, rel_ids, _ = lists_base.random_problem(model, N, D, Q, seed=62)
    tab, src, host = table_pair(table, dt)
    ptr, rows = lists_base.random_lists(Q, N, lengths=(0, 1, 5, 64, 65, 9), seed=63, specials=False)
    q_head = 1000
    pred = lists_base.oracle_pred(oracle, model, host.numpy(), host[fixed].numpy(), rel[rel_ids].numpy(), q_head)
    assert ops.topk_lists_workspace_bytes(model, D, q_head, Q - q_head, len(rows), k, dt) == 0
    got, asked = three_fills(guard, lambda g: ops.topk_lists(model, tab, src, fixed.cuda(), rel.cuda(), rel_ids.cuda(), q_head, dev(ptr), dev(rows),
                                                             k, out=(g.out((Q, k), torch.int64), g.out((Q, k), torch.float32))), (model, D, dtype, Q))
    assert asked == []
    topk_lists_base.check(got, topk_lists_base.expected(pred, ptr, rows, k), (model, D, dtype, Q))


# ------------------------------------------------------------------------------------------------ rank_lists
@pytest.mark.parametrize("Q", [1, 64, 65])
@pytest.mark.parametrize("model,D,dtype", [("transe", 64, "f32"), ("complex", 128, "f32"), ("transe", 300, "f16")])
def test_rank_lists(ops, oracle, guard, model, D, dtype, Q):
    dt, N = DTYPES[dtype], 1000
    table, rel, fixed, rel_ids, true_row = lists_base.random_problem(model, N, D, Q, seed=Q + D)
    tab, src, host = table_pair(table, dt)
    ptr, rows = lists_base.random_lists(Q, N, lengths=lists_base.LENGTHS[2:] + lists_base.LENGTHS[:2], seed=Q + D + 1)  # Q = 1: 63 entries
    nnz = len(rows)
    f, r = host[fixed].numpy(), rel[rel_ids].numpy()
    segs = [np.unique(rows[ptr[q]:ptr[q + 1]][:9]) for q in range(Q)]  # (a value occurs once per segment: blp_filter's contract)
    removed = lists_base.removed_mask(segs, None, None, N)
    args = (model, tab, src, fixed.cuda(), rel.cuda(), rel_ids.cuda())
    for q_head in sorted({0, Q // 2, Q}):
        need = (4 * Q + 255) // 256 * 256
        assert need == 256 * (1 + (Q > 64))
        pred = lists_base.oracle_pred(oracle, model, host.numpy(), f, r, q_head)
        true = pred[np.arange(Q), true_row.numpy()]
        for filt, rm in ((None, None), (lists_base.segment_filter(ops, segs, None, None, 0), removed)):
            what = (model, D, dtype, Q, q_head, filt is not None)
            want = lists_base.expected(pred, true, ptr, rows, removed=rm)
            lists = (q_head, dev(ptr), dev(rows))
            both, asked = three_fills(guard, lambda g: ops.rank_lists(*args, *lists, true_row=true_row.cuda(), filter=filt, want_scores=True,
                                                                      out=(g.out((Q, 4), torch.int32), g.out((nnz,), torch.float32))), what)
            assert asked == [need]
            lists_base.check(both, want, what)
            counts, asked = three_fills(guard, lambda g: ops.rank_lists(*args, *lists, true_row=true_row.cuda(), filter=filt,
                                                                        out=(g.out((Q, 4), torch.int32), None)), what)
            assert asked == [need] and counts[1] is None
            lists_base.check(counts, want, what)
        scores, asked = three_fills(guard, lambda g: ops.rank_lists(*args, q_head, dev(ptr), dev(rows), out=(None, g.out((nnz,), torch.float32))),
                                    (model, D, dtype, Q, q_head, "scores only"))
        assert asked == [] and scores[0] is None  # the scores-only form touches no workspace: none is asked for, NULL is passed
        lists_base.check(scores, lists_base.expected(pred, true, ptr, rows), (model, D, dtype, Q, q_head, "scores only"))


# ------------------------------------------------------------------------------------------------ rank_relations / topk_relations
@pytest.mark.parametrize("Q", [1, 64, 65])
@pytest.mark.parametrize("model,D", [("transe", 64), ("complex", 128)])
def test_rank_relations(ops, oracle, guard, model, D, Q):
    R = 70
    source, rel_w, hr, tr, true_rel = relation_problem(300, D, R, Q, seed=Q + D)
    S = relation_matrix_of(oracle, model, source, rel_w, hr, tr)
    rng = np.random.default_rng(Q)
    segs = [rng.choice(R, size=4, replace=False) for _ in range(Q)]
    args = (model, source.cuda(), hr.cuda(), tr.cuda(), rel_w.cuda())
    need = ops.rank_relations_workspace_bytes(model, D, Q, R)
    assert need == (4 * Q + 255) // 256 * 256 == 256 * (1 + (Q > 64))
    for filt, removed in ((None, np.zeros((Q, R), bool)),
                          (relation_filter(ops, segs, true_rel.numpy()), relation_removed_mask(segs, true_rel.numpy(), Q, R))):
        what = (model, D, Q, filt is not None)
        want = want_counts(S, true_rel.numpy(), removed)
        got, asked = three_fills(guard, lambda g: ops.rank_relations(*args, true_rel.cuda(), filter=filt, return_scores=True,
                                                                     out=g.out((Q, 4), torch.int32)), what)
        assert asked == [need] and np.array_equal(got[0].numpy(), want), what
        same_scores(got[1], S, what)
        got, asked = three_fills(guard, lambda g: ops.rank_relations(*args, true_rel.cuda(), filter=filt, out=g.out((Q, 4), torch.int32)), what)
        assert asked == [need] and np.array_equal(got[0].numpy(), want), what
    got, asked = three_fills(guard, lambda g: ops.rank_relations(*args, return_scores=True), (model, D, Q, "scores only"))
    assert asked == []  # the scores-only form touches no workspace: none is asked for, NULL is passed
    same_scores(got[0], S, (model, D, Q, "scores only"))


@pytest.mark.parametrize("model,D", [("transe", 64), ("distmult", 128)])
def test_topk_relations_takes_no_workspace(ops, oracle, guard, model, D):
    for Q, R in ((1, 11), (65, 70), (7, 300)):
        source, rel_w, hr, tr, true_rel = relation_problem(300, D, R, Q, seed=Q + R)
        S = relation_matrix_of(oracle, model, source, rel_w, hr, tr)
        rng = np.random.default_rng(R)
        segs = [rng.choice(R, size=4, replace=False) for _ in range(Q)]
        args = (model, source.cuda(), hr.cuda(), tr.cuda(), rel_w.cuda())
        for k in (1, 10, 256):
            assert ops.topk_relations_workspace_bytes(model, D, Q, R, k) == 0
            for filt, removed in ((None, np.zeros((Q, R), bool)), (relation_filter(ops, segs, None), relation_removed_mask(segs, np.full(Q, -1), Q, R))):
                what = (model, D, Q, R, k, filt is not None)
                got, asked = three_fills(guard, lambda g: ops.topk_relations(*args, k, filter=filt,
                                                                             out=(g.out((Q, k), torch.int64), g.out((Q, k), torch.float32))), what)
                assert all(n == 0 for n in asked), what  # workspace = NULL reaches the library
                same_topk(got, want_topk(S, removed, k), what)
                assert (got[1].numpy().view(np.int32)[got[0].numpy() < 0] == NAN_BITS).all(), what


# ------------------------------------------------------------------------------------------------ rank_sets / rank_sets_typed
RANK_HEAD_RUNS = (1, 128, 0, 129, 2, 0, 5)  # the 128-query reuse unit, one more, one query; sets with queries of one side only
RANK_TAIL_RUNS = (0, 1, 129, 0, 128, 3, 0)


def rank_sets_cases(G):
    """(name, sizes, head_runs, tail_runs)"""
    if G == 1:
        return [("both", (300,), (129,), (128,)), ("heads only", (300,), (128,), (0,)), ("tails only", (300,), (0,), (1,))]
    pad = lambda runs: tuple(runs[i] if i < len(runs) else int(i % 3 == 0) for i in range(G))
    sizes, hr, tr, none = cycled(SIZE_CYCLE, G), pad(RANK_HEAD_RUNS), pad(RANK_TAIL_RUNS), (0,) * G
    return [("both", sizes, hr, tr), ("heads only", sizes, hr, none), ("tails only", sizes, none, tr), ("every set empty", none, hr, tr)]


@pytest.mark.parametrize("G", [1, 31, 32, 33])
@pytest.mark.parametrize("model,D,dtype", [("transe", 64, "f32"), ("complex", 256, "f32"), ("distmult", 64, "bf16"), ("transe", 256, "f16")])
def test_rank_sets(ops, oracle, guard, model, D, dtype, G):
    """The counts of ops.rank_sets and, on top of them, add_true's host-side + 1 where the true entity is outside the set (two
    thirds of the queries here: plant_true_rows puts every third true row into its set)."""
    dt, N = DTYPES[dtype], 1031
    for name, sizes, hr, tr in rank_sets_cases(G):
        sets, ptr, rows = sets_base.make_sets(N, sizes, seed=G + D)
        p = sets_base.make_problem(model, N, D, hr, tr, seed=G + D + 1)
        sets_base.plant_true_rows(p, sets, seed=G + D + 2)
        if dt is torch.float32:
            tab = src = p["table"].cuda()
        else:
            p["table"] = p["table"].to(dt).float()
            tab, src = sets16_base.dev16(p, dt), p["table"].cuda()
        Q, qh, set_of = p["Q"], p["q_head"], p["set_of"]
        pred, true = sets_base.oracle_pred(oracle, p)
        segs = [sets[g][:4] for g in set_of]
        absent = np.array([p["true_row"][q] not in sets[set_of[q]] for q in range(Q)])
        assert name != "both" or (absent.any() and not absent.all())
        args = (model, tab, src, dev(p["fixed"]), p["rel"].cuda(), dev(p["rel_ids"]), qh, dev(p["true_row"]), dev(ptr), dev(rows), dev(p["qh"]),
                dev(p["qt"]))
        need = ops.rank_sets_workspace_bytes(model, D, qh, Q - qh, G)
        for filt, removed in ((None, None), (sets_base.segment_filter(ops, segs, None, None, 0), sets_base.removed_mask(segs, None, None, N))):
            what = (model, D, dtype, G, name, filt is not None)
            got, asked = three_fills(guard, lambda g: ops.rank_sets(*args, filter=filt, out=g.out((Q, 4), torch.int32)), what)
            assert asked == [need]
            want = sets_base.expected(pred, true, sets, set_of, removed=removed)
            assert np.array_equal(got[0].numpy(), want), what
            with_true = got[0].numpy() + np.array([0, 1, 0, 1], np.int32) * absent[:, None].astype(np.int32)  # ranking.rank_in_sets: add_true
            assert (with_true[:, 1] >= 1).all(), what  # the true entity always competes
    # G + 1 = 32 prefix entries are one 256-byte line exactly: the prefix's last entry is the workspace's last 8 bytes; G = 32
    # starts a second line with that entry alone
    ws = lambda G_: ops.rank_sets_workspace_bytes(model, D, 129, 128, G_)
    assert ws(31) == ws(1) and ws(32) == ws(33) == ws(31) + 256


@pytest.mark.parametrize("rel_model", ["transe", "simple"])
def test_rank_in_sets_with_add_true(guard, rel_model):
    """ranking.rank_in_sets(add_true=True) on a device table (blp_rank_sets under the guards) == its CPU route."""
    from blp_amd import ranking, utils
    g, f = golden(f"eval_toy_{rel_model}"), golden("filters_toy")
    table, triples, ent2idx = torch.from_numpy(g["ent_emb"]), torch.from_numpy(f["triples"]), torch.from_numpy(f["ent2idx"])
    graph = torch.from_numpy(f["graph_edges"])
    index = utils.FilterIndex(graph)
    typed = ranking.relation_candidate_sets(graph, g["rel_w"].shape[0], ent2idx)
    cpu = ranking.rank_in_sets(sets_base._model(rel_model, g["rel_w"]), table, triples, typed, ent2idx, filter_index=index, add_true=True)
    dev_model = sets_base._model(rel_model, g["rel_w"]).cuda()
    got, asked = three_fills(guard, lambda _: ranking.rank_in_sets(dev_model, table.cuda(), triples, typed, ent2idx, filter_index=index, add_true=True),
                             rel_model)
    assert len(asked) == 1 and asked[0] > 0 and torch.equal(got[0], cpu)


# ------------------------------------------------------------------------------------------------ rank_all / rank_all_shard
SHARD_SHAPES = ((1692, 241, 208), (700, 4, 540), (97, 1, 300))  # of test_gpu_parity.py::test_workspace_is_never_overrun
ROUTES = ("shipped", "prepass", "prepass f32 chain")
_shard_problems = {}


def shard_problem(oracle, model, D, N, q_head, q_tail):
    """A block whose queries are made of ``source``, a gathered copy of 300 table rows (source is not table); ties with the true
    entities; a filter; the C oracle's counts.  Built once per shape and shared by the routes."""
    key = (model, D, N, q_head, q_tail)
    if key not in _shard_problems:
        g = torch.Generator().manual_seed(N + D)
        Q = q_head + q_tail
        table = torch.randn(N, D, generator=g)
        table = torch.nn.functional.normalize(table, dim=-1) if model == "transe" else table * 0.1
        dup = table[1::3]
        table[0:3 * dup.shape[0]:3] = dup  # ties: plenty of undecided pairs
        picked = torch.randint(0, N, (300,), generator=g)
        source = table[picked].clone()
        rel_w = (torch.rand(11, D, generator=g) - 0.5) * 0.25
        fixed_row, true_row = torch.randint(0, 300, (Q,), generator=g), torch.randint(0, 300, (Q,), generator=g)
        rel_ids = torch.randint(0, 11, (Q,), generator=g)
        rowptr, col = random_csr(Q, N, picked[true_row].numpy(), seed=N)
        want = oracle_counts(oracle, model, table, source[fixed_row], rel_w[rel_ids], q_head, q_true=source[true_row], csr=(rowptr, col))
        assert (want[:, 1] >= 1).all() and (want[:, 3] < want[:, 1]).any()
        _shard_problems[key] = (table, source, rel_w, fixed_row, true_row, rel_ids, rowptr, col, want)
    return _shard_problems[key]


def set_route(knobs, route):
    if route != "shipped":  # the `routing` fixture of test_gpu_parity.py: the pre-pass kernels from 64 (TransE) / 32 (bilinear) queries on
        knobs("sad_min_queries", 64)
        knobs("small_kernel", 2)
    if route == "prepass f32 chain":  # (a knob of the bilinear pre-pass)
        knobs("gemm_kernel", 1)


@pytest.mark.parametrize("model,D,route", [(m, D, r) for m, D in (("transe", 128), ("transe", 300), ("distmult", 128)) for r in ROUTES
                                           if m != "transe" or r != "prepass f32 chain"])
def test_rank_all_shard(ops, oracle, guard, knobs, model, D, route):
    set_route(knobs, route)
    for N, q_head, q_tail in SHARD_SHAPES:
        Q = q_head + q_tail
        table, source, rel_w, fixed_row, true_row, rel_ids, rowptr, col, want = shard_problem(oracle, model, D, N, q_head, q_tail)
        filt = ops.SegmentFilter(dev(rowptr[:-1].copy()), dev(rowptr[1:].copy()), dev(np.concatenate((col, [0]))), None, None, 0)
        args = (model, table.cuda(), source.cuda(), fixed_row.cuda(), rel_w.cuda(), rel_ids.cuda(), q_head, true_row.cuda())
        what = (model, D, route, N, q_head, q_tail)
        got, asked = three_fills(guard, lambda g: ops.rank_all_shard(*args, filter=filt, out=g.out((Q, 4), torch.int32)), what)
        assert asked == [ops._rank_ws_bytes(ops._lib.lib(), ops._lib.MODEL_IDS[model], N, D, q_head, q_tail)] and asked[0] > 0
        assert np.array_equal(got[0].numpy(), want), what


@pytest.mark.parametrize("route", ROUTES[:2])
@pytest.mark.parametrize("model,D", [("transe", 128), ("complex", 64)])
def test_rank_all_with_its_own_and_with_a_given_workspace(ops, oracle, guard, knobs, model, D, route):
    """ops.rank_all with workspace=None (served by ops._workspace) and with an explicit workspace= of exactly the advertised
    bytes: the same guards, the same three fills."""
    set_route(knobs, route)
    for N, q_head, q_tail in SHARD_SHAPES[:2]:
        Q = q_head + q_tail
        table, source, rel_w, fixed_row, true_row, rel_ids, rowptr, col, want = shard_problem(oracle, model, D, N, q_head, q_tail)
        args = (model, table.cuda(), source[fixed_row].cuda(), rel_w[rel_ids].cuda(), q_head)
        kw = dict(q_true=source[true_row].cuda(), filt_rowptr=dev(rowptr), filt_col=dev(col))
        need = ops._rank_ws_bytes(ops._lib.lib(), ops._lib.MODEL_IDS[model], N, D, q_head, q_tail)
        what = (model, D, route, N, q_head, q_tail)
        got, asked = three_fills(guard, lambda g: ops.rank_all(*args, **kw, out=g.out((Q, 4), torch.int32)), what)
        assert asked == [need] and np.array_equal(got[0].numpy(), want), what
        given, asked = three_fills(guard, lambda g: ops.rank_all(*args, **kw, out=g.out((Q, 4), torch.int32), workspace=g(args[1].device, None, need)),
                                   what)
        assert asked == [need] and np.array_equal(given[0].numpy(), want), what  # (asked by the test itself: ops asked for nothing more)


# ------------------------------------------------------------------------------------------------ rank_all_batches
BATCH_SHAPES = ((2100, 333, 50), (2100, 7, 2), (40000, 7, 2))


@pytest.mark.parametrize("model", ["transe", "distmult"])
@pytest.mark.parametrize("D,dtype,native", [(128, "f32", False), (128, "f16", False), (64, "f16", False), (128, "f16", True), (128, "bf16", True)])
def test_rank_all_batches(ops, oracle, guard, model, D, dtype, native):
    """A float32 table; a 16-bit table widened into the end of the workspace (D = 64 is never read directly; D = 128 with the
    default block is not either); ``native``: a pass per batch (block_triples = batch) over a table long enough for the ring
    kernels to read the 16-bit rows themselves."""
    from blp_amd import utils
    dt, R = DTYPES[dtype], 5
    for N, T, batch in BATCH_SHAPES:
        block = batch if native else 0
        table, rel_w, ent2idx, triples, edges = triples_problem(model, N, D, T, R, seed=T + N % 89)
        tab, _, host = table_pair(table, dt)
        direct = ops.table16_is_read_directly(model, dt, N, D, T, batch, block_triples=block)
        if native and not direct:
            continue  # (2 100 rows: the small-block kernels; 50 triples per batch: not a reference-sized pass)
        assert direct == native
        index = utils.FilterIndex(edges, num_relations=R)
        dev_rel, dev_e2i, dev_triples = rel_w.cuda(), ent2idx.cuda(), triples.cuda()
        source = ops.gather_triple_vectors(dev_triples, dev_e2i, tab)  # float32, widened exactly
        qb = ops.build_queries(dev_triples, dev_e2i, source, dev_rel, batch, index=index, gather=False, by_position=True, num_rows=N)
        torch.cuda.synchronize()
        what = (model, D, dtype, native, N, T, batch)
        got, asked = three_fills(guard, lambda g: ops.rank_all_batches(model, tab, qb.fixed_row, dev_rel, qb.rel_ids, qb.true_row, T, batch,
                                                                       filter=qb.filter, source=source, block_triples=block,
                                                                       out=g.out((2 * T, 4), torch.int32)), what)
        assert len(asked) == 1 and asked[0] > 0
        if dt is not torch.float32 and not native:
            assert asked[0] >= N * D * 4, what  # the widened copy lives in the workspace
        want = triples_oracle_counts(oracle, model, host, rel_w, ent2idx, triples, index)
        head_pos, tail_pos = _loop_positions(T, batch)
        assert np.array_equal(got[0][head_pos].numpy(), want[:T]), what
        assert np.array_equal(got[0][tail_pos].numpy(), want[T:]), what
    if native:
        assert ops.table16_is_read_directly(model, dt, 40000, D, 7, 2, block_triples=2), "no shape took the native 16-bit form"


# ------------------------------------------------------------------------------------------------ the cache's carry-over
def test_stale_contents_of_the_cached_workspace_are_harmless(ops, oracle, monkeypatch):
    """What the cache does in real use, without the patch: topk_sets with a large shape (331 queries, 31 sets), then a small one
    on the same stream (4 queries, one long set: its key lists lie inside the large call's), then a small topk (its coefficient rows and keys lie where the sets calls
    kept coefficients, prefixes and keys).  Each result equals the result of the same call under the guards."""
    model, D, k = "transe", 64, 10
    calls = []
    for N, sizes, hr, tr, seed in ((1031, cycled(SIZE_CYCLE, 31), cycled(TOPK_HEAD_CYCLE, 31), cycled(TOPK_TAIL_CYCLE, 31), 5), (6007, (5000,), (3,), (1,), 3)):
        sets, ptr, rows = topk_sets_base.make_sets(N, sizes, seed=seed)
        p = topk_sets_base.make_problem(model, N, D, hr, tr, seed=seed + 1)
        table = p["table"].cuda()
        args = (model, table, table, dev(p["fixed"]), p["rel"].cuda(), dev(p["rel_ids"]), p["q_head"], k, dev(ptr), dev(rows), dev(p["qh"]), dev(p["qt"]))
        want = topk_sets_base.expected(topk_sets_base.oracle_pred(oracle, p), k, sets, p["set_of"])
        calls.append((ops.topk_sets, args, lambda got, want=want: topk_sets_base.check(got, want)))
    table, rel, fixed, rel_ids = topk_base.random_problem(model, 700, D, 3, seed=7)
    pred = topk_base.oracle_pred(oracle, model, table.numpy(), table.numpy(), fixed.numpy(), rel.numpy(), rel_ids.numpy(), 1)
    t = table.cuda()
    calls.append((ops.topk, (model, t, t, fixed.cuda(), rel.cuda(), rel_ids.cuda(), 1, k), lambda got: topk_base.check(got, topk_base.expected(pred, k))))
    guarded = []
    with monkeypatch.context() as m:
        for fn, args, check in calls:
            g = Guarded(0x00)
            m.setattr(ops, "_workspace", g)
            got = fn(*args)
            g.check()
            check(got)
            guarded.append(got)
    assert not isinstance(ops._workspace, Guarded)
    ops.release_workspaces()
    sizes_seen = []
    for (fn, args, check), want in zip(calls, guarded):
        got = fn(*args)
        torch.cuda.synchronize()
        sizes_seen.append(max(b.numel() for b in ops._workspaces.values()))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert sizes_seen[0] == sizes_seen[1] == sizes_seen[2], "the later calls must have reused the first call's buffer"
