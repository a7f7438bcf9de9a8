"""Non-aggregation queries (SELECT cols WHERE ... LIMIT n) through the C++ driver and the Python mirror of
query/aql_nonaggr_batchexecutor.go, on every backend: dimensions written from row 0, Expand for batches with base counts,
the rows cut to what is still wanted, a D2H flush per batch, and a query that is DONE — and silent — once the limit is met.
Expected rows come from the numpy model of tests/select_model.py, bit for bit; the two hosts must issue the same ABI calls."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import harness as H
import select_model as M
from aresdb_amd import abi
from aresdb_amd.driver import NativeQuery
from aresdb_amd.executor import (BatchContext, BatchExecutor, Binary, Col, Const, DimensionSpec, QueryPlan,
                                 fetch_select_results)

FILTERS = M.MIXED_FILTERS
DIMS = M.MIXED_DIMS  # 16 / 8 / 8 / 4 / 4 / 2 / 2 / 1 byte slots, nulls in every selected column
ALL_ROWS = [("amount", abi.GreaterThan, -2000000)]  # "amount" has no nulls: every row survives


def plan_of(filters, dims, limit, fused=False):
    return QueryPlan(
        filters=[Binary(f, Col(n), Const(c)) for n, f, c in filters],
        dimensions=[DimensionSpec(Col(n) if f is None else Binary(f, Col(n), Const(c)), t) for n, f, c, t in dims],
        measure=Const(1), agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32, use_hash_reduction=True,
        use_fused_extension=fused, is_non_aggregation=True, limit=limit)


class B:
    """one batch: columns, rows, optional base counts (rows + 1 running totals)"""

    def __init__(self, n, seed, base_counts=None, cols=None):
        self.n, self.base_counts = n, base_counts
        self.cols = cols if cols is not None else M.mixed_columns(max(n, 1), seed=seed)


def expected(batches, filters, dims, limit, capacity_of=None):
    """the model: per batch the survivors in order (repeated by run length, cut at the vector's capacity, when the batch has
    base counts), cut at what is still wanted; (rows per dimension, rows contributed per batch)"""
    parts, written, per_batch = [], 0, []
    for i, b in enumerate(batches):
        if limit >= 0 and written >= limit and i > 0:
            per_batch.append(None)  # the query is done: the batch does not run
            continue
        rows, out = M.model_select(b.cols, filters, dims, b.n)
        if b.base_counts is not None and b.n:
            rep = np.diff(b.base_counts.astype(np.int64))[rows]
            out = [(np.repeat(v, rep, axis=0), np.repeat(ok, rep)) for v, ok in out]
            if capacity_of is not None:
                out = [(v[:capacity_of], ok[:capacity_of]) for v, ok in out]
        n = len(out[0][1])
        if limit >= 0:
            n = min(n, max(limit - written, 0))
        parts.append([(v[:n], ok[:n]) for v, ok in out])
        written += n
        per_batch.append(n)
    want = [(np.concatenate([p[d][0] for p in parts]), np.concatenate([p[d][1] for p in parts])) for d in range(len(dims))]
    return want, per_batch


def run(be, plan, batches, native, streams=None, max_batch=None, owned=True):
    """(rows per dimension, ABI calls per batch, done flag after each batch, rows written, fused batches)"""
    names = list(batches[0].cols.keys())
    if native:
        q = NativeQuery(be, plan, names, streams=streams)
        if max_batch:
            q.set_max_batch_size(max_batch)
    else:
        ctx = BatchContext(be, plan, stream=streams[0] if streams else None)
        ctx.max_batch_size = max_batch or 0
        ex = BatchExecutor(ctx)
    calls, done, ran = [], [], 0
    for i, b in enumerate(batches):
        was_done = q.done if native else ctx.done
        dev = {k: c.upload(be) for k, c in b.cols.items()}
        bc = H.Buf(be, b.base_counts) if b.base_counts is not None else None
        before = q.calls if native else ctx.calls
        mine = not owned or was_done  # a done query leaves the batch's columns with the caller
        if native:
            q.run({k: d.vp for k, d in dev.items()}, b.n, base_counts=bc.ptr if bc else None,
                  owned_allocations=[] if mine else [d.buf.ptr for d in dev.values()])
        else:
            if streams and not was_done:  # the Go host swaps its two streams after every batch it runs
                ctx.stream = streams[ran % 2]
            ex.run({k: d.vp for k, d in dev.items()}, b.n, base_counts=bc.ptr if bc else None,
                   owned_columns=[] if mine else [d.free for d in dev.values()])
        calls.append((q.calls if native else ctx.calls) - before)
        ran += 0 if was_done else 1
        done.append(q.done if native else ctx.done)
        if mine:
            for d in dev.values():
                d.free()
        if bc:
            bc.free()
    if native:
        dims, valids, _ = q.fetch()
        written, fused = q.result_size, q.fused_batches
        q.release()
    else:
        dims, valids = fetch_select_results(ctx)
        written, fused = ctx.rows_written, 0
        ctx.release()
    widths = [abi.DATA_TYPE_BYTES[d.data_type] for d in plan.dimensions]
    got = [(v.reshape(written, w), ok) for v, ok, w in zip(dims, valids, widths)]
    return got, calls, done, written, fused


def both_hosts(be, batches, filters, dims, limit, **kw):
    plan = plan_of(filters, dims, limit)
    want, per_batch = expected(batches, filters, dims, limit, kw.pop("capacity_of", None))
    py = run(be, plan, batches, native=False, **kw)
    cpp = run(be, plan, batches, native=True, **kw)
    for got, calls, done, written, _ in (py, cpp):
        assert written == sum(n or 0 for n in per_batch)
        M.assert_rows_equal(got, want)
        for i, n in enumerate(per_batch):
            if n is None:
                assert calls[i] == 0, "a batch run on a done query issued ABI calls"
        wanted_done = [limit >= 0 and sum(x or 0 for x in per_batch[:i + 1]) >= limit for i in range(len(per_batch))]
        assert done == wanted_done
    assert py[1] == cpp[1], "the C++ driver and the Python mirror issued different ABI calls"
    return py, per_batch


def three(seed=1):
    return [B(300, seed), B(700, seed + 1), B(1500, seed + 2)]  # the largest last: the capacity grows twice


@pytest.mark.parametrize("limit", [-1, 0, 1, 10 ** 6])
def test_three_batches_of_growing_size(be, limit):
    (_, calls, _, written, _), per_batch = both_hosts(be, three(), FILTERS, DIMS, limit)
    assert calls[0] > 0
    if limit == 10 ** 6 or limit < 0:
        assert None not in per_batch and written > 1000  # a limit larger than all survivors
    if limit in (0, 1):
        assert per_batch[1:] == [None, None]  # the first batch runs (and yields nothing for limit 0), then the query is done


def test_limit_reached_in_the_middle_of_the_second_batch(be):
    batches = three(seed=4)
    _, per = expected(batches, FILTERS, DIMS, -1)
    limit = per[0] + per[1] // 2
    (_, calls, done, written, _), per_batch = both_hosts(be, batches, FILTERS, DIMS, limit)
    assert written == limit and per_batch == [per[0], per[1] // 2, None]
    assert calls[2] == 0 and done == [False, True, True]


def test_a_batch_without_survivors_and_an_empty_batch(be):
    nothing = B(500, 9)
    nothing.cols["ts"] = M.Col(abi.Uint32, np.zeros(500, np.uint32), np.ones(500, bool), starting_index=3)
    batches = [B(400, 7), nothing, B(0, 8), B(600, 10)]
    _, per_batch = both_hosts(be, batches, FILTERS, DIMS, -1, max_batch=600)
    assert per_batch[1] == 0 and per_batch[2] == 0 and per_batch[0] > 0 and per_batch[3] > 0


def _run_length_batch():
    """64 rows, every row surviving, 56 runs of one and 8 runs of two: 72 rows, exactly the capacity 64 + 64 / 8"""
    n = 64
    lens = np.ones(n, np.int64)
    lens[3::8] = 2
    return B(n, 13, base_counts=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)), lens


def test_base_counts_expand_to_exactly_the_capacity(be):
    b, lens = _run_length_batch()
    assert lens.sum() == 72
    (got, _, _, written, _), _ = both_hosts(be, [b], ALL_ROWS, DIMS, -1, capacity_of=72)
    assert written == 72


def test_base_counts_with_a_limit_inside_a_run(be):
    b, lens = _run_length_batch()
    limit = int(np.cumsum(lens)[3]) - 1  # one row short of the end of the first run of two
    assert lens[3] == 2
    plain = B(200, 14)
    (_, calls, done, written, _), per_batch = both_hosts(be, [plain, b, plain], [], DIMS, 200 + limit, capacity_of=225)
    assert per_batch == [200, limit, None] and written == 200 + limit


def _filtered_run_length_batch():
    """64 rows in runs of two, and filters that drop more than half of them: the expanded survivors outnumber the survivors
    by far more than an eighth, and fit a buffer sized by the batch's 64 rows (72) — not one sized by its survivors"""
    n = 64
    b = B(n, 17, base_counts=(2 * np.arange(n + 1)).astype(np.uint32))
    survivors = len(M.model_select(b.cols, FILTERS, DIMS, n)[0])
    assert 0 < survivors and survivors + survivors // 8 < 2 * survivors <= n + n // 8
    return b, survivors


def test_base_counts_after_filters_that_drop_rows(be):
    """No AresQuerySetMaxBatchSize: the dimension buffers hold the first batch's rows BEFORE its filters plus an eighth, so
    Expand — which cuts its output at the vector's capacity — keeps every repeated survivor."""
    b, survivors = _filtered_run_length_batch()
    (_, _, _, written, _), per_batch = both_hosts(be, [b, B(40, 18)], FILTERS, DIMS, -1, capacity_of=72)
    assert per_batch[0] == 2 * survivors and written == per_batch[0] + per_batch[1]


def test_a_first_batch_without_rows_or_survivors(be):
    nothing = B(500, 9)
    nothing.cols["ts"] = M.Col(abi.Uint32, np.zeros(500, np.uint32), np.ones(500, bool), starting_index=3)
    _, per_batch = both_hosts(be, [B(0, 8), nothing, B(300, 10), B(500, 11)], FILTERS, DIMS, -1)
    assert per_batch[:2] == [0, 0] and per_batch[2] > 0 and per_batch[3] > 0


def test_two_streams(be):
    streams = [be.call("CreateCudaStream", 0), be.call("CreateCudaStream", 0)]
    try:
        both_hosts(be, three(seed=20), FILTERS, DIMS, 700, streams=streams)
    finally:
        for s in streams:
            be.call("DestroyCudaStream", s, 0)


def _mem_stats(be):
    fn = getattr(be._mem, "AresMemStats", None)
    if fn is None:
        return None
    fn.argtypes, fn.restype = [C.c_int] + [C.POINTER(C.c_size_t)] * 4, None
    v = [C.c_size_t(0) for _ in range(4)]
    fn(0, *[C.byref(x) for x in v])
    return v[0].value, v[1].value, v[2].value


def test_owned_columns_are_freed_and_the_books_balance(be):
    """The batch's columns belong to the query (freed in cleanupBeforeAggregation); after AresQueryDestroy libmem's books —
    live bytes, live blocks, blocks held aside — are back where they started.  Only the product's libmem.so keeps such
    books (AresMemStats): on the oracle and the reference build this test checks no more than that handing the columns over
    neither fails nor frees them twice (glibc aborts on a double free), and that the rows are right."""
    assert be.name != "hip" or _mem_stats(be) is not None
    batches = three(seed=30)
    both_hosts(be, batches[:1], FILTERS, DIMS, -1)  # (staging buffers of the test's own uploads exist from here on)
    before = _mem_stats(be)
    both_hosts(be, batches, FILTERS, DIMS, 500, owned=True)
    assert _mem_stats(be) == before


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["ARES_DEFER=0", "ARES_FUSE=0", "ARES_MEM_VERIFY_CLEAN=1"])
def test_results_do_not_depend_on_the_deferral_switches(switch):
    """ARES_DEFER=0, ARES_FUSE=0 and ARES_MEM_VERIFY_CLEAN=1 are read once per process: this module's tests on the product are
    re-run in a child process with each.  In a non-aggregation batch the partial copy of the dimension vector is the first
    reader of the queued transforms — after WaitForCudaStream and the frees of columns, index and predicate vector."""
    name, value = switch.split("=")
    fused = os.path.join(os.path.dirname(__file__), "test_fused_select.py")  # (its driver tests: "fused_extension")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-k", "hip or fused_extension", __file__, fused],
                       cwd=H.ROOT, env={**os.environ, name: value}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (switch, r.stdout[-2000:], r.stderr[-1000:])
