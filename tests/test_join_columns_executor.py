"""Aggregation queries over joined tables through the C++ driver with AresQuerySetJoinColumns: the joined columns of a batch
without base counts are resolved once, in row space (AresJoinColumnsRun), and the batch runs as a join-free one over the
rewritten plan.  Results must equal the setter-off run — key -> value for HashReduce, rows in order for Sort + Reduce, registers
for HyperLogLog — and an independent numpy group-by over the join model of tests/select_join_model.py.

Four batches of 3 000 - 5 000 rows, the second with base counts (it takes the original plan); one and two foreign tables; with
and without foreign filters; a joined dimension, a joined measure and `joined + constant`.  On the oracle (CPU) the library has
no such entry point: the driver falls back silently."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import harness as H
import select_join_model as J
import select_model as M
import test_nonaggr_join_executor as X
from aresdb_amd import abi, smoke
from aresdb_amd.driver import NativeQuery
from aresdb_amd.executor import Binary, Col, Const, DimensionSpec, ForeignTable, QueryPlan, Unary

FILTERS = M.MIXED_FILTERS  # ts >= 1200, ts < 1900, status != 2
FFILTERS = {1: [(0, "region", abi.LessThan, 150)], 2: [(0, "region", abi.LessThan, 150), (1, "rate", abi.LessThan, 40.0)]}
_MEASURE_NP = {abi.Int64: np.int64, abi.Float32: np.float32, abi.Int32: np.int32, abi.Uint32: np.uint32}


def batches_of(tables, seed=1):
    """four batches, the second with base counts (every run one row long: the sums are those of the rows)"""
    return [tables.batch(3000, seed), tables.batch(4000, seed + 1, base_counts=np.arange(4001, dtype=np.uint32)),
            tables.batch(5000, seed + 2), tables.batch(3500, seed + 3)]


def _expr(name, f=None, c=None):
    col = Col(name) if isinstance(name, str) else Col(name[1], table=name[0] + 1)
    return col if f is None else Binary(f, col, Const(c))


def plan_of(tables, filters, ffilters, dims, measure, agg, measure_type, use_hash, fused=False):
    fts = [ForeignTable(join_column="k%d" % k, index=d.index_struct(), batches={n: [c.vp for c in cols] for n, cols in d.batches.items()},
                        data_types=dict(J.Table.TYPES), base_batch_id=J.BASE_BATCH, num_records_in_last_batch=t.num_last)
           for k, (t, d) in enumerate(zip(tables.tables, tables.device))]
    return QueryPlan(filters=[_expr(n, f, c) for n, f, c in filters], foreign_filters=[_expr((k, n), f, c) for k, n, f, c in ffilters],
                     dimensions=[DimensionSpec(_expr(n, f, c), t) for n, f, c, t in dims], foreign_tables=fts, measure=measure,
                     agg=agg, measure_type=measure_type, use_hash_reduction=use_hash, use_fused_extension=fused)


# the plans: (dimensions, measure column or None for COUNT(*), aggregate, measure type, HashReduce?)
def shapes(count):
    second = [((1, "off"), abi.Plus, 1000, abi.Int32)] if count == 2 else []
    return {
        "sum_hash": ([("ts", abi.Floor, 60, abi.Uint32), ((0, "region"), None, None, abi.Uint32)] + second, "ts", abi.AGGR_SUM_SIGNED, abi.Int64, True),
        "count_sort": ([((0, "region"), abi.Plus, 5, abi.Uint32), ("city", None, None, abi.Uint16), ((count - 1, "tz"), None, None, abi.Uint8)],
                       None, abi.AGGR_SUM_UNSIGNED, abi.Uint32, False),
        "min_sort": ([((0, "region"), None, None, abi.Uint32)] + second, (count - 1, "off"), abi.AGGR_MIN_SIGNED, abi.Int32, False),
        "fsum_sort": ([("city", None, None, abi.Uint16)], (0, "rate"), abi.AGGR_SUM_FLOAT, abi.Float32, False),
    }


def build(tables, shape, ffilters, fused=False, filters=FILTERS):
    dims, measure, agg, mtype, use_hash = shape
    m = Const(1) if measure is None else _expr(measure)
    return plan_of(tables, filters, ffilters, dims, m, agg, mtype, use_hash, fused)


def run(be, plan, batches, join_columns, hll=False):
    """(result, ABI calls per batch, fused batches): result = (dims, valids, measures) as fetched, or the HyperLogLog groups"""
    q = NativeQuery(be, plan, list(batches[0].cols.keys()))
    if join_columns:
        q.set_join_columns(True)
    calls = []
    for i, b in enumerate(batches):
        dev = {k: c.upload(be) for k, c in b.cols.items()}
        bc = H.Buf(be, b.base_counts) if b.base_counts is not None else None
        before = q.calls
        q.run({k: d.vp for k, d in dev.items()}, b.n, base_counts=bc.ptr if bc else None, is_last_batch=hll and i == len(batches) - 1,
              owned_allocations=[d.buf.ptr for d in dev.values()])
        calls.append(q.calls - before)
        if bc:
            bc.free()
    res = smoke._hll_groups(*q.fetch_hll()) if hll else q.fetch()
    fused = q.fused_batches
    q.release()
    return res, calls, fused


def groups(plan, res):
    dims, valids, meas = res
    n = len(valids[0])
    m = meas.view(_MEASURE_NP[plan.measure_type])
    out = {}
    for r in range(n):
        key = tuple((bytes(d[r * len(d) // n:(r + 1) * len(d) // n]), int(v[r])) for d, v in zip(dims, valids))
        assert key not in out
        out[key] = m[r]
    return out


def expected(tables, batches, shape, ffilters, filters=FILTERS):
    """the numpy group-by: {key: value}; a null measure contributes the aggregate's identity"""
    dims, measure, agg, mtype, _ = shape
    out = {}
    for b in batches:
        n = b.n
        keep = np.ones(n, bool)
        for name, f, c in filters:
            keep &= M.model_filter(b.cols[name], f, c, n)
        for k, name, f, c in ffilters:
            keep &= M.model_filter(J._resolve(b.cols, tables.joins(), (k, name), n), f, c, n)
        parts = [M.model_dim(J._resolve(b.cols, tables.joins(), name, n), f, c, t, n) for name, f, c, t in dims]
        if measure is None:
            vals, ok = np.ones(n, np.int64), np.ones(n, bool)
        else:
            col = J._resolve(b.cols, tables.joins(), measure, n)
            vals, ok = col.values[:n], M._valid(col, n)
        for i in np.flatnonzero(keep):
            key = tuple((bytes(v[i]), int(o[i])) for v, o in parts)
            if agg == abi.AGGR_MIN_SIGNED:
                out[key] = min(out.get(key, 2 ** 31 - 1), int(vals[i]) if ok[i] else 2 ** 31 - 1)
            elif agg == abi.AGGR_SUM_FLOAT:
                out[key] = out.get(key, 0.0) + (float(vals[i]) if ok[i] else 0.0)
            else:
                out[key] = out.get(key, 0) + (int(vals[i]) if ok[i] else 0)
    return out


def assert_groups(got, want, agg):
    assert got.keys() == want.keys(), (len(got), len(want))
    for k, v in want.items():
        if agg == abi.AGGR_SUM_FLOAT:  # a float32 accumulator: tests/test_hip_parity.py::_float_tolerance
            assert abs(float(got[k]) - v) <= 1e-4 * max(1.0, abs(v)), (k, got[k], v)
        else:
            assert int(got[k]) == v, (k, got[k], v)


def assert_rows(on, off, agg):
    """Sort + Reduce: rows, order and values of the setter-off run"""
    for a, b in zip(on[0] + on[1], off[0] + off[1]):
        assert np.array_equal(a, b)
    if agg == abi.AGGR_SUM_FLOAT:
        x, y = on[2].view(np.float32), off[2].view(np.float32)
        assert len(x) == len(y) and np.all(np.abs(x - y) <= 1e-4 * np.maximum(1.0, np.abs(y)))
    else:
        assert np.array_equal(on[2], off[2])


@pytest.mark.parametrize("with_ffilters", [True, False], ids=["ffilters", "plain"])
@pytest.mark.parametrize("count", [1, 2])
def test_results_equal_the_setter_off_run_and_numpy(be, count, with_ffilters):
    """On the product an eligible batch issues one AresJoinColumnsRun per foreign table the query reads in place of that table's
    HashLookup.  On the oracle nothing changes at all."""
    tables = X.Tables(be, count)
    ffilters = FFILTERS[count] if with_ffilters else []
    try:
        batches = batches_of(tables)
        for name, shape in shapes(count).items():
            plan = build(tables, shape, ffilters)
            off, calls_off, _ = run(be, plan, batches, False)
            stats = be.join_column_stats() if be.name == "hip" else None
            on, calls_on, _ = run(be, plan, batches, True)
            want = expected(tables, batches, shape, ffilters)
            assert len(want) > 3, name
            assert_groups(groups(plan, off), want, shape[2])
            assert_groups(groups(plan, on), want, shape[2])
            if not shape[4]:
                assert_rows(on, off, shape[2])
            # the tables the query reads; a table nothing reads is not probed at all on the new path
            read = len({n[0] for n in [d[0] for d in shape[0]] + [shape[1]] if isinstance(n, tuple)} | {f[0] for f in ffilters})
            if stats is None:
                assert calls_on == calls_off, name
            else:
                assert calls_on == [c - (count - read if b.base_counts is None else 0) for c, b in zip(calls_off, batches)], name
                be.wait()
                after = be.join_column_stats()
                assert after["batches"] - stats["batches"] == 3 * read and after["declined"] == stats["declined"], name
                assert after["rows"] - stats["rows"] == (3000 + 5000 + 3500) * read
                assert 0 < after["probed"] - stats["probed"] < after["rows"] - stats["rows"]  # (the hints pruned)
    finally:
        tables.free()


def test_hyperloglog_registers_are_equal(be):
    tables = X.Tables(be, 1)
    try:
        batches = batches_of(tables, seed=5)
        plan = plan_of(tables, FILTERS, FFILTERS[1], [((0, "region"), None, None, abi.Uint32), ("city", abi.Floor, 100, abi.Uint32)],
                       Unary(abi.GetHLLValue, Col("off", table=1)), abi.AGGR_HLL, abi.Uint32, False)
        off, calls_off, _ = run(be, plan, batches, False, hll=True)
        on, calls_on, _ = run(be, plan, batches, True, hll=True)
        assert len(off) > 3 and on == off and calls_on == calls_off
    finally:
        tables.free()


def test_ineligible_queries_are_untouched(be):
    """a wide joined column (UUID dimension): the setter has no effect, no entry point is asked"""
    tables = X.Tables(be, 1)
    try:
        batches = batches_of(tables, seed=9)[:2]
        plan = plan_of(tables, FILTERS, [], [((0, "uid"), None, None, abi.UUID), ((0, "region"), None, None, abi.Uint32)], Const(1),
                       abi.AGGR_SUM_UNSIGNED, abi.Uint32, False)
        stats = be.join_column_stats() if be.name == "hip" else None
        off, calls_off, _ = run(be, plan, batches, False)
        on, calls_on, _ = run(be, plan, batches, True)
        assert_rows(on, off, plan.agg)
        assert calls_on == calls_off and len(off[1][0]) > 3
        assert stats is None or be.join_column_stats() == stats
    finally:
        tables.free()


# ---- the product ---------------------------------------------------------------------------------------------------------
HOT_FILTERS = FILTERS[:2]  # (4-byte columns only: what AresFusedFilterHashReduce takes)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 2])
def test_with_the_fused_extension_an_eligible_batch_is_one_call_per_table_and_one_fused_call(count):
    hip = H.hip_backend()
    tables = X.Tables(hip, count)
    ffilters = [f for f in FFILTERS[count] if f[1] == "region"]
    try:
        batches = batches_of(tables, seed=3)
        shape = shapes(count)["sum_hash"]
        off, calls_off, fused_off = run(hip, build(tables, shape, ffilters, fused=True, filters=HOT_FILTERS), batches, False)
        on, calls_on, fused_on = run(hip, build(tables, shape, ffilters, fused=True, filters=HOT_FILTERS), batches, True)
        want = expected(tables, batches, shape, ffilters, filters=HOT_FILTERS)
        plan = build(tables, shape, ffilters)
        assert_groups(groups(plan, off), want, shape[2])
        assert_groups(groups(plan, on), want, shape[2])
        assert fused_off == 0 and fused_on == 3  # (a plan with foreign tables never takes the fused call; the rewritten one does)
        assert [calls_on[i] for i in (0, 2, 3)] == [count + 1] * 3 and calls_on[1] == calls_off[1]
    finally:
        tables.free()


def _profile(hip, fn):
    hip.wait()
    hip.profiler_enable(True)
    try:
        fn()
        hip.wait()
        return hip.profiler_report()
    finally:
        hip.profiler_enable(False)


def _launches(kernels, prefix):
    return sum(v[0] for k, v in kernels.items() if k.startswith(prefix))


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 2])
def test_kernels_of_the_eligible_batches(count):
    """One join_columns_kernel per eligible batch and foreign table; no probe over record ids, no foreign transform, no generic
    or predicate filter kernel in those batches; the hot-shape HashReduce plan launches no transform at all (its queue is
    consumed by the reduction).  With the setter off the per-node join sequence is there."""
    hip = H.hip_backend()
    tables = X.Tables(hip, count)
    try:
        batches = [b for b in batches_of(tables, seed=7) if b.base_counts is None]
        for name in ("sum_hash", "count_sort"):
            shape = shapes(count)[name]
            ffilters = [f for f in FFILTERS[count] if f[1] == "region"] if name == "sum_hash" else FFILTERS[count]
            plan = build(tables, shape, ffilters, filters=HOT_FILTERS if name == "sum_hash" else FILTERS)
            run(hip, plan, batches, True)  # priming pass: the shape's generated kernels are compiled
            hip.rtc_wait()
            on = _profile(hip, lambda: run(hip, plan, batches, True))
            off = _profile(hip, lambda: run(hip, plan, batches, False))
            print(name, count, "on:", sorted(on), "off:", sorted(off))
            assert _launches(on, "join_columns_kernel") == len(batches) * count and _launches(off, "join_columns_kernel") == 0
            # (without the deferral machinery there are no row-space filters — a hot-shape filter is filter_pred_kernel — and
            # no queue for the reduction to consume)
            deferral = os.environ.get("ARES_FUSE", "1") != "0" and os.environ.get("ARES_DEFER", "1") != "0"
            for gone in ("hash_lookup_kernel", "transform_foreign_kernel", "filter_kernel") + (("filter_pred_kernel",) if deferral else ()):
                assert _launches(on, gone) == 0, (name, gone, sorted(on))
            for there in ("hash_lookup_kernel", "transform_foreign_kernel", "filter_kernel") + (("filter_pred_kernel",) if deferral else ()):
                assert _launches(off, there) > 0, (name, there, sorted(off))
            if name == "sum_hash" and deferral:
                assert _launches(on, "transform_multi_kernel") == 0, sorted(on)
    finally:
        tables.free()


def _mem_stats(be):
    fn = be._mem.AresMemStats
    fn.argtypes, fn.restype = [C.c_int] + [C.POINTER(C.c_size_t)] * 4, None
    v = [C.c_size_t(0) for _ in range(4)]
    fn(0, *[C.byref(x) for x in v])
    return v[0].value, v[1].value, v[2].value


def _temp_handed_out(be):
    out, cached = C.c_size_t(0), C.c_size_t(0)
    be._algo.AresTempStats.argtypes, be._algo.AresTempStats.restype = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], None
    be._algo.AresTempStats(C.byref(out), C.byref(cached))
    return out.value


@pytest.mark.gpu
def test_the_books_balance_and_temporaries_do_not_pile_up():
    """the joined columns are the query's (DeviceAllocate, released with the batch's input columns): after the query libmem's
    books are back at the start, and libalgorithm's stream temporaries do not grow batch over batch"""
    hip = H.hip_backend()
    tables = X.Tables(hip, 2)
    try:
        batches = batches_of(tables, seed=11)
        plan = build(tables, shapes(2)["sum_hash"], FFILTERS[2])
        run(hip, plan, batches, True)  # (staging buffers of the test's own uploads exist from here on)
        before = _mem_stats(hip)
        run(hip, plan, batches, True)
        assert _mem_stats(hip) == before
        q = NativeQuery(hip, plan, list(batches[0].cols.keys()))
        q.set_join_columns(True)
        handed = []
        for b in [batches[0]] * 5:
            dev = {k: c.upload(hip) for k, c in b.cols.items()}
            q.run({k: d.vp for k, d in dev.items()}, b.n, owned_allocations=[d.buf.ptr for d in dev.values()])
            handed.append(_temp_handed_out(hip))
        q.release()
        assert handed[4] <= handed[1], handed
    finally:
        tables.free()


@pytest.mark.gpu
def test_a_decline_sends_the_batch_down_the_original_plan_and_the_query_stops_asking():
    hip = H.hip_backend()
    tables = X.Tables(hip, 1)
    try:
        batches = batches_of(tables, seed=13)
        shape = shapes(1)["count_sort"]
        plan = build(tables, shape, FFILTERS[1])
        off, calls_off, _ = run(hip, plan, batches, False)
        os.environ["ARES_JOIN_COLUMNS"] = "0"
        hip.reload_env()
        try:
            before = hip.join_column_stats()
            on, calls_on, _ = run(hip, plan, batches, True)
            after = hip.join_column_stats()
        finally:
            del os.environ["ARES_JOIN_COLUMNS"]
            hip.reload_env()
        assert_rows(on, off, shape[2])
        assert [a - b for a, b in zip(calls_on, calls_off)] == [1, 0, 0, 0]
        assert after["declined"] - before["declined"] == 1 and after["batches"] == before["batches"]
    finally:
        tables.free()


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["ARES_DEFER=0", "ARES_MEM_VERIFY_CLEAN=1"])
def test_results_do_not_depend_on_the_deferral_switches(switch):
    """both are read once per process: this module's tests on the product are re-run in a child process with each"""
    name, value = switch.split("=")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-k", "not deferral_switches", "-p", "no:cacheprovider", __file__],
                       cwd=H.ROOT, env={**os.environ, name: value}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (switch, r.stdout[-4000:], r.stderr[-1000:])
