"""Local-time bucketing through the C++ driver with AresQuerySetJoinColumns: an eligible CONVERT_TZ node is one resolved leaf —
AresLocalTimeColumnRun writes time + the zone's offset once per batch as an ordinary column, and the batch runs
`Floor(that column, 3600)` on the fast paths.  Results must equal the setter-off run — key -> value for HashReduce, rows in order
for Sort + Reduce, registers for HyperLogLog — and the numpy group-by over the model of tests/local_time_model.py.

Four batches of 3 000 - 5 000 rows, the second with base counts (it takes the original plan).  Table 0 is joined on a Uint16 key
(fewer rows than key values: the probe flavour unless forced), table 1 on a Uint8 key (the direct flavour).  On the oracle (CPU)
the library has no such entry point: the setter changes nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

import harness as H
import test_fused_select as F
import test_join_columns_executor as XE
import test_local_time_hosts as TH
from aresdb_amd import abi
from aresdb_amd.executor import Col, Const, Unary

FILTERS = TH.FILTERS
HOT_FILTERS = FILTERS[:2]  # (4-byte columns only: what AresFusedFilterHashReduce takes)
HOUR0, HOUR1 = TH.LOCAL_HOUR, (("tz", 1, "zone16"), abi.Floor, 3600, abi.Uint32)
REGION0, REGION1 = ((0, "region"), None, None, abi.Uint32), ((1, "region"), None, None, abi.Uint32)
KEYS = {1: (abi.Uint16,), 2: (abi.Uint16, abi.Uint8)}

# name: (tables, dimensions, measure column or None for COUNT(*), aggregate, measure type, HashReduce?, foreign filters,
#        calls of an eligible batch relative to the setter-off run: - HashLookup per table - the Plus of every CONVERT_TZ node
#        + AresLocalTimeColumnRun per distinct local time + AresJoinColumnsRun per table other leaves read)
SHAPES = {
    "count_sort": (1, [HOUR0, ("city", None, None, abi.Uint16)], None, abi.AGGR_SUM_UNSIGNED, abi.Uint32, False, [], -1 - 1 + 1),
    "sum_hash": (1, [HOUR0, REGION0], "ts", abi.AGGR_SUM_SIGNED, abi.Int64, True, [], -1 - 1 + 1 + 1),
    "two_tables": (2, [HOUR0, HOUR1, REGION1, (("tz", 0, "zone8"), abi.Floor, 86400, abi.Uint32)], "amount", abi.AGGR_SUM_SIGNED, abi.Int64,
                   True, [(0, "zone16", abi.LessThan, 30)], -2 - 3 + 2 + 2),
}


def batches_of(zones, seed=1):
    """four batches, the second with base counts (every run one row long: the sums are those of the rows)"""
    return [zones.batch(3000, seed), zones.batch(4000, seed + 1, base_counts=np.arange(4001, dtype=np.uint32)),
            zones.batch(5000, seed + 2), zones.batch(3500, seed + 3)]


def build(zones, shape, fused=False, filters=FILTERS):
    _, dims, measure, agg, mtype, use_hash, ffilters, _ = shape
    m = Const(1) if measure is None else Col(measure)
    return TH.plan_of(zones, filters, ffilters, dims, m, agg, mtype, use_hash, fused)


def want_of(zones, batches, shape, filters=FILTERS):
    _, dims, measure, agg, _, _, ffilters, _ = shape
    return TH.expected(zones, batches, dims, measure, agg, filters=filters, ffilters=ffilters)


@pytest.mark.parametrize("name", list(SHAPES))
def test_results_equal_the_setter_off_run_and_numpy(be, name):
    shape = SHAPES[name]
    zones = TH.Zones(be, KEYS[shape[0]])
    try:
        batches = batches_of(zones)
        plan = build(zones, shape)
        off, calls_off, _ = XE.run(be, plan, batches, False)
        stats = be.local_time_column_stats() if be.name == "hip" else None
        on, calls_on, _ = XE.run(be, plan, batches, True)
        want = want_of(zones, batches, shape)
        assert len(want) > 20, name
        XE.assert_groups(XE.groups(plan, off), want, shape[3])
        XE.assert_groups(XE.groups(plan, on), want, shape[3])
        if not shape[5]:
            XE.assert_rows(on, off, shape[3])
        if stats is None:  # the oracle: the setter changes nothing
            assert calls_on == calls_off, name
        else:
            assert calls_on == [c + (shape[7] if b.base_counts is None else 0) for c, b in zip(calls_off, batches)], name
            be.wait()
            after = be.local_time_column_stats()
            times = len({d[0][1:] for d in shape[1] if d[0][0] == "tz"})
            assert after["batches"] - stats["batches"] == 3 * times and after["declined"] == stats["declined"], name
            assert after["rows"] - stats["rows"] == (3000 + 5000 + 3500) * times
            assert after["direct"] - stats["direct"] == (3 if name == "two_tables" else 0)  # (the Uint8 key of table 1)
    finally:
        zones.free()


def test_hyperloglog_registers_are_equal(be):
    zones = TH.Zones(be)
    try:
        batches = batches_of(zones, seed=5)
        plan = TH.plan_of(zones, FILTERS, [], [HOUR0, ("city", abi.Floor, 100, abi.Uint32)], Unary(abi.GetHLLValue, Col("region", table=1)),
                          abi.AGGR_HLL, abi.Uint32, False)
        off, calls_off, _ = XE.run(be, plan, batches, False, hll=True)
        on, calls_on, _ = XE.run(be, plan, batches, True, hll=True)
        assert len(off) > 3 and on == off
        # - HashLookup - Plus + AresLocalTimeColumnRun + AresJoinColumnsRun
        assert calls_on == calls_off
    finally:
        zones.free()


def test_ineligible_shapes_are_untouched(be):
    """a CONVERT_TZ node that is a dimension's root, one over a Uint32 column of the table, one whose time is an expression, and
    three distinct local times: the setter has no effect, no entry point is asked"""
    from aresdb_amd.executor import Binary, DimensionSpec
    zones = TH.Zones(be, KEYS[2])
    try:
        batches = batches_of(zones, seed=9)[:2]
        root = DimensionSpec(Binary(abi.Plus, Col(TH.TIME), Col("zone8", table=1), convert_tz=True), abi.Uint32)
        wide_zone = DimensionSpec(TH.expr(("tz", 0, "region"), abi.Floor, 3600), abi.Uint32)
        inner = Binary(abi.Plus, Binary(abi.Plus, Col(TH.TIME), Const(0), out_type=abi.Uint32), Col("zone8", table=1), out_type=abi.Uint32, convert_tz=True)
        expression = DimensionSpec(Binary(abi.Floor, inner, Const(3600)), abi.Uint32)
        three = [DimensionSpec(TH.expr(n, f, c), t) for n, f, c, t in (HOUR0, HOUR1, (("tz", 1, "zone8"), abi.Floor, 3600, abi.Uint32))]
        stats = (be.local_time_column_stats(), be.join_column_stats()) if be.name == "hip" else None
        for dims in ([root], [wide_zone], [expression], three):
            plan = TH.plan_of(zones, FILTERS, [], [], Const(1), abi.AGGR_SUM_UNSIGNED, abi.Uint32, False)
            plan.dimensions = dims
            off, calls_off, _ = XE.run(be, plan, batches, False)
            on, calls_on, _ = XE.run(be, plan, batches, True)
            XE.assert_rows(on, off, plan.agg)
            assert calls_on == calls_off and len(off[1][0]) > 3
        assert stats is None or (be.local_time_column_stats(), be.join_column_stats()) == stats
    finally:
        zones.free()


# ---- the product ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_with_the_fused_extension_an_eligible_batch_is_the_resolving_calls_and_one_fused_call():
    hip = H.hip_backend()
    zones = TH.Zones(hip)
    try:
        batches = batches_of(zones, seed=3)
        shape = SHAPES["sum_hash"]
        off, calls_off, fused_off = XE.run(hip, build(zones, shape, fused=True, filters=HOT_FILTERS), batches, False)
        on, calls_on, fused_on = XE.run(hip, build(zones, shape, fused=True, filters=HOT_FILTERS), batches, True)
        want = want_of(zones, batches, shape, filters=HOT_FILTERS)
        plan = build(zones, shape)
        XE.assert_groups(XE.groups(plan, off), want, shape[3])
        XE.assert_groups(XE.groups(plan, on), want, shape[3])
        assert fused_off == 0 and fused_on == 3  # (a plan with foreign tables never takes the fused call; the rewritten one does)
        # AresJoinColumnsRun (region), AresLocalTimeColumnRun, AresFusedFilterHashReduce
        assert [calls_on[i] for i in (0, 2, 3)] == [3] * 3 and calls_on[1] == calls_off[1]
    finally:
        zones.free()


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ["probe", "direct"])
def test_kernels_of_the_eligible_batches(flavour):
    """One local-time launch per eligible batch (two for the direct flavour: the table, then the rows); no probe over record ids
    — not even HashLookup's for a table only the zone column reads —, no foreign transform, no generic or predicate filter kernel;
    the hot-shape HashReduce plan launches no transform at all (its queue is consumed by the reduction).  With the setter off
    the per-node join sequence is there."""
    hip = H.hip_backend()
    zones = TH.Zones(hip)
    try:
        batches = [b for b in batches_of(zones, seed=7) if b.base_counts is None]
        with F._Env(hip, ARES_LOCAL_TIME=flavour):
            for name in ("sum_hash", "count_sort"):
                plan = build(zones, SHAPES[name], filters=HOT_FILTERS if name == "sum_hash" else FILTERS)
                XE.run(hip, plan, batches, True)  # priming pass: the shape's generated kernels are compiled
                hip.rtc_wait()
                on = XE._profile(hip, lambda: XE.run(hip, plan, batches, True))
                off = XE._profile(hip, lambda: XE.run(hip, plan, batches, False))
                print(name, flavour, "on:", sorted(on), "off:", sorted(off))
                if flavour == "direct":
                    assert XE._launches(on, "local_time_table_kernel") == XE._launches(on, "local_time_rows_kernel") == len(batches)
                    assert XE._launches(on, "local_time_probe_kernel") == 0
                else:
                    assert XE._launches(on, "local_time_probe_kernel") == len(batches) and XE._launches(on, "local_time_table_kernel") == 0
                assert XE._launches(off, "local_time_") == 0
                assert XE._launches(on, "join_columns_kernel") == (len(batches) if name == "sum_hash" else 0)
                deferral = os.environ.get("ARES_FUSE", "1") != "0" and os.environ.get("ARES_DEFER", "1") != "0"
                gone = ("hash_lookup_kernel", "transform_foreign_kernel", "filter_kernel") + (("filter_pred_kernel",) if deferral else ())
                for kernel in gone:
                    assert XE._launches(on, kernel) == 0, (name, kernel, sorted(on))
                # (the setter-off run probes per survivor; its Plus through the offset table is a generic transform into scratch)
                assert XE._launches(off, "hash_lookup_kernel") == len(batches), (name, sorted(off))
                if name == "sum_hash" and deferral:
                    assert XE._launches(on, "transform_multi_kernel") == 0, sorted(on)
    finally:
        zones.free()


@pytest.mark.gpu
def test_the_books_balance_and_temporaries_do_not_pile_up():
    """the local-time columns are the query's (DeviceAllocate, released with the batch's input columns) and the direct flavour's
    table a stream temporary: after the query libmem's books are back at the start, and libalgorithm's temporaries do not grow
    batch over batch"""
    from aresdb_amd.driver import NativeQuery
    hip = H.hip_backend()
    zones = TH.Zones(hip, KEYS[2])
    try:
        batches = batches_of(zones, seed=11)
        plan = build(zones, SHAPES["two_tables"])
        XE.run(hip, plan, batches, True)  # (staging buffers of the test's own uploads exist from here on)
        before = XE._mem_stats(hip)
        XE.run(hip, plan, batches, True)
        assert XE._mem_stats(hip) == before
        q = NativeQuery(hip, plan, list(batches[0].cols.keys()))
        q.set_join_columns(True)
        handed = []
        for b in [batches[0]] * 5:
            dev = {k: c.upload(hip) for k, c in b.cols.items()}
            q.run({k: d.vp for k, d in dev.items()}, b.n, owned_allocations=[d.buf.ptr for d in dev.values()])
            handed.append(XE._temp_handed_out(hip))
        q.release()
        assert handed[4] <= handed[1], handed
    finally:
        zones.free()


@pytest.mark.gpu
def test_a_decline_sends_the_batch_down_the_original_plan_and_the_query_stops_asking():
    hip = H.hip_backend()
    zones = TH.Zones(hip)
    try:
        batches = batches_of(zones, seed=13)
        shape = SHAPES["count_sort"]
        plan = build(zones, shape)
        off, calls_off, _ = XE.run(hip, plan, batches, False)
        with F._Env(hip, ARES_LOCAL_TIME="0"):
            before = hip.local_time_column_stats()
            on, calls_on, _ = XE.run(hip, plan, batches, True)
            after = hip.local_time_column_stats()
        XE.assert_rows(on, off, shape[3])
        assert [a - b for a, b in zip(calls_on, calls_off)] == [1, 0, 0, 0]
        assert after["declined"] - before["declined"] == 1 and after["batches"] == before["batches"]
    finally:
        zones.free()


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["ARES_DEFER=0", "ARES_MEM_VERIFY_CLEAN=1"])
def test_results_do_not_depend_on_the_deferral_switches(switch):
    """both are read once per process: this module's tests on the product are re-run in a child process with each"""
    name, value = switch.split("=")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-k", "not deferral_switches", "-p", "no:cacheprovider", __file__],
                       cwd=H.ROOT, env={**os.environ, name: value}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (switch, r.stdout[-4000:], r.stderr[-1000:])
