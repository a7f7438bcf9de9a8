"""Local-time bucketing on the ordinary path of both hosts: FLOOR(CONVERT_TZ(request_at, table.zone), 3600) as a dimension.  The
Python mirror and the C++ driver hand the foreign leaf directly below the CONVERT_TZ node to the library with the plan's offset
table and every other foreign leaf without it (query/time_series_aggregate.go:506-516): both must equal the numpy group-by over
the model of tests/local_time_model.py, with the same number of ABI calls.

A dimension is select_model's (name, functor, constant, out type); name = (join, column) reads a joined column as it stands,
name = ("tz", join, zone column) is CONVERT_TZ(request_at, that column)."""
import numpy as np
import pytest

import harness as H
import local_time_model as L
import select_join_model as J
import select_model as M
import test_join_columns_executor as XE
import test_nonaggr_executor as E
from aresdb_amd import abi
from aresdb_amd.executor import BatchContext, BatchExecutor, Binary, Col, Const, DimensionSpec, ForeignTable, QueryPlan, fetch_results

FILTERS = M.MIXED_FILTERS  # ts >= 1200, ts < 1900, status != 2
TIME = "request_at"


class Zones:
    """the dimension tables of a query (the mode-0 batch without a default: the hosts pass none), their device copies and the
    offset table on the device"""

    def __init__(self, be, key_dtypes=(abi.Uint16,)):
        self.be = be
        self.tables = [L.make_table(dtype, default=False, seed=11 + 12 * k) for k, dtype in enumerate(key_dtypes)]
        self.device = [t.upload(be) for t in self.tables]
        self.tz = L.tz_offsets()
        self.tz_buf = H.Buf(be, self.tz)

    def joins(self):
        return [("k%d" % k, t) for k, t in enumerate(self.tables)]

    def batch(self, n, seed, base_counts=None, time_dtype=abi.Uint32):
        cols = M.mixed_columns(max(n, 1), seed=seed)
        for k, t in enumerate(self.tables):
            time, cols["k%d" % k] = L.columns(t, max(n, 1), seed + 100 * k + 50, time_dtype)
            if k == 0:
                cols[TIME] = time
        return E.B(n, seed, base_counts=base_counts, cols=cols)

    def free(self):
        for d in self.device + [self.tz_buf]:
            d.free()


def expr(name, f=None, c=None, tz_type=abi.Uint32):
    if isinstance(name, tuple) and name[0] == "tz":
        col = Binary(abi.Plus, Col(TIME), Col(name[2], table=name[1] + 1), out_type=tz_type, convert_tz=True)
    else:
        col = Col(name) if isinstance(name, str) else Col(name[1], table=name[0] + 1)
    return col if f is None else Binary(f, col, Const(c))


def plan_of(zones, filters, ffilters, dims, measure, agg, measure_type, use_hash, fused=False, tz_type=abi.Uint32):
    fts = [ForeignTable(join_column="k%d" % k, index=d.index_struct(), batches={n: [c.vp for c in cols] for n, cols in d.batches.items()},
                        data_types=dict(t.TYPES), base_batch_id=J.BASE_BATCH, num_records_in_last_batch=t.num_last)
           for k, (t, d) in enumerate(zip(zones.tables, zones.device))]
    return QueryPlan(filters=[expr(n, f, c) for n, f, c in filters], foreign_filters=[expr((k, n), f, c) for k, n, f, c in ffilters],
                     dimensions=[DimensionSpec(expr(n, f, c, tz_type), t) for n, f, c, t in dims], foreign_tables=fts, measure=measure,
                     agg=agg, measure_type=measure_type, use_hash_reduction=use_hash, use_fused_extension=fused,
                     timezone_lookup=zones.tz_buf.ptr, timezone_lookup_size=len(zones.tz))


def resolve(zones, b, name, tz_type=abi.Uint32):
    """the column a dimension or measure reads, as a select_model.Col"""
    if isinstance(name, tuple) and name[0] == "tz":
        values, valid, _ = L.local_time(zones.tables[name[1]], zones.tz, b.cols[TIME], b.cols["k%d" % name[1]], name[2], b.n)
        return M.Col(tz_type, values.view(np.int32) if tz_type == abi.Int32 else values, valid)
    return J._resolve(b.cols, zones.joins(), name, b.n)


def expected(zones, batches, dims, measure, agg, filters=FILTERS, ffilters=(), tz_type=abi.Uint32):
    """the numpy group-by: {key: value}; a null measure contributes the aggregate's identity (sums only)"""
    out = {}
    for b in batches:
        n = b.n
        keep = np.ones(n, bool)
        for name, f, c in filters:
            keep &= M.model_filter(b.cols[name], f, c, n)
        for k, name, f, c in ffilters:
            keep &= M.model_filter(resolve(zones, b, (k, name)), f, c, n)
        parts = [M.model_dim(resolve(zones, b, name, tz_type), f, c, t, n) for name, f, c, t in dims]
        if measure is None:
            vals, ok = np.ones(n, np.int64), np.ones(n, bool)
        else:
            col = resolve(zones, b, measure)
            vals, ok = col.values[:n], M._valid(col, n)
        for i in np.flatnonzero(keep):
            key = tuple((bytes(v[i]), int(o[i])) for v, o in parts)
            add = (float(vals[i]) if agg == abi.AGGR_SUM_FLOAT else int(vals[i])) if ok[i] else 0
            out[key] = out.get(key, 0) + add
    return out


def run_mirror(be, plan, batches):
    ctx = BatchContext(be, plan)
    ex = BatchExecutor(ctx)
    for b in batches:
        dev = {k: c.upload(be) for k, c in b.cols.items()}
        bc = H.Buf(be, b.base_counts) if b.base_counts is not None else None
        ex.run({k: d.vp for k, d in dev.items()}, b.n, base_counts=bc.ptr if bc else None, owned_columns=[d.free for d in dev.values()])
        if bc:
            bc.free()
    res = fetch_results(ctx)
    ctx.release()
    return res, ctx.calls


LOCAL_HOUR = (("tz", 0, "zone8"), abi.Floor, 3600, abi.Uint32)


def batches_of(zones, seed=1, **kw):
    return [zones.batch(900, seed, **kw), zones.batch(1, seed + 1, **kw), zones.batch(1300, seed + 2, **kw)]


@pytest.mark.parametrize("use_hash", [True, False], ids=["hash", "sort"])
def test_both_hosts_equal_the_numpy_group_by(be, use_hash):
    """local hour + the zone enum of the same table as it stands + city: the leaf below CONVERT_TZ is read through the offset
    table, the plain leaf of the same column is not — either mistake changes the groups"""
    zones = Zones(be)
    try:
        batches = batches_of(zones)
        dims = [LOCAL_HOUR, ("city", None, None, abi.Uint16), ((0, "zone8"), None, None, abi.Uint8)]
        plan = plan_of(zones, FILTERS, [], dims, Col("amount"), abi.AGGR_SUM_SIGNED, abi.Int64, use_hash)
        want = expected(zones, batches, dims, "amount", abi.AGGR_SUM_SIGNED)
        hours = {k[0] for k in want if k[0][1]}
        assert len(want) > 50 and len(hours) > 10
        enums = {k[2][0][0] for k in want if k[2][1]}  # (read through the table they would be offsets' low bytes)
        assert len(enums) > 10 and any((int(zones.tz[e]) & 0xFF) != e for e in enums if e < L.TZ_SIZE)
        mirror, mirror_calls = run_mirror(be, plan, batches)
        native, native_calls, _ = XE.run(be, plan, batches, False)
        XE.assert_groups(XE.groups(plan, mirror), want, plan.agg)
        XE.assert_groups(XE.groups(plan, native), want, plan.agg)
        assert mirror_calls == sum(native_calls)
        if not use_hash:
            XE.assert_rows(native, mirror, plan.agg)
    finally:
        zones.free()


@pytest.mark.parametrize("time_dtype,tz_type", [(abi.Int32, abi.Int32), (abi.Uint32, abi.Int32)])
def test_an_int32_time_column_and_a_uint16_zone(be, time_dtype, tz_type):
    """a foreign filter on the same table beside the CONVERT_TZ node: it reads its column without the offset table"""
    zones = Zones(be)
    try:
        batches = batches_of(zones, seed=21, time_dtype=time_dtype)
        dims = [(("tz", 0, "zone16"), abi.Floor, 3600, abi.Uint32)]
        ffilters = [(0, "zone16", abi.LessThan, L.TZ_SIZE)]
        plan = plan_of(zones, FILTERS, ffilters, dims, Const(1), abi.AGGR_SUM_UNSIGNED, abi.Uint32, False, tz_type=tz_type)
        want = expected(zones, batches, dims, None, abi.AGGR_SUM_UNSIGNED, ffilters=ffilters, tz_type=tz_type)
        assert len(want) > 10
        mirror, mirror_calls = run_mirror(be, plan, batches)
        native, native_calls, _ = XE.run(be, plan, batches, False)
        XE.assert_groups(XE.groups(plan, mirror), want, plan.agg)
        XE.assert_groups(XE.groups(plan, native), want, plan.agg)
        XE.assert_rows(native, mirror, plan.agg)
        assert mirror_calls == sum(native_calls)
    finally:
        zones.free()


def test_a_plan_without_convert_tz_nodes_hands_no_table_over(be):
    """the plan has an offset table but no node marked: every foreign leaf is read as it stands"""
    zones = Zones(be)
    try:
        batches = batches_of(zones, seed=31)
        dims = [((0, "zone8"), abi.Plus, 0, abi.Uint32), ("city", None, None, abi.Uint16)]
        plan = plan_of(zones, FILTERS, [], dims, Const(1), abi.AGGR_SUM_UNSIGNED, abi.Uint32, True)
        want = expected(zones, batches, dims, None, abi.AGGR_SUM_UNSIGNED)
        mirror, _ = run_mirror(be, plan, batches)
        native, _, _ = XE.run(be, plan, batches, False)
        XE.assert_groups(XE.groups(plan, mirror), want, plan.agg)
        XE.assert_groups(XE.groups(plan, native), want, plan.agg)
    finally:
        zones.free()
