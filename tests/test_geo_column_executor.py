"""Geo intersection queries through the C++ driver with AresQuerySetGeoColumn: the geofence verdict of a batch without base
counts is resolved once, in row space (AresGeoShapeColumnRun), and the batch runs as a geo-free one over the rewritten plan.
Results must equal the setter-off run — key -> value for HashReduce, rows in order for Sort + Reduce, registers for HyperLogLog
— and the independent float64 point-in-polygon group-by of tests/test_executor.py.

The queries are the three of tests/test_executor.py::_geo_query (inside with the shape dimension, inside, outside) plus a
HashReduce SUM of an integer column, a float SUM through Sort + Reduce and a HyperLogLog.  Three batches: that test's two, the
second with base counts (it takes the original plan), and their concatenation.  On the oracle (CPU) the library has no such
entry point: the driver falls back silently."""
import os
import subprocess
import sys

import numpy as np
import pytest

import harness as H
import test_executor as E
import test_join_columns_executor as JX
from aresdb_amd import abi, smoke
from aresdb_amd.columns import DeviceColumn
from aresdb_amd.driver import NativeQuery
from aresdb_amd.executor import Col, Const, DimensionSpec, GeoIntersection, QueryPlan, Unary

FLT_MAX = float(np.finfo(np.float32).max)


class Batch:
    def __init__(self, cols, valid, base_counts=None):
        self.cols, self.valid, self.base_counts = cols, valid, base_counts
        self.n = len(cols["d1"][1])


def concat(a, b):
    cols = {k: (t, np.concatenate([v, b.cols[k][1]])) for k, (t, v) in a.cols.items()}
    valid = {}
    for k in a.cols:
        va, vb = a.valid[k], b.valid[k]
        valid[k] = None if va is None and vb is None else \
            np.concatenate([np.ones(a.n, bool) if va is None else va, np.ones(b.n, bool) if vb is None else vb])
    return Batch(cols, valid)


class Fixture:
    """_geo_query's plan, shapes and expected counts, over three batches: its two — the second with base counts, every run one
    row long — and their concatenation; `user` (HyperLogLog) is added to every batch.  Every row therefore occurs twice:
    the expected COUNT of a key is twice that test's."""

    def __init__(self, be, in_or_out, with_dim, seed=41):
        rng = np.random.default_rng(seed)
        self.plan, two, want, self.shapes = E._geo_query(be, rng, in_or_out, with_dim)
        self.in_or_out, self.with_dim = in_or_out, with_dim
        for cols, valid in two:
            n = len(cols["d1"][1])
            cols["user"] = (abi.Uint32, rng.integers(0, 3000, n).astype(np.uint32))
            valid["user"] = rng.random(n) >= 0.02
        a, b = Batch(*two[0]), Batch(*two[1])
        self.batches = [a, Batch(b.cols, b.valid, np.arange(b.n + 1, dtype=np.uint32)), concat(a, b)]
        self.want_counts = {k: 2 * v for k, v in want.items()}
        blob = self.shapes.buf.read(np.uint8)
        n = self.plan.geo.total_num_points
        self.lats, self.longs = blob[:4 * n].view(np.float32).astype(np.float64), blob[4 * n:8 * n].view(np.float32).astype(np.float64)
        self.sidx = blob[8 * n:9 * n].copy()

    def free(self):
        self.shapes.free()

    def with_plan(self, **kw):
        base = self.plan
        args = dict(filters=base.filters, dimensions=base.dimensions, measure=base.measure, agg=base.agg, measure_type=base.measure_type,
                    use_hash_reduction=base.use_hash_reduction, geo=base.geo)
        args.update(kw)
        return QueryPlan(**args)

    def first_shape(self, lat, lng):
        """even-odd rule in float64 over the uploaded polygon points (the test points sit off every edge): the first shape the
        point lies in, or None"""
        hit = {}
        for p in range(len(self.lats) - 1):
            if self.sidx[p] != self.sidx[p + 1] or self.lats[p] >= FLT_MAX or self.lats[p + 1] >= FLT_MAX:
                continue
            la1, lo1, la2, lo2 = self.lats[p], self.longs[p], self.lats[p + 1], self.longs[p + 1]
            if (lo1 > lng) != (lo2 > lng) and lat < (la2 - la1) * (lng - lo1) / (lo2 - lo1) + la1:
                hit[int(self.sidx[p])] = hit.get(int(self.sidx[p]), 0) ^ 1
        inside = sorted(s for s, c in hit.items() if c)
        return inside[0] if inside else None

    def group_by(self, measure, combine, identity, dims=("d3",)):
        """{key: aggregate} of the plan's filter, geo filter and dimensions (`dims` and, with_dim, the shape) over all batches"""
        out = {}
        for b in self.batches:
            d1, pt = b.cols["d1"][1], b.cols["pt"][1]
            ok = {k: (np.ones(b.n, bool) if v is None else v) for k, v in b.valid.items()}
            for i in range(b.n):
                if not (ok["d1"][i] and d1[i] < 90) or not ok["pt"][i]:  # (the shapes have a first edge: a null point never survives)
                    continue
                s = self.first_shape(float(pt[i, 0]), float(pt[i, 1]))
                if self.in_or_out != (s is not None):
                    continue
                key = [(np.uint32(b.cols[d][1][i]).tobytes(), int(ok[d][i])) for d in dims]  # (Noop keeps a null row's stored value)
                if self.with_dim:
                    key.append((bytes([s]), 1))
                v = identity if measure is None or not ok[measure][i] else b.cols[measure][1][i]
                out[tuple(key)] = combine(out.get(tuple(key), identity), 1 if measure is None else v)
        return out


def run(be, plan, batches, geo_column, hll=False):
    """(result, ABI calls per batch, fused batches): result = (dims, valids, measures) as fetched, or the HyperLogLog groups"""
    names = list(batches[0].cols.keys())
    q = NativeQuery(be, plan, names)
    if geo_column:
        q.set_geo_column(True)
    calls = []
    for i, b in enumerate(batches):
        dev = {k: DeviceColumn(be, t, v, valid=b.valid[k]) for k, (t, v) in b.cols.items()}
        bc = H.Buf(be, b.base_counts) if b.base_counts is not None else None
        before = q.calls
        q.run({k: d.vp for k, d in dev.items()}, b.n, base_counts=bc.ptr if bc else None, is_last_batch=hll and i == len(batches) - 1,
              owned_allocations=[d.ptr for d in dev.values()])
        calls.append(q.calls - before)
        if bc:
            bc.free()
    res = smoke._hll_groups(*q.fetch_hll()) if hll else q.fetch()
    fused = q.fused_batches
    q.release()
    return res, calls, fused


def eligible(batches):
    return [b.base_counts is None and b.n > 0 for b in batches]


def check_calls(be, calls_on, calls_off, batches, rewritten=True):
    """the product: an eligible batch issues AresGeoShapeColumnRun and one more filter in place of GeoBatchIntersects — one call
    more; everything else, and the oracle altogether: the same calls"""
    extra = [1 if e and rewritten and be.name == "hip" else 0 for e in eligible(batches)]
    assert calls_on == [c + x for c, x in zip(calls_off, extra)], (calls_on, calls_off)


QUERIES = [(True, True), (True, False), (False, False)]


@pytest.mark.parametrize("in_or_out,with_dim", QUERIES, ids=["in+dim", "in", "out"])
def test_the_three_geo_queries_equal_the_setter_off_run_and_the_independent_group_by(be, in_or_out, with_dim):
    fx = Fixture(be, in_or_out, with_dim)
    try:
        stats = be.geo_column_stats() if be.name == "hip" else None
        off, calls_off, _ = run(be, fx.plan, fx.batches, False)
        assert stats is None or be.geo_column_stats() == stats
        on, calls_on, _ = run(be, fx.plan, fx.batches, True)
        assert len(fx.want_counts) >= 2
        for res in (off, on):
            assert {k: int(v) for k, v in JX.groups(fx.plan, res).items()} == fx.want_counts
        assert fx.group_by(None, lambda a, v: a + v, 0) == fx.want_counts  # (this module's group-by is that test's)
        JX.assert_rows(on, off, fx.plan.agg)
        check_calls(be, calls_on, calls_off, fx.batches)
        if stats is not None:
            be.wait()
            after = be.geo_column_stats()
            rows = sum(b.n for b, e in zip(fx.batches, eligible(fx.batches)) if e)
            assert after["batches"] - stats["batches"] == 2 and after["declined"] == stats["declined"]
            assert after["rows"] - stats["rows"] == rows and 0 < after["live"] - stats["live"] < rows  # (the hint pruned)
    finally:
        fx.free()


def test_hash_reduce_sum_of_an_integer_column(be):
    fx = Fixture(be, True, True, seed=43)
    try:
        plan = fx.with_plan(measure=Col("d2"), agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32, use_hash_reduction=True)
        off, calls_off, _ = run(be, plan, fx.batches, False)
        on, calls_on, _ = run(be, plan, fx.batches, True)
        want = {k: int(v) for k, v in fx.group_by("d2", lambda a, v: a + int(v), 0).items()}
        assert len(want) >= 4
        for res in (off, on):
            assert {k: int(v) for k, v in JX.groups(plan, res).items()} == want
        check_calls(be, calls_on, calls_off, fx.batches)
    finally:
        fx.free()


def test_float_sum_through_sort_reduce(be):
    fx = Fixture(be, False, False, seed=44)
    try:
        plan = fx.with_plan(measure=Col("m"), agg=abi.AGGR_SUM_FLOAT, measure_type=abi.Float32)
        off, calls_off, _ = run(be, plan, fx.batches, False)
        on, calls_on, _ = run(be, plan, fx.batches, True)
        want = fx.group_by("m", lambda a, v: a + float(v), 0.0)
        assert len(want) >= 2
        JX.assert_groups(JX.groups(plan, off), want, plan.agg)
        JX.assert_groups(JX.groups(plan, on), want, plan.agg)
        JX.assert_rows(on, off, plan.agg)
        check_calls(be, calls_on, calls_off, fx.batches)
    finally:
        fx.free()


def test_hyperloglog_registers_are_equal(be):
    fx = Fixture(be, True, True, seed=45)
    try:
        plan = fx.with_plan(measure=Unary(abi.GetHLLValue, Col("user")), agg=abi.AGGR_HLL, measure_type=abi.Uint32)
        off, calls_off, _ = run(be, plan, fx.batches, False, hll=True)
        on, calls_on, _ = run(be, plan, fx.batches, True, hll=True)
        assert on == off and set(on) == set(fx.group_by(None, lambda a, v: a + v, 0)) and len(on) >= 4
        assert all(regs for regs in on.values()) and sum(len(regs) for regs in on.values()) > 20
        check_calls(be, calls_on, calls_off, fx.batches)
    finally:
        fx.free()


def test_ineligible_queries_are_untouched(be):
    """the shape dimension of the rows outside every shape, and a plan that also has a foreign table: the setter has no effect,
    the entry point is not asked"""
    stats = be.geo_column_stats() if be.name == "hip" else None
    fx = Fixture(be, False, False, seed=46)
    keep = []
    try:
        outside_dim = fx.with_plan(dimensions=[DimensionSpec(Col("d3"), abi.Uint32), DimensionSpec(Const(0), abi.Uint8)],
                                   geo=GeoIntersection(fx.plan.geo.shape_lat_longs, 3, fx.plan.geo.total_num_points, "pt", 0, False, 1))
        rng = np.random.default_rng(5)
        batches = [Batch(dict(b.cols), dict(b.valid), b.base_counts) for b in fx.batches]
        n_all = sum(b.n for b in batches)
        ft, fk, _ = E._join_fixture(be, rng, n_all, keep)
        at = 0
        for b in batches:
            b.cols["fk"], b.valid["fk"] = (abi.Uint32, fk[at:at + b.n]), None
            at += b.n
        joined = fx.with_plan(foreign_tables=[ft], dimensions=[DimensionSpec(Col("region", table=1), abi.Uint32)])
        for plan, bs in ((outside_dim, fx.batches), (joined, batches)):
            off, calls_off, _ = run(be, plan, bs, False)
            on, calls_on, _ = run(be, plan, bs, True)
            JX.assert_rows(on, off, plan.agg)
            assert calls_on == calls_off and len(off[1][0]) >= 2
        assert stats is None or be.geo_column_stats() == stats
    finally:
        fx.free()
        for b in keep:
            b.free()


# ---- the product ---------------------------------------------------------------------------------------------------------
def _launches(kernels, prefix):
    return sum(v[0] for k, v in kernels.items() if k.startswith(prefix))


GEO_PATH = ("geo_intersect_kernel", "geo_shape_dim_kernel")
FILTER_PATH = ("filter_kernel", "filter_pred_kernel", "filter_compact_kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("in_or_out,with_dim", QUERIES, ids=["in+dim", "in", "out"])
def test_kernels_of_the_eligible_batches(in_or_out, with_dim):
    """One geo_shape_column_kernel per eligible batch; no intersect kernel over the index vector, no shape-dimension scan, no
    generic, predicate or compaction filter kernel in those batches.  With the setter off the per-node geo sequence is there."""
    hip = H.hip_backend()
    fx = Fixture(hip, in_or_out, with_dim)
    try:
        batches = [b for b in fx.batches if b.base_counts is None]
        run(hip, fx.plan, batches, True)  # priming pass: whatever the shape compiles at run time is compiled
        hip.rtc_wait()
        on = JX._profile(hip, lambda: run(hip, fx.plan, batches, True))
        off = JX._profile(hip, lambda: run(hip, fx.plan, batches, False))
        print("on:", sorted(on), "off:", sorted(off))
        assert _launches(on, "geo_shape_column_kernel") == len(batches) and _launches(off, "geo_shape_column_kernel") == 0
        # (without the deferral machinery there are no row-space filters: a hot-shape filter is filter_pred_kernel + compaction)
        deferral = os.environ.get("ARES_FUSE", "1") != "0" and os.environ.get("ARES_DEFER", "1") != "0"
        for gone in GEO_PATH + (FILTER_PATH if deferral else FILTER_PATH[:1]):
            assert _launches(on, gone) == 0, (gone, sorted(on))
        assert _launches(off, "geo_intersect_kernel") == len(batches), sorted(off)
        assert _launches(off, "geo_shape_dim_kernel") == (len(batches) if with_dim else 0), sorted(off)
        # the index vector GeoBatchIntersects reads is materialised: the batch's row-space filter is replayed
        assert _launches(off, "filter_pred_kernel") > 0 and _launches(off, "filter_compact_kernel") > 0, sorted(off)
    finally:
        fx.free()


@pytest.mark.gpu
def test_with_the_fused_extension_an_eligible_batch_is_two_calls():
    """4-byte dimensions, no geo dimension: the rewritten plan is one the fused call takes; the plan with geo never is.  (The
    fused call holds the dimension and measure columns and ONE more: d1 is filter and dimension, the shape column the spare.)"""
    hip = H.hip_backend()
    fx = Fixture(hip, True, False, seed=47)
    try:
        plan = fx.with_plan(dimensions=[DimensionSpec(Col("d3"), abi.Uint32), DimensionSpec(Col("d1"), abi.Uint32)], measure=Col("m"),
                            agg=abi.AGGR_SUM_FLOAT, measure_type=abi.Float32, use_hash_reduction=True, use_fused_extension=True)
        off, calls_off, fused_off = run(hip, plan, fx.batches, False)
        on, calls_on, fused_on = run(hip, plan, fx.batches, True)
        want = fx.group_by("m", lambda a, v: a + float(v), 0.0, dims=("d3", "d1"))
        JX.assert_groups(JX.groups(plan, off), want, plan.agg)
        JX.assert_groups(JX.groups(plan, on), want, plan.agg)
        assert fused_off == 0 and fused_on == sum(eligible(fx.batches)) == 2
        assert [calls_on[i] for i in (0, 2)] == [2, 2] and calls_on[1] == calls_off[1]
    finally:
        fx.free()


@pytest.mark.gpu
def test_a_decline_sends_the_batch_down_the_original_plan_and_the_query_stops_asking():
    hip = H.hip_backend()
    fx = Fixture(hip, True, True, seed=48)
    try:
        batches = [fx.batches[0], fx.batches[2], fx.batches[1], fx.batches[0]]
        off, calls_off, _ = run(hip, fx.plan, batches, False)
        os.environ["ARES_GEO_COLUMN"] = "0"
        hip.reload_env()
        try:
            before = hip.geo_column_stats()
            on, calls_on, _ = run(hip, fx.plan, batches, True)
            after = hip.geo_column_stats()
        finally:
            del os.environ["ARES_GEO_COLUMN"]
            hip.reload_env()
        JX.assert_rows(on, off, fx.plan.agg)
        assert [a - b for a, b in zip(calls_on, calls_off)] == [1, 0, 0, 0]
        assert after["declined"] - before["declined"] == 1 and after["batches"] == before["batches"]
    finally:
        fx.free()


@pytest.mark.gpu
def test_the_books_balance_and_temporaries_do_not_pile_up():
    """the shape column is the query's (DeviceAllocate, released with the batch's input columns): after the query libmem's
    books are back at the start, and libalgorithm's stream temporaries do not grow batch over batch"""
    hip = H.hip_backend()
    fx = Fixture(hip, True, True, seed=49)
    try:
        run(hip, fx.plan, fx.batches, True)  # (staging buffers of the test's own uploads exist from here on)
        before = JX._mem_stats(hip)
        run(hip, fx.plan, fx.batches, True)
        assert JX._mem_stats(hip) == before
        b = fx.batches[0]
        q = NativeQuery(hip, fx.plan, list(b.cols.keys()))
        q.set_geo_column(True)
        handed = []
        for _ in range(5):
            dev = {k: DeviceColumn(hip, t, v, valid=b.valid[k]) for k, (t, v) in b.cols.items()}
            q.run({k: d.vp for k, d in dev.items()}, b.n, owned_allocations=[d.ptr for d in dev.values()])
            handed.append(JX._temp_handed_out(hip))
        q.release()
        assert handed[4] <= handed[1], handed
        assert JX._mem_stats(hip) == before
    finally:
        fx.free()


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["ARES_DEFER=0", "ARES_MEM_VERIFY_CLEAN=1"])
def test_results_do_not_depend_on_the_deferral_switches(switch):
    """both are read once per process: this module's tests on the product are re-run in a child process with each"""
    name, value = switch.split("=")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-k", "not deferral_switches", "-p", "no:cacheprovider", __file__],
                       cwd=H.ROOT, env={**os.environ, name: value}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (switch, r.stdout[-4000:], r.stderr[-1000:])
