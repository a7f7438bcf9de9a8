"""Parity of the HIP library against the oracle, through the C ABI, on a real MI355X.

Integer / byte / index outputs must be bit-identical.  Floating-point SUM/AVG reductions are
order-dependent (the reference's own DEVICE build is non-deterministic there);
they are compared with relative tolerance 1e-6 for float64 accumulators (the north-star bound)
and 1e-4 for float32 accumulators."""
import os

import numpy as np
import pytest

import cases
import harness as H
from aresdb_amd import abi

pytestmark = pytest.mark.gpu


def hip():
    return H.hip_backend()


@pytest.mark.parametrize("arity", [1, 2])
@pytest.mark.parametrize("as_filter", [False, True])
@pytest.mark.parametrize("block", range(6))
def test_transform_and_filter_small(arity, as_filter, block):
    o, h = H.oracle_backend(), hip()
    for seed in range(block * 30, block * 30 + 30):
        c = cases.TransformCase(seed * 4 + arity * 2 + int(as_filter), arity, as_filter)
        cases.assert_same(c.run(h), c.run(o), repr(c))


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("as_filter", [False, True])
def test_transform_and_filter_multi_tile(seed, as_filter):
    """Sizes spanning many tiles: exercises the chained scan and the grid-stride loops."""
    rows = [5000, 70001, 262144, 1000003][seed % 4]
    c = cases.TransformCase(9000 + seed, 2 if seed % 2 else 1, as_filter, rows=rows,
                            index_style="identity" if seed < 4 else "subset")
    cases.assert_same(c.run(hip()), c.run(H.oracle_backend()), repr(c))


FAST_ROWS = [1, 2, 3, 5, 63, 1000, 4095, 4096, 4099, 8191, 8192, 8197, 40000, 300001]


@pytest.mark.parametrize("as_filter", [False, True], ids=["transform", "filter"])
@pytest.mark.parametrize("seed", range(42))
def test_fast_path_shapes(seed, as_filter):
    """4-byte column x constant -> 4-byte vector / measure: the vectorised quad kernels, across
    tile boundaries, ragged ends, unaligned output offsets and sparse / permuted index vectors."""
    rows = FAST_ROWS[seed % len(FAST_ROWS)]
    style = ["identity", "subset", "perm"][(seed // 2) % 3]
    c = cases.fast_path_case(seed, as_filter, rows, style)
    cases.assert_same(c.run(hip()), c.run(H.oracle_backend()), repr(c))


@pytest.mark.parametrize("seed", range(24))
def test_hash_lookup(seed):
    c = cases.HashLookupCase(seed, n=(20000 if seed % 3 == 0 else None))
    cases.assert_same(c.run(hip()), c.run(H.oracle_backend()), f"HashLookupCase({seed})")


def _float_tolerance(c):
    """Tolerances of float aggregates (integer ones, keys, counts and MIN / MAX are bit-exact).
    * float64 sums — what the Go compiler emits for every SUM / AVG over floats (MeasureBytes = 8: query/aql_compiler.go:1198-1202,
      SURVEY.md 8a quirk 8) — hold north_star's 1e-6 relative.
    * float32 ACCUMULATORS (valueBytes = 4 with AGGR_SUM_FLOAT: accepted by the ABI, never produced by the Go host) are held to
      1e-4: a float32 sum is order-dependent in its own arithmetic — n additions carry a forward error of up to n x 2^-24 of the
      sum of magnitudes (Higham, Accuracy and Stability of Numerical Algorithms, ch. 4), 6e-3 for the 100 000-row runs of these
      cases — so the reference's own two builds (HOST: sequential in sorted order; DEVICE: thrust::reduce_by_key's tree /
      unordered atomics, query/sort_reduce.cu:135-160) differ from one another by more than 1e-6, and neither is "the" value.
      What is pinned bit-exactly for them is everything that does not depend on the order: groups, representatives, keys.
    * AVG packs {float32 average, uint32 count}: the count is exact, the rolling average (query/functor.hpp:1414-1436) is
      float32 arithmetic whose value depends on the order of merges: 1e-4 likewise."""
    vt = c.value_dtype()
    if vt == "avg":
        return 1e-4
    if vt == np.float64:
        return 1e-6
    if vt == np.float32:
        return 1e-4
    return None


def _values_close(c, a, b):
    vt = c.value_dtype()
    tol = _float_tolerance(c)
    if tol is None or c.agg in (abi.AGGR_MIN_FLOAT, abi.AGGR_MAX_FLOAT):
        return np.array_equal(a, b)
    if vt == "avg":
        ua, ub = a.view(np.uint32).reshape(-1, 2), b.view(np.uint32).reshape(-1, 2)
        if not np.array_equal(ua[:, 1], ub[:, 1]):
            return False
        fa, fb = ua[:, 0].copy().view(np.float32), ub[:, 0].copy().view(np.float32)
    else:
        fa, fb = a.view(vt), b.view(vt)
    return np.allclose(fa, fb, rtol=tol, atol=tol)


@pytest.mark.parametrize("seed", range(40))
def test_sort_reduce(seed):
    length = [None, None, 5000, 100000][seed % 4]
    c = cases.GroupByCase(seed, length=length)
    g, w = c.run_sort_reduce(hip()), c.run_sort_reduce(H.oracle_backend())
    assert np.array_equal(g["sorted_hash"], w["sorted_hash"])
    assert np.array_equal(g["sorted_index"], w["sorted_index"])  # stable sort: bit-exact order
    assert g["groups"] == w["groups"]
    assert np.array_equal(g["out_index"], w["out_index"])
    assert g["out_dims"] == w["out_dims"]
    assert _values_close(c, g["out_values"], w["out_values"]), f"GroupByCase({seed})"


@pytest.fixture(params=["lds", "global"])
def hash_path(request):
    """Both HashReduce implementations: the partitioned LDS path (default) and the global-table path
    (taken for AVG / float min-max, and as overflow fallback).  The library latches ARES_HASH_REDUCE;
    AresReloadEnv makes it read the variable again, and the kernel log proves which path ran."""
    be = hip()
    saved = os.environ.get("ARES_HASH_REDUCE")
    if request.param == "global":
        os.environ["ARES_HASH_REDUCE"] = "global"
    else:
        os.environ.pop("ARES_HASH_REDUCE", None)
    be.reload_env()
    be.profiler_enable(True)
    try:
        yield request.param
        be.call("WaitForCudaStream", None, 0)
        ran = set(k.split("<")[0] for k in be.profiler_report())
        partitioned = {k for k in ran if k.startswith("hr_")}
        if request.param == "global":
            assert "hash_insert_kernel" in ran and not partitioned, ran
        else:
            # (AVG and float min/max take the global table on both settings)
            assert partitioned or "hash_insert_kernel" in ran, ran
    finally:
        be.profiler_enable(False)
        if saved is None:
            os.environ.pop("ARES_HASH_REDUCE", None)
        else:
            os.environ["ARES_HASH_REDUCE"] = saved
        be.reload_env()


def _hash_reduce_same(c, what):
    g, w = c.run_hash_reduce(hip()), c.run_hash_reduce(H.oracle_backend())
    assert g["groups"] == w["groups"], what
    assert g["map"].keys() == w["map"].keys(), what
    keys = sorted(g["map"].keys())
    a = np.frombuffer(b"".join(g["map"][k] for k in keys), np.uint8)
    b = np.frombuffer(b"".join(w["map"][k] for k in keys), np.uint8)
    assert _values_close(c, a, b), what


@pytest.mark.parametrize("seed", range(12))
def test_hash_reduce_many_groups(seed, hash_path):
    """Enough rows and groups for several partitions, table flushes and multi-round merges: length
    up to 400k with a third of the rows distinct (the oracle's HOST-style map is O(groups) here)."""
    length = [30000, 70001, 150000, 400000][seed % 4]
    groups = [length // 3, length // 50, 7, length - 5][(seed // 4) % 4] if seed < 8 else length // 2
    aggs = [abi.AGGR_SUM_FLOAT, abi.AGGR_SUM_SIGNED, abi.AGGR_SUM_UNSIGNED]
    c = cases.GroupByCase(5000 + seed, length=length, groups=max(1, groups), agg=aggs[seed % 3],
                          ndw=[(0, 0, 4, 0, 0), (0, 1, 1, 1, 1), (1, 0, 0, 0, 2)][seed % 3],
                          value_bytes=[8, 4][seed % 2])
    _hash_reduce_same(c, f"GroupByCase({5000 + seed}) {hash_path}")


@pytest.mark.parametrize("seed", range(40))
def test_hash_reduce(seed, hash_path):
    length = [None, None, 5000, 100000][seed % 4]
    aggs = [abi.AGGR_SUM_UNSIGNED, abi.AGGR_SUM_SIGNED, abi.AGGR_SUM_FLOAT, abi.AGGR_AVG_FLOAT]
    c = cases.GroupByCase(1000 + seed, length=length, agg=aggs[seed % 4])
    g, w = c.run_hash_reduce(hip()), c.run_hash_reduce(H.oracle_backend())
    assert g["groups"] == w["groups"]
    assert g["map"].keys() == w["map"].keys()
    keys = sorted(g["map"].keys())
    a = np.frombuffer(b"".join(g["map"][k] for k in keys), np.uint8)
    b = np.frombuffer(b"".join(w["map"][k] for k in keys), np.uint8)
    assert _values_close(c, a, b), f"GroupByCase({1000 + seed}) hash"


@pytest.mark.parametrize("agg,np_op", [(abi.AGGR_MIN_UNSIGNED, np.minimum), (abi.AGGR_MAX_SIGNED, np.maximum),
                                       (abi.AGGR_MIN_FLOAT, np.minimum), (abi.AGGR_MAX_FLOAT, np.maximum)])
def test_hash_reduce_min_max_against_numpy(agg, np_op):
    """The reference's HOST map starts MIN/MAX groups from 0; the device
    semantics (cudf: start from the identity) are what the HIP library implements."""
    c = cases.GroupByCase(4242, length=20000, agg=agg, ndw=(0, 0, 1, 0, 0))
    g = c.run_hash_reduce(hip())
    vt = c.value_dtype()
    vals = c.values.view(vt)
    keys = {}
    din = H.DimVector(H.oracle_backend(), c.capacity, c.ndw, with_hash=False, with_index=False, init=c.blob)
    rows = din.rows(c.length)
    for r, v in zip(rows, vals):
        keys[r] = v if r not in keys else np_op(keys[r], v)
    assert g["groups"] == len(keys)
    got = {k: np.frombuffer(v, vt)[0] for k, v in g["map"].items()}
    assert got == keys


def test_filter_large_property():
    """16M rows, 1% nulls: survivors == numpy, order preserved, count exact."""
    be = hip()
    n = 1 << 24
    rng = np.random.default_rng(1)
    vals = rng.integers(0, 1000, n).astype(np.uint32)
    valid = rng.random(n) > 0.01
    col = H.Column(be, abi.Uint32, vals, valid=valid, alignment=64)
    idx = H.Buf(be, nbytes=4 * n)
    pred = H.Buf(be, nbytes=n)
    be.call("InitIndexVector", idx.ptr, 0, n, None, 0)
    cnt = be.call("BinaryFilter", col.input(), H.const_int(500), idx.ptr, pred.ptr, n, None, 0, None, 0,
                  abi.LessThan, None, 0)
    want = np.nonzero((vals < 500) & valid)[0].astype(np.uint32)
    assert cnt == len(want)
    assert np.array_equal(idx.read(np.uint32, cnt), want)
    assert np.array_equal(pred.read(np.uint8, n), ((vals < 500) & valid).astype(np.uint8))
    for b in (col, idx, pred):
        b.free()


def _colliding_segments(h):
    """(short, long): runs of equal top halves of the sorted hashes that hold more than one distinct hash, up to 64 entries
    long / longer — what Sort's fix-up after the four top-half passes has to put in order (sort_reduce.hip)"""
    top = h >> np.uint64(32)
    bounds = np.concatenate([[0], np.nonzero(top[1:] != top[:-1])[0] + 1, [len(h)]])
    short = long_ = 0
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b - a > 1 and h[a] != h[b - 1]:
            if b - a > 64:
                long_ += 1
            else:
                short += 1
    return short, long_


@pytest.mark.parametrize("length,groups,want_long", [(1 << 22, 50000, False), (1 << 23, 200000, True), (1 << 22, 3000000, False)],
                         ids=["50k_groups", "200k_groups_long_segments", "3M_groups_short_segments"])
def test_sort_large_property(length, groups, want_long):
    """Millions of rows: output is sorted by hash, is a permutation, and equal hashes keep input order — with hashes that
    share their top half in short runs (one thread's insertion sort) and in long ones (two groups of dozens of rows each:
    ranked in LDS)."""
    be = hip()
    c = cases.GroupByCase(77, length=length, groups=groups, ndw=(0, 0, 2, 0, 0), agg=abi.AGGR_SUM_UNSIGNED,
                          value_bytes=4, capacity_slack=0)
    r = c.run_sort_reduce(be)
    h, ix = r["sorted_hash"], r["sorted_index"]
    short, long_ = _colliding_segments(h)
    if want_long:
        assert long_ >= 1, "the test data holds no long run of equal top halves any more"
    elif groups > 1000000:
        assert short >= 10
    assert np.all(h[1:] >= h[:-1])
    assert np.array_equal(np.sort(ix), np.arange(c.length, dtype=np.uint32))
    same = h[1:] == h[:-1]
    assert np.all(ix[1:][same] > ix[:-1][same])
    vals = c.values.view(np.uint32)
    starts = np.concatenate([[0], np.nonzero(~same)[0] + 1])
    sums = np.add.reduceat(vals[ix].astype(np.uint64), starts).astype(np.uint32)
    assert r["groups"] == len(starts)
    assert np.array_equal(r["out_values"].view(np.uint32), sums)
    assert np.array_equal(r["out_index"], ix[starts])


@pytest.mark.parametrize("seed", range(30))
def test_hyperloglog(seed):
    """Every observable buffer of every batch (sorted keys, values, rows, dimension rows, encoded
    registers) is bit-identical: the sort and the merge are stable."""
    c = cases.HllCase(seed)
    cases.assert_same(c.run(hip()), c.run(H.oracle_backend()), repr(c))


@pytest.mark.parametrize("seed,batches,rows,groups,registers", [
    (700, 3, 30000, 40, 1 << 14),     # dense and sparse dimensions, several merge tiles
    (701, 4, 250000, 3000, 1 << 14),  # many dimensions, multi-tile head scans
    (702, 2, 300000, 1, 7),           # one dimension, a handful of registers: very long runs
    (703, 3, 100000, 200000, 50),     # nearly every entry its own dimension
    (704, 5, 0, 5, 100),              # only empty batches
])
def test_hyperloglog_multi_tile(seed, batches, rows, groups, registers):
    c = cases.HllCase(seed, batches=batches, batch_rows=rows, groups=groups, registers=registers)
    cases.assert_same(c.run(hip()), c.run(H.oracle_backend()), repr(c))


def test_hyperloglog_estimate_property():
    """4M rows in 2 batches, 3 dimensions with known distinct counts: the registers decode to the
    HyperLogLog estimate (p = 14: standard error 0.8 %) of each dimension's distinct count."""
    cases.hll_estimate_check(hip(), 1 << 21, [2000, 150000, 1200000])


@pytest.mark.parametrize("seed", range(40))
def test_geo_intersects(seed):
    """Predicate words, compacted index / RecordID vectors and the shape dimension are bit-identical
    (same float operations in the same order as the reference: no contraction, IEEE division)."""
    c = cases.GeoCase(seed)
    cases.assert_same(c.run(hip()), c.run(H.oracle_backend()), repr(c))


@pytest.mark.parametrize("seed,rows,shapes,foreign,max_ring", [
    (900, 150000, 200, False, None), (901, 100000, 33, True, None), (902, 300000, 1, False, None), (903, 70000, 70, False, None),
    # rings of up to 150 vertices (three 64-edge chunks) and 256 shapes (all eight predicate words)
    (904, 6000, 256, False, 150), (905, 5000, 256, True, 150), (906, 20000, 3, False, 150), (907, 9000, 70, True, 150)],
    ids=["900-150000-200-False", "901-100000-33-True", "902-300000-1-False", "903-70000-70-False",
         "904-long-rings-256", "905-long-rings-256-joined", "906-long-rings-3", "907-long-rings-70-joined"])
def test_geo_intersects_multi_tile(seed, rows, shapes, foreign, max_ring):
    c = cases.GeoCase(seed, rows=rows, shapes=shapes, foreign_points=foreign, max_ring=max_ring)
    cases.assert_same(c.run(hip()), c.run(H.oracle_backend()), repr(c))


def _dim_out(values_ptr, nulls_ptr):
    return H.dimension_output(values_ptr, nulls_ptr, abi.Uint32)


@pytest.mark.parametrize("be_name", ["hip"])
def test_deferred_transforms_respect_dependencies(be_name):
    """Cross-call fusion (include/ares_extensions.h) holds root transforms back; a transform that
    READS what a queued one WRITES, or overwrites what a queued one reads/writes, must still see
    program order.  Chain: X = a + 1;  Y = X * 3 (reads X);  X = a + 5 (overwrites X);  Z = X - 1."""
    be = H.get_backend(be_name)
    n = 100003
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1000, n).astype(np.uint32)
    col = H.Column(be, abi.Uint32, a)
    idx = H.Buf(be, np.arange(n, dtype=np.uint32))
    bufs = {k: (H.Buf(be, nbytes=4 * n + 16), H.Buf(be, nbytes=n + 16)) for k in "XYZ"}
    from aresdb_amd.columns import slice_from_pointer
    from aresdb_amd.executor import column_input, constant_input

    def call(src, const, functor, dst):
        be.call("BinaryTransform", src, constant_input(const), _dim_out(bufs[dst][0].ptr, bufs[dst][1].ptr), idx.ptr, n,
                None, 0, functor, None, 0)
    x_as_column = column_input(slice_from_pointer(bufs["X"][0].ptr, abi.Uint32, n))
    call(col.input(), 1, abi.Plus, "X")
    call(x_as_column, 3, abi.Multiply, "Y")
    call(col.input(), 5, abi.Plus, "X")
    call(x_as_column, 1, abi.Minus, "Z")
    got = {k: bufs[k][0].read(np.uint32, n) for k in "XYZ"}
    assert np.array_equal(got["Y"], (a + 1) * 3)
    assert np.array_equal(got["X"], a + 5)
    assert np.array_equal(got["Z"], a + 4)
    for k in "XYZ":
        assert bufs[k][1].read(np.uint8, n).all()
    for b in [col, idx] + [x for pair in bufs.values() for x in pair]:
        b.free()
