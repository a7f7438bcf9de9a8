"""The idea behind AresJoinColumnsRun, pinned on the oracle (no GPU, no new code): a joined value is a pure function of the
row's key, so a joined column can be resolved once per batch into an ordinary mode-2 column, and the query run as a join-free
one over it.

* The model of a resolved column, select_join_model.Table.joined(keys, key validity, name), is what HashLookup +
  UnaryTransform(Noop, ForeignColumnInput) leave in a dimension slot — for Uint32 / Uint8 / Float32 / Int16 columns over the
  model's three batch modes (bitmap, values only, mode 0 with and without a default), null keys, missing keys, a record in a
  batch outside the table and stale records of the last batch.
* A joined aggregation through the Python mirror equals its rewritten twin — the model's columns uploaded as mode-2 main-table
  columns, the foreign filters as main filters, no foreign tables: key -> value for HashReduce, row for row in order for
  Sort + Reduce, registers for HyperLogLog.  The foreign filters include one whose answer depends on how a null operand
  compares (NotEqual).  (The mirror hands the library no default for a foreign column: the mode-0 batch of these tables is
  without one; defaults are covered by the first check.)"""
import numpy as np
import pytest

import harness as H
import select_join_model as J
import select_model as M
import test_join_columns_executor as XE
import test_nonaggr_join_executor as X
from aresdb_amd import abi, smoke
from aresdb_amd.executor import BatchContext, BatchExecutor, Col, Unary, fetch_hll_results, fetch_results

ORDER = ["region", "rate", "off", "tz"]  # Uint32, Float32, Int16, Uint8 in vector order


@pytest.fixture(scope="module")
def oracle():
    return H.oracle_backend()


@pytest.mark.parametrize("default", [True, False], ids=["default", "no_default"])
@pytest.mark.parametrize("key_dtype", [abi.Uint32, abi.Int64])
def test_the_model_is_what_the_per_node_sequence_leaves_in_a_dimension_slot(oracle, key_dtype, default):
    n = 700
    t, key = J.fixture(n, key_dtype, default=default)
    outside = [k for k, rec in t.placed.items() if rec[0] - J.BASE_BATCH >= 3][0]
    key.values[5], key.valid[5] = np.frombuffer(outside, key.values.dtype)[0], True  # (the hand-placed record is met for sure)
    keys, key_valid = J.key_bytes_of(key, n, t.key_bytes), M._valid(key, n)
    # the fixture reaches every case of the rule
    recs = [t.placed.get(k) if v else None for k, v in zip(keys, key_valid)]
    assert not key_valid.all() and any(r is None and v for r, v in zip(recs, key_valid))          # null keys, missing keys
    assert any(r is not None and r[0] - J.BASE_BATCH >= 3 for r in recs)                            # a batch outside the table
    assert any(r is not None and r[0] - J.BASE_BATCH == 2 and r[1] >= t.num_last for r in recs)    # stale records
    assert {r[0] - J.BASE_BATCH for r in recs if r is not None} >= {0, 1, 2}                        # every batch mode
    dcols, dt = {"k0": key.upload(oracle)}, t.upload(oracle)
    try:
        dims = [((0, name), None, None, t.COLUMNS[name]) for name in ORDER]
        count, vec = J.per_node(oracle, dcols, [dt], [], [("k0", t)], [], dims, n)
        try:
            assert count == n
            for name, (values, ok) in zip(ORDER, M.read_dim_rows(oracle, vec, n)):
                col = t.joined(keys, key_valid, name)
                assert np.array_equal(ok.astype(bool), col.valid), name
                assert np.array_equal(values, col.values.view(np.uint8).reshape(n, -1)), name
                assert col.valid[[r is not None and r[0] - J.BASE_BATCH == 2 and r[1] < t.num_last for r in recs]].all() == default
        finally:
            vec.free()
    finally:
        dcols["k0"].free()
        dt.free()


# ---- a joined aggregation and its rewritten twin through the Python mirror ------------------------------------------------
def _twin_name(name):
    return name if isinstance(name, str) else "j%d_%s" % name


def twin_batches(tables, batches, names):
    """the batches with the model's joined columns `names` = [(join, column)] behind their own, as mode-2 columns"""
    out = []
    for b in batches:
        cols = dict(b.cols)
        for name in names:
            col = J._resolve(b.cols, tables.joins(), name, b.n)
            cols[_twin_name(name)] = M.Col(col.dtype, col.values, col.valid)
        out.append(X.E.B(b.n, 0, cols=cols))
    return out


def twin_shape(shape):
    dims, measure, agg, mtype, use_hash = shape
    return ([(_twin_name(n), f, c, t) for n, f, c, t in dims], None if measure is None else _twin_name(measure), agg, mtype, use_hash)


def run_mirror(be, plan, batches, hll=False):
    ctx = BatchContext(be, plan)
    ex = BatchExecutor(ctx)
    for i, b in enumerate(batches):
        dev = {k: c.upload(be) for k, c in b.cols.items()}
        ex.run({k: d.vp for k, d in dev.items()}, b.n, is_last_batch=hll and i == len(batches) - 1,
               owned_columns=[d.free for d in dev.values()])
    res = smoke._hll_groups(*fetch_hll_results(ctx)) if hll else fetch_results(ctx)
    ctx.release()
    return res


def _referenced(shape, ffilters):
    names = [d[0] for d in shape[0]] + [shape[1]] + [(k, n) for k, n, _, _ in ffilters]
    return sorted({n for n in names if isinstance(n, tuple)})


FFILTERS = {1: [(0, "region", abi.NotEqual, 7), (0, "off", abi.LessThanOrEqual, 400)],
            2: [(0, "region", abi.NotEqual, 7), (1, "rate", abi.LessThan, 40.0)]}


@pytest.mark.parametrize("count", [1, 2])
@pytest.mark.parametrize("name", ["sum_hash", "count_sort", "min_sort", "fsum_sort"])
def test_a_joined_aggregation_equals_its_rewritten_twin(oracle, name, count):
    tables = X.Tables(oracle, count)
    try:
        batches = [tables.batch(900, 41), tables.batch(1, 42), tables.batch(1300, 43)]
        shape, ffilters = XE.shapes(count)[name], FFILTERS[count]
        # the NotEqual filter meets null operands among the rows the main filters leave: its answer for them matters
        b = batches[0]
        main = np.ones(b.n, bool)
        for column, f, c in XE.FILTERS:
            main &= M.model_filter(b.cols[column], f, c, b.n)
        assert (main & ~M._valid(J._resolve(b.cols, tables.joins(), (0, "region"), b.n), b.n)).any()
        joined = run_mirror(oracle, XE.build(tables, shape, ffilters), batches)
        names = _referenced(shape, ffilters)
        twin_filters = XE.FILTERS + [(_twin_name((k, n)), f, c) for k, n, f, c in ffilters]
        plan = XE.plan_of(tables, twin_filters, [], twin_shape(shape)[0], XE.build(tables, twin_shape(shape), []).measure, shape[2],
                          shape[3], shape[4])
        plan.foreign_tables = []
        twin = run_mirror(oracle, plan, twin_batches(tables, batches, names))
        assert len(joined[1][0]) > 3
        if shape[4]:  # HashReduce: key -> value
            assert XE.groups(plan, joined) == XE.groups(plan, twin)
        else:         # Sort + Reduce: row for row, in order, bit for bit (one library, one order of additions)
            for a, b_ in zip(joined[0] + joined[1] + [joined[2]], twin[0] + twin[1] + [twin[2]]):
                assert np.array_equal(a, b_)
        XE.assert_groups(XE.groups(plan, twin), XE.expected(tables, batches, shape, ffilters), shape[2])
    finally:
        tables.free()


def test_a_joined_hyperloglog_query_equals_its_rewritten_twin(oracle):
    tables = X.Tables(oracle, 1)
    try:
        batches = [tables.batch(900, 51), tables.batch(1300, 52)]
        dims = [((0, "region"), None, None, abi.Uint32), ("city", abi.Floor, 100, abi.Uint32)]
        ffilters = FFILTERS[1]
        joined = run_mirror(oracle, XE.plan_of(tables, XE.FILTERS, ffilters, dims, Unary(abi.GetHLLValue, Col("off", table=1)), abi.AGGR_HLL,
                                               abi.Uint32, False), batches, hll=True)
        twin_filters = XE.FILTERS + [(_twin_name((k, n)), f, c) for k, n, f, c in ffilters]
        plan = XE.plan_of(tables, twin_filters, [], [(_twin_name(n), f, c, t) for n, f, c, t in dims],
                          Unary(abi.GetHLLValue, Col("j0_off")), abi.AGGR_HLL, abi.Uint32, False)
        plan.foreign_tables = []
        twin = run_mirror(oracle, plan, twin_batches(tables, batches, [(0, "region"), (0, "off")]), hll=True)
        assert len(joined) > 3 and joined == twin
    finally:
        tables.free()
