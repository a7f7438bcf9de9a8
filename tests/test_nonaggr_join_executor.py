"""Non-aggregation queries with joins through the C++ driver and the Python mirror (helpers of tests/test_nonaggr_executor.py):
HashLookup per foreign table over the survivors, foreign filters with the record-id vectors carried along, joined dimensions,
Expand for the batch with base counts, the rows cut to what is still wanted.  Expected rows come from the numpy model of
tests/select_join_model.py, bit for bit; the two hosts must issue the same ABI calls."""
import numpy as np
import pytest

import select_join_model as J
import select_model as M
import test_nonaggr_executor as E
from aresdb_amd import abi
from aresdb_amd.executor import Binary, Col, Const, DimensionSpec, ForeignTable, QueryPlan

FILTERS = M.MIXED_FILTERS
ONE = dict(ffilters=[(0, "region", abi.LessThan, 150)],
           dims=M.MIXED_DIMS[:3] + [((0, "region"), abi.Plus, 5, abi.Uint32)] + M.MIXED_DIMS[4:7] + [((0, "tz"), None, None, abi.Uint8)])
TWO = dict(ffilters=[(0, "region", abi.LessThan, 150), (1, "rate", abi.LessThan, 40.0)],
           dims=[("big", None, None, abi.Int64), ((0, "region"), None, None, abi.Uint32), ((1, "off"), abi.Plus, 1000, abi.Int32),
                 ("city", None, None, abi.Uint16), ((1, "tz"), abi.Plus, 1, abi.Uint8)])


class Tables:
    """the dimension tables of a query (the mode-0 batch without a default: the hosts pass none) and their device copies"""

    def __init__(self, be, count):
        self.be = be
        self.tables = [J.fixture(8, dtype, default=False, seed=seed)[0] for dtype, seed in [(abi.Uint32, 11), (abi.Uint16, 23)][:count]]
        self.device = [t.upload(be) for t in self.tables]

    def joins(self):
        return [("k%d" % k, t) for k, t in enumerate(self.tables)]

    def batch(self, n, seed, base_counts=None):
        cols = M.mixed_columns(max(n, 1), seed=seed)
        for k, t in enumerate(self.tables):
            cols["k%d" % k] = J.key_column(t, max(n, 1), seed + 100 * k)
        return E.B(n, seed, base_counts=base_counts, cols=cols)

    def plan(self, filters, ffilters, dims, limit, fused=False):
        def expr(name, f, c):
            col = Col(name) if isinstance(name, str) else Col(name[1], table=name[0] + 1)
            return col if f is None else Binary(f, col, Const(c))
        fts = [ForeignTable(join_column="k%d" % k, index=d.index_struct(), batches={n: [c.vp for c in cols] for n, cols in d.batches.items()},
                            data_types=dict(J.Table.TYPES), base_batch_id=J.BASE_BATCH, num_records_in_last_batch=t.num_last)
               for k, (t, d) in enumerate(zip(self.tables, self.device))]
        return QueryPlan(filters=[expr(n, f, c) for n, f, c in filters], foreign_filters=[expr((k, n), f, c) for k, n, f, c in ffilters],
                         dimensions=[DimensionSpec(expr(n, f, c), t) for n, f, c, t in dims], foreign_tables=fts,
                         measure=Const(1), agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32, use_hash_reduction=True,
                         use_fused_extension=fused, is_non_aggregation=True, limit=limit)

    def free(self):
        for d in self.device:
            d.free()


def expected(tables, batches, filters, ffilters, dims, limit, capacity_of=None):
    """test_nonaggr_executor.expected with the join model: (rows per dimension, rows contributed per batch)"""
    parts, written, per_batch = [], 0, []
    for i, b in enumerate(batches):
        if limit >= 0 and written >= limit and i > 0:
            per_batch.append(None)
            continue
        rows, out = J.model_join_select(b.cols, filters, tables.joins(), ffilters, dims, b.n)
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


def three(tables, seed=1):
    """three batches, the second with base counts (64 rows, 8 runs of two)"""
    lens = np.ones(64, np.int64)
    lens[3::8] = 2
    return [tables.batch(300, seed), tables.batch(64, seed + 1, base_counts=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)),
            tables.batch(1500, seed + 2)]


def both_hosts(be, tables, batches, filters, ffilters, dims, limit, **kw):
    want, per_batch = expected(tables, batches, filters, ffilters, dims, limit, kw.pop("capacity_of", None))
    plan = tables.plan(filters, ffilters, dims, limit)
    py = E.run(be, plan, batches, native=False, **kw)
    cpp = E.run(be, plan, batches, native=True, **kw)
    for got, calls, done, written, _ in (py, cpp):
        assert written == sum(n or 0 for n in per_batch)
        M.assert_rows_equal(got, want)
        for i, n in enumerate(per_batch):
            if n is None:
                assert calls[i] == 0, "a batch run on a done query issued ABI calls"
    assert py[1] == cpp[1], "the C++ driver and the Python mirror issued different ABI calls"
    return py, per_batch


@pytest.mark.parametrize("count,shape", [(1, ONE), (2, TWO)])
@pytest.mark.parametrize("limit", [-1, 0, 10, "across"])
def test_joined_columns_selected_and_filtered(be, count, shape, limit):
    tables = Tables(be, count)
    try:
        batches = three(tables)
        _, per = expected(tables, batches, FILTERS, shape["ffilters"], shape["dims"], -1)
        assert per[0] > 10 and per[1] > 0 and per[2] > 0
        if limit == "across":
            limit = per[0] + per[1] + per[2] // 2
        (_, calls, _, written, _), per_batch = both_hosts(be, tables, batches, FILTERS, shape["ffilters"], shape["dims"], limit)
        assert calls[0] > 0
        if limit < 0:
            assert per_batch == per
        elif limit in (0, 10):
            assert per_batch == [limit, None, None]
        else:
            assert written == limit and None not in per_batch
    finally:
        tables.free()


def test_a_join_without_a_foreign_filter(be):
    tables = Tables(be, 1)
    try:
        both_hosts(be, tables, three(tables, seed=5), FILTERS, [], ONE["dims"], -1)
    finally:
        tables.free()
