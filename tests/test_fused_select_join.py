"""AresFusedFilterJoinSelect (include/ares_extensions.h): the select scan with the cuckoo probe inside, against the numpy model
of tests/select_join_model.py and, for the same batch, against the per-node ABI sequence on the same library — bit for bit.
Shapes as in tests/test_fused_select.py (tile edges, ragged quads, limits at tile boundaries, ticket rounds, the early out),
plus what the join adds: every key type and index geometry, the stash, a second candidate of a bucket, stale and missing
records, mode-0 batches with and without a default, two joins, and the two places the probe happens."""
import numpy as np
import pytest

import harness as H
import select_join_model as J
import select_model as M
import select_runs as R
import test_fused_select as F
from aresdb_amd import abi

pytestmark = pytest.mark.gpu
TILE = 4096
FFILTER = [(0, "region", abi.LessThan, 150)]
# the mixed plan (every slot width) with two joined dimensions: a 4-byte one with Plus and a bare Uint8
DIMS = M.MIXED_DIMS[:3] + [((0, "region"), abi.Plus, 5, abi.Uint32)] + M.MIXED_DIMS[4:7] + [((0, "tz"), None, None, abi.Uint8)]


@pytest.fixture(scope="module")
def hip():
    return H.hip_backend()


class Batch:
    """columns and tables of one batch on the device, uploaded once per module; joins[k] = (key column, Table)"""

    def __init__(self, be, cols, joins):
        self.be, self.cols, self.joins = be, cols, joins
        self.dcols = {k: c.upload(be) for k, c in cols.items()}
        self.dtables = [t.upload(be) for _, t in joins]

    def query(self, filters, ffilters, dims, joins=None, **kw):
        joins = self.joins if joins is None else joins
        return J.fused_query(self.dcols, self.dtables[:max(len(joins), 1)], filters, joins, ffilters, dims, **kw)

    def free(self):
        for c in list(self.dcols.values()) + self.dtables:
            c.free()


def make_batch(be, n, key_dtype=abi.Uint32, seed=7, second=None, **kw):
    t, key = J.fixture(n, key_dtype, **kw)
    cols = M.mixed_columns(n, seed=seed)
    cols["k0"] = key
    joins = [("k0", t)]
    if second is not None:
        t1, cols["k1"] = J.fixture(n, second, seed=23)
        joins.append(("k1", t1))
    return Batch(be, cols, joins)


def check(b, filters, ffilters, dims, n, limit=-1, capacity=None, per_node=True, joins=None):
    """fused == model, rows at and beyond res untouched, fused == per-node sequence on the same library; (res, bytes)"""
    be = b.be
    joins = b.joins if joins is None else joins
    rows, want = J.model_join_select(b.cols, filters, joins, ffilters, dims, n, limit)
    capacity = capacity if capacity is not None else max(n, 1) + 3
    res, vec = J.fused(be, b.query(filters, ffilters, dims, joins), dims, n, limit, capacity)
    try:
        assert res == len(rows)
        got = M.read_dim_rows(be, vec, res)
        M.assert_rows_equal(got, want, "fused against the model")
        blob = vec.values.read(np.uint8)
        F._sentinel_intact(vec, blob, res)
    finally:
        vec.free()
    if per_node:
        count, pv = J.per_node(be, b.dcols, b.dtables, filters, joins, ffilters, dims, n)
        try:
            assert res == (count if limit < 0 else min(count, limit))
            M.assert_rows_equal(got, M.read_dim_rows(be, pv, res), "fused against the per-node sequence")
        finally:
            pv.free()
    return res, blob


@pytest.fixture(scope="module")
def mixed(hip):
    b = make_batch(hip, 3 * TILE + 5, second=abi.Uint16)
    yield b
    b.free()


@pytest.mark.parametrize("n", [1, 3, 4095, 4096, 4097, 3 * TILE + 5])
def test_batch_sizes_around_the_tile(mixed, n):
    res, _ = check(mixed, M.MIXED_FILTERS, FFILTER, DIMS, n, joins=mixed.joins[:1])
    assert res > 0 or n < 4


@pytest.mark.parametrize("key_dtype", [abi.Uint32, abi.Int32, abi.Uint16, abi.Uint8, abi.Int64, abi.UUID])
def test_every_key_type(hip, key_dtype):
    n = TILE + 9
    b = make_batch(hip, n, key_dtype)
    try:
        assert (b.joins[0][1].stash_signatures() != 0).any() or key_dtype == abi.Uint8
        check(b, M.MIXED_FILTERS[:1], [(0, "off", abi.GreaterThan, -300)], DIMS, n)
    finally:
        b.free()


@pytest.mark.parametrize("geometry", [dict(num_buckets=1, nkeys=11), dict(num_hashes=2), dict(default=False)])
def test_index_geometries_and_a_table_without_default(hip, geometry):
    n = TILE + 9
    b = make_batch(hip, n, **geometry)
    try:
        check(b, M.MIXED_FILTERS[:1], [], DIMS, n)
        check(b, [], FFILTER, DIMS, n, limit=TILE)
    finally:
        b.free()


def test_joined_expressions_into_every_slot_width(mixed):
    dims = [((0, "region"), abi.Plus, 5, abi.Uint32), ((0, "rate"), abi.Multiply, 2.0, abi.Float32), ((0, "off"), None, None, abi.Int32),
            ((0, "region"), abi.Floor, 7, abi.Uint32), ((0, "rate"), abi.Plus, 1, abi.Float32), ((0, "off"), abi.Multiply, 3, abi.Int16),
            ((0, "region"), None, None, abi.Uint16), ((0, "tz"), abi.Plus, 1, abi.Uint8)]
    check(mixed, M.MIXED_FILTERS, [(0, "rate", abi.GreaterThan, 5.0), (0, "off", abi.LessThanOrEqual, 400)], dims, TILE + 301,
          joins=mixed.joins[:1])


def test_two_joins(mixed):
    """a filter on one join and dimensions from both; then join 1 read by dimensions only (probed after the look-back)"""
    n = 2 * TILE + 77
    dims = [((0, "region"), None, None, abi.Uint32), ((1, "off"), abi.Plus, 1000, abi.Int32), ("city", None, None, abi.Uint16),
            ((1, "tz"), abi.Plus, 1, abi.Uint8)]
    check(mixed, M.MIXED_FILTERS, FFILTER, dims, n)
    check(mixed, M.MIXED_FILTERS, FFILTER + [(1, "rate", abi.LessThan, 40.0)], dims, n, limit=TILE)
    before = mixed.be.select_join_stats()
    res, _ = check(mixed, M.MIXED_FILTERS, FFILTER, dims[1:], n, limit=7, per_node=False)
    after = mixed.be.select_join_stats()
    survivors_of_main = len(M.model_select(mixed.cols, M.MIXED_FILTERS, M.MIXED_DIMS, n)[0])
    assert res == 7 and 7 <= after["probed"] - before["probed"] <= survivors_of_main + 7


def test_limits_at_the_tile_boundaries(mixed):
    """the survivors of tile 0 depend on the join"""
    n = 2 * TILE + 100
    joins = mixed.joins[:1]
    rows, _ = J.model_join_select(mixed.cols, M.MIXED_FILTERS, joins, FFILTER, DIMS, n)
    main_only = len(M.model_select(mixed.cols, M.MIXED_FILTERS, M.MIXED_DIMS, n)[0])
    total, in_tile0 = len(rows), int((rows < TILE).sum())
    assert 0 < in_tile0 < total < main_only
    for limit in [0, 1, in_tile0, in_tile0 + 1, total - 1, total, total + 1, -1]:
        res, _ = check(mixed, M.MIXED_FILTERS, FFILTER, DIMS, n, limit=limit, per_node=limit in (in_tile0, -1), joins=joins)
        assert res == (total if limit < 0 else min(total, limit))


def test_a_foreign_filter_that_no_row_passes(mixed):
    res, _ = check(mixed, [], [(0, "region", abi.GreaterThan, 10 ** 6)], DIMS, 2 * TILE + 3, joins=mixed.joins[:1])
    assert res == 0


def test_every_key_missing(hip):
    n = TILE + 9
    b = make_batch(hip, n, misses=1.1, pair=False)
    try:
        res, blob = check(b, M.MIXED_FILTERS, [], DIMS, n)
        rows, want = J.model_join_select(b.cols, M.MIXED_FILTERS, b.joins, [], DIMS, n)
        assert res == len(rows) > 0 and not want[3][1].any() and not want[7][1].any()  # rows emitted, joined dimensions null
    finally:
        b.free()


def test_a_run_length_filter_column_with_a_join(hip):
    """tile 1 lies inside one run that fails the comparison: rejected, counted, and the join's tiles around it are right"""
    n = 3 * TILE + 5
    t, key = J.fixture(n)
    pairs = dict(M.mixed_columns(n))
    pairs["k0"] = key
    rng = np.random.default_rng(5)
    lens = np.concatenate([R.run_lengths(rng, TILE - 10, 40), [TILE + 20], R.run_lengths(rng, n - 2 * TILE - 10, 40)])
    values = R.values_of(rng, abi.Uint16, len(lens))
    values[np.flatnonzero(lens == TILE + 20)[0]] = 499
    pairs["city"] = R.run_col(abi.Uint16, values, np.ones(len(lens), bool), lens, starting_index=1)
    up, twin = R.split(pairs)
    b = Batch(hip, twin, [("k0", t)])
    for c in b.dcols.values():
        c.free()
    b.dcols = {k: c.upload(hip) for k, c in up.items()}
    try:
        r0, s0 = hip.select_run_stats(), hip.select_join_stats()
        res, _ = check(b, [("city", abi.LessThan, 499)], FFILTER, DIMS, n)
        r1, s1 = hip.select_run_stats(), hip.select_join_stats()
        assert res > 0 and r1["rejected"] - r0["rejected"] == 1 and s1["tiles"] - s0["tiles"] == 4
    finally:
        b.free()


@pytest.fixture(scope="module")
def twenty(hip):
    b = make_batch(hip, 20 * TILE - 7, seed=5, second=abi.Uint16)
    yield b
    b.free()


def test_ten_ticket_rounds_equal_the_default_grid(twenty):
    n = 20 * TILE - 7
    joins = twenty.joins[:1]
    _, default = check(twenty, M.MIXED_FILTERS, FFILTER, DIMS, n, joins=joins)
    with F._Env(twenty.be, ARES_SELECT_GRID="2"):
        before = twenty.be.select_join_stats()
        _, two = check(twenty, M.MIXED_FILTERS, FFILTER, DIMS, n, per_node=False, joins=joins)
        after = twenty.be.select_join_stats()
    assert np.array_equal(default, two)
    assert after["tiles"] - before["tiles"] == 20 and after["batches"] - before["batches"] == 1


@pytest.mark.parametrize("num_joins", [1, 2])
def test_early_out_with_joins_read_by_dimensions_only(twenty, num_joins):
    """Every row passes the main filter, ten are wanted, two workgroups: at most two tiles are read and exactly ten keys per
    join are probed — conditions of the design, not measurements; the per-node sequence probes all 81 913 rows."""
    n = 20 * TILE - 7
    dims = [((0, "region"), abi.Plus, 5, abi.Uint32), ("city", None, None, abi.Uint16), ((num_joins - 1, "tz"), None, None, abi.Uint8)]
    with F._Env(twenty.be, ARES_SELECT_GRID="2"):
        before = twenty.be.select_join_stats()
        res, _ = check(twenty, [("amount", abi.GreaterThan, -2000000)], [], dims, n, limit=10, per_node=False, joins=twenty.joins[:num_joins])
        after = twenty.be.select_join_stats()
    assert res == 10
    assert after["tiles"] - before["tiles"] <= 2
    assert after["probed"] - before["probed"] == 10 * num_joins
    assert after["rows"] - before["rows"] == 10


def test_early_out_with_a_foreign_filter(twenty):
    n = 20 * TILE - 7
    with F._Env(twenty.be, ARES_SELECT_GRID="2"):
        before = twenty.be.select_join_stats()
        res, _ = check(twenty, [("amount", abi.GreaterThan, -2000000)], FFILTER, DIMS, n, limit=10, per_node=False, joins=twenty.joins[:1])
        after = twenty.be.select_join_stats()
    assert res == 10
    assert after["tiles"] - before["tiles"] <= 2
    assert after["probed"] - before["probed"] <= 2 * TILE


def _declined(be, q, dims, n=100):
    be.wait()
    be.profiler_enable(True)
    try:
        with pytest.raises(abi.AresError, match="^not fusable"):
            J.fused(be, q, dims, n, -1, n)
        be.wait()
        assert be.profiler_report() == {}, "a declined shape launched a kernel"
    finally:
        be.profiler_enable(False)


def test_declined_shapes_launch_nothing(hip):
    n = 100
    b = make_batch(hip, n, second=abi.Uint16)
    rng = np.random.default_rng(3)
    extra = {"absent": M.Col(abi.Uint32, None, default=5).upload(hip),
             "rl": R.run_col(abi.Uint32, rng.integers(0, 9, 10), np.ones(10, bool), np.full(10, 10))[0].upload(hip)}
    b.dcols.update(extra)
    t = b.joins[0][1]
    dims = [((0, "region"), None, None, abi.Uint32)]
    one = b.joins[:1]
    try:
        before = hip.select_join_stats()
        _declined(hip, b.query([], [], dims, [("rl", t)]), dims)      # a mode-3 key
        _declined(hip, b.query([], [], dims, [("absent", t)]), dims)  # a mode-0 key
        for dtype in (abi.Bool, abi.UUID):                             # a Bool and a wide joined column
            q = b.query([], [], dims, one)
            q.dims[0].lhs.Vector.ForeignVP.DataType = dtype
            _declined(hip, q, dims)
            q = b.query([], FFILTER, dims, one)
            q.foreignFilters[0].lhs.Vector.ForeignVP.DataType = dtype
            _declined(hip, q, dims)
        tz = H.Buf(hip, np.zeros(16, np.int16))
        q = b.query([], [], dims, one)
        q.dims[0].lhs.Vector.ForeignVP.TimezoneLookup, q.dims[0].lhs.Vector.ForeignVP.TimezoneLookupSize = tz.ptr, 16
        _declined(hip, q, dims)                                        # a non-null timezone table
        _declined(hip, b.query([], [], [("ts", None, None, abi.Uint32)], one, num_joins=0), dims)
        _declined(hip, b.query([], [], dims, one, num_joins=3), dims)
        _declined(hip, b.query([], [], [((1, "region"), None, None, abi.Uint32)], one), dims)  # join index out of range
        _declined(hip, b.query([], [(2, "region", abi.LessThan, 5)], dims), dims)
        with F._Env(hip, ARES_SELECT="0"):
            _declined(hip, b.query(M.MIXED_FILTERS, FFILTER, dims, one), dims)
        tz.free()
        after = hip.select_join_stats()
        assert after["declined"] - before["declined"] == 12 and after["batches"] == before["batches"]
        res, _ = check(b, M.MIXED_FILTERS, FFILTER, dims, n, joins=one)  # the same plan once the switch is back
        assert res > 0
    finally:
        b.free()


def test_too_small_a_capacity_is_an_error_not_a_decline(mixed):
    q = mixed.query(M.MIXED_FILTERS, FFILTER, DIMS, mixed.joins[:1])
    for limit, capacity in [(-1, 99), (50, 49)]:
        with pytest.raises(abi.AresError) as e:
            J.fused(mixed.be, q, DIMS, 100, limit, capacity)
        assert "VectorCapacity" in str(e.value) and "not fusable" not in str(e.value)


def test_zero_rows_and_zero_limit_launch_nothing(mixed):
    be = mixed.be
    q = mixed.query(M.MIXED_FILTERS, FFILTER, DIMS, mixed.joins[:1])
    be.wait()
    be.profiler_enable(True)
    try:
        for n, limit in [(0, -1), (100, 0)]:
            res, vec = J.fused(be, q, DIMS, n, limit, 8)
            assert res == 0
            F._sentinel_intact(vec, vec.values.read(np.uint8), 0)
            vec.free()
        be.wait()
        assert be.profiler_report() == {}
    finally:
        be.profiler_enable(False)


# ---- the C++ driver with useFusedExtension (helpers of tests/test_nonaggr_join_executor.py) ------------------------------
@pytest.mark.parametrize("count", [1, 2])
def test_driver_takes_the_eligible_batches(hip, count):
    """Batches without base counts take ONE call — AresFusedFilterJoinSelect, no record-id vectors — and the batch with base
    counts the ordinary sequence; the rows are the model's and the unfused run's."""
    import test_nonaggr_executor as E
    import test_nonaggr_join_executor as X
    tables = X.Tables(hip, count)
    shape = X.ONE if count == 1 else X.TWO
    try:
        batches = X.three(tables)
        for limit in (-1, 15):
            want, per_batch = X.expected(tables, batches, X.FILTERS, shape["ffilters"], shape["dims"], limit)
            before = hip.select_join_stats()
            plain = E.run(hip, tables.plan(X.FILTERS, shape["ffilters"], shape["dims"], limit), batches, native=True)
            assert hip.select_join_stats() == before
            fused = E.run(hip, tables.plan(X.FILTERS, shape["ffilters"], shape["dims"], limit, fused=True), batches, native=True)
            M.assert_rows_equal(plain[0], want)
            M.assert_rows_equal(fused[0], want)
            eligible = [i for i, (b, n) in enumerate(zip(batches, per_batch)) if n is not None and b.base_counts is None]
            assert plain[4] == 0 and fused[4] == len(eligible) and fused[2] == plain[2] and fused[3] == plain[3]
            assert hip.select_join_stats()["batches"] - before["batches"] == len(eligible)
            for i, n in enumerate(per_batch):
                if i in eligible:
                    assert fused[1][i] == 1 < plain[1][i]
                else:
                    assert fused[1][i] == plain[1][i]  # base counts (or a done query): the ordinary sequence
    finally:
        tables.free()


def test_driver_stops_asking_after_a_decline(hip):
    """a UUID joined column: the first batch pays one extra ABI call, the later ones none; the rows are the ordinary sequence's"""
    import test_nonaggr_executor as E
    import test_nonaggr_join_executor as X
    tables = X.Tables(hip, 1)
    dims = [((0, "uid"), None, None, abi.UUID), ((0, "region"), None, None, abi.Uint32), ("city", None, None, abi.Uint16)]
    try:
        batches = [tables.batch(300, 50), tables.batch(400, 51), tables.batch(200, 52)]
        before = hip.select_join_stats()
        plain = E.run(hip, tables.plan(X.FILTERS, X.ONE["ffilters"], dims, -1), batches, native=True)
        fused = E.run(hip, tables.plan(X.FILTERS, X.ONE["ffilters"], dims, -1, fused=True), batches, native=True)
        after = hip.select_join_stats()
        M.assert_rows_equal(fused[0], plain[0])
        assert plain[3] > 50 and fused[4] == 0
        assert [f - p for f, p in zip(fused[1], plain[1])] == [1, 0, 0]
        assert after["declined"] - before["declined"] == 1 and after["batches"] == before["batches"]
    finally:
        tables.free()


def test_a_join_free_plan_still_goes_through_the_join_free_entry_point(hip):
    import test_nonaggr_executor as E
    batches = [E.B(5000, 40), E.B(300, 42)]
    s0, j0 = hip.select_stats(), hip.select_join_stats()
    fused = E.run(hip, E.plan_of(E.FILTERS, E.DIMS, -1, fused=True), batches, native=True)
    s1, j1 = hip.select_stats(), hip.select_join_stats()
    assert fused[1] == [1, 1] and fused[4] == 2
    assert s1["batches"] - s0["batches"] == 2 and s1["declined"] == s0["declined"] and j1 == j0
