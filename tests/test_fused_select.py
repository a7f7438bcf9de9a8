"""AresFusedFilterSelect (include/ares_extensions.h): the limit-aware select scan against the numpy model of
tests/select_model.py and, for the same batch, against the per-node ABI sequence on the same library — bit for bit, at the
smallest shapes at which the kernel can go wrong: tile edges (4096 rows), ragged quads, validity bit offsets, limits at tile
boundaries, several ticket rounds, the early out."""
import os

import numpy as np
import pytest

import harness as H
import select_model as M
from aresdb_amd import abi

pytestmark = pytest.mark.gpu
TILE = 4096


@pytest.fixture(scope="module")
def hip():
    return H.hip_backend()


class Batch:
    """columns of one batch on the device, uploaded once per module"""

    def __init__(self, be, cols):
        self.be, self.cols = be, cols
        self.dcols = {k: c.upload(be) for k, c in cols.items()}

    def free(self):
        for c in self.dcols.values():
            c.free()


def _sentinel_intact(vec, blob, res):
    for vo, no, w in vec.dim_offsets():
        assert (blob[vo + res * w: vo + vec.capacity * w] == M.SENTINEL).all(), "value rows at or beyond res were written"
        assert (blob[no + res: no + vec.capacity] == M.SENTINEL).all(), "validity rows at or beyond res were written"


def check(b, filters, dims, n, limit=-1, capacity=None, per_node=True):
    """fused == model, rows at and beyond res untouched, fused == per-node sequence on the same library; returns the bytes"""
    be = b.be
    rows, want = M.model_select(b.cols, filters, dims, n, limit)
    capacity = capacity if capacity is not None else max(n, 1) + 3
    res, vec = M.fused(be, b.dcols, filters, dims, n, limit, capacity)
    try:
        assert res == len(rows)
        got = M.read_dim_rows(be, vec, res)
        M.assert_rows_equal(got, want, "fused against the model")
        blob = vec.values.read(np.uint8)
        _sentinel_intact(vec, blob, res)
    finally:
        vec.free()
    if per_node:
        count, pv = M.per_node(be, b.dcols, filters, dims, n)
        try:
            assert res == (count if limit < 0 else min(count, limit))
            M.assert_rows_equal(got, M.read_dim_rows(be, pv, res), "fused against the per-node sequence")
        finally:
            pv.free()
    return res, blob


@pytest.fixture(scope="module")
def mixed(hip):
    b = Batch(hip, M.mixed_columns(3 * TILE + 5))
    yield b
    b.free()


@pytest.mark.parametrize("n", [1, 3, 4095, 4096, 4097, 3 * TILE + 5])
def test_batch_sizes_around_the_tile(mixed, n):
    """every slot width in one plan, validity offsets that are no multiple of 8, a column read by a filter and a dimension"""
    res, _ = check(mixed, M.MIXED_FILTERS, M.MIXED_DIMS, n)
    assert res > 0 or n < 4


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_zero_to_four_filters(mixed, k):
    filters = (M.MIXED_FILTERS + [("fare", abi.LessThan, 80.0)])[:k]
    check(mixed, filters, M.MIXED_DIMS, 2 * TILE + 77)


def test_one_dimension(mixed):
    check(mixed, M.MIXED_FILTERS, [("city", abi.Plus, 7, abi.Uint32)], TILE + 9)
    check(mixed, M.MIXED_FILTERS[:1], [("key", None, None, abi.UUID)], TILE + 9)


def test_expressions_and_conversions(mixed):
    dims = [("amount", abi.Divide, 7, abi.Int32), ("amount", abi.Mod, 1000, abi.Int32), ("fare", abi.Multiply, 2.0, abi.Float32),
            ("ts", abi.Minus, 1500, abi.Int32), ("city", abi.Plus, 3, abi.Uint32), ("delta", None, None, abi.Int32),
            ("amount", None, None, abi.Uint16), ("city", abi.Multiply, 3, abi.Uint8)]
    filters = [("fare", abi.GreaterThan, 12.5), ("delta", abi.LessThanOrEqual, 250), ("amount", abi.GreaterThan, -900000),
               ("city", abi.NotEqual, 17)]
    check(mixed, filters, dims, TILE + 301)


def test_survivors_only_in_the_last_partial_tile(hip):
    n = 3 * TILE + 5
    cols = M.mixed_columns(n, seed=3)
    ts = np.full(n, 1000, np.uint32)
    ts[3 * TILE:] = 1500
    cols["ts"] = M.Col(abi.Uint32, ts, np.ones(n, bool), starting_index=3)
    b = Batch(hip, cols)
    try:
        res, _ = check(b, [("ts", abi.Equal, 1500)], M.MIXED_DIMS, n)
        assert res == 5
        res, _ = check(b, [("ts", abi.Equal, 1500)], M.MIXED_DIMS, n, limit=2)
        assert res == 2
        res, _ = check(b, [("ts", abi.Equal, 77)], M.MIXED_DIMS, n)  # no survivors at all
        assert res == 0
    finally:
        b.free()


def test_limits_at_the_tile_boundaries(mixed):
    n = 2 * TILE + 100
    rows, _ = M.model_select(mixed.cols, M.MIXED_FILTERS, M.MIXED_DIMS, n)
    total, in_tile0 = len(rows), int((rows < TILE).sum())
    assert 0 < in_tile0 < total
    for limit in [0, 1, in_tile0, in_tile0 + 1, total - 1, total, total + 1, -1]:
        res, _ = check(mixed, M.MIXED_FILTERS, M.MIXED_DIMS, n, limit=limit, per_node=limit in (in_tile0, -1))
        assert res == (total if limit < 0 else min(total, limit))


def test_every_row_surviving(mixed):
    n = 2 * TILE + 1
    for limit in [-1, n, n - 1, TILE]:
        res, _ = check(mixed, [("amount", abi.GreaterThan, -2000000)], M.MIXED_DIMS, n, limit=limit, per_node=limit < 0)
        assert res == (n if limit < 0 else min(n, limit))


def test_capacity_may_be_the_limit(mixed):
    res, _ = check(mixed, [], M.MIXED_DIMS, 2 * TILE, limit=10, capacity=10, per_node=False)
    assert res == 10


class _Env:
    def __init__(self, be, **kv):
        self.be, self.kv = be, kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)
        self.be.reload_env()

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        self.be.reload_env()


@pytest.fixture(scope="module")
def twenty(hip):
    b = Batch(hip, M.mixed_columns(20 * TILE - 7, seed=5))
    yield b
    b.free()


def test_ten_ticket_rounds_equal_the_default_grid(twenty):
    n = 20 * TILE - 7
    _, default = check(twenty, M.MIXED_FILTERS, M.MIXED_DIMS, n)
    with _Env(twenty.be, ARES_SELECT_GRID="2"):
        before = twenty.be.select_stats()
        _, two = check(twenty, M.MIXED_FILTERS, M.MIXED_DIMS, n, per_node=False)
        after = twenty.be.select_stats()
    assert np.array_equal(default, two)
    assert after["tiles"] - before["tiles"] == 20 and after["batches"] - before["batches"] == 1


def test_early_out_scans_one_round_of_the_grid(twenty):
    """Every row survives and ten are wanted: with two workgroups at most two tiles are read (a condition of the design —
    one round of the grid — not a measurement); without the early out all twenty would be."""
    n = 20 * TILE - 7
    with _Env(twenty.be, ARES_SELECT_GRID="2"):
        before = twenty.be.select_stats()
        res, _ = check(twenty, [("amount", abi.GreaterThan, -2000000)], M.MIXED_DIMS, n, limit=10, per_node=False)
        after = twenty.be.select_stats()
    assert res == 10
    assert after["tiles"] - before["tiles"] <= 2
    assert after["rows"] - before["rows"] == 10


def test_default_grid_takes_a_second_ticket_round(hip):
    n = 2098177
    rng = np.random.default_rng(21)
    cols = {"ts": M.Col(abi.Uint32, rng.integers(1000, 2000, n), rng.random(n) < 0.95, starting_index=3),
            "city": M.Col(abi.Uint16, rng.integers(0, 500, n), rng.random(n) < 0.9, starting_index=1),
            "key": M.Col(abi.UUID, rng.integers(0, 256, (n, 16), dtype=np.uint8), rng.random(n) < 0.9, starting_index=5)}
    b = Batch(hip, cols)
    try:
        filters = [("ts", abi.GreaterThanOrEqual, 1300), ("ts", abi.LessThan, 1800)]
        dims = [("key", None, None, abi.UUID), ("ts", abi.Floor, 60, abi.Uint32), ("city", None, None, abi.Uint16)]
        res, _ = check(b, filters, dims, n)
        assert res > n // 3
        res, _ = check(b, filters, dims, n, limit=500003, per_node=False)
        assert res == 500003
    finally:
        b.free()


def _declined(be, b, filters, dims, n=100):
    be.wait()
    be.profiler_enable(True)
    try:
        with pytest.raises(abi.AresError, match="^not fusable"):
            M.fused(be, b.dcols, filters, dims, n, -1, n)
        be.wait()
        assert be.profiler_report() == {}, "a declined shape launched a kernel"
    finally:
        be.profiler_enable(False)


def test_declined_shapes_launch_nothing(hip):
    n = 100
    cols = M.mixed_columns(n)
    cols["flag"] = M.Col(abi.Bool, np.arange(n) % 3 == 0, np.ones(n, bool))
    cols["absent"] = M.Col(abi.Uint32, None, default=5)
    b = Batch(hip, cols)
    try:
        ok_dims = [("ts", None, None, abi.Uint32)]
        before = hip.select_stats()
        _declined(hip, b, [], [("flag", None, None, abi.Uint8)])
        _declined(hip, b, [("flag", abi.Equal, 1)], ok_dims)
        _declined(hip, b, [], [("absent", None, None, abi.Uint32)])
        _declined(hip, b, [("absent", abi.Equal, 5)], ok_dims)
        _declined(hip, b, [], [("big", abi.Plus, 1, abi.Int64)])
        _declined(hip, b, [("ts", abi.GreaterThan, 0)] * 5, ok_dims)
        _declined(hip, b, [], [("ts", None, None, abi.Uint32)] * 9)
        with _Env(hip, ARES_SELECT="0"):
            _declined(hip, b, M.MIXED_FILTERS, M.MIXED_DIMS)
        after = hip.select_stats()
        assert after["declined"] - before["declined"] == 8 and after["batches"] == before["batches"]
        res, _ = check(b, M.MIXED_FILTERS, M.MIXED_DIMS, n)  # the same plan once the switch is back
        assert res > 0
    finally:
        b.free()


def test_too_small_a_capacity_is_an_error_not_a_decline(mixed):
    for limit, capacity in [(-1, 99), (50, 49)]:
        with pytest.raises(abi.AresError) as e:
            M.fused(mixed.be, mixed.dcols, M.MIXED_FILTERS, M.MIXED_DIMS, 100, limit, capacity)
        assert "VectorCapacity" in str(e.value) and "not fusable" not in str(e.value)


def test_zero_rows_and_zero_limit_launch_nothing(mixed):
    be = mixed.be
    be.wait()
    be.profiler_enable(True)
    try:
        for n, limit in [(0, -1), (100, 0)]:
            res, vec = M.fused(be, mixed.dcols, M.MIXED_FILTERS, M.MIXED_DIMS, n, limit, 8)
            assert res == 0
            _sentinel_intact(vec, vec.values.read(np.uint8), 0)
            vec.free()
        be.wait()
        assert be.profiler_report() == {}
    finally:
        be.profiler_enable(False)


# ---- the C++ driver with useFusedExtension (helpers of tests/test_nonaggr_executor.py) -----------------------------------
def _fused_against_plain(hip, batches, filters, limit, capacity_of, **kw):
    import test_nonaggr_executor as E
    want, per_batch = E.expected(batches, filters, E.DIMS, limit, capacity_of=capacity_of)
    plain = E.run(hip, E.plan_of(filters, E.DIMS, limit), batches, native=True, **kw)
    fused = E.run(hip, E.plan_of(filters, E.DIMS, limit, fused=True), batches, native=True, **kw)
    M.assert_rows_equal(plain[0], want)
    M.assert_rows_equal(fused[0], want)
    assert plain[4] == 0 and fused[2] == plain[2] and fused[3] == plain[3]
    return plain, fused, per_batch


@pytest.mark.parametrize("max_batch", [9000, None])
def test_fused_extension_takes_the_eligible_batches(hip, max_batch):
    """useFusedExtension: every batch without base counts goes through AresFusedFilterSelect (the limit handed down is what
    is still wanted), the batch with base counts takes the ordinary sequence, and the rows equal the unfused run's — with the
    buffers sized by AresQuerySetMaxBatchSize and by the batches themselves (the largest comes third)."""
    import test_nonaggr_executor as E
    rl, _ = E._run_length_batch()
    batches = [E.B(5000, 40), rl, E.B(9000, 41), E.B(300, 42)]
    for limit in (-1, 4000):
        _, fused, per_batch = _fused_against_plain(hip, batches, E.FILTERS, limit, 5000 + 5000 // 8, max_batch=max_batch)
        assert fused[4] == sum(1 for b, n in zip(batches, per_batch) if n is not None and b.base_counts is None)
        for i, n in enumerate(per_batch):
            if n is not None and batches[i].base_counts is None:
                assert fused[1][i] == 1  # one ABI call for the batch


def test_fused_extension_and_a_filtered_batch_with_base_counts(hip):
    """The batch with base counts comes FIRST and its filters drop rows, no AresQuerySetMaxBatchSize: both runs size the
    buffers by the batch's 64 rows, Expand keeps every repeated survivor, and the two runs return the same rows."""
    import test_nonaggr_executor as E
    b, survivors = E._filtered_run_length_batch()
    _, fused, per_batch = _fused_against_plain(hip, [b, E.B(50, 43), b], E.FILTERS, -1, 72)
    assert per_batch[0] == per_batch[2] == 2 * survivors and fused[4] == 1


def test_fused_extension_stops_asking_after_a_decline(hip):
    """A plan the library declines (a float result into a 2-byte slot: the generic transform kernel's case): the first batch
    pays one extra ABI call, the later ones none, and the rows are the ordinary sequence's."""
    import test_nonaggr_executor as E
    from aresdb_amd.executor import Binary, Col, Const, DimensionSpec
    batches = [E.B(300, 50), E.B(400, 51), E.B(200, 52)]

    def plan(fused):
        p = E.plan_of(E.FILTERS, E.DIMS[3:], -1, fused=fused)
        p.dimensions.append(DimensionSpec(Binary(abi.Multiply, Col("fare"), Const(2.0)), abi.Uint16))
        return p
    plain = E.run(hip, plan(False), batches, native=True)
    fused = E.run(hip, plan(True), batches, native=True)
    M.assert_rows_equal(fused[0], plain[0])
    assert plain[3] > 100 and fused[4] == 0
    assert [f - p for f, p in zip(fused[1], plain[1])] == [1, 0, 0]
