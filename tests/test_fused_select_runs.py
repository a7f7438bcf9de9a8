"""AresFusedFilterSelect over run-length (mode 3) columns — the sort columns of archive batches — against the numpy model over
their row-space twins (tests/select_runs.py; tests/test_select_runs_model.py pins that reading to the per-node sequence) and
against the per-node sequence over the same uploaded columns, bit for bit, at the smallest shapes at which the kernel can go
wrong: run ends at tile, wave, lane and quad seams, tiles of one run and of 4096, null runs, validity bit offsets, limits at
run and tile ends, tiles rejected by a run, several ticket rounds."""
import numpy as np
import pytest

import harness as H
import select_model as M
import select_runs as R
import test_fused_select as F
from aresdb_amd import abi

pytestmark = pytest.mark.gpu
TILE = 4096
N = 3 * TILE + 5


@pytest.fixture(scope="module")
def hip():
    return H.hip_backend()


class Batch:
    """columns of one batch on the device: `dcols` as uploaded (mode 3 among them), `cols` what the model reads"""

    def __init__(self, be, pairs):
        self.be = be
        up, self.cols = R.split(pairs)
        self.dcols = {k: c.upload(be) for k, c in up.items()}

    def free(self):
        for c in self.dcols.values():
            c.free()


def check(b, filters, dims, n, limit=-1, capacity=None, model=True):
    """fused == model, rows at and beyond res untouched, fused == per-node sequence on the same library"""
    be = b.be
    capacity = capacity if capacity is not None else max(n, 1) + 3
    res, vec = M.fused(be, b.dcols, filters, dims, n, limit, capacity)
    try:
        got = M.read_dim_rows(be, vec, res)
        if model:
            rows, want = M.model_select(b.cols, filters, dims, n, limit)
            assert res == len(rows)
            M.assert_rows_equal(got, want, "fused against the model")
        F._sentinel_intact(vec, vec.values.read(np.uint8), res)
    finally:
        vec.free()
    count, pv = M.per_node(be, b.dcols, filters, dims, n)
    try:
        assert res == (count if limit < 0 else min(count, limit))
        M.assert_rows_equal(got, M.read_dim_rows(be, pv, res), "fused against the per-node sequence")
    finally:
        pv.free()
    return res


class Counted:
    """tiles scanned / rejected / staged by the calls inside the block"""

    def __init__(self, be):
        self.be = be

    def __enter__(self):
        self.t0, self.r0 = self.be.select_stats(), self.be.select_run_stats()
        return self

    def __exit__(self, *exc):
        t1, r1 = self.be.select_stats(), self.be.select_run_stats()
        self.tiles = t1["tiles"] - self.t0["tiles"]
        self.rejected, self.staged = r1["rejected"] - self.r0["rejected"], r1["staged"] - self.r0["staged"]


def _plain(n, seed=7):
    return M.mixed_columns(n, seed=seed)


def _runs_at(ends, n):
    """run lengths of runs that end at the given rows (and at n)"""
    ends = sorted(set(e for e in ends if 0 < e < n)) + [n]
    return np.diff(np.concatenate([[0], ends]))


def _col_with_ends(rng, dtype, ends, n, starting_index=0, valid_share=0.85):
    lens = _runs_at(ends, n)
    return R.run_col(dtype, R.values_of(rng, dtype, len(lens)), rng.random(len(lens)) < valid_share, lens, starting_index)


# ---- run ends at the tile seam ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("end,staged", [(4095, 1), (4096, 0), (4097, 1)])
def test_a_run_ends_at_the_tile_seam(hip, end, staged):
    """Two runs, the second from `end` to the batch's end: it covers tiles 1 (or most of it), 2 and 3, whose tiles are
    single-run; only a run end INSIDE a tile stages (none when the run ends with tile 0)."""
    rng = np.random.default_rng(end)
    pairs = dict(_plain(N))
    pairs["city"] = R.run_col(abi.Uint16, [7, 9], [True, True], [end, N - end], starting_index=1)
    b = Batch(hip, pairs)
    try:
        with Counted(hip) as c:
            res = check(b, [("city", abi.NotEqual, 8)], [("city", None, None, abi.Uint16)], N)
        assert res == N and (c.tiles, c.rejected, c.staged) == (4, 0, staged)
        res = check(b, [("city", abi.Equal, 9)], [("ts", None, None, abi.Uint32), ("city", abi.Plus, 1, abi.Uint16)], N)
        assert res == N - end
    finally:
        b.free()


# ---- the smallest and the largest tiles ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4095, 4096, 4097])
def test_runs_of_one_row(hip, n):
    """every row a run of its own: a tile of 4096 runs stages 4095 ends, the most there can be"""
    rng = np.random.default_rng(n)
    pairs = dict(_plain(n))
    pairs["city"] = R.run_col(abi.Uint16, rng.integers(0, 500, n), rng.random(n) < 0.9, np.ones(n, np.int64), starting_index=1)
    pairs["key"] = R.run_col(abi.UUID, rng.integers(0, 256, (n, 16), dtype=np.uint8), rng.random(n) < 0.9, np.ones(n, np.int64), starting_index=3)
    b = Batch(hip, pairs)
    try:
        with Counted(hip) as c:
            check(b, [("city", abi.LessThan, 400)], [("key", None, None, abi.UUID), ("ts", None, None, abi.Uint32), ("city", None, None, abi.Uint16)], n)
        assert c.staged == (1 if n > 1 else 0) and c.rejected <= 1  # (the lone row of n = 1 or of 4097's second tile may fail)
    finally:
        b.free()


# ---- run ends inside quads and at lane seams ------------------------------------------------------------------------------
def test_run_ends_inside_quads_and_at_the_seams(hip):
    """Lane l's quad q starts at row (256 q + l) * 4 of the tile.  Run ends one, two and three rows into a quad, at the seam
    between lanes 63 and 0 (which is the wave's: row 256), at the seam between quad indices (row 1024), at the tile's first
    and last rows, in the first tile and in the last, partial one; two columns with different ends in one plan."""
    rng = np.random.default_rng(31)
    inside = [1, 2, 3, 5, 10, 15, 21, 22, 23, 252, 253, 254, 255, 256, 257, 258, 259, 260, 511, 512, 513, 1021, 1022, 1023, 1024,
              1025, 1026, 1027, 1028, 2047, 2048, 2049, 3071, 3072, 3073, 4092, 4093, 4094, 4095]
    ends_a = inside + [TILE + e for e in (2, 1024, 1025)] + [3 * TILE + e for e in (1, 2, 3, 4)]
    ends_b = [e + 1 for e in inside[::2]] + [2 * TILE - 1, 2 * TILE, 2 * TILE + 1]
    pairs = dict(_plain(N))
    pairs["city"] = _col_with_ends(rng, abi.Uint16, ends_a, N, starting_index=1)
    pairs["status"] = _col_with_ends(rng, abi.Uint8, ends_b, N, starting_index=7)
    pairs["big"] = _col_with_ends(rng, abi.Int64, ends_a, N, starting_index=5)
    b = Batch(hip, pairs)
    try:
        dims = [("big", None, None, abi.Int64), ("ts", None, None, abi.Uint32), ("city", None, None, abi.Uint16), ("status", None, None, abi.Uint8)]
        assert check(b, [], dims, N) == N
        assert 0 < check(b, [("city", abi.LessThan, 400), ("status", abi.NotEqual, 2)], dims, N) < N
    finally:
        b.free()


# ---- null runs ----------------------------------------------------------------------------------------------------------------
def test_a_long_null_run_in_a_filter_column(hip):
    """rows [0, 2 TILE + 10) are one null run: no survivors there, tiles 0 and 1 are rejected by it, tile 2 stages"""
    pairs = dict(_plain(N))
    pairs["city"] = R.run_col(abi.Uint16, [3, 3, 4], [False, True, True], [2 * TILE + 10, 100, N - 2 * TILE - 110], starting_index=1)
    b = Batch(hip, pairs)
    try:
        with Counted(hip) as c:
            res = check(b, [("city", abi.Equal, 3)], [("ts", None, None, abi.Uint32), ("city", None, None, abi.Uint16)], N)
        assert res == 100 and (c.tiles, c.rejected, c.staged) == (4, 3, 1)  # (tile 3 lies in the run of 4s)
        with Counted(hip) as c:  # NotEqual does not let a null through either
            res = check(b, [("city", abi.NotEqual, 5)], [("ts", None, None, abi.Uint32)], N)
        assert res == N - 2 * TILE - 10 and c.rejected == 2
    finally:
        b.free()


@pytest.mark.parametrize("starting_index", [0, 1, 3, 7])
def test_null_runs_in_dimension_columns(hip, starting_index):
    """bare: a null run's rows keep the stored bits; with a binary functor their bits are 0; the run bitmap starts at bit
    StartingIndex"""
    rng = np.random.default_rng(40 + starting_index)
    pairs = dict(_plain(N))
    for name, dtype in [("ts", abi.Uint32), ("city", abi.Uint16), ("status", abi.Uint8), ("big", abi.Int64), ("key", abi.UUID)]:
        pairs[name] = R.random_run_col(rng, dtype, N, 3000, starting_index=starting_index, valid_share=0.6)
    b = Batch(hip, pairs)
    try:
        dims = [("key", None, None, abi.UUID), ("big", None, None, abi.Int64), ("ts", None, None, abi.Uint32), ("ts", abi.Floor, 60, abi.Uint32),
                ("city", None, None, abi.Uint16), ("city", abi.Plus, 7, abi.Uint16), ("status", None, None, abi.Uint8), ("status", abi.Multiply, 3, abi.Uint8)]
        assert check(b, [("amount", abi.GreaterThan, -500000)], dims, N) > N // 2
    finally:
        b.free()


# ---- plan shapes --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def archive(hip):
    """every column that can be run-length is, runs of mixed lengths; "fare", "amount" and "point" stay as they are"""
    rng = np.random.default_rng(50)
    pairs = dict(_plain(N))
    for name, dtype, si in [("ts", abi.Uint32, 3), ("city", abi.Uint16, 1), ("status", abi.Uint8, 7), ("delta", abi.Int16, 2),
                            ("big", abi.Int64, 5), ("key", abi.UUID, 1)]:
        pairs[name] = R.random_run_col(rng, dtype, N, 700, starting_index=si)
    pairs["tiny"] = R.random_run_col(rng, abi.Int8, N, 700, starting_index=4)
    pairs["plain_city"] = M.Col(abi.Uint16, rng.integers(0, 500, N), rng.random(N) < 0.9, starting_index=1)
    b = Batch(hip, pairs)
    yield b
    b.free()


def test_every_slot_width_from_a_run_length_column(archive):
    """16 / 8 / 4 / 4 / 2 / 2 / 1 / 1 byte slots; "ts", "status" and "delta" are read by a filter and a dimension at once"""
    dims = [("key", None, None, abi.UUID), ("big", None, None, abi.Int64), ("ts", abi.Floor, 60, abi.Uint32), ("delta", None, None, abi.Int32),
            ("city", None, None, abi.Uint16), ("delta", abi.Plus, 1000, abi.Int16), ("status", None, None, abi.Uint8), ("tiny", None, None, abi.Int8)]
    for n in (N, TILE + 9, 100):
        assert check(archive, [("ts", abi.GreaterThanOrEqual, 1200), ("status", abi.NotEqual, 2), ("delta", abi.LessThan, 250)], dims, n) > 0


def test_run_length_filters_with_plain_dimensions_and_the_reverse(archive):
    plain_dims = [("point", None, None, abi.GeoPoint), ("fare", abi.Multiply, 2.0, abi.Float32), ("amount", abi.Mod, 1000, abi.Int32),
                  ("plain_city", None, None, abi.Uint16)]
    assert check(archive, [("city", abi.LessThan, 400), ("status", abi.NotEqual, 2)], plain_dims, N) > 0
    run_dims = [("key", None, None, abi.UUID), ("ts", abi.Minus, 1500, abi.Int32), ("city", abi.Plus, 3, abi.Uint32), ("status", None, None, abi.Uint8)]
    assert check(archive, [("fare", abi.GreaterThan, 12.5), ("amount", abi.GreaterThan, -900000), ("plain_city", abi.NotEqual, 17)], run_dims, N) > 0


def test_four_run_length_filters_and_signed_columns(archive):
    """Int8 / Int16 run values are sign-extended, in the comparison and in the wider slot"""
    filters = [("delta", abi.GreaterThan, -250), ("tiny", abi.LessThan, 50), ("city", abi.NotEqual, 17), ("ts", abi.LessThan, 1950)]
    dims = [("delta", None, None, abi.Int32), ("tiny", abi.Multiply, 5, abi.Int32), ("tiny", None, None, abi.Int16), ("tiny", None, None, abi.Int8)]
    assert check(archive, filters, dims, N) > 0
    assert check(archive, [("tiny", abi.LessThan, 0), ("delta", abi.LessThan, 0)], dims, N) > 0


# ---- limits ---------------------------------------------------------------------------------------------------------------------
def test_limits_inside_a_run_at_a_run_end_and_at_a_tile_end(hip):
    pairs = dict(_plain(N))
    pairs["city"] = R.run_col(abi.Uint16, [1, 2, 3, 4], [True] * 4, [1000, 3096, 5000, N - 9096], starting_index=1)
    b = Batch(hip, pairs)
    try:
        dims = [("key", None, None, abi.UUID), ("ts", None, None, abi.Uint32), ("city", None, None, abi.Uint16)]
        for limit in (500, 1000, TILE, TILE + 1, 0, -1):
            res = check(b, [("city", abi.GreaterThan, 0)], dims, N, limit=limit)
            assert res == (N if limit < 0 else limit)
        for limit in (1, 3096, 3097, -1):  # survivors start inside tile 0 and end with it
            res = check(b, [("city", abi.Equal, 2)], dims, N, limit=limit)
            assert res == (3096 if limit < 0 else min(limit, 3096))
    finally:
        b.free()


# ---- tile rejection, observed ---------------------------------------------------------------------------------------------------
def _tile_census(counts, n, passing):
    """(tiles rejected, tiles staged) for a filter on a column with these counts whose runs pass as given"""
    rejected = staged = 0
    for t in range((n + TILE - 1) // TILE):
        lo = np.searchsorted(counts[:-1], t * TILE, side="right") - 1
        hi = np.searchsorted(counts[:-1], min((t + 1) * TILE, n) - 1, side="right") - 1
        staged += lo != hi
        rejected += lo == hi and not passing[lo]
    return rejected, staged


@pytest.mark.parametrize("grid", [None, "2"])
def test_tiles_wholly_inside_a_failing_run_are_rejected(hip, grid):
    """Twenty tiles, three runs, the middle one passing: the tiles that lie wholly in the two others are rejected — they read
    neither "ts" nor a dimension column — and the rows are the model's; with two workgroups the rejected tiles come between
    live ones over ten ticket rounds."""
    n = 20 * TILE - 7
    lens = [5 * TILE + 100, 6 * TILE + 17, n - 11 * TILE - 117]
    pairs = dict(_plain(n, seed=5))
    pairs["city"] = R.run_col(abi.Uint16, [11, 12, 13], [True] * 3, lens, starting_index=1)
    b = Batch(hip, pairs)
    try:
        want = _tile_census(pairs["city"][0].counts, n, [False, True, False])
        assert want == (13, 2)
        filters = [("city", abi.Equal, 12), ("ts", abi.GreaterThanOrEqual, 1200)]
        dims = [("key", None, None, abi.UUID), ("ts", abi.Floor, 60, abi.Uint32), ("city", None, None, abi.Uint16)]
        env = F._Env(hip, ARES_SELECT_GRID=grid) if grid else None
        if env:
            env.__enter__()
        try:
            with Counted(hip) as c:
                res = check(b, filters, dims, n)
        finally:
            if env:
                env.__exit__()
        assert 0 < res < lens[1]
        assert (c.tiles, c.rejected, c.staged) == (20, 13, 2)
    finally:
        b.free()


# ---- a column whose runs end before the batch does ---------------------------------------------------------------------------
def test_rows_past_the_last_count_take_the_last_run(hip):
    """the last count is 50 rows short of n (and, a second column, more than a tile short): compared with the per-node
    sequence only — the model does not define these rows"""
    rng = np.random.default_rng(60)
    pairs = dict(_plain(N))
    pairs["city"] = R.random_run_col(rng, abi.Uint16, N - 50, 900, starting_index=1)
    pairs["status"] = R.random_run_col(rng, abi.Uint8, N - TILE - 300, 900, starting_index=7)
    pairs["key"] = R.random_run_col(rng, abi.UUID, N - 50, 900, starting_index=1)
    b = Batch(hip, pairs)
    try:
        dims = [("key", None, None, abi.UUID), ("ts", None, None, abi.Uint32), ("city", None, None, abi.Uint16), ("status", None, None, abi.Uint8)]
        assert check(b, [], dims, N, model=False) == N
        check(b, [("city", abi.LessThan, 400), ("status", abi.NotEqual, 2)], dims, N, model=False)
    finally:
        b.free()


# ---- still declined, launching nothing -------------------------------------------------------------------------------------------
def test_declined_run_length_shapes_launch_nothing(hip):
    n = 100
    rng = np.random.default_rng(70)
    pairs = dict(_plain(n))
    lens = R.run_lengths(rng, n, 20)
    pairs["flag"] = (R.RunCol(abi.Bool, rng.random(len(lens)) < 0.5, np.ones(len(lens), bool), counts=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)),
                     None)
    pairs["big"] = R.random_run_col(rng, abi.Int64, n, 20)
    pairs["point"] = R.random_run_col(rng, abi.GeoPoint, n, 20)
    pairs["empty"] = (R.RunCol(abi.Uint16, np.zeros(0, np.uint16), np.zeros(0, bool), counts=np.zeros(1, np.uint32)), None)
    b = Batch(hip, pairs)
    try:
        ok_dims = [("ts", None, None, abi.Uint32)]
        before = hip.select_stats()
        F._declined(hip, b, [], [("flag", None, None, abi.Uint8)])
        F._declined(hip, b, [("flag", abi.Equal, 1)], ok_dims)
        F._declined(hip, b, [], [("big", abi.Plus, 1, abi.Int64)])
        F._declined(hip, b, [], [("point", None, None, abi.GeoPoint)])  # (never decoded by the per-node sequence either)
        F._declined(hip, b, [], [("empty", None, None, abi.Uint16)])
        F._declined(hip, b, [("empty", abi.Equal, 1)], ok_dims)
        after = hip.select_stats()
        assert after["declined"] - before["declined"] == 6 and after["batches"] == before["batches"]
    finally:
        b.free()


# ---- through the C++ driver (helpers of tests/test_nonaggr_executor.py) ----------------------------------------------------------
def _archive_batch(E, n, seed):
    """a batch whose filter column "status" and dimension column "city" are run-length; (batch to run, its row-space twin)"""
    rng = np.random.default_rng(seed)
    pairs = dict(M.mixed_columns(n, seed=seed))
    pairs["status"] = R.random_run_col(rng, abi.Uint8, n, 2500, starting_index=7)
    pairs["city"] = R.random_run_col(rng, abi.Uint16, n, 300, starting_index=1)
    up, twin = R.split(pairs)
    return E.B(n, seed, cols=up), E.B(n, seed, cols=twin)


@pytest.mark.parametrize("limit", [-1, 3000])
def test_the_driver_fuses_live_archive_live(hip, limit):
    """[live, archive with a mode-3 filter column, live] with useFusedExtension: all three batches go through the extension
    (before, the archive batch was declined and the query stopped asking), and the rows equal the unfused run's and the
    model's over the row-space twin; limit 3000 is met inside the archive batch."""
    import test_nonaggr_executor as E
    arch, twin = _archive_batch(E, N, 81)
    batches, twins = [E.B(2000, 80), arch, E.B(300, 82)], [E.B(2000, 80), twin, E.B(300, 82)]
    want, per_batch = E.expected(twins, E.FILTERS, E.DIMS, limit)
    if limit >= 0:
        assert 0 < per_batch[0] < limit < per_batch[0] + len(M.model_select(twin.cols, E.FILTERS, E.DIMS, N)[0]) and per_batch[2] is None
    plain = E.run(hip, E.plan_of(E.FILTERS, E.DIMS, limit), batches, native=True)
    fused = E.run(hip, E.plan_of(E.FILTERS, E.DIMS, limit, fused=True), batches, native=True)
    M.assert_rows_equal(plain[0], want)
    M.assert_rows_equal(fused[0], want)
    assert plain[4] == 0 and fused[2] == plain[2] and fused[3] == plain[3]
    assert fused[4] == (3 if limit < 0 else 2)
    for i, ran in enumerate(per_batch):
        if ran is not None:
            assert fused[1][i] == 1  # one ABI call for the batch
