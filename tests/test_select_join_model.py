"""The numpy model of a non-aggregation batch with joins (tests/select_join_model.py) pinned to the per-node ABI sequence —
InitIndexVector, main-table filters, HashLookup per join, foreign filters, transforms — on every backend: what
AresFusedFilterJoinSelect is compared with.  One join fixture throughout: a dimension table of a mode-2, a mode-1 and a mode-0
batch, stale records, keys in the stash, two keys of one bucket and signature byte, misses and null keys."""
import numpy as np
import pytest

import select_join_model as J
import select_model as M
from aresdb_amd import abi

JOINED_DIMS = [((0, "region"), abi.Plus, 5, abi.Uint32), ((0, "rate"), abi.Multiply, 2.0, abi.Float32), ((0, "off"), None, None, abi.Int32),
               ((0, "region"), abi.Floor, 7, abi.Uint32), ("ts", None, None, abi.Uint32), ((0, "off"), abi.Multiply, 3, abi.Int16),
               ((0, "region"), None, None, abi.Uint16), ((0, "tz"), None, None, abi.Uint8)]


def check(be, cols, filters, joins, ffilters, dims, n):
    dcols = {k: c.upload(be) for k, c in cols.items()}
    dtables = [t.upload(be) for _, t in joins]
    try:
        count, vec = J.per_node(be, dcols, dtables, filters, joins, ffilters, dims, n)
        rows, want = J.model_join_select(cols, filters, joins, ffilters, dims, n)
        assert count == len(rows)
        M.assert_rows_equal(M.read_dim_rows(be, vec, count), want)
        vec.free()
    finally:
        for c in list(dcols.values()) + dtables:
            c.free()
    return len(rows)


def batch(n, key_dtype=abi.Uint32, **kw):
    t, key = J.fixture(n, key_dtype, **kw)
    cols = M.mixed_columns(n)
    cols["k0"] = key
    return cols, t


def test_the_fixture_reaches_the_stash_the_second_candidate_and_stale_records():
    n = 4097
    cols, t = batch(n)
    assert (t.stash_signatures() != 0).any(), "no key in the stash"
    keys = J.key_bytes_of(cols["k0"], n, 4)
    valid = M._valid(cols["k0"], n)
    hit = np.array([v and k in t.placed for k, v in zip(keys, valid)])
    assert 0.08 < 1 - valid.mean() < 0.12 and 0.10 < 1 - hit[valid].mean() < 0.25
    recs = [t.placed[k] for k, h in zip(keys, hit) if h]
    assert any(b == J.BASE_BATCH + 2 and i >= t.num_last for b, i in recs), "no stale record is looked up"
    assert any(b == J.BASE_BATCH + 7 for b, _ in recs), "the record outside the table is not looked up"
    region = t.joined(keys, valid, "region")
    assert 0.05 < 1 - region.valid[hit].mean() < 0.35


@pytest.mark.parametrize("n", [1, 4097])
def test_model_matches_the_per_node_sequence(be, n):
    cols, t = batch(n)
    res = check(be, cols, M.MIXED_FILTERS, [("k0", t)], [(0, "region", abi.LessThan, 150)], JOINED_DIMS, n)
    assert res > 0 or n == 1


@pytest.mark.parametrize("key_dtype", [abi.Uint32, abi.Int32, abi.Uint16, abi.Uint8, abi.Int64, abi.UUID])
def test_every_key_type(be, key_dtype):
    n = 600
    cols, t = batch(n, key_dtype)
    assert t.key_bytes == {abi.Uint32: 4, abi.Int32: 4, abi.Uint16: 2, abi.Uint8: 1, abi.Int64: 8, abi.UUID: 16}[key_dtype]
    check(be, cols, M.MIXED_FILTERS[:1], [("k0", t)], [(0, "off", abi.GreaterThan, -300)], JOINED_DIMS, n)


@pytest.mark.parametrize("geometry", [dict(num_buckets=1, nkeys=11), dict(num_hashes=2), dict(default=False)])
def test_index_geometries_and_a_table_without_default(be, geometry):
    n = 600
    cols, t = batch(n, **geometry)
    check(be, cols, [], [("k0", t)], [], JOINED_DIMS, n)


def test_two_joins_a_filter_on_one_and_dimensions_from_the_other(be):
    n = 4097
    cols, t0 = batch(n)
    t1, cols["k1"] = J.fixture(n, abi.Uint16, seed=23)
    joins = [("k0", t0), ("k1", t1)]
    dims = [((1, "region"), abi.Plus, 1, abi.Uint32), ((1, "rate"), None, None, abi.Float32), ("city", None, None, abi.Uint16),
            ((1, "tz"), None, None, abi.Uint8)]
    check(be, cols, M.MIXED_FILTERS, joins, [(0, "region", abi.GreaterThanOrEqual, 20)], dims, n)
    both = [((0, "region"), None, None, abi.Uint32), ((1, "off"), abi.Plus, 1000, abi.Int32), ((0, "tz"), abi.Plus, 1, abi.Uint8)]
    check(be, cols, M.MIXED_FILTERS, joins, [(0, "region", abi.GreaterThanOrEqual, 20), (1, "rate", abi.LessThan, 40.0)], both, n)
