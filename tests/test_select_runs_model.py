"""The row-space reading of run-length (mode 3) columns pinned to the per-node ABI sequence on every backend: the numpy model
of tests/select_model.py over the np.repeat twins of tests/select_runs.py equals InitIndexVector, the filters and the
transforms over the uploaded run arrays — run validity with a StartingIndex, the value bytes of null rows (stored bits for a
bare column, 0 for a binary functor), Int64 and UUID columns.  This is what the fused select scan is compared with.

A GeoPoint column in the run-length layout is not here: neither the reference nor the oracle decodes one (it is bound as a
column with validity and read row by row, past the run arrays), so no row-space reading of it exists, and the select scan
declines it (tests/test_fused_select_runs.py)."""
import numpy as np
import pytest

import select_model as M
import select_runs as R
from aresdb_amd import abi


def _check(be, pairs, filters, dims, n):
    up, twin = R.split(pairs)
    dcols = {k: c.upload(be) for k, c in up.items()}
    try:
        count, vec = M.per_node(be, dcols, filters, dims, n)
        try:
            rows, want = M.model_select(twin, filters, dims, n)
            assert count == len(rows)
            M.assert_rows_equal(M.read_dim_rows(be, vec, count), want)
        finally:
            vec.free()
    finally:
        for c in dcols.values():
            c.free()
    return count


def _columns(n, seed):
    rng = np.random.default_rng(seed)
    longest = max(1, n // 3)
    return {"ts": R.random_run_col(rng, abi.Uint32, n, longest, starting_index=3),
            "city": R.random_run_col(rng, abi.Uint16, n, longest, starting_index=1),
            "status": R.random_run_col(rng, abi.Uint8, n, longest, starting_index=7),
            "delta": R.random_run_col(rng, abi.Int16, n, longest, starting_index=2),
            "tiny": R.random_run_col(rng, abi.Int8, n, longest, starting_index=5),
            "big": R.random_run_col(rng, abi.Int64, n, longest, starting_index=5),
            "key": R.random_run_col(rng, abi.UUID, n, longest, starting_index=1)}


NARROW_DIMS = [("ts", abi.Floor, 60, abi.Uint32), ("ts", None, None, abi.Uint32), ("city", None, None, abi.Uint16),
               ("delta", abi.Plus, 1000, abi.Int16), ("status", None, None, abi.Uint8), ("tiny", abi.Minus, 3, abi.Int8)]


@pytest.mark.parametrize("n", [1, 37, 4097])
def test_narrow_run_length_columns_of_each_width(be, n):
    """1-, 2- and 4-byte columns, signed and unsigned, as filters and as dimensions (bare: stored bits of null runs; with a
    functor: 0)"""
    for filters in ([], [("ts", abi.GreaterThanOrEqual, 1200), ("status", abi.NotEqual, 2), ("delta", abi.LessThan, 200)]):
        _check(be, _columns(n, seed=n), filters, NARROW_DIMS, n)


@pytest.mark.parametrize("n", [1, 37, 4097])
@pytest.mark.parametrize("name,dtype", [("big", abi.Int64), ("key", abi.UUID)])
def test_wide_run_length_columns(be, n, name, dtype):
    count = _check(be, _columns(n, seed=100 + n), [("city", abi.LessThan, 400)], [(name, None, None, dtype), ("city", None, None, abi.Uint16)], n)
    assert count > 0 or n == 1
