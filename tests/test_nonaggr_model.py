"""The numpy model of a non-aggregation batch (tests/select_model.py) pinned to the per-node ABI sequence — InitIndexVector,
filters, transforms into a dimension vector, copied back whole — on every backend: what the fused select scan and the
non-aggregation executor are compared with."""
import numpy as np
import pytest

import select_model as M
from aresdb_amd import abi


def _check(be, cols, filters, dims, n):
    dcols = {k: c.upload(be) for k, c in cols.items()}
    try:
        count, vec = M.per_node(be, dcols, filters, dims, n)
        rows, want = M.model_select(cols, filters, dims, n)
        assert count == len(rows)
        M.assert_rows_equal(M.read_dim_rows(be, vec, count), want)
        vec.free()
    finally:
        for c in dcols.values():
            c.free()


@pytest.mark.parametrize("n", [1, 37, 4097])
def test_model_matches_the_per_node_sequence_on_the_mixed_batch(be, n):
    _check(be, M.mixed_columns(n), M.MIXED_FILTERS, M.MIXED_DIMS, n)


def test_model_matches_the_per_node_sequence_on_expressions(be):
    n = 301
    cols = M.mixed_columns(n, seed=11)
    filters = [("fare", abi.GreaterThan, 12.5), ("delta", abi.LessThanOrEqual, 250), ("amount", abi.GreaterThan, -900000),
               ("city", abi.NotEqual, 17)]
    dims = [("amount", abi.Divide, 7, abi.Int32), ("amount", abi.Mod, 1000, abi.Int32), ("fare", abi.Multiply, 2.0, abi.Float32),
            ("ts", abi.Minus, 1500, abi.Int32), ("city", abi.Plus, 3, abi.Uint32), ("delta", None, None, abi.Int32),
            ("amount", None, None, abi.Uint16), ("city", abi.Multiply, 3, abi.Uint8)]
    _check(be, cols, filters, dims, n)
