"""tests/geo_column_model.py pinned, on the CPU, to GeoBatchIntersects + WriteGeoShapeDim of the C checker and of the
reference's host build: over the main-table cases of every group of tests/test_geo_semantics.py, run with the identity index
vector over the whole column and a cleared predicate vector, the model's valid rows are the index entries the call keeps, and
— when the filter asks for the inside — the valid rows' values, in row order, are the dimension bytes it writes."""
import numpy as np
import pytest

import geo_column_model as GC
import test_geo_semantics as S
from test_edge_semantics import CPU, _cpu_backend


def row_space(c):
    """the case over every row of its column: identity index vector, no prefill, no RecordID vectors"""
    n = len(c.points)
    return c.with_(index=np.arange(n, dtype=np.uint32), n=n, prefill=None, rids=[])


def main_cases(group):
    """the group's cases whose points are a main-table column, in row space"""
    return [row_space(c) for c in S.cases_of(group, joined=False) if c.joined is None]


def model_of(c, keep=None):
    return GC.expected_column(c.lats, c.longs, c.shape, c.words, c.points, c.valid, c.in_or_out, keep)


@CPU
@pytest.mark.parametrize("group", list(S.GROUPS))
def test_the_column_is_what_the_per_node_calls_keep_and_write(which, group):
    be, ran, seen_valid, seen_null = _cpu_backend(which), 0, 0, 0
    for c in main_cases(group):
        if which == "ref" and len(c.lats) == 0:   # (geo_model: the reference divides by the point count)
            continue
        values, row_valid, live = model_of(c)
        got = c.run(be)
        tag = f"{c!r} on {be.name}"
        assert got["kept"] == int(row_valid.sum()), tag
        assert np.array_equal(got["index"], np.flatnonzero(row_valid).astype(np.uint32)), tag
        assert not values[~row_valid].any(), tag
        if c.in_or_out:
            assert np.array_equal(got["dim_values"][:got["kept"]], values[row_valid]), tag
            assert got["dim_nulls"][:got["kept"]].all() and not got["dim_nulls"][got["kept"]:].any(), tag
        else:
            assert not values.any(), tag
        assert np.array_equal(live, np.ones(c.n, bool) if c.valid is None else c.valid), tag
        ran += 1
        seen_valid += int(row_valid.sum())
        seen_null += int((~row_valid).sum())
    print(f"{which} {group}: {ran} compared calls, {seen_valid} valid rows, {seen_null} null rows")
    assert ran >= 2 and seen_valid > 0 and seen_null > 0


def test_pruned_rows_are_null_and_not_live():
    c = main_cases("half_open")[1]
    keep = np.arange(c.n) % 3 != 1
    values, row_valid, live = model_of(c, keep)
    base_values, base_valid, base_live = model_of(c)
    assert not row_valid[~keep].any() and not values[~keep].any() and not live[~keep].any()
    assert np.array_equal(row_valid[keep], base_valid[keep]) and np.array_equal(values[keep], base_values[keep])
    assert np.array_equal(live[keep], base_live[keep]) and 0 < live.sum() < base_live.sum()


def test_layout_and_chunk_count():
    bitmap, values = GC.layout(np.arange(70, dtype=np.uint8), np.arange(70) % 2 == 0)
    assert len(bitmap) == 64 and len(values) == 70 and GC.column_bytes(70) == 64 + 128
    assert bitmap[:9].tolist() == [0x55] * 8 + [0x15] and not bitmap[9:].any()
    live = np.zeros(3 * 1024 + 1, bool)
    live[:65] = True          # tile 0: 65 live rows, two chunks
    live[1024:2048] = True    # tile 1: full, sixteen chunks
    live[3072] = True         # tile 3: its one row (tile 2: none)
    assert GC.chunks_walked(live) == 2 + 16 + 0 + 1
