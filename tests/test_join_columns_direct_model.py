"""The idea behind the direct flavour of AresJoinColumnsRun, pinned on the oracle (no GPU, no new code): a key column of a 1- or
2-byte type has 256 or 65 536 stored values, so the per-node sequence — HashLookup, then UnaryTransform(Noop,
ForeignColumnInput) — run ONCE over a column that enumerates them gives a table of (value, validity) per stored value and joined
column, and a row's joined value is that table indexed by the row's stored key: (entry value, entry validity) for a valid key,
(0, null) for a null one.  Checked against the same sequence run over the rows, and against the dictionary model
(select_join_model.Table.joined), for every narrow key type — Int8 / Int16 keys are sign-extended before keyBytes of them are
kept — and for an index whose keyBytes are narrower or wider than the key column."""
import numpy as np
import pytest

import harness as H
import narrow_join_model as N
import select_join_model as J
import select_model as M
from aresdb_amd import abi

ORDER = ["region", "rate", "off", "tz"]  # Uint32, Float32, Int16, Uint8 in vector order


@pytest.fixture(scope="module")
def oracle():
    return H.oracle_backend()


def per_node(be, dt, t, key, n):
    """[(value bytes (n, width), validity)] per column of ORDER: what the per-node sequence leaves in dimension slots"""
    dkey = key.upload(be)
    try:
        dims = [((0, name), None, None, t.COLUMNS[name]) for name in ORDER]
        count, vec = J.per_node(be, {"k0": dkey}, [dt], [], [("k0", t)], [], dims, n)
        try:
            assert count == n
            return [(values.copy(), ok.astype(bool)) for values, ok in M.read_dim_rows(be, vec, n)]
        finally:
            vec.free()
    finally:
        dkey.free()


@pytest.mark.parametrize("key_dtype,kb", [(d, None) for d in N.NARROW] + [(abi.Int8, 4), (abi.Int16, 4), (abi.Uint16, 1), (abi.Int16, 1)],
                         ids=lambda x: str(x))
def test_the_table_indexed_by_the_stored_key_is_the_per_row_sequence(oracle, key_dtype, kb):
    n = 700
    t = N.make_table(key_dtype, kb, default=kb is None)
    key = N.key_column(t, n, 21)
    assert N.reached(t, key, n) == N.CASES
    keys, key_valid = J.key_bytes_of(key, n, t.key_bytes), M._valid(key, n)
    if key_dtype in (abi.Int8, abi.Int16):  # negative keys that are in the table
        assert any(v < 0 and ok and k in t.placed for v, ok, k in zip(key.values[:n], key_valid, keys))
    dt = t.upload(oracle)
    try:
        space = N.KEY_SPACE[key_dtype]
        table = per_node(oracle, dt, t, N.enumerated(key_dtype), space)
        rows = per_node(oracle, dt, t, key, n)
        at = N.stored(key, n)
        for name, (tv, tok), (rv, rok) in zip(ORDER, table, rows):
            want_values = np.where(key_valid[:, None], tv[at], 0)
            want_valid = key_valid & tok[at]
            assert np.array_equal(rok, want_valid), name
            assert np.array_equal(rv, want_values), name
            col = t.joined(keys, key_valid, name)  # the dictionary model says the same
            assert np.array_equal(col.valid, want_valid), name
            assert np.array_equal(col.values.view(np.uint8).reshape(n, -1), want_values), name
            assert want_valid.any() and not want_valid.all()
    finally:
        dt.free()
