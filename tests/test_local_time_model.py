"""The numpy model of tests/local_time_model.py pinned to the per-node sequence on the oracle: HashLookup over every row, then
BinaryTransform(Plus, time, the zone column read through its TimezoneLookup) into a 4-byte dimension slot.  The fixtures must
reach every case the rule names (local_time_model.CASES)."""
import numpy as np
import pytest

import harness as H
import local_time_model as L
import select_join_model as J
from aresdb_amd import abi

N = 4097
SHAPES = [  # (key type, keyBytes of the index or None for the column's width, zone column, time type, table has defaults)
    (abi.Uint16, None, "zone8", abi.Uint32, True),
    (abi.Uint16, None, "zone16", abi.Uint32, False),
    (abi.Int16, 4, "zone16", abi.Int32, True),
    (abi.Int8, None, "zone8", abi.Uint32, True),
    (abi.Uint8, 2, "zone16", abi.Uint32, False),
    (abi.Uint32, None, "zone16", abi.Int32, True),
    (abi.Int64, None, "zone8", abi.Uint32, True),
    (abi.UUID, None, "zone16", abi.Uint32, False),
]


def per_node(be, dtable, dtime, dkey, zone, tz, n, out_type):
    """(values uint32, validity bytes) the per-node sequence leaves in a dimension slot for the n rows of the batch"""
    idx, rids = H.Buf(be, nbytes=4 * n), H.Buf(be, nbytes=8 * n)
    vec = H.DimVector(be, n, (0, 0, 1, 0, 0), with_hash=False, with_index=False)
    try:
        be.call("InitIndexVector", idx.ptr, 0, n, None, 0)
        be.call("HashLookup", dkey.input(), rids.ptr, idx.ptr, n, None, 0, dtable.index_struct(), None, 0)
        (vo, no, _), = vec.dim_offsets()
        out = H.dimension_output(vec.values.ptr + vo, vec.values.ptr + no, out_type)
        be.call("BinaryTransform", dtime.input(), L.zone_input(dtable, zone, rids.ptr, tz.ptr, len(tz.data)), out, idx.ptr, n, None, 0,
                abi.Plus, None, 0)
        be.wait()
        return vec.values.read(np.uint32, n, vo), vec.values.read(np.uint8, n, no)
    finally:
        for b in (idx, rids, vec):
            b.free()


class Tz:
    def __init__(self, be, data):
        self.data, self.buf = data, H.Buf(be, data)
        self.ptr = self.buf.ptr

    def free(self):
        self.buf.free()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(x) for x in s))
def test_the_model_is_the_per_node_sequence_on_the_oracle(shape):
    key_dtype, key_bytes, zone, time_dtype, default = shape
    be = H.oracle_backend()
    t, time, key = L.fixture(N, key_dtype, key_bytes, time_dtype, default=default)
    tz = Tz(be, L.tz_offsets())
    dtable, dtime, dkey = t.upload(be), time.upload(be), key.upload(be)
    try:
        want_values, want_valid, cases = L.local_time(t, tz.data, time, key, zone, N)
        for out_type in (abi.Uint32, abi.Int32):
            values, valid = per_node(be, dtable, dtime, dkey, zone, tz, N, out_type)
            assert np.array_equal(valid != 0, want_valid)
            assert np.array_equal(values, want_values)
        assert 0.2 < want_valid.mean() < 0.9
        if key_dtype in (abi.Int8, abi.Int16):
            assert (key.values[want_valid] < 0).any(), "no negative key found its record"
        if zone == "zone16":
            assert L.CASES_U16 <= cases, L.CASES_U16 - cases
        assert L.CASES - {"mode 0 default", "mode 0 none"} <= cases, L.CASES - cases
        assert ("mode 0 default" if default else "mode 0 none") in cases
    finally:
        for d in (dtable, dtime, dkey, tz):
            d.free()


def test_the_fixtures_reach_every_case():
    """the union over the shapes above: every case the rule names"""
    reached = set()
    for key_dtype, key_bytes, zone, time_dtype, default in SHAPES:
        t, time, key = L.fixture(N, key_dtype, key_bytes, time_dtype, default=default)
        reached |= L.local_time(t, L.tz_offsets(), time, key, zone, N)[2]
    assert L.CASES | L.CASES_U16 <= reached, (L.CASES | L.CASES_U16) - reached


def test_the_default_passes_without_the_lookup():
    t, time, key = L.fixture(64, abi.Uint16)
    tz = L.tz_offsets()
    k = next(k for k, rec in t.placed.items() if rec[0] == J.BASE_BATCH + 2 and rec[1] < t.num_last)
    assert L.zone_offset(t, tz, k, True, "zone8") == (L.DEFAULT_ZONE, True, ["mode 0 default"]) and tz[L.DEFAULT_ZONE] != L.DEFAULT_ZONE
