"""AresLocalTimeColumnRun (include/ares_extensions.h): time + the UTC offset of the joined zone, resolved once per batch into an
ordinary mode-2 column.  The output is compared byte for byte with the numpy model of tests/local_time_model.py (a dictionary
join, not a probe) and with what the per-node sequence — HashLookup, then BinaryTransform(Plus, time, the zone column with its
TimezoneLookup) into a dimension slot — leaves on the same library, in both flavours (ARES_LOCAL_TIME=direct | probe).

Rows: 1, 63, 64, 65 (wavefront and bitmap-word edges), 4097 (sixteen whole 256-row chunks of the direct flavour and a tail), and
1500 rows on two workgroups and on one (the second round of either flavour's grid-stride loop)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import harness as H
import local_time_model as L
import select_model as M
import select_runs as R
import test_fused_select as F
import test_local_time_model as TM
from aresdb_amd import abi

gpu = pytest.mark.gpu
ROWS = [1, 63, 64, 65, 4097]
HINTS = M.MIXED_FILTERS  # two comparisons of a Uint32 column and one of a Uint8 column, nulls in both
NARROW = [abi.Uint8, abi.Int8, abi.Int16, abi.Uint16]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def hip():
    return H.hip_backend()


class Batch:
    """a table, the time and key columns of one batch and the columns the hints read, on the device"""

    def __init__(self, be, n, key_dtype=abi.Uint16, key_bytes=None, time_dtype=abi.Uint32, default=True, **kw):
        self.be, self.n = be, n
        self.table, self.time, self.key = L.fixture(n, key_dtype, key_bytes, time_dtype, default=default, **kw)
        self.cols = M.mixed_columns(n)
        self.dcols = {k: c.upload(be) for k, c in self.cols.items()}
        self.dtime, self.dkey, self.dtable = self.time.upload(be), self.key.upload(be), self.table.upload(be)
        self.tz = TM.Tz(be, L.tz_offsets())
        self.models = {}

    def model(self, zone, n):
        if (zone, n) not in self.models:
            self.models[zone, n] = L.local_time(self.table, self.tz.data, self.time, self.key, zone, n)[:2]
        return self.models[zone, n]

    def free(self):
        for c in list(self.dcols.values()) + [self.dtime, self.dkey, self.dtable, self.tz]:
            c.free()


def query(b, zone, out, hints=(), out_type=abi.Uint32):
    q = abi.LocalTimeColumn()
    q.numFilters = len(hints)
    for k, (name, functor, c) in enumerate(hints):
        e = q.filters[k]
        e.lhs, e.rhs = b.dcols[name].input(), M._const_input(c)
        e.arity, e.functor, e.outType = 2, functor, abi.Bool
    q.time = b.dtime.input()
    q.join.key, q.join.index = b.dkey.input(), b.dtable.index_struct()
    q.zone = L.zone_input(b.dtable, zone, None, b.tz.ptr, len(b.tz.data))
    q.outType, q.out = out_type, out
    return q


def aligned(buf):
    return (buf.ptr + 63) // 64 * 64


def bitmap_bytes(n):
    return ((n + 7) // 8 + 63) // 64 * 64


def run(b, n, zone, hints=(), out_type=abi.Uint32):
    """(bitmap bytes of the written words, value bytes, keys probed by the call, direct?): everything around them is checked to
    be untouched"""
    be = b.be
    size = be.join_column_bytes(n, abi.Uint32)
    assert size == bitmap_bytes(n) + (4 * n + 63) // 64 * 64
    buf = H.Buf(be, np.full(size + 128, SENTINEL, np.uint8))
    try:
        be.wait()
        before = be.local_time_column_stats()
        s = be.local_time_column_run(query(b, zone, aligned(buf), hints, out_type), n)
        be.wait()
        after = be.local_time_column_stats()
        assert after["batches"] - before["batches"] == 1 and after["rows"] - before["rows"] == n and after["declined"] == before["declined"]
        assert (s.BasePtr, s.NullsOffset, s.ValuesOffset, s.StartingIndex, s.Length, s.DataType) == (aligned(buf), 0, bitmap_bytes(n), 0, n, out_type)
        off = aligned(buf) - buf.ptr
        blob = buf.read(np.uint8)
        words = 8 * ((n + 63) // 64)
        untouched = np.concatenate([blob[:off], blob[off + words:off + bitmap_bytes(n)], blob[off + bitmap_bytes(n) + 4 * n:]])
        assert (untouched == SENTINEL).all(), "bytes outside the written words and values were written"
        return (blob[off:off + words].copy(), blob[off + bitmap_bytes(n):off + bitmap_bytes(n) + 4 * n].copy(),
                after["probed"] - before["probed"], after["direct"] - before["direct"] == 1)
    finally:
        buf.free()


def check(b, n, zone, hints=(), direct=None, out_type=abi.Uint32):
    """against the model; rows that fail a hint are (0, null) in the probe flavour and not probed.  Returns keys probed."""
    bitmap, values, probed, was_direct = run(b, n, zone, hints, out_type)
    want_values, want_valid = b.model(zone, n)
    keep = np.ones(n, bool)
    if not was_direct:
        for name, functor, c in hints:
            keep &= M.model_filter(b.cols[name], functor, c, n)
    want_bitmap, want_bytes = L.column_bytes(np.where(keep, want_values, 0).astype(np.uint32), want_valid & keep, n)
    assert np.array_equal(bitmap, want_bitmap[:len(bitmap)]), "validity bitmap"  # (bits at or past n in the last word: 0)
    assert np.array_equal(values, want_bytes), "values"
    if direct is not None:
        assert was_direct == direct
    if was_direct:
        assert probed == (256 if abi.DATA_TYPE_BYTES[b.key.dtype] == 1 else 65536)
    else:
        assert probed == int((keep & M._valid(b.key, n)).sum())
    return probed


def both(b, n, zone, hints=()):
    for flavour in ("direct", "probe"):
        with F._Env(b.be, ARES_LOCAL_TIME=flavour):
            check(b, n, zone, hints, direct=flavour == "direct")


@pytest.fixture(scope="module")
def big(hip):
    b = Batch(hip, 4097)
    yield b
    b.free()


@pytest.mark.parametrize("n", ROWS)
@gpu
def test_rows_at_the_wave_chunk_and_word_edges(big, n):
    both(big, n, "zone8")
    both(big, n, "zone16", HINTS)


@gpu
def test_the_second_round_of_the_grid_stride_loops(big):
    for grid in ("2", "1"):  # (two workgroups: three rounds of the probe flavour; one: two of the direct flavour's 1024-row tiles)
        with F._Env(big.be, ARES_LOCAL_TIME_GRID=grid):
            both(big, 1500, "zone16", HINTS[:1])


@pytest.mark.parametrize("key_bytes", [None, 4], ids=["width", "keyBytes4"])
@pytest.mark.parametrize("key_dtype", NARROW)
@gpu
def test_narrow_keys_in_both_flavours(hip, key_dtype, key_bytes):
    """negative keys of the signed types are sign-extended before keyBytes of them are kept, as HashLookup widens them"""
    n = 1100
    b = Batch(hip, n, key_dtype, key_bytes, default=key_bytes is None)
    try:
        want_valid = b.model("zone16", n)[1]
        if key_dtype in (abi.Int8, abi.Int16):
            assert (b.key.values[:n][want_valid] < 0).any()
        both(b, n, "zone16", HINTS[2:])
        both(b, 300, "zone8")
    finally:
        b.free()


@gpu
def test_a_key_column_wider_than_the_index_key(hip):
    """a Uint16 column over an index of 1-byte keys: the low byte is the key"""
    b = Batch(hip, 700, abi.Uint16, 1)
    try:
        both(b, 700, "zone8")
    finally:
        b.free()


@pytest.mark.parametrize("key_dtype", [abi.Uint32, abi.Int64, abi.UUID])
@gpu
def test_wide_keys_take_the_probe_flavour(hip, key_dtype):
    n = 1100
    b = Batch(hip, n, key_dtype, time_dtype=abi.Int32)
    try:
        for flavour in ("direct", "probe", None):  # (forced where applicable: not here)
            with F._Env(hip, **({"ARES_LOCAL_TIME": flavour} if flavour else {})):
                assert check(b, n, "zone16", HINTS, direct=False, out_type=abi.Int32) > 0
    finally:
        b.free()


@pytest.mark.parametrize("time_valid,key_valid", [(False, False), (True, False), (False, True)])
@gpu
def test_mode_1_time_and_key_columns(hip, time_valid, key_valid):
    b = Batch(hip, 1100, abi.Int16, time_valid=time_valid, key_valid=key_valid)
    try:
        assert (b.dtime.vp.ValuesOffset != 0) == time_valid and (b.dkey.vp.ValuesOffset != 0) == key_valid
        both(b, 1100, "zone8")
    finally:
        b.free()


@pytest.mark.parametrize("time_start,key_start", [(0, 0), (5, 7), (7, 1)])
@gpu
def test_starting_indexes_of_the_validity_bitmaps(hip, time_start, key_start):
    b = Batch(hip, 1100, abi.Uint8, time_start=time_start, key_start=key_start)
    try:
        assert (b.dtime.vp.StartingIndex, b.dkey.vp.StartingIndex) == (time_start, key_start)
        both(b, 1100, "zone16")
    finally:
        b.free()


@gpu
def test_the_default_choice(hip):
    """direct when the key is narrow and the batch has at least as many rows as the key has values"""
    b8, b16 = Batch(hip, 300, abi.Uint8), Batch(hip, 4097, abi.Uint16)
    try:
        check(b8, 255, "zone8", HINTS, direct=False)
        check(b8, 256, "zone8", HINTS, direct=True)
        check(b16, 4097, "zone16", HINTS, direct=False)
    finally:
        b8.free()
        b16.free()


@gpu
def test_a_hint_that_kills_every_row(big):
    hint = [("ts", abi.GreaterThan, 10 ** 6)]
    with F._Env(big.be, ARES_LOCAL_TIME="probe"):
        bitmap, values, probed, _ = run(big, 4097, "zone8", hint)
        assert probed == 0 and not bitmap.any() and not values.any()
    with F._Env(big.be, ARES_LOCAL_TIME="direct"):
        check(big, 4097, "zone8", hint, direct=True)  # (hints are not evaluated: no row is pruned)


@gpu
def test_an_unevaluable_hint_is_ignored(big):
    n, be = 1100, big.be
    rng = np.random.default_rng(3)
    lens = R.run_lengths(rng, n, 40)
    big.dcols["rl"] = R.run_col(abi.Uint32, R.values_of(rng, abi.Uint32, len(lens)), np.ones(len(lens), bool), lens)[0].upload(be)
    try:
        with F._Env(be, ARES_LOCAL_TIME="probe"):
            q = query(big, "zone8", None, HINTS[:1])
            q.numFilters = 3
            for k, name in ((1, "rl"), (2, "big")):  # (evaluated, they would kill every row)
                e = q.filters[k]
                e.lhs, e.rhs = big.dcols[name].input(), M._const_input(0)
                e.arity, e.functor, e.outType = 2, abi.LessThan, abi.Bool
            buf = H.Buf(be, nbytes=be.join_column_bytes(n, abi.Uint32) + 64)
            q.out = aligned(buf)
            before = be.local_time_column_stats()
            be.local_time_column_run(q, n)
            be.wait()
            probed = be.local_time_column_stats()["probed"] - before["probed"]
            buf.free()
            assert probed == check(big, n, "zone8", HINTS[:1], direct=False)
    finally:
        big.dcols.pop("rl").free()


@pytest.mark.parametrize("flavour", ["direct", "probe"])
@pytest.mark.parametrize("n", [257, 4097])
@gpu
def test_the_output_is_what_the_per_node_sequence_leaves(big, n, flavour):
    """HashLookup + BinaryTransform(Plus, time, zone with its TimezoneLookup) into a dimension slot on the same library"""
    be = big.be
    with F._Env(be, ARES_LOCAL_TIME=flavour):
        for zone, out_type in (("zone8", abi.Uint32), ("zone16", abi.Int32)):
            bitmap, values, _, _ = run(big, n, zone, out_type=out_type)
            want_values, want_valid = TM.per_node(be, big.dtable, big.dtime, big.dkey, zone, big.tz, n, out_type)
            assert np.array_equal(np.unpackbits(bitmap, bitorder="little")[:n], want_valid)
            assert np.array_equal(values.view(np.uint32), want_values)


def _declined(be, q, n=100):
    be.wait()
    be.profiler_enable(True)
    try:
        with pytest.raises(abi.AresError, match="^not fusable"):
            be.local_time_column_run(q, n)
        be.wait()
        assert be.profiler_report() == {}, "a declined shape launched a kernel"
    finally:
        be.profiler_enable(False)


@gpu
def test_declined_shapes_launch_nothing_and_write_nothing(hip):
    n = 100
    b = Batch(hip, n)
    rng = np.random.default_rng(3)
    absent = M.Col(abi.Uint32, None, default=5).upload(hip)
    absent16 = M.Col(abi.Uint16, None, default=5).upload(hip)
    rl = R.run_col(abi.Uint32, rng.integers(0, 9, 10), np.ones(10, bool), np.full(10, 10))[0].upload(hip)
    rl16 = R.run_col(abi.Uint16, rng.integers(0, 9, 10), np.ones(10, bool), np.full(10, 10))[0].upload(hip)
    size = hip.join_column_bytes(n, abi.Uint32)
    buf = H.Buf(hip, np.full(size + 128, SENTINEL, np.uint8))
    out = aligned(buf)
    try:
        before = hip.local_time_column_stats()
        shapes = []

        def shape(change):
            q = query(b, "zone8", out, HINTS)
            change(q)
            shapes.append(q)

        def zone_field(name, value):
            return lambda q: setattr(q.zone.Vector.ForeignVP, name, value)

        shape(zone_field("TimezoneLookup", None))
        for dtype in (abi.Uint32, abi.Int16, abi.Bool):
            shape(zone_field("DataType", dtype))
        shape(lambda q: setattr(q, "zone", b.dkey.input()))  # no foreign column
        for dtype in (abi.Float32, abi.Uint16, abi.Int64):
            shape(lambda q, dtype=dtype: setattr(q.time.Vector.VP, "DataType", dtype))
        shape(lambda q: setattr(q, "outType", abi.Float32))
        shape(lambda q: setattr(q, "time", absent.input()))           # a mode-0 time column
        shape(lambda q: setattr(q, "time", rl.input()))               # a run-length time column
        shape(lambda q: setattr(q.time.Vector.VP, "Length", n - 1))   # shorter than the batch
        shape(lambda q: setattr(q.join, "key", absent16.input()))     # the same for the key
        shape(lambda q: setattr(q.join, "key", rl16.input()))
        shape(lambda q: setattr(q.join.key.Vector.VP, "Length", n - 1))
        for field, value in (("keyBytes", 0), ("keyBytes", 17), ("numHashes", 5), ("numBuckets", 0), ("buckets", None)):
            shape(lambda q, field=field, value=value: setattr(q.join.index, field, value))
        shape(lambda q: setattr(q, "out", None))
        shape(lambda q: setattr(q, "out", out + 32))
        for q in shapes:
            _declined(hip, q)
        with F._Env(hip, ARES_LOCAL_TIME="0"):
            _declined(hip, query(b, "zone8", out, HINTS))
        hip.wait()
        after = hip.local_time_column_stats()
        assert after["declined"] - before["declined"] == len(shapes) + 1 == 23
        assert {k: after[k] for k in ("batches", "rows", "probed", "direct")} == {k: before[k] for k in ("batches", "rows", "probed", "direct")}
        assert (buf.read(np.uint8) == SENTINEL).all(), "a declined shape wrote its output"
        check(b, n, "zone8", HINTS)  # the same plan once the switch is back
    finally:
        for x in (absent, absent16, rl, rl16, buf):
            x.free()
        b.free()


@gpu
def test_zero_rows_launch_nothing(big):
    be = big.be
    out = H.Buf(be, nbytes=128)
    be.wait()
    be.profiler_enable(True)
    try:
        for flavour in ("direct", "probe"):
            with F._Env(be, ARES_LOCAL_TIME=flavour):
                s = be.local_time_column_run(query(big, "zone8", aligned(out)), 0)
        be.wait()
        assert be.profiler_report() == {} and s.Length == 0
    finally:
        be.profiler_enable(False)
        out.free()


# ---- the boundary: no GPU needed, nothing is called ----------------------------------------------------------------------
PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "ares_extensions.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
int main(void) {
  printf("AresLocalTimeColumn %zu\n", sizeof(AresLocalTimeColumn));
  F(AresLocalTimeColumn, numFilters); F(AresLocalTimeColumn, filters); F(AresLocalTimeColumn, time); F(AresLocalTimeColumn, join);
  F(AresLocalTimeColumn, zone); F(AresLocalTimeColumn, outType); F(AresLocalTimeColumn, out);
  return 0;
}
"""


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(abi.REPO_ROOT, "include"), str(src), "-o", str(exe)])
    seen = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert len(seen) == 8
    for name, value in seen.items():
        _, _, member = name.partition(".")
        want = getattr(abi.LocalTimeColumn, member).offset if member else C.sizeof(abi.LocalTimeColumn)
        assert int(value) == want, name
    assert {"AresLocalTimeColumn." + f[0] for f in abi.LocalTimeColumn._fields_} <= set(seen)


def test_the_new_symbols_are_declared_and_exported():
    import re
    import test_abi_exports as X
    algo, _ = X._built()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(abi.REPO_ROOT, "include", "ares_extensions.h")).read(), flags=re.S)
    declared = set(re.findall(r"^(?:void|size_t|CGoCallResHandle)\s+(\w+)\s*\(", src, flags=re.M))
    lib = C.CDLL(algo, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    for name in ("AresLocalTimeColumnRun", "AresLocalTimeColumnStats"):
        assert name in declared and getattr(lib, name) is not None
