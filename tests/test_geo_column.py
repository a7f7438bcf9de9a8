"""AresGeoShapeColumnRun (include/ares_extensions.h): the geofence verdict of a batch resolved once, in row space, into an
ordinary mode-2 Uint8 column.  The output — every byte of the bitmap and of the values, and the bytes the call must NOT write —
is compared with tests/geo_column_model.py (tests/geo_model.py over the identity index vector + the entry point's contract), and
the device's counters with the model's: live rows, and wavefront-chunks walked = the sum over the 1024-row tiles of
ceil(live rows / 64), which only a kernel that compacts the live rows of a tile reaches.

Inputs: every case group of tests/test_geo_semantics.py with main-table points, both ways of the filter; the row counts around
a wavefront, a workgroup and a tile; tiles with exactly 0, 1, 63, 64, 65, 255, 256, 257 and 1024 live rows, steered with a hint
column and with null points; two workgroups over five tiles and one row."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import geo_column_model as GC
import harness as H
import select_model as M
import select_runs as R
import test_abi_exports as X
import test_fused_select as F
import test_geo_semantics as S
from aresdb_amd import abi

gpu = pytest.mark.gpu
FILL = 0xA5
LIVE_PER_TILE = (0, 1, 63, 64, 65, 255, 256, 257, 1024)
INSTANCE = {1: "<1>", 2: "<2>", 3: "<4>", 4: "<4>", 5: "<8>", 8: "<8>"}


@pytest.fixture(scope="module")
def hip():
    return H.hip_backend()


def main_cases(group):
    """the group's cases whose points are a main-table column (a prefilled predicate vector has no meaning in row space)"""
    return [c for c in S.cases_of(group, joined=False) if c.joined is None and c.prefill is None]


def aligned(buf):
    return (buf.ptr + 63) // 64 * 64


def expr(dcol, functor, c):
    e = abi.FusedExpr()
    e.lhs, e.rhs = dcol.input(), M._const_input(c)
    e.arity, e.functor, e.outType = 2, functor, abi.Bool
    return e


def query(shapes, points, in_or_out, out, exprs=()):
    q = abi.GeoShapeColumn()
    q.numFilters = len(exprs)
    for k, e in enumerate(exprs):
        q.filters[k] = e
    q.shapes, q.points, q.inOrOut, q.out = shapes.struct(), points.input(), int(in_or_out), out
    return q


class Device:
    """the shapes and the point column of a case on the device"""

    def __init__(self, be, c):
        self.shapes = H.GeoShapes(be, c.lats, c.longs, c.shape, 32 * c.words)
        self.points = H.geo_column(be, c.points, valid=c.valid, starting_index=c.starting_index)

    def free(self):
        self.shapes.free()
        self.points.free()


def run(be, dev, n, in_or_out, exprs=()):
    """(the AresGeoShapeColumnBytes(n) bytes behind `out` after the call into a buffer filled with FILL, live rows and chunks
    this call added to the counters)"""
    size = be.geo_shape_column_bytes(n)
    assert size == GC.column_bytes(n)
    buf = H.Buf(be, np.full(size + 64, FILL, np.uint8))
    try:
        be.wait()
        before = be.geo_column_stats()
        s = be.geo_shape_column_run(query(dev.shapes, dev.points, in_or_out, aligned(buf), exprs), n)
        be.wait()
        after = be.geo_column_stats()
        assert after["batches"] - before["batches"] == 1 and after["rows"] - before["rows"] == n and after["declined"] == before["declined"]
        assert (s.BasePtr, s.NullsOffset, s.ValuesOffset, s.StartingIndex, s.Length, s.DataType) == \
            (aligned(buf), 0, GC.bitmap_bytes(n), 0, n, abi.Uint8)
        off = aligned(buf) - buf.ptr
        blob = buf.read(np.uint8)
        assert (blob[:off] == FILL).all() and (blob[off + size:] == FILL).all(), "written outside the output"
        return blob[off:off + size].copy(), after["live"] - before["live"], after["chunks"] - before["chunks"]
    finally:
        buf.free()


def want_bytes(values, row_valid):
    """the output over a buffer that held FILL: the bitmap's 8-byte words that hold a row, then FILL; n value bytes, then FILL"""
    n = len(values)
    bitmap, vals = GC.layout(values, row_valid)
    out = np.full(GC.column_bytes(n), FILL, np.uint8)
    words = 8 * ((n + 63) // 64)
    out[:words] = bitmap[:words]
    out[GC.bitmap_bytes(n):GC.bitmap_bytes(n) + n] = vals
    return out


def check(be, c, in_or_out, n=None, hints=(), extra=(), dev=None):
    """hints: (device column, host select_model.Col, functor, constant) — evaluated; extra: expressions the kernel ignores"""
    n = len(c.points) if n is None else n
    own = dev is None
    dev = dev or Device(be, c)
    try:
        keep = np.ones(n, bool)
        for _, col, functor, const in hints:
            keep &= M.model_filter(col, functor, const, n)
        valid = None if c.valid is None else c.valid[:n]
        values, row_valid, live = GC.expected_column(c.lats, c.longs, c.shape, c.words, c.points[:n], valid, in_or_out, keep)
        got, got_live, got_chunks = run(be, dev, n, in_or_out, [expr(d, f, k) for d, _, f, k in hints] + list(extra))
        want = want_bytes(values, row_valid)
        tag = f"{c!r} n={n} in={in_or_out}"
        bad = np.flatnonzero(got != want)
        assert not len(bad), (tag, bad[:8], got[bad[:8]], want[bad[:8]])
        assert got_live == int(live.sum()), (tag, "live rows", got_live, int(live.sum()))
        assert got_chunks == GC.chunks_walked(live), (tag, "wavefront-chunks", got_chunks, GC.chunks_walked(live))
        return values, row_valid, live
    finally:
        if own:
            dev.free()


@gpu
@pytest.mark.parametrize("group", list(S.GROUPS))
def test_every_case_group_both_ways(hip, group):
    cs = main_cases(group)
    hip.wait()
    hip.profiler_enable(True)
    try:
        seen = [0, 0]
        for c in cs:
            for in_or_out in (True, False):
                _, row_valid, _ = check(hip, c, in_or_out)
                seen[0] += int(row_valid.sum())
                seen[1] += int((~row_valid).sum())
        hip.wait()
        ran = S.kernel_names(hip)
    finally:
        hip.profiler_enable(False)
    print(f"{group}: {len(cs)} cases x 2; {seen[0]} valid rows, {seen[1]} null rows; {ran}")
    assert len(cs) >= 2 and seen[0] > 0 and seen[1] > 0
    for inst in set(INSTANCE.values()):
        assert ran.get("geo_shape_column_kernel" + inst, 0) == 2 * sum(INSTANCE[c.words] == inst and len(c.points) > 0 for c in cs), (inst, ran)
    assert set(ran) <= {"geo_shape_column_kernel" + i for i in INSTANCE.values()}, ran
    if group == "words":
        assert all(ran.get("geo_shape_column_kernel" + i, 0) > 0 for i in ("<1>", "<2>", "<4>", "<8>")), ran


def pattern_case(n, words=1):
    """a square, the 64-point pattern of test_geo_semantics (vertices, edges, inside, outside) repeated, nulls every ninth row;
    the validity bitmap starts at bit 3"""
    c = S.Case(f"pattern_{n}", *S.batch(S.square(0, 2.0)), words, np.resize(S.PATTERN, (n, 2)), valid=np.resize(S.PATTERN_VALID, n))
    assert c.starting_index == 3
    return c


@pytest.fixture(scope="module")
def big(hip):
    c = pattern_case(5 * 1024 + 1)
    dev = Device(hip, c)
    yield c, dev
    dev.free()


@gpu
@pytest.mark.parametrize("n", S.ENTRY_COUNTS)
def test_row_counts_the_bitmap_tail_and_the_partial_tile(hip, big, n):
    """n rows of a longer column with a bitmap at StartingIndex 3: bits at or past n inside the last word are zero, nothing
    behind that word and nothing behind value n is written"""
    c, dev = big
    for in_or_out in (True, False):
        values, row_valid, _ = check(hip, c, in_or_out, n=n, dev=dev)
        assert n < 64 or (row_valid.any() and not row_valid.all())


def steered_case():
    """one tile per entry of LIVE_PER_TILE: tiles at even positions lose their other rows to a hint column (h == 1 keeps),
    tiles at odd positions to null points; the live rows lie at seeded random places of the tile"""
    rng = np.random.default_rng(1024)
    n = 1024 * len(LIVE_PER_TILE)
    valid, h = np.ones(n, bool), np.ones(n, np.uint32)
    for t, live in enumerate(LIVE_PER_TILE):
        dead = t * 1024 + rng.permutation(1024)[live:]
        if t % 2 == 0:
            h[dead] = 0
        else:
            valid[dead] = False
    c = S.Case("steered", *S.batch(S.square(0, 2.0), S.square(1, 1.0, cx=5.0)), 1, np.resize(S.PATTERN, (n, 2)), valid=valid)
    return c, M.Col(abi.Uint32, h)


@gpu
def test_live_rows_per_tile_at_the_chunk_boundaries(hip):
    c, hcol = steered_case()
    dcol = hcol.upload(hip)
    try:
        for in_or_out in (True, False):
            _, _, live = check(hip, c, in_or_out, hints=[(dcol, hcol, abi.Equal, 1)])
            assert tuple(int(live[t:t + 1024].sum()) for t in range(0, c.n, 1024)) == LIVE_PER_TILE
            assert GC.chunks_walked(live) == sum((x + 63) // 64 for x in LIVE_PER_TILE) < (int(live.sum()) + 63) // 64 + len(LIVE_PER_TILE)
    finally:
        dcol.free()


@gpu
def test_hints_over_narrow_and_nullable_columns(hip, big):
    """the three hints of select_model.MIXED_FILTERS: two comparisons of a Uint32 column, one of a Uint8 column, nulls in both"""
    c, dev = big
    n = 4097
    cols = M.mixed_columns(n)
    dcols = {k: cols[k].upload(hip) for k in ("ts", "status")}
    try:
        hints = [(dcols[name], cols[name], f, k) for name, f, k in M.MIXED_FILTERS]
        _, _, live = check(hip, c, True, n=n, hints=hints, dev=dev)
        _, _, every = check(hip, c, True, n=n, dev=dev)
        assert 0 < live.sum() < every.sum()
    finally:
        for d in dcols.values():
            d.free()


@gpu
def test_a_hint_the_kernel_cannot_evaluate_is_ignored(hip, big):
    """a run-length column, a wide column and a column shorter than the batch: nothing is pruned (evaluated, each would kill rows)"""
    c, dev = big
    n = 1025
    rng = np.random.default_rng(3)
    lens = R.run_lengths(rng, n, 40)
    rl = R.run_col(abi.Uint32, R.values_of(rng, abi.Uint32, len(lens)), np.ones(len(lens), bool), lens)[0].upload(hip)
    wide = M.Col(abi.Int64, np.arange(n, dtype=np.int64)).upload(hip)
    short = M.Col(abi.Uint32, np.ones(n - 1, np.uint32)).upload(hip)
    try:
        extra = [expr(rl, abi.LessThan, 0), expr(wide, abi.LessThan, 0), expr(short, abi.Equal, 0)]
        _, _, live = check(hip, c, True, n=n, extra=extra, dev=dev)
        assert live.sum() == c.valid[:n].sum()
    finally:
        for d in (rl, wide, short):
            d.free()


@gpu
def test_two_workgroups_over_five_tiles_and_one_row(hip, big):
    """the second and third round of the grid-stride loop, the last of them a tile of one row"""
    c, dev = big
    assert c.n == 5 * 1024 + 1
    with F._Env(hip, ARES_GEO_COLUMN_GRID="2"):
        for in_or_out in (True, False):
            check(hip, c, in_or_out, dev=dev)


@gpu
def test_total_words_outside_1_to_8_is_the_error_of_geo_batch_intersects(hip, big):
    c, dev = big
    buf = H.Buf(hip, np.full(GC.column_bytes(100) + 64, FILL, np.uint8))
    try:
        for words in (0, 9):
            q = query(dev.shapes, dev.points, True, aligned(buf))
            q.shapes.TotalWords = words
            with pytest.raises(abi.AresError, match="geo intersection supports up to 256 shapes"):
                hip.geo_shape_column_run(q, 100)
        hip.wait()
        assert (buf.read(np.uint8) == FILL).all()
    finally:
        buf.free()


def _declined(be, q, buf, n=100):
    be.wait()
    be.profiler_enable(True)
    try:
        with pytest.raises(abi.AresError, match="^not fusable"):
            be.geo_shape_column_run(q, n)
        be.wait()
        assert be.profiler_report() == {}, "a declined shape launched a kernel"
    finally:
        be.profiler_enable(False)
    assert (buf.read(np.uint8) == FILL).all(), "a declined shape wrote"


@gpu
def test_declined_shapes_launch_nothing_and_write_nothing(hip):
    n = 100
    c = pattern_case(n)
    dev = Device(hip, c)
    buf = H.Buf(hip, np.full(GC.column_bytes(n) + 128, FILL, np.uint8))
    out = aligned(buf)
    absent = H.Column(hip, abi.GeoPoint)  # mode 0
    counts = np.arange(0, n + 1, 10, dtype=np.uint32)
    rl = H.Column(hip, abi.GeoPoint, raw_values=np.float32(c.points[:10]).tobytes(), valid=np.ones(10, bool), counts=counts)
    short = H.geo_column(hip, c.points[:n - 1], valid=c.valid[:n - 1], starting_index=3)
    try:
        before = hip.geo_column_stats()
        for points in (absent, rl, short):
            _declined(hip, query(dev.shapes, points, True, out), buf)
        _declined(hip, query(dev.shapes, dev.points, True, None), buf)
        _declined(hip, query(dev.shapes, dev.points, True, out + 32), buf)
        with F._Env(hip, ARES_GEO_COLUMN="0"):
            _declined(hip, query(dev.shapes, dev.points, True, out), buf)
        hip.wait()
        after = hip.geo_column_stats()
        assert after["declined"] - before["declined"] == 6
        assert {k: after[k] for k in ("batches", "rows", "live", "chunks")} == {k: before[k] for k in ("batches", "rows", "live", "chunks")}
        check(hip, c, True, dev=dev)  # the same query once the switch is back
    finally:
        for d in (absent, rl, short, dev, buf):
            d.free()


@gpu
def test_zero_rows_launch_nothing(hip, big):
    c, dev = big
    buf = H.Buf(hip, nbytes=128)
    hip.wait()
    hip.profiler_enable(True)
    try:
        s = hip.geo_shape_column_run(query(dev.shapes, dev.points, True, aligned(buf)), 0)
        hip.wait()
        assert hip.profiler_report() == {} and s.Length == 0 and hip.geo_shape_column_bytes(0) == 0
    finally:
        hip.profiler_enable(False)
        buf.free()


# ---- the boundary: no GPU needed, nothing is called ----------------------------------------------------------------------
PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "ares_extensions.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
int main(void) {
  printf("AresGeoShapeColumn %zu\n", sizeof(AresGeoShapeColumn));
  F(AresGeoShapeColumn, numFilters); F(AresGeoShapeColumn, filters); F(AresGeoShapeColumn, shapes); F(AresGeoShapeColumn, points);
  F(AresGeoShapeColumn, inOrOut); F(AresGeoShapeColumn, out);
  return 0;
}
"""


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(abi.REPO_ROOT, "include"), str(src), "-o", str(exe)])
    seen = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert len(seen) == 7
    for name, value in seen.items():
        _, _, member = name.partition(".")
        want = getattr(abi.GeoShapeColumn, member).offset if member else C.sizeof(abi.GeoShapeColumn)
        assert int(value) == want, name
    assert {"AresGeoShapeColumn." + f[0] for f in abi.GeoShapeColumn._fields_} <= set(seen)


def test_the_new_symbols_are_declared_and_exported():
    algo, _ = X._built()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(abi.REPO_ROOT, "include", "ares_extensions.h")).read(), flags=re.S)
    declared = set(re.findall(r"^(?:void|size_t|CGoCallResHandle)\s+(\w+)\s*\(", src, flags=re.M))
    lib = C.CDLL(algo, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    for name in ("AresGeoShapeColumnRun", "AresGeoShapeColumnBytes", "AresGeoShapeColumnStats"):
        assert name in declared and getattr(lib, name) is not None
    driver = C.CDLL(os.path.join(os.path.dirname(algo), "libaresdriver.so"), mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert driver.AresQuerySetGeoColumn is not None


def test_the_steered_tiles_hold_what_they_are_meant_to():
    c, hcol = steered_case()
    live = c.valid & (hcol.values == 1)
    assert tuple(int(live[t:t + 1024].sum()) for t in range(0, c.n, 1024)) == LIVE_PER_TILE
    assert (~c.valid).any() and (hcol.values == 0).any()
