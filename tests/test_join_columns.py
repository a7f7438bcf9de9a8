"""AresJoinColumnsRun (include/ares_extensions.h): the joined columns of a batch resolved once, in row space, into ordinary
mode-2 columns.  Every output is compared byte for byte with the numpy model of tests/select_join_model.py (Table.joined: a
dictionary from key bytes to record, not a probe), the probe count with the model's exactly, and the returned slices — handed
back to the per-node calls as main-table columns — with the per-node join sequence on the same library.

Rows: 1, 63, 64, 65 (wavefront and bitmap-word edges), 255, 256, 257 (workgroup edges), 4097, and 1025 rows on two workgroups
(the second round of the grid-stride loop)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import harness as H
import select_join_model as J
import select_model as M
import select_runs as R
import test_abi_exports as X
import test_fused_select as F
from aresdb_amd import abi

gpu = pytest.mark.gpu
ROWS = [1, 63, 64, 65, 255, 256, 257, 4097]
NAMES = ["region", "off", "tz", "rate"]  # widths 4 / 2 / 1 and Float32
HINTS = M.MIXED_FILTERS                  # two comparisons of a Uint32 column and one of a Uint8 column, nulls in both


@pytest.fixture(scope="module")
def hip():
    return H.hip_backend()


class Batch:
    """the fact columns (select_model.mixed_columns + the key column "k0", validity bitmap at StartingIndex 3) and the table of
    one batch, on the device"""

    def __init__(self, be, n, key_dtype=abi.Uint32, **kw):
        kw.setdefault("misses", 0.10)
        self.be, self.n = be, n
        self.table, key = J.fixture(n, key_dtype, **kw)
        self.cols = M.mixed_columns(n)
        self.cols["k0"] = M.Col(key.dtype, key.values, key.valid, starting_index=3)
        self.dcols = {k: c.upload(be) for k, c in self.cols.items()}
        self.dtable = self.table.upload(be)

    def free(self):
        for c in list(self.dcols.values()) + [self.dtable]:
            c.free()


def expr(dcol, functor, c):
    e = abi.FusedExpr()
    e.lhs, e.rhs = dcol.input(), M._const_input(c)
    e.arity, e.functor, e.outType = 2, functor, abi.Bool
    return e


def query(b, names, outs, hints=(), key="k0", exprs=()):
    q = abi.JoinColumns()
    es = [expr(b.dcols[name], functor, c) for name, functor, c in hints] + list(exprs)
    q.numFilters = len(es)
    for k, e in enumerate(es):
        q.filters[k] = e
    q.join.key, q.join.index = b.dcols[key].input(), b.dtable.index_struct()
    q.numColumns = len(names)
    for c, (name, out) in enumerate(zip(names[:4], outs)):
        q.columns[c].column, q.columns[c].out = b.dtable.input(name), out
    return q


def aligned(buf):
    return (buf.ptr + 63) // 64 * 64


def bitmap_bytes(n):
    return ((n + 7) // 8 + 63) // 64 * 64


def run(b, n, names, hints=(), exprs=()):
    """([(bitmap bytes of the written words, value bytes) per column], slices, buffers, keys probed by this call)"""
    be = b.be
    bufs = [H.Buf(be, nbytes=be.join_column_bytes(n, b.table.COLUMNS[name]) + 64) for name in names]
    be.wait()
    before = be.join_column_stats()
    try:
        slices = be.join_columns_run(query(b, names, [aligned(x) for x in bufs], hints, exprs=exprs), n)
    except Exception:
        for x in bufs:
            x.free()
        raise
    be.wait()
    after = be.join_column_stats()
    assert after["batches"] - before["batches"] == 1 and after["rows"] - before["rows"] == n and after["declined"] == before["declined"]
    outs = []
    for name, x, s in zip(names, bufs, slices):
        dtype = b.table.COLUMNS[name]
        width = abi.DATA_TYPE_BYTES[dtype]
        assert be.join_column_bytes(n, dtype) == bitmap_bytes(n) + (n * width + 63) // 64 * 64
        assert (s.BasePtr, s.NullsOffset, s.ValuesOffset, s.StartingIndex, s.Length, s.DataType) == \
            (aligned(x), 0, bitmap_bytes(n), 0, n, dtype)
        want_default = b.dtable.batches[name][2].vp.DefaultValue
        assert bytes(s.DefaultValue) == bytes(want_default)
        off = aligned(x) - x.ptr
        blob = x.read(np.uint8)
        outs.append((blob[off:off + bitmap_bytes(n)].copy(), blob[off + bitmap_bytes(n):off + bitmap_bytes(n) + n * width].copy()))
    return outs, slices, bufs, after["probed"] - before["probed"]


def model(b, n, names, hints=()):
    """([(bitmap bytes, value bytes)], keys probed): rows that fail a hint are (0, null) and are not probed"""
    keep = np.ones(n, bool)
    for name, functor, c in hints:
        keep &= M.model_filter(b.cols[name], functor, c, n)
    key = b.cols["k0"]
    keys, key_valid = J.key_bytes_of(key, n, b.table.key_bytes), M._valid(key, n)
    outs = []
    for name in names:
        col = b.table.joined(keys, key_valid, name)
        values = np.where(keep, col.values, np.zeros(1, col.values.dtype))
        bits = np.zeros(bitmap_bytes(n) * 8, bool)  # (tail bits of the last word, and the padding, are zero)
        bits[:n] = col.valid & keep
        outs.append((np.packbits(bits, bitorder="little"), values.astype(col.values.dtype).view(np.uint8)))
    return outs, int((keep & key_valid).sum())


def check(b, n, names, hints=()):
    got, slices, bufs, probed = run(b, n, names, hints)
    want, want_probed = model(b, n, names, hints)
    try:
        for name, (gb, gv), (wb, wv) in zip(names, got, want):
            assert np.array_equal(gb, wb), (name, "validity bitmap")
            assert np.array_equal(gv, wv), (name, "values")
        assert probed == want_probed
    finally:
        for x in bufs:
            x.free()
    return probed


@pytest.fixture(scope="module")
def big(hip):
    b = Batch(hip, 4097)
    yield b
    b.free()


@pytest.mark.parametrize("n", ROWS)
@gpu
def test_rows_at_the_wave_workgroup_and_word_edges(big, n):
    assert (big.table.stash_signatures() != 0).any()
    check(big, n, NAMES)
    check(big, n, NAMES[:1], HINTS)


@gpu
def test_the_second_round_of_the_grid_stride_loop(big):
    with F._Env(big.be, ARES_JOIN_COLUMNS_GRID="2"):
        check(big, 1025, NAMES, HINTS[:1])


@pytest.mark.parametrize("key_dtype", [abi.Uint32, abi.Uint16, abi.Uint8, abi.Int64, abi.UUID])
@gpu
def test_every_key_type(hip, key_dtype):
    n = 257
    b = Batch(hip, n, key_dtype)
    try:
        assert b.cols["k0"].starting_index == 3 and not b.cols["k0"].valid.all()
        assert check(b, n, NAMES, HINTS[2:]) > 0
    finally:
        b.free()


@pytest.mark.parametrize("geometry", [dict(num_hashes=0), dict(num_hashes=4), dict(num_buckets=1, nkeys=11), dict(default=False)])
@gpu
def test_index_geometries_and_a_table_without_defaults(hip, geometry):
    """numHashes 0: every key lies in the stash or nowhere; numBuckets 1; a table whose mode-0 batch has no default"""
    n = 257
    b = Batch(hip, n, **geometry)
    try:
        check(b, n, NAMES)
        for count in (1, 2, 3):
            check(b, n, NAMES[:count], HINTS)
    finally:
        b.free()


@gpu
def test_the_pair_that_shares_bucket_and_signature_is_found(big):
    """both keys of place_pair occur among the fact rows and resolve to their own records"""
    t = big.table
    k1, k2 = t.used[-2], t.used[-1]
    keys = J.key_bytes_of(big.cols["k0"], big.n, t.key_bytes)
    assert t.placed[k1] != t.placed[k2] and k1 in keys and k2 in keys
    check(big, big.n, NAMES[:2])


@gpu
def test_a_hint_that_kills_every_row(big):
    n = 4097
    got, _, bufs, probed = run(big, n, NAMES, [("ts", abi.GreaterThan, 10 ** 6)])
    for x in bufs:
        x.free()
    assert probed == 0
    for bitmap, values in got:
        assert not bitmap.any() and not values.any()


@gpu
def test_an_unevaluable_hint_changes_nothing_but_the_probe_count(big):
    """a run-length column and a wide column: ignored — the outputs are those of the evaluated hints alone"""
    n, be = 1025, big.be
    rng = np.random.default_rng(3)
    lens = R.run_lengths(rng, n, 40)
    rl = R.run_col(abi.Uint32, R.values_of(rng, abi.Uint32, len(lens)), np.ones(len(lens), bool), lens)[0].upload(be)
    try:
        none, _, bufs0, probed_none = run(big, n, NAMES)
        base, _, bufs1, probed_base = run(big, n, NAMES, HINTS[:1])
        unevaluable = [expr(rl, abi.LessThan, 0), expr(big.dcols["big"], abi.LessThan, 0)]  # (evaluated, they would kill rows)
        only, _, bufs2, probed_only = run(big, n, NAMES, exprs=unevaluable)
        both, _, bufs3, probed_both = run(big, n, NAMES, HINTS[:1], exprs=unevaluable)
        for x in bufs0 + bufs1 + bufs2 + bufs3:
            x.free()
        want_none, want_base = model(big, n, NAMES), model(big, n, NAMES, HINTS[:1])
        assert probed_only == probed_none == want_none[1] and probed_both == probed_base == want_base[1] < probed_none
        for a, b_, w in ((only, none, want_none[0]), (both, base, want_base[0])):
            for (ab, av), (bb, bv), (wb, wv) in zip(a, b_, w):
                assert np.array_equal(ab, bb) and np.array_equal(av, bv) and np.array_equal(ab, wb) and np.array_equal(av, wv)
    finally:
        rl.free()


class _Slice:
    """a returned slice as a main-table column of the per-node calls"""

    def __init__(self, vp):
        self.vp = vp

    def input(self):
        iv = abi.InputVector()
        iv.Vector.VP = self.vp
        iv.Type = abi.VectorPartyInput
        return iv


@pytest.mark.parametrize("n", [257, 4097])
@gpu
def test_the_slices_read_as_the_per_node_join_sequence_reads(big, n):
    """UnaryTransform / BinaryTransform / BinaryFilter over the returned slices against HashLookup + the same calls over the
    foreign column with record ids: survivor count and every dimension byte"""
    be = big.be
    _, slices, bufs, _ = run(big, n, NAMES)
    try:
        dcols = dict(big.dcols, **{"j_" + name: _Slice(s) for name, s in zip(NAMES, slices)})
        order = ["region", "rate", "off", "tz"]  # (vector order: widths descending)
        types = big.table.COLUMNS
        for ffilters in ([], [("region", abi.LessThan, 150)], [("rate", abi.GreaterThan, 5.0), ("off", abi.LessThanOrEqual, 400)]):
            jdims = [((0, name), None, None, types[name]) for name in order]
            jdims[0] = ((0, "region"), abi.Plus, 5, abi.Uint32)
            sdims = [("j_" + d[0][1],) + d[1:] for d in jdims]
            count, want = J.per_node(be, big.dcols, [big.dtable], HINTS[2:], [("k0", big.table)],
                                     [(0, name, f, c) for name, f, c in ffilters], jdims, n)
            got_count, got = M.per_node(be, dcols, HINTS[2:] + [("j_" + name, f, c) for name, f, c in ffilters], sdims, n)
            try:
                assert got_count == count > 0
                M.assert_rows_equal(M.read_dim_rows(be, got, count), M.read_dim_rows(be, want, count), "slices against the per-node join")
            finally:
                want.free()
                got.free()
    finally:
        for x in bufs:
            x.free()


def _declined(be, q, n=100):
    be.wait()
    be.profiler_enable(True)
    try:
        with pytest.raises(abi.AresError, match="^not fusable"):
            be.join_columns_run(q, n)
        be.wait()
        assert be.profiler_report() == {}, "a declined shape launched a kernel"
    finally:
        be.profiler_enable(False)


@gpu
def test_declined_shapes_launch_nothing(hip):
    n = 100
    b = Batch(hip, n)
    rng = np.random.default_rng(3)
    b.dcols["absent"] = M.Col(abi.Uint32, None, default=5).upload(hip)
    b.dcols["rl"] = R.run_col(abi.Uint32, rng.integers(0, 9, 10), np.ones(10, bool), np.full(10, 10))[0].upload(hip)
    out = H.Buf(hip, nbytes=4 * (hip.join_column_bytes(n, abi.Uint32) + 64))
    outs = [aligned(out) + c * hip.join_column_bytes(n, abi.Uint32) for c in range(4)]
    tz = H.Buf(hip, np.zeros(16, np.int16))
    try:
        before = hip.join_column_stats()
        for dtype in (abi.Bool, abi.UUID, abi.Int64):  # a Bool and two wide joined columns
            q = query(b, NAMES[:2], outs)
            q.columns[1].column.Vector.ForeignVP.DataType = dtype
            _declined(hip, q)
        q = query(b, NAMES[:1], outs)
        q.columns[0].column.Vector.ForeignVP.TimezoneLookup, q.columns[0].column.Vector.ForeignVP.TimezoneLookupSize = tz.ptr, 16
        _declined(hip, q)
        _declined(hip, query(b, NAMES[:1], outs, key="absent"))  # a mode-0 key
        _declined(hip, query(b, NAMES[:1], outs, key="rl"))      # a run-length key
        for count in (0, 5):
            q = query(b, NAMES, outs)
            q.numColumns = count
            _declined(hip, q)
        _declined(hip, query(b, NAMES[:2], [outs[0], None]))
        _declined(hip, query(b, NAMES[:2], [outs[0], outs[1] + 32]))
        with F._Env(hip, ARES_JOIN_COLUMNS="0"):
            _declined(hip, query(b, NAMES, outs, HINTS))
        hip.wait()
        after = hip.join_column_stats()
        assert after["declined"] - before["declined"] == 11
        assert (after["batches"], after["rows"], after["probed"]) == (before["batches"], before["rows"], before["probed"])
        check(b, n, NAMES, HINTS)  # the same plan once the switch is back
    finally:
        tz.free()
        out.free()
        b.free()


@gpu
def test_zero_rows_launch_nothing(big):
    be = big.be
    out = H.Buf(be, nbytes=128)
    be.wait()
    be.profiler_enable(True)
    try:
        slices = be.join_columns_run(query(big, NAMES[:1], [aligned(out)]), 0)
        be.wait()
        assert be.profiler_report() == {} and slices[0].Length == 0
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
  printf("AresJoinedColumn %zu\nAresJoinColumns %zu\n", sizeof(AresJoinedColumn), sizeof(AresJoinColumns));
  F(AresJoinedColumn, column); F(AresJoinedColumn, out);
  F(AresJoinColumns, numFilters); F(AresJoinColumns, filters); F(AresJoinColumns, join); F(AresJoinColumns, numColumns);
  F(AresJoinColumns, columns);
  return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(abi.REPO_ROOT, "include"), str(src), "-o", str(exe)])
    seen = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    mirrors = {"AresJoinedColumn": abi.JoinedColumn, "AresJoinColumns": abi.JoinColumns}
    assert len(seen) == 9
    for name, value in seen.items():
        struct, _, member = name.partition(".")
        want = getattr(mirrors[struct], member).offset if member else C.sizeof(mirrors[struct])
        assert int(value) == want, name
    for name, struct in mirrors.items():
        assert {name + "." + f[0] for f in struct._fields_} <= set(seen)


def test_the_new_symbols_are_declared_and_exported():
    import re
    algo, _ = X._built()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(abi.REPO_ROOT, "include", "ares_extensions.h")).read(), flags=re.S)
    declared = set(re.findall(r"^(?:void|size_t|CGoCallResHandle)\s+(\w+)\s*\(", src, flags=re.M))
    lib = C.CDLL(algo, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    for name in ("AresJoinColumnsRun", "AresJoinColumnBytes", "AresJoinColumnStats"):
        assert name in declared and getattr(lib, name) is not None
