"""The direct flavour of AresJoinColumnsRun (include/ares_extensions.h): for a key column of a 1- or 2-byte type every stored key
value is probed once into a table and the rows stream through it, four per lane.  Every output byte is compared with the numpy
model of tests/select_join_model.py (Table.joined, no hints: a dictionary, not a probe) AND with the same call under
ARES_JOIN_COLUMNS=probe without hints; the bytes around the written words and values must stay untouched.

Rows: 1, 63, 64, 65 (the tail's wavefront and bitmap-word edges), 255, 256, 257 (one whole 256-row chunk and its edges), 1023,
1024, 1025 (one workgroup's tile), 4097 (sixteen chunks and a tail; with two workgroups the third round of the tile loop)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import harness as H
import narrow_join_model as N
import select_join_model as J
import select_model as M
import test_abi_exports as X
import test_fused_select as F
import test_join_columns as TJ
from aresdb_amd import abi

gpu = pytest.mark.gpu
ROWS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
NAMES = TJ.NAMES          # widths 4 / 2 / 1 and Float32
HINTS = M.MIXED_FILTERS   # two comparisons of a Uint32 column and one of a Uint8 column, nulls in both
SENTINEL = 0xA5
ROWS_PER_KEY = 64         # the default choice: direct from this many rows per stored key value (profiles/r21_join_direct.md)


@pytest.fixture(scope="module")
def hip():
    return H.hip_backend()


class Batch:
    """test_join_columns.Batch over a narrow key: the fact columns (select_model.mixed_columns + the key column "k0") and the
    table of one batch, on the device"""

    def __init__(self, be, n, key_dtype=abi.Uint16, kb=None, key_start=3, key_valid=True, seed=11, **geometry):
        self.be, self.n = be, n
        self.table = N.make_table(key_dtype, kb, seed=seed, **geometry)
        self.cols = M.mixed_columns(n)
        self.cols["k0"] = N.key_column(self.table, n, seed + 1, key_start, key_valid)
        self.dcols = {k: c.upload(be) for k, c in self.cols.items()}
        self.dtable = self.table.upload(be)
        self.space = N.KEY_SPACE[key_dtype]

    def free(self):
        for c in list(self.dcols.values()) + [self.dtable]:
            c.free()


def run(b, n, names, hints=(), key="k0"):
    """([(bitmap bytes of the written words, value bytes) per column], deltas of the counters): everything around the written
    words and values is checked to be untouched"""
    be = b.be
    sizes = [be.join_column_bytes(n, b.table.COLUMNS[name]) for name in names]
    bufs = [H.Buf(be, np.full(size + 128, SENTINEL, np.uint8)) for size in sizes]
    try:
        be.wait()
        before = dict(be.join_column_stats(), **be.join_column_flavour_stats())
        slices = be.join_columns_run(TJ.query(b, names, [TJ.aligned(x) for x in bufs], hints, key=key), n)
        be.wait()
        after = dict(be.join_column_stats(), **be.join_column_flavour_stats())
        delta = {k: after[k] - before[k] for k in after}
        assert (delta["batches"], delta["rows"], delta["declined"]) == (1, n, 0)
        outs = []
        words = 8 * ((n + 63) // 64)
        for name, x, s in zip(names, bufs, slices):
            dtype = b.table.COLUMNS[name]
            width = abi.DATA_TYPE_BYTES[dtype]
            assert (s.BasePtr, s.NullsOffset, s.ValuesOffset, s.StartingIndex, s.Length, s.DataType) == \
                (TJ.aligned(x), 0, TJ.bitmap_bytes(n), 0, n, dtype)
            off, bm = TJ.aligned(x) - x.ptr, TJ.bitmap_bytes(n)
            blob = x.read(np.uint8)
            untouched = np.concatenate([blob[:off], blob[off + words:off + bm], blob[off + bm + n * width:]])
            assert (untouched == SENTINEL).all(), (name, "bytes outside the written words and values were written")
            outs.append((blob[off:off + words].copy(), blob[off + bm:off + bm + n * width].copy()))
        return outs, delta
    finally:
        for x in bufs:
            x.free()


def model(b, n, names, hints=(), key="k0"):
    """[(bitmap bytes of the written words, value bytes)]: Table.joined; rows that fail a hint are (0, null)"""
    keep = np.ones(n, bool)
    for name, functor, c in hints:
        keep &= M.model_filter(b.cols[name], functor, c, n)
    col = b.cols[key]
    keys, key_valid = J.key_bytes_of(col, n, b.table.key_bytes), M._valid(col, n)
    outs = []
    for name in names:
        j = b.table.joined(keys, key_valid, name)
        bits = np.zeros((n + 63) // 64 * 64, bool)  # (bits at or past n in the last word: 0)
        bits[:n] = j.valid & keep
        values = np.where(keep, j.values, np.zeros(1, j.values.dtype)).astype(j.values.dtype)
        outs.append((np.packbits(bits, bitorder="little"), values.view(np.uint8)))
    return outs, int((keep & key_valid).sum())


def same(got, want, what):
    assert len(got) == len(want)
    for c, ((gb, gv), (wb, wv)) in enumerate(zip(got, want)):
        assert np.array_equal(gb, wb), (what, c, "validity bitmap")
        assert np.array_equal(gv, wv), (what, c, "values")


def check_direct(b, n, names, hints=(), key="k0"):
    """under ARES_JOIN_COLUMNS=direct, with `hints` handed in: the model without hints, the probe flavour without hints, and
    the counters of one direct batch"""
    with F._Env(b.be, ARES_JOIN_COLUMNS="direct"):
        got, delta = run(b, n, names, hints, key)
    assert (delta["direct"], delta["probe"], delta["entries"], delta["probed"]) == (1, 0, b.space, b.space)
    same(got, model(b, n, names, key=key)[0], "direct against the model")
    with F._Env(b.be, ARES_JOIN_COLUMNS="probe"):
        probe, pdelta = run(b, n, names, key=key)
    assert (pdelta["direct"], pdelta["probe"], pdelta["entries"]) == (0, 1, 0)
    assert pdelta["probed"] == int(M._valid(b.cols[key], n).sum())
    same(got, probe, "direct against probe")
    return got


@pytest.fixture(scope="module")
def big(hip):
    b = Batch(hip, 4097)
    yield b
    b.free()


@pytest.fixture(scope="module")
def big8(hip):
    b = Batch(hip, 4097, abi.Uint8)
    yield b
    b.free()


@gpu
def test_the_fixture_reaches_every_case_of_the_rule(big, big8):
    for b in (big, big8):
        assert N.reached(b.table, b.cols["k0"], 300) == N.CASES
    assert (big.table.stash_signatures() != 0).any()


@pytest.mark.parametrize("n", ROWS)
@gpu
def test_rows_at_the_wave_chunk_tile_and_word_edges(big, big8, n):
    check_direct(big, n, NAMES)
    check_direct(big, n, NAMES[:1])
    check_direct(big8, n, NAMES)
    check_direct(big8, n, NAMES[3:])


@pytest.mark.parametrize("grid", ["2", "1000"])
@gpu
def test_the_rounds_of_the_tile_loop(big, big8, grid):
    """4097 rows are five 1024-row tiles: two workgroups take three rounds; a grid larger than the tile count is capped"""
    with F._Env(big.be, ARES_JOIN_COLUMNS_GRID=grid):
        check_direct(big, 4097, NAMES)
        check_direct(big8, 4097, NAMES[1:3])


@pytest.mark.parametrize("kb", [None, 4], ids=["width", "keyBytes4"])
@pytest.mark.parametrize("key_dtype", N.NARROW)
@gpu
def test_every_narrow_key_type(hip, key_dtype, kb):
    """negative keys of the signed types are sign-extended before keyBytes of them are kept, as HashLookup widens them"""
    n = 1100
    b = Batch(hip, n, key_dtype, kb, default=kb is None)
    try:
        col = b.cols["k0"]
        want = b.table.joined(J.key_bytes_of(col, n, b.table.key_bytes), M._valid(col, n), "region")
        if key_dtype in (abi.Int8, abi.Int16):
            assert (col.values[:n][want.valid] < 0).any()
        assert want.valid.any() and not want.valid.all()
        check_direct(b, n, NAMES)
        check_direct(b, 300, NAMES[:2])
    finally:
        b.free()


@pytest.mark.parametrize("key_dtype", [abi.Uint16, abi.Int16])
@gpu
def test_a_key_column_wider_than_the_index_key(hip, key_dtype):
    """a 2-byte column over an index of 1-byte keys: the low byte is the key"""
    b = Batch(hip, 700, key_dtype, 1)
    try:
        assert b.table.key_bytes == 1
        check_direct(b, 700, NAMES)
    finally:
        b.free()


@pytest.mark.parametrize("key_start", [0, 3, 5, 7])
@pytest.mark.parametrize("key_dtype", [abi.Uint8, abi.Int16])
@gpu
def test_starting_indexes_of_the_key_bitmap(hip, key_dtype, key_start):
    """5 and 7: a lane's four validity bits straddle two bytes"""
    b = Batch(hip, 1100, key_dtype, key_start=key_start)
    try:
        assert b.dcols["k0"].vp.StartingIndex == key_start and not b.cols["k0"].valid.all()
        check_direct(b, 1100, NAMES[:2])
    finally:
        b.free()


@pytest.mark.parametrize("key_dtype", [abi.Uint8, abi.Uint16])
@gpu
def test_a_mode_1_key(hip, key_dtype):
    b = Batch(hip, 1100, key_dtype, key_valid=False)
    try:
        assert b.dcols["k0"].vp.ValuesOffset == 0
        check_direct(b, 1100, NAMES)
    finally:
        b.free()


@pytest.mark.parametrize("geometry", [dict(num_hashes=0), dict(num_hashes=4), dict(num_buckets=1, nkeys=11), dict(default=False)],
                         ids=["stash_only", "four_hashes", "one_bucket", "no_default"])
@pytest.mark.parametrize("key_dtype", [abi.Uint8, abi.Int16])
@gpu
def test_index_geometries_and_a_table_without_defaults(hip, key_dtype, geometry):
    """numHashes 0: every key lies in the stash or nowhere; numBuckets 1; a table whose mode-0 batch has no default.  The
    record in a batch outside the table and the stale records of the last batch are in every one of them that holds its keys."""
    n = 1100
    b = Batch(hip, n, key_dtype, **geometry)
    try:
        if geometry.get("num_hashes") == 0:
            assert (b.table.stash_signatures() != 0).any() and 0 < len(b.table.placed) <= 8
        else:
            assert {"outside the table", "stale record"} <= N.reached(b.table, b.cols["k0"], n)
        check_direct(b, n, NAMES)
        check_direct(b, 257, NAMES[:3], HINTS)
    finally:
        b.free()


@gpu
def test_hints_change_no_byte_of_a_direct_batch(big, big8):
    """hints are not evaluated: not even one that kills every row"""
    for b in (big, big8):
        with F._Env(b.be, ARES_JOIN_COLUMNS="direct"):
            free, _ = run(b, 4097, NAMES)
        for hints in (HINTS, [("ts", abi.GreaterThan, 10 ** 6)]):
            same(check_direct(b, 4097, NAMES, hints), free, "hints against none")
        with F._Env(b.be, ARES_JOIN_COLUMNS="probe"):  # (the probe flavour does prune)
            pruned, delta = run(b, 4097, NAMES, HINTS)
        want, want_probed = model(b, 4097, NAMES, HINTS)
        same(pruned, want, "probe with hints against the model")
        assert delta["probed"] == want_probed < int(M._valid(b.cols["k0"], 4097).sum())


@gpu
def test_a_four_byte_key_under_direct_is_a_probe_batch(hip):
    n = 1100
    b = TJ.Batch(hip, n, abi.Uint32)
    b.space = 0
    try:
        with F._Env(hip, ARES_JOIN_COLUMNS="direct"):
            got, delta = run(b, n, NAMES, HINTS)
        want, want_probed = model(b, n, NAMES, HINTS)
        same(got, want, "a 4-byte key")
        assert (delta["probe"], delta["direct"], delta["entries"], delta["probed"]) == (1, 0, 0, want_probed)
    finally:
        b.free()


@gpu
def test_the_default_choice(hip):
    """direct when the key is narrow and the batch has at least ROWS_PER_KEY rows per stored key value"""
    edge = ROWS_PER_KEY * 256
    b8, b16 = Batch(hip, edge, abi.Uint8), Batch(hip, 4097, abi.Uint16)
    try:
        for value in ("", "1"):  # (anything but 0, probe and direct)
            with F._Env(hip, ARES_JOIN_COLUMNS=value):
                got, delta = run(b8, edge, NAMES, HINTS)
                assert (delta["direct"], delta["probe"], delta["entries"], delta["probed"]) == (1, 0, 256, 256)
                same(got, model(b8, edge, NAMES)[0], "the default choice at the edge")
                got, delta = run(b8, edge - 1, NAMES, HINTS)
                want, want_probed = model(b8, edge - 1, NAMES, HINTS)
                assert (delta["direct"], delta["probe"], delta["entries"], delta["probed"]) == (0, 1, 0, want_probed)
                same(got, want, "the default choice below the edge")
        got, delta = run(b16, 4097, NAMES, HINTS)
        want, want_probed = model(b16, 4097, NAMES, HINTS)
        assert (delta["direct"], delta["probe"], delta["entries"], delta["probed"]) == (0, 1, 0, want_probed)
        same(got, want, "a Uint16 key at 4097 rows")
    finally:
        b8.free()
        b16.free()


@gpu
def test_zero_rows_launch_nothing_in_either_flavour(big):
    be = big.be
    out = H.Buf(be, nbytes=128)
    be.wait()
    be.profiler_enable(True)
    try:
        before = be.join_column_flavour_stats()
        for flavour in ("direct", "probe"):
            with F._Env(be, ARES_JOIN_COLUMNS=flavour):
                slices = be.join_columns_run(TJ.query(big, NAMES[:1], [TJ.aligned(out)]), 0)
                assert slices[0].Length == 0
        be.wait()
        assert be.profiler_report() == {} and be.join_column_flavour_stats() == before
    finally:
        be.profiler_enable(False)
        out.free()


@gpu
def test_the_kernels_of_either_flavour(big):
    be = big.be
    out = H.Buf(be, nbytes=be.join_column_bytes(4097, abi.Uint32) + 64)
    try:
        for flavour, want in (("direct", {"join_columns_table_kernel", "join_columns_rows_kernel"}), ("probe", {"join_columns_kernel"})):
            with F._Env(be, ARES_JOIN_COLUMNS=flavour):
                be.wait()
                be.profiler_enable(True)
                try:
                    be.join_columns_run(TJ.query(big, NAMES[:1], [TJ.aligned(out)]), 4097)
                    be.wait()
                    report = be.profiler_report()
                finally:
                    be.profiler_enable(False)
            assert set(report) == want and all(v[0] == 1 for v in report.values()), report
    finally:
        out.free()


@gpu
def test_the_slices_read_as_the_per_node_join_sequence_reads(big):
    """UnaryTransform / BinaryTransform / BinaryFilter over the slices a direct batch returns against HashLookup + the same
    calls over the foreign column with record ids: survivor count and every dimension byte"""
    be, n = big.be, 4097
    bufs = [H.Buf(be, nbytes=be.join_column_bytes(n, big.table.COLUMNS[name]) + 64) for name in NAMES]
    try:
        with F._Env(be, ARES_JOIN_COLUMNS="direct"):
            before = be.join_column_flavour_stats()
            slices = be.join_columns_run(TJ.query(big, NAMES, [TJ.aligned(x) for x in bufs], HINTS[2:]), n)
            be.wait()
            assert be.join_column_flavour_stats()["direct"] - before["direct"] == 1
        dcols = dict(big.dcols, **{"j_" + name: TJ._Slice(s) for name, s in zip(NAMES, slices)})
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


# ---- the boundary: no GPU needed, nothing is called ----------------------------------------------------------------------
def test_the_flavour_counters_are_declared_and_exported():
    algo, _ = X._built()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(abi.REPO_ROOT, "include", "ares_extensions.h")).read(), flags=re.S)
    declared = set(re.findall(r"^(?:void|size_t|CGoCallResHandle)\s+(\w+)\s*\(", src, flags=re.M))
    lib = C.CDLL(algo, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    assert "AresJoinColumnFlavourStats" in declared and getattr(lib, "AresJoinColumnFlavourStats") is not None
    assert callable(getattr(abi.Backend, "join_column_flavour_stats"))


def test_the_environment_values_are_documented():
    text = open(os.path.join(abi.REPO_ROOT, "INTEGRATION.md")).read()
    rows = [line for line in text.splitlines() if line.startswith("|") and "ARES_JOIN_COLUMNS" in line]
    assert any("ARES_JOIN_COLUMNS=probe" in line for line in rows) and any("ARES_JOIN_COLUMNS=direct" in line for line in rows)
    assert any("ARES_JOIN_COLUMNS=0" in line for line in rows)
    header = open(os.path.join(abi.REPO_ROOT, "include", "ares_extensions.h")).read()
    assert "=probe / =direct" in header and "AresJoinColumnFlavourStats" in header
