"""Sort + Reduce over group keys in dimension slots of 8 and 16 bytes — Int64 / Uint64, GeoPoint, UUID — without a row sort.

A transform into a wide slot runs at once (transform_wide_kernel), so the rows of such a query always exist when the Go host's
Sort arrives: the path they take is the wide layout of sort_reduce_fused.hip (fused_sort_reduce_vectors), whose generated scan
(hr_rtc.hip: generate_vector, sort64) reads and hashes the rows.  Everything a host can observe must be what the oracle
leaves: the groups in ascending order of lo64(murmur3_x64_128) of the packed row, bit for bit, and — for a host that looks —
the hash and index vectors between and after the two calls.  The kernel log says which path ran."""
import ctypes
import os

import numpy as np
import pytest

import harness as H
from aresdb_amd import abi
from test_sort_fused import _fusion_on, _kernels_of, _temp_stats, assert_same

pytestmark = pytest.mark.gpu

WIDTH = {abi.UUID: 16, abi.Int64: 8, abi.Uint64: 8, abi.GeoPoint: 8, abi.Uint32: 4, abi.Int32: 4, abi.Uint16: 2, abi.Uint8: 1}


class WideShape:
    """dims: data types in vector order (descending width: query/aql_compiler.go:1341-1362), one source column each;
    measure None = COUNT(*) (SUM over the literal 1 into 4 bytes), "m" = SUM of a Uint32 column into 8 bytes (Int64)."""

    def __init__(self, name, dims, measure=None):
        self.name, self.dims, self.measure = name, dims, measure
        self.ndw = tuple(sum(1 for t in dims if WIDTH[t] == w) for w in H.DIM_WIDTHS)
        assert [WIDTH[t] for t in dims] == sorted((WIDTH[t] for t in dims), reverse=True)
        self.agg = abi.AGGR_SUM_UNSIGNED
        self.value_type = abi.Uint32 if measure is None else abi.Int64
        self.value_bytes = abi.DATA_TYPE_BYTES[self.value_type]


def _sized(name, dims):
    return [WideShape(name + "_count", dims), WideShape(name + "_sum8", dims, "m")]


LAYOUTS = {
    "int64_u32": [abi.Int64, abi.Uint32],                          # (0,1,1,0,0)
    "uuid_u32": [abi.UUID, abi.Uint32],                            # (1,0,1,0,0)
    "geopoint": [abi.GeoPoint],                                    # (0,1,0,0,0)
    "uuid_int64_2xu32": [abi.UUID, abi.Int64, abi.Uint32, abi.Uint32],  # (1,1,2,0,0): 32 value bytes, the widest row taken
    "int64_u32_u16_u8": [abi.Int64, abi.Uint32, abi.Uint16, abi.Uint8],  # (0,1,1,1,1)
}
SHAPES = [s for name, dims in LAYOUTS.items() for s in _sized(name, dims)]


def _values(rng, dtype, n, distinct):
    """n values of `dtype` as an (n, width) byte array drawn from `distinct` keys whose bytes differ in EVERY word of the slot
    or in just one of them: the pool is a few base keys, each varied in one 32-bit word at a time."""
    w = WIDTH[dtype]
    words = max(1, w // 4)
    base = rng.integers(0, 1 << 32, (max(1, distinct // (words * 3)) + 1, words), dtype=np.uint64).astype(np.uint32)
    pool = [base]
    for k in range(words):  # same key but for word k (high word only, low word only, one of a UUID's four)
        for delta in (1, 0x80000000):
            v = base.copy()
            v[:, k] ^= np.uint32(delta)
            pool.append(v)
    pool = np.concatenate(pool)[:max(1, distinct)]
    if dtype == abi.GeoPoint:  # -0.0 against 0.0, NaNs that differ in their payload: keys are bytes
        special = np.array([[0x00000000, 0x80000000], [0x00000000, 0x00000000], [0x7FC00001, 0x3F800000], [0x7FC00002, 0x3F800000]], np.uint32)
        pool = np.concatenate([special, pool])
    picked = pool[rng.integers(0, len(pool), n)]
    if w < 4:
        picked = picked & np.uint32((1 << (8 * w)) - 1)
    return np.ascontiguousarray(picked).view(np.uint8).reshape(n, -1)[:, :w].copy()


def make_batch(rng, shape, n, null_fraction=0.03, distinct=40):
    cols = {}
    for d, t in enumerate(shape.dims):
        valid = rng.random(n) >= null_fraction if null_fraction > 0 else None
        cols[f"d{d}"] = (t, _values(rng, t, n, distinct), valid)
    cols["k"] = (abi.Uint32, rng.integers(0, 10, n).astype(np.uint32).view(np.uint8).reshape(n, 4), rng.random(n) >= null_fraction)
    cols["m"] = (abi.Uint32, rng.integers(0, 1 << 31, n).astype(np.uint32).view(np.uint8).reshape(n, 4), rng.random(n) >= null_fraction)
    return cols


def _rows(dv, n):
    """The first n rows of a dimension vector as one byte matrix: [values in slot order][validity bytes]."""
    blob = dv.values.read(np.uint8)
    parts = [blob[vo:vo + n * w].reshape(n, w) for vo, _, w in dv.dim_offsets()] + [blob[no:no + n].reshape(n, 1) for _, no, _ in dv.dim_offsets()]
    return np.concatenate(parts, axis=1) if n else np.zeros((0, 0), np.uint8)


def run_sequence(b, shape, batches, read=frozenset(), cap_slack=7, keep_k_below=8):
    """The Go host's per-batch sequence (query/aql_batchexecutor.go:236-251) at the ABI, result buffers ping-ponged as
    query/aql_processor.go:718-724 does; the observables of test_sort_fused.run_sequence.  The filter k < keep_k_below leaves
    batch sizes that are no multiples of four, so the rows the scan reads start at any row of the vector."""
    cap = sum(len(bt["k"][1]) for bt in batches) + cap_slack
    vb = shape.value_bytes
    dv = [H.DimVector(b, cap, shape.ndw, True, False) for _ in range(2)]
    iv = [H.Buf(b, nbytes=4 * cap) for _ in range(2)]
    vv = [H.Buf(b, nbytes=vb * cap) for _ in range(2)]
    vtype = np.uint32 if vb == 4 else np.int64
    res, log = 0, []

    def vec(i, index):
        s = dv[i].struct()
        s.IndexVector = index.ptr
        return s

    for bt in batches:
        n = len(bt["k"][1])
        cols = {k: H.Column(b, t, raw_values=v.tobytes(), valid=ok) for k, (t, v, ok) in bt.items()}
        idx, pred = H.Buf(b, nbytes=4 * n), H.Buf(b, nbytes=n)
        b.call("InitIndexVector", idx.ptr, 0, n, None, 0)
        kept = b.call("BinaryFilter", cols["k"].input(), H.const_int(keep_k_below), idx.ptr, pred.ptr, n, None, 0, None, 0, abi.LessThan, None, 0)
        offs = dv[0].dim_offsets()
        if kept > 0:
            for d, t in enumerate(shape.dims):
                out = H.dimension_output(dv[0].values.ptr + offs[d][0] + offs[d][2] * res, dv[0].values.ptr + offs[d][1] + res, t)
                b.call("UnaryTransform", cols[f"d{d}"].input(), out, idx.ptr, kept, None, 0, abi.Noop, None, 0)
            mout = H.measure_output(vv[0].ptr + vb * res, shape.value_type, shape.agg)
            src = H.const_int(1) if shape.measure is None else cols[shape.measure].input()
            b.call("UnaryTransform", src, mout, idx.ptr, kept, None, 0, abi.Noop, None, 0)
        b.wait()
        for c in cols.values():
            c.free()
        idx.free(), pred.free()
        length = res + kept
        entry = {"kept": kept}
        kin, kout = vec(0, iv[0]), vec(1, iv[1])
        b.call("InitIndexVector", iv[0].ptr, 0, length, None, 0)
        b.call("Sort", kin, length, None, 0)
        if "sorted" in read:
            entry["hash"] = dv[0].hash.read(np.uint64, length)
            entry["index"] = iv[0].read(np.uint32, length)
        groups = b.call("Reduce", kin, vv[0].ptr, kout, vv[1].ptr, vb, length, shape.agg, None, 0)
        b.wait()
        entry["groups"] = groups
        if "after" in read:
            entry["hash_after"] = dv[0].hash.read(np.uint64, length)
            entry["index_after"] = iv[0].read(np.uint32, length)
            entry["out_index"] = iv[1].read(np.uint32, groups)
        if "inputs" in read:
            entry["in_rows"] = _rows(dv[0], length)
            entry["in_values"] = vv[0].read(vtype, length)
        entry["rows"] = _rows(dv[1], groups)
        entry["values"] = vv[1].read(vtype, groups)
        log.append(entry)
        res = groups
        dv[0], dv[1] = dv[1], dv[0]
        vv[0], vv[1] = vv[1], vv[0]
    for x in dv + iv + vv:
        x.free()
    return log


def _wide_path_expected():
    return _fusion_on() and os.environ.get("ARES_SORT_VECTORS", "1") != "0"


def _assert_ordered_groups_not_rows(kernels):
    assert any(k.startswith("sr_vector_scan_rtc") for k in kernels) and any(k.startswith("sr_split_kernel") for k in kernels), sorted(kernels)
    assert any(k.startswith("sr_merge_kernel") for k in kernels), sorted(kernels)
    assert not any(k.startswith(("radix_pass_kernel", "reduce_kernel")) for k in kernels), sorted(kernels)


@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_wide_keys_are_grouped_without_a_row_sort(shape):
    """Three batches whose sizes are no multiples of four over a previous result of odd size, 3 % nulls in every dimension:
    rows, values and order are the oracle's, and neither a radix pass nor the segmented reduce ran."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    for seed in range(8):  # (the first seed that leaves a previous result whose size is no multiple of four: misaligned quads)
        rng = np.random.default_rng(sum(map(ord, shape.name)) + seed)
        batches = [make_batch(rng, shape, n) for n in (5003, 40001, 703)]
        want = run_sequence(oracle, shape, batches)
        if any(e["groups"] % 4 for e in want[:-1]):
            break
    assert any(e["groups"] % 4 for e in want[:-1])
    got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches))
    assert_same(got, want, shape.name)
    if _wide_path_expected():
        _assert_ordered_groups_not_rows(kernels)
        assert any(k.startswith("sr_bounds_kernel") for k in kernels), sorted(kernels)  # (the previous result was recognised)


def _fixed_batch(shape, rows, valid):
    """A batch of hand-made rows: rows[d] is an (n, width) byte array, valid[d] its validity."""
    n = len(valid[0])
    cols = {f"d{d}": (t, np.ascontiguousarray(rows[d], np.uint8), np.asarray(valid[d], bool)) for d, t in enumerate(shape.dims)}
    cols["k"] = (abi.Uint32, np.zeros((n, 4), np.uint8), np.ones(n, bool))
    cols["m"] = (abi.Uint32, np.arange(1, n + 1, dtype=np.uint32).view(np.uint8).reshape(n, 4), np.ones(n, bool))
    return cols


def _words(rows):
    return np.array(rows, np.uint32).view(np.uint8).reshape(len(rows), -1)


@pytest.mark.parametrize("measure", [None, "m"], ids=["count", "sum8"])
def test_keys_that_differ_in_one_word_stay_apart(measure):
    """Int64 keys that differ only in the high or only in the low word, UUIDs that differ in exactly one of their four words,
    GeoPoints -0.0 / 0.0 and NaNs of different payloads, and null rows whose value bytes differ: the oracle decides what is one
    group, and the generated hash must agree with it word for word."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    i64 = _words([[5, 0], [5, 1], [6, 0], [5, 0x80000000], [0x80000005, 0], [0, 5], [5, 5], [0, 0], [0xFFFFFFFF, 0xFFFFFFFF], [5, 0]])
    uuid = _words([[1, 2, 3, 4], [9, 2, 3, 4], [1, 9, 3, 4], [1, 2, 9, 4], [1, 2, 3, 9], [1, 2, 3, 4], [4, 3, 2, 1], [0, 0, 0, 0], [0, 0, 0, 1],
                   [1, 0, 0, 0]])
    geo = _words([[0x00000000, 0x80000000], [0x00000000, 0x00000000], [0x80000000, 0x00000000], [0x7FC00001, 0x3F800000], [0x7FC00002, 0x3F800000],
                  [0x7FC00001, 0x3F800000], [0xFFC00001, 0x3F800000], [0x3F800000, 0x7FC00001], [0, 0], [0, 0x80000000]])
    u32 = _words([[7]] * 10)
    cases = [(WideShape("int64", [abi.Int64, abi.Uint32], measure), [i64, u32]), (WideShape("uuid", [abi.UUID, abi.Uint32], measure), [uuid, u32]),
             (WideShape("geo", [abi.GeoPoint], measure), [geo])]
    all_valid = np.ones(10, bool)
    nulls = np.array([1, 1, 0, 1, 0, 1, 1, 0, 1, 1], bool)  # rows 2, 4 and 7 are null — with different value bytes behind them
    for shape, rows in cases:
        batches = [_fixed_batch(shape, [np.tile(r, (3, 1)) for r in rows], [np.tile(all_valid, 3)] + [np.tile(all_valid, 3)] * (len(rows) - 1)),
                   _fixed_batch(shape, [np.tile(r, (2, 1))[:17] for r in rows], [np.tile(nulls, 2)[:17]] + [np.tile(all_valid, 2)[:17]] * (len(rows) - 1)),
                   _fixed_batch(shape, [r[::-1] for r in rows], [nulls[::-1]] + [all_valid] * (len(rows) - 1))]
        want = run_sequence(oracle, shape, batches)
        got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches))
        assert_same(got, want, shape.name)
        assert got[0]["groups"] == len(np.unique(np.concatenate(rows, axis=1), axis=0)) >= 7  # (every distinct byte pattern is a group)
        if _wide_path_expected():
            _assert_ordered_groups_not_rows(kernels)


@pytest.mark.parametrize("read", [("sorted",), ("after",), ("inputs",), ("sorted", "after", "inputs")], ids=lambda r: "+".join(r))
@pytest.mark.parametrize("layout", ["int64_u32", "uuid_u32"])
def test_wide_keys_materialise_for_a_host_that_looks(layout, read):
    """The hash / index vectors between Sort and Reduce and after, the input rows after: what a real sort leaves."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    shape = WideShape(layout, LAYOUTS[layout])
    rng = np.random.default_rng(299 + len(read))
    batches = [make_batch(rng, shape, n) for n in (3001, 9002, 51)]
    got = run_sequence(hip, shape, batches, read=frozenset(read))
    want = run_sequence(oracle, shape, batches, read=frozenset(read))
    assert_same(got, want, (layout, read))


@pytest.mark.parametrize("part_bits", [0, 3, 12], ids=["1_partition", "8_partitions", "4096_partitions"])
@pytest.mark.parametrize("layout", ["int64_u32", "uuid_int64_2xu32", "int64_u32_u16_u8"])
def test_wide_keys_through_forced_partition_counts(layout, part_bits, monkeypatch):
    """One level of partitions, and two with a fan-out of 8, on small inputs."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    shape = WideShape(layout, LAYOUTS[layout], "m")
    rng = np.random.default_rng(17 + part_bits)
    # (a single partition's table takes ~1100 rows: beyond, Reduce declines before it launches anything)
    sizes, distinct = ((401, 603, 1), 300) if part_bits == 0 else ((2501, 6003, 1), 1500)
    batches = [make_batch(rng, shape, n, distinct=distinct) for n in sizes]
    want = run_sequence(oracle, shape, batches)
    monkeypatch.setenv("ARES_SRV_PART_BITS", str(part_bits))
    hip.reload_env()
    try:
        got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches))
    finally:
        monkeypatch.undo()
        hip.reload_env()
    assert_same(got, want, (layout, part_bits))
    if _wide_path_expected():
        assert any(k.startswith("sr_vector_scan_rtc") for k in kernels) and any(k.startswith("sr_split_kernel") for k in kernels), sorted(kernels)


def test_too_many_wide_groups_fall_back_to_the_real_sort(monkeypatch):
    """A partition's table overflows (ARES_SR_MAX_GROUPS = 20, two partitions): the ordinary Sort + Reduce runs over the same
    buffers — the fallback a wide-keyed query had as its only path before."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    shape = WideShape("uuid_u32", LAYOUTS["uuid_u32"])
    rng = np.random.default_rng(6)
    batches = [make_batch(rng, shape, n, null_fraction=0, distinct=400) for n in (600, 500)]
    want = run_sequence(oracle, shape, batches, read=frozenset(("after",)))
    monkeypatch.setenv("ARES_SR_MAX_GROUPS", "20")
    monkeypatch.setenv("ARES_SRV_PART_BITS", "1")
    hip.reload_env()
    try:
        got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches, read=frozenset(("after",))))
    finally:
        monkeypatch.undo()
        hip.reload_env()
    assert_same(got, want, "fallback")
    assert any(k.startswith(("radix_pass_kernel", "sort_")) for k in kernels), sorted(kernels)


def test_rows_beyond_32_value_bytes_keep_the_real_sort():
    """Two UUIDs and an Int64 are 40 value bytes: Sort is not defined lazily, the result is right all the same."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    shape = WideShape("two_uuids_int64", [abi.UUID, abi.UUID, abi.Int64])
    rng = np.random.default_rng(40)
    batches = [make_batch(rng, shape, n) for n in (2001, 3002)]
    want = run_sequence(oracle, shape, batches)
    got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches))
    assert_same(got, want, shape.name)
    assert not any(k.startswith("sr_vector_scan_rtc") for k in kernels), sorted(kernels)


def test_switching_the_vector_path_off_gives_the_same_result(monkeypatch):
    hip, oracle = H.hip_backend(), H.oracle_backend()
    shape = WideShape("uuid_int64_2xu32", LAYOUTS["uuid_int64_2xu32"], "m")
    rng = np.random.default_rng(12)
    batches = [make_batch(rng, shape, n) for n in (4001, 9003, 202)]
    want = run_sequence(oracle, shape, batches)
    monkeypatch.setenv("ARES_SORT_VECTORS", "0")
    hip.reload_env()
    try:
        got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches))
    finally:
        monkeypatch.undo()
        hip.reload_env()
    assert_same(got, want, "ARES_SORT_VECTORS=0")
    assert not any(k.startswith("sr_vector_scan_rtc") for k in kernels), sorted(kernels)


def test_wide_key_batches_do_not_pile_up_temporaries():
    hip = H.hip_backend()
    shape = WideShape("uuid_u32", LAYOUTS["uuid_u32"])
    rng = np.random.default_rng(73)
    few = [make_batch(rng, shape, 20001) for _ in range(3)]
    many = [make_batch(rng, shape, 20001) for _ in range(24)]
    run_sequence(hip, shape, few)
    hip.wait()
    base, _ = _temp_stats(hip)
    run_sequence(hip, shape, many)
    hip.wait()
    after, _ = _temp_stats(hip)
    assert after <= base + (1 << 20), (base, after)


def _murmur_lo64(rows):
    lib = ctypes.CDLL(H.ORACLE_SO)
    lib.oracle_murmur3_128.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    h = (ctypes.c_uint64 * 2)()
    out = np.empty(len(rows), np.uint64)
    for i, r in enumerate(rows):
        lib.oracle_murmur3_128(r.tobytes(), len(r), 0, h)
        out[i] = h[0]
    return out


def test_wide_keys_at_scale_against_an_independent_group_by():
    """8 Mi rows in four batches, ~1 M distinct UUIDs x a Uint32 of two values, COUNT(*): every key's count against numpy's
    own group-by of the same rows, and the fetched rows' 64-bit hashes ascend."""
    hip = H.hip_backend()
    shape = WideShape("uuid_u32", LAYOUTS["uuid_u32"])
    rng = np.random.default_rng(2026)
    nkeys, per_batch = 1 << 20, 2 << 20
    keys = rng.integers(0, 1 << 63, (nkeys, 2), dtype=np.int64).astype(np.uint64)
    keys[: nkeys // 2, 1] = keys[nkeys // 2:, 1][: nkeys // 2]  # half of the keys share their upper 8 bytes with another
    batches, picks = [], []
    for _ in range(4):
        pick = rng.integers(0, nkeys, per_batch)
        second = rng.integers(0, 2, per_batch).astype(np.uint32)
        picks.append(pick.astype(np.int64) * 2 + second)
        batches.append({"d0": (abi.UUID, keys[pick].view(np.uint8).reshape(per_batch, 16), None),
                        "d1": (abi.Uint32, second.view(np.uint8).reshape(per_batch, 4), None),
                        "k": (abi.Uint32, np.zeros((per_batch, 4), np.uint8), None),
                        "m": (abi.Uint32, np.zeros((per_batch, 4), np.uint8), None)})
    got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches)[-1])
    want_ids, want_counts = np.unique(np.concatenate(picks), return_counts=True)
    assert got["groups"] == len(want_ids)
    rows = got["rows"]
    assert rows.shape == (len(want_ids), 16 + 4 + 2) and (rows[:, 20:] == 1).all()
    got_uuid = rows[:, :16].copy().view(np.uint64)
    got_second = rows[:, 16:20].copy().view(np.uint32)[:, 0]
    # key -> id through a sort of the 2^20 keys (unique with overwhelming probability; asserted)
    order = np.lexsort((keys[:, 0], keys[:, 1]))
    sk = keys[order]
    assert ((sk[1:, 1] != sk[:-1, 1]) | (sk[1:, 0] != sk[:-1, 0])).all()
    pair = np.dtype([("hi", np.uint64), ("lo", np.uint64)])
    sk_pair = np.empty(nkeys, pair)
    sk_pair["hi"], sk_pair["lo"] = sk[:, 1], sk[:, 0]
    got_pair = np.empty(len(rows), pair)
    got_pair["hi"], got_pair["lo"] = got_uuid[:, 1], got_uuid[:, 0]
    at = np.searchsorted(sk_pair, got_pair)
    assert (at < nkeys).all() and (sk_pair[np.minimum(at, nkeys - 1)] == got_pair).all()
    got_ids = order[at].astype(np.int64) * 2 + got_second
    by_id = np.argsort(got_ids)
    assert np.array_equal(got_ids[by_id], want_ids)
    assert np.array_equal(got["values"][by_id].astype(np.int64), want_counts)
    sample = np.concatenate([np.arange(0, 4096), np.arange(len(rows) - 4096, len(rows)), rng.integers(0, len(rows), 8192)])
    sample.sort()
    hashes = _murmur_lo64(rows[sample])
    assert (hashes[1:] >= hashes[:-1]).all()
    if _wide_path_expected():
        _assert_ordered_groups_not_rows(kernels)


def test_wide_dimensions_through_the_native_driver():
    """The Go call order end to end: the C++ driver with an Int64 and with a UUID DimensionSpec, use_hash_reduction off,
    against the Python executor on the oracle."""
    from aresdb_amd import smoke
    from aresdb_amd.executor import Col, DimensionSpec, QueryPlan
    hip, oracle = H.hip_backend(), H.oracle_backend()
    rng = np.random.default_rng(55)
    for wide_type in (abi.Int64, abi.UUID):
        w = WIDTH[wide_type]
        plan = QueryPlan(filters=[], dimensions=[DimensionSpec(Col("key"), wide_type), DimensionSpec(Col("d1"), abi.Uint32)],
                         measure=Col("m"), agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32, use_hash_reduction=False)
        batches = []
        for n in (3001, 7002, 13):
            key = rng.integers(0, 256, (50, w), dtype=np.uint8)[rng.integers(0, 50, n)]
            if wide_type == abi.Int64:
                key = key.view(np.int64)[:, 0]
            batches.append(({"key": (wide_type, key), "d1": (abi.Uint32, rng.integers(0, 3, n).astype(np.uint32)),
                             "m": (abi.Uint32, rng.integers(0, 1000, n).astype(np.uint32))},
                            {"key": rng.random(n) >= 0.03, "d1": rng.random(n) >= 0.03, "m": None}))
        got, _ = smoke.run_query_native(hip, plan, batches)
        want, _ = smoke.run_query(oracle, plan, batches)
        assert len(want) > 100 and got == want, wide_type
