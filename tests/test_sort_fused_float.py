"""Float aggregates through Sort + Reduce without a row sort (aresdb_amd/csrc/algo/sort_reduce_fused.hip): SUM_FLOAT into 8 and
4 bytes, MIN_FLOAT, MAX_FLOAT on the scan-fed and the wide layout, AVG_FLOAT on the wide one.  The Go host's sequence
(InitIndexVector, transforms, Sort, Reduce, result buffers ping-ponged) is replayed at the ABI as tests/test_sort_fused.py does
for integers.  Everything that does not depend on the order of additions — group count, output order (ascending 64-bit row
hash), dimension rows, validity, the output's index vector, AVG's counts, MIN / MAX — is the oracle's bit for bit; sums and
averages hold the bounds the project documents:
  * float64 sums: n_g additions in ANY order are within n_g 2^-53 sum|x| of the exact sum (tests/test_edge_semantics.py), so two
    orders differ by at most twice that;
  * float32 sums: 1e-4 sum|x|;  rolling averages: 1e-4 sum|x| / count.
sum|x| and n_g per group come from the oracle itself: the same query over |measure| into a float64 sum, and COUNT(*)."""
import os

import numpy as np
import pytest

import harness as H
from aresdb_amd import abi

pytestmark = pytest.mark.gpu

F32_MAX = float(np.finfo(np.float32).max)


def _kernels_of(hip, fn):
    hip.profiler_enable(True)
    try:
        res = fn()
        hip.wait()
        return res, hip.profiler_report()
    finally:
        hip.profiler_enable(False)


def _fusion_on():
    return all(os.environ.get(k, "1") != "0" for k in ("ARES_FUSE", "ARES_DEFER", "ARES_SORT_FUSE", "ARES_RTC", "ARES_SR_FLOAT"))


def _wide_on():
    return _fusion_on() and os.environ.get("ARES_SORT_VECTORS", "1") != "0"


class Shape:
    """cols: name -> (data type, upper bound) for integer columns, (Float32, "hard" | "pool") for float ones; filters:
    (column, functor, constant); dims: (column, functor or None, constant, output type); measure: ("col", name),
    ("expr", name, functor, float constant) or ("const", float); measure_type: what the measure transform stores (Float64 /
    Float32; AVG_FLOAT, an 8-byte measure, packs {f32 average, u32 count})."""

    def __init__(self, name, cols, filters, dims, measure, agg, measure_type, value_bytes, ndw):
        self.name, self.cols, self.filters, self.dims, self.measure, self.agg, self.measure_type, self.value_bytes, self.ndw = \
            name, cols, filters, dims, measure, agg, measure_type, value_bytes, ndw

    def magnitudes(self):
        """the same groups, SUM(|measure|) into float64"""
        m = self.measure if self.measure[0] != "const" else ("const", abs(self.measure[1]))
        return Shape(self.name + "/abs", self.cols, self.filters, self.dims, m, abi.AGGR_SUM_FLOAT, abi.Float64, 8, self.ndw)

    def counts(self):
        return Shape(self.name + "/count", self.cols, self.filters, self.dims, None, abi.AGGR_SUM_UNSIGNED, abi.Uint32, 4, self.ndw)


def hard_floats(rng, n):
    """full-mantissa float32 values over seven decades of magnitude, mixed sign (tests/test_edge_semantics.py)"""
    return ((1.0 + rng.random(n)) * 10.0 ** rng.uniform(-3, 4, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def pool_floats(rng, n, nan=False):
    """MIN / MAX material: infinities, +-FLT_MAX, denormals, ONE kind of zero, ordinary values; no NaN unless asked for"""
    pool = np.array([np.inf, -np.inf, F32_MAX, -F32_MAX, 1e-45, -1e-45, 1.1754942e-38, -5.9e-39, 0.0, 1.0, -1.0, 3.5, -2.25e10], np.float32)
    x = np.where(rng.random(n) < 0.02, pool[rng.integers(0, len(pool), n)], hard_floats(rng, n)).astype(np.float32)
    if nan:
        x[rng.integers(0, n, 3)] = np.nan
    return x


_NP = {abi.Uint32: np.uint32, abi.Int32: np.int32, abi.Uint16: np.uint16, abi.Uint8: np.uint8}


def make_batch(rng, shape, n, null_fraction=0.03, nan=False):
    cols = {}
    for name, (dtype, spec) in shape.cols.items():
        if dtype == abi.Float32:
            vals = hard_floats(rng, n) if spec == "hard" else pool_floats(rng, n, nan)
        else:
            vals = rng.integers(0, spec, n).astype(_NP[dtype])
        cols[name] = (dtype, vals, (rng.random(n) >= null_fraction) if null_fraction > 0 else None)
    return cols


def _column(b, dtype, vals, valid, rle=False):
    if not rle:
        return H.Column(b, dtype, vals, valid=valid)
    ok = np.ones(len(vals), bool) if valid is None else valid
    cut = np.flatnonzero((vals[1:] != vals[:-1]) | (ok[1:] != ok[:-1])) + 1
    starts = np.concatenate([[0], cut])
    return H.Column(b, dtype, vals[starts], valid=ok[starts], counts=np.concatenate([starts, [len(vals)]]).astype(np.uint32))


def run_sequence(b, shape, batches, read=frozenset(), eager=False, absolute=False, cap_slack=10):
    """The Go host's per-batch sequence.  read: "sorted" (hash + index vector between Sort and Reduce), "after" (the output's
    index vector after Reduce); eager: the host reads the batch's rows before Sort (they are written: the wide layout);
    absolute: float columns are replaced by their magnitudes (Shape.magnitudes)."""
    cap = sum(len(next(iter(bt.values()))[1]) for bt in batches) + cap_slack
    vb = shape.value_bytes
    dv = [H.DimVector(b, cap, shape.ndw, True, False) for _ in range(2)]
    iv = [H.Buf(b, nbytes=4 * cap) for _ in range(2)]
    vv = [H.Buf(b, nbytes=vb * cap) for _ in range(2)]
    raw = np.uint64 if vb == 8 else np.uint32
    res, log = 0, []

    def vec(i, index):
        s = dv[i].struct()
        s.IndexVector = index.ptr
        return s

    for bt in batches:
        n = len(next(iter(bt.values()))[1])
        cols = {}
        for k, spec in bt.items():
            dtype, vals = spec[0], spec[1]
            cols[k] = _column(b, dtype, np.abs(vals) if absolute and dtype == abi.Float32 else vals, *spec[2:])
        idx, pred = H.Buf(b, nbytes=4 * n), H.Buf(b, nbytes=n)
        b.call("InitIndexVector", idx.ptr, 0, n, None, 0)
        kept = n
        for col, ft, k in shape.filters:
            kept = b.call("BinaryFilter", cols[col].input(), H.const_int(k), idx.ptr, pred.ptr, kept, None, 0, None, 0, ft, None, 0)
        offs = dv[0].dim_offsets()
        for d, (col, ft, k, otype) in enumerate(shape.dims):
            out = H.dimension_output(dv[0].values.ptr + offs[d][0] + offs[d][2] * res, dv[0].values.ptr + offs[d][1] + res, otype)
            if kept <= 0:
                continue
            if ft is None:
                b.call("UnaryTransform", cols[col].input(), out, idx.ptr, kept, None, 0, abi.Noop, None, 0)
            else:
                b.call("BinaryTransform", cols[col].input(), H.const_int(k), out, idx.ptr, kept, None, 0, ft, None, 0)
        if kept > 0:
            mout = H.measure_output(vv[0].ptr + vb * res, shape.measure_type, shape.agg)
            m = shape.measure
            if m is None:
                b.call("UnaryTransform", H.const_int(1), mout, idx.ptr, kept, None, 0, abi.Noop, None, 0)
            elif m[0] == "const":
                b.call("UnaryTransform", H.const_float(m[1]), mout, idx.ptr, kept, None, 0, abi.Noop, None, 0)
            elif m[0] == "expr":
                b.call("BinaryTransform", cols[m[1]].input(), H.const_float(m[3]), mout, idx.ptr, kept, None, 0, m[2], None, 0)
            else:
                b.call("UnaryTransform", cols[m[1]].input(), mout, idx.ptr, kept, None, 0, abi.Noop, None, 0)
        b.wait()
        if eager and kept > 0:
            dv[0].rows(res + kept), vv[0].read(raw, res + kept)
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
            entry["out_index"] = iv[1].read(np.uint32, groups)
        entry["rows"] = dv[1].rows(groups)
        entry["values"] = vv[1].read(raw, groups)
        log.append(entry)
        res = groups
        dv[0], dv[1] = dv[1], dv[0]
        vv[0], vv[1] = vv[1], vv[0]
    for x in dv + iv + vv:
        x.free()
    return log


def references(oracle, shape, batches, **kw):
    """the oracle's result, and per batch and group sum|x| (float64) and the number of rows"""
    want = run_sequence(oracle, shape, batches, **kw)
    mags = run_sequence(oracle, shape.magnitudes(), batches, absolute=True)
    counts = run_sequence(oracle, shape.counts(), batches)
    for w, m, c in zip(want, mags, counts):
        assert w["rows"] == m["rows"] == c["rows"]  # (the same groups in the same order)
    return want, [m["values"].view(np.float64) for m in mags], [c["values"].astype(np.float64) for c in counts]


def assert_close(got, refs, shape):
    """Everything but sums and averages bit for bit; those within their bounds."""
    want, mags, counts = refs
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        where = (shape.name, "batch", k)
        assert set(g) == set(w), where
        assert g["kept"] == w["kept"] and g["groups"] == w["groups"], where
        assert g["rows"] == w["rows"], where
        for key in ("hash", "index", "out_index"):
            if key in w:
                assert np.array_equal(g[key], w[key]), where + (key,)
        gv, wv = g["values"], w["values"]
        if shape.agg in (abi.AGGR_MIN_FLOAT, abi.AGGR_MAX_FLOAT):
            assert np.array_equal(gv, wv), where + (gv[:8], wv[:8])
        elif shape.agg == abi.AGGR_AVG_FLOAT:
            gp, wp = gv.view(np.uint32).reshape(-1, 2), wv.view(np.uint32).reshape(-1, 2)
            assert np.array_equal(gp[:, 1], wp[:, 1]), where + ("counts",)
            ga, wa = gp[:, 0].copy().view(np.float32).astype(np.float64), wp[:, 0].copy().view(np.float32).astype(np.float64)
            assert np.all(np.abs(ga - wa) <= 1e-4 * mags[k] / np.maximum(wp[:, 1], 1)), where
        elif shape.value_bytes == 8:
            gs, ws = gv.view(np.float64), wv.view(np.float64)
            assert np.all(np.abs(gs - ws) <= 2.0 * counts[k] * 2.0 ** -53 * mags[k]), where + (float(np.max(np.abs(gs - ws))),)
        else:
            gs, ws = gv.view(np.float32).astype(np.float64), wv.view(np.float32).astype(np.float64)
            assert np.all(np.abs(gs - ws) <= 1e-4 * mags[k]), where


def _starts(kernels, *prefixes):
    return any(k.startswith(prefixes) for k in kernels)


_C3_COLS = {"ts": (abi.Uint32, 86400 * 7), "d1": (abi.Uint32, 100), "d2": (abi.Uint32, 50), "d3": (abi.Uint32, 2), "m": (abi.Float32, "hard")}
_C3_DIMS = [("ts", abi.Floor, 3600, abi.Uint32), ("d1", None, 0, abi.Uint32), ("d2", None, 0, abi.Uint32), ("d3", None, 0, abi.Uint32)]
_C3_NDW = (0, 0, 4, 0, 0)
_TRIPS_COLS = {"request_at": (abi.Uint32, 86400 * 3), "city_id": (abi.Uint16, 300), "status": (abi.Uint8, 4), "fare": (abi.Float32, "hard")}
_ONE_DIM = {"d1": (abi.Uint32, 3000)}

C3_SUM = Shape("c3_sum_f64", _C3_COLS, [("d1", abi.LessThan, 90)], _C3_DIMS, ("col", "m"), abi.AGGR_SUM_FLOAT, abi.Float64, 8, _C3_NDW)
# examples/1k_trips/queries/total_fare.aql with the reference's shipped enable_hash_reduction = false
TRIPS_FARE = Shape("trips_sum_fare", _TRIPS_COLS,
                   [("request_at", abi.GreaterThanOrEqual, 1000), ("request_at", abi.LessThan, 200000), ("status", abi.Equal, 2)],
                   [("request_at", abi.Floor, 3600, abi.Uint32), ("city_id", None, 0, abi.Uint16)],
                   ("col", "fare"), abi.AGGR_SUM_FLOAT, abi.Float64, 8, (0, 0, 1, 1, 0))
MIN_F = Shape("min_float", {**_ONE_DIM, "m": (abi.Float32, "pool")}, [], [("d1", None, 0, abi.Uint32)], ("col", "m"),
              abi.AGGR_MIN_FLOAT, abi.Float32, 4, (0, 0, 1, 0, 0))
MAX_F = Shape("max_float", {"d1": (abi.Uint32, 70), "d2": (abi.Uint32, 9), "m": (abi.Float32, "pool")}, [("d2", abi.NotEqual, 3)],
              [("d1", abi.Plus, 5, abi.Uint32), ("d2", None, 0, abi.Uint32)], ("col", "m"), abi.AGGR_MAX_FLOAT, abi.Float32, 4, (0, 0, 2, 0, 0))
SUM_F32 = Shape("sum_f32", {"ts": (abi.Uint32, 86400), "d1": (abi.Uint32, 40), "m": (abi.Float32, "hard")},
                [("ts", abi.GreaterThanOrEqual, 3600), ("ts", abi.LessThan, 80000)],
                [("ts", abi.Floor, 600, abi.Uint32), ("d1", None, 0, abi.Uint32)], ("col", "m"), abi.AGGR_SUM_FLOAT, abi.Float32, 4, (0, 0, 2, 0, 0))
CONST_SUM = Shape("const_float_sum", {"d1": (abi.Uint32, 3000), "d2": (abi.Uint32, 5)}, [("d2", abi.LessThan, 4)],
                  [("d1", None, 0, abi.Uint32), ("d2", None, 0, abi.Uint32)], ("const", 2.7182817), abi.AGGR_SUM_FLOAT, abi.Float64, 8, (0, 0, 2, 0, 0))
EXPR_SUM = Shape("expression_sum", _C3_COLS, [("d1", abi.LessThan, 90)], _C3_DIMS[:2], ("expr", "m", abi.Multiply, 1.5),
                 abi.AGGR_SUM_FLOAT, abi.Float64, 8, (0, 0, 2, 0, 0))
AVG_F = Shape("avg_float", {"d1": (abi.Uint32, 900), "d2": (abi.Uint32, 4), "m": (abi.Float32, "hard")}, [("d2", abi.NotEqual, 3)],
              [("d1", None, 0, abi.Uint32), ("d2", None, 0, abi.Uint32)], ("col", "m"), abi.AGGR_AVG_FLOAT, abi.Float64, 8, (0, 0, 2, 0, 0))

SCAN_FED = [C3_SUM, TRIPS_FARE, MIN_F, MAX_F, SUM_F32, CONST_SUM, EXPR_SUM]
_SIZES = (5000, 1, 40000, 700)


def _batches(shape, seed=0, sizes=_SIZES, **kw):
    rng = np.random.default_rng(sum(map(ord, shape.name)) + seed)
    return [make_batch(rng, shape, n, **kw) for n in sizes]


@pytest.mark.parametrize("shape", SCAN_FED, ids=[s.name for s in SCAN_FED])
def test_float_aggregates_consume_pending_transforms(shape):
    """Scan-fed: nothing is sorted, no transform is launched, the float values meet their groups in the merge's LDS tables."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    batches = _batches(shape, sizes=(5000, 40, 40000, 700))
    got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches))
    assert_close(got, references(oracle, shape, batches), shape)
    assert all(e["kept"] > 0 for e in got)  # (a batch without survivors queues no transforms: the real sort would run)
    if _fusion_on():
        assert _starts(kernels, "sr_scan_rtc") and _starts(kernels, "sr_merge_kernel"), sorted(kernels)
        assert not _starts(kernels, "radix_pass_kernel", "reduce_kernel", "transform_"), sorted(kernels)
    # ... and the output's index vector (the groups' representatives), for a host that looks
    read = frozenset(("after",))
    assert_close(run_sequence(hip, shape, batches, read=read), references(oracle, shape, batches, read=read), shape)


WIDE = [C3_SUM, TRIPS_FARE, MIN_F, MAX_F, SUM_F32, AVG_F]


@pytest.mark.parametrize("part_bits", [None, 7, 12], ids=["default_bits", "128_partitions", "4096_partitions"])
@pytest.mark.parametrize("shape", WIDE, ids=[s.name for s in WIDE])
def test_float_aggregates_over_materialised_rows(shape, part_bits, monkeypatch):
    """An eager host (the rows are written and waited for before Sort): the wide layout — and AVG_FLOAT, whose counts are exact."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    batches = _batches(shape, seed=7)
    refs = references(oracle, shape, batches, eager=True)
    if part_bits is not None:
        monkeypatch.setenv("ARES_SRV_PART_BITS", str(part_bits))
    hip.reload_env()
    try:
        got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches, eager=True))
    finally:
        monkeypatch.undo()
        hip.reload_env()
    assert_close(got, refs, shape)
    if _wide_on():
        assert _starts(kernels, "sr_split_kernel") and _starts(kernels, "sr_merge_kernel"), sorted(kernels)
        assert not _starts(kernels, "radix_pass_kernel"), sorted(kernels)


@pytest.mark.parametrize("shape", [C3_SUM, TRIPS_FARE, MIN_F, SUM_F32], ids=lambda s: s.name)
def test_scan_fed_float_shapes_handed_to_the_wide_layout(shape, monkeypatch):
    hip, oracle = H.hip_backend(), H.oracle_backend()
    batches = _batches(shape, seed=41, sizes=(6000, 20000, 300))
    refs = references(oracle, shape, batches)
    monkeypatch.setenv("ARES_SR_SCAN_FED", "0")
    hip.reload_env()
    try:
        got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches))
    finally:
        monkeypatch.undo()
        hip.reload_env()
    assert_close(got, refs, shape)
    if _wide_on():
        assert _starts(kernels, "sr_split_kernel") and not _starts(kernels, "radix_pass_kernel", "sr_scan_rtc"), sorted(kernels)


@pytest.mark.parametrize("eager", [False, True], ids=["scan_fed", "wide"])
@pytest.mark.parametrize("shape", [MIN_F, MAX_F], ids=lambda s: s.name)
def test_nan_among_min_max_values_takes_the_real_sort(shape, eager, monkeypatch):
    """The LDS instructions drop a NaN (IEEE minNum / maxNum), a comparison-based merge keeps or drops it by its position
    (tests/edge_model.py, UNDEFINED: nan_in_float_min_max).  The merge does not pick a third behaviour: it notices the NaN and
    the call falls back — groups, order and representatives are the oracle's, the values bit for bit what the real sort gives
    with float aggregates switched off, and the oracle's in every group but the few that hold a NaN.  Without the NaN: the
    fused path, the oracle's bits."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    batches = _batches(shape, seed=3, sizes=(6000, 9000, 400), nan=True)
    nans = sum(int(np.isnan(bt["m"][1][bt["m"][2]]).sum()) for bt in batches)
    assert nans > 0
    got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches, eager=eager))
    monkeypatch.setenv("ARES_SR_FLOAT", "0")
    hip.reload_env()
    try:
        sorted_rows = run_sequence(hip, shape, batches, eager=eager)
    finally:
        monkeypatch.undo()
        hip.reload_env()
    want = run_sequence(oracle, shape, batches, eager=eager)
    for k, (g, s, w) in enumerate(zip(got, sorted_rows, want)):
        assert g["groups"] == w["groups"] and g["rows"] == w["rows"], (shape.name, k)
        assert np.array_equal(g["values"], s["values"]), (shape.name, k)
        assert int(np.count_nonzero(g["values"] != w["values"])) <= nans, (shape.name, k)
    if _fusion_on():
        assert _starts(kernels, "radix_pass_kernel"), sorted(kernels)
    clean = [{k: (s[0], np.where(np.isnan(s[1]), np.float32(1.5), s[1]) if s[0] == abi.Float32 else s[1], s[2]) for k, s in bt.items()} for bt in batches]
    got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, clean, eager=eager))
    assert_close(got, references(oracle, shape, clean, eager=eager), shape)
    if _fusion_on() and (not eager or _wide_on()):
        assert _starts(kernels, "sr_merge_kernel") and not _starts(kernels, "radix_pass_kernel"), sorted(kernels)


def test_float_sum_with_too_many_groups_falls_back_to_the_real_sort(monkeypatch):
    hip, oracle = H.hip_backend(), H.oracle_backend()
    shape = Shape("distinct_sum", {"d1": (abi.Uint32, 1 << 30), "m": (abi.Float32, "hard")}, [], [("d1", None, 0, abi.Uint32)], ("col", "m"),
                  abi.AGGR_SUM_FLOAT, abi.Float64, 8, (0, 0, 1, 0, 0))
    batches = _batches(shape, sizes=(30000, 30000, 2000), null_fraction=0)
    monkeypatch.setenv("ARES_SR_MAX_GROUPS", "100")
    hip.reload_env()
    try:
        got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches, read=frozenset(("after",))))
    finally:
        monkeypatch.undo()
        hip.reload_env()
    assert_close(got, references(oracle, shape, batches, read=frozenset(("after",))), shape)
    assert _starts(kernels, "radix_pass_kernel"), sorted(kernels)


@pytest.mark.parametrize("shape", [C3_SUM, MIN_F], ids=lambda s: s.name)
def test_switch_gives_the_sequential_order_back(shape, monkeypatch):
    """ARES_SR_FLOAT=0: float aggregates keep the real sort (every sum in the sorted order: the oracle's bits); =1 after a
    reload: the fused path again."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    batches = _batches(shape, seed=5, sizes=(4000, 7000, 300))
    refs = references(oracle, shape, batches)
    monkeypatch.setenv("ARES_SR_FLOAT", "0")
    hip.reload_env()
    try:
        got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches))
        assert_close(got, refs, shape)
        assert _starts(kernels, "radix_pass_kernel") and not _starts(kernels, "sr_merge_kernel"), sorted(kernels)
        monkeypatch.setenv("ARES_SR_FLOAT", "1")
        hip.reload_env()
        got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches))
    finally:
        monkeypatch.undo()
        hip.reload_env()
    assert_close(got, refs, shape)
    if _fusion_on():
        assert _starts(kernels, "sr_merge_kernel") and not _starts(kernels, "radix_pass_kernel"), sorted(kernels)


def test_archive_batch_with_a_float_sum():
    """Run-length encoded sort columns (ts, d3), decoded once each; the float measure plain."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    rng = np.random.default_rng(71)

    def archive(n):
        ts = np.sort(rng.integers(0, 86400 * 2, max(1, n // 40)).astype(np.uint32))[rng.integers(0, max(1, n // 40), n)]
        ts.sort()
        d3 = ((np.arange(n) // 23) % 3).astype(np.uint32)
        ok_ts = np.repeat(rng.random((n + 99) // 100) >= 0.04, 100)[:n]
        ok_d3 = np.repeat(rng.random((n + 22) // 23) >= 0.03, 23)[:n]
        plain = lambda hi: (rng.integers(0, hi, n).astype(np.uint32), rng.random(n) >= 0.03)
        return {"ts": (abi.Uint32, np.where(ok_ts, ts, 0).astype(np.uint32), ok_ts, True), "d3": (abi.Uint32, d3, ok_d3, True),
                "d1": (abi.Uint32, *plain(100)), "d2": (abi.Uint32, *plain(50)), "m": (abi.Float32, hard_floats(rng, n), rng.random(n) >= 0.03)}

    shape = Shape("archive_float_sum", {}, [("ts", abi.GreaterThanOrEqual, 3600), ("ts", abi.LessThan, 150000), ("d1", abi.LessThan, 90)],
                  _C3_DIMS, ("col", "m"), abi.AGGR_SUM_FLOAT, abi.Float64, 8, _C3_NDW)
    batches = [archive(n) for n in (30000, 45000, 1200)]
    refs = references(oracle, shape, batches)
    for attempt in range(2):
        got, kernels = _kernels_of(hip, lambda: run_sequence(hip, shape, batches))
        assert_close(got, refs, shape)
    if _fusion_on():
        assert kernels["expand_runs_kernel"][0] == 2 * len(batches), kernels.get("expand_runs_kernel")
        assert _starts(kernels, "sr_scan_rtc") and not _starts(kernels, "transform", "filter_pred", "radix_pass"), sorted(kernels)


@pytest.mark.parametrize("eager", [False, True], ids=["scan_fed", "wide"])
@pytest.mark.parametrize("shape", [C3_SUM, MAX_F], ids=lambda s: s.name)
def test_a_host_that_looks_between_sort_and_reduce(shape, eager):
    """HashValues / IndexVector read between Sort and Reduce are the oracle's bytes (the lazy definition is materialised on
    demand), and the result is the oracle's."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    batches = _batches(shape, seed=99, sizes=(3000, 9000, 50))
    read = frozenset(("sorted", "after"))
    got = run_sequence(hip, shape, batches, read=read, eager=eager)
    assert_close(got, references(oracle, shape, batches, read=read, eager=eager), shape)
