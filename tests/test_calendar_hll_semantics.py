"""The eight calendar functors and GetHLLValue against the independent model of tests/edge_model.py: the calendar from the
proleptic Gregorian calendar (numpy's datetime64, itself checked against Python's datetime here), the HLL value from
MurmurHash3_x64_128 as published and the original's bit walk stated as a rotation.

Timestamps are every month boundary of 1970 ... 2106 with its neighbours, Feb 28 / Feb 29 / Mar 1 / Dec 31, the first four days
of the epoch and the seams at 2^31 and 2^32 (2100, the one non-leap century year a Uint32 reaches, included), plus a seeded
fill; HLL inputs are the pre-images of tests/golden/hll_preimages.json: every rho up to 17, and the inputs past the last bit
the original can probe (rho = 50), where a shift count that wraps would read the register bits instead (rho = 18, 19, 20 ...).  On the CPU the model is pinned to the C checker and to the reference's host build; on the GPU every kernel
that evaluates these functors (transform32_kernel, its load of a joined column included, filter_kernel and transform_wide_kernel) is compared
with the model bit for bit, as are two query plans that must decline the fused routes."""
import ctypes as C
import datetime
import json
import os

import numpy as np
import pytest

import edge_model as M
import harness as H
import test_edge_semantics as E
from aresdb_amd import abi, check, smoke
from aresdb_amd.executor import Col, DimensionSpec, QueryPlan, Unary
from test_edge_semantics import CPU, FILTER, TILE_ROWS, EdgeCase, Sink, Vec, _cpu_backend, kernel_log

FUNCTORS = M.CALENDAR + M.HLL_VALUE
COL_TYPES = E.COL_TYPES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hll_preimages.json")
FILL = 3000   # seeded random timestamps on top of the boundary pool


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _epoch(y, m, d):
    return (datetime.date(y, m, d).toordinal() - datetime.date(1970, 1, 1).toordinal()) * 86400


def boundary_timestamps():
    pts = {0, 1, 345599, 345600, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1}
    for y in range(1970, 2107):
        for m in range(1, 13):
            b = _epoch(y, m, 1)
            pts.update((b - 1, b, b + 1, b + 86399, b + 86400))
        leap = y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)
        for m, d in ((2, 28), (2, 29), (3, 1), (12, 31)):
            if (m, d) == (2, 29) and not leap:
                continue
            b = _epoch(y, m, d)
            pts.update((b - 1, b, b + 86399))
    return np.array(sorted(p for p in pts if 0 <= p < 2 ** 32), np.uint32)


BOUNDARY = boundary_timestamps()
PRE = json.load(open(GOLDEN))


def _preimages(name):
    p = PRE[name]
    return sorted({v for vs in p["by_rho"].values() for v in vs} | set(p["deep"]))


HLL_U32 = np.array(_preimages("uint32"), np.uint32)
HLL_I64 = np.array(_preimages("int64"), np.int64)
POOL32 = np.concatenate([BOUNDARY, np.random.default_rng(2106).integers(0, 2 ** 32, FILL).astype(np.uint32), HLL_U32])


def pool_of(dtype):
    """stored values of a column of `dtype`: timestamps and HLL pre-images for the 4-byte integers, the type's edge pool else"""
    if dtype == abi.Uint32:
        return POOL32
    if dtype == abi.Int32:
        return POOL32.view(np.int32)
    return E._np_pool(dtype)


# UUIDs whose lo ^ hi has its lowest set bit above the register bits at 14 + r (r = 50: none), under several registers
def uuid_pool():
    lo, hi = [], []
    for r in (0, 17, 18, 19, 31, 49, 50):
        for reg in (0, 1, 2, 0x2000, 0x3FFF, 0x1555):
            h = ((1 << (14 + r)) if r < 50 else 0) | reg
            for mask in (0, 0x0123456789ABCDEF, M.M64):
                lo.append(h ^ mask), hi.append(mask)
    return np.array(lo, np.uint64), np.array(hi, np.uint64)


def _wrapped_rho(h):
    """rho of a hash if the original's 32-bit shift count wrapped mod 32 (none of the reference's builds does that)"""
    rho = 0
    while rho + 14 < 64 and not (h & 0xFFFFFFFF) >> ((rho + 14) % 32) & 1:
        rho += 1
    return rho


def test_boundary_pool_and_preimages_are_what_the_issue_asks_for():
    assert 8000 < len(BOUNDARY) < 10000 and BOUNDARY[-1] == 2 ** 32 - 1
    assert _epoch(2100, 3, 1) - _epoch(2100, 2, 28) == 86400 and _epoch(2100, 2, 28) + 86399 in BOUNDARY
    for name, values, width in (("uint32", HLL_U32.astype(np.uint64), 4), ("int64", HLL_I64.view(np.uint64), 8)):
        h = M.murmur3_x64_128_low(values, width)
        rho = M.hll_from_hash(h) >> 16
        assert set(rho.tolist()) == set(range(18)) | {50}, name
        assert (rho >= 18).sum() >= 4, name
        wrapped = {_wrapped_rho(int(x)) for x in h[rho >= 18]}   # the reading these inputs must tell apart from the model's
        assert set(range(18, 21)) <= wrapped and 50 not in wrapped, (name, wrapped)
    lo, hi = uuid_pool()
    assert set((M.unary_wide(M.GetHLLValue, M.UUID, lo, hi, True)[0] >> 16).tolist()) == {0, 17, 50}
    assert {_wrapped_rho(int(x)) for x in lo ^ hi} >= {0, 17, 18, 19, 31, 50}


def test_model_calendar_is_pythons_datetime():
    """numpy's datetime64 (the model) against datetime / date.weekday on the whole pool: two calendars, no shared arithmetic"""
    epoch = datetime.datetime(1970, 1, 1)
    want = np.zeros((len(POOL32), 8), np.int64)
    for i, t in enumerate(POOL32.tolist()):
        d = epoch + datetime.timedelta(seconds=t)
        q = (d.month - 1) // 3
        want[i] = [0 if t < 345600 else _epoch(d.year, d.month, d.day) - d.weekday() * 86400, _epoch(d.year, d.month, 1),
                   _epoch(d.year, 3 * q + 1, 1), _epoch(d.year, 1, 1), d.day - 1, d.timetuple().tm_yday - 1, d.month - 1, q]
    for j, ft in enumerate(M.CALENDAR):
        got = M.calendar(ft, POOL32).astype(np.int64)
        assert np.array_equal(got, want[:, j]), (M.FUNCTOR_NAMES[1][ft], POOL32[got != want[:, j]][:3])


def test_model_murmur_and_bit_walk():
    """the model's hash on Python integers, on numpy uint64 and in aresdb_amd.check agree; the rotation is the original's walk"""
    keys = np.concatenate([HLL_U32[:50].astype(np.uint64), [0, 1, 2 ** 32 - 1]]).astype(np.uint64)
    for width, ks in ((4, keys), (8, np.concatenate([HLL_I64.view(np.uint64)[:50], keys])), (1, np.array([0, 1], np.uint64))):
        h = M.murmur3_x64_128_low(ks, width)
        assert [M.murmur3_x64_128_low(int(k), width) for k in ks] == [int(x) for x in h]
        rows = np.ascontiguousarray(ks.astype("<u8")).view(np.uint8).reshape(-1, 8)[:, :width]
        assert np.array_equal(check.murmur3_128_lo64_rows(np.ascontiguousarray(rows)), h)
    rng = np.random.default_rng(5)
    hs = np.concatenate([rng.integers(0, 2 ** 64, 2000, dtype=np.uint64), uuid_pool()[0], rng.integers(0, 2 ** 14, 500).astype(np.uint64),
                         rng.integers(0, 2 ** 32, 500, dtype=np.uint64) << np.uint64(32)])
    for h, got in zip(hs.tolist(), M.hll_from_hash(hs).tolist()):
        rho = 0
        while rho + 14 < 64 and not (rho + 14 < 32 and (h & 0xFFFFFFFF) >> (rho + 14) & 1):   # (no mask from bit 32 on)
            rho += 1
        assert got == rho << 16 | (h & 0x3FFF), hex(h)


# ---- operands the shared Vec does not carry -----------------------------------------------------------------------------
class WideVec:
    """An Int64 / UUID / GeoPoint column in mode 0, 1 or 2 (lo, hi: the value's two 8-byte halves as uint64)."""
    kind = "col"

    def __init__(self, dtype, lo, hi=None, valid=None, mode=1, default=None):
        self.dtype, self.valid, self.mode, self.default = dtype, valid, mode, default
        self.lo = np.asarray(lo, np.uint64)
        self.hi = np.zeros(len(self.lo), np.uint64) if hi is None else np.asarray(hi, np.uint64)
        self._built = {}

    def input(self, be):
        if be.name not in self._built:
            if self.mode == 0:
                self._built[be.name] = H.Column(be, self.dtype, default=self.default)
            else:
                raw = self.lo if self.dtype != abi.UUID else np.stack([self.lo, self.hi], 1)
                self._built[be.name] = H.Column(be, self.dtype, raw_values=np.ascontiguousarray(raw).tobytes(), valid=self.valid,
                                                starting_index=3 if self.valid is not None else 0)
        return self._built[be.name].input()

    def evaluate(self, ft, rows, n):
        if self.mode == 0:
            lo = np.full(n, 0 if self.default is None else self.default & M.M64, np.uint64)
            return M.unary_wide(ft, self.dtype, lo, np.zeros(n, np.uint64), np.full(n, self.default is not None)) + (lo,)
        ok = np.ones(len(self.lo), bool) if self.valid is None else np.asarray(self.valid, bool)
        r, rok = M.unary_wide(ft, self.dtype, self.lo[rows], self.hi[rows], ok[rows])
        return r, rok, self.lo[rows]

    def free(self):
        for b in self._built.values():
            b.free()
        self._built = {}

    def name(self):
        return f"col:{M.TYPE_NAMES[self.dtype]}:mode{self.mode}"


class ForeignVec:
    """A Uint32 column of a joined table read through RecordIDs (no timezone table): batches of (values, valid or None)."""
    kind, dtype = "foreign", abi.Uint32
    BASE = -2147483648

    def __init__(self, batches, rids, last):
        self.batches, self.rids, self.last = batches, rids, last
        self._built = {}

    def input(self, be):
        if be.name not in self._built:
            cols = [H.Column(be, abi.Uint32, v, valid=ok, starting_index=0 if ok is None else 5) for v, ok in self.batches]
            slices = (abi.VectorPartySlice * len(cols))(*[c.vp for c in cols])
            rids = H.Buf(be, H.record_id_array([(self.BASE + b, x) for b, x in self.rids]))
            self._built[be.name] = (cols, slices, rids)
        cols, slices, rids = self._built[be.name]
        iv = abi.InputVector()
        f = iv.Vector.ForeignVP
        f.RecordIDs, f.Batches = rids.ptr, C.addressof(slices)
        f.BaseBatchID, f.NumBatches, f.NumRecordsInLastBatch = self.BASE, len(cols), self.last
        f.TimezoneLookup, f.TimezoneLookupSize, f.DataType = None, 0, abi.Uint32
        iv.Type = abi.ForeignColumnInput
        return iv

    def evaluate(self, ft, rows, n):
        """output position i reads RecordID i; a record past the last batch's count is null"""
        bits, ok = np.zeros(n, np.uint32), np.zeros(n, bool)
        for i, (b, x) in enumerate(self.rids[:n]):
            if b < len(self.batches) - 1 or x < self.last:
                v, valid = self.batches[b]
                bits[i], ok[i] = v[x], True if valid is None else valid[x]
        bits = np.where(ok, bits, 0).astype(np.uint32)
        return M.unary(ft, M.K_U32, bits, ok) + (bits,)

    def free(self):
        for cols, _, rids in self._built.values():
            rids.free()
            for c in cols:
                c.free()
        self._built = {}

    def name(self):
        return "foreign:Uint32"


class OtherCase(EdgeCase):
    """EdgeCase over a WideVec or ForeignVec: the result is of the uint32 kind"""

    def evaluate(self):
        r, ok, a = self.a.evaluate(self.functor, self.index.astype(np.int64), self.n)
        return r, ok, M.K_U32, (a & np.uint64(M.M32)).astype(np.uint32), None, M.K_U32


# ---- case builders -----------------------------------------------------------------------------------------------------
def sinks_for(ft, offsets=(3, 1, 5, 1)):
    out = [FILTER, Sink("scratch", abi.Uint32), Sink("dim", abi.Uint32, offset=offsets[0]), Sink("dim", abi.Uint16, offset=offsets[1]),
           Sink("dim", abi.Uint8, offset=offsets[2])]
    return out + ([Sink("measure", abi.Uint32, M.AGGR_HLL, offset=offsets[3])] if ft == M.GetHLLValue else [])


def column(ta, ft, sink, shape, rows=None, for_ref=False, shift=0):
    """(Vec, row count) over pool_of(ta) minus what edge_model.UNDEFINED excludes (float results into integer sinks), or None.
    shape: 1, 2, 3 = the column's mode, "scratch" = a scratch vector.  `rows` given: a window of the pool starting at `shift`."""
    pa = pool_of(ta)
    pa = pa[E._result_defined(M.KIND_OF[ta], M.widen(pa, ta), None, None, ft, sink, unary=True, for_ref=for_ref)]
    if not len(pa):
        return None
    pa = np.roll(pa, -(shift % len(pa)))
    if shape == 3:   # run lengths 1, 2, 3, 1, ...
        vals = np.resize(pa, rows // 2 if rows else 2 * len(pa) + 1)
        counts = np.concatenate([[0], np.cumsum(1 + np.arange(len(vals)) % 3)]).astype(np.uint32)
        if rows:   # (the last run is stretched to the row count asked for)
            counts[-1] = max(rows, int(counts[-2]) + 1)
        return Vec("col", ta, vals, E._validity("alt", len(vals), len(pa)), mode=3, counts=counts), int(counts[-1])
    rows = rows or 2 * len(pa) + 5
    if shape == "scratch":
        return Vec("scratch", ta, np.resize(pa, rows), E._validity("alt", rows, len(pa))), rows
    return Vec("col", ta, np.resize(pa, rows), E._validity("alt", rows, len(pa)) if shape == 2 else None, mode=shape), rows


def shapes_of(ta):
    return [1, 2, 3] + (["scratch"] if ta in E.SCRATCH_TYPES else [])


def wide_vectors():
    """Int64: the 32-bit pool, the same values under high words (only the low word counts for the calendar) and the 8-byte HLL
    pre-images; UUID: the constructed lo ^ hi; GeoPoint: anything (always null)"""
    low = POOL32.astype(np.uint64)
    high = np.arange(len(low), dtype=np.uint64) * np.uint64(0x9E3779B1) << np.uint64(32) | np.uint64(1 << 63)
    i64 = np.concatenate([low, low | high, HLL_I64.view(np.uint64)])
    ulo, uhi = uuid_pool()
    geo = (M.f32_bits(np.float32([37.5, -90.0, 0.0])).astype(np.uint64) | M.f32_bits(np.float32([-122.25, 180.0, 0.0])).astype(np.uint64) << np.uint64(32))
    for mode in (1, 2):
        v = (lambda n: E._validity("alt", n, n // 2) if mode == 2 else None)  # noqa: E731
        yield WideVec(abi.Int64, np.resize(i64, 2 * len(i64) + 5), valid=v(2 * len(i64) + 5), mode=mode)
        yield WideVec(abi.UUID, np.resize(ulo, 2 * len(ulo) + 3), np.resize(uhi, 2 * len(ulo) + 3), valid=v(2 * len(ulo) + 3), mode=mode)
        yield WideVec(abi.GeoPoint, np.resize(geo, 9), valid=v(9), mode=mode)
    yield WideVec(abi.Int64, [0], mode=0, default=int(HLL_I64[-1]))
    yield WideVec(abi.Int64, [0], mode=0, default=None)


def wide_cases(be):
    ran = 0
    for a in wide_vectors():
        n = len(a.lo) if a.mode else 9
        for ft in FUNCTORS:
            for sink in (Sink("scratch", abi.Uint32), Sink("dim", abi.Uint32, offset=3), Sink("measure", abi.Uint32, M.AGGR_HLL, offset=1)):
                if sink.kind == "measure" and ft != M.GetHLLValue:
                    continue
                OtherCase(a, None, ft, sink, E._style_index(["identity", "subset", "perm"][(ft + ran) % 3] if a.mode else "identity", n, seed=ft)).check(be)
                ran += 1
        a.free()
    return ran


def foreign_cases(be):
    """GetMonthStart, GetDayOfMonth and GetHLLValue over RecordIDs that walk two batches of the pool; the second batch has nulls
    and three records lie past its record count"""
    half = len(POOL32) // 2
    b0, b1 = POOL32[:half], POOL32[half:]
    ok1 = np.arange(len(b1)) % 7 != 3
    last = len(b1) - 3
    rng = np.random.default_rng(11)
    rids = [(0, int(x)) for x in rng.permutation(half)] + [(1, int(x)) for x in rng.permutation(len(b1))]
    rids = [rids[i] for i in rng.permutation(len(rids))]
    a, ran = ForeignVec([(b0, None), (b1, ok1)], rids, last), 0
    for ft in (M.GetMonthStart, M.GetDayOfMonth, M.GetHLLValue):
        for sink in sinks_for(ft)[1:]:
            for n in (len(rids), TILE_ROWS[ran % 2]):
                OtherCase(a, None, ft, sink, np.arange(n, dtype=np.uint32)).check(be)
                ran += 1
    a.free()
    return ran


def filter_with_record_ids(be, a, ft, rows, seed):
    """UnaryFilter over a subset index with two RecordID vectors to compact: survivors, index and RecordIDs against the model"""
    index = E._style_index("subset", rows, seed=seed)
    case = EdgeCase(a, None, ft, FILTER, index)
    r, ok, rk = case.evaluate()[:3]
    keep = M.convert(r, rk, M.K_BOOL) != 0
    rng = np.random.default_rng(seed)
    rids = [np.stack([rng.integers(1, 5, len(index)), rng.integers(0, 1000, len(index))], 1).astype(np.uint32) for _ in range(2)]
    idx, pred, rbufs = H.Buf(be, index), H.Buf(be, nbytes=len(index) + 8), [H.Buf(be, x) for x in rids]
    vecs = (C.c_void_p * 2)(*[b.ptr for b in rbufs])
    count = be.call("UnaryFilter", a.input(be), idx.ptr, pred.ptr, len(index), C.addressof(vecs), 2, None, 0, ft, None, 0)
    assert count == int(keep.sum()), (case, count, int(keep.sum()))
    assert np.array_equal(pred.read(np.uint8, len(index)), keep.astype(np.uint8)), case
    assert np.array_equal(idx.read(np.uint32, count), index[keep]), case
    for b, x in zip(rbufs, rids):
        assert np.array_equal(b.read(np.uint32, 2 * count).reshape(-1, 2), x[keep]), case
    for b in [idx, pred] + rbufs:
        b.free()
    return keep, case


def filter_cases(be):
    ran = 0
    for ft in FUNCTORS:
        for ta in COL_TYPES:
            for shape in (1, 2):
                a, rows = column(ta, ft, FILTER, shape)
                keep, case = filter_with_record_ids(be, a, ft, rows, seed=ft + ta)
                if ta == abi.Uint32 and shape == 1 and ft in (M.GetDayOfMonth, M.GetWeekStart):
                    ts = POOL32[np.resize(np.arange(len(POOL32)), rows)[case.index]]
                    must_drop = (ts < 345600) if ft == M.GetWeekStart else np.isin(ts, [_epoch(y, m, 1) for y in (1970, 2000, 2100) for m in range(1, 13)])
                    assert must_drop.any() and not keep[must_drop].any() and keep.any(), case
                a.free()
                ran += 1
    return ran


# ---- CPU: the model against the C checker and the reference's host build --------------------------------------------------
@CPU
@pytest.mark.parametrize("ta", COL_TYPES, ids=lambda t: M.TYPE_NAMES[t])
def test_model_calendar_and_hll_value_on_columns(which, ta):
    """every functor x modes 1, 2, 3 and a scratch operand x every sink, over the whole pool of the column type"""
    be, ref, ran = _cpu_backend(which), which == "ref", 0
    for ft in FUNCTORS:
        for shape in shapes_of(ta):
            for sink in sinks_for(ft):
                built = column(ta, ft, sink, shape, for_ref=ref)
                if built is None:
                    continue
                a, rows = built
                EdgeCase(a, None, ft, sink, E._style_index("identity", rows)).check(be)
                a.free()
                ran += 1
    print(f"{which} {M.TYPE_NAMES[ta]}: {ran} cases")
    assert ran > 130   # (9 functors x 3 shapes x 5 sinks, + the HLL measure)


@CPU
def test_model_constants_defaults_and_run_length_location(which):
    """a null and a valid constant (int32 kind: -1 is 2106), float constants (handed back), mode-0 columns with and without a
    default; a run-length column located through baseCounts and through startCount"""
    be, ran = _cpu_backend(which), 0
    for b in (Vec("cint", value=-1), Vec("cint", value=951782400), Vec("cint", value=5, const_valid=False), Vec("cfloat", value=np.float32(86400.0)),
              Vec("col", abi.Uint32, mode=0, value=4107542400), Vec("col", abi.Int16, mode=0, value=-2), Vec("col", abi.Bool, mode=0, value=True),
              Vec("col", abi.Uint32, mode=0, value=None), Vec("col", abi.Float32, mode=0, value=1.5)):
        for ft in FUNCTORS:
            for sink in (FILTER, E.natural_sink(b.model_kind(), None, ft, arity=1)):
                EdgeCase(b, None, ft, sink, E._style_index("identity", 9)).check(be)
                ran += 1
        b.free()
    ran += run_length_location(be)
    print(f"{which}: {ran} cases")
    assert ran > 150


def run_length_location(be):
    ran = 0
    for ft in FUNCTORS:
        for ta in (abi.Uint32, abi.Int32, abi.Int16):
            sink = sinks_for(ft)[1 + ft % 2]
            a, rows = column(ta, ft, sink, 3)
            n = rows // 2
            base = np.sort(np.random.default_rng(ft).choice(rows, n + 1, replace=False)).astype(np.uint32)
            EdgeCase(a, None, ft, sink, E._style_index("perm", n, seed=ft), base_counts=base, locate=True).check(be)
            EdgeCase(a, None, ft, sink, E._style_index("subset", n, seed=ft), start_count=rows - n).check(be)
            a.free()
            ran += 2
    return ran


@CPU
def test_model_wide_and_foreign_inputs(which):
    """Int64 (low word for the calendar, 8 hashed bytes for GetHLLValue), UUID (lo ^ hi unhashed), GeoPoint (null), null rows
    and mode 0; a Uint32 column of a joined table through RecordIDs.  Uint64 columns are not admitted by the ABI."""
    be = _cpu_backend(which)
    ran = wide_cases(be) + foreign_cases(be)
    print(f"{which}: {ran} cases")
    assert ran > 100


@CPU
def test_model_filters_compact_index_and_record_ids(which):
    ran = filter_cases(_cpu_backend(which))
    print(f"{which}: {ran} cases")
    assert ran >= 9 * 8 * 2


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ta", COL_TYPES, ids=lambda t: M.TYPE_NAMES[t])
def test_hip_transform32_calendar_and_hll_value(ta):
    """transform32_kernel: every functor x modes 1, 2, 3 and scratch x every sink at unaligned offsets; the full pool and the
    ragged tile row counts, identity / subset / permuted index vectors"""
    be, ran = H.hip_backend(), 0
    with kernel_log(be) as kernels:
        for ft in FUNCTORS:
            for si, shape in enumerate(shapes_of(ta)):
                for k, sink in enumerate(sinks_for(ft, offsets=(1 + ft % 7, 1 + (ft + si) % 3, 5 - si, 1 + si))[1:]):
                    built = column(ta, ft, sink, shape, rows=[None, TILE_ROWS[0], TILE_ROWS[1]][(ft + si + k) % 3], shift=1009 * (ft + k))
                    if built is None:
                        continue
                    a, rows = built
                    EdgeCase(a, None, ft, sink, E._style_index(["identity", "subset", "perm"][(ft + k) % 3], rows, seed=ft)).check(be)
                    a.free()
                    ran += 1
        ran += run_length_location(be) if ta == abi.Uint32 else 0
    print(f"{M.TYPE_NAMES[ta]}: {ran} cases")
    assert ran > (60 if ta == abi.Float32 else 100)
    assert kernels == {"transform32_kernel"}, kernels


@pytest.mark.gpu
def test_hip_filter_kernel_calendar_and_hll_value():
    """filter_kernel: each functor as the root of a UnaryFilter; survivors, compacted index and RecordID vectors.  The first of
    a month under GetDayOfMonth and the first four days of 1970 under GetWeekStart are rows that must drop."""
    be = H.hip_backend()
    with kernel_log(be) as kernels:
        ran = filter_cases(be)
    print(f"{ran} cases")
    assert ran >= 9 * 8 * 2
    assert "filter_kernel" in kernels and not kernels & E.FAST_FILTERS, kernels


@pytest.mark.gpu
def test_hip_transform_wide_kernel_calendar_and_hll_value():
    be = H.hip_backend()
    with kernel_log(be) as kernels:
        ran = wide_cases(be)
    print(f"{ran} cases")
    assert ran > 100
    assert "transform_wide_kernel" in kernels and not kernels & E.FAST_TRANSFORMS, kernels


@pytest.mark.gpu
def test_hip_foreign_column_calendar_and_hll_value():
    """a joined column under a functor is transform32_kernel's OP_FOREIGN load (RecordIDs across two batches, null rows, records
    past the last batch's count); transform_foreign_kernel itself takes Noop only and never evaluates these functors"""
    be = H.hip_backend()
    with kernel_log(be) as kernels:
        ran = foreign_cases(be)
    print(f"{ran} cases")
    assert ran >= 20
    assert kernels == {"transform32_kernel"}, kernels


# ---- plans ---------------------------------------------------------------------------------------------------------------
PLAN_ROWS = (120000, 1, 80003)
# the scans that evaluate a plan's expressions themselves (sr_vector_scan_rtc only hashes the dimension vector the transforms wrote)
FUSED_SCANS = {"hr_scan_rtc", "hr_table_scan_rtc", "hr_fused_scan_kernel", "sr_scan_rtc"}


def plan_batches():
    """ts walks the whole pool and then a seeded fill; user walks the HLL pre-images among random ids; m is any Uint32"""
    rng = np.random.default_rng(1970)
    total = sum(PLAN_ROWS)
    ts = np.concatenate([POOL32, rng.integers(0, 2 ** 32, total - len(POOL32)).astype(np.uint32)])[rng.permutation(total)]
    user = np.where(np.arange(total) % 5 == 0, np.resize(HLL_U32, total), rng.integers(0, 50000, total).astype(np.uint32))
    m = rng.integers(0, 2 ** 32, total).astype(np.uint32)
    out, at = [], 0
    for n in PLAN_ROWS:
        s = slice(at, at + n)
        out.append(({"ts": (abi.Uint32, ts[s]), "user": (abi.Uint32, user[s]), "m": (abi.Uint32, m[s])},
                    {"ts": np.arange(at, at + n) % 13 != 0, "user": None, "m": np.arange(at, at + n) % 17 != 0}))
        at += n
    return out


def calendar_plan(use_hash):
    return QueryPlan(filters=[], dimensions=[DimensionSpec(Unary(abi.GetMonthStart, Col("ts")), abi.Uint32),
                                             DimensionSpec(Unary(abi.GetDayOfYear, Col("ts")), abi.Uint16)],
                     measure=Col("m"), agg=abi.AGGR_SUM_SIGNED, measure_type=abi.Int64, use_hash_reduction=use_hash)


def hll_plan(use_hash):
    return QueryPlan(filters=[], dimensions=[DimensionSpec(Unary(abi.GetWeekStart, Col("ts")), abi.Uint32)],
                     measure=Unary(abi.GetHLLValue, Col("user")), agg=abi.AGGR_HLL, measure_type=abi.Uint32, use_hash_reduction=use_hash)


def _model_rows(plan, batches):
    """(packed key of every row: value bytes and validity of each dimension; the row's stored measure element)"""
    keys, meas = [], []
    for cols, valid in batches:
        n = len(cols["ts"][1])
        parts = []
        for d in plan.dimensions:
            bits = M.widen(cols["ts"][1], abi.Uint32)
            r, ok = M.unary(d.expr.op, M.K_U32, bits, valid["ts"])
            parts += [M.store_typed(d.data_type, r, M.K_U32), ok.astype(np.uint8).reshape(-1, 1)]
        keys.append(np.hstack(parts))
        if plan.is_hll:
            r, ok = M.unary(M.GetHLLValue, M.K_U32, M.widen(cols["user"][1], abi.Uint32), np.ones(n, bool))
            meas.append(r)
        else:
            meas.append(M.store_measure(plan.measure_type, plan.agg, M.widen(cols["m"][1], abi.Uint32), valid["m"], M.K_U32).view(np.uint64).reshape(n))
    return np.vstack(keys), np.concatenate(meas)


def _key_tuples(plan, keys):
    """the {((value bytes, valid), ...)} keys of smoke.run_query from the packed rows"""
    out, at = [], 0
    for d in plan.dimensions:
        w = d.width
        out.append([(bytes(k[at:at + w]), int(k[at + w])) for k in keys])
        at += w + 1
    return list(zip(*out))


def check_calendar_plan(be, plan, batches, run=smoke.run_query):
    got, _ = run(be, plan, batches)
    keys, meas = _model_rows(plan, batches)
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)
    sums = np.zeros(len(uniq), np.uint64)
    np.add.at(sums, inv.reshape(-1), meas)
    want = dict(zip(_key_tuples(plan, uniq), sums.tolist()))
    assert got.keys() == want.keys(), (len(got), len(want), sorted(set(got) ^ set(want))[:3])
    bad = [(k, int(got[k]) % 2 ** 64, v) for k, v in want.items() if int(got[k]) % 2 ** 64 != v]
    assert not bad, bad[:3]
    return len(want)


def check_hll_plan(be, plan, batches):
    got, _ = smoke.run_hll_query(be, plan, batches)
    keys, vals = _model_rows(plan, batches)
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = inv.reshape(-1).astype(np.int64)
    pair = np.unique(inv << 16 | (vals & 0xFFFF).astype(np.int64))   # (group, register) pairs
    best = np.zeros(len(pair), np.int64)
    np.maximum.at(best, np.searchsorted(pair, inv << 16 | (vals & 0xFFFF).astype(np.int64)), (vals >> 16).astype(np.int64))
    want = {k: [] for k in _key_tuples(plan, uniq)}
    names = list(want)
    for p, r in zip(pair.tolist(), best.tolist()):
        want[names[p >> 16]].append((p & 0xFFFF, r + 1))   # (the encoded vector holds rho + 1: query/hll.cu)
    assert max(len(v) for v in want.values()) >= 4096 > min(len(v) for v in want.values())   # both encodings are met
    assert got.keys() == want.keys(), (len(got), len(want), sorted(set(got) ^ set(want))[:3])
    bad = [(k, got[k][:4], v[:4]) for k, v in want.items() if got[k] != v]
    assert not bad, bad[:3]
    return len(want)


@pytest.mark.parametrize("use_hash", [False, True], ids=["sort_reduce", "hash_reduce"])
def test_model_plans_on_the_checker(use_hash):
    data = plan_batches()
    assert check_calendar_plan(H.oracle_backend(), calendar_plan(use_hash), data) > 20000
    assert check_hll_plan(H.oracle_backend(), hll_plan(use_hash), data) > 5000


@pytest.mark.gpu
@pytest.mark.parametrize("native", [False, True], ids=["python_host", "native_driver"])
@pytest.mark.parametrize("use_hash", [False, True], ids=["sort_reduce", "hash_reduce"])
def test_hip_plan_with_calendar_dimensions(use_hash, native):
    """group by month start and day of year, SUM of an integer measure, >= 200 000 rows over the whole pool: the fused scans
    cannot evaluate a calendar functor, so they must decline and transform32_kernel must have written the dimensions"""
    be, data = H.hip_backend(), plan_batches()
    run = smoke.run_query_native if native else smoke.run_query
    run(be, calendar_plan(use_hash), data[1:2])   # (kernels built, as a query's first batch does)
    with kernel_log(be) as kernels:
        groups = check_calendar_plan(be, calendar_plan(use_hash), data, run)
    print(f"{groups} groups; kernels {sorted(kernels)}")
    assert groups > 20000
    assert "transform32_kernel" in kernels and not kernels & FUSED_SCANS, kernels


@pytest.mark.gpu
@pytest.mark.parametrize("use_hash", [False, True], ids=["sort_reduce", "hash_reduce"])
def test_hip_plan_with_week_dimension_and_hll_measure(use_hash):
    """group by week start, count distinct users: the register sets of every group against the model"""
    be, data = H.hip_backend(), plan_batches()
    with kernel_log(be) as kernels:
        groups = check_hll_plan(be, hll_plan(use_hash), data)
    print(f"{groups} groups; kernels {sorted(kernels)}")
    assert groups > 5000
    assert "transform32_kernel" in kernels and not kernels & FUSED_SCANS, kernels
