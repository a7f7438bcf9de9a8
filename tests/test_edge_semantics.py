"""Operator and aggregate semantics at the edges of their types, through every evaluator, against an exact model
(tests/edge_model.py) that shares no code with any of them.

Every case is the cross product of the operand pools (edge_model.EDGE_POOLS: type extremes, powers of two and their
neighbours, IEEE specials), minus the pairs edge_model.UNDEFINED lists, repeated to the row count asked for.  On the CPU
the model is pinned to the C checker and to the reference's own host build; on the GPU each of the four hand-written
evaluators (generic kernels, fast kernels, precompiled fused scan, generated scans and merges) is compared with the model
bit for bit, and each test proves from the kernel log which kernel it exercised."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_model as M
import harness as H
from aresdb_amd import abi, smoke
from aresdb_amd.executor import Binary, Col, Const, DimensionSpec, QueryPlan
from test_hip_parity import hash_path  # noqa: F401  (the fixture that selects, and proves, the HashReduce implementation)

INT_TYPES = [abi.Int8, abi.Uint8, abi.Int16, abi.Uint16, abi.Int32, abi.Uint32]
COL_TYPES = [abi.Bool] + INT_TYPES + [abi.Float32]
SCRATCH_TYPES = [abi.Int32, abi.Uint32, abi.Float32]
DIM_TYPES = [abi.Bool] + INT_TYPES + [abi.Float32]
MEASURE_TYPES = [abi.Int32, abi.Uint32, abi.Float32, abi.Int64, abi.Float64]
AGGS = [M.SUM_UNSIGNED, M.SUM_SIGNED, M.SUM_FLOAT, M.MIN_UNSIGNED, M.MIN_SIGNED, M.MIN_FLOAT, M.MAX_UNSIGNED, M.MAX_SIGNED,
        M.MAX_FLOAT, M.AVG_FLOAT]
TILE_ROWS = [4099, 8197]  # the row counts of test_hip_parity.FAST_ROWS that exceed a pool product's tile: ragged ends past 4096 / 8192


def _np_pool(dtype):
    return np.array(M.EDGE_POOLS[dtype], bool if dtype == abi.Bool else H._NP_OF[dtype])


def _validity(pattern, n, period):
    """all-valid (None) / alternating, flipping phase with every repetition of the product / one null"""
    if pattern == "all":
        return None
    r = np.arange(n)
    if pattern == "alt":
        return (r + r // max(period, 1)) % 2 == 0
    v = np.ones(n, bool)
    v[min(1, n - 1)] = False
    return v


class Vec:
    """One operand: a column (modes 0-3), a scratch vector or a constant; device copies are built once per backend."""

    def __init__(self, kind, dtype=None, values=None, valid=None, mode=1, counts=None, value=None, const_valid=True):
        self.kind, self.dtype, self.values, self.valid, self.mode, self.counts = kind, dtype, values, valid, mode, counts
        self.value, self.const_valid = value, const_valid
        self._built = {}

    def model_kind(self):
        if self.kind == "cint":
            return M.K_I32
        if self.kind == "cfloat":
            return M.K_F32
        return M.KIND_OF[self.dtype]

    def rows(self, rows, n, located=None):
        """(bits, validity) at output positions 0..n-1 whose table rows are `rows`; `located`: where the call's baseCounts /
        startCount put those rows in a run-length column's uncompressed space (the rows themselves by default)"""
        if self.kind == "cint":
            return np.full(n, M.u32(self.value), np.uint32), np.full(n, self.const_valid)
        if self.kind == "cfloat":
            return np.full(n, M.f32_bits(np.float32(self.value)), np.uint32), np.full(n, self.const_valid)
        if self.kind == "scratch":
            return M.widen(self.values, self.dtype)[:n], np.asarray(self.valid, bool)[:n]
        if self.mode == 0:   # the column is its default value
            return np.full(n, M.widen(np.array([self.value if self.value is not None else 0]), self.dtype)[0], np.uint32), \
                np.full(n, self.value is not None)
        phys = np.searchsorted(self.counts, rows if located is None else located, side="right") - 1 if self.mode == 3 else rows
        bits = M.widen(self.values, self.dtype)[phys]
        return bits, (np.ones(n, bool) if self.valid is None else np.asarray(self.valid, bool)[phys])

    def input(self, be):
        if self.kind == "cint":
            return H.const_int(self.value, self.const_valid)
        if self.kind == "cfloat":
            iv = H.const_float(0.0, self.const_valid)   # the exact bits, NaN payload and -0.0 included
            iv.Vector.Constant.Value.FloatVal = C.c_float(float(self.value)).value
            return iv
        if be.name not in self._built:
            if self.kind == "scratch":
                self._built[be.name] = H.Scratch(be, len(self.values), self.dtype, self.values, self.valid)
            elif self.mode == 0:
                self._built[be.name] = H.Column(be, self.dtype, default=self.value)
            else:
                self._built[be.name] = H.Column(be, self.dtype, self.values, valid=self.valid, counts=self.counts,
                                                starting_index=3 if (self.valid is not None or self.dtype == abi.Bool) and
                                                self.mode != 1 or self.dtype == abi.Bool else 0)
        return self._built[be.name].input()

    def free(self):
        for b in self._built.values():
            b.free()
        self._built = {}

    def name(self):
        if self.kind in ("cint", "cfloat"):
            return f"{self.kind}({self.value!r}{'' if self.const_valid else ', null'})"
        return f"{self.kind}:{M.TYPE_NAMES[self.dtype]}" + (f":mode{self.mode}" if self.kind == "col" else "")


class Sink:
    def __init__(self, kind, dtype=None, agg=None, offset=0):
        self.kind, self.dtype, self.agg, self.offset = kind, dtype, agg, offset

    def name(self):
        return self.kind + (f":{M.TYPE_NAMES[self.dtype]}" if self.dtype is not None else "") + (f":agg{self.agg}" if self.agg else "")


FILTER = Sink("filter")


class EdgeCase:
    """One ABI call over prepared operands, with the `run(be) -> dict` contract of tests/cases.py, and `expect()`: the same
    dict from the model."""

    def __init__(self, a, b, functor, sink, index, base_counts=None, init_index=False, start_count=0, locate=False):
        self.a, self.b, self.functor, self.sink = a, b, functor, sink
        self.start_count, self.locate = start_count, locate or start_count != 0   # locate: run-length operands follow base_counts
        self.index, self.n, self.base_counts, self.init_index = np.asarray(index, np.uint32), len(index), base_counts, init_index

    def __repr__(self):
        names = M.FUNCTOR_NAMES[1 if self.b is None else 2]
        return f"EdgeCase({self.a.name()} {names[self.functor]} {self.b.name() if self.b else ''} -> {self.sink.name()}, n={self.n})"

    def evaluate(self):
        """(result bits, validity, result kind, a bits, b bits, common kind) per output position"""
        rows = self.index.astype(np.int64)
        located = None if not self.locate else self.base_counts.astype(np.int64)[rows] if self.base_counts is not None \
            else rows + self.start_count
        a, aok = self.a.rows(rows, self.n, located)
        if self.b is None:
            k = self.a.model_kind()
            r, ok = M.unary(self.functor, k, a, aok)
            return r, ok, M.unary_result_kind(self.functor, k), a, None, k
        b, bok = self.b.rows(rows, self.n)
        k = M.common_kind(self.a.model_kind(), self.b.model_kind())
        ca, cb = M.convert(a, self.a.model_kind(), k), M.convert(b, self.b.model_kind(), k)
        r, ok = M.binary(self.functor, k, ca, aok, cb, bok)
        return r, ok, M.binary_result_kind(self.functor, k), ca, cb, k

    def expect(self):
        r, ok, rk = self.evaluate()[:3]
        s, n = self.sink, self.n
        if s.kind == "filter":
            keep = M.convert(r, rk, M.K_BOOL) != 0
            pred = np.zeros(n + 8, np.uint8)
            pred[:n] = keep
            return {"count": int(keep.sum()), "pred": pred, "index": self.index[keep]}
        if s.kind == "scratch":
            return {"ret": n, "values": M.store_typed(s.dtype, r, rk).reshape(-1), "valid": ok.astype(np.uint8)}
        w, off = abi.DATA_TYPE_BYTES[s.dtype], s.offset
        values = np.zeros(w * (n + off) + 8, np.uint8)
        if s.kind == "dim":
            values[w * off:w * (off + n)] = M.store_typed(s.dtype, r, rk).reshape(-1)
            valid = np.zeros(n + off + 8, np.uint8)
            valid[off:off + n] = ok
            return {"ret": n, "values": values, "valid": valid}
        counts = None if self.base_counts is None else np.diff(self.base_counts.astype(np.int64))[self.index]
        values[w * off:w * (off + n)] = M.store_measure(s.dtype, s.agg, r, ok, rk, counts).reshape(-1)
        return {"ret": n, "values": values}

    def run(self, be):
        ins = [self.a.input(be)] + ([self.b.input(be)] if self.b is not None else [])
        s, n = self.sink, self.n
        idx = H.Buf(be, self.index)
        bc = H.Buf(be, self.base_counts) if self.base_counts is not None else None
        keep = [idx] + ([bc] if bc else [])
        res = {}
        if s.kind == "filter":
            pred = H.Buf(be, nbytes=n + 8)
            keep.append(pred)
            if self.init_index:   # an index vector the library has numbered itself: filters are counted in row space
                be.call("InitIndexVector", idx.ptr, 0, n, None, 0)
            res["count"] = be.call("UnaryFilter" if self.b is None else "BinaryFilter", *ins, idx.ptr, pred.ptr, n, None, 0,
                                   bc.ptr if bc else None, self.start_count, self.functor, None, 0)
            res["pred"] = pred.read(np.uint8, n + 8)
            res["index"] = idx.read(np.uint32, res["count"])
        else:
            if s.kind == "scratch":
                sc = H.Scratch(be, n, s.dtype)
                keep.append(sc)
                ov = sc.output()
                read = lambda: {"values": sc.buf.read(np.uint8, 4 * n), "valid": sc.valid()}  # noqa: E731
            else:
                w, off = abi.DATA_TYPE_BYTES[s.dtype], s.offset
                vb = H.Buf(be, nbytes=w * (n + off) + 8)
                keep.append(vb)
                if s.kind == "dim":
                    nb = H.Buf(be, nbytes=n + off + 8)
                    keep.append(nb)
                    ov = H.dimension_output(vb.ptr + w * off, nb.ptr + off, s.dtype)
                    read = lambda: {"values": vb.read(np.uint8, w * (n + off) + 8), "valid": nb.read(np.uint8, n + off + 8)}  # noqa: E731
                else:
                    ov = H.measure_output(vb.ptr + w * off, s.dtype, s.agg)
                    read = lambda: {"values": vb.read(np.uint8, w * (n + off) + 8)}  # noqa: E731
            res["ret"] = be.call("UnaryTransform" if self.b is None else "BinaryTransform", *ins, ov, idx.ptr, n,
                                 bc.ptr if bc else None, self.start_count, self.functor, None, 0)
            res.update(read())
        for k in keep:
            k.free()
        return res

    def explain(self, got, want, who):
        """None when equal; else a message naming the first differing (a, b, functor, types)"""
        if got.keys() != want.keys():
            return f"{self!r}: {who} returned {sorted(got)} for {sorted(want)}"
        for key in ("pred", "valid", "values", "count", "ret", "index"):
            if key not in want:
                continue
            g, w = got[key], want[key]
            if not isinstance(w, np.ndarray):
                if g == w:
                    continue
                return f"{self!r}: {key} {who} {g!r} != model {w!r}"
            if g.shape == w.shape and np.array_equal(g, w):
                continue
            if g.shape != w.shape:
                return f"{self!r}: {key} has shape {g.shape} on {who}, {w.shape} in the model"
            at = int(np.flatnonzero(g != w)[0])
            per = {"pred": 1, "valid": 1, "index": 1}.get(key) or (4 if self.sink.kind == "scratch" else abi.DATA_TYPE_BYTES[self.sink.dtype])
            i = at // per - (self.sink.offset if key != "index" and self.sink.kind in ("dim", "measure") else 0)
            if not 0 <= i < self.n:
                return f"{self!r}: {key} byte {at} OUTSIDE the output range differs: {who} {int(g[at])} != model {int(w[at])}"
            r, ok, rk, a, b, k = self.evaluate()
            lo = i * per + (self.sink.offset * per if key != "index" and self.sink.kind in ("dim", "measure") else 0)
            return (f"{self!r}: {key}[{i}] (row {int(self.index[i])}): a={M.describe(a[i], k)}"
                    + (f" b={M.describe(b[i], k)}" if b is not None else "") + f" as {M.KIND_NAMES[k]}: {who} "
                    f"{bytes(g[lo:lo + per]).hex()} != model {bytes(w[lo:lo + per]).hex()} (result {M.describe(r[i], rk)}, valid {bool(ok[i])})")
        return None

    def check(self, be):
        msg = self.explain(self.run(be), self.expect(), be.name)
        assert msg is None, msg


# ---- case builders ---------------------------------------------------------------------------------------------------
def _result_defined(ka, a, kb, b, ft, sink, unary=False, for_ref=False):
    """pairs (bits of their own kinds) that edge_model.UNDEFINED does not exclude — the only filter on values in this file"""
    if unary:
        r, _ = M.unary(ft, ka, a, True)
        ok, rk = np.ones(len(a), bool), M.unary_result_kind(ft, ka)
        if for_ref:
            ok &= ~M.signed_overflow(ft, ka, a)
    else:
        k = M.common_kind(ka, kb)
        ca, cb = M.convert(a, ka, k), M.convert(b, kb, k)
        ok = M.binary_defined(ft, k, ca, cb)
        r, _ = M.binary(ft, k, ca, True, cb, True)
        rk = M.binary_result_kind(ft, k)
        if for_ref:
            ok &= ~M.signed_overflow(ft, k, ca, cb)
    if sink.dtype is not None:
        ok &= M.store_defined(sink.dtype, r, rk)
    return ok


def _style_index(style, rows, seed=0):
    if style == "identity":
        return np.arange(rows, dtype=np.uint32)
    rng = np.random.default_rng(seed)
    if style == "subset":
        idx = np.flatnonzero(rng.random(rows) > 0.4).astype(np.uint32)
        return idx if len(idx) else np.array([0], np.uint32)
    return rng.permutation(rows).astype(np.uint32)


def pair_vectors(ta, tb, ft, sink, rows=None, for_ref=False, b_kind="col", a_mode=2, b_mode=1, pattern="alt"):
    """column ta (x) column / scratch vector tb over pool x pool, or None when no pair is defined"""
    pa, pb = _np_pool(ta), _np_pool(tb)
    A, B = np.repeat(pa, len(pb)), np.tile(pb, len(pa))
    ok = _result_defined(M.KIND_OF[ta], M.widen(A, ta), M.KIND_OF[tb], M.widen(B, tb), ft, sink, for_ref=for_ref)
    A, B = A[ok], B[ok]
    if not len(A):
        return None
    period = len(A)
    rows = rows or 2 * period + 5
    A, B = np.resize(A, rows), np.resize(B, rows)
    a = Vec("col", ta, A, _validity(pattern, rows, period) if a_mode == 2 else None, mode=a_mode)
    if b_kind == "scratch":
        b = Vec("scratch", tb, B, _validity("one", rows, period))
    else:
        b = Vec("col", tb, B, _validity("one", rows, period) if b_mode == 2 else None, mode=b_mode)
    return a, b


def column_for_constant(ta, b, ft, sink, rows=None, mode=2, pattern="alt", for_ref=False, extra=None):
    """column ta over its pool (plus `extra` values), minus the values undefined against constant operand b"""
    pa = _np_pool(ta)
    if extra is not None:
        pa = np.concatenate([pa, np.asarray(extra).astype(pa.dtype)])
    bbits, _ = b.rows(np.zeros(1, np.int64), 1)
    ok = _result_defined(M.KIND_OF[ta], M.widen(pa, ta), b.model_kind(), np.full(len(pa), bbits[0], np.uint32), ft, sink, for_ref=for_ref)
    pa = pa[ok]
    if not len(pa):
        return None
    rows = rows or 2 * len(pa) + 5
    return Vec("col", ta, np.resize(pa, rows), _validity(pattern, rows, len(pa)) if mode == 2 else None, mode=mode)


def unary_vector(ta, ft, sink, rows=None, mode=2, kind="col", for_ref=False, pattern="alt"):
    pa = _np_pool(ta)
    ok = _result_defined(M.KIND_OF[ta], M.widen(pa, ta), None, None, ft, sink, unary=True, for_ref=for_ref)
    pa = pa[ok]
    if not len(pa):
        return None
    if kind == "scratch":
        rows = rows or 2 * len(pa) + 5
        return Vec("scratch", ta, np.resize(pa, rows), _validity(pattern, rows, len(pa))), rows
    if mode == 3:   # run lengths 1, 2, 3, 1, ... over two repetitions of the pool
        vals = np.resize(pa, 2 * len(pa) + 1)
        counts = np.concatenate([[0], np.cumsum(1 + np.arange(len(vals)) % 3)]).astype(np.uint32)
        return Vec("col", ta, vals, _validity(pattern, len(vals), len(pa)), mode=3, counts=counts), int(counts[-1])
    rows = rows or 2 * len(pa) + 5
    return Vec("col", ta, np.resize(pa, rows), _validity(pattern, rows, len(pa)) if mode == 2 else None, mode=mode), rows


def natural_sink(kind_a, kind_b, ft, arity=2):
    """the scratch vector of the result's own kind (Uint32 for predicates)"""
    rk = M.binary_result_kind(ft, M.common_kind(kind_a, kind_b)) if arity == 2 else M.unary_result_kind(ft, kind_a)
    return Sink("scratch", {M.K_BOOL: abi.Uint32, M.K_I32: abi.Int32, M.K_U32: abi.Uint32, M.K_F32: abi.Float32}[rk])


def constants():
    return [Vec("cint", value=int(v)) for v in M.CONST_INT_POOL] + [Vec("cfloat", value=v) for v in M.CONST_FLOAT_POOL] + \
        [Vec("cint", value=7, const_valid=False)]


def all_sinks():
    out = [Sink("scratch", t) for t in SCRATCH_TYPES] + [Sink("dim", t, offset=3) for t in DIM_TYPES]
    out += [Sink("measure", t, g, offset=1) for t in MEASURE_TYPES for g in AGGS if M.identity_defined(g, t)
            and (g != M.AVG_FLOAT or t == abi.Float64)]
    return out


# ---- CPU: the model against the C checker and against the reference's host build ---------------------------------------
def _cpu_backend(which):
    if which == "ref":
        if not H.have_ref():
            pytest.skip("reference HOST build absent")
        return H.ref_backend()
    return H.oracle_backend()


CPU = pytest.mark.parametrize("which", ["oracle", "ref"])


@CPU
@pytest.mark.parametrize("ta", COL_TYPES, ids=lambda t: M.TYPE_NAMES[t])
def test_model_binary_functors_on_two_vectors(which, ta):
    """column (validity alternating) x column / scratch vector, pool x pool, all 17 functors, as filter and into scratch"""
    be, ref, ran = _cpu_backend(which), which == "ref", 0
    for tb, b_kind in [(t, "col") for t in COL_TYPES] + [(t, "scratch") for t in SCRATCH_TYPES]:
        for ft in M.BINARY:
            for sink in (FILTER, natural_sink(M.KIND_OF[ta], M.KIND_OF[tb], ft)):
                pair = pair_vectors(ta, tb, ft, sink, for_ref=ref, b_kind=b_kind, b_mode=1 + (ft + tb) % 2)
                if pair is None:
                    continue
                a, b = pair
                EdgeCase(a, b, ft, sink, _style_index("identity", len(a.values))).check(be)
                a.free(), b.free()
                ran += 1
    assert ran > 300


@CPU
@pytest.mark.parametrize("ta", COL_TYPES, ids=lambda t: M.TYPE_NAMES[t])
def test_model_column_against_every_constant(which, ta):
    """column (modes 1 and 2) x every constant of the pools (integer constants are int32, so a Uint32 column compares as
    int32), all functors, as filter and into scratch; a mode-0 column as the constant keeps its own kind"""
    be, ref, ran = _cpu_backend(which), which == "ref", 0
    consts = constants() + [Vec("col", abi.Uint32, mode=0, value=int(v)) for v in (0, 1, 3, 3600, 2 ** 31, 2 ** 32 - 1)] + \
        [Vec("col", abi.Uint32, mode=0, value=None)]
    for b in consts:
        for ft in M.BINARY:
            for sink in (FILTER, natural_sink(M.KIND_OF[ta], b.model_kind(), ft)):
                a = column_for_constant(ta, b, ft, sink, mode=1 + ft % 2, for_ref=ref)
                if a is None:
                    continue
                EdgeCase(a, b, ft, sink, _style_index("identity", len(a.values))).check(be)
                a.free()
                ran += 1
        b.free()
    assert ran > 1500


@CPU
def test_model_unary_functors(which):
    be, ref, ran = _cpu_backend(which), which == "ref", 0
    for ta in COL_TYPES:
        shapes = [("col", 1), ("col", 2), ("col", 3)] + ([("scratch", 0)] if ta in SCRATCH_TYPES else [])
        for kind, mode in shapes:
            for ft in M.UNARY:
                for sink in (FILTER, natural_sink(M.KIND_OF[ta], None, ft, arity=1)):
                    built = unary_vector(ta, ft, sink, mode=mode, kind=kind, for_ref=ref)
                    if built is None:
                        continue
                    a, rows = built
                    EdgeCase(a, None, ft, sink, _style_index("identity", rows)).check(be)
                    a.free()
                    ran += 1
    for b in (Vec("cint", value=-2 ** 31 + 1), Vec("cfloat", value=np.float32(-0.0)), Vec("cint", value=5, const_valid=False),
              Vec("col", abi.Uint16, mode=0, value=65535), Vec("col", abi.Int8, mode=0, value=None)):
        for ft in M.UNARY:
            EdgeCase(b, None, ft, natural_sink(b.model_kind(), None, ft, arity=1), _style_index("identity", 9)).check(be)
            ran += 1
        b.free()
    assert ran > 250


@CPU
@pytest.mark.parametrize("ta", COL_TYPES, ids=lambda t: M.TYPE_NAMES[t])
def test_model_every_sink(which, ta):
    """a result of every kind into every scratch type, dimension slot type and measure type x aggregate: bare columns in
    modes 1, 2 and 3 (run-length), sums of two columns, and measures scaled by a compressed base column's run lengths"""
    be, ref, ran = _cpu_backend(which), which == "ref", 0
    for sink in all_sinks():
        for mode in (1, 2, 3):
            built = unary_vector(ta, M.Noop, sink, mode=mode, for_ref=ref)
            if built is None:
                continue
            a, rows = built
            EdgeCase(a, None, M.Noop, sink, _style_index("subset" if mode == 2 else "identity", rows, seed=mode)).check(be)
            if sink.kind == "measure" and mode == 2:
                lens = 1 + np.arange(rows) % 4
                lens[rows // 2] = 3000000000 if sink.dtype in (abi.Uint32, abi.Int64, abi.Float64) and not ref else 5
                bc = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
                EdgeCase(a, None, M.Noop, sink, _style_index("identity", rows), base_counts=bc).check(be)
                ran += 1
            a.free()
            ran += 1
        for ft in (M.Plus, M.Multiply, M.Equal):
            pair = pair_vectors(ta, ta, ft, sink, for_ref=ref)
            if pair is None:
                continue
            a, b = pair
            EdgeCase(a, b, ft, sink, _style_index("identity", len(a.values))).check(be)
            a.free(), b.free()
            ran += 1
    assert ran > 150


# ---- GPU: each HIP evaluator against the model, with the kernel log as proof of which one ran ---------------------------
FAST_TRANSFORMS = {"transform_fast_kernel", "transform_multi_kernel"}   # (held-back root outputs launch as one multi kernel)
GENERIC_TRANSFORMS = {"transform32_kernel"}
FAST_FILTERS = {"filter_rows_kernel", "filter_pred_kernel"}
GENERIC_FILTERS = {"filter_kernel"}


@contextlib.contextmanager
def kernel_log(be):
    """names (template arguments stripped) of the kernels launched inside the block"""
    names = set()
    be.profiler_enable(True)
    try:
        yield names
        be.call("WaitForCudaStream", None, 0)
        names.update(k.split("<")[0] for k in be.profiler_report())
        if os.environ.get("ARES_EDGE_KERNEL_LOG"):   # diagnostics: which kernels each test saw, one line per test
            with open(os.environ["ARES_EDGE_KERNEL_LOG"], "a") as f:
                f.write(os.environ.get("PYTEST_CURRENT_TEST", "?") + " " + " ".join(sorted(names)) + "\n")
    finally:
        be.profiler_enable(False)


def gpu_constants():
    return [Vec("cint", value=v) for v in (-2 ** 31, -2 ** 31 + 1, -86400, -129, -7, -1, 0, 1, 2, 3, 7, 255, 3600, 65536, 86400,
                                           2 ** 24 + 1, 2 ** 31 - 1)] + \
        [Vec("cfloat", value=np.float32(v)) for v in (0.0, -0.0, 0.1, 3.0, 16777216.0, 2147483520.0, -2147483648.0, 1e-45, M.FLT_MAX,
                                                      np.inf, -np.inf, np.nan)] + [Vec("cint", value=7, const_valid=False)]


@pytest.mark.gpu
@pytest.mark.parametrize("ta", COL_TYPES, ids=lambda t: M.TYPE_NAMES[t])
def test_hip_generic_kernels_on_two_vectors(ta):
    """two-column and scratch-operand shapes never qualify for the fast kernels: the descriptor-driven model (cvt32 / binary32 /
    store_typed32) on pool x pool rows past the tile boundaries, as filter and into scratch / narrow dimension slots"""
    be, ran = H.hip_backend(), 0
    with kernel_log(be) as kernels:
        for tb, b_kind in [(t, "col") for t in (abi.Bool, abi.Uint8, abi.Int16, abi.Int32, abi.Uint32, abi.Float32)] + \
                [(t, "scratch") for t in SCRATCH_TYPES]:
            for ft in M.BINARY:
                sinks = [FILTER, natural_sink(M.KIND_OF[ta], M.KIND_OF[tb], ft)]
                sinks.append(Sink("dim", [abi.Int8, abi.Uint8, abi.Int16, abi.Uint16, abi.Bool][(ft + tb) % 5], offset=ft % 5))
                for k, sink in enumerate(sinks):
                    pair = pair_vectors(ta, tb, ft, sink, rows=[None, TILE_ROWS[0], TILE_ROWS[1]][(ft + k) % 3], b_kind=b_kind,
                                        b_mode=1 + (ft + tb) % 2)
                    if pair is None:
                        continue
                    a, b = pair
                    style = "identity" if b_kind == "scratch" or (sink.kind == "filter" and ft % 2) else "subset" if sink.kind == "filter" \
                        else ["identity", "subset", "perm"][ft % 3]
                    EdgeCase(a, b, ft, sink, _style_index(style, len(a.values), seed=ft)).check(be)
                    a.free(), b.free()
                    ran += 1
    assert ran > 300
    assert kernels & GENERIC_TRANSFORMS and kernels & GENERIC_FILTERS, kernels
    assert not kernels & (FAST_TRANSFORMS | FAST_FILTERS), kernels


@pytest.mark.gpu
def test_hip_unary_functors_and_run_length_columns():
    """unary functors over every column type in modes 1, 2 and 3 and over scratch vectors; every sink from a run-length column;
    measures scaled by a compressed base column (store_measure32's value x count)"""
    be, ran = H.hip_backend(), 0
    with kernel_log(be) as kernels:
        for ta in COL_TYPES:
            for kind, mode in [("col", 1), ("col", 2), ("col", 3)] + ([("scratch", 0)] if ta in SCRATCH_TYPES else []):
                for ft in M.UNARY:
                    for sink in (FILTER, natural_sink(M.KIND_OF[ta], None, ft, arity=1)):
                        built = unary_vector(ta, ft, sink, mode=mode, kind=kind)
                        if built is None:
                            continue
                        a, rows = built
                        EdgeCase(a, None, ft, sink, _style_index("identity", rows)).check(be)
                        a.free()
                        ran += 1
            for sink in all_sinks():
                built = unary_vector(ta, M.Noop, sink, mode=3)
                if built is None:
                    continue
                a, rows = built
                EdgeCase(a, None, M.Noop, sink, _style_index("identity", rows)).check(be)
                a.free()
                if sink.kind == "measure":
                    a, rows = unary_vector(ta, M.Noop, sink, mode=2, rows=TILE_ROWS[0])
                    lens = 1 + np.arange(rows) % 4
                    lens[rows // 2] = 3000000000 if sink.dtype in (abi.Uint32, abi.Int64, abi.Float64) else 5
                    EdgeCase(a, None, M.Noop, sink, _style_index("identity", rows),
                             base_counts=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)).check(be)
                    a.free()
                ran += 1
    assert ran > 500
    assert kernels & (GENERIC_TRANSFORMS | FAST_TRANSFORMS) and kernels & (GENERIC_FILTERS | FAST_FILTERS), kernels


_FAST_SINKS = {
    M.K_I32: [Sink("scratch", abi.Int32), Sink("dim", abi.Int32, offset=3), Sink("dim", abi.Int16, offset=1), Sink("dim", abi.Uint8, offset=5),
              Sink("measure", abi.Int64, M.SUM_SIGNED, offset=1), Sink("measure", abi.Int32, M.MIN_SIGNED, offset=2),
              Sink("dim", abi.Uint32, offset=7), Sink("measure", abi.Float64, M.SUM_FLOAT, offset=3)],
    M.K_U32: [Sink("scratch", abi.Uint32), Sink("dim", abi.Uint32, offset=2), Sink("dim", abi.Uint16, offset=3), Sink("dim", abi.Int8, offset=6),
              Sink("measure", abi.Int64, M.SUM_SIGNED, offset=1), Sink("measure", abi.Uint32, M.MAX_UNSIGNED, offset=5),
              Sink("measure", abi.Float32, M.SUM_FLOAT, offset=2)],
    M.K_F32: [Sink("scratch", abi.Float32), Sink("dim", abi.Float32, offset=1), Sink("measure", abi.Float64, M.SUM_FLOAT, offset=3),
              Sink("measure", abi.Float32, M.MIN_FLOAT, offset=2), Sink("dim", abi.Int32, offset=4), Sink("measure", abi.Int64, M.SUM_SIGNED)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ta", INT_TYPES + [abi.Float32], ids=lambda t: M.TYPE_NAMES[t])
def test_hip_fast_kernels_column_against_constants(ta, mode):
    """the vectorised restatement (eval_quad / compare_tile): 4-, 2- and 1-byte columns against constants of every sign and kind
    (a mode-0 Uint32 column keeps the unsigned kind), six comparisons as filters — index vectors uploaded (identity, subset)
    and numbered by the library (row-space count) — and Plus ... Floor into scratch / dimension slots / measures at unaligned offsets"""
    be, ran = H.hip_backend(), 0
    consts = gpu_constants() + [Vec("col", abi.Uint32, mode=0, value=v) for v in (1, 3, 3600, 2 ** 31, 2 ** 32 - 1)]
    with kernel_log(be) as kernels:
        for ci, b in enumerate(consts):
            k = M.common_kind(M.KIND_OF[ta], b.model_kind())
            for ft in M.COMPARISONS:
                rows = TILE_ROWS[(ci + ft) % 2]
                a = column_for_constant(ta, b, ft, FILTER, rows=rows, mode=mode)
                style = ["identity", "subset", "init"][(ci + ft) % 3]
                EdgeCase(a, b, ft, FILTER, _style_index("identity" if style == "init" else style, rows, seed=ci),
                         init_index=style == "init").check(be)
                a.free()
                ran += 1
            for ft in range(M.Plus, M.Floor + 1):
                sink = _FAST_SINKS[k][(ci + ft) % len(_FAST_SINKS[k])]
                rows = TILE_ROWS[(ci + ft) % 2]
                a = column_for_constant(ta, b, ft, sink, rows=rows, mode=mode)
                if a is None:
                    continue
                EdgeCase(a, b, ft, sink, _style_index(["identity", "subset", "perm"][(ci + ft) % 3], rows, seed=ci)).check(be)
                a.free()
                ran += 1
            b.free()
    assert ran > 400
    assert kernels & FAST_TRANSFORMS and kernels >= FAST_FILTERS, kernels
    assert not kernels & (GENERIC_TRANSFORMS | GENERIC_FILTERS), kernels


def _division_dividends(d, signed):
    """k d - 1, k d, k d + 1 for k near 1, 2^16 / d, 2^31 / d and 2^32 / d, both signs on the signed kind"""
    mag = abs(int(d))
    out = []
    for top in (1, 2 ** 16 // mag, 2 ** 31 // mag, 2 ** 32 // mag):
        for k in (top - 1, top, top + 1):
            out += [k * mag - 1, k * mag, k * mag + 1]
    lo, hi = (-2 ** 31, 2 ** 31 - 1) if signed else (0, 2 ** 32 - 1)
    out = [x for x in out + [-x for x in out if signed] if lo <= x <= hi]
    return np.array(sorted(set(out)), np.int64)


SIGNED_DIVISORS = [1, 2, 3, 7, 3600, 86400, 2 ** 31 - 1, -1, -2, -3, -7, -3600, -86400, -2 ** 31 + 1, -2 ** 31]
UNSIGNED_DIVISORS = [1, 2, 3, 7, 3600, 86400, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1]


def _division_cases(signed):
    for d in (SIGNED_DIVISORS if signed else UNSIGNED_DIVISORS):
        b = Vec("cint", value=d) if signed else Vec("col", abi.Uint32, mode=0, value=d)
        for ta in ([abi.Int32, abi.Uint32, abi.Int16, abi.Uint8] if signed else [abi.Uint32, abi.Uint16]):
            extra = _division_dividends(d, signed) if ta in (abi.Int32, abi.Uint32) else None
            if extra is not None and signed and ta == abi.Uint32:   # the same bits: a Uint32 column against an int constant is int32
                extra = extra & M.M32
            for ft in (M.Divide, M.Mod, M.Floor):
                t4 = abi.Int32 if signed else abi.Uint32
                sink = [Sink("scratch", t4), Sink("dim", t4, offset=1 + ft % 3)][ft % 2]
                a = column_for_constant(ta, b, ft, sink, rows=TILE_ROWS[ft % 2], mode=1 + ft % 2, extra=extra)
                yield a, b, EdgeCase(a, b, ft, sink, _style_index("identity", TILE_ROWS[ft % 2]))


@pytest.mark.parametrize("signed", [True, False], ids=["int32", "uint32"])
def test_model_division_sweep(signed):
    """the sweep's dividends and divisors through the C checker (exact C division)"""
    for a, b, case in _division_cases(signed):
        case.check(H.oracle_backend())
        a.free(), b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("signed", [True, False], ids=["int32", "uint32"])
def test_hip_division_sweep_fast_kernel(signed):
    """fast_divmod (one multiply-high by floor(2^32 / d) and one correction) against exact division: every divisor of the pool,
    dividends around every multiple where the estimate can be off by one, magnitudes up to 2^31 / 2^32 - 1"""
    be, ran = H.hip_backend(), 0
    with kernel_log(be) as kernels:
        for a, b, case in _division_cases(signed):
            case.check(be)
            a.free(), b.free()
            ran += 1
    assert ran >= 60
    assert kernels & FAST_TRANSFORMS and not kernels & GENERIC_TRANSFORMS, kernels


# ---- fused routes: whole query plans whose constants, keys and measures are edge values ----------------------------------
def _plan_eval(e, cols, valid, n):
    if isinstance(e, Col):
        t, v = cols[e.name]
        return M.widen(v, t), (np.ones(n, bool) if valid[e.name] is None else valid[e.name]), M.KIND_OF[t]
    if isinstance(e, Const):
        if isinstance(e.value, float):
            return np.full(n, M.f32_bits(np.float32(e.value)), np.uint32), np.ones(n, bool), M.K_F32
        return np.full(n, M.u32(e.value), np.uint32), np.ones(n, bool), M.K_I32
    a, aok, ka = _plan_eval(e.lhs, cols, valid, n)
    b, bok, kb = _plan_eval(e.rhs, cols, valid, n)
    k = M.common_kind(ka, kb)
    r, ok = M.binary(e.op, k, M.convert(a, ka, k), aok, M.convert(b, kb, k), bok)
    return r, ok, M.binary_result_kind(e.op, k)


def model_query(plan, batches):
    """{key in query dimension order: [raw measure elements]} — filter, project and group with the model alone"""
    order = range(len(plan.dimensions))
    groups = {}
    for cols, valid in batches:
        n = len(next(iter(cols.values()))[1])
        keep = np.ones(n, bool)
        for f in plan.filters:
            r, ok, rk = _plan_eval(f, cols, valid, n)
            keep &= M.convert(r, rk, M.K_BOOL) != 0
        dims = []
        for d in plan.dimensions:
            r, ok, rk = _plan_eval(d.expr, cols, valid, n)
            dims.append((M.store_typed(d.data_type, r, rk), ok))
        r, ok, rk = _plan_eval(plan.measure, cols, valid, n)
        meas = M.store_measure(plan.measure_type, plan.agg, r, ok, rk)
        for i in np.flatnonzero(keep):
            key = tuple((bytes(dims[j][0][i]), int(dims[j][1][i])) for j in order)
            groups.setdefault(key, []).append(meas[i])
    return groups


def compare_with_model(plan, got, groups, what):
    assert got.keys() == groups.keys(), f"{what}: group keys differ: {len(got)} vs {len(groups)}; " \
        f"only there {sorted(set(got) - set(groups))[:3]}, only in the model {sorted(set(groups) - set(got))[:3]}"
    w = plan.measure_bytes
    for key, vals in groups.items():
        want = M.aggregate(plan.agg, w, np.stack(vals))
        g = got[key]
        if plan.agg == M.SUM_FLOAT:
            total, mags, n = want
            assert abs(np.longdouble(g) - total) <= n * 2.0 ** (-53 if w == 8 else -24) * mags, (what, key, g, total)
        elif plan.agg in (M.MIN_FLOAT, M.MAX_FLOAT):
            assert float(g) == want, (what, key, g, want)
        else:
            assert int(g) % (1 << (8 * w)) == want % (1 << (8 * w)), (what, key, int(g), want, len(vals))


def edge_batches(sizes, narrow=(abi.Uint8, abi.Int16)):
    """columns whose rows walk the product of the Uint32 and Int32 pools; s8 / s16 narrow columns at full range; f finite floats"""
    pu, pi = _np_pool(abi.Uint32), _np_pool(abi.Int32)
    p8, p16 = _np_pool(narrow[0]), _np_pool(narrow[1])
    # (a sum that meets +inf and -inf, or overflows, is a NaN whose bits are open: UNDEFINED["nan_result_bits"])
    pf = np.array([x for x in M.EDGE_POOLS[abi.Float32] if np.isfinite(x) and abs(x) < 1e30], np.float32)
    out, at = [], 0
    for n in sizes:
        r = at + np.arange(n)
        cols = {"u": (abi.Uint32, pu[r % len(pu)]), "i": (abi.Int32, pi[(r // len(pu)) % len(pi)]), "s8": (narrow[0], p8[(r // 5) % len(p8)]),
                "s16": (narrow[1], p16[(r // 3) % len(p16)]), "f": (abi.Float32, pf[(r // 2) % len(pf)])}
        valid = {k: None if k == "s8" else (r + j) % (11 + j) != 0 for j, k in enumerate(cols)}
        out.append((cols, valid))
        at += n
    return out


def fused_plan(variant, use_hash=True):
    c = lambda v: Const(int(v))  # noqa: E731
    if variant == 0:   # a Uint32 column against integer constants compares as int32: 3000000000 < 5; 4-byte sums wrap
        return QueryPlan(filters=[Binary(abi.LessThan, Col("u"), c(86401)), Binary(abi.NotEqual, Col("i"), c(-1))],
                         dimensions=[DimensionSpec(Binary(abi.Floor, Col("u"), c(3600)), abi.Uint32), DimensionSpec(Col("i"), abi.Int32)],
                         measure=Col("u"), agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32, use_hash_reduction=use_hash)
    if variant == 1:   # negative divisor, keys 0xFFFFFFFF / 0x80000000, 8-byte signed sum of negative Int32 (sign extension)
        return QueryPlan(filters=[Binary(abi.GreaterThanOrEqual, Col("i"), c(-2 ** 31 + 1))],
                         dimensions=[DimensionSpec(Binary(abi.Divide, Col("i"), c(-7)), abi.Int32), DimensionSpec(Col("u"), abi.Uint32)],
                         measure=Col("i"), agg=abi.AGGR_SUM_SIGNED, measure_type=abi.Int64, use_hash_reduction=use_hash)
    if variant == 2:   # 8-byte signed sum of Uint32 >= 2^31 (zero extension), group totals past 2^33
        return QueryPlan(filters=[Binary(abi.GreaterThan, Col("u"), c(-2 ** 31))],
                         dimensions=[DimensionSpec(Binary(abi.Mod, Col("i"), c(86400)), abi.Int32)],
                         measure=Col("u"), agg=abi.AGGR_SUM_SIGNED, measure_type=abi.Int64, use_hash_reduction=use_hash)
    if variant == 3:   # narrow columns at full range in their own slots, a 32-bit result truncated into a 2-byte slot
        return QueryPlan(filters=[Binary(abi.GreaterThanOrEqual, Col("s8"), c(1)), Binary(abi.LessThan, Col("u"), c(2 ** 31 - 1))],
                         dimensions=[DimensionSpec(Col("s16"), abi.Int16), DimensionSpec(Col("s8"), abi.Uint8),
                                     DimensionSpec(Binary(abi.Plus, Col("u"), c(1)), abi.Uint16)],
                         measure=Col("f"), agg=abi.AGGR_SUM_FLOAT, measure_type=abi.Float64, use_hash_reduction=use_hash)
    return QueryPlan(filters=[Binary(abi.NotEqual, Col("s16"), c(-32768))],   # variant 4: unsigned maximum above 2^31
                     dimensions=[DimensionSpec(Binary(abi.Floor, Col("s16"), c(256)), abi.Int16), DimensionSpec(Col("s8"), abi.Uint8)],
                     measure=Col("u"), agg=abi.AGGR_MAX_UNSIGNED, measure_type=abi.Uint32, use_hash_reduction=use_hash)


def _rtc_on():
    return all(os.environ.get(k, "1") != "0" for k in ("ARES_FUSE", "ARES_DEFER", "ARES_RTC"))


def _run_fused(be, plan, data, what, native=False):
    run = smoke.run_query_native if native else smoke.run_query
    if be.name != "hip":
        got, _ = smoke.run_query(be, plan, data)
        compare_with_model(plan, got, model_query(plan, data), what)
        return set()
    run(be, plan, data)   # (builds the shape's kernels and learns its cardinality, as a query's first batches do)
    with kernel_log(be) as kernels:
        got, _ = run(be, plan, data)
    compare_with_model(plan, got, model_query(plan, data), what)
    return kernels


@pytest.mark.parametrize("use_hash", [False, True], ids=["sort_reduce", "hash_reduce"])
@pytest.mark.parametrize("variant", range(5))
def test_model_plans_on_the_checker(variant, use_hash):
    """the plans of the fused tests on the C checker: the model's group-by is the checker's (MIN / MAX plans through Sort +
    Reduce only: the host-style HashReduce starts them from 0, see edge_model.UNDEFINED)"""
    if use_hash and variant == 4:
        pytest.skip(M.UNDEFINED["host_hash_reduce_min_max"])
    _run_fused(H.oracle_backend(), fused_plan(variant, use_hash), edge_batches((3000, 1, 2500)), f"plan {variant}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", range(5))
def test_hip_fused_plan_hash_reduce(variant):
    """filter constants, dimension expressions and measures from the pools through HashReduce consuming the pending transforms:
    the generated scan (hr_table_scan_rtc / hr_scan_rtc) by default, the generated DIRECT-mode scan and merge (hr_scan_rtc +
    hr_merge_rtc) with ARES_LEAN_MIN_GROUPS=0, the precompiled hr_fused_scan_kernel with ARES_RTC=0
    (test_hip_fused_plans_with_the_switches_that_are_read_once runs this test again in such processes)"""
    data = edge_batches((6000, 1, 9000, 300))
    kernels = _run_fused(H.hip_backend(), fused_plan(variant), data, f"fused plan {variant}", native=bool(variant % 2))
    if _rtc_on():   # generated scan; the merge is the generated one for narrow layouts and in DIRECT mode, else the precompiled one
        assert kernels & {"hr_scan_rtc", "hr_table_scan_rtc"} and kernels & {"hr_merge_rtc", "hr_fused_merge_kernel"}, kernels
        if os.environ.get("ARES_LEAN_MIN_GROUPS") == "0":
            assert "hr_scan_rtc" in kernels and "hr_merge_rtc" in kernels, kernels
    elif variant < 3:   # (plans with 1- / 2-byte slots are fused by generated kernels only)
        assert "hr_fused_scan_kernel" in kernels, kernels
    if _rtc_on() or variant < 3:
        assert not kernels & (FAST_TRANSFORMS | GENERIC_TRANSFORMS), kernels


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 4])
def test_hip_fused_plan_sort_reduce(variant):
    """the same plans through Sort + Reduce: the hash-keyed route's generated scans (sr_scan_rtc / sr_vector_scan_rtc)"""
    data = edge_batches((5000, 7000, 2))
    kernels = _run_fused(H.hip_backend(), fused_plan(variant, use_hash=False), data, f"sort plan {variant}")
    if _rtc_on():
        assert any(k.startswith("sr_") for k in kernels), kernels


def _division_plan(d):
    divs = _division_dividends(d, True)
    pool = np.concatenate([_np_pool(abi.Int32).astype(np.int64), divs])
    data = []
    for n, shift in ((6000, 0), (4099, 17), (3, 1)):
        v = pool[(shift + np.arange(n)) % len(pool)].astype(np.int32)
        data.append(({"i": (abi.Int32, v), "u": (abi.Uint32, v.view(np.uint32))}, {"i": (shift + np.arange(n)) % 13 != 0, "u": None}))
    plan = QueryPlan(filters=[Binary(abi.NotEqual, Col("u"), Const(12345))],
                     dimensions=[DimensionSpec(Binary(abi.Divide, Col("i"), Const(d)), abi.Int32),
                                 DimensionSpec(Binary(abi.Mod, Col("u"), Const(d)), abi.Int32),
                                 DimensionSpec(Binary(abi.Floor, Col("i"), Const(d)), abi.Int32)],
                     measure=Col("u"), agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32, use_hash_reduction=True)
    return plan, data


_PLAN_DIVISORS = [3, 3600, 86400, 2 ** 31 - 1, -7]


@pytest.mark.parametrize("d", _PLAN_DIVISORS)
def test_model_division_plan_on_the_checker(d):
    plan, data = _division_plan(d)
    _run_fused(H.oracle_backend(), plan, data, f"division by {d}")


@pytest.mark.gpu
@pytest.mark.parametrize("d", _PLAN_DIVISORS)
def test_hip_division_sweep_fused_plan(d):
    """the generated kernels hand a LITERAL divisor to the compiler: Divide / Mod / Floor by d as the dimensions of one fused plan,
    on the dividends of the sweep"""
    plan, data = _division_plan(d)
    kernels = _run_fused(H.hip_backend(), plan, data, f"division by {d}")
    if _rtc_on():
        assert kernels & {"hr_scan_rtc", "hr_table_scan_rtc"}, kernels
    else:
        assert "hr_fused_scan_kernel" in kernels, kernels


@pytest.mark.gpu
def test_hip_fused_plans_with_the_switches_that_are_read_once():
    """ARES_RTC and ARES_LEAN_MIN_GROUPS are read once per process: the fused plans again in a child process with ARES_RTC=0
    (the precompiled hr_fused_scan_kernel), then in one with ARES_LEAN_MIN_GROUPS=0 (every batch through the generated DIRECT-mode
    scan and the generated merge; ARES_MIN_PART_BITS=2 gives these small batches the partitions that merge needs).  One child at a
    time; the first that does not return 0 ends the test, nothing is started after it."""
    for env in ({"ARES_RTC": "0"}, {"ARES_LEAN_MIN_GROUPS": "0", "ARES_MIN_PART_BITS": "2"}):
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "tests/test_edge_semantics.py", "-k",
                            "test_hip_fused_plan_hash_reduce or test_hip_division_sweep_fused_plan"], cwd=H.ROOT,
                           env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            pytest.fail(f"{env}: exit status {r.returncode}\n{r.stdout[-2500:]}\n{r.stderr[-500:]}")


# ---- aggregates --------------------------------------------------------------------------------------------------------
_EDGE_KEYS = np.array([0xFFFFFFFF, 0x80000000, 0, 1, 0x7FFFFFFF, 65536, 0x80000001], np.uint32)
_GROUP_SIZES = [1, 2, 63, 64, 65, 5000, 3]


def reduce_batches(be, how, batches, agg, vb):
    """HashReduce or Sort + Reduce over consecutive batches of (uint32 keys, raw measure elements), the previous result in front
    of every batch like the Go host lays it out; returns (keys, raw aggregates)"""
    cap = sum(len(k) for k, _ in batches) + 8
    sort = how == "sort"
    d = [H.DimVector(be, cap, (0, 0, 1, 0, 0), with_hash=sort, with_index=sort) for _ in range(2)]
    m = [H.Buf(be, nbytes=vb * cap + 8) for _ in range(2)]
    size = 0
    for keys, vals in batches:
        n = len(keys)
        d[0].values.write(np.ascontiguousarray(keys, np.uint32).view(np.uint8), offset=4 * size)
        d[0].values.write(np.ones(n, np.uint8), offset=4 * cap + size)
        m[0].write(np.ascontiguousarray(vals).view(np.uint8).reshape(-1), offset=vb * size)
        length = size + n
        if sort:
            be.call("InitIndexVector", d[0].index.ptr, 0, length, None, 0)
            be.call("Sort", d[0].struct(), length, None, 0)
            size = be.call("Reduce", d[0].struct(), m[0].ptr, d[1].struct(), m[1].ptr, vb, length, agg, None, 0)
        else:
            size = be.call("HashReduce", d[0].struct(), m[0].ptr, d[1].struct(), m[1].ptr, vb, length, agg, None, 0)
        d.reverse(), m.reverse()
    keys = d[0].values.read(np.uint32, size)
    vals = m[0].read(np.uint8, vb * size).reshape(size, vb)
    valid = d[0].values.read(np.uint8, size, offset=4 * cap)
    for x in d + m:
        x.free()
    assert valid.all() and len(np.unique(keys)) == size, "a group appears twice or lost its validity"
    return keys, vals


def _aggregate_values(agg, vb, n):
    """n raw measure elements at the edges of the aggregate's type"""
    r = np.arange(n)
    if agg in (M.MIN_FLOAT, M.MAX_FLOAT):
        pool = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, M.FLT_MAX, -M.FLT_MAX, 1e-45, -1e-45, 0.1], np.float32)
        return pool[(r * 7) % len(pool)]
    if agg in (M.MIN_UNSIGNED, M.MAX_UNSIGNED, M.SUM_UNSIGNED):
        pool = _np_pool(abi.Uint32)
        if agg == M.SUM_UNSIGNED:
            pool = pool[pool >= 2 ** 24]   # a 4-byte sum wraps every few rows
        v = pool[(r * 5) % len(pool)]
        return v.astype(np.uint64) if vb == 8 else v
    pool = _np_pool(abi.Int32)
    if vb == 8:   # what the scans hand to the merge: Uint32 values zero-extended, Int32 values sign-extended
        wide = np.concatenate([pool.astype(np.int64), _np_pool(abi.Uint32).astype(np.int64)])
        return wide[(r * 5) % len(wide)]
    return pool[(r * 5) % len(pool)]


def _check_groups(agg, vb, keys, vals, truth, what):
    assert sorted(keys.tolist()) == sorted(truth), (what, len(keys), len(truth))
    for k, row in zip(keys.tolist(), vals):
        want = M.aggregate(agg, vb, np.stack(truth[k]))
        if agg in (M.MIN_FLOAT, M.MAX_FLOAT):
            got = float(row.view(np.float32)[0])
            assert got == want, (what, hex(k), got, want)   # (as numbers: see UNDEFINED["min_max_of_both_zeros"])
        else:
            got = int(row.view(np.uint64 if vb == 8 else np.uint32)[0])
            assert got == want % (1 << (8 * vb)), (what, hex(k), got, want % (1 << (8 * vb)), len(truth[k]))


_AGG_EDGES = [(M.MIN_UNSIGNED, 4), (M.MAX_UNSIGNED, 4), (M.MIN_SIGNED, 4), (M.MAX_SIGNED, 4), (M.MIN_FLOAT, 4), (M.MAX_FLOAT, 4),
              (M.SUM_UNSIGNED, 4), (M.SUM_SIGNED, 4), (M.SUM_UNSIGNED, 8), (M.SUM_SIGNED, 8)]
_AGG_IDS = [f"agg{a}x{b}" for a, b in _AGG_EDGES]


def _aggregate_edge_batches(agg, vb, one_group):
    group = np.concatenate([np.full(s, g) for g, s in enumerate(_GROUP_SIZES)])
    if one_group:
        group[:] = 0
    n = len(group)
    vals = _aggregate_values(agg, vb, n)
    order = np.random.default_rng(11).permutation(n)
    keys, vals = _EDGE_KEYS[group[order]], vals[order]
    cuts = [0, n // 3, n // 3 + 1, 2 * n // 3, n]   # four batches, one of a single row: the previous result is merged three times
    truth = {}
    raw = np.ascontiguousarray(vals).view(np.uint8).reshape(n, vb)
    for k, v in zip(keys.tolist(), raw):
        truth.setdefault(k, []).append(v)
    return [(keys[a:b], vals[a:b]) for a, b in zip(cuts[:-1], cuts[1:])], truth


@pytest.mark.gpu
@pytest.mark.parametrize("one_group", [False, True], ids=["sizes_1_2_63_64_65", "one_group"])
@pytest.mark.parametrize("agg,vb", _AGG_EDGES, ids=_AGG_IDS)
def test_hip_hash_reduce_aggregate_edges(agg, vb, one_group, hash_path):
    """MIN / MAX by signedness at and beyond 2^31, 4-byte sums that wrap, 8-byte sums that carry out of the low word, over four
    batches — through the LDS tables and the global table — against the model (groups start from the identity)"""
    batches, truth = _aggregate_edge_batches(agg, vb, one_group)
    keys, vals = reduce_batches(H.hip_backend(), "hash", batches, agg, vb)
    _check_groups(agg, vb, keys, vals, truth, f"HashReduce {hash_path} agg {agg} x {vb}")


@pytest.mark.gpu
@pytest.mark.parametrize("one_group", [False, True], ids=["sizes_1_2_63_64_65", "one_group"])
@pytest.mark.parametrize("agg,vb", _AGG_EDGES, ids=_AGG_IDS)
def test_hip_sort_reduce_aggregate_edges(agg, vb, one_group):
    be = H.hip_backend()
    batches, truth = _aggregate_edge_batches(agg, vb, one_group)
    with kernel_log(be) as kernels:
        keys, vals = reduce_batches(be, "sort", batches, agg, vb)
    _check_groups(agg, vb, keys, vals, truth, f"Sort + Reduce agg {agg} x {vb}")
    assert any(k.startswith(("reduce_", "sr_")) for k in kernels), kernels


@pytest.mark.parametrize("agg,vb", _AGG_EDGES, ids=_AGG_IDS)
def test_model_sort_reduce_aggregate_edges(agg, vb):
    """the same batches through the C checker's Sort + Reduce: the model's aggregates are the checker's"""
    batches, truth = _aggregate_edge_batches(agg, vb, False)
    keys, vals = reduce_batches(H.oracle_backend(), "sort", batches, agg, vb)
    _check_groups(agg, vb, keys, vals, truth, f"checker Sort + Reduce agg {agg} x {vb}")


# ---- float sums whose order matters ----------------------------------------------------------------------------------------
def _hard_floats(rng, n):
    """full-mantissa float32 values over seven decades of magnitude, mixed sign"""
    return ((1.0 + rng.random(n)) * 10.0 ** rng.uniform(-3, 4, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _group_sums(group, x, weights=None):
    """per group (ascending id): sum of x (x weights) in longdouble, sum of magnitudes, row count"""
    order = np.argsort(group, kind="stable")
    g = group[order]
    starts = np.concatenate([[0], np.flatnonzero(g[1:] != g[:-1]) + 1])
    v = x[order].astype(np.longdouble) * (1 if weights is None else weights[order].astype(np.longdouble))
    return g[starts], np.add.reduceat(v, starts), np.add.reduceat(np.abs(v), starts), np.diff(np.concatenate([starts, [len(g)]]))


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [7, 50000, 1000000])
def test_hip_float64_sums_hold_the_any_order_bound(groups, hash_path):
    """4 Mi full-mantissa floats into 8-byte accumulators: whatever order the kernels add in, the forward error of n_g float64
    additions is at most n_g 2^-53 sum|x| — far inside the documented 1e-6, and independent of cancellation"""
    be = H.hip_backend()
    rng = np.random.default_rng(groups)
    n = 1 << 22
    group = rng.integers(0, groups, n).astype(np.uint32)
    x = _hard_floats(rng, n)
    cut = n // 2 + 12345
    keys, vals = reduce_batches(be, "hash", [(group[:cut], x[:cut].astype(np.float64)), (group[cut:], x[cut:].astype(np.float64))],
                                M.SUM_FLOAT, 8)
    got = vals.view(np.float64).reshape(-1)[np.argsort(keys)]
    ids, total, mags, counts = _group_sums(group, x)
    assert np.array_equal(np.sort(keys), ids)
    err = np.abs(got.astype(np.longdouble) - total)
    bound = counts * np.longdouble(2.0 ** -53) * mags
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), (int(ids[worst]), got[worst], total[worst], float(err[worst]), float(bound[worst]))
    big = np.abs(total) >= 1e-3 * mags
    assert np.all(err[big] <= 1e-6 * np.abs(total[big]))


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [7, 50000])
def test_hip_float64_sums_fused_route_hold_the_any_order_bound(groups):
    be = H.hip_backend()
    rng = np.random.default_rng(100 + groups)
    n = 1 << 21
    data, gs, xs = [], [], []
    for _ in range(2):
        g, x = rng.integers(0, groups, n).astype(np.uint32), _hard_floats(rng, n)
        data.append(({"g": (abi.Uint32, g), "f": (abi.Float32, x)}, {"g": None, "f": None}))
        gs.append(g), xs.append(x)
    plan = QueryPlan(filters=[Binary(abi.GreaterThanOrEqual, Col("g"), Const(0))], dimensions=[DimensionSpec(Col("g"), abi.Uint32)],
                     measure=Col("f"), agg=abi.AGGR_SUM_FLOAT, measure_type=abi.Float64, use_hash_reduction=True)
    smoke.run_query(be, plan, data)
    with kernel_log(be) as kernels:
        got, _ = smoke.run_query(be, plan, data)
    ids, total, mags, counts = _group_sums(np.concatenate(gs), np.concatenate(xs))
    assert len(got) == len(ids)
    for k, t, m, c in zip(ids.tolist(), total, mags, counts):
        g = got[((np.uint32(k).tobytes(), 1),)]
        assert abs(np.longdouble(g) - t) <= c * np.longdouble(2.0 ** -53) * m, (k, g, t)
    if _rtc_on():
        assert kernels & {"hr_scan_rtc", "hr_table_scan_rtc"}, kernels


@pytest.mark.gpu
@pytest.mark.parametrize("agg", [M.SUM_FLOAT, M.AVG_FLOAT], ids=["sum_float32", "avg"])
def test_hip_float32_accumulators_hold_1e4_of_the_magnitudes(agg, hash_path):
    """4-byte float accumulators and the rolling average at 100 000 rows: the documented 1e-4, stated relative to sum|x| (a
    float32 sum carries n 2^-24 sum|x| in the worst order); AVG counts are exact"""
    be = H.hip_backend()
    rng = np.random.default_rng(agg)
    n, groups = 100000, 37
    group = rng.integers(0, groups, n).astype(np.uint32)
    x = _hard_floats(rng, n)
    if agg == M.AVG_FLOAT:
        w = rng.integers(1, 4, n).astype(np.uint32)
        raw = np.stack([x.view(np.uint32), w], 1).reshape(-1).view(np.uint64)
        keys, vals = reduce_batches(be, "hash", [(group[:40000], raw[:40000]), (group[40000:], raw[40000:])], agg, 8)
        pair = vals.view(np.uint32).reshape(-1, 2)[np.argsort(keys)]
        ids, total, mags, _ = _group_sums(group, x, w)
        wsum = _group_sums(group, w.astype(np.float32))[1]
        assert np.array_equal(pair[:, 1].astype(np.int64), wsum.astype(np.int64))
        got = M.as_f32(pair[:, 0].copy()).astype(np.longdouble)
        assert np.all(np.abs(got - total / wsum) <= 1e-4 * mags / wsum)
    else:
        keys, vals = reduce_batches(be, "hash", [(group[:40000], x[:40000]), (group[40000:], x[40000:])], agg, 4)
        got = vals.view(np.float32).reshape(-1)[np.argsort(keys)].astype(np.longdouble)
        ids, total, mags, _ = _group_sums(group, x)
        assert np.all(np.abs(got - total) <= 1e-4 * mags)
    assert np.array_equal(np.sort(keys), ids)
