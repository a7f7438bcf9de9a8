"""A non-aggregation batch (SELECT cols WHERE ... LIMIT n) three ways: an independent numpy model, the per-node ABI
sequence (InitIndexVector, a filter call per comparison, a transform call per dimension into a dimension vector) and the
fused extension AresFusedFilterSelect.  The model evaluates filters and expressions per row, takes the surviving rows in
order and cuts at the limit; tests/test_nonaggr_model.py pins it to the per-node sequence on the oracle.

A column is a `Col`; a filter is (column name, comparison functor, constant); a dimension is
(column name, binary functor or None for a bare column, constant, output DataType), dimensions in vector order (slot widths
descending).  Constants are Python ints (ConstInt) or floats (ConstFloat)."""
import numpy as np

import harness as H
from aresdb_amd import abi

_NP = {abi.Int8: np.int8, abi.Uint8: np.uint8, abi.Int16: np.int16, abi.Uint16: np.uint16, abi.Int32: np.int32,
       abi.Uint32: np.uint32, abi.Float32: np.float32, abi.Int64: np.int64}
_KIND = {abi.Int8: "i", abi.Int16: "i", abi.Int32: "i", abi.Uint8: "u", abi.Uint16: "u", abi.Uint32: "u", abi.Float32: "f"}
WIDE = (abi.Int64, abi.GeoPoint, abi.UUID)
SENTINEL = 0xA5


class Col:
    """values: numpy array of the column's own type, or (rows, width) uint8 for GeoPoint / UUID; valid: bools or None
    (mode 1); mode 0: values None with a default; counts: run-length counts (mode 3)."""

    def __init__(self, dtype, values=None, valid=None, starting_index=0, default=None, counts=None):
        self.dtype, self.valid, self.starting_index, self.default, self.counts = dtype, valid, starting_index, default, counts
        if values is not None and dtype in (abi.GeoPoint, abi.UUID):
            values = np.ascontiguousarray(values, np.uint8).reshape(-1, abi.DATA_TYPE_BYTES[dtype])
        elif values is not None and dtype != abi.Bool:
            values = np.asarray(values).astype(_NP[dtype])
        self.values = values

    def upload(self, be):
        if self.values is None:
            return H.Column(be, self.dtype, default=self.default)
        if self.dtype in (abi.GeoPoint, abi.UUID):
            return H.Column(be, self.dtype, raw_values=self.values.tobytes(), valid=self.valid, starting_index=self.starting_index)
        return H.Column(be, self.dtype, values=self.values, valid=self.valid, counts=self.counts,
                        starting_index=self.starting_index)


# ---- the model --------------------------------------------------------------------------------------------------------
def _bits(col, n):
    """the column's stored values widened to 32 bits (sign- or zero-extended), as uint32"""
    v = col.values[:n]
    if _KIND[col.dtype] == "f":
        return v.view(np.uint32).copy()
    return v.astype(np.int64).astype(np.uint32) if _KIND[col.dtype] == "i" else v.astype(np.uint32)


def _valid(col, n):
    return np.ones(n, bool) if col.valid is None else np.asarray(col.valid[:n], bool)


def _convert(bits, frm, to):
    """bits of kind `frm` as kind `to` (C++ conversions: int -> float rounds to nearest, float -> int truncates)"""
    if frm == to or (frm != "f" and to != "f"):
        return bits
    if to == "f":
        src = bits.view(np.int32) if frm == "i" else bits
        return src.astype(np.float32).view(np.uint32)
    f = bits.view(np.float32)
    return np.trunc(f).astype(np.int64).astype(np.uint32)


def _const(c, kind):
    """the constant as kind `kind`: (bits as a one-element uint32 array)"""
    if isinstance(c, float):
        return _convert(np.array([c], np.float32).view(np.uint32), "f", kind)
    return _convert(np.array([c], np.int64).astype(np.uint32), "i", kind)


def _common(kind, c):
    return "f" if kind == "f" or isinstance(c, float) else "i"  # (an integer constant is an Int32: never "u")


def _typed(bits, kind):
    return bits.view(np.float32) if kind == "f" else bits.view(np.int32) if kind == "i" else bits


def model_filter(col, functor, c, n):
    kind = _KIND[col.dtype]
    common = _common(kind, c)
    x, y = _typed(_convert(_bits(col, n), kind, common), common), _typed(_const(c, common), common)[0]
    keep = {abi.Equal: x == y, abi.NotEqual: x != y, abi.LessThan: x < y, abi.LessThanOrEqual: x <= y,
            abi.GreaterThan: x > y, abi.GreaterThanOrEqual: x >= y}[functor]
    return keep & _valid(col, n)


def model_dim(col, functor, c, out_type, n):
    """(value bytes (n, width) uint8, validity bytes) of every row of the batch"""
    width = abi.DATA_TYPE_BYTES[out_type]
    ok = _valid(col, n)
    if col.dtype in WIDE:
        assert functor is None and out_type == col.dtype
        v = col.values[:n]
        raw = v.view(np.uint8).reshape(n, 8) if col.dtype == abi.Int64 else v.reshape(n, width)
        return raw.copy(), ok.astype(np.uint8)
    kind = _KIND[col.dtype]
    bits = _bits(col, n)
    if functor is None:
        rk = kind  # a null row keeps its stored bits
    else:
        rk = _common(kind, c)
        x, y = _typed(_convert(bits, kind, rk), rk), _typed(_const(c, rk), rk)[0]
        with np.errstate(all="ignore"):
            if rk == "f":
                r = {abi.Plus: x + y, abi.Minus: x - y, abi.Multiply: x * y, abi.Divide: x / y}[functor].astype(np.float32)
            else:
                x64, y64 = x.astype(np.int64), int(y)
                trunc_q = np.sign(x64) * np.sign(y64) * (np.abs(x64) // abs(y64)) if y64 else np.zeros_like(x64)
                rem = x64 - trunc_q * y64 if y64 else np.zeros_like(x64)
                r = {abi.Plus: x64 + y64, abi.Minus: x64 - y64, abi.Multiply: x64 * y64, abi.Divide: trunc_q, abi.Mod: rem,
                     abi.Floor: x64 - rem, abi.BitwiseAnd: x64 & y64}[functor]
                r = (r & 0xFFFFFFFF).astype(np.uint32)
        bits = np.where(ok, r.view(np.uint32), np.uint32(0))  # a null operand of a binary functor: bits 0
    if width == 4:
        out = _convert(bits, rk, _KIND[out_type])
        return out.view(np.uint8).reshape(n, 4).copy(), ok.astype(np.uint8)
    assert rk != "f"
    out = bits.astype(np.uint16 if width == 2 else np.uint8)  # truncated
    return out.view(np.uint8).reshape(n, width).copy(), ok.astype(np.uint8)


def model_select(cols, filters, dims, n, limit=-1):
    """(survivor rows cut at the limit, [(value bytes (res, width), validity bytes (res,)) per dimension])"""
    keep = np.ones(n, bool)
    for name, functor, c in filters:
        keep &= model_filter(cols[name], functor, c, n)
    rows = np.flatnonzero(keep)
    if limit >= 0:
        rows = rows[:limit]
    out = []
    for name, functor, c, out_type in dims:
        v, ok = model_dim(cols[name], functor, c, out_type, n)
        out.append((v[rows], ok[rows]))
    return rows, out


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def ndw_of(dims):
    widths = [abi.DATA_TYPE_BYTES[d[3]] for d in dims]
    assert widths == sorted(widths, reverse=True), "dimensions are given in vector order"
    return tuple(widths.count(w) for w in H.DIM_WIDTHS)


def _const_input(c):
    return H.const_float(c) if isinstance(c, float) else H.const_int(c)


def read_dim_rows(be, vec, rows):
    """[(value bytes (rows, width), validity bytes (rows,))] of the first `rows` rows of a DimVector"""
    blob = vec.values.read(np.uint8)
    return [(blob[vo:vo + rows * w].reshape(rows, w).copy(), blob[no:no + rows].copy()) for vo, no, w in vec.dim_offsets()]


def per_node(be, dcols, filters, dims, n, capacity=None, sentinel=False):
    """The per-node sequence on `be` over uploaded columns `dcols` (name -> harness.Column); (count, DimVector)."""
    capacity = max(n, 1) if capacity is None else capacity
    row_bytes = sum(abi.DATA_TYPE_BYTES[d[3]] for d in dims) + len(dims)
    vec = H.DimVector(be, capacity, ndw_of(dims), with_hash=False, with_index=False,
                      init=np.full(row_bytes * capacity, SENTINEL, np.uint8) if sentinel else None)
    idx, pred = H.Buf(be, nbytes=4 * max(n, 1)), H.Buf(be, nbytes=max(n, 1))
    count = n
    be.call("InitIndexVector", idx.ptr, 0, n, None, 0)
    for name, functor, c in filters:
        count = be.call("BinaryFilter", dcols[name].input(), _const_input(c), idx.ptr, pred.ptr, count, None, 0, None, 0,
                        functor, None, 0)
    for (name, functor, c, out_type), (vo, no, _) in zip(dims, vec.dim_offsets()):
        out = H.dimension_output(vec.values.ptr + vo, vec.values.ptr + no, out_type)
        if functor is None:
            be.call("UnaryTransform", dcols[name].input(), out, idx.ptr, count, None, 0, abi.Noop, None, 0)
        else:
            be.call("BinaryTransform", dcols[name].input(), _const_input(c), out, idx.ptr, count, None, 0, functor, None, 0)
    be.wait()
    idx.free()
    pred.free()
    return count, vec


def fused_query(dcols, filters, dims):
    q = abi.FusedSelect()
    q.numFilters, q.numDims = len(filters), len(dims)
    for k, (name, functor, c) in enumerate(filters[:4]):
        q.filters[k].lhs, q.filters[k].rhs = dcols[name].input(), _const_input(c)
        q.filters[k].arity, q.filters[k].functor, q.filters[k].outType = 2, functor, abi.Bool
    for d, (name, functor, c, out_type) in enumerate(dims[:8]):
        q.dims[d].lhs = dcols[name].input()
        q.dims[d].arity, q.dims[d].functor, q.dims[d].outType = (1, abi.Noop, out_type) if functor is None else (2, functor, out_type)
        if functor is not None:
            q.dims[d].rhs = _const_input(c)
    return q


def fused(be, dcols, filters, dims, n, limit, capacity, stream=None):
    """AresFusedFilterSelect into a sentinel-filled vector; (res, DimVector)."""
    row_bytes = sum(abi.DATA_TYPE_BYTES[d[3]] for d in dims[:8]) + len(dims[:8])
    vec = H.DimVector(be, capacity, ndw_of(dims[:8]), with_hash=False, with_index=False,
                      init=np.full(row_bytes * capacity, SENTINEL, np.uint8))
    try:
        res = be.fused_filter_select(fused_query(dcols, filters, dims), n, limit, vec.struct(), stream)
    except Exception:
        vec.free()
        raise
    return res, vec


# ---- a batch with every slot width ------------------------------------------------------------------------------------
def mixed_columns(n, seed=7, valid_share=0.9):
    """Columns of every width the select scan takes, nulls in each but one, validity bit offsets that are no multiple of 8."""
    rng = np.random.default_rng(seed)

    def some():
        return rng.random(n) < valid_share

    return {
        "ts": Col(abi.Uint32, rng.integers(1000, 2000, n), some(), starting_index=3),
        "city": Col(abi.Uint16, rng.integers(0, 500, n), some(), starting_index=1),
        "status": Col(abi.Uint8, rng.integers(0, 4, n), some(), starting_index=7),
        "delta": Col(abi.Int16, rng.integers(-300, 300, n), some(), starting_index=2),
        "fare": Col(abi.Float32, (rng.random(n) * 100).astype(np.float32), some(), starting_index=5),
        "amount": Col(abi.Int32, rng.integers(-10 ** 6, 10 ** 6, n)),
        "big": Col(abi.Int64, rng.integers(-2 ** 60, 2 ** 60, n), some(), starting_index=5),
        "point": Col(abi.GeoPoint, rng.integers(0, 256, (n, 8), dtype=np.uint8), some(), starting_index=6),
        "key": Col(abi.UUID, rng.integers(0, 256, (n, 16), dtype=np.uint8), some(), starting_index=1),
    }


MIXED_FILTERS = [("ts", abi.GreaterThanOrEqual, 1200), ("ts", abi.LessThan, 1900), ("status", abi.NotEqual, 2)]
# slot widths 16 / 8 / 8 / 4 / 4 / 2 / 2 / 1; "ts" and "status" are read by a filter and a dimension at once
MIXED_DIMS = [("key", None, None, abi.UUID), ("big", None, None, abi.Int64), ("point", None, None, abi.GeoPoint),
              ("ts", abi.Floor, 60, abi.Uint32), ("fare", None, None, abi.Float32), ("city", None, None, abi.Uint16),
              ("delta", abi.Plus, 1000, abi.Int16), ("status", None, None, abi.Uint8)]


def assert_rows_equal(got, want, what=""):
    assert len(got) == len(want)
    for d, ((gv, gn), (wv, wn)) in enumerate(zip(got, want)):
        assert gv.shape == wv.shape, (what, d, gv.shape, wv.shape)
        assert np.array_equal(gn, wn), (what, "validity of dimension", d, np.flatnonzero(gn != wn)[:8])
        assert np.array_equal(gv, wv), (what, "values of dimension", d, np.flatnonzero((gv != wv).any(axis=1))[:8])
