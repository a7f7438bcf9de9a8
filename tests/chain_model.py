"""A numpy model of constant chains — the time dimensions the AQL compiler builds (query/time_bucketizer.go:72-174, 206-260):
`((column op1 c1) op2 c2) ...` evaluated node by node as the functors of query/functor.hpp do, written from their rules:
  * the common kind of (a, b) is float if either is, else signed if either is, else unsigned (query/utils.hpp:83-126); an integer
    literal is signed, so every integer node over a literal computes in int32;
  * Plus / Minus / Multiply wrap around at 32 bits; Divide and Mod are C's (truncating, the remainder has the dividend's sign),
    a zero divisor yields 0; Floor(x, y) = x - x % y;
  * a null operand yields bits 0 and null (functor.hpp:337-351), a bare column keeps its stored bits;
  * a node's value is stored in its scratch frame as the frame's type — between the integer types that keeps the bits.
Shared by tests/test_chain_model.py, test_chain_plans.py and test_chain_deferral.py."""
import numpy as np

from aresdb_amd import abi
from aresdb_amd.executor import Binary, Col, Const

EDGE_TS = np.array([0, 1, 3599, 3600, 28799, 28800, 86399, 345599, 345600, 2**31 - 1, 2**31, 2**32 - 1], np.uint32)
OFFSETS = (-43200, -28800, -1, 0, 19800, 50400)

_SIGNED = (abi.Int32, abi.Int16, abi.Int8)
_UNSIGNED = (abi.Uint32, abi.Uint16, abi.Uint8)


def _kind_of(dtype):
    return "i" if dtype in _SIGNED else "u" if dtype in _UNSIGNED else "f"


def _convert(bits, frm, to):
    """value conversion between the 32-bit kinds: integer <-> integer keeps the bits"""
    if frm == to or (frm != "f" and to != "f"):
        return bits
    if to == "f":
        x = bits.view(np.int32).astype(np.float32) if frm == "i" else bits.astype(np.float32)
        return x.view(np.uint32)
    f = bits.view(np.float32).astype(np.float64)
    return (f.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)


def evaluate(e, cols, valid, store=None):
    """(bits uint32, ok bool, kind) of expression `e` over {name: (data type, values)} / {name: validity or None}; store: the
    data type the node's value is stored as (default: its scratch frame's, e.out_type)."""
    if isinstance(e, Col):
        t, v = cols[e.name]
        ok = np.ones(len(v), bool) if valid[e.name] is None else np.asarray(valid[e.name], bool)
        kind = _kind_of(t)
        wide = v.astype(np.int64) if kind == "i" else v.astype(np.uint64).astype(np.int64)
        return (wide & 0xFFFFFFFF).astype(np.uint32) if kind != "f" else v.astype(np.float32).view(np.uint32), ok, kind
    assert isinstance(e, Binary) and isinstance(e.rhs, Const), e
    a, ok, ka = evaluate(e.lhs, cols, valid)
    n = len(a)
    if isinstance(e.rhs.value, float):
        kb, b = "f", np.full(n, np.float32(e.rhs.value)).view(np.uint32)
    else:
        kb, b = "i", np.full(n, int(e.rhs.value) & 0xFFFFFFFF, np.uint32)
    common = "f" if "f" in (ka, kb) else "i" if "i" in (ka, kb) else "u"
    x, y = _convert(a, ka, common), _convert(b, kb, common)
    if common == "f":
        fx, fy = x.view(np.float32), y.view(np.float32)
        with np.errstate(all="ignore"):
            r = {abi.Plus: fx + fy, abi.Minus: fx - fy, abi.Multiply: fx * fy, abi.Divide: fx / fy}[e.op].astype(np.float32).view(np.uint32)
    else:
        if common == "i":
            sx, sy = x.view(np.int32).astype(np.int64), y.view(np.int32).astype(np.int64)
        else:
            sx, sy = x.astype(np.int64), y.astype(np.int64)
        if e.op in (abi.Plus, abi.Minus, abi.Multiply):
            wide = sx + sy if e.op == abi.Plus else sx - sy if e.op == abi.Minus else sx * sy
        else:
            nz = np.where(sy == 0, 1, sy)
            q = np.where(sy == 0, 0, np.sign(sx) * np.sign(nz) * (np.abs(sx) // np.abs(nz)))
            m = np.where(sy == 0, 0, sx - q * nz)
            wide = q if e.op == abi.Divide else m if e.op == abi.Mod else sx - m
        r = (wide & 0xFFFFFFFF).astype(np.uint32)
    r = np.where(ok, r, np.uint32(0)).astype(np.uint32)
    stored = _kind_of(e.out_type if store is None else store)
    return _convert(r, common, stored), ok, stored


def dimension_bits(spec, cols, valid):
    """(value bytes per row as a uint array of the slot's width, validity) of a DimensionSpec, as the dimension vector stores it"""
    if isinstance(spec.expr, Col):
        t, v = cols[spec.expr.name]
        ok = np.ones(len(v), bool) if valid[spec.expr.name] is None else np.asarray(valid[spec.expr.name], bool)
        return v, ok
    bits, ok, _ = evaluate(spec.expr, cols, valid, store=spec.data_type)  # (an integer slot narrower than 4 bytes truncates)
    width = abi.DATA_TYPE_BYTES[spec.data_type]
    return bits.astype({4: np.uint32, 2: np.uint16, 1: np.uint8}[width]), ok


def grouped(dim_specs, batches, keep_of, add_of):
    """{key: sum} over `batches` = [(cols, valid)]: keep_of(cols, valid) -> bool rows, add_of(cols, valid) -> per-row addend.
    Keys as smoke.run_query returns them: ((value bytes, validity), ...) in query dimension order."""
    order = list(range(len(dim_specs)))
    out = {}
    for cols, valid in batches:
        keep = keep_of(cols, valid)
        add = add_of(cols, valid)
        fields = [dimension_bits(s, cols, valid) for s in dim_specs]
        rows = np.flatnonzero(keep)
        if not len(rows):
            continue
        packed = np.stack([fields[i][0][rows].astype(np.uint64) for i in order] + [fields[i][1][rows].astype(np.uint64) for i in order], axis=1)
        uniq, inverse = np.unique(packed, axis=0, return_inverse=True)
        sums = np.zeros(len(uniq), np.float64)
        np.add.at(sums, inverse.reshape(-1), add[rows].astype(np.float64))
        nd = len(order)
        for u, s in zip(uniq, sums):
            key = tuple((fields[i][0].dtype.type(u[k]).tobytes(), int(u[nd + k])) for k, i in enumerate(order))
            out[key] = out.get(key, 0.0) + s
    return out


def shapes(offset=-28800, inner=None):
    """The five rows of the compiler's table, by name: {name: expression over the column "request_at"}."""
    from aresdb_amd.queries import time_dimension
    return {
        "fixed_zone_hour": time_dimension("hour", "request_at", offset, inner),                 # Floor(Plus(ts, off), 3600)
        "hour_of_day": time_dimension("hour of day", "request_at", 0, inner),                   # Floor(Mod(ts, 86400), 3600)
        "fixed_zone_time_of_day": time_dimension("time of day", "request_at", offset, inner),   # Mod(Plus(ts, off), 86400)
        "hour_of_week": time_dimension("hour of week", "request_at", 0, inner),                 # Floor(Mod(Minus(ts, 4 d), 7 d), 3600)
        "fixed_zone_hour_of_week": time_dimension("hour of week", "request_at", offset, inner),  # ... over Plus(ts, off): four nodes
    }
