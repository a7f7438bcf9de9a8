"""The ways a chosen-hash Program (tests/hash_sets.py) reaches HashReduce, and the child process the GPU tests run them in.

  run_plain        HashReduce over materialised vectors (cases.ExplicitGroupBy), batch behind the previous result
  run_query        the batch executor: the per-node sequence (whose pending transforms HashReduce consumes) through the
                   Python mirror or the C++ driver, or the C++ driver's one fused call per batch
  run_fused_calls  AresFusedFilterHashReduce called directly, batch by batch, with the host's fallback written out: a
                   declined batch takes the per-node sequence — so the decline, its message and the state of the previous
                   result's vectors around it can be observed

main(MODE, [NAME:AGG ...]) is the body of a child process: it runs every NAME:AGG on the HIP backend in MODE, compares each
with the model, and prints one `KERNELS` line (the kernel log of that run) and one `FACTS` line per case.  The library
latches its environment switches, so the GPU tests start one such child per environment (CHILD is its command line)."""
import ctypes as C
import json
import sys

import numpy as np

import cases
import harness as H
import hash_sets as S
from aresdb_amd import abi

_COL = {4: abi.Uint32, 2: abi.Uint16, 1: abi.Uint8}
_NP = {4: np.uint32, 2: np.uint16, 1: np.uint8}
# aggregate -> (type of the measure column, type of the measure vector) on the query paths
_QUERY_MEASURE = {"sum_u32": (abi.Uint32, abi.Uint32), "min_u32": (abi.Uint32, abi.Uint32), "max_u32": (abi.Uint32, abi.Uint32),
                  "sum_i32": (abi.Int32, abi.Int32), "min_i32": (abi.Int32, abi.Int32), "max_i32": (abi.Int32, abi.Int32),
                  "sum_i64": (abi.Int32, abi.Int64), "sum_f32": (abi.Float32, abi.Float32), "sum_f64": (abi.Float32, abi.Float64)}
_NP_OF = {abi.Uint32: np.uint32, abi.Int32: np.int32, abi.Float32: np.float32, abi.Int64: np.int64, abi.Float64: np.float64}


def assert_result(prog, agg_name, b, groups, table):
    """groups and {key: value} after batch b are the model's"""
    want, _ = prog.expected(agg_name, b)
    table = {k: S.decode_value(agg_name, v) for k, v in table.items()}
    assert groups == len(want) == len(table), (prog.name, agg_name, b, groups, len(want), len(table))
    if table != want:
        bad = [(k, table.get(k), want.get(k)) for k in list(want) + list(table) if table.get(k) != want.get(k)]
        raise AssertionError((prog.name, agg_name, b, len(bad), bad[:4]))


def run_plain(be, prog, agg_name):
    _, abi_agg, dtype, _ = S.AGGS[agg_name]
    values = prog.values(agg_name)
    batches = [(r, o, S.pack_avg(v) if agg_name == "avg" else v) for (r, o, _), v in zip(prog.batches, values)]
    return cases.ExplicitGroupBy(prog.ndw, batches, abi_agg, dtype).run_hash_reduce(be)


# ---- query paths ------------------------------------------------------------------------------------------------------------
def query_plan(prog, agg_name, fused_extension=False):
    from aresdb_amd.executor import Col, DimensionSpec, QueryPlan
    _, abi_agg, _, _ = S.AGGS[agg_name]
    dims = [DimensionSpec(Col(f"k{d}"), _COL[w]) for d, w in enumerate(prog.widths)]  # (vector order: widest first already)
    return QueryPlan(filters=[], dimensions=dims, measure=Col("m"), agg=abi_agg, measure_type=_QUERY_MEASURE[agg_name][1],
                     use_hash_reduction=True, use_fused_extension=fused_extension)


def column_batches(prog, agg_name):
    """the batches as source columns (smoke.run_query's format): dimension d is column k<d>, a null dimension is a null
    entry of its column, the measure is column m"""
    col_type = _QUERY_MEASURE[agg_name][0]
    out = []
    for (rows, valids, _), values in zip(prog.batches, prog.values(agg_name)):
        r = np.asarray(rows, np.uint64).reshape(len(rows), prog.nd)
        o = np.asarray(valids, bool).reshape(len(rows), prog.nd)
        cols = {f"k{d}": (_COL[w], r[:, d].astype(_NP[w])) for d, w in enumerate(prog.widths)}
        valid = {f"k{d}": (None if o[:, d].all() else o[:, d].copy()) for d in range(prog.nd)}
        cols["m"] = (col_type, np.asarray(values).astype(_NP_OF[col_type]))
        valid["m"] = None
        out.append((cols, valid))
    return out


def decode_query_result(prog, agg_name, got):
    """smoke.run_query's {((value bytes, valid), ...): numpy scalar} as the model states it"""
    out = {}
    for key, v in got.items():
        k = (tuple(int.from_bytes(b, "little") for b, _ in key), tuple(ok for _, ok in key))
        out[k] = v.item()
    return out


def run_query(be, prog, agg_name, how):
    """how: mirror (Python executor, per-node sequence) | driver (C++ driver, per-node sequence) | fused (C++ driver, one
    fused call per batch).  Returns (groups, {key: value}, fused batches or None)."""
    from aresdb_amd import smoke
    data = column_batches(prog, agg_name)
    if how == "mirror":
        got, _ = smoke.run_query(be, query_plan(prog, agg_name), data)
        fused = None
    else:
        got, _ = smoke.run_query_native(be, query_plan(prog, agg_name, how == "fused"), data)
        fused = smoke.run_query_native.last_fused_batches
    table = decode_query_result(prog, agg_name, got)
    assert len(table) == len(got)
    return len(got), table, fused


# ---- AresFusedFilterHashReduce, called directly -----------------------------------------------------------------------------
class _FusedQuery(C.Structure):
    """AresFusedQuery (include/ares_extensions.h)"""
    _fields_ = [("numFilters", C.c_int), ("filters", abi.FusedExpr * 4), ("numDims", C.c_int), ("dims", abi.FusedExpr * 4),
                ("measure", abi.FusedExpr), ("aggFunc", C.c_int)]


def _bare(column, out_type):
    e = abi.FusedExpr()
    e.lhs, e.arity, e.functor, e.outType = column.input(), 1, abi.Noop, out_type
    return e


def _fused_entry(be):
    fn = be._algo.AresFusedFilterHashReduce
    if fn.restype is not abi.CGoCallResHandle:  # (set once per library handle)
        fn.argtypes = [C.POINTER(_FusedQuery), C.c_int, abi.DimensionVector, C.c_void_p, C.c_int, abi.DimensionVector, C.c_void_p,
                       C.c_void_p, C.c_int]
        fn.restype = abi.CGoCallResHandle
    return fn


def run_fused_calls(be, prog, agg_name, read_fused=True):
    """Every batch through AresFusedFilterHashReduce, into result vectors allocated once; a batch the library declines
    ("not fusable ...") takes the per-node sequence: Noop transforms into the rows behind the previous result, then
    HashReduce.  Per batch: groups, the result, the decline message (None: fused), and for a declined batch whether the
    previous result's dimension rows were still in place; its values, read back after the declined attempt (which writes the
    ones that were still only defined by a table image), are compared with the model here.
    read_fused=False: the result of a batch that WAS fused is not read (map None) unless it is the last — reading the measure
    vector writes lazy values, and a host does not read between batches."""
    assert all(w == 4 for w in prog.widths)
    _, abi_agg, dtype, _ = S.AGGS[agg_name]
    out_type = _QUERY_MEASURE[agg_name][1]
    v = cases.ResultVectors(be, prog.ndw, sum(len(b[0]) for b in prog.batches) + 3, dtype)
    fn = _fused_entry(be)
    out, size = [], 0
    for b, (cols, valid) in enumerate(column_batches(prog, agg_name)):
        n = len(cols["m"][1])
        dev = {k: H.Column(be, t, c, valid=valid[k]) for k, (t, c) in cols.items()}
        q = _FusedQuery()
        q.numFilters, q.numDims, q.aggFunc = 0, prog.nd, abi_agg
        for d in range(prog.nd):
            q.dims[d] = _bare(dev[f"k{d}"], abi.Uint32)
        q.measure = _bare(dev["m"], out_type)
        keys_before = v.keys(0, size)  # (dimension rows only: reading the values would write the lazy ones)
        message, prev_intact = None, None
        try:
            g = abi._check(fn(C.byref(q), n, v.dims[0].struct(), v.meas[0].ptr, size, v.dims[1].struct(), v.meas[1].ptr, None, 0))
            be.wait()
        except abi.AresError as e:
            message = str(e)
            assert message.startswith("not fusable"), message
            table, keys_after = v.result(0, size)
            prev_intact = keys_after == keys_before
            if b:
                assert_result(prog, agg_name, b - 1, size, table)
            idx = H.Buf(be, nbytes=4 * max(n, 1))
            be.call("InitIndexVector", idx.ptr, 0, n, None, 0)
            for d, (vo, no, w) in enumerate(v.dims[0].dim_offsets()):
                be.call("UnaryTransform", dev[f"k{d}"].input(),
                        H.dimension_output(v.dims[0].values.ptr + vo + w * size, v.dims[0].values.ptr + no + size, abi.Uint32),
                        idx.ptr, n, None, 0, abi.Noop, None, 0)
            be.call("UnaryTransform", dev["m"].input(), H.measure_output(v.meas[0].ptr + v.vb * size, out_type, abi_agg), idx.ptr, n,
                    None, 0, abi.Noop, None, 0)
            g = v.hash_reduce(size + n, abi_agg)
            idx.free()
        for c in dev.values():
            c.free()
        last = b == len(prog.batches) - 1
        table = v.result(1, g)[0] if read_fused or message is not None or last else None
        out.append({"groups": g, "map": table, "declined": message, "prev_intact": prev_intact})
        size = g
        v.swap()
    v.free()
    return out


# ---- the child process ------------------------------------------------------------------------------------------------------
CHILD = [sys.executable, "-c", "import sys; sys.path.insert(0, 'tests'); import hash_paths; hash_paths.main(sys.argv[1], sys.argv[2:])"]


def main(mode, wanted):
    hip = H.hip_backend()
    programs = S.all_programs()
    for item in wanted:
        name, agg_name = item.split(":")[:2]  # (a third field only tells two runs of one case apart)
        prog = programs[name]()
        facts = {"case": item, "rows": [len(b[0]) for b in prog.batches]}
        hip.profiler_enable(True)
        if mode == "plain":
            res = run_plain(hip, prog, agg_name)
            for b, r in enumerate(res):
                assert_result(prog, agg_name, b, r["groups"], r["map"])
            # (collisions: the emitted dimensions are the lowest row's — the keys of the model's map — checked above)
            facts["groups"] = [r["groups"] for r in res]
        elif mode in ("mirror", "driver", "fused"):
            groups, table, fused = run_query(hip, prog, agg_name, mode)
            assert_result(prog, agg_name, len(prog.batches) - 1, groups, table)
            facts["groups"], facts["fused_batches"] = [groups], fused
        elif mode in ("fused_calls", "fused_calls_unread"):
            res = run_fused_calls(hip, prog, agg_name, read_fused=mode == "fused_calls")
            for b, r in enumerate(res):
                if r["map"] is None:
                    assert r["groups"] == len(prog.expected(agg_name, b)[0]), (item, b, r["groups"])
                else:
                    assert_result(prog, agg_name, b, r["groups"], r["map"])
            facts["groups"] = [r["groups"] for r in res]
            facts["declined"] = [r["declined"] for r in res]
            facts["prev_intact"] = [r["prev_intact"] for r in res]
        else:
            raise SystemExit(f"unknown mode {mode}")
        hip.wait()
        kernels = hip.profiler_report()
        hip.profiler_enable(False)
        print("KERNELS", json.dumps({"case": item, "kernels": {k.split("<")[0]: v[0] for k, v in kernels.items()}}))
        print("FACTS", json.dumps(facts), flush=True)
    print("DONE", len(wanted))

