"""The ways a chosen-hash Program (tests/sort_sets.py) reaches Sort + Reduce, and the child process the GPU tests run them in.

  run_vectors   Sort + Reduce over vectors the host wrote itself (cases.ExplicitGroupBy.run_sort_reduce): the real sort when the
                host reads the hash / index vector between the two calls (or ARES_SORT_FUSE=0), else the wide layout
                (fused_sort_reduce_vectors) — any slot widths, any validity bytes
  run_columns   the Go host's per-batch sequence at the ABI: the dimensions are bare columns (Uint32; Int64 / UUID for the wide
                slots) through Noop transforms, the measure a column through its transform; InitIndexVector, Sort, Reduce.
                Pending Uint32 transforms are consumed by the scan-fed path (fused_sort_reduce_run); an eager host (it reads
                the rows before it sorts) and wide slots take the wide layout over rows that exist
  run_query     the batch executor, use_hash_reduction off, through the Python mirror or the C++ driver: the final result in
                the order it is fetched

main(MODE, [NAME:AGG ...]) is the body of a child process: it runs every NAME:AGG on the HIP backend in MODE, compares each with
the model — group count, output rows IN ORDER, values, and the hash / index vectors where the mode reads them — bit for bit, and
prints one `KERNELS` line (the kernel log of that run) and one `FACTS` line per case.  The library latches its environment
switches, so the GPU tests start one such child per environment (CHILD is its command line)."""
import json
import sys

import numpy as np

import cases
import harness as H
import sort_model as M
import sort_sets as S
from aresdb_amd import abi

_WIDE_TYPE = {4: abi.Uint32, 8: abi.Int64, 16: abi.UUID}
MODES = ("vectors", "vectors_unread", "columns", "columns_read", "columns_eager", "columns_eager_read", "mirror", "driver")


def assert_batch(prog, agg_name, b, got, exp, what):
    """one Sort + Reduce call's observables against the model's account of it"""
    tag = (prog.name, agg_name, what, "batch", b)
    assert got["groups"] == exp.groups, tag + (got["groups"], exp.groups)
    if not np.array_equal(got["rows"], exp.rows):
        bad = np.flatnonzero((got["rows"] != exp.rows).any(axis=1))
        raise AssertionError(tag + ("rows differ", len(bad), bad[:4].tolist(), got["rows"][bad[:2]].tolist(), exp.rows[bad[:2]].tolist()))
    want = S.encode_values(agg_name, exp.values)
    if got["values"].tobytes() != want.tobytes():
        bad = np.flatnonzero(got["values"].view(want.dtype) != want)
        raise AssertionError(tag + ("values differ", len(bad), bad[:4].tolist(), got["values"][bad[:4]].tolist(), want[bad[:4]].tolist()))
    for key, model in (("hash", exp.sorted_hash), ("index", exp.sorted_index), ("hash_after", exp.sorted_hash), ("index_after", exp.sorted_index),
                       ("out_index", exp.out_index)):
        if key in got and not np.array_equal(got[key], model):
            bad = np.flatnonzero(got[key] != model)
            raise AssertionError(tag + (key, "differs", len(bad), bad[:4].tolist(), got[key][bad[:4]].tolist(), model[bad[:4]].tolist()))


def run_vectors(be, prog, agg_name, read=("sorted", "after")):
    _, abi_agg, dtype, _, _, _ = S.AGGS[agg_name]
    batches = []
    for rows, values in zip(prog.rows, prog.values(agg_name)):
        cols, oks = M.slot_columns(rows, prog.widths)
        batches.append((cols, oks, S.encode_values(agg_name, values)))
    return cases.ExplicitGroupBy(prog.ndw, batches, abi_agg, dtype).run_sort_reduce(be, read=read)


def run_columns(be, prog, agg_name, read=(), eager=False):
    """the per-batch sequence of query/aql_batchexecutor.go:236-251 with transforms in front (tests/test_sort_fused.py
    run_sequence, for given rows); every dimension must be valid — a transform writes zero bytes under a null"""
    assert all(prog.valids), "a null dimension's chosen value bytes cannot come out of a transform"
    _, abi_agg, dtype, _, col_type, out_type = S.AGGS[agg_name]
    vb = np.dtype(dtype).itemsize
    cap = sum(prog.sizes) + 5
    dv = [H.DimVector(be, cap, prog.ndw, True, False) for _ in range(2)]
    iv = [H.Buf(be, nbytes=4 * cap) for _ in range(2)]
    vv = [H.Buf(be, nbytes=vb * cap) for _ in range(2)]
    offs = dv[0].dim_offsets()

    def vec(i):
        s = dv[i].struct()
        s.IndexVector = iv[i].ptr
        return s

    def rows_of(d, n):
        blob = d.values.read(np.uint8)
        parts = [blob[vo:vo + n * w].reshape(n, w) for vo, _, w in offs] + [blob[no:no + n].reshape(n, 1) for _, no, _ in offs]
        return np.concatenate(parts, axis=1)

    out, res = [], 0
    for rows, measure in zip(prog.rows, prog.column_values(agg_name)):
        n = len(rows)
        slot_cols, _ = M.slot_columns(rows, prog.widths)
        dims = [H.Column(be, _WIDE_TYPE[w], raw_values=c.tobytes()) for c, w in zip(slot_cols, prog.widths)]
        mcol = H.Column(be, col_type, measure)
        idx = H.Buf(be, nbytes=4 * n)
        be.call("InitIndexVector", idx.ptr, 0, n, None, 0)
        for d, (vo, no, w) in enumerate(offs):
            o = H.dimension_output(dv[0].values.ptr + vo + w * res, dv[0].values.ptr + no + res, _WIDE_TYPE[w])
            be.call("UnaryTransform", dims[d].input(), o, idx.ptr, n, None, 0, abi.Noop, None, 0)
        be.call("UnaryTransform", mcol.input(), H.measure_output(vv[0].ptr + vb * res, out_type, abi_agg), idx.ptr, n, None, 0, abi.Noop, None, 0)
        be.wait()
        length = res + n
        if eager:  # the host looks at the batch's rows before it sorts: they are written
            rows_of(dv[0], length), vv[0].read(dtype, length)
        for c in dims + [mcol, idx]:  # cleanupBeforeAggregation
            c.free()
        entry = {}
        be.call("InitIndexVector", iv[0].ptr, 0, length, None, 0)
        be.call("Sort", vec(0), length, None, 0)
        if "sorted" in read:
            entry["hash"] = dv[0].hash.read(np.uint64, length)
            entry["index"] = iv[0].read(np.uint32, length)
        g = be.call("Reduce", vec(0), vv[0].ptr, vec(1), vv[1].ptr, vb, length, abi_agg, None, 0)
        be.wait()
        if "after" in read:
            entry["hash_after"] = dv[0].hash.read(np.uint64, length)
            entry["index_after"] = iv[0].read(np.uint32, length)
            entry["out_index"] = iv[1].read(np.uint32, g)
        entry.update(groups=g, rows=rows_of(dv[1], g), values=vv[1].read(dtype, g))
        out.append(entry)
        res = g
        dv.reverse()
        vv.reverse()
    for x in dv + iv + vv:
        x.free()
    return out


def run_query(be, prog, agg_name, how):
    """how: mirror (Python executor) | driver (C++ driver), the dimensions bare Uint32 columns, use_hash_reduction off.  Returns
    the fetched result as run_columns returns a batch's: groups, rows in order, values."""
    from aresdb_amd import smoke
    from aresdb_amd.executor import Col, DimensionSpec, QueryPlan
    assert prog.widths == (4, 4, 4, 4) and all(prog.valids)
    _, abi_agg, dtype, _, col_type, out_type = S.AGGS[agg_name]
    plan = QueryPlan(filters=[], dimensions=[DimensionSpec(Col(f"k{d}"), abi.Uint32) for d in range(4)], measure=Col("m"), agg=abi_agg,
                     measure_type=out_type, use_hash_reduction=False)
    data = []
    for rows, measure in zip(prog.rows, prog.column_values(agg_name)):
        slot_cols, _ = M.slot_columns(rows, prog.widths)
        cols = {f"k{d}": (abi.Uint32, c.copy().view(np.uint32).reshape(-1)) for d, c in enumerate(slot_cols)}
        cols["m"] = (col_type, measure)
        data.append((cols, {k: None for k in cols}))
    got, _ = (smoke.run_query if how == "mirror" else smoke.run_query_native)(be, plan, data)
    keys = list(got)  # (in the order the rows were fetched)
    rows = np.frombuffer(b"".join(b"".join(v for v, _ in k) + bytes(ok for _, ok in k) for k in keys), np.uint8).reshape(len(keys), -1) \
        if keys else np.zeros((0, 20), np.uint8)
    return {"groups": len(keys), "rows": rows, "values": np.array([got[k] for k in keys]).astype(dtype)}


# ---- the child process ------------------------------------------------------------------------------------------------------
CHILD = [sys.executable, "-c", "import sys; sys.path.insert(0, 'tests'); import sort_paths; sort_paths.main(sys.argv[1], sys.argv[2:])"]


def main(mode, wanted):
    assert mode in MODES, mode
    hip = H.hip_backend()
    programs = S.all_programs()
    compared = 0
    for item in wanted:
        name, agg_name = item.split(":")[:2]  # (a third field only tells two runs of one case apart)
        prog = programs[name]()
        census = [prog.census(b) for b in range(len(prog.sizes))]
        facts = {"case": item, "rows": prog.sizes, "model": prog.facts, "top_half_passes": prog.radix_passes(),
                 "listed": [[len(c.short), len(c.long), len(c.beyond)] for c in census]}
        hip.profiler_enable(True)
        if mode in ("mirror", "driver"):
            exp = prog.expected(agg_name, True)
            assert_batch(prog, agg_name, len(exp) - 1, run_query(hip, prog, agg_name, mode), exp[-1], mode)
            facts["groups"] = [exp[-1].groups]
            compared += 1
        else:
            read = ("sorted", "after") if mode in ("vectors", "columns_read", "columns_eager_read") else ()
            if mode.startswith("vectors"):
                exp, res = prog.expected(agg_name), run_vectors(hip, prog, agg_name, read)
            else:
                exp, res = prog.expected(agg_name, True), run_columns(hip, prog, agg_name, read, eager="eager" in mode)
            assert len(res) == len(exp)
            for b, (r, e) in enumerate(zip(res, exp)):
                assert_batch(prog, agg_name, b, r, e, mode)
            facts["groups"] = [r["groups"] for r in res]
            compared += len(res)
        hip.wait()
        kernels = hip.profiler_report()
        hip.profiler_enable(False)
        log = {}
        for k, v in kernels.items():
            log[k.split("<")[0]] = log.get(k.split("<")[0], 0) + v[0]
        print("KERNELS", json.dumps({"case": item, "kernels": log}))
        print("FACTS", json.dumps(facts), flush=True)
    print("DONE", len(wanted), "compared", compared)
