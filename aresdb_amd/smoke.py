"""One tiny end-to-end pass of the hot path, checked against the oracle (used by
__graft_entry__.smoke() and tests/test_executor.py): filter d1 < 90, dimensions
[floor(ts, 3600), d1, d2, d3], sum(m) — the shape of BASELINE config C3 — through both reduction
paths, over several batches."""
import numpy as np

from . import abi
from .columns import DeviceColumn
from .executor import BatchContext, BatchExecutor, fetch_results
from .queries import c3_plan  # noqa: F401  (re-exported for tests)


_MEASURE_NP = {abi.Float64: np.float64, abi.Int64: np.int64, abi.Float32: np.float32, abi.Int32: np.int32,
               abi.Uint32: np.uint32}


def synth_batch(rng, n, null_fraction=0.0):
    cols = {
        "ts": (abi.Uint32, rng.integers(0, 86400 * 7, n).astype(np.uint32)),
        "d1": (abi.Uint32, rng.integers(0, 100, n).astype(np.uint32)),
        "d2": (abi.Uint32, np.minimum(rng.zipf(1.1, n) - 1, 49).astype(np.uint32)),
        "d3": (abi.Uint32, rng.integers(0, 2, n).astype(np.uint32)),
        "m": (abi.Float32, (rng.integers(0, 400, n) / 4).astype(np.float32)),
    }
    valid = {k: (rng.random(n) >= null_fraction) if null_fraction else None for k in cols}
    return cols, valid


def run_query(be, plan, batches):
    ctx = BatchContext(be, plan)
    ex = BatchExecutor(ctx)
    for cols, valid in batches:
        dev = {k: DeviceColumn(be, t, v, valid=valid[k]) for k, (t, v) in cols.items()}
        n = len(next(iter(cols.values()))[1])
        # like the Go host, the batch's columns are released before the aggregation stage
        ex.run({k: d.vp for k, d in dev.items()}, n, owned_columns=[d.free for d in dev.values()])
    dims, valids, meas = fetch_results(ctx)
    calls = ctx.calls
    ctx.release()
    n = len(valids[0]) if valids else 0
    out = {}
    m = meas.view(_MEASURE_NP[plan.measure_type])
    for r in range(n):
        key = tuple((bytes(d[r * len(d) // n:(r + 1) * len(d) // n]), int(v[r])) for d, v in zip(dims, valids))
        out[key] = m[r]
    return out, calls


def run_query_native(be, plan, batches, stream=None, streams=None, join_columns=False):
    """The same query through the C++ host driver (libaresdriver.so) instead of the Python mirror.
    streams: two handles -> batches alternate between them like the Go host (query/aql_processor.go:218).
    join_columns: AresQuerySetJoinColumns — joined columns resolved once per batch, in row space."""
    from .driver import NativeQuery
    names = list(batches[0][0].keys())
    q = NativeQuery(be, plan, names, stream=stream, streams=streams)
    if join_columns:
        q.set_join_columns(True)
    if streams:
        stream = streams[0]
    for cols, valid in batches:
        dev = {k: DeviceColumn(be, t, v, valid=valid[k], stream=stream) for k, (t, v) in cols.items()}
        n = len(next(iter(cols.values()))[1])
        q.run({k: d.vp for k, d in dev.items()}, n, owned_allocations=[d.ptr for d in dev.values()])
        for d in dev.values():
            d.ptr = 0  # released by the driver before the aggregation stage, like the Go host
    dims, valids, meas = q.fetch()
    calls = q.calls
    n = q.result_size
    run_query_native.last_fused_batches = q.fused_batches
    q.release()
    out = {}
    m = meas.view(_MEASURE_NP[plan.measure_type])
    for r in range(n):
        key = tuple((bytes(d[r * len(d) // n:(r + 1) * len(d) // n]), int(v[r])) for d, v in zip(dims, valids))
        out[key] = m[r]
    return out, calls


def _hll_groups(dims, valids, counts, vec):
    """{dimension key: sorted register list [(register, rho)]} from the encoded HLL vector
    (sparse: uint32 rho << 16 | register; dense: one rho byte per register; query/common/hll.go:547-575)."""
    n = len(counts)
    out, off = {}, 0
    for r in range(n):
        key = tuple((bytes(d[r * len(d) // n:(r + 1) * len(d) // n]), int(v[r])) for d, v in zip(dims, valids))
        c = int(counts[r])
        if c < 4096:
            words = vec[off:off + 4 * c].view(np.uint32)
            regs = sorted((int(w & 0xFFFF), int(w >> 16)) for w in words)
            off += 4 * c
        else:
            dense = vec[off:off + 16384]
            regs = [(int(i), int(dense[i])) for i in np.nonzero(dense)[0]]
            off += 16384
        assert key not in out
        out[key] = regs
    assert off == len(vec)
    return out


def run_hll_query(be, plan, batches, native=False, stream=None):
    """A HyperLogLog query (plan.agg == AGGR_HLL) over `batches`; returns ({key: registers}, calls)."""
    from .executor import fetch_hll_results
    if native:
        from .driver import NativeQuery
        q = NativeQuery(be, plan, list(batches[0][0].keys()), stream=stream)
    else:
        ctx = BatchContext(be, plan)
        ex = BatchExecutor(ctx)
    for b, (cols, valid) in enumerate(batches):
        dev = {k: DeviceColumn(be, t, v, valid=valid[k], stream=stream) for k, (t, v) in cols.items()}
        n = len(next(iter(cols.values()))[1])
        last = b == len(batches) - 1
        if native:
            q.run({k: d.vp for k, d in dev.items()}, n, is_last_batch=last)
        else:
            ex.run({k: d.vp for k, d in dev.items()}, n, is_last_batch=last)
        for d in dev.values():
            d.free()
    if native:
        res, calls = q.fetch_hll(), q.calls
        q.release()
    else:
        res, calls = fetch_hll_results(ctx), ctx.calls
        ctx.release()
    return _hll_groups(*res), calls


def compare_results(got, want, rel=1e-6):
    assert got.keys() == want.keys(), f"group keys differ: {len(got)} vs {len(want)}"
    for k, v in want.items():
        g = got[k]
        assert abs(g - v) <= rel * max(1.0, abs(v)), (k, g, v)


def run_select_native(be, plan, batches):
    """A non-aggregation query through the C++ driver: (rows, per-dimension value bytes, validity bytes, fused batches)."""
    from .driver import NativeQuery
    q = NativeQuery(be, plan, list(batches[0][0].keys()))
    for cols, valid, *rest in batches:  # (an archive-shaped batch brings {column: run-length counts}: archive_batch)
        counts = rest[0] if rest else {}
        dev = {k: DeviceColumn(be, t, v, valid=valid[k], counts=counts.get(k)) for k, (t, v) in cols.items()}
        n = max(len(v) if k not in counts else int(counts[k][-1]) for k, (t, v) in cols.items())
        q.run({k: d.vp for k, d in dev.items()}, n)
        for d in dev.values():
            d.free()
    dims, valids, _ = q.fetch()
    out = (q.result_size, [bytes(d) for d in dims], [bytes(v) for v in valids], q.fused_batches)
    q.release()
    return out


def archive_batch(cols, valid, key):
    """The batch sorted by column `key` (nulls first), that column packed run-length as an archive batch stores its sort
    column — counts, a validity bit and a value per run: (cols, valid, {key: counts})."""
    t, v = cols[key]
    ok = np.ones(len(v), bool) if valid[key] is None else np.asarray(valid[key], bool)
    order = np.lexsort((v, ok))
    cols = {k: (tt, vv[order]) for k, (tt, vv) in cols.items()}
    valid = {k: (None if x is None else np.asarray(x)[order]) for k, x in valid.items()}
    v, ok = v[order], ok[order]
    head = np.ones(len(v), bool)
    head[1:] = (v[1:] != v[:-1]) | (ok[1:] != ok[:-1])
    starts = np.flatnonzero(head)
    cols[key], valid[key] = (t, v[starts]), ok[starts]
    return cols, valid, {key: np.concatenate([starts, [len(v)]]).astype(np.uint32)}


def stash_table(be, attr, attr_valid, join_column, num_last, zone=None):
    """A dimension table of at most four keys 0, 1, ... without any hashing: a cuckoo index with numHashes = 0 whose entries
    all lie in the stash (memstore/cuckoo_index.go layout: [RecordID x8][signature x8][key x8] per bucket, the stash behind
    the numBuckets buckets).  Key i -> record (batch 1, index i) of the one-batch column "attr" and, when given, of the Uint8
    time-zone enum column "zone".  (ForeignTable, what to free)"""
    from .executor import ForeignTable
    keys = len(attr)
    assert keys <= 4  # HASH_STASH_SIZE
    bucket = 8 * (8 + 1 + 4)
    table = np.zeros(2 * bucket, np.uint8)
    stash = table[bucket:]
    stash[:8 * keys].view(np.uint32)[:] = np.stack([np.ones(keys, np.uint32), np.arange(keys, dtype=np.uint32)], axis=1).reshape(-1)
    stash[64:64 + keys] = 1
    stash[72:72 + 4 * keys].view(np.uint32)[:] = np.arange(keys, dtype=np.uint32)
    index_buf = DeviceColumn(be, abi.Uint8, table)
    column = DeviceColumn(be, abi.Uint32, attr, valid=attr_valid)
    idx = abi.CuckooHashIndex()
    idx.buckets = index_buf.vp.BasePtr
    idx.keyBytes, idx.numHashes, idx.numBuckets = 4, 0, 1
    ft = ForeignTable(join_column=join_column, index=idx, batches={"attr": [column.vp]}, data_types={"attr": abi.Uint32},
                      base_batch_id=1, num_records_in_last_batch=num_last)
    keep = [index_buf, column]
    if zone is not None:
        keep.append(DeviceColumn(be, abi.Uint8, zone))
        ft.batches["zone"], ft.data_types["zone"] = [keep[-1].vp], abi.Uint8
    return ft, keep


def run_smoke(hip, oracle, n=20000, batches=3, seed=7):
    rng = np.random.default_rng(seed)
    data = [synth_batch(rng, n, null_fraction=0.01) for _ in range(batches)]
    for use_hash in (True, False):
        got, _ = run_query(hip, c3_plan(use_hash), data)
        want, _ = run_query(oracle, c3_plan(use_hash), data)
        compare_results(got, want)
    # one small select (SELECT floor(ts, 3600), d1, m WHERE d1 < 90 LIMIT n + 100): the fused select scan against the
    # ordinary sequence on the product, and against the oracle
    from .executor import Binary, Col, Const
    from .queries import select_plan
    columns = [(Binary(abi.Floor, Col("ts"), Const(3600)), abi.Uint32), (Col("d1"), abi.Uint32), (Col("m"), abi.Float32)]
    filters = [Binary(abi.LessThan, Col("d1"), Const(90))]
    plain = run_select_native(hip, select_plan(columns, filters, n + 100), data)
    fused = run_select_native(hip, select_plan(columns, filters, n + 100, use_fused_extension=True), data)
    want = run_select_native(oracle, select_plan(columns, filters, n + 100), data)
    assert plain[0] == n + 100 and plain[3] == 0 and fused[3] == 2, (plain[0], plain[3], fused[3])
    assert fused[:3] == plain[:3], "the fused select scan and the ordinary sequence disagree"
    assert plain[:3] == want[:3], "the select query disagrees with the oracle"
    # the same select over archive-shaped batches (sorted by d1, d1 run-length): every batch through the select scan, which
    # reads the runs where they lie, and the rows of the ordinary sequence
    arch = [archive_batch(cols, valid, "d1") for cols, valid in data]
    plain = run_select_native(hip, select_plan(columns, filters, -1), arch)
    fused = run_select_native(hip, select_plan(columns, filters, -1, use_fused_extension=True), arch)
    assert plain[0] > 0 and plain[3] == 0 and fused[3] == batches, (plain[0], plain[3], fused[3])
    assert fused[:3] == plain[:3], "the fused select scan and the ordinary sequence disagree on archive-shaped batches"
    # one tiny joined aggregation (d2 joined to a four-key table: filter on the joined attribute, group by the hour and the
    # attribute, SUM(m)) both ways through the C++ driver: the per-node join sequence, and the joined column resolved once per
    # batch in row space (AresJoinColumnsRun) with the batch run as a join-free one
    from .executor import DimensionSpec, QueryPlan
    ft, keep = stash_table(hip, np.array([10, 20, 600, 30]), np.array([1, 1, 1, 0], bool), "d2", 4)
    for use_hash in (True, False):
        plan = QueryPlan(filters=filters, foreign_tables=[ft], foreign_filters=[Binary(abi.LessThan, Col("attr", table=1), Const(500))],
                         dimensions=[DimensionSpec(Binary(abi.Floor, Col("ts"), Const(3600)), abi.Uint32),
                                     DimensionSpec(Col("attr", table=1), abi.Uint32)],
                         measure=Col("m"), agg=abi.AGGR_SUM_FLOAT, measure_type=abi.Float64, use_hash_reduction=use_hash)
        before = hip.join_column_stats()
        per_node, _ = run_query_native(hip, plan, data)
        assert hip.join_column_stats() == before
        resolved, _ = run_query_native(hip, plan, data, join_columns=True)
        assert hip.join_column_stats()["batches"] - before["batches"] == batches
        assert len(per_node) > 100, len(per_node)
        compare_results(resolved, per_node)
    for d in keep:
        d.free()
    # one tiny time-zone query — group by the hour in the joined zone's local time, FLOOR(CONVERT_TZ(ts, zone), 3600), and
    # SUM(m) — both ways through the C++ driver: the per-node sequence (HashLookup, Plus through the offset table into scratch,
    # Floor), and local time resolved once per batch in row space (AresLocalTimeColumnRun) with Floor over that column
    ft, keep = stash_table(hip, np.array([10, 20, 600, 30]), None, "d2", 4, zone=np.array([2, 0, 1, 9]))
    offsets = DeviceColumn(hip, abi.Int16, np.array([-18000, 19800, 3600], np.int16))  # (enum 9 lies past the table: offset 0)
    local_hour = Binary(abi.Floor, Binary(abi.Plus, Col("ts"), Col("zone", table=1), out_type=abi.Uint32, convert_tz=True), Const(3600))
    plan = QueryPlan(filters=filters, foreign_tables=[ft], dimensions=[DimensionSpec(local_hour, abi.Uint32), DimensionSpec(Col("d2"), abi.Uint32)],
                     measure=Col("m"), agg=abi.AGGR_SUM_FLOAT, measure_type=abi.Float64, use_hash_reduction=True,
                     timezone_lookup=offsets.vp.BasePtr, timezone_lookup_size=3)
    before = hip.local_time_column_stats()
    per_node, _ = run_query_native(hip, plan, data)
    assert hip.local_time_column_stats() == before
    resolved, _ = run_query_native(hip, plan, data, join_columns=True)
    assert hip.local_time_column_stats()["batches"] - before["batches"] == batches
    assert len(per_node) > 100, len(per_node)
    compare_results(resolved, per_node)
    for d in keep + [offsets]:
        d.free()
    # the last queries' shapes may still be compiling on the background thread: a process must not run into its exit handlers
    # with a compilation in flight (the compiler's own statics are torn down under it)
    hip.rtc_wait()
