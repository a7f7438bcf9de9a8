"""BASELINE configs C2 and C4 at bench scale on one GPU (supplementary to bench.py, which is C3):
  C2  100 M rows, single uint32 predicate + COUNT(*)            (filter + reduce only)
  C4  N rows, fk -> cuckoo HashLookup join, group by (fk, joined attr) through Sort + Reduce
Prints one JSON line per config with per-kernel HIP-event times."""
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from aresdb_amd import abi, queries, workload
from aresdb_amd.driver import NativeQuery
from aresdb_amd.executor import Col, DimensionSpec, ForeignTable, QueryPlan


def timed(be, fn, reps=3):
    fn()
    best, rep = 1e9, None
    for _ in range(reps):
        be.profiler_enable(True); torch.cuda.synchronize(); t0 = time.perf_counter()
        r = fn(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
        k = be.profiler_report(); be.profiler_enable(False)
        if dt < best: best, rep, res = dt, k, r
    return best, rep, res


def c2(be, dev, rows):
    g = torch.Generator(device=dev); g.manual_seed(1)
    hi = 86400 * 30
    ts = torch.randint(0, hi, (rows,), dtype=torch.int32, device=dev, generator=g)
    valid = torch.rand((rows,), device=dev, generator=g) >= 0.01
    tsz = torch.where(valid, ts, torch.zeros((), dtype=torch.int32, device=dev))
    out = []
    for nbatches in (1, 4):  # one archive batch, and the same rows as four batches (the count accumulates across Reduce calls)
        edges = [rows * b // nbatches for b in range(nbatches + 1)]
        cols = [workload._pack_column(tsz[a:b], valid[a:b], abi.Uint32) for a, b in zip(edges[:-1], edges[1:])]
        for sel in (0.1, 0.5, 0.9):
            thr = int(hi * sel)
            def run():
                q = NativeQuery(be, queries.c2_plan(thr), ["ts"])
                for c in cols:
                    q.run({"ts": c.vp}, c.length)
                m = torch.empty(1, dtype=torch.int32, device=dev)
                be.call("AsyncCopyDeviceToDevice", m.data_ptr(), q.measure_vector, 4, None, 0); be.wait()
                c = int(m.item()); q.release(); return c
            dt, k, cnt = timed(be, run)
            want = int(((ts < thr) & valid).sum())
            filt = sum(ms for n, (c, ms) in k.items() if n.startswith("filter_"))
            out.append({"config": "C2", "rows": rows, "batches": nbatches, "selectivity": sel, "count": cnt, "count_ok": cnt == want,
                        "ms": dt * 1e3, "rows_per_s": rows / dt, "algorithmic_GBps": rows * 4.125 / dt / 1e9,
                        "kernel_ms": sum(ms for c, ms in k.values()),
                        "filter_kernels_roofline_frac": rows * 4.125 / (filt * 1e-3) / 1e9 / 8000.0 if filt else None,
                        "kernels": {n: round(ms / c, 4) for n, (c, ms) in k.items()}})
        del cols
    return out


def c4(be, dev, rows, nkeys):
    import cases, harness as H
    rng = np.random.default_rng(6)
    per_batch = 1 << 20
    keys = rng.choice(1 << 30, nkeys, replace=False).astype(np.uint32)
    attr = rng.integers(0, 1000, nkeys).astype(np.uint32)
    seeds = [int(x) for x in rng.integers(0, 1 << 32, 4)]
    nb = (nkeys + per_batch - 1) // per_batch
    table, placed = cases.build_cuckoo([int(k).to_bytes(4, "little") for k in keys], 4, max(nkeys // 6, 1), seeds, rng,
                                       record_of=lambda i: (1 + i // per_batch, i % per_batch))
    usable = np.array([i for i, k in enumerate(keys) if int(k).to_bytes(4, "little") in placed])
    tb = H.Buf(be, table)
    idx = abi.CuckooHashIndex(); idx.buckets = tb.ptr
    for i, s in enumerate(seeds): idx.seeds[i] = s
    idx.keyBytes, idx.numHashes, idx.numBuckets = 4, 4, max(nkeys // 6, 1)
    dcols = [H.Column(be, abi.Uint32, attr[b * per_batch:(b + 1) * per_batch]) for b in range(nb)]
    ft = ForeignTable(join_column="fk", index=idx, batches={"attr": [c.vp for c in dcols]}, data_types={"attr": abi.Uint32},
                      base_batch_id=1, num_records_in_last_batch=nkeys - (nb - 1) * per_batch)
    plan = QueryPlan(filters=[], foreign_tables=[ft], foreign_filters=[],
                     dimensions=[DimensionSpec(Col("fk"), abi.Uint32), DimensionSpec(Col("attr", table=1), abi.Uint32)],
                     measure=Col("amount"), agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32, use_hash_reduction=False)
    g = torch.Generator(device=dev); g.manual_seed(2)
    pick = torch.randint(0, len(usable), (rows,), device=dev, generator=g)
    fk = torch.from_numpy(keys[usable].astype(np.int64)).to(dev)[pick].to(torch.int32)
    amount = torch.randint(0, 100, (rows,), dtype=torch.int32, device=dev, generator=g)
    cf, ca = workload._pack_column(fk, None, abi.Uint32), workload._pack_column(amount, None, abi.Uint32)
    def run():
        q = NativeQuery(be, plan, ["fk", "amount"]); q.run({"fk": cf.vp, "amount": ca.vp}, rows)
        n = q.result_size
        m = torch.empty(n, dtype=torch.int32, device=dev)
        be.call("AsyncCopyDeviceToDevice", m.data_ptr(), q.measure_vector, 4 * n, None, 0); be.wait()
        tot = int(m.to(torch.int64).sum()); q.release(); return n, tot
    dt, k, (groups, tot) = timed(be, run)
    return [{"config": "C4", "rows": rows, "keys": int(len(usable)), "groups": groups, "sum_ok": tot == int(amount.to(torch.int64).sum()),
             "ms": dt * 1e3, "rows_per_s": rows / dt, "kernels": {n: round(ms / c, 4) for n, (c, ms) in k.items()}}]


def c4_spec(be, dev, rows, nkeys, batch_rows=1 << 26, join_columns=False):
    """C4 at BASELINE's stated size: `rows` fact rows in batches of `batch_rows`, an `nkeys`-key cuckoo index
    (every probe an HBM access), one group per key, Sort + Reduce with the previous result merged per batch.
    Every (fk, attr) -> sum is checked against a torch bincount of the same rows.
    join_columns (C4_JOIN_COLUMNS=1): AresQuerySetJoinColumns — the joined attribute resolved once per batch, in row space."""
    import harness as H
    from test_scale_parity import build_cuckoo_u32
    rng = np.random.default_rng(6)
    per_batch = 1 << 20
    t0 = time.perf_counter()
    keys = rng.permutation(np.arange(1, 4 * nkeys + 1, 4, dtype=np.uint32))[:nkeys]
    attr = (keys * np.uint32(2654435761) >> np.uint32(20)).astype(np.uint32)
    seeds = [int(x) for x in rng.integers(0, 1 << 32, 4)]
    num_buckets = nkeys // 5
    table, placed = build_cuckoo_u32(keys, num_buckets, seeds, per_batch)
    usable = np.nonzero(placed)[0]
    build_s = time.perf_counter() - t0
    nb = (nkeys + per_batch - 1) // per_batch
    tb = H.Buf(be, table)
    idx = abi.CuckooHashIndex(); idx.buckets = tb.ptr
    for i, s in enumerate(seeds): idx.seeds[i] = s
    idx.keyBytes, idx.numHashes, idx.numBuckets = 4, 4, num_buckets
    dcols = [H.Column(be, abi.Uint32, attr[b * per_batch:(b + 1) * per_batch]) for b in range(nb)]
    ft = ForeignTable(join_column="fk", index=idx, batches={"attr": [c.vp for c in dcols]}, data_types={"attr": abi.Uint32},
                      base_batch_id=1, num_records_in_last_batch=nkeys - (nb - 1) * per_batch)
    plan = QueryPlan(filters=[], foreign_tables=[ft], foreign_filters=[],
                     dimensions=[DimensionSpec(Col("fk"), abi.Uint32), DimensionSpec(Col("attr", table=1), abi.Uint32)],
                     measure=Col("amount"), agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32, use_hash_reduction=False)
    g = torch.Generator(device=dev); g.manual_seed(2)
    keys_d = torch.from_numpy(keys[usable].astype(np.int64)).to(dev)
    sums = torch.zeros(len(usable), dtype=torch.float64, device=dev)
    nbatches = (rows + batch_rows - 1) // batch_rows
    # priming pass, as bench.py's legs do: the shape's run-time kernel (the vector-sourced sort scan: dimension count and level-1
    # partition bits) is compiled in the background on first use — the batches that arrive before it is loaded take the real sort
    compiles = -1
    for _ in range(3):
        pq = NativeQuery(be, plan, ["fk", "amount"])
        pq.set_join_columns(join_columns)
        pn = 1 << 21
        pick = torch.randint(0, len(usable), (pn,), device=dev, generator=g)
        pcf = workload._pack_column(keys_d[pick].to(torch.int32), None, abi.Uint32)
        pca = workload._pack_column(torch.ones(pn, dtype=torch.int32, device=dev), None, abi.Uint32)
        pq.run({"fk": pcf.vp, "amount": pca.vp}, pn)
        be.wait(); pq.release(); del pcf, pca, pick
        state = be.rtc_wait()
        if state is None or state["compiles"] == compiles:
            break
        compiles = state["compiles"]
    q = NativeQuery(be, plan, ["fk", "amount"])
    q.set_join_columns(join_columns)
    probed0 = be.join_column_stats()["probed"]
    kernels, busy = {}, 0.0
    model = {}  # algorithmic bytes per kernel over the whole leg (the C4 table)
    def account(name, nbytes):
        model[name] = model.get(name, 0) + nbytes
    for b in range(nbatches):
        n = min(batch_rows, rows - b * batch_rows)
        prev_groups = q.result_size if b else 0
        # the first batches walk the keys in order so that every key occurs; the rest draw at random
        pick = (torch.arange(b * batch_rows, b * batch_rows + n, device=dev) % len(usable)) if (b + 1) * batch_rows <= len(usable) + batch_rows \
            else torch.randint(0, len(usable), (n,), device=dev, generator=g)
        amount = torch.randint(0, 100, (n,), dtype=torch.int32, device=dev, generator=g)
        sums += torch.bincount(pick, weights=amount.to(torch.float64), minlength=len(usable))
        cf, ca = workload._pack_column(keys_d[pick].to(torch.int32), None, abi.Uint32), workload._pack_column(amount, None, abi.Uint32)
        del pick, amount
        be.profiler_enable(True); torch.cuda.synchronize(); t0 = time.perf_counter()
        q.run({"fk": cf.vp, "amount": ca.vp}, n)
        torch.cuda.synchronize(); busy += time.perf_counter() - t0
        for name, (c, ms) in be.profiler_report().items():
            c0, m0 = kernels.get(name, (0, 0.0)); kernels[name] = (c0 + c, m0 + ms)
        be.profiler_enable(False)
        del cf, ca
        ng = q.result_size
        nd = 2
        account("hash_lookup_kernel", n * (128 + 4 + 8))             # one 104-byte bucket (two sectors pairs) + key + RecordID out
        account("transform_foreign_kernel", n * (8 + 32 + 4 + 1))   # RecordID + the value's sector + dimension slot + validity byte
        account("transform32_kernel", n * (8 + 32 + 4 + 1))         # (the same work when ARES_FOREIGN_GATHER=0)
        account("transform_fast_kernel", n * (4 + 4 + 1) + n * (4 + 4))  # fk -> dimension slot, amount -> measure vector
        account("sr_vector_scan_rtc", n * (nd * 5 + 4 + 16))        # dimension rows + value read, one 16-byte record written
        account("sr_count_kernel", n * 16)
        account("sr_split_kernel", n * (16 + 16))                   # (the second read of a workgroup's records comes from L2)
        account("sr_merge_kernel", n * 16 + prev_groups * (8 + 4) + ng * 24)  # records + previous hashes / values in, staged groups out
        account("sr_emit_kernel", ng * (24 + nd * 5 + nd * 5 + 4 + 8))    # staged group + its dimension row in; row, value, hash out
    groups = q.result_size
    dims, valids, meas = q.fetch()
    got_fk, got_attr, got_sum = dims[0].view(np.uint32), dims[1].view(np.uint32), meas.view(np.uint32)
    order = np.argsort(got_fk)
    korder = usable[np.argsort(keys[usable])]
    present = (sums > 0).cpu().numpy()[np.argsort(keys[usable])]
    want_sum = sums.cpu().numpy()[np.argsort(keys[usable])]
    ok = (groups == int(present.sum()) and np.array_equal(got_fk[order], keys[korder][present])
          and np.array_equal(got_attr[order], attr[korder][present])
          and np.array_equal(got_sum[order].astype(np.int64), want_sum[present].astype(np.int64)))
    q.release()
    for x in [tb] + dcols: x.free()
    # HashLookup: one 104-byte bucket probe per row and hash function tried, sector-granular: >= 128 B / row
    look = kernels.get("hash_lookup_kernel")
    out = {"config": "C4-spec", "join_columns": join_columns, "keys_probed_in_row_space": be.join_column_stats()["probed"] - probed0, "rows": rows, "batches": nbatches, "batch_rows": batch_rows, "keys": int(len(usable)),
           "cuckoo_table_MB": len(table) / 1e6, "cuckoo_build_s": build_s, "groups": groups, "key_level_check": "ok" if ok else "MISMATCH",
           "ms": busy * 1e3, "rows_per_s": rows / busy,
           "kernels": {n: {"launches": c, "avg_ms": ms / c, "total_ms": ms} for n, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}}
    out["kernel_rooflines"] = {
        name: {"bound": "hbm", "unit": "GB/s", "peak": 8000.0, "algorithmic_GB": model[name] / 1e9,
               "achieved": model[name] / (kernels[name][1] * 1e-3) / 1e9, "frac": model[name] / (kernels[name][1] * 1e-3) / 1e9 / 8000.0}
        for name in model if name in kernels and kernels[name][1] > 0}
    if look:
        per_launch_rows = rows / look[0]
        out["hash_lookup_roofline"] = {"bound": "hbm", "unit": "GB/s", "peak": 8000.0, "bytes_per_row": 128 + 4 + 8,
                                       "achieved": per_launch_rows * 140 / (look[1] / look[0] * 1e-3) / 1e9}
        out["hash_lookup_roofline"]["frac"] = out["hash_lookup_roofline"]["achieved"] / 8000.0
    return [out]


def trips_leg(be, dev, rows, batch_rows=1 << 26, steps=3):
    """The reference's example table and queries at bench scale (aresdb_amd/trips.py): request_at Uint32, city_id Uint16,
    status Uint8, fare Float32; two time filters + status == completed; dimensions [Floor(request_at, 3600), city_id in its
    2-byte slot]; SUM(fare) through HashReduce and COUNT(*) through Sort + Reduce (where the Go compiler sends it), both
    checked key by key.  One JSON row per query."""
    from aresdb_amd import trips
    batches = trips.trips_shard(rows, batch_rows, seed=11, device=dev)
    names = [n for n, _ in trips.COLUMNS]
    vps = [({k: rc.vp for k, rc in b.items()}, b["fare"].length) for b in batches]
    expected = trips.exact_groups(batches)
    streams = [be.call("CreateCudaStream", 0) for _ in range(2)]
    bytes_per_row = 4 + 2 + 1 + 4 + 4 / 8  # the four columns + their validity bits
    out = []
    for count in (False, True):
        plan = trips.trips_plan(count=count)
        packed = None
        def run():
            nonlocal packed
            q = NativeQuery(be, plan, names, streams=streams)
            if packed is None:
                packed = q.pack_batches(vps)
            q.run_batches(packed)
            return q
        compiles = -1
        for _ in range(4):       # priming passes: the shape's kernels are compiled in the background (a narrow plan's first
            run().release()      # batch, its later batches and their merges are different kernels) ... wait for them, as
            state = be.rtc_wait()  # bench.py does, until a pass builds nothing new
            if state is None or state["compiles"] == compiles:
                break
            compiles = state["compiles"]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(steps):
            q = run(); q.release()
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
        be.profiler_enable(True)
        q = run(); torch.cuda.synchronize()
        kernels = be.profiler_report(); be.profiler_enable(False)
        rep = trips.compare(q.fetch(), expected, count=count)
        groups = q.result_size
        q.release()
        top = max(kernels.items(), key=lambda kv: kv[1][1]) if kernels else None
        row = {"config": "trips-shaped", "query": "COUNT(*) via Sort+Reduce" if count else "SUM(fare) via HashReduce",
               "rows": rows, "batches": len(vps), "batch_rows": batch_rows, "groups": groups, "key_level_check": rep["status"],
               "merged_by_32bit_hash": rep.get("merged_by_32bit_hash"), "ms_per_step": dt * 1e3, "rows_per_s": rows / dt,
               "algorithmic_bytes_per_row": bytes_per_row, "algorithmic_GBps": rows * bytes_per_row / dt / 1e9,
               "kernel_ms_per_step": sum(ms for c, ms in kernels.values()),
               "kernels": {n: {"launches": c, "avg_ms": ms / c, "total_ms": ms} for n, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}}
        if top:
            ach = rows * bytes_per_row / (top[1][1] * 1e-3) / 1e9
            row["roofline"] = {"bound": "hbm", "kernel": top[0], "unit": "GB/s", "peak": 8000.0, "achieved": ach, "frac": ach / 8000.0,
                               "avg_launch_ms": top[1][1] / top[1][0], "launches": top[1][0],
                               "note": "algorithmic bytes of the whole job / total time of the dominant kernel"}
        out.append(row)
    return out


def chains_leg(be, dev, rows, batch_rows=1 << 26, steps=3, offset=-28800):
    """chains: the trips query (two time filters plus status) grouped by city_id and a time dimension that is a constant chain
    (aresdb_amd/queries.py: time_dimension, from query/time_bucketizer.go) — (a) the hourly bucket in a fixed zone,
    Floor(Plus(ts, off), 3600); (b) hour of day, Floor(Mod(ts, 86400), 3600); (c) hour of week in a fixed zone, four nodes.
    Each as SUM(fare) through HashReduce and as COUNT(*) through Sort + Reduce, checked key by key against an exact torch
    group-by of the same expression.  The inner nodes' scratch frames are defined, not written (ARES_CHAINS=0: written, and
    the root runs on the generic kernel); kernel times name which."""
    import dataclasses
    from aresdb_amd import trips
    from aresdb_amd.executor import DimensionSpec as Dim
    batches = trips.trips_shard(rows, batch_rows, seed=11, device=dev)
    names = [n for n, _ in trips.COLUMNS]
    vps = [({k: rc.vp for k, rc in b.items()}, b["fare"].length) for b in batches]
    streams = [be.call("CreateCudaStream", 0) for _ in range(2)]
    bytes_per_row = 4 + 2 + 1 + 4 + 4 / 8
    null_city = 1023

    def wrap(x):  # int64 -> the int32 it wraps to (an integer literal makes every node signed)
        return ((x + (1 << 31)) % (1 << 32)) - (1 << 31)

    def floor_to(x, y):  # x - x % y with C's remainder
        return x - torch.fmod(x, y)
    values = {"a": lambda t: floor_to(wrap(t + offset), 3600),
              "b": lambda t: floor_to(torch.fmod(t, 86400), 3600),
              "c": lambda t: floor_to(torch.fmod(wrap(wrap(t + offset) - 345600), 604800), 3600)}
    exprs = {"a": ("hour", offset), "b": ("hour of day", 0), "c": ("hour of week", offset)}
    labels = {"a": "fixed-zone hour", "b": "hour of day", "c": "fixed-zone hour of week"}

    def exact(which):
        """numpy (key = value u32 * 1024 + city code, sum(fare), count, first row) of the groups"""
        keys, sums, counts, firsts, base = [], [], [], [], 0
        for b in batches:
            ts, city, st, fare = (trips.column_values(b[k]) for k in ("request_at", "city_id", "status", "fare"))
            ok = {k: b[k].valid() for k in b}
            keep = (ts >= trips.TIME_RANGE[0]) & (ts < trips.TIME_RANGE[1]) & (st == trips.COMPLETED)
            for k in ("request_at", "status"):
                if ok[k] is not None:
                    keep &= ok[k]
            v = values[which](ts.to(torch.int64)) & 0xFFFFFFFF
            c = city.to(torch.int64) & 0xFFFF
            if ok["city_id"] is not None:
                c = torch.where(ok["city_id"], c, torch.full_like(c, null_city))
            mm = fare.to(torch.float64)
            if ok["fare"] is not None:
                mm = torch.where(ok["fare"], mm, torch.zeros_like(mm))
            rows_ = torch.arange(base, base + ts.numel(), dtype=torch.int64, device=dev)[keep]
            uniq, inv = torch.unique((v * 1024 + c)[keep], return_inverse=True)
            acc = torch.zeros(uniq.numel(), dtype=torch.float64, device=dev).index_add_(0, inv, mm[keep])
            cnt = torch.zeros(uniq.numel(), dtype=torch.int64, device=dev).index_add_(0, inv, torch.ones_like(inv))
            first = torch.full((uniq.numel(),), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, rows_, reduce="amin")
            keys.append(uniq.cpu().numpy()); sums.append(acc.cpu().numpy()); counts.append(cnt.cpu().numpy()); firsts.append(first.cpu().numpy())
            base += ts.numel()
            del ts, city, st, fare, keep, v, c, mm, rows_, uniq, inv, acc, cnt, first
        key, inv = np.unique(np.concatenate(keys), return_inverse=True)
        total, n, first = np.zeros(len(key)), np.zeros(len(key), np.int64), np.full(len(key), np.iinfo(np.int64).max)
        np.add.at(total, inv, np.concatenate(sums)); np.add.at(n, inv, np.concatenate(counts)); np.minimum.at(first, inv, np.concatenate(firsts))
        return key, total, n, first

    def compare(fetched, expected, count):
        dims, valids, meas = fetched
        key, sums, counts, first = expected
        if not np.frombuffer(valids[0], np.uint8).all():
            return {"status": "MISMATCH: a null time bucket survived the time filter"}
        g_ok = np.frombuffer(valids[1], np.uint8).astype(bool)
        got_key = np.frombuffer(dims[0], np.uint32).astype(np.int64) * 1024 + np.where(g_ok, np.frombuffer(dims[1], np.uint16).astype(np.int64), null_city)
        got_val = np.frombuffer(meas, np.uint32).astype(np.float64) if count else np.frombuffer(meas, np.float64)
        want_key, want_val, merged = key, counts.astype(np.float64), 0
        if not count:  # HashReduce: groups are 32-bit hashes, rows with equal hashes merge under the first
            c = key % 1024
            h = trips.murmur3_32_packed((key // 1024).astype(np.uint32), np.where(c == null_city, 0, c).astype(np.uint32), (c != null_city).astype(np.uint8))
            order = np.lexsort((first, h))
            head = np.ones(len(order), bool)
            head[1:] = h[order][1:] != h[order][:-1]
            ms = np.zeros(int(head.sum()))
            np.add.at(ms, np.cumsum(head) - 1, sums[order])
            want_key, want_val, merged = key[order][head], ms, int(len(key) - head.sum())
        why = None
        if len(got_key) != len(want_key):
            why = f"group count {len(got_key)} != expected {len(want_key)}"
        else:
            go, wo = np.argsort(got_key, kind="stable"), np.argsort(want_key, kind="stable")
            if (got_key[go] != want_key[wo]).any():
                why = f"{int((got_key[go] != want_key[wo]).sum())} dimension rows differ"
            elif (got_val[go] != want_val[wo]).any():
                why = f"{int((got_val[go] != want_val[wo]).sum())} values differ"
        return {"status": "ok" if why is None else "MISMATCH: " + why, "merged_by_32bit_hash": merged}
    out = []
    for which in os.environ.get("CHAINS_QUERIES", "a,b,c").split(","):
        expected = exact(which)
        dim = Dim(queries.time_dimension(exprs[which][0], "request_at", exprs[which][1]), abi.Uint32)
        for count in (False, True):
            base = trips.trips_plan(count=count)
            plan = dataclasses.replace(base, dimensions=[dim, base.dimensions[1]])
            packed = None
            def run():
                nonlocal packed
                q = NativeQuery(be, plan, names, streams=streams)
                if packed is None:
                    packed = q.pack_batches(vps)
                q.run_batches(packed)
                return q
            compiles = -1
            for _ in range(4):  # priming passes: until a pass builds no new kernel (trips_leg)
                run().release()
                state = be.rtc_wait()
                if state is None or state["compiles"] == compiles:
                    break
                compiles = state["compiles"]
            passes = []
            for _ in range(steps):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                q = run(); q.release()
                torch.cuda.synchronize(); passes.append((time.perf_counter() - t0) * 1e3)
            be.profiler_enable(True)
            q = run(); torch.cuda.synchronize()
            kernels = be.profiler_report(); be.profiler_enable(False)
            rep = compare(q.fetch(), expected, count)
            groups = q.result_size
            q.release()
            out.append({"config": "chains", "dimension": labels[which], "query": "COUNT(*) via Sort+Reduce" if count else "SUM(fare) via HashReduce",
                        "rows": rows, "batches": len(vps), "batch_rows": batch_rows, "offset": exprs[which][1], "groups": groups,
                        "key_level_check": rep["status"], "merged_by_32bit_hash": rep.get("merged_by_32bit_hash"),
                        "ms_per_pass": passes, "ms_per_step": float(np.median(passes)), "rows_per_s": rows / (float(np.median(passes)) * 1e-3),
                        "algorithmic_bytes_per_row": bytes_per_row, "kernel_ms_per_step": sum(ms for c, ms in kernels.values()),
                        "kernels": {n: {"launches": c, "avg_ms": ms / c, "total_ms": ms} for n, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}})
    for s in streams:
        be.call("DestroyCudaStream", s, 0)
    return out


def select_leg(be, dev, rows, batch_rows=1 << 26, steps=3, limits=(100, 1000000, -1)):
    """The non-aggregation query over the trips shard (aresdb_amd/trips.py: trips_select_plan — request_at, city_id, fare and a
    UUID key WHERE the two time filters AND status == completed) with limits 100, 1 M and none, through the ordinary sequence
    and through AresFusedFilterSelect, in the C++ driver.  The limited runs of the two paths are compared row for row, the
    unlimited ones by their row counts and first million rows.  One JSON row per (limit, path): ms per step and per 1 B rows,
    the per-kernel split, and for the unlimited query the algorithmic bytes — the five columns read once + dimRowBytes per
    survivor written — against 8 TB/s."""
    from aresdb_amd import trips
    gen = torch.Generator(device=dev)
    gen.manual_seed(12)
    batches = trips.trips_shard(rows, batch_rows, seed=11, device=dev)
    for b in batches:
        b["key"] = trips.key_column(b["fare"].length, gen, dev)
    names = [n for n, _ in trips.COLUMNS] + ["key"]
    vps = [({k: rc.vp for k, rc in b.items()}, b["fare"].length) for b in batches]
    streams = [be.call("CreateCudaStream", 0) for _ in range(2)]
    col_bytes = 4 + 2 + 1 + 4 + 16 + 5 / 8  # the five columns + their validity bits
    row_bytes = 4 + 2 + 4 + 16 + 4           # dimRowBytes: the four slots + one validity byte each
    out, first = [], {}
    for limit in limits:
        for fused in (False, True):
            plan = trips.trips_select_plan(limit=limit, fused=fused)
            packed = None
            def run():
                nonlocal packed
                q = NativeQuery(be, plan, names, streams=streams)
                q.set_max_batch_size(batch_rows)
                if packed is None:
                    packed = q.pack_batches(vps)
                q.run_batches(packed)
                return q
            run().release()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps):
                q = run(); q.release()
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
            be.profiler_enable(True)
            stats0 = be.select_stats()
            q = run(); torch.cuda.synchronize()
            kernels = be.profiler_report(); be.profiler_enable(False)
            stats1 = be.select_stats()
            n, fused_batches = q.result_size, q.fused_batches
            dims, valids, _ = q.fetch()
            q.release()
            head = [bytes(d[:w * min(n, 1000000)]) for d, w in zip(dims, (4, 2, 4, 16))] + [bytes(v[:min(n, 1000000)]) for v in valids]
            del dims, valids
            check = "first"
            if not fused:
                first[limit] = (n, head)
            else:
                check = "ok" if first[limit] == (n, head) else "MISMATCH against the ordinary sequence"
            kernel_ms = sum(ms for c, ms in kernels.values())
            row = {"config": "select", "limit": limit, "path": "extension" if fused else "ordinary", "rows": rows, "batches": len(vps),
                   "batch_rows": batch_rows, "result_rows": n, "fused_batches": fused_batches, "check": check,
                   "tiles_scanned": stats1["tiles"] - stats0["tiles"], "ms_per_step": dt * 1e3, "ms_per_1B_rows": dt * 1e3 * 1e9 / rows,
                   "kernel_ms_per_step": kernel_ms, "kernel_ms_per_1B_rows": kernel_ms * 1e9 / rows,
                   "kernels": {k: {"launches": c, "avg_ms": ms / c, "total_ms": ms} for k, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}}
            if limit < 0 and kernel_ms > 0:
                algo = rows * col_bytes + n * row_bytes
                row["algorithmic_bytes"] = algo
                row["algorithmic_GBps_of_kernel_time"] = algo / (kernel_ms * 1e-3) / 1e9
                row["frac_of_8TBps"] = row["algorithmic_GBps_of_kernel_time"] / 8000.0
            out.append(row)
    return out


def _trips_join_table(be, dev, batches, nkeys, gen, per_batch=1 << 20):
    """A dimension table for the trips shard with one 4-byte attribute `attr` of 0..999: a few thousand keys joined on city_id
    (index and attribute cache-resident), or — above 65536 keys — C4's table joined on a 4-byte column `fk` of random keys that
    is added to every batch, 1 % of them unknown to the table (every probe an HBM access).
    (ForeignTable, join column, index buffer, attribute columns)"""
    import cases, harness as H
    from test_scale_parity import build_cuckoo_u32
    rng = np.random.default_rng(6)
    seeds = [int(x) for x in rng.integers(0, 1 << 32, 4)]
    if nkeys <= 65536:  # joined on city_id (Uint16): keys 0 .. nkeys - 1, the cities among them
        join_column, key_bytes, num_buckets = "city_id", 2, max(nkeys // 5, 1)
        table, placed = cases.build_cuckoo([int(k).to_bytes(2, "little") for k in range(nkeys)], 2, num_buckets, seeds, rng,
                                           record_of=lambda i: (1 + i // per_batch, i % per_batch))
        attr = rng.integers(0, 1000, nkeys).astype(np.uint32)
    else:               # joined on `fk`: random keys of the table, 1 % unknown to it
        join_column, key_bytes, num_buckets = "fk", 4, nkeys // 5
        keys = rng.permutation(np.arange(1, 4 * nkeys + 1, 4, dtype=np.uint32))[:nkeys]
        attr = (keys * np.uint32(2654435761) >> np.uint32(20)).astype(np.uint32) % np.uint32(1000)
        table, _ = build_cuckoo_u32(keys, num_buckets, seeds, per_batch)
        keys_d = torch.from_numpy(keys.astype(np.int64)).to(dev)
        for b in batches:
            n = b["fare"].length
            pick = keys_d[torch.randint(0, nkeys, (n,), device=dev, generator=gen)]
            pick = torch.where(torch.rand((n,), device=dev, generator=gen) < 0.01, pick + 1, pick)  # (keys are 1 mod 4)
            b["fk"] = workload._pack_column(pick.to(torch.int32), None, abi.Uint32)
        del keys_d
    tb = H.Buf(be, table)
    idx = abi.CuckooHashIndex(); idx.buckets = tb.ptr
    for i, sd in enumerate(seeds): idx.seeds[i] = sd
    idx.keyBytes, idx.numHashes, idx.numBuckets = key_bytes, 4, num_buckets
    nb = (nkeys + per_batch - 1) // per_batch
    dcols = [H.Column(be, abi.Uint32, attr[b * per_batch:(b + 1) * per_batch]) for b in range(nb)]
    ft = ForeignTable(join_column=join_column, index=idx, batches={"attr": [c.vp for c in dcols]}, data_types={"attr": abi.Uint32},
                      base_batch_id=1, num_records_in_last_batch=nkeys - (nb - 1) * per_batch)
    return ft, join_column, tb, dcols


def join_agg_leg(be, dev, rows, batch_rows=1 << 26, steps=3, table_keys=(4000, 50_000_000)):
    """joinagg: the typical joined aggregation — the trips query (two time filters plus status) joined to a dimension table
    (select_join_leg's two tables), grouped by the hour and the joined attribute, with the foreign filter attr < 500 on or off:
    SUM(fare) through HashReduce and COUNT(*) through Sort + Reduce, each through the per-node join sequence, with
    AresQuerySetJoinColumns (the flavour AresJoinColumnsRun picks: direct for the 2-byte city_id) and — for city_id — with it under
    ARES_JOIN_COLUMNS=probe, on the same build, results compared key by key.  The paths alternate pass by pass; ms_per_step is a
    path's median of at least five.  One JSON row per (keys, foreign filter, query, path): wall ms, the per-kernel split, the
    keys probed in row space and the batches of either flavour."""
    from aresdb_amd import trips
    from aresdb_amd.executor import Binary, Const
    gen = torch.Generator(device=dev)
    gen.manual_seed(12)
    batches = trips.trips_shard(rows, batch_rows, seed=11, device=dev)
    streams = [be.call("CreateCudaStream", 0) for _ in range(2)]
    out = []
    for nkeys in table_keys:
        ft, join_column, tb, dcols = _trips_join_table(be, dev, batches, nkeys, gen)
        names = list(batches[0].keys())
        vps = [({k: rc.vp for k, rc in b.items()}, b["fare"].length) for b in batches]
        key_narrow = join_column == "city_id"
        for with_filter in (True, False):
            for count in (False, True):
                # per-node: the setter off; default: the setter on, the flavour the library picks (direct for the 2-byte city_id at
                # these batch sizes); probe: the setter on under ARES_JOIN_COLUMNS=probe (a 4-byte key probes anyway: no such leg)
                paths = ("per-node", "default", "probe") if key_narrow else ("per-node", "default")
                plan = trips.trips_plan(count=count)
                plan.dimensions[1] = DimensionSpec(Col("attr", table=1), abi.Uint32)
                plan.foreign_tables = [ft]
                plan.foreign_filters = [Binary(abi.LessThan, Col("attr", table=1), Const(500))] if with_filter else []
                packed = None
                def run(path):
                    nonlocal packed
                    if path == "probe":
                        os.environ["ARES_JOIN_COLUMNS"] = "probe"
                    else:
                        os.environ.pop("ARES_JOIN_COLUMNS", None)
                    be.reload_env()
                    q = NativeQuery(be, plan, names, streams=streams)
                    q.set_join_columns(path != "per-node")
                    if packed is None:
                        packed = q.pack_batches(vps)
                    q.run_batches(packed)
                    return q
                for path in paths:
                    compiles = -1
                    for _ in range(4):  # priming passes: the shape's kernels are compiled in the background
                        run(path).release()
                        state = be.rtc_wait()
                        if state is None or state["compiles"] == compiles:
                            break
                        compiles = state["compiles"]
                passes = {path: [] for path in paths}
                for _ in range(max(steps, 5)):  # the paths alternate, one pass each; the median per path is reported
                    for path in paths:
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                        run(path).release()
                        torch.cuda.synchronize(); passes[path].append((time.perf_counter() - t0) * 1e3)
                first = None
                for path in paths:
                    dt = float(np.median(passes[path])) / 1e3
                    be.profiler_enable(True)
                    stats0, flavours0 = be.join_column_stats(), be.join_column_flavour_stats()
                    q = run(path); torch.cuda.synchronize()
                    kernels = be.profiler_report(); be.profiler_enable(False)
                    stats1, flavours1 = be.join_column_stats(), be.join_column_flavour_stats()
                    n, calls = q.result_size, q.calls
                    dims, valids, meas = q.fetch()
                    q.release()
                    values = meas.view(np.uint32 if count else np.float64)
                    keyed = np.stack([dims[0].view(np.uint32), dims[1].view(np.uint32), valids[0].astype(np.uint32), valids[1].astype(np.uint32)], axis=1)
                    result = {tuple(k): v for k, v in zip(keyed.tolist(), values.tolist())}
                    check = "first"
                    if first is None:
                        first = result
                    elif result == first:
                        check = "ok"
                    else:  # (HashReduce groups by a 32-bit hash: which of two colliding rows represents their group depends on the path)
                        differing = len(set(result.items()) ^ set(first.items()))
                        check = "%d (key, value) pairs differ; totals %s" % (differing, "equal" if sum(result.values()) == sum(first.values()) else "DIFFER")
                    kernel_ms = sum(ms for c, ms in kernels.values())
                    out.append({"config": "joinagg", "table_keys": nkeys, "join_column": join_column, "foreign_filter": with_filter,
                                "query": "COUNT(*) via Sort+Reduce" if count else "SUM(fare) via HashReduce", "path": path,
                                "join_columns": path != "per-node", "rows": rows,
                                "batches": len(vps), "batch_rows": batch_rows, "groups": n, "abi_calls": calls, "check": check,
                                "keys_probed_in_row_space": stats1["probed"] - stats0["probed"],
                                "direct_batches": flavours1["direct"] - flavours0["direct"], "probe_batches": flavours1["probe"] - flavours0["probe"],
                                "ms_per_step": dt * 1e3, "ms_per_pass": [round(x, 3) for x in passes[path]],
                                "ms_per_1B_rows": dt * 1e3 * 1e9 / rows, "kernel_ms_per_step": kernel_ms, "kernel_ms_per_1B_rows": kernel_ms * 1e9 / rows,
                                "kernels": {k: {"launches": c, "avg_ms": ms / c, "total_ms": ms} for k, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}})
                    print(json.dumps(out[-1]), flush=True)
                os.environ.pop("ARES_JOIN_COLUMNS", None)
                be.reload_env()
        tb.free()
        for c in dcols:
            c.free()
    return out


def tz_agg_leg(be, dev, rows, batch_rows=1 << 26, steps=3, nkeys=4000, zones=400):
    """tzagg: trips per hour in each city's local time — the trips query (two time filters plus status) joined on city_id
    (Uint16) to joinagg's 4 000-key table given a Uint8 zone column and a 400-entry offset table, grouped by
    FLOOR(CONVERT_TZ(request_at, zone), 3600) and city_id: SUM(fare) through HashReduce and COUNT(*) through Sort + Reduce, each
    through the per-node sequence (setter off), with AresQuerySetJoinColumns (the direct flavour of AresLocalTimeColumnRun: the
    batches have more rows than the key has values) and with it under ARES_LOCAL_TIME=probe, on one build; results compared key
    by key.  One JSON row per (query, path): wall ms per step, the per-kernel split and the keys probed in row space."""
    import harness as H
    from aresdb_amd import trips
    from aresdb_amd.executor import Binary, Const
    gen = torch.Generator(device=dev)
    gen.manual_seed(12)
    batches = trips.trips_shard(rows, batch_rows, seed=11, device=dev)
    streams = [be.call("CreateCudaStream", 0) for _ in range(2)]
    ft, join_column, tb, dcols = _trips_join_table(be, dev, batches, nkeys, gen)
    rng = np.random.default_rng(8)
    zone = H.Column(be, abi.Uint8, rng.integers(0, 256, nkeys).astype(np.uint8))
    ft.batches["zone"], ft.data_types["zone"] = [zone.vp], abi.Uint8
    offsets = H.Buf(be, (rng.integers(-48, 57, zones) * 900).astype(np.int16))
    names = list(batches[0].keys())
    vps = [({k: rc.vp for k, rc in b.items()}, b["fare"].length) for b in batches]
    out = []
    for count in (False, True):
        first = None
        for path in ("per-node", "direct", "probe"):
            plan = trips.trips_plan(count=count)
            local = Binary(abi.Plus, Col("request_at"), Col("zone", table=1), out_type=abi.Uint32, convert_tz=True)
            plan.dimensions[0] = DimensionSpec(Binary(abi.Floor, local, Const(3600)), abi.Uint32)
            plan.foreign_tables = [ft]
            plan.timezone_lookup, plan.timezone_lookup_size = offsets.ptr, zones
            if path == "probe":
                os.environ["ARES_LOCAL_TIME"] = "probe"
            else:
                os.environ.pop("ARES_LOCAL_TIME", None)
            be.reload_env()
            packed = None
            def run():
                nonlocal packed
                q = NativeQuery(be, plan, names, streams=streams)
                q.set_join_columns(path != "per-node")
                if packed is None:
                    packed = q.pack_batches(vps)
                q.run_batches(packed)
                return q
            compiles = -1
            for _ in range(4):  # priming passes: the shape's kernels are compiled in the background
                run().release()
                state = be.rtc_wait()
                if state is None or state["compiles"] == compiles:
                    break
                compiles = state["compiles"]
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps):
                run().release()
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
            be.profiler_enable(True)
            stats0 = be.local_time_column_stats()
            q = run(); torch.cuda.synchronize()
            kernels = be.profiler_report(); be.profiler_enable(False)
            stats1 = be.local_time_column_stats()
            n, calls = q.result_size, q.calls
            dims, valids, meas = q.fetch()
            q.release()
            values = meas.view(np.uint32 if count else np.float64)
            keyed = np.stack([dims[0].view(np.uint32), dims[1].view(np.uint16).astype(np.uint32), valids[0].astype(np.uint32),
                              valids[1].astype(np.uint32)], axis=1)
            result = {tuple(k): v for k, v in zip(keyed.tolist(), values.tolist())}
            check = "first"
            if first is None:
                first = result
            elif result == first:
                check = "ok"
            else:  # (HashReduce groups by a 32-bit hash: which of two colliding rows represents their group depends on the path)
                differing = len(set(result.items()) ^ set(first.items()))
                check = "%d (key, value) pairs differ; totals %s" % (differing, "equal" if sum(result.values()) == sum(first.values()) else "DIFFER")
            kernel_ms = sum(ms for c, ms in kernels.values())
            out.append({"config": "tzagg", "table_keys": nkeys, "zones": zones, "query": "COUNT(*) via Sort+Reduce" if count else "SUM(fare) via HashReduce",
                        "path": path, "rows": rows, "batches": len(vps), "batch_rows": batch_rows, "groups": n, "abi_calls": calls, "check": check,
                        "local_time_batches": stats1["batches"] - stats0["batches"], "direct_batches": stats1["direct"] - stats0["direct"],
                        "keys_probed_in_row_space": stats1["probed"] - stats0["probed"], "ms_per_step": dt * 1e3,
                        "ms_per_1B_rows": dt * 1e3 * 1e9 / rows, "kernel_ms_per_step": kernel_ms, "kernel_ms_per_1B_rows": kernel_ms * 1e9 / rows,
                        "kernels": {k: {"launches": c, "avg_ms": ms / c, "total_ms": ms} for k, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}})
            print(json.dumps(out[-1]), flush=True)
    os.environ.pop("ARES_LOCAL_TIME", None)
    be.reload_env()
    for c in [tb, zone, offsets] + dcols:
        c.free()
    return out


def select_join_leg(be, dev, rows, batch_rows=1 << 26, steps=3, limits=(100, 1000000, -1), table_keys=(4000, 50_000_000)):
    """select_leg's query with a join: the trips select plus one 4-byte attribute of a dimension table, selected, once with a
    foreign filter on it (attr < 500 of 0..999) and once without; limits 100, 1 M and none; through the ordinary sequence
    (HashLookup over every survivor, filters carrying the record ids, a foreign gather) and through AresFusedFilterJoinSelect on
    the same build, rows compared as select_leg compares them.  Two table sizes: a few thousand keys joined on city_id (the
    realistic one, index and attribute cache-resident) and C4's 50 M keys joined on a 4-byte column of random keys `fk`
    (every probe an HBM access).  One JSON row per (keys, foreign filter, limit, path): ms per step, the per-kernel split, tiles
    scanned and keys probed."""
    import cases, harness as H
    from aresdb_amd import trips
    from aresdb_amd.executor import Binary, Const
    from test_scale_parity import build_cuckoo_u32
    gen = torch.Generator(device=dev)
    gen.manual_seed(12)
    batches = trips.trips_shard(rows, batch_rows, seed=11, device=dev)
    for b in batches:
        b["key"] = trips.key_column(b["fare"].length, gen, dev)
    streams = [be.call("CreateCudaStream", 0) for _ in range(2)]
    per_batch = 1 << 20
    out = []
    for nkeys in table_keys:
        ft, join_column, tb, dcols = _trips_join_table(be, dev, batches, nkeys, gen)
        names = list(batches[0].keys())
        vps = [({k: rc.vp for k, rc in b.items()}, b["fare"].length) for b in batches]
        first = {}
        for with_filter in (True, False):
            for limit in limits:
                for fused in (False, True):
                    plan = trips.trips_select_plan(limit=limit, fused=fused)
                    plan.dimensions.insert(2, DimensionSpec(Col("attr", table=1), abi.Uint32))
                    plan.foreign_tables = [ft]
                    plan.foreign_filters = [Binary(abi.LessThan, Col("attr", table=1), Const(500))] if with_filter else []
                    packed = None
                    def run():
                        nonlocal packed
                        q = NativeQuery(be, plan, names, streams=streams)
                        q.set_max_batch_size(batch_rows)
                        if packed is None:
                            packed = q.pack_batches(vps)
                        q.run_batches(packed)
                        return q
                    run().release()
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    for _ in range(steps):
                        q = run(); q.release()
                    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
                    be.profiler_enable(True)
                    stats0 = be.select_join_stats()
                    q = run(); torch.cuda.synchronize()
                    kernels = be.profiler_report(); be.profiler_enable(False)
                    stats1 = be.select_join_stats()
                    n, fused_batches = q.result_size, q.fused_batches
                    dims, valids, _ = q.fetch()
                    q.release()
                    widths = [abi.DATA_TYPE_BYTES[d.data_type] for d in plan.dimensions]
                    head = [bytes(d[:w * min(n, 1000000)]) for d, w in zip(dims, widths)] + [bytes(v[:min(n, 1000000)]) for v in valids]
                    del dims, valids
                    check = "first"
                    if not fused:
                        first[(with_filter, limit)] = (n, head)
                    else:
                        check = "ok" if first[(with_filter, limit)] == (n, head) else "MISMATCH against the ordinary sequence"
                    kernel_ms = sum(ms for c, ms in kernels.values())
                    out.append({"config": "select_join", "table_keys": nkeys, "join_column": join_column, "foreign_filter": with_filter, "limit": limit,
                                "path": "extension" if fused else "ordinary", "rows": rows, "batches": len(vps), "batch_rows": batch_rows,
                                "result_rows": n, "fused_batches": fused_batches, "check": check,
                                "tiles_scanned": stats1["tiles"] - stats0["tiles"], "keys_probed": stats1["probed"] - stats0["probed"],
                                "ms_per_step": dt * 1e3, "ms_per_1B_rows": dt * 1e3 * 1e9 / rows,
                                "kernel_ms_per_step": kernel_ms, "kernel_ms_per_1B_rows": kernel_ms * 1e9 / rows,
                                "kernels": {k: {"launches": c, "avg_ms": ms / c, "total_ms": ms} for k, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}})
                    print(json.dumps(out[-1]), flush=True)
        tb.free()
        for c in dcols:
            c.free()
    return out


def select_archive_leg(be, dev, rows, batch_rows=1 << 26, steps=3, limits=(100, 1000000, -1), city=7):
    """select_leg's query plus city_id == `city` over ARCHIVE-shaped batches: every batch of the trips shard sorted by
    (city_id, status) and those two columns packed run-length (workload._pack_run_length), as an archive batch stores its
    sort columns.  Ordinary sequence and AresFusedFilterSelect on the same build, rows compared as select_leg compares them.
    One JSON row per (limit, path) with the tiles scanned, rejected by a run of a filter column, and staged in LDS."""
    from aresdb_amd import trips
    from aresdb_amd.executor import Binary, Const
    gen = torch.Generator(device=dev)
    gen.manual_seed(12)
    batches = []
    for b in trips.trips_shard(rows, batch_rows, seed=11, device=dev):
        n = b["fare"].length
        key = trips.key_column(n, gen, dev)
        vals = {k: trips.column_values(b[k]) for k, _ in trips.COLUMNS}
        ok = {k: b[k].valid() for k, _ in trips.COLUMNS}
        code = lambda k: torch.where(ok[k], vals[k].to(torch.int64) + 1, torch.zeros((), dtype=torch.int64, device=dev))
        order = torch.argsort(code("city_id") * 256 + code("status"), stable=True)
        out = {}
        for k, dt in trips.COLUMNS:
            v, o = vals[k][order], ok[k][order]
            out[k] = workload._pack_run_length(v, o, dt) if k in ("city_id", "status") else trips._pack(v, o, dt)
        k64 = key.blob[key.values_off:key.values_off + 16 * n].view(torch.int64).view(n, 2)
        kraw = torch.stack([k64[:, 0][order], k64[:, 1][order]], dim=1).reshape(-1).view(torch.uint8)
        kok = key.valid()[order].to(torch.uint8)
        nb = (n + 7) // 8
        if nb * 8 != n:
            kok = torch.cat([kok, torch.zeros(nb * 8 - n, dtype=torch.uint8, device=dev)])
        weights = (1 << torch.arange(8, device=dev, dtype=torch.int32)).to(torch.uint8)
        off = workload._align64(nb)
        blob = torch.zeros(off + kraw.numel() + 64, dtype=torch.uint8, device=dev)
        blob[:nb] = (kok.view(nb, 8) * weights).sum(dim=1, dtype=torch.int32).to(torch.uint8)
        blob[off:off + kraw.numel()] = kraw
        out["key"] = workload.ResidentColumn(blob, off, abi.UUID, n, True)
        batches.append(out)
        del vals, ok, order, key, k64, kraw, kok, b
    names = [n for n, _ in trips.COLUMNS] + ["key"]
    vps = [({k: rc.vp for k, rc in b.items()}, b["fare"].length) for b in batches]
    runs = {k: sum(b[k].runs for b in batches) for k in ("city_id", "status")}
    streams = [be.call("CreateCudaStream", 0) for _ in range(2)]
    out, first = [], {}
    for limit in limits:
        for fused in (False, True):
            plan = trips.trips_select_plan(limit=limit, fused=fused)
            plan.filters.insert(0, Binary(abi.Equal, Col("city_id"), Const(int(city))))
            packed = None
            def run():
                nonlocal packed
                q = NativeQuery(be, plan, names, streams=streams)
                q.set_max_batch_size(batch_rows)
                if packed is None:
                    packed = q.pack_batches(vps)
                q.run_batches(packed)
                return q
            run().release()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps):
                q = run(); q.release()
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
            be.profiler_enable(True)
            stats0, runs0 = be.select_stats(), be.select_run_stats()
            q = run(); torch.cuda.synchronize()
            kernels = be.profiler_report(); be.profiler_enable(False)
            stats1, runs1 = be.select_stats(), be.select_run_stats()
            n, fused_batches = q.result_size, q.fused_batches
            dims, valids, _ = q.fetch()
            q.release()
            head = [bytes(d[:w * min(n, 1000000)]) for d, w in zip(dims, (4, 2, 4, 16))] + [bytes(v[:min(n, 1000000)]) for v in valids]
            del dims, valids
            check = "first"
            if not fused:
                first[limit] = (n, head)
            else:
                check = "ok" if first[limit] == (n, head) else "MISMATCH against the ordinary sequence"
            kernel_ms = sum(ms for c, ms in kernels.values())
            out.append({"config": "selectarchive", "limit": limit, "path": "extension" if fused else "ordinary", "rows": rows, "batches": len(vps),
                        "batch_rows": batch_rows, "city": city, "cities": trips.CITIES, "runs": runs, "result_rows": n, "fused_batches": fused_batches,
                        "check": check, "tiles": sum((r + 4095) // 4096 for _, r in vps), "tiles_scanned": stats1["tiles"] - stats0["tiles"],
                        "tiles_rejected": runs1["rejected"] - runs0["rejected"], "tiles_staged": runs1["staged"] - runs0["staged"],
                        "ms_per_step": dt * 1e3, "ms_per_1B_rows": dt * 1e3 * 1e9 / rows, "kernel_ms_per_step": kernel_ms,
                        "kernel_ms_per_1B_rows": kernel_ms * 1e9 / rows,
                        "kernels": {k: {"launches": c, "avg_ms": ms / c, "total_ms": ms} for k, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}})
    return out


def wide_key_legs(be, dev, which, rows, batch_rows=1 << 26, steps=3):
    """Sort + Reduce over group keys in dimension slots of 8 and 16 bytes (rows of such a query exist when Sort arrives: a
    transform into a wide slot runs at once), through the C++ driver in the Go call order, COUNT(*):
      c3int64  C3's query with d2 stored as an Int64 dimension;
      uuid     a UUID key of ~2 M distinct values and a Uint32 dimension of two, no filter.
    Every key's count is compared with a torch bincount of the same rows, and the fetched rows must come in ascending order
    of their 64-bit row hash.  ARES_SORT_VECTORS=0 in the environment gives the same legs on the real row sort."""
    from aresdb_amd import check
    from aresdb_amd.executor import Const
    gen = torch.Generator(device=dev); gen.manual_seed(21)
    nb = (rows + batch_rows - 1) // batch_rows
    if which == "c3int64":
        shard = workload.c3_shard(rows, batch_rows, seed=1, device=dev)
        plan = queries.c3_plan(sort_measure="count")
        plan.dimensions[2] = DimensionSpec(Col("d2"), abi.Int64)
        names = ["ts", "d1", "d2", "d3"]
        space = 169 * 101 * 51 * 3
        want = torch.zeros(space, dtype=torch.int64, device=dev)
        batches = []
        for b in shard:
            v = {k: b[k].values().to(torch.int64) for k in names}
            ok = {k: b[k].valid() for k in names}
            code = lambda k, x: torch.where(ok[k], x + 1, torch.zeros((), dtype=torch.int64, device=dev))
            c = ((code("ts", v["ts"] // 3600) * 101 + code("d1", v["d1"])) * 51 + code("d2", v["d2"])) * 3 + code("d3", v["d3"])
            want += torch.bincount(c[ok["d1"] & (v["d1"] < 90)], minlength=space)
            cols = {k: b[k] for k in ("ts", "d1", "d3")}
            cols["d2"] = workload._pack_column(v["d2"], ok["d2"], abi.Int64)  # the same values in an 8-byte column
            batches.append(cols)
            del v, ok, c
        bytes_per_row = 4 + 4 + 8 + 4 + 4 / 8
    else:
        nkeys = 2_000_000
        keys = torch.randint(-(1 << 62), 1 << 62, (nkeys, 2), dtype=torch.int64, device=dev, generator=gen)
        names = ["key", "d3"]
        plan = QueryPlan(filters=[], dimensions=[DimensionSpec(Col("key"), abi.UUID), DimensionSpec(Col("d3"), abi.Uint32)], measure=Const(1),
                         agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32, use_hash_reduction=False)
        want = torch.zeros(3 * nkeys, dtype=torch.int64, device=dev)
        batches = []
        for b in range(nb):
            n = min(batch_rows, rows - b * batch_rows)
            pick = torch.randint(0, nkeys, (n,), device=dev, generator=gen)
            d3 = torch.randint(0, 2, (n,), dtype=torch.int32, device=dev, generator=gen)
            ok3 = torch.rand((n,), device=dev, generator=gen) >= 0.01
            d3 = torch.where(ok3, d3, torch.zeros((), dtype=torch.int32, device=dev))
            want += torch.bincount(pick * 3 + torch.where(ok3, d3.to(torch.int64) + 1, torch.zeros((), dtype=torch.int64, device=dev)),
                                   minlength=3 * nkeys)
            kc = workload._pack_column(torch.stack([keys[:, 0][pick], keys[:, 1][pick]], dim=1).reshape(-1), None, abi.UUID)
            kc.length = n  # (two int64 per value)
            batches.append({"key": kc, "d3": workload._pack_column(d3, ok3, abi.Uint32)})
            del pick, d3, ok3
        bytes_per_row = 16 + 4 + 1 / 8
    vps = [({k: rc.vp for k, rc in b.items()}, b[names[-1]].length) for b in batches]
    streams = [be.call("CreateCudaStream", 0) for _ in range(2)]
    packed = None
    def run():
        nonlocal packed
        q = NativeQuery(be, plan, names, streams=streams)
        if packed is None:
            packed = q.pack_batches(vps)
        q.run_batches(packed)
        return q
    compiles = -1
    for _ in range(4):  # priming passes: the shape's scan is compiled in the background — until a pass builds nothing new
        run().release()
        state = be.rtc_wait()
        if state is None or state["compiles"] == compiles:
            break
        compiles = state["compiles"]
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        run().release()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
    be.profiler_enable(True)
    q = run(); torch.cuda.synchronize()
    kernels = be.profiler_report(); be.profiler_enable(False)
    groups = q.result_size
    dims, valids, meas = q.fetch()
    q.release()
    counts = meas.view(np.uint32).astype(np.int64)
    width_order = sorted(range(len(dims)), key=lambda i: -plan.dimensions[i].width)  # (stable: vector order)
    hashes = check.row_hashes_of_fetched([dims[i] for i in width_order], [valids[i] for i in width_order])
    ordered = bool((hashes[1:] > hashes[:-1]).all())
    want = want.cpu().numpy()
    if which == "c3int64":
        code = lambda v, ok, dt_: np.where(ok != 0, v.view(dt_).astype(np.int64) + 1, 0)
        got = np.where(valids[0] != 0, dims[0].view("<u4").astype(np.int64) // 3600 + 1, 0) * 101 + code(dims[1], valids[1], "<u4")
        got = (got * 51 + code(dims[2], valids[2], "<i8")) * 3 + code(dims[3], valids[3], "<u4")
    else:
        hk = keys.cpu().numpy().view(np.uint64)
        pair = np.dtype([("hi", np.uint64), ("lo", np.uint64)])
        kp = np.empty(len(hk), pair); kp["hi"], kp["lo"] = hk[:, 1], hk[:, 0]
        order = np.argsort(kp)
        gk = dims[0].view(np.uint64).reshape(-1, 2)
        gp = np.empty(len(gk), pair); gp["hi"], gp["lo"] = gk[:, 1], gk[:, 0]
        at = np.minimum(np.searchsorted(kp[order], gp), len(hk) - 1)
        found = kp[order][at] == gp
        got = np.where(found, order[at].astype(np.int64) * 3 + np.where(valids[1] != 0, dims[1].view("<u4").astype(np.int64) + 1, 0), -1)
    ok = bool(groups == int((want > 0).sum()) and (got >= 0).all() and len(np.unique(got)) == len(got) and np.array_equal(want[got], counts))
    return [{"config": "wide-keys", "leg": which, "sort_vectors": os.environ.get("ARES_SORT_VECTORS", "1") != "0", "rows": rows, "batches": nb,
             "batch_rows": batch_rows, "groups": groups, "key_level_check": "ok" if ok else "MISMATCH", "ascending_row_hashes": ordered,
             "ms_per_step": dt * 1e3, "rows_per_s": rows / dt, "algorithmic_bytes_per_row": bytes_per_row,
             "kernel_ms_per_step": sum(ms for c, ms in kernels.values()),
             "kernels": {n: {"launches": c, "avg_ms": ms / c, "total_ms": ms} for n, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}}]


def sort_float_leg(be, dev, rows, batch_rows=1 << 26, steps=3):
    """c3sortfloat: the headline query under the reference's SHIPPED configuration (enable_hash_reduction: false): SUM(m) of a
    Float32 column into float64 through Sort + Reduce, `rows` rows as 64 Mi-row batches resident in HBM, a measure column of
    full-mantissa floats (workload.c3_shard(quantised=False)).  Float aggregates order GROUPS in LDS tables
    (sort_reduce_fused.hip); ARES_SR_FLOAT=0 in the environment gives the same leg on the real row sort.  Every key's sum is
    compared at rel = 1e-6 with the exact group-by of aresdb_amd/check.py and the rows must come in ascending order of their
    64-bit row hash.  ms_per_step: wall time of a whole pass; kernel_ms_per_step: the kernels' own (HIP events)."""
    from aresdb_amd import check
    shard = workload.c3_shard(rows, batch_rows, seed=1, device=dev, quantised=False)
    names = [n for n, _ in workload.C3_COLUMNS]
    plan = queries.c3_plan(use_hash_reduction=False)
    vps = [({k: rc.vp for k, rc in b.items()}, b["m"].length) for b in shard]
    streams = [be.call("CreateCudaStream", 0) for _ in range(2)]
    packed = None
    def run():
        nonlocal packed
        q = NativeQuery(be, plan, names, streams=streams)
        if packed is None:
            packed = q.pack_batches(vps)
        q.run_batches(packed)
        return q
    compiles = -1
    for _ in range(4):  # priming passes: the shape's scan is compiled in the background — until a pass builds nothing new
        run().release()
        state = be.rtc_wait()
        if state is None or state["compiles"] == compiles:
            break
        compiles = state["compiles"]
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        run().release()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
    be.profiler_enable(True)
    q = run(); torch.cuda.synchronize()
    kernels = be.profiler_report(); be.profiler_enable(False)
    groups = q.result_size
    rep = check.compare_result(q.fetch(), check.exact_groups(shard), hash_identity=False, rel=1e-6, ordered=True)
    q.release()
    bytes_per_row = 5 * (4 + 1 / 8)
    return [{"config": "c3-sort-float", "query": "SUM(m) float64 via Sort+Reduce", "float_aggregates_fused": os.environ.get("ARES_SR_FLOAT", "1") != "0",
             "rows": rows, "batches": len(vps), "batch_rows": batch_rows, "groups": groups, "key_level_and_order_check_rel_1e-6": rep["status"],
             "ms_per_step": dt * 1e3, "ms_per_1e9_rows": dt * 1e3 * 1e9 / rows, "rows_per_s": rows / dt, "algorithmic_bytes_per_row": bytes_per_row,
             "kernel_ms_per_step": sum(ms for c, ms in kernels.values()),
             "kernels": {n: {"launches": c, "avg_ms": ms / c, "total_ms": ms} for n, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}}]


def sort_avg_legs(be, dev, which, rows, batch_rows=1 << 26, steps=3):
    """c3sortavg: AVG(m) over the C3 shard with full-mantissa measures (sort_float_leg's shard and query, AGGR_AVG_FLOAT: the Go
    compiler's 8-byte {f32 average, u32 count} measure, always through Sort + Reduce).  tripsavg: AVG(fare) over the trips-shaped
    shard (67 k groups, a Uint16 slot, a Uint8 filter column).  Rows must come in ascending order of their 64-bit row hash (C3),
    every key's count must be exact and its average within 1e-4 * sum|x| / count of the exact group-by (check.compare_means).
    ARES_SR_SCAN_FED=0 in the environment gives the same legs on the wide layout over materialised rows."""
    import dataclasses
    from aresdb_amd import check, trips
    if which == "c3sortavg":
        shard = workload.c3_shard(rows, batch_rows, seed=1, device=dev, quantised=False)
        names, last = [n for n, _ in workload.C3_COLUMNS], "m"
        plan = dataclasses.replace(queries.c3_plan(use_hash_reduction=False), agg=abi.AGGR_AVG_FLOAT)
        bytes_per_row = 5 * (4 + 1 / 8)
    else:
        shard = trips.trips_shard(rows, batch_rows, seed=11, device=dev)
        names, last = [n for n, _ in trips.COLUMNS], "fare"
        plan = dataclasses.replace(trips.trips_plan(), agg=abi.AGGR_AVG_FLOAT, use_hash_reduction=False)
        bytes_per_row = 4 + 2 + 1 + 4 + 4 / 8
    vps = [({k: rc.vp for k, rc in b.items()}, b[last].length) for b in shard]
    streams = [be.call("CreateCudaStream", 0) for _ in range(2)]
    packed = None
    def run():
        nonlocal packed
        q = NativeQuery(be, plan, names, streams=streams)
        if packed is None:
            packed = q.pack_batches(vps)
        q.run_batches(packed)
        return q
    compiles = -1
    for _ in range(4):  # priming passes: the shape's scan is compiled in the background — until a pass builds nothing new
        run().release()
        state = be.rtc_wait()
        if state is None or state["compiles"] == compiles:
            break
        compiles = state["compiles"]
    passes = []
    for _ in range(steps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        run().release()
        torch.cuda.synchronize(); passes.append((time.perf_counter() - t0) * 1e3)
    dt = sum(passes) / len(passes) * 1e-3
    be.profiler_enable(True)
    q = run(); torch.cuda.synchronize()
    kernels = be.profiler_report(); be.profiler_enable(False)
    groups = q.result_size
    fetched = q.fetch()
    if which == "c3sortavg":
        rep = check.compare_mean_result(fetched, check.exact_means(shard))
    else:
        why = check.compare_means(trips.fetched_codes(fetched), fetched[2], trips.exact_means(shard))
        rep = {"status": "ok" if why is None else "MISMATCH: " + why}
    q.release()
    return [{"config": "c3-sort-avg" if which == "c3sortavg" else "trips-shaped", "query": "AVG(%s) via Sort+Reduce" % last,
             "scan_fed": os.environ.get("ARES_SR_SCAN_FED", "1") != "0", "rows": rows, "batches": len(vps), "batch_rows": batch_rows, "groups": groups,
             "counts_exact_and_averages_rel_1e-4": rep["status"], "groups_without_a_valid_measure": rep.get("groups_without_a_valid_measure"),
             "ms_per_step": dt * 1e3, "ms_per_pass": passes, "ms_per_1e9_rows": dt * 1e3 * 1e9 / rows, "rows_per_s": rows / dt,
             "algorithmic_bytes_per_row": bytes_per_row, "kernel_ms_per_step": sum(ms for c, ms in kernels.values()),
             "kernels": {n: {"launches": c, "avg_ms": ms / c, "total_ms": ms} for n, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}}]


def hll(be, dev, rows, groups, users, batches=2):
    """countdistincthll(user) group by g: `batches` batches of `rows` rows through the C++ driver."""
    from aresdb_amd.executor import Unary
    plan = QueryPlan(filters=[], dimensions=[DimensionSpec(Col("g"), abi.Uint32)], measure=Unary(abi.GetHLLValue, Col("user")),
                     agg=abi.AGGR_HLL, measure_type=abi.Uint32)
    gen = torch.Generator(device=dev); gen.manual_seed(3)
    cols = []
    for _ in range(batches):
        gcol = torch.randint(0, groups, (rows,), dtype=torch.int32, device=dev, generator=gen)
        ucol = torch.randint(0, users, (rows,), dtype=torch.int32, device=dev, generator=gen)
        cols.append((workload._pack_column(gcol, None, abi.Uint32), workload._pack_column(ucol, None, abi.Uint32)))
    import ctypes
    def preagg():  # {batches pre-aggregated, declined after the scan, their rows, the surviving entries} (ARES_HLL_PREAGG=0: all zero)
        c = (ctypes.c_ulonglong * 4)()
        be._algo.AresHllPreaggStats.argtypes, be._algo.AresHllPreaggStats.restype = [ctypes.POINTER(ctypes.c_ulonglong)], None
        be._algo.AresHllPreaggStats(c)
        return [int(x) for x in c]
    def run():
        q = NativeQuery(be, plan, ["g", "user"])
        before, ratios, start = preagg(), [], preagg()
        for b, (cg, cu) in enumerate(cols):
            q.run({"g": cg.vp, "user": cu.vp}, rows, is_last_batch=b == batches - 1)
            now = preagg()
            ratios.append(round((now[3] - before[3]) / (now[2] - before[2]), 4) if now[2] > before[2] else None)  # m / n; None: rows were sorted
            before = now
        n = q.result_size
        dims, valids, counts, vec = q.fetch_hll()
        end = preagg()
        q.release(); return n, int(counts.astype(np.int64).sum()), len(vec), (ratios, end[0] - start[0], end[1] - start[1])
    run(); be.rtc_wait()  # (the scan generated for the layout is compiled in the background: the timed runs find it loaded)
    dt, k, (n, regs, nbytes, (ratios, took, declined)) = timed(be, run)
    total = sum(ms for c, ms in k.values())
    front = ("hll_scan_rtc", "hll_dedup_kernel", "hll_index_range_kernel", "sort_key_hist_kernel", "sort_hash_hist_kernel", "digit_start_kernel",
             "radix_pass_kernel", "hll_reduce_kernel")  # steps 1 + 2; everything else is the merge, the encoding and the transforms
    return [{"config": "HLL", "rows": rows * batches, "batches": batches, "groups": groups, "users": users, "result_dims": n, "registers": regs,
             "hll_bytes": nbytes, "ms": dt * 1e3, "rows_per_s": rows * batches / dt, "survivors_per_row": ratios, "batches_preaggregated": took, "batches_declined": declined,
             "kernel_ms": round(total, 3), "sort_reduce_share": round(sum(ms for n_, (c, ms) in k.items() if n_ in front) / total, 3) if total else None,
             "kernels": {n_: round(ms / c, 4) for n_, (c, ms) in k.items()},
             "kernel_total_ms": {n_: round(ms, 3) for n_, (c, ms) in sorted(k.items(), key=lambda kv: -kv[1][1])}}]


def _geo_shapes(num_shapes, pts_per_shape):
    """`num_shapes` closed rings of `pts_per_shape` vertices, radii 3..12 degrees, centres uniform over +-80: (lats, longs, shape numbers)"""
    rng = np.random.default_rng(9)
    lats, longs, sidx = [], [], []
    for sh in range(num_shapes):
        cx, cy = rng.uniform(-80, 80, 2)
        ang = np.sort(rng.uniform(0, 2 * np.pi, pts_per_shape)); rad = rng.uniform(3, 12)
        ys, xs = (cy + rad * np.sin(ang)).astype(np.float32), (cx + rad * np.cos(ang)).astype(np.float32)
        lats += list(ys) + [ys[0]]; longs += list(xs) + [xs[0]]; sidx += [sh] * (pts_per_shape + 1)
    return lats, longs, sidx


def geo(be, dev, rows, num_shapes, pts_per_shape, geo_column=False):
    """geography_intersects filter + shape dimension + COUNT over `rows` points.  geo_column (GEO_COLUMN=1):
    AresQuerySetGeoColumn — the verdict resolved in row space; no filter, every row live: the shape where row space gains nothing."""
    import harness as H
    from aresdb_amd.executor import Const, GeoIntersection
    lats, longs, sidx = _geo_shapes(num_shapes, pts_per_shape)
    shapes = H.GeoShapes(be, np.float32(lats), np.float32(longs), sidx, num_shapes)
    plan = QueryPlan(filters=[], dimensions=[DimensionSpec(Const(0), abi.Uint8)], measure=Const(1), agg=abi.AGGR_SUM_UNSIGNED,
                     measure_type=abi.Uint32, use_hash_reduction=False,
                     geo=GeoIntersection(shapes.buf.ptr, num_shapes, len(lats), "pt", 0, True, 0))
    gen = torch.Generator(device=dev); gen.manual_seed(4)
    pts = (torch.rand((rows, 2), device=dev, generator=gen) * 200 - 100).to(torch.float32).contiguous()
    vp = abi.VectorPartySlice()
    vp.BasePtr, vp.NullsOffset, vp.ValuesOffset, vp.DataType, vp.Length, vp.StartingIndex = pts.data_ptr(), 0, 0, abi.GeoPoint, rows, 0
    def run():
        q = NativeQuery(be, plan, ["pt"]); q.set_geo_column(geo_column); q.run({"pt": vp}, rows)
        n = q.result_size
        m = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        be.call("AsyncCopyDeviceToDevice", m.data_ptr(), q.measure_vector, 4 * n, None, 0); be.wait()
        tot = int(m[:n].to(torch.int64).sum()); q.release(); return n, tot
    dt, k, (n, inside) = timed(be, run)
    shapes.free()
    return [{"config": "GEO", "geo_column": geo_column, "rows": rows, "shapes": num_shapes, "polygon_points": len(lats), "groups": n, "inside": inside,
             "ms": dt * 1e3, "rows_per_s": rows / dt, "edge_tests_per_s": rows * (len(lats) - 1) / dt,
             "kernels": {n_: round(ms / c, 4) for n_, (c, ms) in k.items()}}]


def geo_query_leg(be, dev, rows, batch_rows=1 << 26, steps=3, shape_sets=((100, 20), (250, 400))):
    """geoquery: trips per geofence — the trips table plus a GeoPoint column (5 % null points, uniform over +-100 degrees), two time
    filters that keep 2 of the 8 days and status == completed, grouped by the hour and the shape: COUNT(*) through Sort + Reduce and
    SUM(fare) through HashReduce, each through the per-node geo sequence and with AresQuerySetGeoColumn on the same build, results
    compared key by key.  One JSON row per (shapes, query, path): wall ms per step (median of `steps`), the per-kernel split, and
    for the row-space kernel the live rows, the wavefront-chunks walked and the edge tests per second over live rows."""
    import harness as H
    from aresdb_amd import trips
    from aresdb_amd.executor import Const, GeoIntersection
    from aresdb_amd.workload import ResidentColumn, _align64
    gen = torch.Generator(device=dev)
    gen.manual_seed(14)
    batches = trips.trips_shard(rows, batch_rows, seed=13, device=dev)
    for b in batches:
        n = b["fare"].length
        pts = (torch.rand((n, 2), device=dev, generator=gen) * 200 - 100).to(torch.float32).contiguous().view(torch.uint8).reshape(-1)
        valid = (torch.rand((n,), dtype=torch.float32, device=dev, generator=gen) >= 0.05).to(torch.uint8)
        nb = (n + 7) // 8
        if nb * 8 != n:
            valid = torch.cat([valid, torch.zeros(nb * 8 - n, dtype=torch.uint8, device=dev)])
        weights = (1 << torch.arange(8, device=dev, dtype=torch.int32)).to(torch.uint8)
        off = _align64(nb)
        blob = torch.zeros(off + pts.numel() + 64, dtype=torch.uint8, device=dev)
        blob[:nb] = (valid.view(nb, 8) * weights).sum(dim=1, dtype=torch.int32).to(torch.uint8)
        blob[off:off + pts.numel()] = pts
        b["pt"] = ResidentColumn(blob, off, abi.GeoPoint, n, True)
        del pts, valid
    streams = [be.call("CreateCudaStream", 0) for _ in range(2)]
    names = list(batches[0].keys())
    vps = [({k: rc.vp for k, rc in b.items()}, b["fare"].length) for b in batches]
    time_range = (86400 * 3, 86400 * 5)
    out = []
    for num_shapes, pts_per_shape in shape_sets:
        lats, longs, sidx = _geo_shapes(num_shapes, pts_per_shape)
        shapes = H.GeoShapes(be, np.float32(lats), np.float32(longs), sidx, num_shapes)
        for count in (True, False):
            first = None
            for on in (False, True):
                plan = trips.trips_plan(count=count, time_range=time_range)
                plan.dimensions[1] = DimensionSpec(Const(0), abi.Uint8)  # placeholder: the shape number
                plan.geo = GeoIntersection(shapes.buf.ptr, num_shapes, len(lats), "pt", 0, True, 1)
                packed = None
                def run():
                    nonlocal packed
                    q = NativeQuery(be, plan, names, streams=streams)
                    q.set_geo_column(on)
                    if packed is None:
                        packed = q.pack_batches(vps)
                    q.run_batches(packed)
                    return q
                compiles = -1
                for _ in range(4):  # priming passes: the shape's kernels are compiled in the background
                    run().release()
                    state = be.rtc_wait()
                    if state is None or state["compiles"] == compiles:
                        break
                    compiles = state["compiles"]
                times = []
                for _ in range(steps):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    run().release()
                    torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
                dt = float(np.median(times))
                be.profiler_enable(True)
                stats0 = be.geo_column_stats()
                q = run(); torch.cuda.synchronize()
                kernels = be.profiler_report(); be.profiler_enable(False)
                stats1 = be.geo_column_stats()
                n, calls = q.result_size, q.calls
                dims, valids, meas = q.fetch()
                q.release()
                values = meas.view(np.uint32 if count else np.float64)
                keyed = np.stack([dims[0].view(np.uint32), dims[1].astype(np.uint32), valids[0].astype(np.uint32), valids[1].astype(np.uint32)], axis=1)
                result = {tuple(k): v for k, v in zip(keyed.tolist(), values.tolist())}
                check = "first"
                if not on:
                    first = result
                elif result == first:
                    check = "ok"
                else:  # (HashReduce groups by a 32-bit hash: which of two colliding rows represents their group depends on the path)
                    differing = len(set(result.items()) ^ set(first.items()))
                    check = "%d (key, value) pairs differ; totals %s" % (differing, "equal" if sum(result.values()) == sum(first.values()) else "DIFFER")
                live, chunks = stats1["live"] - stats0["live"], stats1["chunks"] - stats0["chunks"]
                walk = {k: ms for k, (c, ms) in kernels.items() if k.startswith("geo_shape_column_kernel") or k.startswith("geo_intersect_kernel")}
                walk_ms = sum(walk.values())
                kernel_ms = sum(ms for c, ms in kernels.values())
                out.append({"config": "geoquery", "shapes": num_shapes, "polygon_points": len(lats),
                            "query": "COUNT(*) via Sort+Reduce" if count else "SUM(fare) via HashReduce", "geo_column": on, "rows": rows,
                            "batches": len(vps), "batch_rows": batch_rows, "groups": n, "abi_calls": calls, "check": check,
                            "live_rows": live, "wavefront_chunks": chunks, "lanes_filled": live / (64.0 * chunks) if chunks else None,
                            "walk_kernel_ms": walk_ms, "edge_tests_per_s_over_live_rows": live * (len(lats) - 1) / (walk_ms * 1e-3) if on and walk_ms else None,
                            "step_times_ms": [t * 1e3 for t in times], "ms_per_step": dt * 1e3, "kernel_ms_per_step": kernel_ms,
                            "kernels": {k: {"launches": c, "avg_ms": ms / c, "total_ms": ms} for k, (c, ms) in sorted(kernels.items(), key=lambda kv: -kv[1][1])}})
                print(json.dumps(out[-1]), flush=True)
        shapes.free()
    return out


def main():
    be = abi.load_hip_backend(); be.call("BootstrapDevice")
    dev = torch.device("cuda:0")
    which = sys.argv[1:] or ["c2", "c4", "hll", "geo"]
    res = []
    if "c2" in which: res += c2(be, dev, 100_000_000)
    if "c4" in which: res += c4(be, dev, 1 << 26, 200_000)
    if "c4spec" in which: res += c4_spec(be, dev, int(float(os.environ.get("C4_ROWS", "1e9"))), int(float(os.environ.get("C4_KEYS", "5e7"))),
                                         join_columns=os.environ.get("C4_JOIN_COLUMNS", "0") == "1")
    if "trips" in which: res += trips_leg(be, dev, int(float(os.environ.get("TRIPS_ROWS", "1e9"))))
    if "chains" in which:  # CHAINS_ROWS / CHAINS_BATCH_ROWS; CHAINS_QUERIES: a, b, c (comma separated)
        res += chains_leg(be, dev, int(float(os.environ.get("CHAINS_ROWS", str(1 << 28)))), batch_rows=int(float(os.environ.get("CHAINS_BATCH_ROWS", str(1 << 26)))))
    if "select" in which:  # SELECT_BATCH_ROWS / SELECT_LIMITS (comma separated, -1 = none): other batch sizes, fewer limits
        res += select_leg(be, dev, int(float(os.environ.get("SELECT_ROWS", str(1 << 28)))), batch_rows=int(float(os.environ.get("SELECT_BATCH_ROWS", str(1 << 26)))),
                          limits=tuple(int(x) for x in os.environ.get("SELECT_LIMITS", "100,1000000,-1").split(",")))
    if "selectjoin" in which:  # the same switches as "select"; SELECT_JOIN_KEYS: the table sizes, comma separated
        res += select_join_leg(be, dev, int(float(os.environ.get("SELECT_ROWS", str(1 << 28)))), batch_rows=int(float(os.environ.get("SELECT_BATCH_ROWS", str(1 << 26)))),
                               limits=tuple(int(x) for x in os.environ.get("SELECT_LIMITS", "100,1000000,-1").split(",")),
                               table_keys=tuple(int(float(x)) for x in os.environ.get("SELECT_JOIN_KEYS", "4000,5e7").split(",")))
    if "joinagg" in which:  # JOINAGG_ROWS / JOINAGG_BATCH_ROWS; JOINAGG_KEYS: the table sizes, comma separated
        res += join_agg_leg(be, dev, int(float(os.environ.get("JOINAGG_ROWS", str(1 << 28)))), batch_rows=int(float(os.environ.get("JOINAGG_BATCH_ROWS", str(1 << 26)))),
                            table_keys=tuple(int(float(x)) for x in os.environ.get("JOINAGG_KEYS", "4000,5e7").split(",")))
    if "tzagg" in which:  # TZAGG_ROWS / TZAGG_BATCH_ROWS
        res += tz_agg_leg(be, dev, int(float(os.environ.get("TZAGG_ROWS", str(1 << 28)))), batch_rows=int(float(os.environ.get("TZAGG_BATCH_ROWS", str(1 << 26)))))
    if "selectarchive" in which:  # the same switches as "select"
        res += select_archive_leg(be, dev, int(float(os.environ.get("SELECT_ROWS", str(1 << 28)))), batch_rows=int(float(os.environ.get("SELECT_BATCH_ROWS", str(1 << 26)))),
                                  limits=tuple(int(x) for x in os.environ.get("SELECT_LIMITS", "100,1000000,-1").split(",")))
    for leg in ("c3int64", "uuid"):
        if leg in which: res += wide_key_legs(be, dev, leg, int(float(os.environ.get("WIDE_ROWS", str(1 << 28)))))
    if "c3sortfloat" in which: res += sort_float_leg(be, dev, int(float(os.environ.get("SORT_FLOAT_ROWS", "1e9"))))
    for leg in ("c3sortavg", "tripsavg"):
        if leg in which: res += sort_avg_legs(be, dev, leg, int(float(os.environ.get("SORT_AVG_ROWS", "1e9"))))
    if "hll" in which:
        res += hll(be, dev, 1 << 25, 1000, 5_000_000) + hll(be, dev, 1 << 25, 4, 50_000_000) + hll(be, dev, 1 << 25, 100, 50_000_000, batches=4)
    if "geo" in which:  # GEO_COLUMN=1: AresQuerySetGeoColumn
        on = os.environ.get("GEO_COLUMN", "0") == "1"
        res += geo(be, dev, 1 << 24, 100, 20, geo_column=on) + geo(be, dev, 1 << 22, 250, 400, geo_column=on)
    if "geoquery" in which:  # GEOQUERY_ROWS / GEOQUERY_BATCH_ROWS
        res += geo_query_leg(be, dev, int(float(os.environ.get("GEOQUERY_ROWS", str(1 << 28)))), batch_rows=int(float(os.environ.get("GEOQUERY_BATCH_ROWS", str(1 << 26)))))
    for r in res: print(json.dumps(r), flush=True)
    os.makedirs("gpurun_out", exist_ok=True)
    json.dump(res, open("gpurun_out/bench_configs_%s.json" % "_".join(which), "w"), indent=1)
main()
