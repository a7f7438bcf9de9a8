"""A non-aggregation batch with joined columns three ways: a numpy model, the per-node ABI sequence (InitIndexVector, main-table
filters, a HashLookup per join over the survivors, foreign filters with the record-id vectors carried along, a transform per
dimension) and the fused extension AresFusedFilterJoinSelect.

The model's join is a dictionary from key bytes to record — what cases.build_cuckoo placed plus hand-placed entries — not a
probe.  A joined value follows the rule of the header (include/ares_extensions.h): a missing or null key, a record whose batch
lies outside the table and an index at or past NumRecordsInLastBatch in the last batch give (bits 0, null); a mode-0 batch
gives the default and its validity; a batch with a bitmap takes validity from it; any other batch is valid.  Expressions over
the gathered values go through select_model's model_filter / model_dim.

A join is (fact key column name, Table); a foreign filter is (join index, table column, functor, constant); a dimension is
select_model's (name, functor, constant, out type) with name = (join index, table column) for a joined one."""
import ctypes as C

import numpy as np

import cases
import harness as H
import select_model as M
from aresdb_amd import abi

KEY_BYTES = {abi.Uint32: 4, abi.Int32: 4, abi.Uint16: 2, abi.Uint8: 1, abi.Int64: 8, abi.UUID: 16}
BASE_BATCH = 3
SEEDS = [0x9747b28c, 0x1b873593, 0xe6546b64, 0x85ebca6b]


def key_bytes_of(col, n, key_bytes):
    """the probe's key of every row: the first key_bytes bytes of the widened value (raw bytes of Int64 / UUID)"""
    if col.dtype == abi.UUID:
        raw = col.values[:n]
    elif col.dtype == abi.Int64:
        raw = col.values[:n].view(np.uint8).reshape(n, 8)
    else:
        raw = M._bits(col, n).view(np.uint8).reshape(n, 4)
    return [bytes(r[:key_bytes]) for r in raw]


class Table:
    """A dimension table: three batches (a mode-2, a mode-1 and a mode-0 batch) of `per_batch` records, four columns, and the
    cuckoo index over `keys` (bytes).  Record of key i: batch BASE_BATCH + i % 3, index i // 3; NumRecordsInLastBatch is half
    of per_batch, so the upper half of the mode-0 batch's records are stale.  `extra`: hand-placed {key: record}."""

    COLUMNS = {"region": abi.Uint32, "tz": abi.Uint8, "rate": abi.Float32, "off": abi.Int16}
    TYPES = dict(COLUMNS, uid=abi.UUID)  # "uid": a wide column, for plans the fused path declines (not modelled)

    def __init__(self, rng, keys, key_bytes, num_buckets, num_hashes=4, default=True, extra=None):
        self.key_bytes, self.num_buckets, self.num_hashes = key_bytes, num_buckets, num_hashes
        self.per_batch = (len(keys) + 2) // 3 + 1
        self.num_last = self.per_batch // 2
        extra = extra or {}
        all_keys = list(keys) + list(extra)
        recs = [(BASE_BATCH + i % 3, i // 3) for i in range(len(keys))] + list(extra.values())
        self.table, self.placed = cases.build_cuckoo(all_keys, key_bytes, num_buckets, SEEDS[:num_hashes], rng, record_of=lambda i: recs[i])
        r = self.per_batch
        self.cols = {}
        for name, dtype in self.COLUMNS.items():
            def values():
                if dtype == abi.Float32:
                    return (rng.random(r) * 50).astype(np.float32)
                if dtype == abi.Int16:
                    return rng.integers(-500, 500, r)
                return rng.integers(0, 200, r)
            d = {abi.Uint32: 77, abi.Uint8: 9, abi.Float32: 2.5, abi.Int16: -4}[dtype] if default else None
            self.cols[name] = [M.Col(dtype, values(), rng.random(r) < 0.75, starting_index=3), M.Col(dtype, values()),
                               M.Col(dtype, None, default=d)]

        self.wide = {"uid": [M.Col(abi.UUID, rng.integers(0, 256, (r, 16), dtype=np.uint8), rng.random(r) < 0.75, starting_index=3),
                             M.Col(abi.UUID, rng.integers(0, 256, (r, 16), dtype=np.uint8)), M.Col(abi.UUID, None)]}

    @classmethod
    def forged(cls, ix, keys, per_batch):
        """A table over the bytes and geometry of a cuckoo_model.Index as given — forged signatures, duplicates, stale slots:
        `placed` is what cuckoo_model.probe answers for each of `keys` (their first key_bytes bytes), not what an inserter did.
        One Uint32 column "rec" in three mode-1 batches of per_batch records, all inside the table, whose value at
        (batch b, index i) is b << 16 | i: a joined value names its record."""
        import cuckoo_model
        t = cls.__new__(cls)
        t.key_bytes, t.num_buckets, t.num_hashes, t.seeds = ix.key_bytes, ix.num_buckets, ix.num_hashes, list(ix.seeds)
        t.per_batch = t.num_last = per_batch
        t.table = np.array(ix.table, np.uint8)
        t.placed = {}
        for k in keys:
            rec = cuckoo_model.probe(ix, k)
            if rec != (0, 0):
                t.placed[bytes(k[:ix.key_bytes])] = rec
        t.COLUMNS = t.TYPES = {"rec": abi.Uint32}
        t.cols = {"rec": [M.Col(abi.Uint32, ((BASE_BATCH + b) << 16) | np.arange(per_batch)) for b in range(3)]}
        t.wide = {}
        return t

    def stash_signatures(self):
        base = self.num_buckets * 8 * (9 + self.key_bytes)
        return self.table[base + 64: base + 68]

    def place_pair(self, k1, k2, bucket):
        """writes two keys of one bucket and one signature byte into slots 0 and 1 of that bucket (whatever lay there leaves
        the index): the probe of k2 meets k1's signature first"""
        bb = 8 * (9 + self.key_bytes)
        base = bucket * bb
        for j, (k, rec) in enumerate([(k1, (BASE_BATCH, 0)), (k2, (BASE_BATCH + 1, 1))]):
            old = bytes(self.table[base + 72 + j * self.key_bytes: base + 72 + (j + 1) * self.key_bytes])
            if self.table[base + 64 + j]:
                self.placed.pop(old, None)
            self.table[base + 8 * j: base + 8 * j + 8] = np.array(rec, np.uint32).view(np.uint8)
            self.table[base + 64 + j] = max(1, cases._murmur3_32(k1, SEEDS[0]) >> 24)
            self.table[base + 72 + j * self.key_bytes: base + 72 + (j + 1) * self.key_bytes] = np.frombuffer(k, np.uint8)
            self.placed[k] = rec

    def joined(self, keys, key_valid, name):
        """the joined column `name` for the fact rows' keys as a select_model.Col (values, validity)"""
        dtype = self.COLUMNS[name]
        n = len(keys)
        bits, ok = np.zeros(n, np.uint32), np.zeros(n, bool)
        for i, (k, kv) in enumerate(zip(keys, key_valid)):
            rec = self.placed.get(k) if kv else None
            if rec is None or rec[0] == 0:
                continue
            rel, idx = rec[0] - BASE_BATCH, rec[1]
            if not (rel < 2 or idx < self.num_last):
                continue
            b = self.cols[name][rel]
            if b.values is None:
                if b.default is not None:
                    bits[i], ok[i] = M._bits(M.Col(dtype, [b.default]), 1)[0], True
                continue
            bits[i] = M._bits(b, len(b.values))[idx]
            ok[i] = True if b.valid is None else bool(b.valid[idx])
        values = bits.view(np.float32) if dtype == abi.Float32 else bits.view(np.int32).astype(M._NP[dtype]) \
            if M._KIND[dtype] == "i" else bits.astype(M._NP[dtype])
        return M.Col(dtype, values, ok)

    def upload(self, be):
        return DeviceTable(be, self)


class DeviceTable:
    def __init__(self, be, t):
        self.t = t
        self.index = H.Buf(be, t.table)
        self.batches = {name: [c.upload(be) for c in cols] for name, cols in {**t.cols, **t.wide}.items()}
        self.slices = {name: (abi.VectorPartySlice * 3)(*[c.vp for c in cols]) for name, cols in self.batches.items()}

    def index_struct(self):
        hi = abi.CuckooHashIndex()
        hi.buckets = self.index.ptr
        for i, s in enumerate(getattr(self.t, "seeds", SEEDS)):
            hi.seeds[i] = s
        hi.keyBytes, hi.numHashes, hi.numBuckets = self.t.key_bytes, self.t.num_hashes, self.t.num_buckets
        return hi

    def input(self, name, rids=None, timezone=None):
        iv = abi.InputVector()
        f = iv.Vector.ForeignVP
        f.RecordIDs, f.Batches = rids, C.addressof(self.slices[name])
        f.BaseBatchID, f.NumBatches, f.NumRecordsInLastBatch = BASE_BATCH, 3, self.t.num_last
        f.TimezoneLookup, f.TimezoneLookupSize = timezone, 0
        f.DataType = self.t.TYPES[name]
        f.DefaultValue = self.batches[name][2].vp.DefaultValue
        iv.Type = abi.ForeignColumnInput
        return iv

    def free(self):
        self.index.free()
        for cols in self.batches.values():
            for c in cols:
                c.free()


# ---- the fixture --------------------------------------------------------------------------------------------------------
def _random_keys(rng, dtype, count):
    kb = KEY_BYTES[dtype]
    if dtype == abi.UUID or dtype == abi.Int64:
        return [bytes(rng.integers(0, 256, kb, dtype=np.uint8)) for _ in range(count)]
    lo, hi = {abi.Uint32: (0, 1 << 31), abi.Int32: (-(10 ** 6), 0), abi.Uint16: (0, 1 << 16), abi.Uint8: (0, 256)}[dtype]
    raw = rng.choice(hi - lo, size=min(count, (hi - lo) // 2), replace=False) + lo
    return [int(v).to_bytes(4, "little", signed=True)[:kb] for v in raw]


def _colliding_pair(rng, dtype, num_buckets, taken):
    """two fresh keys with one bucket and one signature byte under the first seed (cases._murmur3_32)"""
    seen = {}
    for _ in range(400):
        for k in _random_keys(rng, dtype, 64):
            if k in taken:
                continue
            hv = cases._murmur3_32(k, SEEDS[0])
            at = (hv % num_buckets, max(1, hv >> 24))
            if at in seen and seen[at] != k:
                return seen[at], k, at[0]
            seen[at] = k
    raise AssertionError("no two keys share bucket and signature byte")


def _key_column(rng, dtype, keys, n, misses=0.15, nulls=0.10):
    """a fact column of n rows over `keys`: about 15 % keys the table does not hold, about 10 % null"""
    kb = KEY_BYTES[dtype]
    pick = [keys[i] for i in rng.integers(0, len(keys), n)]
    other = _random_keys(np.random.default_rng(99), dtype, max(n // 4, 8))
    for i in np.flatnonzero(rng.random(n) < misses):
        pick[i] = other[i % len(other)]
    valid = rng.random(n) >= nulls
    raw = np.frombuffer(b"".join(pick), np.uint8).reshape(n, kb)
    if dtype == abi.UUID:
        return M.Col(dtype, raw, valid, starting_index=2)
    if dtype == abi.Int64:
        return M.Col(dtype, raw.copy().view(np.int64).reshape(n), valid, starting_index=2)
    wide = np.zeros((n, 4), np.uint8)
    wide[:, :kb] = raw
    v = wide.view(np.uint32).reshape(n)
    if dtype == abi.Int32:
        v = v.view(np.int32)
    return M.Col(dtype, v.astype(M._NP[dtype]), valid, starting_index=2)


def fixture(n, key_dtype=abi.Uint32, nkeys=300, num_buckets=None, num_hashes=4, default=True, seed=11, pair=True, misses=0.15):
    """(Table, fact key column of n rows).  About 300 keys in so few buckets that the stash holds some; one pair of keys
    shares bucket and signature byte; a hand-placed record lies in a batch outside the table."""
    rng = np.random.default_rng(seed)
    if key_dtype == abi.Uint8:
        nkeys = min(nkeys, 100)
    if num_buckets is None:
        num_buckets = max(1, nkeys // 8)
    keys = _random_keys(rng, key_dtype, nkeys)
    outside = _random_keys(np.random.default_rng(seed + 1000), key_dtype, 40)
    outside = [k for k in outside if k not in keys][0]
    t = Table(rng, keys, KEY_BYTES[key_dtype], num_buckets, num_hashes, default, extra={outside: (BASE_BATCH + 7, 10 ** 6)})
    used = list(keys) + [outside]
    if pair and num_buckets > 1 and num_hashes > 0:
        k1, k2, bucket = _colliding_pair(rng, key_dtype, num_buckets, set(used))
        t.place_pair(k1, k2, bucket)
        used += [k1, k2]
    t.key_dtype, t.used = key_dtype, used
    return t, _key_column(rng, key_dtype, used, n, misses=misses)


def key_column(t, n, seed):
    """another batch's key column over the fixture's table"""
    return _key_column(np.random.default_rng(seed), t.key_dtype, t.used, n)


# ---- the model ----------------------------------------------------------------------------------------------------------
def _resolve(cols, joins, name, n):
    if isinstance(name, str):
        return cols[name]
    k, column = name
    key_col, table = joins[k]
    key = cols[key_col]
    return table.joined(key_bytes_of(key, n, table.key_bytes), M._valid(key, n), column)


def model_join_select(cols, filters, joins, ffilters, dims, n, limit=-1):
    keep = np.ones(n, bool)
    for name, functor, c in filters:
        keep &= M.model_filter(cols[name], functor, c, n)
    for k, column, functor, c in ffilters:
        keep &= M.model_filter(_resolve(cols, joins, (k, column), n), functor, c, n)
    rows = np.flatnonzero(keep)
    if limit >= 0:
        rows = rows[:limit]
    out = []
    for name, functor, c, out_type in dims:
        v, ok = M.model_dim(_resolve(cols, joins, name, n), functor, c, out_type, n)
        out.append((v[rows], ok[rows]))
    return rows, out


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def per_node(be, dcols, dtables, filters, joins, ffilters, dims, n):
    """the per-node sequence over uploaded columns and tables (dtables[k]: DeviceTable of join k); (count, DimVector)"""
    capacity = max(n, 1)
    vec = H.DimVector(be, capacity, M.ndw_of(dims), with_hash=False, with_index=False)
    idx, pred = H.Buf(be, nbytes=4 * capacity), H.Buf(be, nbytes=capacity)
    rids = [H.Buf(be, nbytes=8 * capacity) for _ in joins]
    count = n
    be.call("InitIndexVector", idx.ptr, 0, n, None, 0)
    for name, functor, c in filters:
        count = be.call("BinaryFilter", dcols[name].input(), M._const_input(c), idx.ptr, pred.ptr, count, None, 0, None, 0,
                        functor, None, 0)
    for (key_col, _), dt, r in zip(joins, dtables, rids):
        if count > 0:
            be.call("HashLookup", dcols[key_col].input(), r.ptr, idx.ptr, count, None, 0, dt.index_struct(), None, 0)
    vecs = (C.c_void_p * max(len(rids), 1))(*[r.ptr for r in rids])
    for k, column, functor, c in ffilters:
        count = be.call("BinaryFilter", dtables[k].input(column, rids[k].ptr), M._const_input(c), idx.ptr, pred.ptr, count, vecs,
                        len(rids), None, 0, functor, None, 0)
    for (name, functor, c, out_type), (vo, no, _) in zip(dims, vec.dim_offsets()):
        out = H.dimension_output(vec.values.ptr + vo, vec.values.ptr + no, out_type)
        lhs = dcols[name].input() if isinstance(name, str) else dtables[name[0]].input(name[1], rids[name[0]].ptr)
        if functor is None:
            be.call("UnaryTransform", lhs, out, idx.ptr, count, None, 0, abi.Noop, None, 0)
        else:
            be.call("BinaryTransform", lhs, M._const_input(c), out, idx.ptr, count, None, 0, functor, None, 0)
    be.wait()
    for b in [idx, pred] + rids:
        b.free()
    return count, vec


def fused_query(dcols, dtables, filters, joins, ffilters, dims, num_joins=None):
    q = abi.FusedJoinSelect()
    q.numFilters, q.numDims, q.numForeignFilters = len(filters), len(dims), len(ffilters)
    q.numJoins = len(joins) if num_joins is None else num_joins
    for k, (name, functor, c) in enumerate(filters[:4]):
        q.filters[k].lhs, q.filters[k].rhs = dcols[name].input(), M._const_input(c)
        q.filters[k].arity, q.filters[k].functor, q.filters[k].outType = 2, functor, abi.Bool
    for k, ((key_col, _), dt) in enumerate(list(zip(joins, dtables))[:2]):
        q.joins[k].key, q.joins[k].index = dcols[key_col].input(), dt.index_struct()
    for k, (j, column, functor, c) in enumerate(ffilters[:4]):
        e = q.foreignFilters[k]
        e.lhs, e.rhs = dtables[min(max(j, 0), len(dtables) - 1)].input(column), M._const_input(c)
        e.arity, e.functor, e.outType = 2, functor, abi.Bool
        q.foreignFilterJoin[k] = j
    for d, (name, functor, c, out_type) in enumerate(dims[:8]):
        e = q.dims[d]
        if isinstance(name, str):
            e.lhs, q.dimJoin[d] = dcols[name].input(), -1
        else:
            e.lhs, q.dimJoin[d] = dtables[min(max(name[0], 0), len(dtables) - 1)].input(name[1]), name[0]
        e.arity, e.functor, e.outType = (1, abi.Noop, out_type) if functor is None else (2, functor, out_type)
        if functor is not None:
            e.rhs = M._const_input(c)
    return q


def fused(be, q, dims, n, limit, capacity, stream=None):
    """AresFusedFilterJoinSelect into a sentinel-filled vector; (res, DimVector)."""
    row_bytes = sum(abi.DATA_TYPE_BYTES[d[3]] for d in dims) + len(dims)
    vec = H.DimVector(be, capacity, M.ndw_of(dims), with_hash=False, with_index=False,
                      init=np.full(row_bytes * capacity, M.SENTINEL, np.uint8))
    try:
        res = be.fused_filter_join_select(q, n, limit, vec.struct(), stream)
    except Exception:
        vec.free()
        raise
    return res, vec
