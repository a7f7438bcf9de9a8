"""Inputs for the cuckoo probe at chosen hashes: forged and honest tables with the keys to probe them with.

A set is a cuckoo_model.Index, a key column (DataType, values, validity, layout) and the set's family; every builder asserts
the property it exists for on the model before it returns (`_is`: the place the model finds the key at, `assert` on hashes and
slots).  Tables stay under 8 MB and probes under 5000 rows.  Records are (batch 3..5, index < 512): inside the dimension table the
fused entry points join against, so a joined value names its record.

Families and the key widths (keyBytes) they run at:
  clamp      1 2 4 8 16  keys whose hash has a zero top byte (signature 1); width 1 has 256 keys, so its table has one bucket and
                         the seed is searched until a second such key and a neighbour of true signature 1 exist
  zero       1 2 4 8 16  the all-zero key under a seed that gives it a zero top byte, present and absent
  stale      1 2 4 8 16  slots with signature 0, the probed key's bytes and a record, in a bucket and in the stash
  full       1 2 4 8 16  a bucket whose eight signatures are the probed key's, the key in slot 7
  byte       1 2 3 4 5 8 13 16  decoys under a forged signature that differ in one byte: the last, the first, word 1, word 3, the
                         last byte of an odd tail (3: a Uint32 column, 5: Int64, 13: UUID)
  order      1 2 4 8 16  duplicates: hash order, slot order, bucket before stash, stash order; hash 3 only; stash slot 3 only
  hashes     1 2 4 8 16  numHashes 0..4 with garbage in the unused seeds
  buckets    1 2 4 8 16  hashes at the edges of hv % d for d in 1, 2, 3, 641 (and 65535, 65536, 65537 at width 4: wider keys
                         would pass 8 MB).  A 1- or 2-byte key cannot be inverted to a hash; its hash is chosen through the
                         seed, one key per seed: d = 3 and 641 only, four hashes per table
  widths     1..5 8 13 16  keyBytes below the column's width, negative Int8 / Int16 keys, Int64 and UUID prefixes
  rows       4           null keys, modes 0 / 1 / 2, a constant key, a subset index vector, 1 / 63 / 64 / 65 / 257 rows
  honest     1 2 4 8 16  tables of the model's own inserter, with evictions and a used stash; nulls and misses among 257 rows
"""
import numpy as np

import cuckoo_model as cm
from aresdb_amd import abi

BASE_BATCH, NUM_BATCHES, PER_BATCH = 3, 3, 512
SEEDS = [0x9747b28c, 0x1b873593, 0xe6546b64, 0x85ebca6b]
GARBAGE = [0xdeadbeef, 0x0badf00d, 0x12345678, 0xffffffff]
DTYPE_OF_WIDTH = {1: abi.Uint8, 2: abi.Uint16, 4: abi.Uint32, 8: abi.Int64, 16: abi.UUID}
WIDTHS = (1, 2, 4, 8, 16)
_STORED = {abi.Int8: 1, abi.Uint8: 1, abi.Int16: 2, abi.Uint16: 2, abi.Int32: 4, abi.Uint32: 4, abi.Int64: 8, abi.UUID: 16}
_SIGNED = (abi.Int8, abi.Int16, abi.Int32, abi.Int64)
MAX_TABLE_BYTES, MAX_ROWS = 8 << 20, 5000


def value_of(dtype, key, above=b""):
    """the column value whose widened bytes start with `key`, then `above`, then zeros"""
    raw = (bytes(key) + bytes(above)).ljust(_STORED[dtype], b"\0")[:_STORED[dtype]]
    return raw if dtype == abi.UUID else int.from_bytes(raw, "little", signed=dtype in _SIGNED)


class ProbeSet:
    """layout: "mode2" (validity bitmap at StartingIndex `starting_index`), "mode1", "mode0" (every row is `default`, None: no
    default) or "const" (every row is the ConstInt `default`); `values` / `valid` are the rows' effective keys either way.
    index_vector: the rows that are looked up, in order (None: all).  Only mode 1 / 2 columns without an index vector can go
    through the fused entry points (`fusable`)."""

    def __init__(self, name, family, ix, dtype, values, valid=None, layout="mode2", starting_index=3, default=None, index_vector=None):
        self.name, self.family, self.ix, self.dtype, self.layout = name, family, ix, dtype, layout
        self.values, self.n = list(values), len(values)
        self.valid = np.ones(self.n, bool) if valid is None else np.asarray(valid, bool)
        self.starting_index, self.default = starting_index, default
        self.index_vector = None if index_vector is None else np.asarray(index_vector, np.uint32)
        assert ix.table.nbytes <= MAX_TABLE_BYTES and 0 < self.n <= MAX_ROWS and len(self.valid) == self.n
        assert ix.key_bytes <= len(cm.widened(dtype, self.values[0]))  # (a wider key reads past the value: undefined)
        self.fusable = layout in ("mode1", "mode2") and index_vector is None

    def __repr__(self):
        return self.name

    def widened(self):
        return [cm.widened(self.dtype, v) for v in self.values]

    def records(self, probe=cm.probe):
        """the record of every row (a null key: (0, 0)) under `probe`, (n, 2) uint32"""
        memo, out = {}, np.zeros((self.n, 2), np.uint32)
        for i, (k, ok) in enumerate(zip(self.widened(), self.valid)):
            if ok:
                if k not in memo:
                    memo[k] = probe(self.ix, k)
                out[i] = memo[k]
        return out

    def expected(self, probe=cm.probe):
        """what HashLookup writes: the records of the looked-up rows, flat uint32"""
        r = self.records(probe)
        return (r if self.index_vector is None else r[self.index_vector]).reshape(-1)

    def column_values(self):
        if self.dtype == abi.UUID:
            return np.frombuffer(b"".join(self.values), np.uint8).reshape(self.n, 16)
        return np.array(self.values, np.int64 if self.dtype in _SIGNED else np.uint64)


class _Builder:
    def __init__(self, name, family, kb, dtype=None, num_buckets=5, num_hashes=4, seeds=SEEDS, rng_seed=1):
        self.name, self.family, self.kb = name, family, kb
        self.dtype = DTYPE_OF_WIDTH[kb] if dtype is None else dtype
        self.ix = cm.Index(kb, num_buckets, num_hashes, seeds)
        self.rng = np.random.default_rng([rng_seed, kb, num_buckets])
        self.used, self.values, self.valid, self.records_given = set(), [], [], 0

    def rec(self):
        i = self.records_given
        self.records_given += 1
        assert i < NUM_BATCHES * PER_BATCH
        return (BASE_BATCH + i % NUM_BATCHES, i // NUM_BATCHES)

    def fresh(self, pred=lambda k: True):
        """a key no other of this set's keys equals, with pred(key)"""
        if self.kb <= 2:
            k = cm.find_key(pred, self.kb, start=int(self.rng.integers(0, 1 << (8 * self.kb))), exclude=self.used)
        else:
            for _ in range(1 << 16):
                k = bytes(self.rng.integers(1, 256, self.kb, dtype=np.uint8))
                if k not in self.used and pred(k):
                    break
            else:
                raise LookupError(f"{self.name}: no key with the wanted property")
        self.used.add(k)
        return k

    def at(self, h, top, bucket=None):
        """a fresh key whose hash under seed h has top byte `top` and, if given, names `bucket`"""
        ix = self.ix
        if self.kb in (4, 8, 16):
            for _ in range(1 << 20):
                t = (top << 24) | int(self.rng.integers(0, 1 << 24))
                if bucket is not None:
                    t += (bucket - t) % ix.num_buckets
                if t >> 24 != top:
                    continue
                k = cm.key_with_hash(t, ix.seeds[h], self.kb, bytes(self.rng.integers(1, 256, self.kb - 4, dtype=np.uint8)))
                if k not in self.used:
                    assert ix.hash(k, h) == t
                    self.used.add(k)
                    return k
        return self.fresh(lambda k: ix.hash(k, h) >> 24 == top and (bucket is None or ix.bucket_of(k, h) == bucket))

    def ask(self, key, above=b"", valid=True):
        self.values.append(value_of(self.dtype, key, above))
        self.valid.append(valid)

    def _is(self, key, place, record=None):
        """the model finds `key` at `place` ((hash index or STASH, slot), None: nowhere) with `record`"""
        got = cm.trace(self.ix, key)
        assert got[1] == place and (record is None or got[0] == tuple(record)), (self.name, key.hex(), got, place, record)

    def done(self, **kw):
        self.ask(next(iter(sorted(self.used))), valid=False)  # every set ends in a null row over one of its keys
        return ProbeSet(self.name, self.family, self.ix, self.dtype, self.values, self.valid, **kw)


# ---- clamp ----------------------------------------------------------------------------------------------------------------
def _clamp_keys(b):
    ix = b.ix
    a = b.at(0, 0)
    home = ix.bucket_of(a, 0)
    n = b.at(0, 1, home)
    z = b.at(0, 0)
    return a, n, z, home


def clamp(kb):
    """A (top byte 0 under seed 0, stored with signature 1 in slot 3), N (true signature 1, slot 1 of the same bucket: A's
    probe compares N's key first) and Z (top byte 0, absent, its bucket has empty slots)"""
    seeds = list(SEEDS)
    for attempt in range(4096):
        b = _Builder(f"clamp-{kb}", "clamp", kb, num_buckets=1 if kb == 1 else 3, seeds=seeds)
        try:
            a, n, z, home = _clamp_keys(b)
            break
        except LookupError:  # (widths 1 and 2: not under this seed — choose the hash of one key through the seed)
            seeds[0] = cm.seed_with_hash((attempt * 2654435761) & 0xFFFFFF, bytes([attempt % 251 + 1] * kb))
    else:
        raise LookupError(f"clamp-{kb}: no seed with the three keys")
    ix = b.ix
    ra, rn = b.rec(), b.rec()
    ix.put(home, 3, a, ra, hash_index=0)
    ix.put(home, 1, n, rn, hash_index=0)
    assert ix.hash(a, 0) >> 24 == 0 and ix.hash(z, 0) >> 24 == 0 and ix.hash(n, 0) >> 24 == 1
    assert ix.slot(home, 3)[0] == 1 and ix.slot(home, 1)[0] == 1 and ix.free_slots(ix.bucket_of(z, 0))
    b._is(a, (0, 3), ra)
    b._is(n, (0, 1), rn)
    b._is(z, None)
    for k in (a, n, z, a):
        b.ask(k)
    return b.done()


def zero_key(kb, present):
    """the all-zero key under a seed that gives it top byte 0"""
    zero = bytes(kb)
    seed0 = cm.seed_with_hash(0x00C0FFEE + kb, zero)
    b = _Builder(f"zero-{kb}-{'present' if present else 'absent'}", "clamp", kb, seeds=[seed0] + SEEDS[1:])
    ix = b.ix
    b.used.add(zero)
    assert ix.hash(zero, 0) == 0x00C0FFEE + kb
    home = ix.bucket_of(zero, 0)
    other = b.fresh(lambda k: ix.bucket_of(k, 0) == home)
    ro, rz = b.rec(), b.rec()
    ix.put(home, 0, other, ro, hash_index=0)
    if present:
        ix.put(home, 2, zero, rz, hash_index=0)
        assert ix.slot(home, 2)[0] == 1
    b._is(zero, (0, 2) if present else None)
    b._is(other, (0, 0), ro)
    assert ix.free_slots(home)  # (empty slots: signature 0 and all-zero key bytes, which the clamp keeps apart from the key)
    b.ask(zero)
    b.ask(other)
    return b.done()


# ---- stale ----------------------------------------------------------------------------------------------------------------
def stale(kb):
    """signature 0 over the probed key's bytes and a record: S1 only so (bucket): misses; S2 so in slot 1 and properly in slot 5;
    S3 so in slot 2 and properly under hash 1; T1 only so in the stash: misses; T2 so in stash slot 1 and properly in slot 2;
    T3 in stash slot 5, which no probe reads"""
    b = _Builder(f"stale-{kb}", "stale", kb)
    ix = b.ix
    s1, s2, s3, t1, t2, t3 = (b.fresh() for _ in range(6))
    ix.put(ix.bucket_of(s1, 0), 0, s1, b.rec(), signature=0)
    ix.put(ix.bucket_of(s2, 0), 1, s2, b.rec(), signature=0)
    r2 = b.rec()
    ix.place(s2, r2, 0, 5)
    ix.put(ix.bucket_of(s3, 0), 2, s3, b.rec(), signature=0)
    r3 = b.rec()
    ix.place(s3, r3, 1, 3)
    ix.put(cm.STASH, 0, t1, b.rec(), signature=0)
    ix.put(cm.STASH, 1, t2, b.rec(), signature=0)
    rt = b.rec()
    ix.put(cm.STASH, 2, t2, rt)
    ix.put(cm.STASH, 5, t3, b.rec(), signature=1)
    for k, slot in ((s1, 0), (s2, 1), (s3, 2)):
        sig, key, rec = ix.slot(ix.bucket_of(k, 0), slot)
        assert sig == 0 and key == k and rec != (0, 0)
    assert ix.slot(cm.STASH, 0)[0] == 0 and ix.slot(cm.STASH, 0)[2] != (0, 0)
    b._is(s1, None)
    b._is(s2, (0, 5), r2)
    assert cm.trace(ix, s3)[0] == r3 and cm.trace(ix, s3)[1][1] == 3
    b._is(t1, None)
    b._is(t2, (cm.STASH, 2), rt)
    b._is(t3, None)
    for k in (s1, s2, s3, t1, t2, t3):
        b.ask(k)
    return b.done()


# ---- decoys ---------------------------------------------------------------------------------------------------------------
def full_bucket(kb):
    """slots 0..6: other keys under the probed key's signature; slot 7: the key"""
    b = _Builder(f"full-{kb}", "decoys", kb)
    ix = b.ix
    k = b.fresh()
    home, sig = ix.bucket_of(k, 0), ix.signature_of(k, 0)
    others = [b.fresh() for _ in range(7)]
    for j, d in enumerate(others):
        ix.put(home, j, d, b.rec(), signature=sig)
    rk = b.rec()
    ix.put(home, 7, k, rk, hash_index=0)
    assert all(ix.slot(home, j)[0] == sig for j in range(8)) and all(ix.slot(home, j)[1] != k for j in range(7))
    b._is(k, (0, 7), rk)
    for key in [k] + others:  # (the decoys themselves: the model decides — found only if their own hash names this slot)
        b.ask(key)
    return b.done()


BYTE_CONFIGS = [(abi.Uint8, 1), (abi.Uint16, 2), (abi.Uint32, 3), (abi.Uint32, 4), (abi.Int64, 5), (abi.Int64, 8), (abi.UUID, 13),
                (abi.UUID, 16)]


def one_byte(dtype, kb):
    """per byte position (the last, the first, the first of word 1 and of word 3): the key in slot 4 of its bucket, and in slot 1
    a decoy under the key's signature that differs from it in that byte alone"""
    b = _Builder(f"byte-{kb}", "decoys", kb, dtype=dtype, num_buckets=11)
    ix = b.ix
    homes = set()
    above = bytes(b.rng.integers(1, 256, _STORED[dtype] - kb, dtype=np.uint8))
    for pos in sorted({kb - 1, 0} | ({4} if kb >= 8 else set()) | ({12} if kb >= 13 else set())):
        k = b.fresh(lambda key: ix.bucket_of(key, 0) not in homes)
        home = ix.bucket_of(k, 0)
        homes.add(home)
        d = bytearray(k)
        d[pos] ^= 0x81
        d = bytes(d)
        assert d not in b.used and [i for i in range(kb) if d[i] != k[i]] == [pos]
        b.used.add(d)
        rd, rk = b.rec(), b.rec()
        ix.put(home, 1, d, rd, signature=ix.signature_of(k, 0))
        ix.put(home, 4, k, rk, hash_index=0)
        b._is(k, (0, 4), rk)
        b.ask(k, above)
        b.ask(d, above)
    return b.done()


# ---- order ----------------------------------------------------------------------------------------------------------------
def order(kb):
    b = _Builder(f"order-{kb}", "order", kb, num_buckets=7)
    ix = b.ix
    o1 = b.fresh(lambda k: ix.bucket_of(k, 0) != ix.bucket_of(k, 1))
    o2, o3, o4, o6 = (b.fresh() for _ in range(4))
    o5 = b.fresh(lambda k: ix.bucket_of(k, 3) not in [ix.bucket_of(k, h) for h in range(3)])
    r = [b.rec() for _ in range(10)]
    ix.place(o1, r[0], 1, 2)
    ix.place(o1, r[1], 0, 6)
    ix.place(o2, r[2], 0, 1)
    ix.place(o2, r[3], 0, 5)
    ix.place(o3, r[4], 0, 3)
    ix.put(cm.STASH, 0, o3, r[5])
    ix.put(cm.STASH, 1, o4, r[6])
    ix.put(cm.STASH, 2, o4, r[7])
    ix.place(o5, r[8], 3, 0)
    ix.put(cm.STASH, 3, o6, r[9])
    b._is(o1, (0, 6), r[1])
    b._is(o2, (0, 1), r[2])
    b._is(o3, (0, 3), r[4])
    b._is(o4, (cm.STASH, 1), r[6])
    b._is(o5, (3, 0), r[8])
    b._is(o6, (cm.STASH, 3), r[9])
    for k in (o1, o2, o3, o4, o5, o6):
        b.ask(k)
    return b.done()


# ---- hash count -----------------------------------------------------------------------------------------------------------
def hash_count(kb, nh):
    """numHashes = nh, garbage seeds behind: `beyond` lies only where hash index nh points (misses), `last` only where index
    nh - 1 points (hits), `stashed` in the stash (with nh = 0 the only place that answers)"""
    b = _Builder(f"hashes-{kb}-{nh}", "hash count", kb, num_buckets=7, num_hashes=nh, seeds=SEEDS[:nh] + GARBAGE[nh:])
    ix = b.ix
    if nh < 4:
        def elsewhere(k):  # no hash in use names the slot's bucket with the slot's signature
            return all((ix.bucket_of(k, h), ix.signature_of(k, h)) != (ix.bucket_of(k, nh), ix.signature_of(k, nh)) for h in range(nh))
        beyond = b.fresh(elsewhere)
        ix.place(beyond, b.rec(), nh, 0)
        b._is(beyond, None)
        assert cm.trace(ix, beyond, all_four=True)[1] == (nh, 0)
        b.ask(beyond)
    if nh > 0:
        last = b.fresh(lambda k: ix.bucket_of(k, nh - 1) not in [ix.bucket_of(k, h) for h in range(nh - 1)])
        rl = b.rec()
        ix.place(last, rl, nh - 1, 4)
        b._is(last, (nh - 1, 4), rl)
        b.ask(last)
    stashed = b.fresh()
    rs = b.rec()
    ix.put(cm.STASH, 2, stashed, rs)
    b._is(stashed, (cm.STASH, 2), rs)
    b.ask(stashed)
    b.ask(b.fresh())  # absent
    return b.done()


# ---- buckets --------------------------------------------------------------------------------------------------------------
DIVISORS = (1, 2, 3, 641, 65535, 65536, 65537)
assert (1 << 32) - 641 * ((1 << 32) // 641) == 640  # 641: floor(2^32 / d) errs most


def bucket_hashes(d):
    q = 0xFFFFFFFF // d
    return sorted({0, d - 1, d, d + 1, q * d - 1, q * d, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF})


def buckets(kb, d):
    """keys inverted to the hashes at the edges of hv % d under seed 0, each stored in the bucket exact % names and nowhere else"""
    b = _Builder(f"buckets-{kb}-{d}", "buckets", kb, num_buckets=d)
    ix = b.ix
    for t in bucket_hashes(d):
        k = cm.key_with_hash(t, ix.seeds[0], kb, bytes(b.rng.integers(1, 256, kb - 4, dtype=np.uint8)))
        assert k not in b.used and ix.hash(k, 0) == t
        b.used.add(k)
        home = t % d
        r = b.rec()
        slot = ix.free_slots(home)[0]
        ix.put(home, slot, k, r, hash_index=0)
        assert d > 1 or home == 0
        b._is(k, (0, slot), r)
        b.ask(k)
    return b.done()


def buckets_by_seed(kb, d, part):
    """widths 1 and 2: key i is given its hash through seed i and stored in the bucket exact % names for hash i, nowhere else"""
    hashes = bucket_hashes(d)
    targets = (hashes[:4], hashes[4:8], hashes[-4:])[part]
    keys = [bytes([17 * i + 3 + part] * kb) for i in range(4)]
    b = _Builder(f"buckets-{kb}-{d}-{'abc'[part]}", "buckets", kb, num_buckets=d, seeds=[cm.seed_with_hash(t, k) for t, k in zip(targets, keys)])
    ix = b.ix
    for i, (t, k) in enumerate(zip(targets, keys)):
        assert ix.hash(k, i) == t
        b.used.add(k)
        r = b.rec()
        ix.put(t % d, i, k, r, hash_index=i)
        assert cm.probe(ix, k) == r and cm.trace(ix, k)[1][1] == i
        b.ask(k)
    return b.done()


# ---- widths ---------------------------------------------------------------------------------------------------------------
def prefix(dtype, kb):
    """keyBytes below the column's width: values that agree in the first kb bytes and differ above resolve to one record"""
    b = _Builder(f"prefix-{kb}-of-{_STORED[dtype]}", "widths", kb, dtype=dtype)
    ix = b.ix
    spare = _STORED[dtype] - kb
    k1, k2, absent = b.fresh(), b.fresh(), b.fresh()
    r1, r2 = b.rec(), b.rec()
    s1 = ix.free_slots(ix.bucket_of(k1, 0))[0]
    ix.place(k1, r1, 0, s1)
    ix.put(cm.STASH, 1, k2, r2)
    b._is(k1, (0, s1), r1)
    b._is(k2, (cm.STASH, 1), r2)
    b._is(absent, None)
    for above in (bytes(spare), b"\xff" * spare, bytes(b.rng.integers(1, 256, spare, dtype=np.uint8)), b"\x80" + bytes(spare - 1)):
        for k in (k1, k2, absent):
            b.ask(k, above)
            assert cm.widened(dtype, b.values[-1])[:kb] == k and cm.widened(dtype, b.values[-1])[kb:kb + spare] == above
    return b.done()


def signed_keys(dtype, kb):
    """negative Int8 / Int16 keys.  keyBytes 4: the sign-extended bytes are stored, and for one value the zero-extended bytes too,
    under another record — the probe finds the former; keyBytes 1 / 2: the stored width"""
    b = _Builder(f"signed-{_STORED[dtype]}-as-{kb}", "widths", kb, dtype=dtype)
    ix = b.ix
    bits = 8 * _STORED[dtype]
    values = [-(1 << (bits - 1)), -1, -37, 5, (1 << (bits - 1)) - 1]
    for v in values:
        k = cm.widened(dtype, v)[:kb]
        assert kb < 4 or (k[3] == 0xFF) == (v < 0)
        b.used.add(k)
        r = b.rec()
        ix.place(k, r, 1, ix.free_slots(ix.bucket_of(k, 1))[0])
        assert cm.probe(ix, cm.widened(dtype, v)) == r
        b.values.append(v)
        b.valid.append(True)
    if kb == 4:
        zero_extended = (values[0] & ((1 << bits) - 1)).to_bytes(4, "little")
        ix.place(zero_extended, b.rec(), 0, ix.free_slots(ix.bucket_of(zero_extended, 0))[0])
        assert cm.trace(ix, zero_extended)[1] is not None and cm.trace(ix, cm.widened(dtype, values[0]))[1][0] == 1
    b.values.append(-2)  # absent
    b.valid.append(True)
    assert cm.probe(ix, cm.widened(dtype, -2)) == (0, 0)
    return b.done()


# ---- rows -----------------------------------------------------------------------------------------------------------------
def _honest_index(b, count):
    ix = b.ix
    ix.kicks, keys = 0, []
    for _ in range(count):
        k = b.fresh()
        full = all(not ix.free_slots(ix.bucket_of(k, h)) for h in range(ix.num_hashes))
        ix.kicks += int(full)
        cm.insert(ix, k, b.rec(), b.rng)
        keys.append(k)
    return keys


def _honest_rows(b, keys, n, nulls=0.1, misses=0.2):
    absent = [b.fresh() for _ in range(8)]
    for i in range(n):
        miss = b.rng.random() < misses
        b.ask((absent if miss else keys)[int(b.rng.integers(0, len(absent if miss else keys)))], valid=b.rng.random() >= nulls or n == 1)


def rows(layout, n):
    """one honest 4-byte table (42 keys in 5 buckets: the stash is used) read through every layout of the key column"""
    b = _Builder(f"rows-{layout}-{n}", "rows", 4)
    keys = _honest_index(b, 42)
    assert b.ix.free_slots(cm.STASH) != list(range(cm.STASH_SLOTS))
    if layout in ("mode0", "const"):  # (a ConstInt is an Int32)
        k = keys[7]
        assert cm.probe(b.ix, k) != (0, 0)
        dtype = abi.Int32 if layout == "const" else abi.Uint32
        v = value_of(dtype, k)
        return ProbeSet(b.name, "rows", b.ix, dtype, [v] * n, None, layout=layout, default=v)
    if layout == "mode0-no-default":
        return ProbeSet(b.name, "rows", b.ix, abi.Uint32, [value_of(abi.Uint32, keys[7])] * n, np.zeros(n, bool), layout="mode0", default=None)
    _honest_rows(b, keys, n, nulls=0.0 if layout == "mode1" else 0.3)
    if layout == "mode1":
        return ProbeSet(b.name, "rows", b.ix, b.dtype, b.values, None, layout="mode1")
    if layout == "subset":
        picked = np.sort(b.rng.choice(n, size=64, replace=False))
        return ProbeSet(b.name, "rows", b.ix, b.dtype, b.values, b.valid, starting_index=5, index_vector=picked)
    assert layout == "mode2"
    assert n == 1 or not all(b.valid)
    return ProbeSet(b.name, "rows", b.ix, b.dtype, b.values, b.valid, starting_index=5)


def honest(kb):
    """57 keys into 7 buckets (56 slots) by the model's inserter: residents are evicted and the stash is used"""
    b = _Builder(f"honest-{kb}", "honest", kb, num_buckets=7)
    keys = _honest_index(b, 57)
    assert b.ix.kicks > 0 and len(b.ix.free_slots(cm.STASH)) < cm.STASH_SLOTS
    for k in keys:
        assert cm.probe(b.ix, k) != (0, 0)
    _honest_rows(b, keys, 257)
    assert not all(b.valid)
    return ProbeSet(b.name, "honest", b.ix, b.dtype, b.values, b.valid, starting_index=5)


# ---- all of them ----------------------------------------------------------------------------------------------------------
def _all():
    out = []
    for kb in WIDTHS:
        out += [clamp(kb), zero_key(kb, True), zero_key(kb, False), stale(kb), full_bucket(kb), order(kb), honest(kb)]
        out += [hash_count(kb, nh) for nh in range(5)]
    out += [one_byte(dtype, kb) for dtype, kb in BYTE_CONFIGS]
    out += [buckets(kb, d) for kb in (4, 8, 16) for d in DIVISORS if kb == 4 or d <= 641]
    out += [buckets_by_seed(kb, d, part) for kb in (1, 2) for d in (3, 641) for part in range(3)]
    out += [prefix(abi.Uint32, kb) for kb in (1, 2, 3)] + [prefix(abi.Int64, 5), prefix(abi.UUID, 13)]
    out += [signed_keys(abi.Int8, 4), signed_keys(abi.Int16, 4), signed_keys(abi.Int8, 1), signed_keys(abi.Int16, 2)]
    out += [rows("mode2", n) for n in (1, 63, 64, 65, 257)]
    out += [rows("mode1", 65), rows("mode0", 64), rows("mode0-no-default", 64), rows("const", 63), rows("subset", 257)]
    names = [s.name for s in out]
    assert len(set(names)) == len(names)
    return out


_cache = []


def all_sets():
    if not _cache:
        _cache.extend(_all())
    return _cache


def by_name(name):
    return next(s for s in all_sets() if s.name == name)


def names(fusable=None):
    return [s.name for s in all_sets() if fusable is None or s.fusable == fusable]


# ---- a set through HashLookup on any backend ------------------------------------------------------------------------------
PAD = 8  # record slots behind the looked-up rows, which the call must leave alone
FILL = 0xAAAAAAAA


def key_col(s):
    """the key column of a mode 1 / 2 set as a select_model.Col"""
    import select_model as M
    return M.Col(s.dtype, s.column_values(), None if s.layout == "mode1" else s.valid, starting_index=s.starting_index if s.layout == "mode2" else 0)


def index_struct(s, table_ptr, **geometry):
    hi = abi.CuckooHashIndex()
    hi.buckets = table_ptr
    for i, seed in enumerate(s.ix.seeds):
        hi.seeds[i] = seed
    hi.keyBytes, hi.numHashes, hi.numBuckets = s.ix.key_bytes, s.ix.num_hashes, s.ix.num_buckets
    for k, v in geometry.items():
        setattr(hi, k, v)
    return hi


def hash_lookup(be, s, table=None, **geometry):
    """HashLookup of the set into a FILL-ed output of n + PAD records; all of its uint32 words.  `table`: the index already on
    the backend (a harness.Buf)."""
    import harness as H
    col = None
    if s.layout == "const":
        key = H.const_int(s.default)
    else:
        col = H.Column(be, s.dtype, default=s.default) if s.layout == "mode0" else key_col(s).upload(be)
        key = col.input()
    rows = np.arange(s.n, dtype=np.uint32) if s.index_vector is None else s.index_vector
    n = len(rows)
    tb = table or H.Buf(be, s.ix.table)
    idx, out = H.Buf(be, rows), H.Buf(be, np.full(2 * (n + PAD), FILL, np.uint32))
    try:
        assert be.call("HashLookup", key, out.ptr, idx.ptr, n, None, 0, index_struct(s, tb.ptr, **geometry), None, 0) == n
        be.wait()
        return out.read(np.uint32, 2 * (n + PAD))
    finally:
        for x in (col, idx, out, None if table else tb):
            if x:
                x.free()


def assert_lookup(got, s, what):
    want = s.expected()
    n = len(want)
    bad = np.flatnonzero(got[:n] != want) // 2
    assert not len(bad), (what, s.name, "rows", bad[:8], got[:n].reshape(-1, 2)[bad[:8]], want.reshape(-1, 2)[bad[:8]])
    assert (got[n:] == FILL).all(), (what, s.name, "records past n were written")
