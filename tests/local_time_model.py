"""Local time of a batch — FLOOR(CONVERT_TZ(time, table.zone), bucket)'s inner node — as a numpy model, written from the rule of
AresLocalTimeColumnRun (include/ares_extensions.h):

  value = time + offset (mod 2^32), valid = time valid and key valid and record found and joined value valid; a null row is 0;
  offset = tz[enum] for enum < len(tz), else 0; a mode-0 batch of the zone column yields its default WITHOUT the lookup; a stale
  record of the last batch and a batch outside the table give (0, null).

The join is a dictionary from key bytes to record (what cases.build_cuckoo placed plus a hand-placed entry), not a probe.  Every
row is tagged with the cases it exercises, so that a test can assert its fixture reaches them all (CASES).

A ZoneTable has select_join_model.Table's shape — a mode-2, a mode-1 and a mode-0 batch, the upper half of the last batch's
records stale — with a Uint8 and a Uint16 zone column and a plain Uint32 column beside them."""
import numpy as np

import cases
import select_join_model as J
import select_model as M
from aresdb_amd import abi

TZ_SIZE = 40
DEFAULT_ZONE = 7  # the mode-0 batch's default: it is the offset itself, not tz[7]
KEY_WIDTH = {abi.Int8: 1, abi.Uint8: 1, abi.Int16: 2, abi.Uint16: 2, abi.Int32: 4, abi.Uint32: 4, abi.Int64: 8, abi.UUID: 16}
NARROW_RANGE = {abi.Int8: (-128, 128), abi.Uint8: (0, 256), abi.Int16: (-32768, 32768), abi.Uint16: (0, 65536)}

CASES = {"null key", "missing key", "outside the table", "stale record", "mode 2", "mode 1", "mode 0 default", "mode 0 none",
         "null zone", "null time", "enum size - 1", "enum size", "offset -32768", "offset -1", "offset 0", "offset 32767",
         "wraps past 2^32", "wraps below 0"}
CASES_U16 = {"enum 32768", "enum 65535"}


def tz_offsets(size=TZ_SIZE, seed=5):
    """the int16 offset table: the extremes first, a non-zero last entry, and tz[DEFAULT_ZONE] != DEFAULT_ZONE"""
    rng = np.random.default_rng(seed)
    tz = (rng.integers(-48, 57, size) * 900).clip(-32768, 32767).astype(np.int16)
    tz[:4] = [-32768, -1, 0, 32767]
    tz[DEFAULT_ZONE] = 3600
    tz[size - 1] = -12600
    return tz


class ZoneTable(J.Table):
    COLUMNS = {"region": abi.Uint32, "zone8": abi.Uint8, "zone16": abi.Uint16}
    TYPES = COLUMNS

    def __init__(self, rng, keys, key_bytes, num_buckets, num_hashes=4, default=True, extra=None, tz_size=TZ_SIZE):
        self.key_bytes, self.num_buckets, self.num_hashes = key_bytes, num_buckets, num_hashes
        self.per_batch = (len(keys) + 2) // 3 + 1
        self.num_last = self.per_batch // 2
        extra = extra or {}
        recs = [(J.BASE_BATCH + i % 3, i // 3) for i in range(len(keys))] + list(extra.values())
        self.table, self.placed = cases.build_cuckoo(list(keys) + list(extra), key_bytes, num_buckets, J.SEEDS[:num_hashes], rng,
                                                     record_of=lambda i: recs[i])
        r = self.per_batch
        self.wide = {}
        self.cols = {}
        for name, dtype in self.COLUMNS.items():
            def values():
                if name == "region":
                    return rng.integers(0, 200, r)
                # the first records carry the edge enums: the offset extremes, the table's last entry and the first past it
                edge = [0, 1, 2, 3, tz_size - 1, tz_size] + ([32768, 65535] if dtype == abi.Uint16 else [255])
                v = rng.integers(0, tz_size + 4, r)
                v[:len(edge)] = edge[:r]
                return v
            d = {"region": 77, "zone8": DEFAULT_ZONE, "zone16": DEFAULT_ZONE}[name] if default else None
            valid = rng.random(r) < 0.8
            valid[:8] = True
            self.cols[name] = [M.Col(dtype, values(), valid, starting_index=3), M.Col(dtype, values()), M.Col(dtype, None, default=d)]


def _narrow_key_bytes(value, key_bytes):
    return int(value).to_bytes(4, "little", signed=True)[:key_bytes]


def make_table(key_dtype=abi.Uint16, key_bytes=None, nkeys=300, default=True, seed=11):
    """A ZoneTable over keys of `key_dtype`; one further key leads to a record in a batch outside the table.  key_bytes: the
    index's, when it differs from the column's width."""
    rng = np.random.default_rng(seed)
    kb = key_bytes or KEY_WIDTH[key_dtype]
    extra_record = (J.BASE_BATCH + 7, 10 ** 6)
    if key_dtype in NARROW_RANGE:
        lo, hi = NARROW_RANGE[key_dtype]
        pool = rng.permutation(np.arange(lo, hi))
        if lo < 0:  # negative keys first: they are certainly in the table
            pool = np.concatenate([pool[pool < 0][:20], pool])
        seen, values = set(), []
        for v in pool:
            k = _narrow_key_bytes(v, kb)
            if k not in seen:
                seen.add(k)
                values.append(int(v))
        count = min(nkeys, len(values) // 2)
        t = ZoneTable(rng, [_narrow_key_bytes(v, kb) for v in values[:count]], kb, count // 6 + 1, default=default,
                      extra={_narrow_key_bytes(values[count], kb): extra_record})
        t.used, t.others = values[:count + 1], values[count + 1:]  # (stored values, not key bytes)
    else:
        assert kb == KEY_WIDTH[key_dtype]
        keys = J._random_keys(rng, key_dtype, nkeys)
        outside = [k for k in J._random_keys(np.random.default_rng(seed + 1000), key_dtype, 40) if k not in keys][0]
        t = ZoneTable(rng, keys, kb, nkeys // 6 + 1, default=default, extra={outside: extra_record})
        t.used = list(keys) + [outside]
    t.key_dtype = key_dtype
    return t


def columns(t, n, seed, time_dtype=abi.Uint32, key_start=2, time_start=3, time_valid=True, key_valid=True):
    """(time column, key column) of a batch of n rows over the table: about a tenth of the keys are null, a sixth are not in
    the table; the times lie around now and at both ends of the 32-bit range, where the extreme offsets wrap them.
    time_valid / key_valid False: mode-1 columns."""
    rng = np.random.default_rng(seed)
    if t.key_dtype in NARROW_RANGE:
        pick = np.array([t.used[i] for i in rng.integers(0, len(t.used), n)], np.int64)
        miss = np.flatnonzero(rng.random(n) < 0.15)
        if t.others:
            pick[miss] = [t.others[i % len(t.others)] for i in miss]
        key = M.Col(t.key_dtype, pick, rng.random(n) >= 0.10 if key_valid else None, starting_index=key_start if key_valid else 0)
    else:
        key = J._key_column(rng, t.key_dtype, t.used, n)
        key = M.Col(t.key_dtype, key.values, key.valid if key_valid else None, starting_index=key_start if key_valid else 0)
    times = rng.integers(1_500_000_000, 1_700_000_000, n, dtype=np.int64)
    ends = rng.random(n)
    times[ends < 0.15] = rng.integers(0, 30000, int((ends < 0.15).sum()))
    times[ends > 0.85] = 2 ** 32 - 1 - rng.integers(0, 30000, int((ends > 0.85).sum()))
    times = times.astype(np.uint32)
    time = M.Col(time_dtype, times.view(np.int32) if time_dtype == abi.Int32 else times,
                 rng.random(n) >= 0.10 if time_valid else None, starting_index=time_start if time_valid else 0)
    return time, key


def fixture(n, key_dtype=abi.Uint16, key_bytes=None, time_dtype=abi.Uint32, nkeys=300, default=True, seed=11, **kw):
    """(ZoneTable, time column, key column of n rows)"""
    t = make_table(key_dtype, key_bytes, nkeys, default, seed)
    time, key = columns(t, n, seed + 1, time_dtype, **kw)
    return t, time, key


def zone_offset(table, tz, key, key_valid, zone):
    """(offset as a Python int, joined value valid, tags) of one fact key"""
    if not key_valid:
        return 0, False, ["null key"]
    rec = table.placed.get(key)
    if rec is None or rec[0] == 0:
        return 0, False, ["missing key"]
    rel, idx = rec[0] - J.BASE_BATCH, rec[1]
    if rel > 2:
        return 0, False, ["outside the table"]
    if rel == 2 and idx >= table.num_last:
        return 0, False, ["stale record"]
    batch = table.cols[zone][rel]
    if batch.values is None:  # mode 0: the default as it stands
        if batch.default is None:
            return 0, False, ["mode 0 none"]
        return int(batch.default), True, ["mode 0 default"]
    enum = int(batch.values[idx])
    ok = True if batch.valid is None else bool(batch.valid[idx])
    offset = int(tz[enum]) if enum < len(tz) else 0
    tags = ["mode 2" if batch.valid is not None else "mode 1"]
    if not ok:
        tags.append("null zone")
    else:
        tags += ["enum %s" % what for what, e in (("size - 1", len(tz) - 1), ("size", len(tz)), ("32768", 32768), ("65535", 65535)) if enum == e]
        tags += ["offset %d" % offset] if offset in (-32768, -1, 0, 32767) and enum < len(tz) else []
    return offset, ok, tags


def local_time(table, tz, time, key, zone, n):
    """(values uint32, validity bool, the set of cases the rows reach)"""
    keys = J.key_bytes_of(key, n, table.key_bytes)
    key_valid, time_valid = M._valid(key, n), M._valid(time, n)
    bits = M._bits(time, n)
    values, valid, reached = np.zeros(n, np.uint32), np.zeros(n, bool), set()
    for i in range(n):
        offset, ok, tags = zone_offset(table, tz, keys[i], bool(key_valid[i]), zone)
        reached.update(tags)
        if not time_valid[i]:
            reached.add("null time")
        if ok and time_valid[i]:
            total = int(bits[i]) + offset
            if total >= 2 ** 32:
                reached.add("wraps past 2^32")
            if total < 0:
                reached.add("wraps below 0")
            values[i], valid[i] = total % 2 ** 32, True
    return values, valid, reached


def column_bytes(values, valid, n):
    """the entry point's output: (bitmap bytes of the padded bitmap, value bytes of the n rows)"""
    bits = np.zeros(((n + 7) // 8 + 63) // 64 * 64 * 8, bool)
    bits[:n] = valid[:n]
    return np.packbits(bits, bitorder="little"), values[:n].astype(np.uint32).view(np.uint8)


def zone_input(dtable, zone, rids, tz_ptr, tz_size):
    """the zone column of a select_join_model.DeviceTable as a foreign operand read through the offset table"""
    iv = dtable.input(zone, rids)
    iv.Vector.ForeignVP.TimezoneLookup, iv.Vector.ForeignVP.TimezoneLookupSize = tz_ptr, tz_size
    return iv
