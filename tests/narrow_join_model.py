"""Fixtures for the direct flavour of AresJoinColumnsRun (include/ares_extensions.h): select_join_model.Table — four joined
columns of widths 4 / 2 / 1 and Float32 in a mode-2, a mode-1 and a mode-0 batch, stale records in the last batch, a hand-placed
record in a batch outside the table — over keys of the 1- and 2-byte types, signed ones among them, and over an index whose
keyBytes differ from the key column's width.  The model of a joined column is Table.joined: a dictionary, not a probe."""
import numpy as np

import select_join_model as J
import select_model as M
from aresdb_amd import abi

NARROW = [abi.Uint8, abi.Int8, abi.Uint16, abi.Int16]
RANGE = {abi.Int8: (-128, 128), abi.Uint8: (0, 256), abi.Int16: (-32768, 32768), abi.Uint16: (0, 65536)}
KEY_SPACE = {abi.Int8: 256, abi.Uint8: 256, abi.Int16: 65536, abi.Uint16: 65536}


def key_bytes(value, kb):
    """the probe's key of a stored value: the first kb bytes of the value widened to 32 bits"""
    return int(value).to_bytes(4, "little", signed=True)[:kb]


def make_table(key_dtype, kb=None, nkeys=300, num_buckets=None, num_hashes=4, default=True, seed=11):
    """A select_join_model.Table over stored values of `key_dtype`; the negative values of a signed type come first, so they are
    in the table.  kb: the index's keyBytes when they differ from the column's width (distinct values that share their first kb
    bytes are one key).  t.used: the stored values in the table, the last one leading to a batch outside it; t.others: values
    the table does not hold."""
    rng = np.random.default_rng(seed)
    kb = kb or abi.DATA_TYPE_BYTES[key_dtype]
    lo, hi = RANGE[key_dtype]
    pool = rng.permutation(np.arange(lo, hi))
    if lo < 0:
        pool = np.concatenate([pool[pool < 0][:20], pool])
    seen, values = set(), []
    for v in pool:
        k = key_bytes(v, kb)
        if k not in seen:
            seen.add(k)
            values.append(int(v))
    count = min(nkeys, len(values) // 2)
    if num_buckets is None:
        num_buckets = count // 7 + 1  # (every key finds a place; with most seeds the stash holds some)
    t = J.Table(rng, [key_bytes(v, kb) for v in values[:count]], kb, num_buckets, num_hashes, default,
                extra={key_bytes(values[count], kb): (J.BASE_BATCH + 7, 10 ** 6)})
    held = set(key_bytes(v, kb) for v in values[:count + 1])
    t.key_dtype, t.used = key_dtype, values[:count + 1]
    t.others = [v for v in values[count + 1:] if key_bytes(v, kb) not in held]
    return t


def key_column(t, n, seed, starting_index=3, valid=True):
    """a fact column of n rows over the table: about a tenth of the keys null, a seventh not in the table; the key that leads
    outside the table is met for sure.  valid False: a mode-1 column."""
    rng = np.random.default_rng(seed)
    pick = np.array([t.used[i] for i in rng.integers(0, len(t.used), n)], np.int64)
    miss = np.flatnonzero(rng.random(n) < 0.15)
    if t.others:
        pick[miss] = [t.others[i % len(t.others)] for i in miss]
    ok = rng.random(n) >= 0.10
    if n > 5:
        pick[5], ok[5] = t.used[-1], True
    return M.Col(t.key_dtype, pick, ok if valid else None, starting_index=starting_index if valid else 0)


def stored(col, n):
    """the stored key values of the rows as table indices: the low 8 or 16 bits"""
    return (M._bits(col, n) & (KEY_SPACE[col.dtype] - 1)).astype(np.int64)


def enumerated(key_dtype):
    """a mode-1 column that holds every stored value of the type once, value v (as stored bits) at row v"""
    space = KEY_SPACE[key_dtype]
    raw = np.arange(space, dtype=np.uint32).astype(np.uint16 if space == 65536 else np.uint8)
    return M.Col(key_dtype, raw.view(M._NP[key_dtype]))


def reached(t, key, n):
    """the cases of the joined-value rule the rows reach"""
    keys, valid = J.key_bytes_of(key, n, t.key_bytes), M._valid(key, n)
    out = set()
    for k, v in zip(keys, valid):
        rec = t.placed.get(k) if v else None
        if not v:
            out.add("null key")
        elif rec is None:
            out.add("missing key")
        elif rec[0] - J.BASE_BATCH >= 3:
            out.add("outside the table")
        elif rec[0] - J.BASE_BATCH == 2 and rec[1] >= t.num_last:
            out.add("stale record")
        else:
            out.add("mode %d" % (2 - (rec[0] - J.BASE_BATCH)))
    return out


CASES = {"null key", "missing key", "outside the table", "stale record", "mode 2", "mode 1", "mode 0"}
