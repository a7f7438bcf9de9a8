"""An independent model of Sort + Reduce's group identity and order, and the inverse of its hash.

Sort + Reduce identifies a group by lo64(murmur3_x64_128, seed 0) of the packed dimension row [dimension values, widest slot
first, little-endian][one validity byte per dimension]: one group per distinct hash, groups emitted in ascending hash order,
a group's dimensions those of its lowest row in [previous result, then batch] (a stable sort of an iota index vector) — two
different rows with one hash are ONE group.  Everything that decides correctness in the kernels (radix digit, fix-up
segment, partition, home bucket, run boundary) is a function of that hash, so the tests choose hashes and compute the rows
that have them.  A packed row whose values fill exactly one 16-byte block, followed by its validity bytes as the tail, is
invertible: the block step from seed 0 is a bijection on (k1, k2), the tail XORs a constant into h1, the finalisation is a
bijection on 128 bits, and the returned word is fmix(h1') + fmix(h2') — for a target T and any free word G set
fmix(h2') = G, fmix(h1') = T - G and undo every step (all multipliers are odd).  Two values of G give two different rows
with one 64-bit hash.

Written from the murmur3 definition with Python integers (and once more with numpy uint64 arrays, so that 50 k rows build in
about a second); nothing of the project's hashing or grouping code is imported."""
from fractions import Fraction
import struct

import numpy as np

M64 = (1 << 64) - 1
C1, C2 = 0x87c37b91114253d5, 0x4cf5ad432745937f
N1, N2 = 0x52dce729, 0x38495ab5
F1, F2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
C1_INV, C2_INV, F1_INV, F2_INV, FIVE_INV = (pow(x, -1, 1 << 64) for x in (C1, C2, F1, F2, 5))

# layouts whose values are exactly one 16-byte block (slot widths in vector order)
LAYOUTS = ((4, 4, 4, 4), (8, 4, 4), (16,))

# What the model does NOT state (an input that would need it is refused by an assertion):
UNDEFINED = [
    "AVG_FLOAT over a group that holds a non-zero average and more than one pair: the rolling float32 average "
    "(avg / total * count, pair by pair) depends on the order of the merges, which differs between a sort and a table",
    "SUM_FLOAT over a group whose sum of magnitudes reaches 2^24 eighths (float32) / 2^53 eighths (float64): a partial sum "
    "could round, and then the order of additions shows",
    "float values that are no multiples of 1/8, NaNs among MIN_FLOAT / MAX_FLOAT values (the table paths hand those to the sort)",
    "rows that are null in a hashed slot with other than zero value bytes on the scan-fed path: a transform writes zero "
    "bytes under a null, so such rows exist only in vectors a host wrote itself",
]


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _rotr(x, r):
    return ((x >> r) | (x << (64 - r))) & M64


def _fmix(k):
    k ^= k >> 33
    k = (k * F1) & M64
    k ^= k >> 33
    k = (k * F2) & M64
    return k ^ (k >> 33)


def _unfmix(k):
    k ^= k >> 33   # (x ^ x >> 33 is its own inverse: 2 * 33 > 64)
    k = (k * F2_INV) & M64
    k ^= k >> 33
    k = (k * F1_INV) & M64
    return k ^ (k >> 33)


def _mix1(k):
    return (_rotl((k * C1) & M64, 31) * C2) & M64


def _mix2(k):
    return (_rotl((k * C2) & M64, 33) * C1) & M64


def _unmix1(k):
    return (_rotr((k * C2_INV) & M64, 31) * C1_INV) & M64


def _unmix2(k):
    return (_rotr((k * C1_INV) & M64, 33) * C2_INV) & M64


def murmur3_128_lo64(data: bytes) -> int:
    """The low 64 bits (h1) of murmur3_x64_128 of `data`, seed 0."""
    h1 = h2 = 0
    nb = len(data) // 16
    for i in range(nb):
        k1 = int.from_bytes(data[16 * i:16 * i + 8], "little")
        k2 = int.from_bytes(data[16 * i + 8:16 * i + 16], "little")
        h1 ^= _mix1(k1)
        h1 = ((_rotl(h1, 27) + h2) * 5 + N1) & M64
        h2 ^= _mix2(k2)
        h2 = ((_rotl(h2, 31) + h1) * 5 + N2) & M64
    tail = data[16 * nb:]
    if len(tail) > 8:
        h2 ^= _mix2(int.from_bytes(tail[8:], "little"))
    if tail:
        h1 ^= _mix1(int.from_bytes(tail[:8], "little"))
    h1 ^= len(data)
    h2 ^= len(data)
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    h1, h2 = _fmix(h1), _fmix(h2)
    return (h1 + h2) & M64


def pack_row(values, valids, widths) -> bytes:
    assert len(values) == len(valids) == len(widths)
    return b"".join(int(v).to_bytes(w, "little") for v, w in zip(values, widths)) + bytes(int(bool(o)) for o in valids)


def row_with_hash64(target, free, valids, widths):
    """The slot values (vector order) of the row with validity bytes `valids` in layout `widths` (16 value bytes) whose hash
    is `target`; `free`: any 64-bit word — every value of it gives another row."""
    widths = tuple(widths)
    assert sum(widths) == 16 and len(valids) == len(widths) <= 8
    total = 16 + len(valids)
    h2 = _unfmix(free & M64)                   # h2' = h2a + h1'
    h1 = _unfmix((target - free) & M64)        # h1' = h1a + h2a
    h2 = (h2 - h1) & M64
    h1 = (h1 - h2) & M64
    h1 ^= total
    h2 ^= total
    h1 ^= _mix1(int.from_bytes(bytes(int(bool(o)) for o in valids), "little"))  # the tail: at most 8 bytes, all in k1
    # the block, from h1 = h2 = 0: h1 = rotl(mix1(k1), 27) * 5 + n1, h2 = (rotl(mix2(k2), 31) + h1) * 5 + n2
    k2 = _unmix2(_rotr(((((h2 - N2) * FIVE_INV) & M64) - h1) & M64, 31))
    k1 = _unmix1(_rotr(((h1 - N1) * FIVE_INV) & M64, 27))
    block = k1 | (k2 << 64)
    out, at = [], 0
    for w in widths:
        out.append((block >> (8 * at)) & ((1 << (8 * w)) - 1))
        at += w
    return tuple(out)


# ---- the same with numpy uint64 arrays ------------------------------------------------------------------------------------
def _u(x):
    return np.uint64(x)


def _vrotl(x, r):
    return (x << _u(r)) | (x >> _u(64 - r))


def _vrotr(x, r):
    return (x >> _u(r)) | (x << _u(64 - r))


def _vfmix(k):
    k = k ^ (k >> _u(33))
    k = k * _u(F1)
    k = k ^ (k >> _u(33))
    k = k * _u(F2)
    return k ^ (k >> _u(33))


def _vunfmix(k):
    k = k ^ (k >> _u(33))
    k = k * _u(F2_INV)
    k = k ^ (k >> _u(33))
    k = k * _u(F1_INV)
    return k ^ (k >> _u(33))


def _vmix1(k):
    return _vrotl(k * _u(C1), 31) * _u(C2)


def _vmix2(k):
    return _vrotl(k * _u(C2), 33) * _u(C1)


def _le_words(mat):
    """the little-endian uint64 of every row of a uint8 matrix of at most 8 columns"""
    out = np.zeros(len(mat), np.uint64)
    for j in range(mat.shape[1]):
        out |= mat[:, j].astype(np.uint64) << _u(8 * j)
    return out


def hash_rows(packed):
    """murmur3_128_lo64 of every row of a uint8 matrix [n, row bytes]."""
    packed = np.ascontiguousarray(packed, np.uint8)
    n, nbytes = packed.shape
    h1 = np.zeros(n, np.uint64)
    h2 = np.zeros(n, np.uint64)
    with np.errstate(over="ignore"):
        nb = nbytes // 16
        for i in range(nb):
            h1 ^= _vmix1(_le_words(packed[:, 16 * i:16 * i + 8]))
            h1 = (_vrotl(h1, 27) + h2) * _u(5) + _u(N1)
            h2 ^= _vmix2(_le_words(packed[:, 16 * i + 8:16 * i + 16]))
            h2 = (_vrotl(h2, 31) + h1) * _u(5) + _u(N2)
        tail = packed[:, 16 * nb:]
        if tail.shape[1] > 8:
            h2 ^= _vmix2(_le_words(tail[:, 8:]))
        if tail.shape[1]:
            h1 ^= _vmix1(_le_words(tail[:, :8]))
        h1 ^= _u(nbytes)
        h2 ^= _u(nbytes)
        h1 = h1 + h2
        h2 = h2 + h1
        return _vfmix(h1) + _vfmix(h2)


def rows_with_hash64(targets, frees, valids, widths):
    """row_with_hash64 for arrays of targets and free words: the packed rows, a uint8 matrix [n, 16 + dimensions]."""
    assert sum(widths) == 16 and len(valids) == len(widths)
    targets = np.asarray(targets, np.uint64)
    frees = np.asarray(frees, np.uint64)
    total = 16 + len(valids)
    tail = int.from_bytes(bytes(int(bool(o)) for o in valids), "little")
    with np.errstate(over="ignore"):
        h2 = _vunfmix(frees)
        h1 = _vunfmix(targets - frees)
        h2 = h2 - h1
        h1 = h1 - h2
        h1 = h1 ^ _u(total) ^ _u(_mix1(tail))
        h2 = h2 ^ _u(total)
        k2 = _vrotr((h2 - _u(N2)) * _u(FIVE_INV) - h1, 31) * _u(C1_INV)
        k2 = _vrotr(k2, 33) * _u(C2_INV)
        k1 = _vrotr((h1 - _u(N1)) * _u(FIVE_INV), 27) * _u(C2_INV)
        k1 = _vrotr(k1, 31) * _u(C1_INV)
    n = len(targets)
    out = np.empty((n, total), np.uint8)
    out[:, 0:8] = np.ascontiguousarray(k1).view(np.uint8).reshape(n, 8)
    out[:, 8:16] = np.ascontiguousarray(k2).view(np.uint8).reshape(n, 8)
    out[:, 16:] = np.array([int(bool(o)) for o in valids], np.uint8)
    return out


def slot_columns(packed, widths):
    """the packed rows as one uint8 matrix [n, width] per dimension, and one validity byte column per dimension"""
    cols, at = [], 0
    for w in widths:
        cols.append(np.ascontiguousarray(packed[:, at:at + w]))
        at += w
    return cols, [np.ascontiguousarray(packed[:, at + d]) for d in range(len(widths))]


# ---- aggregates -----------------------------------------------------------------------------------------------------------
_INT_BITS = {"u32": (32, False), "i32": (32, True), "i64": (64, True), "u64": (64, False)}
_FLOAT_EXACT = {"f32": 1 << 24, "f64": 1 << 53}   # eighths


def _wrap(x, kind):
    bits, signed = _INT_BITS[kind]
    x &= (1 << bits) - 1
    return x - (1 << bits) if signed and x >> (bits - 1) else x


def _exact_float(x, kind):
    f = float(x)
    if kind == "f32":
        f = struct.unpack("<f", struct.pack("<f", f))[0]
    assert Fraction(f) == x, f"{x} is not exactly representable as {kind}: the case is not bit-exact"
    return f


def _fold(op, kind, vals):
    """op over the values of one group, from the operator's identity"""
    if op == "avg":
        pairs = [(Fraction(a), int(c)) for a, c in vals]
        count = sum(c for _, c in pairs)
        assert len(pairs) == 1 or all(a == 0 for a, _ in pairs), UNDEFINED[0]
        mean = sum(a * c for a, c in pairs) / count if count else Fraction(0)
        return (_exact_float(mean, "f32"), count)   # (exact mean, rounded once)
    if kind in _FLOAT_EXACT:
        fr = [Fraction(v) for v in vals]
        assert all((8 * v).denominator == 1 for v in fr), UNDEFINED[2]
        if op == "sum":
            assert sum(abs(8 * v) for v in fr) < _FLOAT_EXACT[kind], UNDEFINED[1]
            return _exact_float(sum(fr, Fraction(0)), kind)
        return _exact_float(min(fr) if op == "min" else max(fr), kind)   # (from +inf / -inf: the group has a value)
    bits, signed = _INT_BITS[kind]
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    if op == "sum":
        return _wrap(sum(int(v) for v in vals), kind)
    return min([hi] + [int(v) for v in vals]) if op == "min" else max([lo] + [int(v) for v in vals])


class Reduced:
    """What a host can observe of one Sort + Reduce call."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def groups_by_hash64(prev_rows, batch_rows, values, agg):
    """The exact result of Sort + Reduce over the packed rows [prev_rows, then batch_rows] (uint8 matrices; prev_rows may be
    None) and `values` (one per row: Python ints, Fractions / floats for the float kinds, (average, count) pairs for avg),
    agg = (op, kind):
      sorted_hash, sorted_index   the hash and index vector between Sort and Reduce (stable sort of an iota by the hash);
      hashes, out_index, rows, values   per group, ascending hash: its hash, its representative (lowest position), the
                                        representative's packed row, the aggregate."""
    op, kind = agg
    rows = batch_rows if prev_rows is None or not len(prev_rows) else np.concatenate([prev_rows, batch_rows])
    assert len(rows) == len(values)
    h = hash_rows(rows)
    order = np.argsort(h, kind="stable")
    sh = h[order]
    heads = np.flatnonzero(np.concatenate([[True], sh[1:] != sh[:-1]])) if len(sh) else np.zeros(0, np.int64)
    ends = np.concatenate([heads[1:], [len(sh)]]).astype(np.int64)
    out_index = order[heads]
    olist = order.tolist()
    out_values = [_fold(op, kind, [values[i] for i in olist[a:b]]) for a, b in zip(heads.tolist(), ends.tolist())]
    return Reduced(sorted_hash=sh, sorted_index=order.astype(np.uint32), hashes=sh[heads], out_index=out_index.astype(np.uint32),
                   rows=rows[out_index], values=out_values, groups=len(heads))


# ---- the top-half sort's fix-up, from its definition ----------------------------------------------------------------------
def fixup_census(hashes, max_run, long_max, block=256):
    """What the fix-up after four stable passes over the TOP halves finds in the hash vector `hashes` (input order): the
    segments (runs of equal top half in the order those passes leave) that hold a descent of the low halves, by length —
    short (<= max_run), long (<= long_max), beyond — and, per `block` consecutive positions, the number of short segments
    whose FIRST descent lies in it."""
    h = np.asarray(hashes, np.uint64)
    order = np.argsort(h >> _u(32), kind="stable")
    k = h[order]
    top, low = k >> _u(32), k & _u(0xFFFFFFFF)
    n = len(k)
    starts = np.flatnonzero(np.concatenate([[True], top[1:] != top[:-1]])) if n else np.zeros(0, np.int64)
    ends = np.concatenate([starts[1:], [n]]).astype(np.int64)
    descent = np.concatenate([[False], (top[1:] == top[:-1]) & (low[1:] < low[:-1])]) if n else np.zeros(0, bool)
    at = np.flatnonzero(descent)
    seg_of = np.searchsorted(starts, at, side="right") - 1
    short, long_, beyond, per_block = [], [], [], {}
    seen = set()
    for i, s in zip(at.tolist(), seg_of.tolist()):
        if s in seen:
            continue
        seen.add(s)
        length = int(ends[s] - starts[s])
        if length <= max_run:
            short.append((int(starts[s]), int(ends[s])))
            per_block[i // block] = per_block.get(i // block, 0) + 1
        elif length <= long_max:
            long_.append((int(starts[s]), int(ends[s])))
        else:
            beyond.append((int(starts[s]), int(ends[s])))
    return Reduced(short=short, long=long_, beyond=beyond, per_block=per_block, descents=len(at), keys=k)
