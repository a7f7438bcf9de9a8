"""An independent model of HashReduce's group identity, and the inverse of its hash.

HashReduce identifies a group by the 32-bit murmur3 (x86_32, seed 0) of the packed dimension row
[dimension values, widest slot first, little-endian][one validity byte per dimension]: two different rows with one hash are
ONE group, whose dimensions are those of its lowest row.  Everything that decides correctness in the partitioned kernels
(partition, table slot, merge round) is a function of that hash, so the tests choose hashes and compute the rows that have
them: murmur3_x86_32 is invertible in its first 4-byte block (every step is an odd multiply, a rotate, an xor or an
xorshift), and the first block of a packed row is the first 4-byte dimension.

Written from the murmur3 definition with Python integers; nothing of the project's hashing or grouping code is imported.
"""
from fractions import Fraction
import struct

M32 = 0xFFFFFFFF
C1, C2 = 0xcc9e2d51, 0x1b873593
F1, F2 = 0x85ebca6b, 0xc2b2ae35
N1 = 0xe6546b64
# inverses modulo 2^32 of the odd multipliers
C1_INV, C2_INV, F1_INV, F2_INV, FIVE_INV = (pow(x, -1, 1 << 32) for x in (C1, C2, F1, F2, 5))


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def _rotr(x, r):
    return ((x >> r) | (x << (32 - r))) & M32


def _mix_k(k):
    return (_rotl((k * C1) & M32, 15) * C2) & M32


def _unmix_k(k):
    return (_rotr((k * C2_INV) & M32, 15) * C1_INV) & M32


def murmur3_32(data: bytes) -> int:
    """murmur3_x86_32 of `data`, seed 0."""
    h = 0
    nb = len(data) // 4
    for i in range(nb):
        h ^= _mix_k(int.from_bytes(data[4 * i:4 * i + 4], "little"))
        h = (_rotl(h, 13) * 5 + N1) & M32
    tail = data[4 * nb:]
    if tail:
        h ^= _mix_k(int.from_bytes(tail, "little"))
    h ^= len(data)
    h ^= h >> 16
    h = (h * F1) & M32
    h ^= h >> 13
    h = (h * F2) & M32
    h ^= h >> 16
    return h


def pack_row(values, valids, widths=None) -> bytes:
    """The bytes HashReduce hashes: the slots' values in vector order, then one validity byte per dimension."""
    widths = widths or [4] * len(values)
    assert len(values) == len(valids) == len(widths)
    return b"".join(int(v).to_bytes(w, "little") for v, w in zip(values, widths)) + bytes(int(bool(o)) for o in valids)


def row_hash(values, valids, widths=None) -> int:
    return murmur3_32(pack_row(values, valids, widths))


def row_with_hash(target, others, valids, widths=None) -> int:
    """The value of dimension 0 (a 4-byte slot: the packed row's first block) for which the row
    [x, others...] with validity bytes `valids` hashes to `target`.  `widths`: the slot widths of all dimensions in vector
    order (default: all 4 bytes; a 2- or 1-byte slot may follow the 4-byte ones)."""
    widths = widths or [4] * (len(others) + 1)
    assert widths[0] == 4 and len(widths) == len(others) + 1 == len(valids)
    # behind the first block: the other slots, then all validity bytes
    rest = b"".join(int(v).to_bytes(w, "little") for v, w in zip(others, widths[1:])) + bytes(int(bool(o)) for o in valids)
    total = 4 + len(rest)
    # undo the finaliser
    h = target & M32
    h ^= h >> 16
    h = (h * F2_INV) & M32
    h ^= (h >> 13) ^ (h >> 26)
    h = (h * F1_INV) & M32
    h ^= h >> 16
    h ^= total
    # undo the tail and the blocks behind the first, last to first
    nb = len(rest) // 4
    tail = rest[4 * nb:]
    if tail:
        h ^= _mix_k(int.from_bytes(tail, "little"))
    for i in range(nb - 1, -1, -1):
        h = _rotr(((h - N1) * FIVE_INV) & M32, 13)
        h ^= _mix_k(int.from_bytes(rest[4 * i:4 * i + 4], "little"))
    # h is the state behind block 0, which started from seed 0: h = rotl(mix(x), 13) * 5 + n
    return _unmix_k(_rotr(((h - N1) * FIVE_INV) & M32, 13))


# ---- aggregates -----------------------------------------------------------------------------------------------------------
# (operation, value kind): the kinds are the measure vector's element types
_INT_BITS = {"u32": (32, False), "i32": (32, True), "i64": (64, True), "u64": (64, False)}


def _wrap(x, kind):
    bits, signed = _INT_BITS[kind]
    x &= (1 << bits) - 1
    return x - (1 << bits) if signed and x >> (bits - 1) else x


def _identity(op, kind):
    if op == "sum":
        return Fraction(0) if kind in ("f32", "f64") else 0
    if kind == "f32":  # the operator's neutral element (aggregate.hpp: a group slot starts from +inf / -inf): no value yet
        return None
    bits, signed = _INT_BITS[kind]
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    return hi if op == "min" else lo


def _exact_float(x, kind):
    f = float(x)
    if kind == "f32":
        f = struct.unpack("<f", struct.pack("<f", f))[0]
    assert Fraction(f) == x, f"{x} is not exactly representable as {kind}: the case is not bit-exact"
    return f


def groups_by_hash(rows, valids, values, agg, widths=None):
    """The exact result of HashReduce over `rows` (tuples of dimension values in vector order), `valids` (tuples of validity
    bytes) and `values` (Python ints, or floats / Fractions for the float kinds, or (average, count) pairs for op = avg),
    agg = (op, kind) with op in sum / min / max / avg:
    group = hash32, representative = lowest row index, value = the aggregate from its identity — integer sums wrap like the
    measure type, float sums are exact rationals that must stay representable at every step.
    Returns ({(representative values, representative valids): value}, {hash: representative row index})."""
    op, kind = agg
    is_float = kind in ("f32", "f64")
    acc, first = {}, {}
    for i, (r, o, v) in enumerate(zip(rows, valids, values)):
        h = row_hash(r, o, widths)
        if h not in first:
            first[h] = i
            acc[h] = [] if op == "avg" else _identity(op, kind)
        if op == "avg":
            acc[h].append(v)
        elif is_float and op != "sum":
            acc[h] = Fraction(v) if acc[h] is None else (min if op == "min" else max)(acc[h], Fraction(v))
        elif is_float:
            acc[h] = acc[h] + Fraction(v)
            _exact_float(acc[h], kind)
        elif op == "sum":
            acc[h] = _wrap(acc[h] + int(v), kind)
        else:
            acc[h] = min(acc[h], int(v)) if op == "min" else max(acc[h], int(v))
    out = {}
    for h, i in first.items():
        key = (tuple(int(x) for x in rows[i]), tuple(int(bool(x)) for x in valids[i]))
        assert key not in out
        if op == "avg":
            out[key] = _average(acc[h])
        else:
            out[key] = _exact_float(acc[h], kind) if is_float else acc[h]
    return out, first


def _average(pairs):
    """AVG carries {float32 average, uint32 count} and merges by a rolling float32 average whose value depends on the order
    of merges; it is exact, whatever the order, for a group of one pair with count 1 and for a group whose averages are all
    0 — the only groups the cases build."""
    if len(pairs) == 1 and pairs[0][1] == 1:
        return (_exact_float(Fraction(pairs[0][0]), "f32"), 1)
    assert all(v == 0 for v, _ in pairs)
    return (0.0, sum(c for _, c in pairs))
