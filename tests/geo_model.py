"""An independent model of GeoBatchIntersects and WriteGeoShapeDim, written from the definition of the operation (numpy and
fractions only; nothing here follows oracle/aql_oracle.c or geo.hip line by line).

Layout.  A shape batch is three arrays of N polygon points: latitudes, longitudes (float32) and shape numbers (uint8).  Points p
and p + 1 are joined by an edge when both carry the same shape number and neither latitude is >= FLT_MAX (a comparison that is
false for NaN): that is the (FLT_MAX, FLT_MAX) ring separator, and +inf / NaN latitudes with it.

Crossing rule.  For a valid test point (lat, x), edge p toggles bit shape[p] of the entry's predicate words iff
(long1 > x) != (long2 > x) and lat < t, where t is the latitude at which the edge meets the meridian of x (even-odd rule with a
ray towards larger latitudes; the longitude test is half open, so a vertex belongs to exactly one of its two edges).

Two statements of the verdict:
  * exact_verdict: fractions.Fraction on the float32 inputs.  The straddle test compares floats and is exact as it stands; t is
    the exact rational lat1 + (lat2 - lat1)(x - long1) / (long2 - long1).  Per straddling pair it also gives the margin
    |lat - t| and the bound 8 * 2^-24 * (|t - lat1| + |lat1|) on what the float32 evaluation of
    (lat2 - lat1) * (x - long1) / (long2 - long1) + lat1 can be off by: three differences, a product and a quotient carry one
    relative error of 2^-24 each into the quotient (5 * 2^-24 * |t - lat1|), the final sum one more on |t|; 8 covers the
    second-order terms.  A pair is *decided* when margin > bound.  The bound only holds where no step overflows and neither
    the product nor the quotient falls into the denormal range, so pairs with a non-finite input, an intermediate of
    magnitude >= FLT_MAX or a non-zero product / quotient below 2^-126 are left undecided, as are on-edge pairs (margin 0).
  * f32_verdict: the same expression in numpy float32, one operation per step, vectorised over entries x edges.  It is the
    only statement of the rounding behaviour and decides what exact_verdict leaves open.

Null points (invalid entries): if N >= 2 and shape[0] == shape[1] every predicate word of the entry becomes !inOrOut (the
numeric value 0 or 1, in every word), otherwise the words stay as they were.  Only the shape numbers count here: the latitudes
of points 0 and 1 are not looked at.

Words that hold something already are XORed into.  Compaction: the first set bit of an entry's words is read as an int8, so
shapes 128..255 read as "no shape"; entry i is dropped when inOrOut == (no shape); the index vector and every RecordID vector
are compacted in order.  WriteGeoShapeDim: the first shape (0..127) of every entry that has one, in entry order, validity 1.

Joined points (tests/harness.py, cases.GeoCase): entry i reads RecordID i = (batchID, index).  batchID 0 is null; a record
with batchID - BaseBatchID >= NumBatches - 1 and index >= NumRecordsInLastBatch is null; a constant batch (no base pointer)
yields the default value with HasDefault as its validity; otherwise the batch's value and validity bit.

Where the model had to be settled by the reference's behaviour rather than by the definition:
  * TotalNumPoints == 0 is not defined by the reference: its iterator divides by the point count when it is advanced
    (query/iterator.hpp, GeoBatchIntersectIterator::advance), so its host build stops with a division by zero.  The model, the
    C checker and the HIP library all leave the words alone and compact on them; the reference build is not run on that case.
"""
from fractions import Fraction

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
_FLT_MAX_Q = Fraction(float(FLT_MAX))
_FLT_MIN_Q = Fraction(1, 2 ** 126)
_EPS8 = Fraction(8, 2 ** 24)

# what the ABI does not define and no test sends (the reference writes outside the entry's words, or reads outside the batches)
UNDEFINED = (
    "a shape number >= 32 * TotalWords",
    "TotalWords == 0, TotalWords > 8 (beyond the error return for > 8)",
    "a RecordID with batchID < BaseBatchID, or with batchID - BaseBatchID >= NumBatches and index < NumRecordsInLastBatch",
    "TotalNumPoints == 0 on the reference build (division by zero, see above); the other implementations are compared",
    "the index vector and RecordID vectors past the kept count",
)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def edge_mask(lats, shape):
    """bool[N - 1]: points p and p + 1 form an edge"""
    lats, shape = _f32(lats), np.asarray(shape, np.uint8)
    if len(lats) < 2:
        return np.zeros(0, bool)
    with np.errstate(invalid="ignore"):
        return (shape[:-1] == shape[1:]) & (lats[:-1] < FLT_MAX) & (lats[1:] < FLT_MAX)


def straddles(longs, plong):
    """bool[n, N - 1]: (long1 > x) != (long2 > x); comparisons of floats, exact as they stand"""
    longs, x = _f32(longs), _f32(plong)[:, None]
    if len(longs) < 2:
        return np.zeros((len(x), 0), bool)
    with np.errstate(invalid="ignore"):
        return (longs[None, :-1] > x) != (longs[None, 1:] > x)


def f32_verdict(lats, longs, shape, plat, plong):
    """bool[n, N - 1]: edge p toggles for point i, every step rounded to float32 once, in the order
    (lat2 - lat1) * (x - long1) / (long2 - long1) + lat1"""
    lats, longs = _f32(lats), _f32(longs)
    y, x = _f32(plat)[:, None], _f32(plong)[:, None]
    if len(lats) < 2:
        return np.zeros((len(x), 0), bool)
    with np.errstate(all="ignore"):
        dlat = lats[1:] - lats[:-1]
        dx = x - longs[None, :-1]
        prod = dlat[None, :] * dx
        dlong = longs[1:] - longs[:-1]
        quot = prod / dlong[None, :]
        t = quot + lats[None, :-1]
        assert t.dtype == np.float32
        below = y < t
    return edge_mask(lats, shape)[None, :] & straddles(longs, plong) & below


class Exact:
    """exact_verdict's result: toggles / straddling / decided / on_edge are bool[n, N - 1]; margin and bound are float64 (for
    reports; the decision itself is taken on the rationals).  `decided` is True for every pair that does not straddle."""


def exact_verdict(lats, longs, shape, plat, plong):
    lats, longs, plat, plong = _f32(lats), _f32(longs), _f32(plat), _f32(plong)
    n, e = len(plat), max(len(lats) - 1, 0)
    r = Exact()
    r.straddling = (edge_mask(lats, shape)[None, :] & straddles(longs, plong)) if e else np.zeros((n, 0), bool)
    r.toggles, r.on_edge = np.zeros((n, e), bool), np.zeros((n, e), bool)
    r.decided = ~r.straddling
    r.margin, r.bound = np.full((n, e), np.nan), np.full((n, e), np.nan)
    q = {}

    def frac(v):
        v = float(v)
        if v not in q:
            q[v] = Fraction(v) if np.isfinite(v) else None
        return q[v]

    for i, p in zip(*np.nonzero(r.straddling)):
        lat, x = frac(plat[i]), frac(plong[i])
        lat1, lat2, long1, long2 = frac(lats[p]), frac(lats[p + 1]), frac(longs[p]), frac(longs[p + 1])
        if None in (lat, x, lat1, lat2, long1, long2):
            continue
        dlat, dx, dlong = lat2 - lat1, x - long1, long2 - long1   # (dlong != 0: the edge straddles)
        prod = dlat * dx
        quot = prod / dlong
        t = quot + lat1
        margin, bound = abs(lat - t), _EPS8 * (abs(quot) + abs(lat1))
        r.toggles[i, p], r.on_edge[i, p] = lat < t, margin == 0
        r.margin[i, p], r.bound[i, p] = float(margin), float(bound)
        in_range = all(abs(v) < _FLT_MAX_Q for v in (dlat, dx, dlong, prod, quot, t)) and \
            all(v == 0 or abs(v) >= _FLT_MIN_Q for v in (prod, quot))
        r.decided[i, p] = in_range and margin > bound
    return r


def main_points(points, valid, index):
    """(lat, long, ok) of every entry of a main-table column read through the index vector"""
    points = _f32(points).reshape(-1, 2)
    rows = np.asarray(index, np.int64)
    ok = np.ones(len(rows), bool) if valid is None else np.asarray(valid, bool)[rows]
    return points[rows, 0], points[rows, 1], ok


def joined_points(rids, base, batches, last, default):
    """rids: (batchID, index) per entry; batches: None (constant batch) or (points, valid or None); default: (lat, long) or None"""
    n = len(rids)
    lat, lng, ok = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, bool)
    for i, (b, x) in enumerate(rids):
        if b == 0 or not (b - base < len(batches) - 1 or x < last):
            continue
        batch = batches[b - base]
        if batch is None:
            if default is not None:
                lat[i], lng[i], ok[i] = default[0], default[1], True
            continue
        pts, valid = batch
        lat[i], lng[i] = _f32(pts).reshape(-1, 2)[x]
        ok[i] = True if valid is None else bool(valid[x])
    return lat, lng, ok


def predicate_words(toggles, shape, total_words, ok, in_or_out, prefill=None):
    """uint32[n, total_words] after GeoBatchIntersects, from the per-edge verdicts of the valid entries"""
    n = len(ok)
    shape = np.asarray(shape, np.uint8)
    words = np.zeros((n, total_words), np.uint32) if prefill is None else np.array(prefill, np.uint32).reshape(n, total_words)
    edge_shape = shape[:-1] if len(shape) else shape
    for s in np.unique(edge_shape):
        parity = (np.count_nonzero(toggles[:, edge_shape == s], axis=1) & 1).astype(np.uint32)
        words[:, int(s) >> 5] ^= np.where(ok, parity << np.uint32(int(s) & 31), 0).astype(np.uint32)
    if len(shape) >= 2 and shape[0] == shape[1]:
        words[~np.asarray(ok, bool)] = 0 if in_or_out else 1
    return words


def first_shape(words):
    """int64[n]: the first set bit of each entry's words read as an int8 (128..255 wrap negative), -1 when none is set"""
    words = np.asarray(words, np.uint32)
    out = np.full(len(words), -1, np.int64)
    for w in range(words.shape[1] - 1, -1, -1):
        col = words[:, w].astype(np.int64)
        low = col & -col
        bit = np.zeros(len(col), np.int64)
        for k in range(32):
            bit[low == (1 << k)] = k
        out = np.where(col != 0, w * 32 + bit, out)
    return np.where(out >= 128, out - 256, out)


def compact(words, in_or_out, index, rids):
    """(kept count, compacted index vector, compacted RecordID vectors)"""
    keep = (first_shape(words) < 0) != bool(in_or_out)
    return int(keep.sum()), np.asarray(index)[keep], [np.asarray(r)[keep] for r in rids]


def shape_dim(words):
    """(values uint8, validity uint8) WriteGeoShapeDim writes: compacted, in entry order"""
    s = first_shape(words)
    s = s[s >= 0]
    return s.astype(np.uint8), np.ones(len(s), np.uint8)


def run(lats, longs, shape, total_words, plat, plong, ok, in_or_out, index, rids=(), prefill=None, verdict=f32_verdict):
    """the whole of GeoBatchIntersects + WriteGeoShapeDim for resolved entry points"""
    toggles = verdict(lats, longs, shape, plat, plong)
    words = predicate_words(toggles, shape, total_words, ok, in_or_out, prefill)
    kept, idx, rr = compact(words, in_or_out, index, rids)
    values, nulls = shape_dim(words)
    return {"pred": words, "kept": kept, "index": idx, "rids": rr, "dim_values": values, "dim_nulls": nulls}
