"""The model of AresGeoShapeColumnRun (include/ares_extensions.h): the geofence verdict of every row of a batch as one byte of a
mode-2 Uint8 column.  It is tests/geo_model.py's GeoBatchIntersects over the identity index vector with predicate words that
start at zero, plus the contract of the entry point:

    s = first shape of the row's words, read as an int8 (shapes 128..255 read as none)
    row valid  iff  (s < 0) != inOrOut        -- the rows GeoBatchIntersects keeps
    value = s  when inOrOut and the row is valid, else 0

A row that fails a pruning hint (`keep` false) is (0, null).  A live row is one that passes every hint and has a valid point:
the rows whose polygon walk runs; the kernel walks them in wavefront-chunks of 64 per 1024-row tile."""
import numpy as np

import geo_model as G

TILE = 1024


def expected_column(lats, longs, shape, total_words, points, valid, in_or_out, keep=None):
    """(values uint8[n], row validity bool[n], live bool[n])"""
    points = np.float32(points).reshape(-1, 2)
    n = len(points)
    rows = np.arange(n, dtype=np.uint32)
    plat, plong, ok = G.main_points(points, valid, rows)
    words = G.run(lats, longs, shape, total_words, plat, plong, ok, in_or_out, rows)["pred"]
    s = G.first_shape(words)
    keep = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    row_valid = ((s < 0) != bool(in_or_out)) & keep
    values = np.where(row_valid & bool(in_or_out), s, 0).astype(np.uint8)
    return values, row_valid, ok & keep


def bitmap_bytes(n):
    return ((n + 7) // 8 + 63) // 64 * 64


def column_bytes(n):
    return bitmap_bytes(n) + (n + 63) // 64 * 64


def layout(values, row_valid):
    """(bitmap bytes, value bytes) as the entry point writes them: bits at or past n inside the last written 8-byte word are
    zero — and so is everything behind it in a buffer that started cleared"""
    n = len(values)
    bits = np.zeros(bitmap_bytes(n) * 8, bool)
    bits[:n] = row_valid
    return np.packbits(bits, bitorder="little"), np.asarray(values, np.uint8)


def chunks_walked(live):
    """sum over the 1024-row tiles of ceil(live rows of the tile / 64)"""
    live = np.asarray(live, bool)
    return int(sum((int(live[t:t + TILE].sum()) + 63) // 64 for t in range(0, len(live), TILE)))
