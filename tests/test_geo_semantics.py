"""GeoBatchIntersects and WriteGeoShapeDim against the independent model of tests/geo_model.py, on the smallest inputs at which
each mechanism of geo_intersect_kernel<W> / geo_shape_dim_kernel can fail: rings that end on, one before and one past a 64-edge
chunk (the 65th longitude bit, ring separators and shape changes at lanes 0 and 63, a chunk without an edge), test longitudes
equal to vertex longitudes, points on vertices and on edges, degenerate edges, +-0.0, denormal / huge / inf / NaN coordinates,
every TotalWords the four template instances take with shapes 128..255, null points against batches with and without a first
edge, the entry counts around a wavefront, a block and a dimension tile, and the second round of both kernels' loops.

Except for the specials pool every coordinate is a multiple of 1/4 with |c| <= 16: there the float32 evaluation is exact, so
every off-edge pair is decided by exact arithmetic alone.  On the CPU the model is checked against itself (exact against float32
wherever decided), its undecided share is bounded, and it is pinned bit for bit to the C checker and the reference's host build;
on the GPU the HIP library is compared with the model bit for bit, with main-table and joined points."""
import ctypes as C

import numpy as np
import pytest

import geo_model as G
import harness as H
from aresdb_amd import abi
from test_edge_semantics import CPU, _cpu_backend

FLT_MAX = G.FLT_MAX
SEAM_EDGES = (63, 64, 65, 66, 127, 128, 129, 200)
ENTRY_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
GRID_STRIDE_N = 524288 + 257      # geo_intersect_kernel: 2048 blocks x 256 entries, then the second grid-stride iteration
TICKET_ROUND_N = 2049 * 1024 + 1  # geo_shape_dim_kernel: 2050 tiles of 1024 for 2048 blocks, a look-back over 2049 tiles
FILL_SEEDS = range(20)
UNDECIDED_CAP = 0.001


class Case:
    """One call of GeoBatchIntersects + WriteGeoShapeDim.  Points come from a main-table column (points, valid, index) or, when
    `joined` is set, through RecordIDs: joined = (rids, base, batches, last, default) as geo_model.joined_points takes them."""

    def __init__(self, name, lats, longs, shape, words, points, valid=None, index=None, in_or_out=True, prefill=None, rids=0,
                 joined=None, starting_index=3):
        self.name, self.words, self.in_or_out = name, words, bool(in_or_out)
        self.lats, self.longs, self.shape = np.float32(lats), np.float32(longs), np.uint8(shape)
        assert len(self.lats) == len(self.longs) == len(self.shape)
        assert not len(self.shape) or int(self.shape.max()) < 32 * words   # (geo_model.UNDEFINED)
        self.points = np.float32(points).reshape(-1, 2)
        self.valid = None if valid is None else np.asarray(valid, bool)
        self.starting_index = starting_index if valid is not None else 0
        self.joined = joined
        self.index = np.arange(len(self.points) if joined is None else len(joined[0]), dtype=np.uint32) if index is None \
            else np.asarray(index, np.uint32)
        self.n = len(self.index)
        rng = np.random.default_rng(self.n + 7 * rids)
        self.rids = [H.record_id_array(list(zip(rng.integers(-5, 5, self.n).tolist(), rng.integers(0, 1000, self.n).tolist())))
                     for _ in range(rids)]
        self.prefill = None if prefill is None else np.asarray(prefill, np.uint32).reshape(self.n, words)

    def __repr__(self):
        return f"{self.name}(N={len(self.lats)}, W={self.words}, n={self.n}, in={self.in_or_out}, {'joined' if self.joined else 'main'})"

    def entry_points(self):
        if self.joined is None:
            return G.main_points(self.points, self.valid, self.index)
        return G.joined_points(*self.joined)

    def model(self, verdict=G.f32_verdict):
        plat, plong, ok = self.entry_points()
        return G.run(self.lats, self.longs, self.shape, self.words, plat, plong, ok, self.in_or_out, self.index,
                     [r.view(np.uint64) for r in self.rids], self.prefill, verdict)

    def with_(self, name=None, **kw):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(kw)
        c.name = name or self.name
        return c

    def as_joined(self):
        """the same entries through a join: the column split into two batches behind RecordIDs, after a constant batch"""
        assert self.joined is None
        half = len(self.points) // 2
        parts = [(self.points[:half], None if self.valid is None else self.valid[:half]),
                 (self.points[half:], None if self.valid is None else self.valid[half:])]
        base = -7
        rids = [(base + 1, int(r)) if r < half else (base + 2, int(r) - half) for r in self.index]
        return self.with_(self.name + "/joined", joined=(rids, base, [None] + parts, len(self.points) - half, None))

    def run(self, be):
        shapes = H.GeoShapes(be, self.lats, self.longs, self.shape, 32 * self.words)
        keep = [shapes]
        idx = H.Buf(be, self.index)
        rid_bufs = [H.Buf(be, r) for r in self.rids]
        vecs = (C.c_void_p * max(len(rid_bufs), 1))(*[b.ptr for b in rid_bufs])
        pred = H.Buf(be, self.prefill) if self.prefill is not None else H.Buf(be, nbytes=4 * self.n * self.words)
        if self.joined is not None:
            rids, base, batches, last, default = self.joined
            slices = (abi.VectorPartySlice * len(batches))()
            for b, batch in enumerate(batches):
                if batch is None:
                    slices[b].BasePtr, slices[b].DataType = None, abi.GeoPoint
                    continue
                col = H.geo_column(be, batch[0], valid=batch[1], starting_index=5 if batch[1] is not None else 0)
                keep.append(col)
                slices[b] = col.vp
            point_rids = H.Buf(be, H.record_id_array(rids))
            keep.append(point_rids)
            iv = abi.InputVector()
            f = iv.Vector.ForeignVP
            f.RecordIDs, f.Batches = point_rids.ptr, C.addressof(slices)
            f.BaseBatchID, f.NumBatches, f.NumRecordsInLastBatch = base, len(batches), last
            f.TimezoneLookup, f.TimezoneLookupSize, f.DataType = None, 0, abi.GeoPoint
            f.DefaultValue.HasDefault = default is not None
            if default is not None:
                f.DefaultValue.Value.GeoPointVal.Lat, f.DefaultValue.Value.GeoPointVal.Long = float(default[0]), float(default[1])
            iv.Type = abi.ForeignColumnInput
        else:
            col = H.geo_column(be, self.points, valid=self.valid, starting_index=self.starting_index)
            keep.append(col)
            iv = col.input()
        kept = be.call("GeoBatchIntersects", shapes.struct(), iv, idx.ptr, self.n, 0, C.addressof(vecs) if rid_bufs else None,
                       len(rid_bufs), pred.ptr, self.in_or_out, None, 0)
        dim = H.Buf(be, nbytes=2 * self.n + 16)
        dv = abi.DimensionOutputVector()
        dv.DimValues, dv.DimNulls, dv.DataType = dim.ptr, dim.ptr + self.n + 8, abi.Uint8
        be.call("WriteGeoShapeDim", self.words, dv, self.n, pred.ptr, None, 0)
        be.wait()
        res = {"kept": kept, "pred": pred.read(np.uint32, self.n * self.words).reshape(self.n, self.words),
               "index": idx.read(np.uint32, max(kept, 0)), "rids": [b.read(np.uint64, max(kept, 0)) for b in rid_bufs],
               "dim_values": dim.read(np.uint8, self.n), "dim_nulls": dim.read(np.uint8, self.n, self.n + 8)}
        for b in keep + [idx, pred, dim] + rid_bufs:
            b.free()
        return res

    def check(self, be, want=None):
        """predicate words, kept count, index vector, RecordID vectors, dimension values and validity (and nothing written past
        the last dimension value)"""
        want, got = want or self.model(), self.run(be)
        tag = f"{self!r} on {be.name}"
        bad = np.flatnonzero((got["pred"] != want["pred"]).any(axis=1))
        assert not len(bad), (tag, "pred", bad[:5], got["pred"][bad[:5]], want["pred"][bad[:5]])
        assert got["kept"] == want["kept"], (tag, "kept", got["kept"], want["kept"])
        assert np.array_equal(got["index"], want["index"]), (tag, "index")
        for t, (g, w) in enumerate(zip(got["rids"], want["rids"])):
            assert np.array_equal(g, w), (tag, "rids", t)
        inside = len(want["dim_values"])
        for key in ("dim_values", "dim_nulls"):
            full = np.zeros(self.n, np.uint8)
            full[:inside] = want[key]
            assert np.array_equal(got[key], full), (tag, key, inside)
        return want


# ---- polygons ------------------------------------------------------------------------------------------------------------
def ring(xs, ys, s):
    """a closed ring of shape s over the given vertices: (lats, longs, shape numbers), the first vertex repeated at the end"""
    xs, ys = list(xs) + [xs[0]], list(ys) + [ys[0]]
    return ys, xs, [s] * len(xs)


def batch(*parts):
    lats, longs, shape = [], [], []
    for la, lo, sh in parts:
        lats += list(la)
        longs += list(lo)
        shape += list(sh)
    return np.float32(lats), np.float32(longs), np.uint8(shape)


def square(s, half, cx=0.0, cy=0.0, x0=None, x1=None):
    x0, x1 = cx - half if x0 is None else x0, cx + half if x1 is None else x1
    return ring([x0, x1, x1, x0], [cy - half, cy - half, cy + half, cy + half], s)


ROTATE = 10   # a comb starts ten vertices before its closing edge ends, so that no 64th edge is the closing one


def comb(edges, s=0, offset=0, xshift=0.0):
    """A ring of `edges` edges on the 1/4 grid: teeth of three heights over a sweep to the right and, for rings of more than
    100 edges, a sweep back to the left; the last edge of the cycle closes it along the bottom (latitude -16), and the ring
    starts ROTATE vertices before the cycle does.  Every edge covers a longitude interval of its own within its sweep, 1/4 of
    a degree wide, 1/2 within two edges of every 64th edge of the batch (the ring starts at batch point `offset`).  There the
    sweep stands on a high base and the other sweep on a low one, so those edges are the topmost of their meridians: a
    point right under one of them is crossed by that edge alone.  `xshift` moves the ring along the longitude axis."""
    chain = edges - 1
    per = chain if chain <= 100 else (chain + 1) // 2           # edges of the first sweep
    near = [min(abs(((i + ROTATE) % edges) + offset - k) for k in range(0, edges + offset + 64, 64)) for i in range(edges)]
    wide = [near[i] <= 2 and near[(i + 1) % edges] <= 2 or near[i] <= 1 for i in range(edges)]   # of cycle edge i
    width = sum(0.5 if wide[i] else 0.25 for i in range(per))
    xs, ys, x = [], [], xshift - 0.25 * round(2 * width)
    for i in range(edges):
        xs.append(x)
        if i < chain:
            x += (0.5 if wide[i] else 0.25) * (1 if i < per else -1)
        ys.append(-16.0 if i in (0, chain) else (8.0 if near[i] <= 3 else -8.0) + (2.0 + i % 3) * (i % 2))
    xs, ys = xs[-ROTATE:] + xs[:-ROTATE], ys[-ROTATE:] + ys[:-ROTATE]
    return ring(xs, ys, s)


def spring(edges, s=0):
    """a ring of `edges` edges every one of which straddles the meridians near 0: a zigzag between two longitudes that climbs
    1/4 of a degree of latitude every second edge (so every other edge has lat1 == lat2), closed by one long edge"""
    xs = [(-1) ** j * (2.0 + 0.25 * (j % 7)) for j in range(edges)]
    ys = [-16.0 + 0.25 * (j // 2) for j in range(edges)]
    return ring(xs, ys, s)


def grid_points(x0, x1, y0, y1, step=0.25):
    xs, ys = np.arange(x0, x1 + step / 2, step), np.arange(y0, y1 + step / 2, step)
    return np.stack([np.repeat(ys, len(xs)), np.tile(xs, len(ys))], 1).astype(np.float32)


def seam_points(lats, longs, shape, aim=()):
    """from a 1/4 x 1/2 grid over the batch: for every 64th edge of the batch, its predecessor and the edges of `aim` the points
    that edge alone crosses, every grid point on the meridian of the vertex between the two, and every 29th point of the rest"""
    cand = grid_points(-16, 16, -16, 16)
    cand = cand[(cand[:, 0] * 2) % 1 == 0]
    t = G.f32_verdict(lats, longs, shape, cand[:, 0], cand[:, 1])
    single = t.sum(1) == 1
    picks = set(range(0, len(cand), 29))
    for seam in range(64, len(lats) - 1 + 64, 64):
        for e in (seam - 1, seam):
            if e < t.shape[1]:
                picks.update(np.flatnonzero(single & t[:, e])[:3].tolist())
        if seam < len(longs) and longs[seam] < FLT_MAX:
            picks.update(np.flatnonzero(cand[:, 1] == longs[seam])[::5].tolist())
    for e in aim:
        picks.update(np.flatnonzero(single & t[:, e])[:3].tolist())
        picks.update(np.flatnonzero(cand[:, 1] == longs[e])[::7].tolist())
    return cand[sorted(picks)]


def some_nulls(n, period=11):
    return np.arange(n) % period != 4


# ---- the named cases -----------------------------------------------------------------------------------------------------
# (name, edges of the first ring, longitude of a separator after it or None, shape of the second ring): where the first ring
# ends decides which lane holds the separator or the shape change.  The first ring's points are 0 .. edges.  A separator is any
# point whose latitude is FLT_MAX: the "sepx" ones carry an ordinary longitude, so that an edge wrongly drawn to or from them
# would cross test meridians at finite latitudes.
JOINTS = [(f"{kind}_at_{first + 1}", first, x, 0) for first in (62, 63, 64, 126, 127) for kind, x in (("sep", FLT_MAX), ("sepx", -6.0))] + \
    [(f"change_{first}_{first + 1}", first, None, 1) for first in (63, 64, 127, 128)]


def joint_case(name, first, separator, second_shape):
    """two combs in a row, far apart in longitude: the first ends at batch point `first`; then a separator and a second ring of
    the same shape, or at once a ring of another shape.  c.non_edges are the one or two point pairs across the joint that form
    no edge; c.aimed the real edges on either side of them, each the only crossing of some test point."""
    start = first + (1 if separator is None else 2)
    parts = [comb(first, 0, xshift=4.0)] + ([] if separator is None else [([FLT_MAX], [separator], [0])]) + \
        [comb(20, second_shape, offset=start, xshift=-12.5)]
    b = batch(*parts)
    c = Case("seam_" + name, *b, 1, seam_points(*b, aim=(first - 1, start)), in_or_out=first % 2 == 0)
    c.non_edges, c.aimed = list(range(first, start)), [first - 1, start]
    return c


def seam_cases():
    out = []
    for e in SEAM_EDGES:
        for kind, make in (("comb", comb), ("spring", spring)):
            b = batch(make(e))
            pts = seam_points(*b)
            out.append(Case(f"seam_{kind}_{e}", *b, 1, pts, valid=some_nulls(len(pts)), in_or_out=e % 2 == 0))
    for e in (65, 129):
        for lead in range(4):   # the chunk seams move along the ring; the batch ends 1 .. 4 edges into its last chunk
            b = batch(([12.0 + 0.25 * k for k in range(lead)], [-3.0 + 1.5 * k for k in range(lead)], [0] * lead), comb(e, 1, offset=lead))
            out.append(Case(f"seam_comb_{e}_lead{lead}", *b, 1, seam_points(*b), in_or_out=lead % 2 == 0))
    out += [joint_case(*j) for j in JOINTS]
    # a chunk that holds no edge at all: 64 one-point shapes, then a square
    lone = ([0.25 * k - 8 for k in range(64)], [0.5 * (k % 9) - 2 for k in range(64)], list(range(64)))
    b = batch(lone, square(64, 2.0))
    out.append(Case("no_edge_chunk", *b, 3, grid_points(-3, 3, -3, 3, 0.5), valid=some_nulls(169)))
    return out


def half_open_batch():
    return batch(
        # 0: concave, with local longitude extremes (4, -4), pass-through vertices (0, +-2), vertical and horizontal edges
        ring([-4, 0, 4, 4, 2, 0, -4, -4], [-4, -2, -4, 4, 1, 2, 4, 0], 0),
        # 1: 45-degree edges; 2: slopes 3/4 (exact quotient) and 1/3, 2/3 (inexact)
        ring([0, 3, 0, -3], [-3, 0, 3, 0], 1), ring([-4, 0, 3, 4], [-3, 0, 1, 3], 2),
        # 3: a repeated vertex (long1 == long2 and lat1 == lat2) and a vertical edge; 4: zero area, there and back
        ring([-2, -2, 2, 2, 2], [-1, -1, -1, 3, 3], 3), ring([-3, 1, 4, 1], [2, 2.5, 4, 2.5], 4),
        # 5: -0.0 and +0.0 as vertex coordinates, on both axes
        ring([-0.0, 2, 2, 0.0], [-0.0, 0.0, 2, 2], 5),
        # 6: two rings behind a separator, the inner one a hole
        square(6, 3.0), ([FLT_MAX], [FLT_MAX], [6]), square(6, 1.0))


def half_open_cases():
    b = half_open_batch()
    pts = np.concatenate([grid_points(-5, 5, -5, 5), np.float32([[-0.0, -0.0], [-0.0, 0.0], [0.0, -0.0], [1.0, -0.0], [-0.0, 1.0],
                                                                 [-0.0, 2.0], [2.0, -0.0]])])
    return [Case("half_open", *b, 1, pts, in_or_out=True), Case("half_open_out", *b, 1, pts, valid=some_nulls(len(pts)), in_or_out=False)]


SPECIALS = np.float32([0.0, -0.0, 1e-40, -1e-40, 1e-45, 0.5, 1.0, -1.0, 3.0, 1e30, -1e30, 3e38, FLT_MAX, np.inf, -np.inf, np.nan])


def specials_cases():
    """float32 alone decides these: the exact side leaves non-finite, overflowing and denormal evaluations open"""
    d, h, inf, nan = 1e-40, 1e30, np.inf, np.nan
    b = batch(ring([-d, d, d, -d], [-d, -d, d, d], 0), ring([-h, h, h, -h], [-h, -h, h, h], 1),   # denormal; the product overflows
              ring([-2, 2, nan, -2], [-2, -2, 2, 2], 2), ring([-2, inf, 2, -2], [-2, -2, 2, 2], 3), ring([-inf, 2, 2, -2], [-2, -2, 2, 2], 4),
              ring([-2, 2, 2, -2], [-inf, -2, 2, 2], 5), ring([-2, 2, 2, -2], [-2, -2, inf, 2], 6), ring([-2, 2, 2, -2], [-2, nan, 2, 2], 7),
              ring([-2, 2, 2, -2], [-2, -2, FLT_MAX, 2], 8), ring([-h, 2, h], [-1, 3e38, -1], 9), ring([-1, 1, 0.5], [-h, -h, d], 10))
    pts = np.stack([np.repeat(SPECIALS, len(SPECIALS)), np.tile(SPECIALS, len(SPECIALS))], 1)
    return [Case("specials", *b, 1, pts, in_or_out=True),
            Case("specials_out", *b, 1, pts, valid=some_nulls(len(pts), 7), in_or_out=False)]


NESTED = (0, 31, 32, 63, 64, 127, 128, 255)   # shape numbers of the nested squares, innermost first


def nested_batch(words):
    parts = []
    for k, s in enumerate(NESTED):
        if s < 32 * words:   # 255 stops short at longitude 5.5: (0, 5.75) is inside {127, 128} only
            parts.append(square(s, k + 1.0, x1=5.5) if s == 255 else square(s, k + 1.0))
    return batch(*parts)


def words_cases():
    out = []
    pts = np.concatenate([grid_points(-9, 9, 0, 0), grid_points(-9, 9, 0.25, 0.25, 0.5), grid_points(-9, 9, 7.5, 8.25, 0.75),
                          np.float32([[0, 0], [0, -6.5], [0, 5.75], [0, 6.5], [0, -7.5]])])
    n = len(pts)
    rng = np.random.default_rng(255)
    for words in (1, 2, 3, 4, 5, 8):
        b = nested_batch(words)
        for in_or_out in (True, False):
            plain = Case(f"words_{words}", *b, words, pts, valid=some_nulls(n, 13), in_or_out=in_or_out, rids=1)
            out.append(plain)
            out.append(plain.with_(f"words_{words}_prefill", prefill=rng.integers(0, 2 ** 32, (n, words), dtype=np.uint64).astype(np.uint32)))
            # the XOR clears every word of the even entries back to zero
            clear = np.where((np.arange(n) % 2 == 0)[:, None], plain.model()["pred"], np.uint32(1 << 5)).astype(np.uint32)
            out.append(plain.with_(f"words_{words}_prefill_clears", prefill=clear))
            if words >= 5:   # the only bit already set is one that reads as "no shape"
                high = np.zeros((n, words), np.uint32)
                high[:, 4] = 1 << 3
                out.append(plain.with_(f"words_{words}_prefill_high", prefill=high))
    return out


def null_cases():
    sq = square(0, 2.0)
    batches = {"first_edge": batch(sq), "lone_first": batch(([9.0], [9.0], [0]), square(1, 2.0)),
               "separator_first": batch(([FLT_MAX, FLT_MAX], [FLT_MAX, FLT_MAX], [0, 0]), square(0, 2.0)),
               "N0": batch(), "N1": batch(([1.0], [1.0], [0])), "N2_same": batch(([-1.0, 1.0], [-1.0, 2.0], [1, 1])),
               "N2_differ": batch(([-1.0, 1.0], [-1.0, 2.0], [0, 1]))}
    pts = np.float32([[0, 0], [1, 1], [5, 5], [0, 0], [1.5, -1.5], [2, 2], [0, 3], [-1, 0.25], [0.5, 0.5]])
    valid = np.array([1, 0, 1, 0, 1, 1, 0, 1, 0], bool)
    base = 40
    # RecordIDs: batch id 0, the last batch past its record count, a batch past the last past that count, a constant batch
    rids = [(base + 1, 0), (0, 1), (base + 1, 2), (base + 2, 3), (base + 2, 2), (base, 0), (base + 3, 7), (base + 1, 7), (base + 1, 3), (0, 0)]
    parts = [None, (pts, valid), (pts, None)]
    out = []
    for name, b in batches.items():
        for in_or_out in (True, False):
            for pre in (False, True):
                tag = f"null_{name}{'_prefill' if pre else ''}"
                fill = (lambda n: np.random.default_rng(n).integers(0, 2 ** 32, (n, 2), dtype=np.uint64).astype(np.uint32) if pre else None)  # noqa: E731
                out.append(Case(tag, *b, 2, pts, valid=valid, in_or_out=in_or_out, prefill=fill(len(pts)), rids=1))
                for default in (None, (0.5, 0.5)):
                    out.append(Case(f"{tag}_joined{'_default' if default else ''}", *b, 2, pts, in_or_out=in_or_out, prefill=fill(len(rids)),
                                    joined=(rids, base, parts, 3, default), rids=2))
    return out


PATTERN = np.float32([[0, 0], [2, 2], [-2, 2], [2, -2], [-2, -2], [0, 2], [0, -2], [2, 0], [-2, 0], [3, 0], [0, 3], [1.75, 1.75], [-1.75, 0.25]] +
                     [[0.25 * (k % 19) - 2.25, 0.25 * (k % 23) - 2.75] for k in range(51)])   # 64 points: vertices, edges, in, out
PATTERN_VALID = np.arange(64) % 9 != 5


def entry_case(n, style, rids, in_or_out=True, words=1):
    rng = np.random.default_rng(n)
    rows = 2 * n if style == "subset" else n
    index = {"identity": np.arange(n), "perm": rng.permutation(n),
             "subset": np.sort(rng.choice(rows, n, replace=False))}[style].astype(np.uint32)
    return Case(f"entries_{n}_{style}", *batch(square(0, 2.0)), words, np.resize(PATTERN, (rows, 2)), valid=np.resize(PATTERN_VALID, rows),
                index=index, in_or_out=in_or_out, rids=rids)


def entry_cases():
    """every entry count with every index style; the number of RecordID vectors takes all of 0, 1, 2 for each count and for each style"""
    return [entry_case(n, style, (k + j) % 3, in_or_out=(k + j) % 2 == 0)
            for k, n in enumerate(ENTRY_COUNTS) for j, style in enumerate(("identity", "subset", "perm"))]


def fill_case(seed):
    """random float32 polygons of 3 - 40 vertices, radii drawn per vertex (concave), x 500 random points, one of them on a vertex"""
    rng = np.random.default_rng(seed)
    parts = []
    for s in range(int(rng.integers(1, 4))):
        k = int(rng.integers(3, 41))
        ang, rad = np.sort(rng.uniform(0, 2 * np.pi, k)), rng.uniform(3, 40, k)
        cx, cy = rng.uniform(-30, 30, 2)
        parts.append(ring(np.float32(cx + rad * np.cos(ang)).tolist(), np.float32(cy + rad * np.sin(ang)).tolist(), s))
    b = batch(*parts)
    pts = rng.uniform(-60, 60, (500, 2)).astype(np.float32)
    j = int(rng.integers(0, len(b[0])))   # one point on a vertex: such pairs have margin 0 and count as undecided
    pts[int(rng.integers(0, 500))] = (b[0][j], b[1][j])
    return Case(f"fill_{seed}", *b, 1, pts, valid=rng.random(500) > 0.05, in_or_out=seed % 2 == 0, rids=seed % 3)


GROUPS = {"seams": seam_cases, "half_open": half_open_cases, "specials": specials_cases, "words": words_cases, "nulls": null_cases,
          "entries": entry_cases, "fill": lambda: [fill_case(s) for s in FILL_SEEDS]}
_built = {}


def cases_of(group, joined=True):
    """the group's cases, built once; with `joined`, each main-table case is followed by the same entries through a join"""
    if group not in _built:
        _built[group] = GROUPS[group]()
    out = []
    for c in _built[group]:
        out.append(c)
        if joined and c.joined is None and len(c.points) >= 2:
            out.append(c.as_joined())
    return out


def kernel_names(be):
    """launches by full kernel name, template arguments included"""
    return {k: v[0] for k, v in be.profiler_report().items()}


# ---- CPU: the inputs are what they are meant to be -----------------------------------------------------------------------
def _lone(t, e):
    """some point is crossed by edge e and by no other"""
    return bool(((t.sum(1) == 1) & t[:, e]).any())


def test_seam_inputs_reach_the_edges_they_are_aimed_at():
    seen = set()
    for c in cases_of("seams", joined=False):
        edges = G.edge_mask(c.lats, c.shape)
        if c.name == "no_edge_chunk":
            assert not edges[:64].any() and edges[64:].sum() == 4
            continue
        plat, plong, ok = c.entry_points()
        t = G.f32_verdict(c.lats, c.longs, c.shape, plat, plong)
        if hasattr(c, "non_edges"):   # a separator or a shape change at the named batch points, real edges on both sides of it
            at = [int(x) for x in c.name.split("_") if x.isdigit()]
            if "sep" in c.name:
                assert np.flatnonzero(c.lats == FLT_MAX).tolist() == at and len(set(c.shape.tolist())) == 1, c
            else:
                assert np.flatnonzero(np.diff(c.shape)).tolist() == at[:1] and not (c.lats == FLT_MAX).any(), c
            assert not edges[c.non_edges].any() and edges.sum() == len(edges) - len(c.non_edges), c
            for e in c.aimed:
                assert edges[e] and _lone(t, e), (c, e)
                assert (plong == c.longs[e]).sum() >= 3, (c, e)
            seen.update(p % 64 for p in c.non_edges)
            continue
        lead = int(c.name[-1]) if "lead" in c.name else 0
        want = int(c.name.split("_")[2])
        assert edges[lead:lead + want].all() and edges.sum() == want + max(lead - 1, 0) and len(edges) == lead + want, c
        if "comb" in c.name:   # both sides of every seam are the only crossing of some point; the seam vertex's meridian is used
            for seam in range(64, len(edges) + 64, 64):
                for e in (seam - 1, seam):
                    if lead <= e < len(edges):
                        assert _lone(t, e), (c, e)
                if seam < len(c.longs):
                    assert (plong == c.longs[seam]).sum() >= 3, (c, seam)
        else:                  # many edges of the ring cross one meridian
            assert t.sum(1).max() >= min(want, 64) // 2 - 2, (c, t.sum(1).max())
    assert {62, 63, 0, 1} <= seen   # a non-edge in lanes 62, 63 (its far end is the 65th longitude), 0 and 1
    assert {(len(c.lats) - 1) % 64 for c in cases_of("seams", joined=False)} >= {0, 1, 2, 3, 4, 63}


def test_word_and_null_inputs_cover_what_the_issue_names():
    seen = {}
    for c in cases_of("words", joined=False):
        if c.prefill is None and c.in_or_out:
            want = c.model()["pred"]
            seen[c.words] = {tuple(s for s in NESTED if s < 32 * c.words and w[s >> 5] >> (s & 31) & 1) for w in want}
    assert set(seen) == {1, 2, 3, 4, 5, 8}
    assert {NESTED, (128, 255), (127, 128)} <= seen[8] and (128,) in seen[5] and (127,) in seen[4]
    names = {c.name for c in cases_of("words", joined=False)}
    assert {"words_8_prefill_high", "words_5_prefill_high", "words_1_prefill_clears"} <= names
    for c in cases_of("nulls"):
        _, _, ok = c.entry_points()
        assert not ok.all() and ok.any(), c
    assert {len(c.lats) for c in cases_of("nulls")} >= {0, 1, 2}


# ---- CPU: the model against itself -----------------------------------------------------------------------------------------
def _accounting(cs):
    """(straddling pairs, undecided among them, undecided off-edge pairs, on-edge pairs); asserts exact == f32 wherever decided"""
    pairs = undecided = off_edge_open = on_edge = 0
    for c in cs:
        plat, plong, ok = c.entry_points()
        plat, plong = plat[ok], plong[ok]
        ex = G.exact_verdict(c.lats, c.longs, c.shape, plat, plong)
        f32 = G.f32_verdict(c.lats, c.longs, c.shape, plat, plong)
        assert not (f32 & ~ex.straddling).any(), c
        differ = ex.decided & (ex.toggles != f32)
        assert not differ.any(), (c, np.argwhere(differ)[:3])
        pairs += int(ex.straddling.sum())
        undecided += int((ex.straddling & ~ex.decided).sum())
        off_edge_open += int((ex.straddling & ~ex.decided & ~ex.on_edge).sum())
        on_edge += int(ex.on_edge.sum())
    return pairs, undecided, off_edge_open, on_edge


@pytest.mark.parametrize("group", ["seams", "half_open", "words", "nulls", "entries"])
def test_model_exact_and_float32_agree_on_the_grid(group):
    """every off-edge pair of the grid cases is decided, and decided pairs have one verdict"""
    pairs, undecided, off_edge_open, on_edge = _accounting(cases_of(group, joined=False))
    print(f"{group}: {pairs} straddling pairs, {on_edge} on an edge, {undecided} undecided, {off_edge_open} of them off-edge")
    assert pairs > 0 and off_edge_open == 0 and undecided == on_edge


def test_model_on_edge_points_of_exact_edges_do_not_toggle():
    """axis-parallel, 45-degree and power-of-two edges of the half-open batch: a point on such an edge is not below it"""
    c = cases_of("half_open", joined=False)[0]
    plat, plong, _ = c.entry_points()
    ex = G.exact_verdict(c.lats, c.longs, c.shape, plat, plong)
    f32 = G.f32_verdict(c.lats, c.longs, c.shape, plat, plong)
    dlat, dlong = np.diff(c.lats.astype(np.float64)), np.diff(c.longs.astype(np.float64))
    with np.errstate(all="ignore"):
        exact_edge = (dlat == 0) | (np.abs(dlat) == np.abs(dlong)) | (np.log2(np.abs(dlong)) % 1 == 0)
    on = ex.on_edge & exact_edge[None, :]
    assert on.sum() > 100 and not ex.toggles[on].any() and not f32[on].any()
    assert (ex.on_edge & ~exact_edge[None, :]).any()   # (inexact quotients are met too: float32 alone decides those)


def test_model_undecided_share_of_the_seeded_fill():
    pairs, undecided, _, _ = _accounting(cases_of("fill", joined=False))
    print(f"fill: {pairs} straddling pairs, {undecided} undecided ({undecided / pairs:.5%})")
    assert pairs > 40000 and undecided <= UNDECIDED_CAP * pairs


# ---- CPU: the model pinned to the C checker and the reference's host build --------------------------------------------------
@CPU
@pytest.mark.parametrize("group", list(GROUPS))
def test_model_is_the_checker_and_the_reference(which, group):
    be, ran = _cpu_backend(which), 0
    for c in cases_of(group):
        if which == "ref" and len(c.lats) == 0:   # (geo_model: the reference divides by the point count)
            continue
        c.check(be)
        ran += 1
    print(f"{which} {group}: {ran} compared calls")
    assert ran >= 2


# ---- GPU -----------------------------------------------------------------------------------------------------------------
INSTANCE = {1: "<1>", 2: "<2>", 3: "<4>", 4: "<4>", 5: "<8>", 8: "<8>"}


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_hip_geo_is_the_model(group):
    be, cs = H.hip_backend(), cases_of(group)
    be.profiler_enable(True)
    try:
        for c in cs:
            c.check(be)
        be.wait()
        ran = kernel_names(be)
    finally:
        be.profiler_enable(False)
    print(f"{group}: {len(cs)} compared calls; {ran}")
    for inst in set(INSTANCE.values()):
        assert ran.get("geo_intersect_kernel" + inst, 0) == sum(INSTANCE[c.words] == inst for c in cs), (inst, ran)
    assert ran.get("geo_shape_dim_kernel", 0) == len(cs), ran
    if group == "words":
        assert all(ran.get("geo_intersect_kernel" + i, 0) > 0 for i in ("<1>", "<2>", "<4>", "<8>")), ran


def _large(n, rids):
    c = Case(f"large_{n}", *batch(square(0, 2.0)), 1, np.resize(PATTERN, (n, 2)), valid=np.resize(PATTERN_VALID, n), rids=rids)
    want = c.model()
    assert 0 < want["kept"] < n and len(want["dim_values"]) == want["kept"]
    return c, want


@pytest.mark.gpu
def test_hip_intersect_second_grid_stride_iteration():
    """2048 blocks x 256 entries fill the capped grid once; 257 entries more are a second iteration with a ragged last block"""
    be = H.hip_backend()
    c, want = _large(GRID_STRIDE_N, 1)
    be.profiler_enable(True)
    try:
        c.check(be, want)
        ran = kernel_names(be)
    finally:
        be.profiler_enable(False)
    assert ran.get("geo_intersect_kernel<1>") == 1 and ran.get("geo_shape_dim_kernel") == 1, ran


@pytest.mark.gpu
def test_hip_shape_dim_second_ticket_round():
    """2050 tiles of 1024 entries for a grid of at most 2048 blocks: the ticket loop goes round again, and the last tile
    looks back over 2049 predecessors"""
    be = H.hip_backend()
    c, want = _large(TICKET_ROUND_N, 0)
    be.profiler_enable(True)
    try:
        c.check(be, want)
        ran = kernel_names(be)
    finally:
        be.profiler_enable(False)
    assert ran.get("geo_intersect_kernel<1>") == 1 and ran.get("geo_shape_dim_kernel") == 1, ran
