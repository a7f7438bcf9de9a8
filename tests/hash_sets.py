"""The chosen-hash inputs of HashReduce (one builder each, shared by the CPU tests and by every GPU path).

A builder returns a Program: batches of dimension rows, validity rows and raw measures whose 32-bit row hashes were CHOSEN —
the rows are computed from the hashes with hash_model.row_with_hash — and asserts, through the model's own murmur and before
anything touches a GPU, the property it is named for.  Raw measures are small integers; `measure_values` turns them into
the values of one aggregate so that every comparison is bit-exact: integer sums wrap like their type, float values are
multiples of 1/8 below 2^12 in magnitude, few enough per group for every partial sum to be exact in float32."""
import functools

import numpy as np

import hash_model as M
from aresdb_amd import abi

FULL = 0xFFFFFFFF
PART_BITS = (2, 3, 9)   # partition bits the tests force (ARES_MIN_PART_BITS); small inputs have 0 .. 3 by themselves
FLAG_PATTERNS = (1, 0, 0xFFFFFFFF, 0xFFFFFFFE, 0x40000000, 0x80000000, 0xC0000000, 0x3FFFFFFF, 0x7FFFFFFF)

# name -> (model aggregate, ABI aggregate, numpy type of the measure vector, value of raw measure m in [-2000, 2000])
AGGS = {
    "sum_u32": (("sum", "u32"), abi.AGGR_SUM_UNSIGNED, np.uint32, lambda m: (m + 2000) * 1000003),
    "sum_i32": (("sum", "i32"), abi.AGGR_SUM_SIGNED, np.int32, lambda m: m * 1000),
    "sum_i64": (("sum", "i64"), abi.AGGR_SUM_SIGNED, np.int64, lambda m: m * 1000),
    "min_u32": (("min", "u32"), abi.AGGR_MIN_UNSIGNED, np.uint32, lambda m: (m + 2000) * 1000003),
    "max_u32": (("max", "u32"), abi.AGGR_MAX_UNSIGNED, np.uint32, lambda m: (m + 2000) * 1000003),
    "min_i32": (("min", "i32"), abi.AGGR_MIN_SIGNED, np.int32, lambda m: m * 1000),
    "max_i32": (("max", "i32"), abi.AGGR_MAX_SIGNED, np.int32, lambda m: m * 1000),
    "sum_f32": (("sum", "f32"), abi.AGGR_SUM_FLOAT, np.float32, lambda m: m / 8),
    "sum_f64": (("sum", "f64"), abi.AGGR_SUM_FLOAT, np.float64, lambda m: m / 8),
    "min_f32": (("min", "f32"), abi.AGGR_MIN_FLOAT, np.float32, lambda m: m / 8),
    "max_f32": (("max", "f32"), abi.AGGR_MAX_FLOAT, np.float32, lambda m: m / 8),
    # {float32 average, uint32 count} in 8 bytes; the values depend on the group (Program.values)
    "avg": (("avg", "f32"), abi.AGGR_AVG_FLOAT, np.uint64, None),
}
MAX_ROWS_PER_GROUP = 4000  # 4000 x 2000 eighths < 2^24: every partial float32 sum is exact


def measure_values(raw, agg_name):
    return [AGGS[agg_name][3](m) for m in raw]


def pack_avg(pairs):
    """(average, count) pairs as the measure vector holds them"""
    f = np.array([p[0] for p in pairs], np.float32).view(np.uint32).astype(np.uint64)
    return f | (np.array([p[1] for p in pairs], np.uint64) << np.uint64(32))


def decode_value(agg_name, x):
    """a value read from the measure vector, as the model states it"""
    if agg_name != "avg":
        return x
    return (float(np.array([x & 0xFFFFFFFF], np.uint32).view(np.float32)[0]), x >> 32)


class Program:
    def __init__(self, name, widths, batches, hashes):
        self.name, self.widths = name, list(widths)
        self.nd = len(widths)
        self.ndw = tuple(sum(1 for w in widths if w == x) for x in (16, 8, 4, 2, 1))
        self.batches = batches   # [(rows, valids, raw measures)]
        self.hashes = hashes     # per batch: the hash every row was built for
        for (rows, valids, raw), hs in zip(batches, hashes):  # the rows do have the hashes they were built for
            assert len(rows) == len(valids) == len(raw) == len(hs)
            assert all(M.row_hash(r, o, self.widths) == h for r, o, h in zip(rows, valids, hs)), name
        per_group = {}
        for hs in hashes:
            for h in hs:
                per_group[h] = per_group.get(h, 0) + 1
        assert max(per_group.values()) <= MAX_ROWS_PER_GROUP
        # the reference's host map drops the key (hash 0, row 0) on extraction (its "unused" marker; the oracle restates
        # that): the hash-0 group never starts at the query's very first row here
        assert hashes[0][0] != 0
        self.distinct = len(per_group)

    def prefix(self, b):
        """rows, valids, raw measures of batches 0 .. b as one list each (what the query has seen after batch b)"""
        rows, valids, raw = [], [], []
        for r, o, m in self.batches[:b + 1]:
            rows += r
            valids += o
            raw += m
        return rows, valids, raw

    def flattened(self):
        """the same rows as ONE batch"""
        rows, valids, raw = self.prefix(len(self.batches) - 1)
        return Program(self.name + "/flat", self.widths, [(rows, valids, raw)], [[h for hs in self.hashes for h in hs]])

    def values(self, agg_name):
        """per batch, the measure values of aggregate `agg_name` ((average, count) pairs for avg: a group of one row gets
        (m / 8, 1), the rows of larger groups (0, 1 .. 3) — what the rolling average is exact for)"""
        if agg_name != "avg":
            return [measure_values(raw, agg_name) for _, _, raw in self.batches]
        count = {}
        for hs in self.hashes:
            for h in hs:
                count[h] = count.get(h, 0) + 1
        return [[(m / 8, 1) if count[h] == 1 else (0.0, 1 + m % 3) for m, h in zip(raw, hs)]
                for (_, _, raw), hs in zip(self.batches, self.hashes)]

    @functools.lru_cache(maxsize=None)
    def expected(self, agg_name, b=None):
        """the model's result after batch b (default: the last): ({key: value}, {hash: representative row})"""
        b = len(self.batches) - 1 if b is None else b
        rows, valids, _ = self.prefix(b)
        values = [v for vs in self.values(agg_name)[:b + 1] for v in vs]
        return M.groups_by_hash(rows, valids, values, AGGS[agg_name][0], self.widths)


def _raw(i):
    return (i * 37 + 11) % 4001 - 2000


def _ordinary(i):
    """the i-th of a fixed sequence of distinct, well spread hashes"""
    return (i * 2654435761 + 0x1234567) & FULL


class _Rows:
    """collects the rows of one batch"""

    def __init__(self, widths):
        self.widths = widths
        self.rows, self.valids, self.raw, self.hashes = [], [], [], []

    def add(self, h, others=None, valids=None, at=None):
        nd = len(self.widths)
        others = tuple(others) if others is not None else tuple(7 + d for d in range(1, nd))
        valids = tuple(valids) if valids is not None else (1,) * nd
        row = (M.row_with_hash(h, others, valids, self.widths),) + others
        at = len(self.rows) if at is None else at
        self.rows.insert(at, row)
        self.valids.insert(at, valids)
        self.hashes.insert(at, h)

    def batch(self, first_raw=0):
        self.raw = [_raw(first_raw + i) for i in range(len(self.rows))]
        return (self.rows, self.valids, self.raw)


def _program(name, widths, collected):
    batches, hashes, at = [], [], 0
    for c in collected:
        batches.append(c.batch(at))
        hashes.append(c.hashes)
        at += len(c.rows)
    return Program(name, widths, batches, hashes)


def _spread(hashes, reps):
    """every hash `reps` times, spread over the batch (each pass starts elsewhere)"""
    out = []
    for r in range(reps):
        k = (r * 5) % max(1, len(hashes))
        out += hashes[k:] + hashes[:k]
    return out


def sentinel_hashes(part_bits=PART_BITS):
    hs = list(FLAG_PATTERNS)
    families = {}
    for P in part_bits:
        kept = 32 - P
        for p in range(1 << P):
            hs += [p << kept, ((p + 1) << kept) - 1]                  # kept bits all 0 / all 1
        fam = [(p << kept) | (0x00ABCDE5 & ((1 << kept) - 1)) for p in range(1 << P)]  # differ in the partition bits only
        families[P] = fam
        hs += fam
        hs += [(1 << (kept - 1)) | 0x155, 0x155]                          # differ in the highest kept bit only
    seen, out = set(), []
    for h in hs:
        if h not in seen:
            seen.add(h)
            out.append(h)
    return out, families


@functools.lru_cache(maxsize=None)
def sentinels(variant="plain", widths=(4, 4), part_bits=(2, 3), reps=3):
    """variant: plain | first_last (the 0xFFFFFFFF rows are the batch's first and last rows) | prev (an earlier batch has
    left the 0xFFFFFFFF group, and a few others, in the previous result)"""
    hs, families = sentinel_hashes(part_bits)
    for P, fam in families.items():
        assert len({h >> (32 - P) for h in fam}) == 1 << P and len({h & ((1 << (32 - P)) - 1) for h in fam}) == 1
    assert set(FLAG_PATTERNS) <= set(hs)
    body = _spread(hs, reps)
    batches = []
    if variant == "first_last":
        body = [FULL] + [h for h in body if h != FULL] + [FULL]
        assert body[0] == body[-1] == FULL and FULL not in body[1:-1]
    elif variant == "prev":
        first = _Rows(widths)
        for h in [FULL, 0, 0x40000000] + [_ordinary(i) for i in range(5)] + [FULL]:
            first.add(h)
        batches.append(first)
    main = _Rows(widths)
    for h in body:
        main.add(h)
    batches.append(main)
    prog = _program(f"sentinels/{variant}/{'x'.join(map(str, widths))}/P{'_'.join(map(str, part_bits))}", widths, batches)
    assert prog.distinct == len(set(hs)) + (5 if variant == "prev" else 0)
    return prog


@functools.lru_cache(maxsize=None)
def collisions(widths=(4, 4)):
    """Different rows with one hash, in two batches: members of one quad, of one wavefront (256 consecutive rows), far apart,
    in different batches, and null-versus-valid pairs.  The representative must be the lowest row."""
    nd = len(widths)
    assert nd >= 2

    def others(k, null=False):
        return ((0 if null else 100 + k),) + tuple(9 for _ in range(2, nd)), ((1, 0) if null else (1, 1)) + (1,) * (nd - 2)

    first, second = _Rows(widths), _Rows(widths)
    for i in range(300):
        first.add(_ordinary(i))
    for i in range(600):
        second.add(_ordinary(200 + i))  # (a third of them are groups of the first batch)
    # (batch, position, hash, member number, null second dimension); positions are final: inserted in ascending order
    H1, H2, H3, H4, H5, H6, H7 = 0xDEADBEEF, 0x0BADF00D, 0xFFFFFFFF, 0x13572468, 0x40000000, 0x00000000, 0x7FFFFFFF
    plan = [
        (1, 8, H1, 0, False), (1, 9, H1, 1, False),                        # one quad
        (1, 70, H2, 0, False), (1, 100, H2, 1, False),                     # one wavefront, two quads
        (1, 5, H3, 0, False), (1, 300, H3, 1, False), (1, 612, H3, 2, False),  # a triple, far apart, at the empty marker's value
        (1, 40, H4, 0, True), (1, 41, H4, 1, False),                       # null first, then valid
        (1, 20, H5, 0, False), (1, 500, H5, 1, True),                      # valid first, then null
        (0, 10, H6, 0, False), (1, 200, H6, 1, False),                     # one member in the previous result, one in the batch
        (0, 150, H7, 0, False), (1, 3, H7, 1, False), (1, 4, H7, 2, True),  # the same with a triple
    ]
    for b, at, h, k, null in sorted(plan, key=lambda x: (x[0], x[1])):
        o, v = others(k, null)
        (first, second)[b].add(h, o, v, at=at)
    prog = _program(f"collisions/{'x'.join(map(str, widths))}", widths, [first, second])
    # the property: per hash the members are different rows, and the model's representative is the lowest of them
    for flat in (False, True):
        p = prog.flattened() if flat else prog
        rows, valids, _ = p.prefix(len(p.batches) - 1)
        _, rep = M.groups_by_hash(rows, valids, [0] * len(rows), ("sum", "u32"), widths)
        offset = len(prog.batches[0][0])
        for h in (H1, H2, H3, H4, H5, H6, H7):
            members = sorted((offset if b else 0) + at for b, at, hh, _, _ in plan if hh == h)
            keys = {(rows[i], valids[i]) for i in members}
            assert len(keys) == len(members) >= 2 and all(M.row_hash(rows[i], valids[i], widths) == h for i in members)
            assert rep[h] == members[0]
    return prog


CHAIN_TOP = 0xA  # the top 4 bits of every chain member: one partition for up to 4 partition bits


def chain_hashes(n, low13):
    return [(CHAIN_TOP << 28) | (j << 13) | low13 for j in range(n)]


@functools.lru_cache(maxsize=None)
def chains(dup=1, widths=(4, 4), long_chain=3000):
    """Distinct hashes equal in their low 13 bits (the generic tables' slot; the low 11 are the generated tables' bucket) and
    in their top 4 bits (the partition): a bucket exactly full (4) and one more (5), a chain of 300, and a chain of
    `long_chain` whose home is the LAST slot / bucket, so that it wraps to 0."""
    sets = [chain_hashes(4, 0x0123), chain_hashes(5, 0x0456), chain_hashes(300, 0x1000), chain_hashes(long_chain, 0x1FFF)]
    for s in sets:
        assert len(set(s)) == len(s) and len({h & 0x1FFF for h in s}) == 1 and len({h >> 28 for h in s}) == 1
    assert sets[3][0] & 0x1FFF == 0x1FFF and sets[3][0] & 0x7FF == 0x7FF
    hs = [h for s in sets for h in s]
    c = _Rows(widths)
    for h in _spread(hs, dup):
        c.add(h)
    prog = _program(f"chains/dup{dup}/{'x'.join(map(str, widths))}", widths, [c])
    assert prog.distinct == len(hs)
    return prog


NARROW_BASES = {"top": 0xFFFFE000, "bottom": 0x00000000, "middle": 0x5A5A5123}
NARROW_GROUPS = 7500  # more than kMergeLimit (7040) groups: one merge round cannot hold them


@functools.lru_cache(maxsize=None)
def narrow(where, dup=1, widths=(4, 4)):
    """NARROW_GROUPS distinct hashes inside 8192 consecutive hash values of one partition (for up to 9 partition bits)."""
    base = NARROW_BASES[where]
    rng = np.random.default_rng(8192)
    pick = set(rng.choice(8192, NARROW_GROUPS, replace=False).tolist())
    must = {0, 8191, 4095, 4096}  # the interval's ends, and the boundary between two rounds of 4096 values
    for m in must - pick:
        pick.remove(next(x for x in pick if x not in must))
        pick.add(m)
    hs = [base + k for k in sorted(pick)]
    assert len(hs) == NARROW_GROUPS > 7040 and hs[-1] - hs[0] == 8191 and hs[-1] <= FULL
    assert len({h >> 23 for h in hs}) == 1
    if where == "top":
        assert hs[-1] == FULL
    if where == "bottom":
        assert hs[0] == 0
    order = [hs[i] for i in rng.permutation(len(hs))]
    if order[0] == 0:
        order[0], order[1] = order[1], order[0]
    c = _Rows(widths)
    for h in _spread(order, dup):
        c.add(h)
    prog = _program(f"narrow/{where}/dup{dup}", widths, [c])
    assert prog.distinct == NARROW_GROUPS
    return prog


# Region A of a partition holds capA = ((2 * (rows / partitions) + 2 * 8192) | 63) + 18 records (make_regions), and a skewed
# input sends one record per row into ONE partition's region:
#   512 partitions (ARES_MIN_PART_BITS=9): capA = ((2 * (n / 512) + 16384) | 63) + 18 = 16529 for n in 16384 .. 32767
#     -> 12000 rows are absorbed (no overflow), 17000 rows overflow;
#   natural partition count: n <= 32768 has at most 4 partitions and capA >= n / 2 + 16384 >= n (never overflows);
#     n = 33000 has 8 partitions, capA = ((2 * 4125 + 16384) | 63) + 18 = 24657 < 33000 -> overflows.
SKEW_ABSORBED, SKEW_OVERFLOW_P9, SKEW_OVERFLOW_NATURAL = 12000, 17000, 33000


def region_a_capacity(rows, part_bits):
    return ((2 * (rows // (1 << part_bits)) + 2 * 8192) | 63) + 18


assert region_a_capacity(SKEW_ABSORBED, 9) > SKEW_ABSORBED and region_a_capacity(SKEW_OVERFLOW_P9, 9) < SKEW_OVERFLOW_P9
assert region_a_capacity(SKEW_OVERFLOW_NATURAL, 3) < SKEW_OVERFLOW_NATURAL and region_a_capacity(32768, 2) >= 32768

@functools.lru_cache(maxsize=None)
def narrow_crowded(widths=(4, 4)):
    """narrow("top") interleaved row by row with as many ordinary rows (1500 groups over all partitions): one partition holds
    more groups than a merge table while every scanning workgroup sees the same mix — the input of a DIRECT scan whose
    merge must hand the crowded partition to the multi-round merge."""
    crowded = narrow("top").hashes[0]
    filler = _spread([_ordinary(i) for i in range(1500)], 5)
    c = _Rows(widths)
    for a, b in zip(crowded, filler):
        c.add(b)
        c.add(a)
    prog = _program("narrow/crowded", widths, [c])
    assert prog.distinct == NARROW_GROUPS + 1500
    return prog


@functools.lru_cache(maxsize=None)
def images(widths=(4, 4)):
    """Three batches sized like a query whose result vectors are allocated once (the host grows them to 9/8 of what the
    first batch needs; a batch that fits leaves them — and the table image kept with them — in place): many rows and few
    groups first, then batches that bring sentinel rows for existing groups, a bucket chain that wraps to bucket 0 and grows
    from batch to batch, and rows that collide with groups of the previous result."""
    nd = len(widths)
    hs, _ = sentinel_hashes((2, 3))
    chain = chain_hashes(110, 0x1FFF)

    def other(k):
        return (k,) + tuple(9 for _ in range(2, nd))

    a, b, c = _Rows(widths), _Rows(widths), _Rows(widths)
    for h in _spread(hs, 8):
        a.add(h)
    for h in [FULL] + _spread(hs, 1) + chain[:60]:
        b.add(h)
    for k, h in enumerate([FULL, 0, 0x40000000, 0x80000000, chain[0]]):  # other rows with hashes the result already holds
        b.add(h, other(200 + k))
    b.add(FULL)
    for h in chain[40:] + _spread(hs, 1):
        c.add(h)
    for k, h in enumerate([FULL, chain[80], chain[59], 0x3FFFFFFF]):
        c.add(h, other(300 + k))
    prog = _program(f"images/{'x'.join(map(str, widths))}", widths, [a, b, c])
    sizes = [len(x.rows) for x in (a, b, c)]
    capacity = sizes[0] + sizes[0] // 8
    assert len(hs) + sizes[1] <= capacity and len(hs) + 60 + sizes[2] <= capacity  # no batch makes the host reallocate
    assert prog.distinct == len(hs) + 110
    return prog


SKEW_PARTITION = 0x155  # of 512: the top 9 bits of every skewed hash


def skew_hashes(n, first=0):
    """n distinct hashes of ONE partition (top 9 bits), their other 23 bits well spread (an odd multiplier is a bijection)"""
    return [(SKEW_PARTITION << 23) | (((first + i) * 0x9E3779B1 + 0x3039) & 0x7FFFFF) for i in range(n)]


@functools.lru_cache(maxsize=None)
def skew(n, batches=1, widths=(4, 4)):
    """All rows distinct, all in one partition.  batches = 3: an ordinary batch, the skewed one, another ordinary one (which
    shares groups with both)."""
    hs = skew_hashes(n)
    assert len(set(hs)) == n and len({h >> 23 for h in hs}) == 1
    collected = []
    if batches == 3:
        a = _Rows(widths)
        for h in _spread([_ordinary(i) for i in range(1000)], 3):
            a.add(h)
        collected.append(a)
    s = _Rows(widths)
    for h in hs:
        s.add(h)
    collected.append(s)
    if batches == 3:
        c = _Rows(widths)
        for h in _spread([_ordinary(500 + i) for i in range(1000)] + hs[:200], 2):
            c.add(h)
        collected.append(c)
    return _program(f"skew/{n}/b{batches}", widths, collected)


SKEW_LAZY = 16700  # > region_a_capacity(17900, 9) = 16529, and small enough to fit the vectors the first batch allocated


@functools.lru_cache(maxsize=None)
def skew_lazy(widths=(4, 4)):
    """Ordinary / ordinary / skewed / ordinary, sized like a query whose result vectors are allocated once (9/8 of what the
    first batch needs): under the DIRECT kernels the second batch is merged from the first one's table image and leaves the
    measure vector unwritten, so the skewed batch is tried — and declined — while the previous result's values are lazy."""
    a, b, c, d = (_Rows(widths) for _ in range(4))
    for h in _spread([_ordinary(i) for i in range(1000)], 16):
        a.add(h)
    for h in _spread([_ordinary(900 + i) for i in range(250)], 2):  # 100 groups of the first batch, 150 new ones
        b.add(h)
    hs = skew_hashes(SKEW_LAZY)
    for h in hs:
        c.add(h)
    for h in _spread([_ordinary(1100 + i) for i in range(150)] + hs[:50], 2):
        d.add(h)
    prog = _program("skew/lazy", widths, [a, b, c, d])
    capacity = len(a.rows) + len(a.rows) // 8
    assert 1000 + len(b.rows) <= capacity and 1150 + SKEW_LAZY <= capacity  # neither batch makes the host reallocate
    assert region_a_capacity(1150 + SKEW_LAZY, 9) < SKEW_LAZY
    return prog


def all_programs():
    """{name: builder} of every chosen-hash input (built on first use, then shared)"""
    return {
        "sentinels": lambda: sentinels("plain"),
        "sentinels_first_last": lambda: sentinels("first_last"),
        "sentinels_prev": lambda: sentinels("prev"),
        "sentinels_p9": lambda: sentinels("prev", part_bits=PART_BITS, reps=2),
        "sentinels_1d": lambda: sentinels("first_last", widths=(4,)),
        "sentinels_3d": lambda: sentinels("prev", widths=(4, 4, 4)),
        "sentinels_4d": lambda: sentinels("plain", widths=(4, 4, 4, 4)),
        "sentinels_4x2": lambda: sentinels("prev", widths=(4, 2)),
        "collisions": lambda: collisions(),
        "collisions_flat": lambda: collisions().flattened(),
        "collisions_4d": lambda: collisions((4, 4, 4, 4)),
        "collisions_4x2": lambda: collisions((4, 2)),
        "chains": lambda: chains(1),
        "chains_dup4": lambda: chains(4),
        "chains_4x2": lambda: chains(1, widths=(4, 2), long_chain=600),
        "narrow_top": lambda: narrow("top"),
        "narrow_bottom": lambda: narrow("bottom"),
        "narrow_middle": lambda: narrow("middle"),
        "narrow_top_dup2": lambda: narrow("top", dup=2),
        "narrow_crowded": lambda: narrow_crowded(),
        "images": lambda: images(),
        "images_3d": lambda: images((4, 4, 4)),
        "skew_absorbed": lambda: skew(SKEW_ABSORBED),
        "skew_overflow": lambda: skew(SKEW_OVERFLOW_P9),
        "skew_overflow_natural": lambda: skew(SKEW_OVERFLOW_NATURAL),
        "skew_three_batches": lambda: skew(SKEW_OVERFLOW_P9, batches=3),
        "skew_lazy": lambda: skew_lazy(),
    }
