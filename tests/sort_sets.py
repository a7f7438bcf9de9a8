"""The chosen-hash inputs of Sort + Reduce (one builder each, shared by the CPU tests and by every GPU path).

A builder returns a Program: batches of packed dimension rows and raw measures whose 64-bit row hashes were CHOSEN — the rows
are computed from the hashes with sort_model.rows_with_hash64 — and asserts, through the model's own murmur and before
anything touches a GPU, the property it is named for (segment lengths, descents, home buckets, run boundaries).  The
constants below are mirrored from the kernels and cited by name.  Raw measures are small integers; hash_sets.AGGS-style
value functions turn them into the values of one aggregate so that every comparison is bit-exact."""
import functools

import numpy as np

import sort_model as M
from aresdb_amd import abi

FULL = (1 << 64) - 1
LOW = 0xFFFFFFFF

# ---- mirrored from aresdb_amd/csrc/algo/sort_reduce.hip -------------------------------------------------------------------
K_FIXUP_MAX_RUN = 64        # kFixupMaxRun: the longest segment one thread sorts by insertion
K_FIXUP_LONG_MAX = 4096     # kFixupLongMax: the longest segment a workgroup sorts by ranking
K_FIXUP_LONG_SLOTS = 1024   # kFixupLongSlots: the claim table; kFixupLongSlots / 2 long segments are listed at most
K_DETECT_BLOCK = 256        # kBlock: one detect workgroup's consecutive positions (while the grid is not capped: < 4096 * 256 rows)
K_SORT_TILE = 4096          # kBlock * kSortKPT: a radix pass's tile
K_REDUCE_KPT, K_REDUCE_TILE = 8, 2048   # kReduceKPT, kReduceTile: a lane's consecutive positions, a tile of reduce_kernel


def cap_per_group(length):
    """capPerGroup = length / 8 / fixGrid + 64 with fixGrid = ceil(length / kBlock) (not capped below 2^20 rows)"""
    fix_grid = (length + K_DETECT_BLOCK - 1) // K_DETECT_BLOCK
    return length // 8 // fix_grid + 64


# ---- mirrored from aresdb_amd/csrc/algo/sort_reduce_fused.hip -------------------------------------------------------------
# Table<VW, WIDE>: name -> (kSlots, kTail); kHomes = kSlots - kTail, home buckets of four slots, kMaxGroups = kHomes * 13 / 16
TABLES = {"narrow4": (8192, 256), "narrow8": (6912, 256), "wide": (2048, 128)}
K_WIDE_ENTRIES = 1024   # kWideEntries: the wide layout takes one partition per 1024 rows


def table_limits(table):
    slots, tail = TABLES[table]
    homes = slots - tail
    return homes // 4, homes * 13 // 16   # (home buckets, kMaxGroups)


def home_bucket(h, part_bits, table):
    """sr_merge_kernel's home_bucket: the 32 key bits right below the partition's, scaled to the home buckets"""
    x = (int(h) >> (32 - part_bits)) & LOW
    return (x * table_limits(table)[0]) >> 32


def partition_of(h, part_bits):
    return int(h) >> (64 - part_bits) if part_bits else 0


# ---- aggregates: name -> (model aggregate, ABI aggregate, numpy type of the measure vector, value of raw measure m in
# [-2000, 2000], type of the source column, output type of the measure transform) ------------------------------------------
AGGS = {
    "sum_u32": (("sum", "u32"), abi.AGGR_SUM_UNSIGNED, np.uint32, lambda m: (m + 2000) * 1000003, abi.Uint32, abi.Uint32),
    "sum_u64": (("sum", "u64"), abi.AGGR_SUM_UNSIGNED, np.uint64, lambda m: (m + 2000) * 1000003, abi.Uint32, abi.Int64),
    "min_i32": (("min", "i32"), abi.AGGR_MIN_SIGNED, np.int32, lambda m: m * 1000, abi.Int32, abi.Int32),
    "max_u32": (("max", "u32"), abi.AGGR_MAX_UNSIGNED, np.uint32, lambda m: (m + 2000) * 1000003, abi.Uint32, abi.Uint32),
    "sum_f32": (("sum", "f32"), abi.AGGR_SUM_FLOAT, np.float32, lambda m: m / 8, abi.Float32, abi.Float32),
    "min_f32": (("min", "f32"), abi.AGGR_MIN_FLOAT, np.float32, lambda m: m / 8, abi.Float32, abi.Float32),
    "max_f32": (("max", "f32"), abi.AGGR_MAX_FLOAT, np.float32, lambda m: m / 8, abi.Float32, abi.Float32),
    # {float32 average, uint32 count} in 8 bytes; the values depend on the group (Program.values)
    "avg": (("avg", "f32"), abi.AGGR_AVG_FLOAT, np.uint64, None, abi.Float32, abi.Float64),
}
INT_AGGS = ["sum_u32", "sum_u64", "min_i32", "max_u32"]
ALL_AGGS = list(AGGS)
MAX_ROWS_PER_FLOAT_GROUP = 4000  # 4000 x 2000 eighths < 2^24: every partial float32 sum is exact, in any order


def pack_avg(pairs):
    """(average, count) pairs as the measure vector holds them"""
    f = np.array([p[0] for p in pairs], np.float32).view(np.uint32).astype(np.uint64)
    return f | (np.array([p[1] for p in pairs], np.uint64) << np.uint64(32))


def encode_values(agg_name, values):
    """model values as the bytes of the measure vector"""
    if agg_name == "avg":
        return pack_avg(values)
    return np.array(values).astype(AGGS[agg_name][2]) if len(values) else np.zeros(0, AGGS[agg_name][2])


def _raw(i):
    return (np.asarray(i, np.int64) * 37 + 11) % 4001 - 2000


def default_free(hashes):
    """the free word a hash gets unless a collision is asked for: equal hashes are equal rows"""
    with np.errstate(over="ignore"):
        return np.asarray(hashes, np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x0123456789ABCDEF)


class Program:
    """batches: [(hashes, free words or None)] in input order."""

    def __init__(self, name, batches, widths=(4, 4, 4, 4), valids=None, facts=None):
        self.name, self.widths = name, tuple(widths)
        self.nd = len(self.widths)
        self.valids = tuple(valids) if valids is not None else (1,) * self.nd
        self.ndw = tuple(sum(1 for w in self.widths if w == x) for x in (16, 8, 4, 2, 1))
        self.facts = facts or {}
        self.hashes, self.rows, self.raw = [], [], []
        at = 0
        for hs, frees in batches:
            hs = np.asarray(hs, np.uint64)
            frees = default_free(hs) if frees is None else np.asarray(frees, np.uint64)
            rows = M.rows_with_hash64(hs, frees, self.valids, self.widths)
            assert np.array_equal(M.hash_rows(rows), hs), name   # the rows do have the hashes they were built for
            self.hashes.append(hs)
            self.rows.append(rows)
            self.raw.append(_raw(np.arange(at, at + len(hs))))
            at += len(hs)
        k = min(len(self.hashes[0]), 3)   # ... by the scalar murmur too
        assert [M.murmur3_128_lo64(bytes(r)) for r in self.rows[0][:k]] == [int(h) for h in self.hashes[0][:k]]
        allh, counts = np.unique(np.concatenate(self.hashes), return_counts=True)
        self.distinct, self.largest_group = len(allh), int(counts.max())
        self._count = dict(zip(allh.tolist(), counts.tolist()))

    @property
    def sizes(self):
        return [len(h) for h in self.hashes]

    def float_ok(self):
        return self.largest_group <= MAX_ROWS_PER_FLOAT_GROUP

    def values(self, agg_name, unit_counts=False):
        """per batch, the model's measure values of aggregate `agg_name`.  avg: a row whose hash occurs once in the whole
        program carries (m / 8, 1), the rows of larger groups (0, 1 .. 3) — what the rolling average is exact for;
        unit_counts: every count is 1 (what a measure transform produces from a column)."""
        if agg_name != "avg":
            f = AGGS[agg_name][3]
            return [[f(int(m)) for m in raw] for raw in self.raw]
        return [[(int(m) / 8, 1) if self._count[int(h)] == 1 else (0.0, 1 if unit_counts else 1 + int(m) % 3) for m, h in zip(raw, hs)]
                for raw, hs in zip(self.raw, self.hashes)]

    def column_values(self, agg_name):
        """per batch, the source column a measure transform reads (avg: the float whose pair is (value, 1))"""
        if agg_name == "avg":
            return [np.array([v for v, _ in vs], np.float32) for vs in self.values("avg", unit_counts=True)]
        t = {abi.Uint32: np.uint32, abi.Int32: np.int32, abi.Float32: np.float32}[AGGS[agg_name][4]]
        return [np.array(vs).astype(t) for vs in self.values(agg_name)]

    @functools.lru_cache(maxsize=None)
    def expected(self, agg_name, unit_counts=False):
        """the model's account of every batch's Sort + Reduce (sort_model.Reduced), result buffers ping-ponged: the previous
        result's rows and values are the model's own"""
        out, prev_rows, prev_values = [], None, []
        for rows, values in zip(self.rows, self.values(agg_name, unit_counts)):
            r = M.groups_by_hash64(prev_rows, rows, prev_values + values, AGGS[agg_name][0])
            r.prev = len(prev_values)
            out.append(r)
            prev_rows, prev_values = r.rows, list(r.values)
        return out

    def sort_inputs(self, b):
        """the hash vector Sort sees for batch b in input order: [previous result ascending, then the batch]"""
        prev = np.unique(np.concatenate(self.hashes[:b])) if b else np.zeros(0, np.uint64)
        return np.concatenate([prev, self.hashes[b]])

    def census(self, b=0):
        return M.fixup_census(self.sort_inputs(b), K_FIXUP_MAX_RUN, K_FIXUP_LONG_MAX, K_DETECT_BLOCK)

    def radix_passes(self):
        """radix_pass_kernel launches of the top-half sort over all batches: four per Sort, and eight more where the fix-up
        gives up (a segment beyond kFixupLongMax, more than kFixupLongSlots / 2 long segments, a detect workgroup that lists
        more than capPerGroup short ones)"""
        total = 0
        for b in range(len(self.hashes)):
            c = self.census(b)
            n = len(self.sort_inputs(b))
            full_list = any(k > cap_per_group(n) for k in c.per_block.values())
            total += 12 if c.beyond or len(c.long) > K_FIXUP_LONG_SLOTS // 2 or full_list else 4
        return total


def H64(top, low):
    return (int(top) << 32) | int(low)


# ---- layouts in the order the top-half passes leave ------------------------------------------------------------------------
class _Layout:
    """Builds a hash vector segment by segment in ascending order of the top half: position = place after the four passes.
    The input order then keeps each segment's rows together and in order, and shuffles the segments."""

    def __init__(self, seed, top_step):   # (top_step: so that the segments spread over the whole range of top halves — every partition gets some)
        self.segments, self.n, self.top, self.step = [], 0, 0x1000, top_step
        self.rng = np.random.default_rng(seed)

    def segment(self, lows):
        """a run of equal top halves with these low halves, in this order; returns its [start, end)"""
        self.top += self.step
        self.segments.append([H64(self.top, lo) for lo in lows])
        self.n += len(lows)
        return self.n - len(lows), self.n

    def singles(self, count):
        for _ in range(count):
            self.segment([int(self.rng.integers(0, 1 << 32))])

    def pad_to(self, position):
        assert position >= self.n, (position, self.n)
        self.singles(position - self.n)

    def hashes(self, shuffle=True):
        order = self.rng.permutation(len(self.segments)) if shuffle else range(len(self.segments))
        out = np.array([h for s in order for h in self.segments[s]], np.uint64)
        # the property: four stable passes over the top halves leave the layout
        want = np.array([h for s in self.segments for h in s], np.uint64)
        assert np.array_equal(out[np.argsort(out >> np.uint64(32), kind="stable")], want)
        return out


def _descending(n, base=0x70000000):
    return [base - 17 * i for i in range(n)]


def _few_groups(n, groups, seed):
    """n rows of `groups` distinct low halves, scrambled (the production shape of a long segment: a few groups whose hashes
    share their top half, each with many rows), the largest low half first so that the segment holds a descent"""
    lows = [0x10000000 * (g + 1) + 0x321 for g in range(groups)]
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, groups, n).tolist()
    pick[0], pick[1] = groups - 1, 0
    return [lows[g] for g in pick]


@functools.lru_cache(maxsize=None)
def fixup_short():
    """Segments the short fix-up (sort_fixup_detect_kernel -> sort_fixup_sort_kernel) must list and sort, or must leave alone:
    lengths 2, 3, 63 and 64 (kFixupMaxRun) and 65 (the first long one); one at positions [0, 3) and one ending at n - 1; one
    straddling a 256-entry detect workgroup and one a 4096-entry sort tile; one with several descents (only the first lists
    it); one already ascending (never listed); 5000 EQUAL keys (no descent, never walked); equal keys inside an out-of-order
    segment (stability: index order kept)."""
    L = _Layout(11, top_step=1 << 20)
    listed = [L.segment([30, 20, 10])]                       # at [0, 3)
    L.singles(5)
    for n in (2, 3, 63, 64):
        listed.append(L.segment(_descending(n)))
        L.singles(3)
    long_one = L.segment(_descending(65))
    L.pad_to(K_DETECT_BLOCK - 6)
    straddle_block = L.segment(_descending(10))
    listed.append(straddle_block)
    L.singles(7)
    listed.append(L.segment([5, 4, 3, 2, 1, 9, 8, 7]))       # several descents
    L.singles(2)
    ascending = L.segment(list(range(1, 31)))
    L.singles(2)
    listed.append(L.segment([7, 7, 3, 7, 3, 1, 7, 1]))       # equal keys among the disorder
    L.singles(4)
    equal = L.segment([0x5555] * 5000)
    L.pad_to(2 * K_SORT_TILE - 9)
    straddle_tile = L.segment(_descending(20))
    listed.append(straddle_tile)
    L.singles(30)
    listed.append(L.segment([4, 3, 2, 1]))                   # ends at n - 1
    prog = Program("fixup_short", [(L.hashes(), None)])
    c = prog.census()
    assert sorted(c.short) == sorted(listed) and c.long == [long_one] and not c.beyond, (c.short, c.long, c.beyond)
    assert listed[0][0] == 0 and listed[-1][1] == L.n == prog.sizes[0]
    assert straddle_block[0] < K_DETECT_BLOCK < straddle_block[1] and straddle_tile[0] % K_SORT_TILE > straddle_tile[1] % K_SORT_TILE > 0
    assert ascending not in c.short and equal not in c.short and equal[1] - equal[0] == 5000
    prog.facts = {"short": len(c.short), "long": len(c.long), "passes": 4}
    return prog


_LONG_LENGTHS = (65, 66, 1000, 4095, 4096)


@functools.lru_cache(maxsize=None)
def fixup_long():
    """Segments of 65, 66, 1000, 4095 and 4096 (kFixupLongMax) entries for sort_fixup_long_kernel, each as two to four groups
    with many rows and as all-distinct low halves in descending order (many descents, claimed once); the first at position 0,
    the last ending at n - 1, neighbours adjacent (no other top half between them)."""
    L = _Layout(12, top_step=1 << 26)
    segs = []
    for k, n in enumerate(_LONG_LENGTHS):
        segs.append(L.segment(_few_groups(n, 2 + k % 3, 100 + k)))
        segs.append(L.segment(_descending(n)))
        if k == 1:
            L.singles(40)
    prog = Program("fixup_long", [(L.hashes(), None)])
    c = prog.census()
    assert c.long == segs and not c.short and not c.beyond, (c.short, c.long, c.beyond)
    assert segs[0][0] == 0 and segs[-1][1] == prog.sizes[0] and segs[0][1] == segs[1][0]
    assert len(c.long) <= K_FIXUP_LONG_SLOTS // 2 and c.descents > 4000
    prog.facts = {"short": 0, "long": len(c.long), "passes": 4}
    return prog


@functools.lru_cache(maxsize=None)
def fixup_fallback(which):
    """Inputs the fix-up must hand to the eight passes (`fallback`):
    beyond     one out-of-order segment of kFixupLongMax + 1 = 4097 entries;
    claims     kFixupLongSlots / 2 + 1 = 513 long segments of 65 entries: the claim list is full (33 345 rows);
    list       one detect workgroup lists more segments than its list holds.  A batch of 4 x 256 rows has fixGrid = 4 detect
               workgroups and capPerGroup = 1024 / 8 / 4 + 64 = 96; a 256-row block of 128 descending PAIRS of distinct top
               halves lists 128 > 96 segments, all from one workgroup (a pair's descent is its odd position: pairs do not
               straddle blocks).  Blocks 0 and 2 are such blocks."""
    L = _Layout(13 + len(which), top_step=1 << 22)
    if which == "beyond":
        L.singles(20)
        L.segment(_descending(K_FIXUP_LONG_MAX + 1))
        L.singles(20)
    elif which == "claims":
        for _ in range(K_FIXUP_LONG_SLOTS // 2 + 1):
            L.segment(_descending(K_FIXUP_MAX_RUN + 1))
    else:
        for block in range(4):
            if block % 2 == 0:
                for _ in range(K_DETECT_BLOCK // 2):
                    L.segment([9, 2])
            else:
                L.singles(K_DETECT_BLOCK)
    prog = Program(f"fixup_fallback/{which}", [(L.hashes(), None)])
    c = prog.census()
    if which == "beyond":
        assert len(c.beyond) == 1 and c.beyond[0][1] - c.beyond[0][0] == K_FIXUP_LONG_MAX + 1
    elif which == "claims":
        assert len(c.long) == K_FIXUP_LONG_SLOTS // 2 + 1 and prog.sizes[0] == 33345 and not c.beyond
    else:
        n = prog.sizes[0]
        assert n == 4 * K_DETECT_BLOCK and cap_per_group(n) == 96 and not c.long and not c.beyond
        assert c.per_block == {0: 128, 2: 128} and max(c.per_block.values()) > cap_per_group(n)
    prog.facts = {"short": len(c.short), "long": len(c.long), "passes": 12}
    return prog


# ---- ordinary hashes ------------------------------------------------------------------------------------------------------
def ordinary(i):
    """the i-th of a fixed sequence of distinct, well spread hashes (an odd multiplier is a bijection)"""
    with np.errstate(over="ignore"):
        return np.asarray(i, np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567)


def _spread(hashes, reps):
    """every hash `reps` times, spread over the batch (each pass starts elsewhere)"""
    hashes = list(hashes)
    out = []
    for r in range(reps):
        k = (r * 5) % max(1, len(hashes))
        out += hashes[k:] + hashes[:k]
    return out


@functools.lru_cache(maxsize=None)
def collisions64(batches=2):
    """Pairs and triples of DIFFERENT rows with one 64-bit hash: in one wavefront, far apart, in different batches, previous
    result row versus batch row.  One group, the first row's dimensions, all values aggregated — on every path (on the
    scan-fed path through the re-evaluated representative)."""
    sizes = [300, 700, 150][:batches] if batches > 1 else [1000]
    body = [list(ordinary(np.arange(at, at + n)).tolist()) for at, n in zip((0, 200, 600), sizes)]
    free = [list(default_free(np.array(b, np.uint64)).tolist()) for b in body]
    C = [0xDEADBEEF0BADF00D, 0x0123456789ABCDEF, 0x13572468ACE02468, 0x00000000FFFFFFFF, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFF00000001]
    last = batches - 1
    # (batch, position, hash, member number): positions are final — inserted in ascending order
    plan = [(last, 8, C[0], 0), (last, 9, C[0], 1),                          # neighbours
            (last, 70, C[1], 0), (last, 100, C[1], 1),                        # one wavefront of the reduce / merge kernels
            (last, 5, C[2], 0), (last, 120, C[2], 1), (last, sizes[last] - 1, C[2], 2),   # a triple, far apart
            (0, 10, C[3], 0), (last, 40, C[3], 1),                            # previous result (or far apart) versus batch
            (0, 150, C[4], 0), (last, 3, C[4], 1), (last, 4, C[4], 2),
            (0, 20, C[5], 0), (min(1, last), 60, C[5], 1), (last, 130, C[5], 2)]   # one member per batch
    for b, at, h, k in sorted(plan, key=lambda x: (x[0], x[1])):
        body[b].insert(at, h)
        free[b].insert(at, (0xC0111DE * (k + 1) + h * 3) & FULL)
    prog = Program(f"collisions64/b{batches}", [(b, f) for b, f in zip(body, free)])
    rows = np.concatenate(prog.rows)
    flat = np.concatenate(prog.hashes)
    exp = prog.expected("sum_u64")[-1]
    for h in C:
        members = np.flatnonzero(flat == np.uint64(h))
        assert len(members) >= 2 and len({bytes(rows[i]) for i in members}) == len(members)   # different rows, one hash
        g = int(np.flatnonzero(exp.hashes == np.uint64(h))[0])
        assert bytes(exp.rows[g]) == bytes(rows[members[0]])                                  # the model keeps the first
    assert prog.distinct == len(set(flat.tolist())) and exp.groups == prog.distinct
    return prog


SENTINELS = [0, 1, (1 << 32) - 1, 1 << 32, 1 << 63, FULL - 1, FULL, H64(LOW, 0x1234), H64(0x1234, LOW)]


@functools.lru_cache(maxsize=None)
def sentinels64(variant="plain", widths=(4, 4, 4, 4), valids=None):
    """Hashes 0, 1, 2^32 - 1, 2^32, 2^63, 2^64 - 2 and 2^64 - 1 (the merge table's empty word and the radix pass's padding
    key), an all-ones high word over another low word and the reverse (the empty test is (hi & lo) == ~0), among ordinary
    rows, three times each.  variant: plain | first_last (the 2^64 - 1 rows are the batch's first and last) | prev (an earlier
    batch left the 2^64 - 1 group, and a few others, in the previous result) | no_empty (without 2^64 - 1: the table paths
    must take everything else themselves)."""
    hs = [h for h in SENTINELS if not (variant == "no_empty" and h == FULL)] + ordinary(np.arange(40)).tolist()
    body = _spread(hs, 3)
    batches = []
    if variant == "first_last":
        body = [FULL] + [h for h in body if h != FULL] + [FULL]
        assert body[0] == body[-1] == FULL and FULL not in body[1:-1]
    elif variant == "prev":
        batches.append(([FULL, 0, 1 << 63] + ordinary(np.arange(100, 105)).tolist() + [FULL, H64(LOW, 0x1234)], None))
    batches.append((body, None))
    prog = Program(f"sentinels64/{variant}/{'x'.join(map(str, widths))}", batches, widths, valids)
    assert prog.distinct == len(set(hs)) + (5 if variant == "prev" else 0)
    assert (FULL in np.concatenate(prog.hashes).tolist()) == (variant != "no_empty")
    return prog


@functools.lru_cache(maxsize=None)
def partitions(part_bits, variant="bounds"):
    """For 2^part_bits partitions (the top part_bits bits of the hash select one):
    bounds       every partition's lowest and highest hash (but 2^64 - 1: 2^64 - 2), a family that differs in the partition
                 bits only, and another that differs in the bit right below them only — in two batches, the first of which
                 leaves the even partitions' bounds in the previous result: its ranges END EXACTLY at a partition bound;
    alternating  rows in the odd partitions only (empty and full partitions alternate), a previous result included;
    one          all rows in one partition (the last but one)."""
    P = part_bits
    shift = 64 - P
    n = 1 << P
    low_of = [p << shift for p in range(n)]
    high_of = [min(((p + 1) << shift) - 1, FULL - 1) for p in range(n)]
    if variant == "bounds":
        family = [(p << shift) | (0x00ABCDE5F0123457 & ((1 << shift) - 1)) for p in range(n)]
        below = [(1 << (shift - 1)) | 0x155, 0x155]
        first = [h for p in range(0, n, 2) for h in (low_of[p], high_of[p])]
        second = _spread(low_of + high_of + family + below, 2)
        batches = [(first[::-1], None), (second, None)]
        prog = Program(f"partitions/{variant}/P{P}", batches)
        assert len({partition_of(h, P) for h in family}) == n and len({h & ((1 << shift) - 1) for h in family}) == 1
        prev = np.unique(prog.hashes[0])
        for p in range(0, n, 2):  # the previous result's range of partition p is exactly [low, high]: it ends at the bound
            mine = prev[(prev >> np.uint64(shift)) == np.uint64(p)] if P else prev
            assert mine.tolist() == [low_of[p], high_of[p]]
    elif variant == "alternating":
        per = max(2, 600 // n)
        rows = [(p << shift) | int(x) for p in range(1, n, 2) for x in (ordinary(np.arange(p * per, (p + 1) * per)) >> np.uint64(P)).tolist()]
        prog = Program(f"partitions/{variant}/P{P}", [(rows[::3], None), (_spread(rows, 2), None)])
        assert {partition_of(h, P) % 2 for h in rows} == {1} and len({partition_of(h, P) for h in rows}) == n // 2
    else:
        p = n - 2 if n > 1 else 0
        rows = [(p << shift) | int(x) for x in (ordinary(np.arange(900)) >> np.uint64(P)).tolist()]
        prog = Program(f"partitions/{variant}/P{P}", [(rows[:200], None), (_spread(rows, 2), None)])
        assert {partition_of(h, P) for h in rows} == {p}
    return prog


def cluster_keys(count, bucket, part_bits, table, partition=0, step=1):
    """`count` distinct hashes of partition `partition` whose home bucket is `bucket`, ascending"""
    hb = table_limits(table)[0]
    x0 = -((-bucket << 32) // hb)   # the first 32-bit value that scales to `bucket`
    out = []
    for j in range(count):
        x = x0 + j * step
        h = (x << (32 - part_bits)) | (0x2B + 5 * j if part_bits < 32 else 0)
        h |= partition << (64 - part_bits) if part_bits else 0
        out.append(h & FULL)
    assert all(home_bucket(h, part_bits, table) == bucket and partition_of(h, part_bits) == partition for h in out)
    return out


@functools.lru_cache(maxsize=None)
def clusters(table, part_bits, order="shuffled", tail=None):
    """Keys aimed at single home buckets of one partition's table (format `table`, 2^part_bits partitions):
    tail = None   clusters of 4, 5, 200 and 1000 keys with one home bucket each (ranking walks over a long cluster: the output
                  must ascend), two clusters that grow into one (150 keys homed 30 buckets apart), inserted ascending,
                  descending or shuffled, every key twice;
    tail = k      a cluster of kTail + k keys (k = -8, 0, 8) homed in the LAST home bucket, whose overflow room is the kTail
                  slots at the table's end: kTail + 4 slots in all — k = 8 runs off the table with far fewer groups than
                  kMaxGroups and must be declined to the real sort, the others must not."""
    hb, max_groups = table_limits(table)
    ktail = TABLES[table][1]
    part = (1 << part_bits) - 2 if part_bits else 0
    if tail is None:
        # (the wide layout takes 1024 rows per partition: its clusters are smaller — 479 keys, each twice, in one partition)
        mid, big, pair, gap = (200, 1000, 150, 30) if table != "wide" else (100, 250, 60, 10)
        sets = [cluster_keys(4, 10, part_bits, table, part), cluster_keys(5, 50, part_bits, table, part),
                cluster_keys(mid, 100, part_bits, table, part), cluster_keys(big, 200, part_bits, table, part),
                cluster_keys(pair, hb - 120, part_bits, table, part), cluster_keys(pair, hb - 120 + gap, part_bits, table, part)]
        assert 4 * gap < pair and 200 + big // 4 < hb - 120   # the pair's first cluster reaches the second one's home bucket
        name = f"clusters/{table}/P{part_bits}/{order}"
    else:
        sets = [cluster_keys(ktail + tail, hb - 1, part_bits, table, part), cluster_keys(30, 5, part_bits, table, part)]
        name = f"clusters/{table}/P{part_bits}/tail{tail:+d}"
    for s in sets:
        assert len(set(s)) == len(s) and s == sorted(s)
    hs = [h for s in sets for h in s]
    assert len(hs) < max_groups and FULL not in hs
    if tail is not None:
        assert sets[0][-1] >> (64 - part_bits) == part if part_bits else True
        assert (len(sets[0]) > ktail + 4) == (tail > 4)   # the cluster's slots: the last home bucket's four and the tail
    if order == "descending":
        hs = hs[::-1]
    elif order == "shuffled":
        hs = [hs[i] for i in np.random.default_rng(len(hs)).permutation(len(hs))]
    prog = Program(name, [(hs + hs[::-1], None)])
    assert prog.distinct == len(hs)
    prog.facts = {"declines": tail is not None and tail > 4}
    return prog


def _runs_from_sizes(sizes, seed):
    """a batch whose groups, in ascending hash order, have these sizes; rows in shuffled order"""
    hs = np.sort(ordinary(np.arange(len(sizes)) + 1000 * seed))
    assert len(np.unique(hs)) == len(sizes)
    body = np.repeat(hs, sizes)
    return body[np.random.default_rng(seed).permutation(len(body))]


@functools.lru_cache(maxsize=None)
def runs(variant):
    """reduce_kernel's run boundaries (a lane owns kReduceKPT = 8 consecutive sorted positions, a tile is 2048):
    heads    group sizes chosen so that heads fall on sorted positions 7 / 8 / 9, 2047 / 2048 / 2049 and 4095 / 4096 / 4097;
    span     one group of 3 x 2048 + 1 rows between two singletons;
    n1, n2, n2048, n2049   batches of that many rows (distinct but for one pair);
    one_group, distinct    2500 rows in one group; 2500 distinct rows."""
    if variant == "heads":
        want = [7, 8, 9, 2047, 2048, 2049, 4095, 4096, 4097]
        cuts = [0] + want + [4200]
        sizes = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
        body = _runs_from_sizes(sizes, 1)
        starts = np.cumsum([0] + sizes[:-1]).tolist()
        assert starts[1:] == want
    elif variant == "span":
        body = _runs_from_sizes([1, 3 * K_REDUCE_TILE + 1, 1], 2)
    elif variant in ("n1", "n2", "n2048", "n2049"):
        n = int(variant[1:])
        body = ordinary(np.arange(n) + 77).copy()
        if n > 2:
            body[n - 1] = body[0]
    elif variant == "one_group":
        body = np.full(2500, ordinary(5), np.uint64)
    else:
        body = ordinary(np.arange(2500) + 9)
    prog = Program(f"runs/{variant}", [(body, None)])
    if variant == "heads":
        e = prog.expected("sum_u64")[0]
        assert np.flatnonzero(np.concatenate([[True], e.sorted_hash[1:] != e.sorted_hash[:-1]])).tolist() == [0] + want
    return prog


@functools.lru_cache(maxsize=None)
def three_batches():
    """Three batches with the result buffers ping-ponged: from the second on Sort sees the previous result ASCENDING by hash
    in front of the batch — the input the top-half sort meets in production — with short and long segments whose members lie
    partly in the previous result."""
    L = [_Layout(21 + b, top_step=1 << 25) for b in range(3)]
    for b, lay in enumerate(L):
        lay.top = 0x1000          # the same top halves in every batch
        for k in range(6):
            lay.segment([(0x40000000 - 1000 * b) - 7 * i for i in range(5 + k)])   # lower low halves in later batches
            lay.singles(2)
        lay.segment(_descending(200, 0x70000000 - 5000 * b))
        lay.segment(_few_groups(300, 3, 40))
        lay.singles(50)
    prog = Program("three_batches", [(lay.hashes(), None) for lay in L])
    for b in (1, 2):
        c = prog.census(b)
        assert len(c.short) >= 6 and len(c.long) >= 1 and not c.beyond, (b, len(c.short), len(c.long))
    prog.facts = {"short": [len(prog.census(b).short) for b in range(3)], "long": [len(prog.census(b).long) for b in range(3)]}
    return prog


def all_programs():
    """{name: builder} of every chosen-hash input (built on first use, then shared)"""
    out = {
        "fixup_short": fixup_short, "fixup_long": fixup_long,
        "fallback_beyond": lambda: fixup_fallback("beyond"), "fallback_claims": lambda: fixup_fallback("claims"),
        "fallback_list": lambda: fixup_fallback("list"),
        "collisions64": lambda: collisions64(2), "collisions64_b3": lambda: collisions64(3), "collisions64_flat": lambda: collisions64(1),
        "sentinels64": lambda: sentinels64("plain"), "sentinels64_first_last": lambda: sentinels64("first_last"),
        "sentinels64_prev": lambda: sentinels64("prev"), "sentinels64_no_empty": lambda: sentinels64("no_empty"),
        "sentinels64_844": lambda: sentinels64("prev", (8, 4, 4), (1, 0, 1)), "sentinels64_uuid": lambda: sentinels64("prev", (16,)),
        "sentinels64_844_no_empty": lambda: sentinels64("no_empty", (8, 4, 4)), "sentinels64_uuid_no_empty": lambda: sentinels64("no_empty", (16,)),
        "sentinels64_nulls": lambda: sentinels64("no_empty", (4, 4, 4, 4), (1, 0, 1, 0)),
        "three_batches": three_batches,
    }
    for P in (0, 2, 3, 9, 12):
        for v in ("bounds", "alternating", "one"):
            if not (P == 0 and v != "bounds"):
                out[f"partitions_{v}_p{P}"] = functools.partial(partitions, P, v)
    # (one partition's rows reach a narrow table only while its record streams hold them: up to 8 partitions at these sizes)
    for table, P in (("narrow4", 2), ("narrow8", 3), ("wide", 3), ("wide", 0)):
        for order in ("ascending", "descending", "shuffled"):
            out[f"clusters_{table}_p{P}_{order}"] = functools.partial(clusters, table, P, order)
        for k in (-8, 0, 8):
            out[f"clusters_{table}_p{P}_tail{k:+d}"] = functools.partial(clusters, table, P, "shuffled", k)
    for v in ("heads", "span", "n1", "n2", "n2048", "n2049", "one_group", "distinct"):
        out[f"runs_{v}"] = functools.partial(runs, v)
    return out
