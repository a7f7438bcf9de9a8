"""Sort + Reduce at CHOSEN 64-bit row hashes, on every path that reaches it, against the exact model of tests/sort_model.py.

Everything a host can observe of Sort + Reduce is a function of the 64-bit row hash — the group, the output order (ascending
hash), the representative (the lowest row of a stable sort) — and so is every decision inside the kernels: the radix digits
and the fix-up's segments of equal top halves (sort_reduce.hip), the partition, the monotone home bucket, the overflow slots
at a table's end and the all-ones empty word (sort_reduce_fused.hip), the run boundaries of reduce_kernel.  Random keys reach
almost none of these at test sizes (about n^2 / 2^33 pairs share a top half: under one pair at 10^5 rows).  tests/sort_sets.py
builds rows FOR such hashes (murmur3_x64_128 inverted in its one block); every case below runs them in a child process per
environment (the library latches its switches), which compares the group count, the output rows IN ORDER, the values and —
where the path exposes them — the hash / index vectors between Sort and Reduce and after with the model, bit for bit, and
prints the kernel log; the tests here assert from that log, or from the library's own trace, that the path they are named for
ran.  The three fix-up kernels are always launched, so the log cannot tell which of them did the work: there the input's own
CPU-side assertion (sort_sets: the listed short and long segments, computed from the order four stable passes leave) is the
proof, and the number of radix_pass_kernel launches (4 per Sort, 12 where the fix-up gives up) its consequence."""
import json
import os
import re
import subprocess

import pytest

import harness as H
import sort_paths as P
import sort_sets as S

pytestmark = pytest.mark.gpu

_SWITCHES = ("ARES_SORT_FUSE", "ARES_SORT_TOPBITS", "ARES_SR_SCAN_FED", "ARES_SR_MAX_GROUPS", "ARES_MIN_PART_BITS", "ARES_SRV_PART_BITS",
             "ARES_SORT_VECTORS", "ARES_SORT_STATE", "ARES_SR_FLOAT", "ARES_RTC", "ARES_FUSE", "ARES_DEFER", "ARES_HR_TRACE")

FIXUP = ["fixup_short", "fixup_long", "three_batches"]
FALLBACK = ["fallback_beyond", "fallback_claims", "fallback_list"]
COLLISIONS = ["collisions64", "collisions64_b3", "collisions64_flat"]
SENTINELS = ["sentinels64", "sentinels64_first_last", "sentinels64_prev", "sentinels64_no_empty"]
WIDE_SLOTS = ["sentinels64_844", "sentinels64_uuid", "sentinels64_844_no_empty", "sentinels64_uuid_no_empty"]
RUNS = [f"runs_{v}" for v in ("heads", "span", "n1", "n2", "n2048", "n2049", "one_group", "distinct")]
AGGS4 = ["sum_u32", "min_i32", "max_u32", "sum_f32", "min_f32", "max_f32"]   # 4-byte values: Table<4>
AGGS8 = ["sum_u64", "avg"]                                                   # 8-byte values: Table<8>


def _with_aggs(names, aggs=S.INT_AGGS, shift=0):
    return [f"{n}:{aggs[(i + shift) % len(aggs)]}" for i, n in enumerate(names)]


def _every_agg(names, aggs=S.ALL_AGGS):
    return [f"{n}:{a}" for n in names for a in aggs]


def _partitions(bits):
    return [f"partitions_{v}_p{bits}" for v in ("bounds", "alternating", "one")]


def _clusters(table, bits, tails=(-8, 0, 8)):
    return [f"clusters_{table}_p{bits}_{o}" for o in ("ascending", "descending", "shuffled")] + [f"clusters_{table}_p{bits}_tail{k:+d}" for k in tails]


def run_child(mode, wanted, env, timeout=300):
    """One child process in the given environment; ({case: kernel log}, {case: facts}, stderr)."""
    full = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    full.update(env)
    try:
        r = subprocess.run(P.CHILD + [mode] + list(wanted), cwd=H.ROOT, env=full, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"a chosen-hash child ({mode} {wanted}) hung: nothing more is started on this GPU\n{(e.stderr or b'')[-2000:]}", 3)
    if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in r.stderr:
        pytest.exit(f"a chosen-hash child ({mode} {wanted}) faulted (exit {r.returncode}): nothing more is started on this GPU\n"
                    f"{r.stderr[-3000:]}", 3)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-4000:])
    kernels, facts = {}, {}
    for line in r.stdout.splitlines():
        if line.startswith("KERNELS "):
            d = json.loads(line[8:])
            kernels[d["case"]] = d["kernels"]
        elif line.startswith("FACTS "):
            d = json.loads(line[6:])
            facts[d["case"]] = d
    assert list(kernels) == list(wanted) == list(facts), (list(kernels), r.stdout[-500:])
    return kernels, facts, r.stderr


def _has(log, *prefixes):
    return [k for k in log if k.startswith(prefixes)]


def _holds_empty_word(case):
    """the input holds the hash 2^64 - 1: every table path must hand the call to the real sort"""
    return any(S.FULL in h.tolist() for h in S.all_programs()[case.split(":")[0]]().hashes)


# ---- the real sort ------------------------------------------------------------------------------------------------------------
REAL = {
    "fixup": _with_aggs(FIXUP + FALLBACK),
    "collisions": _every_agg(COLLISIONS),
    "sentinels": _with_aggs(SENTINELS + ["sentinels64_nulls"] + WIDE_SLOTS, shift=1),
    "partitions": _with_aggs(_partitions(3) + _partitions(12), shift=2),
    "clusters": _with_aggs(_clusters("narrow4", 2) + _clusters("wide", 0), shift=3),
    "runs": _with_aggs(RUNS),
}


@pytest.mark.parametrize("family", list(REAL))
def test_real_sort_top_half_and_fix_up(family):
    """ARES_SORT_FUSE=0: four radix passes over the top halves, then the fix-up — short segments by insertion, long ones by
    ranking in LDS, and the eight-pass fallback where a segment is longer than kFixupLongMax, the claim list is full or one
    detect workgroup's list is (12 radix_pass_kernel launches for that Sort instead of 4).  The host reads the hash and index
    vector between Sort and Reduce and after: the stable order by all 64 bits, bit for bit; reduce_kernel's runs start and end
    at every position of a lane's 8, at a 2048-entry tile, and span tiles."""
    kernels, facts, _ = run_child("vectors", REAL[family], {"ARES_SORT_FUSE": "0"})
    for case, log in kernels.items():
        assert not _has(log, "sr_") and "reduce_kernel" in log, (case, log)
        assert log.get("radix_pass_kernel") == facts[case]["top_half_passes"], (case, log.get("radix_pass_kernel"), facts[case])
        assert log["sort_fixup_detect_kernel"] == log["sort_fixup_long_kernel"] == len(facts[case]["rows"]), (case, log)
    if family == "fixup":
        f = {c.split(":")[0]: v for c, v in facts.items()}
        assert f["fixup_short"]["listed"] == [[10, 1, 0]] and f["fixup_long"]["listed"] == [[0, 10, 0]], f
        assert f["fallback_beyond"]["listed"][0][2] == 1 and f["fallback_claims"]["listed"][0][1] == 513 and f["fallback_list"]["listed"][0][0] == 256
        assert [f[n]["top_half_passes"] for n in FIXUP + FALLBACK] == [4, 4, 12, 12, 12, 12], f
        assert all(short >= 6 and long_ >= 1 for short, long_, _ in f["three_batches"]["listed"][1:]), f["three_batches"]


@pytest.mark.parametrize("family", list(REAL))
def test_real_sort_eight_passes(family):
    """ARES_SORT_TOPBITS=0: all eight passes, no fix-up — compared with the same model, so the bytes are those of the top-half
    path on every input."""
    kernels, facts, _ = run_child("vectors", REAL[family], {"ARES_SORT_FUSE": "0", "ARES_SORT_TOPBITS": "0"})
    for case, log in kernels.items():
        assert not _has(log, "sr_", "sort_fixup") and log.get("radix_pass_kernel") == 8 * len(facts[case]["rows"]), (case, log)


def test_a_host_that_reads_between_sort_and_reduce_gets_the_real_sort():
    """Default switches: Sort over vectors the host wrote is only DEFINED; reading the hash / index vector makes it run."""
    wanted = _with_aggs(["fixup_short", "collisions64", "sentinels64_prev", "three_batches", "runs_heads"])
    kernels, facts, _ = run_child("vectors", wanted, {})
    for case, log in kernels.items():
        assert log.get("radix_pass_kernel") == facts[case]["top_half_passes"] and "reduce_kernel" in log, (case, log)


# ---- the wide layout over rows that exist ----------------------------------------------------------------------------------------
def _assert_wide(case, log, declined):
    assert _has(log, "sr_vector_scan_rtc") and _has(log, "sr_split_kernel") and _has(log, "sr_merge_kernel"), (case, log)
    assert bool(_has(log, "radix_pass_kernel", "reduce_kernel")) == declined, (case, declined, log)


WIDE = {
    # variant -> (environment, cases)
    "natural": ({}, _every_agg(COLLISIONS) + _with_aggs(SENTINELS + ["sentinels64_nulls"] + WIDE_SLOTS + ["three_batches", "runs_span", "runs_heads"])),
    "1_partition": ({"ARES_SRV_PART_BITS": "0"}, _every_agg(_clusters("wide", 0, tails=(-8, 0))) + ["clusters_wide_p0_tail+8:sum_u32", "clusters_wide_p0_tail+8:avg"]),
    "8_partitions": ({"ARES_SRV_PART_BITS": "3"}, _every_agg(_clusters("wide", 3, tails=(-8, 0)), ["sum_u32", "sum_u64", "min_f32", "avg"])
                     + ["clusters_wide_p3_tail+8:max_u32", "clusters_wide_p3_tail+8:sum_u64"] + _with_aggs(_partitions(3) + ["sentinels64_no_empty"])),
    "4096_partitions": ({"ARES_SRV_PART_BITS": "12"}, _with_aggs(_partitions(12)[:2] + ["collisions64_b3", "sentinels64_no_empty", "sentinels64_uuid_no_empty"], shift=1)),
}


@pytest.mark.parametrize("variant", list(WIDE))
def test_wide_layout_over_vectors_the_host_wrote(variant):
    """Default switches, a host that does not look between the calls: fused_sort_reduce_vectors — generated vector scan, split,
    2048-slot tables (kTail 128), emit — natural and forced partition counts (ARES_SRV_PART_BITS: one level, and two).  Any
    slot widths ((8, 4, 4), UUID) and validity bytes (a null slot with its chosen value bytes) ride here: the vectors carry the
    bytes the model hashed.  Declined to the real sort, and still the model's bytes: an input that holds the hash 2^64 - 1
    (the tables' empty word), and a cluster of kTail + 8 keys homed in the last home bucket (it runs off the table's end with
    a tenth of kMaxGroups); kTail - 8 and kTail keys there must NOT be declined."""
    env, wanted = WIDE[variant]
    kernels, facts, _ = run_child("vectors_unread", wanted, env)
    for case, log in kernels.items():
        _assert_wide(case, log, declined=_holds_empty_word(case) or "tail+8" in case)


@pytest.mark.parametrize("variant", ["natural", "8_partitions"])
def test_wide_layout_behind_an_eager_host(variant):
    """The rows come out of transforms and the host looks at them before it sorts: the wide layout again, and from the second
    batch on the previous result's row hashes are known — each partition's range of them is found by sr_bounds_kernel (the
    partitions inputs: lowest and highest hash of every partition, ranges that end exactly at a bound, empty partitions)."""
    env = {} if variant == "natural" else {"ARES_SRV_PART_BITS": "3"}
    wanted = _with_aggs(["collisions64", "collisions64_b3", "three_batches", "sentinels64_no_empty"] + _partitions(3), S.ALL_AGGS)
    kernels, facts, _ = run_child("columns_eager", wanted, env)
    for case, log in kernels.items():
        assert _has(log, "sr_split_kernel") and _has(log, "sr_merge_kernel") and not _has(log, "radix_pass_kernel", "reduce_kernel"), (case, log)
        if len(facts[case]["rows"]) > 1:
            assert _has(log, "sr_bounds_kernel"), (case, log)


def test_scan_fed_path_switched_off_hands_over_to_the_wide_layout():
    """ARES_SR_SCAN_FED=0: the pending transforms are launched and the groups ordered over the rows they wrote; a host that
    reads the vectors afterwards sees what a sort would have left."""
    wanted = _with_aggs(["collisions64_b3", "three_batches", "partitions_bounds_p3", "sentinels64_no_empty"], S.ALL_AGGS, 2)
    for mode in ("columns", "columns_read"):
        kernels, _, _ = run_child(mode, wanted, {"ARES_SR_SCAN_FED": "0"})
        for case, log in kernels.items():
            assert _has(log, "transform_") and not _has(log, "sr_scan_rtc"), (case, log)
            if mode == "columns":
                assert _has(log, "sr_split_kernel") and not _has(log, "radix_pass_kernel"), (case, log)


# ---- the scan-fed path -----------------------------------------------------------------------------------------------------------
SCAN_FED = {
    "natural": ({}, _every_agg(COLLISIONS) + _with_aggs(["sentinels64_no_empty", "three_batches", "runs_heads", "runs_span", "partitions_bounds_p0"])),
    "4_partitions": ({"ARES_MIN_PART_BITS": "2"}, _every_agg(_clusters("narrow4", 2), AGGS4) + _with_aggs(_partitions(2) + ["collisions64_b3"])),
    "8_partitions": ({"ARES_MIN_PART_BITS": "3"}, _every_agg(_clusters("narrow8", 3), AGGS8) + _with_aggs(_partitions(3) + ["collisions64_b3"], shift=1)),
    "512_partitions": ({"ARES_MIN_PART_BITS": "9"}, _with_aggs(["partitions_bounds_p9", "partitions_alternating_p9", "collisions64_b3", "sentinels64_no_empty"], shift=2)),
}


@pytest.mark.parametrize("variant", list(SCAN_FED))
def test_scan_fed_path(variant):
    """The dimensions are bare Uint32 columns whose transforms are still pending at Sort: fused_sort_reduce_run — the generated
    scan hashes the source columns, one 8192- or 6912-slot table per partition (kTail 256) orders the groups, the emit
    re-evaluates the representatives (a collision's group comes out under its FIRST row's dimensions).  Natural and forced
    partition counts: every partition's lowest and highest hash, families that differ in the partition bits only, empty
    partitions between full ones, a previous result found by binary search over its known hashes.  clusters: 4, 5, 200 and
    1000 keys with one home bucket each, ascending / descending / shuffled, two clusters that grow into one — every key of one
    partition, whose record streams overflow once or twice (the stream slack grows for the process, the call starts again)
    and must then hold them.  A cluster of kTail + 8 keys homed in the last home bucket runs off the table: declined — the wide
    layout or the real sort takes the call; with kTail - 8 and kTail keys (run first: the slack they leave holds 16 more
    rows) nothing may be declined."""
    env, wanted = SCAN_FED[variant]
    kernels, facts, _ = run_child("columns", wanted, env)
    for case, log in kernels.items():
        declined = "tail+8" in case
        assert _has(log, "sr_scan_rtc") and _has(log, "sr_merge_kernel") and bool(_has(log, "transform_")) == declined, (case, log)
        assert bool(_has(log, "radix_pass_kernel", "reduce_kernel", "sr_split_kernel")) == declined, (case, log)


def test_scan_fed_all_rows_in_one_of_512_partitions_are_handed_on():
    """2000 rows in ONE of 512 partitions: its record streams cannot hold them at any slack, the call is declined and the wide
    layout orders the groups over the rows the transforms then write."""
    kernels, _, _ = run_child("columns", ["partitions_one_p9:sum_u32", "partitions_one_p9:sum_u64"], {"ARES_MIN_PART_BITS": "9"})
    for case, log in kernels.items():
        assert _has(log, "sr_scan_rtc") and _has(log, "transform_") and _has(log, "sr_split_kernel", "radix_pass_kernel"), (case, log)


def test_more_than_the_tables_or_streams_hold_takes_the_real_sort():
    """fixup_long holds segments of 4095 and 4096 distinct hashes at neighbouring top halves: more groups in ONE partition than
    a table orders (kMaxGroups: 6448 / 1560), on the scan-fed path and then on the wide layout — the real sort finishes the
    call.  partitions_one_p12: 2000 rows in one of 4096 partitions arrive in one level-1 stream of the wide layout, which no
    slack makes hold them."""
    kernels, _, _ = run_child("columns", ["fixup_long:sum_u32", "fixup_long:sum_u64"], {})
    for case, log in kernels.items():
        assert _has(log, "sr_scan_rtc") and _has(log, "sr_merge_kernel") and log.get("radix_pass_kernel") == 4 and "reduce_kernel" in log, (case, log)
    kernels, _, _ = run_child("vectors_unread", ["fixup_long:min_i32", "partitions_one_p12:max_u32"], {"ARES_SRV_PART_BITS": "12"})
    for case, log in kernels.items():
        assert _has(log, "sr_vector_scan_rtc") and _has(log, "radix_pass_kernel") and "reduce_kernel" in log, (case, log)


def test_scan_fed_sort_materialises_for_a_host_that_looks():
    """The host reads the hash / index vector between Sort and Reduce and after: the defined sort is run, the vectors are the
    model's."""
    wanted = _with_aggs(["collisions64_b3", "three_batches", "sentinels64_prev", "fixup_short"], S.ALL_AGGS, 1)
    kernels, facts, _ = run_child("columns_read", wanted, {})
    for case, log in kernels.items():
        assert log.get("radix_pass_kernel") == facts[case]["top_half_passes"], (case, log, facts[case])


EMPTY_WORD = re.compile(r"fused_sort_reduce_run: .* emptykey 1\b")
EMPTY_WORD_WIDE = re.compile(r"fused_sort_reduce_vectors: .* emptykey 1\b")


@pytest.mark.parametrize("bits", [None, 3], ids=["natural", "8_partitions"])
def test_the_empty_word_takes_the_real_sort(bits):
    """A hash of 0xFFFFFFFFFFFFFFFF — first and last row of the batch (the straight-line "round one" over home buckets meets
    it), in the middle, and already in the previous result — raises the tables' empty-key flag on the scan-fed path and on
    the wide layout (the library's trace says so for both), and the real sort finishes the call; an all-ones high word over
    another low word, and the reverse, are ordinary keys (sentinels64_no_empty, on the table paths above)."""
    env = {"ARES_HR_TRACE": "1", **({"ARES_MIN_PART_BITS": str(bits), "ARES_SRV_PART_BITS": str(bits)} if bits else {})}
    wanted = _with_aggs(["sentinels64", "sentinels64_first_last", "sentinels64_prev"], ["sum_u32", "sum_u64", "min_f32", "avg"], bits or 0)
    kernels, facts, stderr = run_child("columns", wanted, env)
    for case, log in kernels.items():
        assert _has(log, "sr_scan_rtc") and log.get("radix_pass_kernel", 0) >= 4 and "reduce_kernel" in log, (case, log)
    assert len(EMPTY_WORD.findall(stderr)) >= len(wanted) and len(EMPTY_WORD_WIDE.findall(stderr)) >= len(wanted), stderr[-3000:]


# ---- the batch executor ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [None, 3], ids=["natural", "8_partitions"])
@pytest.mark.parametrize("mode", ["mirror", "driver"])
def test_through_the_batch_executor(mode, bits):
    """The same batches as a query with use_hash_reduction off, through the Python mirror and the C++ driver: the fetched rows
    in order and their values are the model's; the scan-fed kernels ran and no row was sorted."""
    env = {"ARES_MIN_PART_BITS": str(bits)} if bits else {}
    wanted = _with_aggs(["collisions64", "collisions64_b3", "three_batches", "sentinels64_no_empty"] + _partitions(3), S.INT_AGGS + ["max_f32", "sum_f32"])
    kernels, _, _ = run_child(mode, wanted, env)
    for case, log in kernels.items():
        assert _has(log, "sr_scan_rtc") and _has(log, "sr_merge_kernel") and not _has(log, "radix_pass_kernel", "reduce_kernel"), (case, log)


# ---- slots of 8 and 16 bytes -----------------------------------------------------------------------------------------------------
def test_wide_slots_through_transforms():
    """The (8, 4, 4) and UUID layouts as Int64 / UUID columns through Noop transforms (the path tests/test_wide_slot_sort.py
    drives): the rows exist when Sort arrives, the wide layout's generated scan hashes slots of 16 / 8 / 4 bytes."""
    wanted = _with_aggs(["sentinels64_844_no_empty", "sentinels64_uuid_no_empty"], ["sum_u32", "sum_u64", "max_f32", "avg"])
    for mode in ("columns", "columns_read"):
        kernels, facts, _ = run_child(mode, wanted, {})
        for case, log in kernels.items():
            if mode == "columns":
                _assert_wide(case, log, declined=False)
            else:
                assert log.get("radix_pass_kernel") == facts[case]["top_half_passes"], (case, log)
