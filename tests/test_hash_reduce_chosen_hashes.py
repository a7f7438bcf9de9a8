"""HashReduce at CHOSEN 32-bit row hashes, on every path that reaches it, against the exact model of tests/hash_model.py.

In the partitioned kernels everything that decides correctness is a function of the row's hash — the partition (top
partBits bits), the table slot (low 13 bits; a bucket of four by the low 11 in the generated kernels), the merge round (a
sub-range of the kept bits), the group itself — and several paths exist only for particular hashes: the generated tables'
empty marker 0xFFFFFFFF, their flag bits 0x40000000 / 0x80000000 and key 0, probe chains that wrap from the last slot to
slot 0, merge rounds narrowed to a few thousand hash values at the very top of the range, a partition's record region
overflowing.  Random keys never get there.  tests/hash_sets.py builds rows FOR such hashes (murmur3 inverted in its first
block); every case below runs them in a child process per environment (the library latches its switches), which compares
groups, the key -> value map and — the map's keys — the emitted representative rows with the model, bit for bit, and
prints the kernel log; the tests here assert from that log, from the child's stderr or from the decline message that the
path they are named for ran.

What a deliberate one-line break of the code under test would do (argued from the cases' construction; such breaks are
never committed or run):
  * the generated TABLE scan without its EMPTY test (`q.spill = h == EMPTY`, `h != EMPTY` in the first probe): a row whose
    hash is 0xFFFFFFFF "matches" every empty slot, is aggregated into a slot whose key stays EMPTY and is never flushed —
    the 0xFFFFFFFF group of sentinels / sentinels_first_last / sentinels_prev / collisions loses rows or vanishes
    (test_generated_table_scan);
  * in_round's upper bound inclusive (`u <= hi`): a hash whose left-aligned kept bits equal a round's end is merged and
    emitted by two rounds; narrow_* force rounds of 4096 consecutive values and hold the values at their boundaries, so
    the group count comes out one too high per boundary (test_generic_lds[narrow], test_generated_table_scan[narrow],
    test_generated_direct_scan_hands_a_crowded_partition_to_the_generic_merge);
  * the `at < ws.capA` guards' fallback skipped (no overflow word): the records behind a full region A are dropped and
    nothing falls back — skew_overflow ends with fewer groups than rows (test_skew_overflow_*);
  * HMASK one bit narrower: the two hashes that differ only in their highest kept bit (hash_sets.sentinel_hashes) become one
    key — one group too few (test_generated_direct_scan).  HMASK one bit WIDER is not observable by any input: the extra
    bit is the lowest partition bit, equal for every key of a workgroup's table (at partBits = 2 it is the OCC bit itself).
"""
import json
import os
import re
import subprocess

import pytest

import harness as H
import hash_paths as P
import hash_sets as S

pytestmark = pytest.mark.gpu

_SWITCHES = ("ARES_RTC", "ARES_HASH_REDUCE", "ARES_MIN_PART_BITS", "ARES_LEAN_MIN_GROUPS", "ARES_COMPACT", "ARES_IMAGE",
             "ARES_GROUPED", "ARES_FUSE", "ARES_DEFER", "ARES_HR_TRACE")
OVERFLOW_LINE = "hash-partition region overflowed"
_LDS_AGGS = ["sum_u32", "sum_i64", "min_i32", "sum_f32", "max_u32", "sum_i32", "min_u32", "sum_f64", "max_i32"]

FAMILIES = {
    "sentinels": ["sentinels_prev", "sentinels", "sentinels_first_last", "sentinels_1d", "sentinels_3d", "sentinels_4d"],
    "collisions": ["collisions", "collisions_flat", "collisions_4d"],
    "chains": ["chains", "chains_dup4"],
    "narrow": ["narrow_top", "narrow_bottom", "narrow_middle", "narrow_top_dup2"],
}
TWO_BYTE_SLOT = ["sentinels_4x2", "collisions_4x2", "chains_4x2"]


def _with_aggs(names, aggs, shift=0):
    return [f"{n}:{aggs[(i + shift) % len(aggs)]}" for i, n in enumerate(names)]


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


def _ran(log, *names):
    return all(n in log for n in names)


# ---- plain HashReduce over materialised vectors -----------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_generic_lds(family):
    """The precompiled partition + merge kernels (TABLE-mode flushes into region A, the multi-round merge), low- and
    high-duplicate inputs, one to four dimensions, every LDS aggregate.  Of hr_partition4_kernel only TABLE mode runs: a
    workgroup turns to DIRECT mode on its second tile at the earliest, which takes more than 256 x 4096 rows — no chosen-hash
    input reaches DIRECT mode of the generic kernel or its spill of a full private stream (the log shows the kernel's name only).
    narrow: more groups (7500) than one merge round holds (7040) inside 8192 consecutive hash values, at the top of the
    range (ending at 0xFFFFFFFF), at the bottom and in between — merge_body must narrow its rounds to that scale and emit
    every group once.  Its loop terminates: `width` halves on every discarded round while a completed round advances `lo` by
    at least one value, and a round of width one holds a single hash value — one group — which cannot overflow the table."""
    wanted = _with_aggs(FAMILIES[family], _LDS_AGGS, list(FAMILIES).index(family))
    kernels, _, stderr = run_child("plain", wanted, {"ARES_RTC": "0"})
    for case, log in kernels.items():
        assert _ran(log, "hr_partition4_kernel", "hr_merge_kernel") and "hash_insert_kernel" not in log, (case, log)
    assert OVERFLOW_LINE not in stderr


def test_generic_layout_with_a_two_byte_slot():
    """ndw with a 2-byte dimension behind the inverted 4-byte one: the layout-generic partition kernel."""
    kernels, _, _ = run_child("plain", _with_aggs(TWO_BYTE_SLOT, _LDS_AGGS), {"ARES_RTC": "0"})
    for case, log in kernels.items():
        assert _ran(log, "hr_partition_kernel", "hr_merge_kernel") and "hash_insert_kernel" not in log, (case, log)


def test_global_table_forced():
    """ARES_HASH_REDUCE=global: one global table, linear probing — the chains are its probe sequences."""
    names = ["sentinels_prev", "sentinels_first_last", "collisions", "collisions_4x2", "chains", "chains_dup4", "narrow_top"]
    kernels, _, _ = run_child("plain", _with_aggs(names, _LDS_AGGS, 2), {"ARES_HASH_REDUCE": "global"})
    for case, log in kernels.items():
        assert "hash_insert_kernel" in log and not [k for k in log if k.startswith("hr_")], (case, log)


def test_global_table_takes_avg_and_float_min_max():
    """The aggregates the LDS path does not serve take the global table on the default setting."""
    wanted = ["sentinels_prev:avg", "collisions:min_f32", "chains:max_f32", "chains_dup4:avg", "narrow_top:avg",
              "sentinels_first_last:max_f32", "collisions_flat:avg"]
    kernels, _, _ = run_child("plain", wanted, {})
    for case, log in kernels.items():
        assert "hash_insert_kernel" in log and not [k for k in log if k.startswith("hr_")], (case, log)


# ---- generated kernels, reached through the batch executor --------------------------------------------------------------------
def _shape(prog):
    """what the library keys a first batch's cardinality by, as far as these plans differ: dimensions and null columns"""
    return (prog.nd, tuple(all(o[d] for o in prog.batches[0][1]) for d in range(prog.nd)))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_generated_table_scan(family):
    """ARES_MIN_PART_BITS=2, fewer groups than ARES_LEAN_MIN_GROUPS: a batch behind a previous result, and a first batch
    whose plan shape (dimensions, null columns, measure) was last seen with few groups, take the TABLE scan generated for
    the shape, whose 32-bit keys use 0xFFFFFFFF as the empty marker; the generic merge follows (narrow: in rounds, over
    region A).  One aggregate per child, so shapes repeat; a case whose shape the child has not seen runs twice, and in
    front of every narrow case a small one brings the shape's cardinality down again (those runs carry a third field in
    their id, are compared with the model like every run, and prove no path)."""
    programs = S.all_programs()
    wanted, seen = [], set()
    for i, n in enumerate(FAMILIES[family]):
        if family == "narrow":
            wanted.append(f"sentinels:sum_u32:small{i}")
        elif _shape(programs[n]()) not in seen:
            wanted.append(f"{n}:sum_u32:first")
        seen.add(_shape(programs[n]()))
        wanted.append(f"{n}:sum_u32")
    kernels, facts, _ = run_child("fused", wanted, {"ARES_MIN_PART_BITS": "2"})
    for case, log in kernels.items():
        batches = len(facts[case]["rows"])
        assert facts[case]["fused_batches"] == batches, facts[case]
        if case.count(":") == 1:
            assert log.get("hr_table_scan_rtc", 0) == batches and "hr_fused_merge_kernel" in log, (case, log)
            assert not [k for k in log if k in ("hr_fused_scan_kernel", "hr_scan_rtc", "hash_insert_kernel")], (case, log)


@pytest.mark.parametrize("mode,agg", [("mirror", "sum_u32"), ("driver", "sum_f64")])
def test_generated_table_scan_and_merge_with_a_two_byte_slot(mode, agg):
    """A plan with a 2-byte slot runs on generated kernels only: TABLE scan into region A, generated merge (keys
    (h & HMASK) | OCC, empty = 0) reading region A; through the Python mirror and the C++ driver (pending transforms
    consumed by HashReduce)."""
    kernels, _, _ = run_child(mode, [f"{n}:{agg}" for n in TWO_BYTE_SLOT], {})
    for case, log in kernels.items():
        assert _ran(log, "hr_table_scan_rtc", "hr_merge_rtc") and not [k for k in log if k.startswith("transform_")], (case, log)


# variant -> (mode, environment, aggregate, programs): one aggregate per child keeps the number of generated kernels down
# (compact lines exist from 8 partitions on: ARES_MIN_PART_BITS=2 means 16-byte lines whatever ARES_COMPACT says)
_DIRECT = {
    "lines16_p2_fused": ("fused", {"ARES_LEAN_MIN_GROUPS": "0", "ARES_MIN_PART_BITS": "2", "ARES_COMPACT": "0"}, "sum_u32",
                         ["images", "sentinels", "collisions", "chains_dup4"]),
    "compact_p3_fused": ("fused", {"ARES_LEAN_MIN_GROUPS": "0", "ARES_MIN_PART_BITS": "3"}, "sum_i64",
                         ["images", "sentinels_first_last", "collisions_flat", "chains"]),
    "lines16_p3_driver": ("driver", {"ARES_LEAN_MIN_GROUPS": "0", "ARES_MIN_PART_BITS": "3", "ARES_COMPACT": "0"}, "min_i32",
                          ["images_3d", "sentinels_prev", "collisions_4d"]),
    "lines16_p2_mirror": ("mirror", {"ARES_LEAN_MIN_GROUPS": "0", "ARES_MIN_PART_BITS": "2"}, "sum_f64",
                          ["images", "sentinels_3d", "collisions", "chains"]),
}


@pytest.mark.parametrize("variant", list(_DIRECT))
def test_generated_direct_scan(variant):
    """ARES_LEAN_MIN_GROUPS=0: every batch through the generated DIRECT scan (16-byte lines, or compact lines where the
    batch allows them) and the generated merge.  Keys are (h & HMASK) | OCC with NEWG for this call's groups and 0 for
    empty: hashes 0, the flag patterns, all-zero / all-one kept bits, families that differ in the partition bits or in the
    highest kept bit only, bucket chains of 750 that wrap to bucket 0 (a chain is one partition's: its streams may overflow
    and the call start again with more room, but it must end on these kernels — no call is declined, nothing reaches
    hash_reduce_lds or the global table).
    images: three batches that fit the result vectors the first one allocated, so the table image survives — the first merge
    leaves an image (mode 1), the next two start from it (mode 2), append only new groups and leave the measure vector to
    be written when the host fetches it."""
    mode, env, agg, names = _DIRECT[variant]
    kernels, facts, _ = run_child(mode, [f"{n}:{agg}" for n in names], env)
    for case, log in kernels.items():
        assert _ran(log, "hr_scan_rtc", "hr_merge_rtc"), (case, log)
        assert not [k for k in log if k in ("hash_insert_kernel", "hr_merge_kernel", "hr_fused_scan_kernel", "hr_table_scan_rtc")], (case, log)
        if case.startswith("images"):
            assert log["hr_merge_rtc"] >= 3 and "hr_image_values_kernel" in log, (case, log)
            assert not [k for k in log if k in ("hr_partition4_kernel", "hr_fused_merge_kernel")], (case, log)
        if mode == "fused":
            assert facts[case]["fused_batches"] == len(facts[case]["rows"]), facts[case]


@pytest.mark.parametrize("env", [{"ARES_MIN_PART_BITS": "2", "ARES_COMPACT": "0"}, {"ARES_MIN_PART_BITS": "3"}], ids=["lines16_p2", "compact_p3"])
def test_generated_direct_scan_hands_a_crowded_partition_to_the_generic_merge(env):
    """7500 groups of one partition inside 8192 consecutive hash values at the top of the range, among ordinary rows: the
    DIRECT scan's streams of that partition overflow once or twice (the stream slack grows, the call starts again), the
    generated merge raises its crowded-partition word, and the generic multi-round merge takes the same records — 16-byte
    lines and compact lines — in rounds narrowed to that interval."""
    wanted = ["narrow_crowded:sum_u32", "narrow_crowded:sum_i64"]
    kernels, facts, _ = run_child("fused", wanted, {"ARES_LEAN_MIN_GROUPS": "0", **env})
    for case, log in kernels.items():
        assert _ran(log, "hr_scan_rtc", "hr_merge_rtc", "hr_fused_merge_kernel"), (case, log)
        assert "hash_insert_kernel" not in log and "hr_merge_kernel" not in log and facts[case]["fused_batches"] == 1, (case, log)


# ---- skew: all rows distinct, all in one partition --------------------------------------------------------------------------
def test_skew_absorbed_by_region_a():
    """12000 rows in one of 512 partitions: 300 times the partition's share, still inside its region A (16529 records,
    hash_sets.region_a_capacity) — no overflow, no fallback.  sentinels_p9: every partition's lowest and highest hash and the
    partition-bit family at 512 partitions.
    (The other spill — a full PRIVATE stream into region A, hr_kernels.hpp partition_body — needs a workgroup's second tile:
    more than 256 x 4096 rows.  No quick test reaches it.)"""
    kernels, _, stderr = run_child("plain", ["skew_absorbed:sum_u32", "sentinels_p9:sum_i64"], {"ARES_RTC": "0", "ARES_MIN_PART_BITS": "9"})
    for case, log in kernels.items():
        assert _ran(log, "hr_partition4_kernel", "hr_merge_kernel") and "hash_insert_kernel" not in log, (case, log)
    assert OVERFLOW_LINE not in stderr


@pytest.mark.parametrize("case,env", [("skew_overflow:sum_i32", {"ARES_MIN_PART_BITS": "9"}), ("skew_overflow_natural:sum_f64", {}),
                                      ("skew_three_batches:sum_u32", {"ARES_MIN_PART_BITS": "9"})],
                         ids=["17000_rows_512_partitions", "33000_rows_natural", "three_batches"])
def test_skew_overflow_falls_back_to_the_global_table(case, env):
    """Region A of the one partition overflows (17000 rows > 16529 records at 512 partitions; 33000 rows > 24657 at the
    natural 8): outCount[1] is raised, hash_reduce_lds returns -1 and says so on stderr, the global table takes the call —
    with a previous result in the input vectors, and with an ordinary batch behind it (three_batches)."""
    kernels, _, stderr = run_child("plain", [case], {"ARES_RTC": "0", **env})
    assert _ran(kernels[case], "hr_partition4_kernel", "hr_merge_kernel", "hash_insert_kernel"), kernels[case]
    assert OVERFLOW_LINE in stderr, stderr[-2000:]


# the library's own account of a fused attempt (ARES_HR_TRACE): the skewed batch of skew_lazy, tried while the previous
# result's values are defined by its table image only, from that image
LAZY_AT_THE_DECLINE = re.compile(rf"fused_hash_reduce_run: batch {S.SKEW_LAZY} prev \d+ .*image 1 lazy 1\).* -> image mode 2 ")


@pytest.mark.parametrize("lean", [False, True], ids=["table_scan", "direct_scan_lazy_values"])
def test_skew_fused_call_is_declined_and_leaves_the_previous_result(lean):
    """AresFusedFilterHashReduce, result vectors allocated once; the skewed batch is declined with the overflow message
    AFTER the attempt has written into the output vectors; the previous result's dimension rows are in place and its values,
    read back, are the model's; the per-node sequence (whose HashReduce overflows again, down to the global table) gives the
    model's result, and so does the batch behind it.
    table_scan: ordinary / skewed / ordinary on the generated TABLE scan (region A overflows).
    direct_scan_lazy_values: ordinary / ordinary / skewed / ordinary on the DIRECT kernels — the second batch is an
    image-mode-2 merge, so at the decline the previous result's measure vector has never been written: the library's trace
    of the skewed attempt must say `lazy 1` and `image mode 2`, and hr_image_values_kernel writes the values when they are
    read back.  The DIRECT scan's streams overflow, the process-wide stream slack grows twice, then the call is declined; a
    second, ordinary query in the same process is right with the grown slack."""
    env = {"ARES_MIN_PART_BITS": "9", **({"ARES_LEAN_MIN_GROUPS": "0", "ARES_HR_TRACE": "1"} if lean else {})}
    wanted = ["skew_lazy:sum_i64", "collisions:sum_i64"] if lean else ["skew_three_batches:sum_u32"]
    # (direct_scan_lazy_values: fused results are not read between batches — reading the measure vector writes it)
    kernels, facts, stderr = run_child("fused_calls_unread" if lean else "fused_calls", wanted, env)
    f, log, at = facts[wanted[0]], kernels[wanted[0]], 2 if lean else 1
    assert f["declined"][:at] == [None] * at and f["declined"][at] is not None, f["declined"]
    assert f["declined"][at].startswith("not fusable: a hash partition overflowed"), f["declined"]
    assert f["prev_intact"][at] is True, f
    assert OVERFLOW_LINE in stderr and "hash_insert_kernel" in log, (log, stderr[-1000:])
    if lean:
        assert LAZY_AT_THE_DECLINE.search(stderr), [ln[22:] for ln in stderr.splitlines() if ln.startswith("fused_hash_reduce_run: batch 16")]
        assert _ran(log, "hr_scan_rtc", "hr_merge_rtc", "hr_image_values_kernel"), log
        for case in wanted[1:]:
            assert facts[case]["declined"] == [None] * len(facts[case]["rows"]) and _ran(kernels[case], "hr_scan_rtc", "hr_merge_rtc"), facts[case]
    else:
        assert "hr_table_scan_rtc" in log, log


@pytest.mark.parametrize("lazy", [False, True], ids=["table_scan", "direct_scan_lazy_values"])
@pytest.mark.parametrize("mode", ["fused", "driver", "mirror"])
def test_skew_through_the_batch_executor(mode, lazy):
    """The same batches as a query, compared by the result the host fetches.  fused: the C++ driver's fused call is declined
    for the skewed batch, the driver latches the decline (no fused batch behind it) and the per-node sequence finishes the
    query.  driver / mirror: the per-node sequence from the start — HashReduce tries the pending queue fused, launches the
    transforms when the attempt overflows (they show in the kernel log), and falls back to the global table.
    direct_scan_lazy_values: skew_lazy on the DIRECT kernels; its batches fit the vectors the host allocated for the first,
    so the skewed attempt meets a previous result whose values are lazy (the library's trace says so)."""
    case = "skew_lazy:sum_i64" if lazy else "skew_three_batches:sum_i64"
    env = {"ARES_MIN_PART_BITS": "9", **({"ARES_LEAN_MIN_GROUPS": "0", "ARES_HR_TRACE": "1"} if lazy else {})}
    kernels, facts, stderr = run_child(mode, [case], env)
    assert "hash_insert_kernel" in kernels[case] and OVERFLOW_LINE in stderr, (kernels[case], stderr[-1000:])
    if lazy:
        assert LAZY_AT_THE_DECLINE.search(stderr), [ln[22:] for ln in stderr.splitlines() if ln.startswith("fused_hash_reduce_run: batch 16")]
    if mode == "fused":
        assert facts[case]["fused_batches"] == (2 if lazy else 1), facts[case]
    else:
        assert [k for k in kernels[case] if k.startswith("transform_")], kernels[case]
