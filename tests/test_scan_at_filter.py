"""Scan at filter (AresHintFusedBatch, include/ares_extensions.h): a host that says what a batch will be before the batch's
filters has the batch's LAST filter counted by the compact DIRECT scan itself, and HashReduce merges what that scan wrote.

Every test runs the per-node sequence on the HIP backend and on the oracle and compares counts, keys and sums bit for bit
(the measures are drawn in quarter steps, so float sums are exact in any order).  ARES_LEAN_MIN_GROUPS=0 (the documented test
knob) sends these small batches to the DIRECT kernels and ARES_MIN_PART_BITS=3 gives them the eight partitions the compact
record format needs; one priming pass and rtc_wait() load the kernels first.

  honoured      the C++ driver (which sends the hint itself) and a per-node Python sequence with hints: counts returned by
                BinaryFilter, the result, AresScanAtFilterStats and the kernel log (no filter_rows_kernel launch)
  mispredicted  sequences that differ from their hint end in the oracle's result and in the right discard counter
  declined      a hint over a column shorter than the batch launches nothing
"""
import os

import numpy as np
import pytest

import harness as H
from aresdb_amd import abi, smoke
from aresdb_amd.columns import DeviceColumn
from aresdb_amd.executor import BatchContext, BatchExecutor, Binary, Col, Const, QueryPlan, column_input, constant_input, fetch_results
from aresdb_amd.queries import c3_plan

pytestmark = pytest.mark.gpu

_ENV = {"ARES_LEAN_MIN_GROUPS": "0", "ARES_MIN_PART_BITS": "3"}
# rows per batch: one row, the tile edge (4096 rows per tile), several tiles and a rest, and 257 tiles — 256 workgroups
# of two tiles each, of which the last 127 find their chunk empty
SIZES = [1, 4095, 4096, 4097, 3 * 4096 + 17, 257 * 4096]


@pytest.fixture
def hip():
    be = H.hip_backend()
    if not be.has_scan_at_filter:
        pytest.fail("libalgorithm.so exports no AresHintFusedBatch")
    saved = {k: os.environ.get(k) for k in list(_ENV) + ["ARES_HR_TRACE", "ARES_SCAN_AT_FILTER"]}
    os.environ.update(_ENV)
    be.reload_env()
    yield be
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    be.reload_env()
    be.rtc_wait()


def batches(sizes, seed, nulls=0.01, keep="some", few=True):
    """synth_batch's columns (m in quarter steps); keep = none / all: d1 fails / passes `d1 < 90` in every row.  few: a query of
    few groups, so that the host's result buffers (sized for the first batch's survivors plus an eighth) do not grow again:
    a previous result that has just moved to larger buffers is re-partitioned by HashReduce, which then takes no scan"""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        cols, valid = smoke.synth_batch(rng, n, null_fraction=nulls)
        if few:  # ten values of d1 pass the filter, one hour, d2 and d3 constant: some eighty groups with the null variants
            cols["ts"] = (abi.Uint32, rng.integers(0, 3600, n).astype(np.uint32))
            cols["d1"] = (abi.Uint32, rng.integers(80, 100, n).astype(np.uint32))
            cols["d2"] = (abi.Uint32, np.full(n, 3, np.uint32))
            cols["d3"] = (abi.Uint32, np.full(n, 1, np.uint32))
        if keep != "some":
            cols["d1"] = (abi.Uint32, np.full(n, 95, np.uint32) if keep == "none" else rng.integers(0, 90, n).astype(np.uint32))
            valid["d1"] = None
        out.append((cols, valid))
    return out


def three(n):
    return [n, n, max(1, n // 2)]  # (the third batch smaller)


def one_row_batches(seed):
    """three batches of one row, all of one group: the result (one group) outgrows its buffers (capacity 1) at the second
    batch only"""
    data = batches([1, 1, 1], seed=seed, nulls=0.0)
    for cols, _ in data:
        cols["d1"] = (abi.Uint32, np.full(1, 5, np.uint32))
    return data


def delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def as_bits(table):
    return {k: np.asarray(v).tobytes() for k, v in table.items()}


# ---- a per-node sequence with hints -----------------------------------------------------------------------------------------
def fused_expr(ctx, e, out_type):
    x = abi.FusedExpr()
    x.outType = out_type
    if isinstance(e, Col):
        x.lhs, x.arity, x.functor = column_input(ctx.columns[e.name]), 1, abi.Noop
    else:
        x.lhs, x.rhs, x.arity, x.functor = column_input(ctx.columns[e.lhs.name]), constant_input(e.rhs.value), 2, e.op
    return x


def fused_query(ctx, plan):
    q = abi.FusedQuery()
    q.numFilters, q.numDims, q.aggFunc = len(plan.filters), len(plan.dimensions), plan.agg
    for k, f in enumerate(plan.filters):
        q.filters[k] = fused_expr(ctx, f, abi.Bool)
    for d, dim in enumerate(plan.dimensions):  # (all four bytes wide: vector order = query order)
        q.dims[d] = fused_expr(ctx, dim.expr, dim.data_type)
    q.measure = fused_expr(ctx, plan.measure, plan.measure_type)
    return q


class Hinted(BatchExecutor):
    """The Python mirror of the batch executor with a hint before every batch's InitIndexVector.  `hint_plan(b)`: the plan
    the hint of batch b states (None: no hint); rows / prev: what it adds to the true batch size and result size;
    `after_filter(b, ctx)` runs between filter() and project(); a batch in `abandon` ends after its filters."""

    def __init__(self, ctx, hint_plan, rows=0, prev=0, after_filter=None, abandon=()):
        super().__init__(ctx)
        self.hint_plan, self.rows, self.prev, self.after_filter, self.abandon = hint_plan, rows, prev, after_filter, abandon
        self.batch, self.counts = -1, []
        inner = ctx.filter_action

        def counted(functor, inputs):
            inner(functor, inputs)
            self.counts[-1].append(ctx.size)
        ctx.filter_action = counted

    def pre_exec(self):
        c = self.ctx
        self.batch += 1
        self.counts.append([])
        plan = self.hint_plan(self.batch)
        if plan is not None and c.be.has_scan_at_filter:
            c.be.hint_fused_batch(fused_query(c, plan), c.size + self.rows, c.result_size + self.prev, plan.measure_bytes, c.stream, c.device)
        super().pre_exec()

    def join(self):
        super().join()
        if self.after_filter:
            self.after_filter(self.batch, self.ctx)

    def project(self):
        if self.batch in self.abandon:  # the host gives the batch up: its buffers go, no transform, no HashReduce
            c = self.ctx
            c.be.wait(c.stream, c.device)
            c.cleanup_before_aggregation()
            c.size = 0
            return
        super().project()

    def reduce(self):
        if self.batch not in self.abandon:
            super().reduce()

    def post_exec(self):
        if self.batch not in self.abandon:  # (nothing was reduced: the result stays where it is)
            super().post_exec()


def run_hinted(be, plan, data, **how):
    """(result {key: value bytes}, filter counts per batch) of the sequence with hints"""
    how.setdefault("hint_plan", lambda b: plan)
    # a stream of its own: what the library remembers per stream (the two-discard latch, the filters of the previous batch)
    # begins and ends with the run
    stream = be.call("CreateCudaStream", 0) or None
    ctx = BatchContext(be, plan, stream=stream)
    ex = Hinted(ctx, **how)
    for cols, valid in data:
        dev = {k: DeviceColumn(be, t, v, valid=valid[k], stream=stream) for k, (t, v) in cols.items()}
        ex.run({k: d.vp for k, d in dev.items()}, len(cols["m"][1]), owned_columns=[d.free for d in dev.values()])
    dims, valids, meas = fetch_results(ctx)
    ctx.release()
    be.call("DestroyCudaStream", stream, 0)
    n = len(valids[0]) if valids else 0
    m = meas.view(np.float64)
    table = {tuple((bytes(d[r * len(d) // n:(r + 1) * len(d) // n]), int(v[r])) for d, v in zip(dims, valids)): m[r].tobytes()
             for r in range(n)}
    return table, ex.counts


def numpy_counts(plan, data):
    """survivors after each filter of each batch: comparisons of a column with a constant, a null row fails"""
    ops = {abi.LessThan: np.less, abi.GreaterThanOrEqual: np.greater_equal}
    out = []
    for cols, valid in data:
        keep = np.ones(len(cols["m"][1]), bool)
        per = []
        for f in plan.filters:
            ok = valid[f.lhs.name]
            keep &= ops[f.op](cols[f.lhs.name][1], f.rhs.value) & (ok if ok is not None else True)
            per.append(int(keep.sum()))
            if per[-1] == 0:
                break
        out.append(per)
    return out


def check(hip, plan, data, expect, kernels_without=("filter_rows_kernel",), prime=True, **how):
    """primes, runs the hinted sequence on both backends, compares, and returns the counters' change over the HIP run"""
    want, want_counts = run_hinted(H.oracle_backend(), plan, data, **how)
    if prime:
        run_hinted(hip, plan, data, **how)  # priming pass: the kernels of these shapes are loaded afterwards
    hip.rtc_wait()
    before = hip.scan_at_filter_stats()
    hip.profiler_enable(True)
    try:
        got, got_counts = run_hinted(hip, plan, data, **how)
        hip.wait()
        kernels = {k.split("<")[0] for k in hip.profiler_report()}
    finally:
        hip.profiler_enable(False)
    change = delta(before, hip.scan_at_filter_stats())
    print("scan at filter:", change, sorted(kernels))
    assert got_counts == want_counts
    assert got == want and len(got) > 0
    check.last_change, check.last_kernels = change, kernels
    if expect is not None:
        assert change == expect, (change, expect)
    for k in kernels_without:
        assert k not in kernels, (k, sorted(kernels))
    return got_counts


C3 = c3_plan(True)
TIMED = QueryPlan(filters=[Binary(abi.GreaterThanOrEqual, Col("ts"), Const(600)), Binary(abi.LessThan, Col("ts"), Const(3000)),
                           Binary(abi.LessThan, Col("d1"), Const(90))],
                  dimensions=C3.dimensions, measure=C3.measure, agg=C3.agg, measure_type=C3.measure_type, use_hash_reduction=True)


# ---- honoured ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_driver_sends_the_hint_and_every_batch_is_honoured(hip, n):
    data = one_row_batches(n) if n == 1 else million_row_batches(n, n) if n > 100000 else batches(three(n), seed=n)
    want, _ = smoke.run_query_native(H.oracle_backend(), C3, data)
    # (one row: the second batch finds the result buffers full — capacity 1 —, the result moves, and its scan is not taken)
    expect = {"hints": 3, "scans": 3, "honoured": 3} if n > 1 else {"hints": 3, "scans": 3, "honoured": 2, "discard_shape": 1}
    smoke.run_query_native(hip, C3, data)  # priming pass
    hip.rtc_wait()
    before = hip.scan_at_filter_stats()
    hip.profiler_enable(True)
    try:
        got, _ = smoke.run_query_native(hip, C3, data)
        hip.wait()
        kernels = {k.split("<")[0] for k in hip.profiler_report()}
    finally:
        hip.profiler_enable(False)
    change = delta(before, hip.scan_at_filter_stats())
    print("scan at filter:", change, sorted(kernels))
    assert as_bits(got) == as_bits(want) and len(got) > 0
    assert change == expect, change
    assert "filter_rows_kernel" not in kernels and "hr_scan_rtc" in kernels, sorted(kernels)


def million_row_batches(n, seed):
    """two hours of ts and synth_batch's own dimensions — some twenty thousand groups, well below the eighth of the survivors
    the result buffers have to spare, evenly spread over the partitions; the third batch only three tiles smaller: at half
    the rows HashReduce chooses fewer partitions, re-partitions the previous result and, rightly, takes no scan"""
    data = batches([n, n, n - 3 * 4096], seed=seed, few=False)
    for cols, _ in data:
        cols["ts"] = (abi.Uint32, cols["ts"][1] % np.uint32(7200))
    return data


@pytest.mark.parametrize("n", SIZES)
def test_sequence_with_hints_returns_numpys_counts(hip, n):
    data = one_row_batches(100 + n) if n == 1 else million_row_batches(n, 100 + n) if n > 100000 else batches(three(n), seed=100 + n)
    expect = {"hints": 3, "scans": 3, "honoured": 3} if n > 1 else {"hints": 3, "scans": 3, "honoured": 2, "discard_shape": 1}
    counts = check(hip, C3, data, expect)
    assert counts == numpy_counts(C3, data)


def test_time_filter_pair_in_front(hip):
    data = batches(three(3 * 4096 + 17), seed=5)
    counts = check(hip, TIMED, data, {"hints": 3, "scans": 3, "honoured": 3}, kernels_without=())
    assert counts == numpy_counts(TIMED, data)


def run_child(body, env):
    """`body` (statements over T = this module and hip) in a process of its own, with the suite's switches and `env`;
    returns the finished process.  For what is latched per process: ARES_HR_TRACE, the record streams' slack."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, 'tests'); import harness as H, test_scan_at_filter as T; hip = H.hip_backend(); "
            + body + "; hip.rtc_wait()")
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                         env={**os.environ, **_ENV, "ARES_RTC_ASYNC": "0", **env}, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    return out


def test_over_a_table_image(hip):
    """ARES_HR_TRACE is read once per process: a child prints the trace; its merges of batches two and three start from the
    previous call's table image (image mode 2) over scans launched at the filter"""
    out = run_child("T.check(hip, T.C3, T.batches(T.three(3 * 4096 + 17), seed=6), {'hints': 3, 'scans': 3, 'honoured': 3})",
                    {"ARES_HR_TRACE": "1"})
    runs = [ln for ln in out.stderr.splitlines() if ln.startswith("fused_hash_reduce_run: batch")]
    assert sum("image mode 2" in ln for ln in runs[-3:]) == 2, runs[-3:]
    assert sum("scan at filter honoured" in ln for ln in out.stderr.splitlines()) == 6  # (priming pass and measured pass)


def test_filter_that_keeps_everything(hip):
    data = batches(three(4097), seed=7, keep="all")
    counts = check(hip, C3, data, {"hints": 3, "scans": 3, "honoured": 3})
    assert counts == [[4097], [4097], [2048]]


def chosen_hash_overflow(hip):
    """body of test_record_stream_overflow_at_chosen_hashes' child process"""
    import hash_paths as P
    import hash_sets as S
    prog, agg = S.all_programs()["skew_lazy"](), "sum_i64"
    data = []
    for cols, valid in P.column_batches(prog, agg):  # (every row passes the one filter: the hashes are the builders')
        cols["f"], valid["f"] = (abi.Uint32, np.ones(len(cols["m"][1]), np.uint32)), None
        data.append((cols, valid))
    base = P.query_plan(prog, agg)
    plan = QueryPlan(filters=[Binary(abi.LessThan, Col("f"), Const(2))], dimensions=base.dimensions, measure=base.measure, agg=base.agg,
                     measure_type=base.measure_type, use_hash_reduction=True)
    counts = check(hip, plan, data, {"hints": 4, "scans": 4, "honoured": 2, "retried": 1, "discard_shape": 1}, kernels_without=(), prime=False)
    assert counts == [[len(cols["m"][1])] for cols, _ in data], counts
    assert counts[2] == [S.SKEW_LAZY]
    assert "hash_insert_kernel" in check.last_kernels, check.last_kernels
    want, _ = run_hinted(H.oracle_backend(), plan, data)
    assert len(want) == len(prog.expected(agg)[0])  # (every group of the one partition is there)


def test_record_stream_overflow_at_chosen_hashes(hip):
    """hash_sets.skew_lazy — rows built for chosen hashes: ordinary / ordinary / 16700 DISTINCT groups all of ONE of 512
    partitions / ordinary, sized so that the host never reallocates — as a query with one filter that every row passes, in a
    fresh process (the record streams' slack grows for the process), once, without a priming pass (kernels are compiled
    inline), so that every counter is determined:
      batches one and two   scan at the filter, merged by HashReduce (the second from the first one's table image);
      the skewed batch      its scan, launched at the filter, overflows the one partition's record streams — it goes on
                            evaluating with its cursors clamped, so the filter's count is exact: 16700 —; HashReduce takes
                            the stash, finds the overflow flag, grows the slack and scans again, twice, then falls back to
                            the per-node sequence and the global table: one scan "retried", none honoured;
      the last batch        finds a previous result that is not grouped (the global table's): region A is needed, its scan
                            is dropped for that reason.
    The result is the oracle's, group for group."""
    run_child("T.chosen_hash_overflow(hip)", {"ARES_MIN_PART_BITS": "9"})


def test_filter_that_keeps_nothing_leaves_a_scan_that_dies_with_the_next_batch(hip):
    data = batches([4097], seed=8) + batches([4097], seed=9, keep="none") + batches([2048], seed=10)
    counts = check(hip, C3, data, {"hints": 3, "scans": 3, "honoured": 2, "discard_abandoned": 1})
    assert counts[1] == [0]


# ---- mispredicted -----------------------------------------------------------------------------------------------------------
def test_a_fourth_filter_follows_the_hinted_last_one(hip):
    data = batches(three(4097), seed=11)
    four = QueryPlan(filters=TIMED.filters + [Binary(abi.LessThan, Col("d2"), Const(40))], dimensions=C3.dimensions, measure=C3.measure,
                     agg=C3.agg, measure_type=C3.measure_type, use_hash_reduction=True)
    # the third filter is taken for the last: scanned, then replayed for the fourth; after two such batches the third hint is ignored
    counts = check(hip, four, data, {"hints": 2, "scans": 2, "discard_plan": 2, "latched": 1}, kernels_without=(), hint_plan=lambda b: TIMED)
    assert counts == numpy_counts(four, data)


def test_transforms_read_another_column_than_hinted(hip):
    data = batches([4097], seed=12)
    other = QueryPlan(filters=C3.filters, dimensions=[C3.dimensions[0], C3.dimensions[1], C3.dimensions[3], C3.dimensions[2]],
                      measure=C3.measure, agg=C3.agg, measure_type=C3.measure_type, use_hash_reduction=True)
    check(hip, C3, data, {"hints": 1, "scans": 1, "discard_plan": 1}, hint_plan=lambda b: other)


def test_wrong_previous_size(hip):
    data = batches([4097], seed=13)
    check(hip, C3, data, {"hints": 1, "scans": 1, "discard_shape": 1}, prev=1)


def test_hinted_column_overwritten_before_hash_reduce(hip):
    data = batches([4097], seed=14)
    fresh = (np.random.default_rng(15).integers(0, 400, 4097) / 4).astype(np.float32)

    def overwrite(b, ctx):  # the measure column's values: behind the validity bits of a mode-2 vector party
        vp = ctx.columns["m"]
        H.upload(ctx.be, vp.BasePtr + vp.ValuesOffset, fresh, ctx.stream)
    check(hip, C3, data, {"hints": 1, "scans": 1, "discard_touched": 1}, after_filter=overwrite)


def test_index_vector_read_between_filter_and_transforms(hip):
    data = batches([4097], seed=16)
    cols, valid = data[0]
    keep = (cols["d1"][1] < 90) & valid["d1"]
    seen = {}

    def read(b, ctx):
        seen[ctx.be.name] = H.download(ctx.be, ctx.index_vec, 4 * ctx.size, ctx.stream).view(np.uint32).copy()
    # (the copy applies the pending filters to the vector and ends the journal: the transforms are launched, HashReduce finds
    # nothing pending and reduces the materialised rows)
    check(hip, C3, data, {"hints": 1, "scans": 1, "discard_abandoned": 1}, after_filter=read)
    for name, vec in seen.items():
        assert np.array_equal(vec, np.nonzero(keep)[0].astype(np.uint32)), name


def test_hash_reduce_never_comes(hip):
    data = batches(three(4097), seed=17)
    check(hip, C3, data, {"hints": 3, "scans": 3, "honoured": 2, "discard_abandoned": 1}, abandon=(1,))


def test_latch_after_two_discards(hip):
    data = batches([4097] * 4, seed=18)
    check(hip, C3, data, {"hints": 2, "scans": 2, "discard_shape": 2, "latched": 2}, kernels_without=(), prev=1)


def test_hint_over_a_short_column_is_declined(hip):
    data = batches([4097], seed=19)
    check(hip, C3, data, {"declined": 1}, kernels_without=(), rows=1)


def test_switch_off(hip):
    os.environ["ARES_SCAN_AT_FILTER"] = "0"
    hip.reload_env()
    data = batches([4097], seed=20)
    check(hip, C3, data, {"declined": 1}, kernels_without=())


# ---- hints in a sequence fuzzer ---------------------------------------------------------------------------------------------
# tests/test_sequence_fuzz.py's Program issues its ABI calls itself and knows no point at which a hint could be given without
# editing it, so this is a small generator of its own over the executor above: seeded programs of two to four batches in
# one of three plan shapes, with a right hint, no hint or a wrong one (previous size, plan, rows) per batch, and — at random
# points — a read of every buffer a host can reach (index vector, predicate vector, a source column, the result so far) or
# a write into a hinted column.  Every observation must be the oracle's, on one host thread and on four at once: the
# per-stream hints and stashes, their mutex beside the deferral lock, and write / free hooks arriving from other threads.
FUZZ_SEED, FUZZ_PROGRAMS = 20260218, 32
_FUZZ_SIZES = [1, 700, 4095, 4096, 4097, 9000, 3 * 4096 + 17]


def _fuzz_plans(k):
    d1 = Binary(abi.LessThan, Col("d1"), Const(k))
    mk = lambda filters, dims=C3.dimensions: QueryPlan(filters=filters, dimensions=dims, measure=C3.measure, agg=C3.agg,  # noqa: E731
                                                      measure_type=C3.measure_type, use_hash_reduction=True)
    return [mk([d1]), mk(TIMED.filters[:2] + [d1]), mk([d1, Binary(abi.LessThan, Col("d2"), Const(40))]),
            mk([d1], [C3.dimensions[0], C3.dimensions[1], C3.dimensions[3], C3.dimensions[2]])]


class Fuzzed(Hinted):
    def __init__(self, ctx, program):
        self.program, self.obs = program, []
        super().__init__(ctx, hint_plan=lambda b: program["steps"][b]["hint"], after_filter=self.look)

    def pre_exec(self):
        step = self.program["steps"][self.batch + 1]
        self.rows, self.prev = step["rows"], step["prev"]
        super().pre_exec()

    def look(self, b, c):
        step = self.program["steps"][b]
        what = step["look"]
        self.obs.append(("counts", b, tuple(self.counts[b])))
        if c.size <= 0 or what == "nothing":
            return
        if what == "index":
            self.obs.append(("index", b, H.download(c.be, c.index_vec, 4 * c.size, c.stream).tobytes()))
        elif what == "predicate":  # (as the last filter left it: one byte per row that filter was called with)
            self.obs.append(("predicate", b, H.download(c.be, c.pred_vec, self.counts[b][-2] if len(self.counts[b]) > 1 else c.batch_rows,
                                                         c.stream).tobytes()))
        elif what == "column":
            vp = c.columns["d1"]
            self.obs.append(("column", b, H.download(c.be, vp.BasePtr + vp.ValuesOffset, 4 * c.batch_rows, c.stream).tobytes()))
        elif what == "write":  # a hinted column changes between the filter and HashReduce: the result reflects the new bytes
            vp = c.columns["m"]
            H.upload(c.be, vp.BasePtr + vp.ValuesOffset, step["fresh"], c.stream)

    def post_exec(self):
        super().post_exec()
        if self.program["steps"][self.batch]["result"]:
            dims, valids, meas = fetch_results(self.ctx)
            n = len(valids[0]) if valids else 0
            self.obs.append(("result", self.batch, tuple(sorted(
                (tuple(bytes(d[4 * r:4 * r + 4]) + bytes(v[r:r + 1]) for d, v in zip(dims, valids)), bytes(meas[8 * r:8 * r + 8])) for r in range(n)))))


def fuzz_program(seed):
    rng = np.random.default_rng(seed)
    plans = _fuzz_plans(int(rng.integers(80, 100)))  # (d1 lies in [80, 100): the constant 80 keeps nothing)
    shape = int(rng.integers(0, 3))
    sizes = [int(rng.choice(_FUZZ_SIZES)) for _ in range(int(rng.integers(2, 5)))]
    steps = []
    for n in sizes:
        kind = str(rng.choice(["right"] * 5 + ["none", "previous size", "plan", "columns", "rows"]))
        steps.append({"hint": None if kind == "none" else plans[(shape + 1) % 3] if kind == "plan" else plans[3] if kind == "columns" else plans[shape],
                      "prev": 1 if kind == "previous size" else 0, "rows": 1 if kind == "rows" else 0,
                      "look": str(rng.choice(["nothing"] * 4 + ["index", "predicate", "column", "write"])),
                      "fresh": (rng.integers(0, 400, n) / 4).astype(np.float32), "result": bool(rng.integers(0, 3) == 0)})
    return {"seed": seed, "plan": plans[shape], "data": batches(sizes, seed), "steps": steps}


def run_fuzzed(be, program):
    stream = be.call("CreateCudaStream", 0) or None
    ctx = BatchContext(be, program["plan"], stream=stream)
    ex = Fuzzed(ctx, program)
    for cols, valid in program["data"]:
        dev = {k: DeviceColumn(be, t, v, valid=valid[k], stream=stream) for k, (t, v) in cols.items()}
        ex.run({k: d.vp for k, d in dev.items()}, len(cols["m"][1]), owned_columns=[d.free for d in dev.values()])
    dims, valids, meas = fetch_results(ctx)
    n = len(valids[0]) if valids else 0
    ex.obs.append(("final", len(program["data"]), tuple(sorted(
        (tuple(bytes(d[4 * r:4 * r + 4]) + bytes(v[r:r + 1]) for d, v in zip(dims, valids)), bytes(meas[8 * r:8 * r + 8])) for r in range(n)))))
    ctx.release()
    be.call("DestroyCudaStream", stream, 0)
    return ex.obs


def _same_observations(got, want, seed):
    assert len(got) == len(want), (seed, len(got), len(want))
    for g, w in zip(got, want):
        assert g[:2] == w[:2], (seed, g[:2], w[:2])
        assert g == w, (seed, g[:2], "differs from the oracle's")


@pytest.mark.parametrize("threads", [1, 4])
def test_random_programs_with_right_and_wrong_hints(hip, threads):
    import threading
    programs = [fuzz_program(FUZZ_SEED + k) for k in range(FUZZ_PROGRAMS)]
    oracle = H.oracle_backend()
    want = [run_fuzzed(oracle, p) for p in programs]
    before = hip.scan_at_filter_stats()
    got, errors = [None] * len(programs), []

    def work(t):
        try:
            for k in range(t, len(programs), threads):
                got[k] = run_fuzzed(hip, programs[k])
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))
    if threads == 1:
        work(0)
    else:
        pool = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
        for th in pool:
            th.start()
        for th in pool:
            th.join()
    assert not errors, errors
    for p, g, w in zip(programs, got, want):
        _same_observations(g, w, p["seed"])
    change = delta(before, hip.scan_at_filter_stats())
    print("scan at filter:", change)
    # Every scan launched at a filter ended in exactly one of the outcomes.  On one thread the programs do reach the honoured
    # path; with four, another thread's entry points flush the device's pending queues (every entry point does), so a
    # HashReduce seldom still finds its batch's transforms pending and most scans end "abandoned": nothing is asked of the mix.
    ended = sum(change.get(k, 0) for k in ("honoured", "discard_plan", "discard_shape", "discard_touched", "discard_abandoned", "retried"))
    assert change.get("scans", 0) == ended and change.get("scans", 0) >= FUZZ_PROGRAMS // 2, change
    if threads == 1:
        assert change.get("honoured", 0) >= FUZZ_PROGRAMS // 8, change
