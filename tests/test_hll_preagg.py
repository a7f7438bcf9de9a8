"""HyperLogLog's pre-aggregation stage (aresdb_amd/csrc/algo/hll.hip): on large batches a generated scan deals {key, row,
value} records out to partitions by a scramble of the key, one workgroup per partition folds them in an LDS table (max value,
min row), and the radix sort and the run reduce see the surviving entries instead of the rows.  What a host can observe after
every call must stay what the row sort leaves — and what the oracle computes — bit for bit, for any key distribution; a batch
the stage cannot take (record streams overflow under a few hot keys) declines to the row sort before anything is written."""
import ctypes as C

import numpy as np
import pytest

import cases
import harness as H
from aresdb_amd import abi, smoke
from aresdb_amd.executor import Binary, Col, Const, DimensionSpec, QueryPlan, Unary

pytestmark = pytest.mark.gpu

NEW_KERNELS = ("hll_scan_rtc", "hll_dedup_kernel")


def hip():
    return H.hip_backend()


def _kernels_of(b, fn):
    b.profiler_enable(True)
    try:
        res = fn()
        b.wait()
        return res, b.profiler_report()
    finally:
        b.profiler_enable(False)


def _stats(b):
    """{batches pre-aggregated, batches declined after the scan, rows of the former, their surviving entries}"""
    c = (C.c_ulonglong * 4)()
    b._algo.AresHllPreaggStats.argtypes, b._algo.AresHllPreaggStats.restype = [C.POINTER(C.c_ulonglong)], None
    b._algo.AresHllPreaggStats(c)
    return [int(x) for x in c]


def _temp_stats(b):
    out, cached = C.c_size_t(0), C.c_size_t(0)
    b._algo.AresTempStats.argtypes, b._algo.AresTempStats.restype = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], None
    b._algo.AresTempStats(C.byref(out), C.byref(cached))
    return out.value, cached.value


@pytest.fixture
def forced(monkeypatch):
    """The stage takes every batch, however small, and keeps no memory of the previous one's outcome."""
    def set_env(**extra):
        env = {"ARES_HLL_PREAGG": "1", "ARES_HLL_PREAGG_MIN_ROWS": "0"}
        env.update(extra)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        hip().reload_env()
    set_env()
    yield set_env
    for k in ("ARES_HLL_PREAGG", "ARES_HLL_PREAGG_MIN_ROWS", "ARES_HLL_PREAGG_TABLE_KEYS"):
        monkeypatch.delenv(k, raising=False)
    hip().reload_env()


def _run_counted(c):
    """(result, batches pre-aggregated, batches declined, rows, survivors) of one run on the HIP backend"""
    b = hip()
    before = _stats(b)
    res = c.run(b)
    after = _stats(b)
    return (res,) + tuple(x - y for x, y in zip(after, before))


# ---- 1. the stage runs, and the sort sees entries --------------------------------------------------------------------------
def test_new_kernels_launch_and_the_sort_runs_once_per_batch(forced, monkeypatch):
    c = cases.HllCase(810, batches=4, batch_rows=20000, groups=40, registers=1 << 14)
    c.run(hip())  # (kernels compiled and loaded)
    b = hip()
    before = _stats(b)
    _, report = _kernels_of(b, lambda: c.run(b))
    took = _stats(b)[0] - before[0]
    assert took == 4, (took, report)
    for name in NEW_KERNELS:
        assert report[name][0] == 4, report
    assert report["sort_key_hist_kernel"][0] == 4 and "sort_hash_hist_kernel" not in report, report
    assert report["radix_pass_kernel"][0] == 8 * 4 and report["hll_reduce_kernel"][0] == 4, report
    monkeypatch.setenv("ARES_HLL_PREAGG", "0")
    b.reload_env()
    _, report = _kernels_of(b, lambda: c.run(b))
    for name in NEW_KERNELS + ("sort_key_hist_kernel",):
        assert name not in report, report
    assert report["sort_hash_hist_kernel"][0] == 4 and report["radix_pass_kernel"][0] == 8 * 4, report


def test_default_threshold_keeps_small_batches_on_the_row_sort():
    b = hip()
    b.reload_env()
    c = cases.HllCase(811, batches=2, batch_rows=5000, groups=5, registers=1 << 14)
    _, report = _kernels_of(b, lambda: c.run(b))
    for name in NEW_KERNELS:
        assert name not in report, report


# ---- 2. bit-exact against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(820, 830))
def test_every_layout_matches_the_oracle(forced, seed):
    """seed % 5 walks the five layouts (4; 1; 4 2 1; 8 1 1; 16 4): null dimensions, register counts and group counts drawn."""
    rng = np.random.default_rng(seed)
    c = cases.HllCase(seed, batches=int(rng.integers(1, 5)), batch_rows=int(rng.choice([63, 4095, 8193, 30000])),
                      groups=int(rng.choice([1, 40, 5000])), registers=int(rng.choice([5000, 1 << 14])))
    res, took, declined, _, _ = _run_counted(c)
    cases.assert_same(res, c.run(H.oracle_backend()), repr(c))
    assert took + declined == len([s for s in c.sizes if s]), (took, declined, c)


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 4095, 4096, 8193, 300000])
@pytest.mark.parametrize("registers,groups", [(3, 1), (50, 40), (5000, 5000), (1 << 14, 40), (1 << 14, 1)])
def test_batch_sizes_registers_and_groups(forced, rows, registers, groups):
    seed = 840 + rows % 7 + registers % 5
    c = cases.HllCase(seed, batches=2, batch_rows=rows, groups=groups, registers=registers)
    cases.assert_same(c.run(hip()), c.run(H.oracle_backend()), repr(c))


@pytest.mark.parametrize("seed,ndw", [(850, (0, 0, 1, 0, 0)), (851, (0, 0, 0, 0, 1)), (852, (0, 0, 1, 1, 1)), (853, (0, 1, 0, 0, 2)),
                                      (854, (1, 0, 1, 0, 0)), (855, (0, 0, 8, 0, 0))])
def test_an_empty_batch_in_the_middle(forced, seed, ndw):
    """Four calls, the second one empty; sparse and dense dimensions in one result (group 0 is hot and crosses the dense
    threshold, the others stay sparse); every size, hash, value, index and dimension row of every call, the encoded vector
    and the register counts."""
    c = cases.HllCase(seed, batches=4, batch_rows=40000, groups=40, registers=1 << 14, ndw=ndw)
    c.sizes[1] = 0
    vals, valid, hll = c.batches[1]
    c.batches[1] = ([v[:0] for v in vals], valid[:0], hll[:0])
    res, took, declined, rows, survivors = _run_counted(c)
    want = c.run(H.oracle_backend())
    cases.assert_same(res, want, repr(c))
    assert (took, declined) == (3, 0) and rows == 3 * 40000 and 0 < survivors < rows, (took, declined, rows, survivors)
    reg = np.asarray(want["reg_counts"])
    assert (reg >= 4096).any() and (reg < 4096).any(), reg  # dense and sparse


# ---- 3. adversarial key distributions --------------------------------------------------------------------------------------
def _custom_case(seed, batches, capacity_slack=7):
    """An HllCase over one 4-byte dimension whose batches are given: [(dimension values uint32, hll values uint32)]."""
    c = cases.HllCase(seed, batches=len(batches), batch_rows=1, groups=1, registers=3, ndw=(0, 0, 1, 0, 0))
    c.sizes = [len(h) for _, h in batches]
    c.batches = [([np.ascontiguousarray(d.astype(np.uint32)).view(np.uint8).reshape(-1, 4)], np.ones((len(h), 1), np.uint8),
                  h.astype(np.uint32)) for d, h in batches]
    c.capacity = sum(c.sizes) + capacity_slack
    return c


def test_all_rows_one_key_declines_cleanly(forced):
    """Every record of the batch lands in one partition's streams: they overflow, the call sorts its rows — same bytes."""
    n = 50000
    rng = np.random.default_rng(860)
    c = _custom_case(860, [(np.full(n, 7), (rng.integers(0, 40, n) << 16) | 5)] * 2)
    res, took, declined, _, _ = _run_counted(c)
    cases.assert_same(res, c.run(H.oracle_backend()), repr(c))
    assert (took, declined) == (0, 2)
    assert res["size0"] == 1


def test_every_row_its_own_key(forced):
    """m = n: nothing folds; the stage is pure overhead and still exact."""
    n = 60000
    rng = np.random.default_rng(861)
    c = _custom_case(861, [(np.arange(n) + b * n, (rng.integers(0, 40, n) << 16) | rng.integers(0, 1 << 14, n)) for b in range(2)])
    res, took, declined, rows, survivors = _run_counted(c)
    cases.assert_same(res, c.run(H.oracle_backend()), repr(c))
    assert (took, declined) == (2, 0) and survivors == rows == 2 * n


def test_a_partition_overflows_its_table_many_times(forced):
    """A table emitted whenever it holds more than 16 keys after a chunk of 1024 records: with ~3000 records per partition
    every partition goes through several rounds and most of its ~100 keys survive more than once; the run reduce folds them
    (max value, min row)."""
    forced(ARES_HLL_PREAGG_TABLE_KEYS="16")
    c = cases.HllCase(862, batches=2, batch_rows=1600000, groups=3, registers=1 << 14)
    res, took, declined, rows, survivors = _run_counted(c)
    cases.assert_same(res, c.run(H.oracle_backend()), repr(c))
    distinct = res["size0"]  # (of the first batch; the second draws from the same keys)
    assert (took, declined) == (2, 0) and survivors > 3 * distinct, (took, declined, survivors, distinct)


def test_value_bits_14_and_15_do_not_split_a_key(forced):
    """The key takes the value's low 14 bits only: values that differ in bits 14-15 share a key and the whole 32-bit value
    decides the maximum."""
    n = 40000
    rng = np.random.default_rng(863)
    hll = (rng.integers(0, 40, n) << 16) | (rng.integers(0, 4, n) << 14) | rng.integers(0, 2000, n)
    c = _custom_case(863, [(rng.integers(0, 6, n), hll)])
    res, took, declined, _, _ = _run_counted(c)
    cases.assert_same(res, c.run(H.oracle_backend()), repr(c))
    assert (took, declined) == (1, 0)


def test_minimum_row_in_the_last_tile(forced):
    """Keys that occur in the batch's last (partial) 4096-row tile only, beside keys spread over all tiles: the index is the
    lowest row of each."""
    n = 3 * 4096 + 777
    rng = np.random.default_rng(864)
    dims = rng.integers(0, 4, n)
    hll = (rng.integers(0, 40, n) << 16) | rng.integers(0, 3000, n)
    dims[-500:] = 99  # a dimension row of the last tile only
    hll[-1] = (50 << 16) | 16383  # ... and a register the very last row carries alone
    c = _custom_case(864, [(dims, hll), (dims[::-1].copy(), hll[::-1].copy())])
    res, took, declined, _, _ = _run_counted(c)
    cases.assert_same(res, c.run(H.oracle_backend()), repr(c))
    assert (took, declined) == (2, 0)


# ---- 4. both paths agree ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [870, 871, 872, 873, 874])
def test_switch_on_and_off_leave_the_same_bytes(forced, monkeypatch, seed):
    c = cases.HllCase(seed, batches=3, batch_rows=50000, groups=[1, 40, 5000, 40, 7][seed % 5], registers=[1 << 14, 5000, 1 << 14, 50, 1 << 14][seed % 5])
    on = c.run(hip())
    monkeypatch.setenv("ARES_HLL_PREAGG", "0")
    hip().reload_env()
    before = _stats(hip())
    off = c.run(hip())
    assert _stats(hip()) == before
    cases.assert_same(on, off, repr(c))


# ---- 5. through the host driver, above the default threshold ---------------------------------------------------------------
def _numpy_registers(batches):
    """Registers per group, computed independently: murmur3_x64_128 of the user's 4 bytes, register = low 14 bits, rho =
    trailing zeros of the rest (query/functor.hpp:431-466); a null user counts as value 0 into register 0."""
    lib = C.CDLL(H.ORACLE_SO)
    lib.oracle_murmur3_128.argtypes = [C.c_char_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint64)]
    h = (C.c_uint64 * 2)()
    cache, out = {}, {}
    for cols, valid in batches:
        ts, d1, d3, user = (cols[k][1] for k in ("ts", "d1", "d3", "user"))
        n = len(ts)
        ok = {k: (np.ones(n, bool) if valid[k] is None else valid[k]) for k in cols}
        for i in np.nonzero((d1 < 90) & ok["d1"])[0]:
            key = ((np.uint32(ts[i] - ts[i] % 86400 if ok["ts"][i] else 0).tobytes(), int(ok["ts"][i])),
                   (np.uint32(d3[i]).tobytes(), int(ok["d3"][i])))
            reg, rho = 0, 0
            if ok["user"][i]:
                u = int(user[i])
                if u not in cache:
                    lib.oracle_murmur3_128(np.uint32(u).tobytes(), 4, 0, h)
                    r, rest, z = h[0] & 0x3FFF, h[0] >> 14, 0
                    while z + 14 < 32 and not (rest >> z) & 1:
                        z += 1
                    cache[u] = (r, z)
                reg, rho = cache[u]
            g = out.setdefault(key, {})
            g[reg] = max(g.get(reg, 0), rho + 1)
    return {k: sorted(v.items()) for k, v in out.items()}


def test_native_driver_above_the_default_threshold(monkeypatch):
    """No switch set: two batches of 1.25 M rows (about 1.1 M pass the filter) take the stage by default."""
    for k in ("ARES_HLL_PREAGG", "ARES_HLL_PREAGG_MIN_ROWS", "ARES_HLL_PREAGG_TABLE_KEYS"):
        monkeypatch.delenv(k, raising=False)
    b = hip()
    b.reload_env()
    rng = np.random.default_rng(880)
    data = []
    for n in (1250000, 1250000):
        cols, valid = smoke.synth_batch(rng, n, null_fraction=0.02)
        cols["user"] = (abi.Uint32, rng.integers(0, 30000, n).astype(np.uint32))
        valid["user"] = rng.random(n) >= 0.02
        data.append((cols, valid))
    plan = QueryPlan(filters=[Binary(abi.LessThan, Col("d1"), Const(90))],
                     dimensions=[DimensionSpec(Binary(abi.Floor, Col("ts"), Const(86400)), abi.Uint32), DimensionSpec(Col("d3"), abi.Uint32)],
                     measure=Unary(abi.GetHLLValue, Col("user")), agg=abi.AGGR_HLL, measure_type=abi.Uint32)
    before = _stats(b)
    got, _ = smoke.run_hll_query(b, plan, data, native=True)
    after = _stats(b)
    assert got == _numpy_registers(data)
    assert after[0] - before[0] == 2 and after[3] - before[3] < (after[2] - before[2]) // 2, (before, after)


# ---- 6. temporaries do not pile up -----------------------------------------------------------------------------------------
def test_stream_temporaries_return_to_their_level(forced):
    b = hip()
    c = cases.HllCase(890, batches=4, batch_rows=30000, groups=40, registers=1 << 14)
    c.run(b)
    b.wait()
    base, _ = _temp_stats(b)
    for _ in range(4):  # 16 batches
        c.run(b)
    b.wait()
    after, _ = _temp_stats(b)
    assert after == base, (base, after)
