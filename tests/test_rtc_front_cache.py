"""The map in front of the kernel cache (hr_rtc.hip: rtc_lookup) is keyed by the kernel's shape spec: comparison and + - x
constants are not part of it, divisors are, and the vector-sourced kernels go through it like the plan-sourced ones.  One
query shape — 4100 rows (a full 4096-row tile and a 4-row tail that straddles a quad), dimensions [Floor(ts, d), d1],
SUM(v + k) of an Int32 column, filter ts < c — run twice in one process; every result is the oracle's, and AresRtcWait's
counters say what was built."""
import os
import subprocess
import sys

import numpy as np
import pytest

import harness as H
from aresdb_amd import abi, smoke
from aresdb_amd.executor import Binary, Col, Const, DimensionSpec, QueryPlan

ROWS = 4100


def batch(rng):
    cols = {"ts": (abi.Uint32, rng.integers(0, 86400, ROWS).astype(np.uint32)),
            "d1": (abi.Uint32, rng.integers(0, 50, ROWS).astype(np.uint32)),
            "v": (abi.Int32, rng.integers(-1000, 1000, ROWS).astype(np.int32))}
    return cols, {k: rng.random(ROWS) >= 0.02 for k in cols}


def plan(c, k, d):
    return QueryPlan(filters=[Binary(abi.LessThan, Col("ts"), Const(c))],
                     dimensions=[DimensionSpec(Binary(abi.Floor, Col("ts"), Const(d)), abi.Uint32), DimensionSpec(Col("d1"), abi.Uint32)],
                     measure=Binary(abi.Plus, Col("v"), Const(k)), agg=abi.AGGR_SUM_SIGNED, measure_type=abi.Int64,
                     use_hash_reduction=True)


def _fusion_on():
    return all(os.environ.get(k, "1") != "0" for k in ("ARES_FUSE", "ARES_DEFER", "ARES_RTC"))


def _run_pair(monkeypatch, first, second):
    """Both plans over the same batch on the DIRECT-mode kernels; the counters after each."""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    data = [batch(np.random.default_rng(23))]
    monkeypatch.setenv("ARES_LEAN_MIN_GROUPS", "0")  # every batch to the generated kernels, whatever its cardinality
    monkeypatch.setenv("ARES_MIN_PART_BITS", "2")    # (the generated merge needs four partitions)
    hip.reload_env()
    states = []
    try:
        for p in (first, second):
            hip.profiler_enable(True)
            got = smoke.run_query(hip, p, data)[0]
            hip.wait()
            kernels = hip.profiler_report()
            hip.profiler_enable(False)
            smoke.compare_results(got, smoke.run_query(oracle, p, data)[0])
            if _fusion_on():
                assert any(k.startswith("hr_scan_rtc") for k in kernels) and any(k.startswith("hr_merge_rtc") for k in kernels), sorted(kernels)
            states.append(hip.rtc_wait())
    finally:
        monkeypatch.undo()
        hip.reload_env()
    return states


@pytest.mark.gpu
def test_new_constants_run_the_loaded_kernels(monkeypatch):
    """(c, k) = (50000, 7), then (20000, -3): the same shape, so the second query compiles nothing and reads nothing from disk."""
    a, b = _run_pair(monkeypatch, plan(50000, 7, 3600), plan(20000, -3, 3600))
    assert (b["compiles"], b["disk_hits"]) == (a["compiles"], a["disk_hits"]), (a, b)


@pytest.mark.gpu
def test_a_new_divisor_is_a_new_kernel(monkeypatch):
    """Floor(ts, 3600), then Floor(ts, 60): the divisor is a literal of the text, so a second scan (and merge) is built."""
    a, b = _run_pair(monkeypatch, plan(50000, 7, 3600), plan(50000, 7, 60))
    if _fusion_on():
        assert b["compiles"] + b["disk_hits"] > a["compiles"] + a["disk_hits"], (a, b)


_VECTOR_SCRIPT = r"""
import numpy as np, sys, os
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import harness as H
from aresdb_amd import smoke
import test_rtc_front_cache as T
hip, oracle = H.hip_backend(), H.oracle_backend()
p = T.plan(50000, 7, 3600)
# three batches each: the result vectors grow (and move) ahead of the second, the third meets a previous result that is known
# to be grouped by partition — what the vector-sourced scan starts from
for run, seed in enumerate((31, 32)):
    rng = np.random.default_rng(seed)
    data = [T.batch(rng), T.batch(rng), T.batch(rng)]
    hip.profiler_enable(True)
    got = smoke.run_query(hip, p, data)[0]
    hip.wait(); kernels = hip.profiler_report(); hip.profiler_enable(False)
    smoke.compare_results(got, smoke.run_query(oracle, p, data)[0])
    print("KERNELS", run, sorted(k for k in kernels if k.startswith(("hr_", "transform_"))))
    print("STATE", run, hip.rtc_wait())
"""


@pytest.mark.gpu
def test_vector_sourced_kernels_hit_the_front_cache():
    """ARES_FUSE=0: the transforms are launched and HashReduce runs on the materialised vectors (two 4-byte dimensions) with
    its generated vector-sourced scan and merge; the same query over other data finds both loaded."""
    env = {**os.environ, "ARES_FUSE": "0", "ARES_LEAN_MIN_GROUPS": "0", "ARES_MIN_PART_BITS": "2", "ARES_RTC_ASYNC": "0"}
    r = subprocess.run([sys.executable, "-c", _VECTOR_SCRIPT], cwd=H.ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    kernels = [ln for ln in r.stdout.splitlines() if ln.startswith("KERNELS")]
    states = [eval(ln.split(" ", 2)[2]) for ln in r.stdout.splitlines() if ln.startswith("STATE")]
    assert len(kernels) == 2 and len(states) == 2, r.stdout[-2000:]
    for ln in kernels:
        assert "hr_scan_rtc" in ln and "hr_merge_rtc" in ln and "transform_" in ln, ln
    assert (states[1]["compiles"], states[1]["disk_hits"]) == (states[0]["compiles"], states[0]["disk_hits"]), states
    assert states[0]["kernels"] >= 2, states
