"""Time dimensions that are constant chains — a fixed non-UTC zone, hour of day, time of day, hour of week
(aresdb_amd.queries.time_dimension, from query/time_bucketizer.go) — through the fused paths: the inner nodes' scratch frames are
DEFINED (deferral.hpp: FrameDef), the root composes into an ordinary queued job, and HashReduce / Sort + Reduce evaluate the
whole chain from the source column with the kernels generated for the plan's shape.  Results: the oracle's and the numpy model's
(tests/chain_model.py), bit for bit — fares are quarters, so float sums are exact in any order."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_model as M
import harness as H
from aresdb_amd import abi, smoke
from aresdb_amd.executor import Binary, Col, Const, DimensionSpec, QueryPlan, Unary

SIZES = (4099, 1, 5, 1025, 45000)  # odd, one row, under a tile, over a tile, many workgroups
STATUS = 2
SHAPES = ("fixed_zone_hour", "hour_of_day", "fixed_zone_time_of_day", "hour_of_week", "fixed_zone_hour_of_week", "two_chains")


def batches_of(seed, sizes=SIZES, null_fraction=0.02):
    """trips batches (request_at Uint32 over ten days from 1970-01-03, city_id Uint16, status Uint8, fare Float32); the first one
    carries the timestamps where a day, a week, the sign of local time and the 32-bit range turn, with status = STATUS"""
    rng = np.random.default_rng(seed)
    out = []
    for b, n in enumerate(sizes):
        cols = {"request_at": (abi.Uint32, (2 * 86400 + rng.integers(0, 10 * 86400, n)).astype(np.uint32)),
                "city_id": (abi.Uint16, rng.integers(0, 40, n).astype(np.uint16)),
                "status": (abi.Uint8, rng.integers(0, 4, n).astype(np.uint8)),
                "fare": (abi.Float32, (rng.integers(0, 400, n) / 4).astype(np.float32))}
        valid = {k: rng.random(n) >= null_fraction for k in cols}
        if b == 0:
            e = len(M.EDGE_TS)
            cols["request_at"][1][:e] = M.EDGE_TS
            cols["status"][1][:e] = STATUS
            valid["request_at"][:e] = True
            valid["status"][:e] = True
        out.append((cols, valid))
    return out


def plan_of(shape, count, offset=-28800):
    """The trips shape: the Go host's two time filters (here: the whole signed range, so that every valid timestamp passes) and
    status = k; grouped by the chain and city_id in its 2-byte slot.  "two_chains": two chain dimensions whose inner nodes reuse
    one scratch frame, city_id, and only the status filter — null timestamps reach the chains."""
    s = M.shapes(offset)
    city = DimensionSpec(Col("city_id"), abi.Uint16)
    status = Binary(abi.Equal, Col("status"), Const(STATUS))
    if shape == "two_chains":
        filters = [status]
        dims = [DimensionSpec(s["fixed_zone_hour"], abi.Uint32), city, DimensionSpec(s["hour_of_day"], abi.Uint32)]
    else:
        filters = [Binary(abi.GreaterThanOrEqual, Col("request_at"), Const(-2**31)),
                   Binary(abi.LessThanOrEqual, Col("request_at"), Const(2**31 - 1)), status]
        dims = [DimensionSpec(s[shape], abi.Uint32), city]
    if count:  # COUNT(*) through Sort + Reduce
        return QueryPlan(filters=filters, dimensions=dims, measure=Const(1), agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32,
                         use_hash_reduction=False)
    return QueryPlan(filters=filters, dimensions=dims, measure=Col("fare"), agg=abi.AGGR_SUM_FLOAT, measure_type=abi.Float64,
                     use_hash_reduction=True)


def model_of(shape, count, batches, offset=-28800):
    plan = plan_of(shape, count, offset)

    def keep(cols, valid):
        k = valid["status"] & (cols["status"][1] == STATUS)
        return k if shape == "two_chains" else k & valid["request_at"]

    def add(cols, valid):
        return np.ones(len(cols["fare"][1])) if count else np.where(valid["fare"], cols["fare"][1], 0).astype(np.float64)
    return M.grouped(plan.dimensions, batches, keep, add)


def exact(results):
    return {k: float(v) for k, v in results.items()}


@pytest.mark.parametrize("count", [False, True], ids=["sum_hash_reduce", "count_sort_reduce"])
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_agrees_with_the_model(shape, count):
    batches = batches_of(11, sizes=(700, 1, 300))
    got, _ = smoke.run_query(H.oracle_backend(), plan_of(shape, count), batches)
    assert exact(got) == model_of(shape, count, batches)


def _kernels_of(hip, fn):
    hip.profiler_enable(True)
    try:
        res = fn()
        hip.wait()
        return res, hip.profiler_report()
    finally:
        hip.profiler_enable(False)


def _fused_on():
    return all(os.environ.get(k, "1") != "0" for k in ("ARES_FUSE", "ARES_DEFER", "ARES_RTC", "ARES_CHAINS", "ARES_SORT_FUSE"))


@pytest.fixture(scope="module")
def shared():
    """the batches and, per (shape, count), the oracle's result and the model's: computed once"""
    batches = batches_of(23)
    cache = {}

    def expected(shape, count):
        if (shape, count) not in cache:
            want, _ = smoke.run_query(H.oracle_backend(), plan_of(shape, count), batches)
            cache[(shape, count)] = (exact(want), model_of(shape, count, batches))
        return cache[(shape, count)]
    return batches, expected


@pytest.mark.gpu
@pytest.mark.parametrize("count", [False, True], ids=["sum_hash_reduce", "count_sort_reduce"])
@pytest.mark.parametrize("native", [True, False], ids=["cpp_driver", "python_mirror"])
@pytest.mark.parametrize("shape", SHAPES)
def test_chain_plans_run_without_a_transform_kernel(shared, shape, native, count):
    """The Go call sequence: once the shape's kernels exist (the first run builds them) no kernel whose name starts with
    transform_ runs — no frame is written, no job launched — and the fused scan evaluates the chain.  On the code before chains,
    transform_fast_kernel wrote the inner frame and transform32_kernel read it."""
    hip = H.hip_backend()
    batches, expected = shared
    plan = plan_of(shape, count)
    run = smoke.run_query_native if native else smoke.run_query
    run(hip, plan, batches)
    (got, _), kernels = _kernels_of(hip, lambda: run(hip, plan, batches))
    want, model = expected(shape, count)
    assert exact(got) == want
    assert exact(got) == model
    if _fused_on():
        scans = ("sr_scan_rtc",) if count else ("hr_scan_rtc", "hr_table_scan_rtc")
        assert any(k.startswith(scans) for k in kernels), kernels
        assert not any(k.startswith("transform_") for k in kernels), kernels


_SCRIPT = r"""
import os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import harness as H
from aresdb_amd import smoke
import test_chain_plans as T
hip, oracle = H.hip_backend(), H.oracle_backend()
batches = T.batches_of(29, sizes=(4099, 5, 20000))
for shape in T.SHAPES:
    for count in (False, True):
        plan = T.plan_of(shape, count)
        smoke.run_query_native(hip, plan, batches)
        hip.profiler_enable(True)
        got = smoke.run_query_native(hip, plan, batches)[0]
        hip.wait(); kernels = hip.profiler_report(); hip.profiler_enable(False)
        assert T.exact(got) == T.exact(smoke.run_query(oracle, plan, batches)[0]), (shape, count)
        assert T.exact(got) == T.model_of(shape, count, batches), (shape, count)
        print("KERNELS", shape, int(count), sorted(k for k in kernels if k.startswith(("hr_", "sr_", "transform"))))
"""


def _run_script(env):
    r = subprocess.run([sys.executable, "-c", _SCRIPT], cwd=H.ROOT, env={**os.environ, **env}, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("KERNELS")]
    assert len(lines) == 2 * len(SHAPES), r.stdout[-2000:]
    return lines


@pytest.mark.gpu
def test_chain_plans_on_the_direct_kernels():
    """ARES_LEAN_MIN_GROUPS=0: every HashReduce batch takes the DIRECT scans and the generated merge, in a process of its own"""
    for ln in _run_script({"ARES_LEAN_MIN_GROUPS": "0"}):
        if _fused_on():
            assert "transform" not in ln, ln
            if " 0 " in ln:
                assert "hr_scan_rtc" in ln and "hr_merge_rtc" in ln and "hr_table_scan_rtc" not in ln, ln


@pytest.mark.gpu
def test_chains_switched_off_run_the_kernels_they_always_ran():
    """ARES_CHAINS=0: the inner node is written by transform_fast_kernel, the root reads the frame on transform32_kernel — and
    the results are the same"""
    for ln in _run_script({"ARES_CHAINS": "0"}):
        if all(os.environ.get(k, "1") != "0" for k in ("ARES_FUSE", "ARES_DEFER")):
            assert "transform_fast_kernel" in ln and "transform32_kernel" in ln, ln


@pytest.mark.gpu
@pytest.mark.parametrize("native", [True, False], ids=["cpp_driver", "python_mirror"])
def test_hyperloglog_over_an_hour_of_day_dimension(native):
    """HyperLogLog reads the batch's dimension rows: the queued chain job is launched (transform_multi_kernel / _fast_kernel
    evaluate the chain) and the registers are the oracle's"""
    hip = H.hip_backend()
    batches = batches_of(31, sizes=(4099, 1, 9000))
    plan = QueryPlan(filters=[Binary(abi.Equal, Col("status"), Const(STATUS))],
                     dimensions=[DimensionSpec(M.shapes()["hour_of_day"], abi.Uint32), DimensionSpec(Col("city_id"), abi.Uint16)],
                     measure=Unary(abi.GetHLLValue, Col("request_at")), agg=abi.AGGR_HLL, measure_type=abi.Uint32, use_hash_reduction=False)
    got, _ = smoke.run_hll_query(hip, plan, batches, native=native)
    want, _ = smoke.run_hll_query(H.oracle_backend(), plan, batches)
    assert len(want) > 100 and got == want
