"""SUM over full-mantissa floats through Sort + Reduce at scale: C3 under the reference's shipped configuration
(c3_plan(use_hash_reduction=False)), 40 Mi rows in three batches, a measure column that is NOT quantised — the first time the
float tolerance (rel = 1e-6, aresdb_amd/check.py) is exercised at this size.  Scan-fed, with the scan-fed path declining
everything (the wide layout over the rows the transforms wrote), and with float aggregates on the real sort.  Each runs in a
child process: the switches are read once per process."""
import json
import os
import subprocess
import sys

import pytest
import torch

import harness as H
from aresdb_amd import workload

ARGS = ["--rows", str(40 << 20), "--batch-rows", str(16 << 20)]  # 16 + 16 + 8 Mi rows
VARIANTS = [
    ("scan_fed", {}, ARGS),
    ("materialised_rows", {"ARES_SR_SCAN_FED": "0"}, ARGS),
    ("real_sort", {"ARES_SR_FLOAT": "0"}, ["--rows", str(20 << 20), "--batch-rows", str(8 << 20)]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,args", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_c3_float_sum_through_sort_reduce_at_scale(name, env, args):
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "scale_float_check.py"), *args], cwd=H.ROOT,
                       env={**os.environ, **env}, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    report = json.loads(lines[-1])
    assert r.returncode == 0 and report["status"] == "ok", report
    assert report["groups"] == report["expected_groups"] > 1_000_000
    assert report["batches"] >= 3 and report["result_sizes"][-1] == report["groups"]
    fused = all(os.environ.get(k, "1") != "0" for k in ("ARES_FUSE", "ARES_DEFER", "ARES_SORT_FUSE", "ARES_RTC", "ARES_SR_FLOAT", "ARES_SORT_VECTORS"))
    kernels = report["kernels"]
    if name == "real_sort":
        assert any(k.startswith("radix_pass_kernel") for k in kernels) and not any(k.startswith("sr_merge_kernel") for k in kernels), kernels
    elif fused:
        assert any(k.startswith("sr_merge_kernel") for k in kernels) and not any(k.startswith("radix_pass_kernel") for k in kernels), kernels
        assert any(k.startswith("sr_scan_rtc" if name == "scan_fed" else "sr_split_kernel") for k in kernels), kernels


def test_c3_measure_stays_quantised_unless_asked():
    """workload.c3_batch: the default measure is what it was (quarter steps: the benchmark's sums are exact in any order);
    quantised=False changes the measure column only."""
    dev = torch.device("cpu")
    a = workload.c3_shard(5000, 2048, seed=3, device=dev)
    b = workload.c3_shard(5000, 2048, seed=3, device=dev, quantised=True)
    c = workload.c3_shard(5000, 2048, seed=3, device=dev, quantised=False)
    assert len(a) == len(b) == len(c) == 3
    for x, y in zip(a, b):
        for name in x:
            assert torch.equal(x[name].blob, y[name].blob)
    m = torch.cat([x["m"].values() for x in a])
    assert torch.equal(m * 4, torch.round(m * 4)) and float(m.max()) < 100.0
    f = torch.cat([x["m"].values() for x in c])
    assert float(f.min()) >= 0.0 and float(f.max()) < 100.0 and not torch.equal(f * 4, torch.round(f * 4))
    for x, z in zip(a, c):
        assert torch.equal(x["ts"].blob, z["ts"].blob) and torch.equal(x["d1"].blob, z["d1"].blob)
