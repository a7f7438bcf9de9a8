#!/usr/bin/env python3
"""The headline query under the reference's SHIPPED configuration (enable_hash_reduction: false — SUM(m) into float64 through
Sort + Reduce) at sizes only the GPU reaches, with a measure column of full-mantissa floats, as a child process (the path
switches are read once per process):

    python tests/scale_float_check.py --rows R --batch-rows B

Runs c3_plan(use_hash_reduction=False) through the C++ host driver on the HIP libraries and compares group count, every
(dimension row -> sum) at rel = 1e-6 — the project's float tolerance — and the order of the rows (ascending 64-bit row hash)
with the independent exact group-by of aresdb_amd/check.py.  Prints one JSON report; exit code 1 on mismatch."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from aresdb_amd import abi, check, workload  # noqa: E402
from aresdb_amd.driver import NativeQuery  # noqa: E402
from aresdb_amd.queries import c3_plan  # noqa: E402

NAMES = [n for n, _ in workload.C3_COLUMNS]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=float(40 << 20))
    ap.add_argument("--batch-rows", type=float, default=float(16 << 20))
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--streams", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    be = abi.load_hip_backend()
    be.call("BootstrapDevice")
    streams = [be.call("CreateCudaStream", 0) for _ in range(args.streams)]
    batches = workload.c3_shard(int(args.rows), int(args.batch_rows), seed=args.seed, device=dev, quantised=False)
    torch.cuda.synchronize()
    plan = c3_plan(use_hash_reduction=False)
    ctx = NativeQuery(be, plan, NAMES, device=0, stream=streams[0], streams=streams)
    sizes = []
    be.profiler_enable(True)
    for b in batches:
        ctx.run({k: rc.vp for k, rc in b.items()}, next(iter(b.values())).length)
        sizes.append(ctx.result_size)
    kernels = sorted(be.profiler_report())
    be.profiler_enable(False)
    report = check.compare_result(ctx.fetch(), check.exact_groups(batches), hash_identity=False, rel=1e-6, ordered=True)
    report.update({"kernels": kernels, "rows": int(args.rows), "batch_rows": int(args.batch_rows), "batches": len(batches),
                   "result_sizes": sizes, "env": {k: v for k, v in os.environ.items() if k.startswith("ARES_")}})
    ctx.release()
    for s in streams:
        be.call("DestroyCudaStream", s, 0)
    print(json.dumps(report), flush=True)
    sys.exit(0 if report["status"] == "ok" else 1)


if __name__ == "__main__":
    main()
