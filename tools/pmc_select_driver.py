"""One unlimited non-aggregation batch of the trips-shaped select (tools/bench_configs.py select) through the C++ driver —
`ordinary` or `extension` — for a rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE pass of its own (tools/pmc_summary.py reads the CSVs)."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aresdb_amd import abi, trips
from aresdb_amd.driver import NativeQuery

path, n = sys.argv[1], int(float(sys.argv[2])) if len(sys.argv) > 2 else 1 << 25
be = abi.load_hip_backend(); be.call("BootstrapDevice")
dev = torch.device("cuda:0"); g = torch.Generator(device=dev); g.manual_seed(12)
batch = trips.trips_shard(n, n, seed=11, device=dev)[0]
batch["key"] = trips.key_column(n, g, dev)
torch.cuda.synchronize()
names = [c for c, _ in trips.COLUMNS] + ["key"]
for _ in range(2):
    q = NativeQuery(be, trips.trips_select_plan(limit=-1, fused=path == "extension"), names)
    q.run({k: rc.vp for k, rc in batch.items()}, n)
    print(path, "rows", q.result_size, "fused batches", q.fused_batches)
    q.release()
