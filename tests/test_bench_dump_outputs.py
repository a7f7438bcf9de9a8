"""bench.py --dump-outputs DIR: the group table of the last timed step as .npy files (float32 / float64 only, bounded in
size, rows in ascending order of their dimensions), identical from run to run with the same arguments — what two builds
of the project are compared on.  Here on the oracle backend (bench.main's injected backend, as in
tests/test_bench_distributed.py)."""
import json
import os
import sys

import numpy as np
import torch

import harness as H

sys.path.insert(0, H.ROOT)
import bench  # noqa: E402
from aresdb_amd import check, workload  # noqa: E402

NAMES = sorted([f"dim{q}_{what}.npy" for q in range(4) for what in ("value", "valid")] + ["measure.npy"])


def _load(directory):
    assert sorted(os.listdir(directory)) == NAMES
    return {n[:-4]: np.load(os.path.join(directory, n)) for n in NAMES}


def test_dump_is_the_last_steps_table_and_repeats(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))  # (bench_full.json lands there)
    argv = ["--gpus", "1", "--rows", "6000", "--batch-rows", "2500", "--steps", "2", "--warmup", "0", "--full", "--no-cpu-baseline",
            "--no-legs"]
    for d in ("a", "b"):
        assert bench.main(argv + ["--dump-outputs", str(tmp_path / d)], backend=H.oracle_backend(), tensor_device="cpu") == 0
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["check_groups"]["status"] == "ok"
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    groups = line["config"]["groups_per_shard"]
    for name, arr in a.items():
        assert arr.dtype == (np.float32 if name.endswith("_valid") else np.float64), name
        assert arr.shape == (groups,), name
        assert np.array_equal(arr, b[name]), name  # the same arguments: the same inputs, the same arrays
    assert _ascending(a)
    # the dumped arrays ARE the result: they pass the key-level check the benchmark runs on what it fetched
    fetched = ([a[f"dim{q}_value"].astype(np.uint32).tobytes() for q in range(4)],
               [a[f"dim{q}_valid"].astype(np.uint8).tobytes() for q in range(4)], a["measure"].tobytes())
    shard = workload.c3_shard(6000, 2500, seed=1, device=torch.device("cpu"), null_fraction=0.01)
    rep = check.compare_result(fetched, check.exact_groups(shard), hash_identity=True)
    assert rep["status"] == "ok" and rep["groups"] == groups > 1000, rep


def test_plain_run_times_and_dumps_but_measures_and_checks_nothing_else(tmp_path, capsys, monkeypatch):
    """Without --full: the contract keys and the same dump as with it, and none of what --full adds is even started."""
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    argv = ["--gpus", "1", "--rows", "6000", "--batch-rows", "2500", "--steps", "2", "--warmup", "1"]
    assert bench.main(argv + ["--full", "--dump-outputs", str(tmp_path / "full")], backend=H.oracle_backend(), tensor_device="cpu") == 0
    full = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert full["check_groups"]["status"] == "ok"

    def never(*a, **kw):
        raise AssertionError("a plain run went beyond its timed steps")
    for name in ("cpu_baseline", "host_batch_leg", "measure_traffic", "run_leg"):
        monkeypatch.setattr(bench, name, never)
    for name in ("exact_groups", "compare_result"):
        monkeypatch.setattr(bench.check, name, never)
    backend = H.oracle_backend()
    monkeypatch.setattr(backend, "has_profiler", True, raising=False)
    monkeypatch.setattr(backend, "profiler_enable", never, raising=False)
    assert bench.main(argv + ["--dump-outputs", str(tmp_path / "plain")], backend=backend, tensor_device="cpu") == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "scaling", "data"):
        assert line[k] == full[k], k
    assert line["steps"] == 2 and line["warmup"] == 1 and line["higher_is_better"] is True and line["unit"] == "rows/s"
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 / 6000 - 1) < 1e-4  # rows / step time
    assert line["config"]["groups_per_shard"] == full["config"]["groups_per_shard"] > 1000
    for k in ("check_groups", "check_merged_groups", "reference_host_check", "roofline", "cpu_baseline"):
        assert line[k] is None, k
    a, b = _load(tmp_path / "plain"), _load(tmp_path / "full")
    assert all(np.array_equal(a[k], b[k]) for k in a)


def _ascending(a):
    """rows strictly ascending by (dim0 valid, dim0 value, dim1 valid, ...): Python's tuple order"""
    rows = list(zip(*[a[f"dim{q}_{what}"].tolist() for q in range(4) for what in ("valid", "value")]))
    return all(x < y for x, y in zip(rows, rows[1:]))


def test_large_table_is_cut_to_a_fixed_sample_of_its_rows(tmp_path, monkeypatch):
    n = 5000
    rng = np.random.default_rng(7)
    dims = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(3)] + [np.arange(n, dtype=np.uint32)]
    dims[0] %= 3  # (ties on the leading dimensions: the later ones decide)
    valids = [(rng.random(n) < 0.9).astype(np.uint8) for _ in range(4)]
    meas = rng.random(n)
    fetched = ([d.tobytes() for d in dims], [v.tobytes() for v in valids], meas.tobytes())
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 * 1000)
    for d in ("a", "b"):
        kept, of = bench.dump_outputs(str(tmp_path / d), fetched)
        assert of == n and 1000 < kept < n
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in NAMES) <= 64 * 1000
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # one set of rows for every array: each dumped row is a row of the table, and they come in ascending order
    rows = np.array([int(np.flatnonzero(meas == m)[0]) for m in a["measure"]])
    assert len(rows) == kept == len(set(rows.tolist()))
    assert _ascending(a)
    for q in range(4):
        assert np.array_equal(a[f"dim{q}_value"], dims[q][rows].astype(np.float64))  # uint32 is exact in float64
        assert np.array_equal(a[f"dim{q}_valid"], valids[q][rows].astype(np.float32))
