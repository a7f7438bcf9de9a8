"""AresHintFusedBatch is optional for a host: the C++ driver binds it when the library has it and runs unchanged — the same
calls, the same result — against a library that does not (the oracle), and the Python binding says which is which."""
import numpy as np

import harness as H
from aresdb_amd import smoke
from aresdb_amd.queries import c3_plan


def test_driver_runs_unchanged_against_a_library_without_the_hint():
    oracle = H.oracle_backend()
    assert not oracle.has_scan_at_filter
    assert not hasattr(oracle._algo, "AresHintFusedBatch") and not hasattr(oracle._algo, "AresScanAtFilterStats")
    rng = np.random.default_rng(3)
    data = [smoke.synth_batch(rng, n, null_fraction=0.01) for n in (4097, 4097, 2048)]
    native, native_calls = smoke.run_query_native(oracle, c3_plan(True), data)
    mirror, mirror_calls = smoke.run_query(oracle, c3_plan(True), data)
    assert len(native) > 1000
    assert {k: np.asarray(v).tobytes() for k, v in native.items()} == {k: np.asarray(v).tobytes() for k, v in mirror.items()}
    assert native_calls == mirror_calls  # (a hint is not an ABI call: the per-node sequence is what it was)
