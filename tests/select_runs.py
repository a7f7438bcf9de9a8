"""Run-length (mode 3) columns for the select tests: a column given as (run values, run validity, run lengths) becomes a
`RunCol` — the run arrays with their cumulative counts, uploaded as they are — and its row-space twin (np.repeat), which is
what the numpy model of tests/select_model.py evaluates.  Row r of the batch lies in the run whose [counts[k], counts[k + 1])
holds it; validity is bit k + StartingIndex of the run bitmap; the value is values[k]."""
import numpy as np

import harness as H
import select_model as M
from aresdb_amd import abi


class RunCol(M.Col):
    """select_model.Col with counts; uploads GeoPoint / UUID run arrays with their counts too (Col.upload drops them)"""

    def upload(self, be):
        if self.counts is not None and self.dtype in (abi.GeoPoint, abi.UUID):
            return H.Column(be, self.dtype, raw_values=self.values.tobytes(), valid=self.valid, counts=self.counts,
                            starting_index=self.starting_index)
        return super().upload(be)


def run_col(dtype, run_values, run_valid, run_lengths, starting_index=0):
    """(the mode-3 column for upload, its row-space twin for model_select)"""
    lens = np.asarray(run_lengths, np.int64)
    assert (lens >= 1).all() and len(lens) == len(run_valid)
    valid = np.asarray(run_valid, bool)
    counts = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    up = RunCol(dtype, run_values, valid, starting_index, counts=counts)
    assert len(up.values) == len(lens)
    twin = M.Col(dtype, np.repeat(up.values, lens, axis=0), np.repeat(valid, lens), starting_index)
    return up, twin


def run_lengths(rng, n, longest):
    """run lengths in [1, longest] that sum to exactly n, short and long ones mixed"""
    lens = []
    left = n
    while left > 0:
        k = int(min(left, rng.integers(1, longest + 1) if rng.random() < 0.5 else rng.integers(1, 4)))
        lens.append(k)
        left -= k
    return np.asarray(lens, np.int64)


def values_of(rng, dtype, k):
    """k run values of the type, small ranges for the narrow ones (filters select a share of them)"""
    if dtype == abi.UUID:
        return rng.integers(0, 256, (k, 16), dtype=np.uint8)
    if dtype == abi.GeoPoint:
        return rng.integers(0, 256, (k, 8), dtype=np.uint8)
    if dtype == abi.Int64:
        return rng.integers(-2 ** 60, 2 ** 60, k)
    if dtype == abi.Float32:
        return (rng.random(k) * 100).astype(np.float32)
    lo, hi = {abi.Int8: (-100, 100), abi.Uint8: (0, 6), abi.Int16: (-300, 300), abi.Uint16: (0, 500), abi.Int32: (-10 ** 6, 10 ** 6),
              abi.Uint32: (1000, 2000)}[dtype]
    return rng.integers(lo, hi, k)


def random_run_col(rng, dtype, n, longest, starting_index=0, valid_share=0.85):
    lens = run_lengths(rng, n, longest)
    return run_col(dtype, values_of(rng, dtype, len(lens)), rng.random(len(lens)) < valid_share, lens, starting_index)


def split(pairs):
    """{name: (upload, twin) or a plain Col} -> ({name: column to upload}, {name: column the model reads})"""
    up = {k: (v[0] if isinstance(v, tuple) else v) for k, v in pairs.items()}
    twin = {k: (v[1] if isinstance(v, tuple) else v) for k, v in pairs.items()}
    return up, twin
