"""Searches inputs whose GetHLLValue has a given rho, with the model of tests/edge_model.py alone, and writes them to
hll_preimages.json.

The original's bit walk leaves the bits it can probe after rho = 17 (edge_model.hll_from_hash: rho jumps to 50 there), which a
random input reaches with probability 2^-18: no seeded test ever does.  An implementation whose shift count wraps mod 32
would go on probing the register bits instead (rho = 18, 19, ...); inputs are therefore filed under the rho of THAT reading
(wrapped_rho below), which splits the model's rho = 50 class by the register's low bits, and every rho 0 ... 20 of it must be
present so that the two readings differ on several of the committed inputs.  The scan covers the Uint32 inputs 0 ... 2^26 - 1 (hashed as 4
bytes) and as many Int64 inputs that differ in their high words (hashed as 8 bytes; every other one negative).  Needs nothing but
numpy; the JSON is committed so that no test repeats the scan.

    python tests/golden/make_hll_preimages.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import edge_model as M  # noqa: E402

SCAN_BITS = 26
CHUNK = 1 << 22
PER_RHO, DEEP_FROM, DEEP_CAP = 4, 18, 64


def int64_input(i):
    """high word i + 1, low word i, the sign bit set for odd i (as uint64 bits)"""
    i = np.asarray(i, np.uint64)
    return ((i + np.uint64(1)) << np.uint64(32)) | i | ((i & np.uint64(1)) << np.uint64(63))


def wrapped_rho(h):
    """rho if the 32-bit shift count wrapped mod 32: trailing zeros of the low word rotated right by 14, 50 for a zero word;
    equal to the model's rho up to 17"""
    low = (np.asarray(h, np.uint64) & np.uint64(M.M32)).astype(np.int64)
    rot = ((low >> 14) | (low << 18)) & M.M32
    return np.where(rot == 0, 50, np.log2(np.maximum(rot & -rot, 1).astype(np.float64)).astype(np.int64))


def scan(width):
    by_rho, deep = {}, []
    for start in range(0, 1 << SCAN_BITS, CHUNK):
        i = np.arange(start, start + CHUNK, dtype=np.uint64)
        x = i if width == 4 else int64_input(i)
        h = M.murmur3_x64_128_low(x, width)
        rho = wrapped_rho(h)
        assert np.array_equal(np.where(rho >= DEEP_FROM, 50, rho), M.hll_from_hash(h) >> 16)
        for r in np.unique(rho):
            have = by_rho.setdefault(int(r), [])
            if len(have) < PER_RHO:
                have += [int(v) for v in x[rho == r][:PER_RHO - len(have)]]
        deep += [int(v) for v in x[rho >= DEEP_FROM]]
    return by_rho, sorted(deep)[:DEEP_CAP], len(deep)


def main():
    out = {"source": "tests/golden/make_hll_preimages.py: inputs by the rho their GetHLLValue would have if the original's "
                     "shift count wrapped mod 32 (up to 17 that is the rho of edge_model.hll_from_hash, from 18 on the model says 50); "
                     "int64 inputs as signed values", "scan_bits": SCAN_BITS}
    for name, width in (("uint32", 4), ("int64", 8)):
        by_rho, deep, found = scan(width)
        missing = [r for r in range(21) if r not in by_rho]
        assert not missing, f"{name}: no input with rho {missing}"
        assert found >= 4, f"{name}: {found} inputs with rho >= {DEEP_FROM}"
        signed = (lambda v: v - (1 << 64) if v >> 63 else v) if width == 8 else (lambda v: v)
        out[name] = {"by_rho": {str(r): [signed(v) for v in by_rho[r]] for r in sorted(by_rho)}, "deep": [signed(v) for v in deep],
                     "deep_found": found}
        print(name, "rho reached:", sorted(by_rho), "inputs with rho >=", DEEP_FROM, ":", found)
    with open(os.path.join(HERE, "hll_preimages.json"), "w") as f:
        json.dump(out, f)
    print("wrote hll_preimages.json")


if __name__ == "__main__":
    main()
