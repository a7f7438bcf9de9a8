"""CPU checks of the chosen-hash machinery (tests/hash_model.py, tests/hash_sets.py): the murmur3 inverse against the
project's two murmur helpers, and the exact model against the C oracle (and the reference's own host build where it has
been built) on every chosen-hash input the GPU tests run."""
import itertools

import numpy as np
import pytest

import harness as H
import hash_model as M
import hash_paths as P
import hash_sets as S
from aresdb_amd import check

LAYOUTS = [(4,), (4, 4), (4, 4, 4), (4, 4, 4, 4), (4, 2), (4, 1), (4, 4, 2), (4, 2, 1), (4, 4, 2, 1), (4, 2, 2, 1, 1)]


def _targets(rng, n):
    edge = [0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0x40000000, 0x80000000, 0xC0000000, 0x3FFFFFFF, 0x7FFFFFFF]
    return edge + [int(x) for x in rng.integers(0, 1 << 32, n - len(edge), dtype=np.uint64)]


@pytest.mark.parametrize("widths", LAYOUTS, ids=lambda w: "x".join(map(str, w)))
def test_inverse_reproduces_the_project_murmur(widths):
    """row_with_hash names a hash and gets the row: checked against check.murmur3_32_bytes on the packed rows of every
    layout, and against check.murmur3_32_rows for the all-4-byte ones, for every validity pattern."""
    nd = len(widths)
    rng = np.random.default_rng(1000 + sum(widths) * 7 + nd)
    rows, valids, targets = [], [], []
    for pattern in itertools.product((0, 1), repeat=nd):
        for t in _targets(rng, 40):
            others = tuple(int(rng.integers(0, 1 << (8 * w), dtype=np.uint64)) if ok else 0 for w, ok in zip(widths[1:], pattern[1:]))
            x = M.row_with_hash(t, others, pattern, list(widths))
            assert 0 <= x < 1 << 32
            rows.append((x,) + others)
            valids.append(pattern)
            targets.append(t)
    packed = np.frombuffer(b"".join(M.pack_row(r, o, list(widths)) for r, o in zip(rows, valids)), np.uint8).reshape(len(rows), -1)
    assert np.array_equal(check.murmur3_32_bytes(packed), np.array(targets, np.uint32))
    assert [M.row_hash(r, o, list(widths)) for r, o in zip(rows, valids)] == targets
    if all(w == 4 for w in widths) and nd <= 4:
        cols = [np.array([r[d] for r in rows], np.uint32) for d in range(nd)]
        oks = [np.array([o[d] for o in valids], np.uint8) for d in range(nd)]
        assert np.array_equal(check.murmur3_32_rows(cols, oks), np.array(targets, np.uint32))


def test_model_aggregates_from_the_identity_and_keeps_the_lowest_row():
    rows = [(5, 1), (6, 1), (5, 1), (9, 0)]
    valids = [(1, 1), (1, 1), (1, 1), (1, 0)]
    got, rep = M.groups_by_hash(rows, valids, [3, -7, 4, 1], ("min", "i32"))
    assert got == {((5, 1), (1, 1)): 3, ((6, 1), (1, 1)): -7, ((9, 0), (1, 0)): 1}
    assert sorted(rep.values()) == [0, 1, 3]
    got, _ = M.groups_by_hash(rows, valids, [0xFFFFFFFF, 1, 2, 3], ("sum", "u32"))
    assert got[((5, 1), (1, 1))] == 1  # wraps like the measure type
    got, _ = M.groups_by_hash(rows, valids, [0.125, 1, 2.5, 3], ("sum", "f32"))
    assert got[((5, 1), (1, 1))] == 2.625
    with pytest.raises(AssertionError):
        M.groups_by_hash(rows, valids, [2.0 ** 24, 1, 1, 3], ("sum", "f32"))  # 2^24 + 1 is no float32: the case is refused
    # two different rows with one hash are one group under the lower row's dimensions
    a = (M.row_with_hash(0xFFFFFFFF, (1,), (1, 1)), 1)
    b = (M.row_with_hash(0xFFFFFFFF, (2,), (1, 1)), 2)
    got, _ = M.groups_by_hash([b, a, b], [(1, 1)] * 3, [1, 10, 100], ("sum", "i64"))
    assert a != b and got == {(b, (1, 1)): 111}


# aggregates the oracle (and the reference's host build) can be compared on: its map starts a new group from 0, not from the
# aggregate's identity, which only sums and maxima over values >= 0 do not notice
_ON_HOST_MAP = ["sum_u32", "sum_i32", "sum_i64", "sum_f32", "sum_f64", "max_u32"]


def _run_and_compare(be, prog, agg_name):
    got = P.run_plain(be, prog, agg_name)
    for b, res in enumerate(got):
        P.assert_result(prog, agg_name, b, res["groups"], res["map"])


@pytest.mark.parametrize("name", sorted(S.all_programs()))
def test_model_equals_the_oracle(name):
    prog = S.all_programs()[name]()
    k = sorted(S.all_programs()).index(name)
    for agg_name in (_ON_HOST_MAP[k % len(_ON_HOST_MAP)], _ON_HOST_MAP[(k + 3) % len(_ON_HOST_MAP)]):
        _run_and_compare(H.oracle_backend(), prog, agg_name)


@pytest.mark.parametrize("name", sorted(S.all_programs()))
def test_model_equals_the_reference_host_build(name):
    if not H.have_ref():
        pytest.skip("oracle/_ref has not been built")
    prog = S.all_programs()[name]()
    _run_and_compare(H.ref_backend(), prog, ["sum_i64", "max_u32", "sum_u32"][sorted(S.all_programs()).index(name) % 3])


@pytest.mark.parametrize("name,agg_name", [("collisions", "sum_i64"), ("sentinels_prev", "sum_u32"), ("collisions_4x2", "sum_f64"),
                                           ("sentinels_4x2", "max_u32"), ("chains", "sum_i32")])
def test_model_equals_the_oracle_through_the_batch_executor(name, agg_name):
    """The same inputs as source columns of a query (dimension = bare column, a null dimension = a null column entry): the
    per-node sequence on the oracle ends with the model's groups."""
    prog = S.all_programs()[name]()
    groups, table, _ = P.run_query(H.oracle_backend(), prog, agg_name, "mirror")
    P.assert_result(prog, agg_name, len(prog.batches) - 1, groups, table)
