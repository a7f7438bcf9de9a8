"""CPU checks of the chosen-hash machinery of Sort + Reduce (tests/sort_model.py, tests/sort_sets.py): the murmur3_x64_128
inverse against the project's murmur helper and the model's own forward hash, and the exact model against the C oracle and the
reference's own host build on every chosen-hash input the GPU tests run — true 64-bit collisions included, where the
reference's reduce_by_key compares hashes only."""
import itertools

import numpy as np
import pytest

import harness as H
import sort_model as M
import sort_paths as P
import sort_sets as S
from aresdb_amd import check

EDGE = [0, 1, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 2, (1 << 64) - 1, 0xFFFFFFFF00001234, 0x00001234FFFFFFFF]


@pytest.mark.parametrize("widths", M.LAYOUTS, ids=lambda w: "x".join(map(str, w)))
def test_inverse_reproduces_the_project_murmur(widths):
    """row_with_hash64 names a hash and gets the row, for every validity tail of the three layouts: checked against the model's
    forward hash (scalar and vectorised) and against check.murmur3_128_lo64_rows; the vectorised inverse gives the same rows."""
    nd = len(widths)
    rng = np.random.default_rng(64 + nd)
    for pattern in itertools.product((0, 1), repeat=nd):
        targets = EDGE + [int(x) for x in rng.integers(0, 1 << 64, 60, dtype=np.uint64)]
        frees = [int(x) for x in rng.integers(0, 1 << 64, len(targets), dtype=np.uint64)]
        frees[:3] = [0, 1, (1 << 64) - 1]
        packed = []
        for t, g in zip(targets, frees):
            values = M.row_with_hash64(t, g, pattern, widths)
            assert all(0 <= v < 1 << (8 * w) for v, w in zip(values, widths))
            row = M.pack_row(values, pattern, widths)
            assert len(row) == 16 + nd and M.murmur3_128_lo64(row) == t
            packed.append(np.frombuffer(row, np.uint8))
        packed = np.stack(packed)
        want = np.array(targets, np.uint64)
        assert np.array_equal(M.hash_rows(packed), want)
        assert np.array_equal(check.murmur3_128_lo64_rows(packed), want)
        assert np.array_equal(M.rows_with_hash64(want, np.array(frees, np.uint64), pattern, widths), packed)


def test_forward_hash_of_other_lengths():
    """the model's two forward hashes agree with each other and with the project's helper on rows of 0 .. 40 bytes (tails of
    every length, two blocks)"""
    rng = np.random.default_rng(3)
    assert M.murmur3_128_lo64(b"") == 0
    for nbytes in range(1, 41):
        rows = rng.integers(0, 256, (7, nbytes), dtype=np.uint8)
        want = np.array([M.murmur3_128_lo64(bytes(r)) for r in rows], np.uint64)
        assert np.array_equal(M.hash_rows(rows), want) and np.array_equal(check.murmur3_128_lo64_rows(rows), want)


def test_two_free_words_give_two_rows_with_one_hash():
    for t in EDGE:
        a = M.row_with_hash64(t, 1, (1, 1, 1, 1), (4, 4, 4, 4))
        b = M.row_with_hash64(t, 2, (1, 1, 1, 1), (4, 4, 4, 4))
        assert a != b and M.murmur3_128_lo64(M.pack_row(a, (1,) * 4, (4,) * 4)) == M.murmur3_128_lo64(M.pack_row(b, (1,) * 4, (4,) * 4)) == t


def test_model_orders_by_hash_keeps_the_lowest_row_and_folds_from_the_identity():
    hs = np.array([9, 5, 9, 1 << 63, 5, (1 << 64) - 1], np.uint64)
    frees = np.array([1, 2, 3, 4, 5, 6], np.uint64)   # rows 0 and 2 (hash 9), 1 and 4 (hash 5) are DIFFERENT rows with one hash
    rows = M.rows_with_hash64(hs, frees, (1,) * 4, (4,) * 4)
    assert len({bytes(r) for r in rows}) == 6
    r = M.groups_by_hash64(None, rows, [3, -7, 4, 1, -9, 8], ("min", "i32"))
    assert r.hashes.tolist() == [5, 9, 1 << 63, (1 << 64) - 1] and r.out_index.tolist() == [1, 0, 3, 5] and r.values == [-9, 3, 1, 8]
    assert r.sorted_index.tolist() == [1, 4, 0, 2, 3, 5] and np.array_equal(r.rows, rows[[1, 0, 3, 5]])
    assert M.groups_by_hash64(None, rows, [0xFFFFFFFF, 1, 2, 3, 4, 5], ("sum", "u32")).values[1] == 1   # wraps like the measure type
    assert M.groups_by_hash64(None, rows, [0.125, 1, 2.5, 3, 0, 0], ("sum", "f32")).values[1] == 2.625
    # a previous result in front: its row represents the group, its value is a partial
    r2 = M.groups_by_hash64(r.rows[:2], rows, [100, 200, 1, 1, 1, 1, 1, 1], ("sum", "u64"))
    assert r2.out_index.tolist() == [0, 1, 5, 7] and r2.values == [102, 202, 1, 1]
    r3 = M.groups_by_hash64(None, rows, [(0.0, 2), (0.0, 1), (0.0, 3), (2.5, 1), (0.0, 1), (7.0, 1)], ("avg", "f32"))
    assert r3.values == [(0.0, 2), (0.0, 5), (2.5, 1), (7.0, 1)]
    with pytest.raises(AssertionError):
        M.groups_by_hash64(None, rows, [2.0 ** 24, 1, 1, 3, 0, 0], ("sum", "f32"))   # could round: refused, not approximated
    with pytest.raises(AssertionError):
        M.groups_by_hash64(None, rows, [(1.0, 2), (1.5, 1), (2.0, 3), (2.0, 1), (0.0, 1), (7.0, 1)], ("avg", "f32"))


def test_fixup_census_counts_segments_by_their_first_descent():
    H64 = S.H64
    hs = [H64(5, 9), H64(5, 3), H64(5, 1), H64(7, 1), H64(7, 2), H64(9, 4), H64(9, 4), H64(3, 8), H64(3, 7)]
    c = M.fixup_census(np.array(hs, np.uint64), 64, 4096, block=4)
    assert c.short == [(0, 2), (2, 5)] and not c.long and c.descents == 3 and c.per_block == {0: 2}
    c = M.fixup_census(np.array(hs, np.uint64), 2, 3)
    assert c.short == [(0, 2)] and c.long == [(2, 5)]


def _aggs_for(name, prog):
    """one integer aggregate per input; the collision and cluster inputs take every aggregate"""
    names = sorted(S.all_programs())
    if name.startswith(("collisions64", "clusters")):
        return [a for a in S.ALL_AGGS if prog.float_ok() or a in S.INT_AGGS]
    return [S.INT_AGGS[names.index(name) % len(S.INT_AGGS)]]


def _run_and_compare(be, prog, agg_name):
    got = P.run_vectors(be, prog, agg_name)
    exp = prog.expected(agg_name)
    assert len(got) == len(exp)
    for b, (g, e) in enumerate(zip(got, exp)):
        P.assert_batch(prog, agg_name, b, g, e, be.name)


@pytest.mark.parametrize("name", sorted(S.all_programs()))
def test_model_equals_the_oracle(name):
    """group count, output rows in order, values, the sorted hash / index vectors and the output index vector, bit for bit"""
    prog = S.all_programs()[name]()
    for agg_name in _aggs_for(name, prog):
        _run_and_compare(H.oracle_backend(), prog, agg_name)


@pytest.mark.parametrize("name", sorted(S.all_programs()))
def test_model_equals_the_reference_host_build(name):
    if not H.have_ref():
        pytest.skip("oracle/_ref has not been built")
    prog = S.all_programs()[name]()
    for agg_name in _aggs_for(name, prog)[:3]:
        _run_and_compare(H.ref_backend(), prog, agg_name)


@pytest.mark.parametrize("name,agg_name", [("collisions64", "sum_u64"), ("sentinels64_prev", "sum_u32"), ("three_batches", "min_i32"),
                                           ("sentinels64_uuid", "max_u32"), ("collisions64_b3", "avg"), ("clusters_narrow4_p2_shuffled", "sum_f32")])
def test_model_equals_the_oracle_through_transforms(name, agg_name):
    """The same inputs as source columns of the per-batch sequence (dimension = bare column through a Noop transform): the
    transforms do carry the bytes the model hashed."""
    prog = S.all_programs()[name]()
    got = P.run_columns(H.oracle_backend(), prog, agg_name, read=("sorted", "after"))
    for b, (g, e) in enumerate(zip(got, prog.expected(agg_name, True))):
        P.assert_batch(prog, agg_name, b, g, e, "oracle/columns")


@pytest.mark.parametrize("name,agg_name", [("collisions64_b3", "sum_u64"), ("sentinels64_prev", "min_i32")])
def test_model_equals_the_oracle_through_the_batch_executor(name, agg_name):
    prog = S.all_programs()[name]()
    exp = prog.expected(agg_name, True)
    P.assert_batch(prog, agg_name, len(exp) - 1, P.run_query(H.oracle_backend(), prog, agg_name, "mirror"), exp[-1], "oracle/mirror")
