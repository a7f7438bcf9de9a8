"""The cuckoo model (tests/cuckoo_model.py) pinned on the CPU: against the C oracle and the reference's own host build on every
set of tests/cuckoo_sets.py, against the tables of cases.build_cuckoo that the older tests use, and — the point of the sets —
every wrong probe of cuckoo_model.MUTANTS disagrees with the model on a row of the family built against it."""
import numpy as np
import pytest

import cases
import cuckoo_model as cm
import cuckoo_sets as S
import harness as H

NAMES = S.names()
needs_ref = pytest.mark.skipif(not H.have_ref(), reason="oracle/_ref not built")

# which family must kill which wrong probe
KILLED_BY = {
    "no clamp": "clamp",
    "slots 7..0": "order",
    "hashes last to first": "order",
    "stash before buckets": "order",
    "stash ignores the signature": "stale",
    "bucket slots match signature 0": "stale",
    "key compared without its odd tail": "decoys",
    "key compared on 4 bytes": "decoys",
    "key not truncated": "widths",
    "quotient without correction": "buckets",
    "numHashes taken as 4": "hash count",
}


def test_murmur_known_answers():
    """published murmur3_x86_32 vectors"""
    for key, seed, want in [(b"", 0, 0), (b"", 1, 0x514E28B7), (b"", 0xFFFFFFFF, 0x81F16F39), (b"\xff\xff\xff\xff", 0, 0x76293B50),
                            (b"\x21\x43\x65\x87", 0, 0xF55B516B), (b"\x21\x43\x65\x87", 0x5082EDEE, 0x2362F9DE),
                            (b"\x21\x43\x65", 0, 0x7E4A8634), (b"\x21\x43", 0, 0xA0F7B07A), (b"\x21", 0, 0x72661CF4),
                            (b"\0\0\0\0", 0, 0x2362F9DE), (b"\0\0\0", 0, 0x85F0B427), (b"\0\0", 0, 0x30F4C306), (b"\0", 0, 0x514E28B7)]:
        assert cm.murmur3_32(key, seed) == want, (key, seed)


@pytest.mark.parametrize("width", [4, 8, 16])
def test_key_with_hash_round_trips(width):
    rng = np.random.default_rng(width)
    targets = [0, 1, 0x00FFFFFF, 0x01000000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF] + [int(x) for x in rng.integers(0, 1 << 32, 200)]
    for i, t in enumerate(targets):
        seed = [0, 0xFFFFFFFF, S.SEEDS[i % 4], int(rng.integers(0, 1 << 32))][i % 4]
        rest = bytes(rng.integers(0, 256, width - 4, dtype=np.uint8))
        key = cm.key_with_hash(t, seed, width, rest)
        assert len(key) == width and key[4:] == rest and cm.murmur3_32(key, seed) == t


@pytest.mark.parametrize("width", [1, 2, 3, 4, 5, 8, 13, 16])
def test_seed_with_hash_round_trips(width):
    rng = np.random.default_rng(100 + width)
    keys = [bytes(width), b"\xff" * width] + [bytes(rng.integers(0, 256, width, dtype=np.uint8)) for _ in range(100)]
    for i, key in enumerate(keys):
        t = [0, 0x00ABCDEF, 0xFFFFFFFF, int(rng.integers(0, 1 << 32))][i % 4]
        seed = cm.seed_with_hash(t, key)
        assert 0 <= seed <= 0xFFFFFFFF and cm.murmur3_32(key, seed) == t


def test_find_key_finds_or_raises():
    assert cm.find_key(lambda k: k[0] == 200, 1) == bytes([200])
    assert cm.find_key(lambda k: True, 2, start=0xFFFF, exclude={b"\xff\xff"}) == b"\0\0"
    with pytest.raises(LookupError):
        cm.find_key(lambda k: False, 1)
    with pytest.raises(LookupError):
        cm.find_key(lambda k: False, 8, limit=1000)


def test_every_family_has_a_width_and_every_set_its_limits():
    families = {s.family for s in S.all_sets()}
    assert families == {"clamp", "stale", "decoys", "order", "hash count", "buckets", "widths", "rows", "honest"}
    for s in S.all_sets():
        assert s.ix.table.nbytes <= 8 << 20 and s.n <= 5000
    assert {s.ix.key_bytes for s in S.all_sets() if s.family == "honest"} == {1, 2, 4, 8, 16}
    assert {s.ix.num_buckets for s in S.all_sets() if s.family == "buckets"} == set(S.DIVISORS)
    assert {s.ix.num_hashes for s in S.all_sets() if s.family == "hash count"} == {0, 1, 2, 3, 4}
    assert {s.n for s in S.all_sets() if s.family == "rows"} >= {1, 63, 64, 65, 257}


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_oracle(name):
    s = S.by_name(name)
    S.assert_lookup(S.hash_lookup(H.oracle_backend(), s), s, "oracle")


@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_reference_build(name):
    s = S.by_name(name)
    S.assert_lookup(S.hash_lookup(H.ref_backend(), s), s, "reference build")


@pytest.mark.parametrize("seed", range(12))
def test_model_on_the_tables_of_the_older_tests(seed):
    """cases.build_cuckoo's table bytes, probed by the model: every placed key at its record, and the oracle's answer for the
    case's own probe rows"""
    c = cases.HashLookupCase(seed)
    ix = cm.Index(c.key_bytes, c.num_buckets, 4, c.seeds)
    assert ix.table.nbytes == c.table.nbytes
    ix.table[:] = c.table
    for key, rec in c.placed.items():
        assert cm.probe(ix, key) == tuple(rec)
    got = c.run(H.oracle_backend())["rids"].reshape(-1, 2)
    for i, row in enumerate(c.index):
        key = int(c.probe[row]).to_bytes(c.key_bytes, "little")
        want = cm.probe(ix, key) if c.valid[row] else (0, 0)
        assert tuple(int(x) for x in got[i]) == want, (seed, i)


@pytest.mark.parametrize("mutant", sorted(cm.MUTANTS))
def test_the_sets_bite(mutant):
    """a condition on the inputs: the family built against a wrong probe has a row on which it differs from the model"""
    family = KILLED_BY[mutant]
    killers = [s.name for s in S.all_sets() if s.family == family and not np.array_equal(s.expected(cm.MUTANTS[mutant]), s.expected())]
    assert killers, f"no set of family {family!r} tells the model from the probe with {mutant!r}"


def test_every_mutant_is_listed():
    assert set(KILLED_BY) == set(cm.MUTANTS) and len(cm.MUTANTS) == 11


# sets that must each tell the model from a wrong probe on their own: the property they assert when built is the one that bites
EACH_BITES = {
    "no clamp": [f"clamp-{w}" for w in S.WIDTHS] + [f"zero-{w}-present" for w in S.WIDTHS],
    "slots 7..0": [f"order-{w}" for w in S.WIDTHS],
    "hashes last to first": [f"order-{w}" for w in S.WIDTHS],
    "stash before buckets": [f"order-{w}" for w in S.WIDTHS],
    "stash ignores the signature": [f"stale-{w}" for w in S.WIDTHS],
    "bucket slots match signature 0": [f"stale-{w}" for w in S.WIDTHS],
    "key compared without its odd tail": ["byte-1", "byte-2", "byte-3", "byte-5", "byte-13"],
    "key compared on 4 bytes": ["byte-5", "byte-8", "byte-13", "byte-16"],
    "key not truncated": ["prefix-1-of-4", "prefix-2-of-4", "prefix-3-of-4", "prefix-5-of-8", "prefix-13-of-16"],
    "quotient without correction": ["buckets-4-3", "buckets-4-641", "buckets-4-65535", "buckets-4-65537", "buckets-8-641", "buckets-16-641",
                                    "buckets-1-641-a", "buckets-2-641-c"],
    "numHashes taken as 4": [f"hashes-{w}-{nh}" for w in S.WIDTHS for nh in range(4)],
}


@pytest.mark.parametrize("mutant", sorted(EACH_BITES))
def test_each_targeted_set_bites(mutant):
    for name in EACH_BITES[mutant]:
        s = S.by_name(name)
        assert s.family == KILLED_BY[mutant]
        assert not np.array_equal(s.expected(cm.MUTANTS[mutant]), s.expected()), (mutant, name)
