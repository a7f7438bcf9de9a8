"""The cuckoo probe (cuckoo_probe.hpp) at chosen hashes: every set of tests/cuckoo_sets.py through the three kernels that share
the probe — hash_lookup_kernel (HashLookup), join_columns_kernel (AresJoinColumnsRun) and the join flavours of select_scan_kernel
(AresFusedFilterJoinSelect, probed before the ranking and after the look-back) — against tests/cuckoo_model.py, bit for bit.

The dimension table of the fused entry points has one Uint32 column whose value at (batch b, index i) is b << 16 | i, so a
joined value names the record the probe returned; what the outputs must be is computed twice, by select_join_model (whose
dictionary is filled from cuckoo_model.probe, Table.forged) and directly from the set's records.

AresSelectJoinStats counts the rows handed to the probe, null keys among them (include/ares_extensions.h: a join is probed "for
the rows the main-table filters left alive" / "for the rows that are written"); AresJoinColumnStats counts valid keys only."""
import numpy as np
import pytest

import cuckoo_sets as S
import harness as H
import select_join_model as J
import select_model as M
import test_fused_select as F
import test_fused_select_join as TS
import test_join_columns as TJ
from aresdb_amd import abi

pytestmark = pytest.mark.gpu
FUSABLE = S.names(fusable=True)
HINT = [("hint", abi.LessThan, 2)]
DIMS = [((0, "rec"), None, None, abi.Uint32), ("row", None, None, abi.Uint32)]
HITS_ONLY = [(0, "rec", abi.GreaterThanOrEqual, 0)]  # b << 16 | i is a positive Int32: true for every hit, false for a null
# what the library refuses: HashLookup with an error, the fused entry points by declining
REFUSED = [dict(keyBytes=0), dict(keyBytes=17), dict(numHashes=-1), dict(numHashes=5), dict(numBuckets=0)]


@pytest.fixture(scope="module")
def hip():
    return H.hip_backend()


class Dev:
    """a fusable set on the device: the forged table, the key column "k0", the row numbers "row" and the pruning column
    "hint" (Uint8, i % 3, every fifth null) — shaped as the batches of test_join_columns and test_fused_select_join"""

    def __init__(self, be, s):
        self.be, self.s, self.n = be, s, s.n
        self.table = J.Table.forged(s.ix, s.widened(), S.PER_BATCH)
        assert J.BASE_BATCH == S.BASE_BATCH
        rows = np.arange(s.n)
        self.cols = {"k0": S.key_col(s), "row": M.Col(abi.Uint32, rows), "hint": M.Col(abi.Uint8, rows % 3, rows % 5 != 0, starting_index=7)}
        self.joins = [("k0", self.table)]
        self.dcols = {k: c.upload(be) for k, c in self.cols.items()}
        self.dtable = self.table.upload(be)
        self.dtables = [self.dtable]
        self.keep = M.model_filter(self.cols["hint"], *HINT[0][1:], s.n)
        rec = s.records()
        self.hit = rec[:, 0] != 0
        self.code = np.where(self.hit, (rec[:, 0] << 16) | rec[:, 1], 0).astype(np.uint32)

    query = TS.Batch.query

    def free(self):
        for c in list(self.dcols.values()) + [self.dtable]:
            c.free()


@pytest.fixture(scope="module")
def dev(hip):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Dev(hip, S.by_name(name))
        return made[name]
    yield get
    for d in made.values():
        d.free()


# ---- HashLookup -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.names())
def test_hash_lookup(hip, dev, name):
    s = S.by_name(name)
    S.assert_lookup(S.hash_lookup(hip, s, table=dev(name).dtable.index if s.fusable else None), s, "HashLookup")


# ---- AresJoinColumnsRun ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FUSABLE)
def test_join_columns(dev, name):
    d = dev(name)
    n = d.n
    for hints, keep in (([], np.ones(n, bool)), (HINT, d.keep)):
        got, _, bufs, probed = TJ.run(d, n, ["rec"], hints)
        for x in bufs:
            x.free()
        [(want_bitmap, want_values)], want_probed = TJ.model(d, n, ["rec"], hints)  # (select_join_model over Table.forged)
        assert want_probed == int((keep & d.s.valid).sum())
        bitmap, values = got[0]
        assert np.array_equal(values.view(np.uint32), np.where(keep, d.code, 0)), "values against the set's records"
        assert np.array_equal(np.unpackbits(bitmap, bitorder="little")[:n].astype(bool), d.hit & keep), "validity against the set's records"
        assert np.array_equal(bitmap, want_bitmap) and np.array_equal(values, want_values)
        assert probed == want_probed


# ---- AresFusedFilterJoinSelect --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hinted", [False, True], ids=["all-rows", "hinted"])
@pytest.mark.parametrize("early", [True, False], ids=["probe-before-ranking", "probe-after-look-back"])
@pytest.mark.parametrize("name", FUSABLE)
def test_fused_select(dev, name, early, hinted):
    """without a main-table filter every row of the set reaches the probe; with one, the rows it kills are not probed"""
    d = dev(name)
    n, be = d.n, d.be
    filters, alive = (HINT, d.keep) if hinted else ([], np.ones(n, bool))
    before = be.select_join_stats()
    res, blob = TS.check(d, filters, HITS_ONLY if early else [], DIMS, n, per_node=False)  # (against select_join_model)
    after = be.select_join_stats()
    rows = np.flatnonzero(alive & d.hit) if early else np.flatnonzero(alive)
    assert res == len(rows)
    assert after["probed"] - before["probed"] == int(alive.sum()) and after["batches"] - before["batches"] == 1
    cap = n + 3  # (check's capacity: two 4-byte value vectors, then two validity vectors)
    joined, row = blob[:4 * res].view(np.uint32), blob[4 * cap:4 * cap + 4 * res].view(np.uint32)
    joined_ok, row_ok = blob[8 * cap:8 * cap + res], blob[9 * cap:9 * cap + res]
    assert np.array_equal(row, rows) and row_ok.all()
    assert np.array_equal(joined, d.code[rows]), "joined values against the set's records"
    assert np.array_equal(joined_ok.astype(bool), d.hit[rows])


# ---- geometry the library refuses -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", REFUSED, ids=[f"{k}={v}" for g in REFUSED for k, v in g.items()])
def test_refused_geometry(hip, dev, geometry):
    d = dev("honest-4")
    s, n = d.s, d.n
    # HashLookup: the error, and not a byte of the output
    idx, out = H.Buf(hip, np.arange(n, dtype=np.uint32)), H.Buf(hip, np.full(2 * n, S.FILL, np.uint32))
    try:
        with pytest.raises(abi.AresError, match="Unsupported cuckoo hash index geometry"):
            hip.call("HashLookup", d.dcols["k0"].input(), out.ptr, idx.ptr, n, None, 0, S.index_struct(s, d.dtable.index.ptr, **geometry), None, 0)
        hip.wait()
        assert (out.read(np.uint32) == S.FILL).all()
    finally:
        idx.free()
        out.free()
    # AresJoinColumnsRun: declined, nothing launched, nothing written
    size = hip.join_column_bytes(n, abi.Uint32) + 64
    buf = H.Buf(hip, np.full(size, M.SENTINEL, np.uint8))
    try:
        q = TJ.query(d, ["rec"], [TJ.aligned(buf)])
        for k, v in geometry.items():
            setattr(q.join.index, k, v)
        TJ._declined(hip, q, n)
        assert (buf.read(np.uint8) == M.SENTINEL).all()
    finally:
        buf.free()
    # AresFusedFilterJoinSelect, both flavours
    for ffilters in (HITS_ONLY, []):
        q = d.query(HINT, ffilters, DIMS)
        for k, v in geometry.items():
            setattr(q.joins[0].index, k, v)
        vec = H.DimVector(hip, n, M.ndw_of(DIMS), with_hash=False, with_index=False, init=np.full(10 * n, M.SENTINEL, np.uint8))
        hip.wait()
        hip.profiler_enable(True)
        try:
            with pytest.raises(abi.AresError, match="^not fusable"):
                hip.fused_filter_join_select(q, n, -1, vec.struct())
            hip.wait()
            assert hip.profiler_report() == {}, "a declined shape launched a kernel"
            F._sentinel_intact(vec, vec.values.read(np.uint8), 0)
        finally:
            hip.profiler_enable(False)
            vec.free()
