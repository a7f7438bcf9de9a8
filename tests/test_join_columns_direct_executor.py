"""Aggregation queries over tables joined on 1- and 2-byte keys through the C++ driver with AresQuerySetJoinColumns, the direct
flavour of AresJoinColumnsRun forced (ARES_JOIN_COLUMNS=direct): every stored key value is probed once per batch and table, the
rows stream through the table that leaves.  Results must equal the setter-off run — key -> value for HashReduce, rows in order
for Sort + Reduce — and the numpy group-by over the join model; the ABI calls are those of the probe flavour.

The batches of tests/test_local_time_executor.py: four of 3 000 - 5 000 rows, the second with base counts (it takes the original
plan).  Table 0 is joined on a Uint8 key, table 1 on a Uint16 key.  On the oracle (CPU) the library has no such entry point: the
setter and the switch change nothing."""
import numpy as np
import pytest

import narrow_join_model as N
import select_model as M
import test_fused_select as F
import test_join_columns_executor as XE
import test_nonaggr_join_executor as X
from aresdb_amd import abi

KEYS = [(abi.Uint8, 11), (abi.Uint16, 23)]
FFILTERS = XE.FFILTERS[2]  # region of table 0 < 150, rate of table 1 < 40.0
SHAPES = ["sum_hash", "count_sort"]  # SUM through HashReduce, COUNT(*) through Sort + Reduce; both read both tables


class Tables(X.Tables):
    """the dimension tables of a query over narrow keys (the mode-0 batch without a default: the hosts pass none)"""

    def __init__(self, be):
        self.be = be
        self.tables = [N.make_table(dtype, default=False, seed=seed) for dtype, seed in KEYS]
        self.device = [t.upload(be) for t in self.tables]

    def batch(self, n, seed, base_counts=None):
        cols = M.mixed_columns(max(n, 1), seed=seed)
        for k, t in enumerate(self.tables):
            cols["k%d" % k] = N.key_column(t, max(n, 1), seed + 100 * k)
        return X.E.B(n, seed, base_counts=base_counts, cols=cols)


def flavour_stats(be):
    return be.join_column_flavour_stats() if be.name == "hip" else None


@pytest.mark.parametrize("name", SHAPES)
def test_results_equal_the_setter_off_run_and_numpy(be, name):
    tables = Tables(be)
    try:
        batches = XE.batches_of(tables)
        shape = XE.shapes(2)[name]
        plan = XE.build(tables, shape, FFILTERS)
        want = XE.expected(tables, batches, shape, FFILTERS)
        assert len(want) > 3, name
        off, calls_off, _ = XE.run(be, plan, batches, False)
        XE.assert_groups(XE.groups(plan, off), want, shape[2])
        runs = {}
        for flavour in ("probe", "direct"):
            with F._Env(be, ARES_JOIN_COLUMNS=flavour):
                before = flavour_stats(be)
                on, calls_on, _ = XE.run(be, plan, batches, True)
                be.wait()
                after = flavour_stats(be)
            XE.assert_groups(XE.groups(plan, on), want, shape[2])
            if not shape[4]:
                XE.assert_rows(on, off, shape[2])
            runs[flavour] = calls_on
            if before is not None:  # three eligible batches, two tables read
                delta = {k: after[k] - before[k] for k in after}
                if flavour == "direct":
                    assert delta == {"probe": 0, "direct": 3 * 2, "entries": 3 * (256 + 65536)}, name
                else:
                    assert delta == {"probe": 3 * 2, "direct": 0, "entries": 0}, name
        assert runs["direct"] == runs["probe"], name
        if be.name != "hip":
            assert runs["direct"] == calls_off, name
    finally:
        tables.free()


@pytest.mark.gpu
def test_kernels_of_the_eligible_batches_under_direct():
    """one table kernel and one rows kernel per eligible batch and table; no per-row probe of either kind"""
    import harness as H
    hip = H.hip_backend()
    tables = Tables(hip)
    try:
        batches = [b for b in XE.batches_of(tables, seed=7) if b.base_counts is None]
        plan = XE.build(tables, XE.shapes(2)["count_sort"], FFILTERS)
        with F._Env(hip, ARES_JOIN_COLUMNS="direct"):
            XE.run(hip, plan, batches, True)  # priming pass: the shape's generated kernels are compiled
            hip.rtc_wait()
            on = XE._profile(hip, lambda: XE.run(hip, plan, batches, True))
        assert XE._launches(on, "join_columns_table_kernel") == XE._launches(on, "join_columns_rows_kernel") == 2 * len(batches), sorted(on)
        assert XE._launches(on, "join_columns_kernel") == 0 and XE._launches(on, "hash_lookup_kernel") == 0, sorted(on)
    finally:
        tables.free()
