"""The numpy model of constant chains (tests/chain_model.py) pinned to the oracle over the edges of local time: the five
expression shapes the AQL compiler builds for fixed-zone and recurring time dimensions (aresdb_amd.queries.time_dimension), at
the timestamps where a day, a week, the sign of local time and the 32-bit range turn, for every offset sign, with the inner
nodes stored as Uint32 and as Int32.  Signed and unsigned Floor differ once local time is negative: the oracle decides."""
import numpy as np
import pytest

import chain_model as M
import harness as H
from aresdb_amd import abi, queries, smoke
from aresdb_amd.executor import Binary, Col, Const, DimensionSpec, QueryPlan


def edge_batch():
    ts = np.concatenate([M.EDGE_TS, M.EDGE_TS[:4]])  # (the last four rows are nulls)
    valid = np.ones(len(ts), bool)
    valid[len(M.EDGE_TS):] = False
    return {"request_at": (abi.Uint32, ts)}, {"request_at": valid}


def per_row_plan(expr):
    """COUNT(*) grouped by (the bare column, the chain): one group per distinct (timestamp, validity)"""
    return QueryPlan(filters=[], dimensions=[DimensionSpec(Col("request_at"), abi.Uint32), DimensionSpec(expr, abi.Uint32)],
                     measure=Const(1), agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32, use_hash_reduction=False)


@pytest.mark.parametrize("inner", [abi.Uint32, abi.Int32], ids=["inner_uint32", "inner_int32"])
@pytest.mark.parametrize("offset", M.OFFSETS)
def test_model_is_the_oracle_at_the_edges(offset, inner):
    cols, valid = edge_batch()
    for name, expr in M.shapes(offset, inner).items():
        plan = per_row_plan(expr)
        got, _ = smoke.run_query(H.oracle_backend(), plan, [(cols, valid)])
        want = M.grouped(plan.dimensions, [(cols, valid)], lambda c, v: np.ones(len(c["request_at"][1]), bool),
                         lambda c, v: np.ones(len(c["request_at"][1])))
        assert {k: int(x) for k, x in got.items()} == {k: int(x) for k, x in want.items()}, (name, offset, inner)


def test_model_by_hand():
    """Values worked out on paper.  08:00 UTC is midnight in UTC-8; an integer literal makes every node signed, and Floor is
    x - x % y with C's remainder, so a negative local time is floored TOWARDS zero: -1 -> 0, -28801 -> -28800."""
    cols = {"request_at": (abi.Uint32, np.array([28800, 28799, 0, 345600, 2**32 - 1], np.uint32))}
    valid = {"request_at": None}
    s = M.shapes(-28800)

    def bits(e):
        return M.evaluate(e, cols, valid)[0].view(np.int32).tolist()
    assert bits(s["fixed_zone_hour"]) == [0, 0, -28800, 316800, -28800]
    assert bits(s["fixed_zone_time_of_day"]) == [0, -1, -28800, 57600, -28801]
    assert bits(s["hour_of_day"]) == [28800, 25200, 0, 0, 0]  # (2^32 - 1 reads as -1: -1 % 86400 = -1, floored to 0)
    assert bits(s["hour_of_week"]) == [-316800, -316800, -345600, 0, -345600]  # 1970-01-05 00:00 UTC, a Monday, is hour 0
    nulls = {"request_at": np.array([True, False, True, True, False])}
    got, ok, _ = M.evaluate(s["fixed_zone_hour_of_week"], cols, nulls)
    assert got.tolist()[1] == 0 and got.tolist()[4] == 0 and ok.tolist() == [True, False, True, True, False]


@pytest.mark.parametrize("bucketizer,want", [("minute", 60), ("hour", 3600), ("day", 86400), ("quarter-hour", 900), ("15m", 900),
                                             ("4 hours", 14400), ("2h", 7200), ("30 minutes", 1800)])
def test_regular_buckets(bucketizer, want):
    assert queries.regular_bucket_seconds(bucketizer) == want
    e = queries.time_dimension(bucketizer, "ts")
    assert isinstance(e, Binary) and e.op == abi.Floor and isinstance(e.lhs, Col) and e.rhs.value == want


@pytest.mark.parametrize("bad", ["7 minutes", "5 hours", "2 days", "fortnight", "1 minutes of day", "7 minutes of day"])
def test_bucketizers_the_compiler_rejects(bad):
    with pytest.raises(ValueError):
        queries.time_dimension(bad, "ts")


def test_expression_shapes():
    def text(e):
        if isinstance(e, Col):
            return e.name
        if isinstance(e, Const):
            return repr(e.value)
        return {abi.Plus: "Plus", abi.Minus: "Minus", abi.Mod: "Mod", abi.Floor: "Floor", abi.Divide: "Divide"}[e.op] + f"({text(e.lhs)}, {text(e.rhs)})"
    td = queries.time_dimension
    assert text(td("hour", "ts", -28800)) == "Floor(Plus(ts, -28800), 3600)"
    assert text(td("hour of day", "ts")) == "Floor(Mod(ts, 86400), 3600)"
    assert text(td("10 minutes of day", "ts")) == "Floor(Mod(ts, 86400), 600)"
    assert text(td("time of day", "ts", 19800)) == "Mod(Plus(ts, 19800), 86400)"
    assert text(td("hour of week", "ts")) == "Floor(Mod(Minus(ts, 345600), 604800), 3600)"
    assert text(td("hour of week", "ts", 3600)) == "Floor(Mod(Minus(Plus(ts, 3600), 345600), 604800), 3600)"
    assert text(td("day of week", "ts")) == "Divide(Floor(Mod(Minus(ts, 345600), 604800), 86400), 86400.0)"
    assert td("hour", "ts", -28800).lhs.out_type == abi.Int32 and td("hour of day", "ts").lhs.out_type == abi.Uint32
