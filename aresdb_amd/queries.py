"""Query plans of the BASELINE configurations, as the AQL compiler would
hand them to the batch executor."""
from . import abi
from .executor import Binary, Col, Const, DimensionSpec, QueryPlan


def c3_plan(use_hash_reduction=True, with_filter=True, dims=("ts", "d1", "d2", "d3"), d1_below=90, ts_range=None, sort_measure=None,
            eight_dims=False):
    """BASELINE config C3; `dims` selects a subset of its four group-by dimensions (lower-cardinality variants of the
    same query: the filter and the measure stay), `d1_below` the filter constant.  ts_range = (from, to): the two time
    filters the Go host puts in front of every fact-table query's own filters — ts >= from, ts < to
    (query/aql_processor.go:543-559, query/common/time_filter.go:371-397).  sort_measure: the same group-by through the
    reference's DEFAULT path, Sort + Reduce (config/ares.yaml:11 enable_hash_reduction: false; query/aql_context.go:426-434):
    "count" = COUNT(*), a column name = SUM over that unsigned column."""
    specs = {"ts": DimensionSpec(Binary(abi.Floor, Col("ts"), Const(3600)), abi.Uint32),
             "d1": DimensionSpec(Col("d1"), abi.Uint32), "d2": DimensionSpec(Col("d2"), abi.Uint32),
             "d3": DimensionSpec(Col("d3"), abi.Uint32)}
    time_filters = [] if ts_range is None else [Binary(abi.GreaterThanOrEqual, Col("ts"), Const(int(ts_range[0]))),
                                                Binary(abi.LessThan, Col("ts"), Const(int(ts_range[1])))]
    filters = time_filters + ([Binary(abi.LessThan, Col("d1"), Const(d1_below))] if with_filter else [])
    dimensions = [specs[d] for d in dims]
    if eight_dims:  # MAX_DIMENSIONS (query/time_series_aggregate.h:36-37): four more, functions of the first four — the same groups
        dimensions = dimensions + [DimensionSpec(Binary(abi.Plus, Col("d1"), Const(5)), abi.Uint32),
                                   DimensionSpec(Binary(abi.Multiply, Col("d2"), Const(3)), abi.Uint32),
                                   DimensionSpec(Binary(abi.Plus, Col("d3"), Const(1)), abi.Uint32),
                                   DimensionSpec(Binary(abi.Mod, Col("d2"), Const(7)), abi.Uint32)]
    if sort_measure == "count":  # COUNT(*): SUM_UNSIGNED over the literal 1 into 4 bytes, never hash-reduced (aql_compiler.go:1191-1197)
        return QueryPlan(filters=filters, dimensions=dimensions, measure=Const(1), agg=abi.AGGR_SUM_UNSIGNED,
                         measure_type=abi.Uint32, use_hash_reduction=False)
    if sort_measure:  # SUM over an unsigned column: 8 bytes, output type Int64 (time_series_aggregate.go:352-361); Sort + Reduce
        return QueryPlan(filters=filters, dimensions=dimensions, measure=Col(sort_measure), agg=abi.AGGR_SUM_UNSIGNED,
                         measure_type=abi.Int64, use_hash_reduction=False)
    return QueryPlan(
        filters=filters,
        dimensions=dimensions,
        measure=Col("m"), agg=abi.AGGR_SUM_FLOAT, measure_type=abi.Float64,
        use_hash_reduction=use_hash_reduction)


def c2_plan(threshold):
    """BASELINE config C2: single uint32 predicate + COUNT(*) — measure literal 1, AGGR_SUM_UNSIGNED,
    4-byte measure, no dimensions, sort path (query/aql_compiler.go:1191-1197)."""
    return QueryPlan(filters=[Binary(abi.LessThan, Col("ts"), Const(threshold))], dimensions=[],
                     measure=Const(1), agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32,
                     use_hash_reduction=False)


def select_plan(columns, filters, limit=-1, use_fused_extension=False):
    """A non-aggregation query, SELECT columns WHERE filters LIMIT limit (limit < 0: none): `columns` = [(expression, output
    DataType)], `filters` = comparison expressions.  The AQL compiler flags such a query by its measure, the number literal 1
    (query/aql_compiler.go:1147-1153); the non-aggregation executor never evaluates it."""
    return QueryPlan(filters=list(filters), dimensions=[DimensionSpec(e, t) for e, t in columns], measure=Const(1),
                     agg=abi.AGGR_SUM_UNSIGNED, measure_type=abi.Uint32, use_hash_reduction=True,
                     use_fused_extension=use_fused_extension, is_non_aggregation=True, limit=limit)


# ---- time dimensions (query/time_bucketizer.go:72-174, 176-273) -------------------------------------------------------------
SECONDS_PER_HOUR, SECONDS_PER_DAY, SECONDS_PER_WEEK, SECONDS_PER_4_DAYS = 3600, 86400, 604800, 345600
_UNIT_SECONDS = {"m": 60, "h": SECONDS_PER_HOUR, "d": SECONDS_PER_DAY}
_UNIT_NAMES = {"minutes": "m", "minute": "m", "day": "d", "hours": "h", "hour": "h"}
# "x of y": (base unit, bucket size)
_RECURRING = {"time of day": (1, SECONDS_PER_DAY), "hour of day": (SECONDS_PER_HOUR, SECONDS_PER_DAY),
              "hour of week": (SECONDS_PER_HOUR, SECONDS_PER_WEEK), "day of week": (SECONDS_PER_DAY, SECONDS_PER_WEEK)}


def regular_bucket_seconds(bucketizer):
    """Seconds of a regular time bucket: "minute", "hour", "day", "quarter-hour", "N minutes", "N hours", "Nm", "Nh"
    (query/common/time_bucketizer.go:79-137: N minutes divide an hour, N hours a day)."""
    s = "15m" if bucketizer == "quarter-hour" else bucketizer.lower()
    parts = s.split(" ", 1)
    if len(parts) == 2:
        if parts[1] not in _UNIT_NAMES:
            raise ValueError(f"unknown time bucketizer {bucketizer!r}")
        size, unit = parts[0], _UNIT_NAMES[parts[1]]
    else:
        s = _UNIT_NAMES.get(s, s)
        size, unit = s[:-1] or "1", s[-1:]
        if unit not in _UNIT_SECONDS:
            raise ValueError(f"unknown time bucketizer {bucketizer!r}")
    if s[:-1] or len(parts) == 2:  # an explicit size: minutes and hours only
        n = int(size)
        if unit == "d" or not (0 < n < 60 and ((unit == "m" and 60 % n == 0) or (unit == "h" and 24 % n == 0))):
            raise ValueError(f"invalid bucket size in {bucketizer!r}")
        return n * _UNIT_SECONDS[unit]
    return _UNIT_SECONDS[unit]


def time_dimension(bucketizer, column, fixed_offset=0, inner_type=None):
    """The expression the AQL compiler builds for a time dimension over the time column `column` (buildTimeDimensionExpr,
    query/time_bucketizer.go:72-174) in UTC or — fixed_offset != 0 — in a fixed zone whose offset does not change inside the
    query's range: CONVERT_TZ is the Plus functor over (column, offset).
      regular buckets ("hour", "15m", "4 hours", "day"):   Floor(t, seconds)
      "time of day":                                         Mod(t, 86400)
      "hour of day", "N minutes of day":                     Floor(Mod(t, 86400), unit)
      "hour of week":                                        Floor(Mod(Minus(t, 345600), 604800), 3600)   (1970-01-01 is a Thursday)
      "day of week":                                         Divide(Floor(Mod(Minus(t, 345600), 604800), 86400), 86400.0)
    with t = column, or Plus(column, fixed_offset).  inner_type: the data type of the inner nodes' scratch frames (default:
    Int32 where an offset makes the time signed, Uint32 otherwise)."""
    if inner_type is None:
        inner_type = abi.Int32 if fixed_offset else abi.Uint32
    t = Col(column) if isinstance(column, str) else column
    if fixed_offset:
        t = Binary(abi.Plus, t, Const(int(fixed_offset)), out_type=inner_type)  # (CONVERT_TZ over a literal reads no offset table)
    recurring = None
    if bucketizer.endswith("minutes of day"):
        parts = bucketizer.split()
        if len(parts) < 4:
            raise ValueError(f"a number goes before minutes of day: {bucketizer!r}")
        n = int(parts[0])
        if n < 2 or n > 30 or 30 % n:
            raise ValueError(f"only 2, 3, 5, 6, 10, 15 or 30 minutes of day: {bucketizer!r}")
        recurring = (60 * n, SECONDS_PER_DAY)
    elif bucketizer in _RECURRING:
        recurring = _RECURRING[bucketizer]
    if recurring is None:
        return Binary(abi.Floor, t, Const(regular_bucket_seconds(bucketizer)), out_type=inner_type)
    unit, size = recurring
    if unit == 1:
        return Binary(abi.Mod, t, Const(size), out_type=inner_type)
    if size == SECONDS_PER_WEEK:  # weeks start on Monday
        t = Binary(abi.Minus, t, Const(SECONDS_PER_4_DAYS), out_type=inner_type)
    e = Binary(abi.Floor, Binary(abi.Mod, t, Const(size), out_type=inner_type), Const(unit), out_type=inner_type)
    if unit >= SECONDS_PER_DAY:  # the day's number: "for division, everything is converted to float"
        e = Binary(abi.Divide, e, Const(float(unit)), out_type=abi.Float32)
    return e
