// Partitioned, LDS-resident HashReduce (hash_reduce_lds.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <memory>

#include "aggregate.hpp"
#include "ares_algorithm.h"
#include "dim_layout.hpp"
#include "fast_eval.hpp"

namespace ares {

// true when the aggregate has a native LDS atomic (sums of 4/8-byte integers and floats, integer
// min/max); AVG and float min/max stay on the global-table path.
bool hash_reduce_lds_supported(const AggSpec &a);

// Returns the number of groups, or -1 when a partition region overflowed (the caller then runs the
// global-table path; outputs written so far are simply overwritten).
int hash_reduce_lds(int device, const DimensionVector &inputKeys, const uint8_t *inputValues,
                    const DimensionVector &outputKeys, uint8_t *outputValues, const AggSpec &a, int length,
                    hipStream_t stream);

// ---- fused scan: filter + projection evaluated from the source columns ------------------------------
// (kFusedFilters: the Go host's two time filters, a cutoff filter on live batches and three of the query's own)
// kFusedDims / kFusedCols (round 6): what the ABI allows — MAX_DIMENSIONS = 8 (query/time_series_aggregate.h:36-37) — in slots
// of 4, 2 or 1 bytes; eight dimensions + measure + a filter column = ten column slots.  More than four dimensions run on the
// kernels generated for the plan's shape only (the precompiled generic kernels are instantiated for one to four).
constexpr int kFusedCols = 10, kFusedFilters = 6, kFusedDims = 8;
constexpr int kGenericFusedDims = 4;
constexpr int kExtensionFilters = 4;  // AresFusedQuery::filters (include/ares_extensions.h)
// Sort + Reduce over rows that exist (fused_sort_reduce_vectors) also takes slots of 8 and 16 bytes (Int64 / Uint64 / GeoPoint,
// UUID).  Its generated scan holds four rows per lane in registers: up to eight dimensions of 4 / 2 / 1 bytes as before, and —
// once a slot is wider than that — up to kSortVectorValueBytes value bytes per row (the eight-dimension shape's footprint).
// ONE predicate for Sort (which defines itself lazily), Reduce (which consumes the definition) and the generator: a layout
// beyond it keeps the real Sort + Reduce.
constexpr int kSortVectorValueBytes = 32;
inline bool sort_vector_layout_supported(const uint8_t numDimsPerDimWidth[NUM_DIM_WIDTH]) {
  int nd = 0;
  for (int w = 0; w < NUM_DIM_WIDTH; w++) nd += numDimsPerDimWidth[w];
  const bool wide = numDimsPerDimWidth[0] || numDimsPerDimWidth[1];
  return nd >= 1 && nd <= kFusedDims && (!wide || dim_value_bytes(numDimsPerDimWidth) <= static_cast<size_t>(kSortVectorValueBytes));
}
struct FusedColumn {
  const uint32_t *vals;
  const uint8_t *nulls;
  uint32_t bitOff;
  uint32_t step;  // bytes per stored value (FastOperands::step): 4, 2 or 1; 0 reads as 4
};
struct FusedExpr {
  FastOperands f;  // akind / arity / functor / I / rk / constant / divLike / chain (pointers unused)
  int col;
  int outKind;     // kind of the stored dimension value
};
struct FusedPlanD {
  int numCols;
  FusedColumn cols[kFusedCols];
  int numFilters;
  FusedExpr filters[kFusedFilters];
  FusedExpr dims[kFusedDims];
  FusedExpr measure;
  int measureDtype, measureWidth;
  uint64_t identity;  // measure-transform identity of the aggregate (query/utils.hpp:169-184)
  // bytes of dimension d's slot in the dimension vector, in vector (= descending width) order: 4, 2 or 1; 0 reads as 4.
  // Plans with a narrow slot or a narrow column ("narrow plans") run on the kernels generated for their shape only
  // (hr_rtc.hip); the precompiled generic kernels read 4-byte columns and write 4-byte slots.
  uint8_t dimWidth[kFusedDims];
  // AVG_FLOAT (Sort + Reduce only): the measure's record carries the FLOAT the measure transform would have stored as the
  // pair's average — the value as measureDtype, then as a float (avg_measure_float) — and the top bit of its row word says
  // "null measure": the pair {0, 0} instead of {average, 1}
  int measureAvg;
};
// Two plans describe the same scan over the same columns: every field a scan, a merge or a spec maker reads, one by one
// (the structs hold padding: their bytes are not compared).  What a hinted plan and the plan HashReduce derives from the
// stream's queue must satisfy before a scan launched from the first is taken for the second's.
inline bool fused_expr_equal(const FusedExpr &a, const FusedExpr &b) {
  return a.col == b.col && a.outKind == b.outKind && a.f.akind == b.f.akind && a.f.arity == b.f.arity && a.f.functor == b.f.functor &&
         a.f.I == b.f.I && a.f.rk == b.f.rk && a.f.bkind == b.f.bkind && a.f.bbits == b.f.bbits && a.f.bok == b.f.bok &&
         a.f.divLike == b.f.divLike && (a.f.step ? a.f.step : 4) == (b.f.step ? b.f.step : 4) && fast_chain_equal(a.f.chain, b.f.chain);
}
inline bool fused_plan_equal(const FusedPlanD &a, const FusedPlanD &b, int nd) {
  if (a.numCols != b.numCols || a.numFilters != b.numFilters || a.measureDtype != b.measureDtype || a.measureWidth != b.measureWidth ||
      a.identity != b.identity || a.measureAvg != b.measureAvg)
    return false;
  for (int c = 0; c < a.numCols; c++)
    if (a.cols[c].vals != b.cols[c].vals || a.cols[c].nulls != b.cols[c].nulls || a.cols[c].bitOff != b.cols[c].bitOff ||
        (a.cols[c].step ? a.cols[c].step : 4) != (b.cols[c].step ? b.cols[c].step : 4))
      return false;
  for (int k = 0; k < a.numFilters; k++)
    if (!fused_expr_equal(a.filters[k], b.filters[k])) return false;
  for (int d = 0; d < nd; d++)
    if (!fused_expr_equal(a.dims[d], b.dims[d]) || (a.dimWidth[d] ? a.dimWidth[d] : 4) != (b.dimWidth[d] ? b.dimWidth[d] : 4)) return false;
  return fused_expr_equal(a.measure, b.measure);
}
inline int fused_dim_width(const FusedPlanD &p, int d) { return p.dimWidth[d] ? p.dimWidth[d] : 4; }
inline int fused_col_step(const FusedPlanD &p, int c) { return p.cols[c].step ? static_cast<int>(p.cols[c].step) : 4; }
// a dimension or the measure is a constant chain (FastOperands::chain)
inline bool fused_plan_chained(const FusedPlanD &p, int nd) {
  for (int d = 0; d < nd; d++)
    if (p.dims[d].f.chain.n) return true;
  return p.measure.col >= 0 && p.measure.f.chain.n != 0;
}
inline bool fused_plan_narrow(const FusedPlanD &p, int nd) {
  if (nd > kGenericFusedDims) return true;  // (generated kernels only, like a plan with narrow slots)
  if (fused_plan_chained(p, nd)) return true;  // (the precompiled generic scan and merge evaluate one node per expression)
  for (int d = 0; d < nd; d++)
    if (fused_dim_width(p, d) != 4) return true;
  for (int c = 0; c < p.numCols; c++)
    if (fused_col_step(p, c) != 4) return true;
  return false;
}

// ---- building a plan ------------------------------------------------------------------------------------------------
// One copy of each decision for everybody who writes a FusedPlanD: the two fusions over a stream's pending work
// (fused_consumers.hip), the fused extension (hash_reduce_lds.hip) and the vector-sourced launcher (hr_rtc.hip).  The struct is
// memset to zero first; the spec makers (hr_rtc_gen.hpp) and the launches read it field by field.
inline FusedColumn fused_column_of(const FastOperands &f) { return FusedColumn{f.vals, f.nulls, f.bitOff, static_cast<uint32_t>(f.step ? f.step : 4)}; }
// the expression without what belongs to one launch (the column lives in its slot, the rows come from the scan); its chain
// is shape and stays
inline FastOperands fused_strip(FastOperands f) {
  f.vals = nullptr;
  f.nulls = nullptr;
  f.idx = nullptr;
  f.pad = 0;
  return f;
}
// kind of the value a sink of `dtype` stores
inline int fused_kind_of(int dtype) { return (dtype == Int32 || dtype == Int16 || dtype == Int8) ? K_I32 : (dtype == Uint32 || dtype == Uint16 || dtype == Uint8) ? K_U32 : K_F32; }
// The plan's column slot for the operand's column, or a new one behind the slots in use; -1: no room among `maxCols`.
// A plan may hold one column in several slots (a dimension and the measure of the same column are simply loaded twice; the
// second load hits L1).  Which of them a filter is given shows in the plan, hence in cache keys and generated sources, and
// the two kinds of caller have always differed: the extension's filters take the first, a journal's filters the last.
enum FusedReuse { kFusedNoReuse, kFusedReuseFirst, kFusedReuseLast };
inline int fused_column(FusedPlanD &plan, const FastOperands &f, int maxCols, FusedReuse reuse) {
  const FusedColumn col = fused_column_of(f);
  int found = -1;
  for (int c = 0; reuse != kFusedNoReuse && c < plan.numCols; c++)
    if (plan.cols[c].vals == col.vals && plan.cols[c].nulls == col.nulls && plan.cols[c].bitOff == col.bitOff && plan.cols[c].step == col.step &&
        (found < 0 || reuse == kFusedReuseLast))
      found = c;
  if (found >= 0) return found;
  if (plan.numCols >= maxCols) return -1;
  plan.cols[plan.numCols] = col;
  return plan.numCols++;
}
// Dimension d is what a queued transform would have written into the vector's slot d (`width` bytes): column slot d.
inline void fused_plan_dim(FusedPlanD &plan, int d, const FastOperands &f, const SinkD &sink, int width) {
  plan.cols[d] = fused_column_of(f);
  plan.dims[d].f = fused_strip(f);
  plan.dims[d].col = d;
  plan.dims[d].outKind = fused_kind_of(sink.dtype);
  plan.dimWidth[d] = static_cast<uint8_t>(width);
}
// The measure is what a queued transform would have written into the measure vector: column slot nd.
inline void fused_plan_measure(FusedPlanD &plan, int nd, const FastOperands &f, const SinkD &sink, int valueBytes) {
  plan.cols[nd] = fused_column_of(f);
  plan.measure.f = fused_strip(f);
  plan.measure.col = nd;
  plan.measure.outKind = fused_kind_of(sink.dtype);
  plan.measureDtype = sink.dtype;
  plan.measureWidth = valueBytes;
  plan.identity = sink.identity;
  plan.measureAvg = sink.agg == AGGR_AVG_FLOAT ? 1 : 0;
  plan.numCols = nd + 1;
}
// ... or a constant (Sort + Reduce: COUNT(*)): no column
inline void fused_plan_const_measure(FusedPlanD &plan, int nd, uint64_t constBits, int dtype, int valueBytes) {
  plan.measure.col = -1;
  plan.measure.f.bbits = static_cast<uint32_t>(constBits);  // (what the scan's records carry; the merge takes constBits)
  plan.measureDtype = dtype;
  plan.measureWidth = valueBytes;
  plan.numCols = nd;
}
// The filters of a journal, after dimensions and measure: each reuses a slot that holds its column or takes a spare one.
// false: more filters or columns than a plan holds.
inline bool fused_plan_filters(FusedPlanD &plan, const FastOperands *filters, size_t count) {
  if (count > static_cast<size_t>(kFusedFilters)) return false;
  for (size_t k = 0; k < count; k++) {
    const int col = fused_column(plan, filters[k], kFusedCols, kFusedReuseLast);
    if (col < 0) return false;
    plan.filters[k].f = fused_strip(filters[k]);
    plan.filters[k].col = col;
    plan.filters[k].outKind = K_BOOL;
  }
  plan.numFilters = static_cast<int>(count);
  return true;
}
// Column slot d = rows [rowBase, ..) of dimension d of a materialised dimension vector (`widths`: bytes per slot in vector
// order, null = all four bytes); slot nd, the measure's, is the caller's.
inline void fused_plan_vector_columns(FusedPlanD &plan, const uint8_t *dimValues, size_t capacity, int nd, const int *widths, uint32_t rowBase) {
  plan.numCols = nd + 1;
  size_t valueBytes = 0, off = 0;
  for (int d = 0; d < nd; d++) valueBytes += static_cast<size_t>(widths ? widths[d] : 4);
  for (int d = 0; d < nd; d++) {
    const size_t w = static_cast<size_t>(widths ? widths[d] : 4);
    plan.cols[d].vals = reinterpret_cast<const uint32_t *>(dimValues + off * capacity + w * rowBase);
    plan.cols[d].nulls = dimValues + valueBytes * capacity + static_cast<size_t>(d) * capacity + rowBase;
    off += w;
  }
}

// Column slots of a plan of ND dimensions: dimension d -> slot d, measure -> slot ND; a filter reuses
// a slot that already holds its column or takes the one spare slot ND + 1.
// Returns the number of groups; -1: a partition region overflowed (or a partition needs the generic multi-round merge and
// the plan is narrow) — outputs may be partly written; kFusedUnavailable: declined before anything was launched (narrow
// plan whose generated kernels are not loaded yet, previous results not grouped ...).  Either way the caller runs the
// unfused sequence.
constexpr int kFusedUnavailable = -2;
// Room of a scanning workgroup's private record stream of one partition: (2 << slack) x the mean + 64.  Batches whose rows
// arrive SORTED (archive batches: a workgroup's contiguous chunk holds two or three time buckets, hence few distinct groups
// and unevenly filled partitions) overflow the default (slack 0: twice the mean); the call that sees the overflow flag grows
// the slack — it stays grown for the process — and runs again instead of leaving the fast path.
int record_stream_slack();
bool grow_record_stream_slack();  // false: already at its limit (8 x the mean)
// stash: the batch's scan as a filter call launched it ahead of this call (below), or null.  It is taken for this call's own
// scan when the call decides exactly what was decided then — same plan, rows, previous size, partitions, record format and
// stream room, no region A — and dropped otherwise: the call then scans as ever.
struct ScanStash;
int fused_hash_reduce_run(int device, const FusedPlanD &plan, int batchRows, const DimensionVector &prevKeys,
                          const uint8_t *prevValues, int prevSize, const DimensionVector &outKeys, uint8_t *outValues,
                          const AggSpec &a, hipStream_t stream, std::shared_ptr<ScanStash> stash = nullptr);

// ---- scan at filter (hash_reduce_lds.hip; the filter call itself: transform.hip; the hint: fused_consumers.hip)
// What AresHintFusedBatch said about a stream's next InitIndexVector ... HashReduce sequence.
struct ScanHint {
  FusedPlanD plan;  // built like plan_from_queue builds HashReduce's: fused_plan_dim x nd, fused_plan_measure, fused_plan_filters
  int nd, batchRows, prevSize;
  FastOperands filters[kFusedFilters];  // the plan's filters with their columns: what the journal must hold when the last one is called
  struct Range {
    const uint8_t *lo, *hi;
  } ranges[2 * kFusedCols];  // bytes the scan reads: a write or a free inside ends the hint and whatever was launched from it
  int numRanges;
};
// AresScanAtFilterStats: one counter each, in this order
enum ScanAheadCounter {
  kScanAheadHints,             // hints taken
  kScanAheadScans,             // scans launched at a filter
  kScanAheadHonoured,          // ... whose regions HashReduce merged its result from (counted when that call ends well)
  kScanAheadDeclined,          // hints declined (short column, shape, a switch)
  kScanAheadDiscardPlan,       // scans discarded: HashReduce derived another plan
  kScanAheadDiscardShape,      // ... other rows, previous size, partitions, kernel or stream room, or region A was needed
  kScanAheadDiscardTouched,    // ... a hinted column was written or freed
  kScanAheadDiscardAbandoned,  // ... the stream's HashReduce never came (or did not consume the stream's queue)
  kScanAheadDiscardRetry,      // scans taken whose call then scanned again or fell back (stale ranges, record stream overflow)
  kScanAheadLatched,           // hints ignored: the stream's last two scans were discarded
  kScanAheadCounters
};
void scan_ahead_count(int which);
void scan_ahead_stats(unsigned long long *out);
bool scan_at_filter_enabled();  // ARES_SCAN_AT_FILTER (on unless 0), and the sibling libmem.so reports writes and frees
void scan_hint_set(int device, hipStream_t stream, const ScanHint &hint);
void scan_hint_init_index(int device, hipStream_t stream);  // InitIndexVector on the stream: the hint's batch begins, or has ended
bool scan_hint_live(int device, hipStream_t stream, ScanHint *out);  // the hint of the batch that is running, nothing launched from it yet
std::shared_ptr<ScanStash> fused_scan_ahead(int device, const ScanHint &hint, hipStream_t stream, uint32_t *hostCount, int *grid);
void scan_stash_put(int device, hipStream_t stream, std::shared_ptr<ScanStash> stash);
std::shared_ptr<ScanStash> scan_stash_take(int device, hipStream_t stream);
// reason: kScanAheadHonoured or a discard counter; blame: the discard counts towards the stream's two-discard latch
void scan_stash_settled(int device, hipStream_t stream, int reason, bool blame = true);
// a byte range is written (or a copy touches it), or freed: hints that read it die; scans launched from them die unless `freed`
void scan_ahead_note_touch(int device, const void *ptr, size_t bytes, bool freed);
void scan_ahead_stream_gone(int device, hipStream_t stream);

}  // namespace ares
