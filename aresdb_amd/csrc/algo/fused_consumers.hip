// A stream's pending work read as a fused plan: HashReduce and Sort + Reduce consume the queue of root transforms and the
// filter journal instead of having them launched (second-stage fusion, include/ares_extensions.h), the hint that lets a
// batch's last filter launch the fused scan (AresHintFusedBatch), and the lazily defined sorts Reduce consumes.  State,
// lock and invariants: deferral.hpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "ares_extensions.h"

#include "deferral.hpp"
#include "hash_reduce_lds.hpp"
#include "sort_reduce_fused.hpp"

namespace ares {

// ---- a stream's pending work as a fused plan: what HashReduce and Sort + Reduce share ---------------------------------
namespace {
// What a stream's queue is to a Reduce over `length` rows of a dimension vector (match_queue)
struct QueueMatch {
  int prev = 0;                            // rows of the previous result: the queue writes rows [prev, length)
  int dimJob[kFusedDims], measureJob = -1;  // which job writes which dimension, which one the measure (-1: none queued)
  // survivors of the queue's rows: the whole batch (no filter ran: no journal, n0 = the queue's rows) or what the journalled
  // filters keep (n0 = the rows they read)
  const FilterJournal *journal = nullptr;
  int n0 = 0;
};
// Is the queue `pq` "the dimension columns [and the measure] of rows [prev, length) of `in`", with survivors that can be
// re-derived where filters ran?  Only answers: what a caller does on "no" is its own.  Caller holds the device's DeferLock.
bool match_queue(const PendingQueue &pq, const DimensionVector &in, const DimLayoutD &L, int length, QueueMatch *m) {
  const int nd = L.numDims, prev = m->prev = length - pq.n;
  const size_t cap = static_cast<size_t>(in.VectorCapacity);
  if (pq.n <= 0 || prev < 0 || nd < 1 || nd > kFusedDims || in.NumDimsPerDimWidth[0] || in.NumDimsPerDimWidth[1]) return false;
  if (pq.jobs.count != nd && pq.jobs.count != nd + 1) return false;
  for (int c = 0; c < kFusedDims; c++) m->dimJob[c] = -1;
  m->measureJob = -1;
  for (int k = 0; k < pq.jobs.count; k++) {
    const SinkD &s = pq.jobs.s[k];
    if (s.type == SINK_MEASURE) {
      if (m->measureJob >= 0 || s.baseCounts) return false;
      m->measureJob = k;
      continue;
    }
    int d = -1;
    for (int c = 0; c < nd; c++)
      if (s.values == in.DimValues + static_cast<size_t>(L.valueOff[c]) * cap + static_cast<size_t>(L.width[c]) * prev &&
          s.nulls == in.DimValues + static_cast<size_t>(L.valueBytes) * cap + cap * c + prev && s.width == L.width[c])
        d = c;
    if (s.type != SINK_DIM || d < 0 || m->dimJob[d] >= 0) return false;
    m->dimJob[d] = k;
  }
  for (int c = 0; c < nd; c++)
    if (m->dimJob[c] < 0) return false;
  m->n0 = pq.n;
  if (!pq.idx) return true;
  auto j = t_state->journals.find(pq.idx);
  if (j == t_state->journals.end() || !j->second.valid || j->second.start != 0) return false;  // filters ran: the journal must tell
  m->journal = &j->second;
  m->n0 = j->second.n0;
  return true;
}
// the queued measure is this call's: its rows, its width, its aggregate
bool measure_job_matches(const SinkD &s, const uint8_t *measureRows, int valueBytes, int aggFunc) {
  return s.values == measureRows && s.width == valueBytes && s.agg == aggFunc &&
         !(valueBytes == 8 && s.identity != 0);  // records carry 4 bytes: a null must widen to the identity
}
// every source column holds the n0 rows a scan reads
bool columns_cover(const uint32_t *colRows, size_t count, int n0) {
  for (size_t k = 0; k < count; k++)
    if (colRows[k] < static_cast<uint32_t>(n0)) return false;
  return true;
}
// The (zeroed) plan of a matched queue whose columns — and the journalled filters' — hold the n0 rows a scan reads: its
// dimensions, its measure job — or, measureJob < 0, the constant measure of Sort + Reduce — and the journal's filters.
// false: a column is too short or the filters do not fit.  Caller holds the device's DeferLock.
bool plan_from_queue(FusedPlanD &plan, const PendingQueue &pq, const DimLayoutD &L, const QueueMatch &m, int valueBytes, uint64_t constBits,
                     int constDtype) {
  if (!columns_cover(pq.colRows, pq.jobs.count, m.n0)) return false;
  const int nd = L.numDims;
  for (int c = 0; c < nd; c++) fused_plan_dim(plan, c, pq.jobs.f[m.dimJob[c]], pq.jobs.s[m.dimJob[c]], L.width[c]);
  if (m.measureJob >= 0) fused_plan_measure(plan, nd, pq.jobs.f[m.measureJob], pq.jobs.s[m.measureJob], valueBytes);
  else fused_plan_const_measure(plan, nd, constBits, constDtype, valueBytes);
  return !m.journal || (columns_cover(m.journal->colRows.data(), m.journal->filters.size(), m.n0) &&
                        fused_plan_filters(plan, m.journal->filters.data(), m.journal->filters.size()));
}
// A fused scan evaluates the queue instead of launching it: `q` takes it over.  Caller holds the device's DeferLock.
void take_queue(PendingQueue &pq, PendingQueue &q) {
  q = pq;  // taken out of the queue: nobody else launches it
  pq.jobs.count = 0;
  pq.reads.clear();
  pq.writes.clear();
  pq.keep.clear();  // (the copy holds the decoded columns from here on: left in place they piled up, two per batch, for the life
                    // of the stream — 86 GB after 143 archive batches — and every later copy of the queue took the pile along)
  pq.overWait = false;
  if (q.idx) {  // (decoded columns only the filters read live as long as the consumed queue does: the scan is launched by the caller)
    auto jk = t_state->journals.find(q.idx);
    if (jk != t_state->journals.end()) q.keep.insert(q.keep.end(), jk->second.keep.begin(), jk->second.keep.end());
    t_state->journals.erase(q.idx);
  }
}
// *a: the aggregate of the call, when there is such an aggregate and the fused consumer asked (`supported`) takes it
template <typename Supported>
bool supported_agg_spec(int aggFunc, int valueBytes, Supported &&supported, AggSpec *a) {
  try {
    *a = make_agg_spec(aggFunc, valueBytes);
    return supported(*a);
  } catch (std::exception &) {
    return false;
  }
}
// Runs a fused attempt.  An exception it throws still means "declined" (-1: the caller runs the ordinary sequence), but what
// it said is kept: a line in the ARES_RTC_TRACE file and, with ARES_HR_TRACE, on stderr.
template <typename Attempt>
int guarded_attempt(const char *what, Attempt &&attempt) {
  try {
    return attempt();
  } catch (std::exception &e) {
    const std::string line = std::string(what) + " threw, the call falls back: " + e.what();
    slow_trace(line.c_str(), 0.0);
    if (hr_trace_enabled()) fprintf(stderr, "%s\n", line.c_str());
    return -1;
  }
}
}  // namespace

// HashReduce's first move: when the stream's pending queue is exactly "the dimension columns and the
// measure of rows [prev, prev + n) of inputKeys / inputValues", evaluate it on the fly (the fused
// scan of hash_reduce_lds.hip) instead of launching it.  Returns false when the call must take the
// ordinary path (whatever was pending has been launched, in stream order).
bool fuse_pending_into_hash_reduce(int device, hipStream_t stream, const DimensionVector &in, const uint8_t *inValues,
                                   const DimensionVector &out, uint8_t *outValues, int valueBytes, int length, int aggFunc,
                                   int *groups) {
  if (!fuse_available()) return false;
  const bool forcedGlobal = global_table_forced();
  PendingQueue q;
  FusedPlanD plan;
  memset(&plan, 0, sizeof(plan));
  int nd = 0;
  QueueMatch m;
  AggSpec a;
  {
    DeferLock lock(device);
    auto it = t_state->pending.find(stream);
    if (it == t_state->pending.end() || it->second.jobs.count == 0) {
      // (nothing is pending — the batch's transforms were launched, or there were none: a scan launched at the filter goes unread)
      if (scan_stash_take(device, stream)) scan_stash_settled(device, stream, kScanAheadDiscardAbandoned);
      return false;
    }
    PendingQueue &pq = it->second;
    bool ok = !forcedGlobal;
    // dimension slots of 4, 2 or 1 bytes, in the vector's (descending width) order
    nd = in.NumDimsPerDimWidth[2] + in.NumDimsPerDimWidth[3] + in.NumDimsPerDimWidth[4];
    for (int k = 0; k < NUM_DIM_WIDTH; k++)
      ok = ok && (k >= 2 || in.NumDimsPerDimWidth[k] == 0) && out.NumDimsPerDimWidth[k] == in.NumDimsPerDimWidth[k];
    ok = ok && nd >= 1 && nd <= kFusedDims;
    DimLayoutD L;
    memset(&L, 0, sizeof(L));
    if (ok) L = make_dim_layout(in.NumDimsPerDimWidth);
    // every dimension column and the measure of rows [prev, prev + n) must be a pending sink
    ok = ok && match_queue(pq, in, L, length, &m) && m.measureJob >= 0 &&
         measure_job_matches(pq.jobs.s[m.measureJob], inValues + static_cast<size_t>(valueBytes) * m.prev, valueBytes, aggFunc);
    ok = ok && supported_agg_spec(aggFunc, valueBytes, hash_reduce_lds_supported, &a);
    ok = ok && plan_from_queue(plan, pq, L, m, valueBytes, 0, 0);
    // the precompiled generic scan holds nd + 2 column slots; a narrow plan only ever runs on generated kernels (kFusedCols)
    ok = ok && (plan.numCols <= nd + 2 || fused_plan_narrow(plan, nd));
    if (!ok) {  // the ordinary path: the pending work runs now, ahead of this call on the same stream
      launch_queue(stream, pq, /*inOrder=*/true);
      g_releaseHeld(device, hold_tag(stream));
      if (scan_stash_take(device, stream)) scan_stash_settled(device, stream, kScanAheadDiscardPlan);  // (a scan launched at the filter goes unread)
      return false;
    }
    take_queue(pq, q);
  }
  DimensionVector prevKeys = in;
  // (the batch's scan as its last filter launched it from a hint, if it did: the run takes it for its own or drops it)
  const int result = fused_hash_reduce_run(device, plan, m.n0, prevKeys, inValues, m.prev, out, outValues, a, stream, scan_stash_take(device, stream));
  DeferLock lock(device);
  if (result < 0) {  // a partition region overflowed, or the call was declined: materialise the inputs after all
    launch_queue(stream, q, /*inOrder=*/true);
    lock.unlock();
    g_releaseHeld(device, hold_tag(stream));
    return false;
  }
  t_state->limbo[stream] = q;  // launchable until the next batch begins (begin_batch)
  *groups = result;
  return true;
}

// ---- scan at filter: the hint (AresHintFusedBatch) ---------------------------------------------------------------------------
// The hinted plan is put together by the functions plan_from_queue uses, in its order, from the operands the batch's calls
// will bind: what HashReduce derives from the stream's queue and journal is then equal field for field (fused_plan_equal)
// whenever the calls arrive as hinted.  Anything that does not fit declines the hint: nothing is launched from it.
namespace {
// the operand of one hinted expression as the call that carries it will see it (run_transform / run_filter); false: not the hot shape
bool hinted_operands(const AresFusedExpr &e, bool compareOnly, int batchRows, hipStream_t stream, FastOperands &f) {
  if (e.arity != 1 && e.arity != 2) return false;
  if (e.lhs.Type != VectorPartyInput || (e.arity == 2 && e.rhs.Type != ConstantInput)) return false;
  if (static_cast<int64_t>(e.lhs.Vector.VP.Length) < batchRows) return false;  // (no speculative read may leave an allocation)
  InputVector ins[2] = {e.lhs, e.arity == 2 ? e.rhs : e.lhs};
  EvalParams p;
  CallTemps temps;
  build_params(ins, e.arity, stream, nullptr, nullptr, 0, e.functor, p, temps);
  return p.a.length >= static_cast<uint32_t>(batchRows) && fast_operands(p, f, compareOnly) && f.step == 4;
}
bool hint_fused_batch(int device, hipStream_t stream, const AresFusedQuery &q, int batchRows, int prevSize, int measureBytes) {
  if (!fuse_available() || !row_space_enabled() || !scan_at_filter_enabled()) return false;
  if (q.numDims < 1 || q.numDims > kGenericFusedDims || q.numFilters < 1 || q.numFilters > kExtensionFilters) return false;
  if (batchRows <= 0 || prevSize < 0 || static_cast<int64_t>(batchRows) + prevSize > INT32_MAX) return false;
  if (measureBytes != 4 && measureBytes != 8) return false;
  const int mt = q.measure.outType;
  if (!(mt == Int32 || mt == Uint32 || mt == Float32 || mt == Int64 || mt == Float64) || measureBytes != ((mt == Int64 || mt == Float64) ? 8 : 4))
    return false;
  AggSpec a;
  if (!supported_agg_spec(q.aggFunc, measureBytes, hash_reduce_lds_supported, &a)) return false;
  ScanHint h;
  memset(&h, 0, sizeof(h));
  const int nd = q.numDims;
  h.nd = nd;
  h.batchRows = batchRows;
  h.prevSize = prevSize;
  auto note = [&](const FastOperands &f) {
    column_ranges(f, static_cast<uint32_t>(batchRows), [&](const ByteRange &c) { h.ranges[h.numRanges++] = ScanHint::Range{c.lo, c.hi}; });
  };
  SinkD sink;
  FastOperands f;
  for (int d = 0; d < nd; d++) {
    const int t = q.dims[d].outType;
    if (!(t == Int32 || t == Uint32 || t == Float32) || !hinted_operands(q.dims[d], false, batchRows, stream, f)) return false;
    memset(&sink, 0, sizeof(sink));
    sink.type = SINK_DIM;
    sink.dtype = t;
    sink.width = 4;
    fused_plan_dim(h.plan, d, f, sink, 4);
    note(f);
  }
  if (!hinted_operands(q.measure, false, batchRows, stream, f)) return false;
  memset(&sink, 0, sizeof(sink));
  sink.type = SINK_MEASURE;
  sink.dtype = mt;
  sink.width = measureBytes;
  sink.agg = q.aggFunc;
  sink.identity = identity_bits(q.aggFunc, mt);
  if (sink.agg == AGGR_AVG_FLOAT || (measureBytes == 8 && sink.identity != 0)) return false;
  fused_plan_measure(h.plan, nd, f, sink, measureBytes);
  note(f);
  for (int k = 0; k < q.numFilters; k++) {
    if (!hinted_operands(q.filters[k], true, batchRows, stream, f)) return false;
    f.idx = nullptr;  // (as the journal keeps them)
    h.filters[k] = f;
    note(f);
  }
  if (!fused_plan_filters(h.plan, h.filters, static_cast<size_t>(q.numFilters))) return false;
  if (h.plan.numCols > nd + 2 || fused_plan_narrow(h.plan, nd)) return false;
  scan_hint_set(device, stream, h);
  return true;
}
}  // namespace

// ---- Sort + Reduce over pending transforms (sort_reduce_fused.hip) ---------------------------------------------------------
namespace {
bool same_vector(const DimensionVector &a, const DimensionVector &b) {
  return a.DimValues == b.DimValues && a.HashValues == b.HashValues && a.IndexVector == b.IndexVector && a.VectorCapacity == b.VectorCapacity &&
         memcmp(a.NumDimsPerDimWidth, b.NumDimsPerDimWidth, sizeof(a.NumDimsPerDimWidth)) == 0;
}
}  // namespace

// caller holds the device's DeferLock: [at, at + bytes) is from now on what the lazily defined Sort (+ Reduce) `ps` would
// write there — lazy fills under it retire, a marker among the fills takes their place
static void mark_sort_output(const PendingSort &ps, void *at, size_t bytes, int unit) {
  uint8_t *p = static_cast<uint8_t *>(at);
  retire_fills(range_of(p, bytes), false);
  t_state->fills[p] = PendingFill{ps.stream, bytes, 0, unit, false, ps.keys.IndexVector};
}
// caller holds the device's DeferLock: Sort(ps.keys, ps.length) is defined, not run — the hash vector becomes a marker, the
// index vector's iota entry `io` "what Sort leaves" (nobody takes it for an iota any more, only its own readers write it)
// (`io` lives in t_state->iotas, and retire_fills below may run drop_sort / materialize_sort over OTHER definitions: they erase
// an iota entry only where it is `sorted` and its own sort is entered — `io` is neither until the lines after the call, so the
// reference holds.  The flags are therefore set last.)
static void define_sort(const PendingSort &ps, PendingIota &io) {
  mark_sort_output(ps, ps.keys.HashValues, 8ull * static_cast<size_t>(ps.length), 8);
  t_state->sorts[ps.keys.IndexVector] = ps;
  io.consumed = true;
  io.sorted = true;
}

// caller holds the device's DeferLock.  A lazily defined Sort has been consumed by a Reduce whose kernels wrote `result` groups:
// the hash vector, the input's index vector and the output's index vector stay DEFINED (what Sort and Reduce would have left
// there); whoever reads them replays the sequence (materialize_sort)
static void enter_reduced_sort(hipStream_t stream, PendingSort ps, const DimensionVector &in, uint8_t *inValues,
                               const DimensionVector &out, uint8_t *outValues, int valueBytes, int length, int aggFunc, int result) {
  ps.reduced = true;
  ps.outKeys = out;
  ps.inValues = inValues;
  ps.outValues = outValues;
  ps.valueBytes = valueBytes;
  ps.aggFunc = aggFunc;
  ps.groups = result;
  // (ps is the definition this Reduce consumed: ps.keys is `in`, ps.length is `length`, ps.stream is `stream`)
  define_sort(ps, t_state->iotas[in.IndexVector] = PendingIota{stream, 0, length});
  if (result > 0) mark_sort_output(ps, out.IndexVector, 4ull * static_cast<size_t>(result), 4);
}

// Sort(keys, length) when the rows [length - n, length) of `keys` are what this stream's pending transforms would write and
// the index vector is still the iota InitIndexVector defined: nothing is hashed or sorted — the hash vector (a marker among
// the lazy fills) and the index vector (its iota entry, `sorted`) are DEFINED as what Sort leaves.  Reduce consumes the
// definition (below); every other reader runs it (materialize_sort).
bool define_lazy_sort(int device, hipStream_t stream, const DimensionVector &keys, int length) {
  if (!fuse_available() || !fused_sort_reduce_enabled() || length <= 0 || !keys.DimValues || !keys.HashValues || !keys.IndexVector ||
      keys.VectorCapacity < length)
    return false;
  DimLayoutD L;
  try {
    L = make_dim_layout(keys.NumDimsPerDimWidth);
  } catch (std::exception &) {
    return false;
  }
  DeferLock lock(device);
  PendingIota *io = lazy_iota(keys.IndexVector, length);
  if (!io || io->consumed) return false;
  auto it = t_state->pending.find(stream);
  if (it == t_state->pending.end() || it->second.jobs.count == 0) return false;
  QueueMatch m;
  if (!match_queue(it->second, keys, L, length, &m)) return false;  // (the survivors must be re-derivable from the filter journal)
  PendingSort ps{};
  ps.stream = stream;
  ps.keys = keys;
  ps.length = length;
  define_sort(ps, *io);
  return true;
}

// ---- Sort + Reduce over materialised vectors -----------------------------------------------------------------------------
// The batch's dimension rows were written by kernels (a joined column, a generic expression, an eager host): Sort still need
// not order ROWS for Reduce to order GROUPS (fused_sort_reduce_vectors).  Sort asks before its flush (the index vector's lazy
// iota is marked consumed: the flush does not write it) ...
namespace {
bool vector_sort_enabled() {
  static EnvSwitch<bool> on("ARES_SORT_VECTORS", [](const char *e) { return !(e && e[0] == '0'); });
  return on.get();
}
// (the predicate fused_sort_reduce_vectors declines by: Sort is never defined for a layout Reduce would turn away)
bool vector_sort_layout(const DimensionVector &keys) { return sort_vector_layout_supported(keys.NumDimsPerDimWidth); }
}  // namespace

bool lazy_vector_sort_candidate(int device, const DimensionVector &keys, int length) {
  const bool trace = hr_trace_enabled();  // diagnostics
  if (trace)
    fprintf(stderr, "lazy_vector_sort_candidate: rows %d fuse %d enabled %d switch %d layout %d capacity %d\n", length, fuse_available() ? 1 : 0,
            fused_sort_reduce_enabled() ? 1 : 0, vector_sort_enabled() ? 1 : 0, vector_sort_layout(keys) ? 1 : 0, keys.VectorCapacity);
  if (!fuse_available() || !fused_sort_reduce_enabled() || !vector_sort_enabled() || length <= 0 || !keys.DimValues || !keys.HashValues ||
      !keys.IndexVector || keys.VectorCapacity < length || !vector_sort_layout(keys))
    return false;
  DeferLock lock(device);
  PendingIota *io = lazy_iota(keys.IndexVector, length);
  if (!io || io->consumed) {
    if (trace)
      fprintf(stderr, "lazy_vector_sort_candidate: index vector is %s\n", t_state->iotas.count(keys.IndexVector) ? "a lazy iota of another kind" : "not a lazy iota");
    return false;
  }
  io->consumed = true;
  return true;
}

// ... and defines itself after it (every pending writer of the rows has been launched).  false: the index vector is written,
// the caller sorts.
bool define_lazy_sort_vectors(int device, hipStream_t stream, const DimensionVector &keys, int length) {
  {
    DeferLock lock(device);
    PendingIota *io = lazy_iota(keys.IndexVector, length);
    if (io && io->consumed) {  // (lazy_vector_sort_candidate marked it)
      PendingSort ps{};
      ps.stream = stream;
      ps.keys = keys;
      ps.length = length;
      ps.fromVectors = true;
      define_sort(ps, *io);
      return true;
    }
  }
  materialize_index_vector(device, keys.IndexVector);
  return false;
}

// ---- Reduce over a lazily defined Sort: what the scan-fed and the vector-sourced attempt share ------------------------------
// The outputs are about to be rewritten: lazy work that targets them is retired or dropped.  Rows [0, readRows) of the input
// vectors are read by this call's kernels: whatever still only defines them is written (no flush: a scan-fed batch's own lazy
// compaction must stay lazy); readRows == 0: no previous result, nothing is read.
static void prepare_sort_reduce(int device, const DimensionVector &in, const uint8_t *inValues, const DimensionVector &out, uint8_t *outValues,
                                int valueBytes, int length, int readRows) {
  const size_t dimBytes = dim_vector_bytes(in);  // (the caller has checked: out's layout is in's, and its capacity holds `length` rows)
  retire_fills_for_write(device, outValues, static_cast<size_t>(valueBytes) * length);
  retire_fills_for_write(device, out.IndexVector, 4ull * static_cast<size_t>(length));
  grouped_note_write(device, out);
  grouped_note_write(device, outValues, static_cast<size_t>(valueBytes) * length);
  drop_skipped_outputs(device, out.DimValues, dimBytes, outValues, static_cast<size_t>(valueBytes) * length);
  if (readRows <= 0) return;
  launch_pending_writers(device, in.DimValues, dimBytes);
  launch_pending_writers(device, inValues, static_cast<size_t>(valueBytes) * readRows);
  materialize_fills_for_read(device, in.DimValues, dimBytes);
  materialize_fills_for_read(device, inValues, static_cast<size_t>(valueBytes) * readRows);
}
// The kernels wrote `result` groups: the reduced state is entered; `consumed` (scan-fed only) is the queue the scan evaluated —
// launchable until the next batch begins (begin_batch).  Returns true.
static bool reduced_sort_done(int device, hipStream_t stream, const PendingSort &ps, const DimensionVector &in, uint8_t *inValues,
                              const DimensionVector &out, uint8_t *outValues, int valueBytes, int length, int aggFunc, int result,
                              const PendingQueue *consumed, int *groups) {
  mem_note_dim_rows(device, out, 0, static_cast<size_t>(result));
  mem_note_write(device, outValues, static_cast<size_t>(valueBytes) * static_cast<size_t>(result));
  DeferLock lock(device);
  if (consumed) t_state->limbo[stream] = *consumed;
  enter_reduced_sort(stream, ps, in, inValues, out, outValues, valueBytes, length, aggFunc, result);
  *groups = result;
  return true;
}
// The real thing: InitIndexVector, Sort (the ordinary Reduce follows).  Returns false.
static bool sort_for_real(int device, hipStream_t stream, const DimensionVector &in, int length) {
  {
    DeferLock lock(device);
    launch_init_index(in.IndexVector, 0, length, stream);
  }
  sort_keys_now(in, length, stream);
  return false;
}

// Reduce over a Sort defined over materialised vectors.  Caller: fuse_pending_into_sort_reduce.
static bool reduce_lazy_vector_sort(int device, hipStream_t stream, const DimensionVector &in, uint8_t *inValues, const DimensionVector &out,
                                    uint8_t *outValues, int valueBytes, int length, int aggFunc, int *groups) {
  PendingSort ps{};
  AggSpec a{};
  {
    DeferLock lock(device);
    auto st = t_state->sorts.find(in.IndexVector);
    if (st == t_state->sorts.end()) return false;
    ps = st->second;
    bool ok = !ps.reduced && ps.fromVectors && ps.stream == stream && ps.length == length && same_vector(ps.keys, in) &&
              inValues && out.DimValues && out.IndexVector && outValues && out.VectorCapacity >= length && in.VectorCapacity >= length &&
              memcmp(out.NumDimsPerDimWidth, in.NumDimsPerDimWidth, sizeof(in.NumDimsPerDimWidth)) == 0 && (valueBytes == 4 || valueBytes == 8);
    ok = ok && supported_agg_spec(aggFunc, valueBytes, fused_sort_reduce_supported, &a);
    if (!ok) {
      materialize_sort(in.IndexVector);
      return false;
    }
    drop_sort(in.IndexVector);  // (while the kernels run nothing is defined; the reduced state is entered below)
  }
  // every row is read by this call's kernels
  prepare_sort_reduce(device, in, inValues, out, outValues, valueBytes, length, /*readRows=*/length);
  const int result = guarded_attempt("fused_sort_reduce_vectors", [&] { return fused_sort_reduce_vectors(device, length, in, inValues, out, outValues, a, stream); });
  if (result < 0) return sort_for_real(device, stream, in, length);  // declined (a kernel still being compiled, too many rows), or a table overflowed
  return reduced_sort_done(device, stream, ps, in, inValues, out, outValues, valueBytes, length, aggFunc, result, nullptr, groups);
}

bool fuse_pending_into_sort_reduce(int device, hipStream_t stream, const DimensionVector &in, uint8_t *inValues, const DimensionVector &out,
                                   uint8_t *outValues, int valueBytes, int length, int aggFunc, int *groups) {
  if (!fuse_available() || !in.IndexVector) return false;
  {
    bool vectors = false;
    {
      DeferLock lock(device);
      auto st = t_state->sorts.find(in.IndexVector);
      vectors = st != t_state->sorts.end() && st->second.fromVectors && !st->second.reduced;
    }
    if (vectors) return reduce_lazy_vector_sort(device, stream, in, inValues, out, outValues, valueBytes, length, aggFunc, groups);
  }
  PendingQueue q;
  FusedPlanD plan;
  memset(&plan, 0, sizeof(plan));
  PendingSort ps{};
  AggSpec a{};
  int nd = 0;
  QueueMatch m;
  bool constMeasure = false;
  uint64_t constBits = 0;
  PendingFill fill{};
  uint8_t *fillAt = nullptr;
  {
    DeferLock lock(device);
    auto st = t_state->sorts.find(in.IndexVector);
    if (st == t_state->sorts.end()) return false;  // nothing lazy about this Sort
    ps = st->second;
    bool ok = !ps.reduced && ps.stream == stream && ps.length == length && same_vector(ps.keys, in) && inValues &&
              out.DimValues && out.IndexVector && outValues && out.VectorCapacity >= length &&
              memcmp(out.NumDimsPerDimWidth, in.NumDimsPerDimWidth, sizeof(in.NumDimsPerDimWidth)) == 0;
    DimLayoutD L;
    memset(&L, 0, sizeof(L));
    if (ok) L = make_dim_layout(in.NumDimsPerDimWidth);
    nd = L.numDims;
    auto it = t_state->pending.find(stream);
    ok = ok && it != t_state->pending.end() && it->second.jobs.count > 0;
    ok = ok && match_queue(it->second, in, L, length, &m) && supported_agg_spec(aggFunc, valueBytes, fused_sort_reduce_supported, &a);
    if (ok) {
      const PendingQueue &pq = it->second;
      uint8_t *measureRows = inValues + static_cast<size_t>(valueBytes) * m.prev;
      if (m.measureJob >= 0) {
        ok = measure_job_matches(pq.jobs.s[m.measureJob], measureRows, valueBytes, aggFunc);
      } else {  // a constant measure (COUNT(*)): the rows are a lazy fill
        auto f = t_state->fills.find(measureRows);
        ok = f != t_state->fills.end() && !f->second.sortIdx && f->second.unit == valueBytes &&
             f->second.bytes == static_cast<size_t>(valueBytes) * pq.n;
        if (ok) {
          constMeasure = true;
          fill = f->second;
          fillAt = f->first;
          constBits = fill.pattern;
        }
      }
      const int constDtype = a.vtype == V_F64 ? Float64 : a.vtype == V_F32 ? Float32 : valueBytes == 8 ? Int64 : (a.vtype == V_I32 ? Int32 : Uint32);
      ok = ok && plan_from_queue(plan, pq, L, m, valueBytes, constBits, constDtype);
    }
    if (!ok) {  // not this case after all: Sort runs (and the ordinary Reduce follows)
      materialize_sort(in.IndexVector);
      return false;
    }
    take_queue(it->second, q);
    if (constMeasure) t_state->fills.erase(fillAt);
    drop_sort(in.IndexVector);  // (while the kernels run nothing is defined; the reduced state is entered below)
  }
  // the previous result — rows [0, prev) — is read by kernels of this call
  prepare_sort_reduce(device, in, inValues, out, outValues, valueBytes, length, /*readRows=*/m.prev);
  const int result = guarded_attempt("fused_sort_reduce_run", [&] {
    return fused_sort_reduce_run(device, plan, nd, constMeasure, constBits, m.n0, in, inValues, m.prev, out, outValues, a, stream);
  });
  if (result < 0) {  // declined, or a partition overflowed: the batch's rows are written — transforms, the constant rows — ...
    {
      DeferLock lock(device);
      launch_queue(stream, q, /*inOrder=*/true);
      if (constMeasure) launch_fill(fillAt, fill);
    }
    g_releaseHeld(device, hold_tag(stream));
    // ... and the groups are ordered by row hash over the rows that exist now (the wide layout takes results the 512 tables
    // of the scan-fed path do not: millions of groups per batch) ...
    int wide = kFusedUnavailable;
    if (vector_sort_enabled() && vector_sort_layout(in))
      wide = guarded_attempt("fused_sort_reduce_vectors", [&] { return fused_sort_reduce_vectors(device, length, in, inValues, out, outValues, a, stream); });
    if (wide >= 0) {
      ps.fromVectors = true;
      return reduced_sort_done(device, stream, ps, in, inValues, out, outValues, valueBytes, length, aggFunc, wide, nullptr, groups);
    }
    return sort_for_real(device, stream, in, length);  // ... or the real thing
  }
  q.sortIdx = in.IndexVector;
  ps.constMeasure = constMeasure;
  ps.fill = fill;
  ps.fillAt = fillAt;
  return reduced_sort_done(device, stream, ps, in, inValues, out, outValues, valueBytes, length, aggFunc, result, &q, groups);
}

}  // namespace ares

using namespace ares;

extern "C" {

void AresHintFusedBatch(const AresFusedQuery *query, int batchRows, int prevSize, int measureBytes, void *cudaStream, int device) {
  bool taken = false;
  try {  // (a hint has no result: whatever goes wrong with it, the batch runs as if it had not been given)
    taken = query != nullptr && device >= 0 && device < kMaxDevices &&
            hint_fused_batch(device, reinterpret_cast<hipStream_t>(cudaStream), *query, batchRows, prevSize, measureBytes);
  } catch (std::exception &) {
  }
  if (!taken) scan_ahead_count(kScanAheadDeclined);
}

void AresScanAtFilterStats(unsigned long long *counters) {
  if (counters) scan_ahead_stats(counters);
}

}  // extern "C"
