// The deferral state machine of InitIndexVector, Unary/BinaryTransform and Unary/BinaryFilter (host side): the state, its
// lock and the helpers that run under it.  This header is the contract between deferral.hip (the machine), deferral_hooks.hip
// (what libmem.so calls), fused_consumers.hip (HashReduce and Sort + Reduce reading a stream's pending work as a fused plan)
// and transform.hip (the calls).
//
// ---- the deferral state machine: what is held back, and the invariants that keep it unobservable ---------------------
// One DeferState per device, one mutex (DeferLock); nothing below synchronises a stream while it holds the lock (late
// launches that the host believes done are synchronised after the unlock: t_syncAfterUnlock).  The things a call may
// DEFINE instead of doing:
//   * pending[stream]             root transforms of the hot shape, one queue per stream, launched together
//                                 (transform_multi_kernel) or consumed by HashReduce's fused scan;
//   * limbo[stream]               a queue HashReduce consumed: its outputs were never written, it stays launchable until
//                                 the stream's next InitIndexVector (begin_batch) or until its outputs are freed;
//   * journals[index vector]      the hot-shape filters applied to the vector since InitIndexVector: what the fused scan
//                                 replays instead of reading the vector;
//   * compactions[index vector]   filters that were counted (row space: `todo`, survivor bits) or evaluated (predicate
//                                 bytes) but whose compaction of the vector has not run;
//   * iotas[index vector]         InitIndexVector recorded, not written ("virtual iota");
//   * fills[first byte]           a buffer defined as a repeated 4- / 8-byte pattern (constant measures, the hash vector
//                                 of a query without dimensions);
//   * (hash_reduce_lds.hip)       measure rows defined by a table image ("lazy values");
//   * expansions[stream]          run-length encoded (mode-3) columns of an archive batch, decoded ONCE per batch into a
//                                 stream temporary laid out like a mode-2 column; the hot-shape machinery below (row-space
//                                 filters, queued transforms, the fused scans) then reads the copy.  Every definition that
//                                 reads a copy keeps it alive (`keep`); the per-batch cache dies at the stream's next
//                                 InitIndexVector and whenever the source column is written or freed;
//   * sorts[index vector]         Sort over rows whose transforms are still pending: the hash vector (a marker entry of
//                                 `fills`) and the index vector (its `iotas` entry, marked `sorted`) are defined as "what
//                                 Sort would leave"; Reduce consumes the definition with the pending transforms
//                                 (sort_reduce_fused.hip) and leaves its own (`reduced`: the input's hash and index vector
//                                 and the output's index vector are what a replay — skipped transforms, Sort, Reduce —
//                                 would write: materialize_sort).
//   * frames[first byte]          a 4-byte scratch frame DEFINED as a constant chain over one column (FrameDef): an inner node
//                                 of the hot shape — `column (op) constant`, or `a defined frame (op) constant` — is recorded,
//                                 not launched, and nothing else that is pending is flushed for it.  A following BinaryTransform
//                                 `that frame (op) constant` composes: into a scratch sink a new definition, into a dimension or
//                                 measure sink an ordinary queued job whose reads are the COLUMN's (compose_frame).  The exits of
//                                 a definition, each one the only thing that happens to it there:
//                                   - composed: it stays (the frame may have other readers);
//                                   - written (materialize_frame: one transform_fast_kernel with the chain, on the defining stream,
//                                     ordered before the reader — I1): a transform or filter that is handed the frame and does not
//                                     compose (settle_frames_for_call), a copy (hook_on_access), an entry point that names the
//                                     bytes it reads (flush_deferred_for_inputs), an entry point that does not say what it reads
//                                     (ARES_ABI_BEGIN: materialize_all_frames), a filter or InitIndexVector over its index vector,
//                                     a write to its source column or index vector, a free of them the host has not waited for;
//                                   - retired without a launch: overwritten whole by a transform (a new definition included),
//                                     freed (hook_on_free), its stream destroyed (hook_on_stream_destroy) — I2 - I4;
//                                   - never launched by anything else: a flush from an unrelated call, launch_queue, a stream
//                                     wait (I6) — a source column freed after the host waited is held for it, as for a queue.
//                                 ARES_CHAINS=0 (or ARES_DEFER=0) defines none: every node runs the kernel it always ran.
// Invariants (each one is what a reader of device memory relies on; the sequence fuzzer reads every buffer at random
// points and the soak test does so from four threads):
//   I1  Before ANY byte of device memory is read by something other than the consumer a definition was made for — a copy
//       (hook_on_access), an entry point that is handed the buffer (flush_deferred_for_inputs / _for_vector,
//       settle_dimension_vector, launch_pending_writers) — every definition that covers the byte is written, in call order,
//       on the stream it was made on, and that stream is synchronised before the reader proceeds if the reader runs
//       elsewhere (order_before_caller).
//   I2  Before a byte is overwritten or freed, definitions inside the range are retired (retire_fills, drop_skipped_outputs,
//       hook_on_free); work that READS the range and is still pending keeps the block from being reused (libmem holds it
//       under the stream's tag until AresMemReleaseHeld) or is launched first (the free is fenced behind it).
//   I3  A definition never outlives what it refers to: stream destruction (hook_on_stream_destroy) drops the stream's
//       queues, journals, compactions and iotas, hands its fills to "whoever asks", settles its error words; events are
//       destroyed while their stream exists (ROCm 7: querying an event of a destroyed stream is a use after free).
//   I4  State keyed by a pointer (journals, compactions, iotas, fills) dies with the allocation: hook_on_free erases it, so
//       a recycled address never meets a stale entry.  State keyed by a stream dies with the stream (I3).
//   I5  Whatever a call decides under the lock it acts on under the SAME acquisition; a decision taken under an earlier
//       acquisition is re-validated (run_filter_rows re-checks the row-space eligibility its caller established: another
//       thread's flush may have applied the vector's pending filters in between — the round-5 soak finding).
//   I6  A flush from an unrelated call (another stream, another query) launches what is pending but leaves alone what
//       only its own consumer will ever read: limbo, consumed iotas, lazy fills, lazily defined measure rows (I1 covers
//       their readers), and compactions whose only reader is limbo work ("dormant").
// ARES_DEFER=0 switches all of it off (every call launches its own kernel); ARES_FUSE=0 the HashReduce stage.
#pragma once

#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "dim_layout.hpp"
#include "quad_geometry.hpp"

namespace ares {

struct ByteRange {
  const uint8_t *lo, *hi;
  bool overlaps(const ByteRange &o) const { return lo < o.hi && o.lo < hi; }
};
inline ByteRange range_of(const void *ptr, size_t bytes) {  // (a range of no bytes counts as its first byte)
  const uint8_t *lo = static_cast<const uint8_t *>(ptr);
  return ByteRange{lo, lo + (bytes ? bytes : 1)};
}
// the byte ranges a hot-shape operand's column occupies: visit(values) and, where the column has them, visit(validity bits)
template <typename Visit>
void column_ranges(const FastOperands &f, uint32_t colRows, Visit &&visit) {
  visit(range_of(f.vals, fast_value_bytes(f, colRows)));
  if (f.nulls) visit(range_of(f.nulls, (static_cast<uint64_t>(colRows) + f.bitOff + 7) / 8 + 2));
}
inline bool column_overlaps(const FastOperands &f, uint32_t colRows, const ByteRange &r) {
  bool hit = false;
  column_ranges(f, colRows, [&](const ByteRange &c) { hit = hit || c.overlaps(r); });
  return hit;
}
// one of the ranges `v` overlaps the operand's column
inline bool column_ranges_touch(const std::vector<ByteRange> &v, const FastOperands &f, uint32_t colRows) {
  for (const ByteRange &x : v)
    if (column_overlaps(f, colRows, x)) return true;
  return false;
}
inline bool touches(const std::vector<ByteRange> &v, const ByteRange &r) {
  for (const ByteRange &x : v)
    if (x.overlaps(r)) return true;
  return false;
}
// One stream's root transforms of the hot shape, held back to be launched together.  Contract and flush points:
// include/ares_extensions.h.  A queue holds jobs that share the index vector and length; a job whose buffers overlap a queued
// job's (read-after-write or write-after-anything) forces the queue out first, so the fused launch never reorders dependent work.
struct PendingQueue {
  MultiJobs jobs;
  uint32_t colRows[kMaxMultiJobs];  // rows of each job's source column
  const uint32_t *idx = nullptr;
  int n = 0;
  std::vector<ByteRange> reads, writes;
  // the host has waited for the stream since these jobs were queued (second-stage fusion,
  // include/ares_extensions.h): a late launch from outside the stream's own call order must
  // restore "the stream is idle" before anybody looks
  bool overWait = false;
  std::vector<std::shared_ptr<StreamBuffer>> keep;  // decoded copies of run-length columns the jobs read
  // (limbo only) the queue was consumed by a fused Sort + Reduce: whoever launches it replays the whole sequence
  const uint32_t *sortIdx = nullptr;
};
struct DeferState;
// The deferral state is per device: queries on different GPUs of one process never contend, and the
// work done under a device's mutex is bookkeeping and kernel launches only (synchronisations run after
// the unlock, see below).  DeferLock selects the state its holder works on; the helpers marked
// "caller holds the device's DeferLock" reach it through t_state.
extern thread_local DeferState *t_state;
// Stream synchronisations that work done under a DeferLock asks for (a queue the host has already
// waited for was launched late; a copy is about to read what a late launch writes): they run after
// the mutex is released, so one query's late launch never stalls the other streams of the device.
extern thread_local std::vector<hipStream_t> t_syncAfterUnlock;
struct DeferLock {
  std::unique_lock<std::mutex> lock;
  explicit DeferLock(int device);
  void release() {
    if (!lock.owns_lock()) return;
    t_state = nullptr;
    lock.unlock();
  }
  void unlock() {
    release();
    drain();
  }
  static void drain() {
    std::vector<hipStream_t> todo;
    todo.swap(t_syncAfterUnlock);
    for (size_t i = 0; i < todo.size(); i++) {
      bool seen = false;
      for (size_t j = 0; j < i; j++) seen = seen || todo[j] == todo[i];
      if (!seen) hip_check(hipStreamSynchronize(todo[i]), "hipStreamSynchronize");
    }
  }
  ~DeferLock() noexcept(false) {
    release();
    if (std::uncaught_exceptions() == 0) drain();
    else t_syncAfterUnlock.clear();
  }
};

// caller holds a DeferLock: something the calling entry point may read next was just launched on `producer`.  Kernels of
// the call run on the call's own stream: when that is another stream (or unknown: the call came from libmem.so), the
// producer is synchronised once the lock is released — before the caller launches anything.
void order_before_caller(hipStream_t producer);

// Filters of the hot shape that have compacted an index vector since its InitIndexVector: with them
// HashReduce can re-derive the survivors from the source columns instead of reading index, dimension
// and measure vectors.  Any other writer of the index vector invalidates the entry.
struct FilterJournal {
  hipStream_t stream;
  uint32_t start;
  int n0;
  bool valid;
  std::vector<FastOperands> filters;
  std::vector<uint32_t> colRows;
  std::vector<std::shared_ptr<StreamBuffer>> keep;  // decoded copies of run-length columns the filters read
  int lastCount = -1;  // survivors of the last journalled filter (-1: not known), what the next one must be called with
};

extern void (*g_releaseHeld)(int, uintptr_t);  // AresMemReleaseHeld of the sibling libmem.so
extern bool g_fuseEnabled;  // ARES_FUSE
// Blocks are held on behalf of ONE stream's pending work: the tag names that stream, so that one
// query's progress never releases what another query's not-yet-launched kernels still read.
inline uintptr_t hold_tag(hipStream_t stream) { return reinterpret_cast<uintptr_t>(stream) + 1; }
struct ReleaseSet {
  std::vector<uintptr_t> tags;
  void add(hipStream_t s) { tags.push_back(hold_tag(s)); }
  void run(int device) const {
    if (g_releaseHeld)
      for (uintptr_t t : tags) g_releaseHeld(device, t);
  }
};

// One filter that has been counted in row space (filter_rows_kernel) and not applied to the index vector yet.
struct LazyFilter {
  FastOperands f;     // idx = nullptr, pad = 0: the replay fills them in
  uint32_t colRows;   // rows of the column
  uint8_t *pred;      // the predicate vector the host passed with the call
  int rowsBefore;     // length of the index vector before this filter (= the previous filter's count)
  std::shared_ptr<StreamBuffer> keep;  // the decoded copy of a run-length column the filter reads (or null)
};
// A run-length encoded column decoded for the stream's current batch (expand_runs_kernel): what it was made from, and the copy
struct RunExpansion {
  const uint8_t *base;
  uint32_t nullsOff, valuesOff, length, bitOff, step, startCount;
  int rows;
  std::shared_ptr<StreamBuffer> copy;
  size_t valuesAt;  // byte offset of the values behind the validity bitmap
};
// What the next filter call of the stream is expected to be (the previous batch of the stream had the same filter on the
// same column right behind this one): evaluated in the same pass, handed out without a kernel when the call arrives.
struct PredictedFilter {
  bool valid = false;
  FastOperands g;     // on the column of the filter it was evaluated with
  int count = 0;
  std::shared_ptr<StreamBuffer> bits;
};
// The workspace of a two-phase compaction (tile counts, filter_scan_kernel, one filter_compact_kernel per pass), in one
// stream temporary of bytes() bytes:
//   [total, error, one ticket per pass, pad to 64 bytes][tile counts][tile offsets + 1][loaded x passes][extra words]
// pass 0 compacts the index vector, pass k the k-th RecordID vector; the extra words are the caller's.
struct CompactSpace {
  uint32_t *words = nullptr;
  int tiles = 0, passes = 1;
  static size_t bytes(int tiles, int passes, size_t extraWords) {
    return 64 + 4 * (static_cast<size_t>(tiles) * (2 + passes) + 1 + extraWords);
  }
  uint32_t *total() const { return words; }  // {survivors, error}: read back together
  uint32_t *error() const { return words + 1; }
  unsigned int *tickets() const { return words + 2; }
  uint32_t *tileCounts() const { return words + 16; }
  uint32_t *tileOffsets() const { return tileCounts() + tiles; }
  uint32_t *loaded() const { return tileOffsets() + tiles + 1; }
  uint32_t *extra() const { return loaded() + static_cast<size_t>(tiles) * passes; }
};
// A fast filter has written the predicate vector and returned the survivor count, but the compaction
// of its index vector has not run: when HashReduce re-derives the survivors from the filter journal
// nobody ever reads the compacted vector.  Whatever does read it (a second filter, transforms that
// are launched after all, a copy, any other entry point) runs the compaction first.
struct PendingCompact {
  hipStream_t stream;
  uint32_t *idx;
  const uint8_t *pred;
  int n, pad;
  bool virtualIdx;
  std::shared_ptr<StreamBuffer> ws;  // what `space` lies in
  CompactSpace space;                // tile counts filled in (filter_pred_kernel); their scan has not run yet
  // row-space form (todo not empty: the fields from `pred` to `space` are unused).  The index vector holds
  // iota(0 .. n0) — virtual or written — with the first `applied` filters of the journal applied; `todo` are the filters
  // counted since, in call order; `bits` the survivors after the last of them, in row space (one 16-bit word per lane and tile).
  std::vector<LazyFilter> todo;
  int n0 = 0, applied = 0, lastCount = 0;
  std::shared_ptr<StreamBuffer> bits;
  // The last of `todo` was counted by the batch's fused scan (scan at filter): counted, but NO survivor bits exist.  A null
  // `bits` otherwise means "no filter yet, every row alive", so a further filter must not be counted in row space over this
  // entry: it takes the replay (run_compaction, which re-evaluates from the operands) and the two-phase filter.
  bool noBits = false;
  PredictedFilter predicted;
  uint64_t generation = 0;  // of the filter that was booked last (DeferState::filterGeneration)
};

// Filters of the previous and of the current batch of a stream, by shape: what filter_rows_kernel's prediction goes by.
struct FilterShape {
  int akind, functor, I, bkind;
  uint32_t bbits, bok;
  bool sameColumnAsPrevious;
  bool same_as(const FilterShape &o) const {
    return akind == o.akind && functor == o.functor && I == o.I && bkind == o.bkind && bbits == o.bbits && bok == o.bok &&
           sameColumnAsPrevious == o.sameColumnAsPrevious;
  }
};
struct FilterHistory {
  std::vector<FilterShape> previous, current;
};

// Index vectors that InitIndexVector has defined but not written yet ("virtual iota"): the fast
// filter and transform kernels that consume them compute rows = position instead of loading 4 bytes
// per row; any other use (every flush point) materialises them first.
struct PendingIota {
  hipStream_t stream;
  uint32_t start;
  int n;
  // A consumer has already used the vector as what it is defined to be (Reduce over zero dimensions): only somebody
  // who is handed THIS vector, copies it or frees it still cares — unrelated flush points and stream waits leave it.
  bool consumed = false;
  // Sort has been DEFINED over this vector (DeferState::sorts): what it is defined to hold is the sorted order, not the iota
  bool sorted = false;
};

// Buffers that a call has defined as "`unit`-byte pattern, repeated" but that nobody has written yet ("lazy fill"):
// the measure vector a constant transform fills (COUNT(*) is SUM over a literal 1, query/aql_compiler.go:1191-1197),
// the hash vector Sort gives a query without dimensions (every row hashes alike).  A consumer that knows what the
// bytes would be (Reduce over zero dimensions) never makes anybody write them; every other reader, copy or flush
// point writes them first; a free or an overwrite retires them.
struct PendingFill {
  hipStream_t stream;
  size_t bytes;
  uint64_t pattern;
  int unit;  // 4 or 8
  bool streamGone = false;  // the defining stream was destroyed: written on the stream of whoever asks for it
  // not a pattern at all: a buffer a lazily defined Sort (+ Reduce) would write — the hash vector, the output's index vector.
  // Reading it runs the sort (materialize_sort), a free or a whole overwrite drops the definition (drop_sort)
  const uint32_t *sortIdx = nullptr;
};

// Sort over a dimension vector whose batch rows are still pending transforms (define_lazy_sort), and — once `reduced` —
// the Reduce that consumed it together with them (fuse_pending_into_sort_reduce)
struct PendingSort {
  hipStream_t stream;
  DimensionVector keys;
  int length;
  bool reduced = false;
  bool fromVectors = false;  // every row of `keys` exists (define_lazy_sort_vectors): no queue, no limbo — a replay is Sort [+ Reduce]
  // what a replay of the reduced state needs
  DimensionVector outKeys;
  uint8_t *inValues = nullptr, *outValues = nullptr;
  int valueBytes = 0, aggFunc = 0, groups = 0;
  bool constMeasure = false;  // the batch's measure rows were a lazy fill the Reduce consumed: `fill` at `fillAt`
  uint8_t *fillAt = nullptr;
  PendingFill fill;
};

// The error word of a lazily launched compaction (a bounded wait inside filter_compact_kernel timed
// out) cannot be read back where the launch happens — that may be inside a free or a copy.  It is
// copied to pinned memory behind the kernel and looked at by the following entry points of the
// device: the first one that finds it set reports the failure to the host.
// (The event lives no longer than its stream: hook_on_stream_destroy settles the checks of a stream that is going away.
// An event queried after its stream was destroyed is a use after free inside the ROCm 7.x runtime — see FenceEvent in
// mem/memory.hip.)
struct ErrorCheck {
  hipStream_t stream;
  hipEvent_t done;
  uint32_t *pinned;
  std::shared_ptr<StreamBuffer> ws;  // keeps the error word alive until the copy has run
};

// A 4-byte scratch frame defined as a constant chain over one column and not written (see `frames` above)
struct FrameDef {
  hipStream_t stream;
  FastOperands f;        // the column, the chain and — as its functor — the frame's own node: what a launch evaluates.  f.idx: the
                         // index vector a launch reads (null: rows = positions)
  SinkD s;               // the frame: values, validity bytes (values + nulls offset), dtype
  int n;                 // rows
  const uint32_t *idxVec;  // the index vector the defining call was handed (f.idx is null where it was a virtual iota)
  uint32_t colRows;      // rows of the source column
  std::shared_ptr<StreamBuffer> keep;  // the decoded copy of a run-length column the chain reads (or null)
  bool overWait = false;  // the host has waited for the stream since (hook_on_wait): a freed source block is held, not raced
  bool held = false;      // ... and one was
};

// Everything in here belongs to ONE device (`device`): entries are only ever made under a DeferLock of that device, so
// nothing below carries a device number of its own.
struct DeferState {
  std::mutex mutex;
  int device = -1;                               // set once, by state_of
  std::map<hipStream_t, PendingQueue> pending;  // root transforms queued per stream
  std::map<hipStream_t, PendingQueue> limbo;    // queues a HashReduce consumed on the fly
  std::map<const uint32_t *, FilterJournal> journals;
  std::map<const uint32_t *, PendingCompact> compactions;
  std::map<hipStream_t, FilterHistory> filterHistory;
  uint64_t filterGeneration = 0;
  std::map<uint32_t *, PendingIota> iotas;
  std::map<uint8_t *, PendingFill> fills;  // by first byte; ranges never overlap
  std::map<const uint32_t *, PendingSort> sorts;  // by index vector
  std::map<hipStream_t, std::vector<RunExpansion>> expansions;  // decoded run-length columns of the stream's batch
  std::map<uint8_t *, FrameDef> frames;  // scratch frames defined as constant chains, by first byte; ranges never overlap
  std::vector<ErrorCheck> errorChecks;
  std::vector<uint32_t *> errorSlots;  // recycled pinned words
  bool errorSeen = false;              // a check that was settled outside an entry point failed: the next poll reports it
};
constexpr int kMaxDevices = 64;

// what a dimension vector's rows occupy: every slot of every row of its capacity
inline size_t dim_vector_bytes(const DimensionVector &v) {
  return dim_row_bytes(v.NumDimsPerDimWidth) * static_cast<size_t>(v.VectorCapacity > 0 ? v.VectorCapacity : 0);
}
// erases every entry `dead` says so of.  (Not for actions that erase OTHER entries: those loops restart from begin().)
template <typename Map, typename Dead>
void erase_if(Map &m, Dead &&dead) {
  for (auto it = m.begin(); it != m.end();) it = dead(*it) ? m.erase(it) : std::next(it);
}

// ---- deferral.hip ---------------------------------------------------------------------------------------------------------
// false = deferral is off for this process (ARES_DEFER=0, or no sibling libmem.so) / its second stage is (ARES_FUSE=0)
bool defer_available();
bool fuse_available();
// The helpers below say "caller holds the device's DeferLock" where they are defined: they reach the state through t_state.
bool retire_error_check(size_t i);
void launch_queue(hipStream_t stream, PendingQueue &q, bool inOrder = false);
bool materialize_limbo(const ByteRange *range, ReleaseSet *released);
std::map<hipStream_t, PendingQueue>::iterator drop_limbo(std::map<hipStream_t, PendingQueue>::iterator it, ReleaseSet *released);
void launch_init_index(uint32_t *indexVector, uint32_t start, int n, hipStream_t stream);
PendingIota *lazy_iota(const uint32_t *indexVector, int n);
std::map<uint32_t *, PendingIota>::iterator write_iota(std::map<uint32_t *, PendingIota>::iterator it);
void launch_fill(uint8_t *dst, const PendingFill &f);
void materialize_fills(const ByteRange *r, std::vector<hipStream_t> *touched = nullptr);
void retire_fills(const ByteRange &r, bool gone);
bool sort_touches(const PendingSort &s, const ByteRange &r);
void drop_sort(const uint32_t *indexVector);
void materialize_sort(const uint32_t *indexVector);
void run_compaction(const uint32_t *idx);
bool compaction_touches(const PendingCompact &c, const ByteRange &r);
void forget_run_expansions(const ByteRange &r);
void journal_count(const uint32_t *indexVector, int count);
// scratch frames defined as constant chains (caller holds the device's DeferLock)
bool frame_writes_touch(const FrameDef &d, const ByteRange &r);  // the frame's own bytes
bool frame_reads_touch(const FrameDef &d, const ByteRange &r);   // its source column, its index vector
std::map<uint8_t *, FrameDef>::iterator materialize_frame(std::map<uint8_t *, FrameDef>::iterator it);
void materialize_frames(const ByteRange *r, bool readsToo);  // those whose bytes (readsToo: or sources) overlap r; null: all
void materialize_frames_of_index(const uint32_t *indexVector);
void settle_frames_for_write(const ByteRange &r);  // inside r: retired; cut by r, or reading r: written first
// ... and what transform.hip's calls use; these take the lock themselves where they need it
void flush_deferred_impl(int device, const ByteRange *limboA, const ByteRange *limboB, const uint32_t *exempt = nullptr);
bool chains_enabled();  // ARES_CHAINS (on unless 0) and deferral with its hooks
void begin_batch(int device, hipStream_t stream, const uint32_t *indexVector, uint32_t start, int n);
void journal_filter(int device, const uint32_t *indexVector, const FastOperands *f, uint32_t colRows, int rowsBefore,
                    std::shared_ptr<StreamBuffer> keep = nullptr);
bool journal_is_valid(int device, const uint32_t *indexVector);
bool defer_iota(int device, hipStream_t stream, uint32_t *indexVector, uint32_t start, int n);
bool virtual_iota(int device, uint32_t *indexVector, int n, bool take);
// the launch wrappers of deferral_kernels.hpp's kernels that a call runs eagerly as well (no lock needed)
constexpr int kPredGridCap = 256 * 16;  // workgroups of filter_pred_kernel at most: one partial count each
void launch_fast_transform(FastOperands f, const SinkD &s, int n, hipStream_t stream);
int pred_tiles(int n, int pad);
CompactSpace clear_compact_space(const StreamBuffer &ws, int tiles, int passes, size_t extraWords, hipStream_t stream);
void launch_filter_pred(const FastOperands &f, uint8_t *pred, const CompactSpace &cs, int n, uint32_t *blockTotals, hipStream_t stream);
void launch_compaction(const CompactSpace &cs, const uint8_t *pred, uint32_t *idx, bool virtualIdx, RecordID **recordIDVectors, int pad, int n,
                       hipStream_t stream);
int read_compaction_total(const CompactSpace &cs, hipStream_t stream);
// ---- transform.hip: ARES_FILTER_ROWSPACE ----------------------------------------------------------------------------------
bool row_space_enabled();
// ---- deferral_hooks.hip: what defer_available registers with libmem.so ----------------------------------------------------
void hook_on_wait(int device, void *stream);
uintptr_t hook_on_free(int device, void *ptr, size_t bytes);
void hook_on_access(int device, const void *ptr, size_t bytes);
void hook_on_write(int device, const void *ptr, size_t bytes);
void hook_on_stream_destroy(int device, void *stream);
void hook_trim(int device);
}  // namespace ares
