/* ares_extensions.h — entry points of the MI355X libalgorithm.so that are NOT part of the
 * reference ABI.  A host that only knows query/time_series_aggregate.h never needs them.
 */
#ifndef ARES_EXTENSIONS_H_
#define ARES_EXTENSIONS_H_

#include <stddef.h>
#include <stdint.h>

#include "ares_algorithm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-kernel timing with HIP events recorded on each launch's own stream.  Enable(1) clears the
 * log and starts recording, Enable(0) stops.  Report() resolves the events (the caller has already
 * synchronised its streams) and writes one "kernel launches total_ms" line per kernel name into
 * buf; it returns the buffer size needed.  The Go host's counterpart is the per-stage wall timing
 * of query/stats.go:160-169, which must synchronise the stream after every stage instead. */
void AresProfilerEnable(int on);
size_t AresProfilerReport(char *buf, size_t len);

/* Behaviour switches of libalgorithm.so that are read from the environment (ARES_HASH_REDUCE=global,
 * ARES_GROUPED=0, ARES_LEAN_MIN_GROUPS=n) are parsed once and kept; AresReloadEnv() makes every one of them
 * read its variable again on next use.  For tests that flip a switch inside one process. */
void AresReloadEnv(void);

/* The scan and merge kernels of a high- or low-cardinality HashReduce are compiled for the query's SHAPE at run time
 * (hiprtc; comparison and + - x constants are kernel arguments, so a new time range reuses the kernel) on a background
 * thread — a query never waits for the compiler, it runs the generic kernels until its kernels are loaded.
 * AresRtcWait() blocks until nothing is being compiled and returns the number of kernels in the cache; counters
 * (may be NULL) receives {hiprtc compilations, code objects loaded from the on-disk cache, kernels evicted}.
 * Environment: ARES_RTC=0 (off), ARES_RTC_ASYNC=0 (compile on the calling thread), ARES_RTC_CACHE_DIR (on-disk
 * cache of code objects; default ~/.cache/aresdb_amd/rtc; "off" disables), ARES_RTC_CACHE_ENTRIES (default 256). */
size_t AresRtcWait(long *counters);

/* Cross-call fusion inside the unchanged ABI.  Root transforms of the hot shape (a 4-byte column,
 * optionally combined with a constant, written to a dimension vector or a measure vector) are not
 * launched one by one: libalgorithm.so keeps up to 8 of them per (device, stream) and runs them as
 * ONE kernel that reads the index vector once.  Nothing observable changes: every other
 * libalgorithm.so entry point, and every libmem.so entry point through which the host could read,
 * overwrite or free device memory (WaitForCudaStream, AsyncCopy*, DeviceFree, DestroyCudaStream,
 * CudaProfilerStop), first launches what is pending.  libalgorithm.so finds the sibling libmem.so
 * (same directory) at run time and registers AresFlushDeferred through AresMemSetFlushHook; when
 * that is not possible (another allocator library in use) or ARES_DEFER=0 is set, every transform
 * is launched immediately as before. */
void AresFlushDeferred(int device);                      /* exported by libalgorithm.so */
void AresMemSetFlushHook(void (*hook)(int device));      /* exported by libmem.so */

/* Cross-call fusion, second stage: the pending dimension / measure transforms of a batch are never
 * launched when the HashReduce call that follows can evaluate them on the fly (the kernels of
 * AresFusedFilterHashReduce below): the dimension and measure vectors of the batch's rows are then
 * neither written nor read.  For that the pending work must survive the two things the Go host does
 * between project() and reduce() (query/aql_batchexecutor.go:213-216): WaitForCudaStream, and
 * DeviceFree of the batch's columns and of the index vector.  libmem.so therefore reports those
 * events instead of flushing blindly:
 *   on_wait   — the host waits for `stream`; libalgorithm.so keeps work pending only if nothing but
 *               a later libalgorithm.so call can observe its results;
 *   on_free   — returns a non-zero tag (it names the stream whose work it is) when not-yet-launched work
 *               still reads the block: libmem.so keeps the block aside (not reusable) until
 *               AresMemReleaseHeld is called with that tag; frees of a pending OUTPUT launch the work
 *               first;
 *   on_access — a copy is about to touch [ptr, ptr + bytes): work whose inputs or outputs overlap
 *               is launched first (also work that HashReduce had skipped: the skipped transforms
 *               stay launchable until the next batch begins);
 *   flush     — everything pending on the device is launched (all other entry points).
 * A HashReduce that cannot use the pending work as it is (other aggregate, layout, joins, ...) simply
 * launches it and proceeds as before.  ARES_FUSE=0 switches this stage off, ARES_DEFER=0 both.
 * The same bookkeeping lets a fast filter return its survivor count without compacting the index
 * vector yet (the predicate vector is written): the compaction runs as soon as anything reads the
 * vector — a second filter, transforms that are launched after all, a copy, any other entry point —
 * and never when HashReduce re-derives the survivors itself.  ARES_LAZY_COMPACT=0 compacts at once.
 *
 * Constant chains.  An INNER node of the hot shape — BinaryTransform(column, constant) or BinaryTransform(such a scratch
 * frame, constant) over integer kinds with Plus, Minus, Multiply, Divide, Mod or Floor, into a 4-byte Int32 / Uint32 scratch
 * frame, no base counts — is recorded, not launched, and flushes nothing (the time dimensions of query/time_bucketizer.go:
 * Floor(Plus(ts, off), b), Floor(Mod(ts, 86400), 3600), ... up to four nodes).  The root node over such a frame becomes an
 * ordinary pending transform that reads the COLUMN, so the batch's queue — and the HashReduce / Sort + Reduce that consumes it —
 * stays intact.  Flush points of a defined frame (it is written by one kernel, on its stream, before the reader proceeds):
 *   - a Transform / Filter call that is handed the frame and does not compose (two-column nodes, unary functors, float
 *     constants, a fifth node), HashLookup and every other entry point that does not name the bytes it reads;
 *   - on_access over the frame, over its source column or its index vector; a filter or InitIndexVector over its index vector;
 *   - on_free of its source column or index vector before the host has waited for the stream (after a wait the block is held).
 * It is NOT a flush point for a frame: WaitForCudaStream, an unrelated call's flush, the launch of the stream's queue.  A frame
 * that is overwritten whole, freed, or whose stream is destroyed is dropped unwritten.  ARES_CHAINS=0 switches chains off. */
typedef struct {
  void (*flush)(int device);
  void (*on_wait)(int device, void *stream);
  uintptr_t (*on_free)(int device, void *ptr, size_t bytes);
  void (*on_access)(int device, const void *ptr, size_t bytes);
} AresDeferralHooks;
void AresMemSetDeferralHooks(const AresDeferralHooks *hooks); /* exported by libmem.so */
void AresMemReleaseHeld(int device, uintptr_t tag);           /* exported by libmem.so; tag 0 = every held block */

/* Further notifications from libmem.so to libalgorithm.so (optional; `size` = sizeof of the caller's
 * struct, members past it are taken as absent):
 *   on_write          — a copy / memset is about to WRITE [ptr, ptr + bytes) (on_access is called as
 *                       well): results whose layout libalgorithm.so remembers (partition-grouped
 *                       HashReduce outputs) are no longer trusted;
 *   on_stream_destroy — DestroyCudaStream, after the stream has been synchronised: per-stream caches
 *                       and bookkeeping of libalgorithm.so are released;
 *   trim              — libmem.so could not allocate: libalgorithm.so gives its cached temporaries back.
 * AresMemTrimCache is the opposite direction: libalgorithm.so could not allocate, libmem.so releases its
 * parked blocks of the device. */
typedef struct {
  size_t size;
  void (*on_write)(int device, const void *ptr, size_t bytes);
  void (*on_stream_destroy)(int device, void *stream);
  void (*trim)(int device);
} AresMemAuxHooks;
void AresMemSetAuxHooks(const AresMemAuxHooks *hooks); /* exported by libmem.so */
void AresMemTrimCache(int device);                     /* exported by libmem.so */
/* Write tracking.  DeviceAllocate hands out cleared memory; libmem.so clears a block when it is freed, and
 * only the byte ranges written since the block was last cleared.  libmem.so sees its own copies and fills;
 * libalgorithm.so reports the outputs of its kernels with AresMemNoteWrite and switches tracking on with
 * AresMemEnableWriteTracking (never called: a freed block counts as written all over).  A host component
 * that lets anything else write into DeviceAllocate memory (a collective library receiving into it) reports
 * those writes with AresMemNoteWrite too. */
void AresMemNoteWrite(int device, const void *ptr, size_t bytes);
void AresMemEnableWriteTracking(void);

/* Shared fences.  DeviceFree fences a block with one event per stream; frees that follow one another with NOTHING submitted
 * to the device in between (the Go host frees a batch's columns, index and predicate vector in a row) share the events of
 * the first.  "Nothing submitted" must be known: libalgorithm.so reports every entry point and every kernel launch with
 * AresMemNoteActivity and switches sharing on with AresMemEnableActivityTracking (never called: every free records its
 * own events).  A host component that submits work to the query's streams itself (the driver's RCCL calls) reports it
 * the same way. */
void AresMemNoteActivity(void);
void AresMemEnableActivityTracking(void);

/* Books of libmem.so for one device: bytes / number of blocks the host holds (DeviceAllocate, deviceMalloc;
 * held blocks were freed by the host but are kept aside for deferred work and are NOT counted as live),
 * blocks kept aside, bytes parked in the cache.  Any pointer may be NULL. */
void AresMemStats(int device, size_t *liveBytes, size_t *liveBlocks, size_t *heldBlocks, size_t *parkedBytes);
/* Driver calls libmem.so's block cache could not avoid on `device` since the process started (hipMalloc, hipFree,
 * cache trims): after warm-up a steady workload adds none.  Any pointer may be NULL. */
void AresMemDriverCalls(int device, size_t *mallocs, size_t *frees, size_t *trims);
/* Events of the block cache (fences of parked blocks, recycled events) whose last record was on `stream`.  An event must
 * not be touched once its stream is destroyed (the ROCm 7.x runtime reaches into the stream object: use after free), so
 * DestroyCudaStream retires them while the stream exists: 0 right after it, for tests. */
size_t AresMemStreamEvents(int device, void *stream);
/* the same for libalgorithm.so: error-word watches of lazily launched compactions and unresolved profiler events */
size_t AresStreamEvents(int device, void *stream);
/* libalgorithm.so's stream temporaries (workspaces, decoded run-length columns, row hashes kept beside results): bytes handed
 * out and not yet released, and bytes sitting in its cache.  A steady workload keeps the first bounded (tests: nothing may
 * pile up batch after batch).  Either pointer may be NULL. */
void AresTempStats(size_t *handedOutBytes, size_t *cachedBytes);

/* HyperLogLog folds a large batch's (dimension row, register) pairs in LDS before it sorts: the radix sort and the run
 * reduce then see the entries that survive, not the rows (algo/hll.hip; the result is the same bit for bit).  Switches, all
 * obeying AresReloadEnv: ARES_HLL_PREAGG=0 sorts rows always, =1 pre-aggregates every batch that qualifies, unset does so
 * too but lets a device sort rows for 15 batches after one whose record streams overflowed (a few hot keys) or whose
 * survivors exceeded 3/4 of its rows; ARES_HLL_PREAGG_MIN_ROWS (default 1048576) is the smallest batch that takes the
 * stage; ARES_HLL_PREAGG_TABLE_KEYS (tests; <= 5120) is the number of keys after which a partition's table is emitted.
 * counters receives {batches pre-aggregated, batches that declined after the scan, rows of the former, their surviving
 * entries} since the process started. */
void AresHllPreaggStats(unsigned long long *counters);

/* Fused batch execution: filter -> dimension / measure projection -> hash reduction of ONE batch in
 * a single pass over the source columns, without the index / predicate / dimension vectors the
 * one-call-per-AST-node ABI materialises in between (~145 B/row of HBM traffic on
 * BASELINE config C3; this path moves ~53 B/row).  It replaces, for one batch, the call sequence
 *   InitIndexVector, BinaryFilter x numFilters, Unary/BinaryTransform x (numDims + 1), HashReduce
 * of query/aql_batchexecutor.go:103-273 and produces the same groups and aggregates.
 *
 * Shapes accepted (anything else returns an error string starting with "not fusable", and the host
 * simply runs the ordinary sequence): every expression is a main-table VectorPartyInput of a
 * 4-byte type (modes 1/2), bare (arity 1, Noop) or combined with a ConstantInput by a binary
 * functor (arity 2); filters are comparison functors (ANDed); dimensions are stored as
 * Int32 / Uint32 / Float32; the aggregate is one HashReduce supports with native LDS atomics.
 * prevKeys / prevValues hold the prevSize groups accumulated so far (the reference keeps them as the
 * first rows of the input vectors, query/aql_processor.go:752-774); outKeys.VectorCapacity must be
 * at least prevSize + batchRows.  res = number of groups written to outKeys / outValues. */
typedef struct {
  InputVector lhs, rhs; /* rhs is read only when arity == 2 */
  int arity;
  int functor; /* Unary/BinaryFunctorType */
  enum DataType outType;
} AresFusedExpr;

typedef struct {
  int numFilters;
  AresFusedExpr filters[4];
  int numDims;
  AresFusedExpr dims[4];
  AresFusedExpr measure; /* outType = data type of the measure vector */
  enum AggregateFunction aggFunc;
} AresFusedQuery;

CGoCallResHandle AresFusedFilterHashReduce(const AresFusedQuery *query, int batchRows, DimensionVector prevKeys,
                                           uint8_t *prevValues, int prevSize, DimensionVector outKeys,
                                           uint8_t *outValues, void *cudaStream, int device);

/* Scan at filter: a HINT for hosts that keep the one-call-per-node sequence.  Called before a batch's filters (after the
 * batch's columns are in place, before or after InitIndexVector's buffers exist: no buffer of the sequence is named) it says
 * what the stream's next
 *   InitIndexVector, BinaryFilter x numFilters, Unary/BinaryTransform x (numDims + 1), HashReduce
 * sequence will be: `query` as AresFusedFilterHashReduce takes it, bound to THIS batch's columns; batchRows; prevSize = the
 * query's current result size; measureBytes = the width of the measure vector (4 or 8).  When the sequence then arrives as
 * hinted, its last filter is counted by the batch's fused scan itself, launched in the filter kernel's place — the scan
 * evaluates the filters per row anyway — and HashReduce merges what that scan wrote instead of scanning: one kernel and one
 * pass over the last filter's column less per batch.  No ABI call changes its arguments, its result or what it leaves in any
 * buffer the host can read; a sequence that differs from the hint (another filter follows, other columns, another prevSize,
 * a column written in between, no HashReduce at all) is executed as ever and only costs the scan that was launched for
 * nothing; after two such scans in a row the stream's hints are ignored until one describes another shape.
 * The hint ends with the InitIndexVector after the next one, with the stream, and with any write to or free of a byte of a
 * hinted column.  It is declined without effect when a column is shorter than batchRows, when the shape is not one the
 * compact DIRECT scan takes (1-4 dimensions of 4 bytes, a 4-byte main-table column each, at most 4 comparison filters), and
 * when ARES_DEFER=0, ARES_FUSE=0, ARES_FILTER_ROWSPACE=0 or ARES_SCAN_AT_FILTER=0 is set (the last obeys AresReloadEnv).
 * counters receives 10 words since the process started: {hints taken, scans launched at a filter, scans HashReduce merged its result from,
 * hints declined, scans discarded because HashReduce derived another plan, ... other sizes / partitions / kernel / stream
 * room or needed region A, ... a hinted column was written or freed, ... HashReduce never consumed the stream's queue,
 * scans taken whose call then scanned again or fell back (stale ranges, record stream overflow), hints ignored by the
 * two-discard latch}: every scan launched at a filter ends in exactly one of the counters behind "scans launched". */
void AresHintFusedBatch(const AresFusedQuery *query, int batchRows, int prevSize, int measureBytes, void *cudaStream, int device);
void AresScanAtFilterStats(unsigned long long *counters);

/* Fused select scan: the batch of a NON-AGGREGATION query (SELECT cols WHERE ... LIMIT n, query/aql_nonaggr_batchexecutor.go)
 * in one limit-aware pass over the source columns.  It replaces, for one batch, the call sequence
 *   InitIndexVector, Unary/BinaryFilter x numFilters, Unary/BinaryTransform x numDims into rows [0, survivors) of outKeys
 * with the rows cut at `limit` (< 0: none): the dimension rows (values, one validity byte per dimension) of the first
 * min(survivors, limit) surviving rows, in ascending row order, are written into rows [0, res) of outKeys, byte for byte what
 * the sequence stores for those rows (value bytes of null rows included); rows at or beyond res are not written;
 * res = that count.  Tiles of 4096 rows are handed out in row order, and once a tile's inclusive survivor count has reached
 * the limit no further tile reads a column: a small limit costs one round of the grid whatever the batch size.
 *
 * Shapes accepted (anything else returns an error string starting with "not fusable" before anything is launched, and the
 * host simply runs the ordinary sequence): 0-4 filters, each a comparison of a main-table column (1-, 2- or 4-byte type,
 * modes 1/2/3) with a constant; 1-8 dimensions in vector order (dims[d] is slot d of outKeys, widths descending), each either
 * a main-table column of a 1-, 2- or 4-byte type, bare or combined with a constant by a binary functor, into a slot of
 * 4 / 2 / 1 bytes (outType = the slot's DataType; a narrow slot takes integer results), or a BARE Int64 / GeoPoint / UUID
 * column (modes 1/2; Int64 and UUID mode 3 as well) into a slot of its own type.
 * Mode 3 is the run-length layout of an archive batch's sort columns, [counts u32 x (Length + 1)][validity bit per run]
 * [value per run] with Length = the number of runs (at least 1): rows are raw rows (no base counts, start count 0), row r
 * lies in the run whose [counts[k], counts[k + 1]) holds it, rows past the last count take the last run, and counts[Length]
 * is not read — what the per-node sequence does.  The runs are located inside each 4096-row tile, so the limit's early out
 * holds for archive batches too, and a tile that lies inside ONE run of a filter column that is null or fails the comparison
 * is thrown away without reading any other column (AresSelectRunStats counts them).
 * Declined: Bool and Uint64 columns, mode 0 columns, a GeoPoint column in the mode-3 layout (the per-node sequence never
 * decodes one: it reads it row by row as a mode-2 column), a mode-3 column without runs, foreign-table operands (those go to
 * AresFusedFilterJoinSelect below) and array operands,
 * expressions over a wide column.  outKeys.VectorCapacity must be at least batchRows (limit < 0) or
 * min(batchRows, limit); batchRows == 0 or limit == 0 returns 0 and launches nothing.
 * Environment (both obey AresReloadEnv): ARES_SELECT=0 declines always; ARES_SELECT_GRID=n (tests) sets the number of
 * workgroups, at most 2048. */
typedef struct {
  int numFilters;
  AresFusedExpr filters[4];
  int numDims;
  AresFusedExpr dims[8]; /* outType = the slot's DataType */
} AresFusedSelect;

CGoCallResHandle AresFusedFilterSelect(const AresFusedSelect *query, int batchRows, int limit /* < 0: none */,
                                       DimensionVector outKeys, void *cudaStream, int device);
/* {batches run, batches declined, tiles scanned, rows written} since process start */
void AresSelectStats(unsigned long long *counters);
/* {tiles rejected by one run of a run-length filter column, tiles that staged run ends in LDS} since process start; both are
 * counted among the tiles scanned */
void AresSelectRunStats(unsigned long long *counters);

/* Fused select scan with joins: the batch of a non-aggregation query that selects or filters on columns of joined dimension
 * tables, with the cuckoo probe inside the scan.  For one batch without base counts it replaces the call sequence
 *   InitIndexVector, BinaryFilter x numFilters, HashLookup x numJoins over the survivors (baseCounts NULL, startCount 0),
 *   BinaryFilter x numForeignFilters (the record-id vectors of all joins carried along),
 *   Unary/BinaryTransform x numDims into rows [0, survivors) of outKeys
 * cut at `limit` exactly as AresFusedFilterSelect is: rows [0, res) of outKeys hold, byte for byte, what the sequence stores
 * for the first min(survivors, limit) survivors in ascending row order (value bytes of null rows included), nothing at or
 * beyond res is written, res = that count.
 * An expression with foreignFilterJoin[k] / dimJoin[d] >= 0 has a ForeignColumnInput as lhs: Batches, BaseBatchID, NumBatches,
 * NumRecordsInLastBatch, DataType and DefaultValue mean what they mean for UnaryTransform; RecordIDs is ignored — no record-id
 * vector exists on this path.  A joined value is what the per-node sequence reads: a missing or null key, a batchID outside
 * the table and an index at or past NumRecordsInLastBatch in the last batch give value bits 0 and validity 0; a mode-0 batch
 * gives the default value and the default's validity; a batch with ValuesOffset != 0 takes validity from its bitmap; any other
 * batch is valid.  A foreign filter treats a null operand as the main-table filters do.
 * A join that some foreign filter reads is probed, per 4096-row tile, for the rows the main-table filters left alive; a join
 * that only dimensions read is probed for the rows that are written — with a small limit, that many keys and no more.  The
 * tile-level early out of AresFusedFilterSelect applies unchanged.
 *
 * Shapes accepted: main-table filters and dimensions as AresFusedFilterSelect (run-length columns included); 1-2 joins, the
 * key a bare main-table column in mode 1 or 2 of any type and index geometry HashLookup accepts for one (1-, 2- and 4-byte
 * types, Int64, UUID; keyBytes 1..16, numHashes 0..4, numBuckets >= 1); 0-4 foreign filters, each a comparison of a joined
 * column with a constant; joined dimensions of 1-, 2- or 4-byte types, bare or combined with a constant by a binary functor,
 * into 4 / 2 / 1 byte slots (no float result into a narrow slot).
 * Declined ("not fusable", nothing launched): numJoins == 0 (AresFusedFilterSelect is the entry point for that) or > 2, a
 * run-length or mode-0 key column, a Bool or wide (Int64 / Uint64 / GeoPoint / UUID) joined column, a non-null
 * TimezoneLookup, a join index out of range, everything AresFusedFilterSelect declines, ARES_SELECT=0.  Capacity, zero rows
 * and a zero limit are as for AresFusedFilterSelect. */
typedef struct {
  InputVector key;       /* main-table column the join key comes from: HashLookup's `input` */
  CuckooHashIndex index; /* HashLookup's `hashIndex` */
} AresFusedJoin;

typedef struct {
  int numFilters;
  AresFusedExpr filters[4]; /* main-table filters, as AresFusedSelect */
  int numJoins;
  AresFusedJoin joins[2];
  int numForeignFilters;
  AresFusedExpr foreignFilters[4];
  int foreignFilterJoin[4]; /* the join each foreign filter reads */
  int numDims;
  AresFusedExpr dims[8];
  int dimJoin[8]; /* the join a dimension reads; -1: a main-table column */
} AresFusedJoinSelect;

CGoCallResHandle AresFusedFilterJoinSelect(const AresFusedJoinSelect *query, int batchRows, int limit /* < 0: none */,
                                           DimensionVector outKeys, void *cudaStream, int device);
/* {batches run, batches declined, tiles scanned, rows written, keys probed} of AresFusedFilterJoinSelect since process
 * start (AresSelectStats counts AresFusedFilterSelect's only) */
void AresSelectJoinStats(unsigned long long *counters);

/* Joined columns resolved once per batch, in row space: for an AGGREGATION query over a fact table joined to dimension tables.
 * One kernel of HashLookup's geometry (one probe per lane) probes the key column of a batch without base counts and gathers up
 * to four joined columns, each written as an ordinary main-table column of the batch's length with a validity bitmap.  The host
 * then runs the batch as a join-free query over its columns plus these: foreign filters are row-space filters, joined
 * dimensions are queued transforms, and every fast path of a join-free query applies.  It replaces, for one batch and table,
 *   HashLookup over the survivors and the record-id vectors every later call of the batch carries.
 * Output of column c: [bitmap: ceil(rows / 8) bytes, padded to a multiple of 64][values: rows x width, padded to 64] at
 * columns[c].out, AresJoinColumnBytes(batchRows, type) bytes in all, and
 *   outSlices[c] = {BasePtr = out, NullsOffset = 0, ValuesOffset = the padded bitmap bytes, StartingIndex = 0,
 *                   Length = batchRows, DataType = the joined column's, DefaultValue = the foreign column's}.
 * Row r's (value bits, validity) is what the per-node sequence reads for the record of row r's key, the value stored at the
 * column's width: a null or missing key, a batch outside the table and an index at or past NumRecordsInLastBatch in the last
 * batch give (0, null); a mode-0 batch gives the default and the default's validity; a batch with ValuesOffset != 0 takes
 * validity from its bitmap; any other batch is valid.  Bitmap bits at or past batchRows inside the last written 8-byte word are
 * 0; bytes past that word are not written.
 * filters are pruning HINTS, the main-table filters of the query: a row that fails an evaluated hint is not probed and gets
 * (0, null) — the host's own filters kill it anyway.  A hint the kernel cannot evaluate (anything but a comparison of a
 * mode-1/2 main-table column of a 1-, 2- or 4-byte type with a constant) is ignored: fewer rows are pruned, nothing else.
 * Accepted: the key as AresFusedFilterJoinSelect's (a bare main-table column in mode 1 or 2 of any type and index geometry
 * HashLookup takes); 1-4 joined columns of 1-, 2- or 4-byte non-Bool types (a ForeignColumnInput, fields as for UnaryTransform,
 * RecordIDs ignored).  Declined ("not fusable", nothing launched): a Bool or wide joined column, a non-null TimezoneLookup, a
 * mode-0 or run-length key, numColumns outside 1..4, a null or misaligned `out`, ARES_JOIN_COLUMNS=0.
 * Two flavours, byte-identical on every row that no hint prunes:
 *   probe — one row and one probe per lane, as above, hints evaluated first.  Every key HashLookup accepts; a narrow key on a
 *     batch too short for the direct flavour.
 *   direct — the key column's type is 1 or 2 bytes wide (Int8, Uint8, Int16, Uint16).  A first kernel enumerates all 2^8 or
 *     2^16 stored key values, widens each as HashLookup does (the column's type decides sign extension, keyBytes what is kept),
 *     probes once per value and writes, into stream temporaries, 4 bytes of value bits per value and joined column and one byte
 *     of validity bits per value — at most 65 536 x (4 x 4 + 1) bytes, 1.06 MiB; a second kernel streams over the rows, four
 *     per lane: keys in, four gathers per column from the table, the values out at the column's width.  No probe per row.
 *     Hints are NOT evaluated: a row a hint would prune is written as any other row (the host's own filters kill it), so the
 *     output is the probe flavour's for the same query without hints.  Chosen when the key is narrow and
 *     batchRows >= 64 x the number of key values (16 384 rows for a 1-byte key, 4 Mi rows for a 2-byte key).
 * res = batchRows.  The call does not wait for the stream; the outputs are reported to libmem.so as written (AresMemNoteWrite).
 * Environment (both obey AresReloadEnv): ARES_JOIN_COLUMNS=0 declines always, =probe / =direct force a flavour where it is
 * applicable (direct on a 4-byte or wide key still probes), anything else chooses as above; ARES_JOIN_COLUMNS_GRID=n (tests)
 * sets the number of workgroups. */
typedef struct {
  InputVector column; /* ForeignColumnInput */
  uint8_t *out;       /* device, 64-byte aligned, AresJoinColumnBytes(batchRows, DataType) bytes */
} AresJoinedColumn;

typedef struct {
  int numFilters;
  AresFusedExpr filters[4]; /* optional pruning hints */
  AresFusedJoin join;       /* key column + cuckoo index */
  int numColumns;
  AresJoinedColumn columns[4];
} AresJoinColumns;

size_t AresJoinColumnBytes(int rows, enum DataType type); /* 0 for a type the entry point declines */
CGoCallResHandle AresJoinColumnsRun(const AresJoinColumns *q, int batchRows, VectorPartySlice *outSlices, void *cudaStream,
                                    int device);
/* {batches run, batches declined, rows, keys probed} since process start; keys probed = 256 or 65536 for a direct batch, for a
 * probe batch the rows that passed every evaluated hint and had a valid key, counted on the device: the caller has waited for
 * its streams */
void AresJoinColumnStats(unsigned long long *counters);
/* {probe batches, direct batches, table entries built by direct batches} since process start; a batch of zero rows launches
 * nothing and is neither */
void AresJoinColumnFlavourStats(unsigned long long *counters);

/* The geofence verdict of a batch resolved once, in row space: for an AGGREGATION query with a geography_intersects join whose
 * points are a main-table column.  One kernel classifies every row of a batch without base counts (pruning hints, null
 * points), compacts the live rows of each 1024-row tile in LDS and walks the polygon edges over them alone, as
 * GeoBatchIntersects' kernel walks them over the index vector; the verdict of row r is ONE byte of an ordinary mode-2 Uint8
 * main-table column.  The host then runs the batch as a geo-free query over its columns plus this one: the byte's validity is
 * the geo filter (a comparison of the column with a constant is null, hence false, for a null row), its value the geo
 * dimension, and every fast path of a geo-free query applies.  It replaces, for one batch,
 *   GeoBatchIntersects over the survivors, the predicate words it leaves, and WriteGeoShapeDim.
 * Output: [bitmap: ceil(rows / 8) bytes, padded to a multiple of 64][values: rows bytes, padded to 64] at `out`,
 * AresGeoShapeColumnBytes(batchRows) bytes in all (== AresJoinColumnBytes(batchRows, Uint8): the same layout), and
 *   *outSlice = {BasePtr = out, NullsOffset = 0, ValuesOffset = the padded bitmap bytes, StartingIndex = 0,
 *                Length = batchRows, DataType = Uint8}.
 * Bitmap bits at or past batchRows inside the last written 8-byte word are 0; bytes past that word are not written.
 * Row r: let `words` be what GeoBatchIntersects leaves in a predicate vector that started at zero for an entry whose index is
 * r, and s the first set bit of the words read as an int8 (shapes 128..255 read as none, -1).  Row r is VALID iff
 * (s < 0) != inOrOut — exactly the rows GeoBatchIntersects keeps —; its value is s when inOrOut != 0 and the row is valid,
 * 0 otherwise.  A null point follows the first-edge rule: with TotalNumPoints >= 2 and shape[0] == shape[1] it is null
 * whichever way the filter asks; otherwise its words stay zero, so it is null when inOrOut != 0 and valid with value 0 when
 * inOrOut == 0.  TotalNumPoints == 0 toggles nothing.
 * filters are pruning HINTS exactly as AresJoinColumns::filters: a row that fails an evaluated hint is not walked and gets
 * (0, null); a hint the kernel cannot evaluate is ignored.
 * Accepted: a GeoPoint main-table column in mode 1 or 2.  Declined ("not fusable", nothing launched, nothing written): a mode-0
 * or run-length point column, a column shorter than batchRows, a joined (ForeignColumnInput) point column, a null or misaligned
 * `out`, ARES_GEO_COLUMN=0.  TotalWords outside 1..8 is GeoBatchIntersects' error.
 * res = batchRows.  The call does not wait for the stream; the output is reported to libmem.so as written (AresMemNoteWrite).
 * Environment (both obey AresReloadEnv): ARES_GEO_COLUMN=0 declines always; ARES_GEO_COLUMN_GRID=n (tests) sets the number of
 * workgroups. */
typedef struct {
  int numFilters;
  AresFusedExpr filters[4]; /* optional pruning hints, as AresJoinColumns::filters */
  GeoShapeBatch shapes;     /* as GeoBatchIntersects takes it */
  InputVector points;       /* VectorPartyInput, GeoPoint, main table */
  int inOrOut;
  uint8_t *out;             /* device, 64-byte aligned, AresGeoShapeColumnBytes(batchRows) bytes */
} AresGeoShapeColumn;

size_t AresGeoShapeColumnBytes(int rows);
CGoCallResHandle AresGeoShapeColumnRun(const AresGeoShapeColumn *q, int batchRows, VectorPartySlice *outSlice, void *cudaStream,
                                       int device);
/* {batches run, batches declined, rows, live rows, wavefront-chunks walked} since process start; live rows = rows that passed
 * every evaluated hint and had a valid point, wavefront-chunks = the sum over tiles of ceil(live rows of the tile / 64), both
 * counted on the device: the caller has waited for its streams */
void AresGeoShapeColumnStats(unsigned long long *counters);

/* Local time resolved once per batch, in row space: for an AGGREGATION query that buckets a time column in the time zone of a
 * joined table — FLOOR(CONVERT_TZ(request_at, cities.timezone), bucket), query/time_bucketizer.go:72-92, where CONVERT_TZ is
 * Plus and the joined enum column is read through the int16 offset table (TimezoneLookup, query/iterator.hpp:888-914).  Local
 * time is a pure function of (time, join key): it is written as an ordinary mode-2 main-table column of the batch's length, and
 * the host then runs the batch with `Floor(that column, bucket)` — the "one column (op constant)" shape of every fast path.  It
 * replaces, for one batch without base counts and one (time column, table, zone column),
 *   HashLookup over the survivors, then BinaryTransform(Plus, time, the zone column with its TimezoneLookup) into scratch.
 * Output: AresJoinColumnsRun's layout, [bitmap: ceil(rows / 8) bytes, padded to a multiple of 64][values: rows x 4, padded to
 * 64] at `out`, AresJoinColumnBytes(batchRows, Uint32) bytes in all, and
 *   *outSlice = {BasePtr = out, NullsOffset = 0, ValuesOffset = the padded bitmap bytes, StartingIndex = 0,
 *                Length = batchRows, DataType = outType}.
 * Bitmap bits at or past batchRows inside the last written 8-byte word are 0; bytes past that word are not written.
 * Row r is what the per-node sequence leaves for it: value = time[r] + offset taken mod 2^32, valid = time valid AND key valid
 * AND record found AND joined value valid; a null row is written as value 0.  `offset` is what a foreign operand with a
 * TimezoneLookup reads: tz[enum] for enum < TimezoneLookupSize, else 0; a mode-0 batch yields its default WITHOUT the lookup
 * (query/iterator.hpp:922-926) and the default's validity; a null or missing key, a batch outside the table and an index at or
 * past NumRecordsInLastBatch in the last batch give (0, null).
 * Two flavours, byte-identical on every row that no hint prunes:
 *   direct — the key column's type is 1 or 2 bytes wide (Int8, Uint8, Int16, Uint16).  A first kernel enumerates all 2^8 or
 *     2^16 stored key values, widens each as HashLookup does (the column's type decides sign extension, keyBytes what is kept),
 *     probes once per value and writes an (offset, valid) table of 4 bytes per value — at most 256 KiB — into a stream temporary;
 *     a second kernel streams over the rows: time and key in, one gather from the table, the value out.  No probe per row; hints
 *     are not evaluated.  Chosen when the key is narrow and batchRows >= the number of key values.
 *   probe — every other key HashLookup accepts (4-byte types, Int64, UUID): AresJoinColumnsRun's geometry, one row and one
 *     probe per lane.  filters are pruning HINTS exactly as AresJoinColumns::filters: a row that fails an evaluated hint is not
 *     probed and gets (0, null); a hint the kernel cannot evaluate is ignored.
 * Declined ("not fusable", nothing launched, nothing written): a null TimezoneLookup, a zone type other than Uint8 or Uint16 or
 * a zone that is no ForeignColumnInput, a time type other than Uint32 or Int32 (outType likewise), a mode-0 or run-length time
 * or key column or one shorter than batchRows, index geometry HashLookup rejects, a null or misaligned `out`,
 * ARES_LOCAL_TIME=0.
 * res = batchRows.  The call does not wait for the stream; the output is reported to libmem.so as written (AresMemNoteWrite).
 * Environment (both obey AresReloadEnv): ARES_LOCAL_TIME=0 declines always, =probe / =direct (tests) force a flavour where it
 * is applicable; ARES_LOCAL_TIME_GRID=n (tests) sets the number of workgroups. */
typedef struct {
  int numFilters;
  AresFusedExpr filters[4]; /* pruning hints, as AresJoinColumns::filters (probe flavour only) */
  InputVector time;         /* VectorPartyInput, main table, Uint32 or Int32, mode 1 or 2 */
  AresFusedJoin join;       /* key column + cuckoo index of the zone's table */
  InputVector zone;         /* ForeignColumnInput, Uint8 or Uint16, TimezoneLookup != NULL, RecordIDs ignored */
  enum DataType outType;    /* Uint32 or Int32: the CONVERT_TZ node's outType; same bits either way */
  uint8_t *out;             /* device, 64-byte aligned, AresJoinColumnBytes(batchRows, Uint32) bytes */
} AresLocalTimeColumn;

CGoCallResHandle AresLocalTimeColumnRun(const AresLocalTimeColumn *q, int batchRows, VectorPartySlice *outSlice, void *cudaStream,
                                        int device);
/* {batches run, batches declined, rows, keys probed, direct batches} since process start; keys probed = 256 or 65536 for a
 * direct batch, for a probe batch the rows that passed every evaluated hint and had a valid key, counted on the device: the
 * caller has waited for its streams */
void AresLocalTimeColumnStats(unsigned long long *counters);

#ifdef __cplusplus
}
#endif
#endif /* ARES_EXTENSIONS_H_ */
