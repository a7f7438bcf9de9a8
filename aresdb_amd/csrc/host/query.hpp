// One query on one device: the batch context and the executor's steps.
//   AresQuery (state)  <- oopkBatchContext (query/aql_context.go, query/aql_processor.go:690-804)
//   AresQuery (steps)  <- BatchExecutorImpl / NonAggrBatchExecutorImpl, defined in batch_executor.cpp;
//                         the row-space rewrites (no counterpart in the Go host) in row_space.cpp
// Buffer ownership follows the Go code: the host allocates and frees every buffer through libmem, the result buffers grow by
// 12.5 % and are double-buffered.
#pragma once

#include <memory>
#include <utility>
#include <vector>

#include "plan.hpp"

namespace ares_host {

// A row-space rewrite (AresQuerySetJoinColumns / AresQuerySetGeoColumn, ares_driver.h): decided once per query, it holds the plan
// a batch without base counts runs instead of the query's own, over the batch's columns + the ones one extension call (per
// foreign table) resolves for it.  Every added column is a main-table leaf of `plan` whose column number is patched per batch.
struct RowSpace {
  enum Kind { JOIN_COLUMNS, GEO_COLUMN } kind;
  Plan plan;
  std::vector<std::pair<int, int>> leaves;  // (node of `plan`, position among the added columns)
  int numAdded = 0;                         // columns behind the batch's own
  struct JoinedTable {
    std::vector<int> columns;  // the table's columns the query reads, in order of first reference (at most four)
    int first = 0;             // position of columns[0] among the added columns
  };
  std::vector<JoinedTable> tables;  // JOIN_COLUMNS: one per foreign table
  // JOIN_COLUMNS: the local-time columns (AresLocalTimeColumnRun), behind the joined ones: one per distinct
  // (time column, table, zone column, type) the query's CONVERT_TZ nodes name, at most two
  struct LocalTime {
    int timeColumn;  // main table
    int table;       // foreign table, from 0
    int zoneColumn;  // column of that table
    int outType;     // the CONVERT_TZ nodes' outType: the column's DataType
    bool operator==(const LocalTime &o) const {
      return timeColumn == o.timeColumn && table == o.table && zoneColumn == o.zoneColumn && outType == o.outType;
    }
  };
  std::vector<LocalTime> localTimes;
  RowSpace(Kind k, const Plan &original) : kind(k), plan(original) {}
};

}  // namespace ares_host

struct AresQuery {
  using Plan = ares_host::Plan;
  using IV = ares_host::IV;

  ares_host::AbiLibrary *lib;
  const Plan plan;  // the query's own: what everything outside a batch reads
  // what the running batch executes: `plan`, or the row-space rewrite from resolve() until the batch ends (runBatch)
  const Plan *batchPlan = &plan;
  const ares_host::DimLayout layout;
  int device;
  void *stream;
  // the Go host owns two streams per query and swaps them after every batch
  // (query/aql_processor.go:66-67, :218, :247): batch k's calls go to one, batch k+1's to the other
  void *otherStream = nullptr;
  // oopkBatchContext
  int resultSize = 0, resultCapacity = 0;
  uint8_t *dimVec[2] = {nullptr, nullptr};
  uint8_t *measureVec[2] = {nullptr, nullptr};
  // HyperLogLog queries (query/aql_context.go:289-294): allocated by the library on the last batch
  uint8_t *hllVector = nullptr;
  uint16_t *hllDimRegIDCount = nullptr;
  size_t hllVectorSize = 0;
  bool isLastBatch = false;
  uint32_t *geoPredicateVec = nullptr;
  int sizeBeforeGeoFilter = 0;
  std::vector<void *> ownedColumns;  // device allocations of the batch's columns handed over by the caller
  uint64_t *hashVec[2] = {nullptr, nullptr};
  uint32_t *dimIndexVec[2] = {nullptr, nullptr};
  int size = 0;
  uint32_t *indexVec = nullptr;
  uint8_t *predVec = nullptr;
  uint32_t *baseCounts = nullptr;
  uint32_t startRow = 0;
  const VectorPartySlice *columns = nullptr;
  int numColumns = 0;
  std::vector<uint8_t *> stack;
  std::vector<RecordID *> foreignRids;
  std::vector<std::vector<VectorPartySlice>> foreignSliceArrays;  // Go slices handed to the callee for one call
  long calls = 0, fusedBatches = 0;
  bool fusedDeclined = false;  // the library rejected the plan once: stop asking
  // the row-space rewrite (row_space.cpp)
  std::unique_ptr<ares_host::RowSpace> rowSpace;  // null: the setters are off or the query is not eligible
  bool rowSpaceDeclined = false;                  // the library rejected the shape once: stop asking
  std::vector<VectorPartySlice> extendedColumns;  // the batch's columns + the resolved ones
  std::vector<void *> joinedOutputs;              // the resolved columns' allocations: released with the batch's input columns
  // non-aggregation queries (query/aql_nonaggr_batchexecutor.go): rows flushed to the host batch by batch
  int maxBatchSize = 0;   // qc.maxBatchSizeAfterPrefilter (AresQuerySetMaxBatchSize); 0: the first batch's size
  int batchRows = 0;      // rows of the current batch BEFORE its filters (batch.Size): what the dimension buffers are sized by
  int rowsWritten = 0;    // qc.numberOfRowsWritten
  bool done = false;      // OOPK.done: nothing more is wanted
  // the query's result on the host, the sections of a dimension vector: the values of every dimension, then the validity bytes
  std::vector<std::vector<uint8_t>> hostSections;

  AresQuery(ares_host::AbiLibrary *l, const AresQueryPlan &p, int dev, void *s)
      : lib(l), plan(p), layout(plan.dimTypes), device(dev), stream(s) {}

  // -- device_allocator.go semantics: every byte is allocated and freed by the host through libmem --
  template <typename T = uint8_t>
  T *alloc(size_t bytes) {
    return reinterpret_cast<T *>(ares_host::check(lib->DeviceAllocate(bytes ? bytes : 1, device)));
  }
  void release(void *p) {
    if (p) ares_host::check(lib->DeviceFree(p, device));
  }
  void wait() { ares_host::check(lib->WaitForCudaStream(stream, device)); }
  void d2d(void *dst, void *src, size_t bytes) {
    if (bytes) ares_host::check(lib->AsyncCopyDeviceToDevice(dst, src, bytes, stream, device));
  }
  void d2h(void *dst, void *src, size_t bytes) { ares_host::check(lib->AsyncCopyDeviceToHost(dst, src, bytes, stream, device)); }
  // asyncCopyDimensionVector between two device vectors / from a device vector to a host one
  void copyDimsD2D(uint8_t *to, uint8_t *from, int64_t length, int64_t offset, int64_t toCapacity, int64_t fromCapacity,
                   int64_t fromOffset = 0) {
    ares_host::copy_dimension_vector(layout, to, from, length, offset, toCapacity, fromCapacity,
                                     [this](void *d, void *s, size_t n) { d2d(d, s, n); }, fromOffset);
  }
  void copyDimsD2H(uint8_t *to, uint8_t *from, int64_t length, int64_t toCapacity, int64_t fromCapacity) {
    ares_host::copy_dimension_vector(layout, to, from, length, 0, toCapacity, fromCapacity,
                                     [this](void *d, void *s, size_t n) { d2h(d, s, n); });
  }

  // the context's buffers (batch_executor.cpp)
  void prepareForFiltering(const VectorPartySlice *cols, int ncols, int n, uint32_t *bc, uint32_t start);
  void prepareForDimAndMeasureEval();
  uint8_t *allocateStackFrame(int dataType, uint32_t *nullsOffset);
  void shrinkStackFrame();
  void releaseInputColumns();
  void cleanupBeforeAggregation();
  void swapResultBuffers();
  void releaseAll();
  DimensionVector dimensionVector(int which) const;

  // processExpression (time_series_aggregate.go:491-593)
  // root action: what to do with the operands of the expression's root
  struct Action {
    enum Kind { NONE, FILTER, MEASURE, DIMENSION } kind = NONE;
    int dimType = 0;
    int64_t valueOff = 0, nullOff = 0;
    int prevResultSize = 0;
  };
  IV columnInput(const AresPlanNode &n, bool withRids = true, bool withTimezone = false);
  void runAction(const Action &a, int functor, IV *in, int arity);
  IV processExpression(int nodeIdx, const Action &action, bool underConvertTz = false);

  // BatchExecutorImpl.Run (aql_batchexecutor.go:103-273)
  void preExec();
  void filter();
  void join();
  void evalDimensions(int prev);
  void project();
  void reduce();
  void postExec() { swapResultBuffers(); }
  void swapStreams() {
    if (otherStream) std::swap(stream, otherStream);
  }
  void runBatch(const VectorPartySlice *cols, int ncols, int n, uint32_t *bc, uint32_t start);

  // NonAggrBatchExecutorImpl (query/aql_nonaggr_batchexecutor.go)
  int recordsNeeded() const { return plan.limit < 0 ? -1 : std::max(plan.limit - rowsWritten, 0); }  // getNumberOfRecordsNeeded (:107-117)
  void prepareForDimEval();
  void expandDimensions();
  void projectNonAggr();
  void postExecNonAggr();
  void runBatchNonAggr(const VectorPartySlice *cols, int ncols, int n, uint32_t *bc, uint32_t start);

  // the fused extensions (include/ares_extensions.h): one call per batch
  bool fusedExpr(int nodeIdx, int outType, AresFusedExpr *e, int *join = nullptr);
  bool fusedFilters(const std::vector<int> &roots, AresFusedExpr *out, int *count, int *joins = nullptr);
  bool fusedDims(AresFusedExpr *out, int *count, int *joins = nullptr);
  bool fusedQuery(AresFusedQuery *q);
  void hintBatch();
  bool runBatchFused(const VectorPartySlice *cols, int ncols, int n);
  bool runBatchFusedSelect(const VectorPartySlice *cols, int ncols, int n);

  // the row-space rewrite (row_space.cpp)
  void setRowSpace(ares_host::RowSpace::Kind kind, bool on);
  int pruningHints(AresFusedExpr *out);
  bool runJoinColumns(ares_host::RowSpace &rs, int n);
  bool runLocalTimeColumns(ares_host::RowSpace &rs, int n);
  bool runGeoColumn(int n);
  bool resolve(const VectorPartySlice *cols, int ncols, int n);
};
