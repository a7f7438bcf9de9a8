// libaresdriver.so — C++ mirror of the reference's Go batch executor above the cgo C ABI: the steps of one batch.
//
//   the context's buffers  <- oopkBatchContext (query/aql_processor.go:690-804)
//   processExpression      <- query/time_series_aggregate.go:491-593 (AST walk, one ABI call per node)
//   runBatch               <- BatchExecutorImpl.Run (query/aql_batchexecutor.go:103-273)
//   runBatchNonAggr        <- NonAggrBatchExecutorImpl (query/aql_nonaggr_batchexecutor.go)
//   runBatchFused[Select]  <- no counterpart: the fused extensions of include/ares_extensions.h
//
// Stage order and ABI calls follow the Go code line by line; only the language differs.
#include <algorithm>
#include <cstring>

#include "query.hpp"

using namespace ares_host;

// -- aql_processor.go:726-739 --
void AresQuery::prepareForFiltering(const VectorPartySlice *cols, int ncols, int n, uint32_t *bc, uint32_t start) {
  columns = cols;
  numColumns = ncols;
  size = n;
  batchRows = n;
  baseCounts = bc;
  startRow = start;
  indexVec = alloc<uint32_t>(static_cast<size_t>(n) * 4);
  predVec = alloc<uint8_t>(static_cast<size_t>(n));
}

// -- aql_processor.go:743-804: grow the result buffers by 12.5 % and carry the old results over --
void AresQuery::prepareForDimAndMeasureEval() {
  if (resultSize + size <= resultCapacity) return;
  const int oldCapacity = resultCapacity;
  resultCapacity = resultSize + size;
  resultCapacity += resultCapacity / 8;
  const int64_t cap = resultCapacity;
  {
    uint8_t *old0 = dimVec[0], *old1 = dimVec[1];
    const size_t unit = std::max(layout.rowBytes, 1);
    dimVec[0] = alloc(cap * unit);
    dimVec[1] = alloc(cap * unit);
    if (old0) copyDimsD2D(dimVec[0], old0, resultSize, 0, cap, oldCapacity);
    if (old0 || old1) wait();
    release(old0);
    release(old1);
  }
  if (plan.isHLL() || !plan.useHashReduction) {
    release(dimIndexVec[0]); release(dimIndexVec[1]);
    dimIndexVec[0] = alloc<uint32_t>(cap * 4); dimIndexVec[1] = alloc<uint32_t>(cap * 4);
    uint64_t *old0 = hashVec[0], *old1 = hashVec[1];
    hashVec[0] = alloc<uint64_t>(cap * 8); hashVec[1] = alloc<uint64_t>(cap * 8);
    // HyperLogLog keeps the merged keys of the earlier batches in hash vector [0]
    if (plan.isHLL() && old0 && resultSize) {
      d2d(hashVec[0], old0, static_cast<size_t>(resultSize) * 8);
      wait();
    }
    release(old0); release(old1);
  }
  {
    const int mb = plan.measureBytes();
    uint8_t *old0 = measureVec[0], *old1 = measureVec[1];
    measureVec[0] = alloc(cap * mb);
    measureVec[1] = alloc(cap * mb);
    if (old0 && resultSize) d2d(measureVec[0], old0, static_cast<size_t>(resultSize) * mb);
    if (old0 || old1) wait();
    release(old0);
    release(old1);
  }
}

// -- time_series_aggregate.go:745-769 --
uint8_t *AresQuery::allocateStackFrame(int dataType, uint32_t *nullsOffset) {
  const int w = (dataType == Int64 || dataType == Uint64 || dataType == Float64 || dataType == GeoPoint) ? 8
                : dataType == UUID ? 16 : 4;
  uint8_t *values = alloc(static_cast<size_t>(w + 1) * size);
  stack.push_back(values);
  *nullsOffset = static_cast<uint32_t>(w) * size;
  return values;
}
void AresQuery::shrinkStackFrame() {
  std::swap(stack[stack.size() - 1], stack[stack.size() - 2]);
  release(stack.back());
  stack.pop_back();
}

// the batch's input columns (query/aql_processor.go:695-699), and the columns resolved for it in row space
void AresQuery::releaseInputColumns() {
  for (void *p : ownedColumns) release(p);
  ownedColumns.clear();
  for (void *p : joinedOutputs) release(p);
  joinedOutputs.clear();
}
void AresQuery::cleanupBeforeAggregation() {
  // the batch's input columns go first (query/aql_processor.go:695-699)
  releaseInputColumns();
  release(indexVec); indexVec = nullptr;
  release(predVec); predVec = nullptr;
  for (RecordID *p : foreignRids) release(p);
  foreignRids.clear();
  release(geoPredicateVec); geoPredicateVec = nullptr;
  for (uint8_t *p : stack) release(p);
  stack.clear();
  foreignSliceArrays.clear();
}
void AresQuery::swapResultBuffers() {
  size = 0;
  std::swap(dimVec[0], dimVec[1]);
  std::swap(measureVec[0], measureVec[1]);
  std::swap(hashVec[0], hashVec[1]);
}
void AresQuery::releaseAll() {
  for (int i = 0; i < 2; i++) {
    release(dimVec[i]); release(measureVec[i]); release(hashVec[i]); release(dimIndexVec[i]);
    dimVec[i] = nullptr; measureVec[i] = nullptr; hashVec[i] = nullptr; dimIndexVec[i] = nullptr;
  }
  release(hllVector); release(hllDimRegIDCount);
  hllVector = nullptr; hllDimRegIDCount = nullptr; hllVectorSize = 0;
  resultCapacity = 0;
}

// -- processExpression (time_series_aggregate.go:491-593) --
// withRids = false: a joined column for an extension that has no record-id vectors; withTimezone: the leaf is a direct child
// of a CONVERT_TZ node and is read through the plan's offset table (time_series_aggregate.go:506-516)
IV AresQuery::columnInput(const AresPlanNode &n, bool withRids, bool withTimezone) {
  IV iv;
  if (n.table == 0) {
    if (n.column < 0 || n.column >= numColumns) throw AbiError("column index out of range");
    iv->Vector.VP = columns[n.column];
    iv->Type = VectorPartyInput;
    return iv;
  }
  const Plan::Foreign &ft = batchPlan->foreign.at(n.table - 1);
  foreignSliceArrays.emplace_back(ft.slices.begin() + static_cast<size_t>(n.column) * ft.t.numBatches,
                                  ft.slices.begin() + static_cast<size_t>(n.column + 1) * ft.t.numBatches);
  ForeignColumnVector &f = iv->Vector.ForeignVP;
  f.RecordIDs = withRids ? foreignRids.at(n.table - 1) : nullptr;
  f.Batches = foreignSliceArrays.back().data();
  f.BaseBatchID = ft.t.baseBatchID;
  f.NumBatches = ft.t.numBatches;
  f.NumRecordsInLastBatch = ft.t.numRecordsInLastBatch;
  if (withTimezone) {  // (otherwise TimezoneLookup stays NULL and its size 0: the zeroed box)
    *const_cast<int16_t **>(&f.TimezoneLookup) = const_cast<int16_t *>(plan.timezoneLookup);
    f.TimezoneLookupSize = static_cast<int16_t>(plan.timezoneLookupSize);
  }
  f.DataType = static_cast<DataType>(ft.dataTypes[n.column]);
  iv->Type = ForeignColumnInput;
  return iv;
}

namespace {
IV constantInput(const AresPlanNode &n) {
  IV iv;
  if (n.kind == ARES_NODE_CONST_FLOAT) {
    iv->Vector.Constant.Value.FloatVal = n.fval;
    iv->Vector.Constant.DataType = ConstFloat;
  } else {
    iv->Vector.Constant.Value.IntVal = n.ival;
    iv->Vector.Constant.DataType = ConstInt;
  }
  iv->Vector.Constant.IsValid = true;
  iv->Type = ConstantInput;
  return iv;
}
IV scratchInput(uint8_t *values, uint32_t nullsOffset, int dataType) {
  IV iv;
  iv->Vector.ScratchSpace.Values = values;
  iv->Vector.ScratchSpace.NullsOffset = nullsOffset;
  iv->Vector.ScratchSpace.DataType = static_cast<DataType>(dataType);
  iv->Type = ScratchSpaceInput;
  return iv;
}
OV scratchOutput(uint8_t *values, uint32_t nullsOffset, int dataType) {
  OV ov;
  ov->Vector.ScratchSpace.Values = values;
  ov->Vector.ScratchSpace.NullsOffset = nullsOffset;
  ov->Vector.ScratchSpace.DataType = static_cast<DataType>(dataType);
  ov->Type = ScratchSpaceOutput;
  return ov;
}
}  // namespace

void AresQuery::runAction(const Action &a, int functor, IV *in, int arity) {
  if (size <= 0) return;
  calls++;
  if (a.kind == Action::FILTER) {
    RecordID **vecs = foreignRids.empty() ? nullptr : foreignRids.data();
    const int nf = static_cast<int>(foreignRids.size());
    const intptr_t n =
        arity == 1 ? check(lib->UnaryFilter(in[0].get(), indexVec, predVec, size, vecs, nf, baseCounts, startRow,
                                            static_cast<UnaryFunctorType>(functor), stream, device))
                   : check(lib->BinaryFilter(in[0].get(), in[1].get(), indexVec, predVec, size, vecs, nf, baseCounts, startRow,
                                             static_cast<BinaryFunctorType>(functor), stream, device));
    size = static_cast<int>(n);
    return;
  }
  OV ov;
  if (a.kind == Action::MEASURE) {
    ov->Vector.Measure.Values = reinterpret_cast<uint32_t *>(measureVec[0] + static_cast<size_t>(resultSize) * plan.measureBytes());
    // hll values of the batch go to measure vector [1] (time_series_aggregate.go:404-408)
    if (plan.isHLL()) ov->Vector.Measure.Values = reinterpret_cast<uint32_t *>(measureVec[1]);
    ov->Vector.Measure.DataType = static_cast<DataType>(plan.measureType);
    ov->Vector.Measure.AggFunc = static_cast<AggregateFunction>(plan.aggFunc);
    ov->Type = MeasureOutput;
  } else {
    const int w = data_type_bytes(a.dimType);
    ov->Vector.Dimension.DimValues = dimVec[0] + a.valueOff + static_cast<int64_t>(w) * a.prevResultSize;
    ov->Vector.Dimension.DimNulls = dimVec[0] + a.nullOff + a.prevResultSize;
    ov->Vector.Dimension.DataType = static_cast<DataType>(a.dimType);
    ov->Type = DimensionOutput;
  }
  if (arity == 1)
    check(lib->UnaryTransform(in[0].get(), ov.get(), indexVec, size, baseCounts, startRow, static_cast<UnaryFunctorType>(functor),
                              stream, device));
  else
    check(lib->BinaryTransform(in[0].get(), in[1].get(), ov.get(), indexVec, size, baseCounts, startRow,
                               static_cast<BinaryFunctorType>(functor), stream, device));
}

// returns the node's value as an InputVector (leaf or scratch frame) when action is NONE,
// otherwise performs the root action
IV AresQuery::processExpression(int nodeIdx, const Action &action, bool underConvertTz) {
  const AresPlanNode &n = batchPlan->nodes.at(nodeIdx);
  IV none;
  switch (n.kind) {
    case ARES_NODE_COLUMN:
    case ARES_NODE_CONST_INT:
    case ARES_NODE_CONST_FLOAT: {
      IV iv = n.kind == ARES_NODE_COLUMN ? columnInput(n, true, underConvertTz) : constantInput(n);
      if (action.kind != Action::NONE) {
        runAction(action, Noop, &iv, 1);
        return none;
      }
      return iv;
    }
    case ARES_NODE_UNARY: {
      IV in = processExpression(n.lhs, Action());
      if (action.kind != Action::NONE) {
        runAction(action, n.op, &in, 1);
        return none;
      }
      uint32_t nullsOff;
      uint8_t *values = allocateStackFrame(n.outType, &nullsOff);
      calls++;
      check(lib->UnaryTransform(in.get(), scratchOutput(values, nullsOff, n.outType).get(), indexVec, size, baseCounts,
                                startRow, static_cast<UnaryFunctorType>(n.op), stream, device));
      if (in->Type == ScratchSpaceInput) shrinkStackFrame();
      return scratchInput(values, nullsOff, n.outType);
    }
    case ARES_NODE_BINARY: {
      IV in[2];
      const bool convertTz = batchPlan->isConvertTz(nodeIdx);
      in[0] = processExpression(n.lhs, Action(), convertTz);
      in[1] = processExpression(n.rhs, Action(), convertTz);
      if (action.kind != Action::NONE) {
        runAction(action, n.op, in, 2);
        return none;
      }
      uint32_t nullsOff;
      uint8_t *values = allocateStackFrame(n.outType, &nullsOff);
      calls++;
      check(lib->BinaryTransform(in[0].get(), in[1].get(), scratchOutput(values, nullsOff, n.outType).get(), indexVec, size,
                                 baseCounts, startRow, static_cast<BinaryFunctorType>(n.op), stream, device));
      if (in[1]->Type == ScratchSpaceInput) shrinkStackFrame();
      if (in[0]->Type == ScratchSpaceInput) shrinkStackFrame();
      return scratchInput(values, nullsOff, n.outType);
    }
    default:
      throw AbiError("unsupported expression node");
  }
}

DimensionVector AresQuery::dimensionVector(int which) const {
  DimensionVector dv;
  memset(&dv, 0, sizeof(dv));
  dv.DimValues = dimVec[which];
  dv.HashValues = hashVec[which];
  dv.IndexVector = dimIndexVec[which];
  dv.VectorCapacity = resultCapacity;
  memcpy(dv.NumDimsPerDimWidth, layout.ndw, sizeof(layout.ndw));
  return dv;
}

// ---- BatchExecutorImpl.Run (aql_batchexecutor.go:103-273) ----
void AresQuery::preExec() {
  if (indexVec && size > 0) {
    calls++;
    check(lib->InitIndexVector(indexVec, 0, size, stream, device));
  }
}
void AresQuery::filter() {
  Action a;
  a.kind = Action::FILTER;
  for (int f : batchPlan->filters) processExpression(f, a);
}
void AresQuery::join() {
  const Plan &p = *batchPlan;
  for (const Plan::Foreign &ft : p.foreign) {
    RecordID *rids = alloc<RecordID>(static_cast<size_t>(std::max(size, 1)) * 8);
    foreignRids.push_back(rids);
    if (size > 0) {
      calls++;
      check(lib->HashLookup(columnInput(main_column(ft.t.joinColumn)).get(), rids, indexVec, size, baseCounts, startRow, ft.t.index,
                            stream, device));
    }
  }
  Action a;
  a.kind = Action::FILTER;
  for (int f : p.foreignFilters) processExpression(f, a);
  // geo intersection (query/aql_batchexecutor.go:146-165, query/time_series_aggregate.go:636-660)
  if (p.hasGeo) geoPredicateVec = alloc<uint32_t>(static_cast<size_t>(std::max(size, 1)) * 4 * p.geoWords());
  sizeBeforeGeoFilter = size;
  if (p.hasGeo && size > 0 && p.geo.shapeLatLongs) {
    GeoShapeBatch shapes;
    shapes.LatLongs = const_cast<uint8_t *>(p.geo.shapeLatLongs);
    shapes.TotalNumPoints = p.geo.totalNumPoints;
    shapes.TotalWords = static_cast<uint8_t>(p.geoWords());
    AresPlanNode pointNode = main_column(p.geo.pointColumn);
    pointNode.table = p.geo.pointTable;
    const int nf = static_cast<int>(foreignRids.size());
    calls++;
    size = static_cast<int>(check(lib->GeoBatchIntersects(shapes, columnInput(pointNode).get(), indexVec, size, startRow,
                                                          nf ? foreignRids.data() : nullptr, nf, geoPredicateVec,
                                                          p.geo.inOrOut != 0, stream, device)));
  }
}
// evalDimensions(prevResultSize): the batch's dimension rows are written behind `prev` earlier ones
void AresQuery::evalDimensions(int prev) {
  const Plan &p = *batchPlan;
  for (size_t i = 0; i < p.dimNodes.size(); i++) {
    Action a;
    a.kind = Action::DIMENSION;
    a.dimType = p.dimTypes[i];
    a.prevResultSize = prev;
    layout.offsets(layout.dimVectorIndex[i], resultCapacity, &a.valueOff, &a.nullOff);
    if (p.hasGeo && p.geo.dimIndex == static_cast<int>(i)) {  // the shape number (time_series_aggregate.go:611-634)
      if (size > 0 && p.geo.shapeLatLongs) {
        DimensionOutputVector dv;
        dv.DimValues = dimVec[0] + a.valueOff + prev;
        dv.DimNulls = dimVec[0] + a.nullOff + prev;
        dv.DataType = Uint8;
        calls++;
        check(lib->WriteGeoShapeDim(p.geoWords(), dv, sizeBeforeGeoFilter, geoPredicateVec, stream, device));
      }
      continue;
    }
    processExpression(p.dimNodes[i], a);
  }
}
void AresQuery::project() {
  prepareForDimAndMeasureEval();
  evalDimensions(resultSize);
  Action m;
  m.kind = Action::MEASURE;
  processExpression(batchPlan->measureNode, m);
  wait();
  cleanupBeforeAggregation();
}
void AresQuery::reduce() {
  const int length = resultSize + size;
  const int mb = plan.measureBytes();
  if (plan.isHLL()) {  // query/aql_batchexecutor.go:221-233, query/time_series_aggregate.go:661-680
    calls += 3;
    check(lib->InitIndexVector(dimIndexVec[0], 0, resultSize, stream, device));
    check(lib->InitIndexVector(dimIndexVec[1], static_cast<uint32_t>(resultSize), length, stream, device));
    uint8_t *vec = nullptr;
    uint16_t *counts = nullptr;
    size_t vecSize = 0;
    resultSize = static_cast<int>(check(lib->HyperLogLog(
        dimensionVector(0), dimensionVector(1), reinterpret_cast<uint32_t *>(measureVec[0]),
        reinterpret_cast<uint32_t *>(measureVec[1]), resultSize, size, isLastBatch, &vec, &vecSize, &counts, stream, device)));
    if (vec || counts) {
      release(hllVector); release(hllDimRegIDCount);
      hllVector = vec; hllDimRegIDCount = counts; hllVectorSize = vecSize;
    }
  } else if (plan.useHashReduction) {
    calls++;
    resultSize = static_cast<int>(check(lib->HashReduce(dimensionVector(0), measureVec[0], dimensionVector(1), measureVec[1],
                                                        mb, length, static_cast<AggregateFunction>(plan.aggFunc), stream,
                                                        device)));
  } else {
    calls += 3;
    check(lib->InitIndexVector(dimIndexVec[0], 0, length, stream, device));
    check(lib->Sort(dimensionVector(0), length, stream, device));
    resultSize = static_cast<int>(check(lib->Reduce(dimensionVector(0), measureVec[0], dimensionVector(1), measureVec[1], mb,
                                                    length, static_cast<AggregateFunction>(plan.aggFunc), stream, device)));
  }
  wait();
}

// ---- NonAggrBatchExecutorImpl (query/aql_nonaggr_batchexecutor.go) ----------------------------
// prepareForDimEval (:45-56): the two dimension buffers are allocated once, for the largest batch plus an eighth — and
// again when a batch arrives that is larger than what the query was told (nothing is carried over: every batch's rows
// have gone to the host)
void AresQuery::prepareForDimEval() {
  // (the batch's rows before the filters, not the survivors: Expand may repeat the survivors up to the batch's size and
  // beyond, and cuts its output at the capacity)
  const int rows = std::max(maxBatchSize, batchRows);
  if (dimVec[0] && rows + rows / 8 <= resultCapacity) return;
  maxBatchSize = rows;
  release(dimVec[0]); release(dimVec[1]);
  resultCapacity = rows + rows / 8;
  const size_t unit = std::max(layout.rowBytes, 1);
  dimVec[0] = alloc(static_cast<size_t>(resultCapacity) * unit);
  dimVec[1] = alloc(static_cast<size_t>(resultCapacity) * unit);
}
// expandDimensions (:58-74, time_series_aggregate.go:718-729)
void AresQuery::expandDimensions() {
  const int wanted = recordsNeeded();
  if (size != 0 && baseCounts) {
    calls++;
    resultSize = static_cast<int>(check(lib->Expand(dimensionVector(0), dimensionVector(1), baseCounts, indexVec, size, 0, stream, device)));
    std::swap(dimVec[0], dimVec[1]);
  } else {
    resultSize = size;
  }
  if (wanted >= 0 && resultSize > wanted) resultSize = wanted;
}
void AresQuery::projectNonAggr() {
  prepareForDimEval();
  evalDimensions(0);  // the dimensions are written from row 0, the measure is not evaluated
  expandDimensions();
  wait();
  cleanupBeforeAggregation();
}
// postExec (:76-100): the batch's rows go to the host — HostAlloc, asyncCopyDimensionVector into a vector of exactly that many
// rows, a wait — and are appended to the query's result (flushResultBuffer)
void AresQuery::postExecNonAggr() {
  const size_t n = static_cast<size_t>(resultSize), nd = layout.widths.size();
  hostSections.resize(2 * nd);
  if (n) {
    uint8_t *host = reinterpret_cast<uint8_t *>(check(lib->HostAlloc(n * static_cast<size_t>(layout.rowBytes))));
    copyDimsD2H(host, dimVec[0], resultSize, resultSize, resultCapacity);
    wait();
    const uint8_t *from = host;
    for (size_t s = 0; s < 2 * nd; s++) {
      const size_t bytes = n * (s < nd ? layout.widths[s] : 1);
      hostSections[s].insert(hostSections[s].end(), from, from + bytes);
      from += bytes;
    }
    check(lib->HostFree(host));
  }
  rowsWritten += resultSize;
  if (recordsNeeded() == 0) done = true;
  size = 0;
}

// ---- fused extensions (include/ares_extensions.h): one call per batch --------------------------
// *join (may be null: main-table columns only) receives the leaf column's join, table - 1, or -1 for the main table
bool AresQuery::fusedExpr(int nodeIdx, int outType, AresFusedExpr *e, int *join) {
  const Plan &p = *batchPlan;
  const AresPlanNode &n = p.nodes.at(nodeIdx);
  memset(e, 0, sizeof(*e));
  e->outType = static_cast<DataType>(outType);
  auto leafColumn = [&](const AresPlanNode &c, InputVector *iv) {
    if (c.kind != ARES_NODE_COLUMN || c.table < 0 || c.table > static_cast<int>(p.foreign.size())) return false;
    if (c.table != 0 && !join) return false;
    if (join) *join = c.table - 1;
    memcpy(iv, &columnInput(c, false).get(), sizeof(InputVector));
    return true;
  };
  if (n.kind == ARES_NODE_COLUMN) {
    e->arity = 1;
    e->functor = Noop;
    return leafColumn(n, &e->lhs);
  }
  if (n.kind != ARES_NODE_BINARY) return false;
  const AresPlanNode &l = p.nodes.at(n.lhs), &r = p.nodes.at(n.rhs);
  if (r.kind != ARES_NODE_CONST_INT && r.kind != ARES_NODE_CONST_FLOAT) return false;
  if (!leafColumn(l, &e->lhs)) return false;
  memcpy(&e->rhs, &constantInput(r).get(), sizeof(InputVector));
  e->arity = 2;
  e->functor = n.op;
  return true;
}
// The filters `roots` into out[0 ..) and their number into *count.  joins (where the query struct has them): the join each
// filter reads, and a filter that reads none does not fit.  false: some filter has no fusable shape.
bool AresQuery::fusedFilters(const std::vector<int> &roots, AresFusedExpr *out, int *count, int *joins) {
  *count = static_cast<int>(roots.size());
  for (size_t i = 0; i < roots.size(); i++)
    if (!fusedExpr(roots[i], Bool, &out[i], joins ? &joins[i] : nullptr) || (joins && joins[i] < 0)) return false;
  return true;
}
// The dimensions into out, each at its place in vector order, and their number into *count.  joins (where the query struct
// has them): the join each dimension reads, -1 for a main-table column.
bool AresQuery::fusedDims(AresFusedExpr *out, int *count, int *joins) {
  const Plan &p = *batchPlan;
  *count = static_cast<int>(p.dimNodes.size());
  for (size_t i = 0; i < p.dimNodes.size(); i++) {
    const int at = layout.dimVectorIndex[i];
    if (!fusedExpr(p.dimNodes[i], p.dimTypes[i], &out[at], joins ? &joins[at] : nullptr)) return false;
  }
  return true;
}

// The running batch (`columns` are bound) as the one-call extension and the hint take it; false: a plan neither fits
bool AresQuery::fusedQuery(AresFusedQuery *q) {
  const Plan &p = *batchPlan;
  if (!p.useHashReduction || p.hasGeo || p.isHLL()) return false;
  if (!p.foreign.empty() || !p.foreignFilters.empty() || baseCounts) return false;
  if (p.dimNodes.empty() || p.dimNodes.size() > 4 || p.filters.size() > 4) return false;
  if (!fusedFilters(p.filters, q->filters, &q->numFilters)) return false;
  for (int t : p.dimTypes)  // (all 4 bytes wide: vector order == query order)
    if (data_type_bytes(t) != 4) return false;
  if (!fusedDims(q->dims, &q->numDims)) return false;
  if (!fusedExpr(p.measureNode, p.measureType, &q->measure)) return false;
  q->aggFunc = static_cast<AggregateFunction>(p.aggFunc);
  return true;
}

// The batch takes the ordinary sequence: the library is told beforehand what that sequence will be (AresHintFusedBatch), so
// that it may count the last filter with the batch's fused scan.  A hint only: nothing the batch does depends on it.
void AresQuery::hintBatch() {
  if (!lib->HintFusedBatch || batchPlan->filters.empty()) return;
  Pod<AresFusedQuery> q;
  if (!fusedQuery(&*q)) return;
  lib->HintFusedBatch(&q.get(), batchRows, resultSize, batchPlan->measureBytes(), stream, device);
}

// returns false when this batch must take the ordinary sequence
bool AresQuery::runBatchFused(const VectorPartySlice *cols, int ncols, int n) {
  const Plan &p = *batchPlan;
  if (!p.useFusedExtension || fusedDeclined || !lib->FusedFilterHashReduce) return false;
  columns = cols;
  numColumns = ncols;
  Pod<AresFusedQuery> q;
  if (!fusedQuery(&*q)) return false;
  size = n;
  prepareForDimAndMeasureEval();  // result buffers sized for resultSize + n, previous results carried over
  calls++;
  CGoCallResHandle h = lib->FusedFilterHashReduce(&q.get(), n, dimensionVector(0), measureVec[0], resultSize,
                                                  dimensionVector(1), measureVec[1], stream, device);
  if (declined(h)) {
    fusedDeclined = true;
    size = 0;
    return false;
  }
  resultSize = static_cast<int>(check(h));
  wait();
  releaseInputColumns();
  swapResultBuffers();
  fusedBatches++;
  return true;
}

// The non-aggregation batch through AresFusedFilterSelect or, for a plan with foreign tables, AresFusedFilterJoinSelect
// (include/ares_extensions.h): filters, joins, foreign filters and dimensions of a batch without base counts or geo in one
// limit-aware call; no record-id vectors are allocated.  false: this batch takes the ordinary sequence.
bool AresQuery::runBatchFusedSelect(const VectorPartySlice *cols, int ncols, int n) {
  const bool joins = !plan.foreign.empty() || !plan.foreignFilters.empty();
  if (!plan.useFusedExtension || fusedDeclined || !(joins ? lib->FusedFilterJoinSelect != nullptr : lib->FusedFilterSelect != nullptr)) return false;
  if (baseCounts || plan.hasGeo) return false;
  if (plan.foreign.size() > 2 || plan.foreignFilters.size() > 4) return false;
  if (plan.dimNodes.empty() || plan.dimNodes.size() > 8 || plan.filters.size() > 4) return false;
  columns = cols;
  numColumns = ncols;
  Pod<AresFusedJoinSelect> js;
  Pod<AresFusedSelect> s;
  if (joins) {
    if (!fusedFilters(plan.filters, js->filters, &js->numFilters)) return false;
    js->numJoins = static_cast<int>(plan.foreign.size());
    for (size_t k = 0; k < plan.foreign.size(); k++) {
      memcpy(&js->joins[k].key, &columnInput(main_column(plan.foreign[k].t.joinColumn)).get(), sizeof(InputVector));
      memcpy(&js->joins[k].index, &plan.foreign[k].t.index, sizeof(CuckooHashIndex));
    }
    if (!fusedFilters(plan.foreignFilters, js->foreignFilters, &js->numForeignFilters, js->foreignFilterJoin)) return false;
    if (!fusedDims(js->dims, &js->numDims, js->dimJoin)) return false;
  } else {
    if (!fusedFilters(plan.filters, s->filters, &s->numFilters) || !fusedDims(s->dims, &s->numDims)) return false;
  }
  size = n;
  batchRows = n;
  prepareForDimEval();
  calls++;
  CGoCallResHandle h = joins ? lib->FusedFilterJoinSelect(&js.get(), n, recordsNeeded(), dimensionVector(0), stream, device)
                             : lib->FusedFilterSelect(&s.get(), n, recordsNeeded(), dimensionVector(0), stream, device);
  if (declined(h)) {
    fusedDeclined = true;
    size = 0;
    return false;
  }
  resultSize = static_cast<int>(check(h));
  wait();
  releaseInputColumns();
  postExecNonAggr();
  fusedBatches++;
  return true;
}

void AresQuery::runBatchNonAggr(const VectorPartySlice *cols, int ncols, int n, uint32_t *bc, uint32_t start) {
  if (done) {  // query/aql_processor.go:119, :185, :227: no batch runs once nothing more is wanted
    ownedColumns.clear();  // (its columns stay the caller's)
    return;
  }
  baseCounts = bc;
  if (!runBatchFusedSelect(cols, ncols, n)) {
    prepareForFiltering(cols, ncols, n, bc, start);
    preExec();
    filter();
    join();
    projectNonAggr();
    // reduce(): nothing to do
    postExecNonAggr();
  }
  swapStreams();
}

void AresQuery::runBatch(const VectorPartySlice *cols, int ncols, int n, uint32_t *bc, uint32_t start) {
  if (plan.isNonAggregation) {
    runBatchNonAggr(cols, ncols, n, bc, start);
    return;
  }
  baseCounts = bc;
  // a batch whose row-space columns were resolved runs as a join-free, geo-free batch over the rewritten plan and the
  // extended columns; whatever ends the batch puts the query's own plan back
  struct Restore {
    AresQuery &q;
    ~Restore() { q.batchPlan = &q.plan; }
  } restore{*this};
  if (resolve(cols, ncols, n)) {
    batchPlan = &rowSpace->plan;
    cols = extendedColumns.data();
    ncols = static_cast<int>(extendedColumns.size());
  }
  if (runBatchFused(cols, ncols, n)) {
    swapStreams();
    return;
  }
  prepareForFiltering(cols, ncols, n, bc, start);
  hintBatch();
  preExec();
  filter();
  join();
  project();
  reduce();
  postExec();
  swapStreams();
}

// ---- C API ---------------------------------------------------------------------------------------
extern "C" {

void *AresDriverOpen(const char *libalgorithmPath, const char *libmemPath, char *err, int errLen) {
  try {
    return new AbiLibrary(libalgorithmPath, libmemPath);
  } catch (std::exception &e) {
    set_err(err, errLen, e.what());
    return nullptr;
  }
}

void AresDriverClose(void *driver) { delete static_cast<AbiLibrary *>(driver); }

AresQuery *AresQueryCreate(void *driver, const AresQueryPlan *plan, int device, void *stream, char *err, int errLen) {
  try {
    return new AresQuery(static_cast<AbiLibrary *>(driver), *plan, device, stream);
  } catch (std::exception &e) {
    set_err(err, errLen, e.what());
    return nullptr;
  }
}

int AresQueryRunBatch(AresQuery *q, const VectorPartySlice *columns, int numColumns, int size, uint32_t *baseCounts,
                      uint32_t startRow, char *err, int errLen) {
  try {
    q->runBatch(columns, numColumns, size, baseCounts, startRow);
    return 0;
  } catch (std::exception &e) {
    // the Go host recovers the panic, frees every device buffer and fails the query
    // (query/aql_processor.go:50-64, :263-269)
    set_err(err, errLen, e.what());
    try {
      q->cleanupBeforeAggregation();
    } catch (...) {
    }
    return -1;
  }
}

// Every batch of a shard that is resident on the device, one after the other like ProcessQuery's batch loop
// (query/aql_processor.go:138-161): the host side of a whole query in ONE call, so that a harness written in an
// interpreted language adds nothing between batches (bench.py's timed region: one call per step).
int AresQueryRunResidentBatches(AresQuery *q, const VectorPartySlice *columns, int numColumns, const int *sizes, int numBatches,
                                char *err, int errLen) {
  for (int b = 0; b < numBatches; b++) {
    q->ownedColumns.clear();
    q->isLastBatch = false;
    const int rc = AresQueryRunBatch(q, columns + static_cast<size_t>(b) * numColumns, numColumns, sizes[b], nullptr, 0, err, errLen);
    if (rc != 0) return rc;
  }
  return 0;
}

int AresQueryResultSize(const AresQuery *q) { return q->plan.isNonAggregation ? q->rowsWritten : q->resultSize; }
int AresQueryDone(const AresQuery *q) { return q->done ? 1 : 0; }
void AresQuerySetMaxBatchSize(AresQuery *q, int rows) { q->maxBatchSize = rows > 0 ? rows : 0; }
int AresQueryResultCapacity(const AresQuery *q) { return q->resultCapacity; }
uint8_t *AresQueryDimensionVector(const AresQuery *q) { return q->dimVec[0]; }
uint8_t *AresQueryMeasureVector(const AresQuery *q) { return q->measureVec[0]; }
long AresQueryNumCalls(const AresQuery *q) { return q->calls; }
long AresQueryNumFusedBatches(const AresQuery *q) { return q->fusedBatches; }
void AresQuerySetLastBatch(AresQuery *q, int isLast) { q->isLastBatch = isLast != 0; }
void AresQuerySetSecondStream(AresQuery *q, void *stream) { q->otherStream = stream; }
void AresQueryAdoptColumns(AresQuery *q, void *const *allocations, int count) {
  q->ownedColumns.assign(allocations, allocations + count);
}
int64_t AresQueryHLLVectorSize(const AresQuery *q) { return static_cast<int64_t>(q->hllVectorSize); }

int AresQueryFetchHLL(AresQuery *q, uint16_t *regCounts, uint8_t *hllVector, char *err, int errLen) {
  try {
    const int n = q->resultSize;
    if (n && q->hllDimRegIDCount) q->d2h(regCounts, q->hllDimRegIDCount, static_cast<size_t>(n) * 2);
    if (n && q->hllVector) q->d2h(hllVector, q->hllVector, q->hllVectorSize);
    q->wait();
    return 0;
  } catch (std::exception &e) {
    set_err(err, errLen, e.what());
    return -1;
  }
}

int AresQueryFetch(AresQuery *q, uint8_t *dims, uint8_t *measures, char *err, int errLen) {
  try {
    if (q->plan.isNonAggregation) {  // the rows are on the host already: dimension values in vector order, then validity bytes
      uint8_t *out = dims;
      for (const std::vector<uint8_t> &v : q->hostSections) out = std::copy(v.begin(), v.end(), out);
      return 0;
    }
    const int n = q->resultSize;
    // asyncCopyDimensionVector to the host (query/aql_processor.go:641-671): the host layout uses resultSize as its capacity
    q->copyDimsD2H(dims, q->dimVec[0], n, n, q->resultCapacity);
    if (n && measures) q->d2h(measures, q->measureVec[0], static_cast<size_t>(n) * q->plan.measureBytes());
    q->wait();
    return 0;
  } catch (std::exception &e) {
    set_err(err, errLen, e.what());
    return -1;
  }
}

void AresQueryDestroy(AresQuery *q) {
  if (!q) return;
  try {
    q->cleanupBeforeAggregation();
    q->releaseAll();
  } catch (...) {
  }
  delete q;
}

}  // extern "C"
