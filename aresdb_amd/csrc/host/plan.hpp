// The query as the host holds it, and the layout of its dimension vector:
//   Plan                   <- the OOPK context's expression trees and flags (query/aql_context.go:148-150, :421-424)
//   DimLayout              <- DimCountsPerDimWidth + the dimension order (query/aql_compiler.go:1341-1362, query/common/dim_util.go)
//   copy_dimension_vector  <- asyncCopyDimensionVector (query/aql_processor.go:641-671)
#pragma once

#include <algorithm>
#include <vector>

#include "abi_library.hpp"

namespace ares_host {

constexpr int kDimWidths[NUM_DIM_WIDTH] = {16, 8, 4, 2, 1};

inline int data_type_bytes(int t) {
  switch (t) {
    case Bool: case Int8: case Uint8: return 1;
    case Int16: case Uint16: return 2;
    case Int32: case Uint32: case Float32: return 4;
    case Int64: case Uint64: case Float64: case GeoPoint: return 8;
    case UUID: return 16;
    default: throw AbiError("unknown data type");
  }
}

// a zeroed node that is main-table column `column`
inline AresPlanNode main_column(int column) {
  AresPlanNode n;
  memset(&n, 0, sizeof(n));
  n.kind = ARES_NODE_COLUMN;
  n.column = column;
  return n;
}

struct Plan {
  std::vector<AresPlanNode> nodes;
  std::vector<int> filters, foreignFilters, dimNodes, dimTypes;
  int measureNode, aggFunc, measureType;
  bool useHashReduction;
  bool useFusedExtension;
  // a non-aggregation query (SELECT cols WHERE ... LIMIT n: the measure is a number literal, query/aql_compiler.go:1147-1153)
  bool isNonAggregation;
  int limit;  // < 0: none
  struct Foreign {
    AresForeignTable t;
    std::vector<VectorPartySlice> slices;
    std::vector<int> dataTypes;
  };
  std::vector<Foreign> foreign;
  bool hasGeo = false;
  AresGeoIntersection geo;
  // local-time bucketing: the int16 offset table on the device and, per node, whether it is a CONVERT_TZ node — the foreign
  // leaves directly below one are read through the table (query/time_series_aggregate.go:506-516)
  const int16_t *timezoneLookup = nullptr;
  int timezoneLookupSize = 0;
  std::vector<char> convertTz;
  bool isConvertTz(int node) const { return node >= 0 && node < static_cast<int>(convertTz.size()) && convertTz[node]; }

  explicit Plan(const AresQueryPlan &p)
      : nodes(p.nodes, p.nodes + p.numNodes), filters(p.filters, p.filters + p.numFilters),
        foreignFilters(p.foreignFilters, p.foreignFilters + p.numForeignFilters),
        dimNodes(p.dimNodes, p.dimNodes + p.numDims), dimTypes(p.dimTypes, p.dimTypes + p.numDims),
        measureNode(p.measureNode), aggFunc(p.aggFunc), measureType(p.measureType),
        useHashReduction(p.useHashReduction != 0), useFusedExtension(p.useFusedExtension != 0),
        isNonAggregation(p.isNonAggregation != 0), limit(p.limit) {
    for (int i = 0; i < p.numForeignTables; i++) {
      Foreign f;
      f.t = p.foreignTables[i];
      f.slices.assign(f.t.slices, f.t.slices + static_cast<size_t>(f.t.numColumns) * f.t.numBatches);
      f.dataTypes.assign(f.t.dataTypes, f.t.dataTypes + f.t.numColumns);
      foreign.push_back(std::move(f));
    }
    memset(&geo, 0, sizeof(geo));
    if (p.geo) {
      hasGeo = true;
      geo = *p.geo;
    }
    timezoneLookup = p.timezoneLookup;
    timezoneLookupSize = p.timezoneLookupSize;
    convertTz.assign(nodes.size(), 0);
    for (int i = 0; i < p.numConvertTzNodes; i++) {
      const int node = p.convertTzNodes[i];
      if (node < 0 || node >= p.numNodes || nodes[node].kind != ARES_NODE_BINARY) throw AbiError("a CONVERT_TZ node must be a binary node");
      convertTz[node] = 1;
    }
  }
  int measureBytes() const { return data_type_bytes(measureType); }
  bool isHLL() const { return aggFunc == AGGR_HLL; }  // OOPKContext.IsHLL, query/aql_context.go:421-424
  int geoWords() const { return (geo.numShapes + 31) / 32; }
};

// A dimension vector of capacity C: the values of every dimension, widest first (C * width bytes each), then one validity
// byte vector of C bytes per dimension in the same order.  Built once per query: neither row-space rewrite changes a width.
struct DimLayout {
  uint8_t ndw[NUM_DIM_WIDTH] = {0, 0, 0, 0, 0};  // DimCountsPerDimWidth
  std::vector<int> widths;                        // in vector order
  std::vector<int> dimVectorIndex;                // query dimension -> position in the width-ordered vector
  int rowBytes = 0;                               // of one row: its values and one validity byte per dimension

  // query/aql_compiler.go:1341-1362: dimensions ordered by width 16..1, then query order
  explicit DimLayout(const std::vector<int> &dimTypes) : dimVectorIndex(dimTypes.size(), 0) {
    const int n = static_cast<int>(dimTypes.size());
    std::vector<int> order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return data_type_bytes(dimTypes[a]) > data_type_bytes(dimTypes[b]); });
    for (int p = 0; p < n; p++) {
      const int w = data_type_bytes(dimTypes[order[p]]);
      dimVectorIndex[order[p]] = p;
      widths.push_back(w);
      rowBytes += w + 1;
      for (int k = 0; k < NUM_DIM_WIDTH; k++)
        if (kDimWidths[k] == w) ndw[k]++;
    }
  }
  int numDims() const { return static_cast<int>(widths.size()); }
  // query/common/dim_util.go: (value offset, validity offset) of the dimension at position `dim` of the vector
  void offsets(int dim, int64_t capacity, int64_t *valueOff, int64_t *nullOff) const {
    int64_t before = 0;
    for (int d = 0; d < dim; d++) before += widths[d];
    *valueOff = before * capacity;
    *nullOff = static_cast<int64_t>(rowBytes - numDims()) * capacity + static_cast<int64_t>(dim) * capacity;
  }
};

// asyncCopyDimensionVector: `length` rows of every dimension from the vector at `from` (capacity fromCapacity) to rows
// [offset, offset + length) of the vector at `to` (capacity toCapacity) — the value copies of every dimension, then the
// validity copies, each through copy(dst, src, bytes).  Nothing is copied for no rows.  fromOffset is not in the Go function:
// the partitioned merge packs a slice of its table.
template <typename Copy>
void copy_dimension_vector(const DimLayout &layout, uint8_t *to, uint8_t *from, int64_t length, int64_t offset,
                           int64_t toCapacity, int64_t fromCapacity, Copy &&copy, int64_t fromOffset = 0) {
  if (length <= 0) return;
  for (int pass = 0; pass < 2; pass++)
    for (int d = 0; d < layout.numDims(); d++) {
      int64_t tv, tn, fv, fn;
      layout.offsets(d, toCapacity, &tv, &tn);
      layout.offsets(d, fromCapacity, &fv, &fn);
      const int64_t w = layout.widths[d];
      if (pass == 0) copy(to + tv + offset * w, from + fv + fromOffset * w, static_cast<size_t>(length * w));
      else copy(to + tn + offset, from + fn + fromOffset, static_cast<size_t>(length));
    }
}

}  // namespace ares_host
