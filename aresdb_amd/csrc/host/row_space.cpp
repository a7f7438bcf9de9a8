// Row-space rewrites: columns an extension resolves once per batch, behind the batch's own, and the plan that reads them.  The
// Go host has no counterpart; the contracts are at AresQuerySetJoinColumns / AresQuerySetGeoColumn (ares_driver.h) and at
// AresJoinColumnsRun / AresLocalTimeColumnRun / AresGeoShapeColumnRun (include/ares_extensions.h).
//
// A query holds at most one rewrite — joined columns need foreign tables, the geo column needs none — and both follow one
// protocol per batch (resolve): they differ in their once-per-query planner and in the body that fills the extension's query
// struct and calls it.
#include <algorithm>

#include "query.hpp"

using namespace ares_host;

namespace {

// Joined columns: an aggregation query whose foreign references are all leaf columns of 1-, 2- or 4-byte non-Bool types gets the
// plan with every such leaf turned into a main-table column, the foreign filters appended to the main filters and no foreign
// tables.  Null: not eligible.
//
// A CONVERT_TZ node (Plan::convertTz) is one resolved leaf of its own, local time: eligible when it is an inner node whose lhs is
// a bare main-table column and whose rhs is a foreign leaf of type Uint8 or Uint16, the plan has an offset table and the node's
// outType — the type of the scratch vector it would fill — is Uint32 or Int32.  The walk does not descend into it, so a table
// that only zone columns read has no joined column; the node becomes a main-table column behind the joined ones, identical
// (time column, table, zone column, type) sharing one.  Any other CONVERT_TZ node — a root, whose result type the operands'
// types decide, among them — or more than two distinct local times: not eligible.
std::unique_ptr<RowSpace> plan_joined_columns(const Plan &plan, const AbiLibrary &lib) {
  if (plan.isNonAggregation || plan.foreign.empty() || !lib.JoinColumnsRun || !lib.JoinColumnBytes) return nullptr;
  if (plan.hasGeo && plan.geo.pointTable != 0) return nullptr;  // a geo point from a foreign table
  const int numNodes = static_cast<int>(plan.nodes.size());
  std::vector<char> reached(plan.nodes.size(), 0);
  std::vector<RowSpace::LocalTime> localTimes;
  std::vector<std::pair<int, size_t>> localTimeNodes;  // (node, position inside localTimes)
  bool ok = true;
  // the local time a CONVERT_TZ node stands for; false: no eligible shape
  auto local_time = [&](const AresPlanNode &n, bool isRoot, RowSpace::LocalTime *lt) {
    if (isRoot || !lib.LocalTimeColumnRun || !plan.timezoneLookup) return false;
    if (n.outType != Uint32 && n.outType != Int32) return false;
    if (n.lhs < 0 || n.lhs >= numNodes || n.rhs < 0 || n.rhs >= numNodes) return false;
    const AresPlanNode &time = plan.nodes[n.lhs], &zone = plan.nodes[n.rhs];
    if (time.kind != ARES_NODE_COLUMN || time.table != 0 || zone.kind != ARES_NODE_COLUMN) return false;
    if (zone.table < 1 || zone.table > static_cast<int>(plan.foreign.size())) return false;
    const Plan::Foreign &ft = plan.foreign[zone.table - 1];
    if (zone.column < 0 || zone.column >= ft.t.numColumns) return false;
    if (ft.dataTypes[zone.column] != Uint8 && ft.dataTypes[zone.column] != Uint16) return false;
    *lt = RowSpace::LocalTime{time.column, zone.table - 1, zone.column, n.outType};
    return true;
  };
  // marks what `root` reaches; a foreign leaf below a main-table filter makes the query ineligible
  auto walk = [&](int root, bool foreignAllowed, bool isRoot, auto &&self) -> void {
    if (root < 0 || root >= numNodes) {
      ok = false;
      return;
    }
    const AresPlanNode &n = plan.nodes[root];
    reached[root] = 1;
    if (plan.isConvertTz(root)) {
      RowSpace::LocalTime lt;
      if (!foreignAllowed || !local_time(n, isRoot, &lt)) {
        ok = false;
        return;
      }
      const size_t at = std::find(localTimes.begin(), localTimes.end(), lt) - localTimes.begin();
      if (at == localTimes.size()) localTimes.push_back(lt);
      localTimeNodes.emplace_back(root, at);
      return;
    }
    if (n.kind == ARES_NODE_COLUMN && n.table != 0 && !foreignAllowed) ok = false;
    if (n.kind == ARES_NODE_UNARY || n.kind == ARES_NODE_BINARY) self(n.lhs, foreignAllowed, false, self);
    if (n.kind == ARES_NODE_BINARY) self(n.rhs, foreignAllowed, false, self);
  };
  for (int f : plan.filters) walk(f, false, true, walk);
  for (int f : plan.foreignFilters) walk(f, true, true, walk);
  for (size_t i = 0; i < plan.dimNodes.size(); i++)
    if (!(plan.hasGeo && plan.geo.dimIndex == static_cast<int>(i))) walk(plan.dimNodes[i], true, true, walk);
  walk(plan.measureNode, true, true, walk);
  if (!ok || localTimes.size() > 2) return nullptr;
  std::unique_ptr<RowSpace> rs(new RowSpace(RowSpace::JOIN_COLUMNS, plan));
  rs->tables.assign(plan.foreign.size(), RowSpace::JoinedTable());
  std::vector<std::pair<int, size_t>> leaves;  // (node, position inside its table's list)
  for (int i = 0; i < numNodes; i++) {
    const AresPlanNode &n = plan.nodes[i];
    if (!reached[i] || n.kind != ARES_NODE_COLUMN || n.table == 0) continue;
    if (n.table < 0 || n.table > static_cast<int>(plan.foreign.size())) return nullptr;
    const Plan::Foreign &ft = plan.foreign[n.table - 1];
    if (n.column < 0 || n.column >= ft.t.numColumns) return nullptr;
    const int t = ft.dataTypes[n.column];
    if (!(t == Int8 || t == Uint8 || t == Int16 || t == Uint16 || t == Int32 || t == Uint32 || t == Float32)) return nullptr;
    std::vector<int> &list = rs->tables[n.table - 1].columns;
    size_t at = std::find(list.begin(), list.end(), n.column) - list.begin();
    if (at == list.size()) list.push_back(n.column);
    if (list.size() > 4) return nullptr;
    leaves.emplace_back(i, at);
  }
  for (RowSpace::JoinedTable &jt : rs->tables) {
    jt.first = rs->numAdded;
    rs->numAdded += static_cast<int>(jt.columns.size());
  }
  for (const auto &leaf : leaves) {
    AresPlanNode &n = rs->plan.nodes[leaf.first];
    rs->leaves.emplace_back(leaf.first, rs->tables[n.table - 1].first + static_cast<int>(leaf.second));
    n.table = 0;  // (its column is the batch's column count + the position: set per batch)
  }
  for (const auto &node : localTimeNodes) {
    rs->plan.nodes[node.first] = main_column(0);
    rs->plan.convertTz[node.first] = 0;
    rs->leaves.emplace_back(node.first, rs->numAdded + static_cast<int>(node.second));
  }
  rs->localTimes = localTimes;
  rs->numAdded += static_cast<int>(localTimes.size());
  rs->plan.filters.insert(rs->plan.filters.end(), plan.foreignFilters.begin(), plan.foreignFilters.end());
  rs->plan.foreignFilters.clear();
  rs->plan.foreign.clear();
  return rs;
}

// The geofence verdict: an aggregation query with a geo intersection over a main-table point column and no foreign tables gets
// the plan without geo, with one more filter `shape column < 128` (true for every valid value, null for a null one) and the geo
// dimension, if there is one, as the bare column.  Null: not eligible.
std::unique_ptr<RowSpace> plan_geo_column(const Plan &plan, const AbiLibrary &lib) {
  if (plan.isNonAggregation || !plan.hasGeo || !lib.GeoShapeColumnRun || !lib.GeoShapeColumnBytes) return nullptr;
  if (plan.geo.pointTable != 0 || !plan.geo.shapeLatLongs) return nullptr;
  if (!plan.foreign.empty() || !plan.foreignFilters.empty()) return nullptr;
  const int dim = plan.geo.dimIndex;
  if (dim >= 0 && !plan.geo.inOrOut) return nullptr;  // (every kept row is outside every shape: the reference writes no dimension row)
  if (dim >= static_cast<int>(plan.dimNodes.size())) return nullptr;
  if (dim >= 0 && data_type_bytes(plan.dimTypes[dim]) != 1) return nullptr;  // (the shape number lives in a 1-byte slot)
  std::unique_ptr<RowSpace> rs(new RowSpace(RowSpace::GEO_COLUMN, plan));
  Plan &g = rs->plan;
  g.hasGeo = false;
  const int leaf = static_cast<int>(g.nodes.size());
  AresPlanNode bound, less;
  memset(&bound, 0, sizeof(bound));
  bound.kind = ARES_NODE_CONST_INT;
  bound.ival = 128;
  memset(&less, 0, sizeof(less));
  less.kind = ARES_NODE_BINARY;
  less.op = LessThan;
  less.lhs = leaf;
  less.rhs = leaf + 1;
  less.outType = Bool;
  g.nodes.push_back(main_column(0));  // (its column is the batch's column count: set per batch)
  g.nodes.push_back(bound);
  g.nodes.push_back(less);
  g.filters.push_back(leaf + 2);
  if (dim >= 0) {
    g.dimNodes[dim] = leaf;
    g.dimTypes[dim] = Uint8;
  }
  rs->leaves.emplace_back(leaf, 0);
  rs->numAdded = 1;
  return rs;
}

}  // namespace

// on: plan this kind, or leave what is there (the other kind's rewrite, or nothing); off: drop only one's own kind
void AresQuery::setRowSpace(RowSpace::Kind kind, bool on) {
  if (rowSpace && rowSpace->kind == kind) rowSpace.reset();
  if (!on) return;
  std::unique_ptr<RowSpace> rs = kind == RowSpace::JOIN_COLUMNS ? plan_joined_columns(plan, *lib) : plan_geo_column(plan, *lib);
  if (rs) rowSpace = std::move(rs);
}

// pruning hints: the main-table filters of the leaf-versus-constant shape, at most four; returns their number
int AresQuery::pruningHints(AresFusedExpr *out) {
  int n = 0;
  for (int f : plan.filters)
    if (n < 4 && fusedExpr(f, Bool, &out[n]) && out[n].arity == 2) n++;
  return n;
}

// One AresJoinColumnsRun per foreign table the query reads, into fresh allocations.  false: the library declines the shape.
bool AresQuery::runJoinColumns(RowSpace &rs, int n) {
  for (size_t k = 0; k < rs.tables.size(); k++) {
    const RowSpace::JoinedTable &jt = rs.tables[k];
    if (jt.columns.empty()) continue;
    Pod<AresJoinColumns> q;
    q->numFilters = pruningHints(q->filters);
    memcpy(&q->join.key, &columnInput(main_column(plan.foreign[k].t.joinColumn)).get(), sizeof(InputVector));
    memcpy(&q->join.index, &plan.foreign[k].t.index, sizeof(CuckooHashIndex));
    q->numColumns = static_cast<int>(jt.columns.size());
    for (size_t c = 0; c < jt.columns.size(); c++) {
      AresPlanNode leaf = main_column(jt.columns[c]);
      leaf.table = static_cast<int>(k) + 1;
      memcpy(&q->columns[c].column, &columnInput(leaf, false).get(), sizeof(InputVector));
      joinedOutputs.push_back(alloc(lib->JoinColumnBytes(n, static_cast<DataType>(plan.foreign[k].dataTypes[leaf.column]))));
      q->columns[c].out = static_cast<uint8_t *>(joinedOutputs.back());
    }
    calls++;
    CGoCallResHandle h = lib->JoinColumnsRun(&q.get(), n, &extendedColumns[static_cast<size_t>(numColumns + jt.first)], stream, device);
    if (declined(h)) return false;
    check(h);
  }
  return runLocalTimeColumns(rs, n);
}

// One AresLocalTimeColumnRun per local time of the query, into fresh allocations behind the joined columns.  false: the library
// declines the shape.
bool AresQuery::runLocalTimeColumns(RowSpace &rs, int n) {
  const int first = rs.numAdded - static_cast<int>(rs.localTimes.size());
  for (size_t k = 0; k < rs.localTimes.size(); k++) {
    const RowSpace::LocalTime &lt = rs.localTimes[k];
    const Plan::Foreign &ft = plan.foreign[lt.table];
    Pod<AresLocalTimeColumn> q;
    q->numFilters = pruningHints(q->filters);
    memcpy(&q->time, &columnInput(main_column(lt.timeColumn)).get(), sizeof(InputVector));
    memcpy(&q->join.key, &columnInput(main_column(ft.t.joinColumn)).get(), sizeof(InputVector));
    memcpy(&q->join.index, &ft.t.index, sizeof(CuckooHashIndex));
    AresPlanNode zone = main_column(lt.zoneColumn);
    zone.table = lt.table + 1;
    memcpy(&q->zone, &columnInput(zone, false, true).get(), sizeof(InputVector));
    q->outType = static_cast<DataType>(lt.outType);
    joinedOutputs.push_back(alloc(lib->JoinColumnBytes(n, Uint32)));
    q->out = static_cast<uint8_t *>(joinedOutputs.back());
    calls++;
    CGoCallResHandle h = lib->LocalTimeColumnRun(&q.get(), n, &extendedColumns[static_cast<size_t>(numColumns + first) + k], stream, device);
    if (declined(h)) return false;
    check(h);
  }
  return true;
}

// One AresGeoShapeColumnRun into a fresh allocation.  false: the library declines the shape.
bool AresQuery::runGeoColumn(int n) {
  Pod<AresGeoShapeColumn> q;
  q->numFilters = pruningHints(q->filters);
  q->shapes.LatLongs = const_cast<uint8_t *>(plan.geo.shapeLatLongs);
  q->shapes.TotalNumPoints = plan.geo.totalNumPoints;
  q->shapes.TotalWords = static_cast<uint8_t>(plan.geoWords());
  memcpy(&q->points, &columnInput(main_column(plan.geo.pointColumn)).get(), sizeof(InputVector));
  q->inOrOut = plan.geo.inOrOut;
  joinedOutputs.push_back(alloc(lib->GeoShapeColumnBytes(n)));
  q->out = static_cast<uint8_t *>(joinedOutputs.back());
  calls++;
  CGoCallResHandle h = lib->GeoShapeColumnRun(&q.get(), n, &extendedColumns[static_cast<size_t>(numColumns)], stream, device);
  if (declined(h)) return false;
  check(h);
  return true;
}

// The per-batch protocol, entered with the query's own plan as the batch's: extendedColumns = the batch's columns + the
// resolved ones, their allocations in joinedOutputs (released with the batch's input columns, also when a call failed).
// false: this batch takes the original plan — base counts, no rows, or a decline, after which the query stops asking.
bool AresQuery::resolve(const VectorPartySlice *cols, int ncols, int n) {
  if (!rowSpace || rowSpaceDeclined || baseCounts || n <= 0) return false;
  RowSpace &rs = *rowSpace;
  columns = cols;
  numColumns = ncols;
  extendedColumns.assign(cols, cols + ncols);
  extendedColumns.resize(static_cast<size_t>(ncols + rs.numAdded));
  const bool resolved = rs.kind == RowSpace::JOIN_COLUMNS ? runJoinColumns(rs, n) : runGeoColumn(n);
  foreignSliceArrays.clear();  // (the callee has copied the batch descriptors)
  if (!resolved) {
    rowSpaceDeclined = true;
    for (void *p : joinedOutputs) release(p);
    joinedOutputs.clear();
    return false;
  }
  for (const auto &leaf : rs.leaves) rs.plan.nodes[leaf.first].column = ncols + leaf.second;
  return true;
}

extern "C" {
void AresQuerySetJoinColumns(AresQuery *q, int on) { q->setRowSpace(RowSpace::JOIN_COLUMNS, on != 0); }
void AresQuerySetGeoColumn(AresQuery *q, int on) { q->setRowSpace(RowSpace::GEO_COLUMN, on != 0); }
}
