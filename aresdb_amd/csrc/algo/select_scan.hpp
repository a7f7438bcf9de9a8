// Fused select scan (select_scan.hip): the non-aggregation query's filter -> dimension rows of ONE batch in a single,
// limit-aware pass over the source columns (AresFusedFilterSelect, include/ares_extensions.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "ares_extensions.h"
#include "binding.hpp"
#include "cuckoo_probe.hpp"
#include "device_model.hpp"
#include "fast_eval.hpp"

namespace ares {

constexpr int kSelectFilters = 4;  // AresFusedSelect::filters
constexpr int kSelectDims = 8;     // AresFusedSelect::dims (MAX_DIMENSIONS)
constexpr int kSelectBlock = 256;
constexpr int kSelectQuads = 4;                                   // quads per lane and tile
constexpr int kSelectTile = kSelectBlock * 4 * kSelectQuads;      // 4096 rows
constexpr int kSelectGridCap = 2048;
constexpr int kSelectJoins = 2;           // AresFusedJoinSelect::joins
constexpr int kSelectForeignFilters = 4;  // AresFusedJoinSelect::foreignFilters

// One dimension of the plan.  width 4 / 2 / 1: `f` is the expression (column pointers included) and the slot receives what
// the transform kernels store for it; width 8 / 16: a bare column, f.vals / f.nulls / f.bitOff name it and the slot receives
// the row's stored bytes.  A run-length (mode 3) column: `counts` is non-null, f.vals / f.nulls are the RUN arrays (value and
// validity bit of run r at index r, bit r + f.bitOff) and row r of the batch lies in the run locate() (device_model.hpp) gives.
struct SelectDimD {
  FastOperands f;
  const uint32_t *counts;  // mode 3: counts[0 .. runs], counts[r] = first row of run r; nullptr for modes 1/2
  uint32_t runs;           // mode 3: number of runs (VectorPartySlice::Length), at least 1
  uint32_t pad;
  uint8_t *values;  // the slot's first row
  uint8_t *nulls;   // its validity bytes
  int width;        // bytes per row of the slot: 16, 8, 4, 2 or 1
  int outKind;      // width 4: kind of the stored value
};

// Words the workgroups of one launch share; zeroed before every launch.
struct SelectStateD {
  unsigned int ticket;
  uint32_t error;    // a look-back spin gave up (lookback.hpp)
  uint32_t done;     // workgroups that have left the loop
  uint32_t stop;     // some tile's inclusive prefix has reached the limit
  uint32_t total;    // inclusive prefix of the batch's last tile
  uint32_t scanned;  // tiles whose columns were read
  uint32_t rejected;  // of those: thrown away by ONE run of a mode-3 filter column that is null or fails the comparison
  uint32_t staged;    // of those: tiles that staged the run ends of some mode-3 column in LDS (several runs in the tile)
  uint32_t probed;    // join flavours: rows whose key went to the cuckoo probe
  uint32_t pad;
};
static_assert(sizeof(SelectStateD) == 40, "the state block is cleared as a whole and the status words follow it");

struct SelectPlanD {
  int numFilters, numDims;
  FastOperands filters[kSelectFilters];
  const uint32_t *filterCounts[kSelectFilters];  // mode-3 filter columns, as SelectDimD::counts / runs (FastOperands is pinned
  uint32_t filterRuns[kSelectFilters];           // at 80 bytes: the generated kernels' host code reads it)
  SelectDimD dims[kSelectDims];
  int batchRows, numTiles;
  uint32_t limit;  // 0xFFFFFFFF: none
  SelectStateD *state;
  uint64_t *status;   // one look-back word per tile
  uint32_t *result;   // mapped pinned words of the calling thread: {rows, error, tiles scanned, rejected, staged, keys probed}
};

// The joins of a plan (AresFusedFilterJoinSelect): the second argument of the join flavours of the kernel.  A joined column is
// an OP_FOREIGN operand without record ids — the tile's record ids are staged in LDS by the probe — and its expression is the
// FastOperands of a column with validity (vals / nulls unused): foreignFilters[k] here, SelectDimD::f for a dimension.
struct SelectJoinD {
  OperandD key;    // the main-table key column, modes 1/2
  CuckooD index;
  int early;       // some foreign filter reads the join: probed before ranking, for the survivors of the main-table filters;
  int pad;         // otherwise after the look-back, for the rows that are written
};

struct SelectJoinPlanD {
  int numJoins, numForeignFilters;
  SelectJoinD joins[kSelectJoins];
  FastOperands foreignFilters[kSelectForeignFilters];
  OperandD foreignFilterCols[kSelectForeignFilters];
  int foreignFilterJoin[kSelectForeignFilters];
  OperandD dimCols[kSelectDims];  // of dimensions with dimJoin[d] >= 0
  int dimJoin[kSelectDims];       // -1: a main-table dimension
};

static_assert(sizeof(SelectPlanD) + sizeof(SelectJoinPlanD) <= 4096, "the two plans are the kernel's arguments");

// ---- host side, shared with the joined columns in row space (join_columns.hip) --------------------------------------------
struct NotFusable : std::runtime_error {
  explicit NotFusable(const std::string &why) : std::runtime_error("not fusable: " + why) {}
};

inline bool wide_type(int t) { return t == Int64 || t == Uint64 || t == GeoPoint || t == UUID; }

// the run-length layout [counts][validity][values] (binding.hpp: mode 3)
inline bool run_length_layout(const VectorPartySlice &vp) { return vp.BasePtr && vp.ValuesOffset != 0 && vp.NullsOffset != 0; }

// a join's key column and index: the conditions and messages of HashLookup
inline SelectJoinD bind_join(const AresFusedJoin &j, int batchRows, hipStream_t stream, CallTemps &temps) {
  if (j.key.Type != VectorPartyInput) throw NotFusable("the join key must be a main-table column");
  const VectorPartySlice &vp = j.key.Vector.VP;
  if (!vp.BasePtr) throw NotFusable("mode 0 join key");
  if (run_length_layout(vp)) throw NotFusable("run-length join key");
  if (static_cast<int64_t>(vp.Length) < batchRows) throw NotFusable("column shorter than the batch");
  SelectJoinD J;
  memset(&J, 0, sizeof(J));
  try {
    bind_operand(j.key, true, stream, J.key, temps);
  } catch (const std::invalid_argument &bad) {
    throw NotFusable(bad.what());
  }
  if (J.key.kind == K_GEO) throw NotFusable("Unsupported data type for HashLookup");
  if (!cuckoo_geometry_ok(j.index) || !j.index.buckets) throw NotFusable("Unsupported cuckoo hash index geometry");
  J.index = make_cuckoo(j.index);
  return J;
}

}  // namespace ares
