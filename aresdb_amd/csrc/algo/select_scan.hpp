// Fused select scan (select_scan.hip): the non-aggregation query's filter -> dimension rows of ONE batch in a single,
// limit-aware pass over the source columns (AresFusedFilterSelect, include/ares_extensions.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fast_eval.hpp"

namespace ares {

constexpr int kSelectFilters = 4;  // AresFusedSelect::filters
constexpr int kSelectDims = 8;     // AresFusedSelect::dims (MAX_DIMENSIONS)
constexpr int kSelectBlock = 256;
constexpr int kSelectQuads = 4;                                   // quads per lane and tile
constexpr int kSelectTile = kSelectBlock * 4 * kSelectQuads;      // 4096 rows
constexpr int kSelectGridCap = 2048;

// One dimension of the plan.  width 4 / 2 / 1: `f` is the expression (column pointers included) and the slot receives what
// the transform kernels store for it; width 8 / 16: a bare column, f.vals / f.nulls / f.bitOff name it and the slot receives
// the row's stored bytes.
struct SelectDimD {
  FastOperands f;
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
  uint32_t pad[2];
};
static_assert(sizeof(SelectStateD) == 32, "the state block is cleared as a whole and the status words follow it");

struct SelectPlanD {
  int numFilters, numDims;
  FastOperands filters[kSelectFilters];
  SelectDimD dims[kSelectDims];
  int batchRows, numTiles;
  uint32_t limit;  // 0xFFFFFFFF: none
  SelectStateD *state;
  uint64_t *status;   // one look-back word per tile
  uint32_t *result;   // mapped pinned words of the calling thread: {rows, error, tiles scanned}
};

}  // namespace ares
