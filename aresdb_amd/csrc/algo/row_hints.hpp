// Pruning hints of the row-space kernels (join_columns.hip, geo_column.hip): the query's own main-table filters of the
// column-versus-constant shape, evaluated per row before the expensive part (a cuckoo probe, a polygon walk).  A row that
// fails an evaluated hint is written as (0, null); the host's own filters drop it anyway.  A hint that cannot be bound is
// ignored: fewer rows are pruned, nothing else.
#pragma once

#include <hip/hip_runtime.h>

#include <stdexcept>

#include "ares_extensions.h"
#include "binding.hpp"
#include "device_model.hpp"
#include "fast_eval.hpp"
#include "select_scan.hpp"

namespace ares {

// row `row` of a hint's column against its constant: what the row-space filters decide for it
__device__ __forceinline__ uint32_t hint_keeps(const FastOperands &f, uint32_t row) {
  const DVal x = read_stored32(reinterpret_cast<const uint8_t *>(f.vals), f.akind, f.step, row, 0);
  const uint32_t ok = f.nulls ? get_bit(f.nulls, row + f.bitOff) : 1u;
  DVal y;
  y.bits = f.bbits;
  y.ok = f.bok;
  y = cvt32(y, f.bkind, f.I);
  return compare_fast(f, x.bits, ok, y);
}

// A hint as the kernel evaluates it, or false: anything but a comparison of a mode-1/2 main-table column of a 1-, 2- or 4-byte
// type with a constant is left to the host's own filters.
inline bool bind_hint(const AresFusedExpr &e, int batchRows, hipStream_t stream, FastOperands &f) {
  if (e.arity != 2 || e.lhs.Type != VectorPartyInput || e.rhs.Type != ConstantInput) return false;
  const VectorPartySlice &vp = e.lhs.Vector.VP;
  if (!vp.BasePtr || run_length_layout(vp) || wide_type(vp.DataType) || static_cast<int64_t>(vp.Length) < batchRows) return false;
  InputVector ins[2] = {e.lhs, e.rhs};
  EvalParams p;
  CallTemps temps;  // (a main-table column and a constant upload nothing)
  try {
    build_params(ins, 2, stream, nullptr, nullptr, 0, e.functor, p, temps);
  } catch (const std::invalid_argument &) {
    return false;
  }
  if (!fast_operands(p, f, true)) return false;
  f.idx = nullptr;
  return true;
}

// the layout of a row-space column: [validity bitmap][values], each padded to a multiple of 64 bytes
inline size_t padded64(size_t bytes) { return (bytes + 63) / 64 * 64; }
inline size_t bitmap_bytes(int rows) { return padded64((static_cast<size_t>(rows > 0 ? rows : 0) + 7) / 8); }

}  // namespace ares
