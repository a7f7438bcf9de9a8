// What the direct flavours of the row-space joins share (local_time.hip, join_columns.hip): a key column of a 1- or 2-byte type
// has at most 65 536 stored values, so every value is probed once into a table and the rows stream through it, four rows per
// lane.  Here: a stored value widened as the probe takes it, four rows' keys and validity bits in one load each, and a
// wavefront's four ballots put together into the validity words of its 256 rows.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_model.hpp"

namespace ares {

// Stored key value v (the low 8 * step bits) as cuckoo_load_key / load32 widen a row's: the column's kind decides sign
// extension; cuckoo_probe keeps keyBytes of it.
__device__ __forceinline__ uint32_t widen_stored_key(int kind, int step, uint32_t v) {
  if (kind != K_I32) return v;
  return step == 2 ? static_cast<uint32_t>(static_cast<int32_t>(static_cast<int16_t>(v)))
                   : static_cast<uint32_t>(static_cast<int32_t>(static_cast<int8_t>(v)));
}

struct __attribute__((packed, aligned(4))) Words4 { uint32_t v[4]; };
struct __attribute__((packed, aligned(2))) Halves4 { uint16_t v[4]; };

// validity bits first .. first + 3 of a bitmap
__device__ __forceinline__ uint32_t four_bits(const uint8_t *nulls, uint32_t first) {
  const uint32_t at = first >> 3, shift = first & 7;
  uint32_t w = nulls[at];
  if (shift > 4) w |= static_cast<uint32_t>(nulls[at + 1]) << 8;  // (only then: nothing is read past the bits asked for)
  return (w >> shift) & 15u;
}

// bit k of the low 16 bits to bit 4 * k
__device__ __forceinline__ unsigned long long spread4(unsigned long long x) {
  x = (x | (x << 24)) & 0x000000ff000000ffull;
  x = (x | (x << 12)) & 0x000f000f000f000full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  x = (x | (x << 3)) & 0x1111111111111111ull;
  return x;
}

}  // namespace ares
