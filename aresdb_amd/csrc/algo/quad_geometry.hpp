// Quad and tile geometry of the hot-shape kernels: the __device__ loaders that the kernels of deferral_kernels.hpp
// (launched by deferral.hip) and of transform_kernels.hpp (launched by transform.hip) share, and the host-visible types
// and constants of those kernels that the deferral state (deferral.hpp) is built from.  No __global__ lives here.
#pragma once

#include <hip/hip_runtime.h>

#include "binding.hpp"
#include "common.hpp"
#include "device_model.hpp"
#include "fast_eval.hpp"

namespace ares {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTQ = 4;  // quads per lane per tile: 16 rows per lane, 4096 rows per workgroup tile
constexpr int kPQ = 4;                        // quads per lane per tile
constexpr int kPTile = kBlock * 4 * kPQ;      // 4096 rows
constexpr int kTilesPerTicket = 4;

// ---------------------------------------------------------------------------------------------
// Quad geometry shared by the fast transform / filter kernels
// ---------------------------------------------------------------------------------------------
// Every lane owns QUADS groups of 4 CONSECUTIVE output positions, so the index vector is read and
// the outputs are written 16 bytes per lane per instruction (1 KiB per wavefront instruction), and
// the operand column is read 16 bytes per lane wherever the four rows are consecutive (always for a
// fresh index vector, mostly for a lightly filtered one).  gfx950 global accesses only need dword
// alignment, hence the 4-byte aligned vector types.  Quad k covers positions [4k - pad, 4k - pad + 4)
// with pad = (address of the 1-byte-per-position output) & 3, so that the validity / predicate
// bytes of a quad form one aligned dword.

// Loads rows / values / validity of QUADS quads per lane; positions outside [0, n) get ok = 0.
// Three phases so that every load of the tile is in flight before the first one is consumed:
// (A) index vector, (B) values + one 16-bit window of the validity bitmap per quad, (C) bit
// extraction.  The window starts at the byte holding the first row's bit and covers at least the 8
// following rows, which is where the other three rows of a filtered quad almost always lie; a
// wider quad re-reads single bytes.  Reading one byte past the bitmap is safe: in a mode-2 slice
// the values follow the bitmap inside the same allocation.
template <int QUADS>
__device__ __forceinline__ void load_rows(const uint32_t *idx, int pad, int64_t quad0, int n, uint32_t (&rows)[QUADS][4]) {
#pragma unroll
  for (int q = 0; q < QUADS; q++) {
    const int64_t i0 = (quad0 + static_cast<int64_t>(q) * kBlock) * 4 - pad;
    if (i0 >= 0 && i0 + 3 < n) {
      if (idx) {
        const U32x4 r = *reinterpret_cast<const U32x4 *>(idx + i0);
#pragma unroll
        for (int j = 0; j < 4; j++) rows[q][j] = r.v[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) rows[q][j] = static_cast<uint32_t>(i0) + j;
      }
    } else {
      // ragged quad: positions outside [0, n) read row 0 (always a valid row) and are masked later
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int64_t i = i0 + j;
        rows[q][j] = (i >= 0 && i < n) ? (idx ? idx[i] : static_cast<uint32_t>(i)) : 0u;
      }
    }
  }
}

struct __attribute__((packed, aligned(1))) PU32x2 { uint32_t v[2]; };
struct __attribute__((packed, aligned(1))) PU32s1 { uint32_t v; };
template <int QUADS>
__device__ __forceinline__ void issue_values(const FastOperands &f, const uint32_t (&rows)[QUADS][4], uint32_t (&vals)[QUADS][4],
                                             uint32_t (&window)[QUADS]) {
#pragma unroll
  for (int q = 0; q < QUADS; q++) {
    const uint32_t r0 = rows[q][0];
    if (f.step == 2) {  // Int16 / Uint16 / BigEnum: 8 bytes hold the four rows of a consecutive quad (wave-uniform branch)
      const uint16_t *v16 = reinterpret_cast<const uint16_t *>(f.vals);
      uint32_t raw[4];
      if (rows[q][1] == r0 + 1 && rows[q][2] == r0 + 2 && rows[q][3] == r0 + 3) {
        const PU32x2 v = *reinterpret_cast<const PU32x2 *>(v16 + r0);
        raw[0] = v.v[0] & 0xFFFFu; raw[1] = v.v[0] >> 16; raw[2] = v.v[1] & 0xFFFFu; raw[3] = v.v[1] >> 16;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) raw[j] = v16[rows[q][j]];
      }
#pragma unroll
      for (int j = 0; j < 4; j++) vals[q][j] = f.akind == K_I32 ? static_cast<uint32_t>(static_cast<int32_t>(static_cast<int16_t>(raw[j]))) : raw[j];
    } else if (f.step == 1) {  // Int8 / Uint8 / SmallEnum
      const uint8_t *v8 = reinterpret_cast<const uint8_t *>(f.vals);
      uint32_t raw[4];
      if (rows[q][1] == r0 + 1 && rows[q][2] == r0 + 2 && rows[q][3] == r0 + 3) {
        const uint32_t v = reinterpret_cast<const PU32s1 *>(v8 + r0)->v;
        raw[0] = v & 0xFFu; raw[1] = (v >> 8) & 0xFFu; raw[2] = (v >> 16) & 0xFFu; raw[3] = v >> 24;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) raw[j] = v8[rows[q][j]];
      }
#pragma unroll
      for (int j = 0; j < 4; j++) vals[q][j] = f.akind == K_I32 ? static_cast<uint32_t>(static_cast<int32_t>(static_cast<int8_t>(raw[j]))) : raw[j];
    } else if (rows[q][1] == r0 + 1 && rows[q][2] == r0 + 2 && rows[q][3] == r0 + 3) {
      if (f.streaming) {  // a column that is read once (set by run_filter_rows)
        typedef uint32_t V4 __attribute__((ext_vector_type(4)));
        typedef V4 V4a __attribute__((aligned(4)));
        const V4 v = __builtin_nontemporal_load(reinterpret_cast<const V4a *>(f.vals + r0));
        vals[q][0] = v.x; vals[q][1] = v.y; vals[q][2] = v.z; vals[q][3] = v.w;
      } else {
        const U32x4 v = *reinterpret_cast<const U32x4 *>(f.vals + r0);
#pragma unroll
        for (int j = 0; j < 4; j++) vals[q][j] = v.v[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) vals[q][j] = f.vals[rows[q][j]];
    }
    window[q] = 0xFFFFu;
    if (f.nulls) window[q] = reinterpret_cast<const PU16 *>(f.nulls + ((r0 + f.bitOff) >> 3))->v;
  }
}

template <int QUADS>
__device__ __forceinline__ void extract_valid(const FastOperands &f, int pad, int64_t quad0, int n,
                                              const uint32_t (&rows)[QUADS][4], const uint32_t (&window)[QUADS],
                                              uint32_t (&okb)[QUADS]) {
#pragma unroll
  for (int q = 0; q < QUADS; q++) {
    const int64_t i0 = (quad0 + static_cast<int64_t>(q) * kBlock) * 4 - pad;
    const uint32_t first = (rows[q][0] + f.bitOff) & ~7u;  // bit position of the window's bit 0
    if (i0 >= 0 && i0 + 3 < n && rows[q][3] - rows[q][0] == 3u && rows[q][1] - rows[q][0] == 1u &&
        rows[q][2] - rows[q][0] == 2u) {
      // four consecutive rows inside the batch: their bits are contiguous in the 16-bit window
      okb[q] = (window[q] >> ((rows[q][0] + f.bitOff) & 7u)) & 0xFu;
      continue;
    }
    okb[q] = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int64_t i = i0 + j;
      if (i < 0 || i >= n) continue;
      const uint32_t off = rows[q][j] + f.bitOff - first;  // wraps to a huge value when the row precedes the window
      uint32_t bit;
      if (off < 16u) bit = (window[q] >> off) & 1u;
      else bit = f.nulls ? get_bit(f.nulls, rows[q][j] + f.bitOff) : 1u;
      okb[q] |= bit << j;
    }
  }
}

template <int QUADS>
__device__ __forceinline__ void load_values(const FastOperands &f, int pad, int64_t quad0, int n,
                                            const uint32_t (&rows)[QUADS][4], uint32_t (&vals)[QUADS][4],
                                            uint32_t (&okb)[QUADS]) {
  uint32_t window[QUADS];
  issue_values<QUADS>(f, rows, vals, window);
  extract_valid<QUADS>(f, pad, quad0, n, rows, window, okb);
}

template <int QUADS>
__device__ __forceinline__ void load_quads(const FastOperands &f, int64_t quad0, int n, uint32_t (&rows)[QUADS][4],
                                           uint32_t (&vals)[QUADS][4], uint32_t (&okb)[QUADS]) {
  load_rows<QUADS>(f.idx, f.pad, quad0, n, rows);
  load_values<QUADS>(f, f.pad, quad0, n, rows, vals, okb);
}

constexpr int kMaxMultiJobs = 10;  // eight dimensions (MAX_DIMENSIONS) + the measure + one to spare
struct MultiJobs {
  int count;
  FastOperands f[kMaxMultiJobs];
  SinkD s[kMaxMultiJobs];
};

struct CompactWorkspace {
  unsigned int *ticket;
  uint32_t *error;
  const uint32_t *tileOffsets;
  uint32_t *loaded;  // one word per tile: its input is in registers
};

}  // namespace ares
