// AresFusedFilterSelect and AresFusedFilterJoinSelect (include/ares_extensions.h): the non-aggregation query's batch — SELECT cols WHERE ... LIMIT n,
// query/aql_nonaggr_batchexecutor.go — as ONE limit-aware pass over the source columns.
//
// The per-node sequence it replaces (InitIndexVector, a filter call per comparison, a transform call per dimension) reads
// every filter column over the whole batch, compacts the survivors into an index vector and writes every survivor's
// dimension row, whatever the limit is.  Here 4096-row tiles are handed out by ticket in row order; a tile evaluates the
// filter conjunction from the columns (16 bytes per lane, 16-bit validity windows), ranks its survivors, obtains its
// exclusive prefix by the decoupled look-back of lookback.hpp and writes the survivors' rows at prefix + rank — only ranks
// below the limit.  A workgroup whose tile ends at or beyond the limit takes no further ticket, and a ticket taken after
// some tile has reached the limit is published as empty without reading a column: with every row surviving, one round of
// the grid is scanned whatever the batch size.  Values and validity bytes come from the functions the transform kernels
// use (eval_quad, compare_tile, cvt32), so the bytes written equal the per-node sequence's for the same rows.
//
// Run-length (mode 3) columns — the sort columns of archive batches — are read where they lie (select_scan_kernel<true, 0>): per
// tile and column two scalar binary searches over the counts give the runs of the tile's first and last row.  One run: value
// and validity are a broadcast, and a filter whose run is null or fails the comparison REJECTS the tile — its look-back word is
// published with count 0 and no other column is read.  Several runs: the run ends inside the tile (at most 4095) are staged
// in LDS, a lane searches them once per quad and walks the quad's other rows along them.  Plans without such a column run
// select_scan_kernel<false, 0>, the instruction sequence of before.  A GeoPoint column in the run-length layout is declined: the
// per-node sequence never decodes it (binding.hpp) and reads its rows past the run arrays.
//
// Joined columns (AresFusedFilterJoinSelect; select_scan_kernel<RUNS, 1 or 2>): the cuckoo probe of cuckoo_probe.hpp runs inside
// the tile and the tile's record ids live in LDS (32 KiB per join).  A join that a foreign filter reads is probed before the
// ranking, for the rows the main-table filters left alive; a join that only dimensions read is probed after the look-back, for
// the rows that are written — a small limit costs that many probes.  Joined values are load_foreign32 (device_model.hpp), the
// expressions over them the FastOperands of a column with validity.
//
// Stores go straight to the slots: the survivors of a wavefront's quads have consecutive ranks, so each store instruction
// of a wavefront covers one contiguous byte range, and a quad that survives whole is stored as one 16 / 8 / 4 byte access.
#include "select_scan.hpp"

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>

#include "ares_extensions.h"
#include "binding.hpp"
#include "common.hpp"
#include "device_model.hpp"
#include "dim_layout.hpp"
#include "lookback.hpp"

namespace ares {

namespace {

constexpr int Q = kSelectQuads;

struct __attribute__((packed, aligned(1))) SU16 { uint16_t v; };
struct __attribute__((packed, aligned(1))) SU32 { uint32_t v; };
struct __attribute__((packed, aligned(1))) SU32x2 { uint32_t v[2]; };
struct __attribute__((packed, aligned(1))) SU64 { uint64_t v; };
struct __attribute__((packed, aligned(1))) SU64x2 { uint64_t v[2]; };

__device__ __forceinline__ uint32_t ld_word(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_word(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// first row of quad q of this lane in the tile that starts at row0 (the geometry of filter_rows_kernel)
__device__ __forceinline__ int64_t quad_row(int64_t row0, int q) { return row0 + (static_cast<int64_t>(q) * kSelectBlock + threadIdx.x) * 4; }

// Values (widened as the transform kernels widen them) and validity nibbles of the lane's quads of one column; rows are
// positions.  Positions at or beyond n read nothing: value 0, and a validity bit that the caller masks.
__device__ __forceinline__ void load_column_tile(const FastOperands &f, int64_t row0, int n, uint32_t (&vals)[Q][4], uint32_t (&okb)[Q]) {
#pragma unroll
  for (int q = 0; q < Q; q++) {
    const int64_t i0 = quad_row(row0, q);
    const bool full = i0 + 3 < n;
    uint32_t raw[4] = {0u, 0u, 0u, 0u};
    if (f.step == 2) {
      const uint16_t *v16 = reinterpret_cast<const uint16_t *>(f.vals);
      if (full) {
        const SU32x2 v = *reinterpret_cast<const SU32x2 *>(v16 + i0);
        raw[0] = v.v[0] & 0xFFFFu; raw[1] = v.v[0] >> 16; raw[2] = v.v[1] & 0xFFFFu; raw[3] = v.v[1] >> 16;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (i0 + j < n) raw[j] = v16[i0 + j];
      }
#pragma unroll
      for (int j = 0; j < 4; j++) vals[q][j] = f.akind == K_I32 ? static_cast<uint32_t>(static_cast<int32_t>(static_cast<int16_t>(raw[j]))) : raw[j];
    } else if (f.step == 1) {
      const uint8_t *v8 = reinterpret_cast<const uint8_t *>(f.vals);
      if (full) {
        const uint32_t v = reinterpret_cast<const SU32 *>(v8 + i0)->v;
        raw[0] = v & 0xFFu; raw[1] = (v >> 8) & 0xFFu; raw[2] = (v >> 16) & 0xFFu; raw[3] = v >> 24;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (i0 + j < n) raw[j] = v8[i0 + j];
      }
#pragma unroll
      for (int j = 0; j < 4; j++) vals[q][j] = f.akind == K_I32 ? static_cast<uint32_t>(static_cast<int32_t>(static_cast<int8_t>(raw[j]))) : raw[j];
    } else {
      if (full) {
        if (f.streaming) {  // a column the plan reads once
          typedef uint32_t V4 __attribute__((ext_vector_type(4)));
          typedef V4 V4a __attribute__((aligned(4)));
          const V4 v = __builtin_nontemporal_load(reinterpret_cast<const V4a *>(f.vals + i0));
          raw[0] = v.x; raw[1] = v.y; raw[2] = v.z; raw[3] = v.w;
        } else {
          const U32x4 v = *reinterpret_cast<const U32x4 *>(f.vals + i0);
#pragma unroll
          for (int j = 0; j < 4; j++) raw[j] = v.v[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (i0 + j < n) raw[j] = f.vals[i0 + j];
      }
#pragma unroll
      for (int j = 0; j < 4; j++) vals[q][j] = raw[j];
    }
    // 16-bit window of the bitmap from the byte of the quad's first row (one byte past a mode-2 bitmap lies in the values)
    uint32_t window = 0xFFFFu;
    const uint32_t bit0 = static_cast<uint32_t>(i0) + f.bitOff;
    if (f.nulls && i0 < n) window = reinterpret_cast<const PU16 *>(f.nulls + (bit0 >> 3))->v;
    okb[q] = (window >> (bit0 & 7u)) & 0xFu;
  }
}

// ---- run-length (mode 3) columns ------------------------------------------------------------------------------------
// Runs of rows x0 <= x1 as locate() (device_model.hpp) finds them: the number of counts[0 .. runs) at or below the row, less
// one — rows past the last count take the last run, and counts[runs] is never read.  Both searches advance together; with
// scalar arguments they are scalar loads.
struct RunSpan {
  uint32_t lo, hi;
};
__device__ __forceinline__ RunSpan locate_span(const uint32_t *counts, uint32_t runs, uint32_t x0, uint32_t x1) {
  uint32_t f0 = 0, l0 = runs, f1 = 0, l1 = runs;
  while (f0 < l0 || f1 < l1) {
    const uint32_t m0 = min(f0 + ((l0 - f0) >> 1), runs - 1), m1 = min(f1 + ((l1 - f1) >> 1), runs - 1);
    const uint32_t c0 = counts[m0], c1 = counts[m1];
    if (f0 < l0) {
      if (c0 > x0) l0 = m0; else f0 = m0 + 1;
    }
    if (f1 < l1) {
      if (c1 > x1) l1 = m1; else f1 = m1 + 1;
    }
  }
  RunSpan s;
  s.lo = f0 ? f0 - 1 : 0u;
  s.hi = f1 ? f1 - 1 : 0u;
  return s;
}

// value of run `run`, widened as load_column_tile widens a row's, and its validity bit
__device__ __forceinline__ uint32_t run_value(const FastOperands &f, uint32_t run) {
  if (f.step == 2) {
    const uint32_t raw = reinterpret_cast<const uint16_t *>(f.vals)[run];
    return f.akind == K_I32 ? static_cast<uint32_t>(static_cast<int32_t>(static_cast<int16_t>(raw))) : raw;
  }
  if (f.step == 1) {
    const uint32_t raw = reinterpret_cast<const uint8_t *>(f.vals)[run];
    return f.akind == K_I32 ? static_cast<uint32_t>(static_cast<int32_t>(static_cast<int8_t>(raw))) : raw;
  }
  return f.vals[run];
}
__device__ __forceinline__ uint32_t run_valid(const FastOperands &f, uint32_t run) {
  const uint32_t bit = run + f.bitOff;
  return (static_cast<uint32_t>(f.nulls[bit >> 3]) >> (bit & 7u)) & 1u;
}

// The runs of one column inside one tile.  span.lo == span.hi: one run.  Otherwise ends[i] (i < m = hi - lo) is the end of
// run lo + i relative to the tile's first row, in (0, 4095]: staged in LDS, or — m beyond the tile's rows, which takes runs
// of no rows — read from the counts.
struct TileRuns {
  RunSpan span;
  uint32_t m;
  bool inLds;
  const uint32_t *lds;     // the staged ends
  const uint32_t *counts;  // counts + lo + 1
  uint32_t row0;
  __device__ __forceinline__ uint32_t end(uint32_t i) const { return inLds ? lds[i] : counts[i] - row0; }
};

// (every thread of the workgroup, uniformly)
__device__ __forceinline__ TileRuns tile_runs(const uint32_t *counts, uint32_t runs, uint32_t row0, uint32_t lastRow, uint32_t *sEnds, bool &staged) {
  TileRuns t;
  t.span = locate_span(counts, runs, row0, lastRow);
  t.m = t.span.hi - t.span.lo;
  t.counts = counts + t.span.lo + 1;
  t.row0 = row0;
  t.lds = sEnds;
  t.inLds = false;
  if (t.m > 0 && t.m < static_cast<uint32_t>(kSelectTile)) {
    __syncthreads();  // (the searches of the column staged before are over)
    for (uint32_t i = threadIdx.x; i < t.m; i += kSelectBlock) sEnds[i] = t.counts[i] - row0;
    __syncthreads();
    t.inLds = true;
    staged = true;
  }
  return t;
}

// runs of the four rows of the quad whose first row is `rel` rows into the tile: one search, then a walk along the ends
__device__ __forceinline__ void quad_runs(const TileRuns &t, uint32_t rel, uint32_t (&run)[4]) {
  uint32_t first = 0, last = t.m;
  while (first < last) {
    const uint32_t mid = first + ((last - first) >> 1);
    if (t.end(mid) > rel) last = mid; else first = mid + 1;
  }
  run[0] = t.span.lo + first;
#pragma unroll
  for (uint32_t j = 1; j < 4; j++) {
    while (first < t.m && t.end(first) <= rel + j) first++;
    run[j] = t.span.lo + first;
  }
}

__device__ __forceinline__ void load_runs_tile(const FastOperands &f, const TileRuns &t, uint32_t (&vals)[Q][4], uint32_t (&okb)[Q]) {
  if (t.m == 0) {  // one run: a broadcast
    const uint32_t v = run_value(f, t.span.lo), ok = run_valid(f, t.span.lo) ? 0xFu : 0u;
#pragma unroll
    for (int q = 0; q < Q; q++) {
#pragma unroll
      for (int j = 0; j < 4; j++) vals[q][j] = v;
      okb[q] = ok;
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < Q; q++) {
    uint32_t run[4];
    quad_runs(t, (static_cast<uint32_t>(q) * kSelectBlock + threadIdx.x) * 4u, run);
    okb[q] = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      vals[q][j] = run_value(f, run[j]);
      okb[q] |= run_valid(f, run[j]) << j;
    }
  }
}

// store_wide_dim for a mode-3 column: the surviving rows' RUNS' stored bytes and validity bits
__device__ __forceinline__ void store_wide_runs(const SelectDimD &D, const TileRuns &t, const uint32_t (&alive)[Q], const uint32_t (&base)[Q], uint32_t excl,
                                                uint32_t room) {
  const uint8_t *src = reinterpret_cast<const uint8_t *>(D.f.vals);
  const int w = D.width;
#pragma unroll
  for (int q = 0; q < Q; q++) {
    if (!alive[q]) continue;
    uint32_t run[4] = {t.span.lo, t.span.lo, t.span.lo, t.span.lo};
    if (t.m) quad_runs(t, (static_cast<uint32_t>(q) * kSelectBlock + threadIdx.x) * 4u, run);
    uint32_t r = base[q];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (!((alive[q] >> j) & 1u)) continue;
      if (r < room) {
        const size_t to = static_cast<size_t>(excl) + r;
        const size_t from = run[j];
        if (w == 16) *reinterpret_cast<SU64x2 *>(D.values + 16 * to) = *reinterpret_cast<const SU64x2 *>(src + 16 * from);
        else *reinterpret_cast<SU64 *>(D.values + 8 * to) = *reinterpret_cast<const SU64 *>(src + 8 * from);
        D.nulls[to] = static_cast<uint8_t>(run_valid(D.f, run[j]));
      }
      r++;
    }
  }
}

// ---- joins ------------------------------------------------------------------------------------------------------------
// The record ids of one join for the tile's rows live in LDS, row j of quad q of lane t at (q * kSelectBlock + t) * 4 + j: a
// lane reads back what it wrote itself, so no barrier lies between the probe and the gathers.
__device__ __forceinline__ int rid_slot(int q) { return (q * kSelectBlock + static_cast<int>(threadIdx.x)) * 4; }

// rows of the quads with a local rank below `room`
__device__ __forceinline__ void rows_below(const uint32_t (&alive)[Q], const uint32_t (&base)[Q], uint32_t room, uint32_t (&need)[Q]) {
#pragma unroll
  for (int q = 0; q < Q; q++) {
    need[q] = 0;
    uint32_t r = base[q];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (!((alive[q] >> j) & 1u)) continue;
      if (r < room) need[q] |= 1u << j;
      r++;
    }
  }
}

// Probes the index for the rows in `need`, one after the other (one copy of the probe in the code, and a lane walks only the
// rows it has); a null key is a miss.  Returns the number of rows.  Starting a quad's four probes together — keys, then the
// first signature words of all four, before any probe is finished — was measured and was no faster (profiles/r14_select_join.md).
__device__ __forceinline__ uint32_t probe_rows(const SelectJoinD &J, int64_t row0, const uint32_t (&need)[Q], RecordID *sRid) {
  const FastDivisor bucketDiv = make_fast_divisor(J.index.numBuckets);
  uint32_t todo = 0;
#pragma unroll
  for (int q = 0; q < Q; q++) todo |= need[q] << (4 * q);
  const uint32_t rows = __popc(todo);
  while (todo) {
    const int k = __builtin_ctz(todo);
    todo &= todo - 1;
    const int q = k >> 2, j = k & 3;
    const uint32_t row = static_cast<uint32_t>(quad_row(row0, q)) + j;
    uint32_t key[4] = {0, 0, 0, 0};
    const uint32_t ok = cuckoo_load_key(J.key, row, row, nullptr, 0, key);
    RecordID rid = {0, 0};
    if (ok) rid = cuckoo_probe(J.index, bucketDiv, key);
    sRid[rid_slot(q) + j] = rid;
  }
  return rows;
}

// load_column_tile for a joined column: the rows in `need` through their record ids; other rows read nothing (0, null)
__device__ __forceinline__ void gather_tile(const OperandD &col, const RecordID *sRid, const uint32_t (&need)[Q], uint32_t (&vals)[Q][4], uint32_t (&okb)[Q]) {
#pragma unroll
  for (int q = 0; q < Q; q++) {
    okb[q] = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      vals[q][j] = 0;
      if ((need[q] >> j) & 1u) {
        const DVal v = load_foreign32(col, sRid[rid_slot(q) + j]);
        vals[q][j] = v.bits;
        okb[q] |= (v.ok ? 1u : 0u) << j;
      }
    }
  }
}

struct ExprConst {
  DVal y;
  FastDivisor fd;
};
__device__ __forceinline__ ExprConst expr_const(const FastOperands &f) {  // as store_tile (deferral_kernels.hpp) prepares them
  ExprConst c;
  c.y.bits = f.bbits;
  c.y.ok = f.bok;
  c.y = cvt32(c.y, f.bkind, f.I);
  const uint32_t mag = (f.I == K_I32 && static_cast<int32_t>(c.y.bits) < 0) ? 0u - c.y.bits : c.y.bits;
  c.fd = make_fast_divisor(mag);
  return c;
}

// A dimension of a 4 / 2 / 1 byte slot: the tile's survivors, ranks [base[q] ..) per quad, local ranks below `room` only.
// JOINED: a joined column — the values of the rows in *need (those that are written) through the record ids in sRid.
template <bool RUNS, bool JOINED = false>
__device__ __forceinline__ void store_narrow_dim(const SelectDimD &D, int64_t row0, int n, const uint32_t (&alive)[Q], const uint32_t (&base)[Q],
                                                 uint32_t excl, uint32_t room, const TileRuns *t, const OperandD *col = nullptr,
                                                 const RecordID *sRid = nullptr, const uint32_t (*need)[Q] = nullptr) {
  uint32_t vals[Q][4], okb[Q];
  if constexpr (JOINED) {
    gather_tile(*col, sRid, *need, vals, okb);
  } else if constexpr (RUNS) {
    if (t) load_runs_tile(D.f, *t, vals, okb);
    else load_column_tile(D.f, row0, n, vals, okb);
  } else {
    load_column_tile(D.f, row0, n, vals, okb);
  }
  const ExprConst c = expr_const(D.f);
  const int w = D.width;
#pragma unroll
  for (int q = 0; q < Q; q++) {
    if (!alive[q]) continue;
    uint32_t rb[4], out[4];
    const uint32_t rok = eval_quad(D.f, vals[q], okb[q], c.y, c.fd, rb);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      DVal x;
      x.bits = rb[j];
      x.ok = 1;
      out[j] = w == 4 ? cvt32(x, D.f.rk, D.outKind).bits : rb[j];  // (a narrow slot takes the value truncated, integer kinds only)
    }
    const size_t at = static_cast<size_t>(excl) + base[q];
    if (alive[q] == 0xFu && base[q] + 4u <= room) {  // the quad survives whole: one access per vector
      if (w == 4) {
        U32x4 o;
#pragma unroll
        for (int j = 0; j < 4; j++) o.v[j] = out[j];
        *reinterpret_cast<U32x4 *>(D.values + 4 * at) = o;
      } else if (w == 2) {
        SU32x2 o;
        o.v[0] = (out[0] & 0xFFFFu) | (out[1] << 16);
        o.v[1] = (out[2] & 0xFFFFu) | (out[3] << 16);
        *reinterpret_cast<SU32x2 *>(D.values + 2 * at) = o;
      } else {
        reinterpret_cast<SU32 *>(D.values + at)->v = (out[0] & 0xFFu) | ((out[1] & 0xFFu) << 8) | ((out[2] & 0xFFu) << 16) | (out[3] << 24);
      }
      reinterpret_cast<SU32 *>(D.nulls + at)->v = (rok & 1u) | ((rok & 2u) << 7) | ((rok & 4u) << 14) | ((rok & 8u) << 21);
      continue;
    }
    uint32_t r = base[q];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (!((alive[q] >> j) & 1u)) continue;
      if (r < room) {
        const size_t to = static_cast<size_t>(excl) + r;
        if (w == 4) reinterpret_cast<SU32 *>(D.values + 4 * to)->v = out[j];
        else if (w == 2) reinterpret_cast<SU16 *>(D.values + 2 * to)->v = static_cast<uint16_t>(out[j]);
        else D.values[to] = static_cast<uint8_t>(out[j]);
        D.nulls[to] = static_cast<uint8_t>((rok >> j) & 1u);
      }
      r++;
    }
  }
}

// A dimension of an 8 / 16 byte slot: the surviving rows' stored bytes and validity bits (a gather).
__device__ __forceinline__ void store_wide_dim(const SelectDimD &D, int64_t row0, const uint32_t (&alive)[Q], const uint32_t (&base)[Q], uint32_t excl,
                                               uint32_t room) {
  const uint8_t *src = reinterpret_cast<const uint8_t *>(D.f.vals);
  const int w = D.width;
#pragma unroll
  for (int q = 0; q < Q; q++) {
    if (!alive[q]) continue;
    const int64_t i0 = quad_row(row0, q);
    const uint32_t bit0 = static_cast<uint32_t>(i0) + D.f.bitOff;
    uint32_t okb = 0xFu;
    if (D.f.nulls) okb = (reinterpret_cast<const PU16 *>(D.f.nulls + (bit0 >> 3))->v >> (bit0 & 7u)) & 0xFu;  // (alive: i0 is inside the batch)
    uint32_t r = base[q];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (!((alive[q] >> j) & 1u)) continue;
      if (r < room) {
        const size_t to = static_cast<size_t>(excl) + r;
        const size_t from = static_cast<size_t>(i0 + j);
        if (w == 16) *reinterpret_cast<SU64x2 *>(D.values + 16 * to) = *reinterpret_cast<const SU64x2 *>(src + 16 * from);
        else *reinterpret_cast<SU64 *>(D.values + 8 * to) = *reinterpret_cast<const SU64 *>(src + 8 * from);
        D.nulls[to] = static_cast<uint8_t>((okb >> j) & 1u);
      }
      r++;
    }
  }
}


__device__ __forceinline__ const SelectJoinPlanD *join_plan() { return nullptr; }
__device__ __forceinline__ const SelectJoinPlanD *join_plan(const SelectJoinPlanD &j) { return &j; }

// RUNS: the plan reads a mode-3 column.  JOINS: the number of joins; 0 is the scan of AresFusedFilterSelect — one argument,
// every join step compiled out — and 1 / 2 are the flavours of AresFusedFilterJoinSelect, with the joins' plan as the second
// argument.
// <false, 0> is the kernel of plans without a mode-3 column, instruction for instruction: three workgroups per compute unit,
// 168 VGPRs, no scratch (a bound of four would spill).  <true, 0> spills 11 VGPRs at three, so it is bound to two and keeps
// everything in registers.  The join flavours are bound to two as well: a tile's record ids take 32 KiB of LDS per join
// (<true, 2>: 80 KiB with the run ends, one workgroup per compute unit, bound to one).
template <bool RUNS, int JOINS, typename... JoinPlan>
__global__ __launch_bounds__(kSelectBlock, JOINS == 0 ? (RUNS ? 2 : 3) : (RUNS && JOINS == 2) ? 1 : 2) void select_scan_kernel(SelectPlanD p, JoinPlan... j) {
  [[maybe_unused]] const SelectJoinPlanD *jp = join_plan(j...);
  __shared__ uint64_t sWave[kSelectBlock / 64];
  __shared__ uint32_t sTileExcl;
  __shared__ int sTile;
  RecordID *sRid = nullptr;
  if constexpr (JOINS > 0) {
    __shared__ RecordID rids[JOINS][kSelectTile];  // 32 KiB per join
    sRid = &rids[0][0];
  }
  uint32_t probed = 0;  // (this lane's rows)
  uint32_t *sEnds = nullptr;
  if constexpr (RUNS) {
    __shared__ uint32_t ends[kSelectTile];  // one column's run ends inside the tile, column after column
    sEnds = ends;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = p.batchRows;
  uint32_t scanned = 0;  // (thread 0's copy is the one reported)
  uint32_t rejectedTiles = 0, stagedTiles = 0;
  for (;;) {
    if (threadIdx.x == 0) {
      int t = static_cast<int>(atomicAdd(&p.state->ticket, 1u));
      // A completed tile has reached the limit: this one is published as empty — its successors' look-back passes over it —
      // and the workgroup leaves.  (Never tile 0: nothing completes before tile 0 has published.)
      if (t > 0 && t < p.numTiles && ld_word(&p.state->stop)) {
        st_status(p.status + t, kFlagAggregate);
        t = -1;
      }
      sTile = t;
    }
    __syncthreads();
    const int tile = RUNS ? __builtin_amdgcn_readfirstlane(sTile) : sTile;  // (scalar: the run searches become scalar loads)
    if (tile < 0 || tile >= p.numTiles) break;
    const int64_t row0 = static_cast<int64_t>(tile) * kSelectTile;
    scanned++;
    // mode-3 columns: the tile's first row and its last row inside the batch
    const uint32_t urow0 = static_cast<uint32_t>(row0), lastRow = static_cast<uint32_t>(min(row0 + kSelectTile, static_cast<int64_t>(n)) - 1);
    bool staged = false, rejected = false;

    // ---- the filter conjunction over the tile's rows
    uint32_t in[Q], alive[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const int64_t i0 = quad_row(row0, q);
      in[q] = 0xFu;
      if (i0 + 3 >= n) {
        in[q] = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) in[q] |= (i0 + j < n ? 1u : 0u) << j;
      }
      alive[q] = in[q];
    }
    for (int k = 0; k < p.numFilters; k++) {
      const FastOperands &f = p.filters[k];
      uint32_t vals[Q][4], okb[Q], kb[Q];
      DVal y;
      y.bits = f.bbits;
      y.ok = f.bok;
      y = cvt32(y, f.bkind, f.I);
      if constexpr (RUNS) {
        if (p.filterCounts[k]) {
          const TileRuns t = tile_runs(p.filterCounts[k], p.filterRuns[k], urow0, lastRow, sEnds, staged);
          if (t.m == 0) {  // one run decides for the whole tile (one value for every lane: made scalar, no vote)
            const uint32_t v = __builtin_amdgcn_readfirstlane(run_value(f, t.span.lo)), ok = __builtin_amdgcn_readfirstlane(run_valid(f, t.span.lo));
            if (compare_fast(f, v, ok, y)) continue;
            rejected = true;
            break;
          }
          load_runs_tile(f, t, vals, okb);
        } else {
          load_column_tile(f, row0, n, vals, okb);
        }
      } else {
        load_column_tile(f, row0, n, vals, okb);
      }
      compare_tile<Q>(f, vals, okb, in, y, kb);  // result validity is ignored (functor.hpp:903-915)
#pragma unroll
      for (int q = 0; q < Q; q++) alive[q] &= kb[q];
    }
    if constexpr (RUNS) {
      if (rejected) {
        // No row of the tile survives and no other column is read.  The tile's word says so — as an inclusive prefix when the
        // tile before has one already, so that chains of rejected tiles stay short for the look-back that crosses them — and
        // the workgroup takes the next ticket; the batch's last tile goes on, empty, to publish the total.
        rejectedTiles++;
        if (tile != p.numTiles - 1) {
          if (threadIdx.x == 0) {
            uint64_t w = kFlagAggregate;
            if (tile == 0) w = kFlagInclusive;
            else if (const uint64_t before = ld_status(p.status + tile - 1); (before & kFlagMask) == kFlagInclusive) w = before;
            st_status(p.status + tile, w);
          }
          if (staged) stagedTiles++;
          __syncthreads();  // (sTile has been read by every wave before thread 0 writes the next)
          continue;
        }
#pragma unroll
        for (int q = 0; q < Q; q++) alive[q] = 0;
      }
    }

    // ---- joins that a foreign filter reads: probed for the survivors so far, then the filters over the joined values
    if constexpr (JOINS > 0) {
#pragma unroll
      for (int k = 0; k < JOINS; k++)
        if (jp->joins[k].early) probed += probe_rows(jp->joins[k], row0, alive, sRid + k * kSelectTile);
      for (int k = 0; k < jp->numForeignFilters; k++) {
        const FastOperands &f = jp->foreignFilters[k];
        uint32_t vals[Q][4], okb[Q], kb[Q];
        DVal y;
        y.bits = f.bbits;
        y.ok = f.bok;
        y = cvt32(y, f.bkind, f.I);
        gather_tile(jp->foreignFilterCols[k], sRid + jp->foreignFilterJoin[k] * kSelectTile, alive, vals, okb);
        compare_tile<Q>(f, vals, okb, in, y, kb);
#pragma unroll
        for (int q = 0; q < Q; q++) alive[q] &= kb[q];
      }
    }

    // ---- ranks in row order: quad q of every lane precedes quad q + 1 of any lane — four counts scanned as one word
    uint64_t mine = 0;
#pragma unroll
    for (int q = 0; q < Q; q++) mine |= static_cast<uint64_t>(__popc(alive[q])) << (16 * q);
    uint64_t incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint64_t t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    if (lane == 63) sWave[wave] = incl;
    __syncthreads();
    uint64_t before = incl - mine, tileSum = 0;
#pragma unroll
    for (int w = 0; w < kSelectBlock / 64; w++) {
      if (w < wave) before += sWave[w];
      tileSum += sWave[w];
    }
    uint32_t base[Q], tileCount = 0;
#pragma unroll
    for (int q = 0; q < Q; q++) {
      base[q] = tileCount + static_cast<uint32_t>((before >> (16 * q)) & 0xFFFFu);
      tileCount += static_cast<uint32_t>((tileSum >> (16 * q)) & 0xFFFFu);
    }

    // ---- the tile's exclusive prefix
    if (wave == 0) {
      if (lane == 0) st_status(p.status + tile, (tile == 0 ? kFlagInclusive : kFlagAggregate) | tileCount);
      uint64_t excl = 0;
      if (tile > 0) {
        excl = lookback_wave(p.status, tile, lane, &p.state->error);
        if (lane == 0) st_status(p.status + tile, kFlagInclusive | (excl + tileCount));
      }
      if (lane == 0) {
        sTileExcl = static_cast<uint32_t>(excl);
        if (tile == p.numTiles - 1) st_word(&p.state->total, static_cast<uint32_t>(excl + tileCount));
        if (excl + tileCount >= p.limit) st_word(&p.state->stop, 1u);
      }
    }
    __syncthreads();
    const uint32_t excl = sTileExcl;

    // ---- the survivors' rows, ranks below the limit only
    if (tileCount > 0 && excl < p.limit) {
      const uint32_t room = p.limit - excl;
      uint32_t need[Q];
      if constexpr (JOINS > 0) {  // joins that only dimensions read: probed for the rows that are written
        rows_below(alive, base, room, need);
#pragma unroll
        for (int k = 0; k < JOINS; k++)
          if (!jp->joins[k].early) probed += probe_rows(jp->joins[k], row0, need, sRid + k * kSelectTile);
      }
      for (int d = 0; d < p.numDims; d++) {
        const SelectDimD &D = p.dims[d];
        if constexpr (JOINS > 0) {
          if (jp->dimJoin[d] >= 0) {
            store_narrow_dim<false, true>(D, row0, n, alive, base, excl, room, nullptr, &jp->dimCols[d], sRid + jp->dimJoin[d] * kSelectTile, &need);
            continue;
          }
        }
        if constexpr (RUNS) {
          if (D.counts) {
            const TileRuns t = tile_runs(D.counts, D.runs, urow0, lastRow, sEnds, staged);
            if (D.width <= 4) store_narrow_dim<true>(D, row0, n, alive, base, excl, room, &t);
            else store_wide_runs(D, t, alive, base, excl, room);
            continue;
          }
        }
        if (D.width <= 4) store_narrow_dim<false>(D, row0, n, alive, base, excl, room, nullptr);
        else store_wide_dim(D, row0, alive, base, excl, room);
      }
    }
    if (RUNS && staged) stagedTiles++;
    if (static_cast<uint64_t>(excl) + tileCount >= p.limit) break;  // nothing more is wanted
  }

  // ---- the last workgroup to leave publishes the result in the caller's pinned words
  if constexpr (JOINS > 0) {  // the workgroup's probes, added once
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) probed += __shfl_down(probed, off);
    __syncthreads();  // (sWave's readers of the last tile are through)
    if (lane == 0) sWave[wave] = probed;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (scanned) atomicAdd(&p.state->scanned, scanned);
    if constexpr (JOINS > 0) {
      uint32_t all = 0;
#pragma unroll
      for (int w = 0; w < kSelectBlock / 64; w++) all += static_cast<uint32_t>(sWave[w]);
      if (all) atomicAdd(&p.state->probed, all);
    }
    if constexpr (RUNS) {
      if (rejectedTiles) atomicAdd(&p.state->rejected, rejectedTiles);
      if (stagedTiles) atomicAdd(&p.state->staged, stagedTiles);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const uint32_t left = atomicAdd(&p.state->done, 1u);
    if (left == gridDim.x - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      p.result[0] = ld_word(&p.state->stop) ? p.limit : ld_word(&p.state->total);
      p.result[1] = ld_word(&p.state->error);
      p.result[2] = ld_word(&p.state->scanned);
      if constexpr (RUNS) {
        p.result[3] = ld_word(&p.state->rejected);
        p.result[4] = ld_word(&p.state->staged);
      }
      if constexpr (JOINS > 0) p.result[5] = ld_word(&p.state->probed);
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
std::atomic<unsigned long long> g_stats[4];     // batches run, batches declined, tiles scanned, rows written
std::atomic<unsigned long long> g_runStats[2];  // tiles rejected by a run, tiles that staged run ends
std::atomic<unsigned long long> g_joinStats[5];  // AresFusedFilterJoinSelect: batches run, declined, tiles scanned, rows written, keys probed

bool select_enabled() {
  static EnvSwitch<bool> on("ARES_SELECT", [](const char *e) { return !(e && e[0] == '0'); });
  return on.get();
}

// the kernel of a plan: RUNS x number of joins
const void *select_kernel(bool runs, int joins) {
  if (joins == 0) return runs ? reinterpret_cast<const void *>(&select_scan_kernel<true, 0>) : reinterpret_cast<const void *>(&select_scan_kernel<false, 0>);
  if (joins == 1) return runs ? reinterpret_cast<const void *>(&select_scan_kernel<true, 1, SelectJoinPlanD>) : reinterpret_cast<const void *>(&select_scan_kernel<false, 1, SelectJoinPlanD>);
  return runs ? reinterpret_cast<const void *>(&select_scan_kernel<true, 2, SelectJoinPlanD>) : reinterpret_cast<const void *>(&select_scan_kernel<false, 2, SelectJoinPlanD>);
}

// workgroups of one launch: as many as the device holds at once; ARES_SELECT_GRID=n (tests) overrides
int select_grid(int device, bool runs, int joins) {
  static EnvSwitch<int> forced("ARES_SELECT_GRID", [](const char *e) { return e ? atoi(e) : 0; });
  const int f = forced.get();
  if (f > 0) return std::min(f, kSelectGridCap);
  static std::mutex mu;
  static std::map<std::pair<int, const void *>, int> known;
  std::lock_guard<std::mutex> lock(mu);
  const void *kernel = select_kernel(runs, joins);
  auto it = known.find({device, kernel});
  if (it != known.end()) return it->second;
  int perCU = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, kSelectBlock, 0) != hipSuccess || perCU < 1) {
    (void)hipGetLastError();
    perCU = joins ? 1 : 4;
  }
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) {
    (void)hipGetLastError();
    cus = 256;
  }
  return known[{device, kernel}] = std::max(1, std::min(perCU * cus, kSelectGridCap));
}

void check_column(const AresFusedExpr &e, int batchRows) {
  if (e.arity != 1 && e.arity != 2) throw NotFusable("arity");
  if (e.lhs.Type != VectorPartyInput || (e.arity == 2 && e.rhs.Type != ConstantInput))
    throw NotFusable("operands must be a main-table column and a constant");
  const VectorPartySlice &vp = e.lhs.Vector.VP;
  if (run_length_layout(vp)) {
    // Length is the number of runs; the rows the runs cover are known to the counts only (the per-node sequence does not
    // check them either: rows past the last count take the last run)
    if (vp.Length < 1) throw NotFusable("run-length column without runs");
    if (vp.DataType == GeoPoint) throw NotFusable("run-length GeoPoint column (read undecoded by the per-node sequence)");
    if (reinterpret_cast<uintptr_t>(vp.BasePtr) & 3u) throw NotFusable("run-length counts are not word-aligned");
    return;
  }
  if (static_cast<int64_t>(vp.Length) < batchRows) throw NotFusable("column shorter than the batch");
}

// a joined column of a foreign filter or a joined dimension
void check_foreign_column(const AresFusedExpr &e) {
  if (e.arity != 1 && e.arity != 2) throw NotFusable("arity");
  if (e.lhs.Type != ForeignColumnInput || (e.arity == 2 && e.rhs.Type != ConstantInput))
    throw NotFusable("operands must be a joined column and a constant");
  const ForeignColumnVector &f = e.lhs.Vector.ForeignVP;
  if (f.DataType == Bool || wide_type(f.DataType)) throw NotFusable("Bool or wide joined column");
  if (f.TimezoneLookup) throw NotFusable("timezone lookup");
  if (f.NumBatches < 0 || (f.NumBatches > 0 && !f.Batches)) throw NotFusable("joined column without batches");
}

// the run description of a bound mode-3 column
struct RunsOf {
  const uint32_t *counts = nullptr;
  uint32_t runs = 0;
};

// a filter, or a dimension of a 4 / 2 / 1 byte slot: the operand shape of the fast transform / filter kernels
// `foreign` (join flavour): the expression's column is a joined one — bound into *foreign as an OP_FOREIGN operand, its batch
// descriptors uploaded on the stream and kept in `temps`; the FastOperands are those of a column with validity.
FastOperands narrow_operands(const AresFusedExpr &e, bool compareOnly, int batchRows, hipStream_t stream, RunsOf &runs, CallTemps &temps,
                             OperandD *foreign = nullptr) {
  if (foreign) check_foreign_column(e);
  else check_column(e, batchRows);
  if (!foreign && wide_type(e.lhs.Vector.VP.DataType)) throw NotFusable("expression over a wide column");
  InputVector ins[2] = {e.lhs, e.arity == 2 ? e.rhs : e.lhs};
  EvalParams p;
  try {
    build_params(ins, e.arity, stream, nullptr, nullptr, 0, e.functor, p, temps);
  } catch (const std::invalid_argument &bad) {
    throw NotFusable(bad.what());
  }
  runs = RunsOf();
  if (foreign) {
    if (p.a.type != OP_FOREIGN) throw NotFusable("joined column");
    *foreign = p.a;
    foreign->rids = nullptr;  // (the tile's record ids are the kernel's own)
    p.a.type = OP_COLUMN;
    p.a.mode = 2;
    p.a.base = nullptr;
    p.a.nullsOff = p.a.valuesOff = 0;
    p.a.bitOff = 0;
  }
  if (p.a.type == OP_COLUMN && p.a.mode == 3) {
    // Bound here, not by the deferral machinery's fast_operands(): the expression shapes are the ones it takes for a column
    // with validity (same kinds, widths and functors), and vals / nulls name the RUN arrays
    runs.counts = reinterpret_cast<const uint32_t *>(p.a.base);
    runs.runs = p.a.length;
    p.a.mode = 2;
  }
  FastOperands f;
  if (!fast_operands(p, f, compareOnly)) throw NotFusable("expression shape");
  f.idx = nullptr;
  f.pad = 0;
  return f;
}

// a bare Int64 / GeoPoint / UUID column into a slot of its own type
FastOperands wide_operands(const AresFusedExpr &e, int batchRows, hipStream_t stream, RunsOf &runs) {
  check_column(e, batchRows);
  const int t = e.lhs.Vector.VP.DataType;
  if (e.arity != 1 || e.functor != Noop) throw NotFusable("expression over a wide column");
  if (t != static_cast<int>(e.outType) || t == Uint64) throw NotFusable("a wide column goes into a slot of its own type");
  OperandD op;
  CallTemps temps;
  try {
    bind_operand(e.lhs, true, stream, op, temps);
  } catch (const std::invalid_argument &bad) {
    throw NotFusable(bad.what());
  }
  if (op.type != OP_COLUMN || op.mode > 3) throw NotFusable("column mode");
  runs = RunsOf();
  if (op.mode == 3) {
    runs.counts = reinterpret_cast<const uint32_t *>(op.base);
    runs.runs = op.length;
  }
  FastOperands f;
  memset(&f, 0, sizeof(f));
  f.vals = reinterpret_cast<const uint32_t *>(op.base + op.valuesOff);
  f.nulls = op.mode >= 2 ? op.base + op.nullsOff : nullptr;
  f.bitOff = op.bitOff;
  f.akind = op.kind;
  f.arity = 1;
  f.functor = Noop;
  f.step = op.step;
  return f;
}

// The select scan of one batch; `jq` (may be null): the joins, foreign filters and the joined dimensions of
// AresFusedFilterJoinSelect — filters / dims are then its main-table filters and all its dimensions.
int fused_select(int device, int numFilters, const AresFusedExpr *filters, int numDims, const AresFusedExpr *dims, const AresFusedJoinSelect *jq,
                 int batchRows, int limit, const DimensionVector &outKeys, hipStream_t stream) {
  if (!select_enabled()) throw NotFusable("switched off (ARES_SELECT=0)");
  if (numFilters < 0 || numFilters > kSelectFilters) throw NotFusable("at most 4 filters");
  if (numDims < 1 || numDims > kSelectDims) throw NotFusable("1..8 dimensions");
  if (batchRows < 0) throw NotFusable("size");
  if (jq) {
    if (jq->numJoins < 1 || jq->numJoins > kSelectJoins) throw NotFusable("1..2 joins (none: AresFusedFilterSelect)");
    if (jq->numForeignFilters < 0 || jq->numForeignFilters > kSelectForeignFilters) throw NotFusable("at most 4 foreign filters");
  }
  DimLayoutD L;
  try {
    L = make_dim_layout(outKeys.NumDimsPerDimWidth);
  } catch (const std::invalid_argument &) {
    throw NotFusable("dimension vector layout");
  }
  if (L.numDims != numDims) throw NotFusable("dimension vector layout");

  CallTemps temps;  // (the joined columns' batch descriptors: alive until the launch has finished)
  SelectPlanD plan;
  memset(&plan, 0, sizeof(plan));
  SelectJoinPlanD joins;
  memset(&joins, 0, sizeof(joins));
  for (int d = 0; d < kSelectDims; d++) joins.dimJoin[d] = -1;
  plan.numFilters = numFilters;
  plan.numDims = numDims;
  bool anyRuns = false;
  RunsOf runs;
  for (int k = 0; k < numFilters; k++) {
    plan.filters[k] = narrow_operands(filters[k], true, batchRows, stream, runs, temps);
    plan.filterCounts[k] = runs.counts;
    plan.filterRuns[k] = runs.runs;
    anyRuns |= runs.counts != nullptr;
  }
  if (jq) {
    joins.numJoins = jq->numJoins;
    joins.numForeignFilters = jq->numForeignFilters;
    for (int k = 0; k < jq->numJoins; k++) joins.joins[k] = bind_join(jq->joins[k], batchRows, stream, temps);
    for (int k = 0; k < jq->numForeignFilters; k++) {
      const int j = jq->foreignFilterJoin[k];
      if (j < 0 || j >= jq->numJoins) throw NotFusable("join index out of range");
      joins.foreignFilters[k] = narrow_operands(jq->foreignFilters[k], true, batchRows, stream, runs, temps, &joins.foreignFilterCols[k]);
      joins.foreignFilterJoin[k] = j;
      joins.joins[j].early = 1;
    }
  }
  const size_t capacity = static_cast<size_t>(outKeys.VectorCapacity > 0 ? outKeys.VectorCapacity : 0);
  for (int d = 0; d < numDims; d++) {
    const int t = dims[d].outType;
    const bool narrow = t == Int8 || t == Uint8 || t == Int16 || t == Uint16 || t == Int32 || t == Uint32 || t == Float32;
    if (!narrow && !(t == Int64 || t == GeoPoint || t == UUID)) throw NotFusable("dimension type");
    const int dimJoin = jq ? jq->dimJoin[d] : -1;
    if (dimJoin >= (jq ? jq->numJoins : 0)) throw NotFusable("join index out of range");
    joins.dimJoin[d] = dimJoin < 0 ? -1 : dimJoin;
    SelectDimD &D = plan.dims[d];
    D.width = step_in_bytes(t);
    if (D.width != L.width[d]) throw NotFusable("dimension vector layout");
    if (dimJoin >= 0 && !narrow) throw NotFusable("Bool or wide joined column");
    if (narrow) {
      D.f = narrow_operands(dims[d], false, batchRows, stream, runs, temps, dimJoin >= 0 ? &joins.dimCols[d] : nullptr);
      if (D.width < 4 && !(D.f.rk == K_I32 || D.f.rk == K_U32)) throw NotFusable("float result into a narrow slot");
      D.outKind = t == Int32 ? K_I32 : t == Uint32 ? K_U32 : K_F32;
    } else {
      D.f = wide_operands(dims[d], batchRows, stream, runs);
    }
    D.counts = runs.counts;
    D.runs = runs.runs;
    anyRuns |= runs.counts != nullptr;
    D.values = outKeys.DimValues + static_cast<size_t>(L.valueOff[d]) * capacity;
    D.nulls = outKeys.DimValues + static_cast<size_t>(L.valueBytes) * capacity + static_cast<size_t>(d) * capacity;
  }
  const int64_t wanted = limit < 0 ? batchRows : std::min<int64_t>(batchRows, limit);
  if (static_cast<int64_t>(capacity) < wanted) throw std::invalid_argument("outKeys.VectorCapacity < min(batchRows, limit)");
  if (wanted > 0 && !outKeys.DimValues) throw std::invalid_argument("null dimension vector");
  if (wanted == 0) return 0;

  // a 4-byte column that the plan reads once is loaded non-temporally (modes 1/2: the run arrays of a mode-3 column are
  // small and read again and again; a joined column is gathered)
  auto uses = [&](const uint32_t *vals) {
    int c = 0;
    for (int k = 0; k < plan.numFilters; k++) c += plan.filters[k].vals == vals;
    for (int d = 0; d < plan.numDims; d++) c += plan.dims[d].f.vals == vals;
    for (int k = 0; k < joins.numJoins; k++) c += reinterpret_cast<const uint32_t *>(joins.joins[k].key.base + joins.joins[k].key.valuesOff) == vals;
    return c;
  };
  for (int k = 0; k < plan.numFilters; k++) plan.filters[k].streaming = !plan.filterCounts[k] && uses(plan.filters[k].vals) == 1;
  for (int d = 0; d < plan.numDims; d++) plan.dims[d].f.streaming = joins.dimJoin[d] < 0 && !plan.dims[d].counts && uses(plan.dims[d].f.vals) == 1;

  flush_deferred_for_vector(device, outKeys, nullptr, 0);
  grouped_note_write(device, outKeys);

  plan.batchRows = batchRows;
  plan.numTiles = static_cast<int>((static_cast<int64_t>(batchRows) + kSelectTile - 1) / kSelectTile);
  plan.limit = limit < 0 ? 0xFFFFFFFFu : static_cast<uint32_t>(limit);
  const size_t stateBytes = sizeof(SelectStateD) + sizeof(uint64_t) * static_cast<size_t>(plan.numTiles);
  StreamBuffer ws((stateBytes + 15) / 16 * 16, stream);
  hip_check(hipMemsetAsync(ws.get(), 0, (stateBytes + 15) / 16 * 16, stream), "hipMemsetAsync");
  plan.state = ws.as<SelectStateD>();
  plan.status = reinterpret_cast<uint64_t *>(ws.as<uint8_t>() + sizeof(SelectStateD));
  volatile uint32_t *result = reinterpret_cast<volatile uint32_t *>(pinned_words());
  plan.result = const_cast<uint32_t *>(result);
  result[0] = 0u;
  result[1] = 2u;  // (overwritten by the launch's last workgroup)
  result[2] = result[3] = result[4] = result[5] = 0u;
  const int grid = std::min(select_grid(device, anyRuns, joins.numJoins), plan.numTiles);
  if (joins.numJoins == 2) {
    if (anyRuns) ARES_LAUNCH("select_join_kernel", (select_scan_kernel<true, 2, SelectJoinPlanD>), grid, kSelectBlock, stream, plan, joins);
    else ARES_LAUNCH("select_join_kernel", (select_scan_kernel<false, 2, SelectJoinPlanD>), grid, kSelectBlock, stream, plan, joins);
  } else if (joins.numJoins == 1) {
    if (anyRuns) ARES_LAUNCH("select_join_kernel", (select_scan_kernel<true, 1, SelectJoinPlanD>), grid, kSelectBlock, stream, plan, joins);
    else ARES_LAUNCH("select_join_kernel", (select_scan_kernel<false, 1, SelectJoinPlanD>), grid, kSelectBlock, stream, plan, joins);
  } else if (anyRuns) {
    ARES_LAUNCH("select_scan_kernel", (select_scan_kernel<true, 0>), grid, kSelectBlock, stream, plan);
  } else {
    ARES_LAUNCH("select_scan_kernel", (select_scan_kernel<false, 0>), grid, kSelectBlock, stream, plan);
  }
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
  ws.mark_idle();
  if (result[1] == 2u) throw AlgorithmError("ERROR: select scan: the launch finished without publishing its result");
  if (result[1] != 0u) throw AlgorithmError("ERROR: select scan: a look-back wait gave up");
  const uint32_t rows = result[0];
  std::atomic<unsigned long long> *stats = jq ? g_joinStats : g_stats;
  stats[0]++;
  stats[2] += result[2];
  stats[3] += rows;
  if (jq) stats[4] += result[5];
  g_runStats[0] += result[3];
  g_runStats[1] += result[4];
  mem_note_dim_rows(device, outKeys, 0, rows);
  return static_cast<int>(rows);
}

}  // namespace

}  // namespace ares

extern "C" CGoCallResHandle AresFusedFilterSelect(const AresFusedSelect *query, int batchRows, int limit, DimensionVector outKeys,
                                                  void *cudaStream, int device) {
  ARES_ABI_BEGIN(device)
  if (!query) throw std::invalid_argument("null query");
  try {
    resHandle.res = ares::int_result(ares::fused_select(device, query->numFilters, query->filters, query->numDims, query->dims, nullptr, batchRows, limit,
                                                        outKeys, reinterpret_cast<hipStream_t>(cudaStream)));
  } catch (const ares::NotFusable &) {
    ares::g_stats[1]++;
    throw;
  }
  ARES_ABI_END("AresFusedFilterSelect")
}

extern "C" void AresSelectStats(unsigned long long *counters) {
  if (!counters) return;
  for (int i = 0; i < 4; i++) counters[i] = ares::g_stats[i].load();
}

extern "C" void AresSelectRunStats(unsigned long long *counters) {
  if (!counters) return;
  for (int i = 0; i < 2; i++) counters[i] = ares::g_runStats[i].load();
}

extern "C" CGoCallResHandle AresFusedFilterJoinSelect(const AresFusedJoinSelect *query, int batchRows, int limit, DimensionVector outKeys,
                                                      void *cudaStream, int device) {
  ARES_ABI_BEGIN(device)
  if (!query) throw std::invalid_argument("null query");
  try {
    resHandle.res = ares::int_result(ares::fused_select(device, query->numFilters, query->filters, query->numDims, query->dims, query, batchRows, limit,
                                                        outKeys, reinterpret_cast<hipStream_t>(cudaStream)));
  } catch (const ares::NotFusable &) {
    ares::g_joinStats[1]++;
    throw;
  }
  ARES_ABI_END("AresFusedFilterJoinSelect")
}

extern "C" void AresSelectJoinStats(unsigned long long *counters) {
  if (!counters) return;
  for (int i = 0; i < 5; i++) counters[i] = ares::g_joinStats[i].load();
}
