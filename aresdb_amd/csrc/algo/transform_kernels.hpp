// Device code of Unary/BinaryTransform and Unary/BinaryFilter for MI355X (gfx950): the kernels transform.hip launches for
// the calls themselves.  Included by transform.hip only (kernels are not static: one translation unit each); the kernels
// that write a held-back definition after all — iota, fill, queued transforms, compaction — are in deferral_kernels.hpp.
//
// Reference behaviour: query/algorithm.cu:22-41, query/transform.cu:21-86 + transform.hpp:57-89, query/filter.cu:130-253.
// The reference runs thrust::transform (+ thrust::remove_if for filters: a second and third pass over the batch plus a
// host sync).  Here a transform is ONE pass — decode (value, validity) of every operand, apply the functor, write the sink,
// ITEMS independent coalesced loads per lane issued before any use —, several root transforms of a batch share one pass
// over the index vector (transform_multi_kernel), and a filter of the hot shape is counted in row space without writing
// anything observable (filter_rows_kernel) or, when the compacted vector is needed, runs as predicate pass + scan of the
// tile counts + chain-free in-place compaction.
#pragma once

#include <hip/hip_runtime.h>

#include "lookback.hpp"
#include "quad_geometry.hpp"

namespace ares {

// ---------------------------------------------------------------------------------------------
// 32-bit value path: transform
// ---------------------------------------------------------------------------------------------

template <int ITEMS>
__global__ __launch_bounds__(kBlock) void transform32_kernel(EvalParams p, SinkD s, int n) {
  const int64_t tile = static_cast<int64_t>(kBlock) * ITEMS;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * tile; base < n;
       base += static_cast<int64_t>(gridDim.x) * tile) {
    uint32_t rows[ITEMS];
    DVal va[ITEMS], vb[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
      const int64_t i = base + k * kBlock + threadIdx.x;
      rows[k] = (i < n && p.needRow) ? p.idx[i] : static_cast<uint32_t>(i);
    }
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
      const int64_t i = base + k * kBlock + threadIdx.x;
      if (i < n) {
        va[k] = load32(p.a, static_cast<uint32_t>(i), rows[k], p.baseCounts, p.startCount);
        if (p.arity == 2) vb[k] = load32(p.b, static_cast<uint32_t>(i), rows[k], p.baseCounts, p.startCount);
      }
    }
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
      const int64_t i = base + k * kBlock + threadIdx.x;
      if (i < n) {
        DVal x = cvt32(va[k], p.a.kind, p.I);
        DVal r = p.arity == 1 ? unary32(p.functor, p.I, x)
                              : binary32(p.functor, p.I, x, cvt32(vb[k], p.b.kind, p.I));
        sink_store32(s, static_cast<uint32_t>(i), rows[k], r, p.rk);
      }
    }
  }
}

// A joined column copied into a dimension or measure vector — UnaryTransform(Noop) over a 32-bit foreign column
// (query/iterator.hpp:911-930: RecordID -> batch -> value) — the transform of a join query's hot path.  Three dependent loads
// per row (RecordID, the batch's descriptor, the value [+ its validity bit]): the descriptors sit in LDS and every lane keeps
// ITEMS rows in flight, phase by phase (the generic kernel above walks four rows through an interpreter: 1.38 ms per
// 64 Mi rows over a 50 M-row dimension table where the gathers alone need 0.6).
constexpr int kForeignBatchesInLds = 512;
template <int ITEMS>
__global__ __launch_bounds__(kBlock) void transform_foreign_kernel(EvalParams p, SinkD s, int n) {
  __shared__ ForeignBatchD sBatches[kForeignBatchesInLds];
  const OperandD &a = p.a;
  const bool inLds = a.numBatches <= kForeignBatchesInLds;
  if (inLds)
    for (int b = threadIdx.x; b < a.numBatches; b += kBlock) sBatches[b] = a.batches[b];
  __syncthreads();
  const int64_t tile = static_cast<int64_t>(kBlock) * ITEMS;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * tile; base < n; base += static_cast<int64_t>(gridDim.x) * tile) {
    RecordID rid[ITEMS];
    DVal v[ITEMS];
    const uint8_t *nullAt[ITEMS];
    uint32_t nullBit[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
      const int64_t i = base + k * kBlock + threadIdx.x;
      rid[k] = i < n ? a.rids[i] : RecordID{0, 0};
    }
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
      v[k].bits = 0;
      v[k].ok = 0;
      nullAt[k] = nullptr;
      nullBit[k] = 0;
      if (rid[k].batchID != 0 && (rid[k].batchID - a.baseBatchID < a.numBatches - 1 || rid[k].index < static_cast<uint32_t>(a.numRecLast))) {
        const ForeignBatchD b = inLds ? sBatches[rid[k].batchID - a.baseBatchID] : a.batches[rid[k].batchID - a.baseBatchID];
        if (b.isConst) {
          v[k].bits = a.cbits;
          v[k].ok = a.cok;
        } else {
          const uint32_t at = rid[k].index;
          v[k] = read_stored32(b.base + b.valuesOff, a.kind, a.step, at, at + b.bitOff);
          v[k].ok = 1u;
          if (b.valuesOff != 0) {  // (the validity byte is fetched with the values, looked at below)
            nullAt[k] = b.base + b.nullsOff + ((at + b.bitOff) >> 3);
            nullBit[k] = (at + b.bitOff) & 7u;
          }
        }
      }
    }
    uint32_t nb[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; k++) nb[k] = nullAt[k] ? *nullAt[k] : 0xFFu;
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
      const int64_t i = base + k * kBlock + threadIdx.x;
      if (i < n) {
        if (nullAt[k]) v[k].ok = (nb[k] >> nullBit[k]) & 1u;
        sink_store32(s, static_cast<uint32_t>(i), static_cast<uint32_t>(i), unary32(Noop, p.I, cvt32(v[k], a.kind, p.I)), p.rk);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// wide value path (Int64 / UUID / GeoPoint first operand): rare, one element per lane
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ WVal load_wide(const OperandD &op, uint32_t i, uint32_t row, const uint32_t *baseCounts,
                                          uint32_t startCount) {
  WVal r;
  r.lo = r.hi = 0;
  r.ok = 0;
  const int w = op.kind == K_UUID ? 16 : 8;
  switch (op.type) {
    case OP_CONST:
      r.lo = op.c64[0]; r.hi = op.c64[1]; r.ok = op.cok;
      return r;
    case OP_SCRATCH:
      r.lo = *reinterpret_cast<const uint64_t *>(op.base + static_cast<size_t>(w) * i);
      if (w == 16) r.hi = *reinterpret_cast<const uint64_t *>(op.base + static_cast<size_t>(w) * i + 8);
      r.ok = op.base[op.nullsOff + i] != 0;
      return r;
    case OP_COLUMN: {
      const uint32_t p = locate(op, row, baseCounts, startCount);
      const uint8_t *v = op.base + op.valuesOff + static_cast<size_t>(w) * p;
      r.lo = *reinterpret_cast<const uint64_t *>(v);
      if (w == 16) r.hi = *reinterpret_cast<const uint64_t *>(v + 8);
      r.ok = op.mode >= 2 ? get_bit(op.base + op.nullsOff, p + op.bitOff) : 1u;
      return r;
    }
    default: {
      const RecordID rid = op.rids[i];
      if (rid.batchID != 0 && (rid.batchID - op.baseBatchID < op.numBatches - 1 ||
                               rid.index < static_cast<uint32_t>(op.numRecLast))) {
        const ForeignBatchD b = op.batches[rid.batchID - op.baseBatchID];
        if (b.isConst) { r.lo = op.c64[0]; r.hi = op.c64[1]; r.ok = op.cok; return r; }
        const uint8_t *v = b.base + b.valuesOff + static_cast<size_t>(w) * rid.index;
        r.lo = *reinterpret_cast<const uint64_t *>(v);
        if (w == 16) r.hi = *reinterpret_cast<const uint64_t *>(v + 8);
        r.ok = b.valuesOff != 0 ? get_bit(b.base + b.nullsOff, rid.index + b.bitOff) : 1u;
      }
      return r;
    }
  }
}

__device__ __forceinline__ void store_from_i64(const SinkD &s, uint32_t i, uint32_t row, int64_t v, uint32_t ok) {
  uint8_t *dst = s.values + static_cast<size_t>(s.width) * i;
  if (s.type == SINK_PRED) { s.values[i] = v != 0; return; }
  if (s.type == SINK_MEASURE) {
    if (!ok) {
      if (s.width == 8) *reinterpret_cast<uint64_t *>(dst) = s.identity;
      else *reinterpret_cast<uint32_t *>(dst) = static_cast<uint32_t>(s.identity);
      return;
    }
    const bool isAvg = s.agg == AGGR_AVG_FLOAT;
    uint32_t count = 1;
    if ((isAvg || (s.agg >= AGGR_SUM_UNSIGNED && s.agg <= AGGR_SUM_FLOAT)) && s.baseCounts)
      count = s.baseCounts[row + 1] - s.baseCounts[row];
    if (isAvg) {
      float f;
      switch (s.dtype) {
        case Float64: f = static_cast<float>(static_cast<double>(v)); break;
        case Int32: f = static_cast<float>(static_cast<int32_t>(v)); break;
        case Uint32: f = static_cast<float>(static_cast<uint32_t>(v)); break;
        default: f = static_cast<float>(v); break;
      }
      reinterpret_cast<uint32_t *>(dst)[0] = f_bits(f);
      reinterpret_cast<uint32_t *>(dst)[1] = count;
      return;
    }
    switch (s.dtype) {
      case Int32: case Uint32: *reinterpret_cast<uint32_t *>(dst) = static_cast<uint32_t>(v) * count; break;
      case Float32: *reinterpret_cast<float *>(dst) = static_cast<float>(v) * static_cast<float>(count); break;
      case Int64: *reinterpret_cast<uint64_t *>(dst) = static_cast<uint64_t>(v) * count; break;
      default: *reinterpret_cast<double *>(dst) = static_cast<double>(v) * static_cast<double>(count); break;
    }
    return;
  }
  switch (s.dtype) {
    case Bool: *dst = v != 0; break;
    case Int8: case Uint8: *dst = static_cast<uint8_t>(v); break;
    case Int16: case Uint16: *reinterpret_cast<uint16_t *>(dst) = static_cast<uint16_t>(v); break;
    case Int32: case Uint32: *reinterpret_cast<uint32_t *>(dst) = static_cast<uint32_t>(v); break;
    case Float32: *reinterpret_cast<float *>(dst) = static_cast<float>(v); break;
    case Int64: *reinterpret_cast<int64_t *>(dst) = v; break;
    default: break;
  }
  s.nulls[i] = ok ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void transform_wide_kernel(EvalParams p, SinkD s, int n) {
  for (int64_t i64 = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i64 < n;
       i64 += static_cast<int64_t>(gridDim.x) * kBlock) {
    const uint32_t i = static_cast<uint32_t>(i64);
    const uint32_t row = p.needRow ? p.idx[i] : i;
    const WVal a = load_wide(p.a, i, row, p.baseCounts, p.startCount);
    const int K = p.a.kind;
    const int ft = p.functor;
    const bool sinkWide = s.type != SINK_PRED && s.type != SINK_MEASURE && (s.dtype == UUID || s.dtype == GeoPoint);
    if (p.arity == 2) {  // only Equal against a constant of the same kind (functor.hpp:1079-1133)
      DVal r;
      r.bits = 0;
      r.ok = 0;
      if (!sinkWide && ft == Equal) {
        const WVal b = load_wide(p.b, i, row, p.baseCounts, p.startCount);
        r.ok = a.ok && b.ok;
        if (r.ok) {
          if (K == K_UUID) r.bits = a.lo == b.lo && a.hi == b.hi;
          else {
            const float alat = bits_f(static_cast<uint32_t>(a.lo)), along = bits_f(static_cast<uint32_t>(a.lo >> 32));
            const float blat = bits_f(static_cast<uint32_t>(b.lo)), blong = bits_f(static_cast<uint32_t>(b.lo >> 32));
            r.bits = alat == blat && along == blong;
          }
        }
      }
      sink_store32(s, i, row, r, K_BOOL);
      continue;
    }
    if (K == K_UUID || K == K_GEO) {
      if (sinkWide) {  // X -> X is a copy, anything else (zero, null) (functor.hpp:800-881)
        const bool same = (K == K_UUID) == (s.dtype == UUID);
        uint8_t *dst = s.values + static_cast<size_t>(s.width) * i;
        reinterpret_cast<uint64_t *>(dst)[0] = same ? a.lo : 0;
        if (s.width == 16) reinterpret_cast<uint64_t *>(dst)[1] = same ? a.hi : 0;
        s.nulls[i] = (same && a.ok) ? 1 : 0;
        continue;
      }
      DVal r;
      r.bits = 0;
      r.ok = 0;
      if (K == K_UUID && ft == GetHLLValue && a.ok) {
        r.bits = hll_from_hash(a.lo ^ a.hi);
        r.ok = 1;
      }
      sink_store32(s, i, row, r, K_U32);
      continue;
    }
    // Int64 input: the generic unary functor (functor.hpp:660-697)
    if (sinkWide) {
      uint8_t *dst = s.values + static_cast<size_t>(s.width) * i;
      reinterpret_cast<uint64_t *>(dst)[0] = 0;
      if (s.width == 16) reinterpret_cast<uint64_t *>(dst)[1] = 0;
      s.nulls[i] = 0;
      continue;
    }
    const int64_t v = static_cast<int64_t>(a.lo);
    DVal r;
    switch (ft) {
      case Not: r.ok = a.ok; r.bits = a.ok ? (v == 0) : 0; sink_store32(s, i, row, r, K_BOOL); continue;
      case IsNull: r.ok = 1; r.bits = !a.ok; sink_store32(s, i, row, r, K_BOOL); continue;
      case IsNotNull: r.ok = 1; r.bits = a.ok != 0; sink_store32(s, i, row, r, K_BOOL); continue;
      case Negate: store_from_i64(s, i, row, a.ok ? static_cast<int64_t>(0ull - a.lo) : 0, a.ok); continue;
      case BitwiseNot: store_from_i64(s, i, row, a.ok ? ~v : 0, a.ok); continue;
      case GetHLLValue: {
        r.ok = a.ok;
        r.bits = 0;
        if (a.ok) {
          uint64_t q[2] = {a.lo, 0};
          r.bits = hll_from_hash(murmur3_128_lo<2>(q, 8, 0));
        }
        sink_store32(s, i, row, r, K_U32);
        continue;
      }
      default: break;
    }
    if (ft >= GetWeekStart && ft <= GetQuarterOfYear) {
      DVal t;
      t.bits = static_cast<uint32_t>(a.lo);
      t.ok = a.ok;
      sink_store32(s, i, row, unary32(ft, K_U32, t), K_U32);
      continue;
    }
    store_from_i64(s, i, row, v, a.ok);  // Noop and unknown functors
  }
}

// ---------------------------------------------------------------------------------------------
// array columns: ArrayLength / ArrayContains / ArrayElementAt (query/iterator.hpp:377-451,
// query/functor.hpp:468-640).  An array column is [offset u32, length u32] x Length followed by the
// array values [length u32][elements][validity bits]; output position i reads array i — the
// reference binds the bare iterator, not one zipped with the index vector (binder.hpp:385-426).
// One lane per array: the descriptors load coalesced, the element walks are short and divergent.
// ---------------------------------------------------------------------------------------------
struct ArrayD {
  const uint8_t *descriptors;  // OffsetLengthVector
  const uint8_t *values;       // descriptors + 8 * Length - ValueOffsetAdj
  int dtype, kind, width;      // element type
  int functor;                 // ArrayLength / ArrayContains / ArrayElementAt
  int enabled;                 // 0: the functor / sink / constant combination yields null everywhere
  int index;                   // ArrayElementAt
  uint64_t c[2];               // ArrayContains: the constant, already cast to the element type
  const uint32_t *idx;         // rows for a measure sink's run lengths
};

__device__ __forceinline__ bool array_elem_equals(const ArrayD &a, const uint8_t *e) {
  switch (a.dtype) {
    case Bool: return (*e != 0) == (a.c[0] != 0);
    case Int8: case Uint8: return *e == static_cast<uint8_t>(a.c[0]);
    case Int16: case Uint16: return *reinterpret_cast<const uint16_t *>(e) == static_cast<uint16_t>(a.c[0]);
    case Int32: case Uint32: return *reinterpret_cast<const uint32_t *>(e) == static_cast<uint32_t>(a.c[0]);
    case Float32: return bits_f(*reinterpret_cast<const uint32_t *>(e)) == bits_f(static_cast<uint32_t>(a.c[0]));
    case Int64: {  // elements start 4 bytes into an 8-byte aligned value: read words
      const uint32_t *w = reinterpret_cast<const uint32_t *>(e);
      return w[0] == static_cast<uint32_t>(a.c[0]) && w[1] == static_cast<uint32_t>(a.c[0] >> 32);
    }
    case GeoPoint: {
      const uint32_t *w = reinterpret_cast<const uint32_t *>(e);
      return bits_f(w[0]) == bits_f(static_cast<uint32_t>(a.c[0])) && bits_f(w[1]) == bits_f(static_cast<uint32_t>(a.c[0] >> 32));
    }
    default: {  // UUID
      const uint32_t *w = reinterpret_cast<const uint32_t *>(e);
      return w[0] == static_cast<uint32_t>(a.c[0]) && w[1] == static_cast<uint32_t>(a.c[0] >> 32) &&
             w[2] == static_cast<uint32_t>(a.c[1]) && w[3] == static_cast<uint32_t>(a.c[1] >> 32);
    }
  }
}

__global__ __launch_bounds__(kBlock) void array_transform_kernel(ArrayD a, SinkD s, int n) {
  const bool sinkWide = s.type != SINK_PRED && s.type != SINK_MEASURE && (s.dtype == UUID || s.dtype == GeoPoint);
  for (int64_t i64 = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i64 < n;
       i64 += static_cast<int64_t>(gridDim.x) * kBlock) {
    const uint32_t i = static_cast<uint32_t>(i64);
    const uint32_t row = a.idx ? a.idx[i] : i;
    DVal r;
    r.bits = 0;
    r.ok = 0;
    int rk = K_U32;
    if (a.enabled) {
      const uint2 d = *reinterpret_cast<const uint2 *>(a.descriptors + 8ull * i);  // {offset, length}
      const uint8_t *value = d.y ? a.values + d.x : nullptr;
      const bool present = d.y != 0 || d.x != 0;  // (0, 0) is a null array, (x, 0) an empty one
      if (a.functor == ArrayLength) {
        r.ok = present;
        if (value) r.bits = *reinterpret_cast<const uint32_t *>(value);
      } else if (a.functor == ArrayContains) {
        rk = K_BOOL;
        r.ok = present;
        const int len = value ? static_cast<int>(*reinterpret_cast<const uint32_t *>(value)) : 0;
        if (len > 0) {
          const uint8_t *elems = value + 4, *valid = elems + static_cast<size_t>(a.width) * static_cast<uint32_t>(len);
          for (int j = 0; j < len; j++)
            if (((valid[j >> 3] >> (j & 7)) & 1) && array_elem_equals(a, elems + static_cast<size_t>(a.width) * j)) {
              r.bits = 1;
              break;
            }
        }
      } else if (value) {  // ArrayElementAt (functor.hpp:536-571): a negative index counts from the end
        const uint32_t ulen = *reinterpret_cast<const uint32_t *>(value);
        int index = a.index;
        const bool out = (index >= 0 && ulen <= static_cast<uint32_t>(index)) || (index < 0 && ulen < static_cast<uint32_t>(-index));
        const int len = static_cast<int>(ulen);
        if (index < 0) index = len + index;
        const uint8_t *elems = value + 4, *valid = elems + static_cast<size_t>(a.width) * ulen;
        if (!out && len != 0 && index < len && index >= 0 && ((valid[index >> 3] >> (index & 7)) & 1)) {
          const uint8_t *e = elems + static_cast<size_t>(a.width) * index;
          if (a.kind == K_UUID || a.kind == K_GEO) {  // only into a sink of its own type (checked on the host)
            uint8_t *dst = s.values + static_cast<size_t>(s.width) * i;
            const uint32_t *w = reinterpret_cast<const uint32_t *>(e);
            for (int k = 0; k < a.width / 4; k++) reinterpret_cast<uint32_t *>(dst)[k] = w[k];
            s.nulls[i] = 1;
            continue;
          }
          if (a.kind == K_I64) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(e);
            const int64_t v = static_cast<int64_t>(static_cast<uint64_t>(w[0]) | (static_cast<uint64_t>(w[1]) << 32));
            if (sinkWide) {
              sink_store32(s, i, row, r, rk);
            } else {
              store_from_i64(s, i, row, v, 1u);
            }
            continue;
          }
          r.ok = 1;
          rk = a.kind;
          switch (a.dtype) {
            case Bool: r.bits = *e != 0; break;
            case Int8: r.bits = static_cast<uint32_t>(static_cast<int32_t>(*reinterpret_cast<const int8_t *>(e))); break;
            case Uint8: r.bits = *e; break;
            case Int16: r.bits = static_cast<uint32_t>(static_cast<int32_t>(*reinterpret_cast<const int16_t *>(e))); break;
            case Uint16: r.bits = *reinterpret_cast<const uint16_t *>(e); break;
            default: r.bits = *reinterpret_cast<const uint32_t *>(e); break;
          }
        }
      }
    }
    sink_store32(s, i, row, r, rk);
  }
}

// ---------------------------------------------------------------------------------------------
// filter: fused predicate + stable in-place compaction (decoupled look-back)
// ---------------------------------------------------------------------------------------------
constexpr int kFilterItems = 8;
constexpr int kFilterTile = kBlock * kFilterItems;
struct ScanWorkspace {
  unsigned int *ticket;  // next tile to process
  uint32_t *total;       // number of survivors
  uint32_t *error;       // raised when a look-back spin times out
  uint64_t *status;      // one word per tile: flag | count
};

// MODE 0: evaluate the predicate from the operands, write pred[], compact idx
// MODE 1: read pred[], compact one RecordID vector (8-byte payload)
// MODE 2: read pred[] (already evaluated by the wide-value kernel), compact idx
template <int MODE>
__global__ __launch_bounds__(kBlock) void filter_kernel(EvalParams p, uint8_t *pred, uint32_t *idx, uint64_t *rids,
                                                        ScanWorkspace ws, int n, int numTiles) {
  __shared__ uint32_t sCounts[kFilterItems * kWaves + 1];
  __shared__ int sTile;
  __shared__ uint32_t sBase;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t ltMask = (1ull << lane) - 1;
  for (;;) {
    __syncthreads();  // sTile / sCounts are reused from the previous tile
    if (threadIdx.x == 0) sTile = static_cast<int>(atomicAdd(ws.ticket, 1u));
    __syncthreads();
    const int tile = sTile;
    if (tile >= numTiles) break;
    const int64_t base = static_cast<int64_t>(tile) * kFilterTile;

    uint32_t rows[kFilterItems];
    uint64_t payload[MODE == 1 ? kFilterItems : 1];
    uint32_t keep[kFilterItems];
    if (MODE == 0) {
      DVal va[kFilterItems], vb[kFilterItems];
#pragma unroll
      for (int k = 0; k < kFilterItems; k++) {
        const int64_t i = base + k * kBlock + threadIdx.x;
        rows[k] = i < n ? idx[i] : 0u;
      }
#pragma unroll
      for (int k = 0; k < kFilterItems; k++) {
        const int64_t i = base + k * kBlock + threadIdx.x;
        if (i < n) {
          va[k] = load32(p.a, static_cast<uint32_t>(i), rows[k], p.baseCounts, p.startCount);
          if (p.arity == 2) vb[k] = load32(p.b, static_cast<uint32_t>(i), rows[k], p.baseCounts, p.startCount);
        }
      }
#pragma unroll
      for (int k = 0; k < kFilterItems; k++) {
        const int64_t i = base + k * kBlock + threadIdx.x;
        keep[k] = 0;
        if (i < n) {
          DVal x = cvt32(va[k], p.a.kind, p.I);
          DVal r = p.arity == 1 ? unary32(p.functor, p.I, x)
                                : binary32(p.functor, p.I, x, cvt32(vb[k], p.b.kind, p.I));
          keep[k] = cvt32(r, p.rk, K_BOOL).bits;  // validity is ignored (functor.hpp:903-915)
          pred[i] = static_cast<uint8_t>(keep[k]);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < kFilterItems; k++) {
        const int64_t i = base + k * kBlock + threadIdx.x;
        keep[k] = i < n ? pred[i] : 0u;
        if (MODE == 1) payload[k] = i < n ? rids[i] : 0ull;
        else rows[k] = i < n ? idx[i] : 0u;
      }
    }
    // every input of this tile is in registers before the tile's count becomes visible: later
    // tiles only start overwriting our input range after they have seen our status word
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    uint32_t rank[kFilterItems];
#pragma unroll
    for (int k = 0; k < kFilterItems; k++) {
      const uint64_t m = __ballot(keep[k] != 0);
      rank[k] = __popcll(m & ltMask);
      if (lane == 0) sCounts[k * kWaves + wave] = __popcll(m);
    }
    __syncthreads();
    if (wave == 0) {
      // exclusive scan of the kFilterItems*kWaves (=32) partial counts, position order
      uint32_t c = lane < kFilterItems * kWaves ? sCounts[lane] : 0u;
      uint32_t incl = c;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
      }
      const uint32_t tileCount = __shfl(incl, 63);
      if (lane == 0) st_status(ws.status + tile, (tile == 0 ? kFlagInclusive : kFlagAggregate) | tileCount);
      uint32_t exclusive = 0;
      if (tile > 0) {
        exclusive = static_cast<uint32_t>(lookback_wave(ws.status, tile, lane, ws.error));
        if (lane == 0) st_status(ws.status + tile, kFlagInclusive | (exclusive + tileCount));
      }
      if (lane < kFilterItems * kWaves) sCounts[lane] = incl - c;
      if (lane == 0) {
        sBase = exclusive;
        if (tile == numTiles - 1) *ws.total = exclusive + tileCount;
      }
    }
    __syncthreads();
    const uint32_t blockBase = sBase;
#pragma unroll
    for (int k = 0; k < kFilterItems; k++) {
      if (keep[k]) {
        const uint32_t dst = blockBase + sCounts[k * kWaves + wave] + rank[k];
        if (MODE == 1) rids[dst] = payload[k];
        else idx[dst] = rows[k];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// lazy filter in ROW space: count + survivor bits, no predicate bytes, no index vector
// ---------------------------------------------------------------------------------------------
// While every filter of a batch so far is of the hot shape and nothing has read the index vector, the vector is still
// iota(0 .. n0) "with k filters pending": the survivors of filter k + 1 are the rows of the batch that pass filters
// 1 .. k + 1, whatever order compactions would have put them in.  This kernel evaluates ONE more filter over the batch's
// rows (rows = positions: no index vector is read), ANDs it with the survivors so far — one bit per row — and returns
// the count through one partial per workgroup: 4.1 B/row read + 0.13 B/row of bits each way, against predicate bytes,
// compaction and a gather through the compacted vector for every filter after the first (the Go host puts two time
// filters in front of every fact-table query's own filters, query/aql_processor.go:543-559).  Nothing observable is
// written: the predicate and index vectors are produced by replaying the filters with the kernels above when (if)
// somebody needs them (run_compaction).
// Survivor bits are kept in the kernel's own lane layout: the tile geometry of this file gives lane t of a workgroup the
// rows (1024 tile + 256 q + t) * 4 + j of quads q = 0..3 — 16 rows per lane and tile — so a tile's survivors are one
// 16-bit word per lane (bit 4 q + j), written and read back with ONE coalesced 2-byte access per lane and tile.  (A
// first version kept ballots — bit = lane — and paid 16 ballots, 16 population counts and 16 single-lane stores per
// wavefront and tile: 0.102 ms per 64 Mi rows against the 0.079 ms of the kernel that writes predicate bytes.)
// `TWO`: a second filter `g` over the SAME column is evaluated as well (the host predicts it from the previous batch of
// the stream: ts >= from is followed by ts < to); blockTotals holds two partials per workgroup, bitsOut2 the survivors
// of both.
template <bool TWO, bool HAS_IN>
__global__ __launch_bounds__(kBlock) void filter_rows_kernel(FastOperands f, FastOperands g, const uint16_t *bitsIn,
                                                             uint16_t *bitsOut, uint16_t *bitsOut2, int n, int numTiles,
                                                             uint32_t *blockTotals) {
  __shared__ uint32_t sTotal[2];
  if (threadIdx.x < 2) sTotal[threadIdx.x] = 0;
  uint32_t mine = 0, mine2 = 0;  // survivors among this lane's rows
  const int lane = threadIdx.x & 63;
  DVal y, z;
  y.bits = f.bbits;
  y.ok = f.bok;
  y = cvt32(y, f.bkind, f.I);
  z.bits = g.bbits;
  z.ok = g.bok;
  z = cvt32(z, g.bkind, g.I);
  for (int tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
    const int64_t tq = static_cast<int64_t>(tile) * (kBlock * kPQ);
    const size_t word = static_cast<size_t>(tile) * kBlock + threadIdx.x;
    uint32_t alive = 0xFFFFu;
    if (HAS_IN) alive = bitsIn[word];
    uint32_t rows[kPQ][4], vals[kPQ][4], okb[kPQ];
    load_quads<kPQ>(f, tq + threadIdx.x, n, rows, vals, okb);
    uint32_t in[kPQ], kbs[kPQ], kbs2[kPQ];
#pragma unroll
    for (int q = 0; q < kPQ; q++) {
      const int64_t i0 = (tq + threadIdx.x + static_cast<int64_t>(q) * kBlock) * 4;
      in[q] = 0xFu;
      if (i0 + 3 >= n) {
        in[q] = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) in[q] |= (i0 + j < n ? 1u : 0u) << j;
      }
    }
    compare_tile<kPQ>(f, vals, okb, in, y, kbs);  // result validity is ignored (functor.hpp:903-915)
    uint32_t k1 = 0;
#pragma unroll
    for (int q = 0; q < kPQ; q++) k1 |= kbs[q] << (4 * q);
    k1 &= alive;
    bitsOut[word] = static_cast<uint16_t>(k1);
    mine += __popc(k1);
    if (TWO) {
      compare_tile<kPQ>(g, vals, okb, in, z, kbs2);
      uint32_t k2 = 0;
#pragma unroll
      for (int q = 0; q < kPQ; q++) k2 |= kbs2[q] << (4 * q);
      k2 &= k1;
      bitsOut2[word] = static_cast<uint16_t>(k2);
      mine2 += __popc(k2);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mine += __shfl_xor(mine, off);
    if (TWO) mine2 += __shfl_xor(mine2, off);
  }
  __syncthreads();
  if (lane == 0) {
    if (mine) atomicAdd(&sTotal[0], mine);
    if (mine2) atomicAdd(&sTotal[1], mine2);
  }
  __syncthreads();
  if (threadIdx.x < 2) blockTotals[2 * blockIdx.x + threadIdx.x] = sTotal[threadIdx.x];
}

// ---------------------------------------------------------------------------------------------
// run-length encoded columns (archive batches), decoded once per batch
// ---------------------------------------------------------------------------------------------
// rows [0, n) of a mode-3 column — [counts u32 x (runs + 1)][validity bit per run][value per run], row r lives in the run that
// holds startCount + r (query/iterator.hpp:199-278; locate() of device_model.hpp) — written as [validity bit per row][value
// per row].  A lane decodes 32 consecutive rows: one binary search, then a walk along the counts; one validity word.
__global__ __launch_bounds__(kBlock) void expand_runs_kernel(const uint32_t *counts, int numRuns, const uint8_t *nulls, uint32_t bitOff,
                                                             const uint8_t *values, int step, uint32_t startCount, int n, uint32_t *outNulls,
                                                             uint8_t *outValues) {
  // A wavefront decodes 2048 consecutive rows: lane l walks rows [32 l, 32 l + 32) of the tile (values into LDS, row r at word
  // r + r / 32: the lanes' columns fall into different banks), then the tile leaves the CU as whole lines — lane l stores rows
  // l, l + 64, ... (the first version stored each lane's 128 bytes where the lane walked: 64 scattered 4-byte stores per
  // instruction, 0.90 ms per 64 Mi rows instead of 0.1).
  __shared__ uint32_t sTile[kBlock / 64][2048 + 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t *tile = sTile[wave];
  const int64_t tiles = (static_cast<int64_t>(n) + 2047) / 2048;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave; t < tiles; t += static_cast<int64_t>(gridDim.x) * (kBlock / 64)) {
    const int64_t w = t * 64 + lane;  // this lane's validity word = its 32 rows
    const int64_t r0 = w * 32;
    uint32_t okWord = 0;
    if (r0 < n) {
      const uint32_t x0 = startCount + static_cast<uint32_t>(r0);
      uint32_t first = 0, last = static_cast<uint32_t>(numRuns);
      while (first < last) {
        const uint32_t mid = first + ((last - first) >> 1);
        if (counts[mid] > x0) last = mid; else first = mid + 1;
      }
      uint32_t run = first ? first - 1 : 0u, next = run + 1 < static_cast<uint32_t>(numRuns) ? counts[run + 1] : 0xFFFFFFFFu;
      uint32_t v = step == 4 ? reinterpret_cast<const uint32_t *>(values)[run] : step == 2 ? reinterpret_cast<const uint16_t *>(values)[run] : values[run];
      uint32_t ok = nulls ? get_bit(nulls, run + bitOff) : 1u;
      for (int j = 0; j < 32; j++) {
        const uint32_t x = x0 + static_cast<uint32_t>(j);
        if (x >= next) {
          while (run + 1 < static_cast<uint32_t>(numRuns) && counts[run + 1] <= x) run++;
          next = run + 1 < static_cast<uint32_t>(numRuns) ? counts[run + 1] : 0xFFFFFFFFu;
          v = step == 4 ? reinterpret_cast<const uint32_t *>(values)[run] : step == 2 ? reinterpret_cast<const uint16_t *>(values)[run] : values[run];
          ok = nulls ? get_bit(nulls, run + bitOff) : 1u;
        }
        okWord |= ok << j;
        tile[33 * lane + j] = v;
      }
      if (r0 + 32 > n) okWord &= (1u << static_cast<uint32_t>(n - r0)) - 1u;  // (rows past the end: no bits)
      outNulls[w] = okWord;
    }
    __builtin_amdgcn_wave_barrier();
    const int64_t base = t * 2048;
#pragma unroll 4
    for (int k = 0; k < 32; k++) {
      const int rr = k * 64 + lane;
      const int64_t r = base + rr;
      if (r < n) {
        const uint32_t v = tile[rr + (rr >> 5)];
        if (step == 4) reinterpret_cast<uint32_t *>(outValues)[r] = v;
        else if (step == 2) reinterpret_cast<uint16_t *>(outValues)[r] = static_cast<uint16_t>(v);
        else outValues[r] = static_cast<uint8_t>(v);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace ares
