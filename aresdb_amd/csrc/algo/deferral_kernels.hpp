// The kernels the deferral state machine launches when it WRITES a definition (deferral.hip): a lazy iota, a lazy fill,
// queued root transforms, the two-phase compaction of an index vector.  Included by deferral.hip only: kernels are not
// static, so every __global__ is defined in exactly one translation unit.  (The kernels of the calls themselves:
// transform_kernels.hpp.)
#pragma once

#include "lookback.hpp"
#include "quad_geometry.hpp"

namespace ares {

// ---------------------------------------------------------------------------------------------
// InitIndexVector
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void init_index_kernel(uint32_t *idx, uint32_t start, int n) {
  // 4 consecutive entries per lane -> one 16-byte store per lane
  const int64_t quads = (static_cast<int64_t>(n) + 3) >> 2;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; q < quads;
       q += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t i = q << 2;
    const uint32_t v = start + static_cast<uint32_t>(i);
    if (i + 3 < n && (reinterpret_cast<uintptr_t>(idx) & 15) == 0) {
      *reinterpret_cast<uint4 *>(idx + i) = make_uint4(v, v + 1, v + 2, v + 3);
    } else {
      for (int k = 0; k < 4 && i + k < n; k++) idx[i + k] = v + k;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// fast transform: 32-bit column (x constant) -> 4-byte dimension / scratch vector or measure
// ---------------------------------------------------------------------------------------------
struct __attribute__((packed, aligned(1))) PU32s { uint32_t v; };

// evaluates and stores one tile (kTQ quads per lane) of one transform whose rows are already loaded;
// ALIGNED_NULLS: the quad grid was shifted so that the 4 validity bytes form an aligned dword
template <int QUADS, bool ALIGNED_NULLS>
__device__ __forceinline__ void store_tile(const FastOperands &f, const SinkD &s, int pad, int64_t quad0, int n,
                                           const uint32_t (&rows)[QUADS][4], const uint32_t (&vals)[QUADS][4],
                                           const uint32_t (&okb)[QUADS]) {
  DVal y;
  y.bits = f.bbits;
  y.ok = f.bok;
  y = cvt32(y, f.bkind, f.I);
  const uint32_t ymag = (f.I == K_I32 && static_cast<int32_t>(y.bits) < 0) ? 0u - y.bits : y.bits;
  const FastDivisor fd = make_fast_divisor(ymag);
#pragma unroll
  for (int q = 0; q < QUADS; q++) {
    const int64_t i0 = (quad0 + static_cast<int64_t>(q) * kBlock) * 4 - pad;
    DVal r[4];
    {
      uint32_t rb[4];
      const uint32_t rok = eval_quad(f, vals[q], okb[q], y, fd, rb);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        r[j].bits = rb[j];
        r[j].ok = (rok >> j) & 1u;
      }
    }
    const bool full = i0 >= 0 && i0 + 3 < n;
    if (!full) {  // ragged first / last quad (or past the end): the generic element-wise sink
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int64_t i = i0 + j;
        if (i >= 0 && i < n) sink_store32(s, static_cast<uint32_t>(i), rows[q][j], r[j], f.rk);
      }
    } else if (s.type == SINK_MEASURE) {
      if (s.width == 8) {
        uint64_t o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (!r[j].ok) o[j] = s.identity;
          else if (s.agg == AGGR_AVG_FLOAT) o[j] = (1ull << 32) | f_bits(avg_measure_float(s.dtype, r[j], f.rk));  // {average, count 1}
          else if (s.dtype == Float64) o[j] = static_cast<uint64_t>(__double_as_longlong(to_double32(r[j], f.rk)));
          else o[j] = static_cast<uint64_t>(f.rk == K_F32 ? static_cast<int64_t>(bits_f(r[j].bits))
                                            : f.rk == K_I32 ? static_cast<int64_t>(static_cast<int32_t>(r[j].bits))
                                                            : static_cast<int64_t>(r[j].bits));
        }
        U64x2 lo, hi;
        lo.v[0] = o[0]; lo.v[1] = o[1]; hi.v[0] = o[2]; hi.v[1] = o[3];
        U64x2 *dst = reinterpret_cast<U64x2 *>(s.values + static_cast<size_t>(8) * i0);
        dst[0] = lo;
        dst[1] = hi;
      } else {
        U32x4 o;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (!r[j].ok) o.v[j] = static_cast<uint32_t>(s.identity);
          else o.v[j] = cvt32(r[j], f.rk, s.dtype == Int32 ? K_I32 : s.dtype == Uint32 ? K_U32 : K_F32).bits;
        }
        *reinterpret_cast<U32x4 *>(s.values + static_cast<size_t>(4) * i0) = o;
      }
    } else if (s.width < 4) {  // 1- / 2-byte dimension slot (integer kinds only, see fast_sink): the value truncated, as store_typed32
      uint32_t nb = 0, lo = 0, hi = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) nb |= (r[j].ok ? 1u : 0u) << (8 * j);
      if (s.width == 2) {
        lo = (r[0].bits & 0xFFFFu) | (r[1].bits << 16);
        hi = (r[2].bits & 0xFFFFu) | (r[3].bits << 16);
        PU32x2 o;
        o.v[0] = lo; o.v[1] = hi;
        *reinterpret_cast<PU32x2 *>(s.values + static_cast<size_t>(2) * i0) = o;
      } else {
        lo = (r[0].bits & 0xFFu) | ((r[1].bits & 0xFFu) << 8) | ((r[2].bits & 0xFFu) << 16) | (r[3].bits << 24);
        reinterpret_cast<PU32s *>(s.values + i0)->v = lo;
      }
      if (ALIGNED_NULLS) *reinterpret_cast<uint32_t *>(s.nulls + i0) = nb;
      else reinterpret_cast<PU32s *>(s.nulls + i0)->v = nb;
    } else {  // 4-byte dimension / scratch value + one validity byte per row
      const int ok_kind = s.dtype == Int32 ? K_I32 : s.dtype == Uint32 ? K_U32 : K_F32;
      U32x4 o;
      uint32_t nb = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        o.v[j] = cvt32(r[j], f.rk, ok_kind).bits;
        nb |= (r[j].ok ? 1u : 0u) << (8 * j);
      }
      *reinterpret_cast<U32x4 *>(s.values + static_cast<size_t>(4) * i0) = o;
      if (ALIGNED_NULLS) *reinterpret_cast<uint32_t *>(s.nulls + i0) = nb;  // pad = nulls address & 3
      else reinterpret_cast<PU32s *>(s.nulls + i0)->v = nb;                // byte-aligned dword store
    }
  }
}

__global__ __launch_bounds__(kBlock) void transform_fast_kernel(FastOperands f, SinkD s, int n, int64_t numQuads) {
  const int64_t tileQuads = static_cast<int64_t>(kBlock) * kTQ;
  for (int64_t tq = static_cast<int64_t>(blockIdx.x) * tileQuads; tq < numQuads;
       tq += static_cast<int64_t>(gridDim.x) * tileQuads) {
    uint32_t rows[kTQ][4], vals[kTQ][4], okb[kTQ];
    load_rows<kTQ>(f.idx, f.pad, tq + threadIdx.x, n, rows);
    load_values<kTQ>(f, f.pad, tq + threadIdx.x, n, rows, vals, okb);
    if (f.chain.n) apply_chain<kTQ>(f, vals);  // (a constant chain: launch-uniform, the chain-free path is as it was)
    store_tile<kTQ, true>(f, s, f.pad, tq + threadIdx.x, n, rows, vals, okb);
  }
}

// Several transforms of one batch over the same index vector in ONE pass (cross-call fusion, see
// include/ares_extensions.h): the index vector is read once per tile, each job then reads its own
// column and writes its own sink.  The quad grid is unshifted (pad 0): validity bytes use
// byte-aligned dword stores.  (Measured: running the jobs one after the other per tile, 16 rows per
// lane each, beats issuing every job's loads up front — 4.4 vs 3.2 TB/s on BASELINE config C3.)
__global__ __launch_bounds__(kBlock, 3) void transform_multi_kernel(MultiJobs jobs, const uint32_t *idx, int n, int64_t numQuads) {
  const int64_t tileQuads = static_cast<int64_t>(kBlock) * kTQ;
  for (int64_t tq = static_cast<int64_t>(blockIdx.x) * tileQuads; tq < numQuads;
       tq += static_cast<int64_t>(gridDim.x) * tileQuads) {
    uint32_t rows[kTQ][4];
    load_rows<kTQ>(idx, 0, tq + threadIdx.x, n, rows);
    for (int j = 0; j < jobs.count; j++) {
      uint32_t vals[kTQ][4], okb[kTQ];
      load_values<kTQ>(jobs.f[j], 0, tq + threadIdx.x, n, rows, vals, okb);
      if (jobs.f[j].chain.n) apply_chain<kTQ>(jobs.f[j], vals);
      store_tile<kTQ, false>(jobs.f[j], jobs.s[j], 0, tq + threadIdx.x, n, rows, vals, okb);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// two-phase filter: predicate + per-tile counts, scan, in-place compaction without a chain
// ---------------------------------------------------------------------------------------------
// A one-pass kernel is bound by the latency of its per-tile chain (index -> column loads,
// ranking, look-back, staging).  Splitting it removes every inter-tile dependency from the hot
// loops: (1) a streaming kernel evaluates the predicate, writes the predicate bytes and one
// survivor count per 4096-row tile; (2) a single small workgroup turns the counts into offsets;
// (3) the compaction kernel re-reads predicate bytes + index vector and writes each tile's
// survivors at its known offset.  In-place safety in (3): a tile writes only after every tile whose
// INPUT range overlaps its OUTPUT range has flagged "loaded" (those are earlier tiles, claimed
// earlier by running workgroups through the ticket, so the wait cannot deadlock); with a virtual
// index vector (rows = position, see the iota registry below) nothing is read from the index
// vector and no wait is needed.  Traffic: 9.1 + 8.6 B/row instead of 12.7, at streaming speed.
// blockTotals (not null): one word per workgroup receives the survivors of its tiles — the host adds them up, so that
// the count a filter returns does not wait for the scan of the tile counts (only a compaction needs the offsets) and no
// word is the target of thousands of atomics (4096 workgroups adding to ONE word measured +0.017 ms on a 0.113 ms kernel).
__global__ __launch_bounds__(kBlock) void filter_pred_kernel(FastOperands f, uint8_t *pred, uint32_t *tileCounts, int n,
                                                             int numTiles, uint32_t *blockTotals) {
  __shared__ uint32_t sTotal;
  if (threadIdx.x == 0) sTotal = 0;
  uint32_t mine = 0;  // lane 0 of each wavefront: survivors of the tiles this workgroup has seen
  const int lane = threadIdx.x & 63;
  DVal y;
  y.bits = f.bbits;
  y.ok = f.bok;
  y = cvt32(y, f.bkind, f.I);
  for (int tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
    const int64_t tq = static_cast<int64_t>(tile) * (kBlock * kPQ);
    uint32_t rows[kPQ][4], vals[kPQ][4], okb[kPQ];
    load_quads<kPQ>(f, tq + threadIdx.x, n, rows, vals, okb);
    uint32_t count = 0, in[kPQ], kbs[kPQ];
#pragma unroll
    for (int q = 0; q < kPQ; q++) {
      const int64_t i0 = (tq + threadIdx.x + static_cast<int64_t>(q) * kBlock) * 4 - f.pad;
      in[q] = 0xFu;
      if (i0 < 0 || i0 + 3 >= n) {
        in[q] = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) in[q] |= ((i0 + j >= 0 && i0 + j < n) ? 1u : 0u) << j;
      }
    }
    compare_tile<kPQ>(f, vals, okb, in, y, kbs);  // result validity is ignored (functor.hpp:903-915)
#pragma unroll
    for (int q = 0; q < kPQ; q++) {
      const int64_t i0 = (tq + threadIdx.x + static_cast<int64_t>(q) * kBlock) * 4 - f.pad;
      const uint32_t kb = kbs[q];
      count += __popc(kb);
      const uint32_t bytes = (kb & 1u) | ((kb & 2u) << 7) | ((kb & 4u) << 14) | ((kb & 8u) << 21);
      if (i0 >= 0 && i0 + 3 < n) {
        *reinterpret_cast<uint32_t *>(pred + i0) = bytes;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (i0 + j >= 0 && i0 + j < n) pred[i0 + j] = static_cast<uint8_t>((kb >> j) & 1u);
      }
    }
    // one atomic per wavefront into the (zeroed) tile count: no workgroup barrier in this kernel
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
    if (lane == 0 && count) atomicAdd(tileCounts + tile, count);
    mine += count;
  }
  if (!blockTotals) return;
  __syncthreads();
  if (lane == 0 && mine) atomicAdd(&sTotal, mine);
  __syncthreads();
  if (threadIdx.x == 0) blockTotals[blockIdx.x] = sTotal;
}

// exclusive scan of the tile counts by ONE workgroup (numTiles <= a few hundred thousand)
__global__ __launch_bounds__(1024) void filter_scan_kernel(const uint32_t *tileCounts, uint32_t *tileOffsets, int numTiles,
                                                           uint32_t *total) {
  constexpr int kPer = 8;  // consecutive tiles per lane
  __shared__ uint32_t sWave[16];
  __shared__ uint32_t sCarry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) sCarry = 0;
  __syncthreads();
  for (int base = 0; base < numTiles; base += 1024 * kPer) {
    const int t0 = base + threadIdx.x * kPer;
    uint32_t c[kPer], mine = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
      c[k] = t0 + k < numTiles ? tileCounts[t0 + k] : 0u;
      mine += c[k];
    }
    uint32_t incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t v = __shfl_up(incl, off);
      if (lane >= off) incl += v;
    }
    if (lane == 63) sWave[wave] = incl;
    __syncthreads();
    uint32_t before = sCarry;
    for (int w = 0; w < wave; w++) before += sWave[w];
    uint32_t run = before + incl - mine;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
      if (t0 + k < numTiles) tileOffsets[t0 + k] = run;
      run += c[k];
    }
    __syncthreads();
    if (threadIdx.x == 1023) sCarry = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    tileOffsets[numTiles] = sCarry;
    *total = sCarry;
  }
}

// PAYLOAD: uint32_t (index vector) or uint64_t (RecordID vector).  VIRTUAL: the index vector is
// iota(start) and has not been materialised: nothing is read from it.
template <typename PAYLOAD, bool VIRTUAL>
__global__ __launch_bounds__(kBlock) void filter_compact_kernel(const uint8_t *pred, PAYLOAD *data, uint32_t iotaStart, int pad,
                                                                CompactWorkspace ws, int n, int numTiles) {
  __shared__ PAYLOAD sOut[kPTile];
  __shared__ uint32_t sCounts[kPQ * kWaves];
  __shared__ int sTicket;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) sTicket = static_cast<int>(atomicAdd(ws.ticket, 1u));
    __syncthreads();
    const int firstTile = sTicket * kTilesPerTicket;
    if (firstTile >= numTiles) break;
    // phase A: the input of ALL tiles of this ticket goes to registers, then they are flagged
    // "loaded" at once — nobody ever waits for a tile this workgroup has not reached yet
    PAYLOAD rows[kTilesPerTicket][kPQ][4];
    uint32_t keep[kTilesPerTicket];
#pragma unroll
    for (int tt = 0; tt < kTilesPerTicket; tt++) {
      const int tile = firstTile + tt;
      const int64_t tq = static_cast<int64_t>(tile) * (kBlock * kPQ);
      keep[tt] = 0;
#pragma unroll
      for (int q = 0; q < kPQ; q++) {
        const int64_t i0 = (tq + threadIdx.x + static_cast<int64_t>(q) * kBlock) * 4 - pad;
        uint32_t pb = 0;
        if (tile < numTiles && i0 >= 0 && i0 + 3 < n) {
          pb = *reinterpret_cast<const uint32_t *>(pred + i0);
          if (VIRTUAL) {
#pragma unroll
            for (int j = 0; j < 4; j++) rows[tt][q][j] = static_cast<PAYLOAD>(iotaStart + static_cast<uint32_t>(i0) + j);
          } else if (sizeof(PAYLOAD) == 4) {
            const U32x4 r = *reinterpret_cast<const U32x4 *>(data + i0);
#pragma unroll
            for (int j = 0; j < 4; j++) rows[tt][q][j] = static_cast<PAYLOAD>(r.v[j]);
          } else {
#pragma unroll
            for (int j = 0; j < 4; j++) rows[tt][q][j] = data[i0 + j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int64_t i = i0 + j;
            rows[tt][q][j] = 0;
            if (tile < numTiles && i >= 0 && i < n) {
              pb |= static_cast<uint32_t>(pred[i]) << (8 * j);
              rows[tt][q][j] = VIRTUAL ? static_cast<PAYLOAD>(iotaStart + static_cast<uint32_t>(i)) : data[i];
            }
          }
        }
        const uint32_t kb = ((pb & 0xFFu) ? 1u : 0u) | ((pb & 0xFF00u) ? 2u : 0u) | ((pb & 0xFF0000u) ? 4u : 0u) |
                            ((pb & 0xFF000000u) ? 8u : 0u);
        keep[tt] |= kb << (4 * q);
      }
    }
    if (!VIRTUAL) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (threadIdx.x < kTilesPerTicket && firstTile + static_cast<int>(threadIdx.x) < numTiles)
        __hip_atomic_store(ws.loaded + firstTile + threadIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // phase B: rank, stage in final order, wait for the input tiles under the output range, write
#pragma unroll
    for (int tt = 0; tt < kTilesPerTicket; tt++) {
      const int tile = firstTile + tt;
      if (tile >= numTiles) break;
      uint32_t lanePrefix[kPQ];
#pragma unroll
      for (int q = 0; q < kPQ; q++) {
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint64_t m = __ballot((keep[tt] >> (4 * q + j)) & 1u);
          before += __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
          total += static_cast<uint32_t>(__popcll(m));
        }
        lanePrefix[q] = before;
        if (lane == 0) sCounts[q * kWaves + wave] = total;
      }
      __syncthreads();
      uint32_t base[kPQ];
      {
        uint32_t run = 0;  // every lane scans the 16 partial counts (position order: quad, wave)
#pragma unroll
        for (int q = 0; q < kPQ; q++)
#pragma unroll
          for (int w = 0; w < kWaves; w++) {
            if (w == wave) base[q] = run;
            run += sCounts[q * kWaves + w];
          }
      }
#pragma unroll
      for (int q = 0; q < kPQ; q++) {
        uint32_t at = base[q] + lanePrefix[q];
        const uint32_t kb = (keep[tt] >> (4 * q)) & 0xFu;
#pragma unroll
        for (int j = 0; j < 4; j++)
          if ((kb >> j) & 1u) sOut[at++] = rows[tt][q][j];
      }
      const uint32_t gbase = ws.tileOffsets[tile], count = ws.tileOffsets[tile + 1] - gbase;
      if (!VIRTUAL && count > 0) {
        const int lo = static_cast<int>((static_cast<int64_t>(gbase) + pad) / kPTile);
        const int hi = static_cast<int>((static_cast<int64_t>(gbase) + count - 1 + pad) / kPTile);
        if (threadIdx.x == 0) {
          for (int s2 = lo; s2 <= hi && s2 < firstTile; s2++) {  // this ticket's own tiles are loaded
            uint32_t spins = 0;
            while (__hip_atomic_load(ws.loaded + s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
              __builtin_amdgcn_s_sleep(2);
              if (++spins > kMaxSpins) {
                atomicOr(ws.error, 1u);
                break;
              }
            }
          }
        }
      }
      __syncthreads();
      for (uint32_t k = threadIdx.x; k < count; k += kBlock) data[gbase + k] = sOut[k];
      __syncthreads();  // sOut / sCounts are reused by the next tile
    }
  }
}

// ---------------------------------------------------------------------------------------------
// lazy fills: a buffer defined as a repeated 4- / 8-byte pattern is written after all
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void fill_pattern_kernel(uint8_t *dst, size_t units, uint64_t pattern, int unit) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < units; i += static_cast<size_t>(gridDim.x) * kBlock) {
    if (unit == 8) reinterpret_cast<uint64_t *>(dst)[i] = pattern;
    else reinterpret_cast<uint32_t *>(dst)[i] = static_cast<uint32_t>(pattern);
  }
}

// ---------------------------------------------------------------------------------------------
// compaction by an existing predicate vector (geo intersection)
// ---------------------------------------------------------------------------------------------
// tile counts of an existing predicate vector, in filter_pred_kernel's tile geometry
__global__ __launch_bounds__(kBlock) void pred_count_kernel(const uint8_t *pred, uint32_t *tileCounts, int pad, int n,
                                                            int numTiles) {
  const int lane = threadIdx.x & 63;
  for (int tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
    const int64_t tq = static_cast<int64_t>(tile) * (kBlock * kPQ);
    uint32_t count = 0;
#pragma unroll
    for (int q = 0; q < kPQ; q++) {
      const int64_t i0 = (tq + threadIdx.x + static_cast<int64_t>(q) * kBlock) * 4 - pad;
      if (i0 >= 0 && i0 + 3 < n) {
        const uint32_t pb = *reinterpret_cast<const uint32_t *>(pred + i0);
        count += ((pb & 0xFFu) ? 1u : 0u) + ((pb & 0xFF00u) ? 1u : 0u) + ((pb & 0xFF0000u) ? 1u : 0u) +
                 ((pb & 0xFF000000u) ? 1u : 0u);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (i0 + j >= 0 && i0 + j < n && pred[i0 + j]) count++;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
    if (lane == 0 && count) atomicAdd(tileCounts + tile, count);
  }
}

}  // namespace ares
