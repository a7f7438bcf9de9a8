// The geofence verdict of a batch resolved once, in row space (AresGeoShapeColumnRun, include/ares_extensions.h): row r of the
// batch receives the first shape its point lies in as ONE byte of an ordinary mode-2 Uint8 main-table column.  The byte's
// validity is the geo filter (the rows GeoBatchIntersects keeps), its value the geo dimension (what WriteGeoShapeDim writes).
// The host then runs the batch as a geo-free query over its columns plus this one, on every fast path such a query has.
//
// In row space the kernel sees the batch BEFORE the filters, and the polygon walk costs thousands of instructions per point.
// So a workgroup classifies a tile of 1024 rows first (pruning hints — the query's own main-table filters —, null points),
// compacts the live rows into an LDS list with one ballot and one LDS add per wavefront and round, and walks the polygon edges
// densely over that list (geo_walk.hpp, the walk of geo_intersect_kernel): a wavefront-chunk of the walk holds 64 live points
// except for the list's last one, and the four wavefronts share each chunk's polygon edges.  Predicate words never reach memory.
#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <mutex>

#include "ares_extensions.h"
#include "binding.hpp"
#include "common.hpp"
#include "device_model.hpp"
#include "fast_eval.hpp"
#include "geo_walk.hpp"
#include "row_hints.hpp"
#include "select_scan.hpp"

namespace ares {

namespace {

constexpr int kGeoColBlock = 256;
constexpr int kGeoColWaves = kGeoColBlock / 64;
constexpr int kGeoColRounds = 4;
constexpr int kGeoColTile = kGeoColBlock * kGeoColRounds;  // 1024 rows
constexpr int kGeoColFilters = 4;                          // AresGeoShapeColumn::filters

struct GeoColumnPlanD {
  int numFilters;
  int numPoints, totalWords, inOrOut;
  FastOperands filters[kGeoColFilters];  // the hints that are evaluated
  const uint8_t *pointBase;              // the GeoPoint column: validity bits at the base (mode 2), float2 values
  uint32_t valuesOff, bitOff;            // valuesOff == 0: mode 1, every point is valid
  const float *lats, *longs;
  const uint8_t *shape;
  uint8_t *bitmap;  // validity, bit r = row r; written in 8-byte words
  uint8_t *values;  // one byte per row
  unsigned long long *counters;  // the device's {live rows, wavefront-chunks walked}
};
static_assert(sizeof(GeoColumnPlanD) <= 1024, "the plan is the kernel's argument");

enum { kPruned = 0, kNullPoint = 1, kLive = 2 };

// A lane handles rows tile + k * 256 + tid, k = 0..3: the 64 rows of a wavefront and round start on a multiple of 64, so their
// validity word is one ballot and one 8-byte store by one lane.
template <int W>
__global__ __launch_bounds__(kGeoColBlock) void geo_shape_column_kernel(GeoColumnPlanD p, int n) {
  __shared__ float sLat[kGeoColTile], sLong[kGeoColTile];  // the live list: the points ...
  __shared__ uint16_t sRow[kGeoColTile];                   // ... and their rows in the tile
  __shared__ alignas(16) uint8_t sByte[kGeoColTile];       // by row in the tile: the verdict (int8), then the value byte
  __shared__ uint32_t sAcc[kGeoColWaves - 1][W][64];        // the parities of wavefronts 1..3 for the list chunk in hand
  __shared__ unsigned int sCount;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (a scalar: it strides loops)
  // a null point: "the first edge writes the verdict" (query/iterator.hpp:1372-1381) — if there is one.  Words that start at
  // zero then hold !inOrOut in every word: shape 0 when the filter asks for outside, no shape otherwise.
  const bool firstEdge = p.numPoints >= 2 && p.shape[0] == p.shape[1];
  const int nullVerdict = firstEdge && !p.inOrOut ? 0 : -1;
  const int numTiles = static_cast<int>((static_cast<int64_t>(n) + kGeoColTile - 1) / kGeoColTile);
  unsigned int liveRows = 0, chunks = 0;  // (thread 0's)
  for (int tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
    const int64_t tileStart = static_cast<int64_t>(tile) * kGeoColTile;
    if (tid == 0) sCount = 0;
    __syncthreads();
    // ---- phase A: classify, dense over the tile's rows ----
    int cls[kGeoColRounds];
#pragma unroll
    for (int k = 0; k < kGeoColRounds; k++) {
      const int inTile = k * kGeoColBlock + tid;
      const int64_t row64 = tileStart + inTile;
      const uint32_t row = static_cast<uint32_t>(row64);
      uint32_t alive = row64 < n ? 1u : 0u;
#pragma unroll 1  // (one copy of the comparison; the index is wave-uniform, the operands are scalar loads of the argument)
      for (int f = 0; f < p.numFilters; f++)
        if (alive) alive = hint_keeps(p.filters[f], row);
      float2 pt = make_float2(0.f, 0.f);
      bool ok = false;
      if (alive) {
        pt = reinterpret_cast<const float2 *>(p.pointBase + p.valuesOff)[row];
        ok = p.valuesOff == 0 ? true : get_bit(p.pointBase, row + p.bitOff) != 0;
      }
      cls[k] = !alive ? kPruned : ok ? kLive : kNullPoint;
      const unsigned long long liveMask = __ballot(cls[k] == kLive);
      if (liveMask) {  // (wave-uniform)
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(&sCount, static_cast<unsigned int>(__popcll(liveMask)));
        base = __shfl(base, 0);
        if (cls[k] == kLive) {
          const unsigned int at = base + static_cast<unsigned int>(__popcll(liveMask & ((1ull << lane) - 1ull)));
          sRow[at] = static_cast<uint16_t>(inTile);
          sLat[at] = pt.x;
          sLong[at] = pt.y;
        }
      }
    }
    __syncthreads();
    // ---- phase B: the edge walk, dense over the live list.  Every wavefront walks every list chunk of 64 entries, over a
    // quarter of the polygon's 64-edge chunks (w, w + 4, ...), and the four parities are XORed through LDS: a tile of a
    // filtered batch holds two or three list chunks, which shared out whole would leave one or two of the four wavefronts idle
    const unsigned int count = sCount;  // (block-uniform: so are the trip count and the barriers below)
    for (unsigned int first = 0; first < count; first += 64u) {
      const unsigned int e = first + static_cast<unsigned int>(lane);
      const bool have = e < count;
      const float testLat = have ? sLat[e] : 0.f;
      const float testLong = have ? sLong[e] : __int_as_float(0x7fc00000);  // lanes past the list's end toggle nothing
      uint32_t acc[W];
      geo_walk_edges<W>(p.lats, p.longs, p.shape, p.numPoints, lane, testLat, testLong, acc, wave, kGeoColWaves);
      if (wave > 0) {
#pragma unroll
        for (int w = 0; w < W; w++) sAcc[wave - 1][w][lane] = acc[w];
      }
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int w = 0; w < W; w++)
          for (int o = 0; o < kGeoColWaves - 1; o++) acc[w] ^= sAcc[o][w][lane];
        if (have) sByte[sRow[e]] = static_cast<uint8_t>(first_shape<W>(acc, p.totalWords));
      }
      __syncthreads();  // (sAcc is written again by the next list chunk)
    }
    if (tid == 0) {
      liveRows += count;
      chunks += (count + 63u) / 64u;
    }
    __syncthreads();
    // ---- phase C: (value, valid) of every row; validity by ballot, values packed through LDS ----
#pragma unroll
    for (int k = 0; k < kGeoColRounds; k++) {
      const int inTile = k * kGeoColBlock + tid;
      const int s = cls[k] == kLive ? static_cast<int8_t>(sByte[inTile]) : nullVerdict;
      const bool valid = cls[k] != kPruned && ((s < 0) != (p.inOrOut != 0));  // the rows GeoRemoveFilter keeps
      const unsigned long long word = __ballot(valid);
      const int64_t waveFirst = tileStart + k * kGeoColBlock + wave * 64;
      if (lane == 0 && waveFirst < n) reinterpret_cast<unsigned long long *>(p.bitmap)[waveFirst >> 6] = word;
      sByte[inTile] = valid && p.inOrOut ? static_cast<uint8_t>(s) : static_cast<uint8_t>(0);  // (this lane's own byte)
    }
    __syncthreads();
    {
      const int64_t first = tileStart + 4 * tid;  // (values is 64-byte aligned and tileStart a multiple of 1024)
      if (first + 3 < n) {
        *reinterpret_cast<uint32_t *>(p.values + first) = *reinterpret_cast<const uint32_t *>(&sByte[4 * tid]);
      } else {
        for (int j = 0; j < 4; j++)
          if (first + j < n) p.values[first + j] = sByte[4 * tid + j];
      }
    }
    // (the next round's first write to sByte lies behind two more barriers, its reset of sCount behind phase C's)
  }
  if (tid == 0 && (liveRows | chunks)) {
    atomicAdd(p.counters, static_cast<unsigned long long>(liveRows));
    atomicAdd(p.counters + 1, static_cast<unsigned long long>(chunks));
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
std::atomic<unsigned long long> g_stats[3];  // batches run, batches declined, rows (live rows, chunks: counted on the devices)

std::mutex g_counterMutex;
std::map<int, unsigned long long *> g_counters;  // per device: two words, allocated on first use and kept

unsigned long long *device_counters(int device) {
  std::lock_guard<std::mutex> lock(g_counterMutex);
  auto it = g_counters.find(device);
  if (it != g_counters.end()) return it->second;
  unsigned long long *c = nullptr;
  hip_check(hipMalloc(reinterpret_cast<void **>(&c), 2 * sizeof(*c)), "hipMalloc");
  hip_check(hipMemsetAsync(c, 0, 2 * sizeof(*c), nullptr), "hipMemsetAsync");
  hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");  // (the callers' streams do not wait for the null stream)
  return g_counters[device] = c;
}

bool geo_column_enabled() {
  static EnvSwitch<bool> on("ARES_GEO_COLUMN", [](const char *e) { return !(e && e[0] == '0'); });
  return on.get();
}

int geo_column_grid(int64_t rows) {
  static EnvSwitch<int> forced("ARES_GEO_COLUMN_GRID", [](const char *e) { return e ? atoi(e) : 0; });
  const int f = forced.get();
  const int64_t tiles = (rows + kGeoColTile - 1) / kGeoColTile;
  if (f > 0) return capped_grid(tiles, f);
  return capped_grid(tiles, 256 * 8);  // geo_intersect_kernel's: 8 workgroups per CU
}

int geo_shape_column(int device, const AresGeoShapeColumn &q, int batchRows, VectorPartySlice *outSlice, hipStream_t stream) {
  if (!geo_column_enabled()) throw NotFusable("switched off (ARES_GEO_COLUMN=0)");
  if (batchRows < 0) throw NotFusable("size");
  if (!outSlice) throw std::invalid_argument("null outSlice");
  if (q.points.Type != VectorPartyInput) throw NotFusable("the geo point must be a main-table column");
  const VectorPartySlice &vp = q.points.Vector.VP;
  if (vp.DataType != GeoPoint) throw std::invalid_argument("only geo point column are allowed in geo_intersects");
  if (!vp.BasePtr) throw NotFusable("mode 0 point column");
  if (run_length_layout(vp)) throw NotFusable("run-length point column");
  if (static_cast<int64_t>(vp.Length) < batchRows) throw NotFusable("column shorter than the batch");
  if (!q.out || (reinterpret_cast<uintptr_t>(q.out) & 63u)) throw NotFusable("null or misaligned output");
  const int N = q.shapes.TotalNumPoints, W = q.shapes.TotalWords;
  if (W < 1 || W > 8) throw std::invalid_argument("geo intersection supports up to 256 shapes");
  if (N > 0 && !q.shapes.LatLongs) throw std::invalid_argument("null shape batch");

  GeoColumnPlanD plan;
  memset(&plan, 0, sizeof(plan));
  const int numHints = q.numFilters < 0 ? 0 : q.numFilters > kGeoColFilters ? kGeoColFilters : q.numFilters;
  for (int k = 0; k < numHints; k++)
    if (bind_hint(q.filters[k], batchRows, stream, plan.filters[plan.numFilters])) plan.numFilters++;
  plan.numPoints = N > 0 ? N : 0;
  plan.totalWords = W;
  plan.inOrOut = q.inOrOut ? 1 : 0;
  plan.pointBase = vp.BasePtr;
  plan.valuesOff = vp.ValuesOffset;
  plan.bitOff = vp.StartingIndex;
  plan.lats = reinterpret_cast<const float *>(q.shapes.LatLongs);
  plan.longs = plan.lats + plan.numPoints;
  plan.shape = q.shapes.LatLongs + static_cast<size_t>(plan.numPoints) * 8;
  const size_t bitmapBytes = bitmap_bytes(batchRows);
  plan.bitmap = q.out;
  plan.values = q.out + bitmapBytes;
  plan.counters = device_counters(device);

  memset(outSlice, 0, sizeof(*outSlice));
  outSlice->BasePtr = q.out;
  outSlice->NullsOffset = 0;
  outSlice->ValuesOffset = static_cast<uint32_t>(bitmapBytes);
  outSlice->StartingIndex = 0;
  outSlice->Length = static_cast<uint32_t>(batchRows);
  outSlice->DataType = Uint8;
  if (batchRows > 0) {
    mem_note_write(device, plan.bitmap, 8 * ((static_cast<size_t>(batchRows) + 63) / 64));
    mem_note_write(device, plan.values, static_cast<size_t>(batchRows));
    const int grid = geo_column_grid(batchRows);
    if (W <= 1)
      ARES_LAUNCH("geo_shape_column_kernel<1>", geo_shape_column_kernel<1>, grid, kGeoColBlock, stream, plan, batchRows);
    else if (W <= 2)
      ARES_LAUNCH("geo_shape_column_kernel<2>", geo_shape_column_kernel<2>, grid, kGeoColBlock, stream, plan, batchRows);
    else if (W <= 4)
      ARES_LAUNCH("geo_shape_column_kernel<4>", geo_shape_column_kernel<4>, grid, kGeoColBlock, stream, plan, batchRows);
    else
      ARES_LAUNCH("geo_shape_column_kernel<8>", geo_shape_column_kernel<8>, grid, kGeoColBlock, stream, plan, batchRows);
  }
  g_stats[0]++;
  g_stats[2] += static_cast<unsigned long long>(batchRows);
  return batchRows;
}

}  // namespace

}  // namespace ares

extern "C" size_t AresGeoShapeColumnBytes(int rows) {
  if (rows < 0) return 0;
  return ares::bitmap_bytes(rows) + ares::padded64(static_cast<size_t>(rows));
}

extern "C" CGoCallResHandle AresGeoShapeColumnRun(const AresGeoShapeColumn *q, int batchRows, VectorPartySlice *outSlice, void *cudaStream,
                                                  int device) {
  ARES_ABI_BEGIN(device)
  if (!q) throw std::invalid_argument("null query");
  try {
    resHandle.res = ares::int_result(ares::geo_shape_column(device, *q, batchRows, outSlice, reinterpret_cast<hipStream_t>(cudaStream)));
  } catch (const ares::NotFusable &) {
    ares::g_stats[1]++;
    throw;
  }
  ARES_ABI_END("AresGeoShapeColumnRun")
}

extern "C" void AresGeoShapeColumnStats(unsigned long long *counters) {
  if (!counters) return;
  for (int i = 0; i < 3; i++) counters[i] = ares::g_stats[i].load();
  counters[3] = counters[4] = 0;
  int before = 0;
  if (hipGetDevice(&before) != hipSuccess) (void)hipGetLastError();
  std::lock_guard<std::mutex> lock(ares::g_counterMutex);
  for (const auto &dc : ares::g_counters) {
    unsigned long long v[2] = {0, 0};
    if (hipSetDevice(dc.first) == hipSuccess && hipMemcpy(v, dc.second, sizeof(v), hipMemcpyDeviceToHost) == hipSuccess) {
      counters[3] += v[0];
      counters[4] += v[1];
    } else {
      (void)hipGetLastError();
    }
  }
  if (hipSetDevice(before) != hipSuccess) (void)hipGetLastError();
}
