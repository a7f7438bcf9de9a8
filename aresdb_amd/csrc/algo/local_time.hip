// Local time resolved once per batch, in row space (AresLocalTimeColumnRun, include/ares_extensions.h): row r of the batch
// receives time[r] + the UTC offset of the zone its join key leads to — what HashLookup and BinaryTransform(Plus, time, the zone
// column read through its TimezoneLookup) leave for it — as an ordinary mode-2 main-table column.  The host then buckets that
// column with Floor, the "one column (op constant)" shape of every fast path.
//
// Two flavours.  probe: join_columns_kernel's geometry, one row and one cuckoo probe per lane, pruning hints evaluated first.
// direct, for key columns of 1- or 2-byte types: a time-zone join is on a key with at most 65 536 values, so a first kernel
// probes every stored key value once and leaves (offset, valid) in a table of 4 bytes per value — at most 256 KiB, resident in
// an XCD's L2 — and a second kernel streams the rows through it: 16 bytes of time and 4 or 8 of keys in per lane, four gathers,
// 16 bytes out; a wavefront's 256 rows are four validity words put together from four ballots.  The probe is cuckoo_probe
// (cuckoo_probe.hpp) and the gather load_foreign32 (device_model.hpp), both unchanged, in either flavour.
#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <mutex>

#include "ares_extensions.h"
#include "binding.hpp"
#include "common.hpp"
#include "cuckoo_probe.hpp"
#include "device_model.hpp"
#include "fast_eval.hpp"
#include "narrow_key.hpp"
#include "row_hints.hpp"
#include "select_scan.hpp"

namespace ares {

namespace {

constexpr int kLtBlock = 256;
constexpr int kLtFilters = 4;                          // AresLocalTimeColumn::filters
constexpr int kLtChunk = 256;                          // direct: rows of one wavefront and round, four per lane
constexpr int kLtTile = kLtChunk * (kLtBlock / 64);    // direct: rows of one workgroup and round
constexpr uint32_t kNullEntry = 0x80000000u;           // direct: a table entry without a valid offset (no int16 widens to it)

struct LocalTimePlanD {
  int numFilters;
  int keySpace;                         // direct: 256 or 65 536 stored key values
  FastOperands filters[kLtFilters];     // probe: the hints that are evaluated
  const uint32_t *timeValues;           // the time column: a 4-byte type in mode 1 or 2
  const uint8_t *timeNulls;             // null: mode 1, every row valid; bit r + timeBitOff otherwise
  uint32_t timeBitOff;
  OperandD key;
  OperandD zone;                        // OP_FOREIGN without record ids, with the offset table
  CuckooD index;
  uint8_t *bitmap;                      // validity, bit r = row r; written in 8-byte words
  uint32_t *values;
  uint32_t *table;                      // direct: entry of stored key value v at [v]
  unsigned long long *probed;           // probe: the device's counter of keys probed
};
static_assert(sizeof(LocalTimePlanD) <= 1024, "the plan is the kernel's argument");

// what the row kernel of the direct flavour reads
struct LocalTimeRowsD {
  const uint8_t *timeValues, *timeNulls;  // nulls null: mode 1, every row valid; bit r + bitOff otherwise
  const uint8_t *keyValues, *keyNulls;
  uint32_t timeBitOff, keyBitOff;
  int keyStep;                            // 1 or 2 bytes per stored key
  const uint32_t *table;
  uint8_t *bitmap;
  uint32_t *values;
};

// ---- probe ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLtBlock) void local_time_probe_kernel(LocalTimePlanD p, int n) {
  __shared__ unsigned int sProbed;
  if (threadIdx.x == 0) sProbed = 0;
  __syncthreads();
  const FastDivisor bucketDiv = make_fast_divisor(p.index.numBuckets);
  // whole wavefronts: the lanes past n of the last one take part in its ballot and store nothing else
  const int64_t rounded = (static_cast<int64_t>(n) + 63) / 64 * 64;
  uint32_t probedByWave = 0;
  for (int64_t i64 = static_cast<int64_t>(blockIdx.x) * kLtBlock + threadIdx.x; i64 < rounded;
       i64 += static_cast<int64_t>(gridDim.x) * kLtBlock) {
    const uint32_t i = static_cast<uint32_t>(i64);
    const bool inside = i64 < n;
    uint32_t alive = inside ? 1u : 0u;
#pragma unroll 1  // (one copy of the comparison; the index is wave-uniform, the operands are scalar loads of the argument)
    for (int k = 0; k < p.numFilters; k++)
      if (alive) alive = hint_keeps(p.filters[k], i);
    uint32_t key[4] = {0, 0, 0, 0};
    uint32_t ok = 0;
    if (alive) ok = cuckoo_load_key(p.key, i, i, nullptr, 0, key);
    RecordID rid = {0, 0};
    if (ok) rid = cuckoo_probe(p.index, bucketDiv, key);
    probedByWave += static_cast<uint32_t>(__popcll(__ballot(ok != 0)));
    DVal z, t;
    z.bits = t.bits = 0;
    z.ok = t.ok = 0;
    if (ok) z = load_foreign32(p.zone, rid);
    if (z.ok) {  // (what load32 reads for such a column)
      t.bits = p.timeValues[i];
      t.ok = p.timeNulls ? get_bit(p.timeNulls, i + p.timeBitOff) : 1u;
    }
    const bool valid = z.ok != 0 && t.ok != 0;
    const unsigned long long word = __ballot(valid);
    if ((threadIdx.x & 63) == 0) reinterpret_cast<unsigned long long *>(p.bitmap)[i >> 6] = word;
    if (inside) p.values[i] = valid ? t.bits + z.bits : 0u;
  }
  if ((threadIdx.x & 63) == 0 && probedByWave) atomicAdd(&sProbed, probedByWave);
  __syncthreads();
  if (threadIdx.x == 0 && sProbed) atomicAdd(p.probed, static_cast<unsigned long long>(sProbed));
}

// ---- direct ---------------------------------------------------------------------------------------------------------
// Entry of every stored key value: the value widened as cuckoo_load_key widens a row's (the column's kind decides sign
// extension; cuckoo_probe keeps keyBytes of it), probed once.
__global__ __launch_bounds__(kLtBlock) void local_time_table_kernel(LocalTimePlanD p) {
  const uint32_t v = blockIdx.x * kLtBlock + threadIdx.x;
  if (v >= static_cast<uint32_t>(p.keySpace)) return;
  const FastDivisor bucketDiv = make_fast_divisor(p.index.numBuckets);
  uint32_t key[4] = {widen_stored_key(p.key.kind, p.key.step, v), 0, 0, 0};
  const RecordID rid = cuckoo_probe(p.index, bucketDiv, key);
  const DVal z = load_foreign32(p.zone, rid);
  p.table[v] = z.ok ? z.bits : kNullEntry;
}

__device__ __forceinline__ uint32_t stored_key(const LocalTimeRowsD &p, uint32_t row) {
  return p.keyStep == 2 ? reinterpret_cast<const uint16_t *>(p.keyValues)[row] : p.keyValues[row];
}

// A wavefront takes 256 rows that start on a multiple of 256.  A whole chunk: lane l holds rows 4 l .. 4 l + 3, so validity word
// w of the chunk is the bits of lanes 16 w .. 16 w + 15, interleaved from the four ballots by lanes 0 .. 3.  The batch's last,
// partial chunk goes 64 rows at a time, one per lane, a word per ballot as the probe flavour writes it.
__global__ __launch_bounds__(kLtBlock) void local_time_rows_kernel(LocalTimeRowsD p, int n) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t numTiles = (static_cast<int64_t>(n) + kLtTile - 1) / kLtTile;
  unsigned long long *words = reinterpret_cast<unsigned long long *>(p.bitmap);
  for (int64_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
    const int64_t first = tile * kLtTile + static_cast<int64_t>(wave) * kLtChunk;
    if (first >= n) continue;
    if (first + kLtChunk <= n) {
      const uint32_t row = static_cast<uint32_t>(first) + 4u * static_cast<uint32_t>(lane);
      const Words4 t = *reinterpret_cast<const Words4 *>(p.timeValues + 4 * static_cast<size_t>(row));
      uint32_t k[4];
      if (p.keyStep == 2) {
        const Halves4 h = *reinterpret_cast<const Halves4 *>(p.keyValues + 2 * static_cast<size_t>(row));
#pragma unroll
        for (int j = 0; j < 4; j++) k[j] = h.v[j];
      } else {
        const uint32_t b = reinterpret_cast<const KeyWord *>(p.keyValues + row)->v;
#pragma unroll
        for (int j = 0; j < 4; j++) k[j] = (b >> (8 * j)) & 0xffu;
      }
      uint32_t ok = 15u;
      if (p.timeNulls) ok &= four_bits(p.timeNulls, row + p.timeBitOff);
      if (p.keyNulls) ok &= four_bits(p.keyNulls, row + p.keyBitOff);
      uint32_t e[4];
#pragma unroll
      for (int j = 0; j < 4; j++) e[j] = p.table[k[j]];
      uint4 out;
      unsigned long long mask[4];
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool valid = ((ok >> j) & 1u) != 0 && e[j] != kNullEntry;
        o[j] = valid ? t.v[j] + e[j] : 0u;
        mask[j] = __ballot(valid);
      }
      out.x = o[0]; out.y = o[1]; out.z = o[2]; out.w = o[3];
      *reinterpret_cast<uint4 *>(p.values + row) = out;  // (values is 64-byte aligned and row a multiple of 4)
      if (lane < 4) {
        unsigned long long word = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) word |= spread4((mask[j] >> (16 * lane)) & 0xffffull) << j;
        words[(first >> 6) + lane] = word;
      }
    } else {
      for (int r = 0; r < kLtChunk / 64; r++) {
        const int64_t waveFirst = first + 64 * r;
        if (waveFirst >= n) break;
        const int64_t row64 = waveFirst + lane;
        const uint32_t row = static_cast<uint32_t>(row64);
        bool valid = false;
        uint32_t value = 0;
        if (row64 < n) {
          const uint32_t entry = p.table[stored_key(p, row)];
          valid = entry != kNullEntry && (!p.timeNulls || get_bit(p.timeNulls, row + p.timeBitOff)) &&
                  (!p.keyNulls || get_bit(p.keyNulls, row + p.keyBitOff));
          if (valid) value = reinterpret_cast<const uint32_t *>(p.timeValues)[row] + entry;
        }
        const unsigned long long word = __ballot(valid);
        if (lane == 0) words[waveFirst >> 6] = word;
        if (row64 < n) p.values[row] = value;
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
std::atomic<unsigned long long> g_stats[5];  // batches run, declined, rows, keys probed by direct batches, direct batches

std::mutex g_counterMutex;
std::map<int, unsigned long long *> g_counters;  // per device: keys probed by probe batches, allocated on first use and kept

unsigned long long *probe_counter(int device) {
  std::lock_guard<std::mutex> lock(g_counterMutex);
  auto it = g_counters.find(device);
  if (it != g_counters.end()) return it->second;
  unsigned long long *c = nullptr;
  hip_check(hipMalloc(reinterpret_cast<void **>(&c), sizeof(*c)), "hipMalloc");
  hip_check(hipMemsetAsync(c, 0, sizeof(*c), nullptr), "hipMemsetAsync");
  hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");  // (the callers' streams do not wait for the null stream)
  return g_counters[device] = c;
}

enum { kFlavourOff = 0, kFlavourAuto = 1, kFlavourProbe = 2, kFlavourDirect = 3 };

int local_time_flavour() {
  static EnvSwitch<int> flavour("ARES_LOCAL_TIME", [](const char *e) {
    if (!e) return static_cast<int>(kFlavourAuto);
    if (e[0] == '0') return static_cast<int>(kFlavourOff);
    if (!strcmp(e, "probe")) return static_cast<int>(kFlavourProbe);
    if (!strcmp(e, "direct")) return static_cast<int>(kFlavourDirect);
    return static_cast<int>(kFlavourAuto);
  });
  return flavour.get();
}

int local_time_grid(int64_t units) {
  static EnvSwitch<int> forced("ARES_LOCAL_TIME_GRID", [](const char *e) { return e ? atoi(e) : 0; });
  const int f = forced.get();
  if (f > 0) return capped_grid(units, f);
  return capped_grid(units, 256 * 16);  // hash_lookup_kernel's
}

// a main-table column the kernels read row by row
void check_row_column(const InputVector &in, const char *what, int batchRows) {
  if (in.Type != VectorPartyInput) throw NotFusable(std::string(what) + " must be a main-table column");
  const VectorPartySlice &vp = in.Vector.VP;
  if (!vp.BasePtr) throw NotFusable(std::string("mode 0 ") + what);
  if (run_length_layout(vp)) throw NotFusable(std::string("run-length ") + what);
  if (static_cast<int64_t>(vp.Length) < batchRows) throw NotFusable("column shorter than the batch");
}

int local_time_column(int device, const AresLocalTimeColumn &q, int batchRows, VectorPartySlice *outSlice, hipStream_t stream) {
  const int flavour = local_time_flavour();
  if (flavour == kFlavourOff) throw NotFusable("switched off (ARES_LOCAL_TIME=0)");
  if (batchRows < 0) throw NotFusable("size");
  if (!outSlice) throw std::invalid_argument("null outSlice");
  if (q.zone.Type != ForeignColumnInput) throw NotFusable("the zone must be a ForeignColumnInput");
  const ForeignColumnVector &zone = q.zone.Vector.ForeignVP;
  if (!zone.TimezoneLookup) throw NotFusable("no timezone lookup");
  if (zone.DataType != Uint8 && zone.DataType != Uint16) throw NotFusable("the zone must be a Uint8 or Uint16 column");
  if (zone.NumBatches < 0 || (zone.NumBatches > 0 && !zone.Batches)) throw NotFusable("zone column without batches");
  check_row_column(q.time, "time column", batchRows);
  const int timeType = q.time.Vector.VP.DataType;
  if (timeType != Uint32 && timeType != Int32) throw NotFusable("the time must be a Uint32 or Int32 column");
  if (q.outType != Uint32 && q.outType != Int32) throw NotFusable("local time is a Uint32 or Int32 column");
  if (!q.out || (reinterpret_cast<uintptr_t>(q.out) & 63u)) throw NotFusable("null or misaligned output");

  CallTemps temps;  // (the zone's batch descriptors and the direct flavour's table: released in stream order behind the launches)
  LocalTimePlanD plan;
  memset(&plan, 0, sizeof(plan));
  const SelectJoinD join = bind_join(q.join, batchRows, stream, temps);
  plan.key = join.key;
  plan.index = join.index;
  OperandD time;
  try {
    bind_operand(q.time, true, stream, time, temps);
    bind_operand(q.zone, true, stream, plan.zone, temps);
  } catch (const std::invalid_argument &bad) {
    throw NotFusable(bad.what());
  }
  plan.zone.rids = nullptr;
  plan.timeValues = reinterpret_cast<const uint32_t *>(time.base + time.valuesOff);
  plan.timeNulls = time.mode >= 2 ? time.base + time.nullsOff : nullptr;
  plan.timeBitOff = time.bitOff;
  const size_t bitmapBytes = bitmap_bytes(batchRows);
  plan.bitmap = q.out;
  plan.values = reinterpret_cast<uint32_t *>(q.out + bitmapBytes);

  const int keyType = q.join.key.Vector.VP.DataType;
  const bool narrow = keyType == Int8 || keyType == Uint8 || keyType == Int16 || keyType == Uint16;
  const int keySpace = plan.key.step == 1 ? 256 : 65536;
  bool direct = narrow && (flavour == kFlavourDirect || (flavour == kFlavourAuto && batchRows >= keySpace));
  if (plan.zone.cok && plan.zone.cbits == kNullEntry) direct = false;  // (a default no Uint8 / Uint16 holds: the table cannot say it)
  if (!direct) {
    const int numHints = q.numFilters < 0 ? 0 : q.numFilters > kLtFilters ? kLtFilters : q.numFilters;
    for (int k = 0; k < numHints; k++)
      if (bind_hint(q.filters[k], batchRows, stream, plan.filters[plan.numFilters])) plan.numFilters++;
    plan.probed = probe_counter(device);
  }

  memset(outSlice, 0, sizeof(*outSlice));
  outSlice->BasePtr = q.out;
  outSlice->NullsOffset = 0;
  outSlice->ValuesOffset = static_cast<uint32_t>(bitmapBytes);
  outSlice->StartingIndex = 0;
  outSlice->Length = static_cast<uint32_t>(batchRows);
  outSlice->DataType = q.outType;
  if (batchRows > 0) {
    mem_note_write(device, plan.bitmap, 8 * ((static_cast<size_t>(batchRows) + 63) / 64));
    mem_note_write(device, plan.values, 4 * static_cast<size_t>(batchRows));
    if (direct) {
      plan.keySpace = keySpace;
      temps.buffers.emplace_back(new StreamBuffer(sizeof(uint32_t) * static_cast<size_t>(keySpace), stream));
      plan.table = temps.buffers.back()->as<uint32_t>();
      ARES_LAUNCH("local_time_table_kernel", local_time_table_kernel, keySpace / kLtBlock, kLtBlock, stream, plan);
      LocalTimeRowsD rows;
      memset(&rows, 0, sizeof(rows));
      rows.timeValues = reinterpret_cast<const uint8_t *>(plan.timeValues);
      rows.timeNulls = plan.timeNulls;
      rows.timeBitOff = plan.timeBitOff;
      rows.keyValues = plan.key.base + plan.key.valuesOff;
      rows.keyNulls = plan.key.mode >= 2 ? plan.key.base + plan.key.nullsOff : nullptr;
      rows.keyBitOff = plan.key.bitOff;
      rows.keyStep = plan.key.step;
      rows.table = plan.table;
      rows.bitmap = plan.bitmap;
      rows.values = plan.values;
      const int grid = local_time_grid((static_cast<int64_t>(batchRows) + kLtTile - 1) / kLtTile);
      ARES_LAUNCH("local_time_rows_kernel", local_time_rows_kernel, grid, kLtBlock, stream, rows, batchRows);
      g_stats[3] += static_cast<unsigned long long>(keySpace);
      g_stats[4]++;
    } else {
      const int grid = local_time_grid((static_cast<int64_t>(batchRows) + kLtBlock - 1) / kLtBlock);
      ARES_LAUNCH("local_time_probe_kernel", local_time_probe_kernel, grid, kLtBlock, stream, plan, batchRows);
    }
  }
  g_stats[0]++;
  g_stats[2] += static_cast<unsigned long long>(batchRows);
  return batchRows;
}

}  // namespace

}  // namespace ares

extern "C" CGoCallResHandle AresLocalTimeColumnRun(const AresLocalTimeColumn *q, int batchRows, VectorPartySlice *outSlice,
                                                   void *cudaStream, int device) {
  ARES_ABI_BEGIN(device)
  if (!q) throw std::invalid_argument("null query");
  try {
    resHandle.res = ares::int_result(ares::local_time_column(device, *q, batchRows, outSlice, reinterpret_cast<hipStream_t>(cudaStream)));
  } catch (const ares::NotFusable &) {
    ares::g_stats[1]++;
    throw;
  }
  ARES_ABI_END("AresLocalTimeColumnRun")
}

extern "C" void AresLocalTimeColumnStats(unsigned long long *counters) {
  if (!counters) return;
  for (int i = 0; i < 5; i++) counters[i] = ares::g_stats[i].load();
  int before = 0;
  if (hipGetDevice(&before) != hipSuccess) (void)hipGetLastError();
  std::lock_guard<std::mutex> lock(ares::g_counterMutex);
  for (const auto &dc : ares::g_counters) {
    unsigned long long v = 0;
    if (hipSetDevice(dc.first) == hipSuccess && hipMemcpy(&v, dc.second, sizeof(v), hipMemcpyDeviceToHost) == hipSuccess) counters[3] += v;
    else (void)hipGetLastError();
  }
  if (hipSetDevice(before) != hipSuccess) (void)hipGetLastError();
}
