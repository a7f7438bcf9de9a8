// Joined columns resolved once per batch, in row space (AresJoinColumnsRun, include/ares_extensions.h): the key column of a
// batch is resolved through the cuckoo index and up to four joined columns are gathered into ordinary mode-2 main-table columns
// (validity bitmap + values) of the batch's length.  The host then runs the batch as a join-free query over its columns plus
// these, on every fast path a join-free query has.
//
// Two flavours; the probe is cuckoo_probe (cuckoo_probe.hpp) and the gather load_foreign32 (device_model.hpp), both unchanged, in
// either: row r holds what the per-node sequence (HashLookup, then a foreign operand over the record ids) reads for it.
// probe: HashLookup's geometry, one row and one probe per lane, nothing else held in registers.  A wavefront's 64 rows start on
// a multiple of 64, so a column's validity word is one ballot and one 8-byte store by one lane, and the values of a wavefront are
// one contiguous range.  Rows that fail a pruning hint (the query's own main-table filters, compared with compare_fast as the
// row-space filters do) skip the probe and are written as (0, null).
// direct, for key columns of 1- or 2-byte types: a first kernel probes every stored key value once and leaves, per joined column,
// an array of 4-byte values indexed by the stored key, and one byte of validity bits per key value (bit c: column c) — at most
// 65 536 x (4 x 4 + 1) bytes, resident in an XCD's L2 — and a second kernel streams the rows through it, four rows per lane: 4 or
// 8 bytes of keys in, four gathers and one store of 4, 8 or 16 bytes per column; a wavefront's 256 rows are four validity words
// put together from four ballots.  Hints are not evaluated.
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

constexpr int kJoinBlock = 256;
constexpr int kJoinFilters = 4;  // AresJoinColumns::filters
constexpr int kJoinColumns = 4;  // AresJoinColumns::columns
constexpr int kJoinChunk = 256;                          // direct: rows of one wavefront and round, four per lane
constexpr int kJoinTile = kJoinChunk * (kJoinBlock / 64);  // direct: rows of one workgroup and round
constexpr int kDirectRowsPerKey = 64;                    // auto: direct from this many rows per stored key value (profiles/r21)

struct JoinColumnD {
  OperandD col;     // OP_FOREIGN without record ids
  uint8_t *bitmap;  // validity, bit r = row r; written in 8-byte words
  uint8_t *values;  // `width` bytes per row
  int width, pad;
};

struct JoinColumnsPlanD {
  int numFilters, numColumns;
  FastOperands filters[kJoinFilters];  // the hints that are evaluated
  OperandD key;
  CuckooD index;
  JoinColumnD columns[kJoinColumns];
  unsigned long long *probed;  // probe: the device's counter of keys probed
  int keySpace;                // direct: 256 or 65 536 stored key values
  uint32_t *table;             // direct: value bits of column c for stored key value v at [c * keySpace + v]
  uint8_t *tableValid;         // direct: bit c of [v] = column c's validity for stored key value v
};
static_assert(sizeof(JoinColumnsPlanD) <= 2048, "the plan is the kernel's argument");

// what the row kernel of the direct flavour reads and writes
struct JoinRowsColumnD {
  uint8_t *bitmap, *values;
  int width, pad;
};

struct JoinRowsD {
  const uint8_t *keyValues, *keyNulls;  // nulls null: mode 1, every row valid; bit r + keyBitOff otherwise
  uint32_t keyBitOff;
  int keyStep;                          // 1 or 2 bytes per stored key
  int keySpace, numColumns;
  const uint32_t *table;
  const uint8_t *tableValid;
  JoinRowsColumnD columns[kJoinColumns];
};

// ---- probe ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kJoinBlock) void join_columns_kernel(JoinColumnsPlanD p, int n) {
  __shared__ unsigned int sProbed;
  if (threadIdx.x == 0) sProbed = 0;
  __syncthreads();
  const FastDivisor bucketDiv = make_fast_divisor(p.index.numBuckets);
  // whole wavefronts: the lanes past n of the last one take part in its ballots and store nothing else
  const int64_t rounded = (static_cast<int64_t>(n) + 63) / 64 * 64;
  uint32_t probedByWave = 0;
  for (int64_t i64 = static_cast<int64_t>(blockIdx.x) * kJoinBlock + threadIdx.x; i64 < rounded;
       i64 += static_cast<int64_t>(gridDim.x) * kJoinBlock) {
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
#pragma unroll 1
    for (int c = 0; c < p.numColumns; c++) {
      const JoinColumnD &col = p.columns[c];
      DVal v;
      v.bits = 0;
      v.ok = 0;
      if (ok) v = load_foreign32(col.col, rid);
      const unsigned long long word = __ballot(v.ok != 0);
      if ((threadIdx.x & 63) == 0) reinterpret_cast<unsigned long long *>(col.bitmap)[i >> 6] = word;
      if (inside) {
        if (col.width == 4) reinterpret_cast<uint32_t *>(col.values)[i] = v.bits;
        else if (col.width == 2) reinterpret_cast<uint16_t *>(col.values)[i] = static_cast<uint16_t>(v.bits);
        else col.values[i] = static_cast<uint8_t>(v.bits);
      }
    }
  }
  if ((threadIdx.x & 63) == 0 && probedByWave) atomicAdd(&sProbed, probedByWave);
  __syncthreads();
  if (threadIdx.x == 0 && sProbed) atomicAdd(p.probed, static_cast<unsigned long long>(sProbed));
}

// ---- direct ---------------------------------------------------------------------------------------------------------
// Entries of every stored key value: the value widened as cuckoo_load_key widens a row's, probed once; per joined column what
// load_foreign32 reads for the record.
__global__ __launch_bounds__(kJoinBlock) void join_columns_table_kernel(JoinColumnsPlanD p) {
  const uint32_t v = blockIdx.x * kJoinBlock + threadIdx.x;
  if (v >= static_cast<uint32_t>(p.keySpace)) return;
  const FastDivisor bucketDiv = make_fast_divisor(p.index.numBuckets);
  uint32_t key[4] = {widen_stored_key(p.key.kind, p.key.step, v), 0, 0, 0};
  const RecordID rid = cuckoo_probe(p.index, bucketDiv, key);
  // every column's loads ahead of the first store, so that they are in flight together: with at most one wavefront per SIMD
  // the kernel is a chain of latencies (constant indices keep the entries in registers)
  DVal e[kJoinColumns];
#pragma unroll
  for (int c = 0; c < kJoinColumns; c++) {
    e[c].bits = 0;
    e[c].ok = 0;
    if (c < p.numColumns) e[c] = load_foreign32(p.columns[c].col, rid);
  }
  uint32_t valid = 0;
#pragma unroll
  for (int c = 0; c < kJoinColumns; c++) {
    if (c < p.numColumns) p.table[static_cast<size_t>(c) * p.keySpace + v] = e[c].bits;
    valid |= (e[c].ok ? 1u : 0u) << c;
  }
  p.tableValid[v] = static_cast<uint8_t>(valid);
}

__device__ __forceinline__ uint32_t stored_key(const JoinRowsD &p, uint32_t row) {
  return p.keyStep == 2 ? reinterpret_cast<const uint16_t *>(p.keyValues)[row] : p.keyValues[row];
}

// A wavefront takes 256 rows that start on a multiple of 256.  A whole chunk: lane l holds rows 4 l .. 4 l + 3, so validity word
// w of the chunk is the bits of lanes 16 w .. 16 w + 15, interleaved from the four ballots by lanes 0 .. 3.  The batch's last,
// partial chunk goes 64 rows at a time, one per lane, a word per ballot as the probe flavour writes it.  A row with a valid key
// gets its entry's (value bits, validity), any other (0, null): what the probe flavour writes for a row no hint prunes.
__global__ __launch_bounds__(kJoinBlock) void join_columns_rows_kernel(JoinRowsD p, int n) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t numTiles = (static_cast<int64_t>(n) + kJoinTile - 1) / kJoinTile;
  for (int64_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
    const int64_t first = tile * kJoinTile + static_cast<int64_t>(wave) * kJoinChunk;
    if (first >= n) continue;
    if (first + kJoinChunk <= n) {
      const uint32_t row = static_cast<uint32_t>(first) + 4u * static_cast<uint32_t>(lane);
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
      if (p.keyNulls) ok &= four_bits(p.keyNulls, row + p.keyBitOff);
      uint32_t valid[4];  // bit c: column c of row j is valid; 0 for a null key
#pragma unroll
      for (int j = 0; j < 4; j++) valid[j] = p.tableValid[k[j]];
#pragma unroll
      for (int j = 0; j < 4; j++) valid[j] = ((ok >> j) & 1u) ? valid[j] : 0u;
#pragma unroll 1  // (one copy of the gathers and stores; the column is a scalar load of the argument)
      for (int c = 0; c < p.numColumns; c++) {
        const JoinRowsColumnD &col = p.columns[c];
        const uint32_t *entries = p.table + static_cast<size_t>(c) * p.keySpace;
        uint32_t o[4];
        unsigned long long mask[4];
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = entries[k[j]];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          o[j] = ((ok >> j) & 1u) ? o[j] : 0u;
          mask[j] = __ballot(((valid[j] >> c) & 1u) != 0);
        }
        // (values is 64-byte aligned and row a multiple of 4)
        if (col.width == 4) {
          uint4 out;
          out.x = o[0]; out.y = o[1]; out.z = o[2]; out.w = o[3];
          *reinterpret_cast<uint4 *>(col.values + 4 * static_cast<size_t>(row)) = out;
        } else if (col.width == 2) {
          uint2 out;
          out.x = (o[0] & 0xffffu) | (o[1] << 16);
          out.y = (o[2] & 0xffffu) | (o[3] << 16);
          *reinterpret_cast<uint2 *>(col.values + 2 * static_cast<size_t>(row)) = out;
        } else {
          *reinterpret_cast<uint32_t *>(col.values + row) =
              (o[0] & 0xffu) | ((o[1] & 0xffu) << 8) | ((o[2] & 0xffu) << 16) | (o[3] << 24);
        }
        if (lane < 4) {
          unsigned long long word = 0;
#pragma unroll
          for (int j = 0; j < 4; j++) word |= spread4((mask[j] >> (16 * lane)) & 0xffffull) << j;
          reinterpret_cast<unsigned long long *>(col.bitmap)[(first >> 6) + lane] = word;
        }
      }
    } else {
      for (int r = 0; r < kJoinChunk / 64; r++) {
        const int64_t waveFirst = first + 64 * r;
        if (waveFirst >= n) break;
        const int64_t row64 = waveFirst + lane;
        const uint32_t row = static_cast<uint32_t>(row64);
        const bool inside = row64 < n;
        uint32_t key = 0, valid = 0;
        bool keyOk = false;
        if (inside) {
          key = stored_key(p, row);
          keyOk = !p.keyNulls || get_bit(p.keyNulls, row + p.keyBitOff);
          if (keyOk) valid = p.tableValid[key];
        }
#pragma unroll 1
        for (int c = 0; c < p.numColumns; c++) {
          const JoinRowsColumnD &col = p.columns[c];
          const unsigned long long word = __ballot(((valid >> c) & 1u) != 0);
          if (lane == 0) reinterpret_cast<unsigned long long *>(col.bitmap)[waveFirst >> 6] = word;
          if (inside) {
            const uint32_t bits = keyOk ? p.table[static_cast<size_t>(c) * p.keySpace + key] : 0u;
            if (col.width == 4) reinterpret_cast<uint32_t *>(col.values)[row] = bits;
            else if (col.width == 2) reinterpret_cast<uint16_t *>(col.values)[row] = static_cast<uint16_t>(bits);
            else col.values[row] = static_cast<uint8_t>(bits);
          }
        }
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// batches run, batches declined, rows, table entries built (the keys a direct batch probes), probe batches, direct batches
// (keys probed by probe batches: counted on the devices)
std::atomic<unsigned long long> g_stats[6];

std::mutex g_counterMutex;
std::map<int, unsigned long long *> g_counters;  // per device, allocated on first use and kept

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

int join_columns_flavour() {
  static EnvSwitch<int> flavour("ARES_JOIN_COLUMNS", [](const char *e) {
    if (!e) return static_cast<int>(kFlavourAuto);
    if (e[0] == '0') return static_cast<int>(kFlavourOff);
    if (!strcmp(e, "probe")) return static_cast<int>(kFlavourProbe);
    if (!strcmp(e, "direct")) return static_cast<int>(kFlavourDirect);
    return static_cast<int>(kFlavourAuto);
  });
  return flavour.get();
}

// workgroups for `units` of work: 256-row blocks of the probe flavour, 1024-row tiles of the direct flavour
int join_columns_grid(int64_t units) {
  static EnvSwitch<int> forced("ARES_JOIN_COLUMNS_GRID", [](const char *e) { return e ? atoi(e) : 0; });
  const int f = forced.get();
  if (f > 0) return capped_grid(units, f);
  return capped_grid(units, 256 * 16);  // hash_lookup_kernel's
}

bool joinable_type(int t) { return t == Int8 || t == Uint8 || t == Int16 || t == Uint16 || t == Int32 || t == Uint32 || t == Float32; }

int join_columns(int device, const AresJoinColumns &q, int batchRows, VectorPartySlice *outSlices, hipStream_t stream) {
  const int flavour = join_columns_flavour();
  if (flavour == kFlavourOff) throw NotFusable("switched off (ARES_JOIN_COLUMNS=0)");
  if (q.numColumns < 1 || q.numColumns > kJoinColumns) throw NotFusable("1..4 joined columns");
  if (batchRows < 0) throw NotFusable("size");
  if (!outSlices) throw std::invalid_argument("null outSlices");
  for (int c = 0; c < q.numColumns; c++) {
    const AresJoinedColumn &jc = q.columns[c];
    if (jc.column.Type != ForeignColumnInput) throw NotFusable("a joined column must be a ForeignColumnInput");
    const ForeignColumnVector &f = jc.column.Vector.ForeignVP;
    if (!joinable_type(f.DataType)) throw NotFusable("Bool or wide joined column");
    if (f.TimezoneLookup) throw NotFusable("timezone lookup");
    if (f.NumBatches < 0 || (f.NumBatches > 0 && !f.Batches)) throw NotFusable("joined column without batches");
    if (!jc.out || (reinterpret_cast<uintptr_t>(jc.out) & 63u)) throw NotFusable("null or misaligned output");
  }
  CallTemps temps;  // (the joined columns' batch descriptors and the direct flavour's table: released in stream order behind the launches)
  JoinColumnsPlanD plan;
  memset(&plan, 0, sizeof(plan));
  const SelectJoinD join = bind_join(q.join, batchRows, stream, temps);
  plan.key = join.key;
  plan.index = join.index;
  const int keyType = q.join.key.Vector.VP.DataType;
  const bool narrow = keyType == Int8 || keyType == Uint8 || keyType == Int16 || keyType == Uint16;
  const int keySpace = plan.key.step == 1 ? 256 : 65536;
  const bool direct = narrow && (flavour == kFlavourDirect ||
                                 (flavour == kFlavourAuto && batchRows >= static_cast<int64_t>(kDirectRowsPerKey) * keySpace));
  if (!direct) {
    const int numHints = q.numFilters < 0 ? 0 : q.numFilters > kJoinFilters ? kJoinFilters : q.numFilters;
    for (int k = 0; k < numHints; k++)
      if (bind_hint(q.filters[k], batchRows, stream, plan.filters[plan.numFilters])) plan.numFilters++;
    plan.probed = probe_counter(device);
  }
  plan.numColumns = q.numColumns;
  const size_t bitmapBytes = bitmap_bytes(batchRows);
  for (int c = 0; c < q.numColumns; c++) {
    JoinColumnD &d = plan.columns[c];
    try {
      bind_operand(q.columns[c].column, true, stream, d.col, temps);
    } catch (const std::invalid_argument &bad) {
      throw NotFusable(bad.what());
    }
    d.col.rids = nullptr;
    d.width = d.col.step;
    d.bitmap = q.columns[c].out;
    d.values = q.columns[c].out + bitmapBytes;
  }

  for (int c = 0; c < q.numColumns; c++) {
    const ForeignColumnVector &f = q.columns[c].column.Vector.ForeignVP;
    VectorPartySlice &s = outSlices[c];
    memset(&s, 0, sizeof(s));
    s.BasePtr = q.columns[c].out;
    s.NullsOffset = 0;
    s.ValuesOffset = static_cast<uint32_t>(bitmapBytes);
    s.StartingIndex = 0;
    s.Length = static_cast<uint32_t>(batchRows);
    s.DataType = f.DataType;
    s.DefaultValue = f.DefaultValue;
  }
  if (batchRows > 0) {
    const size_t words = (static_cast<size_t>(batchRows) + 63) / 64;
    for (int c = 0; c < q.numColumns; c++) {
      mem_note_write(device, plan.columns[c].bitmap, 8 * words);
      mem_note_write(device, plan.columns[c].values, static_cast<size_t>(plan.columns[c].width) * static_cast<size_t>(batchRows));
    }
    if (direct) {
      plan.keySpace = keySpace;
      temps.buffers.emplace_back(new StreamBuffer(sizeof(uint32_t) * static_cast<size_t>(keySpace) * q.numColumns, stream));
      plan.table = temps.buffers.back()->as<uint32_t>();
      temps.buffers.emplace_back(new StreamBuffer(static_cast<size_t>(keySpace), stream));
      plan.tableValid = temps.buffers.back()->as<uint8_t>();
      ARES_LAUNCH("join_columns_table_kernel", join_columns_table_kernel, keySpace / kJoinBlock, kJoinBlock, stream, plan);
      JoinRowsD rows;
      memset(&rows, 0, sizeof(rows));
      rows.keyValues = plan.key.base + plan.key.valuesOff;
      rows.keyNulls = plan.key.mode >= 2 ? plan.key.base + plan.key.nullsOff : nullptr;
      rows.keyBitOff = plan.key.bitOff;
      rows.keyStep = plan.key.step;
      rows.keySpace = keySpace;
      rows.numColumns = q.numColumns;
      rows.table = plan.table;
      rows.tableValid = plan.tableValid;
      for (int c = 0; c < q.numColumns; c++) {
        rows.columns[c].bitmap = plan.columns[c].bitmap;
        rows.columns[c].values = plan.columns[c].values;
        rows.columns[c].width = plan.columns[c].width;
      }
      const int grid = join_columns_grid((static_cast<int64_t>(batchRows) + kJoinTile - 1) / kJoinTile);
      ARES_LAUNCH("join_columns_rows_kernel", join_columns_rows_kernel, grid, kJoinBlock, stream, rows, batchRows);
      g_stats[3] += static_cast<unsigned long long>(keySpace);
      g_stats[5]++;
    } else {
      const int grid = join_columns_grid((static_cast<int64_t>(batchRows) + kJoinBlock - 1) / kJoinBlock);
      ARES_LAUNCH("join_columns_kernel", join_columns_kernel, grid, kJoinBlock, stream, plan, batchRows);
      g_stats[4]++;
    }
  }
  g_stats[0]++;
  g_stats[2] += static_cast<unsigned long long>(batchRows);
  return batchRows;
}

}  // namespace

}  // namespace ares

extern "C" size_t AresJoinColumnBytes(int rows, enum DataType type) {
  if (rows < 0 || !ares::joinable_type(type)) return 0;
  return ares::bitmap_bytes(rows) + ares::padded64(static_cast<size_t>(ares::step_in_bytes(type)) * static_cast<size_t>(rows));
}

extern "C" CGoCallResHandle AresJoinColumnsRun(const AresJoinColumns *q, int batchRows, VectorPartySlice *outSlices, void *cudaStream,
                                               int device) {
  ARES_ABI_BEGIN(device)
  if (!q) throw std::invalid_argument("null query");
  try {
    resHandle.res = ares::int_result(ares::join_columns(device, *q, batchRows, outSlices, reinterpret_cast<hipStream_t>(cudaStream)));
  } catch (const ares::NotFusable &) {
    ares::g_stats[1]++;
    throw;
  }
  ARES_ABI_END("AresJoinColumnsRun")
}

extern "C" void AresJoinColumnStats(unsigned long long *counters) {
  if (!counters) return;
  for (int i = 0; i < 3; i++) counters[i] = ares::g_stats[i].load();
  counters[3] = ares::g_stats[3].load();
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

extern "C" void AresJoinColumnFlavourStats(unsigned long long *counters) {
  if (!counters) return;
  counters[0] = ares::g_stats[4].load();
  counters[1] = ares::g_stats[5].load();
  counters[2] = ares::g_stats[3].load();
}
