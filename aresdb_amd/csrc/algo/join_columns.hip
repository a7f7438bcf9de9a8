// Joined columns resolved once per batch, in row space (AresJoinColumnsRun, include/ares_extensions.h): the key column of a
// batch is probed with HashLookup's geometry — one row and one probe per lane, nothing else held in registers — and up to four
// joined columns are gathered into ordinary mode-2 main-table columns (validity bitmap + values) of the batch's length.  The
// host then runs the batch as a join-free query over its columns plus these, on every fast path a join-free query has.
//
// The probe is cuckoo_probe (cuckoo_probe.hpp) and the gather load_foreign32 (device_model.hpp), both unchanged: row r holds
// what the per-node sequence (HashLookup, then a foreign operand over the record ids) reads for it.  A wavefront's 64 rows
// start on a multiple of 64, so a column's validity word is one ballot and one 8-byte store by one lane, and the values of
// a wavefront are one contiguous range.  Rows that fail a pruning hint (the query's own main-table filters, compared with
// compare_fast as the row-space filters do) skip the probe and are written as (0, null).
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
#include "row_hints.hpp"
#include "select_scan.hpp"

namespace ares {

namespace {

constexpr int kJoinBlock = 256;
constexpr int kJoinFilters = 4;  // AresJoinColumns::filters
constexpr int kJoinColumns = 4;  // AresJoinColumns::columns

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
  unsigned long long *probed;  // the device's counter of keys probed
};
static_assert(sizeof(JoinColumnsPlanD) <= 2048, "the plan is the kernel's argument");

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

// ---- host side ------------------------------------------------------------------------------------------------------
std::atomic<unsigned long long> g_stats[3];  // batches run, batches declined, rows (keys probed: counted on the devices)

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

bool join_columns_enabled() {
  static EnvSwitch<bool> on("ARES_JOIN_COLUMNS", [](const char *e) { return !(e && e[0] == '0'); });
  return on.get();
}

int join_columns_grid(int64_t rows) {
  static EnvSwitch<int> forced("ARES_JOIN_COLUMNS_GRID", [](const char *e) { return e ? atoi(e) : 0; });
  const int f = forced.get();
  const int64_t blocks = (rows + kJoinBlock - 1) / kJoinBlock;
  if (f > 0) return capped_grid(blocks, f);
  return capped_grid(blocks, 256 * 16);  // hash_lookup_kernel's
}

bool joinable_type(int t) { return t == Int8 || t == Uint8 || t == Int16 || t == Uint16 || t == Int32 || t == Uint32 || t == Float32; }

int join_columns(int device, const AresJoinColumns &q, int batchRows, VectorPartySlice *outSlices, hipStream_t stream) {
  if (!join_columns_enabled()) throw NotFusable("switched off (ARES_JOIN_COLUMNS=0)");
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
  CallTemps temps;  // (the joined columns' batch descriptors: released in stream order behind the launch)
  JoinColumnsPlanD plan;
  memset(&plan, 0, sizeof(plan));
  const SelectJoinD join = bind_join(q.join, batchRows, stream, temps);
  plan.key = join.key;
  plan.index = join.index;
  const int numHints = q.numFilters < 0 ? 0 : q.numFilters > kJoinFilters ? kJoinFilters : q.numFilters;
  for (int k = 0; k < numHints; k++)
    if (bind_hint(q.filters[k], batchRows, stream, plan.filters[plan.numFilters])) plan.numFilters++;
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
  plan.probed = probe_counter(device);

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
    const int grid = join_columns_grid(batchRows);
    ARES_LAUNCH("join_columns_kernel", join_columns_kernel, grid, kJoinBlock, stream, plan, batchRows);
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
  counters[3] = 0;
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
