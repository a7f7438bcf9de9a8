// InitIndexVector, Unary/BinaryTransform, Unary/BinaryFilter for MI355X (gfx950): the calls themselves — operand binding for
// arrays and run-length columns, the transform and the three filter strategies, the ABI entry points.  What a call may DEFINE
// instead of doing is the deferral state machine's (deferral.hpp, deferral.hip); the kernels launched here: transform_kernels.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>

#include "ares_extensions.h"

#include "binding.hpp"
#include "deferral.hpp"
#include "hash_reduce_lds.hpp"
#include "sort_reduce_fused.hpp"

#include "transform_kernels.hpp"

namespace ares {

// Queues one fast-path transform on its stream's queue.  Caller holds the device's DeferLock.
static void queue_transform(hipStream_t stream, const FastOperands &f, const SinkD &s, int n, uint32_t colRows,
                            std::shared_ptr<StreamBuffer> keep) {
  // everything pending on OTHER streams of the device is unrelated; only this stream's queue matters
  PendingQueue &q = t_state->pending[stream];
  // what the job reads (the column, the index vector) and writes (the sink's values, its validity bytes)
  ByteRange reads[3], writes[2];
  int nr = 0, nw = 0;
  column_ranges(f, colRows, [&](const ByteRange &c) { reads[nr++] = c; });
  if (f.idx) reads[nr++] = range_of(f.idx, 4ull * n);
  writes[nw++] = range_of(s.values, static_cast<uint64_t>(s.width) * n);
  if (s.nulls) writes[nw++] = range_of(s.nulls, n);
  bool conflict = q.jobs.count == kMaxMultiJobs || (q.jobs.count > 0 && (q.idx != f.idx || q.n != n));
  for (const ByteRange &w : q.writes) {
    for (int k = 0; k < nr; k++) conflict = conflict || w.overlaps(reads[k]);
    for (int k = 0; k < nw; k++) conflict = conflict || w.overlaps(writes[k]);
  }
  for (const ByteRange &r : q.reads)
    for (int k = 0; k < nw; k++) conflict = conflict || r.overlaps(writes[k]);
  if (conflict) launch_queue(stream, q);
  q.idx = f.idx;
  q.n = n;
  FastOperands fq = f;
  fq.pad = 0;
  q.jobs.f[q.jobs.count] = fq;
  q.jobs.s[q.jobs.count] = s;
  q.colRows[q.jobs.count] = colRows;
  q.jobs.count++;
  q.reads.insert(q.reads.end(), reads, reads + nr);
  q.writes.insert(q.writes.end(), writes, writes + nw);
  if (keep) q.keep.push_back(std::move(keep));
}
// ... taking the lock; returns false when deferral is unavailable (the caller launches it).
static bool defer_transform(int device, hipStream_t stream, const FastOperands &f, const SinkD &s, int n, uint32_t colRows,
                            std::shared_ptr<StreamBuffer> keep = nullptr) {
  if (!defer_available()) return false;
  DeferLock lock(device);
  queue_transform(stream, f, s, n, colRows, std::move(keep));
  return true;
}

// ---- run-length encoded columns (archive batches) -------------------------------------------------------------------------
// A call's first operand is a run-length encoded column of a 32-bit kind and rows are raw rows (no base counts): the operand
// is re-bound to the column's decoded copy for the stream's batch — made now, on the call's stream, or found in the batch's
// cache.  Returns the copy (to be kept alive by whatever is defined over it), or null when the operand stays as it is.
// The copy is a SNAPSHOT: definitions made over it (journalled filters, queued transforms) see the column as it was when
// their call came, whatever the host writes into the column afterwards — like the call's own kernel would have.
static std::shared_ptr<StreamBuffer> decode_run_length_operand(int device, hipStream_t stream, OperandD &a, const uint32_t *indexVector,
                                                              const uint32_t *baseCounts, uint32_t startCount) {
  static EnvSwitch<bool> on("ARES_EXPAND_RLE", [](const char *e) { return !(e && e[0] == '0'); });
  if (a.type != OP_COLUMN || a.mode != 3 || baseCounts != nullptr || indexVector == nullptr || !on.get() || !fuse_available()) return nullptr;
  if (!(a.kind == K_I32 || a.kind == K_U32 || a.kind == K_F32) || a.length == 0) return nullptr;
  DeferLock lock(device);
  auto j = t_state->journals.find(indexVector);  // the batch's rows: what InitIndexVector was called with
  if (j == t_state->journals.end() || j->second.stream != stream || j->second.start != 0 || j->second.n0 <= 0)
    return nullptr;
  const int rows = j->second.n0;
  std::vector<RunExpansion> &cache = t_state->expansions[stream];
  const RunExpansion *hit = nullptr;
  for (const RunExpansion &e : cache)
    if (e.base == a.base && e.nullsOff == a.nullsOff && e.valuesOff == a.valuesOff && e.length == a.length && e.bitOff == a.bitOff &&
        e.step == a.step && e.startCount == startCount && e.rows == rows)
      hit = &e;
  RunExpansion fresh;
  if (!hit) {
    const size_t nullBytes = ((static_cast<size_t>(rows) + 31) / 32 * 4 + 63) / 64 * 64;
    fresh = RunExpansion{a.base, a.nullsOff, a.valuesOff, a.length, a.bitOff, a.step, startCount, rows,
                         std::make_shared<StreamBuffer>(nullBytes + static_cast<size_t>(a.step) * rows + 64, stream), nullBytes};
    uint8_t *out = fresh.copy->as<uint8_t>();
    const int64_t tiles = (static_cast<int64_t>(rows) + 2047) / 2048;
    ARES_LAUNCH("expand_runs_kernel", expand_runs_kernel, capped_grid((tiles + kBlock / 64 - 1) / (kBlock / 64), 256 * 8), kBlock, stream,
                reinterpret_cast<const uint32_t *>(a.base), static_cast<int>(a.length), a.base + a.nullsOff, static_cast<uint32_t>(a.bitOff),
                a.base + a.valuesOff, static_cast<int>(a.step), startCount, rows, reinterpret_cast<uint32_t *>(out), out + nullBytes);
    cache.push_back(fresh);
    hit = &cache.back();
  }
  a.base = hit->copy->as<uint8_t>();
  a.mode = 2;
  a.nullsOff = 0;
  a.valuesOff = static_cast<uint32_t>(hit->valuesAt);
  a.bitOff = 0;
  a.length = static_cast<uint32_t>(rows);
  return hit->copy;
}

static bool fast_sink(const SinkD &s) {
  const bool four = s.dtype == Int32 || s.dtype == Uint32 || s.dtype == Float32;
  // (AVG_FLOAT: its 8-byte {f32 average, u32 count} pairs; the expressions it takes: avg_hot_shape below)
  if (s.type == SINK_MEASURE) return s.baseCounts == nullptr && (s.agg != AGGR_AVG_FLOAT || s.width == 8);
  // 1- / 2-byte dimension slots (city_id Uint16, status SmallEnum: query/common/dim_util.go:9-12) take integer results
  const bool narrow = s.type == SINK_DIM && (s.dtype == Int8 || s.dtype == Uint8 || s.dtype == Int16 || s.dtype == Uint16);
  return ((s.type == SINK_DIM || s.type == SINK_SCRATCH) && four) || narrow;
}

// An AVG_FLOAT measure is held back only where the Sort + Reduce scan can carry it (hr_rtc.hip, SCAN_SORT64): a bare column, or a
// column combined with a constant by Plus / Minus / Multiply; anything else keeps the generic kernel it has always had.
static bool avg_hot_shape(const FastOperands &f) {
  return f.arity == 1 || (f.arity == 2 && !f.divLike && (f.functor == Plus || f.functor == Minus || f.functor == Multiply));
}

// Binds an array column and its functor (query/binder.hpp:385-426, :458-560): the second operand
// of a binary array functor is a constant whose type fits the element type; `odt` is the value type
// of the sink (Bool for a filter's predicate).  Combinations the reference resolves to its generic
// "null" functor (functor.hpp:468-513, :573-590, :700-723) run with enabled = 0.
static void bind_array(const InputVector *ins, int arity, int functor, int odt, ArrayD &a) {
  const ArrayVectorPartySlice &vp = ins[0].Vector.ArrayVP;
  memset(&a, 0, sizeof(a));
  a.kind = kind_of_datatype(vp.DataType);
  if (a.kind == K_NONE) throw std::invalid_argument("Unsupported data type for ArrayVectorPartyInput");
  a.dtype = vp.DataType;
  a.width = step_in_bytes(vp.DataType);
  a.descriptors = vp.OffsetLengthVector;
  a.values = vp.OffsetLengthVector + 8ull * vp.Length - vp.ValueOffsetAdj;
  a.functor = functor;
  const char *badOperand = "Unsupported data type when value type of first input iterator is ArrayVP Iterator";
  if (arity == 1) {
    a.enabled = functor == ArrayLength && odt == Uint32;
    return;
  }
  if (ins[1].Type != ConstantInput) throw std::invalid_argument(badOperand);
  const ConstantVector &c = ins[1].Vector.Constant;
  const int ct = c.DataType;
  const bool fits = a.kind == K_UUID ? (ct == ConstInt || ct == ConstUUID)
                    : a.kind == K_GEO ? (ct == ConstInt || ct == ConstGeoPoint || ct == ConstUUID)
                                      : (ct == ConstInt || ct == ConstFloat);
  if (!fits) throw std::invalid_argument(badOperand);
  if (functor == ArrayElementAt) {
    a.index = c.Value.IntVal;
    a.enabled = ct == ConstInt && (a.kind == K_UUID) == (odt == UUID) && (a.kind == K_GEO) == (odt == GeoPoint);
    return;
  }
  if (functor != ArrayContains || odt != Bool) return;
  if (a.kind == K_UUID) {
    a.enabled = ct == ConstUUID;
    memcpy(a.c, &c.Value.UUIDVal, 16);
    return;
  }
  if (a.kind == K_GEO) {
    // the reference carries this constant in the upper half of a 64-bit pointer
    // (iterator.hpp:484-516, SimpleIterator<GeoPointT>): only its first four bytes survive, Long is 0
    a.enabled = ct != ConstInt;
    memcpy(a.c, &c.Value.GeoPointVal, 4);
    return;
  }
  a.enabled = 1;  // val = static_cast<element type>(constant) (functor.hpp:655)
  const bool cf = ct == ConstFloat;
  const float fv = c.Value.FloatVal;
  const int32_t iv = c.Value.IntVal;
  switch (vp.DataType) {
    case Bool: a.c[0] = cf ? fv != 0.0f : iv != 0; break;
    case Int8: a.c[0] = static_cast<uint8_t>(cf ? static_cast<int8_t>(fv) : static_cast<int8_t>(iv)); break;
    case Uint8: a.c[0] = cf ? static_cast<uint8_t>(fv) : static_cast<uint8_t>(iv); break;
    case Int16: a.c[0] = static_cast<uint16_t>(cf ? static_cast<int16_t>(fv) : static_cast<int16_t>(iv)); break;
    case Uint16: a.c[0] = cf ? static_cast<uint16_t>(fv) : static_cast<uint16_t>(iv); break;
    case Int32: a.c[0] = static_cast<uint32_t>(cf ? static_cast<int32_t>(fv) : iv); break;
    case Uint32: a.c[0] = cf ? static_cast<uint32_t>(fv) : static_cast<uint32_t>(iv); break;
    case Float32: { const float x = cf ? fv : static_cast<float>(iv); uint32_t b; memcpy(&b, &x, 4); a.c[0] = b; break; }
    default: a.c[0] = static_cast<uint64_t>(cf ? static_cast<int64_t>(fv) : static_cast<int64_t>(iv)); break;  // Int64
  }
}

static void launch_array(const ArrayD &a, const SinkD &s, int n, hipStream_t stream) {
  const int grid = capped_grid((static_cast<int64_t>(n) + kBlock - 1) / kBlock);
  ARES_LAUNCH("array_transform_kernel", array_transform_kernel, grid, kBlock, stream, a, s, n);
}

// reports what a transform launched NOW writes (deferred ones report when their queue is launched)
static void note_sink(int device, const SinkD &s, int n) {
  if (n <= 0) return;
  mem_note_write(device, s.values, static_cast<size_t>(s.width) * n);
  if (s.nulls) mem_note_write(device, s.nulls, static_cast<size_t>(n));
}

// What store_measure32 (device_model.hpp) stores for every row of `Noop(constant)`: host twin, run length 1.
static bool constant_measure_bits(const EvalParams &p, const SinkD &s, uint64_t *out) {
  if (p.rk != p.I || !(p.I == K_I32 || p.I == K_U32 || p.I == K_F32) || !(p.a.kind == K_I32 || p.a.kind == K_U32 || p.a.kind == K_F32))
    return false;
  if (!p.a.cok) {
    *out = s.width == 8 ? s.identity : static_cast<uint32_t>(s.identity);
    return true;
  }
  const uint32_t bits = host_cvt32(p.a.cbits, p.a.kind, p.I);
  const int rk = p.rk;
  auto asf = [](uint32_t b) { float f; memcpy(&f, &b, 4); return f; };
  switch (s.dtype) {
    case Int32: *out = host_cvt32(bits, rk, K_I32); return s.width == 4;
    case Uint32: *out = host_cvt32(bits, rk, K_U32); return s.width == 4;
    case Float32: *out = host_cvt32(bits, rk, K_F32); return s.width == 4;
    case Int64: {
      const int64_t v = rk == K_F32 ? static_cast<int64_t>(asf(bits)) : rk == K_I32 ? static_cast<int64_t>(static_cast<int32_t>(bits))
                                                                                    : static_cast<int64_t>(bits);
      *out = static_cast<uint64_t>(v);
      return s.width == 8;
    }
    case Float64: {
      const double d = rk == K_F32 ? static_cast<double>(asf(bits)) : rk == K_I32 ? static_cast<double>(static_cast<int32_t>(bits))
                                                                                  : static_cast<double>(bits);
      memcpy(out, &d, 8);
      return s.width == 8;
    }
    default: return false;
  }
}

static bool foreign_gather_enabled() {
  static EnvSwitch<bool> on("ARES_FOREIGN_GATHER", [](const char *e) { return !(e && e[0] == '0'); });
  return on.get();
}

// ---- constant chains: scratch frames defined, not written (deferral.hpp: FrameDef) ---------------------------------------------
namespace {
ByteRange scratch_operand_range(const OperandD &op, int n) { return range_of(op.base, static_cast<size_t>(op.nullsOff) + static_cast<size_t>(n)); }
// caller holds the device's DeferLock: a kernel of the calling entry point is about to write the sink's rows
void settle_frames_for_sink(const SinkD &s, int n) {
  if (t_state->frames.empty()) return;
  settle_frames_for_write(range_of(s.values, static_cast<size_t>(s.width) * n));
  if (s.nulls) settle_frames_for_write(range_of(s.nulls, static_cast<size_t>(n)));
}
// the index vector a job over `indexVector` reads: none where rows are positions (caller holds the device's DeferLock)
const uint32_t *rows_of(const uint32_t *indexVector, int n) { return (indexVector && !lazy_iota(indexVector, n)) ? indexVector : nullptr; }
}  // namespace

// A transform call while chains are on.  true: the call is done without a kernel —
//   * its first operand is a DEFINED frame (same pointer, validity offset, kind, rows, index vector and stream), its second an
//     eligible constant and the chain has room: it is composed — into a 4-byte integer scratch sink a new definition, into a
//     dimension or measure sink a queued job that reads the frame's COLUMN;
//   * or it is itself `column (op) constant` of the hot shape into a 4-byte integer scratch frame: the frame is defined.
// false: the call runs as ever; the frames it is handed were written first, those it overwrites retired (I1, I2).
static bool chain_transform(int device, hipStream_t stream, const EvalParams &p, const SinkD &s, const uint32_t *indexVector, int n,
                            const uint32_t *baseCounts, const std::shared_ptr<StreamBuffer> &decoded) {
  DeferLock lock(device);
  const bool intFrame = s.type == SINK_SCRATCH && s.width == 4 && (s.dtype == Int32 || s.dtype == Uint32);
  const bool queuedSink = (s.type == SINK_DIM || s.type == SINK_MEASURE) && fast_sink(s) && !(s.type == SINK_MEASURE && s.agg == AGGR_AVG_FLOAT);
  if (p.arity == 2 && p.a.type == OP_SCRATCH && p.b.type == OP_CONST && !baseCounts && (intFrame || queuedSink)) {
    auto it = t_state->frames.find(const_cast<uint8_t *>(p.a.base));
    if (it != t_state->frames.end()) {
      const FrameDef d = it->second;
      const int frameKind = fused_kind_of(d.s.dtype);
      const bool same = d.stream == stream && d.n == n && d.idxVec == indexVector && d.s.nulls == p.a.base + p.a.nullsOff && frameKind == p.a.kind;
      if (same && d.f.chain.n < kMaxChainSteps &&
          chain_step_eligible(frameKind, p.functor, p.b.kind, p.b.cok, p.I, p.rk, intFrame ? fused_kind_of(s.dtype) : p.rk)) {
        FastOperands g = d.f;
        g.chain.s[g.chain.n++] = chain_step_of(d.f, frameKind);
        g.functor = p.functor;
        g.I = p.I;
        g.rk = p.rk;
        g.bkind = p.b.kind;
        g.bbits = p.b.cbits;
        g.bok = p.b.cok;
        g.divLike = p.functor == Divide || p.functor == Mod || p.functor == Floor;
        g.idx = rows_of(indexVector, n);
        g.pad = 0;
        if (intFrame) {
          if (s.values == d.s.values) t_state->frames.erase(it);  // the frame is overwritten by its own next node: retired
          settle_frames_for_sink(s, n);
          t_state->frames[s.values] = FrameDef{stream, g, s, n, indexVector, d.colRows, d.keep};
        } else {
          settle_frames_for_sink(s, n);
          queue_transform(stream, g, s, n, d.colRows, d.keep);
        }
        return true;
      }
    }
  }
  // not composed: frames the call is handed are written before its kernel reads them, frames it overwrites go
  if (!t_state->frames.empty()) {
    if (p.a.type == OP_SCRATCH) {
      const ByteRange r = scratch_operand_range(p.a, n);
      materialize_frames(&r, false);
    }
    if (p.arity == 2 && p.b.type == OP_SCRATCH) {
      const ByteRange r = scratch_operand_range(p.b, n);
      materialize_frames(&r, false);
    }
    settle_frames_for_sink(s, n);
  }
  FastOperands f;
  if (!intFrame || baseCounts || !fast_operands(p, f, false) || f.arity != 2 ||
      !chain_step_eligible(f.akind, f.functor, f.bkind, f.bok, f.I, f.rk, fused_kind_of(s.dtype)))
    return false;
  f.idx = rows_of(f.idx, n);
  // queued transforms that write into the column come first (call order)
  for (auto &kv : t_state->pending)
    if (kv.second.jobs.count && column_ranges_touch(kv.second.writes, f, p.a.length)) launch_queue(kv.first, kv.second);
  t_state->frames[s.values] = FrameDef{stream, f, s, n, indexVector, p.a.length, decoded};
  return true;
}
// ... and a filter call: the frames it is handed are written, those over its index vector too (the vector is about to change)
static void settle_frames_for_filter(int device, const EvalParams &p, bool isArray, const uint32_t *indexVector, const uint8_t *pred, int n) {
  if (!chains_enabled()) return;
  DeferLock lock(device);
  if (t_state->frames.empty()) return;
  if (!isArray && p.a.type == OP_SCRATCH) {
    const ByteRange r = scratch_operand_range(p.a, n);
    materialize_frames(&r, false);
  }
  if (!isArray && p.arity == 2 && p.b.type == OP_SCRATCH) {
    const ByteRange r = scratch_operand_range(p.b, n);
    materialize_frames(&r, false);
  }
  materialize_frames_of_index(indexVector);
  if (indexVector) settle_frames_for_write(range_of(indexVector, 4ull * static_cast<size_t>(n)));
  settle_frames_for_write(range_of(pred, static_cast<size_t>(n)));
}

static int run_transform(const InputVector *ins, int arity, const OutputVector &output, uint32_t *indexVector,
                         int n, uint32_t *baseCounts, uint32_t startCount, int functor, hipStream_t stream, int device) {
  if (n <= 0) {
    flush_deferred(device);
    return n < 0 ? 0 : n;
  }
  if (ins[0].Type == ArrayVectorPartyInput) {
    SinkD s;
    bind_sink(output, baseCounts, s);
    ArrayD a;
    bind_array(ins, arity, functor, s.dtype, a);
    if (s.type == SINK_MEASURE && s.baseCounts) a.idx = indexVector;
    if (s.type == SINK_DIM || s.type == SINK_MEASURE) {
      grouped_note_write(device, s.values, static_cast<size_t>(s.width) * n);
      if (s.nulls) grouped_note_write(device, s.nulls, static_cast<size_t>(n));
    }
    flush_deferred(device);
    if (chains_enabled()) {
      DeferLock lock(device);
      settle_frames_for_sink(s, n);
    }
    launch_array(a, s, n, stream);
    note_sink(device, s, n);
    return n;
  }
  EvalParams p;
  SinkD s;
  CallTemps temps;
  build_params(ins, arity, stream, indexVector, baseCounts, startCount, functor, p, temps);
  // (archive batches: a run-length encoded column is read through its decoded copy — every fast path below applies)
  const std::shared_ptr<StreamBuffer> decoded = decode_run_length_operand(device, stream, p.a, indexVector, baseCounts, startCount);
  bind_sink(output, baseCounts, s);
  if (s.type == SINK_MEASURE && s.baseCounts && indexVector) p.needRow = 1;
  if (s.type == SINK_DIM || s.type == SINK_MEASURE) {  // rows of a result vector are (about to be) rewritten
    grouped_note_write(device, s.values, static_cast<size_t>(s.width) * n);
    if (s.nulls) grouped_note_write(device, s.nulls, static_cast<size_t>(n));
  }
  // a constant measure (COUNT(*) is SUM over the literal 1, query/aql_compiler.go:1191-1197): the rows are defined,
  // not written — Reduce over zero dimensions adds them up without anybody storing them (sort_reduce.hip)
  if (s.type == SINK_MEASURE && !s.baseCounts && arity == 1 && functor == Noop && p.a.type == OP_CONST && !is_wide(p.a.kind) &&
      s.agg != AGGR_AVG_FLOAT && (s.width == 4 || s.width == 8)) {
    uint64_t pattern = 0;
    if (constant_measure_bits(p, s, &pattern) && defer_fill(device, stream, s.values, static_cast<size_t>(s.width) * n, pattern, s.width))
      return n;
  }
  retire_fills_for_write(device, s.values, static_cast<size_t>(s.width) * n);
  if (s.nulls) retire_fills_for_write(device, s.nulls, static_cast<size_t>(n));
  // constant chains: an inner node of the hot shape is defined, the node over a defined frame composed (no flush, no kernel)
  if (chains_enabled() && chain_transform(device, stream, p, s, indexVector, n, baseCounts, decoded)) return n;
  FastOperands f;
  bool fast = fast_sink(s) && fast_operands(p, f, false);
  if (fast && s.type == SINK_DIM && s.width < 4 && !(f.rk == K_I32 || f.rk == K_U32)) fast = false;  // float -> narrow integer: generic kernel
  if (fast && s.type == SINK_MEASURE && s.agg == AGGR_AVG_FLOAT && !avg_hot_shape(f)) fast = false;
  if (fast && f.idx && virtual_iota(device, indexVector, n, false)) f.idx = nullptr;  // rows = position
  // root outputs of the hot shape are held back and fused with their siblings (same index vector)
  if (fast && (s.type == SINK_DIM || s.type == SINK_MEASURE) && defer_transform(device, stream, f, s, n, p.a.length, decoded)) return n;
  flush_deferred(device);
  materialize_index_vector(device, indexVector);
  note_sink(device, s, n);
  if (fast) {
    launch_fast_transform(f, s, n, stream);
  } else if (is_wide(p.a.kind)) {
    const int grid = capped_grid((static_cast<int64_t>(n) + kBlock - 1) / kBlock);
    ARES_LAUNCH("transform_wide_kernel", transform_wide_kernel, grid, kBlock, stream, p, s, n);
  } else if (foreign_gather_enabled() && p.arity == 1 && functor == Noop && p.a.type == OP_FOREIGN && !p.a.tz && !p.needRow && !s.baseCounts) {
    // a joined column into a dimension / measure vector: the join's transform on its own kernel
    constexpr int ITEMS = 8;
    const int grid = capped_grid((static_cast<int64_t>(n) + kBlock * ITEMS - 1) / (kBlock * ITEMS), 256 * 16);
    ARES_LAUNCH("transform_foreign_kernel", transform_foreign_kernel<ITEMS>, grid, kBlock, stream, p, s, n);
  } else {
    constexpr int ITEMS = 4;
    const int grid = capped_grid((static_cast<int64_t>(n) + kBlock * ITEMS - 1) / (kBlock * ITEMS), 256 * 16);
    ARES_LAUNCH("transform32_kernel", transform32_kernel<ITEMS>, grid, kBlock, stream, p, s, n);
  }
  return n;
}

// ---- filters counted in row space (filter_rows_kernel) -----------------------------------------------------------
// ARES_FILTER_ROWSPACE=0: every filter of the hot shape takes the predicate-vector path (rounds 1-3)
bool row_space_enabled() {
  static EnvSwitch<bool> on("ARES_FILTER_ROWSPACE", [](const char *e) { return !(e && e[0] == '0'); });
  return on.get();
}
namespace {
// compute units of the device, asked once
int compute_units(int device) {
  static std::mutex mu;
  static std::map<int, int> known;
  std::lock_guard<std::mutex> lock(mu);
  auto it = known.find(device);
  if (it != known.end()) return it->second;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) {
    (void)hipGetLastError();
    cus = 256;
  }
  return known[device] = cus;
}
// workgroups of `kernel` the device holds at once (occupancy x compute units), per device and kernel, asked once
int resident_blocks(int device, const void *kernel, int blockSize) {
  static std::mutex mu;
  static std::map<std::pair<int, const void *>, int> known;
  std::lock_guard<std::mutex> lock(mu);
  auto it = known.find({device, kernel});
  if (it != known.end()) return it->second;
  int perCU = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, blockSize, 0) != hipSuccess || perCU < 1) {
    (void)hipGetLastError();
    perCU = 4;
  }
  return known[{device, kernel}] = perCU * compute_units(device);
}

bool same_column(const FastOperands &a, const FastOperands &b) { return a.vals == b.vals && a.nulls == b.nulls && a.bitOff == b.bitOff; }
bool same_filter(const FastOperands &a, const FastOperands &b) {
  return same_column(a, b) && a.akind == b.akind && a.arity == b.arity && a.functor == b.functor && a.I == b.I && a.bkind == b.bkind &&
         a.bbits == b.bbits && a.bok == b.bok;
}

// May the call "filter the first n entries of indexVector by a hot-shape comparison over a column of colRows rows" be
// counted in row space?  The index vector must be iota(0 .. n0) with nothing but journalled filters since, all of them
// either applied or held as pending row-space filters, and n must be what the last of them returned.
// The core of it, for the vector's entries `jr` in the journals and `cp` in the compactions (caller holds the device's
// DeferLock).  `journalled`: the journal already counts the filter in question (journal_filter ran).  Either the filter is the
// batch's first and called with all n0 rows, or every filter before it is applied or held as a pending row-space filter of
// this stream and the last of them left survivor bits and returned n.
bool row_space_open(std::map<const uint32_t *, FilterJournal>::const_iterator jr, std::map<const uint32_t *, PendingCompact>::const_iterator cp,
                    hipStream_t stream, int n, bool journalled) {
  if (jr == t_state->journals.end() || !jr->second.valid || (journalled && jr->second.filters.empty())) return false;
  const size_t before = jr->second.filters.size() - (journalled ? 1 : 0);
  if (cp == t_state->compactions.end()) return before == 0 && jr->second.n0 == n;
  const PendingCompact &c = cp->second;
  return !c.todo.empty() && c.stream == stream && !c.noBits && c.applied + c.todo.size() == before && c.lastCount == n;
}
bool row_space_eligible(int device, hipStream_t stream, const uint32_t *indexVector, int n, uint32_t colRows) {
  if (!fuse_available() || !row_space_enabled()) return false;
  DeferLock lock(device);
  auto j = t_state->journals.find(indexVector);
  if (j == t_state->journals.end() || j->second.stream != stream || j->second.start != 0 ||
      j->second.filters.size() >= static_cast<size_t>(kFusedFilters) || colRows < static_cast<uint32_t>(j->second.n0))
    return false;
  return row_space_open(j, t_state->compactions.find(indexVector), stream, n, /*journalled=*/false);
}
// A filter is booked as counted, not applied (caller holds the device's DeferLock): `bits` are the survivors after it, or null
// with `noBits`.  Booked BEFORE the count is known: a flush from another thread that applies the pending filters meanwhile
// applies this one too.  Returns the booking's generation, what settle_counted_filter finds it by.
uint64_t book_counted_filter(PendingCompact &c, LazyFilter filter, std::shared_ptr<StreamBuffer> bits, bool noBits) {
  c.todo.push_back(std::move(filter));
  c.bits = std::move(bits);
  c.noBits = noBits;
  c.lastCount = -1;
  return c.generation = ++t_state->filterGeneration;
}
// ... and its count has come back (the stream was synchronised outside the lock): the booking, if it is still the vector's
// last, and the journal learn it; `predicted`: the filter counted beside it, or null
void settle_counted_filter(int device, const uint32_t *indexVector, uint64_t generation, int count, const PredictedFilter *predicted) {
  DeferLock lock(device);
  auto it = t_state->compactions.find(indexVector);
  if (it != t_state->compactions.end() && it->second.generation == generation) {
    it->second.lastCount = count;
    if (predicted) it->second.predicted = *predicted;
  }
  journal_count(indexVector, count);
}

// caller holds the device's DeferLock.  The batch's first row-space filter: the vector is iota(0 .. n), nothing applied
std::map<const uint32_t *, PendingCompact>::iterator open_row_space(hipStream_t stream, uint32_t *indexVector, bool virtualIdx, int n) {
  PendingCompact fresh{};
  fresh.stream = stream;
  fresh.idx = indexVector;
  fresh.virtualIdx = virtualIdx;
  fresh.n0 = n;
  fresh.applied = 0;
  fresh.lastCount = n;
  return t_state->compactions.emplace(indexVector, fresh).first;
}
// ... and every row-space filter's shape goes into the stream's history of the running batch (what predictions go by)
FilterShape note_filter_shape(FilterHistory &h, const PendingCompact &c, const FastOperands &f) {
  const FilterShape shape{f.akind, f.functor, f.I, f.bkind, f.bbits, f.bok, !c.todo.empty() && same_column(c.todo.back().f, f)};
  h.current.push_back(shape);
  return shape;
}

// The call itself.  f: the filter (idx and pad are ignored: rows = positions).  Returns the survivor count.
int run_filter_rows(int device, hipStream_t stream, FastOperands f, uint32_t *indexVector, uint8_t *pred, int n, uint32_t colRows,
                    bool virtualIdx, const std::shared_ptr<StreamBuffer> &keep = nullptr) {
  f.idx = nullptr;
  f.pad = 0;
  f.streaming = 1;  // the column is read once by this kernel: 0.060 -> 0.054 ms per 64 Mi rows (profiles/r4_experiments.md)
  constexpr int kGridCap = 2048;  // two partial counts per workgroup come back in one copy
  static_assert(2 * kGridCap <= kPinnedWords, "the partial counts are read back in one copy");
  std::shared_ptr<StreamBuffer> bits1, bits2;
  int grid = 0;
  bool two = false;
  FastOperands g = f;
  uint64_t generation = 0;
  {
    DeferLock lock(device);
    auto ins = t_state->compactions.find(indexVector);
    // The eligibility the caller established (row_space_eligible) is re-established HERE, under the lock that books the
    // filter: between the caller's check and this point another thread's flush may have applied this vector's pending
    // filters (replay + compaction) and dropped the entry — the vector is then no longer "iota with filters pending",
    // and counting this filter over the batch's first n rows would count the wrong rows (found by the soak test: one
    // count in 512 four-thread programs).  The journal already holds this filter (journal_filter ran first).
    if (!row_space_open(t_state->journals.find(indexVector), ins, stream, n, /*journalled=*/true)) return -1;
    if (ins == t_state->compactions.end()) ins = open_row_space(stream, indexVector, virtualIdx, n);
    PendingCompact &c = ins->second;
    FilterHistory &h = t_state->filterHistory[stream];
    const FilterShape shape = note_filter_shape(h, c, f);
    const size_t k = h.current.size() - 1;
    if (c.predicted.valid && same_filter(c.predicted.g, f)) {  // counted together with the previous filter: no kernel
      const int count = c.predicted.count;
      c.todo.push_back(LazyFilter{f, colRows, pred, n, keep});
      c.bits = c.predicted.bits;
      c.lastCount = count;
      c.predicted = PredictedFilter{};
      journal_count(indexVector, count);
      return count;
    }
    c.predicted = PredictedFilter{};
    // the filter the previous batch of this stream had right behind this one, if it was on the same column
    if (k + 1 < h.previous.size() && h.previous[k].same_as(shape) && h.previous[k + 1].sameColumnAsPrevious &&
        h.previous[k + 1].akind == f.akind && c.applied + c.todo.size() + 2 <= static_cast<size_t>(kFusedFilters)) {
      const FilterShape &nx = h.previous[k + 1];
      g.functor = nx.functor;
      g.I = nx.I;
      g.bkind = nx.bkind;
      g.bbits = nx.bbits;
      g.bok = nx.bok;
      two = true;
    }
    const int tiles = pred_tiles(c.n0, 0);
    // one wave of workgroups: as many as the device holds at once (a grid of 1.3 x that runs two rounds, the second a
    // third full — measured: 0.104 ms instead of 0.079 per 64 Mi rows), each striding over its share of the tiles
    const bool hasIn = static_cast<bool>(c.bits);
    auto kernel = two ? (hasIn ? &filter_rows_kernel<true, true> : &filter_rows_kernel<true, false>)
                      : (hasIn ? &filter_rows_kernel<false, true> : &filter_rows_kernel<false, false>);
    {
      // Workgroups: a multiple of the compute units, one fewer per unit than fits.  Measured per 64 Mi rows (16 384 tiles,
      // 7 workgroups fit per unit): 4 per unit 0.083 ms, 5: 0.077, 6: 0.073, 7: 0.094, 2048 in all: 0.089, 1 639 (every
      // workgroup exactly ten tiles, but 103 units with a seventh workgroup): 0.099 — the units, not the workgroups, must
      // carry equal shares (profiles/r4_experiments.md).
      const int resident = resident_blocks(device, reinterpret_cast<const void *>(kernel), kBlock), cus = compute_units(device);
      const int perUnit = std::max(1, std::min(resident / cus - 1, 6));
      grid = capped_grid(tiles, std::min(kGridCap, cus * perUnit));
    }
    const size_t bitBytes = static_cast<size_t>(tiles) * kBlock * sizeof(uint16_t);  // 16 rows per lane and tile
    bits1 = std::make_shared<StreamBuffer>(bitBytes, stream);
    if (two) bits2 = std::make_shared<StreamBuffer>(bitBytes, stream);
    // the partial counts go straight into the calling thread's pinned result slot (host memory the device can write):
    // the call then only waits for the stream — no copy command behind the kernel
    uint32_t *hostPartials = reinterpret_cast<uint32_t *>(pinned_words());
    ARES_LAUNCH("filter_rows_kernel", kernel, grid, kBlock, stream, f, g,
                hasIn ? c.bits->as<uint16_t>() : static_cast<const uint16_t *>(nullptr), bits1->as<uint16_t>(),
                two ? bits2->as<uint16_t>() : static_cast<uint16_t *>(nullptr), c.n0, tiles, hostPartials);
    generation = book_counted_filter(c, LazyFilter{f, colRows, pred, n, keep}, bits1, /*noBits=*/false);
  }
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
  const volatile uint32_t *parts = reinterpret_cast<const volatile uint32_t *>(pinned_words());
  uint32_t count = 0, count2 = 0;
  for (int b = 0; b < grid; b++) {
    count += parts[2 * b];
    count2 += parts[2 * b + 1];
  }
  const PredictedFilter predicted{true, g, static_cast<int>(count2), bits2};
  settle_counted_filter(device, indexVector, generation, static_cast<int>(count), two ? &predicted : nullptr);
  return static_cast<int>(count);
}

// Scan at filter.  The call is the LAST filter of the batch the stream's hint describes (AresHintFusedBatch) and the journal
// holds exactly the hinted filters: the batch's compact DIRECT scan — which evaluates every filter per row anyway — is
// launched in filter_rows_kernel's place, counts the survivors per workgroup into the calling thread's pinned slot and
// leaves its records stashed for the stream's HashReduce.  Decision, launch, booking and stash happen under ONE lock
// acquisition (I5).  The filter is booked exactly like a counted one, except that no survivor bits exist afterwards
// (PendingCompact::noBits).  -1: not such a call (the journal already holds the filter; the caller counts it as ever).
// A record stream that overflows does not touch the count: the scan goes on evaluating with its cursor clamped.
int run_filter_scan(int device, hipStream_t stream, FastOperands f, uint32_t *indexVector, uint8_t *pred, int n, uint32_t colRows,
                    bool virtualIdx, const std::shared_ptr<StreamBuffer> &keep) {
  ScanHint hint;
  if (keep || !scan_at_filter_enabled() || !scan_hint_live(device, stream, &hint)) return -1;
  f.idx = nullptr;
  f.pad = 0;
  int grid = 0;
  uint64_t generation = 0;
  {
    DeferLock lock(device);
    auto jr = t_state->journals.find(indexVector);
    if (jr == t_state->journals.end() || !jr->second.valid || jr->second.stream != stream || jr->second.start != 0 ||
        jr->second.n0 != hint.batchRows || jr->second.filters.size() != static_cast<size_t>(hint.plan.numFilters))
      return -1;
    const FilterJournal &j = jr->second;
    for (size_t k = 0; k < j.filters.size(); k++)
      if (!same_filter(j.filters[k], hint.filters[k]) || j.colRows[k] < static_cast<uint32_t>(j.n0)) return -1;
    auto ins = t_state->compactions.find(indexVector);
    if (!row_space_open(jr, ins, stream, n, /*journalled=*/true)) return -1;
    if (ins != t_state->compactions.end() && ins->second.predicted.valid && same_filter(ins->second.predicted.g, f)) return -1;  // (counted with the previous filter: no kernel at all)
    std::shared_ptr<ScanStash> stash = fused_scan_ahead(device, hint, stream, reinterpret_cast<uint32_t *>(pinned_words()), &grid);
    if (!stash) return -1;  // (not a batch for the compact DIRECT scan, or its kernel is not loaded yet)
    if (ins == t_state->compactions.end()) ins = open_row_space(stream, indexVector, virtualIdx, n);
    PendingCompact &c = ins->second;
    note_filter_shape(t_state->filterHistory[stream], c, f);
    c.predicted = PredictedFilter{};
    generation = book_counted_filter(c, LazyFilter{f, colRows, pred, n, keep}, nullptr, /*noBits=*/true);
    scan_stash_put(device, stream, std::move(stash));
  }
  hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
  const volatile uint32_t *parts = reinterpret_cast<const volatile uint32_t *>(pinned_words());
  uint32_t count = 0;
  for (int b = 0; b < grid; b++) count += parts[b];
  settle_counted_filter(device, indexVector, generation, static_cast<int>(count), nullptr);
  return static_cast<int>(count);
}

// Settles what is pending on the device before a filter runs and says how the filter may run.  A filter of the hot shape
// consumes a not-yet-written iota index vector directly (*virtualIdx); everything else that is pending on the device is
// launched first.  Returns true when the filter may be counted in row space (run_filter_rows).
bool prepare_filter(int device, hipStream_t stream, const EvalParams &p, uint32_t *indexVector, uint8_t *pred, int n,
                    int numForeignTables, const uint32_t *baseCounts, bool *virtualIdx) {
  bool rowSpace = false;
  *virtualIdx = false;
  FastOperands probe;
  if (!is_wide(p.a.kind) && indexVector != nullptr && numForeignTables == 0 && fast_operands(p, probe, true)) {
    *virtualIdx = virtual_iota(device, indexVector, n, true);
    // ... and, while every filter of the batch has been of that shape, is only counted — over the batch's rows, with
    // the filters before it (run_filter_rows): the pending ones of this very vector stay pending through the flush
    rowSpace = baseCounts == nullptr && row_space_eligible(device, stream, indexVector, n, p.a.length);
  }
  if (rowSpace) flush_deferred_impl(device, nullptr, nullptr, indexVector);
  else flush_deferred(device);
  // (the flush may have applied them after all: queued transforms that read the vector were launched)
  rowSpace = rowSpace && row_space_eligible(device, stream, indexVector, n, p.a.length);
  if (!rowSpace) mem_note_write(device, pred, static_cast<size_t>(n));  // (a counted filter writes no predicate bytes unless it is replayed)
  materialize_index_vector(device, indexVector);
  return rowSpace;
}

// The two-phase path of a hot-shape filter: predicate + tile counts, scan, chain-free compaction of the index vector and of
// every RecordID vector.  Without foreign tables and with a valid journal only the count is produced here; the compaction
// is left pending (PendingCompact).
int run_filter_two_phase(int device, hipStream_t stream, FastOperands f, uint32_t *indexVector, uint8_t *pred, int n,
                         RecordID **recordIDVectors, int numForeignTables, bool virtualIdx) {
  f.pad = static_cast<int>(reinterpret_cast<uintptr_t>(pred) & 3);
  const int tiles = pred_tiles(n, f.pad);
  const int passes = 1 + numForeignTables;
  // the workspace's extra words: one partial count per workgroup of the predicate kernel
  static_assert(kPredGridCap <= kPinnedWords, "the partial counts are read back in one copy");
  const int predGrid = capped_grid(tiles, kPredGridCap);
  auto wsBuf = std::make_shared<StreamBuffer>(CompactSpace::bytes(tiles, passes, predGrid), stream);
  const CompactSpace cs = clear_compact_space(*wsBuf, tiles, passes, predGrid, stream);
  if (virtualIdx) f.idx = nullptr;  // rows = position
  // lazy: the tile offsets are computed when the compaction runs; with foreign tables they are needed at once
  const bool lazy = numForeignTables == 0 && journal_is_valid(device, indexVector);
  uint32_t *partials = cs.extra();
  launch_filter_pred(f, pred, cs, n, lazy ? partials : nullptr, stream);
  if (lazy) {
    // The count is known; the compaction waits until somebody needs the compacted vector — a
    // HashReduce that re-derives the survivors from the journal never does.
    uint32_t parts[kPredGridCap];
    read_back_u32(partials, parts, predGrid, stream);
    uint32_t count = 0;
    for (int b = 0; b < predGrid; b++) count += parts[b];
    PendingCompact c;
    c.stream = stream;
    c.idx = indexVector;
    c.pred = pred;
    c.n = n;
    c.pad = f.pad;
    c.virtualIdx = virtualIdx;
    c.ws = wsBuf;
    c.space = cs;
    DeferLock lock(device);
    t_state->compactions[indexVector] = c;
    return static_cast<int>(count);
  }
  mem_note_write(device, indexVector, 4ull * static_cast<size_t>(n));
  for (int t = 0; t < numForeignTables; t++) mem_note_write(device, recordIDVectors[t], 8ull * static_cast<size_t>(n));
  launch_compaction(cs, pred, indexVector, virtualIdx, recordIDVectors, f.pad, n, stream);
  return read_compaction_total(cs, stream);
}

// The generic path — wide operands (arr: an array operand), expressions outside the hot shape and their foreign-table
// passes: one look-back kernel per pass evaluates (wide operands: reads) the predicate and compacts in place.  The index
// vector has been written by now: only a hot-shape filter consumes a lazy iota.
int run_filter_generic(int device, hipStream_t stream, EvalParams p, const ArrayD *arr, uint32_t *indexVector, uint8_t *pred, int n,
                       RecordID **recordIDVectors, int numForeignTables) {
  if (is_wide(p.a.kind)) {
    // wide operands: evaluate the predicate with the wide transform kernel, then compact by pred
    SinkD s;
    bind_pred_sink(pred, s);
    p.needRow = indexVector != nullptr;
    const int grid = capped_grid((static_cast<int64_t>(n) + kBlock - 1) / kBlock);
    if (arr)
      launch_array(*arr, s, n, stream);
    else
      ARES_LAUNCH("transform_wide_kernel", transform_wide_kernel, grid, kBlock, stream, p, s, n);
  }
  mem_note_write(device, indexVector, 4ull * static_cast<size_t>(n));
  for (int t = 0; t < numForeignTables; t++) mem_note_write(device, recordIDVectors[t], 8ull * static_cast<size_t>(n));
  const int numTiles = static_cast<int>((static_cast<int64_t>(n) + kFilterTile - 1) / kFilterTile);
  const int passes = 1 + numForeignTables;
  const size_t passBytes = 16 + sizeof(uint64_t) * static_cast<size_t>(numTiles);
  StreamBuffer wsBuf(passBytes * passes, stream);
  hip_check(hipMemsetAsync(wsBuf.get(), 0, passBytes * passes, stream), "hipMemsetAsync");
  const int grid = capped_grid(numTiles);
  uint32_t *totalDev = nullptr;
  for (int pass = 0; pass < passes; pass++) {
    uint8_t *base = wsBuf.as<uint8_t>() + passBytes * pass;
    ScanWorkspace ws;
    ws.ticket = reinterpret_cast<unsigned int *>(base);
    ws.total = reinterpret_cast<uint32_t *>(base + 4);
    ws.error = reinterpret_cast<uint32_t *>(wsBuf.as<uint8_t>() + 8);  // shared by all passes
    ws.status = reinterpret_cast<uint64_t *>(base + 16);
    if (pass == 0) {
      totalDev = ws.total;
      if (is_wide(p.a.kind)) {
        ARES_LAUNCH("filter_kernel<2>", filter_kernel<2>, grid, kBlock, stream, p, pred, indexVector,
                           static_cast<uint64_t *>(nullptr), ws, n, numTiles);
      } else {
        ARES_LAUNCH("filter_kernel<0>", filter_kernel<0>, grid, kBlock, stream, p, pred, indexVector,
                    static_cast<uint64_t *>(nullptr), ws, n, numTiles);
      }
    } else {
      ARES_LAUNCH("filter_kernel<1>", filter_kernel<1>, grid, kBlock, stream, p, pred, indexVector,
                  reinterpret_cast<uint64_t *>(recordIDVectors[pass - 1]), ws, n, numTiles);
    }
  }
  uint32_t result[2] = {0, 0};  // {survivors, error}
  read_back_u32(totalDev, result, 2, stream);
  if (result[1]) throw AlgorithmError("ERROR: filter: inter-tile scan timed out");
  return static_cast<int>(result[0]);
}
}  // namespace

static int run_filter(const InputVector *ins, int arity, uint32_t *indexVector, uint8_t *pred, int n,
                      RecordID **recordIDVectors, int numForeignTables, uint32_t *baseCounts, uint32_t startCount,
                      int functor, hipStream_t stream, int device) {
  if (numForeignTables < 0 || numForeignTables > 8) throw std::invalid_argument("only support up to 8 foreign tables");
  if (n <= 0) {
    flush_deferred(device);
    return 0;
  }
  EvalParams p;
  CallTemps temps;
  const bool isArray = ins[0].Type == ArrayVectorPartyInput;
  ArrayD arr;
  std::shared_ptr<StreamBuffer> decoded;  // the decoded copy of a run-length encoded column (archive batches), or null
  if (isArray) {
    bind_array(ins, arity, functor, Bool, arr);
    memset(&p, 0, sizeof(p));
    p.a.kind = K_UUID;  // routed like a wide operand: predicate first, then compaction by predicate
  } else {
    build_params(ins, arity, stream, indexVector, baseCounts, startCount, functor, p, temps);
    decoded = decode_run_length_operand(device, stream, p.a, indexVector, baseCounts, startCount);
  }
  p.needRow = 1;
  settle_frames_for_filter(device, p, isArray, indexVector, pred, n);
  bool virtualIdx = false;
  const bool rowSpace = prepare_filter(device, stream, p, indexVector, pred, n, numForeignTables, baseCounts, &virtualIdx);
  FastOperands f;
  const bool fast = !is_wide(p.a.kind) && indexVector != nullptr && fast_operands(p, f, true);
  if (fast && numForeignTables == 0 && baseCounts == nullptr)
    journal_filter(device, indexVector, &f, p.a.length, n, decoded);
  else
    journal_filter(device, indexVector, nullptr, 0, 0);
  if (rowSpace && fast && journal_is_valid(device, indexVector)) {
    const int scanned = run_filter_scan(device, stream, f, indexVector, pred, n, p.a.length, virtualIdx, decoded);
    if (scanned >= 0) return scanned;
    const int counted = run_filter_rows(device, stream, f, indexVector, pred, n, p.a.length, virtualIdx, decoded);
    if (counted >= 0) return counted;
    // (-1: somebody's flush applied the vector's pending filters since the eligibility check: the ordinary filter below)
  }
  if (rowSpace) {  // the predicate vector is written after all
    mem_note_write(device, pred, static_cast<size_t>(n));
    DeferLock lock(device);
    run_compaction(indexVector);
  }
  if (fast) return run_filter_two_phase(device, stream, f, indexVector, pred, n, recordIDVectors, numForeignTables, virtualIdx);
  return run_filter_generic(device, stream, p, isArray ? &arr : nullptr, indexVector, pred, n, recordIDVectors, numForeignTables);
}

}  // namespace ares

using namespace ares;

extern "C" {

CGoCallResHandle InitIndexVector(uint32_t *indexVector, uint32_t start, int indexVectorLength, void *cudaStream,
                                 int device) {
  ARES_ABI_BEGIN_NOFLUSH(device)
  hipStream_t stream = reinterpret_cast<hipStream_t>(cudaStream);
  scan_hint_init_index(device, stream);  // (the hinted batch begins — or it is over, and so is the hint)
  begin_batch(device, stream, indexVector, start, indexVectorLength);
  if (!defer_iota(device, stream, indexVector, start, indexVectorLength)) {
    flush_deferred(device);
    DeferLock lock(device);
    launch_init_index(indexVector, start, indexVectorLength, stream);
  }
  ARES_ABI_END("InitIndexVector")
}

CGoCallResHandle UnaryTransform(InputVector input, OutputVector output, uint32_t *indexVector,
                                int indexVectorLength, uint32_t *baseCounts, uint32_t startCount,
                                enum UnaryFunctorType functorType, void *cudaStream, int device) {
  ARES_ABI_BEGIN_NOFLUSH(device)
  resHandle.res = int_result(run_transform(&input, 1, output, indexVector, indexVectorLength, baseCounts,
                                           startCount, functorType, reinterpret_cast<hipStream_t>(cudaStream), device));
  ARES_ABI_END("UnaryTransform")
}

CGoCallResHandle BinaryTransform(InputVector lhs, InputVector rhs, OutputVector output, uint32_t *indexVector,
                                 int indexVectorLength, uint32_t *baseCounts, uint32_t startCount,
                                 enum BinaryFunctorType functorType, void *cudaStream, int device) {
  ARES_ABI_BEGIN_NOFLUSH(device)
  InputVector ins[2] = {lhs, rhs};
  resHandle.res = int_result(run_transform(ins, 2, output, indexVector, indexVectorLength, baseCounts, startCount,
                                           functorType, reinterpret_cast<hipStream_t>(cudaStream), device));
  ARES_ABI_END("BinaryTransform")
}

CGoCallResHandle UnaryFilter(InputVector input, uint32_t *indexVector, uint8_t *predicateVector,
                             int indexVectorLength, RecordID **recordIDVectors, int numForeignTables,
                             uint32_t *baseCounts, uint32_t startCount, enum UnaryFunctorType functorType,
                             void *cudaStream, int device) {
  ARES_ABI_BEGIN_NOFLUSH(device)
  resHandle.res = int_result(run_filter(&input, 1, indexVector, predicateVector, indexVectorLength, recordIDVectors,
                                        numForeignTables, baseCounts, startCount, functorType,
                                        reinterpret_cast<hipStream_t>(cudaStream), device));
  ARES_ABI_END("UnaryFilter")
}

CGoCallResHandle BinaryFilter(InputVector lhs, InputVector rhs, uint32_t *indexVector, uint8_t *predicateVector,
                              int indexVectorLength, RecordID **recordIDVectors, int numForeignTables,
                              uint32_t *baseCounts, uint32_t startCount, enum BinaryFunctorType functorType,
                              void *cudaStream, int device) {
  ARES_ABI_BEGIN_NOFLUSH(device)
  InputVector ins[2] = {lhs, rhs};
  resHandle.res = int_result(run_filter(ins, 2, indexVector, predicateVector, indexVectorLength, recordIDVectors,
                                        numForeignTables, baseCounts, startCount, functorType,
                                        reinterpret_cast<hipStream_t>(cudaStream), device));
  ARES_ABI_END("BinaryFilter")
}

}  // extern "C"
