// The deferral state machine proper (contract, kinds of state and invariants: deferral.hpp): the per-device state and its
// lock, the registration with libmem.so, and every way a held-back definition is written, retired or dropped — error words,
// queues and limbo, iotas, fills, lazily defined sorts, compactions, the flush family, the filter journal.  The kernels
// that write a definition: deferral_kernels.hpp.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <string>

#include "ares_extensions.h"

#include "deferral.hpp"
#include "hash_reduce_lds.hpp"
#include "sort_reduce_fused.hpp"

#include "deferral_kernels.hpp"

namespace ares {

thread_local DeferState *t_state = nullptr;
thread_local std::vector<hipStream_t> t_syncAfterUnlock;
void (*g_releaseHeld)(int, uintptr_t) = nullptr;
bool g_fuseEnabled = true;

void order_before_caller(hipStream_t producer) {
  if (!t_callStream.known || t_callStream.stream != producer) t_syncAfterUnlock.push_back(producer);
}

// registers the flush hook with the sibling libmem.so; false = deferral is off for this process
bool defer_available() {
  static const bool ok = [] {
    const char *e = getenv("ARES_DEFER");
    if (e && e[0] == '0') return false;
    Dl_info info;
    if (!dladdr(reinterpret_cast<void *>(&AresFlushDeferred), &info) || !info.dli_fname) return false;
    std::string path(info.dli_fname);
    const size_t slash = path.rfind('/');
    path = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/libmem.so";
    void *h = dlopen(path.c_str(), RTLD_NOW | RTLD_NOLOAD);  // only if the host already uses it
    if (!h) return false;
    auto set = reinterpret_cast<void (*)(void (*)(int))>(dlsym(h, "AresMemSetFlushHook"));
    if (!set) return false;
    set(&AresFlushDeferred);
    // second stage (optional: an older libmem.so only knows the flush hook)
    const char *fuse = getenv("ARES_FUSE");
    auto setHooks = reinterpret_cast<void (*)(const AresDeferralHooks *)>(dlsym(h, "AresMemSetDeferralHooks"));
    auto release = reinterpret_cast<void (*)(int, uintptr_t)>(dlsym(h, "AresMemReleaseHeld"));
    g_fuseEnabled = !(fuse && fuse[0] == '0');
    if (setHooks && release) {  // the hooks also tell HashReduce whether its previous results are untouched
      static const AresDeferralHooks hooks = {&AresFlushDeferred, &hook_on_wait, &hook_on_free, &hook_on_access};
      g_releaseHeld = release;
      setHooks(&hooks);
    }
    auto setAux = reinterpret_cast<void (*)(const AresMemAuxHooks *)>(dlsym(h, "AresMemSetAuxHooks"));
    if (setAux) {
      static const AresMemAuxHooks aux = {sizeof(AresMemAuxHooks), &hook_on_write, &hook_on_stream_destroy, &hook_trim};
      setAux(&aux);
    }
    g_memTrimCache = reinterpret_cast<void (*)(int)>(dlsym(h, "AresMemTrimCache"));
    g_memNoteWrite = reinterpret_cast<void (*)(int, const void *, size_t)>(dlsym(h, "AresMemNoteWrite"));
    auto track = reinterpret_cast<void (*)()>(dlsym(h, "AresMemEnableWriteTracking"));
    if (g_memNoteWrite && track) track();  // from here on every kernel output is reported
    else g_memNoteWrite = nullptr;
    g_memNoteActivity = reinterpret_cast<void (*)()>(dlsym(h, "AresMemNoteActivity"));
    auto share = reinterpret_cast<void (*)()>(dlsym(h, "AresMemEnableActivityTracking"));
    if (g_memNoteActivity && share) share();  // from here on every entry point and every launch is reported: frees may share fences
    else g_memNoteActivity = nullptr;
    return true;
  }();
  return ok;
}
// second-stage fusion (HashReduce consumes pending transforms, lazy compaction): ARES_FUSE=0 switches it
// off; the hooks stay in place
bool fuse_available() { return defer_available() && g_releaseHeld != nullptr && g_fuseEnabled; }
bool deferral_hooks_active() { return defer_available() && g_releaseHeld != nullptr; }

static DeferState &state_of(int device) {
  static struct States {
    DeferState of[kMaxDevices];
    States() {
      for (int d = 0; d < kMaxDevices; d++) of[d].device = d;
    }
  } states;
  if (device < 0 || device >= kMaxDevices) throw std::invalid_argument("device index out of range");
  return states.of[device];
}
DeferLock::DeferLock(int device) : lock(state_of(device).mutex, std::defer_lock) {
  {
    SlowScope slow("wait for the device's deferral lock");
    lock.lock();
  }
  t_state = &state_of(device);
}

// caller holds the device's DeferLock
static void watch_error_word(hipStream_t stream, const uint32_t *errorDev, std::shared_ptr<StreamBuffer> ws) {
  ErrorCheck c;
  c.stream = stream;
  c.ws = std::move(ws);
  if (!t_state->errorSlots.empty()) {
    c.pinned = t_state->errorSlots.back();
    t_state->errorSlots.pop_back();
  } else {
    hip_check(hipHostMalloc(reinterpret_cast<void **>(&c.pinned), sizeof(uint32_t), hipHostMallocPortable), "hipHostMalloc");
  }
  hip_check(hipEventCreateWithFlags(&c.done, hipEventDisableTiming), "hipEventCreate");
  *c.pinned = 0;
  hip_check(hipMemcpyAsync(c.pinned, errorDev, sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync");
  hip_check(hipEventRecord(c.done, stream), "hipEventRecord");
  t_state->errorChecks.push_back(std::move(c));
}

// caller holds the device's DeferLock: check i has landed (its event is done, or its stream is idle).  The event goes, the
// pinned word is recycled, the last check takes the slot; true when the compaction reported a failure
bool retire_error_check(size_t i) {
  ErrorCheck &c = t_state->errorChecks[i];
  const bool failed = *c.pinned != 0;
  (void)hipEventDestroy(c.done);
  t_state->errorSlots.push_back(c.pinned);
  t_state->errorChecks[i] = std::move(t_state->errorChecks.back());
  t_state->errorChecks.pop_back();
  return failed;
}

// caller holds the device's DeferLock; throws when a finished lazy compaction reported a failure
static void poll_error_words() {
  bool failed = t_state->errorSeen;
  t_state->errorSeen = false;
  for (size_t i = 0; i < t_state->errorChecks.size();) {
    if (hipEventQuery(t_state->errorChecks[i].done) == hipSuccess) {
      failed = retire_error_check(i) || failed;
    } else {
      (void)hipGetLastError();
      i++;
    }
  }
  if (failed) throw AlgorithmError("ERROR: filter: compaction wait timed out (reported by a deferred compaction)");
}

// tiles of filter_pred_kernel's geometry that n predicate bytes span, counted in quads from `pad` bytes below the first
int pred_tiles(int n, int pad) {
  const int64_t numQuads = (static_cast<int64_t>(n) + pad + 3) / 4;
  return static_cast<int>((numQuads + kBlock * kPQ - 1) / (kBlock * kPQ));
}
// lays a compaction's workspace out over `ws` (CompactSpace::bytes of the same three numbers) and clears it: one fill
// for head, counts and flags
CompactSpace clear_compact_space(const StreamBuffer &ws, int tiles, int passes, size_t extraWords, hipStream_t stream) {
  CompactSpace cs;
  cs.words = ws.as<uint32_t>();
  cs.tiles = tiles;
  cs.passes = passes;
  hip_check(hipMemsetAsync(cs.words, 0, CompactSpace::bytes(tiles, passes, extraWords), stream), "hipMemsetAsync");
  return cs;
}
// Predicate bytes of the first n entries and their tile counts into the (cleared) workspace; blockTotals (or null): one
// partial count per workgroup — capped_grid(cs.tiles, kPredGridCap) of them
void launch_filter_pred(const FastOperands &f, uint8_t *pred, const CompactSpace &cs, int n, uint32_t *blockTotals, hipStream_t stream) {
  ARES_LAUNCH("filter_pred_kernel", filter_pred_kernel, capped_grid(cs.tiles, kPredGridCap), kBlock, stream, f, pred, cs.tileCounts(), n, cs.tiles,
              blockTotals);
}
// The tile counts of `pred` are in place: their scan, then the chain-free in-place compaction of the index vector
// (virtualIdx: it is iota(0 .. n) and not written — nothing is read from it) and of every RecordID vector.
void launch_compaction(const CompactSpace &cs, const uint8_t *pred, uint32_t *idx, bool virtualIdx, RecordID **recordIDVectors, int pad, int n,
                       hipStream_t stream) {
  ARES_LAUNCH("filter_scan_kernel", filter_scan_kernel, 1, 1024, stream, cs.tileCounts(), cs.tileOffsets(), cs.tiles, cs.total());
  const int cgrid = capped_grid((cs.tiles + kTilesPerTicket - 1) / kTilesPerTicket, 256 * 8);
  for (int pass = 0; pass < cs.passes; pass++) {
    CompactWorkspace cw;
    cw.ticket = cs.tickets() + pass;
    cw.error = cs.error();
    cw.tileOffsets = cs.tileOffsets();
    cw.loaded = cs.loaded() + static_cast<size_t>(cs.tiles) * pass;
    if (pass == 0 && virtualIdx)
      ARES_LAUNCH("filter_compact_kernel<iota>", (filter_compact_kernel<uint32_t, true>), cgrid, kBlock, stream, pred, idx, 0u, pad, cw, n,
                  cs.tiles);
    else if (pass == 0)
      ARES_LAUNCH("filter_compact_kernel", (filter_compact_kernel<uint32_t, false>), cgrid, kBlock, stream, pred, idx, 0u, pad, cw, n,
                  cs.tiles);
    else
      ARES_LAUNCH("filter_compact_kernel<rid>", (filter_compact_kernel<uint64_t, false>), cgrid, kBlock, stream, pred,
                  reinterpret_cast<uint64_t *>(recordIDVectors[pass - 1]), 0u, pad, cw, n, cs.tiles);
  }
}
// ... and what an eager caller ends with: the survivor count, or the compaction's bounded wait timed out
int read_compaction_total(const CompactSpace &cs, hipStream_t stream) {
  uint32_t result[2] = {0, 0};  // {survivors, error}
  read_back_u32(cs.total(), result, 2, stream);
  if (result[1]) throw AlgorithmError("ERROR: filter: compaction wait timed out");
  return static_cast<int>(result[0]);
}

// caller holds the device's DeferLock and has selected the device: runs the pending compaction of `idx` (if
// there is one) on the stream its filter ran on
static void replay_lazy_filters(const PendingCompact &c);
void run_compaction(const uint32_t *idx) {
  auto it = t_state->compactions.find(idx);
  if (it == t_state->compactions.end()) return;
  const PendingCompact c = it->second;
  t_state->compactions.erase(it);
  if (!c.todo.empty()) {
    replay_lazy_filters(c);
    return;
  }
  mem_note_write(t_state->device, c.idx, 4ull * static_cast<size_t>(c.n));
  launch_compaction(c.space, c.pred, c.idx, c.virtualIdx, nullptr, c.pad, c.n, c.stream);
  watch_error_word(c.stream, c.space.error(), c.ws);
  order_before_caller(c.stream);
  // (c.ws is released to the stream's cache when the last copy of the shared_ptr goes: behind the launch
  // and the copy of the error word)
}
// Filters that were only counted (filter_rows_kernel) are applied to the index vector after all: each one as the call
// would have run eagerly — predicate bytes over the vector as the previous filter left it, tile counts, offsets,
// in-place compaction — so that predicate and index vectors hold exactly what the reference leaves in them.
// caller holds the device's DeferLock and has selected the device
static void replay_lazy_filters(const PendingCompact &c) {
  bool virtualIdx = c.virtualIdx;
  mem_note_write(t_state->device, c.idx, 4ull * static_cast<size_t>(c.n0));
  for (const LazyFilter &L : c.todo) {
    const int n = L.rowsBefore;
    if (n <= 0) break;
    mem_note_write(t_state->device, L.pred, static_cast<size_t>(n));
    FastOperands f = L.f;
    f.idx = virtualIdx ? nullptr : c.idx;
    f.pad = static_cast<int>(reinterpret_cast<uintptr_t>(L.pred) & 3);
    const int tiles = pred_tiles(n, f.pad);
    auto wsBuf = std::make_shared<StreamBuffer>(CompactSpace::bytes(tiles, 1, 0), c.stream);
    const CompactSpace cs = clear_compact_space(*wsBuf, tiles, 1, 0, c.stream);
    launch_filter_pred(f, L.pred, cs, n, nullptr, c.stream);
    launch_compaction(cs, L.pred, c.idx, virtualIdx, nullptr, f.pad, n, c.stream);
    watch_error_word(c.stream, cs.error(), wsBuf);
    virtualIdx = false;
  }
  order_before_caller(c.stream);
}

// (range_of counts a range of no bytes as its first byte: a filter booked over no rows, or a column of no rows, would hit on
// that byte — neither is ever booked, and a hit only makes a caller launch or hold something early)
bool compaction_touches(const PendingCompact &c, const ByteRange &r) {
  if (!c.todo.empty()) {  // index vector, every predicate vector and every column a replay would read
    bool hit = range_of(c.idx, 4ull * c.n0).overlaps(r);
    for (const LazyFilter &L : c.todo) hit = hit || range_of(L.pred, L.rowsBefore).overlaps(r) || column_overlaps(L.f, L.colRows, r);
    return hit;
  }
  return range_of(c.idx, 4ull * c.n).overlaps(r) || range_of(c.pred, c.n).overlaps(r);
}

// the geometry of transform_fast_kernel / transform_multi_kernel: quads of n positions counted from `pad` bytes below the
// first, and the workgroups that take their tiles
static int64_t fast_quads(int n, int pad) { return (static_cast<int64_t>(n) + pad + 3) / 4; }
static int fast_grid(int64_t numQuads) { return capped_grid((numQuads + kBlock * kTQ - 1) / (kBlock * kTQ), 256 * 16); }
// One fast transform on a kernel of its own: the quads are counted from where the sink's validity bytes are 4-byte aligned
// (a measure has none).
void launch_fast_transform(FastOperands f, const SinkD &s, int n, hipStream_t stream) {
  f.pad = s.type == SINK_MEASURE ? 0 : static_cast<int>(reinterpret_cast<uintptr_t>(s.nulls) & 3);
  const int64_t numQuads = fast_quads(n, f.pad);
  ARES_LAUNCH("transform_fast_kernel", transform_fast_kernel, fast_grid(numQuads), kBlock, stream, f, s, n, numQuads);
}

// caller holds the device's DeferLock and has selected the device.  inOrder: the launch is part of the
// stream's own call sequence (a later call on the same stream follows); otherwise a queue the host
// has already waited for is synchronised after its late launch.
void launch_queue(hipStream_t stream, PendingQueue &q, bool inOrder) {
  if (q.jobs.count == 0) return;
  const bool syncAfter = q.overWait && !inOrder;
  q.overWait = false;
  if (q.idx) run_compaction(q.idx);  // the transforms read the compacted index vector
  if (q.jobs.count == 1) {
    FastOperands f = q.jobs.f[0];
    f.idx = q.idx;
    launch_fast_transform(f, q.jobs.s[0], q.n, stream);
  } else {
    const int64_t numQuads = fast_quads(q.n, 0);
    ARES_LAUNCH("transform_multi_kernel", transform_multi_kernel, fast_grid(numQuads), kBlock, stream, q.jobs, q.idx, q.n, numQuads);
  }
  if (g_memNoteWrite) {
    const int device = current_device();
    for (const ByteRange &w : q.writes) mem_note_write(device, w.lo, static_cast<size_t>(w.hi - w.lo));
  }
  q.jobs.count = 0;
  q.reads.clear();
  q.writes.clear();
  q.keep.clear();  // (released in stream order, behind the kernel that read them)
  if (syncAfter) t_syncAfterUnlock.push_back(stream);  // (DeferLock: after the mutex is released)
}

// ---- scratch frames defined as constant chains --------------------------------------------------------------------------
// ARES_CHAINS=0: no frame is ever defined — every inner node launches its own kernel, as before there were chains
bool chains_enabled() {
  static EnvSwitch<bool> on("ARES_CHAINS", [](const char *e) { return !(e && e[0] == '0'); });
  return on.get() && fuse_available();
}
bool frame_writes_touch(const FrameDef &d, const ByteRange &r) {
  return range_of(d.s.values, 4ull * d.n).overlaps(r) || range_of(d.s.nulls, static_cast<size_t>(d.n)).overlaps(r);
}
bool frame_reads_touch(const FrameDef &d, const ByteRange &r) {
  return column_overlaps(d.f, d.colRows, r) || (d.idxVec && range_of(d.idxVec, 4ull * d.n).overlaps(r));
}
// caller holds the device's DeferLock and has selected the device: the frame is written now — what the defining calls would
// have left in it — on the stream it was defined on, behind the compaction (or the iota) of the index vector it reads
std::map<uint8_t *, FrameDef>::iterator materialize_frame(std::map<uint8_t *, FrameDef>::iterator it) {
  const FrameDef d = it->second;
  it = t_state->frames.erase(it);  // (the entry goes first: nothing below finds it again)
  if (d.f.idx) {
    run_compaction(d.f.idx);
    auto io = t_state->iotas.find(const_cast<uint32_t *>(d.f.idx));
    if (io != t_state->iotas.end()) write_iota(io);
  }
  mem_note_write(t_state->device, d.s.values, 4ull * static_cast<size_t>(d.n));
  mem_note_write(t_state->device, d.s.nulls, static_cast<size_t>(d.n));
  launch_fast_transform(d.f, d.s, d.n, d.stream);
  if (d.overWait) t_syncAfterUnlock.push_back(d.stream);  // the host believes the stream idle
  else order_before_caller(d.stream);
  return it;
}
void materialize_frames(const ByteRange *r, bool readsToo) {
  for (auto it = t_state->frames.begin(); it != t_state->frames.end();) {
    const bool hit = !r || frame_writes_touch(it->second, *r) || (readsToo && frame_reads_touch(it->second, *r));
    if (hit) {
      materialize_frame(it);
      it = t_state->frames.begin();  // (the compaction it ran first may have touched the map's neighbours: start over)
    } else {
      ++it;
    }
  }
}
// the index vector is about to mean something else (a filter compacts it, InitIndexVector redefines it)
void materialize_frames_of_index(const uint32_t *indexVector) {
  for (auto it = t_state->frames.begin(); it != t_state->frames.end();) {
    if (indexVector && it->second.idxVec == indexVector) {
      materialize_frame(it);
      it = t_state->frames.begin();
    } else {
      ++it;
    }
  }
}
void settle_frames_for_write(const ByteRange &r) {
  for (auto it = t_state->frames.begin(); it != t_state->frames.end();) {
    const FrameDef &d = it->second;
    const ByteRange v = range_of(d.s.values, 4ull * d.n), nb = range_of(d.s.nulls, static_cast<size_t>(d.n));
    if (frame_reads_touch(d, r)) {
      materialize_frame(it);
      it = t_state->frames.begin();
    } else if (!v.overlaps(r) && !nb.overlaps(r)) {
      ++it;
    } else if (r.lo <= v.lo && v.hi <= r.hi) {  // the values are overwritten whole (validity bytes follow their values): retired
      it = t_state->frames.erase(it);
    } else {
      materialize_frame(it);
      it = t_state->frames.begin();
    }
  }
}
// for the entry points that do not say what they read (ARES_ABI_BEGIN): every frame of the device is written
void materialize_all_frames(int device) {
  if (!defer_available()) return;
  DeferLock lock(device);
  if (!t_state->frames.empty()) materialize_frames(nullptr, false);
}

// caller holds the device's DeferLock.  Launches the skipped transforms of every limbo entry of the device
// (range == nullptr) or of those whose outputs overlap `range`, and forgets the entries.
bool materialize_limbo(const ByteRange *range, ReleaseSet *released) {
  bool any = false;
  for (auto it = t_state->limbo.begin(); it != t_state->limbo.end();) {
    const bool hit = !range || touches(it->second.writes, *range);
    if (hit && it->second.sortIdx) {  // consumed by a fused Sort + Reduce: the whole sequence is replayed (the entry goes with it)
      materialize_sort(it->second.sortIdx);
      it = t_state->limbo.begin();
      any = true;
    } else if (hit) {
      it->second.overWait = true;  // the host believes this work is long done
      launch_queue(it->first, it->second);
      if (released) released->add(it->first);
      it = t_state->limbo.erase(it);
      any = true;
    } else {
      ++it;
    }
  }
  return any;
}

// caller holds the device's DeferLock.  A limbo entry dies: its skipped outputs will never be written.  The compaction only it
// would need goes with it, the blocks held for its stream may go (`released`; null: the caller releases the stream's
// tag anyway, as begin_batch and hook_on_stream_destroy do), and what a Reduce that consumed the queue left defined cannot be replayed any more.  Returns the next entry.
std::map<hipStream_t, PendingQueue>::iterator drop_limbo(std::map<hipStream_t, PendingQueue>::iterator it, ReleaseSet *released) {
  if (it->second.idx) t_state->compactions.erase(it->second.idx);
  if (released) released->add(it->first);
  const uint32_t *sortIdx = it->second.sortIdx;
  it = t_state->limbo.erase(it);
  if (sortIdx) drop_sort(sortIdx);
  return it;
}

// caller holds the device's DeferLock and has selected the device
void launch_init_index(uint32_t *indexVector, uint32_t start, int n, hipStream_t stream) {
  if (n > 0) mem_note_write(current_device(), indexVector, 4ull * static_cast<size_t>(n));
  if (n <= 0) return;
  const int64_t quads = (static_cast<int64_t>(n) + 3) / 4;
  const int grid = capped_grid((quads + kBlock - 1) / kBlock, 256 * 16);
  ARES_LAUNCH("init_index_kernel", init_index_kernel, grid, kBlock, stream, indexVector, start, n);
  order_before_caller(stream);  // (a lazy iota written at another stream's flush point)
}

// caller holds the device's DeferLock: the entry of `indexVector` when the vector is a lazy iota(0 .. n) that no Sort has
// been defined over, or null.  (What `consumed` must be is the caller's business.)
PendingIota *lazy_iota(const uint32_t *indexVector, int n) {
  auto it = t_state->iotas.find(const_cast<uint32_t *>(indexVector));
  if (it == t_state->iotas.end() || it->second.start != 0 || it->second.n != n || it->second.sorted) return nullptr;
  return &it->second;
}

// caller holds the device's DeferLock and has selected the device: what the entry defines its vector to hold is written
// now — the iota or, once `sorted`, what the lazily defined Sort leaves (materialize_sort: the entry goes with the
// definition).  Returns where a loop over the iotas goes on.
std::map<uint32_t *, PendingIota>::iterator write_iota(std::map<uint32_t *, PendingIota>::iterator it) {
  if (it->second.sorted) {
    materialize_sort(it->first);
    return t_state->iotas.begin();
  }
  launch_init_index(it->first, it->second.start, it->second.n, it->second.stream);
  return t_state->iotas.erase(it);
}

// ---- lazy fills -----------------------------------------------------------------------------------------
// caller holds the device's DeferLock and has selected the device
void launch_fill(uint8_t *dst, const PendingFill &f) {
  if (f.bytes == 0 || f.sortIdx) return;  // (a sort's marker is not a pattern: materialize_sort)
  mem_note_write(t_state->device, dst, f.bytes);
  const size_t units = f.bytes / static_cast<size_t>(f.unit);
  // a fill whose defining stream is gone is written on the caller's stream (or, from a libmem.so hook, on the null stream)
  const hipStream_t stream = f.streamGone ? (t_callStream.known ? t_callStream.stream : nullptr) : f.stream;
  ARES_LAUNCH("fill_pattern_kernel", fill_pattern_kernel, capped_grid(static_cast<int64_t>((units + kBlock - 1) / kBlock), 256 * 8), kBlock,
              stream, dst, units, f.pattern, f.unit);
  order_before_caller(stream);  // whoever made us write it reads (or overwrites) it next, maybe on another stream
}

// caller holds the device's DeferLock: every lazy fill of the device (r == nullptr) or those that overlap r are
// written now
void materialize_fills(const ByteRange *r, std::vector<hipStream_t> *touched) {
  for (auto it = t_state->fills.begin(); it != t_state->fills.end();) {
    const ByteRange v = range_of(it->first, it->second.bytes);
    if (it->second.sortIdx) {
      // a buffer a lazily defined Sort (+ Reduce) would write: only for somebody who looks at these very bytes
      if (r && v.overlaps(*r)) {
        if (touched) touched->push_back(it->second.stream);
        materialize_sort(it->second.sortIdx);  // (erases the marker)
        it = t_state->fills.begin();
      } else {
        ++it;
      }
    } else if (!r || v.overlaps(*r)) {
      launch_fill(it->first, it->second);
      if (touched) touched->push_back(it->second.stream);
      it = t_state->fills.erase(it);
    } else {
      ++it;
    }
  }
}

// caller holds the device's DeferLock: [r.lo, r.hi) is freed (`gone`) or about to be overwritten.  Lazy fills inside
// it die; one that sticks out at an end is shortened (on a pattern boundary); one that is cut in the middle, or off
// a pattern boundary, is written first.
void retire_fills(const ByteRange &r, bool gone) {
  for (auto it = t_state->fills.begin(); it != t_state->fills.end();) {
    uint8_t *lo = it->first;
    PendingFill f = it->second;
    const uint8_t *hi = lo + f.bytes;
    if (!(lo < r.hi && r.lo < hi)) {
      ++it;
      continue;
    }
    if (f.sortIdx) {  // freed, or overwritten whole: the definition dies; cut: what the sort would leave is written first
      if (gone || (r.lo <= lo && hi <= r.hi)) drop_sort(f.sortIdx);
      else materialize_sort(f.sortIdx);
      it = t_state->fills.begin();
      continue;
    }
    it = t_state->fills.erase(it);
    if (gone || (r.lo <= lo && hi <= r.hi)) continue;
    const bool headCut = r.lo <= lo, tailCut = hi <= r.hi;  // (not both: handled above)
    if (headCut && (static_cast<size_t>(r.hi - lo) % static_cast<size_t>(f.unit)) == 0) {
      f.bytes = static_cast<size_t>(hi - r.hi);
      t_state->fills[const_cast<uint8_t *>(r.hi)] = f;
      it = t_state->fills.upper_bound(const_cast<uint8_t *>(r.hi));
    } else if (tailCut && (static_cast<size_t>(r.lo - lo) % static_cast<size_t>(f.unit)) == 0) {
      f.bytes = static_cast<size_t>(r.lo - lo);
      t_state->fills[lo] = f;
      it = t_state->fills.upper_bound(lo);
    } else {
      launch_fill(lo, f);
      it = t_state->fills.upper_bound(lo);
    }
  }
}

// ---- lazily defined sorts ---------------------------------------------------------------------------------------------
// every buffer a lazily defined Sort (+ Reduce) reads or would write
bool sort_touches(const PendingSort &s, const ByteRange &r) {
  auto hit = [&](const void *p, size_t bytes) {
    const uint8_t *lo = static_cast<const uint8_t *>(p);
    return p && bytes && lo < r.hi && r.lo < lo + bytes;
  };
  const size_t n = static_cast<size_t>(s.length > 0 ? s.length : 0);
  bool any = hit(s.keys.DimValues, dim_vector_bytes(s.keys)) || hit(s.keys.HashValues, 8 * n) || hit(s.keys.IndexVector, 4 * n);
  if (s.reduced)
    any = any || hit(s.outKeys.DimValues, dim_vector_bytes(s.outKeys)) || hit(s.outKeys.IndexVector, 4 * n) ||
          hit(s.inValues, static_cast<size_t>(s.valueBytes) * n) || hit(s.outValues, static_cast<size_t>(s.valueBytes) * n);
  return any;
}

// caller holds the device's DeferLock.  The definition is forgotten: its buffers are freed, redefined or overwritten whole,
// or the work a replay needs is gone.  The marker entries go with it; the index vector's iota entry too (nobody may take
// the vector for an iota any more).
void drop_sort(const uint32_t *indexVector) {
  auto it = t_state->sorts.find(indexVector);
  if (it == t_state->sorts.end()) return;
  t_state->sorts.erase(it);
  auto io = t_state->iotas.find(const_cast<uint32_t *>(indexVector));
  if (io != t_state->iotas.end() && io->second.sorted) t_state->iotas.erase(io);
  for (auto f = t_state->fills.begin(); f != t_state->fills.end();) f = (f->second.sortIdx == indexVector) ? t_state->fills.erase(f) : std::next(f);
  for (auto &kv : t_state->limbo)
    if (kv.second.sortIdx == indexVector) kv.second.sortIdx = nullptr;  // (plain skipped work from now on)
}

// caller holds the device's DeferLock and has selected the device.  Somebody reads (or partly overwrites) what a lazily
// defined Sort — and, once `reduced`, the Reduce that consumed it — would have written: the sequence runs for real, on the
// stream it was defined on: the batch's transforms (pending, or in limbo), the constant measure rows the Reduce consumed,
// InitIndexVector, Sort, Reduce.  Integer aggregates only are ever consumed, so the replayed Reduce rewrites the output's
// dimension and measure rows with the bytes they already hold.  (Rare: the Go host never looks at these vectors.  The sort
// synchronises its stream while the lock is held.)
void materialize_sort(const uint32_t *indexVector) {
  auto it = t_state->sorts.find(indexVector);
  if (it == t_state->sorts.end()) return;
  const PendingSort s = it->second;
  drop_sort(indexVector);  // (the entries go first: nothing below finds them again)
  ReleaseSet released;
  if (s.reduced && s.fromVectors) {
    // (the rows exist: nothing to launch first)
  } else if (s.reduced) {
    auto lim = t_state->limbo.find(s.stream);
    if (lim != t_state->limbo.end()) {
      lim->second.overWait = true;  // the host believes this work is long done
      launch_queue(s.stream, lim->second);
      released.add(s.stream);
      t_state->limbo.erase(lim);
    }
    if (s.constMeasure) {
      PendingFill f = s.fill;
      f.sortIdx = nullptr;
      launch_fill(s.fillAt, f);
    }
  } else {
    auto pq = t_state->pending.find(s.stream);
    if (pq != t_state->pending.end() && pq->second.jobs.count) {
      if (pq->second.overWait) released.add(s.stream);
      launch_queue(s.stream, pq->second);
    }
  }
  launch_init_index(const_cast<uint32_t *>(indexVector), 0, s.length, s.stream);
  sort_keys_now(s.keys, s.length, s.stream);
  if (s.reduced) (void)reduce_now(s.keys, s.inValues, s.outKeys, s.outValues, s.valueBytes, s.length, s.aggFunc, s.stream);
  order_before_caller(s.stream);
  released.run(t_state->device);
}

// [dst, dst + bytes) is defined as `pattern` (unit = 4 or 8 bytes) repeated; false = deferral is off, the caller writes
bool defer_fill(int device, hipStream_t stream, void *dst, size_t bytes, uint64_t pattern, int unit) {
  if (!defer_available() || bytes == 0 || (unit != 4 && unit != 8) || bytes % static_cast<size_t>(unit) ||
      reinterpret_cast<uintptr_t>(dst) % static_cast<uintptr_t>(unit))
    return false;
  drop_skipped_outputs(device, dst, bytes, nullptr, 0);  // what an earlier HashReduce skipped and would write there is dead
  DeferLock lock(device);
  uint8_t *p = static_cast<uint8_t *>(dst);
  const ByteRange r = range_of(p, bytes);
  for (auto &kv : t_state->pending)  // queued transforms that write into the range come first (call order)
    if (kv.second.jobs.count && touches(kv.second.writes, r)) launch_queue(kv.first, kv.second);
  retire_fills(r, false);
  t_state->fills[p] = PendingFill{stream, bytes, pattern, unit, false};
  return true;
}

// a lazy fill that covers exactly [dst, dst + bytes)
bool pending_fill_exact(int device, const void *dst, size_t bytes, uint64_t *pattern, int *unit) {
  if (!defer_available()) return false;
  DeferLock lock(device);
  auto it = t_state->fills.find(const_cast<uint8_t *>(static_cast<const uint8_t *>(dst)));
  if (it == t_state->fills.end() || it->second.bytes != bytes || it->second.sortIdx) return false;
  if (pattern) *pattern = it->second.pattern;
  if (unit) *unit = it->second.unit;
  return true;
}

// a lazy fill that covers rows [prev, length) of a vector of `width`-byte values for some prev: *prev and *pattern
bool pending_fill_tail(int device, const void *base, int width, int length, int *prev, uint64_t *pattern) {
  if (!defer_available() || length <= 0) return false;
  DeferLock lock(device);
  const uint8_t *b = static_cast<const uint8_t *>(base), *end = b + static_cast<size_t>(width) * length;
  auto it = t_state->fills.lower_bound(const_cast<uint8_t *>(b));
  if (it == t_state->fills.end() || it->second.unit != width || it->second.sortIdx) return false;
  if (it->first >= end || it->first + it->second.bytes != end || static_cast<size_t>(it->first - b) % static_cast<size_t>(width)) return false;
  *prev = static_cast<int>(static_cast<size_t>(it->first - b) / static_cast<size_t>(width));
  *pattern = it->second.pattern;
  return true;
}

// [ptr, ptr + bytes) is about to be overwritten by a kernel of the calling entry point
void retire_fills_for_write(int device, const void *ptr, size_t bytes) {
  if (!ptr || bytes == 0 || !defer_available()) return;
  DeferLock lock(device);
  if (t_state->fills.empty()) return;
  retire_fills(range_of(ptr, bytes), false);
}

// [ptr, ptr + bytes) is about to be read by a kernel of the calling entry point
void materialize_fills_for_read(int device, const void *ptr, size_t bytes) {
  if (!ptr || bytes == 0 || !defer_available()) return;
  DeferLock lock(device);
  if (t_state->fills.empty()) return;
  const ByteRange r = range_of(ptr, bytes);
  materialize_fills(&r);
}

// true when `indexVector` is defined as iota(0 .. n) and not written yet (InitIndexVector is lazy); consume: the
// caller has used it as such — from now on only whoever is handed this very vector makes anybody write it
bool virtual_iota_peek(int device, const uint32_t *indexVector, int n, bool consume) {
  if (!defer_available()) return false;
  DeferLock lock(device);
  PendingIota *io = lazy_iota(indexVector, n);
  if (io && consume) io->consumed = true;
  return io != nullptr;
}

// an entry point reads (or rewrites) the buffers of a dimension vector with kernels: lazy fills inside them are written
// first, and so is a lazy iota that a consumer has left behind
void settle_dimension_vector(int device, const DimensionVector &v, bool rowsOnly) {
  if (!defer_available()) return;
  const size_t cap = v.VectorCapacity > 0 ? static_cast<size_t>(v.VectorCapacity) : 0;
  materialize_fills_for_read(device, v.DimValues, dim_vector_bytes(v));
  if (rowsOnly) return;  // (the caller is about to DEFINE the hash and index vector: define_lazy_sort_vectors)
  materialize_fills_for_read(device, v.HashValues, 8 * cap);
  materialize_fills_for_read(device, v.IndexVector, 4 * cap);
  materialize_index_vector(device, v.IndexVector);
}

// an entry point is handed `indexVector` and will read it with a kernel: a lazy iota that a consumer has left behind
// is written now (the unconsumed ones are written by the entry point's flush)
void materialize_index_vector(int device, const uint32_t *indexVector) {
  if (!indexVector || !defer_available()) return;
  DeferLock lock(device);
  auto it = t_state->iotas.find(const_cast<uint32_t *>(indexVector));
  if (it != t_state->iotas.end() && it->second.consumed) write_iota(it);
}

// limboA/limboB: when given, only the skipped work whose outputs overlap these byte ranges is
// launched (the caller reads nothing else); otherwise all of it
// exempt: the index vector whose pending filters the caller is about to extend (a filter call of the hot shape): its
// compaction stays pending
void flush_deferred_impl(int device, const ByteRange *limboA, const ByteRange *limboB, const uint32_t *exempt) {
  // (before the deferral lock: measure rows a table image defines are written by hash_reduce_lds.hip under its own lock)
  if (limboA) grouped_materialize_for_read(device, limboA->lo, static_cast<size_t>(limboA->hi - limboA->lo));
  if (limboB) grouped_materialize_for_read(device, limboB->lo, static_cast<size_t>(limboB->hi - limboB->lo));
  DeferLock lock(device);
  poll_error_words();
  // lazy fills (like work a HashReduce skipped, below) are only written for byte ranges the caller reads: they live in
  // measure / hash vectors, which only Sort, Reduce, HashReduce, Expand, HyperLogLog and copies look at
  if (limboA) materialize_fills(limboA);
  if (limboB) materialize_fills(limboB);
  // scratch frames defined as constant chains likewise: written for the bytes the caller names (their own, or — the caller
  // may be about to rewrite them — their sources), left alone by everybody else
  if (!t_state->frames.empty()) {
    if (limboA) materialize_frames(limboA, true);
    if (limboB) materialize_frames(limboB, true);
  }
  for (auto it = t_state->iotas.begin(); it != t_state->iotas.end();) {
    const ByteRange v = range_of(it->first, 4ull * it->second.n);
    const bool wanted = !it->second.consumed || (limboA && v.overlaps(*limboA)) || (limboB && v.overlaps(*limboB));
    it = wanted ? write_iota(it) : std::next(it);
  }
  // pending compactions: whoever comes next may read the index vector — except where only work that a
  // HashReduce skipped would read it (the previous batch of the query's other stream): that stays
  // dormant with its skipped work and dies with it
  auto dormant = [&](const uint32_t *idx) {
    bool skipped = false, queued = false;
    for (auto &kv : t_state->limbo) skipped = skipped || kv.second.idx == idx;
    for (auto &kv : t_state->pending) queued = queued || (kv.second.jobs.count && kv.second.idx == idx);
    return skipped && !queued;
  };
  for (;;) {
    auto c = t_state->compactions.begin();
    while (c != t_state->compactions.end() && (c->first == exempt || dormant(c->first))) ++c;
    if (c == t_state->compactions.end()) break;
    run_compaction(c->first);
  }
  ReleaseSet released;
  for (auto &kv : t_state->pending) {
    if (kv.second.overWait && kv.second.jobs.count) released.add(kv.first);
    launch_queue(kv.first, kv.second);
  }
  // Work that a HashReduce skipped (limbo) is only launched for byte ranges the caller reads: a full
  // flush from an unrelated call (the next batch's first filter on the query's other stream, say)
  // leaves it alone.
  if (limboA) materialize_limbo(limboA, &released);
  if (limboB) materialize_limbo(limboB, &released);
  released.run(device);
}

void flush_deferred(int device) { flush_deferred_impl(device, nullptr, nullptr); }

void flush_deferred_for_vector(int device, const DimensionVector &v, const void *values, size_t valueBytes) {
  flush_deferred_for_inputs(device, v.DimValues, dim_vector_bytes(v), values, valueBytes);
}

// A HashReduce (or any other writer) is about to overwrite [a, a + aBytes) and [b, b + bBytes): work
// that an earlier HashReduce skipped and whose outputs lie in there must never be launched any more —
// it would overwrite the new results (the Go host ping-pongs its result buffers and alternates two
// streams: batch k's skipped transforms target the buffer batch k+1 reduces into).
void drop_skipped_outputs(int device, const void *a, size_t aBytes, const void *b, size_t bBytes) {
  if (!fuse_available()) return;
  const ByteRange ra = range_of(a, aBytes), rb = range_of(b, bBytes);
  ReleaseSet released;
  {
    DeferLock lock(device);
    for (auto it = t_state->limbo.begin(); it != t_state->limbo.end();)
      it = (touches(it->second.writes, ra) || touches(it->second.writes, rb)) ? drop_limbo(it, &released) : std::next(it);
  }
  released.run(device);
}

// for an entry point that reads exactly [a, a + aBytes) and [b, b + bBytes) of device memory
void flush_deferred_for_inputs(int device, const void *a, size_t aBytes, const void *b, size_t bBytes) {
  const ByteRange ra = range_of(a, aBytes), rb = range_of(b, bBytes);
  flush_deferred_impl(device, &ra, &rb);
}

// ARES_RTC_TRACE (diagnostics): who holds decoded run-length columns when a batch begins — every 16th batch, one line when
// more than 16 are held.  Caller holds the device's DeferLock.
static void trace_decoded_columns_held(const DeferState &st) {
  static int calls = 0;
  if ((++calls & 15) != 0) return;
  size_t inJournals = 0, inCompactions = 0, inPending = 0, inLimbo = 0, expansions = 0;
  for (auto &kv : st.journals) inJournals += kv.second.keep.size();
  for (auto &kv : st.compactions)
    for (auto &filter : kv.second.todo) inCompactions += filter.keep ? 1 : 0;
  for (auto &kv : st.pending) inPending += kv.second.keep.size();
  for (auto &kv : st.limbo) inLimbo += kv.second.keep.size();
  for (auto &kv : st.expansions) expansions += kv.second.size();
  if (inJournals + inCompactions + inPending + inLimbo + expansions <= 16) return;
  char what[200];
  snprintf(what, sizeof(what), "decoded columns held at begin_batch: journals %zu (in %zu), compactions %zu (in %zu), pending %zu, limbo %zu, expansions %zu",
           inJournals, st.journals.size(), inCompactions, st.compactions.size(), inPending, inLimbo, expansions);
  slow_trace(what, 0.0);
}

// InitIndexVector opens a batch on the stream: what the previous batch's HashReduce skipped is dead
// now (the host has swapped its result buffers), and the new index vector starts a filter journal.
void begin_batch(int device, hipStream_t stream, const uint32_t *indexVector, uint32_t start, int n) {
  if (!fuse_available()) return;
  bool release = false;  // (no ReleaseSet: this runs once per batch, and a set's first tag is a heap allocation)
  {
    DeferLock lock(device);
    auto lim = t_state->limbo.find(stream);
    if (lim != t_state->limbo.end()) {  // the skipped work of the previous batch dies, and with it the compaction it would need
      drop_limbo(lim, nullptr);
      release = true;
    }
    if (!t_state->frames.empty()) materialize_frames_of_index(indexVector);  // (frames defined over the vector's old contents)
    t_state->compactions.erase(indexVector);  // the vector is redefined
    t_state->expansions.erase(stream);  // (what still reads a decoded column keeps it alive itself)
    trace_decoded_columns_held(*t_state);
    drop_sort(indexVector);                  // ... and so is whatever a lazily defined Sort meant it to hold
    {  // the stream's filters of the batch that just ended are what the new batch's are predicted from
      FilterHistory &h = t_state->filterHistory[stream];
      if (!h.current.empty()) {  // (the Sort path opens a second index vector per batch: no filters there, nothing to learn)
        h.previous.swap(h.current);
        h.current.clear();
      }
    }
    FilterJournal j;
    j.stream = stream;
    j.start = start;
    j.n0 = n;
    j.valid = true;
    t_state->journals[indexVector] = j;
  }
  if (release) g_releaseHeld(device, hold_tag(stream));
}

// a fast filter has compacted `indexVector` (f == nullptr: something else has — forget the journal)
void journal_filter(int device, const uint32_t *indexVector, const FastOperands *f, uint32_t colRows, int rowsBefore,
                           std::shared_ptr<StreamBuffer> keep) {
  if (!fuse_available()) return;
  DeferLock lock(device);
  auto it = t_state->journals.find(indexVector);
  if (it == t_state->journals.end()) return;
  FilterJournal &j = it->second;
  // (a filter that is not called with what the previous one returned works on something the journal does not describe)
  if (!f || !j.valid || j.filters.size() >= static_cast<size_t>(kFusedFilters) ||
      (j.filters.empty() && rowsBefore != j.n0) || (!j.filters.empty() && j.lastCount >= 0 && rowsBefore != j.lastCount)) {
    j.valid = false;
    return;
  }
  j.lastCount = -1;  // (set by the caller once the count is known)
  FastOperands copy = *f;
  copy.idx = nullptr;
  copy.pad = 0;
  j.filters.push_back(copy);
  j.colRows.push_back(colRows);
  if (keep) j.keep.push_back(std::move(keep));
}

void invalidate_filter_journal(int device, const uint32_t *indexVector) { journal_filter(device, indexVector, nullptr, 0, 0); }

// caller holds the device's DeferLock: the filter that was journalled last kept `count` rows
void journal_count(const uint32_t *indexVector, int count) {
  auto it = t_state->journals.find(indexVector);
  if (it != t_state->journals.end() && it->second.valid) it->second.lastCount = count;
}

bool journal_is_valid(int device, const uint32_t *indexVector) {
  if (!fuse_available()) return false;
  static const bool lazy = [] {
    const char *e = getenv("ARES_LAZY_COMPACT");
    return !(e && e[0] == '0');
  }();
  if (!lazy) return false;
  DeferLock lock(device);
  auto it = t_state->journals.find(indexVector);
  return it != t_state->journals.end() && it->second.valid;
}

// InitIndexVector: remember instead of writing (when the flush hook is in place)
bool defer_iota(int device, hipStream_t stream, uint32_t *indexVector, uint32_t start, int n) {
  if (!defer_available() || n <= 0) return false;
  DeferLock lock(device);
  drop_sort(indexVector);
  t_state->iotas[indexVector] = PendingIota{stream, start, n};
  return true;
}

// true when `indexVector` is a virtual iota(0) of exactly n rows on this device; `take` removes it
// (the caller is about to give the vector real contents)
bool virtual_iota(int device, uint32_t *indexVector, int n, bool take) {
  DeferLock lock(device);
  if (!lazy_iota(indexVector, n)) return false;
  if (take) t_state->iotas.erase(indexVector);
  return true;
}

// the host writes into (or frees) [r.lo, r.hi): decoded copies of run-length columns that lie in there are no longer what a
// NEW call would read.  Caller holds the device's DeferLock.
void forget_run_expansions(const ByteRange &r) {
  for (auto &kv : t_state->expansions) {
    auto &v = kv.second;
    for (size_t i = 0; i < v.size();) {
      const ByteRange src = range_of(v[i].base, v[i].valuesOff + static_cast<size_t>(v[i].step) * v[i].length);
      if (src.overlaps(r)) {
        v[i] = v.back();
        v.pop_back();
      } else {
        i++;
      }
    }
  }
}

// An entry point reads [ptr, ptr + bytes) with a kernel without going through a flush (Reduce over zero dimensions
// keeps everything else lazy): queued transforms that write into the range, and work a HashReduce skipped there, run
// first — in call order, on their own stream (a queue the host has already waited for is synchronised after its late
// launch, the blocks held for it are fenced behind it).
void launch_pending_writers(int device, const void *ptr, size_t bytes) {
  if (!ptr || bytes == 0 || !defer_available()) return;
  grouped_materialize_for_read(device, ptr, bytes);
  const ByteRange r = range_of(ptr, bytes);
  ReleaseSet released;
  {
    DeferLock lock(device);
    for (auto &kv : t_state->pending) {
      if (kv.second.jobs.count == 0 || !touches(kv.second.writes, r)) continue;
      if (kv.second.overWait) released.add(kv.first);
      launch_queue(kv.first, kv.second);
    }
    materialize_limbo(&r, &released);
  }
  released.run(device);
}

// Stable in-place compaction of the index vector and of every RecordID vector by an existing
// predicate vector (keep = byte != 0): the tail of the two-phase filter, for callers that compute
// their predicate elsewhere (geo intersection).
int compact_by_predicate(const uint8_t *pred, uint32_t *indexVector, RecordID **recordIDVectors, int numForeignTables,
                         int n, hipStream_t stream) {
  if (n <= 0) return 0;
  {
    const int device = current_device();
    mem_note_write(device, indexVector, 4ull * static_cast<size_t>(n));
    for (int t = 0; t < numForeignTables; t++) mem_note_write(device, recordIDVectors[t], 8ull * static_cast<size_t>(n));
  }
  const int pad = static_cast<int>(reinterpret_cast<uintptr_t>(pred) & 3);
  const int tiles = pred_tiles(n, pad);
  const int passes = 1 + numForeignTables;
  StreamBuffer wsBuf(CompactSpace::bytes(tiles, passes, 0), stream);
  const CompactSpace cs = clear_compact_space(wsBuf, tiles, passes, 0, stream);
  ARES_LAUNCH("pred_count_kernel", pred_count_kernel, capped_grid(tiles, 256 * 16), kBlock, stream, pred, cs.tileCounts(), pad, n, tiles);
  launch_compaction(cs, pred, indexVector, false, recordIDVectors, pad, n, stream);
  return read_compaction_total(cs, stream);
}


}  // namespace ares

using namespace ares;

extern "C" {

size_t AresStreamEvents(int device, void *stream) {
  size_t n = profiler_stream_events(reinterpret_cast<hipStream_t>(stream));
  if (device < 0 || device >= kMaxDevices) return n;
  DeferLock lock(device);
  for (const ErrorCheck &c : t_state->errorChecks) n += c.stream == reinterpret_cast<hipStream_t>(stream);
  return n;
}

void AresTempStats(size_t *handedOutBytes, size_t *cachedBytes) { temp_stats(handedOutBytes, cachedBytes); }

void AresFlushDeferred(int device) {
  int current = 0;
  if (hipGetDevice(&current) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  try {
    if (current != device) hip_check(hipSetDevice(device), "hipSetDevice");
    flush_deferred(device);
    if (current != device) (void)hipSetDevice(current);
  } catch (std::exception &e) {
    fprintf(stderr, "Exception happened when flushing deferred transforms: %s\n", e.what());
  }
}

}  // extern "C"
