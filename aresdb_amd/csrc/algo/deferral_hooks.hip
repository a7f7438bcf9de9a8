// What libmem.so calls (registered by defer_available, deferral.hip): stream waits, frees, copies, writes, trims and stream
// destruction, each settling the deferred state a host action touches (invariants I1 - I4 of deferral.hpp).  Hooks run on
// libmem.so's threads and never throw.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "ares_extensions.h"

#include "deferral.hpp"
#include "hash_reduce_lds.hpp"
#include "sort_reduce_fused.hpp"

namespace ares {

namespace {
// the index vector itself (its first n0 entries) or a column one of the journalled filters read
bool journal_touched(const uint32_t *indexVector, const FilterJournal &j, const ByteRange &r) {
  bool hit = range_of(indexVector, 4ull * (j.n0 > 0 ? j.n0 : 1)).overlaps(r);
  for (size_t k = 0; k < j.filters.size(); k++) hit = hit || column_overlaps(j.filters[k], j.colRows[k], r);
  return hit;
}

struct DeviceGuard {  // hooks run on libmem.so's threads: select the device, restore it afterwards
  int previous = -1;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&previous) != hipSuccess) previous = -1;
    if (previous != device) (void)hipSetDevice(device);
  }
  ~DeviceGuard() {
    if (previous >= 0) (void)hipSetDevice(previous);
  }
};

}  // namespace

// WaitForCudaStream: a queue whose results only a HashReduce on the same stream will consume may stay
void hook_on_wait(int device, void *streamPtr) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(streamPtr);
  try {
    DeviceGuard guard(device);
    DeferLock lock(device);
    // a wait on one stream says nothing about the others: their pending work is left alone
    for (auto it = t_state->iotas.begin(); it != t_state->iotas.end();) {
      it = (it->second.stream == stream && !it->second.consumed) ? write_iota(it) : std::next(it);  // (not consumed: no Sort over it)
    }
    for (auto &kv : t_state->frames)  // a frame nobody has read stays defined: its sources are inputs of pending work from now on
      if (kv.second.stream == stream) kv.second.overWait = true;
    for (auto &kv : t_state->pending) {
      if (kv.first != stream || kv.second.jobs.count == 0 || kv.second.overWait) continue;
      PendingQueue &q = kv.second;
      bool keep = g_fuseEnabled;  // nobody will consume the queue otherwise
      if (keep && q.idx) {  // the survivors must be re-derivable from the filter journal
        auto j = t_state->journals.find(q.idx);
        keep = j != t_state->journals.end() && j->second.valid && j->second.stream == stream && j->second.start == 0;
        if (keep)  // the filters' columns are inputs of the pending work from now on
          for (size_t k = 0; k < j->second.filters.size(); k++)
            column_ranges(j->second.filters[k], j->second.colRows[k], [&](const ByteRange &c) { q.reads.push_back(c); });
      }
      if (keep)
        q.overWait = true;
      else
        launch_queue(kv.first, q);
    }
  } catch (std::exception &e) {
    fprintf(stderr, "Exception happened when handling a stream wait: %s\n", e.what());
  }
}

// DeviceFree: nonzero = keep the block aside on behalf of that stream's pending (or skipped) work,
// which still reads it (the value is the tag AresMemReleaseHeld will be called with)
uintptr_t hook_on_free(int device, void *ptr, size_t bytes) {
  const ByteRange r = range_of(ptr, bytes);
  grouped_note_gone(device, ptr, bytes);
  scan_ahead_note_touch(device, ptr, bytes, /*freed=*/true);
  uintptr_t hold = 0;
  ReleaseSet released;
  try {
    DeviceGuard guard(device);
    DeferLock lock(device);
    for (auto it = t_state->sorts.begin(); it != t_state->sorts.end();) {  // a buffer a lazily defined Sort (+ Reduce) works on goes
      if (sort_touches(it->second, r)) {
        drop_sort(it->first);
        it = t_state->sorts.begin();
      } else {
        ++it;
      }
    }
    erase_if(t_state->iotas, [&](auto &io) { return range_of(io.first, 4ull * io.second.n).overlaps(r); });  // an index vector nobody has read yet
    retire_fills(r, true);  // lazy fills of the block die unwritten
    // scratch frames defined as constant chains: a frame of the block dies unwritten; one that READS the block is treated like
    // a queued job that does — the block is held where the host has waited for the stream, the frame is written now otherwise
    for (auto it = t_state->frames.begin(); it != t_state->frames.end();) {
      FrameDef &d = it->second;
      if (frame_writes_touch(d, r)) {
        const hipStream_t s = d.stream;
        const bool held = d.held;
        it = t_state->frames.erase(it);
        bool others = t_state->limbo.count(s) != 0;
        for (auto &kv : t_state->frames) others = others || kv.second.stream == s;
        auto pq = t_state->pending.find(s);
        others = others || (pq != t_state->pending.end() && pq->second.jobs.count);
        if (held && !others) released.add(s);  // (nothing else of the stream can still read what was held for it)
      } else if (frame_reads_touch(d, r)) {
        if (d.overWait) {
          hold = hold_tag(d.stream);
          d.held = true;
          ++it;
        } else {
          released.add(d.stream);
          materialize_frame(it);
          it = t_state->frames.begin();
        }
      } else {
        ++it;
      }
    }
    forget_run_expansions(r);
    // a journal dies with its index vector or with a column its filters read — unless a queue the
    // host has already waited for still refers to it (then the block is held below, contents intact)
    erase_if(t_state->journals, [&](auto &j) {
      bool kept = false;
      for (auto &kv : t_state->pending) kept = kept || (kv.second.jobs.count && kv.second.overWait && kv.second.idx == j.first);
      return !kept && journal_touched(j.first, j.second, r);
    });
    for (auto &kv : t_state->pending) {
      if (kv.second.jobs.count == 0) continue;
      if (touches(kv.second.writes, r)) {
        released.add(kv.first);
        launch_queue(kv.first, kv.second);  // an output is freed: run the work, the fence follows it
      } else if (touches(kv.second.reads, r)) {
        if (kv.second.overWait) {
          hold = hold_tag(kv.first);
        } else {  // not even waited for: run it now, the free is fenced behind it
          released.add(kv.first);
          launch_queue(kv.first, kv.second);
        }
      }
    }
    for (auto it = t_state->compactions.begin(); it != t_state->compactions.end();) {
      if (!compaction_touches(it->second, r)) {
        ++it;
        continue;
      }
      // the index or predicate vector of a pending compaction is freed
      const uint32_t *key = it->first;
      const hipStream_t owner = it->second.stream;
      bool waited = false, queued = false, skipped = false;
      for (auto &kv : t_state->pending)
        if (kv.second.jobs.count && kv.second.idx == key) (kv.second.overWait ? waited : queued) = true;
      for (auto &kv : t_state->limbo) skipped = skipped || kv.second.idx == key;
      if (waited || skipped) {  // still needed if that work is launched after all: keep the block intact
        hold = hold_tag(owner);
        ++it;
      } else if (queued) {  // transforms the host has not even waited for: run everything now
        for (auto &kv : t_state->pending)
          if (kv.second.jobs.count && kv.second.idx == key) {
            released.add(kv.first);
            launch_queue(kv.first, kv.second);
          }
        it = t_state->compactions.begin();  // (launch_queue erased the entry)
      } else if (range_of(it->second.idx, 4ull * (it->second.todo.empty() ? it->second.n : it->second.n0)).overlaps(r)) {
        it = t_state->compactions.erase(it);  // the index vector itself goes: nobody will read the compacted vector
      } else {
        // only the predicate vector goes, the index vector stays live (a later transform, filter or
        // copy may read it): compact now — the free is fenced behind the launch
        run_compaction(key);
        it = t_state->compactions.begin();
      }
    }
    for (auto it = t_state->limbo.begin(); it != t_state->limbo.end();) {
      if (touches(it->second.writes, r)) {  // the skipped outputs die unseen
        it = drop_limbo(it, &released);
      } else {
        if (touches(it->second.reads, r)) hold = hold_tag(it->first);
        ++it;
      }
    }
  } catch (std::exception &e) {
    fprintf(stderr, "Exception happened when handling a device free: %s\n", e.what());
  }
  released.run(device);
  return hold;
}

// a copy is about to touch [ptr, ptr + bytes)
void hook_on_access(int device, const void *ptr, size_t bytes) {
  const ByteRange r = range_of(ptr, bytes);
  ReleaseSet released;
  try {
    DeviceGuard guard(device);
    grouped_materialize_for_read(device, ptr, bytes);  // (measure rows a table image defines)
    DeferLock lock(device);
    for (auto it = t_state->iotas.begin(); it != t_state->iotas.end();) {
      const ByteRange v = range_of(it->first, 4ull * it->second.n);
      if (v.overlaps(r)) {
        t_syncAfterUnlock.push_back(it->second.stream);  // (the copy may run on another stream)
        it = write_iota(it);
      } else {
        ++it;
      }
    }
    for (auto &kv : t_state->pending) {
      if (kv.second.jobs.count == 0) continue;
      if (touches(kv.second.writes, r) || touches(kv.second.reads, r)) {
        released.add(kv.first);
        launch_queue(kv.first, kv.second);
      }
    }
    // a scratch frame defined as a constant chain: the copy reads it, or writes into it or into what it is made from
    if (!t_state->frames.empty()) materialize_frames(&r, /*readsToo=*/true);
    forget_run_expansions(r);  // (a copy INTO a run-length column: later calls decode it again)
    materialize_fills(&r, &t_syncAfterUnlock);  // (the copy may run on another stream: wait for the fill)
    materialize_limbo(&r, &released);
    for (auto it = t_state->compactions.begin(); it != t_state->compactions.end();) {
      if (compaction_touches(it->second, r)) {
        const hipStream_t cs = it->second.stream;
        run_compaction(it->first);
        t_syncAfterUnlock.push_back(cs);
        it = t_state->compactions.begin();
      } else {
        ++it;
      }
    }
    // a copy into an index vector or into a column a journalled filter has read: the survivors can
    // no longer be re-derived (queues that depended on the journal were launched above)
    erase_if(t_state->journals, [&](auto &j) { return journal_touched(j.first, j.second, r); });
    scan_ahead_note_touch(device, ptr, bytes, /*freed=*/false);  // ... and a scan launched ahead of its HashReduce has read what is no longer there
  } catch (std::exception &e) {
    fprintf(stderr, "Exception happened when handling a device copy: %s\n", e.what());
  }
  released.run(device);
}

void hook_on_write(int device, const void *ptr, size_t bytes) { grouped_note_write(device, ptr, bytes); }

void hook_trim(int device) {
  try {
    DeviceGuard guard(device);
    stream_cache_trim(device);
    grouped_trim(device);
  } catch (std::exception &) {
  }
}

// DestroyCudaStream (the stream has been flushed and synchronised): nothing may outlive the handle —
// a later stream can get the same address
void hook_on_stream_destroy(int device, void *streamPtr) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(streamPtr);
  try {
    DeviceGuard guard(device);
    {
      DeferLock lock(device);
      for (auto it = t_state->sorts.begin(); it != t_state->sorts.end();) {
        if (it->second.stream == stream) {
          drop_sort(it->first);
          it = t_state->sorts.begin();
        } else {
          ++it;
        }
      }
      t_state->pending.erase(stream);
      erase_if(t_state->frames, [&](auto &kv) { return kv.second.stream == stream; });
      t_state->expansions.erase(stream);
      scan_ahead_stream_gone(device, stream);  // (the stream's hint, and the regions of a scan launched from it)
      auto lim = t_state->limbo.find(stream);
      if (lim != t_state->limbo.end()) drop_limbo(lim, nullptr);  // (the stream's tag is released below, whatever was held under it)
      auto ofStream = [&](auto &kv) { return kv.second.stream == stream; };
      erase_if(t_state->journals, ofStream);
      erase_if(t_state->compactions, ofStream);
      erase_if(t_state->iotas, ofStream);
      t_state->filterHistory.erase(stream);
      // lazy fills that were defined on this stream and are still unwritten: from now on they are written on the stream
      // of whoever needs them (the null stream stands for "the caller's", see launch_fill)
      for (auto &kv : t_state->fills)
        if (kv.second.stream == stream) kv.second.streamGone = true;
      // error words of this stream's lazy compactions: the stream is idle, their copies have landed; the events go now
      for (size_t i = 0; i < t_state->errorChecks.size();) {
        if (t_state->errorChecks[i].stream == stream) t_state->errorSeen = retire_error_check(i) || t_state->errorSeen;
        else i++;
      }
    }
    profiler_stream_gone(stream);
    if (g_releaseHeld) g_releaseHeld(device, hold_tag(stream));
    stream_cache_purge(device, stream);
  } catch (std::exception &e) {
    fprintf(stderr, "Exception happened when handling a stream destruction: %s\n", e.what());
  }
}

}  // namespace ares
