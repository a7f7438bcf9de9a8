// Host batches: the transfer pipeline and the device-resident column cache.
//   AresQueryRunHostBatches  <- the upload of batch k+1 beside the execution of batch k on the query's second stream
//                               (query/aql_processor.go:513-540, :850-881, :1345-1431)
//   AresColumnCache          <- no counterpart: columns kept in HBM under (table, batch, column) keys
#include <condition_variable>
#include <map>
#include <mutex>
#include <thread>

#include "query.hpp"

using namespace ares_host;

struct AresColumnCache {
  AbiLibrary *lib;
  int device;
  size_t budget, bytes = 0;
  uint64_t clock = 0;
  struct Entry {
    void *ptr;
    size_t bytes;
    uint64_t lastUse;
    int pins;
  };
  std::map<uint64_t, Entry> entries;
  std::mutex mu;

  // a resident column (pinned until unpin) or nullptr
  void *find(uint64_t key) {
    std::lock_guard<std::mutex> lock(mu);
    auto it = entries.find(key);
    if (it == entries.end()) return nullptr;
    it->second.lastUse = ++clock;
    it->second.pins++;
    return it->second.ptr;
  }
  // takes ownership of `ptr` (an uploaded column) if the budget allows, evicting the least recently used
  // unpinned entries; returns false when the caller keeps ownership
  bool insert(uint64_t key, void *ptr, size_t n) {
    std::vector<void *> evicted;
    {
      std::lock_guard<std::mutex> lock(mu);
      if (n > budget || entries.count(key)) return false;
      while (bytes + n > budget) {
        auto victim = entries.end();
        for (auto it = entries.begin(); it != entries.end(); ++it)
          if (it->second.pins == 0 && (victim == entries.end() || it->second.lastUse < victim->second.lastUse)) victim = it;
        if (victim == entries.end()) return false;
        bytes -= victim->second.bytes;
        evicted.push_back(victim->second.ptr);
        entries.erase(victim);
      }
      entries[key] = Entry{ptr, n, ++clock, 1};
      bytes += n;
    }
    for (void *p : evicted) check(lib->DeviceFree(p, device));
    return true;
  }
  void unpin(uint64_t key) {
    std::lock_guard<std::mutex> lock(mu);
    auto it = entries.find(key);
    if (it != entries.end() && it->second.pins > 0) it->second.pins--;
  }
};

extern "C" {

AresColumnCache *AresColumnCacheCreate(void *driver, int device, size_t budgetBytes) {
  AresColumnCache *c = new AresColumnCache;
  c->lib = static_cast<AbiLibrary *>(driver);
  c->device = device;
  c->budget = budgetBytes;
  return c;
}

void AresColumnCacheDestroy(AresColumnCache *c) {
  if (!c) return;
  for (auto &kv : c->entries) {
    try {
      check(c->lib->DeviceFree(kv.second.ptr, c->device));
    } catch (...) {
    }
  }
  delete c;
}

int AresQueryRunHostBatches(AresQuery *q, const AresHostColumn *columns, int numColumns, const int *batchSizes, int numBatches,
                            AresColumnCache *cache, uint64_t stats[4], char *err, int errLen) {
  uint64_t uploadedBytes = 0, uploads = 0, hits = 0;
  struct Staged {
    std::vector<VectorPartySlice> slices;
    std::vector<void *> owned;
    std::vector<uint64_t> pinned;
    int size = 0;
  };
  std::string workerError;
  auto run_staged = [&](Staged *b) {  // the executor of one batch, on the stream its transfer used
    try {
      q->ownedColumns = b->owned;
      q->runBatch(b->slices.data(), static_cast<int>(b->slices.size()), b->size, nullptr, 0);
    } catch (std::exception &e) {
      workerError = e.what();
      try {
        q->cleanupBeforeAggregation();
      } catch (...) {
      }
    }
    if (cache)
      for (uint64_t k : b->pinned) cache->unpin(k);
  };
  // ONE executor thread for the whole call (a thread per batch pays for its thread-local state in the library — a mapped pinned
  // result slot from hipHostMalloc among it — on every batch): batches are handed over one at a time
  struct Executor {
    std::mutex mu;
    std::condition_variable cv;
    Staged *job = nullptr;
    bool busy = false, quit = false;
    std::thread thread;
  } ex;
  auto submit = [&](Staged *b) {
    std::lock_guard<std::mutex> lock(ex.mu);
    ex.job = b;
    ex.busy = true;
    ex.cv.notify_all();
  };
  auto wait_idle = [&] {
    std::unique_lock<std::mutex> lock(ex.mu);
    ex.cv.wait(lock, [&] { return !ex.busy; });
  };
  auto stop = [&] {
    {
      std::lock_guard<std::mutex> lock(ex.mu);
      ex.quit = true;
      ex.cv.notify_all();
    }
    if (ex.thread.joinable()) ex.thread.join();
  };
  try {
    Staged prev, cur;
    bool havePrev = false;
    auto start_executor = [&] {  // (on the first batch that is handed over: a query whose columns all sit in the cache never starts it)
      ex.thread = std::thread([&] {
        for (;;) {
          Staged *b = nullptr;
          {
            std::unique_lock<std::mutex> lock(ex.mu);
            ex.cv.wait(lock, [&] { return ex.quit || ex.job; });
            if (!ex.job) return;
            b = ex.job;
            ex.job = nullptr;
          }
          run_staged(b);
          {
            std::lock_guard<std::mutex> lock(ex.mu);
            ex.busy = false;
            ex.cv.notify_all();
          }
        }
      });
    };
    for (int k = 0; k < numBatches; k++) {
      // (query/aql_processor.go:850-881) async transfer of batch k ...
      void *xfer = havePrev && q->otherStream ? q->otherStream : q->stream;
      cur = Staged();
      cur.size = batchSizes[k];
      // columns the cache holds first: a batch that needs no upload has nothing to overlap with — batch k-1 then runs on
      // THIS thread (handing it to the executor and waking up again costs ~0.1 ms per batch of condition-variable latency)
      std::vector<void *> devs(static_cast<size_t>(numColumns), nullptr);
      int misses = 0;
      for (int c = 0; c < numColumns; c++) {
        const AresHostColumn &hc = columns[static_cast<size_t>(k) * numColumns + c];
        devs[c] = (cache && hc.cacheKey) ? cache->find(hc.cacheKey) : nullptr;
        if (devs[c]) {
          hits++;
          cur.pinned.push_back(hc.cacheKey);
        } else {
          misses++;
        }
      }
      const bool handOver = havePrev && misses > 0;
      if (handOver) {
        if (!ex.thread.joinable()) start_executor();
        submit(&prev);  // ... while batch k-1 executes
      }
      try {
        for (int c = 0; c < numColumns; c++) {
          const AresHostColumn &hc = columns[static_cast<size_t>(k) * numColumns + c];
          void *dev = devs[c];
          if (!dev) {
            dev = reinterpret_cast<void *>(check(q->lib->DeviceAllocate(hc.bytes ? hc.bytes : 1, q->device)));
            check(q->lib->AsyncCopyHostToDevice(dev, const_cast<void *>(hc.host), hc.bytes, xfer, q->device));
            uploadedBytes += hc.bytes;
            uploads++;
            if (cache && hc.cacheKey && cache->insert(hc.cacheKey, dev, hc.bytes)) cur.pinned.push_back(hc.cacheKey);
            else cur.owned.push_back(dev);
          }
          VectorPartySlice vp = hc.slice;
          vp.BasePtr = static_cast<uint8_t *>(dev) + reinterpret_cast<uintptr_t>(hc.slice.BasePtr);
          cur.slices.push_back(vp);
        }
        if (misses > 0) check(q->lib->WaitForCudaStream(xfer, q->device));  // wait for the data transfer of the current batch
      } catch (...) {
        if (handOver) wait_idle();
        stop();
        throw;
      }
      if (handOver) wait_idle();
      else if (havePrev) run_staged(&prev);
      if (!workerError.empty()) throw AbiError(workerError);
      prev = cur;
      havePrev = true;
    }
    if (havePrev) run_staged(&prev);  // (nothing left to overlap with)
    stop();
    if (!workerError.empty()) throw AbiError(workerError);
    if (stats) {
      stats[0] = uploadedBytes;
      stats[1] = uploads;
      stats[2] = hits;
      stats[3] = cache ? cache->bytes : 0;
    }
    return 0;
  } catch (std::exception &e) {
    stop();
    set_err(err, errLen, e.what());
    return -1;
  }
}

}  // extern "C"
