// Shards across devices: the communicators and the merges of the per-shard group tables.
//   AresQueryMergeShards  <- "previous results + re-reduce" (query/aql_batchexecutor.go:236-251) with the aggregate's own
//                            combine rule (broker/result_merge.go:77-104)
//   AresCommCreateLocal   <- one device per shard inside the server process (query/device_manager.go:185-218)
// What travels is a block: a dimension vector whose capacity is the block's row count, then the rows' measures.  Blocks are
// packed from and appended to the query's result with the one mirror of asyncCopyDimensionVector (plan.hpp).
#include <atomic>
#include <condition_variable>
#include <mutex>

#include "query.hpp"

using namespace ares_host;

struct AresComm {
  int rank = 0, nranks = 1;
  AresAllGatherFn allGather = nullptr;
  void *user = nullptr;
  // RCCL binding (AresCommCreateRccl)
  void *rcclHandle = nullptr, *rcclComm = nullptr;
  int (*ncclAllGather)(const void *, void *, size_t, int, void *, void *) = nullptr;
  int (*ncclSend)(const void *, size_t, int, int, void *, void *) = nullptr;
  int (*ncclRecv)(void *, size_t, int, int, void *, void *) = nullptr;
  int (*ncclGroupStart)() = nullptr;
  int (*ncclGroupEnd)() = nullptr;
  AresAllToAllFn allToAll = nullptr;  // optional: without it blocks travel by padded all-gathers
  void *localRank = nullptr;          // AresCommCreateLocal: this rank's end of the in-process rendezvous
  int (*ncclCommDestroy)(void *) = nullptr;
  const char *(*ncclGetErrorString)(int) = nullptr;
};

namespace {
struct NcclUniqueId { char internal[128]; };

int rccl_all_gather(void *user, const void *send, void *recv, size_t bytesPerRank, void *stream) {
  AresComm *c = static_cast<AresComm *>(user);
  return c->ncclAllGather(send, recv, bytesPerRank, /*ncclUint8*/ 1, c->rcclComm, stream);
}

// all-to-all of byte blocks over RCCL: one grouped send / receive pair per peer
int rccl_all_to_all(void *user, const void *send, const size_t *sendBytes, const size_t *sendOffsets, void *recv,
                    const size_t *recvBytes, const size_t *recvOffsets, void *stream) {
  AresComm *c = static_cast<AresComm *>(user);
  int rc = c->ncclGroupStart();
  for (int r = 0; r < c->nranks && rc == 0; r++) {
    if (sendBytes[r]) rc = c->ncclSend(static_cast<const uint8_t *>(send) + sendOffsets[r], sendBytes[r], /*ncclUint8*/ 1, r, c->rcclComm, stream);
    if (rc == 0 && recvBytes[r]) rc = c->ncclRecv(static_cast<uint8_t *>(recv) + recvOffsets[r], recvBytes[r], 1, r, c->rcclComm, stream);
  }
  const int end = c->ncclGroupEnd();
  return rc ? rc : end;
}

void *open_rccl(std::string *why) {
  for (const char *name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
    if (void *h = dlopen(name, RTLD_NOW | RTLD_LOCAL)) return h;
  }
  *why = std::string("cannot load librccl.so: ") + dlerror();
  return nullptr;
}

bool select_device(int device, std::string *why) {
  void *hip = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
  auto set = hip ? reinterpret_cast<int (*)(int)>(dlsym(hip, "hipSetDevice")) : nullptr;
  if (!set || set(device) != 0) {
    *why = "hipSetDevice failed";
    return false;
  }
  return true;
}

// all_gather of `bytes` host bytes per rank through device staging buffers of the query's allocator
void gather_words(AresQuery *q, AresComm *c, const void *mine, void *all, size_t bytes) {
  uint8_t *send = q->alloc(bytes), *recv = q->alloc(bytes * c->nranks);
  check(q->lib->AsyncCopyHostToDevice(send, const_cast<void *>(mine), bytes, q->stream, q->device));
  q->lib->noteWrite(q->device, recv, bytes * c->nranks);
  if (c->allGather(c->user, send, recv, bytes, q->stream) != 0) throw AbiError("all-gather of the partial sizes failed");
  q->d2h(all, recv, bytes * c->nranks);
  q->wait();
  q->release(send);
  q->release(recv);
}

// rows [fromRow, fromRow + rows) of the query's result into the block at `block`, whose capacity is `capacity` rows
void pack_block(AresQuery *q, uint8_t *block, int64_t capacity, int64_t rows, int64_t fromRow, int mb) {
  q->copyDimsD2D(block, q->dimVec[0], rows, 0, capacity, q->resultCapacity, fromRow);
  q->d2d(block + capacity * q->layout.rowBytes, q->measureVec[0] + fromRow * mb, static_cast<size_t>(rows) * mb);
}
// the block's `rows` rows behind row `toRow` of dimension vector [0], their measures to `measures`
void append_block(AresQuery *q, uint8_t *block, int64_t capacity, int64_t rows, int64_t toRow, uint8_t *measures, int mb) {
  q->copyDimsD2D(q->dimVec[0], block, rows, toRow, q->resultCapacity, capacity);
  q->d2d(measures, block + capacity * q->layout.rowBytes, static_cast<size_t>(rows) * mb);
}
}  // namespace

extern "C" {

AresComm *AresCommCreate(int rank, int nranks, AresAllGatherFn allGather, void *user) {
  if (!allGather || nranks < 1 || rank < 0 || rank >= nranks) return nullptr;
  AresComm *c = new AresComm;
  c->rank = rank;
  c->nranks = nranks;
  c->allGather = allGather;
  c->user = user;
  return c;
}

int AresCommRcclUniqueId(uint8_t id[128], char *err, int errLen) {
  std::string why;
  void *h = open_rccl(&why);
  auto get = h ? reinterpret_cast<int (*)(NcclUniqueId *)>(dlsym(h, "ncclGetUniqueId")) : nullptr;
  NcclUniqueId u;
  if (!get || get(&u) != 0) {
    set_err(err, errLen, h ? "ncclGetUniqueId failed" : why.c_str());
    return -1;
  }
  memcpy(id, u.internal, 128);
  return 0;
}

AresComm *AresCommCreateRccl(const uint8_t id[128], int rank, int nranks, int device, char *err, int errLen) {
  std::string why;
  void *h = open_rccl(&why);
  if (!h || !select_device(device, &why)) {
    set_err(err, errLen, why.c_str());
    return nullptr;
  }
  auto init = reinterpret_cast<int (*)(void **, int, NcclUniqueId, int)>(dlsym(h, "ncclCommInitRank"));
  AresComm *c = new AresComm;
  c->rank = rank;
  c->nranks = nranks;
  c->rcclHandle = h;
  c->ncclAllGather = reinterpret_cast<decltype(c->ncclAllGather)>(dlsym(h, "ncclAllGather"));
  c->ncclCommDestroy = reinterpret_cast<decltype(c->ncclCommDestroy)>(dlsym(h, "ncclCommDestroy"));
  c->ncclGetErrorString = reinterpret_cast<decltype(c->ncclGetErrorString)>(dlsym(h, "ncclGetErrorString"));
  NcclUniqueId u;
  memcpy(u.internal, id, 128);
  int rc = -1;
  if (!init || !c->ncclAllGather || !c->ncclCommDestroy || (rc = init(&c->rcclComm, nranks, u, rank)) != 0) {
    set_err(err, errLen, (std::string("ncclCommInitRank failed: ") +
                          (c->ncclGetErrorString && rc > 0 ? c->ncclGetErrorString(rc) : "missing symbol")).c_str());
    delete c;
    return nullptr;
  }
  c->allGather = &rccl_all_gather;
  c->user = c;
  c->ncclSend = reinterpret_cast<decltype(c->ncclSend)>(dlsym(h, "ncclSend"));
  c->ncclRecv = reinterpret_cast<decltype(c->ncclRecv)>(dlsym(h, "ncclRecv"));
  c->ncclGroupStart = reinterpret_cast<decltype(c->ncclGroupStart)>(dlsym(h, "ncclGroupStart"));
  c->ncclGroupEnd = reinterpret_cast<decltype(c->ncclGroupEnd)>(dlsym(h, "ncclGroupEnd"));
  if (c->ncclSend && c->ncclRecv && c->ncclGroupStart && c->ncclGroupEnd) c->allToAll = &rccl_all_to_all;
  return c;
}

}  // extern "C"

// ---- ranks as threads of ONE process: the reference's process model (one device_manager device per shard inside
// the server process, query/device_manager.go:185-218) ---------------------------------------------------------
// The ranks rendezvous in host memory; a rank copies every peer's block itself — hipMemcpyAsync (peer-to-peer
// over xGMI through unified addressing) on its own stream for device memory, memcpy for host memory.
namespace {
struct LocalHub {
  std::mutex m;
  std::condition_variable cv;
  int nranks = 0, arrived = 0, refs = 0;
  uint64_t phase = 0;
  std::vector<const void *> send;
  int (*copyAsync)(void *, const void *, size_t, int, void *) = nullptr;  // hipMemcpyAsync(dst, src, n, hipMemcpyDefault, stream)
  int (*streamSync)(void *) = nullptr;
  // a rank that failed inside a collective says so here: every rank passes both barriers of the collective whatever
  // happened to it (a rank that left early would leave the others waiting forever) and returns non-zero when any failed
  std::atomic<int> failed{0};
  void barrier() {
    std::unique_lock<std::mutex> lock(m);
    const uint64_t my = phase;
    if (++arrived == nranks) {
      arrived = 0;
      phase++;
      cv.notify_all();
    } else {
      cv.wait(lock, [&] { return phase != my; });
    }
  }
};
struct LocalRank {
  LocalHub *hub;
  int rank;
};

int local_all_gather(void *user, const void *send, void *recv, size_t bytesPerRank, void *stream) {
  LocalRank *me = static_cast<LocalRank *>(user);
  LocalHub *h = me->hub;
  int rc = 0;
  if (h->streamSync && h->streamSync(stream) != 0) rc = 1;  // what this rank contributes has been produced
  if (rc) h->failed.store(1);
  h->send[me->rank] = send;
  h->barrier();
  const bool go = h->failed.load() == 0;  // (written before the barrier every rank has passed)
  for (int r = 0; r < h->nranks && rc == 0 && go; r++) {
    uint8_t *dst = static_cast<uint8_t *>(recv) + bytesPerRank * r;
    if (h->copyAsync) rc = h->copyAsync(dst, h->send[r], bytesPerRank, /*hipMemcpyDefault*/ 4, stream);
    else memcpy(dst, h->send[r], bytesPerRank);
  }
  if (rc == 0 && go && h->streamSync) rc = h->streamSync(stream);  // nobody frees a block a peer is still reading
  if (rc) h->failed.store(1);
  h->barrier();
  return (rc || h->failed.load()) ? 1 : 0;  // sticky: a communicator that failed once stays failed
}
}  // namespace

extern "C" {

int AresCommCreateLocal(int nranks, int deviceMemory, AresComm **out, char *err, int errLen) {
  if (nranks < 1 || !out) {
    set_err(err, errLen, "AresCommCreateLocal: bad arguments");
    return -1;
  }
  LocalHub *hub = new LocalHub;
  hub->nranks = nranks;
  hub->refs = nranks;
  hub->send.assign(nranks, nullptr);
  if (deviceMemory) {
    void *hip = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
    hub->copyAsync = hip ? reinterpret_cast<decltype(hub->copyAsync)>(dlsym(hip, "hipMemcpyAsync")) : nullptr;
    hub->streamSync = hip ? reinterpret_cast<decltype(hub->streamSync)>(dlsym(hip, "hipStreamSynchronize")) : nullptr;
    if (!hub->copyAsync || !hub->streamSync) {
      delete hub;
      set_err(err, errLen, "AresCommCreateLocal: cannot bind hipMemcpyAsync / hipStreamSynchronize");
      return -1;
    }
  }
  for (int r = 0; r < nranks; r++) {
    AresComm *c = new AresComm;
    c->rank = r;
    c->nranks = nranks;
    c->allGather = &local_all_gather;
    c->user = new LocalRank{hub, r};
    c->localRank = c->user;
    out[r] = c;
  }
  return 0;
}

void AresCommSetAllToAll(AresComm *c, AresAllToAllFn allToAll) {
  if (c) c->allToAll = allToAll;
}

void AresCommDestroy(AresComm *c) {
  if (!c) return;
  if (c->rcclComm && c->ncclCommDestroy) c->ncclCommDestroy(c->rcclComm);
  if (c->localRank) {
    LocalRank *lr = static_cast<LocalRank *>(c->localRank);
    bool last;
    {
      std::lock_guard<std::mutex> lock(lr->hub->m);
      last = --lr->hub->refs == 0;
    }
    if (last) delete lr->hub;
    delete lr;
  }
  delete c;
}

// HyperLogLog shard merge.  A shard that has NOT been finalised (every batch ran with isLastBatch = 0) holds its
// state as entries (dimension row, value = rho << 16 | register), one per (group, register) it has seen, in
// rows [0, resultSize) of dimension / measure vector [0].  The ranks exchange those entries in one all-gather;
// every rank then feeds the OTHER ranks' entries to the library's own HyperLogLog call as one more batch — with
// isLastBatch = 1 — behind its own state: the call keeps the maximum rho per (group, register), which is the
// register-max merge of the broker (broker/result_merge.go:95-104, query/common/hll.go:148), and encodes the
// final dense / sparse vector.  Every rank ends with the same set of (group, register) entries and therefore the same
// encoded registers per group; the ORDER of the groups in the result is rank dependent (a rank's own groups come first).
static int merge_shards_hll(AresQuery *q, AresComm *c) {
  // precondition, agreed on by every rank before anybody leaves: a rank that threw ahead of the first collective would
  // leave the others waiting in it
  const bool unfit = q->isLastBatch || q->hllVector;
  const int world = c->nranks, mb = 4;
  std::vector<int64_t> sizes(world, 0);
  const int64_t mine = q->resultSize;
  {
    std::vector<int64_t> pairs(2 * static_cast<size_t>(world), 0);
    const int64_t me[2] = {mine, unfit ? 1 : 0};
    gather_words(q, c, me, pairs.data(), 2 * sizeof(int64_t));
    bool anyUnfit = false;
    for (int r = 0; r < world; r++) {
      sizes[r] = pairs[2 * r];
      anyUnfit = anyUnfit || pairs[2 * r + 1] != 0;
    }
    if (anyUnfit)
      throw AbiError(unfit ? "HyperLogLog shard merge needs the shard's intermediate entries: run every batch with isLastBatch = 0, the merge finalises"
                           : "HyperLogLog shard merge: another rank's shard was already finalised (isLastBatch = 1 before the merge)");
  }
  int64_t gmax = 1, others = 0;
  for (int r = 0; r < world; r++) {
    gmax = std::max(gmax, sizes[r]);
    if (r != c->rank) others += sizes[r];
  }
  if (others + mine > INT32_MAX) throw AbiError("merged result exceeds 2^31 rows");
  const size_t packedBytes = static_cast<size_t>(gmax * (q->layout.rowBytes + mb));
  uint8_t *packed = q->alloc(packedBytes), *gathered = q->alloc(packedBytes * world);
  pack_block(q, packed, gmax, mine, 0, mb);
  q->lib->noteWrite(q->device, gathered, packedBytes * world);
  if (c->allGather(c->user, packed, gathered, packedBytes, q->stream) != 0) throw AbiError("all-gather of the HyperLogLog entries failed");
  q->wait();
  // the other ranks' entries are this rank's last batch: rows [resultSize, resultSize + others) of dimension vector [0],
  // their values in measure vector [1] (where a batch's hll values go, query/time_series_aggregate.go:404-408)
  q->size = static_cast<int>(others);
  q->prepareForDimAndMeasureEval();
  int64_t base = 0;
  for (int r = 0; r < world; r++) {
    if (r == c->rank) continue;
    append_block(q, gathered + packedBytes * r, gmax, sizes[r], q->resultSize + base, q->measureVec[1] + base * mb, mb);
    base += sizes[r];
  }
  q->wait();
  q->release(packed);
  q->release(gathered);
  q->isLastBatch = true;
  q->reduce();
  q->postExec();
  return 0;
}

int AresQueryMergeShards(AresQuery *q, AresComm *c, char *err, int errLen) {
  try {
    if (!c || !c->allGather) throw AbiError("no communicator");
    if (q->plan.isHLL()) return merge_shards_hll(q, c);
    const int mb = q->plan.measureBytes(), world = c->nranks;
    // 1. sizes
    std::vector<int64_t> sizes(world, 0);
    const int64_t mine = q->resultSize;
    gather_words(q, c, &mine, sizes.data(), sizeof(int64_t));
    int64_t gmax = 1, total = 0;
    for (int64_t sz : sizes) {
      gmax = std::max(gmax, sz);
      total += sz;
    }
    if (total > INT32_MAX) throw AbiError("merged result exceeds 2^31 rows");
    // 2. this rank's partial as one block of capacity gmax
    const size_t packedBytes = static_cast<size_t>(gmax * (q->layout.rowBytes + mb));
    uint8_t *packed = q->alloc(packedBytes), *gathered = q->alloc(packedBytes * world);
    pack_block(q, packed, gmax, mine, 0, mb);
    // 3. one exchange
    q->lib->noteWrite(q->device, gathered, packedBytes * world);
    if (c->allGather(c->user, packed, gathered, packedBytes, q->stream) != 0) throw AbiError("all-gather of the partial group tables failed");
    // 4. append every rank's partial into fresh result vectors and re-reduce
    q->wait();
    q->releaseAll();
    q->resultSize = 0;
    q->size = static_cast<int>(total);
    q->prepareForDimAndMeasureEval();  // capacity total + 12.5 %, both buffers of every vector
    int64_t base = 0;
    for (int r = 0; r < world; r++) {
      append_block(q, gathered + packedBytes * r, gmax, sizes[r], base, q->measureVec[0] + base * mb, mb);
      base += sizes[r];
    }
    q->wait();
    q->release(packed);
    q->release(gathered);
    if (total > 0) {
      q->reduce();  // HashReduce or InitIndexVector + Sort + Reduce over rows [0, size) of vector [0] into [1]
      q->postExec();
    } else {
      q->size = 0;
    }
    return 0;
  } catch (std::exception &e) {
    set_err(err, errLen, e.what());
    return -1;
  }
}

// Option (B) of SURVEY.md 8e: every rank ends with the groups whose 64-bit row hash falls into its share
// of the hash range, so no rank ever holds the whole table.  Built from the library's own entry points:
// Sort gives the row hashes and the order, Reduce lays the table out in that order (a shard's rows are
// distinct, so it only gathers), the slice for rank r is then contiguous; blocks travel by one
// all-to-all (or padded all-gathers when the communicator has none) and the receiver re-reduces what
// arrived with the query's own reduction.
int AresQueryMergeShardsPartitioned(AresQuery *q, AresComm *c, int64_t *totalGroups, char *err, int errLen) {
  try {
    if (!c || !c->allGather) throw AbiError("no communicator");
    if (q->plan.isHLL()) throw AbiError("HyperLogLog shards merge through AresQueryMergeShards (all-gather of the entries + register-max)");
    const int mb = q->plan.measureBytes(), world = c->nranks;
    const int64_t rowBytes = q->layout.rowBytes + mb;
    const int n = q->resultSize;
    // 1. the local table in hash order: Sort (hashes + order) and Reduce (gather) of vector [0] into [1]
    std::vector<int64_t> split(world + 1, 0);
    if (n > 0) {
      const int64_t cap = q->resultCapacity;
      const bool ownVectors = q->hashVec[0] == nullptr;
      if (ownVectors) {
        for (int i = 0; i < 2; i++) {
          q->hashVec[i] = q->alloc<uint64_t>(static_cast<size_t>(cap) * 8);
          q->dimIndexVec[i] = q->alloc<uint32_t>(static_cast<size_t>(cap) * 4);
        }
      }
      check(q->lib->InitIndexVector(q->dimIndexVec[0], 0, n, q->stream, q->device));
      check(q->lib->Sort(q->dimensionVector(0), n, q->stream, q->device));
      const int kept = static_cast<int>(check(q->lib->Reduce(q->dimensionVector(0), q->measureVec[0], q->dimensionVector(1),
                                                             q->measureVec[1], mb, n, static_cast<AggregateFunction>(q->plan.aggFunc),
                                                             q->stream, q->device)));
      if (kept != n) throw AbiError("the shard's group table holds rows with equal 64-bit hashes");
      // 2. rank r takes hashes in [r * 2^64 / world, (r + 1) * 2^64 / world): binary searches in the sorted hashes
      auto hashAt = [&](int64_t i) {
        uint64_t h = 0;
        q->d2h(&h, q->hashVec[0] + i, 8);
        q->wait();
        return h;
      };
      for (int r = 1; r < world; r++) {
        const uint64_t bound = static_cast<uint64_t>((static_cast<unsigned __int128>(r) << 64) / static_cast<unsigned>(world));
        int64_t lo = split[r - 1], hi = n;  // first position with hash >= bound
        while (lo < hi) {
          const int64_t mid = (lo + hi) / 2;
          if (hashAt(mid) < bound) lo = mid + 1;
          else hi = mid;
        }
        split[r] = lo;
      }
      split[world] = n;
      q->wait();
      q->swapResultBuffers();  // vector [0] is the table in hash order now
      q->size = 0;
      if (ownVectors) {
        for (int i = 0; i < 2; i++) {
          q->release(q->hashVec[i]); q->release(q->dimIndexVec[i]);
          q->hashVec[i] = nullptr; q->dimIndexVec[i] = nullptr;
        }
      }
    }
    // 3. who sends how much to whom
    std::vector<int64_t> mine(world), all(static_cast<size_t>(world) * world);
    for (int r = 0; r < world; r++) mine[r] = split[r + 1] - split[r];
    gather_words(q, c, mine.data(), all.data(), sizeof(int64_t) * world);
    std::vector<int64_t> recvRows(world);
    int64_t total = 0, maxBlock = 1;
    for (int src = 0; src < world; src++) {
      recvRows[src] = all[static_cast<size_t>(src) * world + c->rank];
      total += recvRows[src];
      for (int dst = 0; dst < world; dst++) maxBlock = std::max(maxBlock, all[static_cast<size_t>(src) * world + dst]);
    }
    if (total > INT32_MAX) throw AbiError("a rank's share of the merged result exceeds 2^31 rows");
    // 4. pack one block per destination, of exactly its rows
    std::vector<size_t> sendBytes(world), sendOff(world), recvBytes(world), recvOff(world);
    size_t sendTotal = 0, recvTotal = 0;
    for (int r = 0; r < world; r++) {
      sendBytes[r] = static_cast<size_t>(mine[r] * rowBytes); sendOff[r] = sendTotal; sendTotal += sendBytes[r];
      recvBytes[r] = static_cast<size_t>(recvRows[r] * rowBytes); recvOff[r] = recvTotal; recvTotal += recvBytes[r];
    }
    uint8_t *packed = q->alloc(sendTotal), *arrived = q->alloc(recvTotal);
    for (int r = 0; r < world; r++) pack_block(q, packed + sendOff[r], mine[r], mine[r], split[r], mb);
    // 5. the exchange
    q->lib->noteWrite(q->device, arrived, recvTotal);
    if (c->allToAll) {
      if (c->allToAll(c->user, packed, sendBytes.data(), sendOff.data(), arrived, recvBytes.data(), recvOff.data(), q->stream) != 0)
        throw AbiError("all-to-all of the group table blocks failed");
    } else {  // destination by destination: everybody contributes its block for rank r, rank r keeps them
      const size_t pad = static_cast<size_t>(maxBlock * rowBytes);
      uint8_t *one = q->alloc(pad), *every = q->alloc(pad * world);
      for (int r = 0; r < world; r++) {
        if (sendBytes[r]) q->d2d(one, packed + sendOff[r], sendBytes[r]);
        q->lib->noteWrite(q->device, every, pad * world);
        if (c->allGather(c->user, one, every, pad, q->stream) != 0) throw AbiError("all-gather of the group table blocks failed");
        if (r == c->rank)
          for (int src = 0; src < world; src++)
            if (recvBytes[src]) q->d2d(arrived + recvOff[src], every + pad * src, recvBytes[src]);
        q->wait();  // `one` is refilled for the next destination
      }
      q->release(one);
      q->release(every);
    }
    // 6. append what arrived into fresh result vectors and re-reduce
    q->wait();
    q->releaseAll();
    q->resultSize = 0;
    q->size = static_cast<int>(total);
    if (total > 0) q->prepareForDimAndMeasureEval();
    int64_t base = 0;
    for (int src = 0; src < world; src++) {
      append_block(q, arrived + recvOff[src], recvRows[src], recvRows[src], base, q->measureVec[0] + base * mb, mb);
      base += recvRows[src];
    }
    q->wait();
    q->release(packed);
    q->release(arrived);
    if (total > 0) {
      q->reduce();
      q->postExec();
    } else {
      q->size = 0;
    }
    // 7. the size of the whole result: every rank's share
    if (totalGroups) {
      std::vector<int64_t> shares(world, 0);
      const int64_t share = q->resultSize;
      gather_words(q, c, &share, shares.data(), sizeof(int64_t));
      *totalGroups = 0;
      for (int64_t v : shares) *totalGroups += v;
    }
    return 0;
  } catch (std::exception &e) {
    set_err(err, errLen, e.what());
    return -1;
  }
}

}  // extern "C"
