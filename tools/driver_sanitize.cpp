// Stand-alone sanitizer run of the host driver (CPU only, no GPU, no Python):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -Iinclude -Iaresdb_amd/csrc/host -I/opt/rocm/include \
//       tools/driver_sanitize.cpp aresdb_amd/csrc/host/batch_executor.cpp aresdb_amd/csrc/host/row_space.cpp \
//       aresdb_amd/csrc/host/shard_merge.cpp aresdb_amd/csrc/host/host_batches.cpp -ldl -lpthread -o /tmp/driver_sanitize
//   /tmp/driver_sanitize oracle/_build/liboracle.so
// The driver's sources are compiled INTO the program and drive the plain-C oracle (host pointers):
//   - the non-aggregation executor: three batches of growing size, SELECT ts, city WHERE ts >= 500 LIMIT n with the limit
//     reached in the middle of the second batch;
//   - the dimension-vector copier: SUM(v) GROUP BY three dimensions 1, 4 and 2 bytes wide (a wrong offset or stride lands in
//     another section) over batches of 5, 40 and 300 rows, so the result buffers grow and carry over twice — once with
//     HashReduce, once with Sort + Reduce — then AresQueryFetch, AresQueryMergeShards and AresQueryMergeShardsPartitioned
//     over a one-rank communicator whose all-gather is memcpy.
// Every fetched result is checked against a loop.  The row-space rewrites do not run here: the oracle has no such entry points.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "ares_driver.h"

static char err[512];

static int run_nonaggr(void *driver) {
  AresPlanNode nodes[4];
  memset(nodes, 0, sizeof(nodes));
  nodes[0].kind = ARES_NODE_COLUMN; nodes[0].column = 0;                                  // ts
  nodes[1].kind = ARES_NODE_CONST_INT; nodes[1].ival = 500;
  nodes[2].kind = ARES_NODE_BINARY; nodes[2].op = GreaterThanOrEqual; nodes[2].lhs = 0; nodes[2].rhs = 1; nodes[2].outType = Bool;
  nodes[3].kind = ARES_NODE_COLUMN; nodes[3].column = 1;                                  // city
  const int filters[1] = {2}, dimNodes[2] = {0, 3}, dimTypes[2] = {Uint32, Uint16};
  const int sizes[3] = {300, 700, 1500};
  std::vector<std::vector<uint32_t>> ts(3);
  std::vector<std::vector<uint16_t>> city(3);
  std::vector<uint32_t> wantTs;
  std::vector<uint16_t> wantCity;
  uint32_t seed = 12345;
  int survivors[3] = {0, 0, 0};
  for (int b = 0; b < 3; b++)
    for (int i = 0; i < sizes[b]; i++) {
      seed = seed * 1664525u + 1013904223u;
      ts[b].push_back((seed >> 8) % 1000);
      city[b].push_back(static_cast<uint16_t>(seed >> 20));
      survivors[b] += ts[b].back() >= 500;
    }
  const int limit = survivors[0] + survivors[1] / 2;
  for (int b = 0; b < 3; b++)
    for (int i = 0; i < sizes[b] && static_cast<int>(wantTs.size()) < limit; i++)
      if (ts[b][i] >= 500) {
        wantTs.push_back(ts[b][i]);
        wantCity.push_back(city[b][i]);
      }
  AresQueryPlan plan;
  memset(&plan, 0, sizeof(plan));
  plan.nodes = nodes; plan.numNodes = 4;
  plan.filters = filters; plan.numFilters = 1;
  plan.dimNodes = dimNodes; plan.dimTypes = dimTypes; plan.numDims = 2;
  plan.measureNode = 1; plan.aggFunc = AGGR_SUM_UNSIGNED; plan.measureType = Uint32; plan.useHashReduction = 1;
  plan.isNonAggregation = 1; plan.limit = limit;
  AresQuery *q = AresQueryCreate(driver, &plan, 0, nullptr, err, sizeof(err));
  if (!q) {
    fprintf(stderr, "create: %s\n", err);
    return 1;
  }
  long callsBeforeThird = 0;
  for (int b = 0; b < 3; b++) {
    VectorPartySlice cols[2];
    memset(cols, 0, sizeof(cols));
    cols[0].BasePtr = reinterpret_cast<uint8_t *>(ts[b].data()); cols[0].DataType = Uint32; cols[0].Length = sizes[b];
    cols[1].BasePtr = reinterpret_cast<uint8_t *>(city[b].data()); cols[1].DataType = Uint16; cols[1].Length = sizes[b];
    if (b == 2) callsBeforeThird = AresQueryNumCalls(q);
    if (AresQueryRunBatch(q, cols, 2, sizes[b], nullptr, 0, err, sizeof(err)) != 0) {
      fprintf(stderr, "batch %d: %s\n", b, err);
      return 1;
    }
  }
  int rc = 0;
  const int n = AresQueryResultSize(q);
  if (n != limit || !AresQueryDone(q) || AresQueryNumCalls(q) != callsBeforeThird) {
    fprintf(stderr, "rows %d (wanted %d), done %d, calls of the third batch %ld\n", n, limit, AresQueryDone(q), AresQueryNumCalls(q) - callsBeforeThird);
    rc = 1;
  }
  std::vector<uint8_t> dims(static_cast<size_t>(n) * (4 + 2 + 2) + 1);
  if (AresQueryFetch(q, dims.data(), nullptr, err, sizeof(err)) != 0) {
    fprintf(stderr, "fetch: %s\n", err);
    rc = 1;
  } else if (rc == 0) {
    if (memcmp(dims.data(), wantTs.data(), 4u * n) != 0 || memcmp(dims.data() + 4u * n, wantCity.data(), 2u * n) != 0) {
      fprintf(stderr, "rows differ from the loop\n");
      rc = 1;
    }
    for (int i = 0; i < 2 * n; i++)
      if (dims[6u * n + i] != 1) rc = 1;
  }
  AresQueryDestroy(q);
  printf(rc == 0 ? "non-aggregation: ok (%d rows)\n" : "non-aggregation: FAILED (%d rows)\n", n);
  return rc;
}

static int memcpy_all_gather(void *, const void *send, void *recv, size_t bytesPerRank, void *) {
  memcpy(recv, send, bytesPerRank);
  return 0;
}

using Groups = std::map<std::tuple<uint32_t, uint16_t, uint8_t>, uint32_t>;

// the query's result, fetched: values of the 4-, 2- and 1-byte dimension in that (vector) order, three validity vectors, measures
static int check_fetch(AresQuery *q, const Groups &want, const char *what) {
  const size_t n = static_cast<size_t>(AresQueryResultSize(q));
  std::vector<uint8_t> dims(n * (4 + 2 + 1 + 3) + 1), measures(n * 4 + 1);
  if (AresQueryFetch(q, dims.data(), measures.data(), err, sizeof(err)) != 0) {
    fprintf(stderr, "%s: fetch: %s\n", what, err);
    return 1;
  }
  Groups got;
  for (size_t i = 0; i < n; i++) {
    uint32_t a, v;
    uint16_t b;
    memcpy(&a, &dims[4 * i], 4);
    memcpy(&b, &dims[4 * n + 2 * i], 2);
    const uint8_t c = dims[6 * n + i];
    memcpy(&v, &measures[4 * i], 4);
    if (dims[7 * n + i] != 1 || dims[8 * n + i] != 1 || dims[9 * n + i] != 1 || !got.emplace(std::make_tuple(a, b, c), v).second) {
      fprintf(stderr, "%s: row %zu is null or a group seen before\n", what, i);
      return 1;
    }
  }
  if (got != want) {
    fprintf(stderr, "%s: %zu groups differ from the loop's %zu\n", what, got.size(), want.size());
    return 1;
  }
  return 0;
}

static int run_aggregation(void *driver, bool useHashReduction) {
  const char *name = useHashReduction ? "HashReduce" : "Sort + Reduce";
  // columns: c (Uint8), a (Uint32), b (Uint16), v (Uint32); SELECT SUM(v) WHERE v >= 100 GROUP BY c, a, b
  AresPlanNode nodes[6];
  memset(nodes, 0, sizeof(nodes));
  for (int i = 0; i < 4; i++) { nodes[i].kind = ARES_NODE_COLUMN; nodes[i].column = i; }
  nodes[4].kind = ARES_NODE_CONST_INT; nodes[4].ival = 100;
  nodes[5].kind = ARES_NODE_BINARY; nodes[5].op = GreaterThanOrEqual; nodes[5].lhs = 3; nodes[5].rhs = 4; nodes[5].outType = Bool;
  const int filters[1] = {5}, dimNodes[3] = {0, 1, 2}, dimTypes[3] = {Uint8, Uint32, Uint16};
  const int sizes[3] = {5, 40, 300};
  AresQueryPlan plan;
  memset(&plan, 0, sizeof(plan));
  plan.nodes = nodes; plan.numNodes = 6;
  plan.filters = filters; plan.numFilters = 1;
  plan.dimNodes = dimNodes; plan.dimTypes = dimTypes; plan.numDims = 3;
  plan.measureNode = 3; plan.aggFunc = AGGR_SUM_UNSIGNED; plan.measureType = Uint32;
  plan.useHashReduction = useHashReduction ? 1 : 0;
  plan.limit = -1;
  AresQuery *q = AresQueryCreate(driver, &plan, 0, nullptr, err, sizeof(err));
  if (!q) {
    fprintf(stderr, "%s: create: %s\n", name, err);
    return 1;
  }
  Groups want;
  uint32_t seed = 2024;
  int lastCapacity = 0, grown = 0;
  for (int k = 0; k < 3; k++) {
    std::vector<uint8_t> c;
    std::vector<uint32_t> a, v;
    std::vector<uint16_t> b;
    for (int i = 0; i < sizes[k]; i++) {
      seed = seed * 1664525u + 1013904223u;
      c.push_back(static_cast<uint8_t>(200 + (seed >> 8) % 3));
      a.push_back(0x01020304u * ((seed >> 12) % 7 + 1));
      b.push_back(static_cast<uint16_t>(0x1100 + (seed >> 16) % 5));
      v.push_back((seed >> 20) % 1000);
      if (v.back() >= 100) want[std::make_tuple(a.back(), b.back(), c.back())] += v.back();
    }
    VectorPartySlice cols[4];
    memset(cols, 0, sizeof(cols));
    cols[0].BasePtr = c.data(); cols[0].DataType = Uint8;
    cols[1].BasePtr = reinterpret_cast<uint8_t *>(a.data()); cols[1].DataType = Uint32;
    cols[2].BasePtr = reinterpret_cast<uint8_t *>(b.data()); cols[2].DataType = Uint16;
    cols[3].BasePtr = reinterpret_cast<uint8_t *>(v.data()); cols[3].DataType = Uint32;
    for (VectorPartySlice &s : cols) s.Length = sizes[k];
    if (AresQueryRunBatch(q, cols, 4, sizes[k], nullptr, 0, err, sizeof(err)) != 0) {
      fprintf(stderr, "%s: batch %d: %s\n", name, k, err);
      return 1;
    }
    grown += AresQueryResultCapacity(q) > lastCapacity;
    lastCapacity = AresQueryResultCapacity(q);
  }
  int rc = 0;
  if (grown != 3) {  // (allocated by the first batch, grown and carried over by the second and the third)
    fprintf(stderr, "%s: the result buffers grew %d times, not 3\n", name, grown);
    rc = 1;
  }
  rc |= check_fetch(q, want, name);
  AresComm *comm = AresCommCreate(0, 1, memcpy_all_gather, nullptr);
  if (!comm || AresQueryMergeShards(q, comm, err, sizeof(err)) != 0) {
    fprintf(stderr, "%s: merge: %s\n", name, comm ? err : "no communicator");
    rc = 1;
  } else {
    rc |= check_fetch(q, want, "AresQueryMergeShards");
  }
  int64_t total = -1;
  if (!comm || AresQueryMergeShardsPartitioned(q, comm, &total, err, sizeof(err)) != 0) {
    fprintf(stderr, "%s: partitioned merge: %s\n", name, comm ? err : "no communicator");
    rc = 1;
  } else {
    if (total != static_cast<int64_t>(want.size())) rc = 1;
    rc |= check_fetch(q, want, "AresQueryMergeShardsPartitioned");
  }
  AresCommDestroy(comm);
  AresQueryDestroy(q);
  printf(rc == 0 ? "%s: ok (%zu groups)\n" : "%s: FAILED (%zu groups)\n", name, want.size());
  return rc;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <liboracle.so>\n", argv[0]);
    return 2;
  }
  void *driver = AresDriverOpen(argv[1], argv[1], err, sizeof(err));
  if (!driver) {
    fprintf(stderr, "open: %s\n", err);
    return 1;
  }
  int rc = run_nonaggr(driver);
  rc |= run_aggregation(driver, true);
  rc |= run_aggregation(driver, false);
  AresDriverClose(driver);
  printf(rc == 0 ? "driver_sanitize: ok\n" : "driver_sanitize: FAILED\n");
  return rc;
}
