// Stand-alone sanitizer run of the host driver's non-aggregation executor (CPU only, no GPU, no Python):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -Iinclude -Iaresdb_amd/csrc/host -I/opt/rocm/include \
//       tools/nonaggr_sanitize.cpp aresdb_amd/csrc/host/ares_driver.cpp -ldl -lpthread -o /tmp/nonaggr_sanitize
//   /tmp/nonaggr_sanitize oracle/_build/liboracle.so
// The driver's sources are compiled INTO the program and drive the plain-C oracle (host pointers): three batches of growing
// size, SELECT ts, city WHERE ts >= 500 LIMIT n with the limit reached in the middle of the second batch, checked against a loop.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ares_driver.h"

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <liboracle.so>\n", argv[0]);
    return 2;
  }
  char err[512] = {0};
  void *driver = AresDriverOpen(argv[1], argv[1], err, sizeof(err));
  if (!driver) {
    fprintf(stderr, "open: %s\n", err);
    return 1;
  }
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
  AresDriverClose(driver);
  printf(rc == 0 ? "nonaggr_sanitize: ok (%d rows)\n" : "nonaggr_sanitize: FAILED (%d rows)\n", n);
  return rc;
}
