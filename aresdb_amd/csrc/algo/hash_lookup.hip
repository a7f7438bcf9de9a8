// HashLookup for MI355X (gfx950): foreign-key column -> RecordID through the cuckoo index.
//
// Reference: query/hash_lookup.cu:70-157 and HashLookupFunctor, query/functor.hpp:1173-1266.
// One lane probes one row; the probe itself is cuckoo_probe (cuckoo_probe.hpp).
#include <hip/hip_runtime.h>

#include "binding.hpp"
#include "common.hpp"
#include "cuckoo_probe.hpp"
#include "device_model.hpp"
#include "fast_eval.hpp"

namespace ares {

constexpr int kBlock = 256;

struct LookupParams {
  OperandD a;
  const uint32_t *idx;
  const uint32_t *baseCounts;
  uint32_t startCount;
  int needRow;
  CuckooD index;
};

__global__ __launch_bounds__(kBlock) void hash_lookup_kernel(LookupParams p, RecordID *out, int n) {
  const FastDivisor bucketDiv = make_fast_divisor(p.index.numBuckets);  // hv % numBuckets by multiply-high
  for (int64_t i64 = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i64 < n;
       i64 += static_cast<int64_t>(gridDim.x) * kBlock) {
    const uint32_t i = static_cast<uint32_t>(i64);
    const uint32_t row = p.needRow ? p.idx[i] : i;
    uint32_t key[4] = {0, 0, 0, 0};
    const uint32_t ok = cuckoo_load_key(p.a, i, row, p.baseCounts, p.startCount, key);
    RecordID rid = {0, 0};
    if (ok) rid = cuckoo_probe(p.index, bucketDiv, key);
    out[i] = rid;
  }
}

}  // namespace ares

using namespace ares;

extern "C" CGoCallResHandle HashLookup(InputVector input, RecordID *output, uint32_t *indexVector,
                                       int indexVectorLength, uint32_t *baseCounts, uint32_t startCount,
                                       CuckooHashIndex hashIndex, void *cudaStream, int device) {
  ARES_ABI_BEGIN(device)
  materialize_index_vector(device, indexVector);
  hipStream_t stream = reinterpret_cast<hipStream_t>(cudaStream);
  if (indexVectorLength > 0) {
    LookupParams p;
    memset(&p, 0, sizeof(p));
    CallTemps temps;
    bind_operand(input, true, stream, p.a, temps);
    if (p.a.kind == K_GEO || ((p.a.type == OP_SCRATCH || p.a.type == OP_FOREIGN) && is_wide(p.a.kind)))
      throw std::invalid_argument("Unsupported data type for HashLookup");
    if (!cuckoo_geometry_ok(hashIndex)) throw std::invalid_argument("Unsupported cuckoo hash index geometry");
    p.idx = indexVector;
    p.baseCounts = baseCounts;
    p.startCount = startCount;
    p.needRow = indexVector != nullptr && p.a.type == OP_COLUMN;
    p.index = make_cuckoo(hashIndex);
    const int grid = capped_grid((static_cast<int64_t>(indexVectorLength) + kBlock - 1) / kBlock, 256 * 16);
    mem_note_write(device, output, sizeof(RecordID) * static_cast<size_t>(indexVectorLength));
    ARES_LAUNCH("hash_lookup_kernel", hash_lookup_kernel, grid, kBlock, stream, p, output, indexVectorLength);
  }
  resHandle.res = int_result(indexVectorLength);
  ARES_ABI_END("HashLookup")
}
