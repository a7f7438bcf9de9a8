// One probe of the cuckoo index (memstore/cuckoo_index.go:42-48), shared by HashLookup (hash_lookup.hip) and the join
// flavour of the select scan (select_scan.hip).
//
// Reference: HashLookupFunctor, query/functor.hpp:1173-1266.  Index layout: numBuckets buckets + 1 stash bucket of
// bucketBytes = 8 * (8 + 1 + keyBytes); bucket = [RecordID x8][signature u8 x8][key x8].
//
// Unlike the reference's byte-wise memequal the slot test is done on the 8 signature bytes at once (one 8-byte load, the
// candidate slots as a bit mask) and a key is only fetched for slots whose signature matches, so a probe normally touches
// 64 B of signatures/keys plus one 8-byte RecordID instead of walking 104 B byte by byte.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_model.hpp"
#include "fast_eval.hpp"

namespace ares {

// the index as the kernels see it
struct CuckooD {
  const uint8_t *buckets;
  uint32_t seeds[4];
  int keyBytes;
  int numHashes;
  uint32_t numBuckets;
  uint32_t bucketBytes;
};

// the geometry HashLookup accepts
inline bool cuckoo_geometry_ok(const CuckooHashIndex &h) {
  return !(h.keyBytes < 1 || h.keyBytes > 16 || h.numBuckets < 1 || h.numHashes < 0 || h.numHashes > 4);
}

inline CuckooD make_cuckoo(const CuckooHashIndex &h) {
  CuckooD c;
  c.buckets = h.buckets;
  for (int i = 0; i < 4; i++) c.seeds[i] = h.seeds[i];
  c.keyBytes = h.keyBytes;
  c.numHashes = h.numHashes;
  c.numBuckets = static_cast<uint32_t>(h.numBuckets);
  c.bucketBytes = HASH_BUCKET_SIZE * (8 + 1 + h.keyBytes);
  return c;
}

struct __attribute__((packed, aligned(1))) KeyWord { uint32_t v; };

__device__ __forceinline__ bool key_equal(const uint8_t *slotKey, const uint32_t (&key)[4], int keyBytes) {
  // keys are stored unaligned (offset 72 + j*keyBytes): word-wise with byte-aligned loads (gfx950 global loads need no
  // alignment), the odd tail byte-wise.  Constant indices into `key`: a run-time index would put it in scratch memory.
  bool same = true;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const int have = keyBytes - 4 * w;
    if (have >= 4) {
      same = same && reinterpret_cast<const KeyWord *>(slotKey)[w].v == key[w];
    } else if (have > 0) {
      uint32_t tail = 0;
      for (int b = 0; b < have; b++) tail |= static_cast<uint32_t>(slotKey[4 * w + b]) << (8 * b);
      same = same && tail == (key[w] & ((1u << (8 * have)) - 1u));
    }
  }
  return same;
}

// The key of output position i (row = indexVector[i] for columns) as the probe takes it: the widened 32-bit value, or the raw
// bytes of an Int64 / UUID; returns the key's validity.
__device__ __forceinline__ uint32_t cuckoo_load_key(const OperandD &a, uint32_t i, uint32_t row, const uint32_t *baseCounts, uint32_t startCount,
                                                    uint32_t (&key)[4]) {
  if (a.kind == K_I64 || a.kind == K_UUID) {
    // wide keys: read the raw value bytes
    const int w = a.kind == K_UUID ? 16 : 8;
    if (a.type == OP_CONST) {
      key[0] = static_cast<uint32_t>(a.c64[0]); key[1] = static_cast<uint32_t>(a.c64[0] >> 32);
      key[2] = static_cast<uint32_t>(a.c64[1]); key[3] = static_cast<uint32_t>(a.c64[1] >> 32);
      return a.cok;
    }
    const uint32_t pos = locate(a, row, baseCounts, startCount);
    const uint32_t *v = reinterpret_cast<const uint32_t *>(a.base + a.valuesOff + static_cast<size_t>(w) * pos);
#pragma unroll  // (constant indices keep the key words in registers)
    for (int k = 0; k < 4; k++)
      if (k < (w >> 2)) key[k] = v[k];
    return a.mode >= 2 ? get_bit(a.base + a.nullsOff, pos + a.bitOff) : 1u;
  }
  const DVal v = load32(a, i, row, baseCounts, startCount);
  key[0] = v.bits;
  return v.ok;
}

// The record of `key` (the widened value's words; everything beyond keyBytes is cleared here), {0, 0} when the index does
// not hold it.  bucketDiv = make_fast_divisor(c.numBuckets): hv % numBuckets by multiply-high.
__device__ __forceinline__ RecordID cuckoo_probe(const CuckooD &c, const FastDivisor &bucketDiv, uint32_t (&key)[4]) {
  // the key is the first keyBytes bytes of the (widened) value: clear everything beyond
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const int have = c.keyBytes - 4 * w;  // bytes of this word that belong to the key
    if (have <= 0) key[w] = 0;
    else if (have < 4) key[w] &= (1u << (8 * have)) - 1u;
  }
  RecordID rid = {0, 0};
  bool found = false;
#pragma unroll  // (constant indices into c.seeds)
  for (int h = 0; h < 4; h++) {
    if (h >= c.numHashes || found) break;
    const uint32_t hv = murmur3_32_words<4>(key, c.keyBytes, c.seeds[h]);
    uint32_t bq, bidx;
    fast_divmod(bucketDiv, hv, bq, bidx);
    if (c.numBuckets == 1) bidx = 0;
    const uint8_t *bucket = c.buckets + static_cast<size_t>(bidx) * c.bucketBytes;
    uint32_t sig = hv >> 24;
    if (sig < 1) sig = 1;
    // 8 signature bytes at offset 64 (bucket start is 8-byte aligned: bucketBytes % 8 == 0)
    const uint64_t sigs = *reinterpret_cast<const uint64_t *>(bucket + 64);
    // candidate slots first (pure ALU on the 8 signature bytes), then only those are visited, in
    // slot order: lanes of a wavefront no longer walk all eight slots in lockstep (4.3 -> 2.4 ms
    // per 64 Mi rows; hashing all four bucket choices up front instead was slower: 2.75 ms)
    uint32_t cand = 0;
#pragma unroll
    for (int j = 0; j < HASH_BUCKET_SIZE; j++) cand |= (((sigs >> (8 * j)) & 0xff) == sig ? 1u : 0u) << j;
    while (cand) {
      const int j = __builtin_ctz(cand);
      cand &= cand - 1;
      if (key_equal(bucket + 72 + j * c.keyBytes, key, c.keyBytes)) {
        rid = reinterpret_cast<const RecordID *>(bucket)[j];
        found = true;
        break;
      }
    }
  }
  if (!found) {
    const uint8_t *stash = c.buckets + static_cast<size_t>(c.numBuckets) * c.bucketBytes;
    for (int j = 0; j < HASH_STASH_SIZE; j++) {
      if (stash[64 + j] != 0 && key_equal(stash + 72 + j * c.keyBytes, key, c.keyBytes)) {
        rid = reinterpret_cast<const RecordID *>(stash)[j];
        break;
      }
    }
  }
  return rid;
}

}  // namespace ares
