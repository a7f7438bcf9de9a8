// The polygon edge walk of the geo kernels (geo.hip: geo_intersect_kernel over the index vector; geo_column.hip:
// geo_shape_column_kernel over the live rows of a tile): one lane owns one test point, a wavefront walks all polygon edges 64
// at a time.  Every lane of the wavefront must call geo_walk_edges together (ballots, v_readlane, ds_bpermute).
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

namespace ares {

// GeoPredicateIterator (query/iterator.hpp:1263-1315): first set bit as an int8 — shape numbers
// 128..255 wrap to negative values, which every consumer reads as "no shape"
template <int W>
__device__ __forceinline__ int first_shape(const uint32_t (&words)[W], int totalWords) {
#pragma unroll
  for (int w = 0; w < W; w++)
    if (w < totalWords && words[w]) return static_cast<int8_t>(w * 32 + __builtin_ctz(words[w]));
  return -1;
}

// One wavefront = 64 test points x all polygon edges, 64 edges at a time:
//   * lane l fetches polygon points e0+l and e0+l+1 (edge l of the chunk) — coalesced, cached;
//   * hot loop, no memory and no branches: for every polygon point k of the chunk the longitude is
//     broadcast with v_readlane and compared with the lane's own test longitude; the 65 results
//     form a per-lane bit string G, and "edge k straddles the test longitude" is G ^ (G >> 1),
//     masked with the wave-uniform set of real edges (same shape, no ring separator);
//   * only the few straddling edges of each lane reach the exact test: the lane pulls that edge's
//     coordinates out of the owning lane with ds_bpermute and evaluates the reference's
//     expression (same operations, same order, IEEE division) — every lane works on its own edge.
// acc[w] receives the crossing parity of shapes 32w .. 32w+31 for (testLat, testLong); a lane without a valid point passes
// the NaN test longitude, which compares false against everything.  The call walks the 64-edge chunks firstChunk,
// firstChunk + chunkStride, ... (both wave-uniform): the parities of calls that share the chunks between them combine with XOR.
template <int W>
__device__ __forceinline__ void geo_walk_edges(const float *lats, const float *longs, const uint8_t *shape, int numPoints,
                                               int lane, float testLat, float testLong, uint32_t (&acc)[W], int firstChunk = 0,
                                               int chunkStride = 1) {
  const int numEdges = numPoints - 1;
#pragma unroll
  for (int w = 0; w < W; w++) acc[w] = 0;
  for (int e0 = 64 * firstChunk; e0 < numEdges; e0 += 64 * chunkStride) {
    const int p = e0 + lane;
    const bool have = p < numEdges;
    float lat1 = 0.f, lat2 = 0.f, long1 = 0.f, long2 = 0.f;
    int s1 = -1, s2 = -2;
    if (p < numPoints) {  // the chunk's last edge ends on a point that starts no edge of its own
      lat1 = lats[p];
      long1 = longs[p];
      s1 = shape[p];
    }
    if (have) {
      lat2 = lats[p + 1];
      long2 = longs[p + 1];
      s2 = shape[p + 1];
    }
    const uint64_t edges = __ballot(have && s1 == s2 && lat1 < FLT_MAX && lat2 < FLT_MAX);
    if (edges == 0) continue;
    // G: bit k = (longitude of polygon point e0+k > test longitude), k = 0..64
    const int long1Bits = __float_as_int(long1);
    uint32_t gLo = 0, gHi = 0;
#pragma unroll
    for (int k = 0; k < 32; k++) {
      const float a = __int_as_float(__builtin_amdgcn_readlane(long1Bits, k));
      const float b = __int_as_float(__builtin_amdgcn_readlane(long1Bits, k + 32));
      gLo |= a > testLong ? (1u << k) : 0u;
      gHi |= b > testLong ? (1u << k) : 0u;
    }
    const float last = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(long2), 63));
    const uint64_t g = (static_cast<uint64_t>(gHi) << 32) | gLo;
    const uint64_t gNext = (g >> 1) | (last > testLong ? (1ull << 63) : 0ull);
    uint64_t cross = (g ^ gNext) & edges;
    const float dLat = __fsub_rn(lat2, lat1);
    while (__ballot(cross != 0)) {
      const bool active = cross != 0;
      const int k = active ? __builtin_ctzll(cross) : 0;
      cross &= cross - 1;
      const float eLat1 = __shfl(lat1, k), eLong1 = __shfl(long1, k), eLong2 = __shfl(long2, k);
      const float eDLat = __shfl(dLat, k);
      const int s = __shfl(s1, k);
      if (active) {
        // (lat2 - lat1) * (testLong - long1) / (long2 - long1) + lat1, in the reference's order
        const float t = __fadd_rn(
            __fdiv_rn(__fmul_rn(eDLat, __fsub_rn(testLong, eLong1)), __fsub_rn(eLong2, eLong1)), eLat1);
        if (testLat < t) {
#pragma unroll
          for (int w = 0; w < W; w++)
            if ((s >> 5) == w) acc[w] ^= 1u << (s & 31);
        }
      }
    }
  }
}

}  // namespace ares
