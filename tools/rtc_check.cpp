// Builds the C3 plan and the other shapes of the matrix by hand, writes the hiprtc source the library generates for each,
// compiles it for gfx950 (no GPU needed) and writes the code object next to it:  tools/bin/rtc_check [out-prefix]
// Then checks every shape's spec against its source (rtc_shapes.hpp: check_specs).
// Links against aresdb_amd/lib/libalgorithm.so (ares::rtc_source is an ordinary exported symbol).
// -DRTC_SOURCES_ONLY: no hiprtc and no library — the sources are written and the specs checked, nothing is compiled; linked with
// hr_rtc_gen.hip alone (the generator is pure host code: this is how it runs under the host sanitizers).
#ifndef RTC_SOURCES_ONLY
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#endif

#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "rtc_shapes.hpp"

using namespace rtc_shapes;

#ifdef RTC_SOURCES_ONLY
namespace ares {
bool phases_enabled() { return false; }  // (hr_rtc.hip's reads the environment)
}
#endif

int main(int argc, char **argv) {
  const FusedPlanD p = c3_plan();
  const std::string prefix = argc > 1 ? argv[1] : "/tmp/hr_scan_rtc";
  std::vector<Shape> shapes;  // everything that is built, for check_specs
#ifdef RTC_SOURCES_ONLY
  auto compile = [&](const std::string &, const char *, const std::string &, const char *) -> int { return 0; };
#else
  const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics"};
  // co: where the code object goes ("" = nowhere)
  auto compile = [&](const std::string &src, const char *file, const std::string &co, const char *what) -> int {
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), file, 0, nullptr, nullptr) != HIPRTC_SUCCESS) return 3;
    const hiprtcResult rc = hiprtcCompileProgram(prog, 4, opts);
    size_t ln = 0; hiprtcGetProgramLogSize(prog, &ln);
    std::string log(ln, 0); if (ln) hiprtcGetProgramLog(prog, &log[0]);
    printf("%s compile rc %d\n%s\n", what, static_cast<int>(rc), log.c_str());
    if (rc != HIPRTC_SUCCESS) return 4;
    if (co.empty()) return 0;
    size_t sz = 0; hiprtcGetCodeSize(prog, &sz);
    std::vector<char> code(sz); hiprtcGetCode(prog, code.data());
    std::ofstream(co, std::ios::binary).write(code.data(), static_cast<std::streamsize>(sz));
    printf("%s code object %zu bytes -> %s\n", what, sz, co.c_str());
    return 0;
  };
#endif
  auto build = [&](const Shape &shape, const std::string &tag, const char *what) -> int {
    shapes.push_back(shape);
    const std::string src = source(shape);
    if (src.empty()) { printf("%s: unsupported plan\n", what); return 2; }
    std::ofstream(prefix + tag + ".hip") << src;
    return compile(src, "hr_rtc.hip", prefix + tag + ".co", what);
  };
  AggSpec agg = make_agg_spec(AGGR_SUM_FLOAT, 8);
  hr::Widen w{1, K_F32, Float64};
  // the same shape with another comparison constant is the same source text (constants are kernel arguments)
  {
    FusedPlanD p2 = p;
    p2.filters[0].f.bbits = 17;
    if (source(scan(p2, 4, 9, true)) != source(scan(p, 4, 9, true))) { puts("comparison constants leak into the source"); return 20; }
    if (spec(scan(p2, 4, 9, true)) != spec(scan(p, 4, 9, true))) { puts("comparison constants leak into the spec"); return 20; }
    p2.dims[0].f.bbits = 60;
    if (source(scan(p2, 4, 9, true)) == source(scan(p, 4, 9, true))) { puts("divisors must be literals"); return 21; }
    if (spec(scan(p2, 4, 9, true)) == spec(scan(p, 4, 9, true))) { puts("divisors must be part of the spec"); return 21; }
  }
  if (int rc = build(scan(p, 4, 9, false), "", "scan")) return rc;
  if (int rc = build(merge(p, 4, 9, agg, w, false), "_merge", "merge")) return rc;
  if (int rc = build(scan(p, 4, 9, true), "_compact", "compact scan")) return rc;
  if (int rc = build(merge(p, 4, 9, agg, w, true), "_cmerge", "compact merge")) return rc;
  if (int rc = build(table_scan(p, 4, 9, agg, w), "_table", "table scan")) return rc;
  // table images (hash_reduce_lds.hip): the merge that leaves its table in HBM, and the one that starts from it
  if (int rc = build(merge(p, 4, 9, agg, w, true, false, 1), "_cmerge_img1", "compact merge + image out")) return rc;
  if (int rc = build(merge(p, 4, 9, agg, w, true, false, 2), "_cmerge_img2", "compact merge from image")) return rc;
  if (int rc = build(merge(p, 4, 9, agg, w, false, false, 2), "_merge_img2", "merge from image")) return rc;
  {  // another shape: two dimensions, int32 measure summed into 4 bytes, no nulls, 8 partitions
    FusedPlanD q = p;
    q.numCols = 3;
    for (int c = 0; c < 3; c++) q.cols[c].nulls = nullptr;
    q.numFilters = 0;
    q.dims[0] = p.dims[1]; q.dims[0].col = 0;
    q.dims[1] = p.dims[2]; q.dims[1].col = 1; q.dims[1].f.arity = 2; q.dims[1].f.functor = Plus; q.dims[1].f.bkind = K_I32; q.dims[1].f.bbits = 5; q.dims[1].f.bok = 1;
    q.measure.f = col(K_I32); q.measure.col = 2; q.measure.outKind = K_I32;
    q.measureDtype = Int32; q.measureWidth = 4; q.identity = 0;
    AggSpec a4 = make_agg_spec(AGGR_SUM_SIGNED, 4);
    hr::Widen w4{0, K_I32, Int32};
    if (int rc = build(scan(q, 2, 3, true), "_compact2", "compact scan (2 dims)")) return rc;
    if (int rc = build(merge(q, 2, 3, a4, w4, true), "_cmerge2", "compact merge (2 dims)")) return rc;
    if (int rc = build(table_scan(q, 2, 0, a4, w4), "_table2", "table scan (2 dims, 1 partition)")) return rc;
  }
  {  // a narrow plan, the reference's example schema (examples/1k_trips/schema/trips.json): dimensions [Floor(request_at, 3600)
     // Uint32, city_id Uint16 -> a 2-byte slot], SUM(fare), filters request_at >= / < (time range), status == k on a Uint8 column
    FusedPlanD t = p;
    t.numCols = 4;
    t.cols[0].step = 4; t.cols[1].step = 2; t.cols[2].step = 4; t.cols[3].step = 1;
    t.dims[1] = p.dims[1]; t.dims[1].col = 1;
    t.dimWidth[0] = 4; t.dimWidth[1] = 2;
    t.measure.f = col(K_F32); t.measure.col = 2; t.measure.outKind = K_F32;
    t.numFilters = 3;
    t.filters[0] = p.filters[0]; t.filters[0].f.functor = GreaterThanOrEqual; t.filters[0].col = 0;
    t.filters[1] = p.filters[0]; t.filters[1].f.functor = LessThan; t.filters[1].col = 0;
    t.filters[2] = p.filters[0]; t.filters[2].f.functor = Equal; t.filters[2].col = 3;
    if (int rc = build(scan(t, 2, 9, true), "_ncompact", "narrow compact scan")) return rc;
    if (int rc = build(merge(t, 2, 9, agg, w, true), "_ncmerge", "narrow compact merge")) return rc;
    if (int rc = build(scan(t, 2, 9, false), "_nlines", "narrow scan")) return rc;
    if (int rc = build(merge(t, 2, 9, agg, w, false), "_nmerge", "narrow merge")) return rc;
    if (int rc = build(table_scan(t, 2, 9, agg, w), "_ntable", "narrow table scan")) return rc;
    if (int rc = build(merge(t, 2, 9, agg, w, false, true), "_namerge", "narrow region-A merge")) return rc;
    if (int rc = build(merge(t, 2, 9, agg, w, true, false, 2), "_ncmerge_img2", "narrow compact merge from image")) return rc;
    // signed narrow columns and a 1-byte slot: dimensions [Int16 column -> 2-byte slot, Int8 column -> 1-byte slot], no nulls
    FusedPlanD u = t;
    u.numFilters = 0; u.numCols = 3;
    for (int c = 0; c < 3; c++) u.cols[c].nulls = nullptr;
    u.cols[0].step = 2; u.cols[1].step = 1; u.cols[2].step = 4;
    u.dims[0].f = col(K_I32); u.dims[0].col = 0; u.dims[0].outKind = K_I32;
    u.dims[1].f = col(K_I32); u.dims[1].col = 1; u.dims[1].outKind = K_I32;
    u.dimWidth[0] = 2; u.dimWidth[1] = 1;
    if (int rc = build(scan(u, 2, 9, true), "_scompact", "signed narrow compact scan")) return rc;
    if (int rc = build(merge(u, 2, 9, agg, w, true), "_scmerge", "signed narrow compact merge")) return rc;
  }
  {  // the Sort + Reduce path (sort_reduce_fused.hip): records keyed by lo64(murmur3_x64_128), constant measure (COUNT(*)) and a
     // column measure summed into 8 bytes, the C3 dimensions and the narrow trips shape
    FusedPlanD c = p;
    c.numCols = 4;  // no measure column: the filter's d1 is dimension 1's column
    c.measure.col = -1; c.measure.f = col(K_U32); c.measure.f.bbits = 1; c.measureDtype = Uint32; c.measureWidth = 4; c.identity = 0;
    if (int rc = build(sort_scan(c, 4, 9), "_sort_count", "sort scan (COUNT)")) return rc;
    {
      FusedPlanD c2 = c;
      c2.measure.f.bbits = 7;
      if (source(sort_scan(c2, 4, 9)) != source(sort_scan(c, 4, 9))) { puts("the constant measure leaks into the source"); return 22; }
      if (spec(sort_scan(c2, 4, 9)) != spec(sort_scan(c, 4, 9))) { puts("the constant measure leaks into the spec"); return 22; }
    }
    FusedPlanD m8 = p;
    m8.measure.f = col(K_U32); m8.measure.outKind = K_I32; m8.measureDtype = Int64; m8.measureWidth = 8;
    if (int rc = build(sort_scan(m8, 4, 9), "_sort_sum8", "sort scan (SUM into 8 bytes)")) return rc;
    // float measures on the same path: SUM(m) of a Float32 column into float64 (the C3 plan's own measure: the headline query
    // with enable_hash_reduction off), MIN_FLOAT into 4 bytes, SUM(m * 1.5); a float column times an INTEGER constant is declined
    if (int rc = build(sort_scan(p, 4, 9), "_sort_fsum8", "sort scan (SUM_FLOAT into 8 bytes)")) return rc;
    FusedPlanD f4 = p;
    f4.measureDtype = Float32; f4.measureWidth = 4; f4.identity = 0x7f7fffffu;  // (FLT_MAX: MIN_FLOAT's null)
    if (int rc = build(sort_scan(f4, 4, 9), "_sort_fmin", "sort scan (MIN_FLOAT)")) return rc;
    FusedPlanD fx = p;
    fx.measure.f.arity = 2; fx.measure.f.functor = Multiply; fx.measure.f.bkind = K_F32; fx.measure.f.bbits = 0x3fc00000u; fx.measure.f.bok = 1;
    if (int rc = build(sort_scan(fx, 4, 9), "_sort_fexpr", "sort scan (float expression)")) return rc;
    fx.measure.f.bkind = K_I32; fx.measure.f.bbits = 2;
    if (!source(sort_scan(fx, 4, 9)).empty()) { puts("a float column times an integer constant must be declined"); return 23; }
    FusedPlanD i4 = f4;  // an integer column stored into a float measure: declined (the transform converts, a record would not)
    i4.measure.f = col(K_U32);
    if (!source(sort_scan(i4, 4, 9)).empty()) { puts("an integer column into a 4-byte float measure must be declined"); return 24; }
    FusedPlanD t = p;  // trips: dims [Floor(request_at, 3600) Uint32, city_id Uint16 -> 2-byte slot], COUNT(*), three filters
    t.numCols = 3;
    t.cols[0].step = 4; t.cols[1].step = 2; t.cols[2].step = 1;
    t.dims[1] = p.dims[1]; t.dims[1].col = 1;
    t.dimWidth[0] = 4; t.dimWidth[1] = 2;
    t.measure = c.measure; t.measureDtype = Uint32; t.measureWidth = 4;
    t.numFilters = 3;
    t.filters[0] = p.filters[0]; t.filters[0].f.functor = GreaterThanOrEqual; t.filters[0].col = 0;
    t.filters[1] = p.filters[0]; t.filters[1].f.functor = LessThan; t.filters[1].col = 0;
    t.filters[2] = p.filters[0]; t.filters[2].f.functor = Equal; t.filters[2].col = 2;
    if (int rc = build(sort_scan(t, 2, 9), "_sort_trips", "narrow sort scan (COUNT)")) return rc;
  }
  {  // eight dimensions (MAX_DIMENSIONS, query/time_series_aggregate.h:36-37): six 4-byte slots, a 2-byte and a 1-byte one, the
     // measure and a filter on a column of its own — ten column slots
    FusedPlanD e = p;
    e.numCols = 10;
    for (int c = 0; c < 10; c++) { e.cols[c].vals = reinterpret_cast<const uint32_t *>(0x1000); e.cols[c].nulls = c % 3 ? reinterpret_cast<const uint8_t *>(0x2000) : nullptr; e.cols[c].step = 4; }
    e.cols[6].step = 2; e.cols[7].step = 1;
    for (int d = 0; d < 8; d++) { e.dims[d].f = col(K_U32); e.dims[d].col = d; e.dims[d].outKind = K_U32; e.dimWidth[d] = 4; }
    e.dims[0] = p.dims[0];
    e.dimWidth[6] = 2; e.dimWidth[7] = 1;
    e.measure.f = col(K_F32); e.measure.col = 8; e.measure.outKind = K_F32;
    e.numFilters = 1; e.filters[0] = p.filters[0]; e.filters[0].col = 9;
    if (int rc = build(scan(e, 8, 9, true), "_8compact", "8-dimension compact scan")) return rc;
    if (int rc = build(merge(e, 8, 9, agg, w, true), "_8cmerge", "8-dimension compact merge")) return rc;
    if (int rc = build(merge(e, 8, 9, agg, w, true, false, 2), "_8cmerge_img2", "8-dimension compact merge from image")) return rc;
    if (int rc = build(table_scan(e, 8, 9, agg, w), "_8table", "8-dimension table scan")) return rc;
    if (int rc = build(merge(e, 8, 9, agg, w, false, true), "_8amerge", "8-dimension region-A merge")) return rc;
    FusedPlanD ec = e;
    ec.numCols = 9; ec.cols[8] = e.cols[9]; ec.filters[0].col = 8;
    ec.measure.col = -1; ec.measure.f = col(K_U32); ec.measure.f.bbits = 1; ec.measureDtype = Uint32; ec.measureWidth = 4;
    if (int rc = build(sort_scan(ec, 8, 9), "_8sort", "8-dimension sort scan (COUNT)")) return rc;
  }
  // the vector-sourced sort scans (Sort + Reduce over materialised vectors: 64-bit row hash, up to eight 4-byte dimensions)
  if (int rc = build(vector_scan(RTC_SORT_VECTOR_SCAN, 2, nullptr, 4, 9), "_vsort2", "vector sort scan nd 2")) return rc;
  if (int rc = build(vector_scan(RTC_SORT_VECTOR_SCAN, 8, nullptr, 4, 9), "_vsort8", "vector sort scan nd 8")) return rc;
  if (int rc = build(vector_scan(RTC_SORT_VECTOR_SCAN, 1, nullptr, 4, 0), "_vsort1", "vector sort scan nd 1, one partition")) return rc;
  {
    const int narrow[4] = {4, 4, 2, 1};
    if (int rc = build(vector_scan(RTC_SORT_VECTOR_SCAN, 4, narrow, 4, 9), "_vsort_narrow", "vector sort scan, slots 4 4 2 1")) return rc;
  }
  {  // ... with slots of 8 and 16 bytes (Int64 / Uint64 / GeoPoint, UUID): UUID + Uint32; two 8-byte + two 4-byte slots; the
     // widest row the scan takes (32 value bytes); Int64 over one slot of every narrower width; a GeoPoint alone, one partition
    const int uuid4[2] = {16, 4}, i8844[4] = {8, 8, 4, 4}, w32[4] = {16, 8, 4, 4}, i8421[4] = {8, 4, 2, 1}, geo[1] = {8};
    if (int rc = build(vector_scan(RTC_SORT_VECTOR_SCAN, 2, uuid4, 4, 9), "_vsort_16_4", "vector sort scan, slots 16 4")) return rc;
    if (int rc = build(vector_scan(RTC_SORT_VECTOR_SCAN, 4, i8844, 4, 9), "_vsort_8_8_4_4", "vector sort scan, slots 8 8 4 4")) return rc;
    if (int rc = build(vector_scan(RTC_SORT_VECTOR_SCAN, 4, w32, 4, 9), "_vsort_16_8_4_4", "vector sort scan, slots 16 8 4 4")) return rc;
    if (int rc = build(vector_scan(RTC_SORT_VECTOR_SCAN, 4, i8421, 4, 9), "_vsort_8_4_2_1", "vector sort scan, slots 8 4 2 1")) return rc;
    if (int rc = build(vector_scan(RTC_SORT_VECTOR_SCAN, 1, geo, 4, 0), "_vsort_8", "vector sort scan, slot 8, one partition")) return rc;
    const int w40[3] = {16, 16, 8};  // beyond 32 value bytes: declined (the real Sort + Reduce runs)
    if (!source(vector_scan(RTC_SORT_VECTOR_SCAN, 3, w40, 4, 9)).empty()) { puts("a 40-byte row must be declined"); return 23; }
  }
  {  // HyperLogLog's pre-aggregation scan (hll.hip): the same rows, keyed by (row hash & ~0xFFFF) | register id, 512 partitions
     // chosen by a scramble of the whole key — one dimension, four narrow ones, eight, a UUID + Uint32, the widest row
    const int one[1] = {4}, narrow[4] = {4, 4, 2, 1}, uuid4[2] = {16, 4}, w32[4] = {16, 8, 4, 4};
    if (int rc = build(vector_scan(RTC_HLL_SCAN, 1, one, 4, 9), "_hll1", "hll scan, slot 4")) return rc;
    if (int rc = build(vector_scan(RTC_HLL_SCAN, 4, narrow, 4, 9), "_hll_narrow", "hll scan, slots 4 4 2 1")) return rc;
    if (int rc = build(vector_scan(RTC_HLL_SCAN, 8, nullptr, 4, 9), "_hll8", "hll scan nd 8")) return rc;
    if (int rc = build(vector_scan(RTC_HLL_SCAN, 2, uuid4, 4, 9), "_hll_16_4", "hll scan, slots 16 4")) return rc;
    if (int rc = build(vector_scan(RTC_HLL_SCAN, 4, w32, 4, 9), "_hll_16_8_4_4", "hll scan, slots 16 8 4 4")) return rc;
    if (!source(vector_scan(RTC_HLL_SCAN, 1, one, 4, 0)).empty()) { puts("an hll scan without partitions must be declined"); return 24; }
  }
  // the vector-sourced scan (HashReduce on materialised dimension / measure vectors) and its merge: every shape is compiled,
  // the widest one (four dimensions, 8-byte values) is written out
  for (int vw = 4; vw <= 8; vw += 4)
    for (int nd = 1; nd <= 4; nd += 3) {
      const bool keep = nd == 4 && vw == 8;
      const Shape vs = vector_scan(RTC_VECTOR_SCAN, nd, nullptr, vw, 9);
      const Shape vm = vector_merge(nd, vw, 9, make_agg_spec(vw == 8 ? AGGR_SUM_FLOAT : AGGR_SUM_UNSIGNED, vw));
      shapes.push_back(vs);
      shapes.push_back(vm);
      const std::string vsrc = source(vs), msrc = source(vm);
      if (vsrc.empty()) { puts("vector scan: unsupported"); return 8; }
      if (msrc.empty()) { puts("vector merge: unsupported"); return 11; }
      if (keep) std::ofstream(prefix + "_vector.hip") << vsrc;
      if (keep) std::ofstream(prefix + "_vmerge.hip") << msrc;
      const std::string what = " nd " + std::to_string(nd) + " vw " + std::to_string(vw);
      if (int rc = compile(vsrc, "hr_vscan_rtc.hip", keep ? prefix + "_vector.co" : "", ("vector scan" + what).c_str())) return rc + 6;
      if (int rc = compile(msrc, "hr_vmerge_rtc.hip", keep ? prefix + "_vmerge.co" : "", ("vector merge" + what).c_str())) return rc + 9;
    }
  return check_specs(shapes) ? 30 : 0;
}
