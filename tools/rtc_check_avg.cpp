// The Sort + Reduce scan (hr_rtc_gen.hip, RTC_SCAN_SORT64) generated for AVG_FLOAT next to its SUM_FLOAT-into-float64 sibling of the
// same shape — the C3 plan and the narrow trips plan of tools/rtc_check.cpp — compiled for gfx950 (no GPU needed):
//   tools/bin/rtc_check_avg [out-prefix]   writes <prefix>_<tag>.hip and <prefix>_<tag>.co
// Links against aresdb_amd/lib/libalgorithm.so like rtc_check.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "rtc_shapes.hpp"

using namespace rtc_shapes;

int main(int argc, char **argv) {
  const FusedPlanD p = c3_plan();
  // trips: dims [Floor(request_at, 3600) Uint32, city_id Uint16 -> 2-byte slot], fare Float32, filters request_at >= / <,
  // status == k on a Uint8 column
  FusedPlanD t = p;
  t.numCols = 4;
  t.cols[0].step = 4; t.cols[1].step = 2; t.cols[2].step = 4; t.cols[3].step = 1;
  t.dims[1] = p.dims[1]; t.dims[1].col = 1;
  t.dimWidth[0] = 4; t.dimWidth[1] = 2;
  t.measure.col = 2;
  t.numFilters = 3;
  t.filters[0] = p.filters[0]; t.filters[0].f.functor = GreaterThanOrEqual; t.filters[0].col = 0;
  t.filters[1] = p.filters[0]; t.filters[1].f.functor = LessThan; t.filters[1].col = 0;
  t.filters[2] = p.filters[0]; t.filters[2].f.functor = Equal; t.filters[2].col = 3;

  const std::string prefix = argc > 1 ? argv[1] : "/tmp/sr_avg_rtc";
  const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics"};
  auto build = [&](const Shape &shape, const std::string &tag, const char *what) -> int {
    const std::string src = source(shape);
    if (src.empty()) { printf("%s: unsupported plan\n", what); return 2; }
    std::ofstream(prefix + tag + ".hip") << src;
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "hr_rtc.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) return 3;
    const hiprtcResult rc = hiprtcCompileProgram(prog, 4, opts);
    size_t ln = 0; hiprtcGetProgramLogSize(prog, &ln);
    std::string log(ln, 0); if (ln) hiprtcGetProgramLog(prog, &log[0]);
    printf("%s compile rc %d\n%s\n", what, static_cast<int>(rc), log.c_str());
    if (rc != HIPRTC_SUCCESS) return 4;
    size_t sz = 0; hiprtcGetCodeSize(prog, &sz);
    std::vector<char> code(sz); hiprtcGetCode(prog, code.data());
    std::ofstream(prefix + tag + ".co", std::ios::binary).write(code.data(), static_cast<std::streamsize>(sz));
    return 0;
  };
  auto averaged = [](FusedPlanD q) { q.measureAvg = 1; return q; };
  if (int rc = build(sort_scan(p, 4, 9), "_c3_fsum8", "C3 sort scan (SUM_FLOAT into 8 bytes)")) return rc;
  if (int rc = build(sort_scan(averaged(p), 4, 9), "_c3_avg", "C3 sort scan (AVG_FLOAT)")) return rc;
  if (int rc = build(sort_scan(t, 2, 9), "_trips_fsum8", "trips sort scan (SUM_FLOAT into 8 bytes)")) return rc;
  if (int rc = build(sort_scan(averaged(t), 2, 9), "_trips_avg", "trips sort scan (AVG_FLOAT)")) return rc;
  // the variant is a different source: the null bit travels in the row word, a null measure is not a zero
  if (source(sort_scan(averaged(p), 4, 9)) == source(sort_scan(p, 4, 9))) { puts("AVG_FLOAT must not share SUM_FLOAT's source"); return 20; }
  if (source(sort_scan(averaged(p), 4, 9)).find("0x80000000u") == std::string::npos) { puts("no null bit in the AVG source"); return 21; }
  if (source(sort_scan(p, 4, 9)).find("0x80000000u") != std::string::npos) { puts("the null bit leaks into the SUM source"); return 22; }
  {  // the conversions of avg_measure_float: integer columns (and column + constant) into Float64- and Int64-typed measures
    FusedPlanD i = averaged(p);
    i.measure.f = col(K_I32); i.measure.outKind = K_F32;
    if (int rc = build(sort_scan(i, 4, 9), "_c3_avg_i32", "C3 sort scan (AVG of an Int32 column)")) return rc;
    i.measure.f = col(K_U32); i.measure.f.arity = 2; i.measure.f.functor = Plus; i.measure.f.bkind = K_I32; i.measure.f.bbits = 5; i.measure.f.bok = 1;
    if (int rc = build(sort_scan(i, 4, 9), "_c3_avg_u32", "C3 sort scan (AVG of a Uint32 column + 5)")) return rc;
    i.measureDtype = Int64;
    if (int rc = build(sort_scan(i, 4, 9), "_c3_avg_u32_i64", "C3 sort scan (AVG into an Int64-typed measure)")) return rc;
    FusedPlanD fx = averaged(p);
    fx.measure.f.arity = 2; fx.measure.f.functor = Multiply; fx.measure.f.bkind = K_F32; fx.measure.f.bbits = 0x3fc00000u; fx.measure.f.bok = 1;
    if (int rc = build(sort_scan(fx, 4, 9), "_c3_avg_fexpr", "C3 sort scan (AVG of m * 1.5)")) return rc;
  }
  {  // declined: a constant AVG measure, a 4-byte AVG measure, and AVG on HashReduce's scans
    FusedPlanD c = averaged(p);
    c.numCols = 4; c.measure.col = -1;
    if (!source(sort_scan(c, 4, 9)).empty()) { puts("a constant AVG measure must be declined"); return 23; }
    FusedPlanD w4 = averaged(p);
    w4.measureDtype = Float32; w4.measureWidth = 4;
    if (!source(sort_scan(w4, 4, 9)).empty()) { puts("a 4-byte AVG measure must be declined"); return 24; }
    if (!source(scan(averaged(p), 4, 9, false)).empty() || !source(scan(averaged(p), 4, 9, true)).empty()) { puts("HashReduce's scans must decline AVG"); return 25; }
  }
  return 0;
}
