// The scans and the merge generated for plans whose time dimension is a constant chain (FastOperands::chain) — the trips shape
// grouped by [chain, city_id Uint16] — next to their chain-free siblings (a bare column, Floor(request_at, 3600)), compiled for
// gfx950 (no GPU needed):
//   tools/bin/rtc_check_chain [out-prefix]   writes <prefix>_<tag>.hip and <prefix>_<tag>.co
// Chains a generator must not answer (a float step, a null constant, a functor outside the six) return an error, and so does a
// source that does not follow its spec.  Links against aresdb_amd/lib/libalgorithm.so like rtc_check.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "rtc_shapes.hpp"

using namespace rtc_shapes;

static FastStep step(int functor, uint32_t bbits) {
  FastStep st;
  memset(&st, 0, sizeof(st));
  st.functor = static_cast<uint8_t>(functor); st.I = K_I32; st.rk = K_I32; st.sk = K_I32; st.bkind = K_I32; st.bbits = bbits;
  st.divLike = functor == Divide || functor == Mod || functor == Floor;
  return st;
}
// dims[0] = ((request_at steps...) root c): a Uint32 column, signed nodes (an integer literal is signed)
static FusedPlanD chained(FusedPlanD t, std::vector<FastStep> steps, int root, uint32_t c) {
  FastOperands &f = t.dims[0].f;
  f = col(K_U32);
  f.arity = 2; f.functor = root; f.I = K_I32; f.rk = K_I32; f.bkind = K_I32; f.bbits = c; f.bok = 1;
  f.divLike = root == Divide || root == Mod || root == Floor;
  f.chain.n = static_cast<int>(steps.size());
  for (size_t k = 0; k < steps.size(); k++) f.chain.s[k] = steps[k];
  return t;
}

int main(int argc, char **argv) {
  const FusedPlanD p = c3_plan();
  // trips: dims [time dimension Uint32, city_id Uint16 -> 2-byte slot], fare Float32, filters request_at >= / <, status == k (Uint8)
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
  FusedPlanD bare = t;  // the chain-free siblings: the bare column, and Floor(request_at, 3600)
  bare.dims[0].f = col(K_U32);
  FusedPlanD floor1 = t;  // (over an integer literal the node is signed, as the calls bind it: common_kind)
  floor1.dims[0].f.I = K_I32; floor1.dims[0].f.rk = K_I32;
  const uint32_t off = static_cast<uint32_t>(-28800);
  const FusedPlanD zoneHour = chained(t, {step(Plus, off)}, Floor, 3600);                                         // Floor(Plus(ts, off), 3600)
  const FusedPlanD hourOfDay = chained(t, {step(Mod, 86400)}, Floor, 3600);                                       // Floor(Mod(ts, 86400), 3600)
  const FusedPlanD zoneTimeOfDay = chained(t, {step(Plus, off)}, Mod, 86400);                                     // Mod(Plus(ts, off), 86400)
  const FusedPlanD hourOfWeek = chained(t, {step(Minus, 345600), step(Mod, 604800)}, Floor, 3600);                // 3 nodes
  const FusedPlanD zoneHourOfWeek = chained(t, {step(Plus, off), step(Minus, 345600), step(Mod, 604800)}, Floor, 3600);  // 4 nodes

  const std::string prefix = argc > 1 ? argv[1] : "/tmp/chain_rtc";
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
  const AggSpec sum = make_agg_spec(AGGR_SUM_FLOAT, 8);
  const hr::Widen widen{1, K_F32, Float64};
  struct Named { const char *tag; const FusedPlanD *plan; };
  const Named plans[] = {{"bare", &bare}, {"floor", &floor1}, {"zone_hour", &zoneHour}, {"hour_of_day", &hourOfDay},
                         {"zone_time_of_day", &zoneTimeOfDay}, {"hour_of_week", &hourOfWeek}, {"zone_hour_of_week", &zoneHourOfWeek}};
  std::vector<Shape> all;
  for (const Named &n : plans) {
    const std::string tag = n.tag;
    const Shape shapes[] = {scan(*n.plan, 2, 9, false), scan(*n.plan, 2, 9, true), table_scan(*n.plan, 2, 9, sum, widen), sort_scan(*n.plan, 2, 9)};
    const char *kinds[] = {"lines16", "compact", "table", "sort64"};
    for (int k = 0; k < 4; k++) {
      if (int rc = build(shapes[k], "_" + tag + "_" + kinds[k], (tag + " " + kinds[k] + " scan").c_str())) return rc;
      all.push_back(shapes[k]);
    }
    if (int rc = build(merge(*n.plan, 2, 9, sum, widen, true), "_" + tag + "_merge", (tag + " merge").c_str())) return rc;
    all.push_back(merge(*n.plan, 2, 9, sum, widen, true));
  }
  // One compiled kernel serves every UTC offset: the Plus constant is an argument, not text ...
  if (source(scan(zoneHour, 2, 9, true)) != source(scan(chained(t, {step(Plus, 19800)}, Floor, 3600), 2, 9, true))) { puts("the offset must not be text"); return 20; }
  // ... a divisor is text
  if (source(scan(hourOfDay, 2, 9, true)) == source(scan(chained(t, {step(Mod, 604800)}, Floor, 3600), 2, 9, true))) { puts("a divisor must be a literal"); return 21; }
  if (source(scan(zoneHour, 2, 9, true)) == source(scan(floor1, 2, 9, true))) { puts("a chain must not share its root's source"); return 22; }
  {  // declined: a float step, a float root over a chain, a null constant, a functor outside the six, more steps than the shape holds
    FastStep fl = step(Plus, 0x3f800000u);
    fl.I = K_F32;
    if (!source(scan(chained(t, {fl}, Floor, 3600), 2, 9, true)).empty()) { puts("a float chain must be declined"); return 23; }
    FusedPlanD froot = zoneHour;
    froot.dims[0].f.I = K_F32; froot.dims[0].f.bkind = K_F32; froot.dims[0].f.divLike = 0; froot.dims[0].f.functor = Divide;
    if (!source(scan(froot, 2, 9, true)).empty()) { puts("a float root over a chain must be declined"); return 24; }
    FusedPlanD nullc = zoneHour;
    nullc.dims[0].f.bok = 0;
    if (!source(scan(nullc, 2, 9, true)).empty() || !source(sort_scan(nullc, 2, 9)).empty()) { puts("a null-constant chain must be declined"); return 25; }
    FastStep bw = step(BitwiseAnd, 7);
    if (!source(scan(chained(t, {bw}, Floor, 3600), 2, 9, true)).empty()) { puts("a bitwise step must be declined"); return 26; }
    FusedPlanD longer = zoneHourOfWeek;
    longer.dims[0].f.chain.n = kMaxChainSteps + 1;
    if (!source(scan(longer, 2, 9, true)).empty() || !source(merge(longer, 2, 9, sum, widen, true)).empty()) { puts("a chain longer than the shape holds must be declined"); return 27; }
  }
  return check_specs(all) ? 30 : 0;
}
