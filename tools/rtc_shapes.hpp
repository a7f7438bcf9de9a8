// What rtc_check.cpp and rtc_check_avg.cpp share: a Shape holds the inputs of one rtc_spec_* maker, so that the tools can name
// a source, and check_specs can perturb those inputs one field at a time and compare specs with sources.
#pragma once

#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "hash_reduce_lds.hpp"
#include "hr_kernels.hpp"
#include "hr_rtc_gen.hpp"

namespace rtc_shapes {
using namespace ares;

inline FastOperands col(int akind) {
  FastOperands f;
  memset(&f, 0, sizeof(f));
  f.akind = akind; f.arity = 1; f.functor = Noop; f.I = akind; f.rk = akind; f.bkind = akind;
  return f;
}

// C3: dims [Floor(ts, 3600), d1, d2, d3], filter d1 < 90, a Float32 measure column into an 8-byte Float64-typed measure
inline FusedPlanD c3_plan() {
  FusedPlanD p;
  memset(&p, 0, sizeof(p));
  p.numCols = 5;
  for (int c = 0; c < 5; c++) { p.cols[c].vals = reinterpret_cast<const uint32_t *>(0x1000); p.cols[c].nulls = reinterpret_cast<const uint8_t *>(0x2000); }
  p.numFilters = 1;
  p.filters[0].f = col(K_U32); p.filters[0].f.arity = 2; p.filters[0].f.functor = LessThan; p.filters[0].f.bkind = K_I32;
  p.filters[0].f.bbits = 90; p.filters[0].f.bok = 1; p.filters[0].col = 1; p.filters[0].outKind = K_BOOL;
  p.dims[0].f = col(K_U32); p.dims[0].f.arity = 2; p.dims[0].f.functor = Floor; p.dims[0].f.bkind = K_I32; p.dims[0].f.bbits = 3600;
  p.dims[0].f.bok = 1; p.dims[0].f.divLike = 1; p.dims[0].col = 0; p.dims[0].outKind = K_U32;
  for (int d = 1; d < 4; d++) { p.dims[d].f = col(K_U32); p.dims[d].col = d; p.dims[d].outKind = K_U32; }
  p.measure.f = col(K_F32); p.measure.col = 4; p.measure.outKind = K_F32;
  p.measureDtype = Float64; p.measureWidth = 8; p.identity = 0;
  return p;
}

struct Shape {
  RtcKind kind;
  FusedPlanD plan;
  int nd, partBits;
  AggSpec a;
  hr::Widen w;
  bool compact, regionA;
  int image, vw;
  bool haveWidths;
  int widths[kFusedDims];
};
inline Shape shape_of(RtcKind kind, int nd, int partBits) {
  Shape s;
  memset(&s, 0, sizeof(s));
  s.kind = kind; s.nd = nd; s.partBits = partBits;
  return s;
}
inline Shape scan(const FusedPlanD &p, int nd, int pb, bool compact) {
  Shape s = shape_of(compact ? RTC_SCAN_COMPACT : RTC_SCAN_LINES16, nd, pb);
  s.plan = p;
  return s;
}
inline Shape sort_scan(const FusedPlanD &p, int nd, int pb) {
  Shape s = shape_of(RTC_SCAN_SORT64, nd, pb);
  s.plan = p;
  return s;
}
inline Shape table_scan(const FusedPlanD &p, int nd, int pb, const AggSpec &a, const hr::Widen &w) {
  Shape s = shape_of(RTC_SCAN_TABLE, nd, pb);
  s.plan = p; s.a = a; s.w = w;
  return s;
}
inline Shape merge(const FusedPlanD &p, int nd, int pb, const AggSpec &a, const hr::Widen &w, bool compact, bool regionA = false, int image = 0) {
  Shape s = shape_of(RTC_MERGE, nd, pb);
  s.plan = p; s.a = a; s.w = w; s.compact = compact; s.regionA = regionA; s.image = image;
  return s;
}
inline Shape vector_scan(RtcKind kind, int nd, const int *widths, int vw, int pb) {  // RTC_VECTOR_SCAN, RTC_SORT_VECTOR_SCAN, RTC_HLL_SCAN
  Shape s = shape_of(kind, nd, pb);
  s.vw = vw; s.haveWidths = widths != nullptr;
  for (int d = 0; widths && d < nd && d < kFusedDims; d++) s.widths[d] = widths[d];
  return s;
}
inline Shape vector_merge(int nd, int vw, int pb, const AggSpec &a) {
  Shape s = shape_of(RTC_VECTOR_MERGE, nd, pb);
  s.vw = vw; s.a = a;
  return s;
}
inline RtcSpec spec(const Shape &s) {
  switch (s.kind) {
    case RTC_SCAN_LINES16: case RTC_SCAN_COMPACT: return rtc_spec_scan(s.plan, s.nd, s.partBits, s.kind == RTC_SCAN_COMPACT);
    case RTC_SCAN_TABLE: return rtc_spec_table_scan(s.plan, s.nd, s.partBits, s.a, s.w);
    case RTC_SCAN_SORT64: return rtc_spec_sort_scan(s.plan, s.nd, s.partBits);
    case RTC_VECTOR_SCAN: return rtc_spec_vector_scan(s.nd, s.vw, s.partBits);
    case RTC_SORT_VECTOR_SCAN: return rtc_spec_sort_vector_scan(s.nd, s.haveWidths ? s.widths : nullptr, s.partBits);
    case RTC_HLL_SCAN: return rtc_spec_hll_scan(s.nd, s.haveWidths ? s.widths : nullptr, s.partBits);
    case RTC_MERGE: return rtc_spec_merge(s.plan, s.nd, s.partBits, s.a, s.w, s.compact, s.regionA, s.image);
    default: return rtc_spec_vector_merge(s.nd, s.vw, s.partBits, s.a);
  }
}
inline std::string source(const Shape &s) { return rtc_source(spec(s)); }

// ---- spec versus source ---------------------------------------------------------------------------------------------
// Every input of a maker, perturbed one at a time.  A source that changes without its spec changing would hand one query
// another query's kernel: never allowed.  A spec that changes without its source changing only costs a cache miss, but each
// such (field, kind) is listed below with its reason, and a pair that is not listed fails.
struct Perturbation {
  std::string field;
  std::function<void(Shape &)> apply;
};
inline void perturb_expr(std::vector<Perturbation> &out, const std::string &role, std::function<FusedExpr &(Shape &)> at) {
  auto add = [&](const char *field, std::function<void(FusedExpr &)> f) {
    out.push_back({role + "." + field, [at, f](Shape &s) { f(at(s)); }});
  };
  add("col", [](FusedExpr &e) { e.col += 1; });
  add("outKind", [](FusedExpr &e) { e.outKind = e.outKind == K_F32 ? K_U32 : K_F32; });
  add("akind", [](FusedExpr &e) { e.f.akind = e.f.akind == K_I32 ? K_U32 : K_I32; });
  add("arity", [](FusedExpr &e) { e.f.arity = e.f.arity == 1 ? 2 : 1; });
  add("functor", [](FusedExpr &e) { e.f.functor += 1; });
  add("I", [](FusedExpr &e) { e.f.I = e.f.I == K_F32 ? K_U32 : K_F32; });
  add("rk", [](FusedExpr &e) { e.f.rk = e.f.rk == K_F32 ? K_U32 : K_F32; });
  add("bkind", [](FusedExpr &e) { e.f.bkind = e.f.bkind == K_F32 ? K_U32 : K_F32; });
  add("bbits", [](FusedExpr &e) { e.f.bbits += 1; });
  add("bok", [](FusedExpr &e) { e.f.bok ^= 1u; });
  add("divLike", [](FusedExpr &e) { e.f.divLike ^= 1; });
  // the constant chain in front of the functor (FastOperands::chain): its length and its first step
  add("chain.n", [](FusedExpr &e) { e.f.chain.n = e.f.chain.n ? e.f.chain.n - 1 : 1; });
  add("chain.functor", [](FusedExpr &e) { e.f.chain.s[0].functor = e.f.chain.s[0].functor == Plus ? Minus : Plus; });
  add("chain.I", [](FusedExpr &e) { e.f.chain.s[0].I = e.f.chain.s[0].I == K_I32 ? K_U32 : K_I32; });
  add("chain.bbits", [](FusedExpr &e) { e.f.chain.s[0].bbits += 1; });
  add("chain.divLike", [](FusedExpr &e) { e.f.chain.s[0].divLike ^= 1; });
}
inline std::vector<Perturbation> perturbations(const Shape &base) {
  std::vector<Perturbation> out;
  const bool plan = base.kind <= RTC_SCAN_SORT64 || base.kind == RTC_MERGE;
  if (plan) {
    for (int k = 0; k < base.plan.numFilters; k++) perturb_expr(out, "filter", [k](Shape &s) -> FusedExpr & { return s.plan.filters[k]; });
    for (int d = 0; d < base.nd; d++) perturb_expr(out, "dim", [d](Shape &s) -> FusedExpr & { return s.plan.dims[d]; });
    perturb_expr(out, "measure", [](Shape &s) -> FusedExpr & { return s.plan.measure; });
    for (int c = 0; c < base.plan.numCols; c++) {
      out.push_back({"col.nulls", [c](Shape &s) { s.plan.cols[c].nulls = s.plan.cols[c].nulls ? nullptr : reinterpret_cast<const uint8_t *>(0x2000); }});
      out.push_back({"col.step", [c](Shape &s) { s.plan.cols[c].step = fused_col_step(s.plan, c) == 4 ? 2 : 4; }});
    }
    for (int d = 0; d < base.nd; d++) out.push_back({"dimWidth", [d](Shape &s) { s.plan.dimWidth[d] = fused_dim_width(s.plan, d) == 4 ? 2 : 4; }});
    out.push_back({"numCols", [](Shape &s) { s.plan.numCols += s.plan.numCols < kFusedCols ? 1 : -1; }});
    out.push_back({"numFilters", [](Shape &s) { s.plan.numFilters += s.plan.numFilters < kFusedFilters ? 1 : -1; }});
    out.push_back({"measureDtype", [](Shape &s) { s.plan.measureDtype = s.plan.measureDtype == Float64 ? Int64 : Float64; }});
    out.push_back({"measureWidth", [](Shape &s) { s.plan.measureWidth = s.plan.measureWidth == 8 ? 4 : 8; }});
    out.push_back({"identity", [](Shape &s) { s.plan.identity ^= 1u; }});
    out.push_back({"measureAvg", [](Shape &s) { s.plan.measureAvg ^= 1; }});
  } else {
    out.push_back({"vw", [](Shape &s) { s.vw = s.vw == 4 ? 8 : 4; }});
    out.push_back({"widths", [](Shape &s) {
                     if (!s.haveWidths) for (int d = 0; d < kFusedDims; d++) s.widths[d] = 4;
                     s.haveWidths = true;
                     s.widths[s.nd - 1] = s.widths[s.nd - 1] == 4 ? 2 : 4;
                   }});
  }
  out.push_back({"nd", [](Shape &s) { s.nd += s.nd < kFusedDims ? 1 : -1; }});
  out.push_back({"partBits", [](Shape &s) { s.partBits += s.partBits < 9 ? 1 : -1; }});
  out.push_back({"agg.vtype", [](Shape &s) { s.a.vtype = s.a.vtype == V_U32 ? V_I32 : V_U32; }});
  out.push_back({"agg.op", [](Shape &s) { s.a.op = s.a.op == OP_SUM ? OP_MIN : OP_SUM; }});
  out.push_back({"agg.width", [](Shape &s) { s.a.width = s.a.width == 8 ? 4 : 8; }});
  out.push_back({"agg.identity", [](Shape &s) { s.a.identity ^= 1u; }});
  out.push_back({"widen.mode", [](Shape &s) { s.w.mode ^= 1; }});
  out.push_back({"widen.rk", [](Shape &s) { s.w.rk = s.w.rk == K_F32 ? K_I32 : K_F32; }});
  out.push_back({"widen.dtype", [](Shape &s) { s.w.dtype = s.w.dtype == Float64 ? Int64 : Float64; }});
  out.push_back({"compact", [](Shape &s) { s.compact = !s.compact; }});
  out.push_back({"regionA", [](Shape &s) { s.regionA = !s.regionA; }});
  out.push_back({"image", [](Shape &s) { s.image = (s.image + 1) % 3; }});
  return out;
}

inline const char *kind_name(int kind) {
  static const char *names[] = {"", "scan16", "compact", "table", "sort64", "vector", "sort_vector", "hll", "merge", "vector_merge"};
  return names[kind];
}

// (field, kind or "*") -> why the spec may change although the text does not.  Everything else must change both or neither.
inline const std::map<std::string, std::string> &over_specified() {
  static const std::map<std::string, std::string> m = {
      {"filter.akind/*", "Int32 and Uint32 columns of 4 bytes read alike: the kinds differ in how a 1- or 2-byte column is widened"},
      {"dim.akind/*", "as filter.akind"},
      {"measure.akind/*", "as filter.akind"},
      {"dim.functor/*", "a division-like functor that is neither Divide nor Mod is written as Floor"},
      {"measureDtype/sort64", "a 4-byte measure's dtype is read as Int32, Uint32 or anything else (a float)"},
      {"dim.chain.I/*", "a step's kind is read where the step divides: Plus / Minus / Multiply wrap alike in both"},
      {"measure.chain.I/*", "as dim.chain.I"},
      {"measure.rk/*", "read for 4-byte measures, AVG and float arithmetic; an 8-byte sum of a bare column carries the stored bits"},
  };
  return m;
}

// 0, or the number of violations (printed)
inline int check_specs(const std::vector<Shape> &shapes) {
  int bad = 0;
  size_t pairs = 0;
  for (const Shape &base : shapes) {
    const RtcSpec s0 = spec(base);
    const std::string t0 = rtc_source(s0);
    for (const Perturbation &p : perturbations(base)) {
      Shape other = base;
      p.apply(other);
      const RtcSpec s1 = spec(other);
      const std::string t1 = rtc_source(s1);
      pairs++;
      if (t0 != t1 && s0 == s1) {
        printf("WRONG KERNEL: %s of a %s shape changes the source and not the spec\n", p.field.c_str(), kind_name(base.kind));
        bad++;
      }
      if (t0 == t1 && s0 != s1 && !over_specified().count(p.field + "/" + kind_name(base.kind)) && !over_specified().count(p.field + "/*")) {
        printf("over-specified: %s of a %s shape changes the spec and not the source\n", p.field.c_str(), kind_name(base.kind));
        bad++;
      }
    }
  }
  printf("spec versus source: %zu shapes, %zu perturbations, %d violations\n", shapes.size(), pairs, bad);
  return bad;
}

}  // namespace rtc_shapes
