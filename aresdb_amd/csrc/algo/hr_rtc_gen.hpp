// Source text of the run-time compiled scan / merge kernels (hr_rtc_gen.hip): the shape spec and the generators.
// Pure host code: no HIP runtime call, no lock, no environment variable.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>

#include "aggregate.hpp"
#include "hash_reduce_lds.hpp"

namespace ares {
namespace hr { struct Widen; }

// slots of Args::k (run-time constants): filter f -> f, dimension d -> kFusedFilters + d, the measure behind them; then the
// constants of the chain steps (FastOperands::chain) of dimension d and — last — of the measure, kMaxChainSteps each
constexpr int kNumRootConsts = kFusedFilters + kFusedDims + 1;
constexpr int kNumConsts = kNumRootConsts + kMaxChainSteps * (kFusedDims + 1);
constexpr int const_slot_filter(int f) { return f; }
constexpr int const_slot_dim(int d) { return kFusedFilters + d; }
constexpr int const_slot_measure() { return kFusedFilters + kFusedDims; }
constexpr int const_slot_dim_chain(int d) { return kNumRootConsts + kMaxChainSteps * d; }  // step k: + k
constexpr int const_slot_measure_chain() { return kNumRootConsts + kMaxChainSteps * kFusedDims; }

// The plan-sourced scans (16-byte line records, compact lines, TABLE mode, Sort + Reduce's 64-bit keys), the scans over
// materialised vectors (HashReduce, Sort + Reduce, HyperLogLog's pre-aggregation) and the two merges.
enum RtcKind : int32_t {
  RTC_SCAN_LINES16 = 1, RTC_SCAN_COMPACT, RTC_SCAN_TABLE, RTC_SCAN_SORT64, RTC_VECTOR_SCAN, RTC_SORT_VECTOR_SCAN, RTC_HLL_SCAN,
  RTC_MERGE, RTC_VECTOR_MERGE
};
// the kernel's entry point
const char *rtc_entry_name(int32_t kind);

// What of a FusedExpr is text.  bbits is kept only where it is a literal (divLike: the compiler strength-reduces the
// division); every other constant travels in Args::k.  The same holds for every step of a constant chain.
struct RtcStep {
  int32_t functor, I, divLike;
  uint32_t bbits;
};
struct RtcExpr {
  int32_t col, outKind, akind, arity, functor, I, rk, bkind;
  uint32_t bbits, bok;
  int32_t divLike;
  int32_t chainN;  // steps applied to the column's value before the functor (0: none)
  RtcStep chain[kMaxChainSteps];
};

// A kernel's SHAPE: everything its generator reads, and nothing else — the generators see no FusedPlanD, so the text cannot
// depend on something the cache key lacks.  Made by rtc_spec_*, which zero it first and leave at zero what the kind's
// generator does not read (pointers and bit offsets never enter); compared and hashed as bytes.
struct RtcSpec {
  uint64_t identity;     // the measure transform's (a literal of 4-byte measures)
  uint64_t aggIdentity;  // AggSpec (TABLE scan and merges)
  int32_t kind, nd, partBits, numCols, numFilters;
  uint32_t nullMask;     // column slots with a validity bitmap
  int32_t step[kFusedCols];     // bytes per stored value of a column slot
  int32_t dimWidth[kFusedDims];  // bytes of a dimension's slot in the dimension vector
  RtcExpr filters[kFusedFilters], dims[kFusedDims], measure;
  int32_t measureDtype, measureWidth, measureAvg;
  int32_t aggVtype, aggOp, aggWidth;
  int32_t widenMode, widenRk, widenDtype;  // hr::Widen (TABLE scan and plan merge)
  int32_t compact, regionA, image;         // merges (generate_merge)
  int32_t vectorVW;                        // bytes of a measure of the vector-sourced scan and merge
  int32_t phases;                          // ARES_HR_PHASES (phases_enabled(), read by the makers)
  int32_t constMeasure;                    // Sort + Reduce: no measure column, the records carry Args::k's measure slot
  int32_t reserved;                        // (zero: the struct has no padding)
};
static_assert(std::has_unique_object_representations<RtcSpec>::value, "compared and hashed as bytes: no padding");
inline bool operator==(const RtcSpec &a, const RtcSpec &b) { return memcmp(&a, &b, sizeof(a)) == 0; }
inline bool operator!=(const RtcSpec &a, const RtcSpec &b) { return !(a == b); }
// ARES_HR_PHASES=1 (diagnostics, read once — by hr_rtc.hip, which defines it): the generated kernels and the Sort + Reduce
// merges time-stamp their phases.  The makers store it in the spec: a different source text, so a separate cache entry.
bool phases_enabled();

// DIRECT-mode scan of `plan` (every surviving row becomes a record in the workgroup's private stream of its
// partition): `compact` = 8-byte records in compact lines (hr::Workspace::lineRecords == 14, ws.chunkRows set),
// otherwise 16-byte records in lines of 8.
RtcSpec rtc_spec_scan(const FusedPlanD &plan, int nd, int partBits, bool compact);
// The scan of the fused Sort + Reduce path (sort_reduce_fused.hip): like the DIRECT scan with 16-byte line records, but keyed
// by lo64(murmur3_x64_128) of the packed row — records {row, hash >> 32, carried measure, (u32)hash}, partition = top bits of
// the 64-bit hash.  plan.measure.col < 0: constant measure (the records carry plan.measure.f.bbits).
RtcSpec rtc_spec_sort_scan(const FusedPlanD &plan, int nd, int partBits);
// TABLE-mode scan of `plan` (low cardinality): LDS aggregation per workgroup, one record per group into region A
// (what hr::flush_table writes), rtc_scan_grid(length) workgroups; the generic merge reads it.
RtcSpec rtc_spec_table_scan(const FusedPlanD &plan, int nd, int partBits, const AggSpec &a, const hr::Widen &w);
// The DIRECT scan over rows of a dimension vector of `nd` 4-byte dimensions and a measure vector of `vw`-byte values
// (HashReduce on materialised vectors); 16-byte records carry the whole value.
RtcSpec rtc_spec_vector_scan(int nd, int vw, int partBits);
// The Sort + Reduce scan over a materialised dimension vector of `nd` dimensions (widths: 16 / 8 / 4 / 2 / 1 bytes in vector
// order — a layout sort_vector_layout_supported admits —, null = all four bytes) and a measure vector of 4-byte values
// (Sort + Reduce after joins or generic expressions): the same records, the value carried whole; the level-1 partition is the
// hash's top partBits bits or — spread — the scrambled low partBits bits of its top totalPartBits bits (sort_reduce_fused.hip)
RtcSpec rtc_spec_sort_vector_scan(int nd, const int *widths, int partBits);
// HyperLogLog's pre-aggregation scan (hll.hip) over a batch's dimension rows (same layouts) and 4-byte hll values:
// records {rowBase + entry, key >> 32, hll value, (u32)key} with key = (row hash & ~0xFFFF) | (value & 0x3FFF), in the stream of
// the partition that the top partBits (1 .. 9) bits of a scramble of the whole key select.
RtcSpec rtc_spec_hll_scan(int nd, const int *widths, int partBits);
// The specialised merge for what the DIRECT scans produce (line records in region B, previous groups in their
// partition-grouped ranges or none, one round over the whole hash range).  It raises outCount[3] when a
// partition holds more groups than one LDS table: the caller then runs the generic merge.
// regionA: the records come from region A as well (TABLE-mode scans) — the merge of narrow plans' low-cardinality batches.
// image: 0 = none; 1 = the merge also leaves the partition's LDS table in HBM ("table image": keys, each group's output
// position, values — 128 KB per partition); 2 = the merge STARTS from the previous call's image, emits the dimension rows of
// new groups only (appended: a group keeps its position) and writes the image again — the measure vector stays unwritten.
RtcSpec rtc_spec_merge(const FusedPlanD &plan, int nd, int partBits, const AggSpec &a, const hr::Widen &w, bool compact = false,
                       bool regionA = false, int image = 0);
// ... and for what the vector-sourced scan produces (launched with an empty plan: every row, old or new, is a row of the
// input vectors passed as prevDims / prevValues)
RtcSpec rtc_spec_vector_merge(int nd, int vw, int partBits, const AggSpec &a);

// the kernel's source (empty = a shape outside the supported ones: the caller keeps the generic kernel)
std::string rtc_source(const RtcSpec &s);

}  // namespace ares
