// Source text of the per-plan specialised scan / merge kernels of the fused HashReduce, compiled at run time with hiprtc
// (hr_rtc.hip: the hiprtc binding, the caches and the launches).
//
// The generic hr_fused_scan_kernel (hr_kernels.hpp) interprets the plan: operation codes, kinds and
// constants arrive as kernel arguments and every expression is dispatched per quad.  That costs
// ~210 VALU + ~80 SALU instructions per row, 266 KB of code and several hundred spilled SGPRs — the
// kernel is bound by instruction issue and instruction fetch, not by HBM.  Here the host writes the
// plan's SHAPE out as straight-line code and hiprtc compiles it for the device's architecture.
//
// What is a literal and what is an argument.  Literals (they select instructions): functors, kinds, null
// mask, column slots, aggregate, widening, partition bits, record format — and DIVISORS (the time bucket
// `Floor(ts, 3600)`: the compiler strength-reduces the division; DESIGN.md 3 measured that this is where the
// gain of specialisation is).  Kernel ARGUMENTS: every comparison constant and every + / - / x constant
// (`Args::k`).  AresDB queries carry per-query `from` / `to` time-filter constants
// (query/common/time_filter.go:371-397): a new time range runs the kernel that is already loaded.
//
// Three scans are generated:
//   * DIRECT, compact lines — high-cardinality queries (more groups than an LDS table holds): every surviving
//     row becomes an 8-byte record {carried measure, (hash << partBits) | row bits}, counting-sorted by
//     partition in LDS; only whole aligned 128-byte lines of 14 records + two 8-byte headers (the low row
//     bits) leave the CU.  9.14 bytes per record instead of 16: the record round trip is what bounds this
//     query shape (the scan moved 1.72x its algorithmic bytes with 16-byte records).
//   * DIRECT, 16-byte records {row, hash, value lo, value hi} in lines of 8 — the vector-sourced scan
//     (HashReduce on materialised dimension / measure vectors, 8-byte values) and batches whose per-workgroup
//     chunk does not fit the compact row field.
//   * TABLE — low-cardinality queries: each workgroup aggregates its rows in an LDS hash table without a
//     barrier in the loop and emits one record per group at the end (region A, read by the generic merge);
//     rows that find the table full spill as single records.
// Write path facts behind the DIRECT kernels (tools/ubench_scatter.hip, profiles/r2_ubench_write_path*.txt):
// reading and hashing the columns runs at 6 TB/s, but a CU retires only one scattered small store per ~4.5
// cycles and HBM write time follows the number of 64-byte write requests — hence the LDS sort and whole lines.
//
// Supported shapes (everything else: generic kernel) — exactly the fast paths of eval_quad /
// compare_tile in fast_eval.hpp, so results are bit-identical:
//   * columns of kind int32 / uint32 / float32 (modes 1 and 2);
//   * dimension / measure: a bare column, or an integer column (Divide | Mod | Floor | Plus | Minus |
//     Multiply) a valid integer constant, stored without a value conversion;
//   * ... or a constant CHAIN over an integer column (FastOperands::chain, apply_chain): up to three such steps in front of
//     that functor, emitted as straight-line code — their + / - / x constants in Args::k, their divisors literals —, the null
//     row zeroed once, behind the functor;
//   * filters: a column compared (==, !=, <, <=, >, >=) with a valid constant in the common kind;
//   * the measure carried as 4 bytes (fused_carry).
#include <cstdio>
#include <functional>
#include <sstream>
#include <string>
#include <vector>

#include "hr_kernels.hpp"
#include "hr_rtc_gen.hpp"

namespace ares {

namespace {

bool int_kind(int k) { return k == K_I32 || k == K_U32; }
bool col_kind(int k) { return k == K_I32 || k == K_U32 || k == K_F32; }

std::string hex(uint32_t v) {
  char b[16];
  snprintf(b, sizeof(b), "0x%08xu", v);
  return b;
}

std::string const_name(int slot) { return "a.k[" + std::to_string(slot) + "]"; }

// `r` = `v` (Divide | Mod | Floor) the literal y in kind I, null handling aside: fast_divmod's rules (d = 0 -> q = r = 0; d = 1 ->
// q = x, r = 0), the signed forms truncating on magnitudes.  Declares ax, q, m, sq, sm [, xneg]: the caller opens a scope.
void gen_divlike(std::ostringstream &o, int functor, int I, uint32_t y, const char *v, const char *r) {
  const bool sgn = I == K_I32;
  const uint32_t mag = (sgn && static_cast<int32_t>(y) < 0) ? 0u - y : y;
  const bool yneg = sgn && static_cast<int32_t>(y) < 0;
  if (sgn) o << "        const bool xneg = (i32)" << v << " < 0; const u32 ax = xneg ? 0u - " << v << " : " << v << ";\n";
  else o << "        const u32 ax = " << v << ";\n";
  if (mag == 0) o << "        const u32 q = 0u, m = 0u;\n";
  else if (mag == 1) o << "        const u32 q = ax, m = 0u;\n";
  else o << "        const u32 q = ax / " << hex(mag) << ", m = ax % " << hex(mag) << ";\n";
  if (sgn) {
    o << "        const u32 sq = (xneg != " << (yneg ? "true" : "false") << ") ? 0u - q : q;\n";
    o << "        const u32 sm = xneg ? 0u - m : m;\n";
  } else {
    o << "        const u32 sq = q, sm = m;\n";
  }
  o << "        " << r << " = " << (functor == Divide ? "sq" : functor == Mod ? "sm" : std::string(v) + " - sm") << ";\n";
}

// value expression of one element: writes `r` (result bits) given `v` (stored bits) and `okb` (0/1);
// `kc` names the run-time constant of the expression.  Returns false when the shape is outside the fast
// paths of eval_quad.
// floatArith (the Sort + Reduce scan's measure only): a float column combined with a float constant by Plus / Minus /
// Multiply (fare * 1.5) — binary32's float branch: one rounding, null -> bits 0.
bool gen_root_value(const RtcExpr &f, std::ostringstream &o, const char *v, const char *okb, const char *r, const std::string &kc,
                    bool floatArith) {
  if (!col_kind(f.akind)) return false;
  const bool intKinds = f.akind != K_F32 && f.I != K_F32 && f.akind != K_BOOL;
  if (f.arity == 1) {
    if (!(f.akind == f.I || intKinds)) return false;
    o << "      " << r << " = " << v << ";\n";  // a null bare column keeps its stored bits (functor.hpp:345-351)
    return true;
  }
  if (floatArith && f.arity == 2 && f.akind == K_F32 && f.I == K_F32 && f.bkind == K_F32 && f.rk == K_F32 && f.bok && !f.divLike &&
      (f.functor == Plus || f.functor == Minus || f.functor == Multiply)) {
    o << "      " << r << " = " << okb << " ? __float_as_uint(__uint_as_float(" << v << ")"
      << (f.functor == Plus ? " + " : f.functor == Minus ? " - " : " * ") << "__uint_as_float(" << kc << ")) : 0u;\n";
    return true;
  }
  if (f.arity != 2 || !intKinds || !int_kind(f.I) || !int_kind(f.bkind) || !f.bok) return false;
  if (f.divLike) {  // the divisor is a literal: the compiler turns the division into multiply + shift
    o << "      {\n";
    gen_divlike(o, f.functor, f.I, f.bbits, v, r);  // cvt32 between the integer kinds keeps the bits
    o << "        if (!" << okb << ") " << r << " = 0u;\n      }\n";
    return true;
  }
  if (f.functor == Plus || f.functor == Minus || f.functor == Multiply) {
    o << "      " << r << " = " << okb << " ? (" << v << (f.functor == Plus ? " + " : f.functor == Minus ? " - " : " * ") << kc
      << ") : 0u;\n";
    return true;
  }
  return false;
}

// ... of an expression with a constant chain in front of its functor (FastOperands::chain): the steps run on the stored bits
// into `ch`, the functor reads `ch` and zeroes a null row once, at the end (apply_chain + eval_quad of fast_eval.hpp).
// chainSlot: Args::k slot of the first step's constant (a Plus / Minus / Multiply constant is an argument, a divisor a literal).
bool gen_value(const RtcExpr &f, std::ostringstream &o, const char *v, const char *okb, const char *r, const std::string &kc, int chainSlot,
               bool floatArith = false) {
  if (f.chainN == 0) return gen_root_value(f, o, v, okb, r, kc, floatArith);
  if (f.chainN < 0 || f.chainN > kMaxChainSteps || chainSlot < 0 || !int_kind(f.akind) || f.arity != 2 || !int_kind(f.I) || !int_kind(f.bkind) ||
      !f.bok)
    return false;
  o << "      {\n      u32 ch = " << v << ";\n";
  for (int k = 0; k < f.chainN; k++) {
    const RtcStep &st = f.chain[k];
    if (!int_kind(st.I)) return false;
    if (st.divLike) {
      if (!(st.functor == Divide || st.functor == Mod || st.functor == Floor)) return false;
      o << "      {\n        u32 t;\n";
      gen_divlike(o, st.functor, st.I, st.bbits, "ch", "t");
      o << "        ch = t;\n      }\n";
    } else if (st.functor == Plus || st.functor == Minus || st.functor == Multiply) {
      o << "      ch = ch " << (st.functor == Plus ? "+" : st.functor == Minus ? "-" : "*") << " " << const_name(chainSlot + k) << ";\n";
    } else {
      return false;
    }
  }
  if (!gen_root_value(f, o, "ch", okb, r, kc, false)) return false;
  o << "      }\n";
  return true;
}

// keep bit of one element for one filter; the constant (converted to the common kind by the host) is `kc`
bool gen_compare(const RtcExpr &f, std::ostringstream &o, const char *v, const char *okb, const char *keep, const std::string &kc) {
  if (!col_kind(f.akind) || f.arity != 2) return false;
  const bool sameBits = f.akind == f.I || (f.akind != K_F32 && f.I != K_F32 && f.akind != K_BOOL);
  if (!sameBits || !f.bok) return false;
  if (f.functor < Equal || f.functor > GreaterThanOrEqual) return false;
  if (!(f.I == K_F32 || f.I == K_I32 || f.I == K_U32)) return false;
  const char *op = f.functor == Equal ? "==" : f.functor == NotEqual ? "!=" : f.functor == LessThan ? "<"
                   : f.functor == LessThanOrEqual ? "<=" : f.functor == GreaterThan ? ">" : ">=";
  if (f.I == K_F32) o << "      " << keep << " &= (" << okb << " && (__uint_as_float(" << v << ") " << op << " __uint_as_float(" << kc << "))) ? 1u : 0u;\n";
  else if (f.I == K_I32) o << "      " << keep << " &= (" << okb << " && ((i32)" << v << " " << op << " (i32)" << kc << ")) ? 1u : 0u;\n";
  else o << "      " << keep << " &= (" << okb << " && (" << v << " " << op << " " << kc << ")) ? 1u : 0u;\n";
  return true;
}

bool plain_store(int rk, int outKind) { return rk == outKind || (rk != K_F32 && outKind != K_F32 && rk != K_BOOL); }

std::string args_text() {
  std::ostringstream o;
  o << "struct Args { const u32 *vals[" << kFusedCols << "]; const u8 *nulls[" << kFusedCols << "]; u32 *recB; u32 *countsB; u32 *overflow; u64 *phases; u32 *hostCount;\n"
       "              uint4 *recA; u32 *cursorsA; u64 capA; u32 bitOff[" << kFusedCols << "]; u32 rowBase; int length; u32 capB; u32 chunkTiles;\n"
       "              u32 k[" << kNumConsts << "]; u32 pad; };\n";
  return o.str();
}

// times5: murmur's h * 5 + c.  The compiler folds `h * 5u + c` into one v_mad_u64_u32 (a 64-bit, slow-rate multiply-add); a
// shift-add and an add are two full-rate instructions (measured in profiles/r3_experiments.md).
const char *kPrelude =
    "__device__ __forceinline__ unsigned int times5(unsigned int r) { unsigned int t; asm(\"v_lshl_add_u32 %0, %1, 2, %1\" : \"=v\"(t) : \"v\"(r)); return t; }\n"
    "#define TIMES5(r) times5(r)\n"
    "typedef unsigned int u32; typedef unsigned long long u64; typedef unsigned char u8; typedef unsigned short u16; typedef int i32; typedef long long i64;\n"
    "struct __attribute__((packed, aligned(1))) PU32x4 { u32 v[4]; };\n"
    "struct __attribute__((packed, aligned(1))) PU32 { u32 v; };\n"
    "struct __attribute__((packed, aligned(1))) PU16 { u16 v; };\n"
    "typedef u32 U4 __attribute__((ext_vector_type(4)));\n"
    "typedef U4 U4a __attribute__((aligned(4)));\n"
    "struct __attribute__((packed, aligned(1))) PU32x2 { u32 v[2]; };\n"
    "typedef u32 U2 __attribute__((ext_vector_type(2)));\n"
    "typedef U2 U2a __attribute__((aligned(2)));\n"
    "typedef u32 U1a __attribute__((aligned(1)));\n"
    "__device__ __forceinline__ u32 rotl(u32 x, int r) { return (x << r) | (x >> (32 - r)); }\n"
    "__device__ __forceinline__ u32 mix(u32 h, u32 k) { k *= 0xcc9e2d51u; k = rotl(k, 15) * 0x1b873593u; h ^= k; return TIMES5(rotl(h, 13)) + 0xe6546b64u; }\n";

void phase_macros(std::ostringstream &o, const RtcSpec &s) {
  if (s.phases)
    o << "#define PH_DECL u64 phT[8] = {0, 0, 0, 0, 0, 0, 0, 0}; u64 phLast = __builtin_readcyclecounter();\n"
         "#define PH(k) { const u64 now = __builtin_readcyclecounter(); phT[k] += now - phLast; phLast = now; }\n"
         "#define PH_OUT if (threadIdx.x == 0u) for (int k = 0; k < 8; k++) a.phases[(u64)blockIdx.x * 8u + k] = phT[k];\n";
  else
    o << "#define PH_DECL\n#define PH(k)\n#define PH_OUT\n";
}

// value of a carried measure (hr::widen_value)
bool gen_widen(std::ostringstream &o, const RtcSpec &s) {
  o << "__device__ __forceinline__ u64 widen(u32 raw) {\n";
  if (s.widenMode == 0) o << "  return raw;\n";
  else if (s.widenDtype == Float64)
    o << (s.widenRk == K_F32 ? "  return (u64)__double_as_longlong((double)__uint_as_float(raw));\n"
          : s.widenRk == K_I32 ? "  return (u64)__double_as_longlong((double)(i32)raw);\n"
                          : "  return (u64)__double_as_longlong((double)raw);\n");
  else
    o << (s.widenRk == K_F32 ? "  return (u64)(i64)__uint_as_float(raw);\n" : s.widenRk == K_I32 ? "  return (u64)(i64)(i32)raw;\n" : "  return (u64)(i64)raw;\n");
  o << "}\n";
  return true;
}

// the aggregate on an LDS slot (hr::lds_aggregate)
bool gen_agg(std::ostringstream &o, const RtcSpec &s) {
  o << "__device__ __forceinline__ void agg(u64 *slot, u64 bits) {\n";
  switch (s.aggVtype) {
    case V_F64: o << "  __hip_atomic_fetch_add(reinterpret_cast<double *>(slot), __longlong_as_double((long long)bits), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"; break;
    case V_U64: case V_I64: o << "  __hip_atomic_fetch_add(slot, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"; break;
    case V_F32: o << "  __hip_atomic_fetch_add(reinterpret_cast<float *>(slot), __uint_as_float((u32)bits), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"; break;
    case V_U32:
      o << "  __hip_atomic_fetch_" << (s.aggOp == OP_SUM ? "add" : s.aggOp == OP_MIN ? "min" : "max")
        << "(reinterpret_cast<u32 *>(slot), (u32)bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n";
      break;
    case V_I32:
      o << "  __hip_atomic_fetch_" << (s.aggOp == OP_SUM ? "add" : s.aggOp == OP_MIN ? "min" : "max")
        << "(reinterpret_cast<i32 *>(slot), (i32)(u32)bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n";
      break;
    default: return false;
  }
  o << "}\n";
  char ident[32];
  snprintf(ident, sizeof(ident), "0x%016llxull", static_cast<unsigned long long>(s.aggIdentity));
  o << "#define IDENT " << ident << "\n";
  return true;
}

// ---- DIRECT scan, 16-byte records in lines of 8 ------------------------------------------------------
// `Raw`, `load_full`, `load_tail` and `eval4(R, a, i0, hh, cv, cw, alive)` are already in `o`; `fourth` is the
// record's fourth word.  One 1024-lane workgroup per CU walks 4096-row tiles (tile = blockIdx + k * grid).
// Records are counting-sorted by partition in LDS and ONLY whole lines of 8 records leave the CU, each written
// by 8 adjacent lanes with one store; the < 8 records a partition has left over stay in LDS and go first in
// the next tile's lines.  Streams are private to the workgroup: no global atomics.
struct Lines16 {
  const char *fourth;                                              // the record's fourth word
  const char *part = "(PB ? hh[j] >> (32 - (PB ? PB : 1)) : 0u)";  // the partition of row j's hash (default: its top PB bits)
  const char *row = "a.rowBase + i0 + j";  // the record's first word (AVG_FLOAT's scan sets its top bit for a null measure: generate)
};
static void kernel_body_lines16(std::ostringstream &o, const RtcSpec &s, const Lines16 &rec) {
  const char *fourth = rec.fourth, *part = rec.part, *row = rec.row, *entry = rtc_entry_name(s.kind);
  phase_macros(o, s);
  o << "#define T 4096u\n"
       "__device__ __forceinline__ u32 lane_up(u32 v, u32 lane, u32 off) { return (u32)__builtin_amdgcn_ds_bpermute((int)((lane - off) << 2), (int)v); }\n"
       "extern \"C\" __global__ void __launch_bounds__(1024) " << entry << "(Args a) {\n"
       "  __shared__ uint4 sRec[T];\n"            // the tile's records, sorted by partition
       "  __shared__ uint4 sLeft[NP * 7u];\n"     // up to 7 records per partition waiting for a full line
       "  __shared__ u32 sCount[2][NP];\n"
       "  __shared__ u32 sStart[NP], sLeftN[NP], sCursor[NP];\n"
       "  __shared__ u32 sLines[(T + NP * 7u) / 8u + 1u];\n"
       "  __shared__ u32 sWave[16];\n"
       "  __shared__ u32 sTotalLines;\n"
       "  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;\n"
       "  for (u32 p = tid; p < NP; p += 1024u) { sCount[0][p] = 0u; sCount[1][p] = 0u; sLeftN[p] = 0u; sCursor[p] = 0u; }\n"
       "  __syncthreads();\n"
       "  uint4 *myB = reinterpret_cast<uint4 *>(a.recB) + (u64)blockIdx.x * NP * a.capB;\n"
       "  const u32 numTiles = ((u32)a.length + T - 1u) / T;\n"
       "  u32 tile = blockIdx.x, par = 0u;\n"
       "  Raw R;\n"
       "  PH_DECL\n"
       "  load_tile(R, a, tile * T + tid * 4u);\n"
       "  while (tile < numTiles) {\n"
       "    u32 i0 = tile * T + tid * 4u;\n"          // eval4p moves it to the first row the lane's registers hold
       "    u32 hh[4], cv[4], cw[4], alive[4], rank[4];\n"
       "    const u32 next = tile + gridDim.x;\n"
       "    eval4p(R, a, i0, hh, cv, cw, alive, next * T + tid * 4u);\n"
       "    u32 *cnt = sCount[par];\n"
       "#pragma unroll\n"
       "    for (int j = 0; j < 4; j++) {\n"
       "      rank[j] = 0u;\n"
       "      if (alive[j]) rank[j] = __hip_atomic_fetch_add(&cnt[" << part << "], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
       "    }\n"
       "    __syncthreads();\n"
       "    PH(0)\n"
       // exclusive scans of (new records, whole lines) per partition, packed in one word
       "    u32 myCount = 0u, myLeft = 0u;\n"
       "    if (tid < NP) { myCount = cnt[tid]; myLeft = sLeftN[tid]; }\n"
       "    const u32 myHave = myCount + myLeft, myLines = myHave >> 3;\n"
       "    const u32 packed = (myCount << 16) | myLines;\n"
       "    u32 incl = packed;\n"
       "#pragma unroll\n"
       "    for (u32 off = 1u; off < 64u; off <<= 1) { const u32 t = lane_up(incl, lane, off); if (lane >= off) incl += t; }\n"
       "    if (lane == 63u) sWave[wave] = incl;\n"
       "    __syncthreads();\n"
       "    u32 before = 0u;\n"
       "#pragma unroll\n"
       "    for (u32 w = 0u; w < (NP + 63u) / 64u; w++) { const u32 t = sWave[w]; before += w < wave ? t : 0u; }\n"
       "    const u32 excl = before + incl - packed;\n"
       "    const u32 myStart = excl >> 16, myLineStart = excl & 0xFFFFu;\n"
       "    if (tid < NP) {\n"
       "      sStart[tid] = myStart;\n"
       "      for (u32 c = 0u; c < myLines; c++) sLines[myLineStart + c] = tid | (c << 9);\n"
       "      if (tid == NP - 1u) sTotalLines = myLineStart + myLines;\n"
       "    }\n"
       "    __syncthreads();\n"
       "    PH(1)\n"
       "#pragma unroll\n"
       "    for (int j = 0; j < 4; j++)\n"
       "      if (alive[j]) sRec[sStart[" << part << "] + rank[j]] = make_uint4(" << row << ", hh[j], cv[j], " << fourth << ");\n"
       "    __syncthreads();\n"
       "    PH(2)\n"
       // whole lines: 8 adjacent lanes write the 8 records of one aligned 128-byte line with one store;
       // four lines per lane are in flight (the LDS look-ups of a line depend on one another)
       "    const u32 totalLines = sTotalLines;\n"
       "    for (u32 L0 = tid >> 3; L0 < totalLines; L0 += 512u) {\n"
       "      const u32 q = tid & 7u;\n"
       "      u32 e[4], lf[4], st[4], cu[4];\n"
       "#pragma unroll\n"
       "      for (u32 j = 0u; j < 4u; j++) { const u32 L = L0 + j * 128u; e[j] = L < totalLines ? sLines[L] : 0u; }\n"
       "#pragma unroll\n"
       "      for (u32 j = 0u; j < 4u; j++) { const u32 p = e[j] & 511u; lf[j] = sLeftN[p]; st[j] = sStart[p]; cu[j] = sCursor[p]; }\n"
       "      uint4 rec[4];\n"
       "#pragma unroll\n"
       "      for (u32 j = 0u; j < 4u; j++) {\n"
       "        const u32 p = e[j] & 511u, idx = (e[j] >> 9) * 8u + q;\n"
       "        const uint4 *src = idx < lf[j] ? sLeft + p * 7u + idx : sRec + ((st[j] + idx - lf[j]) & (T - 1u));\n"
       "        rec[j] = *src;\n"
       "      }\n"
       "#pragma unroll\n"
       "      for (u32 j = 0u; j < 4u; j++) {\n"
       "        const u32 p = e[j] & 511u, at = cu[j] + (e[j] >> 9) * 8u + q;\n"
       "        if (L0 + j * 128u < totalLines && at < a.capB) myB[(u64)p * a.capB + at] = rec[j];\n"
       "      }\n"
       "    }\n"
       "    __syncthreads();\n"
       "    PH(3)\n"
       // what is left of each partition (< 8 records) moves to its LDS remainder; cursors advance
       "    if (tid < NP) {\n"
       "      const u32 rem = myHave & 7u;\n"
       "      const u32 n = myLines ? rem : myCount;\n"
       "      const uint4 *src = sRec + (myLines ? myStart + myLines * 8u - myLeft : myStart);\n"
       "      uint4 *dst = sLeft + tid * 7u + (myLines ? 0u : myLeft);\n"
       "      uint4 t[7];\n"
       "#pragma unroll\n"
       "      for (u32 k = 0u; k < 7u; k++) t[k] = src[k < n ? k : 0u];\n"  // loads first, then stores: one LDS round trip
       "#pragma unroll\n"
       "      for (u32 k = 0u; k < 7u; k++) if (k < n) dst[k] = t[k];\n"
       "      sLeftN[tid] = rem;\n"
       "      u32 cur = sCursor[tid] + myLines * 8u;\n"
       "      if (cur > a.capB) { *a.overflow = 1u; cur = a.capB; }\n"
       "      sCursor[tid] = cur;\n"
       "      cnt[tid] = 0u;\n"  // this counter set is used again two tiles from now
       "    }\n"
       "    par ^= 1u;\n"
       "    tile = next;\n"
       "    PH(4)\n"
       "  }\n"
       "  __syncthreads();\n"
       "  PH(5)\n"
       // the remainders go out as one last line each, padded with null records (row = ~0) the merge skips
       "  for (u32 p = tid >> 3; p < NP; p += 128u) {\n"
       "    const u32 left = sLeftN[p], j = tid & 7u, cur = sCursor[p];\n"
       "    const bool fits = cur + 8u <= a.capB;\n"
       "    if (left && fits) myB[(u64)p * a.capB + cur + j] = j < left ? sLeft[p * 7u + j] : make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);\n"
       "    if (left && !fits) *a.overflow = 1u;\n"
       "    if (j == 0u) a.countsB[(u64)blockIdx.x * NP + p] = (left && fits) ? cur + 8u : cur;\n"
       "  }\n"
       "  PH(6)\n"
       "  PH_OUT\n"
       "}\n";
}

// ---- DIRECT scan, compact lines ------------------------------------------------------------------------
// (format: hr::Workspace::lineRecords == 14.)  Workgroup g scans the contiguous chunk of a.chunkTiles tiles that
// starts at tile g * a.chunkTiles, so that a row is identified by (stream, row within the chunk): 9 of those bits
// travel in the line's header, the rest in the low PB bits of the record's hash word — the PB partition bits of
// the hash are implied by the stream.  The host guarantees chunkTiles * 4096 <= 1 << (PB + 9).
// LDS: records as 8-byte units + a 2-byte array of low row bits; a line is written by 16 adjacent lanes (8 bytes
// each: lanes 0 and 8 the headers), LPL lines per lane in flight; the header of a half-line is the OR of its
// seven lanes' shifted row bits (three DPP steps inside the 8-lane group).
static void kernel_body_compact(std::ostringstream &o, const RtcSpec &s) {
  phase_macros(o, s);
  o << "#define STORE_LINE(p, v) (*(p) = (v))\n"
       "#define T 4096u\n#define LR 14u\n#define LEFT 13u\n#define LPL 5u\n"
       "__device__ __forceinline__ u32 lane_up(u32 v, u32 lane, u32 off) { return (u32)__builtin_amdgcn_ds_bpermute((int)((lane - off) << 2), (int)v); }\n"
       // OR over the 8 lanes of a half-line: xor 1, xor 2 (quad permutes), then the mirrored quad (row_half_mirror)
       "__device__ __forceinline__ u32 or8(u32 v) {\n"
       "  v |= (u32)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);\n"
       "  v |= (u32)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);\n"
       "  v |= (u32)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, true);\n"
       "  return v;\n"
       "}\n"
       // inclusive scan over the wavefront: Hillis-Steele inside each row of 16 (row_shr 1, 2, 4, 8; lanes without a
       // source keep the 0), then lane 15 of rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 and 3
       "__device__ __forceinline__ u32 wave_incl_scan(u32 v) {\n"
       "  v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);\n"
       "  v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);\n"
       "  v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);\n"
       "  v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);\n"
       "  v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);\n"
       "  v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);\n"
       "  return v;\n"
       "}\n"
       "extern \"C\" __global__ void __launch_bounds__(1024) hr_scan_rtc(Args a) {\n"
       "  __shared__ u64 sRec[T + NP * LEFT];\n"   // the tile's records sorted by partition, then up to 13 records per partition waiting for a full line
       "  __shared__ u16 sLo[T + NP * LEFT];\n"    // their low 9 row bits
       "  __shared__ u32 sCount[2][NP];\n"
       "  __shared__ u32 sStart[NP];\n"            // where the tile's records of a partition go
       "  __shared__ uint2 sLines[(T + NP * LEFT) / LR + 2u];\n"   // {partition | line of the tile << 9 | leftovers << 18, first slot | stream cursor << 13}
       "  __shared__ u32 sWave[16];\n"
       "  __shared__ u32 sTotalLines;\n"
       "  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;\n"
       "  for (u32 p = tid; p < NP; p += 1024u) { sCount[0][p] = 0u; sCount[1][p] = 0u; }\n"
       "  u32 myLeftN = 0u, myCursor = 0u, mySeen = 0u;\n"    // thread p < NP keeps partition p's leftover count, stream cursor and survivors in registers
       "  __syncthreads();\n"
       "  u64 *myB = reinterpret_cast<u64 *>(a.recB) + (u64)blockIdx.x * NP * a.capB * 16u;\n"  // capB: lines per stream
       "  const u32 numTiles = ((u32)a.length + T - 1u) / T;\n"
       "  const u32 firstTile = blockIdx.x * a.chunkTiles;\n"
       "  const u32 endTile = firstTile + a.chunkTiles < numTiles ? firstTile + a.chunkTiles : numTiles;\n"
       "  u32 tile = firstTile, par = 0u;\n"
       "  Raw R;\n"
       "  PH_DECL\n"
       "  load_tile(R, a, tile * T + tid * 4u);\n"
       // the lane's place in a line: 16 lanes per line, lanes 0 and 8 carry the two headers
       "  const u32 q = tid & 15u, r8 = q & 7u;\n"
       "  const u32 kk = (q >> 3) * 7u + (r8 ? r8 - 1u : 0u);\n"  // record of the line this lane carries
       "  const u32 sh = r8 ? 9u * (r8 - 1u) : 0u;\n"
       "  while (tile < endTile) {\n"
       "    u32 i0 = tile * T + tid * 4u;\n"          // eval4p moves it to the first row the lane's registers hold
       "    u32 hh[4], cv[4], cw[4], alive[4], rank[4];\n"
       "    const u32 next = tile + 1u;\n"
       "    eval4p(R, a, i0, hh, cv, cw, alive, next * T + tid * 4u);\n"
       "    const u32 rc0 = i0 - firstTile * T;\n"    // row within the chunk
       "    u32 *cnt = sCount[par];\n"
       "#pragma unroll\n"
       "    for (int j = 0; j < 4; j++) {\n"
       "      rank[j] = 0u;\n"
       "      if (alive[j]) rank[j] = __hip_atomic_fetch_add(&cnt[hh[j] >> (32 - PB)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
       "    }\n"
       "    __syncthreads();\n"
       "    PH(0)\n"
       // exclusive scans of (new records, whole lines) per partition, packed in one word
       "    u32 myCount = 0u, myLeft = 0u;\n"
       "    if (tid < NP) { myCount = cnt[tid]; myLeft = myLeftN; }\n"
       "    const u32 myHave = myCount + myLeft, myLines = myHave / LR;\n"
       "    mySeen += myCount;\n"               // alive[] summed per partition: exact whatever the record streams hold
       "    const u32 packed = (myCount << 16) | myLines;\n"
       "    const u32 incl = wave_incl_scan(packed);\n"
       "    if (lane == 63u) sWave[wave] = incl;\n"
       "    __syncthreads();\n"
       "    u32 before = 0u;\n"
       "#pragma unroll\n"
       "    for (u32 w = 0u; w < (NP + 63u) / 64u; w++) { const u32 t = sWave[w]; before += w < wave ? t : 0u; }\n"
       "    const u32 excl = before + incl - packed;\n"
       "    const u32 myStart = excl >> 16, myLineStart = excl & 0xFFFFu;\n"
       "    if (tid < NP) {\n"
       // a partition that completes no line in this tile takes its records straight into its remainder
       "      sStart[tid] = myLines ? myStart : T + tid * LEFT + myLeft;\n"
       "      for (u32 c = 0u; c < myLines; c++) sLines[myLineStart + c] = make_uint2(tid | (c << 9) | (myLeft << 18), myStart | (myCursor << 13));\n"
       "      if (tid == NP - 1u) sTotalLines = myLineStart + myLines;\n"
       "    }\n"
       "    __syncthreads();\n"
       "    PH(1)\n"
       "#pragma unroll\n"
       "    for (int j = 0; j < 4; j++)\n"
       "      if (alive[j]) {\n"
       "        const u32 at = sStart[hh[j] >> (32 - PB)] + rank[j], rc = rc0 + (u32)j;\n"
       "        sRec[at] = ((u64)((hh[j] << PB) | (rc >> 9)) << 32) | cv[j];\n"
       "        sLo[at] = (u16)(rc & 511u);\n"
       "      }\n"
       "    __syncthreads();\n"
       "    PH(2)\n"
       "    const u32 totalLines = sTotalLines;\n"
       "    for (u32 L0 = tid >> 4; L0 < totalLines; L0 += 64u * LPL) {\n"
       "      u32 e[LPL], lf[LPL], st[LPL], cu[LPL], lo[LPL];\n"
       "      u64 rec[LPL];\n"
       "#pragma unroll\n"
       "      for (u32 j = 0u; j < LPL; j++) {\n"
       "        const u32 L = L0 + j * 64u;\n"
       "        const uint2 w = L < totalLines ? sLines[L] : make_uint2(0u, 0u);\n"
       "        e[j] = w.x & 0x3FFFFu; lf[j] = w.x >> 18; st[j] = w.y & 0x1FFFu; cu[j] = w.y >> 13;\n"
       "      }\n"
       "#pragma unroll\n"
       "      for (u32 j = 0u; j < LPL; j++) {\n"
       "        const u32 p = e[j] & 511u, idx = (e[j] >> 9) * LR + kk;\n"
       "        const u32 at = idx < lf[j] ? T + p * LEFT + idx : st[j] + idx - lf[j];\n"
       "        rec[j] = sRec[at];\n"
       "        lo[j] = sLo[at];\n"
       "      }\n"
       "#pragma unroll\n"
       "      for (u32 j = 0u; j < LPL; j++) {\n"
       "        const u64 mine = r8 ? (u64)lo[j] << sh : 0ull;\n"
       "        const u64 hdr = ((u64)or8((u32)(mine >> 32)) << 32) | or8((u32)mine);\n"
       "        const u32 p = e[j] & 511u, line = cu[j] + (e[j] >> 9);\n"
       "        if (L0 + j * 64u < totalLines && line < a.capB) STORE_LINE(&myB[((u64)p * a.capB + line) * 16u + q], r8 ? rec[j] : hdr);\n"
       "      }\n"
       "    }\n"
       "    __syncthreads();\n"
       "    PH(3)\n"
       // what is left of each partition (< 14 records) moves to its LDS remainder; cursors advance
       "    if (tid < NP) {\n"
       "      const u32 rem = myHave - myLines * LR;\n"
       // only after a line: the 13 slots behind the last line go to the remainder as they are (those past `rem` are never read)
       "      if (myLines) {\n"
       "        const u32 from = myStart + myLines * LR - myLeft, to = T + tid * LEFT;\n"
       "        u64 t[LEFT]; u16 tl[LEFT];\n"
       "#pragma unroll\n"
       "        for (u32 k = 0u; k < LEFT; k++) { t[k] = sRec[from + k]; tl[k] = sLo[from + k]; }\n"
       "#pragma unroll\n"
       "        for (u32 k = 0u; k < LEFT; k++) { sRec[to + k] = t[k]; sLo[to + k] = tl[k]; }\n"
       "      }\n"
       "      myLeftN = rem;\n"
       "      u32 cur = myCursor + myLines;\n"
       "      if (cur > a.capB) { *a.overflow = 1u; cur = a.capB; }\n"
       "      myCursor = cur;\n"
       "      cnt[tid] = 0u;\n"  // this counter set is used again two tiles from now
       "    }\n"
       "    par ^= 1u;\n"
       "    tile = next;\n"
       "    PH(4)\n"
       "  }\n"
       "  __syncthreads();\n"
       "  if (tid < NP) sLines[tid] = make_uint2(myLeftN, myCursor);\n"
       "  __syncthreads();\n"
       "  PH(5)\n"
       // the remainders go out as one last, partly filled line each; countsB holds the exact number of records
       "  for (u32 p = tid >> 4; p < NP; p += 64u) {\n"
       "    const uint2 m = sLines[p];\n"
       "    const u32 left = m.x, cur = m.y;\n"
       "    const bool fits = cur < a.capB, has = r8 && kk < left;\n"
       "    const u64 rec = has ? sRec[T + p * LEFT + kk] : 0ull;\n"
       "    const u64 mine = has ? (u64)sLo[T + p * LEFT + kk] << sh : 0ull;\n"
       "    const u64 hdr = ((u64)or8((u32)(mine >> 32)) << 32) | or8((u32)mine);\n"
       "    if (left && fits) STORE_LINE(&myB[((u64)p * a.capB + cur) * 16u + q], r8 ? rec : hdr);\n"
       "    if (left && !fits) *a.overflow = 1u;\n"
       "    if (q == 0u) a.countsB[(u64)blockIdx.x * NP + p] = cur * LR + ((left && fits) ? left : 0u);\n"
       "  }\n"
       // the rows that passed the filters, one word per workgroup, for a host that owes a filter's count (null: nobody asked)
       "  if (a.hostCount) {\n"
       "    const u32 seen = wave_incl_scan(mySeen);\n"
       "    if (lane == 63u) sWave[wave] = seen;\n"
       "    __syncthreads();\n"
       "    if (tid == 0u) { u32 t = 0u; for (u32 w = 0u; w < 16u; w++) t += sWave[w]; a.hostCount[blockIdx.x] = t; }\n"
       "  }\n"
       "  PH(6)\n"
       "  PH_OUT\n"
       "}\n";
}

// ---- TABLE scan ----------------------------------------------------------------------------------------
// Low-cardinality queries: every workgroup aggregates its rows in an LDS hash table (key = hash << 32 | lowest
// row, 8-byte value) and emits one 16-byte record per group {row, hash, value} into region A at the end — the
// layout hr::flush_table writes and hr::merge_body reads.  No barrier inside the loop: the wavefronts run free,
// two tiles per wavefront in flight (two register buffers, each refilled column by column while it is evaluated:
// with two or three columns a single tile per wavefront leaves too few bytes in flight to cover HBM latency).
// The table is the specialised merge's: buckets of four keys (two 16-byte LDS reads).  A row first looks at its
// home bucket with straight-line code — it meets its group there nearly always once the groups exist: one LDS
// atomic more —; rows that do not are queued per wavefront in LDS and taken through the general probe loop 64 at a
// time, every lane busy.  Once the table holds LIMIT groups a row whose group finds no slot is written as a single
// record straight away (one global cursor reservation): always correct, slow when frequent — the host sends
// queries with that many groups to the DIRECT kernels.
static void kernel_body_table(std::ostringstream &o) {  // (reads nothing of the shape: PB, NP, widen and agg are in `o`)
  // table: 32-bit keys (the hash; 0xFFFFFFFF = empty — a row whose hash IS that value travels alone), the groups'
  // lowest rows and their values in arrays of their own: a probe is one 16-byte LDS read and four 32-bit compares
  o << "#define T 4096u\n#define SLOTS " << hr::kSlots << "u\n#define BUCKETS (SLOTS / 4u)\n#define LIMIT " << (hr::kSlots * 3 / 4)
    << "u\n#define EMPTY 0xFFFFFFFFu\n#define QCAP 128u\n"
       "struct Probe { u32 b, slot; bool done, spill; };\n"
       "__device__ __forceinline__ void probe_round(u32 *sKeys, u32 *sClaims, Probe &q, u32 h) {\n"
       "  const uint4 k = *reinterpret_cast<const uint4 *>(sKeys + 4u * q.b);\n"
       "  const bool e0 = k.x == EMPTY, e1 = k.y == EMPTY, e2 = k.z == EMPTY, e3 = k.w == EMPTY;\n"
       "  const bool m0 = k.x == h, m1 = k.y == h, m2 = k.z == h, m3 = k.w == h;\n"
       "  const bool anyM = m0 | m1 | m2 | m3, anyE = e0 | e1 | e2 | e3;\n"
       "  const u32 mi = m0 ? 0u : m1 ? 1u : m2 ? 2u : 3u, ei = e0 ? 0u : e1 ? 1u : e2 ? 2u : 3u;\n"
       "  const bool active = !q.done, hit = active & anyM;\n"
       "  q.slot = hit ? 4u * q.b + mi : q.slot;\n"
       "  bool claimed = false;\n"
       "  if (active & !anyM & anyE) {\n"  // a group this workgroup has not seen yet
       "    if (__hip_atomic_load(sClaims, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= LIMIT) {\n"
       "      q.spill = true; claimed = true;\n"  // the table is full enough: the row travels alone
       "    } else {\n"
       "      u32 expected = EMPTY;\n"
       "      if (__hip_atomic_compare_exchange_strong(sKeys + 4u * q.b + ei, &expected, h, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {\n"
       "        __hip_atomic_fetch_add(sClaims, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
       "        q.slot = 4u * q.b + ei; claimed = true;\n"
       "      }\n"  // lost the slot: the same bucket again next round (the winner may be this very group)
       "    }\n"
       "  }\n"
       "  q.b = (active & !anyM & !anyE) ? (q.b + 1u) & (BUCKETS - 1u) : q.b;\n"
       "  q.done = q.done | hit | claimed;\n"
       "}\n"
       // one row through the general probe loop
       "__device__ __forceinline__ void insert(const Args &a, u32 *sKeys, u32 *sRows, u64 *sVals, u32 *sClaims, u32 row, u32 h, u32 carried) {\n"
       "  const u64 value = widen(carried);\n"
       "  Probe q; q.b = h & (BUCKETS - 1u); q.slot = 0u; q.done = false; q.spill = h == EMPTY;\n"
       "  for (u32 tries = 0u; tries < BUCKETS + 8u && !q.done && !q.spill; tries++) probe_round(sKeys, sClaims, q, h);\n"
       "  if (q.done && !q.spill) {\n"
       "    __hip_atomic_fetch_min(sRows + q.slot, row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
       "    agg(sVals + q.slot, value);\n"
       "  } else {\n"
       "    const u32 p = PB ? h >> (32 - (PB ? PB : 1)) : 0u;\n"
       "    const u64 at = atomicAdd(a.cursorsA + p, 1u);\n"
       "    if (at < a.capA) a.recA[(u64)p * a.capA + at] = make_uint4(row, h, (u32)value, (u32)(value >> 32));\n"
       "    else *a.overflow = 1u;\n"
       "  }\n"
       "}\n"
       "__device__ __forceinline__ void drain(const Args &a, u32 *queue, u32 first, u32 count, u32 lane, u32 *sKeys, u32 *sRows, u64 *sVals, u32 *sClaims) {\n"
       "  asm volatile(\"s_waitcnt lgkmcnt(0)\" ::: \"memory\");\n"
       "  if (lane < count) {\n"
       "    const u32 e = 3u * (first + lane);\n"
       "    insert(a, sKeys, sRows, sVals, sClaims, queue[e], queue[e + 1u], queue[e + 2u]);\n"
       "  }\n"
       "  asm volatile(\"s_waitcnt lgkmcnt(0)\" ::: \"memory\");\n"
       "}\n"
       // one row, round one: the home bucket, straight-line
       "__device__ __forceinline__ void row_one(const Args &a, bool valid, u32 row, u32 h, u32 carried, u32 lane, u32 *sKeys, u32 *sRows, u64 *sVals, u32 *sClaims, u32 *queue, u32 &qn) {\n"
       "  const u32 b = h & (BUCKETS - 1u);\n"
       "  const uint4 k = *reinterpret_cast<const uint4 *>(sKeys + 4u * b);\n"
       "  const bool m0 = k.x == h, m1 = k.y == h, m2 = k.z == h, m3 = k.w == h;\n"
       "  const bool hit = valid && h != EMPTY && (m0 || m1 || m2 || m3);\n"
       "  if (hit) {\n"
       "    const u32 slot = 4u * b + (m0 ? 0u : m1 ? 1u : m2 ? 2u : 3u);\n"
       "    __hip_atomic_fetch_min(sRows + slot, row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
       "    agg(sVals + slot, widen(carried));\n"
       "  }\n"
       "  const bool pend = valid && !hit;\n"
       "  const u64 m = __ballot(pend);\n"
       "  if (m) {\n"
       "    if (pend) {\n"
       "      const u32 e = 3u * (qn + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u)));\n"
       "      queue[e] = row; queue[e + 1u] = h; queue[e + 2u] = carried;\n"
       "    }\n"
       "    qn += (u32)__popcll(m);\n"
       "    if (qn >= 64u) { qn -= 64u; drain(a, queue, qn, 64u, lane, sKeys, sRows, sVals, sClaims); }\n"
       "  }\n"
       "}\n"
       "extern \"C\" __global__ void __launch_bounds__(1024) hr_scan_rtc(Args a) {\n"
       "  __shared__ __attribute__((aligned(16))) u32 sKeys[SLOTS];\n"
       "  __shared__ u32 sRows[SLOTS];\n"
       "  __shared__ u64 sVals[SLOTS];\n"
       "  __shared__ u32 sQueue[16u * QCAP * 3u];\n"
       "  __shared__ u32 sPartCount[NP], sPartBase[NP];\n"
       "  __shared__ u32 sClaims;\n"
       "  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;\n"
       "  for (u32 s = tid; s < SLOTS; s += 1024u) { sKeys[s] = EMPTY; sRows[s] = 0xFFFFFFFFu; sVals[s] = IDENT; }\n"
       "  for (u32 p = tid; p < NP; p += 1024u) sPartCount[p] = 0u;\n"
       "  if (tid == 0u) sClaims = 0u;\n"
       "  __syncthreads();\n"
       "  const u32 numTiles = ((u32)a.length + T - 1u) / T, G = gridDim.x;\n"
       "  u32 tile = blockIdx.x, qn = 0u;\n"
       "  u32 *queue = sQueue + wave * (QCAP * 3u);\n"
       "  Raw R0, R1;\n"
       "  load_tile(R0, a, tile * T + tid * 4u);\n"
       "  load_tile(R1, a, (tile + G) * T + tid * 4u);\n"
       "#define TILE_STEP(R)                                                                                   \\\n"
       "  {                                                                                                    \\\n"
       "    u32 i0 = tile * T + tid * 4u;                                                                      \\\n"
       "    const u32 next = tile + 2u * G;                                                                    \\\n"
       "    u32 hh[4], cv[4], cw[4], alive[4];                                                                 \\\n"
       "    eval4p(R, a, i0, hh, cv, cw, alive, next * T + tid * 4u);                                          \\\n"
       "    const u32 row0 = a.rowBase + i0;                                                                   \\\n"
       "    row_one(a, alive[0] != 0u, row0, hh[0], cv[0], lane, sKeys, sRows, sVals, &sClaims, queue, qn);    \\\n"
       "    row_one(a, alive[1] != 0u, row0 + 1u, hh[1], cv[1], lane, sKeys, sRows, sVals, &sClaims, queue, qn); \\\n"
       "    row_one(a, alive[2] != 0u, row0 + 2u, hh[2], cv[2], lane, sKeys, sRows, sVals, &sClaims, queue, qn); \\\n"
       "    row_one(a, alive[3] != 0u, row0 + 3u, hh[3], cv[3], lane, sKeys, sRows, sVals, &sClaims, queue, qn); \\\n"
       "    tile += G;                                                                                         \\\n"
       "  }\n"
       "  while (tile < numTiles) {\n"
       "    TILE_STEP(R0)\n"
       "    if (tile >= numTiles) break;\n"
       "    TILE_STEP(R1)\n"
       "  }\n"
       "  if (qn) drain(a, queue, 0u, qn, lane, sKeys, sRows, sVals, &sClaims);\n"
       "  __syncthreads();\n"
       // flush (hr::flush_table): counting sort of the entries by partition, one cursor reservation per partition
       "  u32 rank[SLOTS / 1024u];\n"
       "#pragma unroll\n"
       "  for (u32 k = 0u; k < SLOTS / 1024u; k++) {\n"
       "    const u32 key = sKeys[tid + k * 1024u];\n"
       "    rank[k] = 0u;\n"
       "    if (key != EMPTY) rank[k] = __hip_atomic_fetch_add(&sPartCount[PB ? key >> (32 - (PB ? PB : 1)) : 0u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
       "  }\n"
       "  __syncthreads();\n"
       "  for (u32 p = tid; p < NP; p += 1024u) { const u32 c = sPartCount[p]; if (c) sPartBase[p] = atomicAdd(a.cursorsA + p, c); }\n"
       "  __syncthreads();\n"
       "#pragma unroll\n"
       "  for (u32 k = 0u; k < SLOTS / 1024u; k++) {\n"
       "    const u32 s = tid + k * 1024u;\n"
       "    const u32 key = sKeys[s];\n"
       "    if (key == EMPTY) continue;\n"
       "    const u32 p = PB ? key >> (32 - (PB ? PB : 1)) : 0u;\n"
       "    const u64 at = (u64)sPartBase[p] + rank[k], v = sVals[s];\n"
       "    if (at < a.capA) a.recA[(u64)p * a.capA + at] = make_uint4(sRows[s], key, (u32)v, (u32)(v >> 32));\n"
       "    else *a.overflow = 1u;\n"
       "  }\n"
       "}\n";
}

// RTC_SCAN_SORT64: the Sort + Reduce path (sort_reduce_fused.hip) — 16-byte line records {row, hash64 >> 32, carried measure, (u32)hash64}
// keyed by murmur3_x64_128 of the packed row (what Sort hashes: query/sort_reduce.cu:118-133), partitioned by the TOP bits of the
// 64-bit hash so that a partition is a contiguous range of the sorted order; plan.measure.col < 0: a constant measure
// (COUNT(*) is SUM over the literal 1) — no measure column is read, records carry Args::k's measure slot

// ---- dimension slots of 1, 2 or 4 bytes -------------------------------------------------------------------
// The dimension vector holds, for each dimension in descending width order, capacity x width value bytes, then one
// validity byte vector per dimension (dim_layout.hpp); the row that is hashed is [values][validity bytes], every field
// naturally aligned.  With the widths known when the source is written, the packed row becomes a list of 32-bit words,
// each the OR of the fields that fall into it.
struct SlotLayout {
  int nd = 0, valueBytes = 0;
  int width[kFusedDims] = {4, 4, 4, 4, 4, 4, 4, 4}, off[kFusedDims] = {};
  bool all4 = true, ok = true;
};
// widths: the slots' bytes in vector order, powers of two up to maxWidth (4: a plan's slots; 16: Sort + Reduce's vectors)
SlotLayout slot_layout(const int32_t *widths, int nd, int maxWidth) {
  SlotLayout L;
  L.nd = nd;
  int prev = maxWidth;
  for (int d = 0; d < nd && d < kFusedDims; d++) {
    const int w = widths[d];
    L.ok = L.ok && (w == 16 || w == 8 || w == 4 || w == 2 || w == 1) && w <= prev;  // descending: fields never straddle a word
    prev = w;
    L.width[d] = w;
    L.off[d] = L.valueBytes;
    L.valueBytes += w;
    L.all4 = L.all4 && w == 4;
  }
  // (the all-4-byte shortcuts pack the validity bytes of up to four dimensions into one word: beyond, the general word list)
  L.all4 = L.all4 && nd <= 4;
  return L;
}
// The packed row as 32-bit word expressions, each the OR of the fields that fall into it.  `val(d, k)` names 32-bit word k of
// dimension d's value (slots of up to 4 bytes have one), `okb(d)` its validity (0 / 1).
std::vector<std::string> row_words(const SlotLayout &L, const std::function<std::string(int, int)> &val,
                                   const std::function<std::string(int)> &okb) {
  std::vector<std::string> w(static_cast<size_t>((L.valueBytes + L.nd + 3) / 4));
  auto add = [&](int byteOff, const std::string &e) {
    std::string &x = w[static_cast<size_t>(byteOff / 4)];
    const int sh = 8 * (byteOff % 4);
    const std::string term = sh ? "(" + e + " << " + std::to_string(sh) + ")" : e;
    x = x.empty() ? term : x + " | " + term;
  };
  for (int d = 0; d < L.nd; d++)
    for (int k = 0; 4 * k < L.width[d] || k == 0; k++) add(L.off[d] + 4 * k, val(d, k));
  for (int d = 0; d < L.nd; d++) add(L.valueBytes + d, okb(d));
  return w;
}
// murmur3_x86_32 (seed 0) of the packed row: `val(d)` names the dimension's value (already truncated to its width),
// `okb(d)` its validity (0 / 1); writes the statements that leave the hash in `out`
void gen_row_hash(std::ostringstream &o, const SlotLayout &L, const std::function<std::string(int)> &val,
                  const std::function<std::string(int)> &okb, const std::string &out, const char *indent) {
  const int total = L.valueBytes + L.nd, words = (total + 3) / 4;
  const std::vector<std::string> w = row_words(L, [&](int d, int) { return val(d); }, okb);
  o << indent << "{\n" << indent << "  u32 g = 0u;\n";
  for (int k = 0; k < total / 4; k++) o << indent << "  g = mix(g, " << w[static_cast<size_t>(k)] << ");\n";
  if (total % 4) o << indent << "  { u32 k = (" << w[static_cast<size_t>(words - 1)] << ") * 0xcc9e2d51u; k = rotl(k, 15) * 0x1b873593u; g ^= k; }\n";
  o << indent << "  g ^= " << total << "u; g ^= g >> 16; g *= 0x85ebca6bu; g ^= g >> 13; g *= 0xc2b2ae35u; g ^= g >> 16;\n"
    << indent << "  " << out << " = g;\n" << indent << "}\n";
}
// lo64(murmur3_x64_128) (seed 0) of the packed row — Murmur128Stream of dim_layout.hpp, query/utils.cu:157-241 — with the
// same naming of values and validity bits as gen_row_hash; writes the statements that leave the hash in the u64 `out`.
// `val(d, k)` names 32-bit word k of dimension d's value: slots of 8 and 16 bytes are fields of two and four words (widths
// descend from 16, so such a field starts on a word of the packed row and its words go into the murmur lanes as they are)
void gen_row_hash64(std::ostringstream &o, const SlotLayout &L, const std::function<std::string(int, int)> &val,
                    const std::function<std::string(int)> &okb, const std::string &out, const char *indent) {
  const int total = L.valueBytes + L.nd, words = (total + 3) / 4;
  const std::vector<std::string> w = row_words(L, val, okb);
  auto lane64 = [&](int firstWord) {  // 8 row bytes from 32-bit word `firstWord` on, as a u64 expression ("" = none left)
    if (firstWord >= words) return std::string();
    std::string e = "(u64)(" + w[static_cast<size_t>(firstWord)] + ")";
    if (firstWord + 1 < words) e += " | ((u64)(" + w[static_cast<size_t>(firstWord + 1)] + ") << 32)";
    return e;
  };
  const std::string in = indent;
  o << in << "{\n" << in << "  u64 g1 = 0ull, g2 = 0ull, q1, q2;\n";
  const int blocks = total / 16;
  for (int b = 0; b < blocks; b++) {
    o << in << "  q1 = " << lane64(4 * b) << "; q2 = " << lane64(4 * b + 2) << ";\n"
      << in << "  q1 *= MC1; q1 = rotl64(q1, 31); q1 *= MC2; g1 ^= q1; g1 = rotl64(g1, 27); g1 += g2; g1 = g1 * 5ull + 0x52dce729ull;\n"
      << in << "  q2 *= MC2; q2 = rotl64(q2, 33); q2 *= MC1; g2 ^= q2; g2 = rotl64(g2, 31); g2 += g1; g2 = g2 * 5ull + 0x38495ab5ull;\n";
  }
  const int tail = total % 16;
  if (tail > 8) o << in << "  q2 = " << lane64(4 * blocks + 2) << "; q2 *= MC2; q2 = rotl64(q2, 33); q2 *= MC1; g2 ^= q2;\n";
  if (tail > 0) o << in << "  q1 = " << lane64(4 * blocks) << "; q1 *= MC1; q1 = rotl64(q1, 31); q1 *= MC2; g1 ^= q1;\n";
  o << in << "  g1 ^= " << total << "ull; g2 ^= " << total << "ull; g1 += g2; g2 += g1;\n"
    << in << "  g1 = fmix64(g1); g2 = fmix64(g2); g1 += g2;\n"
    << in << "  " << out << " = g1;\n" << in << "}\n";
}
const char *kPrelude64 =
    "#define MC1 0x87c37b91114253d5ull\n#define MC2 0x4cf5ad432745937full\n"
    "__device__ __forceinline__ u64 rotl64(u64 x, int r) { return (x << r) | (x >> (64 - r)); }\n"
    "__device__ __forceinline__ u64 fmix64(u64 k) { k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33; return k; }\n";
// mask that truncates a 32-bit value to a slot's width
const char *width_mask(int w) { return w == 4 ? "" : w == 2 ? " & 0xFFFFu" : " & 0xFFu"; }
// dimension d of row `row` of a dimension vector at `base` (capacity `cap`), zero-extended; and its validity byte
std::string slot_load(const SlotLayout &L, int d, const char *base, const char *cap, const std::string &row) {
  const std::string at = std::string(base) + " + (u64)" + std::to_string(L.off[d]) + " * " + cap + " + " + std::to_string(L.width[d]) + "ull * " + row;
  return L.width[d] == 4 ? "*reinterpret_cast<const u32 *>(" + at + ")" : L.width[d] == 2 ? "(u32)*reinterpret_cast<const u16 *>(" + at + ")" : "(u32)*(" + at + ")";
}
std::string slot_store(const SlotLayout &L, int d, const char *base, const char *cap, const std::string &row, const std::string &v) {
  const std::string at = std::string(base) + " + (u64)" + std::to_string(L.off[d]) + " * " + cap + " + " + std::to_string(L.width[d]) + "ull * " + row;
  return L.width[d] == 4 ? "*reinterpret_cast<u32 *>(" + at + ") = " + v + ";" : L.width[d] == 2 ? "*reinterpret_cast<u16 *>(" + at + ") = (u16)(" + v + ");" : "*(" + at + ") = (u8)(" + v + ");";
}
// element `idx` of a source column of `step` bytes per value, widened to 32 bits (sign-extended for int kinds)
std::string column_elem(int step, bool sgn, const std::string &base, const std::string &idx) {
  if (step == 4) return base + "[" + idx + "]";
  if (step == 2) return sgn ? "(u32)(i32)reinterpret_cast<const short *>(" + base + ")[" + idx + "]" : "(u32)reinterpret_cast<const u16 *>(" + base + ")[" + idx + "]";
  return sgn ? "(u32)(i32)reinterpret_cast<const signed char *>(" + base + ")[" + idx + "]" : "(u32)reinterpret_cast<const u8 *>(" + base + ")[" + idx + "]";
}
// which column slot's stored kind is signed (decides the widening of a narrow column): the expressions that read it say
bool column_signed(const RtcSpec &s, int c) {
  for (int d = 0; d < s.nd; d++)
    if (s.dims[d].col == c) return s.dims[d].akind == K_I32;
  if (!s.constMeasure && s.measure.col == c) return s.measure.akind == K_I32;
  for (int k = 0; k < s.numFilters; k++)
    if (s.filters[k].col == c) return s.filters[k].akind == K_I32;
  return false;
}

// the whole source of a plan-sourced scan; empty when the plan is outside the supported shapes.  The aggregate and the
// widening are read for RTC_SCAN_TABLE only.
std::string generate(const RtcSpec &s) {
  const int nd = s.nd, partBits = s.partBits, kind = s.kind;
  const uint32_t nullMask = s.nullMask;
  if (nd < 1 || nd > kFusedDims || s.numCols < 0 || s.numCols > kFusedCols || s.numFilters < 0 || s.numFilters > kFusedFilters) return "";
  if (kind == RTC_SCAN_COMPACT && partBits < 3) return "";
  const SlotLayout SL = slot_layout(s.dimWidth, nd, 4);
  if (!SL.ok) return "";
  for (int c = 0; c < s.numCols; c++) {
    const int st = s.step[c];
    if (!(st == 4 || st == 2 || st == 1)) return "";
  }
  std::ostringstream o;
  const int nc = s.numCols;
  const bool sort64 = kind == RTC_SCAN_SORT64;
  const bool constMeasure = sort64 && s.constMeasure;  // the records carry Args::k's measure slot as it is
  if (s.constMeasure && !sort64) return "";
  // AVG_FLOAT: the record carries the pair's average (a float, whatever the column's kind) and, in the top bit of its row word,
  // "null measure" — a row index fits 31 bits, a stream's padding records stay row = ~0
  const bool avg = s.measureAvg != 0;
  if (avg && (!sort64 || constMeasure || s.measureWidth != 8 || s.identity != 0)) return "";
  const int firstFilterCol = constMeasure ? nd : nd + 1;  // column slots: dimension d -> d, measure -> nd (if any), then the filters' own
  o << kPrelude << (sort64 ? kPrelude64 : "") << args_text()
    << "#define NC " << nc << "\n#define ND " << nd << "\n#define PB " << partBits << "\n#define NP " << (1 << partBits) << "\n"
       "struct Raw { u32 v[NC][4]; u32 win[NC]; };\n";
  // ---- loads, one column at a time.  Always the full 16 bytes + the 16-bit validity window, from a row index clamped
  // to length - 4: no guarded variant, hence no branch at load time (a branch around a load makes the compiler copy
  // the loaded registers at the join — and wait for the load right there).  The one quad of the shard that straddles
  // its end is shifted into place when its tile is evaluated; lanes past the end hold rows that do not take part.
  // The columns are read once, so their loads are non-temporal; the record lines, which the merge reads back, are stored
  // plainly (profiles/r4_experiments.md measured both, one at a time and together).
  o << "__device__ __forceinline__ u32 clampi(const Args &a, u32 i0) { const u32 lim = a.length >= 4 ? (u32)a.length - 4u : 0u; return i0 < lim ? i0 : lim; }\n";
  for (int c = 0; c < nc; c++) {
    o << "__device__ __forceinline__ void load_col" << c << "(Raw &r, const Args &a, u32 i0c) {\n";
    const int step = s.step[c];
    if (step != 4) {  // a quad of a 2- / 1-byte column is 8 / 4 bytes: one load, widened in registers (query/iterator.hpp:146-165)
      const bool sgn = column_signed(s, c);
      const char *ptr = step == 2 ? "reinterpret_cast<const u16 *>(a.vals[" : "reinterpret_cast<const u8 *>(a.vals[";
      if (step == 2) {
        o << "  const U2 t = __builtin_nontemporal_load(reinterpret_cast<const U2a *>(" << ptr << c << "]) + i0c));\n  const u32 t0 = t.x, t1 = t.y;\n";
        if (sgn) o << "  r.v[" << c << "][0] = (u32)((i32)(t0 << 16) >> 16); r.v[" << c << "][1] = (u32)((i32)t0 >> 16); r.v[" << c << "][2] = (u32)((i32)(t1 << 16) >> 16); r.v[" << c << "][3] = (u32)((i32)t1 >> 16);\n";
        else o << "  r.v[" << c << "][0] = t0 & 0xFFFFu; r.v[" << c << "][1] = t0 >> 16; r.v[" << c << "][2] = t1 & 0xFFFFu; r.v[" << c << "][3] = t1 >> 16;\n";
      } else {
        o << "  const u32 t0 = __builtin_nontemporal_load(reinterpret_cast<const U1a *>(" << ptr << c << "]) + i0c));\n";
        if (sgn) o << "  r.v[" << c << "][0] = (u32)((i32)(t0 << 24) >> 24); r.v[" << c << "][1] = (u32)((i32)(t0 << 16) >> 24); r.v[" << c << "][2] = (u32)((i32)(t0 << 8) >> 24); r.v[" << c << "][3] = (u32)((i32)t0 >> 24);\n";
        else o << "  r.v[" << c << "][0] = t0 & 0xFFu; r.v[" << c << "][1] = (t0 >> 8) & 0xFFu; r.v[" << c << "][2] = (t0 >> 16) & 0xFFu; r.v[" << c << "][3] = t0 >> 24;\n";
      }
    } else {
      o << "  const U4 t = __builtin_nontemporal_load(reinterpret_cast<const U4a *>(a.vals[" << c << "] + i0c)); r.v[" << c << "][0] = t.x; r.v[" << c
        << "][1] = t.y; r.v[" << c << "][2] = t.z; r.v[" << c << "][3] = t.w;\n";
    }
    if (nullMask & (1u << c))
      o << "  r.win[" << c << "] = reinterpret_cast<const PU16 *>(a.nulls[" << c << "] + ((i0c + a.bitOff[" << c << "]) >> 3))->v;\n";
    else
      o << "  r.win[" << c << "] = 0xFFFFu;\n";
    o << "}\n";
  }
  o << "__device__ __forceinline__ void load_tile(Raw &r, const Args &a, u32 i0) {\n  const u32 i0c = clampi(a, i0);\n";
  for (int c = 0; c < nc; c++) o << "  load_col" << c << "(r, a, i0c);\n";
  o << "}\n";
  // ---- evaluate + hash one quad (hash, carried measure bits and "takes part" of its four rows) AND issue
  // the next tile's loads, column by column, as soon as a column's registers are dead: a single register buffer, yet
  // loads are in flight during the whole evaluation instead of only after it (the kernel is HBM-bound: with the loads
  // issued after the evaluation the read pipe idled for a third of every tile).  Scheduling barriers pin each load
  // behind the last use of the registers it refills.  i0n: this lane's first row in the next tile (past the last tile the
  // clamp turns the prefetch into one cache line per column: no branch needed); partial: this tile holds the shard's
  // end (wave-uniform).
  {
    const std::string bar = "  __builtin_amdgcn_sched_barrier(0);\n";
    auto prefetch = [&](int c) { o << bar << "  load_col" << c << "(r, a, i0nc);\n" << bar; };
    o << "__device__ __forceinline__ void eval4p(Raw &r, const Args &a, u32 &i0, u32 (&hh)[4], u32 (&cv)[4], u32 (&cw)[4], u32 (&alive)[4], u32 i0n) {\n"
         "  u32 okc[NC];\n"
         "  cw[0] = cw[1] = cw[2] = cw[3] = 0u;\n"
         "  const u32 i0c = clampi(a, i0), i0nc = clampi(a, i0n);\n"
         // the registers hold rows i0c .. i0c + 3: i0's own rows except in the one quad that straddles the shard's end (loaded
         // `sh` rows early: its first `sh` rows belong to the lane before) and in the lanes past the end (sh = 4: no row).
         // The caller numbers the lane's rows from i0c: no register is moved
         "  const u32 sh = i0 - i0c < 4u ? i0 - i0c : 4u;\n"
         "  i0 = i0c;\n";
    for (int c = 0; c < nc; c++) {
      if (nullMask & (1u << c)) o << "  okc[" << c << "] = (r.win[" << c << "] >> ((i0c + a.bitOff[" << c << "]) & 7u)) & 0xFu;\n";
      else o << "  okc[" << c << "] = 0xFu;\n";
    }
    o << "#pragma unroll\n"
         "  for (int j = 0; j < 4; j++) {\n"
         "    u32 keep = ((u32)j >= sh && (int)(i0c + j) < a.length) ? 1u : 0u;\n";
    for (int k = 0; k < s.numFilters; k++) {
      const RtcExpr &e = s.filters[k];
      if (e.col < 0 || e.col >= nc) return "";
      o << "    {\n      const u32 v = r.v[" << e.col << "][j]; const u32 okb = (okc[" << e.col << "] >> j) & 1u;\n";
      if (!gen_compare(e, o, "v", "okb", "keep", const_name(const_slot_filter(k)))) return "";
      o << "    }\n";
    }
    o << "    alive[j] = keep;\n  }\n";
    for (int c = firstFilterCol; c < nc; c++) prefetch(c);  // columns only the filters read
    if (constMeasure) {
      o << "  cv[0] = cv[1] = cv[2] = cv[3] = " << const_name(const_slot_measure()) << ";\n";
    } else {  // measure: fused_carry
      const RtcExpr &e = s.measure;
      if (e.col != nd) return "";
      o << "#pragma unroll\n  for (int j = 0; j < 4; j++) {\n"
           "    const u32 v = r.v[" << nd << "][j]; const u32 okb = (okc[" << nd << "] >> j) & 1u; u32 x;\n";
      if (!gen_value(e, o, "v", "okb", "x", const_name(const_slot_measure()), const_slot_measure_chain(), sort64)) return "";
      if (avg) {  // avg_measure_float (device_model.hpp) of the expression's value: as measureDtype, then as a float
        const int rk = e.rk;
        if (!(rk == K_F32 || rk == K_I32 || rk == K_U32) || !(s.measureDtype == Float64 || s.measureDtype == Int64)) return "";
        const bool f64 = s.measureDtype == Float64;
        const char *cvt = rk == K_F32 ? (f64 ? "x" : "__float_as_uint((float)(i64)__uint_as_float(x))")
                          : rk == K_I32 ? (f64 ? "__float_as_uint((float)(double)(i32)x)" : "__float_as_uint((float)(i64)(i32)x)")
                                        : (f64 ? "__float_as_uint((float)(double)x)" : "__float_as_uint((float)(i64)x)");
        o << "    cv[j] = okb ? " << cvt << " : 0u;\n"
             "    alive[j] |= (alive[j] & (okb ^ 1u)) << 31;\n";
      } else if (s.measureWidth == 8) {
        if (s.identity != 0) return "";
        o << "    cv[j] = okb ? x : 0u;\n";
      } else {
        const int target = s.measureDtype == Int32 ? K_I32 : s.measureDtype == Uint32 ? K_U32 : K_F32;
        if (!plain_store(e.rk, target)) return "";
        o << "    cv[j] = okb ? x : " << hex(static_cast<uint32_t>(s.identity)) << ";\n";
      }
      o << "  }\n";
      prefetch(nd);
    }
    if (SL.all4 && !sort64) {
    o << "  u32 h[4] = {0u, 0u, 0u, 0u}, okbytes[4] = {0u, 0u, 0u, 0u};\n";
    for (int d = 0; d < nd; d++) {
      const RtcExpr &e = s.dims[d];
      if (e.col != d || !plain_store(e.rk, e.outKind)) return "";
      o << "#pragma unroll\n  for (int j = 0; j < 4; j++) {\n"
           "    const u32 v = r.v[" << d << "][j]; const u32 okb = (okc[" << d << "] >> j) & 1u; u32 x;\n";
      if (!gen_value(e, o, "v", "okb", "x", const_name(const_slot_dim(d)), const_slot_dim_chain(d))) return "";
      o << "    h[j] = mix(h[j], x); okbytes[j] |= okb << " << 8 * d << ";\n  }\n";
      prefetch(d);
    }
    // Murmur32Stream (dim_layout.hpp): the validity bytes are one more block when there are four of them,
    // otherwise the tail
    o << "#pragma unroll\n  for (int j = 0; j < 4; j++) {\n    u32 g = h[j];\n";
    if (nd == 4) o << "    g = mix(g, okbytes[j]);\n";
    else o << "    { u32 k = okbytes[j] * 0xcc9e2d51u; k = rotl(k, 15) * 0x1b873593u; g ^= k; }\n";
    o << "    g ^= " << 5 * nd << "u; g ^= g >> 16; g *= 0x85ebca6bu; g ^= g >> 13; g *= 0xc2b2ae35u; g ^= g >> 16;\n"
         "    hh[j] = g;\n  }\n}\n";
    } else {
      // narrow slots: the values are kept (truncated to their slot, as the dimension vector would hold them) until all
      // are known, then the packed row's words are put together
      for (int d = 0; d < nd; d++) o << "  u32 xv" << d << "[4], xo" << d << "[4];\n";
      for (int d = 0; d < nd; d++) {
        const RtcExpr &e = s.dims[d];
        if (e.col != d || !plain_store(e.rk, e.outKind) || (SL.width[d] != 4 && !int_kind(e.rk))) return "";
        o << "#pragma unroll\n  for (int j = 0; j < 4; j++) {\n"
             "    const u32 v = r.v[" << d << "][j]; const u32 okb = (okc[" << d << "] >> j) & 1u; u32 x;\n";
        if (!gen_value(e, o, "v", "okb", "x", const_name(const_slot_dim(d)), const_slot_dim_chain(d))) return "";
        o << "    xv" << d << "[j] = x" << width_mask(SL.width[d]) << "; xo" << d << "[j] = okb;\n  }\n";
        prefetch(d);
      }
      o << "#pragma unroll\n  for (int j = 0; j < 4; j++) {\n";
      if (sort64) {  // the record's second word holds the hash's upper half (its top bits choose the partition), the fourth the lower
        o << "    u64 h64;\n";
        gen_row_hash64(o, SL, [](int d, int) { return "xv" + std::to_string(d) + "[j]"; }, [](int d) { return "xo" + std::to_string(d) + "[j]"; },
                       "h64", "    ");
        o << "    hh[j] = (u32)(h64 >> 32); cw[j] = (u32)h64;\n";
      } else {
        gen_row_hash(o, SL, [](int d) { return "xv" + std::to_string(d) + "[j]"; }, [](int d) { return "xo" + std::to_string(d) + "[j]"; },
                     "hh[j]", "    ");
      }
      o << "  }\n}\n";
    }
  }
  if (kind == RTC_SCAN_TABLE) {
    if (!gen_widen(o, s) || !gen_agg(o, s)) return "";
    kernel_body_table(o);
  } else if (kind == RTC_SCAN_COMPACT) {
    kernel_body_compact(o, s);
  } else {
    Lines16 rec{sort64 ? "cw[j]" : "0u"};
    if (avg) rec.row = "(a.rowBase + i0 + j) | (alive[j] & 0x80000000u)";
    kernel_body_lines16(o, s, rec);
  }
  return o.str();
}

// The same kernel over rows [rowBase, rowBase + length) of a dimension vector of `nd` 4-byte dimensions
// (values per dimension, then one validity byte per row and dimension) and a measure vector of `vw`-byte
// values — what HashReduce is handed when the batch's transforms were launched (ARES_FUSE=0, plans the
// fused scan does not cover).  Args: vals[d] / nulls[d] = dimension d's values / validity bytes at
// rowBase, vals[nd] = the measures at rowBase.  Records carry the whole value: {row, hash, lo, hi}.
// sort64: the Sort + Reduce path over materialised vectors (sort_reduce_fused.hip): records {row, hash64 >> 32, the 4-byte value,
// (u32)hash64} keyed by lo64(murmur3_x64_128) of the packed row, partition = top bits of the 64-bit hash; up to eight dimensions.
// widths (sort64 only): the dimension slots' bytes in vector order (16 / 8 / 4 / 2 / 1, descending); null: all four bytes.
// A row's values live in 32-bit words of `Raw::v`: one word per slot of 4, 2 or 1 bytes, two per 8-byte slot (Int64, Uint64,
// GeoPoint), four per 16-byte slot (UUID) — at most kSortVectorValueBytes per row (sort_vector_layout_supported), which is
// what four rows per lane leave of 128 VGPRs.
// hll (sort64 only): HyperLogLog's pre-aggregation scan (hll.hip).  The 4-byte value is the row's hll value; the 64-bit key is
// the row hash with its low 16 bits replaced by the value's register id (query/functor.hpp:1296-1305) and the partition the
// top PB bits of a scramble of the WHOLE key: the <= 16384 registers of one dimension row share the key's upper 48 bits.
std::string generate_vector(const RtcSpec &s) {
  const int nd = s.nd, vw = s.vectorVW, partBits = s.partBits;
  const bool hll = s.kind == RTC_HLL_SCAN, sort64 = hll || s.kind == RTC_SORT_VECTOR_SCAN;
  if (nd < 1 || nd > (sort64 ? kFusedDims : kGenericFusedDims) || (vw != 4 && vw != 8) || (sort64 && vw != 4)) return "";
  if (hll && (partBits < 1 || partBits > 9)) return "";
  const SlotLayout SL = slot_layout(s.dimWidth, nd, sort64 ? 16 : 4);
  if (!SL.ok || (!sort64 && !SL.all4)) return "";
  const int *width = SL.width;
  int wb[kFusedDims] = {};  // the first word of `Raw::v` that holds dimension d
  bool narrow = false, wide = false;
  int nw = 0;
  for (int d = 0; d < nd; d++) {
    narrow = narrow || width[d] != 4;
    wide = wide || width[d] > 4;
    wb[d] = nw;
    nw += width[d] > 4 ? width[d] / 4 : 1;
  }
  if (wide && SL.valueBytes > kSortVectorValueBytes) return "";
  std::ostringstream o;
  const int mq = vw / 4;
  o << kPrelude << (sort64 ? kPrelude64 : "") << args_text()
    << "#define ND " << nd << "\n#define MQ " << mq << "\n#define PB " << partBits << "\n#define NP " << (1 << partBits) << "\n";
  if (wide) o << "#define NW " << nw << "\nstruct Raw { u32 v[NW][4]; u32 ok[ND]; u32 m[MQ * 4]; };\n";
  else o << "struct Raw { u32 v[ND][4]; u32 ok[ND]; u32 m[MQ * 4]; };\n";
  o << "__device__ __forceinline__ void load_full(Raw &r, const Args &a, u32 i0) {\n";
  if (narrow) {  // (slot by slot: a 2-byte slot's four rows are one 8-byte load, a 1-byte slot's one 4-byte load, an 8-byte
                 // slot's two 16-byte loads, a 16-byte slot's four — `rowBase` is any row: none of them assumes more than the
                 // slot's own alignment)
    for (int d = 0; d < nd; d++) {
      const int v = wb[d];
      if (width[d] > 4) {
        const int q = width[d] / 4;  // words per row: load k holds words [4k, 4k + 4) of the quad's 4 * q
        o << "  {\n    const PU32x4 *p = reinterpret_cast<const PU32x4 *>(reinterpret_cast<const u8 *>(a.vals[" << d << "]) + " << width[d] << "ull * i0);\n";
        for (int k = 0; k < q; k++) o << "    const PU32x4 t" << k << " = p[" << k << "];\n";
        o << "   ";
        for (int k = 0; k < q; k++)
          for (int e = 0; e < 4; e++) o << " r.v[" << v + (4 * k + e) % q << "][" << (4 * k + e) / q << "] = t" << k << ".v[" << e << "];";
        o << "\n  }\n";
      } else if (width[d] == 4)
        o << "  { const PU32x4 t = *reinterpret_cast<const PU32x4 *>(a.vals[" << d << "] + i0); r.v[" << v << "][0] = t.v[0]; r.v[" << v
          << "][1] = t.v[1]; r.v[" << v << "][2] = t.v[2]; r.v[" << v << "][3] = t.v[3]; }\n";
      else if (width[d] == 2)
        o << "  { const PU32x2 t = *reinterpret_cast<const PU32x2 *>(reinterpret_cast<const u8 *>(a.vals[" << d << "]) + 2ull * i0); r.v[" << v
          << "][0] = t.v[0] & 0xFFFFu; r.v[" << v << "][1] = t.v[0] >> 16; r.v[" << v << "][2] = t.v[1] & 0xFFFFu; r.v[" << v << "][3] = t.v[1] >> 16; }\n";
      else
        o << "  { const u32 t = reinterpret_cast<const PU32 *>(reinterpret_cast<const u8 *>(a.vals[" << d << "]) + i0)->v; r.v[" << v
          << "][0] = t & 0xFFu; r.v[" << v << "][1] = (t >> 8) & 0xFFu; r.v[" << v << "][2] = (t >> 16) & 0xFFu; r.v[" << v << "][3] = t >> 24; }\n";
      o << "  r.ok[" << d << "] = reinterpret_cast<const PU32 *>(a.nulls[" << d << "] + i0)->v;\n";
    }
  } else {
  o << "#pragma unroll\n"
       "  for (int d = 0; d < ND; d++) {\n"
       "    const PU32x4 t = *reinterpret_cast<const PU32x4 *>(a.vals[d] + i0);\n"
       "    r.v[d][0] = t.v[0]; r.v[d][1] = t.v[1]; r.v[d][2] = t.v[2]; r.v[d][3] = t.v[3];\n"
       "    r.ok[d] = reinterpret_cast<const PU32 *>(a.nulls[d] + i0)->v;\n"
       "  }\n";
  }
  o << ""
       "#pragma unroll\n"
       "  for (int q = 0; q < MQ; q++) {\n"
       "    const PU32x4 t = *reinterpret_cast<const PU32x4 *>(a.vals[ND] + (u64)i0 * MQ + 4 * q);\n"
       "    r.m[4 * q] = t.v[0]; r.m[4 * q + 1] = t.v[1]; r.m[4 * q + 2] = t.v[2]; r.m[4 * q + 3] = t.v[3];\n"
       "  }\n"
       "}\n"
       "__device__ __forceinline__ void load_tail(Raw &r, const Args &a, u32 i0) {\n";
  if (narrow) {
    for (int d = 0; d < nd; d++) {
      const char *elem = width[d] == 4 ? "a.vals[%d][i0 + j]" : width[d] == 2 ? "(u32)reinterpret_cast<const u16 *>(a.vals[%d])[i0 + j]" : "(u32)reinterpret_cast<const u8 *>(a.vals[%d])[i0 + j]";
      char buf[128];
      snprintf(buf, sizeof(buf), elem, d);
      o << "  r.ok[" << d << "] = 0u;\n"
           "  for (int j = 0; j < 4; j++) {\n"
           "    const bool in = (int)(i0 + j) < a.length;\n";
      if (width[d] > 4)  // (a wide slot's vector starts on a multiple of its width: word loads are aligned)
        for (int k = 0; k < width[d] / 4; k++)
          o << "    r.v[" << wb[d] + k << "][j] = in ? a.vals[" << d << "][" << width[d] / 4 << "ull * (i0 + j) + " << k << "] : 0u;\n";
      else
        o << "    r.v[" << wb[d] << "][j] = in ? " << buf << " : 0u;\n";
      o << "    r.ok[" << d << "] |= in ? (u32)a.nulls[" << d << "][i0 + j] << (8 * j) : 0u;\n"
           "  }\n";
    }
  } else {
  o << "#pragma unroll\n"
       "  for (int d = 0; d < ND; d++) {\n"
       "    r.ok[d] = 0u;\n"
       "    for (int j = 0; j < 4; j++) {\n"
       "      const bool in = (int)(i0 + j) < a.length;\n"
       "      r.v[d][j] = in ? a.vals[d][i0 + j] : 0u;\n"
       "      r.ok[d] |= in ? (u32)a.nulls[d][i0 + j] << (8 * j) : 0u;\n"
       "    }\n"
       "  }\n";
  }
  o << "  for (int j = 0; j < 4; j++)\n"
       "    for (int q = 0; q < MQ; q++) r.m[j * MQ + q] = (int)(i0 + j) < a.length ? a.vals[ND][(u64)(i0 + j) * MQ + q] : 0u;\n"
       "}\n"
       // Murmur32Stream over the packed row (dim_layout.hpp): values, then the validity bytes — one more block
       // when there are four of them, otherwise the tail
       "__device__ __forceinline__ void eval4(const Raw &r, const Args &a, u32 i0, u32 (&hh)[4], u32 (&cv)[4], u32 (&cw)[4], u32 (&alive)[4]) {\n"
       "#pragma unroll\n"
       "  for (int j = 0; j < 4; j++) {\n"
       "    alive[j] = (int)(i0 + j) < a.length ? 1u : 0u;\n";
  if (sort64) {
    o << "    u64 h64;\n";
    gen_row_hash64(o, SL, [&](int d, int k) { return "r.v[" + std::to_string(wb[d] + k) + "][j]"; },
                   [](int d) { return "((r.ok[" + std::to_string(d) + "] >> (8 * j)) & 0xFFu)"; }, "h64", "    ");
    if (hll) o << "    h64 = (h64 & 0xFFFFFFFFFFFF0000ull) | (u64)(r.m[j] & 0x3FFFu);\n";
    o << "    hh[j] = (u32)(h64 >> 32);\n"
         "    cv[j] = r.m[j];\n"
         "    cw[j] = (u32)h64;\n"
         "  }\n"
         "}\n";
  } else {
  o << "    u32 h = 0u, okbytes = 0u;\n"
       "#pragma unroll\n"
       "    for (int d = 0; d < ND; d++) { h = mix(h, r.v[d][j]); okbytes |= ((r.ok[d] >> (8 * j)) & 0xFFu) << (8 * d); }\n";
  if (nd == 4) o << "    h = mix(h, okbytes);\n";
  else o << "    { u32 k = okbytes * 0xcc9e2d51u; k = rotl(k, 15) * 0x1b873593u; h ^= k; }\n";
  o << "    h ^= " << 5 * nd << "u; h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;\n"
       "    hh[j] = h;\n"
       "    cv[j] = r.m[j * MQ];\n"
       "    cw[j] = MQ == 2 ? r.m[j * MQ + MQ - 1] : 0u;\n"
       "  }\n"
       "}\n";
  }
  o << "__device__ __forceinline__ void load_tile(Raw &r, const Args &a, u32 i0) { if ((int)(i0 + 3u) < a.length) load_full(r, a, i0); else if ((int)i0 < a.length) load_tail(r, a, i0); }\n"
       "__device__ __forceinline__ void eval4p(Raw &r, const Args &a, u32 &i0, u32 (&hh)[4], u32 (&cv)[4], u32 (&cw)[4], u32 (&alive)[4], u32 i0n) {\n"
       "  eval4(r, a, i0, hh, cv, cw, alive);\n"
       "  load_tile(r, a, i0n);\n"
       "}\n";
  // (sort64: the level-1 partition of the wide layout is the hash's top PB bits, or — a.pad set: a previous result whose row
  // hashes are not known is hashed again, rows in ascending hash order of which every tile falls into ONE such partition —
  // the LOW PB bits of the top-bits partition index (a.chunkTiles = 32 - total partition bits) XORed with a scramble of its
  // leading bits: the tiles one workgroup scans lie a multiple of a power of two apart, the plain low bits would repeat)
  Lines16 rec{"cw[j]"};
  if (hll)
    rec.part = "(((hh[j] ^ (cw[j] * 0x9E3779B1u)) * 0x85EBCA6Bu) >> (32 - PB))";
  else if (sort64)
    rec.part = "(a.pad ? (((hh[j] >> a.chunkTiles) ^ ((((hh[j] >> a.chunkTiles) >> PB) * 0x9E3779B1u) >> 23)) & (NP - 1u)) "
               ": (PB ? hh[j] >> (32 - (PB ? PB : 1)) : 0u))";
  kernel_body_lines16(o, s, rec);
  return o.str();
}

// ---- specialised merge ------------------------------------------------------------------------------
// One workgroup per partition, like merge_body<ND, true, 4> (hr_kernels.hpp) for the case the
// specialised scans produce: line records in region B only, previous groups (if any) read
// from their partition-grouped ranges, the whole hash range in one round.  What changes is the cost
// per record: the aggregate, the widening of the carried measure and the dimension expressions are
// literals (the generic kernel spends ~90 VALU + ~120 SALU instructions per record on dispatch), and
// the records a lane holds are probed together — their LDS key reads in flight, then one
// non-returning LDS atomic each for records that meet their group in the first slot (all of them,
// once the groups exist); only misses walk the probe loop.  A partition with more groups than the
// table holds raises a flag and the host runs the generic multi-round merge instead.
// vectorVW = 0: records of the plan-sourced scan (4-byte carried measure, widened here; rows >= prevSize are
// source rows whose dimensions are re-evaluated from the plan's columns), 16-byte lines or — `compact` — compact
// lines.  vectorVW = 4 / 8: records of the vector-sourced scan (the whole value travels; every row, old or new,
// is a row of the input vectors).
// regionA: the partition's records also come from region A — 16-byte {row, hash, value} records, what the TABLE-mode
// scan emits (one per group and workgroup) — ahead of the region-B runs.
// image: the partition's LDS table persists between the HashReduce calls of a query (hash_reduce_lds.hip "table image"):
//   1  the kernel as above, and at the end it leaves its table in HBM — keys (NEWG cleared), the output position of every
//      group where the representative row stood, values: 128 KB per partition, coalesced stores;
//   2  the kernel STARTS from the previous call's image (coalesced loads instead of re-hashing and re-inserting every
//      previous group), takes the batch's records through it, and emits only what is new: dimension rows of the groups
//      first seen in this batch, appended behind the previous result (a group keeps its position for the life of the
//      query), the dimension rows the output vector has not seen yet copied over from the input vector, and the table
//      image again.  The measure vector is NOT written: it is defined by the image (materialised by
//      hr_image_values_kernel when somebody reads it).
std::string generate_merge(const RtcSpec &s) {
  const int nd = s.nd, partBits = s.partBits, image = s.image, vectorVW = s.kind == RTC_VECTOR_MERGE ? s.vectorVW : 0;
  const bool compact = s.compact != 0, regionA = s.regionA != 0;
  if (nd < 1 || nd > kFusedDims) return "";
  if (image && vectorVW) return "";
  if (compact && (vectorVW || partBits < 3)) return "";
  if (partBits < 2) return "";  // the 32-bit table keys need two spare hash bits (small inputs: the generic merge)
  const SlotLayout SL = slot_layout(s.dimWidth, nd, 4);
  if (!SL.ok || (vectorVW && !SL.all4)) return "";
  std::ostringstream o;
  o << kPrelude
    << "struct MArgs { const u32 *vals[" << kFusedCols << "]; const u8 *nulls[" << kFusedCols << "]; const u32 *recB; const u32 *countsB;\n"
       "  const u32 *prevRanges; const u8 *prevDims; const u8 *prevValues; u8 *dimOut; u8 *outValues; u32 *outCount; u32 *outRanges;\n"
       "  u64 prevCapacity, outCapacity; u32 bitOff[" << kFusedCols << "]; u32 capB, streams, prevSize, chunkRows; u64 *phases; u32 k[" << kNumConsts << "]; u32 pad;\n"
       "  const uint4 *recA; const u32 *cursorsA; u64 capA;\n"
       "  const uint4 *imgIn; uint4 *imgOut; const u32 *imgInCount; u32 *imgOutCount; u32 *hostOut; u32 knownOut, pad2; };\n"
       // The call's result words (groups, region overflow, stale ranges, crowded partition) reach the host without a copy
       // command behind the kernel: the workgroup that finishes last writes them into the calling thread's mapped pinned slot
       // (a.hostOut; outCount[4] is the ticket).  The host only waits for the stream.
       "#define FINISH() { __syncthreads(); if (threadIdx.x == 0u && a.hostOut) { __threadfence(); \\\n"
       "  if (atomicAdd(a.outCount + 4, 1u) == gridDim.x - 1u) { __threadfence(); const volatile u32 *oc = a.outCount; \\\n"
       "    a.hostOut[0] = oc[0]; a.hostOut[1] = oc[1]; a.hostOut[2] = oc[2]; a.hostOut[3] = oc[3]; } } }\n"
       "#define ND " << nd << "\n#define VB " << SL.valueBytes << "\n#define PB " << partBits << "\n#define NP " << (1 << partBits) << "\n"
       "#define SLOTS " << hr::kSlots << "\n#define LIMIT " << hr::kMergeLimit << "u\n#define RANGEWORDS " << hr::kRangeWords
    << "\n#define MAXRANGES " << hr::kMaxRanges << "u\n"
       // Table keys are 32 bits: within a partition the top PB bits of every hash are the partition's number, so a
       // key keeps the other 32 - PB bits (HMASK) and uses two of the freed bits as flags — OCC (the slot is taken:
       // an empty slot is 0, "key matches" is one masked compare) and NEWG (the group was first seen in THIS call's
       // records: only then can a record lower the group's representative row — groups that come from the previous
       // result have rows below every row of the batch).  Four keys = one 16-byte LDS read per probe.
       "#define HMASK ((1u << (32 - PB)) - 1u)\n#define OCC 0x40000000u\n#define NEWG 0x80000000u\n";
  gen_widen(o, s);
  if (!gen_agg(o, s)) return "";
  if (s.phases)
    o << "#define STAMP(k) if (threadIdx.x == 0u) a.phases[(u64)blockIdx.x * 8u + (k)] = __builtin_amdgcn_s_memrealtime();\n";
  else
    o << "#define STAMP(k)\n";
  // The table is probed by buckets of four keys (32 bytes, two LDS reads): a record meets its group in
  // its home bucket ~93 % of the time at this load, so a wavefront rarely takes more than two or three
  // rounds — with one key per probe the longest probe sequence among 64 lanes paced every wave.  A
  // lane's records go through the rounds together: their bucket reads are in flight at once.
  // Claims only ever turn the LOWEST empty slot of a bucket into a key, so a hash cannot end up twice.
  o << "#define BUCKETS (SLOTS / 4)\n"
       "struct Probe { u32 b, slot; bool done, isNew; };\n"
       // One round for one record, written without branches except for the rare claim: the merge is bound by
       // instruction issue (divergent control flow costs ~6 scalar instructions per `if`), not by LDS or HBM.
       // want = the occupied key of the record's hash; claimKey = want, with NEWG for a record of the batch.
       "__device__ __forceinline__ void probe_round(u32 *sKeys, u32 *sClaimed, u32 *sOverflow, Probe &q, u32 want, u32 claimKey) {\n"
       "  const uint4 k = *reinterpret_cast<const uint4 *>(sKeys + 4u * q.b);\n"
       "  const bool e0 = k.x == 0u, e1 = k.y == 0u, e2 = k.z == 0u, e3 = k.w == 0u;\n"
       "  const bool m0 = (k.x & ~NEWG) == want, m1 = (k.y & ~NEWG) == want, m2 = (k.z & ~NEWG) == want, m3 = (k.w & ~NEWG) == want;\n"
       "  const bool anyM = m0 | m1 | m2 | m3, anyE = e0 | e1 | e2 | e3;\n"
       "  const u32 mi = m0 ? 0u : m1 ? 1u : m2 ? 2u : 3u, ei = e0 ? 0u : e1 ? 1u : e2 ? 2u : 3u;\n"
       "  const u32 mk = m0 ? k.x : m1 ? k.y : m2 ? k.z : k.w;\n"
       "  const bool active = !q.done, hit = active & anyM;\n"
       "  q.slot = hit ? 4u * q.b + mi : q.slot;\n"
       "  q.isNew = hit ? (mk & NEWG) != 0u : q.isNew;\n"
       "  bool claimed = false;\n"
       "  if (active & !anyM & anyE) {\n"  // a group that is new in this partition: rare once the groups exist
       "    u32 expected = 0u;\n"
       "    if (__hip_atomic_compare_exchange_strong(sKeys + 4u * q.b + ei, &expected, claimKey, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {\n"
       "      if (__hip_atomic_fetch_add(sClaimed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= LIMIT)\n"
       "        __hip_atomic_store(sOverflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
       "      q.slot = 4u * q.b + ei; q.isNew = true; claimed = true;\n"  // (the claimer lowers the row too: rows start at ~0)
       "    }\n"  // lost the slot: the same bucket again next round (the winner may be this very group)
       "  }\n"
       "  q.b = (active & !anyM & !anyE) ? (q.b + 1u) & (BUCKETS - 1u) : q.b;\n"
       "  q.done = q.done | hit | claimed;\n"
       "}\n"
       // one record through the general probe loop; batch = a record of this call's batch (may found a NEWG group)
       "__device__ __forceinline__ void insert(u32 *sKeys, u32 *sRows, u64 *sVals, u32 *sClaimed, u32 *sOverflow, u32 row, u32 h, u64 value, bool batch) {\n"
       "  const u32 want = (h & HMASK) | OCC;\n"
       "  Probe q; q.b = h & (BUCKETS - 1u); q.slot = 0u; q.done = false; q.isNew = false;\n"
       "  for (u32 tries = 0u; tries < 4u * BUCKETS && !q.done; tries++) probe_round(sKeys, sClaimed, sOverflow, q, want, batch ? want | NEWG : want);\n"
       "  if (q.done) {\n"
       "    if (q.isNew || !batch) __hip_atomic_fetch_min(sRows + q.slot, row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
       "    agg(sVals + q.slot, value);\n"
       "  } else {\n"
       "    __hip_atomic_store(sOverflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"  // table full: the round is void anyway
       "  }\n"
       "}\n";
  // Records arrive in segments of 64 sixteen-byte units (one per lane), four segments per register stage — of
  // one long run or of four short ones (small batches leave ~16 records per run: a stage per run would make the
  // merge a chain of dependent loads).  Round one looks at every record's home bucket with straight-line
  // code (no claim, no advance): a record whose group sits there — ~93 % once the groups exist — costs one
  // LDS atomic more.  The rest (the group lives further on, or is new) is queued per wavefront in LDS and
  // taken through the general probe loop 64 at a time, every lane busy: run per record where it occurs,
  // that loop would execute for a handful of lanes after nearly every segment.
  if (vectorVW == 8)  // four words per queued record: a smaller queue, drained from 32 entries on (LDS is full)
    o << "#define QCAP 96u\n#define QW 4u\n#define QDRAIN 32u\n#define VALB(z, w) ((((u64)(w)) << 32) | (z))\n";
  else if (vectorVW == 4)
    o << "#define QCAP 128u\n#define QW 3u\n#define QDRAIN 64u\n#define VALB(z, w) ((u64)(z))\n";
  else
    o << "#define QCAP 128u\n#define QW 3u\n#define QDRAIN 64u\n#define VALB(z, w) widen(z)\n";
  o << "struct Seg { const uint4 *ptr; u32 n, rem, rb; };\n"
       "struct Stage { uint4 r[4]; u32 n[4], rem[4], rb[4]; };\n"
       "__device__ __forceinline__ void drain(u32 *queue, u32 first, u32 count, u32 lane, u32 *sKeys, u32 *sRows, u64 *sVals, u32 *sClaimed, u32 *sOverflow) {\n"
       "  asm volatile(\"s_waitcnt lgkmcnt(0)\" ::: \"memory\");\n"
       "  if (lane < count) {\n"
       "    const u32 e = QW * (first + lane);\n"
       "    const u32 row = queue[e], h = queue[e + 1u], z = queue[e + 2u], w = QW == 4u ? queue[e + QW - 1u] : 0u;\n"
       "    insert(sKeys, sRows, sVals, sClaimed, sOverflow, row, h, VALB(z, w), true);\n"
       "  }\n"
       "  asm volatile(\"s_waitcnt lgkmcnt(0)\" ::: \"memory\");\n"
       "}\n"
       // one record in round one
       "__device__ __forceinline__ void consume_one(bool valid, u32 row, u32 h, u32 z, u32 w, u32 lane, u32 *sKeys, u32 *sRows, u64 *sVals, u32 *sClaimed, u32 *sOverflow, u32 *queue, u32 &qn) {\n"
       "  const u32 b = h & (BUCKETS - 1u), want = (h & HMASK) | OCC;\n"
       "  const uint4 k = *reinterpret_cast<const uint4 *>(sKeys + 4u * b);\n"
       "  const bool m0 = (k.x & ~NEWG) == want, m1 = (k.y & ~NEWG) == want, m2 = (k.z & ~NEWG) == want, m3 = (k.w & ~NEWG) == want;\n"
       "  const bool hit = valid && (m0 || m1 || m2 || m3);\n"
       "  if (hit) {\n"
       "    const u32 mi = m0 ? 0u : m1 ? 1u : m2 ? 2u : 3u;\n"
       "    const u32 mk = m0 ? k.x : m1 ? k.y : m2 ? k.z : k.w;\n"
       "    if (mk & NEWG) __hip_atomic_fetch_min(sRows + 4u * b + mi, row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
       "    agg(sVals + 4u * b + mi, VALB(z, w));\n"
       "  }\n"
       "  const bool pend = valid && !hit;\n"
       "  const u64 m = __ballot(pend);\n"
       "  if (m) {\n"
       "    if (pend) {\n"
       "      const u32 e = QW * (qn + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u)));\n"
       "      queue[e] = row; queue[e + 1u] = h; queue[e + 2u] = z;\n"
       "      if (QW == 4u) queue[e + QW - 1u] = w;\n"
       "    }\n"
       "    qn += (u32)__popcll(m);\n"
       "    if (qn >= QDRAIN) { const u32 take = qn < 64u ? qn : 64u; qn -= take; drain(queue, qn, take, lane, sKeys, sRows, sVals, sClaimed, sOverflow); }\n"
       "  }\n"
       "}\n";
  if (compact)
    // a 16-byte unit holds two 8-byte slots of a line: lanes 8l .. 8l + 7 hold line l of the segment, the first
    // slot of lanes 8l and 8l + 4 is a header (low 9 row bits of the half-line's seven records)
    o << "__device__ __forceinline__ void consume(const Stage &s, u32 lane, u32 p, u32 *sKeys, u32 *sRows, u64 *sVals, u32 *sClaimed, u32 *sOverflow, u32 *queue, u32 &qn) {\n"
         "  const u32 pos = 2u * (lane & 3u);\n"                       // place of the unit's first slot within its half-line
         "  const u32 recBase = (lane >> 3) * 14u + 7u * ((lane >> 2) & 1u);\n"  // record number (within the segment) of the half-line's first record
         "#pragma unroll\n"
         "  for (int k = 0; k < 4; k++) {\n"
         "    const u64 hdr = ((u64)(u32)__builtin_amdgcn_mov_dpp((int)s.r[k].y, 0x00, 0xF, 0xF, true) << 32) | (u32)__builtin_amdgcn_mov_dpp((int)s.r[k].x, 0x00, 0xF, 0xF, true);\n"
         "#pragma unroll\n"
         "    for (u32 j = 0u; j < 2u; j++) {\n"
         "      const u32 ph = pos + j;\n"                             // 0 = the header slot
         "      const u32 k7 = ph ? ph - 1u : 0u;\n"
         "      const bool valid = lane < s.n[k] && ph != 0u && recBase + k7 < s.rem[k];\n"
         "      const u32 z = j ? s.r[k].z : s.r[k].x, hw = j ? s.r[k].w : s.r[k].y;\n"
         "      const u32 lo9 = (u32)(hdr >> (9u * k7)) & 511u;\n"
         "      const u32 h = (p << (32 - PB)) | (hw >> PB);\n"
         "      const u32 row = s.rb[k] + (((hw & ((1u << PB) - 1u)) << 9) | lo9);\n"
         "      consume_one(valid, row, h, z, 0u, lane, sKeys, sRows, sVals, sClaimed, sOverflow, queue, qn);\n"
         "    }\n"
         "  }\n"
         "}\n";
  else
    o << "__device__ __forceinline__ void consume(const Stage &s, u32 lane, u32 p, u32 *sKeys, u32 *sRows, u64 *sVals, u32 *sClaimed, u32 *sOverflow, u32 *queue, u32 &qn) {\n"
         "#pragma unroll\n"
         "  for (int k = 0; k < 4; k++) {\n"
         "    const bool valid = lane < s.n[k] && s.r[k].x != 0xFFFFFFFFu;\n"  // not past the segment / padding of the run's last line
         "    consume_one(valid, s.r[k].x, s.r[k].y, s.r[k].z, s.r[k].w, lane, sKeys, sRows, sVals, sClaimed, sOverflow, queue, qn);\n"
         "  }\n"
         "}\n";
  // dimensions of a source row (hr::fused_eval_row), for groups that are new in this batch
  if (!vectorVW) o << "__device__ __forceinline__ void eval_row(const MArgs &a, u32 row, u32 (&bits)[ND], u32 (&ok)[ND]) {\n";
  for (int d = 0; d < nd && !vectorVW; d++) {
    const RtcExpr &e = s.dims[d];
    const int c = e.col;
    if (c < 0 || c >= kFusedCols || !plain_store(e.rk, e.outKind) || (SL.width[d] != 4 && !int_kind(e.rk))) return "";
    o << "  {\n    const u32 v = " << column_elem(s.step[c], e.akind == K_I32, "a.vals[" + std::to_string(c) + "]", "row") << ";\n";
    if (s.nullMask & (1u << c)) o << "    const u32 bit = row + a.bitOff[" << c << "]; const u32 okb = (a.nulls[" << c << "][bit >> 3] >> (bit & 7u)) & 1u;\n";
    else o << "    const u32 okb = 1u;\n";
    o << "    u32 x;\n";
    if (!gen_value(e, o, "v", "okb", "x", const_name(const_slot_dim(d)), const_slot_dim_chain(d))) return "";
    o << "    bits[" << d << "] = x; ok[" << d << "] = okb;\n  }\n";
  }
  if (!vectorVW) o << "}\n";
  const bool wide = s.aggWidth == 8;
  o << "extern \"C\" __global__ void __launch_bounds__(1024) hr_merge_rtc(MArgs a) {\n"
       "  __shared__ __attribute__((aligned(16))) u32 sKeys[SLOTS];\n"
       "  __shared__ __attribute__((aligned(16))) u32 sRows[SLOTS];\n"
       "  __shared__ __attribute__((aligned(16))) u64 sVals[SLOTS];\n"
       "  __shared__ u32 sRunCount[256];\n"
       "  __shared__ u32 sQueue[16u * QCAP * QW];\n"
       "  __shared__ u32 sClaimed, sOverflow, sCount, sBase, sEmit;\n"
       "  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, p = blockIdx.x;\n"
       "  STAMP(0)\n";
  if (image == 2)  // the table as the query's previous HashReduce left it
    o << "  {\n"
         "    const uint4 *img = a.imgIn + (u64)p * SLOTS;\n"
         "    for (u32 i = tid; i < SLOTS / 4u; i += 1024u) {\n"
         "      reinterpret_cast<uint4 *>(sKeys)[i] = img[i];\n"
         "      reinterpret_cast<uint4 *>(sRows)[i] = img[SLOTS / 4u + i];\n"
         "    }\n"
         "    for (u32 i = tid; i < SLOTS / 2u; i += 1024u) reinterpret_cast<uint4 *>(sVals)[i] = img[SLOTS / 2u + i];\n"
         "    if (tid == 0u) { sClaimed = a.imgInCount[p]; sOverflow = 0u; sCount = 0u; sEmit = 0u; }\n"
         "  }\n";
  else
    o << "  for (u32 s = tid; s < SLOTS; s += 1024u) { sKeys[s] = 0u; sRows[s] = 0xFFFFFFFFu; sVals[s] = IDENT; }\n"
         "  if (tid == 0u) { sClaimed = 0u; sOverflow = 0u; sCount = 0u; sEmit = 0u; }\n";
  o << "  const u32 G = a.streams;\n"
       "  if (tid < G) sRunCount[tid] = a.countsB[(u64)tid * NP + p];\n"
       "  const u32 *ranges = a.prevRanges ? a.prevRanges + (u64)p * RANGEWORDS : nullptr;\n"
       "  u32 nRanges = ranges ? ranges[0] : 0u;\n"
       "  if (nRanges > MAXRANGES) { if (tid == 0u) a.outCount[2] = 1u; nRanges = 0u; }\n"
       "  __syncthreads();\n"
       "  STAMP(1)\n"
       // previous groups of this partition (always the lowest row indices: they stay the representatives)
       "  {\n"
       "    const u8 *nullsIn = a.prevDims + (u64)VB * a.prevCapacity;\n"
       "    for (u32 r = 0u; r < nRanges; r++) {\n"
       "      const u32 start = ranges[1u + 2u * r], cnt = ranges[2u + 2u * r];\n"
       "      for (u32 i0 = 0u; i0 < cnt; i0 += 4096u) {\n"  // four groups per lane: their loads are in flight together
       "        u32 hh[4], rr[4]; u64 vv[4]; bool okk[4];\n"
       "#pragma unroll\n"
       "        for (int k = 0; k < 4; k++) {\n"
       "          const u32 i = i0 + (u32)k * 1024u + tid;\n"
       "          okk[k] = i < cnt;\n"
       "          const u32 row = start + (okk[k] ? i : 0u);\n"
       "          rr[k] = row;\n"
       "          okk[k] = okk[k] && row < a.prevSize;\n"
       "          const u32 safe = row < a.prevSize ? row : 0u;\n"
       "          u32 h = 0u;\n";
  if (SL.all4) {
    o << "          u32 okbytes = 0u;\n"
         "#pragma unroll\n"
         "          for (int d = 0; d < ND; d++) {\n"
         "            h = mix(h, *reinterpret_cast<const u32 *>(a.prevDims + (u64)(4 * d) * a.prevCapacity + 4ull * safe));\n"
         "            okbytes |= (u32)nullsIn[(u64)d * a.prevCapacity + safe] << (8 * d);\n"
         "          }\n";
    if (nd == 4) o << "          h = mix(h, okbytes);\n";
    else o << "          { u32 kk = okbytes * 0xcc9e2d51u; kk = rotl(kk, 15) * 0x1b873593u; h ^= kk; }\n";
    o << "          h ^= " << 5 * nd << "u; h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;\n";
  } else {
    for (int d = 0; d < nd; d++)
      o << "          const u32 pv" << d << " = " << slot_load(SL, d, "a.prevDims", "a.prevCapacity", "safe") << ", po" << d
        << " = (u32)nullsIn[(u64)" << d << " * a.prevCapacity + safe];\n";
    gen_row_hash(o, SL, [](int d) { return "pv" + std::to_string(d); }, [](int d) { return "po" + std::to_string(d); }, "h", "          ");
  }
  o <<
       "          hh[k] = h;\n"
    << (wide ? "          vv[k] = reinterpret_cast<const u64 *>(a.prevValues)[safe];\n"
             : "          vv[k] = reinterpret_cast<const u32 *>(a.prevValues)[safe];\n")
    << "        }\n"
       "#pragma unroll\n"
       "        for (int k = 0; k < 4; k++) {\n"
       "          const u32 i = i0 + (u32)k * 1024u + tid;\n"
       "          if (i >= cnt) continue;\n"
       "          if (!okk[k] || (PB && (hh[k] >> (32 - (PB ? PB : 1))) != p)) { a.outCount[2] = 1u; continue; }\n"
       "          insert(sKeys, sRows, sVals, &sClaimed, &sOverflow, rr[k], hh[k], vv[k], false);\n"
       "        }\n"
       "      }\n"
       "    }\n"
       "  }\n"
       "  __syncthreads();\n"
       "  STAMP(2)\n";
  if (regionA)  // what the TABLE-mode scan left in region A: one record per group and scanning workgroup
    o << "  {\n"
         "    const u32 cur = a.cursorsA[p];\n"
         "    const u32 nA = cur < a.capA ? cur : (u32)a.capA;\n"
         "    const uint4 *recs = a.recA + (u64)p * a.capA;\n"
         "    for (u32 i = tid; i < nA; i += 1024u) {\n"
         "      const uint4 r = recs[i];\n"
         "      insert(sKeys, sRows, sVals, &sClaimed, &sOverflow, r.x, r.y, ((u64)r.w << 32) | r.z, true);\n"
         "    }\n"
         "  }\n"
         "  __syncthreads();\n";
  // Small batches (live batches: 2 Mi rows, 512 tiles, two per scanning workgroup) leave every partition a few hundred runs
  // of a dozen or two records — one to three lines each.  Walking them run by run, sixteen per wavefront, is a chain of
  // dependent loads (20 us of a partition's 33 at 2 Mi rows); when no run is longer than four lines, the first L lines of
  // EVERY run of the partition are fetched at once instead (L = lines of the longest run): a few 16-byte loads per lane, all
  // in flight together.
  o << "  u32 maxRun = 0u;\n"
       "  for (u32 g = lane; g < G; g += 64u) { const u32 c = sRunCount[g]; maxRun = c > maxRun ? c : maxRun; }\n"
       "#pragma unroll\n"
       "  for (int off = 32; off > 0; off >>= 1) { const u32 t = (u32)__shfl_xor((int)maxRun, off); maxRun = t > maxRun ? t : maxRun; }\n"
       "  const u32 LPR = (maxRun + " << (compact ? "13u) / 14u" : "7u) / 8u") << ";\n"   // lines of the longest run
       "  if (G > 0u && LPR <= 4u && LPR <= a.capB" << (compact ? "" : " / 8u") << ") {\n"
       "    u32 qn = 0u;\n"
       "    u32 *queue = sQueue + wave * (QCAP * QW);\n"
       "    const u32 units = G * 8u * LPR;\n"
       "    for (u32 base = 0u; base < units; base += 4096u) {\n"
       "      Stage s;\n"
       "#pragma unroll\n"
       "      for (int k = 0; k < 4; k++) {\n"
       "        const u32 u = base + (u32)k * 1024u + tid;\n"  // unit u = lane (u & 7) of line (u >> 3) % LPR of stream (u >> 3) / LPR
       "        const bool in = u < units;\n"
       "        const u32 ul = in ? u >> 3 : 0u, g = ul / LPR, l = ul - g * LPR, cnt = in ? sRunCount[g] : 0u;\n"
    << (compact ? "        const u32 here = cnt > l * 14u ? cnt - l * 14u : 0u;\n"   // records of the run in this line and behind it
                  "        s.r[k] = reinterpret_cast<const uint4 *>(a.recB)[(((u64)g * NP + p) * a.capB + l) * 8u + (u & 7u)];\n"
                  "        s.n[k] = here ? 64u : 0u; s.rem[k] = (lane >> 3) * 14u + here; s.rb[k] = a.prevSize + g * a.chunkRows;\n"
                : "        const u32 here = cnt > l * 8u ? cnt - l * 8u : 0u;\n"
                  "        s.r[k] = reinterpret_cast<const uint4 *>(a.recB)[((u64)g * NP + p) * a.capB + l * 8u + (u & 7u)];\n"
                  "        s.n[k] = (u & 7u) < here ? 64u : 0u; s.rem[k] = 0u; s.rb[k] = 0u;\n")
    << "      }\n"
       "      consume(s, lane, p, sKeys, sRows, sVals, &sClaimed, &sOverflow, queue, qn);\n"
       "    }\n"
       "    while (qn) { const u32 take = qn < 64u ? qn : 64u; qn -= take; drain(queue, qn, take, lane, sKeys, sRows, sVals, &sClaimed, &sOverflow); }\n"
       "  } else\n"
       // the partition's runs: every wavefront streams whole runs, three register stages
       "  if (G > 0u) {\n"
       "    const uint4 *dummy = reinterpret_cast<const uint4 *>(a.recB);\n"
       "    u32 j = 0u, off = 0u, qn = 0u;\n"
       "    u32 *queue = sQueue + wave * (QCAP * QW);\n"
       // this wavefront's runs are wave, wave + 16, ...: lane i keeps the length of the i-th of them, so that
       // walking the runs costs no LDS round trip per segment
       "    const u32 myRuns = (G + 15u - wave) / 16u;\n"
       "    const u32 myCnt = lane < myRuns ? sRunCount[wave + 16u * lane] : 0u;\n";
  if (compact)
    o << "    auto next = [&]() -> Seg {\n"
         "      Seg c{dummy, 0u, 0u, 0u};\n"
         "      while (j < myRuns) {\n"
         "        const u32 cnt = (u32)__builtin_amdgcn_readlane((int)myCnt, (int)j);\n"
         "        const u32 units = ((cnt + 13u) / 14u) * 8u;\n"         // whole lines, eight 16-byte units each
         "        if (off < units) {\n"
         "          c.ptr = reinterpret_cast<const uint4 *>(a.recB) + ((u64)(wave + 16u * j) * NP + p) * a.capB * 8u + off;\n"
         "          c.n = units - off < 64u ? units - off : 64u;\n"
         "          c.rem = cnt - (off >> 3) * 14u;\n"
         "          c.rb = a.prevSize + (wave + 16u * j) * a.chunkRows;\n"
         "          off += 64u;\n"
         "          break;\n"
         "        }\n"
         "        j++; off = 0u;\n"
         "      }\n"
         "      return c;\n"
         "    };\n";
  else
    o << "    auto next = [&]() -> Seg {\n"
         "      Seg c{dummy, 0u, 0u, 0u};\n"
         "      while (j < myRuns) {\n"
         "        const u32 cnt = (u32)__builtin_amdgcn_readlane((int)myCnt, (int)j);\n"
         "        if (off < cnt) {\n"
         "          c.ptr = reinterpret_cast<const uint4 *>(a.recB) + ((u64)(wave + 16u * j) * NP + p) * a.capB + off;\n"
         "          c.n = cnt - off < 64u ? cnt - off : 64u;\n"
         "          off += 64u;\n"
         "          break;\n"
         "        }\n"
         "        j++; off = 0u;\n"
         "      }\n"
         "      return c;\n"
         "    };\n";
  o << "    auto load = [&](Stage &s) {\n"
       "#pragma unroll\n"
       "      for (int k = 0; k < 4; k++) {\n"
       "        const Seg c = next();\n"
       "        s.n[k] = c.n; s.rem[k] = c.rem; s.rb[k] = c.rb;\n"
       "        s.r[k] = c.ptr[lane < c.n ? lane : (c.n ? c.n - 1u : 0u)];\n"
       "      }\n"
       "    };\n"
       // three register stages: two stages of loads are always in flight behind the one being consumed
       "    Stage s0, s1, s2;\n"
       "    load(s0);\n"
       "    load(s1);\n"
       "    for (;;) {\n"
       "      load(s2);\n"
       "      if (!s0.n[0]) break;\n"
       "      consume(s0, lane, p, sKeys, sRows, sVals, &sClaimed, &sOverflow, queue, qn);\n"
       "      load(s0);\n"
       "      if (!s1.n[0]) break;\n"
       "      consume(s1, lane, p, sKeys, sRows, sVals, &sClaimed, &sOverflow, queue, qn);\n"
       "      load(s1);\n"
       "      if (!s2.n[0]) break;\n"
       "      consume(s2, lane, p, sKeys, sRows, sVals, &sClaimed, &sOverflow, queue, qn);\n"
       "    }\n"
       "    while (qn) { const u32 take = qn < 64u ? qn : 64u; qn -= take; drain(queue, qn, take, lane, sKeys, sRows, sVals, &sClaimed, &sOverflow); }\n"
       "  }\n"
       "  __syncthreads();\n"
       "  STAMP(3)\n"
       "  if (sOverflow) { if (tid == 0u) a.outCount[3] = 1u; FINISH() return; }\n";  // more groups than one table: the generic merge takes over
  // the image's three planes leave (or reach) a partition with 16-byte accesses, consecutive lanes consecutive addresses
  const char *kStoreKeysPos =
      "    for (u32 i = tid; i < SLOTS / 4u; i += 1024u) {\n"
      "      img[i] = reinterpret_cast<const uint4 *>(sKeys)[i];\n"
      "      img[SLOTS / 4u + i] = reinterpret_cast<const uint4 *>(sRows)[i];\n"
      "    }\n";
  const char *kStoreVals = "    for (u32 i = tid; i < SLOTS / 2u; i += 1024u) img[SLOTS / 2u + i] = reinterpret_cast<const uint4 *>(sVals)[i];\n";
  if (image == 2) {
    // ---- groups first seen in this batch: their dimension rows, appended behind the previous result -------------------
    o << "  u32 mineNew = 0u;\n"
         "#pragma unroll\n"
         "  for (int k = 0; k < SLOTS / 1024; k++) mineNew += (sKeys[tid + (u32)k * 1024u] & NEWG) != 0u;\n"
         "  if (mineNew) __hip_atomic_fetch_add(&sCount, mineNew, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
         "  __syncthreads();\n"
         "  const u32 totalNew = sCount;\n"
         "  if (tid == 0u) sBase = a.prevSize + (totalNew ? atomicAdd(a.outCount, totalNew) : 0u);\n"  // (outCount counts the NEW groups)
         "  __syncthreads();\n"
         "  STAMP(4)\n"
         "  u8 *nullsOut = a.dimOut + (u64)VB * a.outCapacity;\n"
         "  if (totalNew) {\n"
         "#pragma unroll\n"
         "    for (int half = 0; half < 2; half++) {\n"
         "      u32 dv[4][ND], nv[4][ND], at[4]; bool has[4];\n"
         "#pragma unroll\n"
         "      for (int kk = 0; kk < 4; kk++) {\n"
         "        const u32 s = tid + (u32)(half * 4 + kk) * 1024u;\n"
         "        has[kk] = (sKeys[s] & NEWG) != 0u;\n"
         "        const u64 m = __ballot(has[kk]);\n"
         "        u32 waveBase = 0u;\n"
         "        if (lane == 0u && m) waveBase = __hip_atomic_fetch_add(&sEmit, (u32)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
         "        waveBase = (u32)__builtin_amdgcn_readfirstlane((int)waveBase);\n"
         "        at[kk] = sBase + waveBase + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));\n"
         "        if (has[kk]) eval_row(a, sRows[s] - a.prevSize, dv[kk], nv[kk]);\n"  // (a new group's representative is a row of the batch)
         "      }\n"
         "#pragma unroll\n"
         "      for (int kk = 0; kk < 4; kk++) {\n"
         "        if (!has[kk]) continue;\n"
         "        const u32 s = tid + (u32)(half * 4 + kk) * 1024u;\n";
    for (int d = 0; d < nd; d++)
      o << "        " << slot_store(SL, d, "a.dimOut", "a.outCapacity", "at[kk]", "dv[kk][" + std::to_string(d) + "]") << " nullsOut[(u64)" << d
        << " * a.outCapacity + at[kk]] = (u8)nv[kk][" << d << "];\n";
    o << "        sRows[s] = at[kk];\n"       // from now on the slot holds the group's position
         "        sKeys[s] &= ~NEWG;\n"
         "      }\n"
         "    }\n"
         "  }\n"
         "  __syncthreads();\n"
         // ---- the image again: values always; keys and positions unless the output's image already holds this very set
         // (a partition's count only grows, and both images descend from one table: equal counts = equal key planes)
         "  {\n"
         "    uint4 *img = a.imgOut + (u64)p * SLOTS;\n"
         "    const u32 newCount = a.imgInCount[p] + totalNew;\n"
         "    if (a.imgOutCount[p] != newCount) {\n"
      << kStoreKeysPos
      << "    }\n"
      << kStoreVals
      << "    __syncthreads();\n"
         "    if (tid == 0u) a.imgOutCount[p] = newCount;\n"
         "  }\n"
         // ---- dimension rows [knownOut, prevSize) the output vector has not seen yet: this workgroup's share, copied over
         "  if (a.knownOut < a.prevSize) {\n"
         "    const u8 *nullsIn = a.prevDims + (u64)VB * a.prevCapacity;\n"
         "    const u32 n = a.prevSize - a.knownOut, share = (n + NP - 1u) / NP;\n"
         "    const u32 lo = a.knownOut + p * share, hi = lo + share < a.prevSize ? lo + share : a.prevSize;\n"
         "    for (u32 r = lo + tid; r < hi; r += 1024u) {\n";
    for (int d = 0; d < nd; d++)
      o << "      " << slot_store(SL, d, "a.dimOut", "a.outCapacity", "r", slot_load(SL, d, "a.prevDims", "a.prevCapacity", "r")) << " nullsOut[(u64)" << d
        << " * a.outCapacity + r] = nullsIn[(u64)" << d << " * a.prevCapacity + r];\n";
    o << "    }\n"
         "  }\n"
         "  STAMP(5)\n"
         "  FINISH()\n"
         "}\n";
    return o.str();
  }
  o << // emit: count occupied slots, reserve output rows once, then copy (as hr::merge_body)
       "  u32 mineCount = 0u;\n"
       "#pragma unroll\n"
       "  for (int k = 0; k < SLOTS / 1024; k++) mineCount += sKeys[tid + (u32)k * 1024u] != 0u;\n"
       "  if (mineCount) __hip_atomic_fetch_add(&sCount, mineCount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
       "  __syncthreads();\n"
       "  const u32 total = sCount;\n"
       "  if (tid == 0u) {\n"
       "    u32 base = 0u;\n"
       "    if (total) base = atomicAdd(a.outCount, total);\n"
       "    sBase = base;\n"
       "    if (a.outRanges) { u32 *o = a.outRanges + (u64)p * RANGEWORDS; o[0] = total ? 1u : 0u; o[1] = base; o[2] = total; }\n"
       "  }\n"
       "  __syncthreads();\n"
       "  STAMP(4)\n"
    << (image == 1 ? "" : "  if (!total) { FINISH() return; }\n")  // (an empty partition leaves an empty image)
    << "  const u8 *nullsIn = a.prevDims + (u64)VB * a.prevCapacity;\n"
       "  u8 *nullsOut = a.dimOut + (u64)VB * a.outCapacity;\n"
       "#pragma unroll\n"
       "  for (int half = 0; half < 2; half++) {\n"
       "    u32 dv[4][ND], nv[4][ND], at[4]; bool has[4];\n"
       "#pragma unroll\n"
       "    for (int kk = 0; kk < 4; kk++) {\n"
       "      const u32 s = tid + (u32)(half * 4 + kk) * 1024u;\n"
       "      has[kk] = sKeys[s] != 0u;\n"
       "      const u64 m = __ballot(has[kk]);\n"
       "      u32 waveBase = 0u;\n"
       "      if (lane == 0u && m) waveBase = __hip_atomic_fetch_add(&sEmit, (u32)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
       "      waveBase = (u32)__builtin_amdgcn_readfirstlane((int)waveBase);\n"
       "      at[kk] = sBase + waveBase + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));\n"
       "      if (!has[kk]) continue;\n"
       "      const u32 row = sRows[s];\n"
    << (vectorVW ? "" : "      if (row >= a.prevSize) { eval_row(a, row - a.prevSize, dv[kk], nv[kk]); continue; }\n");
  if (SL.all4) {
    o << "#pragma unroll\n"
         "      for (int d = 0; d < ND; d++) {\n"
         "        dv[kk][d] = *reinterpret_cast<const u32 *>(a.prevDims + (u64)(4 * d) * a.prevCapacity + 4ull * row);\n"
         "        nv[kk][d] = nullsIn[(u64)d * a.prevCapacity + row];\n"
         "      }\n";
  } else {
    for (int d = 0; d < nd; d++)
      o << "      dv[kk][" << d << "] = " << slot_load(SL, d, "a.prevDims", "a.prevCapacity", "row") << "; nv[kk][" << d << "] = nullsIn[(u64)" << d
        << " * a.prevCapacity + row];\n";
  }
  o << "    }\n"
       "#pragma unroll\n"
       "    for (int kk = 0; kk < 4; kk++) {\n"
       "      if (!has[kk]) continue;\n"
       "      const u32 s = tid + (u32)(half * 4 + kk) * 1024u;\n";
  if (SL.all4) {
    o << "#pragma unroll\n"
         "      for (int d = 0; d < ND; d++) {\n"
         "        *reinterpret_cast<u32 *>(a.dimOut + (u64)(4 * d) * a.outCapacity + 4ull * at[kk]) = dv[kk][d];\n"
         "        nullsOut[(u64)d * a.outCapacity + at[kk]] = (u8)nv[kk][d];\n"
         "      }\n";
  } else {
    for (int d = 0; d < nd; d++)
      o << "      " << slot_store(SL, d, "a.dimOut", "a.outCapacity", "at[kk]", "dv[kk][" + std::to_string(d) + "]") << " nullsOut[(u64)" << d
        << " * a.outCapacity + at[kk]] = (u8)nv[kk][" << d << "];\n";
  }
  o << (wide ? "      reinterpret_cast<u64 *>(a.outValues)[at[kk]] = sVals[s];\n"
             : "      reinterpret_cast<u32 *>(a.outValues)[at[kk]] = (u32)sVals[s];\n")
    << (image == 1 ? "      sRows[s] = at[kk];\n      sKeys[s] &= ~NEWG;\n" : "")  // the image: a group's slot holds its position
    << "    }\n"
       "  }\n";
  if (image == 1)
    o << "  __syncthreads();\n"
         "  {\n"
         "    uint4 *img = a.imgOut + (u64)p * SLOTS;\n"
      << kStoreKeysPos << kStoreVals
      << "    if (tid == 0u) a.imgOutCount[p] = total;\n"
         "  }\n";
  o <<
       "  STAMP(5)\n"
       "  FINISH()\n"
       "}\n";
  return o.str();
}

enum ExprRole { FILTER, DIMENSION, MEASURE };
// filters go through gen_compare, dimensions and the measure through gen_value: what the other does not read stays zero
RtcExpr spec_expr(const FusedExpr &e, ExprRole role) {
  RtcExpr x{};
  x.col = e.col; x.akind = e.f.akind; x.arity = e.f.arity; x.I = e.f.I;
  if (role != FILTER) x.rk = e.f.rk;
  if (role == DIMENSION) x.outKind = e.outKind;
  if (e.f.arity != 2) return x;  // (a bare column, or declined: the second operand is not looked at)
  x.functor = e.f.functor; x.bok = e.f.bok != 0;
  if (role == FILTER) return x;
  x.bkind = e.f.bkind; x.divLike = e.f.divLike != 0;
  if (x.divLike) x.bbits = e.f.bbits;
  // a chain's steps; one this struct cannot hold (or the generator would not answer) declines the whole expression: akind 0
  x.chainN = e.f.chain.n;
  if (x.chainN < 0 || x.chainN > kMaxChainSteps) return RtcExpr{};
  for (int k = 0; k < x.chainN; k++) {
    const FastStep &st = e.f.chain.s[k];
    x.chain[k].functor = st.functor; x.chain[k].I = st.I; x.chain[k].divLike = st.divLike != 0;
    if (st.divLike) x.chain[k].bbits = st.bbits;
  }
  return x;
}
RtcSpec spec_of(RtcKind kind, int nd, int partBits, bool stamps = true) {
  RtcSpec s{};
  s.kind = kind; s.nd = nd; s.partBits = partBits;
  s.phases = stamps && phases_enabled();
  return s;
}
void spec_column(RtcSpec &s, const FusedPlanD &plan, int c) {
  s.step[c] = fused_col_step(plan, c);
  if (plan.cols[c].nulls) s.nullMask |= 1u << c;
}
void spec_dims(RtcSpec &s, const FusedPlanD &plan) {
  for (int d = 0; d < s.nd && d < kFusedDims; d++) {
    s.dimWidth[d] = fused_dim_width(plan, d);
    s.dims[d] = spec_expr(plan.dims[d], DIMENSION);
  }
}
void spec_agg(RtcSpec &s, const AggSpec &a, const hr::Widen &w) {
  s.aggVtype = a.vtype; s.aggIdentity = a.identity;
  if (a.vtype == V_U32 || a.vtype == V_I32) s.aggOp = a.op;  // (the wider and the float aggregates only sum)
  s.widenMode = w.mode;
  if (w.mode) { s.widenRk = w.rk; s.widenDtype = w.dtype; }
}
RtcSpec spec_plan_scan(RtcKind kind, const FusedPlanD &plan, int nd, int partBits) {
  RtcSpec s = spec_of(kind, nd, partBits, kind != RTC_SCAN_TABLE);  // (the TABLE scan has no time stamps)
  s.numCols = plan.numCols; s.numFilters = plan.numFilters;
  for (int c = 0; c < plan.numCols && c < kFusedCols; c++) spec_column(s, plan, c);
  for (int k = 0; k < plan.numFilters && k < kFusedFilters; k++) s.filters[k] = spec_expr(plan.filters[k], FILTER);
  spec_dims(s, plan);
  s.measureAvg = plan.measureAvg != 0;
  s.constMeasure = plan.measure.col < 0;
  if (!s.constMeasure) {
    s.measure = spec_expr(plan.measure, MEASURE);
    s.measureWidth = plan.measureWidth; s.identity = plan.identity;
    if (s.measureAvg || plan.measureWidth != 8) s.measureDtype = plan.measureDtype;  // (an 8-byte sum carries the stored bits)
  }
  return s;
}
RtcSpec spec_vector(RtcKind kind, int nd, const int *widths, int vw, int partBits) {
  RtcSpec s = spec_of(kind, nd, partBits);
  for (int d = 0; d < nd && d < kFusedDims; d++) s.dimWidth[d] = widths ? widths[d] : 4;
  s.vectorVW = vw;
  return s;
}

}  // namespace

const char *rtc_entry_name(int32_t kind) {
  switch (kind) {
    case RTC_SCAN_SORT64: case RTC_SORT_VECTOR_SCAN: return "sr_scan_rtc";
    case RTC_HLL_SCAN: return "hll_scan_rtc";
    case RTC_MERGE: case RTC_VECTOR_MERGE: return "hr_merge_rtc";
    default: return "hr_scan_rtc";
  }
}

RtcSpec rtc_spec_scan(const FusedPlanD &plan, int nd, int partBits, bool compact) {
  return spec_plan_scan(compact ? RTC_SCAN_COMPACT : RTC_SCAN_LINES16, plan, nd, partBits);
}
RtcSpec rtc_spec_sort_scan(const FusedPlanD &plan, int nd, int partBits) { return spec_plan_scan(RTC_SCAN_SORT64, plan, nd, partBits); }
RtcSpec rtc_spec_table_scan(const FusedPlanD &plan, int nd, int partBits, const AggSpec &a, const hr::Widen &w) {
  RtcSpec s = spec_plan_scan(RTC_SCAN_TABLE, plan, nd, partBits);
  spec_agg(s, a, w);
  return s;
}
RtcSpec rtc_spec_vector_scan(int nd, int vw, int partBits) { return spec_vector(RTC_VECTOR_SCAN, nd, nullptr, vw, partBits); }
RtcSpec rtc_spec_sort_vector_scan(int nd, const int *widths, int partBits) { return spec_vector(RTC_SORT_VECTOR_SCAN, nd, widths, 4, partBits); }
RtcSpec rtc_spec_hll_scan(int nd, const int *widths, int partBits) { return spec_vector(RTC_HLL_SCAN, nd, widths, 4, partBits); }
RtcSpec rtc_spec_merge(const FusedPlanD &plan, int nd, int partBits, const AggSpec &a, const hr::Widen &w, bool compact, bool regionA,
                       int image) {
  RtcSpec s = spec_of(RTC_MERGE, nd, partBits);
  spec_dims(s, plan);  // (groups that are new in the batch: their dimensions are evaluated again, from the columns these read)
  for (int d = 0; d < nd && d < kFusedDims; d++)
    if (plan.dims[d].col >= 0 && plan.dims[d].col < kFusedCols) spec_column(s, plan, plan.dims[d].col);
  spec_agg(s, a, w);
  s.aggWidth = a.width;
  s.compact = compact; s.regionA = regionA; s.image = image;
  return s;
}
RtcSpec rtc_spec_vector_merge(int nd, int vw, int partBits, const AggSpec &a) {
  RtcSpec s = spec_vector(RTC_VECTOR_MERGE, nd, nullptr, vw, partBits);
  spec_agg(s, a, hr::Widen{0, 0, 0});
  s.aggWidth = a.width;
  return s;
}

std::string rtc_source(const RtcSpec &s) {
  switch (s.kind) {
    case RTC_SCAN_LINES16: case RTC_SCAN_COMPACT: case RTC_SCAN_TABLE: case RTC_SCAN_SORT64: return generate(s);
    case RTC_VECTOR_SCAN: case RTC_SORT_VECTOR_SCAN: case RTC_HLL_SCAN: return generate_vector(s);
    case RTC_MERGE: case RTC_VECTOR_MERGE: return generate_merge(s);
    default: return "";
  }
}

}  // namespace ares
