"""An exact model of what one AQL operator does to (value, validity) pairs, written from the semantics and
independent of every implementation in this repository: it is what the HIP evaluators, the C checker and the
reference's own build are compared with at the edges of their types (tests/test_edge_semantics.py).

A value of one of the four 32-bit kinds is carried as its bit pattern (numpy uint32) next to a validity flag.
Integer arithmetic is carried out in 64-bit integers, where no 32 x 32-bit operation can overflow, and reduced
mod 2^32; float arithmetic is numpy's float32, whose single operations are correctly rounded (IEEE 754, denormals
kept); float sums are accumulated in numpy longdouble.

The semantics restated here (as aresdb_amd/csrc/algo/device_model.hpp cites them):
  * kinds and their common type                      reference query/utils.hpp:81-94
  * widening of stored 1- / 2- / 4-byte values        query/iterator.hpp:62-289 (146-165 for the narrow loads)
  * conversions between kinds (C static_cast)         query/iterator.hpp:465-537
  * unary / binary functors and their null rules      query/functor.hpp:30-351, 660-1076
  * dimension / scratch / measure sinks               query/iterator.hpp:465-537, 616-727
  * identities of the aggregates                      query/utils.hpp:165-184
  * aggregation of measures                           query/functor.hpp:1380-1436, query/sort_reduce.cu:135-160
  * calendar functors                                  query/functor.cu:70-212 (here: from the proleptic Gregorian calendar)
  * GetHLLValue                                        query/functor.hpp:431-466, MurmurHash3_x64_128 as published
Geo, the HyperLogLog aggregate and the arithmetic of the wide kinds are outside this model (unary_wide carries the wide
inputs of the calendar functors and of GetHLLValue only).
"""
import numpy as np

# ---- enumerations of the C ABI (include/ares_algorithm.h), restated so that this module imports nothing ----
(Bool, Int8, Uint8, Int16, Uint16, Int32, Uint32, Float32, Int64, Uint64, Float64, GeoPoint, UUID) = range(13)
(Negate, Not, BitwiseNot, IsNull, IsNotNull, Noop, GetWeekStart, GetMonthStart, GetQuarterStart, GetYearStart, GetDayOfMonth,
 GetDayOfYear, GetMonthOfYear, GetQuarterOfYear, GetHLLValue) = range(15)
(And, Or, Equal, NotEqual, LessThan, LessThanOrEqual, GreaterThan, GreaterThanOrEqual, Plus, Minus, Multiply, Divide,
 Mod, BitwiseAnd, BitwiseOr, BitwiseXor, Floor) = range(17)
SUM_UNSIGNED, SUM_SIGNED, SUM_FLOAT, MIN_UNSIGNED, MIN_SIGNED, MIN_FLOAT, MAX_UNSIGNED, MAX_SIGNED, MAX_FLOAT = range(1, 10)
AGGR_HLL, AVG_FLOAT = 10, 11

UNARY = (Negate, Not, BitwiseNot, IsNull, IsNotNull, Noop)
CALENDAR = (GetWeekStart, GetMonthStart, GetQuarterStart, GetYearStart, GetDayOfMonth, GetDayOfYear, GetMonthOfYear, GetQuarterOfYear)
HLL_VALUE = (GetHLLValue,)
BINARY = tuple(range(And, Floor + 1))
COMPARISONS = tuple(range(Equal, GreaterThanOrEqual + 1))
FUNCTOR_NAMES = {1: ["Negate", "Not", "BitwiseNot", "IsNull", "IsNotNull", "Noop", "GetWeekStart", "GetMonthStart", "GetQuarterStart",
                     "GetYearStart", "GetDayOfMonth", "GetDayOfYear", "GetMonthOfYear", "GetQuarterOfYear", "GetHLLValue"],
                 2: ["And", "Or", "Equal", "NotEqual", "LessThan", "LessThanOrEqual", "GreaterThan", "GreaterThanOrEqual", "Plus",
                     "Minus", "Multiply", "Divide", "Mod", "BitwiseAnd", "BitwiseOr", "BitwiseXor", "Floor"]}
TYPE_NAMES = ["Bool", "Int8", "Uint8", "Int16", "Uint16", "Int32", "Uint32", "Float32", "Int64", "Uint64", "Float64", "GeoPoint", "UUID"]

K_BOOL, K_I32, K_U32, K_F32 = range(4)
KIND_NAMES = ["bool", "int32", "uint32", "float32"]
KIND_OF = {Bool: K_BOOL, Int8: K_I32, Int16: K_I32, Int32: K_I32, Uint8: K_U32, Uint16: K_U32, Uint32: K_U32, Float32: K_F32}
NP_OF = {Int8: np.int8, Uint8: np.uint8, Int16: np.int16, Uint16: np.uint16, Int32: np.int32, Uint32: np.uint32,
         Float32: np.float32, Int64: np.int64, Float64: np.float64}
BYTES_OF = {Bool: 1, Int8: 1, Uint8: 1, Int16: 2, Uint16: 2, Int32: 4, Uint32: 4, Float32: 4, Int64: 8, Float64: 8}

M32 = 0xFFFFFFFF
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)

# ---- what stays excluded, and why --------------------------------------------------------------------------------
UNDEFINED = {
    "int_div_by_zero": "integer Divide / Mod / Floor by zero: undefined in C; the C checker and the reference's host build trap",
    "int_min_div_minus_one": "INT32_MIN Divide / Mod / Floor -1 on the signed kind: overflow, traps on x86",
    "float_to_int_out_of_range": "float -> integer conversion of a NaN or of a value whose truncation does not fit the target "
                                 "type (a narrow dimension slot included): undefined in C++, the reference's two builds disagree",
    "nan_result_bits": "sign and payload of a NaN that an arithmetic functor PRODUCES or propagates (inf - inf, 0 x inf, 0 / 0, "
                       "NaN + x): IEEE 754 leaves them open, x86 and gfx950 choose differently; NaN operands of comparisons, "
                       "Negate and Noop are defined and stay in",
    "float_identity_in_integer_measure": "MIN_FLOAT into an Int32 / Uint32 / Int64 measure: the identity is "
                                         "static_cast<integer>(FLT_MAX), out of range",
    "signed_overflow_vs_reference": "signed Plus / Minus / Multiply / Negate overflow and signed run-length scaling are undefined in "
                                    "the reference's C++; they wrap in this library and in the checker, so wrap is asserted for "
                                    "those two and the rows are left out of the comparison with the reference's build only",
    "min_max_of_both_zeros": "sign of a zero float MIN / MAX when a group holds +0.0 and -0.0: they compare equal, the result "
                             "depends on the merge order; compared as numbers",
    "nan_in_float_min_max": "NaN in a float MIN / MAX: comparison-based and fmin-based merges differ; no NaN in those pools",
    "host_hash_reduce_min_max": "the reference's HOST HashReduce starts MIN / MAX groups from 0 instead of the identity; its "
                                "device build and this library start from the identity, which is what the model does",
}


def u32(x):
    return (np.asarray(x).astype(np.int64) & M32).astype(np.uint32)


def as_f32(bits):
    return np.ascontiguousarray(np.asarray(bits, np.uint32)).view(np.float32)


def f32_bits(f):
    return np.ascontiguousarray(np.asarray(f, np.float32)).view(np.uint32)


def signed64(bits):
    """int32 reading of the bits, as int64"""
    return np.asarray(bits, np.uint32).view(np.int32).astype(np.int64)


def common_kind(a, b):
    if a == K_F32 or b == K_F32:
        return K_F32
    if a == K_I32 or b == K_I32:
        return K_I32
    return K_U32


def widen(stored, dtype):
    """bits of the 32-bit kind a stored value of column type `dtype` is read as: unsigned types zero-extend, signed ones
    sign-extend, Float32 keeps its bits, Bool is 0 / 1"""
    if dtype == Bool:
        return np.asarray(stored).astype(bool).astype(np.uint32)
    if dtype == Float32:
        return f32_bits(np.asarray(stored, np.float32))
    return u32(np.asarray(stored).astype(NP_OF[dtype]).astype(np.int64))


_INT_RANGE = {Int8: (-128, 127), Uint8: (0, 255), Int16: (-32768, 32767), Uint16: (0, 65535), Int32: (-2 ** 31, 2 ** 31 - 1),
              Uint32: (0, 2 ** 32 - 1), Int64: (-2 ** 63, 2 ** 63 - 1)}


def _trunc_fits(bits, dtype):
    """float (given as bits) whose truncation toward zero is a value of integer type `dtype`"""
    with np.errstate(invalid="ignore"):
        t = np.trunc(as_f32(bits).astype(np.float64))
    lo, hi = _INT_RANGE[dtype]
    return np.isfinite(t) & (t >= float(lo)) & (t < float(hi + 1))  # (both bounds are exact doubles)


def _trunc_int(bits, dtype):
    with np.errstate(invalid="ignore"):
        t = np.trunc(as_f32(bits).astype(np.float64))
    t = np.where(_trunc_fits(bits, dtype), t, 0.0)
    return t.astype(np.int64)


def convert(bits, from_kind, to_kind):
    """static_cast between the kinds; float -> integer only where convert_defined says so (0 elsewhere)"""
    bits = np.asarray(bits, np.uint32)
    if from_kind == to_kind:
        return bits
    if to_kind == K_BOOL:
        return (as_f32(bits) != 0).astype(np.uint32) if from_kind == K_F32 else (bits != 0).astype(np.uint32)
    if to_kind == K_I32:
        return u32(_trunc_int(bits, Int32)) if from_kind == K_F32 else bits
    if to_kind == K_U32:
        return u32(_trunc_int(bits, Uint32)) if from_kind == K_F32 else bits
    if from_kind == K_I32:
        return f32_bits(signed64(bits).astype(np.float32))   # int64 -> float32: one rounding, to nearest even
    return f32_bits(bits.astype(np.int64).astype(np.float32))


def convert_defined(bits, from_kind, to_kind):
    bits = np.asarray(bits, np.uint32)
    if from_kind == K_F32 and to_kind in (K_I32, K_U32):
        return _trunc_fits(bits, Int32 if to_kind == K_I32 else Uint32)
    return np.ones(bits.shape, bool)


def unary_result_kind(ft, kind):
    if ft in CALENDAR or ft in HLL_VALUE:   # (the float specialisation hands its argument back)
        return K_F32 if kind == K_F32 else K_U32
    return K_BOOL if ft in (Not, IsNull, IsNotNull) else kind


# ---- calendar: proleptic Gregorian, UTC, no leap seconds; numpy's datetime64 is the calendar here ------------------------
SECONDS_PER_DAY = 86400
FOUR_DAYS = 4 * SECONDS_PER_DAY   # 1970-01-05, the first Monday of the epoch


def _epoch_seconds(d):
    return d.astype("datetime64[s]").astype(np.int64)


def calendar(ft, ts):
    """the calendar functor `ft` of epoch seconds `ts` (uint32 bits read as unsigned: 1970-01-01 ... 2106-02-07), mod 2^32"""
    ts = np.asarray(ts, np.uint32).astype(np.int64)
    if ft == GetWeekStart:   # 1970-01-01 was a Thursday; the days before the epoch's first Monday belong to "week 0"
        day = ts // SECONDS_PER_DAY
        monday = day - (day + 3) % 7
        return u32(np.where(ts < FOUR_DAYS, 0, monday * SECONDS_PER_DAY))
    t = ts.astype("datetime64[s]")
    day, month, year = t.astype("datetime64[D]"), t.astype("datetime64[M]"), t.astype("datetime64[Y]")
    months = month.astype(np.int64)          # months since 1970-01
    month_of_year = months % 12
    if ft == GetMonthStart:
        return u32(_epoch_seconds(month))
    if ft == GetQuarterStart:
        return u32(_epoch_seconds((months - month_of_year % 3).astype("datetime64[M]")))
    if ft == GetYearStart:
        return u32(_epoch_seconds(year))
    if ft == GetDayOfMonth:
        return u32((day - month.astype("datetime64[D]")).astype(np.int64))
    if ft == GetDayOfYear:
        return u32((day - year.astype("datetime64[D]")).astype(np.int64))
    if ft == GetMonthOfYear:
        return u32(month_of_year)
    if ft == GetQuarterOfYear:
        return u32(month_of_year // 3)
    raise ValueError(ft)


# ---- GetHLLValue ---------------------------------------------------------------------------------------------------------
M64 = 0xFFFFFFFFFFFFFFFF
HLL_BITS = 14


def _c64(x, like):
    return np.uint64(x) if isinstance(like, np.ndarray) else x


def _rotl64(x, r):
    return ((x << _c64(r, x)) | (x >> _c64(64 - r, x))) & _c64(M64, x)


def _fmix64(k):
    k = k ^ (k >> _c64(33, k))
    k = (k * _c64(0xff51afd7ed558ccd, k)) & _c64(M64, k)
    k = k ^ (k >> _c64(33, k))
    k = (k * _c64(0xc4ceb9fe1a85ec53, k)) & _c64(M64, k)
    return k ^ (k >> _c64(33, k))


def murmur3_x64_128_low(key, nbytes, seed=0):
    """low 64 bits (h1) of MurmurHash3_x64_128 of a key of `nbytes` < 16 bytes given as its little-endian integer (so the key
    is all "tail": no 16-byte block, and with at most 8 bytes only k1 is mixed).  `key` is a Python int or a numpy uint64 array:
    the arithmetic is mod 2^64 either way."""
    assert 0 < nbytes <= 8
    c1, c2 = 0x87c37b91114253d5, 0x4cf5ad432745937f
    with np.errstate(over="ignore"):
        k1 = (key * _c64(c1, key)) & _c64(M64, key)
        k1 = (_rotl64(k1, 31) * _c64(c2, key)) & _c64(M64, key)
        h1 = _c64(seed, key) ^ k1
        h2 = _c64(seed, key) ^ (key ^ key)
        h1, h2 = h1 ^ _c64(nbytes, key), h2 ^ _c64(nbytes, key)
        h1 = (h1 + h2) & _c64(M64, key)
        h2 = (h2 + h1) & _c64(M64, key)
        h1, h2 = _fmix64(h1), _fmix64(h2)
        return (h1 + h2) & _c64(M64, key)


def hll_from_hash(h):
    """rho << 16 | register of 64-bit hashes (numpy uint64).  register = the low 14 bits.  rho is the number of probes that find
    a clear bit; probe number rho looks at bit rho + 14 of the hash, for rho + 14 < 64.  The original builds the probe mask by
    shifting a 32-bit 1, so it can only ever look at the LOW 32 bits: bits 14 ... 31 are real probes (rho = 0 ... 17); from bit 32
    on the shift count exceeds the 32-bit type and the mask is empty in both of the reference's builds (x86-64 host code
    compiled with optimisation, and PTX, whose shl clamps the count), so every later probe finds "clear" and rho runs on to 50.
    rho is the number of trailing zeros of bits 14 ... 31 of the low word, or 50 when all of them are clear; the high word and
    the register bits never count.  (A mask whose shift count wraps mod 32 would probe the register bits again from rho = 18:
    that reading is none of the reference's builds, and test_calendar_hll_semantics.py holds the inputs that tell it apart.)"""
    h = np.asarray(h, np.uint64)
    low = (h & np.uint64(M32)).astype(np.int64)
    up = low >> HLL_BITS
    lowest = up & -up                                     # the lowest set bit, a power of two below 2^18: exact in float64
    rho = np.where(up == 0, 64 - HLL_BITS, np.log2(np.maximum(lowest, 1).astype(np.float64)).astype(np.int64))
    return u32((rho << 16) | (low & ((1 << HLL_BITS) - 1)))


def hll_value(kind, bits):
    """GetHLLValue of a 32-bit kind: a Bool hashes its one byte, every other kind the four bytes of its widened value"""
    key = np.asarray(bits, np.uint32).astype(np.uint64)
    return hll_from_hash(murmur3_x64_128_low(key, 1 if kind == K_BOOL else 4))


def unary_wide(ft, dtype, lo, hi, ok):
    """(bits, validity) of a calendar functor or GetHLLValue over a wide column; the result is of kind K_U32.
    lo / hi: the value's low and high 8 bytes as uint64 (hi only for UUID; GeoPoint: lo = latitude | longitude << 32).
    Int64: the calendar functors see the low 32 bits, GetHLLValue hashes the 8 bytes.  UUID: GetHLLValue takes lo ^ hi as the
    hash, unhashed; every calendar functor is null.  GeoPoint: always null."""
    lo, ok = np.asarray(lo, np.uint64), np.asarray(ok, bool)
    zero = np.zeros(lo.shape, np.uint32)
    if ft not in CALENDAR and ft not in HLL_VALUE:
        raise ValueError(ft)
    if dtype == Int64:
        r = calendar(ft, (lo & np.uint64(M32)).astype(np.uint32)) if ft in CALENDAR else hll_from_hash(murmur3_x64_128_low(lo, 8))
    elif dtype == UUID and ft == GetHLLValue:
        r = hll_from_hash(lo ^ np.asarray(hi, np.uint64))
    elif dtype in (UUID, GeoPoint):
        return zero, np.zeros(lo.shape, bool)
    else:
        raise ValueError(dtype)
    return np.where(ok, r, zero).astype(np.uint32), ok


def unary(ft, kind, v, ok):
    """(bits, validity) of functor(v); the result is of unary_result_kind(ft, kind)"""
    v, ok = np.asarray(v, np.uint32), np.asarray(ok, bool)
    zero = np.zeros(v.shape, np.uint32)
    if ft == IsNull:
        return (~ok).astype(np.uint32), np.ones(v.shape, bool)
    if ft == IsNotNull:
        return ok.astype(np.uint32), np.ones(v.shape, bool)
    if ft == Noop:
        return v, ok
    if ft == Not:
        return np.where(ok, convert(v, kind, K_BOOL) ^ 1, zero).astype(np.uint32), ok
    if ft == Negate:
        if kind == K_F32:
            r = v ^ np.uint32(0x80000000)
        elif kind == K_BOOL:
            r = v
        else:
            r = u32(-v.astype(np.int64))
        return np.where(ok, r, zero).astype(np.uint32), ok
    if ft == BitwiseNot:
        if kind == K_F32:      # the float specialisation hands its argument back
            return v, ok
        r = np.ones(v.shape, np.uint32) if kind == K_BOOL else ~v
        return np.where(ok, r, zero).astype(np.uint32), ok
    if ft in CALENDAR or ft in HLL_VALUE:
        if kind == K_F32:      # the float specialisation hands its argument back, kind and validity included
            return v, ok
        # (a negative Int32, or a sign-extended Int8 / Int16, converts to the uint32 kind bit for bit: a date after 2038)
        r = calendar(ft, convert(v, kind, K_U32)) if ft in CALENDAR else hll_value(kind, v)
        return np.where(ok, r, zero).astype(np.uint32), ok
    raise ValueError(ft)


def binary_result_kind(ft, kind):
    return K_BOOL if And <= ft <= GreaterThanOrEqual else kind


def _trunc_divmod(x, y):
    """C's truncating quotient and remainder on int64 arrays (y != 0)"""
    q = np.abs(x) // np.abs(y)
    q = np.where((x < 0) != (y < 0), -q, q)
    return q, x - q * y


def binary(ft, kind, a, aok, b, bok):
    """(bits, validity) of a functor b, both operands already converted to `kind` = common_kind of their own kinds"""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    a, b = np.broadcast_arrays(a, b)
    aok, bok = np.broadcast_to(np.asarray(aok, bool), a.shape), np.broadcast_to(np.asarray(bok, bool), a.shape)
    both = aok & bok
    zero = np.zeros(a.shape, np.uint32)
    if ft == And:
        return np.where(both, convert(a, kind, K_BOOL) & convert(b, kind, K_BOOL), zero).astype(np.uint32), both
    if ft == Or:
        true = ((convert(a, kind, K_BOOL) != 0) & aok) | ((convert(b, kind, K_BOOL) != 0) & bok)
        return true.astype(np.uint32), true | both
    if ft in COMPARISONS:
        if kind == K_F32:
            x, y = as_f32(a), as_f32(b)
        elif kind == K_I32:
            x, y = signed64(a), signed64(b)
        else:
            x, y = a.astype(np.int64), b.astype(np.int64)
        with np.errstate(invalid="ignore"):
            c = {Equal: x == y, NotEqual: x != y, LessThan: x < y, LessThanOrEqual: x <= y, GreaterThan: x > y,
                 GreaterThanOrEqual: x >= y}[ft]
        return np.where(both, c, False).astype(np.uint32), both
    if kind == K_F32:
        if ft not in (Plus, Minus, Multiply, Divide):   # Mod, Floor and the bitwise functors hand the left operand back
            return a, aok
        x, y = as_f32(a), as_f32(b)
        with np.errstate(all="ignore"):
            r = {Plus: np.add, Minus: np.subtract, Multiply: np.multiply, Divide: np.divide}[ft](x, y)
        return np.where(both, f32_bits(r.astype(np.float32)), zero).astype(np.uint32), both
    ux, uy = a.astype(np.int64), b.astype(np.int64)
    if ft == Plus:
        r = ux + uy
    elif ft == Minus:
        r = ux - uy
    elif ft == Multiply:
        r = (a.astype(np.uint64) * b.astype(np.uint64)).astype(np.uint64) & np.uint64(M32)
    elif ft == BitwiseAnd:
        r = ux & uy
    elif ft == BitwiseOr:
        r = ux | uy
    elif ft == BitwiseXor:
        r = ux ^ uy
    else:
        x, y = (signed64(a), signed64(b)) if kind == K_I32 else (ux, uy)
        y = np.where(y == 0, 1, y)   # (undefined: never asked for, see binary_defined)
        q, m = _trunc_divmod(x, y)
        r = q if ft == Divide else m if ft == Mod else x - m
    return np.where(both, u32(r), zero).astype(np.uint32), both


def binary_defined(ft, kind, a, b):
    """rows the reference defines (see UNDEFINED): operands already of `kind`"""
    a, b = np.broadcast_arrays(np.asarray(a, np.uint32), np.asarray(b, np.uint32))
    ok = np.ones(a.shape, bool)
    if kind == K_F32:
        if ft in (Plus, Minus, Multiply, Divide):
            ok &= ~np.isnan(as_f32(binary(ft, kind, a, True, b, True)[0]))
    elif ft in (Divide, Mod, Floor):
        ok &= b != 0
        if kind == K_I32:
            ok &= ~((a == 0x80000000) & (b == M32))
    return ok


def signed_overflow(ft, kind, a, b=None):
    """rows where a signed Plus / Minus / Multiply (binary) or Negate (unary, b None) overflows int32"""
    a = np.asarray(a, np.uint32)
    if kind != K_I32:
        return np.zeros(a.shape, bool)
    x = signed64(a)
    if b is None:
        r = -x if ft == Negate else x
    else:
        y = signed64(np.broadcast_to(np.asarray(b, np.uint32), a.shape))
        if ft not in (Plus, Minus, Multiply):
            return np.zeros(a.shape, bool)
        r = x + y if ft == Plus else x - y if ft == Minus else x * y
    return (r < -2 ** 31) | (r > 2 ** 31 - 1)


# ---- sinks ------------------------------------------------------------------------------------------------------
def store_defined(dtype, bits, rk):
    """rows whose store into an element of type `dtype` (dimension slot, scratch vector or measure) is defined"""
    bits = np.asarray(bits, np.uint32)
    if rk == K_F32 and dtype in _INT_RANGE:
        return _trunc_fits(bits, dtype)
    return np.ones(bits.shape, bool)


def store_typed(dtype, bits, rk):
    """the stored element, as an (n, width) byte matrix: a 32-bit result is truncated into a narrow slot, a float result
    is truncated toward zero into an integer one, integers are converted to float with one rounding"""
    bits = np.asarray(bits, np.uint32)
    if dtype == Bool:
        out = convert(bits, rk, K_BOOL).astype(np.uint8)
    elif dtype in (Int8, Uint8, Int16, Uint16):
        v = _trunc_int(bits, dtype) if rk == K_F32 else bits.astype(np.int64)
        out = (v & ((1 << (8 * BYTES_OF[dtype])) - 1)).astype(NP_OF[dtype] if dtype in (Uint8, Uint16) else
                                                             {Int8: np.uint8, Int16: np.uint16}[dtype])
    elif dtype in (Int32, Uint32, Float32):
        out = convert(bits, rk, KIND_OF[dtype])
    elif dtype == Int64:
        out = _trunc_int(bits, Int64) if rk == K_F32 else signed64(bits) if rk == K_I32 else bits.astype(np.int64)
    elif dtype == Float64:
        out = as_f32(bits).astype(np.float64) if rk == K_F32 else signed64(bits).astype(np.float64) if rk == K_I32 \
            else bits.astype(np.float64)
    else:
        raise ValueError(dtype)
    out = np.ascontiguousarray(out)
    return out.view(np.uint8).reshape(len(out), -1)


def identity_defined(agg, dtype):
    return not (agg == MIN_FLOAT and dtype in (Int32, Uint32, Int64))


def identity_bytes(agg, dtype):
    """the aggregate's identity converted to the measure's type (what a null row contributes)"""
    ident = {MIN_UNSIGNED: 2 ** 32 - 1, MIN_SIGNED: 2 ** 31 - 1, MIN_FLOAT: FLT_MAX, MAX_SIGNED: -2 ** 31, MAX_FLOAT: FLT_MIN}.get(agg, 0)
    if dtype in (Float32, Float64):
        return np.array([ident], NP_OF[dtype]).view(np.uint8)
    ident = int(ident)   # (FLT_MIN truncates to 0)
    width = BYTES_OF[dtype]
    return np.frombuffer((ident & ((1 << (8 * width)) - 1)).to_bytes(width, "little"), np.uint8)


def store_measure(dtype, agg, bits, ok, rk, counts=None):
    """(n, width) bytes of the measure vector: a null row holds the identity; SUM scales by the run length `counts` in the
    measure's own arithmetic; AVG packs {float32 value, uint32 run length}"""
    bits, ok = np.asarray(bits, np.uint32), np.asarray(ok, bool)
    n = len(bits)
    counts = np.ones(n, np.int64) if counts is None else np.asarray(counts, np.int64)
    width = BYTES_OF[dtype]
    if agg == AVG_FLOAT:
        if dtype == Float64:
            f = store_typed(Float64, bits, rk).view(np.float64).reshape(n).astype(np.float32)
        elif dtype == Int64:
            f = store_typed(Int64, bits, rk).view(np.int64).reshape(n).astype(np.float32)
        elif dtype == Int32:
            f = signed64(convert(bits, rk, K_I32)).astype(np.float32)
        elif dtype == Uint32:
            f = convert(bits, rk, K_U32).astype(np.int64).astype(np.float32)
        else:
            f = as_f32(convert(bits, rk, K_F32))
        out = np.zeros((n, 2), np.uint32)
        out[:, 0], out[:, 1] = f32_bits(f), counts.astype(np.uint32)
        out = out.view(np.uint8).reshape(n, 8)[:, :width]
    else:
        scale = counts if agg in (SUM_UNSIGNED, SUM_SIGNED, SUM_FLOAT) else np.ones(n, np.int64)
        raw = store_typed(dtype, bits, rk)
        if dtype in (Int32, Uint32):
            v = u32((raw.view(np.uint32).reshape(n).astype(np.uint64) * scale.astype(np.uint64)) & np.uint64(M32))
        elif dtype == Int64:
            v = raw.view(np.uint64).reshape(n) * scale.astype(np.uint64)
        elif dtype == Float32:
            with np.errstate(all="ignore"):
                v = raw.view(np.float32).reshape(n) * scale.astype(np.float32)
        else:
            with np.errstate(all="ignore"):
                v = raw.view(np.float64).reshape(n) * scale.astype(np.float64)
        out = np.ascontiguousarray(v).view(np.uint8).reshape(n, width)
    out = out.copy()
    out[~ok] = identity_bytes(agg, dtype)[:width]
    return out


# ---- aggregates -------------------------------------------------------------------------------------------------
def aggregate(agg, width, values):
    """One group's aggregate over `values` (raw measure elements of `width` bytes, in any order) as Python / numpy scalars:
    SUM_UNSIGNED / SUM_SIGNED -> int mod 2^(8 width) (read back as unsigned); MIN / MAX -> the element by type;
    SUM_FLOAT -> (sum as longdouble, sum of magnitudes as longdouble, n); AVG_FLOAT -> (mean as longdouble, total count)."""
    raw = np.ascontiguousarray(values).view(np.uint8).reshape(-1, width)
    if agg in (SUM_UNSIGNED, SUM_SIGNED):
        total = sum(int(x) for x in raw.view(np.uint64 if width == 8 else np.uint32).reshape(-1))
        return total % (1 << (8 * width))
    if agg in (MIN_UNSIGNED, MAX_UNSIGNED, MIN_SIGNED, MAX_SIGNED):
        signed = agg in (MIN_SIGNED, MAX_SIGNED)
        t = {(4, False): np.uint32, (4, True): np.int32, (8, False): np.uint64, (8, True): np.int64}[(width, signed)]
        v = raw.view(t).reshape(-1)
        return int(v.min() if agg in (MIN_UNSIGNED, MIN_SIGNED) else v.max())
    if agg in (MIN_FLOAT, MAX_FLOAT):
        v = raw.view(np.float64 if width == 8 else np.float32).reshape(-1)
        return float(v.min() if agg == MIN_FLOAT else v.max())
    if agg == SUM_FLOAT:
        v = raw.view(np.float64 if width == 8 else np.float32).reshape(-1).astype(np.longdouble)
        return v.sum(), np.abs(v).sum(), len(v)
    if agg == AVG_FLOAT:
        pair = raw.view(np.uint32).reshape(-1, 2)
        mean, count = as_f32(pair[:, 0].copy()).astype(np.longdouble), pair[:, 1].astype(np.longdouble)
        return (mean * count).sum() / count.sum(), int(pair[:, 1].astype(np.int64).sum())
    raise ValueError(agg)


# ---- value pools ------------------------------------------------------------------------------------------------
def _pool(dtype, candidates):
    lo, hi = _INT_RANGE[dtype]
    return sorted({c for c in candidates if lo <= c <= hi})


_POW = [2 ** 7, 2 ** 8, 2 ** 15, 2 ** 16, 2 ** 23, 2 ** 24, 2 ** 31, 2 ** 32]
_INT_CANDIDATES = [0, 1, 2, 3, 7, 100, 3600, 86400, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 30, 3000000000] + \
    [p + d for p in _POW for d in (-2, -1, 0, 1)]
_INT_CANDIDATES = _INT_CANDIDATES + [-c for c in _INT_CANDIDATES]

_F = np.float32
EDGE_POOLS = {
    Bool: [False, True],
    Int8: _pool(Int8, _INT_CANDIDATES), Uint8: _pool(Uint8, _INT_CANDIDATES),
    Int16: _pool(Int16, _INT_CANDIDATES), Uint16: _pool(Uint16, _INT_CANDIDATES),
    Int32: [-2 ** 31, -2 ** 31 + 1, -2 ** 30, -2 ** 24 - 1, -2 ** 24, -86400, -65536, -32769, -32768, -3600, -257, -256, -129, -128, -7, -3,
            -2, -1, 0, 1, 2, 3, 7, 127, 128, 255, 256, 3600, 32767, 32768, 65535, 65536, 86400, 2 ** 23, 2 ** 24, 2 ** 24 + 1, 2 ** 30,
            2 ** 31 - 2, 2 ** 31 - 1],
    Uint32: _pool(Uint32, [c for c in _INT_CANDIDATES if c not in (2 ** 7 - 2, 2 ** 8 - 2, 2 ** 15 - 2, 2 ** 16 - 2, 2 ** 23 - 2, 100)]),
    Float32: [_F(x) for x in (0.0, -0.0, 1.0, -1.0, 2.0, 3.0, 0.5, -2.5, 0.1, 1.0 / 3.0, 100.75, 3600.0, 86400.0, 255.0, 256.0, -129.0,
                              32768.0, 65535.0, 16777216.0, 16777217.0, 16777218.0, 2147483520.0, -2147483648.0, 4294967040.0,
                              1e-45, -1e-45, 1.1754942e-38, FLT_MIN, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan)],
}
# integer constants are int32 in the ABI; float constants are floats
CONST_INT_POOL = EDGE_POOLS[Int32]
CONST_FLOAT_POOL = EDGE_POOLS[Float32]


def describe(bits, kind):
    """a value of `kind` for a failure message"""
    bits = int(bits)
    if kind == K_F32:
        return f"{float(as_f32(np.uint32(bits)))!r}f(0x{bits:08x})"
    if kind == K_I32:
        return str(bits - (1 << 32) if bits >> 31 else bits)
    return str(bits)
