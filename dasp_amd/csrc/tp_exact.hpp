// tp_exact.hpp -- the arithmetic of the exact phase 2 of the two-phase form (dasp_options_t::tp_exact), for host and device.
// Included by kernels.hip (dasp_tp_reduce_exact_kernel) and by capi.cpp (dasp_tp_exact_dot_f16, the host mirror that defines the result); nothing else.
//
// An f16 x f16 product p is exact in f32, an integer multiple of 2^-48 (the smallest subnormal squared) and below 2^32 in magnitude: q = p 2^48 is an 80-bit
// integer.  It is kept as TWO integers, q = H 2^40 + L: H in units of 2^-8, L in units of 2^-48.  Integer addition is associative, so the two sums of a row do
// not depend on the order in which its products arrive -- which is what makes a sum built by LDS atomics reproducible -- and they are exact:
//   split():  H = rint(p 2^8), |H| <= 2^40;  L = (p 2^8 - H) 2^40, |L| <= 2^39
//   a row of fewer than 2^22 products (kMaxTerms):  |sum H| < 2^62, |sum L| < 2^61 -- no 64-bit overflow
// The split runs in the f64 domain with the 1.5 x 2^52 rounding constant (no f64 -> i64 conversion, which the GPU emulates): p 2^8 + C has p 2^8 rounded to an
// integer in its low mantissa bits; every operation below is exact, so neither the rounding mode's tie rule nor an fma contraction changes a bit.
// A Pair is the same two numbers still in f64 (hi integer-valued, lo a multiple of 2^-40): sums of up to kMaxPairTerms products stay exact there (|hi| < 2^50,
// |lo 2^40| < 2^49 < 2^51, the range of the constant trick), which covers what one lane (8 elements) and one segment (64) combine before they touch LDS.
// Non-finite products (an operand is inf or NaN; finite f16 operands never overflow f32) have no fixed-point form: they set sticky flags instead -- OR is
// associative too -- and the finite products of such a row are ignored.
// finish(): carry = L >> 40 moves into H, L' in [0, 2^40); d = (double)H' 2^-8 + (double)L' 2^-48: both conversions exact while |sum| < 2^45 (beyond that the
// f16 result is +-inf either way), ONE rounding in the addition: d = RN_f64(exact row sum).  y = (f16)(f32)d, or (f16)((f32)y_old + (f32)d) when accumulating.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define DASP_TPX __host__ __device__ __forceinline__
#else
#define DASP_TPX inline
#endif

namespace dasp {
namespace tpx {

constexpr long long kMaxTerms = 1ll << 22;        // a row of this many products could overflow a 64-bit sum: dasp_plan_set_tp_exact refuses
constexpr int kMaxPairTerms = 1024;               // products a Pair may hold
constexpr double kRound = 6755399441055744.0;     // 1.5 x 2^52: x + kRound has rint(x) in its low mantissa bits for |x| < 2^51
constexpr long long kRoundBits = 0x4338000000000000ll;
constexpr unsigned kPosInf = 1u, kNegInf = 2u, kNaN = 4u;      // the sticky flags of an output position (4 bits per position in LDS)

struct Pair { double hi, lo; };                   // hi: units of 2^-8 (integer-valued); lo: the rest in the same unit (a multiple of 2^-40)
struct Fixed { long long H, L; };                 // H: units of 2^-8; L: units of 2^-48

// a FINITE product p = (float)a * (float)x of two f16 values
DASP_TPX Pair split(float p)
{
    const double s = (double)p * 256.0;
    const double hi = (s + kRound) - kRound;
    return Pair{hi, s - hi};
}
DASP_TPX Pair add(Pair a, Pair b) { return Pair{a.hi + b.hi, a.lo + b.lo}; }
// the integer an integer-valued double |v| < 2^51 holds, without a conversion instruction
DASP_TPX long long int_of(double v) { return __builtin_bit_cast(long long, v + kRound) - kRoundBits; }
DASP_TPX Fixed to_fixed(Pair a) { return Fixed{int_of(a.hi), int_of(a.lo * 1099511627776.0)}; }
DASP_TPX Fixed add(Fixed a, Fixed b) { return Fixed{(long long)((unsigned long long)a.H + (unsigned long long)b.H), (long long)((unsigned long long)a.L + (unsigned long long)b.L)}; }

// 0 for a finite product, else the flag it sets (inf x 0 is a NaN product)
DASP_TPX unsigned flag_of(float p)
{
    const unsigned u = __builtin_bit_cast(unsigned, p);
    if ((u & 0x7f800000u) != 0x7f800000u) return 0u;
    return (u & 0x007fffffu) ? kNaN : (u >> 31) ? kNegInf : kPosInf;
}
// nonzero when one of two packed f16 bit patterns holds an inf or a NaN (exponent field all ones: (h & 0x7fff) + 0x0400 reaches bit 15, no carry between the halves)
DASP_TPX unsigned nonfinite_f16x2(unsigned w) { return ((w & 0x7fff7fffu) + 0x04000400u) & 0x80008000u; }

// d of an output position: its two sums and its flags
DASP_TPX double finish(Fixed s, unsigned flags)
{
    if (flags) {
        if ((flags & kNaN) || (flags & (kPosInf | kNegInf)) == (kPosInf | kNegInf)) return __builtin_nan("");
        return (flags & kPosInf) ? __builtin_inf() : -__builtin_inf();
    }
    const long long carry = s.L >> 40;
    const long long H = s.H + carry, L = s.L - carry * (1ll << 40);
    return (double)H * 0.00390625 + (double)L * 3.552713678800501e-15;      // 2^-8, 2^-48
}

// ---- host mirror: binary16 <-> f32 by bit manipulation (no dependence on the host compiler's _Float16 runtime), the row sum in the kernel's own steps
inline float f16_bits_to_float(uint16_t h)
{
    const unsigned sign = (unsigned)(h & 0x8000u) << 16, em = h & 0x7fffu;
    unsigned u;
    if (em >= 0x7c00u) u = sign | 0x7f800000u | ((em & 0x3ffu) << 13);                          // inf / NaN
    else if (em >= 0x0400u) u = sign | ((em + ((127u - 15u) << 10)) << 13);                      // normal
    else {                                                                                      // zero / subnormal: em 2^-24, exact in f32
        const float f = (float)em * 5.9604644775390625e-08f;
        u = sign | __builtin_bit_cast(unsigned, f);
    }
    return __builtin_bit_cast(float, u);
}
// round to nearest even, as v_cvt_f16_f32 and numpy do
inline uint16_t float_to_f16_bits(float f)
{
    unsigned u = __builtin_bit_cast(unsigned, f);
    const unsigned sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((u >> 13) & 0x3ffu));               // NaN
    if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                                     // >= 65520 rounds to inf
    if (u < 0x38800000u) {                                                                      // below 2^-14: a multiple of 2^-24 after rounding
        const float t = __builtin_bit_cast(float, u) + 0.5f;                                    // (the addition rounds to 2^-24, nearest even)
        return (uint16_t)(sign | (__builtin_bit_cast(unsigned, t) - 0x3f000000u));
    }
    const unsigned odd = (u >> 13) & 1u;
    u += 0xc8000fffu;                                                                           // exponent bias 127 -> 15, + 0xfff
    u += odd;
    return (uint16_t)(sign | (u >> 13));
}
// y of one row: n products a[j] x[j], summed as the kernel sums them (lanes of 8 in the f64 domain, then integers)
inline uint16_t dot_f16(const uint16_t *a, const uint16_t *x, long long n, bool accumulate, uint16_t y_in)
{
    Fixed s{0, 0};
    unsigned flags = 0;
    for (long long j0 = 0; j0 < n; j0 += 8) {
        Pair run{0.0, 0.0};
        for (long long j = j0; j < n && j < j0 + 8; ++j) {
            const float p = f16_bits_to_float(a[j]) * f16_bits_to_float(x[j]);
            const unsigned f = flag_of(p);
            flags |= f;
            if (!f) run = add(run, split(p));
        }
        s = add(s, to_fixed(run));
    }
    const double d = finish(s, flags);
    return float_to_f16_bits(accumulate ? f16_bits_to_float(y_in) + (float)d : (float)d);
}

}  // namespace tpx
}  // namespace dasp
