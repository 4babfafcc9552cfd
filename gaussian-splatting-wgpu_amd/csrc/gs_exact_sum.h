// gs_exact_sum.h -- the exact sum of f32 values and of products of two f32 values (gs_abi.h "moments"), written once: the kernel
// (k_moments.hip) and the host (gs_moments.hip, gs_moments_host) both compile this one copy, the way the packed codec shares
// gs_pack_math.h.  Plain C++ when the compiler is not hipcc (tools/moments_check builds it with a host compiler and sanitizers).
//
// THE SPLIT (host and device).  A finite f32 is m 2^e with an integer |m| < 2^24 and e in [-149, 104]; a product of two is m 2^e
// with |m| < 2^48 and e >= -298.  A term sits at bit position p = e + 298 >= 0 of a fixed-point number whose unit is 2^-298:
// limb L = p / 32, shift = p % 32, and |m| << shift (at most 80 bits) is three 32-bit chunks that are added, with the term's sign,
// to the signed 64-bit limbs L, L + 1, L + 2.  p <= 506, so L + 2 <= 17: GS_EX_LIMBS = 20 limbs cover every case.  One term adds at
// most one chunk (< 2^32) to any one limb, so with fewer than 2^31 terms no limb leaves i64 -- in any order, on any grid: integer
// adds commute.  (The kernels first add a lane's terms, shifted against a base limb, into a 128-bit integer in registers and add
// that integer's four 32-bit words to the limbs: the same sum, the same bound -- gs_exact_dev.h, shared by k_moments.hip and k_pairs.hip.)
// THE FINISH (host only).  Carries are propagated over the limbs into one sign-magnitude integer, which is rounded ONCE to the
// nearest double, ties to even (hi); hi is subtracted exactly and the rest rounded once more (lo).  Integer code throughout: no
// long double, no float add.  Every non-zero term is a multiple of 2^-298 and |sum| < 2^31 2^256, so neither result is subnormal
// or infinite.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_EX __host__ __device__ __forceinline__
#else
#define GS_EX inline
#endif

#define GS_EX_LIMBS 20u
#define GS_EX_BIAS 298 // bit position of 2^0

// ---- the split -------------------------------------------------------------------------------------------------------------------
GS_EX uint32_t ex_bits(float v) { uint32_t b; __builtin_memcpy(&b, &v, 4); return b; }
GS_EX bool ex_finite(uint32_t b) { return (b & 0x7F800000u) != 0x7F800000u; }
// |v| = ex_mant(b) 2^(ex_expo(b) - 150), the sign is bit 31 of b: a denormal has the exponent field of 1 and no hidden bit
GS_EX uint32_t ex_mant(uint32_t b) { return (b & 0x007FFFFFu) | ((b & 0x7F800000u) ? 0x00800000u : 0u); }
GS_EX uint32_t ex_expo(uint32_t b) { const uint32_t e = (b >> 23) & 0xFFu; return e ? e : 1u; }
// bit position of a single value's mantissa, and of the product of two mantissas: (E - 150) + 298, (Ea - 150) + (Eb - 150) + 298
GS_EX uint32_t ex_pos1(uint32_t b) { return ex_expo(b) + (uint32_t)(GS_EX_BIAS - 150); }
GS_EX uint32_t ex_pos2(uint32_t a, uint32_t b) { return ex_expo(a) + ex_expo(b) - (uint32_t)(300 - GS_EX_BIAS); }
// m < 2^48 at bit position p: the chunks c[0..2] for the limbs L, L + 1, L + 2; returns L
GS_EX uint32_t ex_chunks(uint64_t m, uint32_t p, uint32_t c[3]) {
    const uint32_t s = p & 31u;
    const uint64_t t = (m & 0xFFFFFFFFull) << s;      // < 2^63
    const uint64_t mid = (t >> 32) + ((m >> 32) << s); // < 2^31 + 2^47
    c[0] = (uint32_t)t;
    c[1] = (uint32_t)mid;
    c[2] = (uint32_t)(mid >> 32);
    return p >> 5;
}

// ---- host only: the limb table of one quantity, and the finish -----------------------------------------------------------------------
// (plain inline functions: host functions under hipcc)
// limbs[L .. L + 2] += +-chunks of m at bit position p
inline void ex_add(int64_t limbs[GS_EX_LIMBS], uint64_t m, uint32_t p, bool neg) {
    uint32_t c[3];
    const uint32_t L = ex_chunks(m, p, c);
    for (uint32_t k = 0; k < 3u; ++k) limbs[L + k] += neg ? -(int64_t)c[k] : (int64_t)c[k];
}
inline void ex_add_value(int64_t limbs[GS_EX_LIMBS], float v) {
    const uint32_t b = ex_bits(v);
    ex_add(limbs, ex_mant(b), ex_pos1(b), (b >> 31) != 0u);
}
inline void ex_add_product(int64_t limbs[GS_EX_LIMBS], float a, float b) {
    const uint32_t x = ex_bits(a), y = ex_bits(b);
    ex_add(limbs, (uint64_t)ex_mant(x) * ex_mant(y), ex_pos2(x, y), ((x ^ y) >> 31) != 0u);
}

#define GS_EX_DIGITS (GS_EX_LIMBS + 1u) // of the magnitude: the limbs' 640 bits and the carry out of the last
struct ExBig { uint32_t d[GS_EX_DIGITS]; bool neg; };
// sum limbs[k] 2^(32 k) as sign and magnitude
inline ExBig ex_carry(const int64_t limbs[GS_EX_LIMBS]) {
    ExBig r;
    int64_t carry = 0; // |carry| < 2^32 throughout: a limb's upper half and the carry of a 33-bit sum
    for (uint32_t k = 0; k < GS_EX_LIMBS; ++k) {
        const int64_t t = (int64_t)((uint64_t)limbs[k] & 0xFFFFFFFFull) + (carry & 0xFFFFFFFFll);
        r.d[k] = (uint32_t)t;
        carry = (limbs[k] >> 32) + (carry >> 32) + (t >> 32);
    }
    // carry is what stands above 2^640: 0 or, two's complement, the sign (|sum| < 2^640 by far)
    r.neg = carry < 0;
    r.d[GS_EX_LIMBS] = 0u;
    if (r.neg) {
        uint64_t c = 1u;
        for (uint32_t k = 0; k < GS_EX_LIMBS; ++k) {
            c += (uint64_t)(uint32_t)~r.d[k];
            r.d[k] = (uint32_t)c;
            c >>= 32;
        }
    }
    return r;
}
inline int ex_top_bit(const ExBig& a) { // -1: zero
    for (int k = (int)GS_EX_DIGITS - 1; k >= 0; --k)
        if (a.d[k]) return k * 32 + 31 - __builtin_clz(a.d[k]);
    return -1;
}
inline uint32_t ex_bit(const ExBig& a, int i) { return (a.d[i >> 5] >> (i & 31)) & 1u; }
// bits [from, from + 53) of a
inline uint64_t ex_field53(const ExBig& a, int from) {
    uint64_t q = 0;
    for (int i = 52; i >= 0; --i) q = (q << 1) | ((from + i) < (int)(GS_EX_DIGITS * 32u) ? ex_bit(a, from + i) : 0u);
    return q;
}
// q 2^(sh - 298), q < 2^54, exact (a power-of-two scaling of an integer of at most 53 significant bits, in the normal range)
inline double ex_scale(uint64_t q, int sh, bool neg) {
    if (!q) return 0.0;
    int e = sh - GS_EX_BIAS;
    while (!(q >> 52)) { q <<= 1; --e; } // normalise: q in [2^52, 2^53) -- or exactly 2^53 after a round up
    if (q >> 53) { q >>= 1; ++e; }
    const uint64_t bits = ((uint64_t)neg << 63) | ((uint64_t)(e + 52 + 1023) << 52) | (q & 0x000FFFFFFFFFFFFFull);
    double v;
    __builtin_memcpy(&v, &bits, 8);
    return v;
}
// The double nearest to a 2^-298, ties to even; *rest = a 2^-298 - that double, exactly, again in units of 2^-298.
inline double ex_round(const ExBig& a, ExBig* rest) {
    for (uint32_t k = 0; k < GS_EX_DIGITS; ++k) rest->d[k] = 0u;
    rest->neg = false;
    const int top = ex_top_bit(a);
    if (top < 0) return 0.0; // an exact zero is +0.0
    if (top <= 52) return ex_scale(ex_field53(a, 0), 0, a.neg);
    const int sh = top - 52;
    uint64_t q = ex_field53(a, sh);
    bool sticky = false;
    for (int i = 0; i < sh - 1 && !sticky; ++i) sticky = ex_bit(a, i) != 0u;
    const bool half = ex_bit(a, sh - 1) != 0u;
    const bool up = half && (sticky || (q & 1u));
    // the rest: the low sh bits when rounded down, 2^sh minus them (the other sign) when rounded up
    for (int i = 0; i < sh; ++i) rest->d[i >> 5] |= ex_bit(a, i) << (i & 31);
    rest->neg = a.neg;
    if (up) {
        uint64_t c = 1u;
        for (uint32_t k = 0; k < GS_EX_DIGITS; ++k) {
            c += (uint64_t)(uint32_t)~rest->d[k];
            rest->d[k] = (uint32_t)c;
            c >>= 32;
        }
        // (two's complement over all digits: -low; + 2^sh clears everything from bit sh up, low != 0 here since half is set)
        for (int i = sh; i < (int)(GS_EX_DIGITS * 32u); ++i) rest->d[i >> 5] &= ~(1u << (i & 31));
        rest->neg = !a.neg;
        ++q;
    }
    return ex_scale(q, sh, a.neg);
}
// hi = RN(sum), lo = RN(sum - hi)
inline void ex_finish(const int64_t limbs[GS_EX_LIMBS], double* hi, double* lo) {
    const ExBig a = ex_carry(limbs);
    ExBig rest, none;
    *hi = ex_round(a, &rest);
    *lo = ex_round(rest, &none);
}
