// gs_exact_dev.h -- the device half of the exact sums (gs_exact_sum.h has the split and the host's finish): one lane's 128-bit
// accumulator per quantity, its flush to the workgroup's LDS limb table, and the fold over a wave.  Written once: the moments'
// kernel (k_moments.hip) and the pair moments' (k_pairs.hip) both include this copy.  Integer adds only, so what the limbs end up
// holding does not depend on the grid, on the order or on who adds what where.
#pragma once
#include "gs_device.h"
#include "gs_exact_sum.h"

typedef unsigned long long mo_u64;

// The sum over the wave in lane 63: wave_incl_scan's DPP steps on both halves of a 64-bit word.
__device__ __forceinline__ mo_u64 mo_wave_scan64(mo_u64 v) {
#define GS_MO_STEP(ctrl, rm)                                                                                           \
    {                                                                                                                  \
        const uint32_t lo = GS_DPP((uint32_t)v, ctrl, rm), hi = GS_DPP((uint32_t)(v >> 32), ctrl, rm);                 \
        v += ((mo_u64)hi << 32) | lo;                                                                                  \
    }
    GS_MO_STEP(0x111, 0xf)
    GS_MO_STEP(0x112, 0xf)
    GS_MO_STEP(0x114, 0xf)
    GS_MO_STEP(0x118, 0xf)
    GS_MO_STEP(0x142, 0xa)
    GS_MO_STEP(0x143, 0xc)
#undef GS_MO_STEP
    return v;
}

// One quantity's accumulator of one lane: a 128-bit two's complement integer whose unit is limb `base`'s, 2^(32 base - 298).
// base = GS_MO_EMPTY: nothing yet (a = 0; far enough below 0 that no first limb, 0 included, looks like base or base + 1).  A term
// whose limb L is base or base + 1 is |m| < 2^48 shifted by p - 32 base < 64: below 2^111, so 2^16 terms fit (GS_MO_MAX_TRIPS).
#define GS_MO_EMPTY (-8)
#define GS_MO_MAX_TRIPS 16384u // x 4 splats = 2^16 terms per lane and quantity
typedef unsigned __int128 mo_u128;
struct MoAcc { mo_u128 a; int base; };

// what the accumulator adds to limb base + j: its 32-bit words, the last one signed.  Each is below 2^32 in magnitude, and a flush
// follows at least one term, so the limbs keep gs_exact_sum.h's bound of (terms) x 2^32.
__device__ __forceinline__ mo_u64 mo_word(const MoAcc& x, int j) {
    const uint32_t w = (uint32_t)(x.a >> (32 * j));
    return j < 3 ? (mo_u64)w : (mo_u64)(long long)(int)w;
}
// the lane's own flush: its non-zero words to the workgroup's table (limbs base .. base + 3 <= 19: base <= 15 + 1)
__device__ __forceinline__ void mo_flush(MoAcc& x, mo_u64* __restrict__ tab) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const mo_u64 w = mo_word(x, j);
        if (w) atomicAdd(tab + x.base + j, w);
    }
    x.a = 0;
}
// += (neg ? -m : m) 2^(p - 298), m < 2^48
__device__ __forceinline__ void mo_add(MoAcc& x, mo_u64* __restrict__ tab, uint64_t m, uint32_t p, bool neg) {
    if (m == 0ull) return; // (a zero has no limb of its own: it must not move the base)
    const int L = (int)(p >> 5);
    if ((uint32_t)(L - x.base) > 1u) { // the rare path, also the first term (nothing to flush then)
        if (x.base != GS_MO_EMPTY) mo_flush(x, tab);
        x.base = L;
    }
    const uint32_t sh = p - 32u * (uint32_t)x.base; // 0 .. 63
    const long long t = neg ? -(long long)m : (long long)m;
    const mo_u64 lo = (mo_u64)t << sh;
    const long long hi = (t >> 1) >> (63u - sh); // t >> (64 - sh), also for sh = 0
    x.a += ((mo_u128)(mo_u64)hi << 64) | lo;
}
// When the loop has ended: one round per distinct base among the wave's lanes.  Wave-uniform control flow (the DPP steps read
// every lane), the lanes of another base add zeros.
__device__ __forceinline__ void mo_fold(MoAcc& x, mo_u64* __restrict__ tab, uint32_t lane) {
    bool open = x.base != GS_MO_EMPTY;
    while (true) {
        const uint32_t top = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max(open ? (uint32_t)x.base + 1u : 0u), 63);
        if (top == 0u) break; // (uniform)
        const int b = (int)top - 1;
        const bool mine = open && x.base == b;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const mo_u64 sum = mo_wave_scan64(mine ? mo_word(x, j) : 0ull);
            if (lane == 63u && sum) atomicAdd(tab + b + j, sum);
        }
        if (mine) open = false;
    }
}
