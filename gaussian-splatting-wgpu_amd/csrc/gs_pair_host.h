// gs_pair_host.h -- the pair moments (gs_abi.h "registration") on host planes, and the one expression host and device share: when a
// splat and its partner count as a pair.  Plain C++ when the compiler is not hipcc (tools/pairs_check builds it with a host compiler
// and sanitizers); gs_pairs.hip (gs_pair_moments_host) and k_pairs.hip compile this one copy, on top of gs_exact_sum.h.
//
// The 21 quantities, in gs_pair_moments' order: sum_p[3], sum_q[3], pq[9] row-major (a, b), pp[3], qq[3].
#pragma once
#include <stddef.h>

#include "gs_exact_sum.h"

#define GS_PAIR_QUANTITIES 21u
#define GS_PAIR_SUM_P 0u
#define GS_PAIR_SUM_Q 3u
#define GS_PAIR_PQ 6u
#define GS_PAIR_PP 15u
#define GS_PAIR_QQ 18u

// The neighbourhoods' expression on the positions as they are now: d = q - p per component, (dx dx + dy dy) + dz dz, one f32
// rounding per operation (every translation unit that includes this is compiled without contraction).
GS_EX float pair_d2(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    return (dx * dx + dy * dy) + dz * dz;
}
// six finite coordinates and d2 <= max_d2, inclusive; a d2 that overflowed to +inf passes only max_d2 = +inf
GS_EX bool pair_accept(const uint32_t p[3], const uint32_t q[3], float max_d2) {
    for (int a = 0; a < 3; ++a)
        if (!ex_finite(p[a]) || !ex_finite(q[a])) return false;
    float pf[3], qf[3];
    for (int a = 0; a < 3; ++a) { __builtin_memcpy(&pf[a], &p[a], 4); __builtin_memcpy(&qf[a], &q[a], 4); }
    return pair_d2(pf[0], pf[1], pf[2], qf[0], qf[1], qf[2]) <= max_d2;
}

// ---- host only ---------------------------------------------------------------------------------------------------------------------
struct PairSums {
    int64_t t[GS_PAIR_QUANTITIES * GS_EX_LIMBS];
    uint64_t matched, paired;
};
inline void pair_sums_clear(PairSums* s) {
    for (uint32_t k = 0; k < GS_PAIR_QUANTITIES * GS_EX_LIMBS; ++k) s->t[k] = 0;
    s->matched = s->paired = 0;
}
// Splat i of n: counted as matched when it passes the filter (state may be null with the filter (0, 0)), as paired when its
// partner j = partner[i] is below n -- any other id is never read -- and pair_accept holds; then its 21 terms are added.
inline void pair_host_one(PairSums* s, const float* px, const float* py, const float* pz, uint64_t n, const uint32_t* partner, const uint8_t* state,
                          uint32_t mask, uint32_t value, float max_d2, uint64_t i) {
    if ((mask | value) && (state[i] & mask) != value) return;
    ++s->matched;
    const uint64_t j = partner[i];
    if (j >= n) return;
    const float pf[3] = {px[i], py[i], pz[i]}, qf[3] = {px[j], py[j], pz[j]};
    const uint32_t p[3] = {ex_bits(pf[0]), ex_bits(pf[1]), ex_bits(pf[2])}, q[3] = {ex_bits(qf[0]), ex_bits(qf[1]), ex_bits(qf[2])};
    if (!pair_accept(p, q, max_d2)) return;
    ++s->paired;
    for (uint32_t a = 0; a < 3u; ++a) {
        ex_add_value(s->t + (size_t)(GS_PAIR_SUM_P + a) * GS_EX_LIMBS, pf[a]);
        ex_add_value(s->t + (size_t)(GS_PAIR_SUM_Q + a) * GS_EX_LIMBS, qf[a]);
        for (uint32_t b = 0; b < 3u; ++b) ex_add_product(s->t + (size_t)(GS_PAIR_PQ + 3u * a + b) * GS_EX_LIMBS, pf[a], qf[b]);
        ex_add_product(s->t + (size_t)(GS_PAIR_PP + a) * GS_EX_LIMBS, pf[a], pf[a]);
        ex_add_product(s->t + (size_t)(GS_PAIR_QQ + a) * GS_EX_LIMBS, qf[a], qf[a]);
    }
}
