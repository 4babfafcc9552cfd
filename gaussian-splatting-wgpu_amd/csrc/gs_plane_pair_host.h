// gs_plane_pair_host.h -- the plane pair moments (gs_abi.h "registration", point-to-plane) on host planes, and the expressions host
// and device share: the f32 row of one pair, when the pair counts, and which two factors make up each of the 29 quantities.  On top of
// gs_pair_host.h (pair_d2, pair_accept: unchanged).  Plain C++ when the compiler is not hipcc (tools/plane_pairs_check builds it with
// a host compiler and sanitizers); gs_plane_pairs.hip (both entry points) and k_plane_pairs.hip compile this one copy.
//
// The 29 quantities, in gs_pair_plane_moments' order: G[21] the upper triangle of sum g g^T row-major, h[6] = sum g_k r, rr = sum r r,
// d2 = sum of the f32 value d2.  With the row's factors f[0..5] = g = (cx, cy, cz, nx, ny, nz) and f[6] = r, quantity t < 28 is the
// sum of f[plane_fa(t)] f[plane_fb(t)]; quantity 28 is a sum of single values.
#pragma once
#include "gs_pair_host.h"

#define GS_PLANE_QUANTITIES 29u
#define GS_PLANE_PRODUCTS 28u // the quantities that are products of two factors: G, h, rr
#define GS_PLANE_G 0u
#define GS_PLANE_H 21u
#define GS_PLANE_RR 27u
#define GS_PLANE_D2 28u
#define GS_PLANE_FACTORS 7u

// the two factors of quantity t < GS_PLANE_PRODUCTS (constant-folded where t is a constant)
GS_EX constexpr uint32_t plane_fa(uint32_t t) {
    if (t >= GS_PLANE_RR) return 6u;
    if (t >= GS_PLANE_H) return t - GS_PLANE_H;
    uint32_t a = 0u;
    while (t >= 6u - a) { t -= 6u - a; ++a; }
    return a;
}
GS_EX constexpr uint32_t plane_fb(uint32_t t) {
    if (t >= GS_PLANE_H) return 6u;
    uint32_t a = 0u;
    while (t >= 6u - a) { t -= 6u - a; ++a; }
    return a + t;
}

// The row of one pair from the bit patterns of p, q = p_j and n = normal[j]: false when the pair does not count.  The caller has
// checked j < N.  Every line is one f32 rounding per written operation (every translation unit that includes this is compiled
// without contraction).
GS_EX bool plane_row(const uint32_t p[3], const uint32_t q[3], const uint32_t nb[3], const float pivot[3], float max_d2, float f[GS_PLANE_FACTORS],
                     float* d2) {
    if (!pair_accept(p, q, max_d2)) return false;
    if (!ex_finite(nb[0]) || !ex_finite(nb[1]) || !ex_finite(nb[2])) return false;
    float pf[3], qf[3], n[3];
    for (int a = 0; a < 3; ++a) { __builtin_memcpy(&pf[a], &p[a], 4); __builtin_memcpy(&qf[a], &q[a], 4); __builtin_memcpy(&n[a], &nb[a], 4); }
    const float ux = pf[0] - pivot[0], uy = pf[1] - pivot[1], uz = pf[2] - pivot[2];
    const float dx = qf[0] - pf[0], dy = qf[1] - pf[1], dz = qf[2] - pf[2];
    *d2 = (dx * dx + dy * dy) + dz * dz;
    const float r = (n[0] * dx + n[1] * dy) + n[2] * dz;
    const float cx = uy * n[2] - uz * n[1], cy = uz * n[0] - ux * n[2], cz = ux * n[1] - uy * n[0];
    if (!ex_finite(ex_bits(cx)) || !ex_finite(ex_bits(cy)) || !ex_finite(ex_bits(cz)) || !ex_finite(ex_bits(r))) return false;
    f[0] = cx; f[1] = cy; f[2] = cz; f[3] = n[0]; f[4] = n[1]; f[5] = n[2]; f[6] = r;
    return true;
}

// ---- host only ---------------------------------------------------------------------------------------------------------------------
struct PlaneSums {
    int64_t t[GS_PLANE_QUANTITIES * GS_EX_LIMBS];
    uint64_t matched, paired;
};
inline void plane_sums_clear(PlaneSums* s) {
    for (uint32_t k = 0; k < GS_PLANE_QUANTITIES * GS_EX_LIMBS; ++k) s->t[k] = 0;
    s->matched = s->paired = 0;
}
// Splat i of n: counted as matched when it passes the filter (state may be null with the filter (0, 0)), as paired when its partner
// j = partner[i] is below n -- any other id is never an index into the positions or the normals -- and plane_row holds; then its 29
// terms are added.  normal: f32[n][3].
inline void plane_host_one(PlaneSums* s, const float* px, const float* py, const float* pz, uint64_t n, const uint32_t* partner, const float* normal,
                           const uint8_t* state, uint32_t mask, uint32_t value, const float pivot[3], float max_d2, uint64_t i) {
    if ((mask | value) && (state[i] & mask) != value) return;
    ++s->matched;
    const uint64_t j = partner[i];
    if (j >= n) return;
    const uint32_t p[3] = {ex_bits(px[i]), ex_bits(py[i]), ex_bits(pz[i])}, q[3] = {ex_bits(px[j]), ex_bits(py[j]), ex_bits(pz[j])};
    const uint32_t nb[3] = {ex_bits(normal[3u * j]), ex_bits(normal[3u * j + 1u]), ex_bits(normal[3u * j + 2u])};
    float f[GS_PLANE_FACTORS], d2;
    if (!plane_row(p, q, nb, pivot, max_d2, f, &d2)) return;
    ++s->paired;
    for (uint32_t t = 0; t < GS_PLANE_PRODUCTS; ++t) ex_add_product(s->t + (size_t)t * GS_EX_LIMBS, f[plane_fa(t)], f[plane_fb(t)]);
    ex_add_value(s->t + (size_t)GS_PLANE_D2 * GS_EX_LIMBS, d2);
}
