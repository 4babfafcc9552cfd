// gs_surface_math.h -- the surface estimate (gs_abi.h "surface"), written once: the kernels (k_surface.hip), the device entry points
// and the host twin (gs_surface.hip, gs_surface_host) all compile this one copy, the way the cell merge shares gs_merge_math.h.  Plain
// C++ when the compiler is not hipcc (tools/surface_check builds it with a host compiler and sanitizers).
//
//   the scale     sf_check: the refusals of a gs_surface and, from the radius, r2, E, s = 2^(16 - E) and 2^(2 (E - 16)).
//   the sums      sf_quant: the ONE quantisation, q = (int32) rintf(d * s); SfSums / sf_add: count, S[3], M[6] as integers.
//   finishing     sf_finish: ten integers -> eigenvalues and normal, f64 in mg_finish's order of operations with the cell merge's
//                 Jacobi (mg_rotate, mg_order, MG_SWEEPS: gs_merge_math.h, no second copy); sf_orient: the sign towards a point.
//   the features  sf_feature: the seven expressions of gs_state_surface, f32, one rounding per written operation (every translation
//                 unit that includes this is compiled without contraction); sf_member: the range rule.
//   host only     surface_host: the whole call over host positions, all pairs.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gs_merge_math.h" // mg_rotate, mg_order, MG_SWEEPS; GS_PK, pk_finite (gs_pack_math.h); neigh_finite (gs_grid_math.h); gs_abi.h

#define SF_NAN_BITS 0x7FC00000u
#define SF_SUM_WORDS 10u // count, S x y z, M xx xy xz yy yz zz

// ---- the scale ------------------------------------------------------------------------------------------------------------------------
struct SfScale {
    float r2;       // radius * radius, ONE f32 product: the neighbourhoods' bound
    float s;        // 2^(16 - E), E = frexpf(radius)'s exponent: 2^(E-1) <= radius < 2^E
    double unscale; // 2^(2 (E - 16)): quantised squares -> world units, an exact power of two
    int e;
};
// The refusals of a gs_surface that need no context, in the header's order; msg: the message's tail, it names the number.
inline bool sf_check(const gs_surface* q, SfScale* out, char* msg, size_t cap) {
    if (!q) { snprintf(msg, cap, "null query"); return false; }
    if (q->struct_size != sizeof(gs_surface)) { snprintf(msg, cap, "struct_size %u != %zu", q->struct_size, sizeof(gs_surface)); return false; }
    const float radius = q->radius;
    if (!pk_finite(radius) || radius < 0.0f) { snprintf(msg, cap, "radius %g is negative or not finite", (double)radius); return false; }
    if (!(radius > 0.0f)) { snprintf(msg, cap, "radius %g is not above 0", (double)radius); return false; }
    out->r2 = radius * radius;
    if (!pk_finite(out->r2)) { snprintf(msg, cap, "radius %g squared is not finite in f32", (double)radius); return false; }
    (void)frexpf(radius, &out->e);
    if (16 - out->e > 127) { snprintf(msg, cap, "radius %g is below 2^-112: the scale 2^%d is no finite normal f32", (double)radius, 16 - out->e); return false; }
    out->s = ldexpf(1.0f, 16 - out->e);
    out->unscale = ldexp(1.0, 2 * (out->e - 16));
    if (q->flags & ~(GS_SURFACE_ORIENT | GS_SURFACE_KEEP_SUMS)) {
        snprintf(msg, cap, "unknown flags 0x%x", q->flags & ~(GS_SURFACE_ORIENT | GS_SURFACE_KEEP_SUMS));
        return false;
    }
    if (q->reserved != 0u) { snprintf(msg, cap, "reserved %llu is not 0", (unsigned long long)q->reserved); return false; }
    return true;
}

// ---- the sums -------------------------------------------------------------------------------------------------------------------------
// d: one component of p_j - p_i of an ACCEPTED source, |d| <= radius (1 + 2^-22) <= 2^E, so |d * s| <= 2^16 + 1: the product by a
// power of two is exact, the conversion cannot overflow.  rintf rounds half to even (the default rounding mode; v_rndne_f32).
GS_PK int32_t sf_quant(float d, float s) { return (int32_t)rintf(d * s); }
// |q_a q_b| <= 2^32 + 2^18 + 1 and fewer than 2^30 sources (the cell sort's limit): no sum reaches 2^63.
struct SfSums {
    uint32_t n;
    int64_t S[3], M[6];
};
GS_PK void sf_add(SfSums& a, uint32_t one, int32_t qx, int32_t qy, int32_t qz) { // one: 0 or 1; the three q's are 0 with it
    a.n += one;
    a.S[0] += qx; a.S[1] += qy; a.S[2] += qz;
    a.M[0] += (int64_t)qx * qx; a.M[1] += (int64_t)qx * qy; a.M[2] += (int64_t)qx * qz;
    a.M[3] += (int64_t)qy * qy; a.M[4] += (int64_t)qy * qz; a.M[5] += (int64_t)qz * qz;
}

// ---- finishing ------------------------------------------------------------------------------------------------------------------------
// w: count, S[3], M[6] of a query with count >= 3.  eig: l0 >= l1 >= l2 >= 0 in world units; nrm: the unit eigenvector of l2, its
// component of largest magnitude positive (a tie: the lowest axis).  Every i64 -> double conversion rounds to nearest even.
GS_PK void sf_finish(const int64_t w[SF_SUM_WORDS], double unscale, float nrm[3], float eig[3]) {
    const double n = (double)w[0];
    const double mu[3] = {(double)w[1] / n, (double)w[2] / n, (double)w[3] / n};
    double a[3][3], v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    a[0][0] = (double)w[4] / n - mu[0] * mu[0];
    a[0][1] = a[1][0] = (double)w[5] / n - mu[0] * mu[1];
    a[0][2] = a[2][0] = (double)w[6] / n - mu[0] * mu[2];
    a[1][1] = (double)w[7] / n - mu[1] * mu[1];
    a[1][2] = a[2][1] = (double)w[8] / n - mu[1] * mu[2];
    a[2][2] = (double)w[9] / n - mu[2] * mu[2];
    for (int sweep = 0; sweep < MG_SWEEPS; ++sweep) {
        mg_rotate<0, 1>(a, v);
        mg_rotate<0, 2>(a, v);
        mg_rotate<1, 2>(a, v);
    }
    double l[3] = {a[0][0], a[1][1], a[2][2]};
    mg_order<0, 1>(l, v);
    mg_order<1, 2>(l, v);
    mg_order<0, 1>(l, v);
    for (int k = 0; k < 3; ++k) {
        l[k] = l[k] >= 0.0 ? l[k] : 0.0;
        eig[k] = (float)(l[k] * unscale);
    }
    double m[3] = {v[0][2], v[1][2], v[2][2]};
    int big = 0;
    if (fabs(m[1]) > fabs(m[big])) big = 1;
    if (fabs(m[2]) > fabs(m[big])) big = 2;
    if (m[big] < 0.0)
        for (int k = 0; k < 3; ++k) m[k] = -m[k];
    for (int k = 0; k < 3; ++k) nrm[k] = (float)m[k];
}
// GS_SURFACE_ORIENT: the rounded normal is negated when it points away from `toward`; t == 0 and a NaN keep it.
GS_PK void sf_orient(float nrm[3], const float p[3], const float toward[3]) {
    const float ex = toward[0] - p[0], ey = toward[1] - p[1], ez = toward[2] - p[2];
    const float t = (nrm[0] * ex + nrm[1] * ey) + nrm[2] * ez;
    if (t < 0.0f) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
}

// ---- the features -----------------------------------------------------------------------------------------------------------------------
// nrm, eig, count: the planes' values of one splat; axis: as given.
GS_PK float sf_feature(uint32_t kind, const float nrm[3], const float eig[3], uint32_t count, const float axis[3]) {
    const float l0 = eig[0], l1 = eig[1], l2 = eig[2];
    switch (kind) {
    case GS_SURFACE_VARIATION: return l2 / ((l0 + l1) + l2);
    case GS_SURFACE_PLANARITY: return (l1 - l2) / l0;
    case GS_SURFACE_LINEARITY: return (l0 - l1) / l0;
    case GS_SURFACE_SPHERICITY: return l2 / l0;
    case GS_SURFACE_FACING: return fabsf((nrm[0] * axis[0] + nrm[1] * axis[1]) + nrm[2] * axis[2]);
    case GS_SURFACE_FACING_SIGNED: return (nrm[0] * axis[0] + nrm[1] * axis[1]) + nrm[2] * axis[2];
    default: return (float)count; // GS_SURFACE_COUNT
    }
}
GS_PK bool sf_member(float v, float lo, float hi, bool inside) { return (v >= lo && v <= hi) == inside; } // a NaN is in no range

// ---- host only --------------------------------------------------------------------------------------------------------------------------
// The whole call over n host positions (x y z interleaved), all pairs: the acceptance is the neighbourhoods' expression.  state may be
// null when both filters are (0, 0).  normal, eig: f32[n][3]; count: u32[n]; sums: i64[n][10] or null.  The caller has run sf_check.
inline void surface_host(const float* pos, const uint8_t* state, uint64_t n, const gs_surface* q, const SfScale& sc, float* normal, float* eig,
                         uint32_t* count, int64_t* sums, gs_surface_info* info) {
    *info = gs_surface_info{};
    const bool filter = (q->src_mask | q->src_value | q->qry_mask | q->qry_value) != 0u;
    auto is_src = [&](uint64_t i) { return !filter || ((uint32_t)state[i] & q->src_mask) == q->src_value; };
    auto is_qry = [&](uint64_t i) { return !filter || ((uint32_t)state[i] & q->qry_mask) == q->qry_value; };
    uint64_t fin_src = 0, fin_qry = 0;
    for (uint64_t j = 0; j < n; ++j)
        if (is_src(j)) { ++info->sources; fin_src += neigh_finite(pos[3 * j], pos[3 * j + 1], pos[3 * j + 2]) ? 1u : 0u; }
    float nan;
    const uint32_t nan_bits = SF_NAN_BITS;
    memcpy(&nan, &nan_bits, 4);
    for (uint64_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) normal[3 * i + k] = eig[3 * i + k] = nan;
        count[i] = 0u;
        if (sums)
            for (uint32_t k = 0; k < SF_SUM_WORDS; ++k) sums[i * SF_SUM_WORDS + k] = 0;
        if (!is_qry(i)) continue;
        ++info->queried;
        const float* p = pos + 3 * i;
        if (!neigh_finite(p[0], p[1], p[2])) { ++info->unresolved; continue; }
        ++fin_qry;
        SfSums a{};
        for (uint64_t j = 0; j < n; ++j) {
            if (j == i || !is_src(j)) continue;
            const float dx = pos[3 * j] - p[0], dy = pos[3 * j + 1] - p[1], dz = pos[3 * j + 2] - p[2];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (!(d2 <= sc.r2)) continue; // (a NaN or infinite coordinate of j fails)
            sf_add(a, 1u, sf_quant(dx, sc.s), sf_quant(dy, sc.s), sf_quant(dz, sc.s));
        }
        int64_t w[SF_SUM_WORDS] = {(int64_t)a.n, a.S[0], a.S[1], a.S[2], a.M[0], a.M[1], a.M[2], a.M[3], a.M[4], a.M[5]};
        count[i] = a.n;
        if (sums)
            for (uint32_t k = 0; k < SF_SUM_WORDS; ++k) sums[i * SF_SUM_WORDS + k] = w[k];
        if (a.n < 3u) { ++info->unresolved; continue; }
        sf_finish(w, sc.unscale, normal + 3 * i, eig + 3 * i);
        if (q->flags & GS_SURFACE_ORIENT) sf_orient(normal + 3 * i, p, q->toward);
    }
    info->candidates = fin_src * fin_qry; // the distance tests an all-pairs search makes, self included
    info->cells[0] = info->cells[1] = info->cells[2] = (fin_src && fin_qry) ? 1u : 0u;
}
