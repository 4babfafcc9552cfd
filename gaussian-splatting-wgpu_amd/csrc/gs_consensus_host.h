// gs_consensus_host.h -- what host and device share of the consensus calls (gs_abi.h "consensus"): the ONE copy of the value of a
// splat's centre against a point or a plane (attr_of_pos, which the splat attributes' kernels of k_attr.hip use too), the host loop
// that scores h hypotheses against n positions, and the plane through three points.  Plain C++ when the compiler is not hipcc
// (tools/consensus_check builds it with a host compiler and sanitizers); gs_consensus.hip (gs_consensus_host, gs_planes_through),
// k_consensus.hip and k_attr.hip compile this one copy.  Every translation unit that includes it is compiled without contraction.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gs_exact_sum.h" // GS_EX
#include "../../include/gsplat/gs_abi.h"

struct GsAttrDev { float p[4]; }; // a gs_attr's parameters as the kernels read them

// The value of a centre (one rounding per operation; DIST2 is state_member's sphere expression, PLANE the projection's pv.z)
template <int KIND>
GS_EX float attr_of_pos(const GsAttrDev& a, float x, float y, float z) {
    if (KIND == GS_ATTR_DIST2) {
        const float dx = x - a.p[0], dy = y - a.p[1], dz = z - a.p[2];
        return (dx * dx + dy * dy) + dz * dz;
    }
    return ((a.p[0] * x + a.p[1] * y) + a.p[2] * z) + a.p[3];
}

// ---- host only ---------------------------------------------------------------------------------------------------------------------
// Splat i of the planes: counted as matched when it passes the filter (state may be null with the filter (0, 0)); then counts[j] grows
// by one for every hypothesis j whose value of it is in [lo, hi], both ends inclusive.  A NaN value is in no range.
template <int KIND>
inline void consensus_host_one(const float* px, const float* py, const float* pz, const uint8_t* state, uint32_t mask, uint32_t value,
                               const float* params, uint32_t h, float lo, float hi, uint64_t* counts, uint64_t* matched, uint64_t i) {
    if ((mask | value) && (state[i] & mask) != value) return;
    ++*matched;
    const float x = px[i], y = py[i], z = pz[i];
    for (uint32_t j = 0; j < h; ++j) {
        const GsAttrDev a = {{params[4u * j], params[4u * j + 1u], params[4u * j + 2u], params[4u * j + 3u]}};
        const float v = attr_of_pos<KIND>(a, x, y, z);
        if (v >= lo && v <= hi) ++counts[j];
    }
}
// counts[0 .. h) and *matched are ADDED to: the caller zeroes them
inline void consensus_host_loop(uint32_t kind, const float* px, const float* py, const float* pz, uint64_t n, const uint8_t* state, uint32_t mask,
                                uint32_t value, const float* params, uint32_t h, float lo, float hi, uint64_t* counts, uint64_t* matched) {
    for (uint64_t i = 0; i < n; ++i) {
        if (kind == GS_ATTR_DIST2) consensus_host_one<GS_ATTR_DIST2>(px, py, pz, state, mask, value, params, h, lo, hi, counts, matched, i);
        else consensus_host_one<GS_ATTR_PLANE>(px, py, pz, state, mask, value, params, h, lo, hi, counts, matched, i);
    }
}

// The plane through the points a = pt[0..2], b = pt[3..5], c = pt[6..8] as GS_ATTR_PLANE parameters (gs_abi.h states the expressions):
// everything in double, one operation at a time, the four numbers rounded to f32 at the end; four NaNs when the cross product's length
// is not a finite number above 0.
inline void plane_through(const float* pt, float* out) {
    const double a0 = pt[0], a1 = pt[1], a2 = pt[2];
    const double u0 = (double)pt[3] - a0, u1 = (double)pt[4] - a1, u2 = (double)pt[5] - a2;
    const double w0 = (double)pt[6] - a0, w1 = (double)pt[7] - a1, w2 = (double)pt[8] - a2;
    const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
    const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    if (!(__builtin_isfinite(len) && len > 0.0)) {
        out[0] = out[1] = out[2] = out[3] = __builtin_nanf("");
        return;
    }
    double m[3] = {n0 / len, n1 / len, n2 / len};
    double d = -((m[0] * a0 + m[1] * a1) + m[2] * a2);
    int big = 0; // the first component of the largest magnitude
    for (int k = 1; k < 3; ++k)
        if (fabs(m[k]) > fabs(m[big])) big = k;
    if (m[big] < 0.0) {
        for (int k = 0; k < 3; ++k) m[k] = -m[k];
        d = -d;
    }
    out[0] = (float)m[0]; out[1] = (float)m[1]; out[2] = (float)m[2]; out[3] = (float)d;
}
