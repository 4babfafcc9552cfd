// gs_merge_math.h -- the cell merge (gs_abi.h "cell merge"), written once: the kernels (k_merge.hip), the device entry points and the
// host twin (gs_merge.hip, gs_cell_merge_host) all compile this one copy, the way the packed codec shares gs_pack_math.h.  Plain C++
// when the compiler is not hipcc (tools/merge_check builds it with a host compiler and sanitizers).
//
//   per splat   mg_sigmoid, mg_splat: the opacity, the three axis lengths, the six covariance entries and the weight w = a A, in f32, one
//               rounding per written operation (every translation unit that includes this is compiled without contraction).
//               RESTATED, not moved: the projection keeps its own sigmoid_ref and compute_cov3d lines (k_preprocess.hip:118-123,
//               :445-460) because moving them into a header that the host compiles too would put a frame kernel's code generation
//               at risk.  The expression trees are the same, operation for operation, with scale modifier 1 (s * 1 is exact and is
//               not written); tests/merge_restate.py holds both to the numpy restatement of the shaders.  gs_exp is pk_exp (gs_pack_math.h).
//   the grid    the neighbourhoods' (gs_grid_math.h: GsNeighGrid, neigh_cell, neigh_key, neigh_choose_grid), with the requested edge itself.
//   the sums    mg_slot_x: what slot q of a group's 64 doubles adds for one member, before the weight: acc[q] += w * x.
//   finishing   mg_finish: 64 doubles -> one 320-byte record, f64 with a fixed number of cyclic Jacobi sweeps.
//   host only   merge_host: the whole call over host records.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "gs_grid_math.h" // GsNeighGrid, neigh_finite, neigh_key, neigh_choose_grid
#include "gs_pack_math.h" // GS_PK, pk_exp, pk_finite, pk_okey
#include "../../include/gsplat/gs_abi.h"

// the slots of a group's sums (gs_abi.h): W, S[3], M[6] = xx xy xz yy yz zz, H[48] in the SH plane's order 3 k + channel
#define MG_SLOT_W 0u
#define MG_SLOT_S 1u
#define MG_SLOT_M 4u
#define MG_SLOT_H 10u
#define MG_SLOT_COUNT 58u
#define MG_SLOT_FIRST 59u
#define MG_SLOT_C 60u
#define MG_SWEEPS 10 // cyclic Jacobi sweeps of the 3x3 finish: a symmetric 3x3 in double is converged after 6

// ---- per splat ------------------------------------------------------------------------------------------------------------------------
GS_PK float mg_max(float a, float b) { return (a < b) ? b : a; }
// process_gaussians.wgsl:282-294: both branches evaluated, blended by a 0/1 float
GS_PK float mg_sigmoid(float o) {
    const float ez = pk_exp(o);
    const float cond = (o >= 0.0f) ? 1.0f : 0.0f;
    return (cond * (1.0f / (1.0f + pk_exp(-o)))) + ((1.0f - cond) * (ez / (1.0f + ez)));
}
struct MgSplat {
    float w;      // a A
    float sig[6]; // xx xy xz yy yz zz
};
// geo: the splat's eight geometry floats as the scene keeps them -- log-scale x y z, opacity logit, rot r x y z.  Returns whether the
// weight is finite and above 0 and the six entries are finite (the part of "eligible" that does not read state or position).
GS_PK bool mg_splat(const float geo[8], MgSplat* out) {
    const float sc[3] = {pk_exp(geo[0]), pk_exp(geo[1]), pk_exp(geo[2])};
    const float q0 = geo[4], q1 = geo[5], q2 = geo[6], q3 = geo[7];
    const float len = __builtin_sqrtf(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    const float qr = q0 / len, qx = q1 / len, qy = q2 / len, qz = q3 / len;
    float R[3][3]; // [c][r], process_gaussians.wgsl:127-162
    R[0][0] = 1.f - 2.f * (qy * qy + qz * qz); R[0][1] = 2.f * (qx * qy - qr * qz); R[0][2] = 2.f * (qx * qz + qr * qy);
    R[1][0] = 2.f * (qx * qy + qr * qz); R[1][1] = 1.f - 2.f * (qx * qx + qz * qz); R[1][2] = 2.f * (qy * qz - qr * qx);
    R[2][0] = 2.f * (qx * qz - qr * qy); R[2][1] = 2.f * (qy * qz + qr * qx); R[2][2] = 1.f - 2.f * (qx * qx + qy * qy);
    float M[3][3];
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) M[c][r] = sc[r] * R[c][r];
    // Sigma = transpose(M) * M, entry [c][r] = (M[r][0] M[c][0] + M[r][1] M[c][1]) + M[r][2] M[c][2]; the six the projection keeps
#define MG_SIG(c, r) ((M[r][0] * M[c][0] + M[r][1] * M[c][1]) + M[r][2] * M[c][2])
    out->sig[0] = MG_SIG(0, 0); out->sig[1] = MG_SIG(0, 1); out->sig[2] = MG_SIG(0, 2);
    out->sig[3] = MG_SIG(1, 1); out->sig[4] = MG_SIG(1, 2); out->sig[5] = MG_SIG(2, 2);
#undef MG_SIG
    const float A = mg_max(sc[0] * sc[1], mg_max(sc[0] * sc[2], sc[1] * sc[2]));
    out->w = mg_sigmoid(geo[3]) * A;
    bool ok = pk_finite(out->w) && out->w > 0.0f;
    for (int k = 0; k < 6; ++k) ok = ok && pk_finite(out->sig[k]);
    return ok;
}

// ---- the grid ---------------------------------------------------------------------------------------------------------------------------
// The grid record, the finite test, the cell coordinate, the key packing and the choice of the grid are the neighbourhoods'
// (gs_grid_math.h): the cell merge asks neigh_choose_grid for the requested edge itself instead of 1.0011 radius.

// ---- the sums ---------------------------------------------------------------------------------------------------------------------------
// What slot q (0 .. 57) adds for one member before the weight: acc[q] += w * x, w the weight as double.  d = (double)p - c; sh: the
// member's SH float of slot q (q >= 10), anything otherwise.  Slot 0 adds w * 1.0 = w.
GS_PK double mg_slot_x(uint32_t q, double d0, double d1, double d2, const float sig[6], float sh) {
    if (q >= MG_SLOT_H) return (double)sh;
    if (q == MG_SLOT_W) return 1.0;
    if (q < MG_SLOT_M) return q == 1u ? d0 : q == 2u ? d1 : d2;
    const uint32_t e = q - MG_SLOT_M; // xx xy xz yy yz zz
    const double dk = e < 3u ? d0 : e < 5u ? d1 : d2;
    const double dl = (e == 0u) ? d0 : (e == 1u || e == 3u) ? d1 : d2;
    const float s = e == 0u ? sig[0] : e == 1u ? sig[1] : e == 2u ? sig[2] : e == 3u ? sig[3] : e == 4u ? sig[4] : sig[5];
    double t = dk * dl;
    t = (double)s + t;
    return t;
}

// ---- finishing --------------------------------------------------------------------------------------------------------------------------
// One Jacobi rotation that zeroes a[P][Q] of the symmetric a; the rotation is accumulated into the columns P, Q of v.
template <int P, int Q>
GS_PK void mg_rotate(double a[3][3], double v[3][3]) {
    const double apq = a[P][Q];
    if (!(apq != 0.0)) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    for (int k = 0; k < 3; ++k) { const double x = a[k][P], y = a[k][Q]; a[k][P] = c * x - s * y; a[k][Q] = s * x + c * y; }
    for (int k = 0; k < 3; ++k) { const double x = a[P][k], y = a[Q][k]; a[P][k] = c * x - s * y; a[Q][k] = s * x + c * y; }
    for (int k = 0; k < 3; ++k) { const double x = v[k][P], y = v[k][Q]; v[k][P] = c * x - s * y; v[k][Q] = s * x + c * y; }
}
template <int I, int J>
GS_PK void mg_order(double l[3], double v[3][3]) { // the larger eigenvalue first, its column with it
    if (l[I] < l[J]) {
        const double t = l[I]; l[I] = l[J]; l[J] = t;
        for (int k = 0; k < 3; ++k) { const double x = v[k][I]; v[k][I] = v[k][J]; v[k][J] = x; }
    }
}
// s: the 64 doubles of a merged group; rec: the 80 floats of its record (all written).
GS_PK void mg_finish(const double* s, float* rec) {
    for (int k = 0; k < 80; ++k) rec[k] = 0.0f;
    const double W = s[MG_SLOT_W];
    const double mu[3] = {s[1] / W, s[2] / W, s[3] / W};
    for (int k = 0; k < 3; ++k) rec[k] = (float)(s[MG_SLOT_C + k] + mu[k]);
    double a[3][3], v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    a[0][0] = s[4] / W - mu[0] * mu[0];
    a[0][1] = a[1][0] = s[5] / W - mu[0] * mu[1];
    a[0][2] = a[2][0] = s[6] / W - mu[0] * mu[2];
    a[1][1] = s[7] / W - mu[1] * mu[1];
    a[1][2] = a[2][1] = s[8] / W - mu[1] * mu[2];
    a[2][2] = s[9] / W - mu[2] * mu[2];
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
        l[k] = (l[k] >= 1e-30) ? l[k] : 1e-30; // (a NaN too)
        rec[4 + k] = (float)(0.5 * log(l[k]));
    }
    // the eigenvectors are the columns of a rotation: the third is flipped when they are left-handed
    const double det = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0]) +
                       v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
    if (det < 0.0)
        for (int k = 0; k < 3; ++k) v[k][2] = -v[k][2];
    // the quaternion (r, x, y, z) of the rotation v[row][column], by its largest component
    const double tr = v[0][0] + v[1][1] + v[2][2];
    double q[4];
    if (tr > 0.0) {
        const double S = sqrt(tr + 1.0) * 2.0;
        q[0] = 0.25 * S; q[1] = (v[2][1] - v[1][2]) / S; q[2] = (v[0][2] - v[2][0]) / S; q[3] = (v[1][0] - v[0][1]) / S;
    } else if (v[0][0] > v[1][1] && v[0][0] > v[2][2]) {
        const double S = sqrt(1.0 + v[0][0] - v[1][1] - v[2][2]) * 2.0;
        q[0] = (v[2][1] - v[1][2]) / S; q[1] = 0.25 * S; q[2] = (v[0][1] + v[1][0]) / S; q[3] = (v[0][2] + v[2][0]) / S;
    } else if (v[1][1] > v[2][2]) {
        const double S = sqrt(1.0 + v[1][1] - v[0][0] - v[2][2]) * 2.0;
        q[0] = (v[0][2] - v[2][0]) / S; q[1] = (v[0][1] + v[1][0]) / S; q[2] = 0.25 * S; q[3] = (v[1][2] + v[2][1]) / S;
    } else {
        const double S = sqrt(1.0 + v[2][2] - v[0][0] - v[1][1]) * 2.0;
        q[0] = (v[1][0] - v[0][1]) / S; q[1] = (v[0][2] + v[2][0]) / S; q[2] = (v[1][2] + v[2][1]) / S; q[3] = 0.25 * S;
    }
    const double qn = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    const double sgn = q[0] < 0.0 ? -1.0 : 1.0;
    for (int k = 0; k < 4; ++k) rec[8 + k] = (float)(sgn * q[k] / qn);
    // opacity x area is conserved: alpha' A' = W with A' the cross-section of the two largest axes
    const double area = sqrt(l[0] * l[1]);
    double al = W / area;
    al = (al < 0.99) ? al : 0.99;
    rec[12] = (float)log(al / (1.0 - al));
    for (int k = 0; k < 16; ++k)
        for (int ch = 0; ch < 3; ++ch) rec[16 + 4 * k + ch] = (float)(s[MG_SLOT_H + 3 * k + ch] / W);
}

// ---- host only ----------------------------------------------------------------------------------------------------------------------
// What the refusals of the three entry points share; *why: the message's tail.
inline bool merge_params_ok(const gs_merge* p, const char** why) {
    if (!p) { *why = "null params"; return false; }
    if (p->struct_size != sizeof(gs_merge)) { *why = "struct_size is not sizeof(gs_merge)"; return false; }
    if (p->mask > 0xFFu || p->value > 0xFFu) { *why = "the filter does not fit the state byte"; return false; }
    if (!pk_finite(p->cell) || !(p->cell > 0.0f)) { *why = "cell is not a finite number above 0"; return false; }
    if (p->min_members < 2u) { *why = "min_members is below 2"; return false; }
    if (p->op > GS_STATE_ASSIGN) { *why = "unknown op (0, GS_STATE_SET .. GS_STATE_ASSIGN)"; return false; }
    if (p->op == 0u && p->bits != 0u) { *why = "bits without an op"; return false; }
    if (p->bits > 0xFFu) { *why = "bits do not fit the state byte"; return false; }
    return true;
}
inline uint32_t merge_max_members(const gs_merge* p) { return p->max_members ? p->max_members : GS_MERGE_DEFAULT_MAX_MEMBERS; }

// The whole call over n host records (80 floats each).  Returns 0, or 1: the fullest cell exceeds max_members (info filled, nothing
// written), or 2: cap < groups (info filled, nothing written).  aos == null with cap == 0: count only.
inline int merge_host(const float* rec, uint8_t* state, uint64_t n, const gs_merge* p, float* aos, uint64_t cap, double* sums, uint32_t* group_of,
                      gs_merge_info* info) {
    *info = gs_merge_info{};
    const bool filter = (p->mask | p->value) != 0u;
    auto passes = [&](uint64_t i) { return !filter || ((uint32_t)state[i] & p->mask) == p->value; };
    // the bounds: filter plus finite position, in the total order of the bit patterns
    uint32_t klo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, khi[3] = {0u, 0u, 0u};
    uint64_t bounded = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const float* r = rec + i * 80;
        if (!passes(i) || !neigh_finite(r[0], r[1], r[2])) continue;
        ++bounded;
        for (int k = 0; k < 3; ++k) { klo[k] = std::min(klo[k], pk_okey(r[k])); khi[k] = std::max(khi[k], pk_okey(r[k])); }
    }
    if (!bounded) { // nothing to group: every splat reads GS_MERGE_NONE
        if (aos && group_of)
            for (uint64_t i = 0; i < n; ++i) group_of[i] = GS_MERGE_NONE;
        return 0;
    }
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = pk_okey_value(klo[k]); hi[k] = pk_okey_value(khi[k]); }
    GsNeighGrid g;
    neigh_choose_grid(lo, hi, p->cell, &g, &info->cell_edge);
    for (int k = 0; k < 3; ++k) info->cells[k] = g.g[k];
    std::vector<uint64_t> pairs; // key << 32 | id: ascending key, ascending id inside a key
    for (uint64_t i = 0; i < n; ++i) {
        const float* r = rec + i * 80;
        if (!passes(i) || !neigh_finite(r[0], r[1], r[2])) continue;
        const float geo[8] = {r[4], r[5], r[6], r[12], r[8], r[9], r[10], r[11]};
        MgSplat sp;
        if (!mg_splat(geo, &sp)) continue;
        pairs.push_back(((uint64_t)neigh_key(g, r[0], r[1], r[2]) << 32) | i);
    }
    std::sort(pairs.begin(), pairs.end());
    info->eligible = pairs.size();
    struct Run { size_t begin, len; };
    std::vector<Run> merged;
    for (size_t b = 0; b < pairs.size();) {
        size_t e = b + 1;
        while (e < pairs.size() && (pairs[e] >> 32) == (pairs[b] >> 32)) ++e;
        info->largest = std::max<uint64_t>(info->largest, e - b);
        if (e - b >= p->min_members) { merged.push_back(Run{b, e - b}); info->members += e - b; }
        b = e;
    }
    info->groups = merged.size();
    if (info->largest > merge_max_members(p)) return 1;
    if (!aos && !cap) return 0;
    if (cap < info->groups) return 2;
    if (group_of)
        for (uint64_t i = 0; i < n; ++i) group_of[i] = GS_MERGE_NONE;
    for (size_t gi = 0; gi < merged.size(); ++gi) {
        double acc[GS_MERGE_SUM_DOUBLES];
        for (uint32_t q = 0; q < GS_MERGE_SUM_DOUBLES; ++q) acc[q] = 0.0;
        const uint64_t first = pairs[merged[gi].begin] & 0xFFFFFFFFull;
        const double c[3] = {(double)rec[first * 80 + 0], (double)rec[first * 80 + 1], (double)rec[first * 80 + 2]};
        for (size_t m = 0; m < merged[gi].len; ++m) {
            const uint64_t i = pairs[merged[gi].begin + m] & 0xFFFFFFFFull;
            const float* r = rec + i * 80;
            const float geo[8] = {r[4], r[5], r[6], r[12], r[8], r[9], r[10], r[11]};
            MgSplat sp;
            mg_splat(geo, &sp);
            const double w = (double)sp.w, d0 = (double)r[0] - c[0], d1 = (double)r[1] - c[1], d2 = (double)r[2] - c[2];
            for (uint32_t q = 0; q < MG_SLOT_COUNT; ++q) {
                const uint32_t j = q >= MG_SLOT_H ? q - MG_SLOT_H : 0u; // SH plane index 3 k + channel -> record float 16 + 4 k + channel
                double t = mg_slot_x(q, d0, d1, d2, sp.sig, r[16 + 4 * (j / 3u) + j % 3u]);
                t = w * t;
                acc[q] += t;
            }
            if (group_of) group_of[i] = (uint32_t)gi;
        }
        acc[MG_SLOT_COUNT] = (double)merged[gi].len;
        acc[MG_SLOT_FIRST] = (double)first;
        for (int k = 0; k < 3; ++k) acc[MG_SLOT_C + k] = c[k];
        if (sums)
            for (uint32_t q = 0; q < GS_MERGE_SUM_DOUBLES; ++q) sums[gi * GS_MERGE_SUM_DOUBLES + q] = acc[q];
        mg_finish(acc, aos + gi * 80);
    }
    if (p->op) // after the outputs are complete
        for (size_t gi = 0; gi < merged.size(); ++gi)
            for (size_t m = 0; m < merged[gi].len; ++m) {
                uint8_t& s = state[pairs[merged[gi].begin + m] & 0xFFFFFFFFull];
                const uint32_t b = p->bits;
                s = (uint8_t)(p->op == GS_STATE_SET ? (s | b) : p->op == GS_STATE_CLEAR ? (s & ~b) : p->op == GS_STATE_TOGGLE ? (s ^ b) : b);
            }
    return 0;
}
