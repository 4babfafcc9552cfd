// gs_pack_math.h -- the packed scene codec (gs_abi.h "packed scenes"), written once: the host codec (gs_pack_host.hip) and the
// kernels (k_pack.hip) both compile this one copy, the way the transforms and the grades share gs_xform_math / gs_grade_math.
// Plain C++ when the compiler is not hipcc (tools/pack_check builds it with a host compiler and sanitizers).
//
// All arithmetic is f32, one IEEE rounding per written operation (the library is built with -ffp-contract=off and IEEE / and sqrt;
// a host compiler without fused multiply-add contraction gives the same bits).  The helpers that gs_device.h defines for device code
// only -- wg_min / wg_max, f2u_sat / f2i_sat, gs_exp -- have their host-and-device twins here (pk_*), operation for operation:
// tests/test_packed.py holds pk_exp to the oracle's expf.
//
// A minimum or maximum of a chunk is taken in the TOTAL order of the bit patterns (pk_okey: -0.0 below +0.0; every value that
// takes part is finite), so that any reduction order gives the same bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_PK __host__ __device__ __forceinline__
#else
#define GS_PK inline
#endif

#define GS_PACK_CHUNK 256u       // splats per chunk
#define GS_PACK_CHUNK_FLOATS 18u // floats of a chunk record

GS_PK uint32_t pk_bits(float v) { uint32_t b; __builtin_memcpy(&b, &v, 4); return b; }
GS_PK float pk_float(uint32_t b) { float v; __builtin_memcpy(&v, &b, 4); return v; }
GS_PK float pk_max(float a, float b) { return (a < b) ? b : a; }
GS_PK float pk_min(float a, float b) { return (b < a) ? b : a; }
GS_PK int pk_mini(int a, int b) { return (b < a) ? b : a; }
GS_PK int pk_f2i_sat(float x) { // f32 -> i32: truncate, saturate, NaN -> 0
    if (x != x) return 0;
    if (x >= 2147483648.0f) return 2147483647;
    if (x <= -2147483648.0f) return (-2147483647 - 1);
    return (int)x;
}
GS_PK uint32_t pk_f2u_sat(float x) {
    if (x != x) return 0u;
    if (x >= 4294967296.0f) return 0xFFFFFFFFu;
    if (x <= 0.0f) return 0u;
    return (uint32_t)x;
}
// gs_exp (gs_device.h), callable from the host: the same operations in the same order
GS_PK float pk_exp(float x) {
    if (x != x) return x;
    if (x > 88.72283935546875f) return __builtin_inff();
    if (x < -103.97208404541015625f) return 0.0f;
    const float nf = __builtin_rintf(x * 1.44269502162933349609375f);
    float r = __builtin_fmaf(-nf, 0.693145751953125f, x);
    r = __builtin_fmaf(-nf, 1.42860677465796470642e-06f, r);
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float z = r * r;
    float y = __builtin_fmaf(p, z, r);
    y = y + 1.0f;
    const int n = (int)nf;
    const int a = n >> 1;
    const int b = n - a;
    const float sa = pk_float((uint32_t)(a + 127) << 23);
    const float sb = pk_float((uint32_t)(b + 127) << 23);
    return (y * sa) * sb;
}

GS_PK bool pk_finite(float v) { return (pk_bits(v) & 0x7F800000u) != 0x7F800000u; }
GS_PK float pk_fin(float v) { return pk_finite(v) ? v : 0.0f; }
// the order-preserving map of a bit pattern and its inverse
GS_PK uint32_t pk_okey(float v) { const uint32_t b = pk_bits(v); return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
GS_PK float pk_okey_value(uint32_t k) { return pk_float((k >> 31) ? k ^ 0x80000000u : ~k); }

GS_PK uint32_t pk_unorm(float v, float T) { return pk_f2u_sat(pk_min(T, pk_max(0.0f, v * T + 0.5f))); } // T = 2^b - 1
GS_PK float pk_norm(float v, float lo, float hi) { return (hi > lo) ? (v - lo) / (hi - lo) : 0.0f; }
GS_PK float pk_lerp(float lo, float hi, float t) { return lo * (1.0f - t) + hi * t; }
GS_PK float pk_dn(uint32_t code, float T) { return (float)code / T; }

// ---- what an entry contributes before its chunk's bounds are known -----------------------------------------------------------------
struct PkEntry {
    float px, py, pz; // fin(position)
    float sx, sy, sz; // clamped log-scales
    float cr, cg, cb; // base colour
    uint32_t rot;     // packed_rotation
    uint32_t a8;      // unorm(alpha, 8)
    uint32_t bad;     // carried floats that fin replaced, plus a NaN logit
};
GS_PK float pk_scale(float v) { return pk_max(-20.0f, pk_min(20.0f, pk_fin(v))); }
GS_PK float pk_colour(float v) { return pk_fin(v) * 0.28209479177387814f + 0.5f; }
GS_PK float pk_alpha(float o) {
    if (o != o) return 0.0f;
    if (o >= 0.0f) return 1.0f / (1.0f + pk_exp(-o));
    const float ez = pk_exp(o);
    return ez / (1.0f + ez);
}
GS_PK uint32_t pk_rotation(float q0, float q1, float q2, float q3) {
    q0 = pk_fin(q0); q1 = pk_fin(q1); q2 = pk_fin(q2); q3 = pk_fin(q3);
    const float len = __builtin_sqrtf(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    if (!(len > 0.0f) || !pk_finite(len)) { q0 = 1.0f; q1 = q2 = q3 = 0.0f; }
    else { q0 = q0 / len; q1 = q1 / len; q2 = q2 / len; q3 = q3 / len; }
    uint32_t L = 0u;
    float big = __builtin_fabsf(q0);
    if (__builtin_fabsf(q1) > big) { big = __builtin_fabsf(q1); L = 1u; }
    if (__builtin_fabsf(q2) > big) { big = __builtin_fabsf(q2); L = 2u; }
    if (__builtin_fabsf(q3) > big) { big = __builtin_fabsf(q3); L = 3u; }
    const float qL = L == 0u ? q0 : L == 1u ? q1 : L == 2u ? q2 : q3;
    if (qL < 0.0f) { q0 = -q0; q1 = -q1; q2 = -q2; q3 = -q3; }
    const float t0 = L == 0u ? q1 : q0, t1 = L <= 1u ? q2 : q1, t2 = L == 3u ? q2 : q3;
    const float h = 0.70710678118654752f;
    return (L << 30) | (pk_unorm(t0 * h + 0.5f, 1023.0f) << 20) | (pk_unorm(t1 * h + 0.5f, 1023.0f) << 10) | pk_unorm(t2 * h + 0.5f, 1023.0f);
}
// pos, lsc, dc: three floats each; rot: four (r, x, y, z)
GS_PK PkEntry pk_entry(float x, float y, float z, float s0, float s1, float s2, float q0, float q1, float q2, float q3, float logit, float d0, float d1,
                       float d2) {
    PkEntry e;
    e.px = pk_fin(x); e.py = pk_fin(y); e.pz = pk_fin(z);
    e.sx = pk_scale(s0); e.sy = pk_scale(s1); e.sz = pk_scale(s2);
    e.cr = pk_colour(d0); e.cg = pk_colour(d1); e.cb = pk_colour(d2);
    e.rot = pk_rotation(q0, q1, q2, q3);
    e.a8 = pk_unorm(pk_alpha(logit), 255.0f);
    e.bad = (uint32_t)!pk_finite(x) + (uint32_t)!pk_finite(y) + (uint32_t)!pk_finite(z) + (uint32_t)!pk_finite(s0) + (uint32_t)!pk_finite(s1) +
            (uint32_t)!pk_finite(s2) + (uint32_t)!pk_finite(q0) + (uint32_t)!pk_finite(q1) + (uint32_t)!pk_finite(q2) + (uint32_t)!pk_finite(q3) +
            (uint32_t)!pk_finite(d0) + (uint32_t)!pk_finite(d1) + (uint32_t)!pk_finite(d2) + (uint32_t)(logit != logit);
    return e;
}
GS_PK uint32_t pk_pack_11_10_11(float x, float y, float z, const float* lo, const float* hi) {
    return (pk_unorm(pk_norm(x, lo[0], hi[0]), 2047.0f) << 21) | (pk_unorm(pk_norm(y, lo[1], hi[1]), 1023.0f) << 11) |
           pk_unorm(pk_norm(z, lo[2], hi[2]), 2047.0f);
}
// The four words of an entry under its chunk record b (18 floats: min xyz, max xyz of the position, the scale, the colour).
GS_PK void pk_vertex(const PkEntry& e, const float* b, uint32_t* w) {
    w[0] = pk_pack_11_10_11(e.px, e.py, e.pz, b + 0, b + 3);
    w[1] = e.rot;
    w[2] = pk_pack_11_10_11(e.sx, e.sy, e.sz, b + 6, b + 9);
    w[3] = (pk_unorm(pk_norm(e.cr, b[12], b[15]), 255.0f) << 24) | (pk_unorm(pk_norm(e.cg, b[13], b[16]), 255.0f) << 16) |
           (pk_unorm(pk_norm(e.cb, b[14], b[17]), 255.0f) << 8) | e.a8;
}
GS_PK uint32_t pk_sh_byte(float v) { return pk_f2u_sat(pk_min(255.0f, pk_max(0.0f, (pk_fin(v) / 8.0f + 0.5f) * 256.0f))); }
GS_PK float pk_sh_value(uint32_t byte) { return (((float)byte + 0.5f) / 256.0f - 0.5f) * 8.0f; }

// ---- decode -------------------------------------------------------------------------------------------------------------------------
struct PkDecoded { float pos[3], lsc[3], rot[4], logit, dc[3]; };
GS_PK void pk_unpack_11_10_11(uint32_t w, const float* lo, const float* hi, float* out) {
    out[0] = pk_lerp(lo[0], hi[0], pk_dn(w >> 21, 2047.0f));
    out[1] = pk_lerp(lo[1], hi[1], pk_dn((w >> 11) & 1023u, 1023.0f));
    out[2] = pk_lerp(lo[2], hi[2], pk_dn(w & 2047u, 2047.0f));
}
// w: the vertex's four words; b: its chunk record; table: the 256 logits (gs_pack_logit_table)
GS_PK PkDecoded pk_decode(const uint32_t* w, const float* b, const float* table) {
    PkDecoded d;
    pk_unpack_11_10_11(w[0], b + 0, b + 3, d.pos);
    pk_unpack_11_10_11(w[2], b + 6, b + 9, d.lsc);
    const float r2 = 1.41421356237309505f;
    const float t0 = (pk_dn((w[1] >> 20) & 1023u, 1023.0f) - 0.5f) * r2, t1 = (pk_dn((w[1] >> 10) & 1023u, 1023.0f) - 0.5f) * r2,
                t2 = (pk_dn(w[1] & 1023u, 1023.0f) - 0.5f) * r2;
    const float m = __builtin_sqrtf(pk_max(0.0f, 1.0f - ((t0 * t0 + t1 * t1) + t2 * t2)));
    const uint32_t L = w[1] >> 30;
    d.rot[0] = L == 0u ? m : t0;
    d.rot[1] = L == 1u ? m : (L == 0u ? t0 : t1);
    d.rot[2] = L == 2u ? m : (L == 3u ? t2 : t1);
    d.rot[3] = L == 3u ? m : t2;
    d.logit = table[w[3] & 255u];
    d.dc[0] = (pk_lerp(b[12], b[15], pk_dn(w[3] >> 24, 255.0f)) - 0.5f) / 0.28209479177387814f;
    d.dc[1] = (pk_lerp(b[13], b[16], pk_dn((w[3] >> 16) & 255u, 255.0f)) - 0.5f) / 0.28209479177387814f;
    d.dc[2] = (pk_lerp(b[14], b[17], pk_dn((w[3] >> 8) & 255u, 255.0f)) - 0.5f) / 0.28209479177387814f;
    return d;
}

// ---- Morton order -------------------------------------------------------------------------------------------------------------------
GS_PK uint32_t pk_spread3(uint32_t v) { // bit b of a 10-bit number -> bit 3 b
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
#define GS_PACK_KEY_LAST (1u << 30) // a splat with a non-finite coordinate: above every key, it sorts last
GS_PK uint32_t pk_morton_key(float x, float y, float z, const float* lo, const float* hi) {
    if (!pk_finite(x) || !pk_finite(y) || !pk_finite(z)) return GS_PACK_KEY_LAST;
    const uint32_t qx = (uint32_t)pk_mini(1023, pk_f2i_sat(pk_norm(x, lo[0], hi[0]) * 1024.0f));
    const uint32_t qy = (uint32_t)pk_mini(1023, pk_f2i_sat(pk_norm(y, lo[1], hi[1]) * 1024.0f));
    const uint32_t qz = (uint32_t)pk_mini(1023, pk_f2i_sat(pk_norm(z, lo[2], hi[2]) * 1024.0f));
    return pk_spread3(qx) | (pk_spread3(qy) << 1) | (pk_spread3(qz) << 2);
}
