// k_xform.hip -- the kernel behind gs_transform_splats (gs_xform.hip, gs_abi.h "splat transforms"): a similarity applied in place to
// the resident planes of the splats a selection names.  The reference has no counterpart: it is a viewer, and an editor built on
// it would edit its own 320-byte records (the SH rotation included) and upload them again.
//
// One thread per (entry, part), compiled per flag set so that an unflagged part costs no traffic and no thread:
//   part 0    : the position (3 x 4 B each way), the three log-scales and smax (12 B read, 16 B written), the rot quaternion
//               (one float4 each way) -- whichever of them the flag set names;
//   parts 1-3 : (ORIENT only) one colour channel each: the 15 coefficients of bands 1..3 in, 15 out, every output of a band from
//               the old values of the band.  The three channel threads of a splat are adjacent lanes and their 4-byte accesses
//               interleave (packed float 3k + c), so the splat's 180 contiguous bytes are used whole.
// Entry g is splat ids[g] (the ascending list of the splat edits' selection, k_export.hip), or splat g when ids is null (the (0, 0)
// filter: dense over 0..N, as gs_unpack_kernel).  Every id is checked against N.  Every access is per splat -- 4-byte plane words,
// the splat's own 32-byte geometry record, its own 192-byte SH record -- so a plane whose length is no multiple of a vector width
// has no tail to plan: nothing before splat 0 or past splat N - 1 is read or written.
// The gs_xform is passed BY VALUE: its 12 + 4 + 1 + 83 floats are uniform kernel arguments (scalar loads), no vector register
// holds a matrix entry.  One f32 rounding per written operation, left to right (gs_abi.h): the build's -ffp-contract=off keeps
// the multiplies and adds apart, as for the EXACT blend and the state kernels.
// Traffic per matched splat: POSITION 12 + 12 B, ORIENT 196 + 196 B, SIZE 12 + 16 B, 4 B of id when a list is given (what building
// that list costs -- the selection's two reads of the state plane -- is stated with the call in gs_abi.h "splat transforms").
// Bound: HBM.  No MFMA (no contraction; 83 multiply-adds per channel do not come near the issue rate).  Every store is a plain
// vector store.
#include "../../include/gsplat/gs_abi.h"
#include "gs_device.h"
#include "gs_kernels.h"

// out_i = sum_j D[i][j] in_j:  acc = D[i][0] in_0;  acc = acc + D[i][j] in_j  for j ascending
template <int N>
__device__ __forceinline__ void xform_band(const float* D, const float* in, float* out) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float acc = D[i * N] * in[0];
#pragma unroll
        for (int j = 1; j < N; ++j) acc = acc + D[i * N + j] * in[j];
        out[i] = acc;
    }
}

template <uint32_t FL>
__global__ __launch_bounds__(256) void gs_xform_kernel(float* px, float* py, float* pz, float* smax, float4* geo, float* sh, uint32_t n,
                                                        const uint32_t* __restrict__ ids, uint32_t m, const gs_xform x) {
    constexpr uint32_t PARTS = (FL & GS_XFORM_ORIENT) ? 4u : 1u;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)m * PARTS) return;
    const uint32_t g = (uint32_t)(t / PARTS), part = (uint32_t)(t % PARTS);
    const uint32_t id = ids ? ids[g] : g;
    if (id >= n) return; // (never: ids come from the selection over this scene, and m <= n without a list)
    if (part == 0u) {
        if (FL & GS_XFORM_POSITION) {
            const float X = px[id], Y = py[id], Z = pz[id];
            px[id] = ((x.m[0] * X + x.m[1] * Y) + x.m[2] * Z) + x.m[3];
            py[id] = ((x.m[4] * X + x.m[5] * Y) + x.m[6] * Z) + x.m[7];
            pz[id] = ((x.m[8] * X + x.m[9] * Y) + x.m[10] * Z) + x.m[11];
        }
        if (FL & GS_XFORM_SIZE) {
            float* r = reinterpret_cast<float*>(geo + (uint64_t)id * 2); // log-scale xyz; r[3], the opacity, is not touched
            const float l0 = r[0] + x.log_scale, l1 = r[1] + x.log_scale, l2 = r[2] + x.log_scale;
            r[0] = l0; r[1] = l1; r[2] = l2;
            smax[id] = __builtin_fmaxf(l0, __builtin_fmaxf(l1, l2)); // gs_repack_kernel's expression
        }
        if (FL & GS_XFORM_ORIENT) {
            const float4 b = geo[(uint64_t)id * 2 + 1]; // r, x, y, z
            const float ar = x.q[0], ax = x.q[1], ay = x.q[2], az = x.q[3];
            float4 o;
            o.x = ((ar * b.x - ax * b.y) - ay * b.z) - az * b.w;
            o.y = ((ar * b.y + ax * b.x) + ay * b.w) - az * b.z;
            o.z = ((ar * b.z - ax * b.w) + ay * b.x) + az * b.y;
            o.w = ((ar * b.w + ax * b.z) - ay * b.y) + az * b.x;
            geo[(uint64_t)id * 2 + 1] = o;
        }
    } else if (FL & GS_XFORM_ORIENT) {
        float* s = sh + (uint64_t)id * 48 + 3u + (part - 1u); // coefficient k of this channel: s[3 (k - 1)], k = 1..15
        float in[15], out[15];
#pragma unroll
        for (int k = 0; k < 15; ++k) in[k] = s[3 * k];
        xform_band<3>(x.sh1, in, out);
        xform_band<5>(x.sh2, in + 3, out + 3);
        xform_band<7>(x.sh3, in + 8, out + 8);
#pragma unroll
        for (int k = 0; k < 15; ++k) s[3 * k] = out[k];
    }
}

void gs_launch_xform(const GsScene& s, uint32_t n, const uint32_t* ids, uint32_t m, const gs_xform& x, hipStream_t st) {
    const uint32_t fl = x.flags & (GS_XFORM_POSITION | GS_XFORM_ORIENT | GS_XFORM_SIZE);
    if (!m || !fl) return;
    const uint64_t total = (uint64_t)m * ((fl & GS_XFORM_ORIENT) ? 4u : 1u);
    const dim3 grid((uint32_t)((total + 255) / 256));
#define GS_XFORM_LAUNCH(F)                                                                                                        \
    hipLaunchKernelGGL(gs_xform_kernel<F>, grid, dim3(256), 0, st, (float*)s.px, (float*)s.py, (float*)s.pz, (float*)s.smax, (float4*)s.geo, \
                       (float*)s.sh, n, ids, m, x)
    switch (fl) {
    case 1u: GS_XFORM_LAUNCH(1u); break;
    case 2u: GS_XFORM_LAUNCH(2u); break;
    case 3u: GS_XFORM_LAUNCH(3u); break;
    case 4u: GS_XFORM_LAUNCH(4u); break;
    case 5u: GS_XFORM_LAUNCH(5u); break;
    case 6u: GS_XFORM_LAUNCH(6u); break;
    default: GS_XFORM_LAUNCH(7u); break;
    }
#undef GS_XFORM_LAUNCH
}
