// k_grade.hip -- the kernel behind gs_grade_splats (gs_grade.hip, gs_abi.h "colour grades"): an affine map of the displayed colour,
// applied in place to the SH coefficients of the splats a selection names, and a step of their opacity logit.  The reference has no
// counterpart: it is a viewer, and an editor built on it would edit its own 320-byte records and upload them again.
//
// One thread per (entry, part), compiled per flag set so that an unflagged part costs no traffic and no thread:
//   with MATRIX : four parts per entry.  Part p takes the coefficients 4p .. 4p + 3: packed floats 12p .. 12p + 11 of the splat's
//                 192-byte SH record (packed float 3k + c), three float4 each way, 16-byte aligned.  The four part threads of a
//                 splat are adjacent lanes, so a wave's three loads cover 16 whole records: every fetched line is used whole.  Every
//                 output triple comes from the OLD triple.  Part 0 also adds dc to coefficient 0 (OFFSET) and does the opacity
//                 (OPACITY): float 3 of the splat's first geo float4, 4 B each way;
//   without it  : one thread per entry: the three band-0 floats (OFFSET, 12 B each way) and / or the opacity logit.
// Entry g is splat ids[g] (the ascending list of the splat edits' selection, k_export.hip), or splat g when ids is null (the (0, 0)
// filter: dense over 0..N).  Every id is checked against N.  Every access stays inside the splat's own records, so there is no
// tail to plan: nothing before splat 0 or past splat N - 1 is read or written.
// The gs_grade is passed BY VALUE: its 9 + 3 + 1 floats are uniform kernel arguments (scalar loads), no vector register holds a
// matrix entry.  One f32 rounding per written operation, left to right (gs_abi.h): the build's -ffp-contract=off keeps the
// multiplies and adds apart, as for the transforms.
// Traffic per matched splat: MATRIX 192 + 192 B, OFFSET alone 12 + 12 B, OPACITY 4 + 4 B, 4 B of id when a list is given.
// Bound: HBM.  No MFMA (15 flops per triple), no LDS.  Every store is a plain vector store.
#include "../../include/gsplat/gs_abi.h"
#include "gs_device.h"
#include "gs_kernels.h"

// (r, g, b) -> A (r, g, b): out_c = (a[3c] r + a[3c+1] g) + a[3c+2] b, every output from the old triple
__device__ __forceinline__ void grade_triple(const float* a, float& r, float& g, float& b) {
    const float R = (a[0] * r + a[1] * g) + a[2] * b;
    const float G = (a[3] * r + a[4] * g) + a[5] * b;
    const float B = (a[6] * r + a[7] * g) + a[8] * b;
    r = R; g = G; b = B;
}

template <uint32_t FL>
__global__ __launch_bounds__(256) void gs_grade_kernel(float4* geo, float4* sh, uint32_t n, const uint32_t* __restrict__ ids, uint32_t m,
                                                        const gs_grade x) {
    constexpr uint32_t PARTS = (FL & GS_GRADE_MATRIX) ? 4u : 1u;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)m * PARTS) return;
    const uint32_t g = (uint32_t)(t / PARTS), part = (uint32_t)(t % PARTS);
    const uint32_t id = ids ? ids[g] : g;
    if (id >= n) return; // (never: ids come from the selection over this scene, and m <= n without a list)
    if (FL & GS_GRADE_MATRIX) {
        float4* s = sh + (uint64_t)id * 12 + part * 3u; // the splat's record is 12 float4; this part's three
        float4 v0 = s[0], v1 = s[1], v2 = s[2];
        grade_triple(x.a, v0.x, v0.y, v0.z);
        grade_triple(x.a, v0.w, v1.x, v1.y);
        grade_triple(x.a, v1.z, v1.w, v2.x);
        grade_triple(x.a, v2.y, v2.z, v2.w);
        if ((FL & GS_GRADE_OFFSET) && part == 0u) {
            v0.x = v0.x + x.dc[0];
            v0.y = v0.y + x.dc[1];
            v0.z = v0.z + x.dc[2];
        }
        s[0] = v0; s[1] = v1; s[2] = v2;
    } else if (FL & GS_GRADE_OFFSET) {
        float* s = reinterpret_cast<float*>(sh + (uint64_t)id * 12); // band 0: packed floats 0..2; float 3 is not touched
        const float r = s[0] + x.dc[0], gr = s[1] + x.dc[1], b = s[2] + x.dc[2];
        s[0] = r; s[1] = gr; s[2] = b;
    }
    if ((FL & GS_GRADE_OPACITY) && part == 0u) {
        float* o = reinterpret_cast<float*>(geo + (uint64_t)id * 2) + 3; // the opacity logit; the log-scales before it are not touched
        *o = *o + x.opacity_logit;
    }
}

void gs_launch_grade(const GsScene& s, uint32_t n, const uint32_t* ids, uint32_t m, const gs_grade& x, hipStream_t st) {
    const uint32_t fl = x.flags & (GS_GRADE_MATRIX | GS_GRADE_OFFSET | GS_GRADE_OPACITY);
    if (!m || !fl) return;
    const uint64_t total = (uint64_t)m * ((fl & GS_GRADE_MATRIX) ? 4u : 1u);
    const dim3 grid((uint32_t)((total + 255) / 256));
#define GS_GRADE_LAUNCH(F) hipLaunchKernelGGL(gs_grade_kernel<F>, grid, dim3(256), 0, st, (float4*)s.geo, (float4*)s.sh, n, ids, m, x)
    switch (fl) {
    case 1u: GS_GRADE_LAUNCH(1u); break;
    case 2u: GS_GRADE_LAUNCH(2u); break;
    case 3u: GS_GRADE_LAUNCH(3u); break;
    case 4u: GS_GRADE_LAUNCH(4u); break;
    case 5u: GS_GRADE_LAUNCH(5u); break;
    case 6u: GS_GRADE_LAUNCH(6u); break;
    default: GS_GRADE_LAUNCH(7u); break;
    }
#undef GS_GRADE_LAUNCH
}
