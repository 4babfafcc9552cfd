// k_moments.hip -- the moments' kernel: exact sums and sums of products of up to three f32 planes over the resident splats that pass
// a state filter (gs_moments.hip; gs_abi.h "moments").  The reference has no counterpart: it is a viewer.
//
// One kernel, templated on the number of planes K in {1, 2, 3}, not on the attribute kind: POS_X / Y / Z are the scene's own planes,
// every other kind is materialised densely by gs_launch_attr_values first.  Bytes per splat: 4 K of planes and 1 of state when a
// filter other than (0, 0) is given.  Q = K + K (K + 1) / 2 quantities (9 for K = 3), each a table of GS_EX_LIMBS signed 64-bit limbs
// (gs_exact_sum.h: the split is written there, once).  Integer adds only, so the result does not depend on the grid, on the order
// or on who adds what where.
//   thread    : quad q of the persistent grid's stride (gs_state_quad's mapping, one float4 per plane).  Per quantity it keeps ONE
//               128-bit two's complement accumulator in registers, in units of its limb `base`, across its four splats and across
//               its trips: a term whose limb L is base or base + 1 is negated if need be, shifted by p - 32 base < 64 and added
//               with one carry chain, no memory access.  Real scenes concentrate their exponents, so that is nearly every term.
//               Any other L first flushes the lane's four 32-bit words (the top one signed) to the workgroup's LDS table with
//               64-bit LDS atomics and rebases to L: exact for any exponents, slow for adversarial ones only.  A flush adds less
//               than 2^32 to a limb and follows at least one term, so the limbs keep the bound of gs_exact_sum.h.
//   wave      : when the loop ends, the lanes that share a base are added across the wave on DPP (one round per distinct base, as
//               a rule one) and one lane adds the four words' sums to LDS.
//   workgroup : adds its non-zero LDS limbs to one of GS_MOMENTS_SLOTS copies in global memory (64-bit integer atomicAdd), spread as
//               the GS_STATE_SLOTS records are; the host adds the copies and runs the finish.
// Bound: the 64-bit integer VALU work (a product, a negation, two 64-bit shifts and a 128-bit add per quantity): 62 us for (X, Y, Z)
// of 6.1 M splats where the planes' HBM time is 18 (profiles/moments.txt).  No MFMA (no contraction the matrix cores could take: the terms are exact
// 48-bit integers).  Plain C++ and vector atomics only.
#include <algorithm>

#include "gs_device.h"
#include "gs_kernels.h"
#include "gs_exact_dev.h" // MoAcc, mo_add, mo_flush, mo_fold: shared with k_pairs.hip

#define GS_MO_QUANTITIES(K) ((K) + (K) * ((K) + 1) / 2)
// the table of a workgroup and of a slot: Q x GS_EX_LIMBS limbs, then matched, counted
#define GS_MO_WORDS(K) (GS_MO_QUANTITIES(K) * GS_EX_LIMBS + 2u)

template <int K>
__global__ __launch_bounds__(256) void gs_moments_kernel(const uint8_t* __restrict__ state, const float* __restrict__ p0, const float* __restrict__ p1,
                                                          const float* __restrict__ p2, uint32_t n, uint32_t mask, uint32_t value,
                                                          mo_u64* __restrict__ slots) {
    constexpr int Q = GS_MO_QUANTITIES(K);
    constexpr uint32_t W = GS_MO_WORDS(K);
    __shared__ mo_u64 s_tab[W];
    for (uint32_t i = threadIdx.x; i < W; i += 256u) s_tab[i] = 0ull;
    __syncthreads();
    const float* const plane[3] = {p0, p1, p2};
    MoAcc acc[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) { acc[j].a = 0; acc[j].base = GS_MO_EMPTY; }
    uint32_t matched = 0u, counted = 0u;
    const uint32_t quads = (uint32_t)(((uint64_t)n + 3u) / 4u);
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < quads; base += (uint64_t)gridDim.x * 256u) { // (uniform per workgroup)
        const uint32_t q = (uint32_t)base + threadIdx.x;
        const GsStateQuad sq = gs_state_quad(state, n, q); // valid = 0 beyond the last quad
        uint32_t v[K][4];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0u;
            if (sq.valid == 4u) { // a whole quad: one float4 per plane; a partial one goes splat by splat, nothing past N is read
                const float4 t = reinterpret_cast<const float4*>(plane[j])[q];
                v[j][0] = __float_as_uint(t.x); v[j][1] = __float_as_uint(t.y); v[j][2] = __float_as_uint(t.z); v[j][3] = __float_as_uint(t.w);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k)
                    if (k < sq.valid) v[j][k] = __float_as_uint(plane[j][(uint64_t)q * 4u + k]);
            }
        }
        // the quad's four splats in turn, NOT unrolled: nine terms a splat are code enough (the next splat's values move down)
        uint32_t w = sq.w;
#pragma unroll 1
        for (uint32_t k = 0; k < 4u; ++k) {
            const bool in = k < sq.valid && ((w & 0xFFu) & mask) == value;
            uint32_t c[K];
            bool fin = true;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                c[j] = v[j][0];
                v[j][0] = v[j][1]; v[j][1] = v[j][2]; v[j][2] = v[j][3];
                fin = fin && ex_finite(c[j]);
            }
            w >>= 8;
            matched += in ? 1u : 0u;
            if (!(in && fin)) continue;
            ++counted;
            uint32_t m[K], e[K];
#pragma unroll
            for (int j = 0; j < K; ++j) { m[j] = ex_mant(c[j]); e[j] = ex_expo(c[j]); }
#pragma unroll
            for (int j = 0; j < K; ++j) // the sums: quantities 0 .. K
                mo_add(acc[j], s_tab + j * GS_EX_LIMBS, m[j], e[j] + (uint32_t)(GS_EX_BIAS - 150), (c[j] >> 31) != 0u);
#pragma unroll
            for (int j = 0; j < K; ++j) // the products, j <= l in gs_abi.h's order
#pragma unroll
                for (int l = j; l < K; ++l) {
                    const int t = K + j * (2 * K - j + 1) / 2 + (l - j); // (a constant once unrolled)
                    mo_add(acc[t], s_tab + t * GS_EX_LIMBS, (uint64_t)m[j] * m[l], e[j] + e[l] - (uint32_t)(300 - GS_EX_BIAS),
                           ((c[j] ^ c[l]) >> 31) != 0u);
                }
        }
    }
    // converged again: per wave, then the workgroup's table, then one copy of the slots
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int j = 0; j < Q; ++j) mo_fold(acc[j], s_tab + j * GS_EX_LIMBS, lane);
    const uint32_t wm = wave_sum(matched), wc = wave_sum(counted);
    if (lane == 0u && wm) {
        atomicAdd(&s_tab[W - 2u], (mo_u64)wm);
        if (wc) atomicAdd(&s_tab[W - 1u], (mo_u64)wc);
    }
    __syncthreads();
    mo_u64* slot = slots + (size_t)(blockIdx.x % GS_MOMENTS_SLOTS) * GS_MOMENTS_SLOT_WORDS;
    for (uint32_t i = threadIdx.x; i < W; i += 256u) {
        const mo_u64 w = s_tab[i];
        if (w) atomicAdd(slot + i, w);
    }
}

void gs_launch_moments(uint32_t planes, const uint8_t* state, const float* p0, const float* p1, const float* p2, uint32_t n, uint32_t mask,
                       uint32_t value, unsigned long long* slots, uint32_t grid, hipStream_t st) {
    if (!n) return;
    const uint32_t work = (uint32_t)((((uint64_t)n + 3u) / 4u + 255u) / 256u);
    // clamped to the work, and from below so that no thread makes more than GS_MO_MAX_TRIPS trips (a lane's 128-bit accumulators)
    const uint32_t least = (work + GS_MO_MAX_TRIPS - 1u) / GS_MO_MAX_TRIPS;
    const uint32_t blocks = std::max(least, std::min(std::max(grid, 1u), work));
    if (planes == 1u) hipLaunchKernelGGL(gs_moments_kernel<1>, dim3(blocks), dim3(256), 0, st, state, p0, p0, p0, n, mask, value, slots);
    else if (planes == 2u) hipLaunchKernelGGL(gs_moments_kernel<2>, dim3(blocks), dim3(256), 0, st, state, p0, p1, p1, n, mask, value, slots);
    else hipLaunchKernelGGL(gs_moments_kernel<3>, dim3(blocks), dim3(256), 0, st, state, p0, p1, p2, n, mask, value, slots);
}
