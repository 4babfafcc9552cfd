// k_pairs.hip -- the pair moments' kernel: the exact sums a rigid or similarity fit needs over the matched PAIRS (p_i, q_i = p_j,
// j = partner[i]) of the resident splats that pass a state filter (gs_pairs.hip; gs_abi.h "registration").  The reference has no
// counterpart: it is a viewer.
//
// gs_moments_kernel's shape (k_moments.hip) with a gather: a persistent grid, gs_state_quad for the state bytes, one float4 per
// position plane and one uint4 of partner ids per quad; a partial last quad goes splat by splat.  Bytes per splat: 12 of position, 4
// of partner, 1 of state with a filter other than (0, 0), and 12 scattered bytes of px / py / pz[j] for the splats that pass so far
// (the filter, j < N, p finite): an id at or above N -- GS_KNN_NONE among them -- is never used as an index, and nothing at or past N
// is read in the stream either.  The four gathers of a quad are issued together, before the first term is added.
//   quantities: 21, each a table of GS_EX_LIMBS signed 64-bit limbs in gs_pair_host.h's order: sum_p[3], sum_q[3], pq[9], pp[3],
//               qq[3].  A pair counts when pair_accept (gs_pair_host.h: the one copy the host loop runs too) holds.
//   thread    : ONE 128-bit accumulator and base per quantity, all 21 in registers across its splats and trips (gs_exact_dev.h:
//               mo_add; a foreign exponent flushes to LDS and rebases).  The compiler's resource report for gfx950: 158 VGPRs,
//               no AGPRs, no scratch, no spill, 3 waves per SIMD -- so pp / qq did not have to go through the LDS table directly.
//   wave      : mo_fold on DPP, one lane adds the sums to LDS.
//   workgroup : its non-zero limbs to one of GS_PAIRS_SLOTS copies in global memory with 64-bit integer vector atomics; the host
//               adds the copies and runs the finish ONCE per quantity.
// Integer adds only: the result does not depend on the grid, the order, slabs or borrowers.  Plain C++ and vector atomics only.
#include <algorithm>

#include "gs_device.h"
#include "gs_kernels.h"
#include "gs_exact_dev.h"
#include "gs_pair_host.h"

#define GS_PAIRS_WORDS (GS_PAIR_QUANTITIES * GS_EX_LIMBS + 2u) // a workgroup's table: the limbs, then matched, paired
static_assert(GS_PAIRS_SLOT_WORDS >= GS_PAIRS_WORDS, "a slot copy holds 21 limb tables and the two counts");

__global__ __launch_bounds__(256) void gs_pairs_kernel(const uint8_t* __restrict__ state, const float* __restrict__ px, const float* __restrict__ py,
                                                        const float* __restrict__ pz, const uint32_t* __restrict__ partner, uint32_t n, uint32_t mask,
                                                        uint32_t value, float max_d2, mo_u64* __restrict__ slots) {
    constexpr int Q = (int)GS_PAIR_QUANTITIES;
    constexpr uint32_t W = GS_PAIRS_WORDS;
    __shared__ mo_u64 s_tab[W];
    for (uint32_t i = threadIdx.x; i < W; i += 256u) s_tab[i] = 0ull;
    __syncthreads();
    const float* const plane[3] = {px, py, pz};
    MoAcc acc[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) { acc[j].a = 0; acc[j].base = GS_MO_EMPTY; }
    uint32_t matched = 0u, paired = 0u;
    const uint32_t quads = (uint32_t)(((uint64_t)n + 3u) / 4u);
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < quads; base += (uint64_t)gridDim.x * 256u) { // (uniform per workgroup)
        const uint32_t q = (uint32_t)base + threadIdx.x;
        const GsStateQuad sq = gs_state_quad(state, n, q); // valid = 0 beyond the last quad
        uint32_t pv[3][4], qv[3][4], jv[4];
        jv[0] = jv[1] = jv[2] = jv[3] = 0xFFFFFFFFu;
        if (sq.valid == 4u) { // a whole quad: one float4 per plane and one uint4 of ids; a partial one goes splat by splat
            const uint4 t = reinterpret_cast<const uint4*>(partner)[q];
            jv[0] = t.x; jv[1] = t.y; jv[2] = t.z; jv[3] = t.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k)
                if (k < sq.valid) jv[k] = partner[(uint64_t)q * 4u + k];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            pv[a][0] = pv[a][1] = pv[a][2] = pv[a][3] = 0u;
            if (sq.valid == 4u) {
                const float4 t = reinterpret_cast<const float4*>(plane[a])[q];
                pv[a][0] = __float_as_uint(t.x); pv[a][1] = __float_as_uint(t.y); pv[a][2] = __float_as_uint(t.z); pv[a][3] = __float_as_uint(t.w);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k)
                    if (k < sq.valid) pv[a][k] = __float_as_uint(plane[a][(uint64_t)q * 4u + k]);
            }
        }
        // who passes so far, and their gathers, all four in flight together: j < n is checked before j is an index
        uint32_t pass = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const bool in = k < sq.valid && (((sq.w >> (8u * k)) & 0xFFu) & mask) == value;
            matched += in ? 1u : 0u;
            const bool go = in && jv[k] < n && ex_finite(pv[0][k]) && ex_finite(pv[1][k]) && ex_finite(pv[2][k]);
            qv[0][k] = qv[1][k] = qv[2][k] = 0u;
            if (go) {
                pass |= 1u << k;
                qv[0][k] = __float_as_uint(px[jv[k]]);
                qv[1][k] = __float_as_uint(py[jv[k]]);
                qv[2][k] = __float_as_uint(pz[jv[k]]);
            }
        }
        // the quad's four splats in turn, NOT unrolled: 21 terms a splat are code enough (the next splat's values move down)
#pragma unroll 1
        for (uint32_t k = 0; k < 4u; ++k) {
            uint32_t p[3], t[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                p[a] = pv[a][0]; pv[a][0] = pv[a][1]; pv[a][1] = pv[a][2]; pv[a][2] = pv[a][3];
                t[a] = qv[a][0]; qv[a][0] = qv[a][1]; qv[a][1] = qv[a][2]; qv[a][2] = qv[a][3];
            }
            const bool go = (pass & 1u) != 0u;
            pass >>= 1;
            if (!(go && pair_accept(p, t, max_d2))) continue;
            ++paired;
            uint32_t mp[3], ep[3], mq[3], eq[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) { mp[a] = ex_mant(p[a]); ep[a] = ex_expo(p[a]); mq[a] = ex_mant(t[a]); eq[a] = ex_expo(t[a]); }
            constexpr uint32_t kOne = (uint32_t)(GS_EX_BIAS - 150), kTwo = (uint32_t)(300 - GS_EX_BIAS);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                mo_add(acc[GS_PAIR_SUM_P + a], s_tab + (GS_PAIR_SUM_P + a) * GS_EX_LIMBS, mp[a], ep[a] + kOne, (p[a] >> 31) != 0u);
                mo_add(acc[GS_PAIR_SUM_Q + a], s_tab + (GS_PAIR_SUM_Q + a) * GS_EX_LIMBS, mq[a], eq[a] + kOne, (t[a] >> 31) != 0u);
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    mo_add(acc[GS_PAIR_PQ + 3 * a + b], s_tab + (GS_PAIR_PQ + 3 * a + b) * GS_EX_LIMBS, (uint64_t)mp[a] * mq[b], ep[a] + eq[b] - kTwo,
                           ((p[a] ^ t[b]) >> 31) != 0u);
                mo_add(acc[GS_PAIR_PP + a], s_tab + (GS_PAIR_PP + a) * GS_EX_LIMBS, (uint64_t)mp[a] * mp[a], ep[a] + ep[a] - kTwo, false);
                mo_add(acc[GS_PAIR_QQ + a], s_tab + (GS_PAIR_QQ + a) * GS_EX_LIMBS, (uint64_t)mq[a] * mq[a], eq[a] + eq[a] - kTwo, false);
            }
        }
    }
    // converged again: per wave, then the workgroup's table, then one copy of the slots
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int j = 0; j < Q; ++j) mo_fold(acc[j], s_tab + j * GS_EX_LIMBS, lane);
    const uint32_t wm = wave_sum(matched), wp = wave_sum(paired);
    if (lane == 0u && wm) {
        atomicAdd(&s_tab[W - 2u], (mo_u64)wm);
        if (wp) atomicAdd(&s_tab[W - 1u], (mo_u64)wp);
    }
    __syncthreads();
    mo_u64* slot = slots + (size_t)(blockIdx.x % GS_PAIRS_SLOTS) * GS_PAIRS_SLOT_WORDS;
    for (uint32_t i = threadIdx.x; i < W; i += 256u) {
        const mo_u64 w = s_tab[i];
        if (w) atomicAdd(slot + i, w);
    }
}

void gs_launch_pairs(const uint8_t* state, const float* px, const float* py, const float* pz, const uint32_t* partner, uint32_t n, uint32_t mask,
                     uint32_t value, float max_d2, unsigned long long* slots, uint32_t grid, hipStream_t st) {
    if (!n) return;
    const uint32_t work = (uint32_t)((((uint64_t)n + 3u) / 4u + 255u) / 256u);
    // clamped to the work, and from below so that no thread makes more than GS_MO_MAX_TRIPS trips (a lane's 128-bit accumulators)
    const uint32_t least = (work + GS_MO_MAX_TRIPS - 1u) / GS_MO_MAX_TRIPS;
    const uint32_t blocks = std::max(least, std::min(std::max(grid, 1u), work));
    hipLaunchKernelGGL(gs_pairs_kernel, dim3(blocks), dim3(256), 0, st, state, px, py, pz, partner, n, mask, value, max_d2, slots);
}
