// k_plane_pairs.hip -- the plane pair moments' kernel: the exact sums of the point-to-plane normal equations over the matched PAIRS
// (p_i, q_i = p_j, n_i = normal[j], j = partner[i]) of the resident splats that pass a state filter (gs_plane_pairs.hip; gs_abi.h
// "registration").  The reference has no counterpart: it is a viewer.
//
// gs_pairs_kernel's shape (k_pairs.hip) with one more gather: a persistent grid, gs_state_quad for the state bytes, one float4 per
// position plane and one uint4 of partner ids per quad; a partial last quad goes splat by splat.  Bytes per splat: 12 of position, 4
// of partner, 1 of state with a filter other than (0, 0), and for the splats that pass so far (the filter, j < N, p finite) 12
// scattered bytes of px / py / pz[j] and ONE 16-byte record {nx, ny, nz, any} of the normal plane: an id at or above N -- GS_KNN_NONE
// among them -- is never used as an index, and nothing at or past N is read in the stream either.  The eight gathers of a quad are
// issued together, before the first term is added.
//   quantities: 29, each a table of GS_EX_LIMBS signed 64-bit limbs in gs_plane_pair_host.h's order: G[21], h[6], rr, d2.  The row
//               and the acceptance are plane_row (gs_plane_pair_host.h: the one copy the host loop runs too).
//   thread    : ONE 128-bit accumulator and base per quantity, in registers across its splats and trips (gs_exact_dev.h: mo_add).
//               The kernel is a template over a range [LO, HI) of the quantities so that the 29 could be split over two launches
//               (integer adds: the same result); the compiler's resource report for gfx950 decides, and all 29 fit: <0, 29> has
//               214 VGPRs, no AGPRs, 88 SGPRs, no scratch, no spill, 4656 B of LDS, 2 waves per SIMD (gs_pairs_kernel: 158 VGPRs and
//               3 waves with 21).  One launch, one pass over the stream and the gathers.
//   wave      : mo_fold on DPP, one lane adds the sums to LDS.
//   workgroup : its non-zero limbs to one of GS_PLANE_PAIRS_SLOTS copies in global memory with 64-bit integer vector atomics; the
//               host adds the copies and runs the finish ONCE per quantity.  The instantiation with LO = 0 adds the two counts.
// Integer adds only: the result does not depend on the grid, the order, slabs or borrowers.  Plain C++ and vector atomics only.
#include <algorithm>

#include "gs_device.h"
#include "gs_kernels.h"
#include "gs_exact_dev.h"
#include "gs_plane_pair_host.h"

#define GS_PLANE_PAIRS_WORDS (GS_PLANE_QUANTITIES * GS_EX_LIMBS + 2u) // a slot copy: the limbs, then matched, paired
static_assert(GS_PLANE_PAIRS_SLOT_WORDS >= GS_PLANE_PAIRS_WORDS, "a slot copy holds 29 limb tables and the two counts");

template <int LO, int HI>
__global__ __launch_bounds__(256) void gs_plane_pairs_kernel(const uint8_t* __restrict__ state, const float* __restrict__ px, const float* __restrict__ py,
                                                              const float* __restrict__ pz, const uint32_t* __restrict__ partner,
                                                              const float4* __restrict__ normal, uint32_t n, uint32_t mask, uint32_t value, float pvx,
                                                              float pvy, float pvz, float max_d2, mo_u64* __restrict__ slots) {
    static_assert(0 <= LO && LO < HI && HI <= (int)GS_PLANE_QUANTITIES, "a range of the 29 quantities");
    constexpr int Q = HI - LO;
    constexpr uint32_t W = (uint32_t)Q * GS_EX_LIMBS + 2u; // this launch's tables, then matched, paired (added by LO = 0 only)
    __shared__ mo_u64 s_tab[W];
    for (uint32_t i = threadIdx.x; i < W; i += 256u) s_tab[i] = 0ull;
    __syncthreads();
    const float* const plane[3] = {px, py, pz};
    const float pivot[3] = {pvx, pvy, pvz};
    MoAcc acc[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) { acc[j].a = 0; acc[j].base = GS_MO_EMPTY; }
    uint32_t matched = 0u, paired = 0u;
    const uint32_t quads = (uint32_t)(((uint64_t)n + 3u) / 4u);
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < quads; base += (uint64_t)gridDim.x * 256u) { // (uniform per workgroup)
        const uint32_t q = (uint32_t)base + threadIdx.x;
        const GsStateQuad sq = gs_state_quad(state, n, q); // valid = 0 beyond the last quad
        uint32_t pv[3][4], qv[3][4], nv[3][4], jv[4];
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
        // who passes so far, and their gathers, all in flight together: j < n is checked before j is an index
        uint32_t pass = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const bool in = k < sq.valid && (((sq.w >> (8u * k)) & 0xFFu) & mask) == value;
            matched += in ? 1u : 0u;
            const bool go = in && jv[k] < n && ex_finite(pv[0][k]) && ex_finite(pv[1][k]) && ex_finite(pv[2][k]);
            qv[0][k] = qv[1][k] = qv[2][k] = 0u;
            nv[0][k] = nv[1][k] = nv[2][k] = 0u;
            if (go) {
                pass |= 1u << k;
                qv[0][k] = __float_as_uint(px[jv[k]]);
                qv[1][k] = __float_as_uint(py[jv[k]]);
                qv[2][k] = __float_as_uint(pz[jv[k]]);
                const float4 t = normal[jv[k]]; // one 16-byte gather
                nv[0][k] = __float_as_uint(t.x); nv[1][k] = __float_as_uint(t.y); nv[2][k] = __float_as_uint(t.z);
            }
        }
        // the quad's four splats in turn, NOT unrolled (the next splat's values move down)
#pragma unroll 1
        for (uint32_t k = 0; k < 4u; ++k) {
            uint32_t p[3], t[3], nb[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                p[a] = pv[a][0]; pv[a][0] = pv[a][1]; pv[a][1] = pv[a][2]; pv[a][2] = pv[a][3];
                t[a] = qv[a][0]; qv[a][0] = qv[a][1]; qv[a][1] = qv[a][2]; qv[a][2] = qv[a][3];
                nb[a] = nv[a][0]; nv[a][0] = nv[a][1]; nv[a][1] = nv[a][2]; nv[a][2] = nv[a][3];
            }
            const bool go = (pass & 1u) != 0u;
            pass >>= 1;
            float f[GS_PLANE_FACTORS], d2;
            if (!(go && plane_row(p, t, nb, pivot, max_d2, f, &d2))) continue;
            ++paired;
            uint32_t fb[GS_PLANE_FACTORS], m[GS_PLANE_FACTORS], e[GS_PLANE_FACTORS];
#pragma unroll
            for (int a = 0; a < (int)GS_PLANE_FACTORS; ++a) { fb[a] = __float_as_uint(f[a]); m[a] = ex_mant(fb[a]); e[a] = ex_expo(fb[a]); }
            constexpr uint32_t kOne = (uint32_t)(GS_EX_BIAS - 150), kTwo = (uint32_t)(300 - GS_EX_BIAS);
#pragma unroll
            for (int tq = LO; tq < HI; ++tq) {
                if (tq < (int)GS_PLANE_PRODUCTS) {
                    const uint32_t a = plane_fa((uint32_t)tq), b = plane_fb((uint32_t)tq);
                    mo_add(acc[tq - LO], s_tab + (tq - LO) * GS_EX_LIMBS, (uint64_t)m[a] * m[b], e[a] + e[b] - kTwo, ((fb[a] ^ fb[b]) >> 31) != 0u);
                } else { // d2: a single value, never negative
                    const uint32_t db = __float_as_uint(d2);
                    mo_add(acc[tq - LO], s_tab + (tq - LO) * GS_EX_LIMBS, ex_mant(db), ex_expo(db) + kOne, false);
                }
            }
        }
    }
    // converged again: per wave, then the workgroup's table, then one copy of the slots
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int j = 0; j < Q; ++j) mo_fold(acc[j], s_tab + j * GS_EX_LIMBS, lane);
    if (LO == 0) {
        const uint32_t wm = wave_sum(matched), wp = wave_sum(paired);
        if (lane == 0u && wm) {
            atomicAdd(&s_tab[W - 2u], (mo_u64)wm);
            if (wp) atomicAdd(&s_tab[W - 1u], (mo_u64)wp);
        }
    }
    __syncthreads();
    mo_u64* slot = slots + (size_t)(blockIdx.x % GS_PLANE_PAIRS_SLOTS) * GS_PLANE_PAIRS_SLOT_WORDS;
    for (uint32_t i = threadIdx.x; i < W; i += 256u) {
        const mo_u64 w = s_tab[i];
        // this launch's limbs sit at LO's tables of the slot copy, the counts behind all 29
        const uint32_t at = i < (uint32_t)Q * GS_EX_LIMBS ? (uint32_t)LO * GS_EX_LIMBS + i : GS_PLANE_QUANTITIES * GS_EX_LIMBS + (i - (uint32_t)Q * GS_EX_LIMBS);
        if (w) atomicAdd(slot + at, w);
    }
}

template <int LO, int HI>
static void plane_pairs_launch(uint32_t blocks, hipStream_t st, const uint8_t* state, const float* px, const float* py, const float* pz,
                               const uint32_t* partner, const float4* normal, uint32_t n, uint32_t mask, uint32_t value, float pvx, float pvy, float pvz,
                               float max_d2, mo_u64* slots) {
    hipLaunchKernelGGL((gs_plane_pairs_kernel<LO, HI>), dim3(blocks), dim3(256), 0, st, state, px, py, pz, partner, normal, n, mask, value, pvx, pvy,
                       pvz, max_d2, slots);
}

void gs_launch_plane_pairs(const uint8_t* state, const float* px, const float* py, const float* pz, const uint32_t* partner, const void* normal,
                           uint32_t n, uint32_t mask, uint32_t value, float pvx, float pvy, float pvz, float max_d2, unsigned long long* slots,
                           uint32_t grid, hipStream_t st) {
    if (!n) return;
    const uint32_t work = (uint32_t)((((uint64_t)n + 3u) / 4u + 255u) / 256u);
    // clamped to the work, and from below so that no thread makes more than GS_MO_MAX_TRIPS trips (a lane's 128-bit accumulators)
    const uint32_t least = (work + GS_MO_MAX_TRIPS - 1u) / GS_MO_MAX_TRIPS;
    const uint32_t blocks = std::max(least, std::min(std::max(grid, 1u), work));
    plane_pairs_launch<0, (int)GS_PLANE_QUANTITIES>(blocks, st, state, px, py, pz, partner, (const float4*)normal, n, mask, value, pvx, pvy, pvz, max_d2,
                                                    slots);
}
