// k_consensus.hip -- the consensus kernel: how many resident splats that pass a state filter have their GS_ATTR_PLANE / GS_ATTR_DIST2
// value inside [lo, hi], for EACH of h hypotheses (a plane or a centre each) in one pass over the positions (gs_consensus.hip; gs_abi.h
// "consensus").  The scoring loop of a RANSAC.  The reference has no counterpart: it is a viewer.
//
// gs_attr_histogram_kernel's shape (k_attr.hip): a persistent grid strides over the quads, thread q owns whole quads (gs_state_quad for
// the state bytes, one float4 per position plane; a partial last quad goes splat by splat: nothing at or past N is read), a workgroup
// counts into LDS and adds its non-zero words to the u64 result when its loop ends.  What differs:
//   lanes      : the SPLATS.  A lane keeps GS_CONSENSUS_R quads = 4 R splats of a trip in registers (12 R VGPRs).  A splat that fails the
//                filter or lies beyond N has x = NaN: its value is a NaN under either expression, a NaN is in no range, so it is never
//                counted and the loop below needs no exec mask of its own.
//   hypotheses : wave-UNIFORM.  The table f32[hp][4] is read with an index made of kernel arguments and loop counters only, so the
//                parameters arrive by scalar loads (s_load_dwordx4, checked in the .s: GS_CONSENSUS_PAD of them are issued together, the
//                loop is unrolled that far and the table padded to it with NaNs) and live in SGPRs.  Per hypothesis and splat: the value
//                by attr_of_pos<KIND> (gs_consensus_host.h: the ONE copy, which gs_consensus_host runs too), two compares, a ballot;
//                the ballots' popcounts add up in an SGPR.
//   counting   : the wave's count of hypothesis j goes to lane j % 64 of one VGPR (a compare and a select); after 64 hypotheses every lane
//                adds its word to s_count[j] with ONE LDS atomic.  A wave none of whose splats passes skips the loop (a uniform branch on a ballot).
//                The workgroup adds its non-zero words to the u64 counts in global memory when its trips are done; `matched` goes the
//                way of state_block_add (gs_state_sum.h).
// Integer adds only: the counts do not depend on the grid, R, the order, slabs or borrowers.  VALU bound (about 8 VALU instructions per
// hypothesis and 64 splats); the positions are read once, 12 B per splat.  No MFMA (nothing contracts).  Plain C++ and vector atomics only.
#include <algorithm>

#include "gs_device.h"
#include "gs_kernels.h"
#include "gs_state_sum.h"
#include "gs_consensus_host.h"

#define GS_CONSENSUS_R 2u // quads per lane and trip
static_assert(GS_CONSENSUS_MAX % 64u == 0u && 64u % GS_CONSENSUS_PAD == 0u, "whole groups of 64 hypotheses, whole batches within a group");

template <int KIND>
__global__ __launch_bounds__(256) void gs_consensus_kernel(const uint8_t* __restrict__ state, const float* __restrict__ px, const float* __restrict__ py,
                                                            const float* __restrict__ pz, uint32_t n, const float4* __restrict__ params, uint32_t hp,
                                                            float lo, float hi, uint32_t mask, uint32_t value, unsigned long long* __restrict__ counts,
                                                            unsigned long long* __restrict__ slots) {
    constexpr uint32_t R = GS_CONSENSUS_R, V = 4u * R;
    __shared__ uint32_t s_count[GS_CONSENSUS_MAX];
    for (uint32_t i = threadIdx.x; i < hp; i += 256u) s_count[i] = 0u; // (hp <= GS_CONSENSUS_MAX: the launcher's guard)
    state_block_begin();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t quads = (uint32_t)(((uint64_t)n + 3u) / 4u);
    const float nan = __builtin_nanf("");
    uint32_t hits = 0u;
    for (uint64_t base = (uint64_t)blockIdx.x * (256u * R); base < quads; base += (uint64_t)gridDim.x * (256u * R)) { // (uniform per workgroup)
        float x[V], y[V], z[V];
        bool any = false;
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) {
            const uint64_t q64 = base + r * 256u + threadIdx.x;
            const uint32_t q = q64 < quads ? (uint32_t)q64 : quads; // (quad `quads` starts at or past N: valid = 0)
            const GsStateQuad sq = gs_state_quad(state, n, q);
            float4 tx = {0.0f, 0.0f, 0.0f, 0.0f}, ty = tx, tz = tx;
            if (sq.valid == 4u) { // a whole quad: one float4 per plane; a partial one goes splat by splat
                tx = reinterpret_cast<const float4*>(px)[q]; ty = reinterpret_cast<const float4*>(py)[q]; tz = reinterpret_cast<const float4*>(pz)[q];
            } else if (sq.valid) {
                const uint64_t first = (uint64_t)q * 4u;
                tx.x = px[first]; ty.x = py[first]; tz.x = pz[first];
                if (sq.valid > 1u) { tx.y = px[first + 1u]; ty.y = py[first + 1u]; tz.y = pz[first + 1u]; }
                if (sq.valid > 2u) { tx.z = px[first + 2u]; ty.z = py[first + 2u]; tz.z = pz[first + 2u]; }
            }
            const float vx[4] = {tx.x, tx.y, tx.z, tx.w}, vy[4] = {ty.x, ty.y, ty.z, ty.w}, vz[4] = {tz.x, tz.y, tz.z, tz.w};
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                const bool in = k < sq.valid && (((sq.w >> (8u * k)) & 0xFFu) & mask) == value;
                hits += in ? 1u : 0u;
                any |= in;
                x[4u * r + k] = in ? vx[k] : nan;
                y[4u * r + k] = vy[k];
                z[4u * r + k] = vz[k];
            }
        }
        if (__builtin_amdgcn_ballot_w64(any) == 0ull) continue; // no splat of this wave passes: every count it would add is 0
        for (uint32_t jb = 0; jb < hp; jb += 64u) { // (uniform: hp is a kernel argument)
            const uint32_t lim = hp - jb < 64u ? hp - jb : 64u; // a multiple of GS_CONSENSUS_PAD
            uint32_t acc = 0u;                                  // lane l: the wave's count of hypothesis jb + l
            for (uint32_t jj = 0; jj < lim; jj += GS_CONSENSUS_PAD) {
#pragma unroll
                for (uint32_t u = 0; u < GS_CONSENSUS_PAD; ++u) {
                    const float4 p = params[jb + jj + u];
                    const GsAttrDev a = {{p.x, p.y, p.z, p.w}};
                    uint32_t cnt = 0u;
#pragma unroll
                    for (uint32_t i = 0; i < V; ++i) {
                        const float v = attr_of_pos<KIND>(a, x[i], y[i], z[i]);
                        cnt += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(v >= lo && v <= hi));
                    }
                    acc = lane == jj + u ? cnt : acc;
                }
            }
            if (acc) atomicAdd(&s_count[jb + lane], acc); // (a lane at or past lim holds 0; jb + lane < GS_CONSENSUS_MAX)
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < hp; i += 256u) {
        const uint32_t c = s_count[i];
        if (c) atomicAdd(counts + i, (unsigned long long)c);
    }
    state_block_add(hits, slots);
}

void gs_launch_consensus(uint32_t kind, const uint8_t* state, const float* px, const float* py, const float* pz, uint32_t n, const float* params,
                         uint32_t hp, float lo, float hi, uint32_t mask, uint32_t value, unsigned long long* counts, unsigned long long* slots,
                         uint32_t grid, hipStream_t st) {
    if (!n || !hp || hp > GS_CONSENSUS_MAX || hp % GS_CONSENSUS_PAD) return;
    const uint32_t work = (uint32_t)((((uint64_t)n + 3u) / 4u + 256u * GS_CONSENSUS_R - 1u) / (256u * GS_CONSENSUS_R));
    const uint32_t blocks = std::min(std::max(grid, 1u), work);
    const float4* p4 = reinterpret_cast<const float4*>(params);
    if (kind == GS_ATTR_DIST2)
        hipLaunchKernelGGL(gs_consensus_kernel<GS_ATTR_DIST2>, dim3(blocks), dim3(256), 0, st, state, px, py, pz, n, p4, hp, lo, hi, mask, value, counts, slots);
    else if (kind == GS_ATTR_PLANE)
        hipLaunchKernelGGL(gs_consensus_kernel<GS_ATTR_PLANE>, dim3(blocks), dim3(256), 0, st, state, px, py, pz, n, p4, hp, lo, hi, mask, value, counts, slots);
}
