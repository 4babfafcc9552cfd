// gs_neigh_dev.h -- device code that k_neigh.hip (neighbourhoods) and k_cluster.hip (clusters) share: the cell expression, the walk
// over the source records of the 27 cells around a cell (the geometry is argued in k_neigh.hip), and the state pass around a
// membership read from a resident u32 plane.
#pragma once
#include "gs_device.h"
#include "gs_kernels.h"
#include "gs_state_sum.h"

// (neigh_finite, neigh_cell and neigh_key are gs_grid_math.h's, which gs_kernels.h includes: the cell merge's host twin compiles them too)

// What the candidates kernel, the query pass and the clusters' edge pass read of the sources.  nrec bounds what a table entry may
// name (it never names more: gs_neigh_records_kernel).
struct NeighSources {
    const float4* __restrict__ rec;
    const uint32_t* __restrict__ keys;
    const uint2* __restrict__ table;
    uint32_t nrec;
};
// The spans of source records of the x-run around cell x of row (y, z): cells max(x - 1, 0) .. min(x + 1, Gx - 1), consecutive
// keys k0 .. k1, in every block they touch (one or two; three when a block is a cell).  f(lo, hi) takes each non-empty span.
template <class F>
__device__ __forceinline__ void neigh_run(const NeighSources& S, const GsNeighGrid& g, int x, int y, int z, F&& f) {
    if (y < 0 || y >= (int)g.g[1] || z < 0 || z >= (int)g.g[2]) return;
    const uint32_t base = ((uint32_t)z << g.bxy) | ((uint32_t)y << g.bx);
    const uint32_t k0 = base + (uint32_t)(x > 0 ? x - 1 : 0), k1 = base + (uint32_t)(x + 1 < (int)g.g[0] ? x + 1 : (int)g.g[0] - 1);
    for (uint32_t p = k0 >> g.shift; p <= (k1 >> g.shift) && p < g.blocks; ++p) {
        uint2 e = S.table[p]; // an empty block holds {0, 0}
        if (e.y > S.nrec) e.y = S.nrec;
        if (e.x >= e.y) continue;
        uint32_t lo = e.x, hi = e.y;
        if (g.shift) { // the first key >= k0 and the first key > k1 of the block: each search halves [a, b)
            uint32_t a = e.x, b = e.y;
            while (a < b) { const uint32_t m = (a + b) >> 1; if (S.keys[m] < k0) a = m + 1u; else b = m; }
            lo = a;
            b = e.y;
            while (a < b) { const uint32_t m = (a + b) >> 1; if (S.keys[m] <= k1) a = m + 1u; else b = m; }
            hi = a;
        }
        if (lo < hi) f(lo, hi);
    }
}

// The state pass (k_state.hip) around a resident u32 plane, 5 B read per splat -- the state word and one uint4 of the plane: a thread
// takes splats 4q .. 4q+3, one whole word of the state plane.  member(v): whether a splat whose plane value is v is in.
template <class Member>
__device__ __forceinline__ void state_plane_pass(uint8_t* __restrict__ state, const uint32_t* __restrict__ plane, uint32_t n, const Member& member, uint32_t op,
                                                 uint32_t bits, uint32_t wmask, uint32_t wvalue, unsigned long long* __restrict__ matched) {
    state_block_begin();
    const uint32_t q = blockIdx.x * 256u + threadIdx.x; // splats 4q .. 4q+3
    const uint64_t first = (uint64_t)q * 4u;
    uint32_t hits = 0;
    if (first + 4u <= n) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(state)[q];
        const uint4 c4 = reinterpret_cast<const uint4*>(plane)[q];
        const uint32_t C[4] = {c4.x, c4.y, c4.z, c4.w};
        uint32_t nw = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t sv = (w >> (8 * k)) & 0xFFu;
            const bool in = ((sv & wmask) == wvalue) && member(C[k]);
            hits += in ? 1u : 0u;
            nw |= (in ? gs_state_apply(sv, op, bits) : sv) << (8 * k);
        }
        if (nw != w) reinterpret_cast<uint32_t*>(state)[q] = nw; // stored only if it changed
    } else if (first < n) {
        for (uint64_t i = first; i < n; ++i) {
            const uint32_t sv = state[i];
            const bool in = ((sv & wmask) == wvalue) && member(plane[i]);
            hits += in ? 1u : 0u;
            const uint32_t nv = in ? gs_state_apply(sv, op, bits) : sv;
            if (nv != sv) state[i] = (uint8_t)nv;
        }
    }
    state_block_add(hits, matched);
}
inline uint32_t state_plane_blocks(uint32_t n) { return ((n + 3u) / 4u + 255u) / 256u; }
