// gs_neigh_dev.h -- device code that every consumer of the cell grid shares (k_neigh.hip, k_cluster.hip, k_knn.hip, k_surface.hip):
// the walk over the source records of the 27 cells around a cell -- neigh_run, one x-run's spans, and neigh_visit, the wave's walk
// over the nine runs (the geometry is argued in k_neigh.hip) --, and the state pass around a membership read from a resident plane.
#pragma once
#include <type_traits>

#include "gs_device.h"
#include "gs_kernels.h" // NeighSources
#include "gs_state_sum.h"

// (neigh_finite, neigh_cell and neigh_key are gs_grid_math.h's, which gs_kernels.h includes: the cell merge's host twin compiles them too)

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

// THE WALK SKELETON of a query kernel (k_neigh.hip, "query", argues the geometry and the two paths).  A wave holds 64 consecutive
// cell-sorted queries; q is the lane's record (zeros without one).  in: the lane has a record; live: it takes part (in, and whatever
// else the kernel asks of its record: the clusters' id bound).  When every record of the wave is in one cell the nine x-runs' spans
// are wave-uniform: walk(std::true_type, lo, hi) with lo / hi out of SGPRs, called in EVERY lane -- the span walk masks by live
// itself.  Otherwise each live lane walks its own spans: walk(std::false_type, lo, hi).  The tag is a type, so that a kernel selects
// its span walk at compile time.
// GUARD: a wave without a record (the last workgroup's tail) walks nothing.  Its dead lanes sit in the cell of the origin, which
// may be the scene's densest, and they pass the uniform test; a kernel whose uniform span walk does not end by itself (nearest
// neighbours) asks for the guard.  The count's walk ends at its first ballot, and the clusters' edge pass never had the guard: both
// are compiled without it, instruction for instruction as before there was one skeleton (with it both streams change and would have
// to be timed on both paths).  The surface kernel alone keeps this skeleton written out, guard included: through this function its
// uniform path misses the timing rule.  profiles/grid_walks_refactor.txt has the streams, the spellings tried and the timings.
template <bool GUARD, class Walk>
__device__ __forceinline__ void neigh_visit(const NeighSources& S, const GsNeighGrid& g, const float4& q, bool in, bool live, Walk&& walk) {
    const int cx = neigh_cell(q.x, g.lo[0], g.inv_h, g.g[0]), cy = neigh_cell(q.y, g.lo[1], g.inv_h, g.g[1]), cz = neigh_cell(q.z, g.lo[2], g.inv_h, g.g[2]);
    const uint32_t key = ((uint32_t)cz << g.bxy) | ((uint32_t)cy << g.bx) | (uint32_t)cx;
    // the first lane's cell (lane 0 has a record whenever any lane has: the queries of a wave are consecutive)
    const uint32_t key0 = __builtin_amdgcn_readfirstlane(key);
    const bool uniform = __builtin_amdgcn_ballot_w64(in && key != key0) == 0ull;
    const bool any = !GUARD || __builtin_amdgcn_ballot_w64(in) != 0ull;
    if (any && uniform) {
        const int ux = __builtin_amdgcn_readfirstlane(cx), uy = __builtin_amdgcn_readfirstlane(cy), uz = __builtin_amdgcn_readfirstlane(cz);
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                neigh_run(S, g, ux, uy + dy, uz + dz, [&](uint32_t lo, uint32_t hi) {
                    walk(std::true_type{}, __builtin_amdgcn_readfirstlane(lo), __builtin_amdgcn_readfirstlane(hi));
                });
    } else if (live) {
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy) neigh_run(S, g, cx, cy + dy, cz + dz, [&](uint32_t lo, uint32_t hi) { walk(std::false_type{}, lo, hi); });
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
