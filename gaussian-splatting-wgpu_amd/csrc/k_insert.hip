// k_insert.hip -- the grow pass of the splat insertion (gs_insert.hip, gs_abi.h "splat insertion"): the old scene's planes and
// records into an allocation laid out for N + m splats, at the same indices, and the whole new state plane.  The reference has no
// counterpart: its host keeps the 320-byte records it uploaded (renderer.ts:130-137) and would concatenate and upload those.
//
// gs_compact's mirror image without the gather: old splat g IS new splat g, so every plane is a contiguous run.  The plane stride
// np = N rounded up to 64 changes with N, so every plane moves, but every base stays 256-byte aligned on both sides and the index
// is the same: the copy is 16 bytes per lane, lane i at base + 16 i, the widest coalesced access there is.
//   copy  : the items are the 16-byte units of px, py, pz, smax (N / 4 whole quads each), geo (2 N) and sh (12 N), numbered in that
//           order; a grid-stride loop takes four of them per trip, the four loads issued before the four stores.  244 B read and
//           written per resident splat.  Bound: HBM.
//   edges : one small launch.  Threads 0-15: the N mod 4 floats behind the last whole quad of each of the four planes, 4 bytes each
//           (a whole quad there would read floats the old scene does not hold).  Thread 16 + w: word w of the NEW state plane, all
//           np' / 4 of them: byte k is the old byte where 4 w + k < N, new_state where 4 w + k < N + m, else 0.  One thread owns the
//           whole word, the one that straddles N included, so no byte store races with a neighbour's (gs_compact_planes_kernel's
//           rule); the old plane is read by words too, which lie inside its own np >= N bytes.
// The tails -- what fills splats N .. N + m -- are the upload's own kernels with a destination offset: gs_repack_kernel and
// gs_ply_chunk_kernel (k_preprocess.hip), and gs_compact_planes_kernel's gather (k_export.hip) for a duplicate.
// No MFMA anywhere (no contraction).  Every store is a plain vector store.
#include <algorithm>

#include "gs_device.h"
#include "gs_kernels.h"

// Item i of the copy: where its 16 bytes come from and go to.  Q: whole quads per position plane; n: old splats.
struct GsGrowItem { const uint4* src; uint4* dst; };
__device__ __forceinline__ GsGrowItem grow_item(const GsScene& o, const GsScene& d, uint64_t i, uint64_t Q, uint64_t n) {
    const float* sp;
    const float* dp;
    if (i < Q) { sp = o.px; dp = d.px; }
    else if ((i -= Q) < Q) { sp = o.py; dp = d.py; }
    else if ((i -= Q) < Q) { sp = o.pz; dp = d.pz; }
    else if ((i -= Q) < Q) { sp = o.smax; dp = d.smax; }
    else if ((i -= Q) < 2 * n) { sp = (const float*)o.geo; dp = (const float*)d.geo; }
    else { i -= 2 * n; sp = (const float*)o.sh; dp = (const float*)d.sh; }
    return GsGrowItem{reinterpret_cast<const uint4*>(sp) + i, reinterpret_cast<uint4*>(const_cast<float*>(dp)) + i};
}

__global__ __launch_bounds__(256) void gs_grow_copy_kernel(GsScene o, GsScene d, uint32_t n_old, uint64_t total) {
    const uint64_t Q = n_old >> 2, n = n_old;
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256 + threadIdx.x; i0 < total; i0 += 4 * step) {
        GsGrowItem it[4];
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t i = i0 + (uint64_t)k * step;
            if (i < total) {
                it[k] = grow_item(o, d, i, Q, n);
                v[k] = *it[k].src;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + (uint64_t)k * step < total) *it[k].dst = v[k];
    }
}

__global__ __launch_bounds__(256) void gs_grow_edges_kernel(GsScene o, GsScene d, uint32_t n_old, uint32_t n_new, uint32_t new_state,
                                                             uint32_t state_words) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < 16u) {
        const uint32_t p = t >> 2, k = t & 3u;
        if (k >= (n_old & 3u)) return;
        const uint32_t g = (n_old & ~3u) + k; // < n_old
        const float* sp = p == 0u ? o.px : p == 1u ? o.py : p == 2u ? o.pz : o.smax;
        const float* dp = p == 0u ? d.px : p == 1u ? d.py : p == 2u ? d.pz : d.smax;
        const_cast<float*>(dp)[g] = sp[g];
        return;
    }
    const uint32_t w = t - 16u;
    if (w >= state_words) return; // (0 when the scenes keep no state plane)
    const uint64_t b0 = (uint64_t)w * 4u;
    const uint32_t old = b0 < n_old ? reinterpret_cast<const uint32_t*>(o.state)[w] : 0u; // (inside the old plane's np >= n_old bytes)
    uint32_t out = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t b = b0 + k;
        const uint32_t byte = b < n_old ? ((old >> (8u * k)) & 0xFFu) : b < n_new ? new_state : 0u;
        out |= byte << (8u * k);
    }
    reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(d.state))[w] = out;
}

void gs_launch_grow(const GsScene& o, uint32_t n_old, const GsScene& d, uint32_t n_new, uint32_t new_state, uint32_t grid, hipStream_t st) {
    const uint64_t total = 4 * (uint64_t)(n_old >> 2) + 14 * (uint64_t)n_old;
    if (total) {
        const uint64_t want = (total + 4 * 256 - 1) / (4 * 256); // four items per thread and trip
        const uint32_t blocks = (uint32_t)std::min<uint64_t>(want, grid ? grid : 2048u);
        hipLaunchKernelGGL(gs_grow_copy_kernel, dim3(blocks), dim3(256), 0, st, o, d, n_old, total);
    }
    const uint32_t state_words = d.state ? (uint32_t)((((uint64_t)n_new + 63) & ~(uint64_t)63) / 4) : 0u;
    hipLaunchKernelGGL(gs_grow_edges_kernel, dim3((16u + state_words + 255u) / 256u), dim3(256), 0, st, o, d, n_old, n_new, new_state & 0xFFu,
                       state_words);
}
