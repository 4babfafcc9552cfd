// k_pick.hip -- gs_pick: per-pixel splat queries (front, dominant, median) on the last frame's lists.
//
// The reference has no picking; what a query returns is DEFINED by its blend, compute_tiles.wgsl:44-66, in the canonical (EXACT)
// arithmetic of gs_blend_kernel: one f32 rounding per written operation (the library is built with -ffp-contract=off), gs_exp,
// wg_min, the same cond and the same T update -- whatever blend the frame itself used.  No frame kernel is involved: the lists
// (values, ranges) and the GaussianData records of the last frame are still resident, and a query walks ONE tile's list for ONE
// pixel.
//
// One wave64 per query.  A tile list is hundreds to thousands of entries long and a pixel accepts tens of them, so the work is
// split the way the blend splits it:
//   parallel  per chunk of 64 entries, lane l loads values[start + 64 c + l] (coalesced), gathers the three pieces of the record
//             it needs (uv; conic + depth; opacity) and evaluates power and alpha; the next chunk's ids and records are fetched
//             before this chunk is resolved, so their latency is covered by the serial part;
//   serial    the ballot of `power <= 0 && alpha >= 1/255` is walked in list order, the candidate's alpha, depth and id come
//             from its lane with v_readlane, and test / cond / T and the first / max / median / contributor bookkeeping are
//             applied wave-uniformly.
// Entries that fail the ballot have cond = 0.  So does a candidate with test < 1e-4.  Such an entry changes nothing:
// alpha is in [0, 0.99] (wg_min returns 0.99 for a NaN product, and opacities are sigmoids), hence test is finite and
// T = 0 * test + 1 * T = T, D = D + 0 * z * alpha * T = D.  The blend kernels' block culls rest on the same fact.
#include "gs_kernels.h"

#define GS_PICK_NONE_ID 0xFFFFFFFFu

__global__ __launch_bounds__(64) void gs_pick_kernel(const uint4* __restrict__ gdata, const uint32_t* __restrict__ values,
                                                      const uint32_t* __restrict__ ranges, GsFrame f, uint32_t id_mask, uint32_t nrec,
                                                      const uint2* __restrict__ queries, uint32_t* __restrict__ results,
                                                      uint32_t max_contrib, uint2* __restrict__ contrib) {
    const uint32_t q = blockIdx.x, lane = lane_id();
    const uint2 xy = queries[q];
    uint2* const cq = contrib ? contrib + (uint64_t)q * max_contrib : nullptr;
    uint32_t status = 0u, list_length = 0u, hits = 0u;
    uint32_t first_id = GS_PICK_NONE_ID, max_id = GS_PICK_NONE_ID, median_id = GS_PICK_NONE_ID;
    float first_depth = 0.0f, max_w = 0.0f, median_depth = 0.0f;
    float T = 1.0f, D = 0.0f;
    // the slab's pixels, as the blend owns them (the host has rejected pixels outside the canvas)
    if (xy.x >= f.px0 && xy.x - f.px0 < f.slab_w && xy.y < f.height) {
        const uint32_t tile = xy.x / f.tile_size + (xy.y / f.tile_size) * f.ntx; // canvas tile index, as every blend kernel forms it
        const uint2 run = gs_tile_range(ranges, tile, f.capacity);
        const uint32_t start = run.x, end = run.y < start ? start : run.y;
        list_length = end - start;
        const float pxf = (float)xy.x, pyf = (float)xy.y;
        const float Wf = (float)f.width, Hf = (float)f.height;
        const float c255 = (float)(1.0 / 255.0);
        GsListRec cur = gs_list_fetch(gdata, values, start + lane, end, id_mask, 0u, nrec, f.n);
        bool settled = false;
        for (uint32_t b = start; b < end && !settled; b += 64u) {
            const GsListRec nxt = gs_list_fetch(gdata, values, b + 64u + lane, end, id_mask, 0u, nrec, f.n); // in flight while this chunk is resolved
            // compute_tiles.wgsl:52-59, the head of gs_blend_exact
            const float power = gs_blend_power(cur.cx, cur.cy, cur.cz, cur.ux * Wf - pxf, cur.uy * Hf - pyf);
            const float alpha = gs_blend_alpha(cur.op, power);
            unsigned long long m = __ballot(cur.live && power <= 0.0f && alpha >= c255);
            while (m) {
                const int l = __builtin_ctzll(m);
                m &= m - 1ull;
                const float a = gs_bcast(alpha, l);
                const float test = T * (1.0f - a);
                if (!(test >= 0.0001f)) continue; // cond = 0: nothing changes (see the head of the file); later entries may still be accepted
                const float z = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(cur.z), l)); // gs_bcast, written out: through it two register initialisations swap
                const uint32_t id = (uint32_t)__builtin_amdgcn_readlane((int)cur.id, l);
                const float w = a * T; // the entry's weight: T before the entry
                if (cq && hits < max_contrib && lane == 0u) cq[hits] = make_uint2(id, __float_as_uint(w));
                if (hits == 0u) { first_id = id; first_depth = z; }
                if (hits == 0u || w > max_w) { max_id = id; max_w = w; } // strictly larger: the earliest of equal weights stays
                D = D + z * a * T; // cond z alpha T, left to right, cond = 1
                T = test;          // cond test + (1 - cond) T with cond = 1: test + 0
                ++hits;
                if (median_id == GS_PICK_NONE_ID && T <= 0.5f) { median_id = id; median_depth = z; }
                // The blend kernels' exit.  Every later candidate has alpha >= c255, so fl(1 - alpha) <= fl(1 - c255) and
                // fl(T fl(1 - alpha)) <= fl(T fl(1 - c255)) (rounding is monotonic, T > 0): once the right-hand side is below 1e-4
                // no later entry can be accepted, T never changes again, and no field of the result depends on a rejected entry.
                if (gs_pixel_final<true>(T)) { settled = true; break; }
            }
            cur = nxt;
        }
    } else {
        status = 1u; // GS_PICK_OUTSIDE_SLAB: every other field 0 / NONE
    }
    if (cq) // the slots no accepted entry filled
        for (uint32_t k = (hits < max_contrib ? hits : max_contrib) + lane; k < max_contrib; k += 64u) cq[k] = make_uint2(GS_PICK_NONE_ID, 0u);
    // gs_pick_result: 12 words, one per lane (vector stores)
    if (lane < 12u) {
        uint32_t v = 0u;
        switch (lane) {
        case 0: v = status; break;
        case 1: v = list_length; break;
        case 2: v = hits; break;
        case 3: v = first_id; break;
        case 4: v = __float_as_uint(first_depth); break;
        case 5: v = max_id; break;
        case 6: v = __float_as_uint(max_w); break;
        case 7: v = median_id; break;
        case 8: v = __float_as_uint(median_depth); break;
        case 9: v = __float_as_uint(1.0f - T); break;
        case 10: v = __float_as_uint(D); break;
        default: v = 0u; break;
        }
        results[(uint64_t)q * 12 + lane] = v;
    }
}

void gs_launch_pick(const GsLists& L, const void* d_queries, uint32_t n, void* d_results, uint32_t max_contrib, void* d_contrib, hipStream_t st) {
    if (!n) return;
    gs_pick_kernel<<<n, 64, 0, st>>>((const uint4*)L.gdata, L.values, L.ranges, L.f, L.id_mask, L.nrec, (const uint2*)d_queries, (uint32_t*)d_results,
                                     max_contrib, (uint2*)d_contrib);
}
