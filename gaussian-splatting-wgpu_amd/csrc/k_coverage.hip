// k_coverage.hip -- gs_coverage_accumulate: per-splat contribution of the last frame over a set of pixels (the streaming pass of
// gs_state_coverage over the planes it fills is in k_state.hip).
//
// The reference has no counterpart (a viewer).  What a record holds is DEFINED by its blend, compute_tiles.wgsl:44-66, in the
// canonical (EXACT) arithmetic, exactly as gs_pick defines an accepted entry and its weight (k_pick.hip): one f32 rounding per
// written operation, gs_exp, wg_min, the same cond and the same T update -- whatever blend the frame itself used.  No frame kernel
// is involved: the lists (values, ranges) and the GaussianData records of the last frame are still resident.
//
// The blend's shape, not the pick's: one wave64 per 8x8 pixel block that intersects the region, lane = pixel.  Tile sizes are
// multiples of 8, so a block lies in one tile and the wave walks that tile's list:
//   fetch     per chunk of 64 entries, lane l loads values[start + 64 c + l] (coalesced) and gathers the pieces of entry l's
//             record the evaluation needs (uv; conic; opacity); the next chunk is fetched before this one is resolved;
//   evaluate  each entry's record is taken wave-uniformly with v_readlane, every lane evaluates power, alpha, test, cond and T
//             for its own pixel as written;
//   cull      the lane that fetched an entry applies the blend walkers' two parking culls to it (live box, transmittance bound);
//   reduce    only when the ballot of cond is non-zero: hits = its popcount, max_weight a wave maximum on the bit pattern
//             (w > 0), sum_q a wave sum of the two 16-bit halves of floor(w 2^32) in u32 lanes (64 x 65535 < 2^22: no 64-bit
//             cross-lane add).  The result is parked in the lane that fetched the entry;
//   add       after the chunk, the lanes that parked something issue three no-return atomics on their splat's 16-byte record:
//             u64 add, u32 add, u32 max.  One wave-instruction per field and chunk, not one per accepted entry.
// Integer adds and a max: the planes do not depend on the order in which the atomics arrive (DESIGN.md "Coverage").
// Lanes outside the region, the mask, the canvas or the slab are inert from the start; the wave stops when every live lane
// satisfies gs_pixel_final<true>(T) (no later entry can be accepted).  On a tight frame an entry whose sub-block bit
// for this block is clear is skipped before its record is gathered: no pixel of the block can reach alpha >= 1/255 (gs_tight.h),
// so it has cond = 0 on every lane.
#include "gs_kernels.h"
#include "gs_tight.h"

// grid: (blocks in x, blocks in y) of the 8x8 blocks [bx0, ...) x [by0, ...) the host found to intersect region, slab and canvas
__global__ __launch_bounds__(64) void gs_coverage_kernel(const uint4* __restrict__ gdata, const uint32_t* __restrict__ values,
                                                          const uint32_t* __restrict__ ranges, GsFrame f, uint32_t id_mask, uint32_t nrec, uint32_t bx0,
                                                          uint32_t by0, GsCoverDev r, uint32_t* __restrict__ planes) {
    const uint32_t lane = lane_id();
    const uint32_t ox = (bx0 + blockIdx.x) * 8u, oy = (by0 + blockIdx.y) * 8u; // the block's first pixel
    const uint32_t px = ox + (lane & 7u), py = oy + (lane >> 3);
    bool live = px >= r.x0 && px < r.x1 && py >= r.y0 && py < r.y1 && px < f.width && py < f.height && px >= f.px0 && px - f.px0 < f.slab_w;
    if (live && r.mask) live = r.mask[(uint64_t)py * f.width + px] != 0;
    if (!__ballot(live)) return;
    const uint32_t tx = ox / f.tile_size, ty = oy / f.tile_size;
    if (tx >= f.ntx || ty >= f.nty) return; // (cannot happen for a block with a live pixel; keeps the range read inside its array)
    const uint2 run = gs_tile_range(ranges, tx + ty * f.ntx, f.capacity); // canvas tile index, as every blend kernel forms it
    const uint32_t start = run.x, end = run.y < start ? start : run.y;
    // this block's bit of a tight frame's mask: the block itself at tile 16, the 16x16 quadrant holding it at tile 32, the tile at 8
    uint32_t want = 0u;
    if (id_mask != 0xFFFFFFFFu) {
        const uint32_t sub = f.tile_size == 8u ? 8u : f.tile_size / 2u;
        const uint32_t lx = (ox % f.tile_size) / sub, ly = (oy % f.tile_size) / sub;
        want = 1u << (GS_ID_BITS + (f.tile_size == 8u ? 0u : ly * 2u + lx));
    }
    const float pxf = (float)px, pyf = (float)py, oxf = (float)ox, oyf = (float)oy;
    const float Wf = (float)f.width, Hf = (float)f.height;
    const float c255 = (float)(1.0 / 255.0);
    float T = 1.0f;
    GsListRec cur = gs_list_fetch(gdata, values, start + lane, end, id_mask, want, nrec, f.n);
    for (uint32_t b = start; b < end; b += 64u) {
        const GsListRec nxt = gs_list_fetch(gdata, values, b + 64u + lane, end, id_mask, want, nrec, f.n); // in flight while this chunk is resolved
        // The blend walkers' two parking culls (gs_device.h; k_blend.hip tells what they save), taken by the lane that fetched the
        // entry: it stays only if its alpha >= 1/255 ellipse reaches the bounding box of the pixels that are still LIVE, and if
        // the largest T among them leaves room for it (Tmax (1 - alpha_lo) >= 1e-4).  Both are conservative with margins and hold
        // for the whole chunk (the live set only shrinks, T only falls): a culled entry has cond = 0 on every lane.
        const bool done = !live || gs_pixel_final<true>(T);
        const unsigned long long lv = __ballot(!done);
        if (!lv) break; // every live pixel is final
        const GsLiveBox lb = gs_live_box<false>(lv);
        const float Tmax = __uint_as_float(gs_bcast(wave_incl_max(done ? 0u : __float_as_uint(T)), 63));
        bool rel = cur.live;
        if (rel) {
            const float lim = __builtin_amdgcn_logf(cur.op * 255.0f) * 0.693147182464599609375f + 0.01f; // alpha >= c255 <=> q <= ln(255 op)
            const bool pd = (cur.cx > 0.0f) && (cur.cz > 0.0f) && (cur.cx * cur.cz - cur.cy * cur.cy > 0.0f);
            const float dxh = cur.ux * Wf - oxf, dyh = cur.uy * Hf - oyf; // centre - block origin; the box is in offsets centre - pixel
            float mag;
            const float qm = block_qmin(cur.cx, cur.cy, cur.cz, dxh - lb.c1, dxh - lb.c0, dyh - lb.r1, dyh - lb.r0, mag);
            rel = !pd || !(qm > lim + 1.0e-5f * mag); // NaNs compare false: the entry stays
            if (rel && pd && blend_tmax_cull(cur.cx, cur.cy, cur.cz, cur.op, dxh - lb.c1, dxh - lb.c0, dyh - lb.r1, dyh - lb.r0, Tmax)) rel = false;
        }
        unsigned long long m = __ballot(rel);
        uint32_t a_hits = 0u, a_max = 0u; // what this lane's entry gathered over the block
        unsigned long long a_sum = 0ull;
        bool settled = false;
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1ull;
            const float ux = gs_bcast(cur.ux, l), uy = gs_bcast(cur.uy, l);
            const float cx = gs_bcast(cur.cx, l), cy = gs_bcast(cur.cy, l), cz = gs_bcast(cur.cz, l);
            const float op = gs_bcast(cur.op, l);
            // compute_tiles.wgsl:52-63, the head of gs_blend_exact
            const float power = gs_blend_power(cx, cy, cz, ux * Wf - pxf, uy * Hf - pyf);
            const float alpha = gs_blend_alpha(op, power);
            const float test = T * (1.0f - alpha);
            const bool cond = live && power <= 0.0f && alpha >= c255 && test >= 0.0001f;
            const unsigned long long acc = __ballot(cond);
            if (!acc) continue; // cond = 0 on every pixel: nothing changes (k_pick.hip)
            const float w = cond ? alpha * T : 0.0f; // the entry's weight: T before the entry
            if (cond) T = test;                      // cond test + (1 - cond) T
            const uint32_t q = (uint32_t)(w * 4294967296.0f); // floor(w 2^32): the product is exact and w <= 0.99
            const uint32_t wmax = gs_bcast(wave_incl_max(__float_as_uint(w)), 63); // w >= 0: the bits order like the floats
            const uint32_t slo = wave_sum(q & 0xFFFFu), shi = wave_sum(q >> 16);
            if (lane == (uint32_t)l) {
                a_hits = (uint32_t)__popcll(acc);
                a_max = wmax;
                a_sum = ((unsigned long long)shi << 16) + slo;
            }
            if (!__ballot(live && !gs_pixel_final<true>(T))) { settled = true; break; }
        }
        if (a_hits) { // (a lane that parked something fetched a live entry: cur.id < n)
            uint32_t* rec = planes + (uint64_t)cur.id * 4u; // gs_coverage_rec: sum_q @0, hits @8, max_weight @12
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(rec), a_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(rec + 2, a_hits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(rec + 3, a_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (settled) break;
        cur = nxt;
    }
}

void gs_launch_coverage(const GsLists& L, uint32_t bx0, uint32_t by0, uint32_t nbx, uint32_t nby, const GsCoverDev& r, void* planes, hipStream_t st) {
    if (!nbx || !nby) return;
    gs_coverage_kernel<<<dim3(nbx, nby), 64, 0, st>>>((const uint4*)L.gdata, L.values, L.ranges, L.f, L.id_mask, L.nrec, bx0, by0, r, (uint32_t*)planes);
}
