// gs_device.h -- shared device-side definitions for the gfx950 kernels.
//
// Canonical float semantics (DESIGN.md "Bit-exactness"): the kernels that feed integer outputs
// (rects, tile counts, sort keys) evaluate every WGSL expression as written, left to right, one
// IEEE binary32 rounding per operation.  The whole library is compiled with -ffp-contract=off,
// so a*b+c is two roundings unless it is written as __builtin_fmaf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GS_WAVE 64

// ---- frame constants, passed by value to every kernel -------------------------------------------
struct GsFrame {
    uint32_t n;          // gaussians
    uint32_t width, height, tile_size;
    uint32_t ntx, nty;   // ceil(f32(W)/f32(ts)) (process_gaussians.wgsl:79)
    uint32_t col0, col1; // tile-column slab [col0,col1)
    uint32_t px0, slab_w;// first pixel column and pixel width of the slab
    uint32_t capacity;   // entries the (key,value) arrays can hold
    uint32_t full;       // col0==0 && col1==ntx
    uint32_t row_cap;    // row-item slots the arena / the row-sorted array can hold (a multiple of 16: tight row pipeline)
};

// ---- device-resident control block (zeroed by one memset per frame) -----------------------------
// Every word another workgroup polls lives here or in the status arrays that follow it.
// tile_counts[] words: tile count in the low 22 bits, depth bucket u32(min(50*depth,999)) in the high 10
#define GS_COUNT_BITS 22
#define GS_COUNT_MASK 0x3FFFFFu

struct GsControl {
    uint32_t scan_ticket[2];  // dynamic block ids of the tile-count scan (index-order pipeline)
    uint32_t sort_ticket[4];  // dynamic tile ids, one per radix pass of the instance sort
    uint32_t rows_ticket;     // ... of the row sort (k_rows.hip)
    uint32_t num_slots;       // row-item slots of the frame in depth order (written by the gaussian-level sort)
    uint32_t num_items;       // row items of the frame (slots that are not holes; written by the expansion)
    uint32_t fault;           // set when a bounded spin gives up
    uint32_t overflow;        // set when I exceeds capacity, or the row items the arena
    uint32_t num_intersections; // I
    uint32_t num_visible;
    uint32_t pad0;
    uint32_t row_cursor[16];  // tight projection: slots handed out of each of the arena's 16 shards
    uint32_t rec_cursor[16];  // ... and GaussianData records handed out of each of the record array's 16 shards (k_preprocess.hip)
    unsigned long long num_processed[64]; // blend: staged list entries (64 partial sums)
    unsigned long long num_evaluated[64]; // blend: (wave, entry) pairs that survived the 8x8 cull
    uint32_t hist[4][256];    // instance sort: digit histograms -> exclusive digit bases
    uint32_t rowhist[8][256]; // row sort: items per tile row, accumulated by the tight projection in 8 copies (workgroup % 8:
                              // one word would take every workgroup's atomic); readers add the copies up (gs_rowhist)
};
__device__ __forceinline__ uint32_t gs_rowhist(const GsControl* ctl, uint32_t r) {
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += ctl->rowhist[k][r];
    return s;
}

// What gs_wait needs to know about a frame, written by ONE thread of the frame's last binning kernel straight into host-mapped
// (page-locked) memory: no device-to-host copy is enqueued per frame (round 2: two copy kernels of ~4.7 us each behind every
// blend).  sticky: words that survive the per-frame memset -- every frame folds its flags into them, so the report of the last
// frame of a batch also tells about the frames enqueued before it ([0] frames that overflowed a capacity, [1] a bounded spin
// gave up, [2] largest instance count, [3] largest arena demand in slots).
struct GsReport {
    uint32_t fault, overflow, num_intersections, num_visible, num_slots, num_items, pad0, pad1;
    uint32_t row_cursor[16];
    uint32_t sticky[4];
};
__device__ __forceinline__ void gs_frame_report(const GsControl* ctl, uint32_t I, uint32_t num_items, uint32_t capacity, uint32_t* sticky,
                                                GsReport* rep) {
    uint32_t need = 0; // arena slots this frame would have needed: 16 shards as large as the fullest one
    for (int k = 0; k < 16; ++k) need = ctl->row_cursor[k] > need ? ctl->row_cursor[k] : need;
    need = need > 0x07FFFFFFu ? 0x7FFFFFFFu : need * 16u;
    const uint32_t over = (I > capacity || ctl->overflow) ? 1u : 0u;
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    if (sticky) {
        s0 = atomicAdd(&sticky[0], over) + over;
        s1 = atomicOr(&sticky[1], ctl->fault ? 1u : 0u) | (ctl->fault ? 1u : 0u);
        s2 = atomicMax(&sticky[2], I); s2 = s2 > I ? s2 : I;
        s3 = atomicMax(&sticky[3], need); s3 = s3 > need ? s3 : need;
    }
    if (rep) {
        rep->fault = ctl->fault; rep->overflow = over; rep->num_intersections = I; rep->num_visible = ctl->num_visible;
        rep->num_slots = ctl->num_slots; rep->num_items = num_items;
        for (int k = 0; k < 16; ++k) rep->row_cursor[k] = ctl->row_cursor[k];
        rep->sticky[0] = s0; rep->sticky[1] = s1; rep->sticky[2] = s2; rep->sticky[3] = s3;
    }
}

struct GsTightOut { // product-path outputs of the tight projection beside GaussianData and the count words (k_preprocess.hip)
    uint32_t* arena; uint32_t* rowptr; GsControl* ctl;
    unsigned short* unit_off; uint32_t* unit_n; // the entries' third plane and the survivors of every 1024-index unit
    uint32_t rec_shard_cap; // records each of the 16 shards of the record array holds
};
// Records the GaussianData array of a scene of n gaussians holds: the tight projection hands out record slots in 16 shards of
// ceil(workgroups / 16) workgroups' worth of gaussians each (at most 8 cull chunks of 512 per workgroup), so up to 15 workgroups'
// worth lie beyond n.  A frame of the reference's binning uses the first n (slot = index).
#define GS_RECORD_SLACK (16u * 512u * 8u)

struct GsScene {
    const float* px; const float* py; const float* pz; // f32[N] each: all the cull reads
    const float* smax; // f32[N]: largest log-scale of the gaussian (only read by tile-column slabs: conservative radius)
    const float4* geo; // 32 bytes per gaussian: [0] log-scale xyz, opacity logit   [1] rot r,x,y,z
    const float4* sh;  // 192 bytes per gaussian (three 64-byte sectors of its own): 48 SH floats, coefficient-major RGB
                       // Two arrays, not one 256-byte record: the covariance phase reads 32 bytes, the colour phase -- long
                       // after it, behind the tight row counting -- 192; in one record the first 128-byte line was fetched by
                       // both (round 2: 1.19 GB of traffic for 0.78 GB of algorithmic bytes, profiles/README.md)
    const uint8_t* state; // u8[N] state plane (GS_FLAG_SPLAT_STATE; null otherwise): read by the STATE projection with the positions
};

// state byte (gs_abi.h GS_SPLAT_*) and the selection tint as the projection applies it: col + k (t - col), k = a / 255, t = channel / 255
#define GS_ST_HIDDEN 1u
#define GS_ST_SELECTED 2u
struct GsTint { float t[3]; float k; };
// the four operations of gs_abi.h GS_STATE_* on one byte (k_state.hip)
__device__ __forceinline__ uint32_t gs_state_apply(uint32_t s, uint32_t op, uint32_t bits) {
    return op == 1u ? (s | bits) : op == 2u ? (s & ~bits) : op == 3u ? (s ^ bits) : bits;
}
// The state bytes of quad q (splats 4q .. 4q+3) as one word, byte k = splat 4q + k, and how many of them the plane holds (0 beyond
// N).  The last partial word is read byte by byte: nothing past N is read.  A null plane (a context without GS_FLAG_SPLAT_STATE)
// reads as all-zero bytes.  The selection's reader (k_export.hip); the state pass (k_state.hip) reads its word the same way, written
// out, because it also stores what it read.
struct GsStateQuad { uint32_t w, valid; };
__device__ __forceinline__ GsStateQuad gs_state_quad(const uint8_t* __restrict__ state, uint32_t n, uint32_t q) {
    const uint64_t first = (uint64_t)q * 4u;
    uint32_t w = 0u, valid = 0u;
    if (first + 4u <= n) {
        valid = 4u;
        if (state) w = reinterpret_cast<const uint32_t*>(state)[q];
    } else if (first < n) {
        valid = (uint32_t)(n - first);
        if (state)
            for (uint32_t k = 0; k < valid; ++k) w |= (uint32_t)state[first + k] << (8u * k);
    }
    return GsStateQuad{w, valid};
}

struct GsPlyTable { // where the 11 + 48 values of a packed record live in a raw .ply vertex (gs_upload_ply)
    uint32_t stride, nsrc, all_float;
    uint16_t soff[11 + 48];
    uint8_t stype[11 + 48], slot[11 + 48];
};

struct GsUniforms { // 160 B, renderer.ts:15-24
    float view[16];
    float proj[16];
    float cam[3];
    float tan_fovx, tan_fovy, focal_x, focal_y, scale_modifier;
};

// ---- canonical scalar helpers (same definitions as the oracle, written independently) -----------
__device__ __forceinline__ float wg_max(float a, float b) { return (a < b) ? b : a; }
__device__ __forceinline__ float wg_min(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ int wg_maxi(int a, int b) { return (a < b) ? b : a; }
__device__ __forceinline__ int wg_mini(int a, int b) { return (b < a) ? b : a; }

// f32 -> i32: truncate, saturate, NaN -> 0
__device__ __forceinline__ int f2i_sat(float x) {
    if (x != x) return 0;
    if (x >= 2147483648.0f) return 2147483647;
    if (x <= -2147483648.0f) return (-2147483647 - 1);
    return (int)x;
}
__device__ __forceinline__ uint32_t f2u_sat(float x) {
    if (x != x) return 0u;
    if (x >= 4294967296.0f) return 0xFFFFFFFFu;
    if (x <= 0.0f) return 0u;
    return (uint32_t)x;
}

// Canonical exp: Cody-Waite reduction by ln2 (hi/lo), degree-5 polynomial, two-step power-of-two
// scaling.  Only IEEE fma/mul/add/rint, so it is bit-identical to the CPU oracle's exp.
__device__ __forceinline__ float gs_exp(float x) {
    if (x != x) return x;
    if (x > 88.72283935546875f) return __builtin_inff();
    if (x < -103.97208404541015625f) return 0.0f;
    const float nf = __builtin_rintf(x * 1.44269502162933349609375f);
    float r = __builtin_fmaf(-nf, 0.693145751953125f, x);
    r = __builtin_fmaf(-nf, 1.42860677465796470642e-06f, r);
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float z = r * r;
    float y = __builtin_fmaf(p, z, r);
    y = y + 1.0f;
    const int n = (int)nf;
    const int a = n >> 1;
    const int b = n - a;
    const float sa = __uint_as_float((uint32_t)(a + 127) << 23);
    const float sb = __uint_as_float((uint32_t)(b + 127) << 23);
    return (y * sa) * sb;
}

// ---- the canonical (EXACT) blend of one list entry on one pixel: the expression tree of compute_tiles.wgsl:52-66, one rounding
// per written operation.  Shared by both blend kernels (k_blend.hip) and, up to alpha, by the pick (k_pick.hip).
// conic = (x, y, z) of the entry's conic, d = entry centre - pixel centre, in pixels
__device__ __forceinline__ float gs_blend_power(float cx, float cy, float cz, float dx, float dy) {
    const float t1 = cx * dx * dx, t2 = cz * dy * dy, t3 = cy * dx * dy;
    return -0.5f * (t1 + t2) - t3;
}
__device__ __forceinline__ float gs_blend_alpha(float op, float power) { return wg_min(0.99f, op * gs_exp(power)); }
struct GsPixel { float T, cr, cg, cb, cd; }; // a pixel's transmittance, colour and (AUX) accumulated depth
// (in and out by value: with five references the workgroup kernel's EXACT code came out with other registers)
// p1 = conic.xyz, depth; p2 = r, g, b, opacity.  A skipped entry (cond = 0) changes nothing: alpha is in [0, 0.99], so test is finite
template <bool AUX>
__device__ __forceinline__ GsPixel gs_blend_exact(GsPixel p, float4 p1, float4 p2, float dx, float dy) {
    const float power = gs_blend_power(p1.x, p1.y, p1.z, dx, dy);
    const float alpha = gs_blend_alpha(p2.w, power);
    const float test = p.T * (1.0f - alpha);
    const float cond = (power <= 0.0f && alpha >= (float)(1.0 / 255.0) && test >= 0.0001f) ? 1.0f : 0.0f;
    p.cr += cond * p2.x * alpha * p.T;
    p.cg += cond * p2.y * alpha * p.T;
    p.cb += cond * p2.z * alpha * p.T;
    if constexpr (AUX) p.cd += cond * p1.w * alpha * p.T;
    p.T = cond * test + (1.0f - cond) * p.T;
    return p;
}
// The exit criterion: a later entry is only kept with alpha >= c = f32(1/255) and T (1 - alpha) >= 1e-4, and
// fl(T fl(1 - alpha)) <= fl(T fl(1 - c)) for every such alpha, so once that is below 1e-4 the pixel is final.  (fused: its own rounding of it)
template <bool EXACT>
__device__ __forceinline__ bool gs_pixel_final(float T) {
    const float c255 = (float)(1.0 / 255.0);
    return (EXACT ? T * (1.0f - c255) : __builtin_fmaf(-T, c255, T)) < 0.0001f;
}

// ---- the two parking culls of the 8x8-block walkers (k_blend.hip; k_coverage.hip walks the same lists with the same culls) ------------
// Minimum over the pixel block [dxlo,dxhi] x [dylo,dyhi] (offsets g - p) of the quadratic
// q(d) = 0.5*(cx*dx^2 + cz*dy^2) + cy*dx*dy (power = -q).  For a positive-definite conic whose centre
// is outside the block the minimiser lies on an edge facing the centre: at most two 1-D problems.
// (v_rcp_f32 instead of an IEEE division: q is evaluated AT the clamped point, so a 1-ulp error in the
// minimiser only moves q by a second-order amount, far inside the caller's margin.)
__device__ __forceinline__ float block_qmin(float cx, float cy, float cz, float dxlo, float dxhi, float dylo, float dyhi,
                                            float& mag) {
    const float X = __builtin_fminf(__builtin_fmaxf(0.0f, dxlo), dxhi); // clamp(0, lo, hi)
    const float Y = __builtin_fminf(__builtin_fmaxf(0.0f, dylo), dyhi);
    float q = 3.0e38f;
    mag = 0.0f;
    if (X == 0.0f && Y == 0.0f) return 0.0f; // centre inside the block
    if (X != 0.0f) {
        const float dy = __builtin_fminf(__builtin_fmaxf(-cy * X * __builtin_amdgcn_rcpf(cz), dylo), dyhi);
        const float a = 0.5f * cx * X * X, b = 0.5f * cz * dy * dy, c = cy * X * dy;
        q = a + b + c;
        mag = __builtin_fabsf(a) + __builtin_fabsf(b) + __builtin_fabsf(c);
    }
    if (Y != 0.0f) {
        const float dx = __builtin_fminf(__builtin_fmaxf(-cy * Y * __builtin_amdgcn_rcpf(cx), dxlo), dxhi);
        const float a = 0.5f * cx * dx * dx, b = 0.5f * cz * Y * Y, c = cy * dx * Y;
        const float q2 = a + b + c;
        if (q2 < q) { q = q2; mag = __builtin_fabsf(a) + __builtin_fabsf(b) + __builtin_fabsf(c); }
    }
    return q;
}

// The transmittance cull of the blend walkers (see gs_blend_quad_kernel, "... and the transmittance that is left"): true if
// Tmax (1 - alpha_lo) < 1e-4 with margins, alpha_lo a lower bound of the entry's alpha over the box [dxlo,dxhi] x [dylo,dyhi]
// (offsets centre - pixel; the quadratic's maximum over a rectangle is at a corner).  Positive-definite conics only.
__device__ __forceinline__ bool blend_tmax_cull(float cx, float cy, float cz, float op, float dxlo, float dxhi, float dylo, float dyhi, float Tmax) {
    const float ax0 = (0.5f * cx) * dxlo * dxlo, ax1 = (0.5f * cx) * dxhi * dxhi, by0 = (0.5f * cz) * dylo * dylo, by1 = (0.5f * cz) * dyhi * dyhi;
    const float c00 = cy * dxlo * dylo, c01 = cy * dxlo * dyhi, c10 = cy * dxhi * dylo, c11 = cy * dxhi * dyhi;
    const float qmax = __builtin_fmaxf(__builtin_fmaxf(ax0 + by0 + c00, ax0 + by1 + c01), __builtin_fmaxf(ax1 + by0 + c10, ax1 + by1 + c11));
    const float qmag = __builtin_fmaxf(ax0, ax1) + __builtin_fmaxf(by0, by1) +
                       __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(c00), __builtin_fabsf(c01)), __builtin_fmaxf(__builtin_fabsf(c10), __builtin_fabsf(c11)));
    // alpha >= min(0.99, op exp(-qmax)) on every live pixel; 1 % off for the roundings of q, exp and the loop's own alpha
    const float alo = 0.99f * __builtin_fminf(0.99f, op * __builtin_amdgcn_exp2f(-1.44269502162933349609375f * (qmax + 1.0e-5f * qmag)));
    return Tmax * (1.0f - alo) < 0.0000999f; // (NaN anywhere: false, the entry stays)
}

// The bounding box of a block's LIVE pixels (lane = 8 row + column) from their ballot: first / last column and row, as floats.
// EMPTY_OK: lv may be 0 (the scans are guarded; the box is then meaningless and the caller must not use it)
struct GsLiveBox { float c0, c1, r0, r1; };
template <bool EMPTY_OK>
__device__ __forceinline__ GsLiveBox gs_live_box(unsigned long long lv) {
    uint32_t lcm = (uint32_t)lv | (uint32_t)(lv >> 32);
    lcm |= lcm >> 16; lcm |= lcm >> 8; lcm &= 0xFFu; // columns of the block that hold a live pixel
    const unsigned long long lo = EMPTY_OK ? lv | (1ull << 63) : lv, hi = EMPTY_OK ? lv | 1ull : lv;
    return GsLiveBox{(float)__builtin_ctz(lcm | 0x100u), (float)(31 - __builtin_clz(lcm | 1u)), (float)(__builtin_ctzll(lo) >> 3),
                     (float)((63 - __builtin_clzll(hi)) >> 3)};
}

// A tile's run [x, y) of the sorted list (ranges[] holds the inclusive scan of the tile counts), clamped to what the arrays hold
__device__ __forceinline__ uint2 gs_tile_range(const uint32_t* __restrict__ ranges, uint32_t tile, uint32_t capacity) {
    const uint32_t start = tile > 0 ? ranges[tile - 1] : 0u;
    uint32_t end = ranges[tile];
    if (end > capacity) end = capacity;
    return make_uint2(start, end);
}

// ---- an entry of the last frame's lists as a lane holds it between the fetch and the evaluation (k_pick.hip, k_coverage.hip) ------
struct GsListRec {
    float ux, uy, cx, cy, cz, z, op; // uv; conic + depth; opacity
    uint32_t id;
    bool live;
};
// Entry i of [.., end): the three pieces of its GaussianData record.  A list value names the record's SLOT (the gaussian's index
// on a frame of the reference's binning, a slot of the tight projection's otherwise); the gaussian's id is word 2 of the record,
// fetched with the uv.  id_mask: on a tight frame the sub-block mask rides above the slot (gs_tight.h); want: the bit of that mask
// the caller's block needs (0: every entry; an entry without it stays dead and its record is not gathered).  nrec: records the
// array holds; n: gaussians.
__device__ __forceinline__ GsListRec gs_list_fetch(const uint4* __restrict__ gdata, const uint32_t* __restrict__ values, uint32_t i, uint32_t end,
                                                   uint32_t id_mask, uint32_t want, uint32_t nrec, uint32_t n) {
    GsListRec r;
    r.ux = r.uy = r.cx = r.cy = r.cz = r.z = r.op = 0.0f;
    r.id = 0u;
    r.live = false;
    if (i < end) {
        const uint32_t v = values[i];
        const uint32_t g = v & id_mask;
        if (g < nrec && (want == 0u || (v & want) != 0u)) { // (a list never holds a slot >= nrec; never gather out of bounds)
            const uint4 p0 = gdata[(uint64_t)g * 4 + 0];
            const uint4 p1 = gdata[(uint64_t)g * 4 + 1];
            r.op = __uint_as_float(((const uint32_t*)gdata)[(uint64_t)g * 16 + 11]);
            r.ux = __uint_as_float(p0.x); r.uy = __uint_as_float(p0.y);
            r.cx = __uint_as_float(p1.x); r.cy = __uint_as_float(p1.y); r.cz = __uint_as_float(p1.z); r.z = __uint_as_float(p1.w);
            r.id = p0.z;
            r.live = p0.z < n; // (a listed record was written by this frame's projection: always; keeps a caller's per-splat array safe)
        }
    }
    return r;
}
// lane l's value on every lane (v_readlane: l is wave-uniform)
__device__ __forceinline__ uint32_t gs_bcast(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ float gs_bcast(float v, int l) { return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), l)); }

// Columns of a rect that fall in the slab; column ntx aliases to column 0 of the next tile row
// (write_tile_ids.wgsl:26-31).  Returns main-run [xa,xb) and whether the alias column is owned.
// Used by the projection's tile count (k_preprocess.hip) and by the emission (k_binning.hip).
__device__ __forceinline__ void slab_cols(uint32_t rx0, uint32_t rx1, const GsFrame& f, uint32_t& xa, uint32_t& wmain,
                                          uint32_t& alias) {
    const uint32_t hi = rx1 < f.ntx ? rx1 : f.ntx; // real columns end at ntx
    xa = rx0 > f.col0 ? rx0 : f.col0;
    const uint32_t xb = hi < f.col1 ? hi : f.col1;
    wmain = xb > xa ? xb - xa : 0u;
    alias = (rx1 == f.ntx + 1u && f.col0 == 0u) ? 1u : 0u;
}

// ---- wave64 helpers -------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// Scans run on DPP row shifts and row broadcasts (VALU latency, no trip through the LDS crossbar as
// ds_bpermute would make): shr 1,2,4,8 inside each row of 16, then lane 15 -> row 1 and 3, lane 31 -> rows 2,3.
// A lane whose source is out of range or masked off reads `old` = the identity.
#define GS_DPP(v, ctrl, rm) (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), (rm), 0xf, false)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t) {
    v += GS_DPP(v, 0x111, 0xf);
    v += GS_DPP(v, 0x112, 0xf);
    v += GS_DPP(v, 0x114, 0xf);
    v += GS_DPP(v, 0x118, 0xf);
    v += GS_DPP(v, 0x142, 0xa);
    v += GS_DPP(v, 0x143, 0xc);
    return v;
}
__device__ __forceinline__ unsigned long long wave_incl_scan64(unsigned long long v, uint32_t lane) { // k_gsort.hip, k_rows.hip
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
        if ((int)lane >= d) v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v) { // unsigned: the identity is 0
    uint32_t t;
    t = GS_DPP(v, 0x111, 0xf); v = (t > v) ? t : v;
    t = GS_DPP(v, 0x112, 0xf); v = (t > v) ? t : v;
    t = GS_DPP(v, 0x114, 0xf); v = (t > v) ? t : v;
    t = GS_DPP(v, 0x118, 0xf); v = (t > v) ? t : v;
    t = GS_DPP(v, 0x142, 0xa); v = (t > v) ? t : v;
    t = GS_DPP(v, 0x143, 0xc); v = (t > v) ? t : v;
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(v, 0u), 63);
}

// ---- inter-workgroup words (cdna_hip_programming.md Guideline 16, form R2: the data is the flag) --
// A status word is one naturally aligned 4- or 8-byte granule written by ONE relaxed agent-scope
// atomic store (sc1, bypasses L1/keeps no stale copy) and polled with relaxed agent-scope loads.
__device__ __forceinline__ void st_agent(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent64(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long ld_agent64(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#define GS_SPIN_LIMIT (1u << 22) // bounded spins: give up, raise GsControl::fault, never hang the GPU
