// k_attr.hip -- the splat attributes' kernels: select, summarise, histogram and read resident splats by one f32 value per splat
// (gs_attr.hip, gs_state.hip gs_state_attr; gs_abi.h "splat attributes").  The reference has no counterpart: it is a viewer, and an
// editor built on it would scan the 320-byte records its host kept.
//
// The value is defined ONCE, in attr_value<KIND> and the three expression helpers under it (the one of the centre, attr_of_pos, is in
// gs_consensus_host.h, where the consensus kernel and its host loop read it too); the four kernels are instantiated per
// kind and the launchers dispatch with a switch, so no kernel branches on the kind.  Bytes read per splat for the value:
//   POS_X / Y / Z, LOG_SCALE_MAX             4 B   (its own f32 plane; a float4 per quad.  LOG_SCALE_MAX: + 16 B where the plane holds a NaN)
//   DIST2, PLANE                            12 B   (the three position planes; three float4 per quad)
//   OPACITY_LOGIT, LOG_SCALE_MIN / SUM,
//   ANISOTROPY                              16 B   (the first float4 of the 32-byte geometry record: half of each 32-byte sector pair)
//   DC_R / G / B                            12 B   (the head of the 192-byte SH block: one 32-byte sector of six is touched)
//   COVER_HITS / MAX_WEIGHT / SUM           16 B   (the coverage record)
// plus 1 B of state per splat when a filter other than (0, 0) is given (the select pass always reads it, and writes at most 1 B).
//   select    : the state pass of k_state.hip -- thread q owns splats 4q .. 4q+3 and their state word, stores it only if it changed.
//   summary   : the same quad mapping; per workgroup two integer adds, one atomicMin and one atomicMax on u32 keys into one of
//               GS_STATE_SLOTS records.
//   histogram : a persistent grid strides over the quads; each workgroup counts into bins + 3 LDS words and adds its non-zero
//               words to the u64 result when its loop ends: O(grid x bins) global atomics, not O(N).
//   values    : one thread per output float, a gather through the selection's id list or dense.
// Bound: HBM for the plane kinds, sector-granular gathers for the record kinds.  No MFMA (no contraction).  Plain C++ and vector
// atomics only.
#include "gs_device.h"
#include "gs_kernels.h"
#include "gs_state_sum.h"
#include "../../include/gsplat/gs_abi.h"

// ---- the value ---------------------------------------------------------------------------------------------------------------------
// kinds that ARE one float of a 4-byte plane
template <int KIND>
__device__ __forceinline__ const float* attr_plane(const GsScene& s) {
    return KIND == GS_ATTR_POS_X ? s.px : KIND == GS_ATTR_POS_Y ? s.py : KIND == GS_ATTR_POS_Z ? s.pz : KIND == GS_ATTR_LOG_SCALE_MAX ? s.smax : nullptr;
}
template <int KIND> constexpr bool attr_is_plane() {
    return KIND == GS_ATTR_POS_X || KIND == GS_ATTR_POS_Y || KIND == GS_ATTR_POS_Z || KIND == GS_ATTR_LOG_SCALE_MAX;
}
template <int KIND> constexpr bool attr_is_pos() { return KIND == GS_ATTR_DIST2 || KIND == GS_ATTR_PLANE; }
template <int KIND> constexpr bool attr_is_cover() { return KIND >= GS_ATTR_COVER_HITS; }
// ... are an expression of the centre: attr_of_pos<KIND>, gs_consensus_host.h's one copy (the consensus kernel and its host loop use it too)
// fmaxf / fminf as gs_abi.h means them: a NaN operand, quiet OR signalling, is missing data, and the result is a NaN only when both
// are.  (v_max_f32 / v_min_f32 alone, which __builtin_fmaxf compiles to, turn a signalling NaN into a quiet one instead of dropping it.)
__device__ __forceinline__ float attr_fmax(float a, float b) { return a != a ? b : b != b ? a : __builtin_fmaxf(a, b); }
__device__ __forceinline__ float attr_fmin(float a, float b) { return a != a ? b : b != b ? a : __builtin_fminf(a, b); }
// ... of the geometry record's first float4: log-scale x, y, z, opacity logit
template <int KIND>
__device__ __forceinline__ float attr_of_geo(float4 g) {
    if (KIND == GS_ATTR_OPACITY_LOGIT) return g.w;
    if (KIND == GS_ATTR_LOG_SCALE_SUM) return (g.x + g.y) + g.z;
    const float hi = attr_fmax(g.x, attr_fmax(g.y, g.z));
    if (KIND == GS_ATTR_LOG_SCALE_MAX) return hi;
    const float lo = attr_fmin(g.x, attr_fmin(g.y, g.z));
    return KIND == GS_ATTR_LOG_SCALE_MIN ? lo : hi - lo;
}
// LOG_SCALE_MAX is read from the smax plane, which the upload fills with the same expression in the hardware's fmaxf.  The two differ
// only where the plane holds a NaN (a signalling NaN among the log-scales, or three NaNs): such a splat's value comes from its record.
__device__ __forceinline__ float attr_smax(const GsScene& s, float plane, uint32_t i) {
    return plane != plane ? attr_of_geo<GS_ATTR_LOG_SCALE_MAX>(s.geo[(uint64_t)i * 2u]) : plane;
}
// ... of the coverage record {sum_q lo, sum_q hi, hits, max_weight}
template <int KIND>
__device__ __forceinline__ float attr_of_cover(uint4 r) {
    if (KIND == GS_ATTR_COVER_HITS) return (float)r.z;
    if (KIND == GS_ATTR_COVER_MAX_WEIGHT) return __uint_as_float(r.w);
    return (float)r.y + (float)r.x * 0x1p-32f;
}
template <int KIND>
__device__ __forceinline__ float attr_value(const GsScene& s, const uint4* __restrict__ cov, const GsAttrDev& a, uint32_t i) {
    if constexpr (KIND == GS_ATTR_LOG_SCALE_MAX) return attr_smax(s, s.smax[i], i);
    else if constexpr (attr_is_plane<KIND>()) return attr_plane<KIND>(s)[i];
    else if constexpr (attr_is_pos<KIND>()) return attr_of_pos<KIND>(a, s.px[i], s.py[i], s.pz[i]);
    else if constexpr (attr_is_cover<KIND>()) return attr_of_cover<KIND>(cov[i]);
    else if constexpr (KIND >= GS_ATTR_DC_R && KIND <= GS_ATTR_DC_B) return reinterpret_cast<const float*>(s.sh)[(uint64_t)i * 48u + (uint32_t)(KIND - GS_ATTR_DC_R)];
    else return attr_of_geo<KIND>(s.geo[(uint64_t)i * 2u]);
}
// The values of the `valid` first splats of quad q.  A whole quad reads its planes as float4 (they are 256-byte aligned with room
// for a whole last quad behind N, but a partial quad goes splat by splat all the same: nothing past N is read).
template <int KIND>
__device__ __forceinline__ void attr_quad(const GsScene& s, const uint4* __restrict__ cov, const GsAttrDev& a, uint32_t q, uint32_t valid, float v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.0f;
    if (valid == 4u && attr_is_plane<KIND>()) {
        const float4 t = reinterpret_cast<const float4*>(attr_plane<KIND>(s))[q];
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        if constexpr (KIND == GS_ATTR_LOG_SCALE_MAX) {
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) v[k] = attr_smax(s, v[k], q * 4u + k);
        }
    } else if (valid == 4u && attr_is_pos<KIND>()) {
        const float4 x = reinterpret_cast<const float4*>(s.px)[q], y = reinterpret_cast<const float4*>(s.py)[q], z = reinterpret_cast<const float4*>(s.pz)[q];
        v[0] = attr_of_pos<KIND>(a, x.x, y.x, z.x); v[1] = attr_of_pos<KIND>(a, x.y, y.y, z.y);
        v[2] = attr_of_pos<KIND>(a, x.z, y.z, z.z); v[3] = attr_of_pos<KIND>(a, x.w, y.w, z.w);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
            if (k < valid) v[k] = attr_value<KIND>(s, cov, a, q * 4u + k);
    }
}

// ---- select: the state pass (k_state.hip) around (v >= lo && v <= hi) == inside; a NaN is in no range -------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void gs_attr_state_kernel(uint8_t* __restrict__ state, GsScene s, const uint4* __restrict__ cov, uint32_t n, GsAttrDev a,
                                                             float lo, float hi, uint32_t inside, uint32_t op, uint32_t bits, uint32_t wmask,
                                                             uint32_t wvalue, unsigned long long* __restrict__ matched) {
    state_block_begin();
    const uint32_t q = blockIdx.x * 256u + threadIdx.x; // splats 4q .. 4q+3
    const uint64_t first = (uint64_t)q * 4u;
    const bool want = inside != 0u;
    uint32_t hits = 0;
    if (first + 4u <= n) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(state)[q];
        float v[4];
        attr_quad<KIND>(s, cov, a, q, 4u, v);
        uint32_t nw = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t sv = (w >> (8 * k)) & 0xFFu;
            const bool in = ((sv & wmask) == wvalue) && ((v[k] >= lo && v[k] <= hi) == want);
            hits += in ? 1u : 0u;
            nw |= (in ? gs_state_apply(sv, op, bits) : sv) << (8 * k);
        }
        if (nw != w) reinterpret_cast<uint32_t*>(state)[q] = nw; // stored only if it changed
    } else if (first < n) {
        for (uint64_t i = first; i < n; ++i) {
            const uint32_t sv = state[i];
            const float v = attr_value<KIND>(s, cov, a, (uint32_t)i);
            const bool in = ((sv & wmask) == wvalue) && ((v >= lo && v <= hi) == want);
            hits += in ? 1u : 0u;
            const uint32_t nv = in ? gs_state_apply(sv, op, bits) : sv;
            if (nv != sv) state[i] = (uint8_t)nv;
        }
    }
    state_block_add(hits, matched);
}

// ---- summary ------------------------------------------------------------------------------------------------------------------------
// the order-preserving map of an f32's bit pattern (gs_abi.h): unsigned order of the keys = -inf < ... < -0 < +0 < ... < +inf
__device__ __forceinline__ uint32_t attr_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
template <int KIND>
__global__ __launch_bounds__(256) void gs_attr_summary_kernel(const uint8_t* __restrict__ state, GsScene s, const uint4* __restrict__ cov, uint32_t n,
                                                               GsAttrDev a, uint32_t mask, uint32_t value, unsigned long long* __restrict__ slots) {
    __shared__ uint32_t s_matched, s_nan, s_kmin, s_kmax;
    if (threadIdx.x == 0) { s_matched = 0u; s_nan = 0u; s_kmin = 0xFFFFFFFFu; s_kmax = 0u; }
    __syncthreads();
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const GsStateQuad sq = gs_state_quad(state, n, q);
    float v[4];
    attr_quad<KIND>(s, cov, a, q, sq.valid, v);
    uint32_t matched = 0u, nan = 0u, kmin = 0xFFFFFFFFu, kmax = 0u; // (the identities are keys of NaNs: no value has them)
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        if (k < sq.valid && (((sq.w >> (8u * k)) & 0xFFu) & mask) == value) {
            ++matched;
            if (v[k] != v[k]) ++nan;
            else {
                const uint32_t key = attr_key(v[k]);
                kmin = key < kmin ? key : kmin;
                kmax = key > kmax ? key : kmax;
            }
        }
    }
    // per wave (DPP), then per workgroup through LDS, then one record of the slots
    const uint32_t wm = wave_sum(matched), wn = wave_sum(nan);
    const uint32_t wmax = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max(kmax), 63);
    const uint32_t wmin = ~(uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max(~kmin), 63);
    if ((threadIdx.x & 63u) == 0u && wm) {
        atomicAdd(&s_matched, wm);
        if (wn) atomicAdd(&s_nan, wn);
        atomicMin(&s_kmin, wmin);
        atomicMax(&s_kmax, wmax);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_matched) {
        unsigned long long* slot = slots + (blockIdx.x % GS_STATE_SLOTS) * GS_STATE_SLOT_STRIDE;
        atomicAdd(slot, (unsigned long long)s_matched);
        if (s_nan) atomicAdd(slot + 1, (unsigned long long)s_nan);
        uint32_t* keys = reinterpret_cast<uint32_t*>(slot + 2);
        if (s_kmin != 0xFFFFFFFFu) { // a workgroup of NaNs only has neither
            atomicMin(keys, s_kmin);
            atomicMax(keys + 1, s_kmax);
        }
    }
}

// ---- histogram ----------------------------------------------------------------------------------------------------------------------
#define GS_ATTR_MAX_BINS 1024u
// the slot of one value among bins + 3 (gs_abi.h): bins, then below, above, NaN.  The conversion saturates (a NaN product, which only
// an infinite scale makes, is 0); b cannot leave [0, bins) otherwise, the clamp covers the product's rounding at the top edge.
__device__ __forceinline__ uint32_t attr_bin(float v, float lo, float hi, float scale, uint32_t bins) {
    if (v != v) return bins + 2u;
    if (v < lo) return bins;
    if (v >= hi) return bins + 1u;
    const uint32_t b = f2u_sat((v - lo) * scale);
    return b < bins - 1u ? b : bins - 1u;
}
// Workgroup w takes quads [256 (w + trip * grid), ... + 256).  A wave whose 64 values all fall into one slot -- the worst case for
// LDS atomics, 64 adds to one word in turn -- adds them as one.
template <int KIND>
__global__ __launch_bounds__(256) void gs_attr_histogram_kernel(const uint8_t* __restrict__ state, GsScene s, const uint4* __restrict__ cov, uint32_t n,
                                                                 GsAttrDev a, uint32_t mask, uint32_t value, float lo, float hi, float scale, uint32_t bins,
                                                                 unsigned long long* __restrict__ counts) {
    __shared__ uint32_t s_h[GS_ATTR_MAX_BINS + 3u];
    const uint32_t words = bins + 3u; // (bins <= GS_ATTR_MAX_BINS: the launcher's guard)
    for (uint32_t i = threadIdx.x; i < words; i += 256u) s_h[i] = 0u;
    __syncthreads();
    const uint32_t quads = (uint32_t)(((uint64_t)n + 3u) / 4u);
    const uint32_t none = 0xFFFFFFFFu;
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < quads; base += (uint64_t)gridDim.x * 256u) { // (uniform per workgroup)
        const uint32_t q = (uint32_t)base + threadIdx.x;
        const GsStateQuad sq = gs_state_quad(state, n, q); // valid = 0 beyond the last quad
        float v[4];
        attr_quad<KIND>(s, cov, a, q, sq.valid, v);
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const bool in = k < sq.valid && (((sq.w >> (8u * k)) & 0xFFu) & mask) == value;
            const uint32_t b = in ? attr_bin(v[k], lo, hi, scale, bins) : none;
            const uint32_t b0 = gs_bcast(b, 0);
            if (__builtin_amdgcn_ballot_w64(b != b0) == 0ull) { // the whole wave agrees
                if ((threadIdx.x & 63u) == 0u && b0 != none) atomicAdd(&s_h[b0], 64u);
            } else if (b != none) {
                atomicAdd(&s_h[b], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < words; i += 256u) {
        const uint32_t c = s_h[i];
        if (c) atomicAdd(counts + i, (unsigned long long)c);
    }
}

// ---- values -------------------------------------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void gs_attr_values_kernel(GsScene s, const uint4* __restrict__ cov, uint32_t n, GsAttrDev a,
                                                              const uint32_t* __restrict__ ids, uint32_t first, uint32_t m, float* __restrict__ out) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= m) return;
    const uint32_t id = ids ? ids[first + g] : first + g;
    if (id < n) out[g] = attr_value<KIND>(s, cov, a, id); // (always: ids come from the selection over this scene)
}

// ---- launchers: a switch of launches, not a branch in the kernels -------------------------------------------------------------------
#define GS_ATTR_SWITCH(kind, LAUNCH)                                                                        \
    switch (kind) {                                                                                         \
    case GS_ATTR_POS_X: LAUNCH(GS_ATTR_POS_X); break;                                                       \
    case GS_ATTR_POS_Y: LAUNCH(GS_ATTR_POS_Y); break;                                                       \
    case GS_ATTR_POS_Z: LAUNCH(GS_ATTR_POS_Z); break;                                                       \
    case GS_ATTR_OPACITY_LOGIT: LAUNCH(GS_ATTR_OPACITY_LOGIT); break;                                       \
    case GS_ATTR_LOG_SCALE_MIN: LAUNCH(GS_ATTR_LOG_SCALE_MIN); break;                                       \
    case GS_ATTR_LOG_SCALE_MAX: LAUNCH(GS_ATTR_LOG_SCALE_MAX); break;                                       \
    case GS_ATTR_LOG_SCALE_SUM: LAUNCH(GS_ATTR_LOG_SCALE_SUM); break;                                       \
    case GS_ATTR_ANISOTROPY: LAUNCH(GS_ATTR_ANISOTROPY); break;                                             \
    case GS_ATTR_DC_R: LAUNCH(GS_ATTR_DC_R); break;                                                         \
    case GS_ATTR_DC_G: LAUNCH(GS_ATTR_DC_G); break;                                                         \
    case GS_ATTR_DC_B: LAUNCH(GS_ATTR_DC_B); break;                                                         \
    case GS_ATTR_DIST2: LAUNCH(GS_ATTR_DIST2); break;                                                       \
    case GS_ATTR_PLANE: LAUNCH(GS_ATTR_PLANE); break;                                                       \
    case GS_ATTR_COVER_HITS: LAUNCH(GS_ATTR_COVER_HITS); break;                                             \
    case GS_ATTR_COVER_MAX_WEIGHT: LAUNCH(GS_ATTR_COVER_MAX_WEIGHT); break;                                 \
    case GS_ATTR_COVER_SUM: LAUNCH(GS_ATTR_COVER_SUM); break;                                               \
    default: break; /* (the entry points refuse kind >= GS_ATTR_COUNT) */                                   \
    }
static uint32_t quad_blocks(uint32_t n) { return (uint32_t)((((uint64_t)n + 3u) / 4u + 255u) / 256u); }

void gs_launch_attr_state(uint32_t kind, uint8_t* state, const GsScene& s, const void* cov, uint32_t n, const GsAttrDev& a, float lo, float hi,
                          uint32_t inside, uint32_t op, uint32_t bits, uint32_t where_mask, uint32_t where_value, unsigned long long* matched,
                          hipStream_t st) {
    if (!n) return;
    const uint32_t blocks = quad_blocks(n);
#define GS_ATTR_LAUNCH(K) hipLaunchKernelGGL(gs_attr_state_kernel<K>, dim3(blocks), dim3(256), 0, st, state, s, (const uint4*)cov, n, a, lo, hi, inside, op, bits, where_mask, where_value, matched)
    GS_ATTR_SWITCH(kind, GS_ATTR_LAUNCH)
#undef GS_ATTR_LAUNCH
}
void gs_launch_attr_summary(uint32_t kind, const uint8_t* state, const GsScene& s, const void* cov, uint32_t n, const GsAttrDev& a, uint32_t mask,
                            uint32_t value, unsigned long long* slots, hipStream_t st) {
    if (!n) return;
    const uint32_t blocks = quad_blocks(n);
#define GS_ATTR_LAUNCH(K) hipLaunchKernelGGL(gs_attr_summary_kernel<K>, dim3(blocks), dim3(256), 0, st, state, s, (const uint4*)cov, n, a, mask, value, slots)
    GS_ATTR_SWITCH(kind, GS_ATTR_LAUNCH)
#undef GS_ATTR_LAUNCH
}
void gs_launch_attr_histogram(uint32_t kind, const uint8_t* state, const GsScene& s, const void* cov, uint32_t n, const GsAttrDev& a, uint32_t mask,
                              uint32_t value, float lo, float hi, float scale, uint32_t bins, unsigned long long* counts, uint32_t grid, hipStream_t st) {
    if (!n || !bins || bins > GS_ATTR_MAX_BINS) return;
    const uint32_t work = quad_blocks(n), blocks = grid < 1u ? 1u : grid < work ? grid : work;
#define GS_ATTR_LAUNCH(K) hipLaunchKernelGGL(gs_attr_histogram_kernel<K>, dim3(blocks), dim3(256), 0, st, state, s, (const uint4*)cov, n, a, mask, value, lo, hi, scale, bins, counts)
    GS_ATTR_SWITCH(kind, GS_ATTR_LAUNCH)
#undef GS_ATTR_LAUNCH
}
void gs_launch_attr_values(uint32_t kind, const GsScene& s, const void* cov, uint32_t n, const GsAttrDev& a, const uint32_t* ids, uint32_t first,
                           uint32_t m, float* out, hipStream_t st) {
    if (!m) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)m + 255u) / 256u);
#define GS_ATTR_LAUNCH(K) hipLaunchKernelGGL(gs_attr_values_kernel<K>, dim3(blocks), dim3(256), 0, st, s, (const uint4*)cov, n, a, ids, first, m, out)
    GS_ATTR_SWITCH(kind, GS_ATTR_LAUNCH)
#undef GS_ATTR_LAUNCH
}
