// k_export.hip -- the kernels behind the splat edits (gs_export.hip, gs_abi.h "splat edits"): a stable stream compaction over the
// state plane, the inverse of gs_repack_kernel (k_preprocess.hip), and a plane-to-plane gather.  The reference has no
// counterpart: its host keeps the 320-byte records it uploaded (renderer.ts:130-137) and would filter those.
//
// Selection: splats with (s & mask) == value, delivered in ascending index order, in three launches.  A workgroup owns 1024
// consecutive splats = 256 aligned state words, one word per thread as in the region kernel (k_state.hip); the last partial word
// is read byte by byte, nothing past N is read.  A null plane (a context without GS_FLAG_SPLAT_STATE) reads as all-zero bytes.
//   count   : 1 B read per splat, one count per workgroup written.
//   scan    : ONE workgroup loops over the counts with a running carry (5 958 counts at 6.1 M splats, 48 829 at 50 M): in place,
//             exclusive, the total behind the last count.  No look-back, no spin: not a per-frame path.
//   scatter : 1 B read per splat, 4 B written per match: recomputes the flags, ranks them inside the workgroup (popcount per
//             word, DPP wave prefix, the four wave totals through LDS) and stores ids[base + rank] = index.
//   unpack  : one thread per (output record, 16-byte column), 20 columns: 244 B gathered from px/py/pz, geo, sh and 320 B written
//             per kept splat, the 320-byte side fully coalesced (one float4 per thread).  Bound: HBM.
//   compact : the same indexing over the NEW scene's planes, 16 columns per kept splat: 4 position/smax floats, 2 + 12 float4, the
//             state byte.  245 B read and written per kept splat.  Bound: HBM.
// No MFMA anywhere (no contraction).  Every store is a plain vector store.
#include "gs_device.h"
#include "gs_kernels.h"

// Match flags of splats 4q .. 4q+3 (bit k = splat 4q + k); 0 beyond N.
__device__ __forceinline__ uint32_t select_flags(const uint8_t* __restrict__ state, uint32_t n, uint32_t q, uint32_t mask, uint32_t value) {
    const GsStateQuad s = gs_state_quad(state, n, q);
    uint32_t f = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) f |= (k < s.valid && (((s.w >> (8u * k)) & 0xFFu) & mask) == value) ? (1u << k) : 0u;
    return f;
}

__global__ __launch_bounds__(256) void gs_select_count_kernel(const uint8_t* __restrict__ state, uint32_t n, uint32_t mask, uint32_t value,
                                                               uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_w[4];
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const uint32_t ws = wave_sum((uint32_t)__builtin_popcount(select_flags(state, n, q, mask, value)));
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = ws;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// counts[0 .. nb) -> exclusive prefix in place, counts[nb] = total.  One workgroup; the sum is at most N < 2^31.
__global__ __launch_bounds__(256) void gs_select_scan_kernel(uint32_t* __restrict__ counts, uint32_t nb) {
    __shared__ uint32_t s_w[4];
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < nb; base += 256u) { // (uniform trip count: every thread reaches every barrier)
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? counts[i] : 0u;
        const uint32_t incl = wave_incl_scan(v, 0u);
        if ((threadIdx.x & 63u) == 63u) s_w[threadIdx.x >> 6] = incl;
        __syncthreads();
        const uint32_t wv = threadIdx.x >> 6;
        const uint32_t before = (wv > 0u ? s_w[0] : 0u) + (wv > 1u ? s_w[1] : 0u) + (wv > 2u ? s_w[2] : 0u);
        const uint32_t total = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        if (i < nb) counts[i] = carry + before + (incl - v);
        carry += total;
        __syncthreads(); // s_w is rewritten by the next trip
    }
    if (threadIdx.x == 0) counts[nb] = carry;
}

__global__ __launch_bounds__(256) void gs_select_scatter_kernel(const uint8_t* __restrict__ state, uint32_t n, uint32_t mask, uint32_t value,
                                                                 const uint32_t* __restrict__ offsets, uint32_t* __restrict__ ids, uint32_t cap) {
    __shared__ uint32_t s_w[4];
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const uint32_t f = select_flags(state, n, q, mask, value);
    const uint32_t cnt = (uint32_t)__builtin_popcount(f);
    const uint32_t incl = wave_incl_scan(cnt, 0u);
    if ((threadIdx.x & 63u) == 63u) s_w[threadIdx.x >> 6] = incl;
    __syncthreads();
    const uint32_t wv = threadIdx.x >> 6;
    uint32_t at = offsets[blockIdx.x] + (wv > 0u ? s_w[0] : 0u) + (wv > 1u ? s_w[1] : 0u) + (wv > 2u ? s_w[2] : 0u) + (incl - cnt);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        if ((f >> k) & 1u) {
            if (at < cap) ids[at] = q * 4u + k; // (cap = the scanned total: cannot fail; keeps the store inside the list whatever the plane does)
            ++at;
        }
}

uint32_t gs_select_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + 1023u) / 1024u); }
void gs_launch_select_count(const uint8_t* state, uint32_t n, uint32_t mask, uint32_t value, uint32_t* counts, hipStream_t st) {
    const uint32_t nb = gs_select_blocks(n);
    if (nb) hipLaunchKernelGGL(gs_select_count_kernel, dim3(nb), dim3(256), 0, st, state, n, mask, value, counts);
    hipLaunchKernelGGL(gs_select_scan_kernel, dim3(1), dim3(256), 0, st, counts, nb); // (nb = 0: writes the total 0)
}
void gs_launch_select_scatter(const uint8_t* state, uint32_t n, uint32_t mask, uint32_t value, const uint32_t* offsets, uint32_t* ids, uint32_t cap,
                              hipStream_t st) {
    const uint32_t nb = gs_select_blocks(n);
    if (nb && cap) hipLaunchKernelGGL(gs_select_scatter_kernel, dim3(nb), dim3(256), 0, st, state, n, mask, value, offsets, ids, cap);
}

// ---- position planes + geometry / SH records -> 320-byte AoS (ply.ts:190-198): the inverse of gs_repack_kernel ----------------
// Output record g (0 .. m) is splat ids[first + g], or first + g when ids is null (the (0, 0) filter: no selection ran).
// out_ids (may be null) receives that index.  Padding lanes write +0.0f.
__global__ __launch_bounds__(256) void gs_unpack_kernel(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                         const float* __restrict__ geo, const float* __restrict__ sh, uint32_t n,
                                                         const uint32_t* __restrict__ ids, uint32_t first, uint32_t m, float4* __restrict__ aos,
                                                         uint32_t* __restrict__ out_ids) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)m * 20) return;
    const uint32_t g = (uint32_t)(t / 20), c = (uint32_t)(t % 20);
    const uint32_t id = ids ? ids[first + g] : first + g;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (id < n) { // (always: ids come from the selection over this scene)
        const float* r = geo + (uint64_t)id * 8;
        if (c == 0) { v.x = px[id]; v.y = py[id]; v.z = pz[id]; }
        else if (c == 1) { v.x = r[0]; v.y = r[1]; v.z = r[2]; }
        else if (c == 2) { v.x = r[4]; v.y = r[5]; v.z = r[6]; v.w = r[7]; }
        else if (c == 3) { v.x = r[3]; }
        else {
            const float* q = sh + (uint64_t)id * 48 + 3 * (c - 4);
            v.x = q[0]; v.y = q[1]; v.z = q[2];
        }
    }
    aos[t] = v;
    if (c == 0 && out_ids) out_ids[g] = id;
}
void gs_launch_unpack(const GsScene& s, uint32_t n, const uint32_t* ids, uint32_t first, uint32_t m, void* d_aos, uint32_t* out_ids, hipStream_t st) {
    const uint64_t total = (uint64_t)m * 20;
    if (!total) return;
    hipLaunchKernelGGL(gs_unpack_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, s.px, s.py, s.pz, (const float*)s.geo,
                       (const float*)s.sh, n, ids, first, m, (float4*)d_aos, out_ids);
}

// ---- old scene -> new scene: new splat first + g is old splat ids[g] -----------------------------------------------------------
// One thread per (new splat, column), 16 columns: 0 the four plane floats, 1-2 geometry, 3-14 SH, 15 the state byte.  The state
// plane is written one whole word by the column-15 thread of every fourth splat (its own byte and its three neighbours', 0 past
// the new N), so no byte store races with a neighbour's.  A compaction passes first = 0; a duplication (gs_insert.hip) the old N
// and no state words: the words of its plane do not start at a gathered splat, the grow pass has written them.
__global__ __launch_bounds__(256) void gs_compact_planes_kernel(GsScene o, uint32_t n_old, const uint32_t* __restrict__ ids, uint32_t m, uint32_t first,
                                                                 float* px, float* py, float* pz, float* smax, float4* geo, float4* sh,
                                                                 uint32_t* state_words) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)m * 16) return;
    const uint32_t g = (uint32_t)(t >> 4), c = (uint32_t)(t & 15u);
    if (c == 15u) {
        if (!state_words || (g & 3u)) return;
        uint32_t w = 0u;
        for (uint32_t k = 0; k < 4u && g + k < m; ++k) {
            const uint32_t id = ids[g + k];
            if (id < n_old) w |= (uint32_t)o.state[id] << (8u * k);
        }
        state_words[g >> 2] = w;
        return;
    }
    const uint32_t id = ids[g];
    if (id >= n_old) return; // (never: ids come from the selection over the old scene)
    const uint64_t d = (uint64_t)first + g;
    if (c == 0u) { px[d] = o.px[id]; py[d] = o.py[id]; pz[d] = o.pz[id]; smax[d] = o.smax[id]; }
    else if (c < 3u) geo[d * 2 + (c - 1u)] = o.geo[(uint64_t)id * 2 + (c - 1u)];
    else sh[d * 12 + (c - 3u)] = o.sh[(uint64_t)id * 12 + (c - 3u)];
}
void gs_launch_compact_planes(const GsScene& o, uint32_t n_old, const uint32_t* ids, uint32_t m, const GsScene& d, hipStream_t st, uint32_t first,
                              bool with_state) {
    const uint64_t total = (uint64_t)m * 16;
    if (!total) return;
    hipLaunchKernelGGL(gs_compact_planes_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, o, n_old, ids, m, first, (float*)d.px,
                       (float*)d.py, (float*)d.pz, (float*)d.smax, (float4*)d.geo, (float4*)d.sh,
                       with_state ? reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(d.state)) : nullptr);
}
