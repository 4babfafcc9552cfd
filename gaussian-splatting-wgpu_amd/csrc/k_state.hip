// k_state.hip -- the state plane's streaming kernels: region, coverage and id selection, counting (gs_state.hip, gs_abi.h
// "splat state").  The reference has no counterpart: it is a viewer, and an editor built on it would re-upload its records.
//
// The plane is u8[N], 256-byte aligned like the position planes (gs_context.hip scene_alloc).  Every write goes through the 32-bit
// word that holds the byte: the region kernel owns whole words (one thread per four consecutive splats), the id kernel uses word
// atomics, so no byte read-modify-write ever races with a neighbour.
//   region : 13 B read per splat (3 x 4 B position, 1 B state), at most 1 B written.  Bound: HBM.  No MFMA (no contraction).
//   coverage : the same pass, 17 B read per splat (a 16 B coverage record, 1 B state).
//   ids    : one word atomic (two for ASSIGN) per id.  Bound: atomic latency; the lists are a click or a lasso, not the scene.
//   count  : 1 B read per splat.
#include "gs_device.h"
#include "gs_kernels.h"
#include "gs_state_sum.h"

// Membership of one centre (gs_abi.h: one rounding per operation, the projection's own expression tree for ph, pv, px, py).
template <int KIND>
__device__ __forceinline__ bool state_member(const GsRegionDev& r, float x, float y, float z) {
    if (KIND == 0) return true;
    if (KIND == 1) {
        const float dx = x - r.a[0], dy = y - r.a[1], dz = z - r.a[2];
        return (dx * dx + dy * dy) + dz * dz <= r.b[0] * r.b[0];
    }
    if (KIND == 2) return x >= r.a[0] && x <= r.b[0] && y >= r.a[1] && y <= r.b[1] && z >= r.a[2] && z <= r.b[2];
    const float* m = r.proj;
    const float phx = ((m[0] * x + m[4] * y) + m[8] * z) + m[12];
    const float phy = ((m[1] * x + m[5] * y) + m[9] * z) + m[13];
    const float phw = ((m[3] * x + m[7] * y) + m[11] * z) + m[15];
    const float pvz = ((r.viewz[0] * x + r.viewz[1] * y) + r.viewz[2] * z) + r.viewz[3];
    const float pw = 1.0f / (phw + 0.0000001f);
    const float px = ((phx * pw) * 0.5f + 0.5f) * r.W, py = ((phy * pw) * 0.5f + 0.5f) * r.H;
    if (pvz <= 0.2f) return false;
    if (KIND == 3) return px >= r.x0 && px < r.x1 && py >= r.y0 && py < r.y1;
    if (!(px >= 0.0f && px < r.W && py >= 0.0f && py < r.H)) return false; // (a NaN fails here: no index is formed from it)
    const uint32_t ix = (uint32_t)(int)px, iy = (uint32_t)(int)py;
    if (ix >= r.wi || iy >= r.hi) return false; // cannot happen after the float tests; keeps the gather inside the mask whatever W, H are
    return r.mask[(uint64_t)iy * r.wi + ix] != 0;
}

// The kernels' `matched` / `count` go through state_block_begin / state_block_add (gs_state_sum.h).

// The state pass, which the region and the coverage kernel both are, around their own membership test: thread q owns splats
// 4q .. 4q+3, i.e. one whole word of the plane, so no byte read-modify-write races with a neighbour.  A splat with
// (s & wmask) == wvalue that is a member takes the op; the word is stored only if it changed.  The last thread of a plane whose
// length is no multiple of four reads and writes its splats one by one: nothing past N is touched.  (Written out twice: as one
// function template around a membership callable the kernels' code changes and the sphere and box kernels come out 4 % slower,
// profiles/resident_calls_refactor.txt.)
// Region: 13 B read per splat, a whole quad's positions as three float4.
template <int KIND>
__global__ __launch_bounds__(256) void gs_state_region_kernel(uint8_t* __restrict__ state, const float* __restrict__ px, const float* __restrict__ py,
                                                               const float* __restrict__ pz, uint32_t n, GsRegionDev r, uint32_t op, uint32_t bits,
                                                               uint32_t wmask, uint32_t wvalue, unsigned long long* __restrict__ matched) {
    state_block_begin();
    const uint32_t q = blockIdx.x * 256u + threadIdx.x; // splats 4q .. 4q+3
    const uint64_t first = (uint64_t)q * 4u;
    uint32_t hits = 0;
    if (first + 4u <= n) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(state)[q];
        float X[4], Y[4], Z[4];
        if (KIND != 0) {
            const float4 x4 = reinterpret_cast<const float4*>(px)[q], y4 = reinterpret_cast<const float4*>(py)[q], z4 = reinterpret_cast<const float4*>(pz)[q];
            X[0] = x4.x; X[1] = x4.y; X[2] = x4.z; X[3] = x4.w;
            Y[0] = y4.x; Y[1] = y4.y; Y[2] = y4.z; Y[3] = y4.w;
            Z[0] = z4.x; Z[1] = z4.y; Z[2] = z4.z; Z[3] = z4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) X[k] = Y[k] = Z[k] = 0.0f;
        }
        uint32_t nw = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t sv = (w >> (8 * k)) & 0xFFu;
            const bool in = ((sv & wmask) == wvalue) && state_member<KIND>(r, X[k], Y[k], Z[k]);
            hits += in ? 1u : 0u;
            nw |= (in ? gs_state_apply(sv, op, bits) : sv) << (8 * k);
        }
        if (nw != w) reinterpret_cast<uint32_t*>(state)[q] = nw; // stored only if it changed
    } else if (first < n) {
        for (uint64_t i = first; i < n; ++i) {
            const uint32_t sv = state[i];
            const bool in = ((sv & wmask) == wvalue) && state_member<KIND>(r, KIND ? px[i] : 0.0f, KIND ? py[i] : 0.0f, KIND ? pz[i] : 0.0f);
            hits += in ? 1u : 0u;
            const uint32_t nv = in ? gs_state_apply(sv, op, bits) : sv;
            if (nv != sv) state[i] = (uint8_t)nv;
        }
    }
    state_block_add(hits, matched);
}

void gs_launch_state_region(uint32_t kind, uint8_t* state, const GsScene& s, uint32_t n, const GsRegionDev& r, uint32_t op, uint32_t bits,
                            uint32_t where_mask, uint32_t where_value, unsigned long long* matched, hipStream_t st) {
    if (!n) return;
    const uint32_t quads = (n + 3u) / 4u, blocks = (quads + 255u) / 256u;
#define GS_STATE_LAUNCH(K) hipLaunchKernelGGL(gs_state_region_kernel<K>, dim3(blocks), dim3(256), 0, st, state, s.px, s.py, s.pz, n, r, op, bits, where_mask, where_value, matched)
    switch (kind) {
    case 0: GS_STATE_LAUNCH(0); break;
    case 1: GS_STATE_LAUNCH(1); break;
    case 2: GS_STATE_LAUNCH(2); break;
    case 3: GS_STATE_LAUNCH(3); break;
    default: GS_STATE_LAUNCH(4); break;
    }
#undef GS_STATE_LAUNCH
}

// gs_state_coverage: the same pass around the coverage planes' record (gs_coverage_rec: hits @8, max_weight @12), 17 B read per
// splat -- the state word and four 16-byte records.
__device__ __forceinline__ bool cover_member(uint4 rec, uint32_t min_hits, float min_weight, bool covered) {
    return (rec.z >= min_hits && __uint_as_float(rec.w) >= min_weight) == covered;
}
__global__ __launch_bounds__(256) void gs_state_coverage_kernel(uint8_t* __restrict__ state, const uint4* __restrict__ planes, uint32_t n, uint32_t min_hits,
                                                                 float min_weight, uint32_t covered, uint32_t op, uint32_t bits, uint32_t wmask,
                                                                 uint32_t wvalue, unsigned long long* __restrict__ matched) {
    state_block_begin();
    const uint32_t q = blockIdx.x * 256u + threadIdx.x; // splats 4q .. 4q+3
    const uint64_t first = (uint64_t)q * 4u;
    const bool cov = covered != 0u;
    uint32_t hits = 0;
    if (first + 4u <= n) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(state)[q];
        uint32_t nw = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t sv = (w >> (8 * k)) & 0xFFu;
            const bool in = ((sv & wmask) == wvalue) && cover_member(planes[first + k], min_hits, min_weight, cov);
            hits += in ? 1u : 0u;
            nw |= (in ? gs_state_apply(sv, op, bits) : sv) << (8 * k);
        }
        if (nw != w) reinterpret_cast<uint32_t*>(state)[q] = nw; // stored only if it changed
    } else if (first < n) {
        for (uint64_t i = first; i < n; ++i) {
            const uint32_t sv = state[i];
            const bool in = ((sv & wmask) == wvalue) && cover_member(planes[i], min_hits, min_weight, cov);
            hits += in ? 1u : 0u;
            const uint32_t nv = in ? gs_state_apply(sv, op, bits) : sv;
            if (nv != sv) state[i] = (uint8_t)nv;
        }
    }
    state_block_add(hits, matched);
}
void gs_launch_state_coverage(uint8_t* state, const void* planes, uint32_t n, uint32_t min_hits, float min_weight, uint32_t covered, uint32_t op,
                              uint32_t bits, uint32_t where_mask, uint32_t where_value, unsigned long long* matched, hipStream_t st) {
    if (!n) return;
    const uint32_t quads = (n + 3u) / 4u, blocks = (quads + 255u) / 256u;
    hipLaunchKernelGGL(gs_state_coverage_kernel, dim3(blocks), dim3(256), 0, st, state, (const uint4*)planes, n, min_hits, min_weight, covered, op, bits,
                       where_mask, where_value, matched);
}

// One thread per id; the byte is reached through atomics on its word.  Every operation commutes with itself, so duplicates end
// where the sequential application ends: OR / AND are idempotent, XOR twice is the identity, and ASSIGN is an AND that clears
// the bits not in `bits` followed by an OR that sets those in it -- in whatever order several threads interleave the two.
__global__ __launch_bounds__(256) void gs_state_ids_kernel(uint32_t* __restrict__ words, const uint32_t* __restrict__ ids, uint64_t n, uint32_t op,
                                                            uint32_t bits) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const uint32_t id = ids[t], sh = (id & 3u) * 8u;
    uint32_t* w = words + (id >> 2);
    if (op == 1u) atomicOr(w, bits << sh);
    else if (op == 2u) atomicAnd(w, ~(bits << sh));
    else if (op == 3u) atomicXor(w, bits << sh);
    else {
        atomicAnd(w, ~((0xFFu & ~bits) << sh));
        atomicOr(w, bits << sh);
    }
}
void gs_launch_state_ids(uint8_t* state, const uint32_t* ids, uint64_t n, uint32_t op, uint32_t bits, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_state_ids_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, st, reinterpret_cast<uint32_t*>(state), ids, n, op, bits);
}

// Splats with (s & mask) == value: one thread per 16 bytes, the tail byte by byte.
__global__ __launch_bounds__(256) void gs_state_count_kernel(const uint8_t* __restrict__ state, uint32_t n, uint32_t mask, uint32_t value,
                                                              unsigned long long* __restrict__ count) {
    state_block_begin();
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const uint64_t first = (uint64_t)q * 16u;
    uint32_t hits = 0;
    if (first + 16u <= n) {
        const uint4 v = reinterpret_cast<const uint4*>(state)[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) hits += ((((w[j] >> (8 * k)) & 0xFFu) & mask) == value) ? 1u : 0u;
    } else if (first < n) {
        for (uint64_t i = first; i < n; ++i) hits += (((uint32_t)state[i] & mask) == value) ? 1u : 0u;
    }
    state_block_add(hits, count);
}
void gs_launch_state_count(const uint8_t* state, uint32_t n, uint32_t mask, uint32_t value, unsigned long long* count, hipStream_t st) {
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + 16u * 256u - 1u) / (16u * 256u));
    hipLaunchKernelGGL(gs_state_count_kernel, dim3(blocks), dim3(256), 0, st, state, n, mask, value, count);
}
