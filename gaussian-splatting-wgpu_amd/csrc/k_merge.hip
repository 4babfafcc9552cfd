// k_merge.hip -- the cell merge's kernels (gs_merge.hip, gs_abi.h "cell merge"): one moment-matched splat per grid cell.  The reference
// has no counterpart: it is a viewer; an editor on it would export its 320-byte records and decimate them in a host script.
//
// Every expression of the definition is gs_merge_math.h's, which the host twin compiles too.
//   keys    : 44 B read per splat that passes the filter (12 B position, 32 B geometry; 1 B of state with a filter), 8 B written: (cell
//             key, id); a splat that is not eligible gets the key `none`, sorts last and is never looked at again.  The pairs go
//             through the Onesweep sort (k_sort.hip), stable, ids ascending inside a cell.
//   heads   : 1 B per sorted position: whether a run of equal keys begins there.  The stream compaction of the splat edits
//             (k_export.hip: count, scan, scatter over a byte plane) turns the flags into the list of run begins -- no second scan here.
//   runs    : one thread per run: its length from the next run's begin, whether it is merged (a flag plane again, compacted the same
//             way into the merged runs in ascending key = the group numbering), and eligible / largest / members through LDS and
//             three global integer atomics per workgroup.
//   sums    : THE HOT KERNEL.  One wave per merged group, the members one after the other in ascending id: that order is the definition,
//             so there is no cross-lane, cross-wave or atomic float sum anywhere.  A member's id, position and geometry are wave-uniform
//             (scalar loads through readfirstlane'd addresses); every lane evaluates the member's weight and covariance (VALU work
//             that all 64 lanes share -- cheaper than a broadcast through LDS and a barrier per member); lanes 0 .. 47 each own one SH
//             coefficient, so a member's 192-byte SH row is ONE coalesced load; lanes 48 .. 57 own W, S and M; each lane keeps one
//             f64 accumulator: acc += w * x with x = mg_slot_x(slot).  The next member's id, position, geometry and SH float are
//             loaded before the current one is evaluated.  Per member and wave: 236 B read, five gs_exp, ~150 f32 and ~10 f64 VALU
//             operations.  Bound: VALU issue for long runs, load latency for runs of two or three (hidden by occupancy: no LDS, no
//             scratch).  512 B written per group, one coalesced store.  VGPRs and occupancy: profiles/simplify.txt.
//   finish  : one thread per group: 512 B read, the f64 Jacobi finish, 320 B written as 20 float4.
// Every store is a plain vector store.  Every loop is bounded by a length the host has checked against max_members.
#include "gs_device.h"
#include "gs_kernels.h"
#include "gs_merge_math.h"

__global__ __launch_bounds__(256) void gs_merge_keys_kernel(const uint8_t* __restrict__ state, const float* __restrict__ px, const float* __restrict__ py,
                                                             const float* __restrict__ pz, const float4* __restrict__ geo, uint32_t n, uint32_t mask,
                                                             uint32_t value, GsNeighGrid g, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t sv = state ? state[i] : 0u;
    uint32_t key = g.none;
    if ((sv & mask) == value) {
        const float x = px[i], y = py[i], z = pz[i];
        if (neigh_finite(x, y, z)) {
            const float4 a = geo[(uint64_t)i * 2u], b = geo[(uint64_t)i * 2u + 1u];
            const float gg[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            MgSplat sp;
            if (mg_splat(gg, &sp)) key = neigh_key(g, x, y, z);
        }
    }
    keys[i] = key;
    vals[i] = i;
}
void gs_launch_merge_keys(const uint8_t* state, const GsScene& s, uint32_t n, uint32_t mask, uint32_t value, const GsNeighGrid& g, uint32_t* keys,
                          uint32_t* vals, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_merge_keys_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, state, s.px, s.py, s.pz, s.geo, n, mask, value, g, keys, vals);
}

__global__ __launch_bounds__(256) void gs_merge_heads_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint8_t* __restrict__ flag) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    flag[t] = (t == 0u || keys[t] != keys[t - 1u]) ? 1u : 0u;
}
void gs_launch_merge_heads(const uint32_t* keys, uint32_t n, uint8_t* flag, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_merge_heads_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, keys, n, flag);
}

// stats (zeroed by the caller): [0] eligible, [1] largest run, [2] members of merged runs
__global__ __launch_bounds__(256) void gs_merge_runs_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ heads, uint32_t runs, uint32_t n,
                                                             uint32_t none, uint32_t min_members, uint8_t* __restrict__ flag, uint32_t* __restrict__ stats) {
    __shared__ uint32_t s_o[3];
    if (threadIdx.x < 3u) s_o[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r < runs) {
        const uint32_t b = heads[r], e = r + 1u < runs ? heads[r + 1u] : n;
        uint32_t merged = 0u;
        if (b < e && e <= n && keys[b] < none) { // (always b < e <= n: the heads are ascending positions)
            const uint32_t len = e - b;
            merged = len >= min_members ? 1u : 0u;
            atomicAdd(&s_o[0], len);
            atomicMax(&s_o[1], len);
            if (merged) atomicAdd(&s_o[2], len);
        }
        flag[r] = (uint8_t)merged;
    }
    __syncthreads();
    if (threadIdx.x < 3u) {
        const uint32_t v = s_o[threadIdx.x];
        if (v) { if (threadIdx.x == 1u) atomicMax(&stats[1], v); else atomicAdd(&stats[threadIdx.x], v); }
    }
}
void gs_launch_merge_runs(const uint32_t* keys, const uint32_t* heads, uint32_t runs, uint32_t n, uint32_t none, uint32_t min_members, uint8_t* flag,
                          uint32_t* stats, hipStream_t st) {
    if (!runs) return;
    hipLaunchKernelGGL(gs_merge_runs_kernel, dim3((runs + 255u) / 256u), dim3(256), 0, st, keys, heads, runs, n, none, min_members, flag, stats);
}

// What a wave holds of one member between its loads and its evaluation.
struct MgMember {
    uint32_t id;
    float x, y, z;
    float4 g0, g1;
    float sh;
};
__device__ __forceinline__ MgMember mg_load(const uint32_t* __restrict__ vals, uint32_t t, uint32_t n, const float* __restrict__ px,
                                            const float* __restrict__ py, const float* __restrict__ pz, const float4* __restrict__ geo,
                                            const float* __restrict__ sh, uint32_t lane) {
    MgMember m;
    uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)vals[t]); // wave-uniform: the address of everything below
    if (id >= n) id = n - 1u; // (never: the values are a permutation of 0 .. n; keeps the gathers inside the planes whatever the sort left)
    m.id = id;
    m.x = px[id]; m.y = py[id]; m.z = pz[id];
    m.g0 = geo[(uint64_t)id * 2u]; m.g1 = geo[(uint64_t)id * 2u + 1u];
    m.sh = lane < 48u ? sh[(uint64_t)id * 48u + lane] : 0.0f;
    return m;
}

// Groups first .. first + count of the merged runs: sums[(g - first) * 64 + slot].  group_of / member (either may be null): the
// group's number and a 1 byte at every member's index.  Registers and occupancy: profiles/simplify.txt.
__global__ __launch_bounds__(256) void gs_merge_sums_kernel(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ heads, uint32_t runs,
                                                             const uint32_t* __restrict__ mruns, uint32_t first, uint32_t count, uint32_t nsorted,
                                                             uint32_t n, const float* __restrict__ px, const float* __restrict__ py,
                                                             const float* __restrict__ pz, const float4* __restrict__ geo, const float* __restrict__ sh,
                                                             double* __restrict__ sums, uint32_t* __restrict__ group_of, uint8_t* __restrict__ member) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gl = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (gl >= count) return; // (wave-uniform)
    const uint32_t g = first + gl;
    const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)mruns[g]);
    uint32_t b = 0u, e = 0u;
    if (r < runs) {
        b = (uint32_t)__builtin_amdgcn_readfirstlane((int)heads[r]);
        e = r + 1u < runs ? (uint32_t)__builtin_amdgcn_readfirstlane((int)heads[r + 1u]) : nsorted;
    }
    if (e > nsorted) e = nsorted;
    const uint32_t len = b < e ? e - b : 0u;
    const uint32_t slot = lane < 48u ? MG_SLOT_H + lane : lane < 58u ? lane - 48u : lane; // lanes 58 .. 63: the bookkeeping slots 58 .. 63
    double acc = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
    uint32_t first_id = 0u;
    if (len) {
        MgMember cur = mg_load(vals, b, n, px, py, pz, geo, sh, lane);
        first_id = cur.id;
        c0 = (double)cur.x; c1 = (double)cur.y; c2 = (double)cur.z;
        for (uint32_t m = 0; m < len; ++m) {
            MgMember nxt = cur;
            if (m + 1u < len) nxt = mg_load(vals, b + m + 1u, n, px, py, pz, geo, sh, lane); // in flight while `cur` is evaluated
            const float gg[8] = {cur.g0.x, cur.g0.y, cur.g0.z, cur.g0.w, cur.g1.x, cur.g1.y, cur.g1.z, cur.g1.w};
            MgSplat sp;
            mg_splat(gg, &sp);
            const double w = (double)sp.w;
            const double d0 = (double)cur.x - c0, d1 = (double)cur.y - c1, d2 = (double)cur.z - c2;
            double t = mg_slot_x(slot < MG_SLOT_COUNT ? slot : 0u, d0, d1, d2, sp.sig, cur.sh);
            t = w * t;
            acc += t;
            if (lane == 0u) {
                if (group_of) group_of[cur.id] = g;
                if (member) member[cur.id] = 1u;
            }
            cur = nxt;
        }
    }
    double out = acc;
    if (slot == MG_SLOT_COUNT) out = (double)len;
    else if (slot == MG_SLOT_FIRST) out = (double)first_id;
    else if (slot == MG_SLOT_C) out = c0;
    else if (slot == MG_SLOT_C + 1u) out = c1;
    else if (slot == MG_SLOT_C + 2u) out = c2;
    else if (slot == 63u) out = 0.0;
    sums[(uint64_t)gl * GS_MERGE_SUM_DOUBLES + slot] = out;
}
void gs_launch_merge_sums(const uint32_t* vals, const uint32_t* heads, uint32_t runs, const uint32_t* mruns, uint32_t first, uint32_t count,
                          uint32_t nsorted, const GsScene& s, uint32_t n, double* sums, uint32_t* group_of, uint8_t* member, hipStream_t st) {
    if (!count || !n) return;
    hipLaunchKernelGGL(gs_merge_sums_kernel, dim3((count + 3u) / 4u), dim3(256), 0, st, vals, heads, runs, mruns, first, count, nsorted, n, s.px, s.py,
                       s.pz, s.geo, (const float*)s.sh, sums, group_of, member);
}

__global__ __launch_bounds__(256) void gs_merge_finish_kernel(const double* __restrict__ sums, uint32_t count, float4* __restrict__ aos) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= count) return;
    double s[GS_MERGE_SUM_DOUBLES];
    const double2* src = reinterpret_cast<const double2*>(sums + (uint64_t)g * GS_MERGE_SUM_DOUBLES);
#pragma unroll
    for (int k = 0; k < 32; ++k) { const double2 v = src[k]; s[2 * k] = v.x; s[2 * k + 1] = v.y; }
    float rec[80];
    mg_finish(s, rec);
#pragma unroll
    for (int k = 0; k < 20; ++k) aos[(uint64_t)g * 20u + k] = make_float4(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
}
void gs_launch_merge_finish(const double* sums, uint32_t count, void* d_aos, hipStream_t st) {
    if (!count) return;
    hipLaunchKernelGGL(gs_merge_finish_kernel, dim3((count + 255u) / 256u), dim3(256), 0, st, sums, count, (float4*)d_aos);
}
