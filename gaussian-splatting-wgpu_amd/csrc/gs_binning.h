// gs_binning.h -- the device-side primitives the binning kernels share (k_sort.hip, k_rows.hip, k_gsort.hip, k_binning.hip):
// workgroup scans, the stable in-wave rank by digit with what goes before and after it, the owner walk, the 4-byte look-back.
// A site that still writes one of them out names it and says why (the call compiled to other code: profiles/binning_refactor.txt).
#pragma once
#include "gs_device.h"
#define GS_EMIT_CHUNK_SHIFT 10 // output slots per entry of the chunk table = what one wave of the balanced emission emits at a time
__device__ __forceinline__ uint32_t sat32(unsigned long long v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }
// ---- exclusive scans over a workgroup ------------------------------------------------------------
// Step one: the scan inside the wave; lane 63 leaves the wave's sum in s_w[w].  After the caller's barrier ...
__device__ __forceinline__ uint32_t wave_scan_publish(uint32_t v, uint32_t lane, uint32_t w, uint32_t* s_w) {
    const uint32_t incl = wave_incl_scan(v, lane);
    if (lane == 63) s_w[w] = incl;
    return incl;
}
// ... step two: b + the sums of the waves before w, as a loop over them ...
template <typename A, typename T>
__device__ __forceinline__ A waves_before(const T* s_w, uint32_t w, A b = 0) { for (uint32_t k = 0; k < w; ++k) b += s_w[k]; return b; }
// ... or unrolled over all WAVES, which also gives the workgroup's total.
template <int WAVES, typename A, typename T>
__device__ __forceinline__ A waves_before_total(const T* s_w, uint32_t w, A& total) {
    A base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) { const T t = s_w[k]; if (k < (int)w) base += t; total += t; }
    return base;
}
// Both steps and their barriers (v: the sum of the thread's consecutive elements).  32 bits are enough inside a wave wherever this is used; the sum over the waves can need more (A)
template <int WAVES, typename A>
__device__ __forceinline__ A block_excl_u32(uint32_t v, uint32_t tid, uint32_t* s_w, A& total) {
    const uint32_t iv = wave_scan_publish(v, tid & 63, tid >> 6, s_w);
    __syncthreads();
    const A base = waves_before_total<WAVES, A>(s_w, tid >> 6, total);
    __syncthreads();
    return base + (iv - v);
}
// The same for a (count, quantity) pair; the quantity channel is 64 bits wide inside the scan and saturates where it is stored
struct GsPair { uint32_t x; unsigned long long y; };
template <int WAVES>
__device__ __forceinline__ GsPair block_excl2(GsPair v, uint32_t tid, GsPair* s_w /*[WAVES]*/, GsPair& total) {
    const uint32_t lane = tid & 63, w = tid >> 6;
    const uint32_t ix = wave_incl_scan(v.x, lane);
    const unsigned long long iy = wave_incl_scan64(v.y, lane);
    if (lane == 63) { s_w[w].x = ix; s_w[w].y = iy; }
    __syncthreads();
    GsPair base; base.x = 0u; base.y = 0ull;
    total.x = 0u; total.y = 0ull;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) { const GsPair t = s_w[k]; if (k < (int)w) { base.x += t.x; base.y += t.y; } total.x += t.x; total.y += t.y; }
    __syncthreads();
    GsPair r; r.x = base.x + ix - v.x; r.y = base.y + iy - v.y;
    return r;
}
// ---- stable rank by digit inside a wave.  Digits of a canvas dimension (tile rows or columns, at most 256): slots that hold nothing
// take the digit `hole`, which no row / column has, rank last and are not stored; 127 when the dimension fits 7 bits: one ballot less.
struct GsDigits { uint32_t hole; int nbits; };
__device__ __forceinline__ GsDigits gs_digits(uint32_t ndig) { return GsDigits{ndig < 128u ? 127u : 255u, ndig < 128u ? 7 : 8}; }
// The wave calls these once per item j, in ascending j.  peers (plo, phi) = the lanes that hold the same digit d.  cnt[d] is the
// wave's running count of digit d, so the rank is cnt[d] + the peers in lower lanes: the order is (item, lane), which is stable
// when that is the wave's element order.  The lowest peer advances the count (`on`: this lane holds an item at all).  Every peer
// has read the count before that store is issued and sees it at the next item, with no barrier: one wave, in-order LDS; the two
// wavefront fences only hold the compiler to that order.
template <typename C>
__device__ __forceinline__ uint32_t wave_rank_peers(C* cnt, uint32_t d, uint32_t plo, uint32_t phi, bool on, unsigned long long lt_mask) {
    const uint32_t below = __popc(plo & (uint32_t)lt_mask) + __popc(phi & (uint32_t)(lt_mask >> 32));
    const uint32_t n = __popc(plo) + __popc(phi);
    const uint32_t pre = cnt[d];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (on && below == 0) cnt[d] = (C)(pre + n);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return pre + below;
}
// The peers by NB ballots, one per bit of d, starting from the lanes of (plo, phi); then the rank.  (The row kernels, whose number of
// ballots is a run-time 7 or 8, keep this loop in place: inside a callee the compiler stops folding `bal ^ inv` into the AND.)
template <int NB, typename C>
__device__ __forceinline__ uint32_t wave_rank(C* cnt, uint32_t d, uint32_t plo, uint32_t phi, bool on, unsigned long long lt_mask) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const uint32_t bit = (d >> b) & 1u;
        const unsigned long long bal = __ballot(bit != 0u);
        const uint32_t inv = bit - 1u; // 0 when the bit is set, ~0 when clear: peers &= bit ? bal : ~bal
        plo &= (uint32_t)bal ^ inv;
        phi &= (uint32_t)(bal >> 32) ^ inv;
    }
    return wave_rank_peers(cnt, d, plo, phi, on, lt_mask);
}
// The ranks wait in registers for the reorder, two 16-bit ranks per register (j is a constant after unrolling)
template <int N>
__device__ __forceinline__ void rank2_put(uint32_t (&rank2)[N], int j, uint32_t r) { if (j & 1) rank2[j >> 1] |= r << 16; else rank2[j >> 1] = r; }
template <int N>
__device__ __forceinline__ uint32_t rank2_get(const uint32_t (&rank2)[N], int j) { return (j & 1) ? (rank2[j >> 1] >> 16) : (rank2[j >> 1] & 0xFFFFu); }
// After the ranking hist[k][d] is wave k's count of digit d.  The thread that owns digit d reads the counts (returns their sum) and,
// knowing the digit's first position `run` in the workgroup's sorted order, leaves every wave's start: position = hist[wave][d] + rank.
template <int WAVES>
__device__ __forceinline__ uint32_t wave_counts(const uint32_t (*hist)[256], uint32_t d, uint32_t (&cw)[WAVES]) {
    uint32_t total = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) { cw[k] = hist[k][d]; total += cw[k]; }
    return total;
}
template <int WAVES>
__device__ __forceinline__ void wave_starts(uint32_t (*hist)[256], uint32_t d, uint32_t run, const uint32_t (&cw)[WAVES]) {
#pragma unroll
    for (int k = 0; k < WAVES; ++k) { hist[k][d] = run; run += cw[k]; }
}
// ---- owner walk: mark = k + 1 where owner k's first slot is this lane's slot, else 0; carry = owner + 1 of the slot before the
// wave's 64.  A running maximum hands every slot its owner + 1; lane 63's is the carry of the wave's next 64 slots.
__device__ __forceinline__ uint32_t owner_walk(uint32_t mark, uint32_t& carry) {
    const uint32_t m0 = wave_incl_max(mark), m = m0 > carry ? m0 : carry;
    carry = (uint32_t)__builtin_amdgcn_readlane((int)m, 63);
    return m;
}
// ---- decoupled look-back over 4-byte status words {flag:2, count:30} (k_sort.hip sweep_tile, k_rows.hip gs_rows_sort_kernel) ----
// status[tile * 256 + digit]: a tile publishes its own count of the digit (AGG; tile 0 PREFIX at once) and later the count of all
// tiles up to and including itself (PREFIX).  The aggregate is published BEFORE the tile's ranking: it is all a successor needs, and
// the ranking time then lies between "my aggregate is visible" and "I look at my predecessors'": few words are found unpublished.
// The walk over the predecessors loads LB = 8 words at a time: the loads of one round are independent and in flight together, so
// a walk of k tiles costs ~k/LB L2 round trips instead of k (all resident workgroups start together: the first tiles of a launch
// walk back hundreds of tiles).  Only an unpublished word is polled, in a bounded spin: giving up raises GsControl::fault instead of
// hanging the GPU (every predecessor has started: tickets).  The walk is still written out at both sites: as a function it compiled to other code.
#define GS_LB_AGG (1u << 30)
#define GS_LB_PREFIX (2u << 30)
#define GS_LB_FLAGS (3u << 30)
#define GS_LB_VALUE (~GS_LB_FLAGS)
