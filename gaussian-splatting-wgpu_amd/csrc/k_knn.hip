// k_knn.hip -- nearest neighbours: for every query splat the k-th smallest squared distance to a source within a radius and the id
// of the nearest source (gs_knn.hip, gs_abi.h "nearest neighbours").  The reference has no counterpart: it is a viewer; an editor on
// it would build a k-d tree over its host records.
//
// The grid, the records, the cell table, the candidates and the slices are the neighbourhoods' (k_neigh.hip, where the geometry is
// argued: everything within r of a query lies in the 27 cells around it; gs_neigh_dev.h: neigh_run); the distance is their expression
// with nothing changed, d = p_j - p_i, (dx dx + dy dy) + dz dz <= r2, one rounding per operation (-ffp-contract=off), self excluded
// by id, a NaN or infinite coordinate failing every comparison.  What is new is what a lane keeps of the accepted candidates:
//
//   init   : a whole search's start, 1 B read and 8 B written per splat: +inf for a query (a query without a record -- a non-finite
//            coordinate -- keeps it), NaN for the others, GS_KNN_NONE.
//   query  : THE HOT KERNEL, in the count query's shape: a wave takes 64 consecutive cell-sorted queries; when all 64 share a cell the
//            9 x-runs' span bounds and the source records are wave-uniform (scalar loads, the record out of SGPRs), otherwise each
//            lane walks its own spans.  Per lane: the k smallest accepted d2 and the (d2, id) minimum.  k is a run-time value, so the
//            k slots are no register array (dynamic indexing would go to scratch): they live in LDS at word slot * 256 + threadIdx.x
//            -- consecutive lanes in consecutive banks, no conflict --, k KB of dynamic LDS per workgroup; the fill, the current worst
//            and its slot stay in registers.  An accepted candidate is inserted while the fill is below k (the worst is kept up on
//            the way, nothing is rescanned) or when d2 < worst: it replaces the worst slot and the k slots are rescanned for the new
//            worst -- rare once the fill has reached k (the expected number of replacements over m candidates in random order is
//            k ln(m / k)).  The (d2, id) minimum is updated on every accepted candidate; a tie takes the smaller id.  Both results are
//            functions of the multiset of accepted d2 and of the order (d2, id): nothing depends on the order of the visit.
//            The result write, then one ballot popcount and one integer atomicAdd per wave for the queries that end +inf.
//            Every loop is bounded by table contents (positions < the record count by construction, a search halves its interval,
//            a rescan reads k slots); no spin, no hand-off between workgroups, no float atomics, no scratch.
//            Bound: VALU issue (uniform path) / L1 gather rate (per-lane path), as the count; the LDS insertions come on top
//            (profiles/nearest.txt).  Registers, LDS and occupancy: gs_knn_query_kernel.
//   state  : the state pass around the dist2 plane read as words (gs_neigh_dev.h: state_plane_pass) with a float-range membership.
#include "gs_neigh_dev.h"

#define KNN_INF 0x7F800000u
#define KNN_NAN 0x7FC00000u
#define KNN_NONE 0xFFFFFFFFu

__global__ __launch_bounds__(256) void gs_knn_init_kernel(const uint8_t* __restrict__ state, uint32_t n, uint32_t mask, uint32_t value,
                                                           uint32_t* __restrict__ dist2, uint32_t* __restrict__ nearest) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t sv = state ? state[i] : 0u;
    dist2[i] = (sv & mask) == value ? KNN_INF : KNN_NAN;
    nearest[i] = KNN_NONE;
}
void gs_launch_knn_init(const uint8_t* state, uint32_t n, uint32_t mask, uint32_t value, uint32_t* dist2, uint32_t* nearest, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_knn_init_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, state, n, mask, value, dist2, nearest);
}

// What a lane keeps: the slots' fill, the largest of them and where it is, the (d2, id) minimum.
struct KnnLane {
    uint32_t fill, wslot;
    float worst, best;
    uint32_t bid;
};
// One accepted candidate (d2 <= r2, id != self).  slots: the lane's column, slot s at slots[s * 256].
__device__ __forceinline__ void knn_take(float* __restrict__ slots, uint32_t k, float d2, uint32_t id, KnnLane& L) {
    if (d2 < L.best || (d2 == L.best && id < L.bid)) { L.best = d2; L.bid = id; }
    if (L.fill < k) {
        slots[L.fill * 256u] = d2;
        if (L.fill == 0u || d2 > L.worst) { L.worst = d2; L.wslot = L.fill; }
        ++L.fill;
    } else if (d2 < L.worst) {
        slots[L.wslot * 256u] = d2;
        float w = slots[0];
        uint32_t ws = 0u;
        for (uint32_t s = 1u; s < k; ++s) {
            const float v = slots[s * 256u];
            if (v > w) { w = v; ws = s; }
        }
        L.worst = w;
        L.wslot = ws;
    }
}
// One span against the lane's query.  UNIFORM: lo / hi are the same in every lane (scalar loads of the records); otherwise each lane
// walks its own.
template <bool UNIFORM>
__device__ __forceinline__ void knn_walk(const float4* __restrict__ srec, uint32_t lo, uint32_t hi, const float4& q, uint32_t qid, float r2, bool live,
                                         float* __restrict__ slots, uint32_t k, KnnLane& L) {
    const auto test = [&](const float4& p) {
        const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const uint32_t id = __float_as_uint(p.w);
        if (d2 <= r2 && id != qid && (!UNIFORM || live)) knn_take(slots, k, d2, id, L);
    };
    uint32_t s = lo;
    if (!UNIFORM) { // four records -- one 64-byte line -- in flight per lane: a refinement's few queries walk long spans, bound by the load's latency
        for (; s + 4u <= hi; s += 4u) {
            const float4 p0 = srec[s], p1 = srec[s + 1u], p2 = srec[s + 2u], p3 = srec[s + 3u];
            test(p0); test(p1); test(p2); test(p3);
        }
    }
    for (; s < hi; ++s) test(srec[s]);
}

// Sorted queries 256 (first_block + blockIdx.x) ...: dist2[id], nearest[id], *unresolved.  Dynamic LDS: k * 1024 bytes.
// 50 VGPRs, 64 SGPRs, no scratch (private segment 0); LDS 8 KB at k = 8 (8 waves per SIMD, the launch bound's limit), 32 KB at k = 32 (5 workgroups of
// the CU's 160 KB: 5 waves per SIMD).
__global__ __launch_bounds__(256) void gs_knn_query_kernel(const float4* __restrict__ qrec, uint32_t nq, uint32_t first_block, NeighSources S, GsNeighGrid g,
                                                            float r2, uint32_t k, uint32_t n, uint32_t* __restrict__ dist2, uint32_t* __restrict__ nearest,
                                                            uint32_t* __restrict__ unresolved) {
    extern __shared__ float s_slots[]; // [k][256]
    float* slots = s_slots + threadIdx.x;
    const uint64_t t64 = ((uint64_t)first_block + blockIdx.x) * 256u + threadIdx.x;
    const bool live = t64 < nq;
    const float4 q = live ? qrec[(uint32_t)t64] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t qid = __float_as_uint(q.w);
    KnnLane L{0u, 0u, 0.0f, __uint_as_float(KNN_INF), KNN_NONE};
    // guarded: nothing would stop a uniform walk of a wave without a query (gs_neigh_dev.h: neigh_visit)
    neigh_visit<true>(S, g, q, live, live, [&](auto uniform, uint32_t lo, uint32_t hi) {
        constexpr bool U = decltype(uniform)::value;
        knn_walk<U>(S.rec, lo, hi, q, qid, r2, !U || live, slots, k, L);
    });
    const bool resolved = L.fill >= k;
    if (live && qid < n) {
        dist2[qid] = resolved ? __float_as_uint(L.worst) : KNN_INF;
        nearest[qid] = L.bid;
    }
    const unsigned long long open = __builtin_amdgcn_ballot_w64(live && !resolved);
    if (open && (threadIdx.x & 63u) == 0u) atomicAdd(unresolved, (uint32_t)__popcll(open));
}
void gs_launch_knn_query(const NeighView& v, uint32_t first_block, uint32_t blocks, float r2, uint32_t k, uint32_t n, uint32_t* dist2, uint32_t* nearest,
                         uint32_t* unresolved, hipStream_t st) {
    if (!blocks || !k || k > 32u) return; // (GS_KNN_MAX_K: gs_knn_search has refused anything else)
    hipLaunchKernelGGL(gs_knn_query_kernel, dim3(blocks), dim3(256), (size_t)k * 1024u, st, v.qrec, v.nqry, first_block, v.src, v.g, r2, k, n, dist2, nearest,
                       unresolved);
}

// gs_state_knn: the state pass around the dist2 plane with the range membership (v >= lo && v <= hi) == inside on the word read as
// f32 -- gs_state_attr's rule: a NaN is in no range.
struct KnnRange {
    float lo, hi;
    bool inside;
    __device__ __forceinline__ bool operator()(uint32_t w) const {
        const float v = __uint_as_float(w);
        return (v >= lo && v <= hi) == inside;
    }
};
__global__ __launch_bounds__(256) void gs_state_knn_kernel(uint8_t* __restrict__ state, const uint32_t* __restrict__ plane, uint32_t n, float lo, float hi,
                                                            uint32_t inside, uint32_t op, uint32_t bits, uint32_t wmask, uint32_t wvalue,
                                                            unsigned long long* __restrict__ matched) {
    state_plane_pass(state, plane, n, KnnRange{lo, hi, inside != 0u}, op, bits, wmask, wvalue, matched);
}
void gs_launch_state_knn(uint8_t* state, const uint32_t* dist2, uint32_t n, float lo, float hi, uint32_t inside, uint32_t op, uint32_t bits,
                         uint32_t where_mask, uint32_t where_value, unsigned long long* matched, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_state_knn_kernel, dim3(state_plane_blocks(n)), dim3(256), 0, st, state, dist2, n, lo, hi, inside, op, bits, where_mask,
                       where_value, matched);
}
