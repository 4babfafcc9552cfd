// k_cluster.hip -- clusters: the connected components of "within a radius of each other" over the member splats (gs_cluster.hip,
// gs_abi.h "clusters").  The reference has no counterpart: it is a viewer; an editor on it would run a union-find over a k-d tree of
// its host records.
//
// The graph is never built.  Its edges are the hits of the neighbourhoods' candidate walk (k_neigh.hip: the cell grid, the 27 cells,
// the distance expression -- all of it shared through gs_neigh_dev.h), and every hit is fed to a concurrent union-find over
//     parent[i], one u32 per splat, indexed by SPLAT INDEX:  a member starts as its own root (parent[i] = i), a non-member holds
//     GS_CLUSTER_NONE and is never reached (it has no record in the sorted arrays).
// INVARIANT: parent[x] <= x, and a word only ever decreases.  So a find -- follow parent until parent[x] == x -- strictly descends
// and ends after at most x steps whatever it reads; a node that has stopped being a root never becomes one again; and the root of a
// finished tree is the smallest index in it, which is the label the header promises.
//
//   init    : 13 B read (the (0, 0) filter: 12), 8 B written per splat: parent, and the size counter -- 1 for a member with a
//             non-finite coordinate (a singleton nobody links to), 0 otherwise.
//   edges   : THE HOT KERNEL, gs_neigh_query_kernel's walk with a union in place of the count.  See gs_cluster_edges_kernel.
//   flatten : parent[i] = find(i) for every sorted member.  No root changes during this kernel (it stores to non-roots only), so every
//             find ends at the true root however stale the rest of what it reads is (an old parent is still an ancestor).  Bounded
//             by the tree's depth.  Plain loads and stores, no atomics: thread t alone writes the word of its member.
//   sizes   : integer atomicAdds onto the roots' counters, one per distinct root and WAVE: the lanes that share a root go through
//             one ballot and one add of their popcount.  Members arrive in cell order, so in a large cluster that is nearly
//             every lane: a scene-wide cluster costs N / 64 adds on its one word instead of N (profiles/clusters.txt).
//   commit  : label[i] = parent[i], size[i] = counter[parent[i]] (0 for a non-member) into the two resident planes, and the
//             info numbers clusters and largest (integer sum / max: wave folds, LDS, two global atomics per workgroup).
//   seeds   : gs_state_cluster_linked's first pass: flag[label[i]] = 1 for every seed i.  Every writer stores the same value.
//   state   : the state pass around a u32 plane (gs_neigh_dev.h) with the membership "my label's flag is set".
//
// WHAT THE EDGE PASS MAY AND MAY NOT ASSUME.  Workgroups of one launch run in any order, on any XCD, and a load may return a value
// that another workgroup has long overwritten (the vector L1 is per CU and never refreshed, the L2 is per XCD).  Nothing here waits
// for another wave, and nothing depends on a fresh view:
//   * every WRITE of parent[] in the edge pass is a device-scope atomic (CAS for a hook, min for the compression), so no write is
//     lost or torn and the words stay monotone;
//   * a stale READ returns an earlier value of the word, which is a node the splat was hooked under at some time: an ancestor, in
//     the same component.  A find over stale words therefore ends at SOME node of the right component, not necessarily its root;
//   * the hook is atomicCAS(&parent[hi], hi, lo): it succeeds only if hi is a root at that instant (the CAS is exact whatever
//     the loads saw), and then puts a root under a smaller node of a component it is really linked to -- never a wrong union.
//     When it fails it returns the word's present value, below hi: the pair goes on from there, so the larger of the two nodes
//     strictly decreases from one attempt to the next -- a retry happens only after the word it looked at decreased;
//   * staleness can cost retries, never the answer.  The host does not even rely on that: it runs the pass again after the kernel
//     boundary (where every cache is current) and stops only when a whole pass hooked nothing -- in such a pass nothing was
//     written, every read was exact, and every edge found both its ends under one root.
// The edge pass uses vector atomics and vector stores only: no float atomics, no LDS, no scratch.
#include "../../include/gsplat/gs_abi.h" // GS_CLUSTER_NONE
#include "gs_neigh_dev.h"

// Follows parent from x to a node that is its own parent.  p >= x ends the walk: p == x is a root, p > x cannot happen (and would be
// GS_CLUSTER_NONE's non-member, which no record names).  x only decreases, so x < n throughout when it was at the start.
__device__ __forceinline__ uint32_t cluster_find(const uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = ld_agent(parent + x); // (past the L1: a fresher view costs nothing and saves retries; correctness does not need it)
        if (p >= x) return x;
        x = p;
    }
}
// Joins the trees of a and b; returns a node both are now under.  hooked: a root was put under another node.
__device__ __forceinline__ uint32_t cluster_union(uint32_t* parent, uint32_t a, uint32_t b, bool& hooked) {
    a = cluster_find(parent, a);
    b = cluster_find(parent, b);
    while (a != b) {
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(parent + hi, hi, lo); // device scope
        if (old >= hi) { // == hi: hooked (> hi cannot happen: the words only decrease)
            hooked = true;
            return lo;
        }
        a = cluster_find(parent, old); // parent[hi] had dropped to old < hi: max(a, b) <= max(old, lo) < hi
        b = cluster_find(parent, lo);
    }
    return a;
}

__global__ __launch_bounds__(256) void gs_cluster_init_kernel(const uint8_t* __restrict__ state, const float* __restrict__ px, const float* __restrict__ py,
                                                               const float* __restrict__ pz, uint32_t n, uint32_t mask, uint32_t value,
                                                               uint32_t* __restrict__ parent, uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t sv = state ? state[i] : 0u;
    const bool member = (sv & mask) == value;
    parent[i] = member ? i : GS_CLUSTER_NONE;
    count[i] = (member && !neigh_finite(px[i], py[i], pz[i])) ? 1u : 0u;
}
void gs_launch_cluster_init(const uint8_t* state, const GsScene& s, uint32_t n, uint32_t mask, uint32_t value, uint32_t* parent, uint32_t* count,
                            hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_cluster_init_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, state, s.px, s.py, s.pz, n, mask, value, parent, count);
}

// One span against the lane's member: a hit on a record with a SMALLER index is an edge (d2 is symmetric: the pair is seen from its
// larger end only, and never from a splat to itself).  `cur` is a node the lane's member is known to be under; it only moves down.
// UNIFORM: lo / hi are the same in every lane and the record is read once for the wave; the union itself is per lane.
template <bool UNIFORM>
__device__ __forceinline__ void cluster_walk(const float4* __restrict__ srec, uint32_t lo, uint32_t hi, const float4& q, uint32_t qid, float r2, bool live,
                                             uint32_t* parent, uint32_t& cur, bool& hooked) {
    for (uint32_t s = lo; s < hi; ++s) {
        const float4 p = srec[s];
        const uint32_t id = __float_as_uint(p.w);
        const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
        const bool hit = (dx * dx + dy * dy) + dz * dz <= r2 && id < qid && (!UNIFORM || live);
        if (hit) cur = cluster_union(parent, cur, id, hooked);
    }
}

// Sorted members 256 (first_block + blockIdx.x) ...: every member is joined with every member of a smaller index within the radius.
// A wave takes 64 consecutive cell-sorted members; when they share a cell the spans and their records are wave-uniform (read once
// per wave), otherwise each lane walks its own spans -- gs_neigh_query_kernel's two paths.  A lane carries `cur`, the lowest node
// it has seen its member under, so that a candidate of the same tree costs one find of the candidate and one load of parent[cur];
// at the end it hangs the member directly under cur (atomicMin: a compression, never a hook -- cur < qid means the member had
// already stopped being a root when cur was found above it).  The round's `changed` word takes one atomicOr per wave that hooked.
// Every loop ends on its own data: spans by table contents, finds by descent, the CAS retry by the decrease of the word it read.
// 28 VGPRs, 88 SGPRs, 8 waves per SIMD, no LDS, no scratch.
__global__ __launch_bounds__(256) void gs_cluster_edges_kernel(const float4* __restrict__ qrec, uint32_t nq, uint32_t first_block, NeighSources S, GsNeighGrid g,
                                                                float r2, uint32_t n, uint32_t* parent, uint32_t* changed) {
    const uint64_t t64 = ((uint64_t)first_block + blockIdx.x) * 256u + threadIdx.x;
    const float4 q = t64 < nq ? qrec[(uint32_t)t64] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t qid = __float_as_uint(q.w);
    const bool live = t64 < nq && qid < n; // (qid < n always: gs_neigh_records_kernel; keeps every index inside parent[] whatever the records hold)
    uint32_t cur = live ? qid : 0u;
    bool hooked = false;
    // unguarded, as it always was (gs_neigh_dev.h: neigh_visit): a tail wave without a member walks the origin's cell, every union masked
    neigh_visit<false>(S, g, q, t64 < nq, live, [&](auto uniform, uint32_t lo, uint32_t hi) {
        constexpr bool U = decltype(uniform)::value;
        cluster_walk<U>(S.rec, lo, hi, q, qid, r2, !U || live, parent, cur, hooked);
    });
    if (live && cur < qid) atomicMin(parent + qid, cur);
    if (__builtin_amdgcn_ballot_w64(hooked) != 0ull && lane_id() == 0u) atomicOr(changed, 1u);
}
void gs_launch_cluster_edges(const NeighView& v, uint32_t first_block, uint32_t blocks, float r2, uint32_t n, uint32_t* parent, uint32_t* changed,
                             hipStream_t st) {
    if (!blocks) return;
    hipLaunchKernelGGL(gs_cluster_edges_kernel, dim3(blocks), dim3(256), 0, st, v.src.rec, v.src.nrec, first_block, v.src, v.g, r2, n, parent, changed);
}

__global__ __launch_bounds__(256) void gs_cluster_flatten_kernel(const float4* __restrict__ rec, uint32_t nrec, uint32_t n, uint32_t* parent) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nrec) return;
    const uint32_t id = __float_as_uint(rec[t].w);
    if (id >= n) return;
    uint32_t x = id;
    for (;;) { // (a plain load: the roots do not change in this kernel, and any earlier value of a word names an ancestor)
        const uint32_t p = parent[x];
        if (p >= x) break;
        x = p;
    }
    if (x < id) parent[id] = x;
}
void gs_launch_cluster_flatten(const void* rec, uint32_t nrec, uint32_t n, uint32_t* parent, hipStream_t st) {
    if (!nrec) return;
    hipLaunchKernelGGL(gs_cluster_flatten_kernel, dim3((nrec + 255u) / 256u), dim3(256), 0, st, (const float4*)rec, nrec, n, parent);
}

// count[root] += the sorted members under it.  FOLD: the wave takes the root of its first lane that is still to be counted, the lanes
// that share it go through one ballot and one add of their popcount, and so on until no lane is left: one add per distinct root and
// wave (at most 64 turns of a scalar loop; one or two where a large cluster fills the wave).
template <bool FOLD>
__global__ __launch_bounds__(256) void gs_cluster_sizes_kernel(const float4* __restrict__ rec, uint32_t nrec, uint32_t n, const uint32_t* __restrict__ parent,
                                                                uint32_t* __restrict__ count) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t id = t < nrec ? __float_as_uint(rec[t].w) : GS_CLUSTER_NONE;
    const uint32_t root = id < n ? parent[id] : GS_CLUSTER_NONE;
    const bool live = root < n; // (always, for a record: the trees are flat and their roots are members)
    if (FOLD) {
        const uint32_t lane = lane_id();
        for (unsigned long long todo = __builtin_amdgcn_ballot_w64(live); todo != 0ull;) {
            const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
            const uint32_t r = gs_bcast(root, (int)leader);
            const unsigned long long m = __builtin_amdgcn_ballot_w64(live && root == r);
            if (lane == leader) atomicAdd(count + r, (uint32_t)__builtin_popcountll(m));
            todo &= ~m;
        }
    } else if (live) {
        atomicAdd(count + root, 1u);
    }
}
void gs_launch_cluster_sizes(const void* rec, uint32_t nrec, uint32_t n, const uint32_t* parent, uint32_t* count, bool fold, hipStream_t st) {
    if (!nrec) return;
    const dim3 grid((nrec + 255u) / 256u);
    if (fold) hipLaunchKernelGGL(gs_cluster_sizes_kernel<true>, grid, dim3(256), 0, st, (const float4*)rec, nrec, n, parent, count);
    else hipLaunchKernelGGL(gs_cluster_sizes_kernel<false>, grid, dim3(256), 0, st, (const float4*)rec, nrec, n, parent, count);
}

// The two planes, and into the GS_STATE_SLOTS partial records `slots` (gs_kernels.h; zeroed by the caller, folded on the host): word 0
// += the members that are their own label (clusters), word 1 = max(word 1, size) (largest).  Wave folds, two LDS atomics per wave,
// two global atomics per workgroup spread over the slots: one word would take every workgroup's atomic in turn.
__global__ __launch_bounds__(256) void gs_cluster_commit_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ count, uint32_t n,
                                                                 uint32_t* __restrict__ labels, uint32_t* __restrict__ sizes, unsigned long long* __restrict__ slots) {
    __shared__ uint32_t s_fold[2];
    if (threadIdx.x < 2u) s_fold[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t own = 0u, size = 0u;
    if (i < n) {
        const uint32_t l = parent[i];
        size = l < n ? count[l] : 0u;
        own = l == i ? 1u : 0u;
        labels[i] = l < n ? l : GS_CLUSTER_NONE;
        sizes[i] = size;
    }
    const uint32_t roots = wave_sum(own), largest = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max(size), 63);
    if (lane_id() == 0u && largest) { // (a wave without a member adds nothing)
        if (roots) atomicAdd(&s_fold[0], roots);
        atomicMax(&s_fold[1], largest);
    }
    __syncthreads();
    if (threadIdx.x == 0u && s_fold[1]) {
        unsigned long long* slot = slots + (blockIdx.x % GS_STATE_SLOTS) * GS_STATE_SLOT_STRIDE;
        if (s_fold[0]) atomicAdd(slot, (unsigned long long)s_fold[0]);
        atomicMax(slot + 1, (unsigned long long)s_fold[1]);
    }
}
void gs_launch_cluster_commit(const uint32_t* parent, const uint32_t* count, uint32_t n, uint32_t* labels, uint32_t* sizes, unsigned long long* slots,
                              hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_cluster_commit_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, parent, count, n, labels, sizes, slots);
}

__global__ __launch_bounds__(256) void gs_cluster_seeds_kernel(const uint8_t* __restrict__ state, const uint32_t* __restrict__ labels, uint32_t n, uint32_t mask,
                                                                uint32_t value, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = labels[i];
    if (l < n && ((uint32_t)state[i] & mask) == value) flag[l] = 1u;
}
void gs_launch_cluster_seeds(const uint8_t* state, const uint32_t* labels, uint32_t n, uint32_t mask, uint32_t value, uint32_t* flag, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_cluster_seeds_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, state, labels, n, mask, value, flag);
}

// gs_state_cluster_linked's second pass: the state pass around the LABEL plane; a splat is in when its label's flag is set.
struct ClusterLinked {
    const uint32_t* __restrict__ flag;
    uint32_t n;
    __device__ __forceinline__ bool operator()(uint32_t l) const { return l < n && flag[l] != 0u; }
};
__global__ __launch_bounds__(256) void gs_state_cluster_linked_kernel(uint8_t* __restrict__ state, const uint32_t* __restrict__ labels, uint32_t n,
                                                                       const uint32_t* __restrict__ flag, uint32_t op, uint32_t bits, uint32_t wmask,
                                                                       uint32_t wvalue, unsigned long long* __restrict__ matched) {
    state_plane_pass(state, labels, n, ClusterLinked{flag, n}, op, bits, wmask, wvalue, matched);
}
void gs_launch_state_cluster_linked(uint8_t* state, const uint32_t* labels, uint32_t n, const uint32_t* flag, uint32_t op, uint32_t bits, uint32_t where_mask,
                                    uint32_t where_value, unsigned long long* matched, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_state_cluster_linked_kernel, dim3(state_plane_blocks(n)), dim3(256), 0, st, state, labels, n, flag, op, bits, where_mask, where_value,
                       matched);
}
