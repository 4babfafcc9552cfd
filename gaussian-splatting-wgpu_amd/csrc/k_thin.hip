// k_thin.hip -- thinning: a maximal set of member splats no two of which are within a radius of each other, chosen in rank order
// (gs_thin.hip, gs_abi.h "thinning").  The reference has no counterpart: it is a viewer; an editor on it would export its records,
// build a k-d tree and run a sequential greedy on the host.
//
// The graph is never built.  Its edges are the hits of the neighbourhoods' candidate walk (k_neigh.hip: the cell grid, the 27 cells,
// the distance expression -- all of it shared through gs_neigh_dev.h).  Everything a pass reads about a candidate lies at the
// candidate's SORTED POSITION, next to its record: rank[s] (u64) and status[s] (u32) for the member whose record is srec[s].  So a
// candidate costs no gather: where the spans are wave-uniform the rank comes through scalar loads with the record, and in the
// per-lane walk it falls into the cache lines the neighbouring lanes touch anyway.  (By splat index it would be an 8-byte and a
// 4-byte gather per accepted pair.)  Members and sources are one set, so a lane's own position is its query index.
//
//   init    : 13 B read (the (0, 0) filter: 12), 8 B written per splat: the work planes keeper / covers by SPLAT INDEX -- a member
//             with a non-finite coordinate is its own keeper with covers 1 (it has no record), everyone else GS_THIN_NONE / 0.
//   rank    : 16 B + (with a priority) a 4 B gather read, 12 B written per sorted member: rank[t], status[t] = 0 (undecided).  The
//             priority values are the attribute kernels' (gs_launch_attr_values, dense): the sixteen kinds are not restated.
//   round   : THE HOT KERNEL, gs_neigh_query_kernel's walk with the decision in place of the count.  See gs_thin_round_kernel.
//   assign  : the same walk once more, for the DROPPED members only: the highest rank among the linked KEPT candidates names the
//             keeper; kept members name themselves; covers by integer atomicAdd, so it is order-free.  The statuses are final and a
//             kernel boundary behind: plain loads.
//   commit  : keeper / covers into the two resident planes, and the info numbers kept and largest (integer sum / max: wave folds,
//             LDS, two global atomics per workgroup).
//
// WHY THE ROUNDS GIVE THE HEADER'S SET WHATEVER A LANE SEES.  A status word is 0 (undecided) or round << 2 | {1 kept, 2 dropped}; it
// is written once, by the one lane that owns the member, with a relaxed agent-scope atomic store, and read with relaxed agent-scope
// atomic loads.  No barrier, no spin, no hand-off between workgroups.
//   * A decided status is FINAL AND CORRECT, by induction on rank: a member becomes DROPPED only on seeing a linked member that
//     outranks it KEPT -- correct by induction, and enough by the header's second rule --, and KEPT only when EVERY linked member
//     that outranks it was seen DROPPED -- each of them correct by induction, the header's first rule.
//   * So a lane may see any mixture of this round's and earlier rounds' stores (workgroups run in any order, a load may be served
//     from a copy another workgroup has long overwritten), and the RESULT cannot depend on it: an undecided reading of a decided word
//     only makes the lane wait.  Only the NUMBER of rounds could depend on it, and the kernel removes that too: a decision stamped
//     with the current round is read as undecided.  Every decision of an earlier round lies behind a kernel boundary and is seen by
//     everyone, so a round decides exactly what a synchronous model decides, `rounds` is a function of the inputs, and a caller who
//     sets max_rounds from an earlier sample's info gets the same answer again.
//   * Each round decides at least the highest-ranked undecided member (every member that outranks it is decided, in earlier rounds),
//     so the host's loop ends; the host reads back one word per round, the members still undecided.
#include "../../include/gsplat/gs_abi.h" // GS_THIN_NONE
#include "gs_neigh_dev.h"
#include "gs_thin_math.h"

#define THIN_KEPT 1u
#define THIN_DROPPED 2u

__global__ __launch_bounds__(256) void gs_thin_init_kernel(const uint8_t* __restrict__ state, const float* __restrict__ px, const float* __restrict__ py,
                                                            const float* __restrict__ pz, uint32_t n, uint32_t mask, uint32_t value,
                                                            uint32_t* __restrict__ keeper, uint32_t* __restrict__ covers) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t sv = state ? state[i] : 0u;
    const bool lone = (sv & mask) == value && !neigh_finite(px[i], py[i], pz[i]);
    keeper[i] = lone ? i : GS_THIN_NONE;
    covers[i] = lone ? 1u : 0u;
}
void gs_launch_thin_init(const uint8_t* state, const GsScene& s, uint32_t n, uint32_t mask, uint32_t value, uint32_t* keeper, uint32_t* covers,
                         hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_thin_init_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, state, s.px, s.py, s.pz, n, mask, value, keeper, covers);
}

__global__ __launch_bounds__(256) void gs_thin_rank_kernel(const float4* __restrict__ rec, uint32_t nrec, uint32_t n, const uint32_t* __restrict__ prio,
                                                            uint32_t flags, uint32_t seed, unsigned long long* __restrict__ rank,
                                                            uint32_t* __restrict__ status) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nrec) return;
    const uint32_t id = __float_as_uint(rec[t].w);
    const bool have = prio != nullptr && id < n; // (id < n always: gs_neigh_records_kernel; keeps the gather inside the plane)
    rank[t] = thin_rank(id, have, have ? prio[id] : 0u, flags, seed);
    status[t] = 0u;
}
void gs_launch_thin_rank(const void* rec, uint32_t nrec, uint32_t n, const float* prio, uint32_t flags, uint32_t seed, unsigned long long* rank,
                         uint32_t* status, hipStream_t st) {
    if (!nrec) return;
    hipLaunchKernelGGL(gs_thin_rank_kernel, dim3((nrec + 255u) / 256u), dim3(256), 0, st, (const float4*)rec, nrec, n, (const uint32_t*)prio, flags, seed,
                       rank, status);
}

// One span against the lane's member in a round.  A hit that outranks the member: KEPT before this round -> the member is dropped
// (and stops looking); not decided before this round -> the member is blocked; DROPPED -> nothing.  UNIFORM: lo / hi are the same in
// every lane, record and rank are read once for the wave, and the span ends when no lane is still looking.
template <bool UNIFORM>
__device__ __forceinline__ void thin_round_walk(const float4* __restrict__ srec, const unsigned long long* __restrict__ rank, const uint32_t* status,
                                                uint32_t lo, uint32_t hi, const float4& q, uint32_t qid, unsigned long long qr, float r2,
                                                uint32_t stamp, bool& look, bool& blocked) {
    for (uint32_t s = lo; s < hi; ++s) {
        if (UNIFORM ? __builtin_amdgcn_ballot_w64(look) == 0ull : !look) break;
        const float4 p = srec[s];
        const uint32_t id = __float_as_uint(p.w);
        const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
        const bool hit = (dx * dx + dy * dy) + dz * dz <= r2 && id != qid && look;
        if (hit && thin_outranks(rank[s], id, qr, qid)) {
            const uint32_t v = ld_agent(status + s);
            const bool before = v != 0u && v < stamp; // decided in an earlier round (this round's stores read as undecided)
            if (!before) blocked = true;
            else if ((v & 3u) == THIN_KEPT) look = false;
        }
    }
}

// Sorted members 256 (first_block + blockIdx.x) ...: one round.  A wave takes 64 consecutive cell-sorted members; decided lanes, and
// whole waves of them (the tail waves of the last workgroup too: so no GUARD -- a wave without an undecided member returns before
// the walk, and the uniform span walk ends by itself at the ballot of the lanes still looking), do no walk.  A lane that ends
// neither dropped nor blocked is kept.  *undecided += the lanes that stay undecided, one atomicAdd per wave that has any.
// Every loop ends on its own data: spans by table contents, a search halves its interval.  No LDS (nothing is shared between lanes
// that the scalar path does not already share), no scratch, no float atomics.
// 31 VGPRs, 106 SGPRs (they, not the VGPRs, set the occupancy), 7 waves per SIMD, no LDS, no scratch.
__global__ __launch_bounds__(256) void gs_thin_round_kernel(uint32_t first_block, NeighSources S, GsNeighGrid g, float r2, uint32_t round,
                                                             const unsigned long long* __restrict__ rank, uint32_t* status, uint32_t* undecided) {
    const uint64_t t64 = ((uint64_t)first_block + blockIdx.x) * 256u + threadIdx.x;
    const bool in = t64 < S.nrec;
    const uint32_t t = in ? (uint32_t)t64 : 0u;
    const bool live = in && ld_agent(status + t) == 0u;
    if (__builtin_amdgcn_ballot_w64(live) == 0ull) return;
    const float4 q = in ? S.rec[t] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t qid = __float_as_uint(q.w);
    const unsigned long long qr = in ? rank[t] : 0ull;
    const uint32_t stamp = round << 2;
    bool look = live, blocked = false;
    neigh_visit<false>(S, g, q, in, live, [&](auto uniform, uint32_t lo, uint32_t hi) {
        constexpr bool U = decltype(uniform)::value;
        thin_round_walk<U>(S.rec, rank, status, lo, hi, q, qid, qr, r2, stamp, look, blocked);
    });
    const bool dropped = live && !look, kept = live && look && !blocked;
    if (dropped || kept) st_agent(status + t, stamp | (kept ? THIN_KEPT : THIN_DROPPED));
    const unsigned long long wait = __builtin_amdgcn_ballot_w64(live && look && blocked);
    if (wait != 0ull && lane_id() == 0u) atomicAdd(undecided, (uint32_t)__builtin_popcountll(wait));
}
void gs_launch_thin_round(const NeighView& v, uint32_t first_block, uint32_t blocks, float r2, uint32_t round, const unsigned long long* rank, uint32_t* status,
                          uint32_t* undecided, hipStream_t st) {
    if (!blocks) return;
    hipLaunchKernelGGL(gs_thin_round_kernel, dim3(blocks), dim3(256), 0, st, first_block, v.src, v.g, r2, round, rank, status, undecided);
}

// One span against a dropped member: the linked KEPT candidate of the highest rank so far.
template <bool UNIFORM>
__device__ __forceinline__ void thin_assign_walk(const float4* __restrict__ srec, const unsigned long long* __restrict__ rank,
                                                 const uint32_t* __restrict__ status, uint32_t lo, uint32_t hi, const float4& q, uint32_t qid, float r2,
                                                 bool live, bool& found, unsigned long long& br, uint32_t& bid) {
    for (uint32_t s = lo; s < hi; ++s) {
        const float4 p = srec[s];
        const uint32_t id = __float_as_uint(p.w);
        const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
        const bool hit = (dx * dx + dy * dy) + dz * dz <= r2 && id != qid && (!UNIFORM || live);
        if (hit && (status[s] & 3u) == THIN_KEPT) {
            const unsigned long long r = rank[s];
            if (!found || thin_outranks(r, id, br, bid)) { br = r; bid = id; }
            found = true;
        }
    }
}

// Sorted members 256 (first_block + blockIdx.x) ...: keeper[id] and covers[keeper] += 1.  A kept member walks nothing; a wave of
// kept members does no walk at all.  (A dropped member always finds a keeper: it was dropped on seeing one.  One that did not --
// impossible -- keeps GS_THIN_NONE and adds nothing.)  Ids at or past n are never an index.
// 36 VGPRs, 102 SGPRs, 7 waves per SIMD, no LDS, no scratch.
__global__ __launch_bounds__(256) void gs_thin_assign_kernel(uint32_t first_block, NeighSources S, GsNeighGrid g, float r2, uint32_t n,
                                                              const unsigned long long* __restrict__ rank, const uint32_t* __restrict__ status,
                                                              uint32_t* __restrict__ keeper, uint32_t* covers) {
    const uint64_t t64 = ((uint64_t)first_block + blockIdx.x) * 256u + threadIdx.x;
    const bool in = t64 < S.nrec;
    const uint32_t t = in ? (uint32_t)t64 : 0u;
    const float4 q = in ? S.rec[t] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t qid = __float_as_uint(q.w);
    const uint32_t mine = in && qid < n ? (status[t] & 3u) : 0u;
    const bool live = mine == THIN_DROPPED;
    bool found = false;
    unsigned long long br = 0ull;
    uint32_t bid = GS_THIN_NONE;
    if (__builtin_amdgcn_ballot_w64(live) != 0ull)
        neigh_visit<false>(S, g, q, in, live, [&](auto uniform, uint32_t lo, uint32_t hi) {
            constexpr bool U = decltype(uniform)::value;
            thin_assign_walk<U>(S.rec, rank, status, lo, hi, q, qid, r2, live, found, br, bid);
        });
    const uint32_t k = mine == THIN_KEPT ? qid : (live && found) ? bid : GS_THIN_NONE;
    if (k < n) {
        keeper[qid] = k;
        atomicAdd(covers + k, 1u);
    }
}
void gs_launch_thin_assign(const NeighView& v, uint32_t first_block, uint32_t blocks, float r2, uint32_t n, const unsigned long long* rank,
                           const uint32_t* status, uint32_t* keeper, uint32_t* covers, hipStream_t st) {
    if (!blocks) return;
    hipLaunchKernelGGL(gs_thin_assign_kernel, dim3(blocks), dim3(256), 0, st, first_block, v.src, v.g, r2, n, rank, status, keeper, covers);
}

// The two planes, and into the GS_STATE_SLOTS partial records `slots` (gs_kernels.h; zeroed by the caller, folded on the host): word 0
// += the members that are their own keeper (kept), word 1 = max(word 1, covers) (largest).  gs_cluster_commit_kernel's folds.
__global__ __launch_bounds__(256) void gs_thin_commit_kernel(const uint32_t* __restrict__ wkeeper, const uint32_t* __restrict__ wcovers, uint32_t n,
                                                              uint32_t* __restrict__ keeper, uint32_t* __restrict__ covers, unsigned long long* __restrict__ slots) {
    __shared__ uint32_t s_fold[2];
    if (threadIdx.x < 2u) s_fold[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t own = 0u, c = 0u;
    if (i < n) {
        const uint32_t k = wkeeper[i];
        c = wcovers[i];
        own = k == i ? 1u : 0u;
        keeper[i] = k < n ? k : GS_THIN_NONE;
        covers[i] = c;
    }
    const uint32_t kept = wave_sum(own), largest = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max(c), 63);
    if (lane_id() == 0u && largest) { // (a wave without a kept member adds nothing)
        if (kept) atomicAdd(&s_fold[0], kept);
        atomicMax(&s_fold[1], largest);
    }
    __syncthreads();
    if (threadIdx.x == 0u && s_fold[1]) {
        unsigned long long* slot = slots + (blockIdx.x % GS_STATE_SLOTS) * GS_STATE_SLOT_STRIDE;
        if (s_fold[0]) atomicAdd(slot, (unsigned long long)s_fold[0]);
        atomicMax(slot + 1, (unsigned long long)s_fold[1]);
    }
}
void gs_launch_thin_commit(const uint32_t* wkeeper, const uint32_t* wcovers, uint32_t n, uint32_t* keeper, uint32_t* covers, unsigned long long* slots,
                           hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_thin_commit_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, wkeeper, wcovers, n, keeper, covers, slots);
}
