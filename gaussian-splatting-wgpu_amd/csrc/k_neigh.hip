// k_neigh.hip -- neighbourhoods: for every query splat, how many source splats lie within a radius (gs_neigh.hip, gs_abi.h
// "neighbourhoods").  The reference has no counterpart: it is a viewer; an editor on it would build a k-d tree over its host records.
//
// A uniform cell grid over the sources does the work.  The cell coordinate of x on one axis is
//     c(x) = (int)min(max(floorf((x - lo) * inv_h), 0), G - 1)
// for sources and queries alike.  Every step of it is monotone in x (an f32 subtraction of one constant, a product with one positive
// constant, floorf, the clamp), so x1 <= x2 gives c(x1) <= c(x2) whatever the box [lo, lo + G h) is.  Two coordinates that differ by
// at most r have (x - lo) * inv_h at most r / h + e apart, e the rounding of the expression: the grid spans at most 1024 cells per
// axis (the host grows h until it does), so each of the two roundings is below 1025 * 2^-24 < 1e-4 cells and e < 4e-4.  With
// h >= 1.001 r the two values are less than one apart, the floors differ by at most one, and the clamp, monotone too, keeps that.
// (A coordinate more than 1025 cells outside the box has no partner within r inside it on that axis.)  So a neighbour of a query
// always sits in one of the 27 cells around the query's, and CORRECTNESS NEVER DEPENDS ON THE BOX, only speed does: a far outlier
// coarsens the grid, nothing else.
//
// The cell key packs the coordinates, x lowest: key = cz << (bx + by) | cy << bx | cx with bx, by the bits of Gx - 1, Gy - 1.  Up to
// 1024^3 cells is more than a table can hold, so the {start, end} table is indexed by key >> shift (at most 2^24 entries: a BLOCK
// of 2^shift consecutive keys, part of one x-row for the usual shift) and a cell's run inside its block is found by two binary
// searches over the block's sorted keys.  With shift = 0 (up to 2^24 cells) a block is a cell and nothing is searched.
//
// The distance test is the SPHERE region's expression, d = p_j - p_i, (dx dx + dy dy) + dz dz <= r2 (one rounding per operation:
// -ffp-contract=off), symmetric in i and j; a NaN or infinite coordinate fails every comparison.  Self is excluded by id.
//
//   bounds  : 13 B read per splat; integer min / max of order-preserving keys and four counts (LDS, then 10 global atomics a workgroup).
//   keys    : 13 B read, 8 B written per splat: (cell key, id); a splat that fails the filter or has a non-finite coordinate gets
//             the key `none`, above every cell's, sorts last and is never looked at again.  The pairs go through the Onesweep
//             sort (k_sort.hip).
//   records : 8 B + a 12 B gather read, 20 B written per sorted splat: {x, y, z, id} and the key, so that the query pass reads
//             contiguous runs; a block's first and last position go into the zeroed {start, end} table (no scan).
//   cands   : per workgroup of 256 sorted queries, the sources in the 27 cells around them (u64): the host adds them up, checks
//             the work budget and cuts the query pass into slices.
//   query   : THE HOT KERNEL.  A wave takes 64 consecutive cell-sorted queries.  The 27 cells are 9 x-runs of at most 3 cells,
//             contiguous in key order, so each run is one span of source records per block it touches.  When all 64 queries share a
//             cell (dense scenes, large radii) the spans' bounds and their records are wave-uniform: they are read once with scalar
//             loads and every lane tests its own query against the same record out of SGPRs (7 VALU per candidate and lane, no
//             vector memory instruction in the loop).  Otherwise each lane walks its own spans; neighbouring lanes are in the
//             same or in adjacent cells, so their 16-byte loads fall into the same few cache lines.  A lane stops at `limit`, a
//             uniform wave when all its lanes have.  Every loop is bounded by table contents (positions < the record count by
//             construction, a search halves its interval); no spin, no hand-off between workgroups, no float atomics, no scratch,
//             no LDS.  Bound: VALU issue (uniform path) / L1 gather rate (per-lane path).  VGPRs and occupancy: gs_neigh_query_kernel.
//   state   : gs_state_coverage's quad mapping around the u32 plane: 5 B read per splat, at most 1 B written.
#include "gs_neigh_dev.h" // neigh_run, the walk skeleton neigh_visit and the state pass around a plane: shared with the other grid consumers

__device__ __forceinline__ uint32_t neigh_order_key(float v) { // order-preserving map of the bit pattern (gs_abi.h, splat attributes)
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
// out[16]: [0..2] min keys of x, y, z over the finite sources, [3..5] max keys, [6] sources, [7] finite sources, [8] queries,
// [9] finite queries.  The caller initialises it (min keys all ones, the rest 0).  gate (null for everyone but a refining nearest-
// neighbour search, gs_knn.hip): a query must also read +inf there.
__global__ __launch_bounds__(256) void gs_neigh_bounds_kernel(const uint8_t* __restrict__ state, const float* __restrict__ px, const float* __restrict__ py,
                                                               const float* __restrict__ pz, uint32_t n, uint32_t smask, uint32_t svalue, uint32_t qmask,
                                                               uint32_t qvalue, const uint32_t* __restrict__ gate, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_o[10];
    if (threadIdx.x < 10u) s_o[threadIdx.x] = threadIdx.x < 3u ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        const uint32_t sv = state ? state[i] : 0u;
        const bool src = (sv & smask) == svalue, qry = (sv & qmask) == qvalue && (!gate || gate[i] == 0x7F800000u);
        if (src || qry) {
            const float x = px[i], y = py[i], z = pz[i];
            const bool fin = neigh_finite(x, y, z);
            if (src) {
                atomicAdd(&s_o[6], 1u);
                if (fin) {
                    atomicAdd(&s_o[7], 1u);
                    atomicMin(&s_o[0], neigh_order_key(x)); atomicMin(&s_o[1], neigh_order_key(y)); atomicMin(&s_o[2], neigh_order_key(z));
                    atomicMax(&s_o[3], neigh_order_key(x)); atomicMax(&s_o[4], neigh_order_key(y)); atomicMax(&s_o[5], neigh_order_key(z));
                }
            }
            if (qry) {
                atomicAdd(&s_o[8], 1u);
                if (fin) atomicAdd(&s_o[9], 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 10u) {
        const uint32_t v = s_o[threadIdx.x];
        if (threadIdx.x < 3u) atomicMin(&out[threadIdx.x], v);
        else if (threadIdx.x < 6u) atomicMax(&out[threadIdx.x], v);
        else if (v) atomicAdd(&out[threadIdx.x], v);
    }
}
void gs_launch_neigh_bounds(const uint8_t* state, const GsScene& s, uint32_t n, uint32_t smask, uint32_t svalue, uint32_t qmask, uint32_t qvalue,
                            const uint32_t* gate, uint32_t* out, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_neigh_bounds_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, state, s.px, s.py, s.pz, n, smask, svalue, qmask, qvalue, gate, out);
}

__global__ __launch_bounds__(256) void gs_neigh_keys_kernel(const uint8_t* __restrict__ state, const float* __restrict__ px, const float* __restrict__ py,
                                                             const float* __restrict__ pz, uint32_t n, uint32_t mask, uint32_t value,
                                                             const uint32_t* __restrict__ gate, GsNeighGrid g, uint32_t* __restrict__ keys,
                                                             uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t sv = state ? state[i] : 0u;
    uint32_t key = g.none;
    if ((sv & mask) == value && (!gate || gate[i] == 0x7F800000u)) {
        const float x = px[i], y = py[i], z = pz[i];
        if (neigh_finite(x, y, z)) key = neigh_key(g, x, y, z);
    }
    keys[i] = key;
    vals[i] = i;
}
void gs_launch_neigh_keys(const uint8_t* state, const GsScene& s, uint32_t n, uint32_t mask, uint32_t value, const uint32_t* gate, const GsNeighGrid& g,
                          uint32_t* keys, uint32_t* vals, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_neigh_keys_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, state, s.px, s.py, s.pz, n, mask, value, gate, g, keys, vals);
}

// Sorted position t (0 .. n): a key below `none` is a member; its record and, with `table`, its key and the ends of its block's run.
__global__ __launch_bounds__(256) void gs_neigh_records_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t n, GsNeighGrid g,
                                                                const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                                float4* __restrict__ rec, uint32_t* __restrict__ skeys, uint2* __restrict__ table) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const uint32_t k = keys[t];
    if (k >= g.none) return;
    const uint32_t id = vals[t];
    if (id >= n) return; // cannot happen: the values are a permutation of 0 .. n; keeps the gather inside the planes whatever the sort left
    rec[t] = make_float4(px[id], py[id], pz[id], __uint_as_float(id));
    if (table) {
        skeys[t] = k;
        const uint32_t p = k >> g.shift; // < g.blocks: none is a multiple of 2^shift
        if (p >= g.blocks) return;
        if (t == 0u || (keys[t - 1u] >> g.shift) != p) table[p].x = t;
        if (t + 1u == n || keys[t + 1u] >= g.none || (keys[t + 1u] >> g.shift) != p) table[p].y = t + 1u;
    }
}
void gs_launch_neigh_records(const uint32_t* keys, const uint32_t* vals, uint32_t n, const GsNeighGrid& g, const GsScene& s, void* rec, uint32_t* skeys,
                             void* table, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_neigh_records_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, keys, vals, n, g, s.px, s.py, s.pz, (float4*)rec, skeys,
                       (uint2*)table);
}

// sums[b]: the candidates of sorted queries 256 b .. 256 b + 255 (those below nq), self included where the query is a source.
__global__ __launch_bounds__(256) void gs_neigh_cands_kernel(const float4* __restrict__ qrec, uint32_t nq, NeighSources S, GsNeighGrid g,
                                                              unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0ull;
    __syncthreads();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    unsigned long long cand = 0ull;
    if (t < nq) {
        const float4 q = qrec[t];
        const int cx = neigh_cell(q.x, g.lo[0], g.inv_h, g.g[0]), cy = neigh_cell(q.y, g.lo[1], g.inv_h, g.g[1]), cz = neigh_cell(q.z, g.lo[2], g.inv_h, g.g[2]);
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy) neigh_run(S, g, cx, cy + dy, cz + dz, [&](uint32_t lo, uint32_t hi) { cand += hi - lo; });
    }
    if (cand) atomicAdd(&s_sum, cand);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = s_sum;
}
void gs_launch_neigh_cands(const NeighView& v, unsigned long long* sums, hipStream_t st) {
    if (!v.nqry) return;
    hipLaunchKernelGGL(gs_neigh_cands_kernel, dim3((v.nqry + 255u) / 256u), dim3(256), 0, st, v.qrec, v.nqry, v.src, v.g, sums);
}

// One span against the lane's query.  UNIFORM: lo / hi are the same in every lane (scalar loads of the records, one ballot per record
// to stop the wave); otherwise each lane walks its own.
template <bool UNIFORM>
__device__ __forceinline__ void neigh_walk(const float4* __restrict__ srec, uint32_t lo, uint32_t hi, const float4& q, uint32_t qid, float r2, uint32_t limit,
                                           bool live, uint32_t& cnt) {
    if (UNIFORM) {
        for (uint32_t s = lo; s < hi; ++s) {
            if (__builtin_amdgcn_ballot_w64(live && cnt < limit) == 0ull) break;
            const float4 p = srec[s];
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const bool hit = (dx * dx + dy * dy) + dz * dz <= r2 && __float_as_uint(p.w) != qid;
            cnt += (hit && live && cnt < limit) ? 1u : 0u;
        }
    } else {
        for (uint32_t s = lo; s < hi && cnt < limit; ++s) {
            const float4 p = srec[s];
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const bool hit = (dx * dx + dy * dy) + dz * dz <= r2 && __float_as_uint(p.w) != qid;
            cnt += hit ? 1u : 0u;
        }
    }
}

// Sorted queries 256 (first_block + blockIdx.x) ...: plane[id] = min(limit, neighbours).  27 VGPRs, 74 SGPRs, 8 waves per SIMD, no LDS, no scratch.
__global__ __launch_bounds__(256) void gs_neigh_query_kernel(const float4* __restrict__ qrec, uint32_t nq, uint32_t first_block, NeighSources S, GsNeighGrid g,
                                                              float r2, uint32_t limit, uint32_t n, uint32_t* __restrict__ plane) {
    const uint64_t t64 = ((uint64_t)first_block + blockIdx.x) * 256u + threadIdx.x;
    const bool live = t64 < nq;
    const float4 q = live ? qrec[(uint32_t)t64] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t qid = __float_as_uint(q.w);
    uint32_t cnt = 0u;
    neigh_visit<false>(S, g, q, live, live, [&](auto uniform, uint32_t lo, uint32_t hi) { // unguarded: the uniform walk ends at its first ballot
        constexpr bool U = decltype(uniform)::value;
        neigh_walk<U>(S.rec, lo, hi, q, qid, r2, limit, !U || live, cnt);
    });
    if (live && qid < n) plane[qid] = cnt < limit ? cnt : limit;
}
void gs_launch_neigh_query(const NeighView& v, uint32_t first_block, uint32_t blocks, float r2, uint32_t limit, uint32_t n, uint32_t* plane, hipStream_t st) {
    if (!blocks) return;
    hipLaunchKernelGGL(gs_neigh_query_kernel, dim3(blocks), dim3(256), 0, st, v.qrec, v.nqry, first_block, v.src, v.g, r2, limit, n, plane);
}

// gs_state_neigh (and gs_state_cluster over the size plane): the state pass around a u32 plane (gs_neigh_dev.h) with the range
// membership (c >= lo && c <= hi) == inside.
struct NeighRange {
    uint32_t lo, hi;
    bool inside;
    __device__ __forceinline__ bool operator()(uint32_t c) const { return (c >= lo && c <= hi) == inside; }
};
__global__ __launch_bounds__(256) void gs_state_neigh_kernel(uint8_t* __restrict__ state, const uint32_t* __restrict__ plane, uint32_t n, uint32_t lo, uint32_t hi,
                                                              uint32_t inside, uint32_t op, uint32_t bits, uint32_t wmask, uint32_t wvalue,
                                                              unsigned long long* __restrict__ matched) {
    state_plane_pass(state, plane, n, NeighRange{lo, hi, inside != 0u}, op, bits, wmask, wvalue, matched);
}
void gs_launch_state_neigh(uint8_t* state, const uint32_t* plane, uint32_t n, uint32_t min_count, uint32_t max_count, uint32_t inside, uint32_t op,
                           uint32_t bits, uint32_t where_mask, uint32_t where_value, unsigned long long* matched, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_state_neigh_kernel, dim3(state_plane_blocks(n)), dim3(256), 0, st, state, plane, n, min_count, max_count, inside, op, bits,
                       where_mask, where_value, matched);
}
