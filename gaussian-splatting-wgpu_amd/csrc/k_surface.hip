// k_surface.hip -- surface: for every query splat the integer moments of its neighbourhood, and from them a normal and three shape
// eigenvalues (gs_surface.hip, gs_abi.h "surface").  The reference has no counterpart: it is a viewer; an editor on it would build a
// k-d tree over its host records and run a PCA per point.
//
// The grid, the records, the cell table, the candidates and the slices are the neighbourhoods' (k_neigh.hip, where the geometry is
// argued; gs_neigh_dev.h: neigh_run); the distance is their expression with nothing changed, d = p_j - p_i, (dx dx + dy dy) + dz dz
// <= r2, one rounding per operation (-ffp-contract=off), self excluded by id, a NaN or infinite coordinate failing every comparison.
// Every expression of the definition is gs_surface_math.h's.  What is new is what a lane keeps of the accepted candidates:
//
//   init    : a whole estimate's start, 32 B written per splat: NaN in the six floats, count 0 (what a splat that is no query, and a
//             query without a record -- a non-finite coordinate --, keeps).
//   query   : THE HOT KERNEL, in the count query's shape: a wave takes 64 consecutive cell-sorted queries; when all 64 share a cell
//             the 9 x-runs' span bounds and the source records are wave-uniform (scalar loads, the record out of SGPRs), otherwise
//             each lane walks its own spans; four records -- one 64-byte line -- are in flight either way (with one record per
//             trip the uniform loop waits for every scalar load: 52 ms against 33 ms for 1.7e10 candidates, profiles/surface.txt).
//             Per lane: the count and nine i64 sums in registers, no LDS.
//             A candidate costs three multiplies by the scale, three v_rndne_f32, three v_cvt_i32_f32 and nine integer accumulates:
//             S += q is a sign extension (v_ashrrev_i32) and ONE v_lshl_add_u64, M += q q ONE v_mad_i64_i32 (32 x 32 + 64; checked in
//             the compiler's output: six per copy of the candidate test, 60 in all, no v_mul_lo / v_mul_hi anywhere).  The uniform loop is, per
//             candidate and lane, 10 VALU instructions for the distance test (the count's) and 29 for the moments (3 + 3 + 3, 3
//             sign extensions, 7 v_cndmask for the rejection, the count's add, 3 + 6 accumulates): four times the count's
//             instructions per candidate, or more in time (the 64-bit instructions' issue rate was not measured), where every
//             lane takes every candidate.
//             Measured (profiles/surface.txt): at 6.1 M splats, where waves rarely share a cell and a lane adds moments only for
//             the 15 % of its candidates it accepts, 1.17 and 0.98 times the count's query pass at a mean of 10 and 30 neighbours;
//             on the uniform path (131072 splats in one cell, 2 waves per SIMD) 0.75 times: the count waits for one scalar load
//             per record there, and the moments' instructions cost less than that wait.
//             On the uniform path rejection is BRANCHLESS: a rejected candidate's three q's are 0 (in the source the products are
//             replaced by 0.0f before the rint, so that no out-of-range float is ever converted; the compiler selects after the
//             saturating hardware conversion) and the count takes 0: a wave does not serialise on per-lane acceptance, and a
//             candidate costs the same accepted or not.  On the per-lane path a lane adds only what it accepts.
//             The sums are integers: nothing depends on the order of the visit.  Every loop is bounded by table contents (positions <
//             the record count by construction, a search halves its interval); no spin, no hand-off between workgroups, no atomics on
//             results, no float atomics, no scratch, no LDS.  The ten words go to the slice's scratch (word k of sorted query t at
//             k * cap + t - first: consecutive lanes, consecutive words) or, with GS_SURFACE_KEEP_SUMS, to the kept plane (ten words
//             per splat id); then one ballot popcount and one integer atomicAdd per wave for the queries that end with count < 3.
//             Bound: VALU issue (uniform path) / L1 gather rate (per-lane path), as the count.  Registers and occupancy:
//             gs_surface_query_kernel.
//   finish  : one thread per query of the slice, f64: ten words -> 28 bytes (sf_finish; the Jacobi's registers are the reason this is
//             not fused into the hot kernel).  A query with count < 3 gets NaN and its count.
//   state   : the state pass (gs_neigh_dev.h: state_plane_pass's shape) around ONE of the two 16-byte planes -- the eigenvalues for
//             the four shape kinds, the normal and count for the others: 17 B read per splat.
#include "gs_neigh_dev.h"
#include "gs_surface_math.h"

__global__ __launch_bounds__(256) void gs_surface_init_kernel(uint32_t n, float4* __restrict__ nrm, float4* __restrict__ eig) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float nan = __uint_as_float(SF_NAN_BITS);
    nrm[i] = make_float4(nan, nan, nan, __uint_as_float(0u));
    eig[i] = make_float4(nan, nan, nan, 0.0f);
}
void gs_launch_surface_init(uint32_t n, void* nrm, void* eig, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_surface_init_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, (float4*)nrm, (float4*)eig);
}

// One span against the lane's query.  UNIFORM: lo / hi are the same in every lane (scalar loads of the records) and rejection is
// branchless; otherwise each lane walks its own.
template <bool UNIFORM>
__device__ __forceinline__ void surface_walk(const float4* __restrict__ srec, uint32_t lo, uint32_t hi, const float4& q, uint32_t qid, float r2, float sc,
                                             bool live, SfSums& L) {
    const auto test = [&](const float4& p) {
        const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const bool other = __float_as_uint(p.w) != qid;
        const bool hit = (d2 <= r2) & other & (!UNIFORM || live); // (& not &&: no branch around the id's comparison)
        if (UNIFORM) {
            const float fx = hit ? dx * sc : 0.0f, fy = hit ? dy * sc : 0.0f, fz = hit ? dz * sc : 0.0f;
            sf_add(L, hit ? 1u : 0u, (int32_t)rintf(fx), (int32_t)rintf(fy), (int32_t)rintf(fz));
        } else if (hit) {
            sf_add(L, 1u, sf_quant(dx, sc), sf_quant(dy, sc), sf_quant(dz, sc));
        }
    };
    uint32_t s = lo;
    for (; s + 4u <= hi; s += 4u) { // four records -- one 64-byte line -- in flight: per lane, or as one scalar load of 16 words
        const float4 p0 = srec[s], p1 = srec[s + 1u], p2 = srec[s + 2u], p3 = srec[s + 3u];
        test(p0); test(p1); test(p2); test(p3);
    }
    for (; s < hi; ++s) test(srec[s]);
}

// Sorted queries 256 (first_block + blockIdx.x) ...: the ten words of sorted query t at out[slot * slot_stride + k * word_stride],
// slot = the splat id (the kept plane: strides 10, 1) or t - 256 first_block (the slice's scratch: strides 1, cap); *unresolved += the
// queries that end with count < 3.
// 56 VGPRs, 66 SGPRs, no scratch (private segment 0), no LDS: 8 waves per SIMD (the launch bound's limit).
// WRITTEN OUT, not neigh_visit<true> (gs_neigh_dev.h): through it 8 lines of the stream move and the uniform path misses the timing rule (profiles/grid_walks_refactor.txt).
__global__ __launch_bounds__(256) void gs_surface_query_kernel(const float4* __restrict__ qrec, uint32_t nq, uint32_t first_block, NeighSources S, GsNeighGrid g,
                                                                float r2, float sc, uint32_t n, long long* __restrict__ out, uint32_t by_id,
                                                                unsigned long long word_stride, uint32_t* __restrict__ unresolved) {
    const uint64_t t64 = ((uint64_t)first_block + blockIdx.x) * 256u + threadIdx.x;
    const bool live = t64 < nq;
    const float4 q = live ? qrec[(uint32_t)t64] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t qid = __float_as_uint(q.w);
    const int cx = neigh_cell(q.x, g.lo[0], g.inv_h, g.g[0]), cy = neigh_cell(q.y, g.lo[1], g.inv_h, g.g[1]), cz = neigh_cell(q.z, g.lo[2], g.inv_h, g.g[2]);
    const uint32_t key = ((uint32_t)cz << g.bxy) | ((uint32_t)cy << g.bx) | (uint32_t)cx;
    // the first live lane's cell (lane 0 is live whenever any lane is: the queries of a wave are consecutive)
    const uint32_t key0 = __builtin_amdgcn_readfirstlane(key);
    const bool uniform = __builtin_amdgcn_ballot_w64(live && key != key0) == 0ull;
    // a wave without a query (the last workgroup's tail) walks nothing (gs_neigh_dev.h: neigh_visit's GUARD)
    const bool any = __builtin_amdgcn_ballot_w64(live) != 0ull;
    SfSums L{};
    if (any && uniform) {
        const int ux = __builtin_amdgcn_readfirstlane(cx), uy = __builtin_amdgcn_readfirstlane(cy), uz = __builtin_amdgcn_readfirstlane(cz);
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                neigh_run(S, g, ux, uy + dy, uz + dz, [&](uint32_t lo, uint32_t hi) {
                    surface_walk<true>(S.rec, __builtin_amdgcn_readfirstlane(lo), __builtin_amdgcn_readfirstlane(hi), q, qid, r2, sc, live, L);
                });
    } else if (live) {
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                neigh_run(S, g, cx, cy + dy, cz + dz, [&](uint32_t lo, uint32_t hi) { surface_walk<false>(S.rec, lo, hi, q, qid, r2, sc, true, L); });
    }
    if (live && qid < n) {
        long long* o = out + (by_id ? (uint64_t)qid * SF_SUM_WORDS : (uint64_t)(blockIdx.x * 256u + threadIdx.x));
        const uint64_t ws = by_id ? 1ull : word_stride;
        o[0] = (long long)L.n;
        for (uint32_t k = 0; k < 3u; ++k) o[(1u + k) * ws] = L.S[k];
        for (uint32_t k = 0; k < 6u; ++k) o[(4u + k) * ws] = L.M[k];
    }
    const unsigned long long open = __builtin_amdgcn_ballot_w64(live && L.n < 3u);
    if (open && (threadIdx.x & 63u) == 0u) atomicAdd(unresolved, (uint32_t)__popcll(open));
}
void gs_launch_surface_query(const NeighView& v, uint32_t first_block, uint32_t blocks, float r2, float scale, uint32_t n, int64_t* out, bool by_id,
                             uint64_t word_stride, uint32_t* unresolved, hipStream_t st) {
    if (!blocks) return;
    hipLaunchKernelGGL(gs_surface_query_kernel, dim3(blocks), dim3(256), 0, st, v.qrec, v.nqry, first_block, v.src, v.g, r2, scale, n, (long long*)out,
                       by_id ? 1u : 0u, (unsigned long long)word_stride, unresolved);
}

// Sorted queries first .. first + count: the ten words (addressed as the query kernel wrote them) -> the two records of the splat.
// f64 throughout (sf_finish).  72 VGPRs, 24 SGPRs, no scratch: 7 waves per SIMD.
__global__ __launch_bounds__(256) void gs_surface_finish_kernel(const float4* __restrict__ qrec, uint32_t first, uint32_t count, uint32_t n,
                                                                 const long long* __restrict__ in, uint32_t by_id, unsigned long long word_stride,
                                                                 double unscale, uint32_t orient, float tx, float ty, float tz, float4* __restrict__ nrm,
                                                                 float4* __restrict__ eig) {
    const uint32_t local = blockIdx.x * 256u + threadIdx.x;
    if (local >= count) return;
    const float4 q = qrec[first + local];
    const uint32_t qid = __float_as_uint(q.w);
    if (qid >= n) return; // cannot happen: the records hold splat indices
    const long long* w = in + (by_id ? (uint64_t)qid * SF_SUM_WORDS : (uint64_t)local);
    const uint64_t ws = by_id ? 1ull : word_stride;
    int64_t s[SF_SUM_WORDS];
#pragma unroll
    for (uint32_t k = 0; k < SF_SUM_WORDS; ++k) s[k] = w[k * ws];
    const float nan = __uint_as_float(SF_NAN_BITS);
    float nv[3] = {nan, nan, nan}, ev[3] = {nan, nan, nan};
    if (s[0] >= 3) {
        sf_finish(s, unscale, nv, ev);
        if (orient) {
            const float p[3] = {q.x, q.y, q.z}, t[3] = {tx, ty, tz};
            sf_orient(nv, p, t);
        }
    }
    nrm[qid] = make_float4(nv[0], nv[1], nv[2], __uint_as_float((uint32_t)s[0]));
    eig[qid] = make_float4(ev[0], ev[1], ev[2], 0.0f);
}
void gs_launch_surface_finish(const void* qrec, uint32_t first, uint32_t count, uint32_t n, const int64_t* in, bool by_id, uint64_t word_stride,
                              double unscale, bool orient, const float toward[3], void* nrm, void* eig, hipStream_t st) {
    if (!count) return;
    hipLaunchKernelGGL(gs_surface_finish_kernel, dim3((count + 255u) / 256u), dim3(256), 0, st, (const float4*)qrec, first, count, n, (const long long*)in,
                       by_id ? 1u : 0u, (unsigned long long)word_stride, unscale, orient ? 1u : 0u, toward[0], toward[1], toward[2], (float4*)nrm,
                       (float4*)eig);
}

// The planes as gs_surface_read returns them: n x 3 floats out of the records' first three, n words out of the fourth.
__global__ __launch_bounds__(256) void gs_surface_unpack_kernel(const float4* __restrict__ rec, uint32_t n, float* __restrict__ xyz, uint32_t* __restrict__ w) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 r = rec[i];
    if (xyz) { xyz[3u * (uint64_t)i] = r.x; xyz[3u * (uint64_t)i + 1u] = r.y; xyz[3u * (uint64_t)i + 2u] = r.z; }
    if (w) w[i] = __float_as_uint(r.w);
}
void gs_launch_surface_unpack(const void* rec, uint32_t n, float* xyz, uint32_t* w, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(gs_surface_unpack_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, (const float4*)rec, n, xyz, w);
}

// gs_state_surface: state_plane_pass's shape (gs_neigh_dev.h) around a 16-byte plane: a thread takes splats 4q .. 4q+3, one whole word
// of the state plane and four records.  The record is the eigenvalues' for the four shape kinds and the normal's (count in its fourth
// word) for the others: sf_feature reads the triple it needs.  WRITTEN OUT: state_plane_pass over the plane's element type leaves the
// u32 kernels' streams alone but reassociates this one's new state word and hit sum (profiles/grid_walks_refactor.txt).
struct SurfaceRange {
    uint32_t kind;
    float lo, hi;
    bool inside;
    float axis[3];
    __device__ __forceinline__ bool operator()(const float4& r) const {
        const float a[3] = {r.x, r.y, r.z};
        return sf_member(sf_feature(kind, a, a, __float_as_uint(r.w), axis), lo, hi, inside);
    }
};
__global__ __launch_bounds__(256) void gs_state_surface_kernel(uint8_t* __restrict__ state, const float4* __restrict__ plane, uint32_t n, SurfaceRange member,
                                                                uint32_t op, uint32_t bits, uint32_t wmask, uint32_t wvalue,
                                                                unsigned long long* __restrict__ matched) {
    state_block_begin();
    const uint32_t q = blockIdx.x * 256u + threadIdx.x; // splats 4q .. 4q+3
    const uint64_t first = (uint64_t)q * 4u;
    uint32_t hits = 0;
    if (first + 4u <= n) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(state)[q];
        const float4 R[4] = {plane[first], plane[first + 1u], plane[first + 2u], plane[first + 3u]};
        uint32_t nw = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t sv = (w >> (8 * k)) & 0xFFu;
            const bool in = ((sv & wmask) == wvalue) && member(R[k]);
            hits += in ? 1u : 0u;
            nw |= (in ? gs_state_apply(sv, op, bits) : sv) << (8 * k);
        }
        if (nw != w) reinterpret_cast<uint32_t*>(state)[q] = nw; // stored only if it changed
    } else if (first < n) {
        for (uint64_t i = first; i < n; ++i) {
            const uint32_t sv = state[i];
            const bool in = ((sv & wmask) == wvalue) && member(plane[i]);
            hits += in ? 1u : 0u;
            const uint32_t nv = in ? gs_state_apply(sv, op, bits) : sv;
            if (nv != sv) state[i] = (uint8_t)nv;
        }
    }
    state_block_add(hits, matched);
}
void gs_launch_state_surface(uint8_t* state, const void* plane, uint32_t n, uint32_t kind, float lo, float hi, uint32_t inside, const float axis[3], uint32_t op,
                             uint32_t bits, uint32_t where_mask, uint32_t where_value, unsigned long long* matched, hipStream_t st) {
    if (!n) return;
    const SurfaceRange m{kind, lo, hi, inside != 0u, {axis[0], axis[1], axis[2]}};
    hipLaunchKernelGGL(gs_state_surface_kernel, dim3(state_plane_blocks(n)), dim3(256), 0, st, state, (const float4*)plane, n, m, op, bits, where_mask,
                       where_value, matched);
}
