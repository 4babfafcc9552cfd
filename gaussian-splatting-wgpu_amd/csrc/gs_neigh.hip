// gs_neigh.hip -- neighbourhoods' entry points: count the sources within a radius of every query into the count plane, read the
// plane (the selection by count, gs_state_neigh, is with the state calls in gs_state.hip).  Part of the C ABI
// (include/gsplat/gs_abi.h "neighbourhoods"); the kernels are in k_neigh.hip.
//
// The reference has no counterpart: it is a viewer.  An editor on it would export its 320-byte records and build a k-d tree on the
// host; here the positions are resident, a cell grid is one radix sort of (cell, id) pairs away, and 4 bytes per splat come back.
//
// A count is: bounds of the finite sources (one pass, one word-sized read-back: the grid is chosen on the host), keys, the Onesweep
// pair sort behind a private control block (private_sort, gs_runtime.h), records + keys + cell table, the same for the queries when
// their filter differs, the candidates per workgroup of queries (second read-back: the budget and the slices), the query pass.
// Every call drains the context's ring first (gs_wait), runs on the context's stream and returns when done.  None of them launches
// anything in a frame: a context that never calls them launches exactly what it did before.
#include <cmath>

#include "gs_neigh_host.h"
#include "gs_pack_math.h"

static_assert(sizeof(gs_neigh) == 40 && offsetof(gs_neigh, max_candidates) == 32, "gs_neigh layout");
static_assert(sizeof(gs_neigh_info) == 40 && offsetof(gs_neigh_info, cells) == 24 && offsetof(gs_neigh_info, cell_edge) == 36, "gs_neigh_info layout");

size_t plane_bytes(const gs_ctx* c) { return std::max<size_t>((((size_t)c->n * 4) + 15) & ~(size_t)15, 256); }
int32_t neigh_plane(gs_ctx* c, hipStream_t st) {
    if (c->ng.plane) return GS_OK;
    HIP_TRY(hipMalloc(c->ng.plane.out(), plane_bytes(c)));
    HIP_TRY(hipMemsetAsync(c->ng.plane, 0, plane_bytes(c), st));
    return GS_OK;
}

int32_t neigh_bounds(gs_ctx* c, const uint8_t* state, uint32_t smask, uint32_t svalue, uint32_t qmask, uint32_t qvalue, uint32_t hb[16], const uint32_t* gate) {
    gs_ctx::Neigh& s = c->ng;
    const int32_t rc = s.bounds.reserve(16);
    if (rc != GS_OK) return rc;
    for (int k = 0; k < 16; ++k) hb[k] = k < 3 ? 0xFFFFFFFFu : 0u; // (the three minima start at the largest key)
    HIP_TRY(hipMemcpyAsync(s.bounds, hb, 16 * 4, hipMemcpyHostToDevice, c->stream));
    gs_launch_neigh_bounds(state, c->scene, c->n, smask, svalue, qmask, qvalue, gate, s.bounds, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hb, s.bounds, 16 * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

// One filter's members in cell order: keys, the pair sort, the records (and the cell table when `table`).
static int32_t sorted_records(gs_ctx* c, const uint8_t* state, uint32_t mask, uint32_t value, const uint32_t* gate, const GsNeighGrid& g, void* rec, void* table) {
    gs_ctx::Neigh& s = c->ng;
    const uint32_t passes = (neigh_bits_of(g.none) + 7) / 8; // the keys reach `none` itself (no member)
    GsSortPair sorted;
    const int32_t rc = private_sort(c, c->n, passes, [&] { gs_launch_neigh_keys(state, c->scene, c->n, mask, value, gate, g, s.keysA, s.valsA, c->stream); }, &sorted);
    if (rc != GS_OK) return rc;
    gs_launch_neigh_records(sorted.keys, sorted.vals, c->n, g, c->scene, rec, s.skeys, table, c->stream);
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

// Steps 1 to 3 of a count, which a labelling, a search and an estimate share (gs_neigh_host.h): the bounds of the finite sources,
// the grid, the sources and -- when their filter differs -- the queries in cell order, the candidates per workgroup of 256 sorted
// queries.  The caller has drained the ring and c->n is 1 .. 2^30 - 1.  b->grid stays false when there is no finite source or no
// finite query (nothing to find; only the two counts are set).  gate (u32[n], null for a count and a labelling): the queries are further restricted to the
// splats whose word there is +inf's -- where the query set is formed: the bounds' counts and the queries' keys, and so their sort,
// their records and the candidates.
int32_t neigh_build(gs_ctx* c, const char* who, float radius, uint32_t smask, uint32_t svalue, uint32_t qmask, uint32_t qvalue, NeighBuilt* b,
                    const uint32_t* gate) {
    gs_ctx::Neigh& s = c->ng;
    const uint32_t n = c->n;
    const bool same = smask == qmask && svalue == qvalue && !gate;
    b->state = (smask | svalue | qmask | qvalue) ? c->scene.state : nullptr;
    int32_t rc;

    // scratch (all of it before the first launch: a failed allocation leaves the planes as they were)
    const uint32_t nblocks_max = (n + 255u) / 256u;
    if ((rc = private_sort_reserve(c, n, 4)) != GS_OK || (rc = s.skeys.reserve(n)) != GS_OK || (rc = s.src.reserve((uint64_t)n * 16)) != GS_OK ||
        (rc = s.sums.reserve(nblocks_max)) != GS_OK || (!same && (rc = s.qry.reserve((uint64_t)n * 16)) != GS_OK))
        return rc;

    // 1. the bounds of the finite sources and the four counts (the bounds words are reserved there, before the launch)
    uint32_t hb[16];
    if ((rc = neigh_bounds(c, b->state, smask, svalue, qmask, qvalue, hb, gate)) != GS_OK) return rc;
    b->sources = hb[6];
    b->queried = hb[8];
    b->src.nrec = hb[7]; // with finite coordinates: the others have no neighbours
    b->nqry = hb[9];
    if (!b->src.nrec || !b->nqry) return GS_OK;
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = pk_okey_value(hb[k]); hi[k] = pk_okey_value(hb[3 + k]); }
    GsNeighGrid& g = b->g;
    neigh_choose_grid(lo, hi, radius * 1.0011f, &g, &b->cell_edge); // h >= 1.0011 r: the margin the cell expression's rounding needs (k_neigh.hip)

    // 2. sources, then queries, in cell order
    rc = s.table.reserve((uint64_t)g.blocks * 8);
    if (rc != GS_OK) return rc;
    HIP_TRY(hipMemsetAsync(s.table, 0, (size_t)g.blocks * 8, c->stream));
    rc = sorted_records(c, b->state, smask, svalue, nullptr, g, s.src, s.table);
    if (rc != GS_OK) return rc;
    uint32_t fault[2] = {0u, 0u};
    if ((rc = private_sort_fault(c, &fault[0])) != GS_OK) return rc;
    b->src = NeighSources{(const float4*)s.src.get(), s.skeys, (const uint2*)s.table.get(), b->src.nrec};
    b->qrec = b->src.rec;
    if (!same) {
        HIP_TRY(hipStreamSynchronize(c->stream)); // fault[0] is read before the control block is zeroed again
        rc = sorted_records(c, b->state, qmask, qvalue, gate, g, s.qry, nullptr);
        if (rc != GS_OK) return rc;
        if ((rc = private_sort_fault(c, &fault[1])) != GS_OK) return rc;
        b->qrec = (const float4*)s.qry.get();
    }

    // 3. the candidates, exactly, per workgroup of 256 sorted queries: the caller checks the budget and cuts the slices
    const uint32_t nblocks = (b->nqry + 255u) / 256u;
    gs_launch_neigh_cands(*b, s.sums, c->stream);
    HIP_TRY(hipGetLastError());
    b->sums.resize(nblocks);
    HIP_TRY(hipMemcpyAsync(b->sums.data(), s.sums, (size_t)nblocks * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (fault[0] | fault[1]) return fail(GS_ERR_DEVICE_FAULT, "%s: look-back spin bound exceeded in the cell sort", who);
    for (uint32_t k = 0; k < nblocks; ++k) b->candidates += b->sums[k];
    b->grid = true;
    return GS_OK;
}
int32_t neigh_budget(const char* who, uint64_t candidates, uint64_t max_candidates, float radius) {
    const uint64_t budget = max_candidates ? max_candidates : GS_NEIGH_DEFAULT_CANDIDATES;
    if (candidates > budget)
        return fail(GS_ERR_CAPACITY, "%s: %llu candidates exceed the work budget max_candidates = %llu (radius %g puts too many splats into one cell)", who,
                    (unsigned long long)candidates, (unsigned long long)budget, (double)radius);
    return GS_OK;
}
int32_t neigh_check_radius(const char* who, float radius, float* r2) {
    if (!std::isfinite(radius) || radius < 0.0f) return fail(GS_ERR_INVALID_ARGUMENT, "%s: radius %g is negative or not finite", who, (double)radius);
    *r2 = radius * radius; // once, in f32: the kernel and a restating host compare with the same number
    if (!std::isfinite(*r2)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: radius %g squared is not finite in f32", who, (double)radius);
    return GS_OK;
}

int32_t neigh_check_filters(gs_ctx* c, const char* who, uint32_t smask, uint32_t svalue, uint32_t qmask, uint32_t qvalue, float radius, float* r2) {
    int32_t rc = resident_check(c, who, Plane::filtered, smask, svalue);
    if (rc != GS_OK) return rc;
    rc = resident_check(c, who, Plane::filtered, qmask, qvalue);
    return rc != GS_OK ? rc : neigh_check_radius(who, radius, r2);
}

GS_EXPORT int32_t gs_neigh_count(gs_ctx* c, const gs_neigh* q, gs_neigh_info* info) {
    const char* who = "gs_neigh_count";
    float r2;
    int32_t rc = neigh_check_query(c, who, q);
    if (rc != GS_OK) return rc;
    rc = neigh_check_filters(c, who, q->src_mask, q->src_value, q->qry_mask, q->qry_value, q->radius, &r2);
    if (rc != GS_OK) return rc;
    if (q->limit == 0u) return fail(GS_ERR_INVALID_ARGUMENT, "%s: limit %u is not 1 .. 2^32-1", who, q->limit);
    if (q->reserved != 0u) return fail(GS_ERR_INVALID_ARGUMENT, "%s: reserved %u is not 0", who, q->reserved);
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    rc = neigh_plane(c, c->stream);
    if (rc != GS_OK) return rc;
    gs_neigh_info out{};
    if (info) *info = out;
    const uint32_t n = c->n;
    if (!n) { HIP_TRY(hipStreamSynchronize(c->stream)); return GS_OK; }
    NeighBuilt b;
    rc = neigh_grid(c, who, q->radius, q->src_mask, q->src_value, q->qry_mask, q->qry_value, q->max_candidates, &b, [&](const NeighBuilt& b) {
        neigh_report(&out, b);
        if (info) *info = out;
    });
    if (rc != GS_OK) return rc;

    // 4. the query pass, in slices of whole workgroups (without a grid there is nothing to find: every count is 0)
    HIP_TRY(hipMemsetAsync(c->ng.plane, 0, plane_bytes(c), c->stream));
    if (b.grid) {
        neigh_slices(b.sums, [&](uint32_t b0, uint32_t blocks) { gs_launch_neigh_query(b, b0, blocks, r2, q->limit, n, c->ng.plane, c->stream); });
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

int32_t plane_read(gs_ctx* c, const char* who, int32_t (*planes)(gs_ctx*, const uint32_t* [2]), const char* what, void* const dst[2], uint64_t cap, uint64_t* n) {
    int32_t rc = resident_begin(c, who, Plane::none);
    if (rc != GS_OK) return rc;
    const uint32_t* plane[2] = {nullptr, nullptr};
    rc = planes(c, plane);
    if (rc != GS_OK) return rc;
    if (!n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null n", who);
    *n = c->n;
    if (!dst[0] && !dst[1]) { HIP_TRY(hipStreamSynchronize(c->stream)); return GS_OK; }
    if (cap < c->n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %llu %s %llu", who, (unsigned long long)c->n, what, (unsigned long long)cap);
    for (int k = 0; k < 2; ++k)
        if (c->n && dst[k]) HIP_TRY(hipMemcpyAsync(dst[k], plane[k], (size_t)c->n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}
GS_EXPORT int32_t gs_neigh_read(gs_ctx* c, uint32_t* dst, uint64_t cap, uint64_t* n) {
    void* const out[2] = {dst, nullptr};
    const auto planes = [](gs_ctx* c, const uint32_t* p[2]) { const int32_t rc = neigh_plane(c, c->stream); p[0] = c->ng.plane; return rc; };
    return plane_read(c, "gs_neigh_read", planes, "counts needed, the buffer holds", out, cap, n);
}
