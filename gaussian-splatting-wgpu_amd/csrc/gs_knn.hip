// gs_knn.hip -- nearest neighbours' entry points: the k-th nearest squared distance and the nearest source's id of every query into
// the two planes, read the planes (the selection by distance, gs_state_knn, is with the state calls in gs_state.hip).  Part of the
// C ABI (include/gsplat/gs_abi.h "nearest neighbours"); the kernels are in k_knn.hip.
//
// The reference has no counterpart: it is a viewer.  An editor on it would export its 320-byte records and query a k-d tree on the
// host; here a search is a neighbour count's grid (neigh_build, gs_neigh.hip: one copy) with a bounded top-k selection in place of
// the count, and 8 bytes per splat come back.
//
// A search is: the grid, records and candidates (neigh_build; refining, gated by the dist2 plane where the query set is formed), the
// budget, then -- only now is anything written: a call that fails before leaves the planes as they were -- the planes' start (a whole
// search: +inf for the queries, NaN for the others, NONE), the query pass in the count's slices, one word read back (the queries
// the pass left +inf).  Every call drains the context's ring first (gs_wait), runs on the context's stream and returns when done.
// None of them launches anything in a frame: a context that never calls them launches exactly what it did before.
#include "gs_neigh_host.h"

static_assert(sizeof(gs_knn) == 48 && offsetof(gs_knn, max_candidates) == 32 && offsetof(gs_knn, reserved) == 40, "gs_knn layout");
static_assert(sizeof(gs_knn_info) == 48 && offsetof(gs_knn_info, unresolved) == 24 && offsetof(gs_knn_info, cells) == 32 && offsetof(gs_knn_info, cell_edge) == 44,
              "gs_knn_info layout");

int32_t knn_planes(gs_ctx* c, hipStream_t st) {
    if (c->kn.dist2 && c->kn.nearest) return GS_OK;
    HIP_TRY(hipMalloc(c->kn.dist2.out(), plane_bytes(c)));
    HIP_TRY(hipMalloc(c->kn.nearest.out(), plane_bytes(c)));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)c->kn.dist2.get(), 0x7FC00000, plane_bytes(c) / 4, st)); // NaN: no query yet
    HIP_TRY(hipMemsetAsync(c->kn.nearest, 0xFF, plane_bytes(c), st));                                   // GS_KNN_NONE
    c->kn.k = 0;
    return GS_OK;
}

GS_EXPORT int32_t gs_knn_search(gs_ctx* c, const gs_knn* q, gs_knn_info* info) {
    const char* who = "gs_knn_search";
    float r2;
    int32_t rc = neigh_check_query(c, who, q);
    if (rc != GS_OK) return rc;
    rc = neigh_check_filters(c, who, q->src_mask, q->src_value, q->qry_mask, q->qry_value, q->radius, &r2);
    if (rc != GS_OK) return rc;
    if (q->k == 0u || q->k > GS_KNN_MAX_K) return fail(GS_ERR_INVALID_ARGUMENT, "%s: k %u is not 1 .. %u", who, q->k, GS_KNN_MAX_K);
    if (q->flags & ~GS_KNN_REFINE) return fail(GS_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x", who, q->flags & ~GS_KNN_REFINE);
    if (q->reserved != 0u) return fail(GS_ERR_INVALID_ARGUMENT, "%s: reserved %llu is not 0", who, (unsigned long long)q->reserved);
    const bool refine = (q->flags & GS_KNN_REFINE) != 0u;
    if (refine && c->kn.k == 0u) return fail(GS_ERR_INVALID_ARGUMENT, "%s: GS_KNN_REFINE with k %u before any search on this ctx", who, q->k);
    if (refine && c->kn.k != q->k) return fail(GS_ERR_INVALID_ARGUMENT, "%s: GS_KNN_REFINE with k %u, the last search had k %u", who, q->k, c->kn.k);
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    rc = knn_planes(c, c->stream);
    if (rc != GS_OK) return rc;
    gs_knn_info out{};
    if (info) *info = out;
    const uint32_t n = c->n;
    if (!n) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (!refine) c->kn.k = q->k;
        return GS_OK;
    }
    NeighBuilt b;
    rc = neigh_grid(c, who, q->radius, q->src_mask, q->src_value, q->qry_mask, q->qry_value, q->max_candidates, &b, [&](const NeighBuilt& b) {
        neigh_report(&out, b);
        if (info) *info = out;
    }, refine ? c->kn.dist2.get() : nullptr);
    if (rc != GS_OK) return rc;

    // from here on the planes are written.  A query without a record (a non-finite coordinate; every query when there is no grid:
    // nothing to find) keeps the +inf it is given here -- or, refining, the +inf that made it a query.
    if (!refine) {
        gs_launch_knn_init(b.state, n, q->qry_mask, q->qry_value, c->kn.dist2, c->kn.nearest, c->stream);
        HIP_TRY(hipGetLastError());
    }
    uint32_t open = 0; // finite queries the pass leaves +inf
    if (b.grid) {
        rc = neigh_open_word(c, [&](uint32_t* word) {
            neigh_slices(b.sums, [&](uint32_t b0, uint32_t blocks) { gs_launch_knn_query(b, b0, blocks, r2, q->k, n, c->kn.dist2, c->kn.nearest, word, c->stream); });
        }, &open);
        if (rc != GS_OK) return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    out.unresolved = b.grid ? (b.queried - b.nqry) + open : b.queried;
    if (info) *info = out;
    if (!refine) c->kn.k = q->k;
    return GS_OK;
}

GS_EXPORT int32_t gs_knn_read(gs_ctx* c, float* dist2, uint32_t* nearest, uint64_t cap, uint64_t* n) {
    void* const out[2] = {dist2, nearest};
    const auto planes = [](gs_ctx* c, const uint32_t* p[2]) { const int32_t rc = knn_planes(c, c->stream); p[0] = c->kn.dist2; p[1] = c->kn.nearest; return rc; };
    return plane_read(c, "gs_knn_read", planes, "values per plane needed, the buffers hold", out, cap, n);
}
