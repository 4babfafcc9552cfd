// gs_cluster.hip -- clusters' entry points: label the connected components of "within a radius of each other" into the label and
// size planes, read the planes (the two selections, gs_state_cluster and gs_state_cluster_linked, are with the state calls in
// gs_state.hip).  Part of the C ABI (include/gsplat/gs_abi.h "clusters"); the kernels are in k_cluster.hip.
//
// The reference has no counterpart: it is a viewer.  An editor on it would export its 320-byte records, build a k-d tree and run a
// union-find on the host; here a labelling is a neighbour count's grid (neigh_build, gs_neigh.hip: one copy) with a union in place
// of the count, and 8 bytes per splat come back.
//
// A labelling is: the members' grid, records and candidates (neigh_build with the one filter on both sides; the budget), then in
// c->ng's scratch -- the sort's four arrays are free once the records are written -- parent and the size counters, ROUNDS of {edge
// pass in the count's slices, flatten} until a whole edge pass hooked nothing (one word read back per round), the sizes, and at the
// very end the commit into the two planes with the info numbers: a call that fails anywhere before leaves the planes as they were.
// Every call drains the context's ring first (gs_wait), runs on the context's stream and returns when done.  None of them launches
// anything in a frame: a context that never calls them launches exactly what it did before.
#include <cstdlib>

#include "gs_runtime.h"

static_assert(sizeof(gs_cluster) == 32 && offsetof(gs_cluster, max_candidates) == 24, "gs_cluster layout");
static_assert(sizeof(gs_cluster_info) == 56 && offsetof(gs_cluster_info, rounds) == 32 && offsetof(gs_cluster_info, cell_edge) == 48, "gs_cluster_info layout");

int32_t cluster_planes(gs_ctx* c, hipStream_t st) {
    if (c->cl.label && c->cl.size) return GS_OK;
    HIP_TRY(hipMalloc(c->cl.label.out(), plane_bytes(c)));
    HIP_TRY(hipMalloc(c->cl.size.out(), plane_bytes(c)));
    HIP_TRY(hipMemsetAsync(c->cl.label, 0xFF, plane_bytes(c), st)); // GS_CLUSTER_NONE
    HIP_TRY(hipMemsetAsync(c->cl.size, 0, plane_bytes(c), st));
    return GS_OK;
}

GS_EXPORT int32_t gs_cluster_label(gs_ctx* c, const gs_cluster* q, gs_cluster_info* info) {
    const char* who = "gs_cluster_label";
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null ctx", who);
    if (!q) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null query", who);
    if (q->struct_size != sizeof(gs_cluster)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: struct_size %u != %zu", who, q->struct_size, sizeof(gs_cluster));
    int32_t rc = resident_check(c, who, Plane::filtered, q->mask, q->value);
    if (rc != GS_OK) return rc;
    float r2;
    rc = neigh_check_radius(who, q->radius, &r2);
    if (rc != GS_OK) return rc;
    for (int k = 0; k < 2; ++k)
        if (q->reserved[k] != 0u) return fail(GS_ERR_INVALID_ARGUMENT, "%s: reserved[%d] = %u is not 0", who, k, q->reserved[k]);
    rc = resident_drain(c, true); // (the counter: the slots the commit folds clusters and largest into)
    if (rc != GS_OK) return rc;
    rc = cluster_planes(c, c->stream);
    if (rc != GS_OK) return rc;
    gs_cluster_info out{};
    if (info) *info = out;
    const uint32_t n = c->n;
    if (!n) { HIP_TRY(hipStreamSynchronize(c->stream)); return GS_OK; }
    if (n >= (1u << 30)) return fail(GS_ERR_CAPACITY, "%s: %u splats, the cell sort takes fewer than 2^30", who, n); // (gs_sort_pairs_u32's limit)
    gs_ctx::Neigh& s = c->ng;
    NeighBuilt b;
    rc = neigh_build(c, who, q->radius, q->mask, q->value, q->mask, q->value, &b);
    if (rc != GS_OK) return rc;
    out.members = b.sources;
    out.candidates = b.candidates;
    out.cell_edge = b.cell_edge;
    for (int k = 0; k < 3; ++k) out.cells[k] = b.g.g[k];
    if (info) *info = out;
    if (b.grid) {
        rc = neigh_budget(who, b.candidates, q->max_candidates, q->radius);
        if (rc != GS_OK) return rc;
    }

    // the records are written: the sort's arrays are free.  Without a grid (no member with finite coordinates) init alone labels.
    uint32_t *parent = s.keysA, *count = s.valsA, *words = s.bounds; // words[0]: the round's changed
    gs_launch_cluster_init(b.state, c->scene, n, q->mask, q->value, parent, count, c->stream);
    HIP_TRY(hipGetLastError());
    const uint32_t nrec = b.grid ? b.nsrc : 0u;
    for (bool changed = nrec != 0u; changed;) {
        if (out.rounds >= GS_CLUSTER_MAX_ROUNDS)
            return fail(GS_ERR_DEVICE_FAULT, "%s: the edge pass still hooked after %u rounds (GS_CLUSTER_MAX_ROUNDS)", who, out.rounds);
        HIP_TRY(hipMemsetAsync(words, 0, 4, c->stream));
        neigh_slices(b.sums, [&](uint32_t b0, uint32_t blocks) {
            gs_launch_cluster_edges(s.src, nrec, b0, blocks, s.skeys, s.table, b.g, r2, n, parent, words, c->stream);
        });
        gs_launch_cluster_flatten(s.src, nrec, n, parent, c->stream);
        HIP_TRY(hipGetLastError());
        uint32_t hooked = 0;
        HIP_TRY(hipMemcpyAsync(&hooked, words, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        ++out.rounds;
        changed = hooked != 0u;
    }
    bool fold = true;
#ifdef GS_PROFILING
    if (const char* e = getenv("GS_CLUSTER_PLAIN_SIZES")) fold = atoi(e) == 0; // profiles/clusters.txt: what the wave fold buys
#endif
    gs_launch_cluster_sizes(s.src, nrec, n, parent, count, fold, c->stream);
    constexpr size_t kSlotWords = (size_t)GS_STATE_SLOTS * GS_STATE_SLOT_STRIDE;
    HIP_TRY(hipMemsetAsync(c->st.counter, 0, kSlotWords * 8, c->stream));
    gs_launch_cluster_commit(parent, count, n, c->cl.label, c->cl.size, c->st.counter, c->stream);
    HIP_TRY(hipGetLastError());
    unsigned long long h[kSlotWords];
    HIP_TRY(hipMemcpyAsync(h, c->st.counter, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < GS_STATE_SLOTS; ++k) {
        out.clusters += h[k * GS_STATE_SLOT_STRIDE];
        out.largest = std::max<uint64_t>(out.largest, h[k * GS_STATE_SLOT_STRIDE + 1]);
    }
    if (info) *info = out;
    return GS_OK;
}

GS_EXPORT int32_t gs_cluster_read(gs_ctx* c, uint32_t* labels, uint32_t* sizes, uint64_t cap, uint64_t* n) {
    int32_t rc = resident_begin(c, "gs_cluster_read", Plane::none);
    if (rc != GS_OK) return rc;
    rc = cluster_planes(c, c->stream);
    if (rc != GS_OK) return rc;
    if (!n) return fail(GS_ERR_INVALID_ARGUMENT, "gs_cluster_read: null n");
    *n = c->n;
    if (!labels && !sizes) { HIP_TRY(hipStreamSynchronize(c->stream)); return GS_OK; }
    if (cap < c->n)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_cluster_read: %llu words per plane needed, the buffers hold %llu", (unsigned long long)c->n, (unsigned long long)cap);
    if (c->n && labels) HIP_TRY(hipMemcpyAsync(labels, c->cl.label, (size_t)c->n * 4, hipMemcpyDeviceToHost, c->stream));
    if (c->n && sizes) HIP_TRY(hipMemcpyAsync(sizes, c->cl.size, (size_t)c->n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}
