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

#include "gs_neigh_host.h"

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
    float r2;
    int32_t rc = neigh_check_query(c, who, q);
    if (rc != GS_OK) return rc;
    rc = neigh_check_filters(c, who, q->mask, q->value, q->mask, q->value, q->radius, &r2); // (the one filter on both sides)
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
    gs_ctx::Neigh& s = c->ng;
    NeighBuilt b;
    rc = neigh_grid(c, who, q->radius, q->mask, q->value, q->mask, q->value, q->max_candidates, &b, [&](const NeighBuilt& b) {
        out.members = b.sources;
        out.candidates = b.candidates;
        out.cell_edge = b.cell_edge;
        for (int k = 0; k < 3; ++k) out.cells[k] = b.g.g[k];
        if (info) *info = out;
    });
    if (rc != GS_OK) return rc;

    // the records are written: the sort's arrays are free.  Without a grid (no member with finite coordinates) init alone labels.
    uint32_t *parent = s.keysA, *count = s.valsA;
    gs_launch_cluster_init(b.state, c->scene, n, q->mask, q->value, parent, count, c->stream);
    HIP_TRY(hipGetLastError());
    const uint32_t nrec = b.grid ? b.src.nrec : 0u;
    for (bool changed = nrec != 0u; changed;) {
        if (out.rounds >= GS_CLUSTER_MAX_ROUNDS)
            return fail(GS_ERR_DEVICE_FAULT, "%s: the edge pass still hooked after %u rounds (GS_CLUSTER_MAX_ROUNDS)", who, out.rounds);
        uint32_t hooked = 0; // the round's changed word
        rc = neigh_open_word(c, [&](uint32_t* word) {
            neigh_slices(b.sums, [&](uint32_t b0, uint32_t blocks) { gs_launch_cluster_edges(b, b0, blocks, r2, n, parent, word, c->stream); });
            gs_launch_cluster_flatten(s.src, nrec, n, parent, c->stream);
        }, &hooked);
        if (rc != GS_OK) return rc;
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
    void* const out[2] = {labels, sizes};
    const auto planes = [](gs_ctx* c, const uint32_t* p[2]) { const int32_t rc = cluster_planes(c, c->stream); p[0] = c->cl.label; p[1] = c->cl.size; return rc; };
    return plane_read(c, "gs_cluster_read", planes, "words per plane needed, the buffers hold", out, cap, n);
}
