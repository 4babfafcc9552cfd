// gs_neigh_host.h -- what the host calls over the cell grid share: a count (gs_neigh.hip, which defines what is declared here), a
// labelling (gs_cluster.hip), a nearest-neighbour search (gs_knn.hip) and a surface estimate (gs_surface.hip).
#pragma once
#include "gs_runtime.h"

// neigh_check_query: the first refusals of a count, a search and a labelling (null ctx, null query, struct_size); an estimate has
// them in sf_check with its own and enters at neigh_check_filters: the next ones -- both filters (resident_check), then the
// radius; *r2 = radius * radius, once, in f32 (neigh_check_radius).  The call's own refusals follow.
// neigh_build: the cell grid over the finite sources, the sources (c->ng.src, skeys, table) and the queries (qrec: the sources'
// records when both filters are the same) in cell order -- the NeighView the launchers take --, and the candidates of every
// workgroup of 256 sorted queries.  neigh_budget: GS_ERR_CAPACITY when the candidates exceed max_candidates (0:
// GS_NEIGH_DEFAULT_CANDIDATES).  neigh_grid: what follows a call's n == 0 exit -- the 2^30 refusal, neigh_build, report(b) (the
// caller fills its info there: it stands when the budget refuses), the budget when there is a grid.  neigh_report: the five numbers
// every info struct but the clusters' has.  neigh_open_word: one word of c->ng.bounds (neigh_build is done with its 16) zeroed,
// handed to launch(word), whose kernels add into it, and read back into *word_out -- valid once the caller has synchronised.
// neigh_slices: cuts the workgroups into runs of at most GS_NEIGH_SLICE_CANDIDATES (one workgroup where a single one exceeds that)
// and calls launch(first workgroup, workgroups) for each.  plane_read: gs_neigh_read, gs_knn_read and gs_cluster_read -- planes(c, p)
// allocates the call's u32[N] planes on first use and names them in p, in the order of dst; `what` words the capacity refusal.
struct NeighBuilt : NeighView {        // (src.nrec, nqry: the sources and queries with finite coordinates, the records)
    const uint8_t* state = nullptr;    // the state plane, or null when both filters are (0, 0)
    uint64_t sources = 0, queried = 0; // splats that pass the two filters
    bool grid = false;                 // the view and what follows are set: there was something to find
    float cell_edge = 0.0f;
    std::vector<unsigned long long> sums;
    uint64_t candidates = 0;
};
int32_t neigh_check_radius(const char* who, float radius, float* r2);
int32_t neigh_check_filters(gs_ctx* c, const char* who, uint32_t smask, uint32_t svalue, uint32_t qmask, uint32_t qvalue, float radius, float* r2);
template <class Q>
int32_t neigh_check_query(const gs_ctx* c, const char* who, const Q* q) {
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null ctx", who);
    if (!q) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null query", who);
    if (q->struct_size != sizeof(Q)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: struct_size %u != %zu", who, q->struct_size, sizeof(Q));
    return GS_OK;
}
int32_t neigh_build(gs_ctx* c, const char* who, float radius, uint32_t smask, uint32_t svalue, uint32_t qmask, uint32_t qvalue, NeighBuilt* b,
                    const uint32_t* gate = nullptr);
int32_t neigh_budget(const char* who, uint64_t candidates, uint64_t max_candidates, float radius);
template <class Report>
int32_t neigh_grid(gs_ctx* c, const char* who, float radius, uint32_t smask, uint32_t svalue, uint32_t qmask, uint32_t qvalue, uint64_t max_candidates,
                   NeighBuilt* b, Report report, const uint32_t* gate = nullptr) {
    if (c->n >= (1u << 30)) return fail(GS_ERR_CAPACITY, "%s: %u splats, the cell sort takes fewer than 2^30", who, c->n); // (gs_sort_pairs_u32's limit)
    const int32_t rc = neigh_build(c, who, radius, smask, svalue, qmask, qvalue, b, gate);
    if (rc != GS_OK) return rc;
    report(*b);
    return b->grid ? neigh_budget(who, b->candidates, max_candidates, radius) : GS_OK;
}
template <class Info>
void neigh_report(Info* out, const NeighBuilt& b) {
    out->sources = b.sources;
    out->queried = b.queried;
    out->candidates = b.candidates;
    out->cell_edge = b.cell_edge;
    for (int k = 0; k < 3; ++k) out->cells[k] = b.g.g[k];
}
template <class Launch>
int32_t neigh_open_word(gs_ctx* c, Launch launch, uint32_t* word_out) {
    uint32_t* word = c->ng.bounds;
    HIP_TRY(hipMemsetAsync(word, 0, 4, c->stream));
    launch(word);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(word_out, word, 4, hipMemcpyDeviceToHost, c->stream));
    return GS_OK;
}
int32_t plane_read(gs_ctx* c, const char* who, int32_t (*planes)(gs_ctx*, const uint32_t* [2]), const char* what, void* const dst[2], uint64_t cap, uint64_t* n);
template <class Launch>
void neigh_slices(const std::vector<unsigned long long>& sums, Launch launch) {
    const uint32_t nblocks = (uint32_t)sums.size();
    for (uint32_t b0 = 0; b0 < nblocks;) {
        uint64_t sum = sums[b0];
        uint32_t b1 = b0 + 1u;
        while (b1 < nblocks && sum + sums[b1] <= GS_NEIGH_SLICE_CANDIDATES) sum += sums[b1++];
        launch(b0, b1 - b0);
        b0 = b1;
    }
}
