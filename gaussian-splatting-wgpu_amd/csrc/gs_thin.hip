// gs_thin.hip -- thinning's entry points: sample a maximal set of members no two of which are within a radius of each other, in rank
// order, into the keeper and covers planes; read the planes; the host twin (the selection by covers, gs_state_thin, is with the state
// calls in gs_state.hip).  Part of the C ABI (include/gsplat/gs_abi.h "thinning"); the kernels are in k_thin.hip, the rank and the
// host twin in gs_thin_math.h.
//
// The reference has no counterpart: it is a viewer.  An editor on it would export its 320-byte records, build a k-d tree and run a
// sequential greedy on the host; here a sample is a neighbour count's grid (neigh_grid, gs_neigh_host.h: one copy) with a decision in
// place of the count, and 8 bytes per splat come back.
//
// A sample is: the members' grid, records and candidates (the one filter on both sides; the budget), then -- the sort's four arrays
// are free once the records are written -- status by sorted position in keysA, the work planes keeper / covers by splat index in
// valsA / keysB, the priority values in valsB, and the rank by sorted position in th.rank; ROUNDS of the round pass in the count's
// slices until one leaves no member undecided (one word read back per round); the assign pass; and at the very end the commit into
// the two planes with the info numbers: a call that fails anywhere before leaves the planes as they were.  Every call drains the
// context's ring first (gs_wait), runs on the context's stream and returns when done.  None launches anything in a frame.
#include "gs_neigh_host.h"
#include "gs_thin_math.h"

static_assert(sizeof(gs_thin) == 72 && offsetof(gs_thin, max_candidates) == 32 && offsetof(gs_thin, priority) == 40 && offsetof(gs_thin, reserved) == 64,
              "gs_thin layout");
static_assert(sizeof(gs_thin_info) == 64 && offsetof(gs_thin_info, rounds) == 40 && offsetof(gs_thin_info, cell_edge) == 56, "gs_thin_info layout");

int32_t thin_planes(gs_ctx* c, hipStream_t st) {
    if (c->th.keeper && c->th.covers) return GS_OK;
    HIP_TRY(hipMalloc(c->th.keeper.out(), plane_bytes(c)));
    HIP_TRY(hipMalloc(c->th.covers.out(), plane_bytes(c)));
    HIP_TRY(hipMemsetAsync(c->th.keeper, 0xFF, plane_bytes(c), st)); // GS_THIN_NONE
    HIP_TRY(hipMemsetAsync(c->th.covers, 0, plane_bytes(c), st));
    return GS_OK;
}

GS_EXPORT int32_t gs_thin_sample(gs_ctx* c, const gs_thin* q, gs_thin_info* info) {
    const char* who = "gs_thin_sample";
    float r2;
    int32_t rc = neigh_check_query(c, who, q);
    if (rc != GS_OK) return rc;
    rc = neigh_check_filters(c, who, q->mask, q->value, q->mask, q->value, q->radius, &r2); // (the one filter on both sides)
    if (rc != GS_OK) return rc;
    const bool have = q->priority.kind != GS_THIN_NO_PRIORITY;
    char msg[160];
    if (!thin_check(q, have, msg, sizeof(msg))) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %s", who, msg);
    GsAttrDev dev{};
    if (have && (rc = attr_check(who, &q->priority, &dev)) != GS_OK) return rc;
    rc = resident_drain(c, true); // (the counter: the slots the commit folds kept and largest into)
    if (rc != GS_OK) return rc;
    rc = thin_planes(c, c->stream);
    if (rc != GS_OK) return rc;
    if (have && attr_needs_cover(&q->priority) && (rc = cover_planes(c, c->stream)) != GS_OK) return rc;
    gs_thin_info out{};
    if (info) *info = out;
    const uint32_t n = c->n;
    if (!n) { HIP_TRY(hipStreamSynchronize(c->stream)); return GS_OK; }
    gs_ctx::Neigh& s = c->ng;
    rc = c->th.rank.reserve(n); // (before the first launch: a failed allocation leaves the planes as they were)
    if (rc != GS_OK) return rc;
    NeighBuilt b;
    rc = neigh_grid(c, who, q->radius, q->mask, q->value, q->mask, q->value, q->max_candidates, &b, [&](const NeighBuilt& b) {
        out.members = b.sources;
        out.candidates = b.candidates;
        out.cell_edge = b.cell_edge;
        for (int k = 0; k < 3; ++k) out.cells[k] = b.g.g[k];
        if (info) *info = out;
    });
    if (rc != GS_OK) return rc;

    // the records are written: the sort's arrays are free.  Without a grid (no member with finite coordinates) init alone decides.
    uint32_t *status = s.keysA, *wkeeper = s.valsA, *wcovers = s.keysB;
    float* prio = have ? (float*)s.valsB.get() : nullptr;
    unsigned long long* rank = c->th.rank;
    const uint32_t nrec = b.grid ? b.src.nrec : 0u;
    gs_launch_thin_init(b.state, c->scene, n, q->mask, q->value, wkeeper, wcovers, c->stream);
    if (have && nrec) gs_launch_attr_values(q->priority.kind, c->scene, c->cov, n, dev, nullptr, 0u, n, prio, c->stream);
    gs_launch_thin_rank(s.src, nrec, n, prio, q->flags, q->seed, rank, status, c->stream);
    HIP_TRY(hipGetLastError());
    const uint32_t max_rounds = q->max_rounds ? q->max_rounds : GS_THIN_DEFAULT_ROUNDS;
    for (uint32_t undecided = nrec; undecided != 0u;) {
        if (out.rounds >= max_rounds)
            return fail(GS_ERR_CAPACITY, "%s: %u members are still undecided after %u rounds (max_rounds; the order makes chains of linked members that long)",
                        who, undecided, out.rounds);
        const uint32_t round = out.rounds + 1u; // the stamp of this round's decisions: never 0
        rc = neigh_open_word(c, [&](uint32_t* word) {
            neigh_slices(b.sums, [&](uint32_t b0, uint32_t blocks) { gs_launch_thin_round(b, b0, blocks, r2, round, rank, status, word, c->stream); });
        }, &undecided);
        if (rc != GS_OK) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        ++out.rounds;
    }
    if (nrec) neigh_slices(b.sums, [&](uint32_t b0, uint32_t blocks) { gs_launch_thin_assign(b, b0, blocks, r2, n, rank, status, wkeeper, wcovers, c->stream); });
    constexpr size_t kSlotWords = (size_t)GS_STATE_SLOTS * GS_STATE_SLOT_STRIDE;
    HIP_TRY(hipMemsetAsync(c->st.counter, 0, kSlotWords * 8, c->stream));
    gs_launch_thin_commit(wkeeper, wcovers, n, c->th.keeper, c->th.covers, c->st.counter, c->stream);
    HIP_TRY(hipGetLastError());
    unsigned long long h[kSlotWords];
    HIP_TRY(hipMemcpyAsync(h, c->st.counter, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < GS_STATE_SLOTS; ++k) {
        out.kept += h[k * GS_STATE_SLOT_STRIDE];
        out.largest = std::max<uint64_t>(out.largest, h[k * GS_STATE_SLOT_STRIDE + 1]);
    }
    out.dropped = out.members - out.kept;
    if (info) *info = out;
    return GS_OK;
}

GS_EXPORT int32_t gs_thin_read(gs_ctx* c, uint32_t* keeper, uint32_t* covers, uint64_t cap, uint64_t* n) {
    void* const out[2] = {keeper, covers};
    const auto planes = [](gs_ctx* c, const uint32_t* p[2]) { const int32_t rc = thin_planes(c, c->stream); p[0] = c->th.keeper; p[1] = c->th.covers; return rc; };
    return plane_read(c, "gs_thin_read", planes, "words per plane needed, the buffers hold", out, cap, n);
}

GS_EXPORT int32_t gs_thin_host(const float* px, const float* py, const float* pz, uint64_t n, const uint8_t* state, const float* priority, const gs_thin* q,
                               uint32_t* keeper, uint32_t* covers, gs_thin_info* info) {
    char msg[160];
    if (thin_host(px, py, pz, n, state, priority, q, keeper, covers, info, msg, sizeof(msg)) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_thin_host: %s", msg);
    return GS_OK;
}
