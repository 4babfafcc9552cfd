// gs_merge.hip -- the cell merge's entry points: one moment-matched splat per grid cell of the resident splats (gs_cell_merge,
// gs_cell_merge_device) and the same computation over host records (gs_cell_merge_host).  Part of the C ABI (include/gsplat/gs_abi.h
// "cell merge"); the kernels are in k_merge.hip, every expression of the definition and the host loop in gs_merge_math.h.
//
// The reference has no counterpart: it is a viewer.  An editor on it would export the 320-byte records, decimate them in a host script
// and upload the result; here the scene stays resident, 8 bytes per splat go through the neighbourhoods' pair sort, and only the
// merged records exist anywhere else.
//
// A merge is: the bounds of the filter's finite splats (the neighbourhoods' pass and read-back), the grid on the host, keys with the
// eligibility test, the Onesweep pair sort behind the private control block (private_sort), the run heads as a byte plane, the splat
// edits' stream compaction over that plane (the run begins), the runs' lengths and which of them are merged -- a byte plane again,
// compacted into the group numbering -- and, unless only the counts are wanted, the sums kernel and the finishing kernel in trips of
// kTripGroups groups; last, the state pass over the members' ids (gs_state_ids' kernel).  The calls drain the context's ring first
// (gs_wait), run on the context's stream and return when done.  None of them launches anything in a frame.
#include <cmath>

#include "gs_merge_math.h"
#include "gs_runtime.h"

static_assert(sizeof(gs_merge) == 32 && offsetof(gs_merge, cell) == 12 && offsetof(gs_merge, bits) == 28, "gs_merge layout");
static_assert(sizeof(gs_merge_info) == 48 && offsetof(gs_merge_info, largest) == 24 && offsetof(gs_merge_info, cells) == 32 &&
                  offsetof(gs_merge_info, cell_edge) == 44,
              "gs_merge_info layout");

// groups per trip through the sums (128 MB) and, for a host destination, the records (80 MB)
static constexpr uint64_t kTripGroups = 1ull << 18;

// The positions of the bytes that read 1 among flag[0 .. m), ascending, into `out`; *total: how many.  Returns with the count known
// (the stream is synchronised before the scatter is enqueued).
static int32_t ones(gs_ctx* c, const uint8_t* flag, uint32_t m, Scratch<uint32_t>& out, uint32_t* total) {
    const uint32_t nb = gs_select_blocks(m);
    int32_t rc = c->mg.counts.reserve((uint64_t)nb + 1);
    if (rc != GS_OK) return rc;
    gs_launch_select_count(flag, m, 1u, 1u, c->mg.counts, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(total, c->mg.counts.get() + nb, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!*total) return GS_OK;
    rc = out.reserve(*total);
    if (rc != GS_OK) return rc;
    gs_launch_select_scatter(flag, m, 1u, 1u, c->mg.counts, out, *total, c->stream);
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

static int32_t merge_refusals(const char* who, const gs_merge* p, const void* out, uint64_t cap) {
    const char* why = nullptr;
    if (!merge_params_ok(p, &why)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %s", who, why);
    if (!out && cap) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null records with cap_records %llu", who, (unsigned long long)cap);
    return GS_OK;
}
static int32_t merge_too_full(const char* who, const gs_merge* p, const gs_merge_info& I) {
    return fail(GS_ERR_CAPACITY, "%s: the fullest cell holds %llu eligible splats, above max_members = %u (cell edge %g puts too many splats into one cell)", who,
                (unsigned long long)I.largest, merge_max_members(p), (double)I.cell_edge);
}
static int32_t merge_too_small(const char* who, const gs_merge_info& I, uint64_t cap) {
    return fail(GS_ERR_INVALID_ARGUMENT, "%s: %llu records needed, the buffer holds %llu", who, (unsigned long long)I.groups, (unsigned long long)cap);
}

static int32_t merge_common(gs_ctx* c, const char* who, const gs_merge* p, void* out, uint64_t cap, double* sums, uint32_t* group_of,
                            gs_merge_info* info, bool device) {
    int32_t rc = merge_refusals(who, p, out, cap); // (the parameters first: their refusals need no context)
    if (rc != GS_OK) return rc;
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null ctx", who);
    rc = resident_check(c, who, Plane::filtered, p->mask, p->value);
    if (rc != GS_OK) return rc;
    if (p->op && (rc = resident_check(c, who, Plane::always)) != GS_OK) return rc;
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    gs_merge_info I{};
    if (info) *info = I;
    const uint32_t n = c->n;
    const bool count_only = !out;
    auto nothing = [&]() -> int32_t { // no group: every splat reads GS_MERGE_NONE
        if (!count_only && group_of)
            for (uint32_t i = 0; i < n; ++i) group_of[i] = GS_MERGE_NONE;
        HIP_TRY(hipStreamSynchronize(c->stream));
        return GS_OK;
    };
    if (!n) return nothing();
    if (n >= (1u << 30)) return fail(GS_ERR_CAPACITY, "%s: %u splats, the cell sort takes fewer than 2^30", who, n); // (gs_sort_pairs_u32's limit)
    auto& s = c->mg;
    const uint8_t* state = (p->mask | p->value) ? c->scene.state : nullptr;

    // scratch of the counting part (all of it before the first launch)
    if ((rc = private_sort_reserve(c, n, 4)) != GS_OK || (rc = s.flags.reserve(n)) != GS_OK || (rc = s.stats.reserve(4)) != GS_OK ||
        (rc = s.counts.reserve((uint64_t)gs_select_blocks(n) + 1)) != GS_OK)
        return rc;

    // 1. the bounds (filter plus finite position) and the grid
    uint32_t hb[16];
    if ((rc = neigh_bounds(c, state, p->mask, p->value, p->mask, p->value, hb)) != GS_OK) return rc;
    if (!hb[7]) return nothing();
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = pk_okey_value(hb[k]); hi[k] = pk_okey_value(hb[3 + k]); }
    GsNeighGrid g;
    neigh_choose_grid(lo, hi, p->cell, &g, &I.cell_edge);
    for (int k = 0; k < 3; ++k) I.cells[k] = g.g[k];

    // 2. the eligible splats in (cell, id) order
    const uint32_t passes = (neigh_bits_of(g.none) + 7) / 8; // the keys reach `none` itself
    GsSortPair sorted;
    rc = private_sort(c, n, passes, [&] { gs_launch_merge_keys(state, c->scene, n, p->mask, p->value, g, c->ng.keysA, c->ng.valsA, c->stream); }, &sorted);
    if (rc != GS_OK) return rc;
    HIP_TRY(hipGetLastError());
    uint32_t fault = 0;
    if ((rc = private_sort_fault(c, &fault)) != GS_OK) return rc;

    // 3. the runs: their begins, their lengths, which are merged, the group numbering
    gs_launch_merge_heads(sorted.keys, n, s.flags, c->stream);
    HIP_TRY(hipGetLastError());
    uint32_t runs = 0, G = 0, hs[4] = {0u, 0u, 0u, 0u};
    if ((rc = ones(c, s.flags, n, s.heads, &runs)) != GS_OK) { (void)hipStreamSynchronize(c->stream); return rc; } // (the copy into `fault` is done with)
    if (fault) return fail(GS_ERR_DEVICE_FAULT, "%s: look-back spin bound exceeded in the cell sort", who);
    HIP_TRY(hipMemsetAsync(s.stats, 0, 16, c->stream));
    gs_launch_merge_runs(sorted.keys, s.heads, runs, n, g.none, p->min_members, s.flags, s.stats, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hs, s.stats, 16, hipMemcpyDeviceToHost, c->stream));
    if ((rc = ones(c, s.flags, runs, s.mruns, &G)) != GS_OK) { (void)hipStreamSynchronize(c->stream); return rc; } // (... and the one into `hs`)
    I.eligible = hs[0];
    I.largest = hs[1];
    I.members = hs[2];
    I.groups = G;
    if (info) *info = I;
    if (I.largest > merge_max_members(p)) { (void)hipStreamSynchronize(c->stream); return merge_too_full(who, p, I); }
    if (count_only) return nothing();
    if (cap < G) { (void)hipStreamSynchronize(c->stream); return merge_too_small(who, I, cap); }

    // 4. sums and records, in trips
    const uint64_t trip = std::min<uint64_t>(std::max<uint64_t>(G, 1), kTripGroups);
    if ((rc = s.sums.reserve(trip * GS_MERGE_SUM_DOUBLES)) != GS_OK || (!device && (rc = s.rec.reserve(trip * GS_SPLAT_RECORD_BYTES)) != GS_OK) ||
        (group_of && (rc = s.group_of.reserve(n)) != GS_OK) || (p->op && (rc = s.member.reserve(n)) != GS_OK))
        return rc;
    if (group_of) HIP_TRY(hipMemsetAsync(s.group_of, 0xFF, (size_t)n * 4, c->stream));
    if (p->op) HIP_TRY(hipMemsetAsync(s.member, 0, n, c->stream));
    for (uint64_t first = 0; first < G; first += trip) {
        const uint32_t k = (uint32_t)std::min<uint64_t>(trip, G - first);
        gs_launch_merge_sums(sorted.vals, s.heads, runs, s.mruns, (uint32_t)first, k, n, c->scene, n, s.sums, group_of ? s.group_of.get() : nullptr,
                             p->op ? s.member.get() : nullptr, c->stream);
        void* dst = device ? (void*)((char*)out + first * GS_SPLAT_RECORD_BYTES) : (void*)s.rec.get();
        gs_launch_merge_finish(s.sums, k, dst, c->stream);
        HIP_TRY(hipGetLastError());
        if (sums) HIP_TRY(hipMemcpyAsync(sums + first * GS_MERGE_SUM_DOUBLES, s.sums, (size_t)k * GS_MERGE_SUM_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (!device) HIP_TRY(hipMemcpyAsync((char*)out + first * GS_SPLAT_RECORD_BYTES, s.rec, (size_t)k * GS_SPLAT_RECORD_BYTES, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream)); // before the next trip overwrites the scratch
    }
    if (group_of) HIP_TRY(hipMemcpyAsync(group_of, s.group_of, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));

    // 5. the outputs are complete: mark the members
    if (p->op) {
        uint32_t members = 0;
        if ((rc = ones(c, s.member, n, s.ids, &members)) != GS_OK) return rc;
        gs_launch_state_ids(const_cast<uint8_t*>(c->scene.state), s.ids, members, p->op, p->bits, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return GS_OK;
}

GS_EXPORT int32_t gs_cell_merge(gs_ctx* c, const gs_merge* p, void* aos320, uint64_t cap_records, double* sums, uint32_t* group_of, gs_merge_info* info) {
    return merge_common(c, "gs_cell_merge", p, aos320, cap_records, sums, group_of, info, false);
}
GS_EXPORT int32_t gs_cell_merge_device(gs_ctx* c, const gs_merge* p, void* d_aos320, uint64_t cap_records, double* sums, uint32_t* group_of,
                                       gs_merge_info* info) {
    return merge_common(c, "gs_cell_merge_device", p, d_aos320, cap_records, sums, group_of, info, true);
}

GS_EXPORT int32_t gs_cell_merge_host(const void* records, uint8_t* state, uint64_t n, const gs_merge* p, void* aos320, uint64_t cap_records, double* sums,
                                     uint32_t* group_of, gs_merge_info* info) {
    static const char* who = "gs_cell_merge_host";
    const int32_t rc = merge_refusals(who, p, aos320, cap_records);
    if (rc != GS_OK) return rc;
    if (!records && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null records", who);
    if ((p->mask | p->value | p->op) && !state && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null state with a filter or an op", who);
    if (n >= (1ull << 30)) return fail(GS_ERR_CAPACITY, "%s: %llu splats, the cell sort takes fewer than 2^30", who, (unsigned long long)n);
    gs_merge_info I{};
    const int r = merge_host((const float*)records, state, n, p, (float*)aos320, cap_records, sums, group_of, &I);
    if (info) *info = I;
    if (r == 1) return merge_too_full(who, p, I);
    if (r == 2) return merge_too_small(who, I, cap_records);
    return GS_OK;
}
