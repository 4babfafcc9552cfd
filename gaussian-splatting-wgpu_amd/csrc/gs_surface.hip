// gs_surface.hip -- surface's entry points: the integer moments of every query's neighbourhood, finished into a normal and three shape
// eigenvalues in the planes; read the planes and the kept sums; the same computation over host positions (gs_surface_host).  The
// selection by a feature, gs_state_surface, is with the state calls in gs_state.hip.  Part of the C ABI (include/gsplat/gs_abi.h
// "surface"); the kernels are in k_surface.hip, every expression of the definition and the host loop in gs_surface_math.h.
//
// The reference has no counterpart: it is a viewer.  An editor on it would export its 320-byte records, query a k-d tree and run a
// PCA per point on the host; here an estimate is a neighbour count's grid (neigh_build, gs_neigh.hip: one copy) with nine integer
// sums in place of the count, and 28 bytes per splat come back.
//
// An estimate is: the refusals, the grid, records and candidates (neigh_build), the budget, every allocation, then -- only now is
// anything written: a call that fails before leaves the planes and the kept sums as they were -- the planes' start, the query pass
// in the count's slices, each cut into runs of at most kSliceBlocks workgroups and followed by its finishing pass, one word read
// back (the queries that end with count < 3).  Every call drains the context's ring first (gs_wait), runs on the context's stream
// and returns when done.  None of them launches anything in a frame.
#include "gs_neigh_host.h"
#include "gs_surface_math.h"

static_assert(sizeof(gs_surface) == 56 && offsetof(gs_surface, toward) == 28 && offsetof(gs_surface, max_candidates) == 40 && offsetof(gs_surface, reserved) == 48,
              "gs_surface layout");
static_assert(sizeof(gs_surface_info) == 48 && offsetof(gs_surface_info, unresolved) == 24 && offsetof(gs_surface_info, cells) == 32 &&
                  offsetof(gs_surface_info, cell_edge) == 44,
              "gs_surface_info layout");
static_assert(sizeof(gs_surface_range) == 32 && offsetof(gs_surface_range, inside) == 16 && offsetof(gs_surface_range, axis) == 20, "gs_surface_range layout");
static_assert(GS_SURFACE_SUM_WORDS == SF_SUM_WORDS, "the sums' words");

// workgroups of 256 queries per run of the query pass without GS_SURFACE_KEEP_SUMS: 80 MB of sums in flight
static constexpr uint32_t kSliceBlocks = 4096;

static size_t record_bytes(const gs_ctx* c) { return std::max<size_t>((size_t)c->n * 16, 256); }

int32_t surface_planes(gs_ctx* c, hipStream_t st) {
    if (c->sf.nrm && c->sf.eig) return GS_OK;
    DevBuf<> nrm, eig; // both or neither
    HIP_TRY(hipMalloc(nrm.out(), record_bytes(c)));
    HIP_TRY(hipMalloc(eig.out(), record_bytes(c)));
    c->sf.nrm = std::move(nrm);
    c->sf.eig = std::move(eig);
    c->sf.have_sums = false;
    gs_launch_surface_init(c->n, c->sf.nrm, c->sf.eig, st); // NaN / count 0: no estimate yet
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

GS_EXPORT int32_t gs_surface_estimate(gs_ctx* c, const gs_surface* q, gs_surface_info* info) {
    const char* who = "gs_surface_estimate";
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null ctx", who);
    SfScale sc;
    char why[160];
    if (!sf_check(q, &sc, why, sizeof why)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %s", who, why);
    float r2; // (sf_check has refused every radius this refuses; r2 is sc.r2)
    int32_t rc = neigh_check_filters(c, who, q->src_mask, q->src_value, q->qry_mask, q->qry_value, q->radius, &r2);
    if (rc != GS_OK) return rc;
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    rc = surface_planes(c, c->stream);
    if (rc != GS_OK) return rc;
    gs_surface_info out{};
    if (info) *info = out;
    const uint32_t n = c->n;
    const bool keep = (q->flags & GS_SURFACE_KEEP_SUMS) != 0u;
    if (!n) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->sf.have_sums = keep; // (zero splats, zero sums)
        return GS_OK;
    }
    NeighBuilt b;
    rc = neigh_grid(c, who, q->radius, q->src_mask, q->src_value, q->qry_mask, q->qry_value, q->max_candidates, &b, [&](const NeighBuilt& b) {
        neigh_report(&out, b);
        if (info) *info = out;
    });
    if (rc != GS_OK) return rc;
    const uint32_t nblocks = b.grid ? (b.nqry + 255u) / 256u : 0u;
    // the last allocations: the kept plane, or -- with a grid -- the scratch of one run
    if (keep && !c->sf.sums) {
        HIP_TRY(hipMalloc(c->sf.sums.out(), std::max<size_t>((size_t)n * SF_SUM_WORDS * 8, 256)));
    } else if (!keep && b.grid) {
        rc = c->sf.slice.reserve((uint64_t)std::min(nblocks, kSliceBlocks) * 256u * SF_SUM_WORDS);
        if (rc != GS_OK) return rc;
    }

    // from here on the planes are written.  A query without a record (a non-finite coordinate; every query when there is no grid:
    // nothing to find) keeps the NaN and the count 0 it is given here.
    c->sf.have_sums = false;
    gs_launch_surface_init(n, c->sf.nrm, c->sf.eig, c->stream);
    HIP_TRY(hipGetLastError());
    if (keep) HIP_TRY(hipMemsetAsync(c->sf.sums, 0, (size_t)n * SF_SUM_WORDS * 8, c->stream));
    uint32_t open = 0; // finite queries the pass leaves with count < 3
    if (b.grid) {
        const uint64_t stride = keep ? 1u : (uint64_t)std::min(nblocks, kSliceBlocks) * 256u;
        int64_t* sums = keep ? c->sf.sums.get() : c->sf.slice.get();
        const bool orient = (q->flags & GS_SURFACE_ORIENT) != 0u;
        rc = neigh_open_word(c, [&](uint32_t* word) {
            neigh_slices(b.sums, [&](uint32_t b0, uint32_t blocks) {
                for (uint32_t done = 0; done < blocks; done += kSliceBlocks) { // (the finishing pass has read a run's scratch before the next writes it: one stream)
                    const uint32_t first = b0 + done, m = std::min(blocks - done, kSliceBlocks);
                    gs_launch_surface_query(b, first, m, sc.r2, sc.s, n, sums, keep, stride, word, c->stream);
                    const uint32_t t0 = first * 256u;
                    gs_launch_surface_finish(b.qrec, t0, std::min(m * 256u, b.nqry - t0), n, sums, keep, stride, sc.unscale, orient, q->toward, c->sf.nrm,
                                             c->sf.eig, c->stream);
                }
            });
        }, &open);
        if (rc != GS_OK) return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->sf.have_sums = keep;
    out.unresolved = b.grid ? (b.queried - b.nqry) + open : b.queried;
    if (info) *info = out;
    return GS_OK;
}

GS_EXPORT int32_t gs_surface_read(gs_ctx* c, float* normal, float* eig, uint32_t* count, uint64_t cap, uint64_t* n) {
    int32_t rc = resident_begin(c, "gs_surface_read", Plane::none);
    if (rc != GS_OK) return rc;
    rc = surface_planes(c, c->stream);
    if (rc != GS_OK) return rc;
    if (!n) return fail(GS_ERR_INVALID_ARGUMENT, "gs_surface_read: null n");
    *n = c->n;
    if (!normal && !eig && !count) { HIP_TRY(hipStreamSynchronize(c->stream)); return GS_OK; }
    if (cap < c->n)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_surface_read: %llu splats per plane needed, the buffers hold %llu", (unsigned long long)c->n, (unsigned long long)cap);
    if (c->n) {
        const size_t m = c->n;
        rc = c->sf.out.reserve(7 * (uint64_t)m); // normal 3 m, eig 3 m, count m
        if (rc != GS_OK) return rc;
        uint32_t* o = c->sf.out;
        gs_launch_surface_unpack(c->sf.nrm, c->n, (float*)o, o + 6 * m, c->stream);
        gs_launch_surface_unpack(c->sf.eig, c->n, (float*)(o + 3 * m), nullptr, c->stream);
        HIP_TRY(hipGetLastError());
        if (normal) HIP_TRY(hipMemcpyAsync(normal, o, m * 12, hipMemcpyDeviceToHost, c->stream));
        if (eig) HIP_TRY(hipMemcpyAsync(eig, o + 3 * m, m * 12, hipMemcpyDeviceToHost, c->stream));
        if (count) HIP_TRY(hipMemcpyAsync(count, o + 6 * m, m * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

GS_EXPORT int32_t gs_surface_read_sums(gs_ctx* c, int64_t* sums, uint64_t cap, uint64_t* n) {
    int32_t rc = resident_begin(c, "gs_surface_read_sums", Plane::none);
    if (rc != GS_OK) return rc;
    if (!n) return fail(GS_ERR_INVALID_ARGUMENT, "gs_surface_read_sums: null n");
    if (!c->sf.have_sums)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_surface_read_sums: no sums kept: the last gs_surface_estimate on this ctx had no GS_SURFACE_KEEP_SUMS (flag 0x%x), or there was none",
                    GS_SURFACE_KEEP_SUMS);
    *n = c->n;
    if (!sums) return GS_OK;
    if (cap < c->n)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_surface_read_sums: %llu splats needed, the buffer holds %llu", (unsigned long long)c->n, (unsigned long long)cap);
    if (c->n) HIP_TRY(hipMemcpyAsync(sums, c->sf.sums, (size_t)c->n * SF_SUM_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

GS_EXPORT int32_t gs_surface_host(const float* pos, const uint8_t* state, uint64_t n, const gs_surface* q, float* normal, float* eig, uint32_t* count,
                                  int64_t* sums, gs_surface_info* info) {
    const char* who = "gs_surface_host";
    SfScale sc;
    char why[160];
    if (!sf_check(q, &sc, why, sizeof why)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %s", who, why);
    if (q->src_mask > 0xFFu || q->src_value > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "%s: filter (0x%x, 0x%x) does not fit the state byte", who, q->src_mask, q->src_value);
    if (q->qry_mask > 0xFFu || q->qry_value > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "%s: filter (0x%x, 0x%x) does not fit the state byte", who, q->qry_mask, q->qry_value);
    if (n && (!pos || !normal || !eig || !count)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null array with n = %llu", who, (unsigned long long)n);
    if (n && !state && (q->src_mask | q->src_value | q->qry_mask | q->qry_value))
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: null state with a filter other than (0, 0) and n = %llu", who, (unsigned long long)n);
    if (n >= (1ull << 30)) return fail(GS_ERR_CAPACITY, "%s: %llu splats, the sums are proved for fewer than 2^30", who, (unsigned long long)n);
    gs_surface_info out{};
    surface_host(pos, state, n, q, sc, normal, eig, count, sums, &out);
    if (info) *info = out;
    return GS_OK;
}
