// gs_plane_pairs.hip -- the plane pair moments' entry points: the exact sums of the point-to-plane normal equations over the matched
// pairs (p_i, p_partner[i], normal[partner[i]]) of the resident splats that pass a state filter, and the same numbers from host
// planes.  Part of the C ABI (include/gsplat/gs_abi.h "registration"); the kernel is in k_plane_pairs.hip, the row, the pairing rule,
// the quantity order and the host loop in gs_plane_pair_host.h, the arithmetic in gs_exact_sum.h.
//
// The reference has no counterpart: it is a viewer.  An editor on it would export both captures and the normals, run a host ICP and
// upload again; here a step's sums are 480 bytes after one streaming pass, and gsplat.register.fit_plane solves them.
//
// gs_pair_plane_moments drains the context's ring first (gs_wait), runs on the context's stream and returns when done, as
// gs_pair_moments does.  It launches nothing in a frame: a context that never calls it launches exactly what it did before.
#include <cmath>

#include "gs_runtime.h"
#include "gs_plane_pair_host.h"

static_assert(sizeof(struct gs_pair_plane_moments) == 480 && offsetof(struct gs_pair_plane_moments, G) == 16 && offsetof(struct gs_pair_plane_moments, h) == 352 &&
                  offsetof(struct gs_pair_plane_moments, rr) == 448 && offsetof(struct gs_pair_plane_moments, d2) == 464,
              "gs_pair_plane_moments layout");
static_assert(GS_PLANE_PAIRS_SLOT_WORDS >= GS_PLANE_QUANTITIES * GS_EX_LIMBS + 2u, "a slot holds 29 limb tables and the two counts");

// The record from the 29 limb tables in gs_plane_pair_host.h's order, which is the record's own: each sum finished once.
static void plane_finish(const int64_t* tables, uint64_t matched, uint64_t paired, struct gs_pair_plane_moments* out) {
    memset(out, 0, sizeof(*out));
    out->matched = matched;
    out->paired = paired;
    gs_exact* e = out->G; // G, h, rr, d2 are contiguous (the layout is asserted above)
    for (uint32_t t = 0; t < GS_PLANE_QUANTITIES; ++t) ex_finish(tables + (size_t)t * GS_EX_LIMBS, &e[t].hi, &e[t].lo);
}

// what both calls refuse after their own prologue: the bound, the pivot, the record
static int32_t plane_check(const char* who, const float* pivot, float max_dist2, const void* out) {
    if (!(max_dist2 >= 0.0f)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: max_dist2 %g is negative or NaN", who, (double)max_dist2);
    if (!pivot) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null pivot", who);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(pivot[a])) return fail(GS_ERR_INVALID_ARGUMENT, "%s: pivot[%d] = %g is not finite", who, a, (double)pivot[a]);
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null moments", who);
    return GS_OK;
}

GS_EXPORT int32_t gs_pair_plane_moments(gs_ctx* c, uint32_t mask, uint32_t value, const uint32_t* partner, const float* normal, const float pivot[3],
                                        float max_dist2, struct gs_pair_plane_moments* out) {
    static const char* who = "gs_pair_plane_moments";
    int32_t rc = resident_check(c, who, Plane::filtered, mask, value);
    if (rc != GS_OK) return rc;
    rc = plane_check(who, pivot, max_dist2, out);
    if (rc != GS_OK) return rc;
    if (c->n >= 0x80000000u) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %llu splats, a limb holds fewer than 2^31 terms", who, (unsigned long long)c->n);
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    const uint8_t* state = (mask | value) ? c->scene.state : nullptr;
    constexpr size_t kWords = (size_t)GS_PLANE_PAIRS_SLOTS * GS_PLANE_PAIRS_SLOT_WORDS;
    std::vector<unsigned long long> h(kWords, 0ull);
    if (c->n) {
        const uint32_t* ids;
        if (partner) { // a host array: to the context's scratch first
            rc = c->pr.partner.reserve(((uint64_t)c->n + 3u) & ~3ull);
            if (rc != GS_OK) return rc;
            HIP_TRY(hipMemcpyAsync(c->pr.partner, partner, (size_t)c->n * 4, hipMemcpyHostToDevice, c->stream));
            ids = c->pr.partner;
        } else { // the context's own nearest plane, in place: GS_KNN_NONE everywhere when it was never searched or has been dropped
            rc = knn_planes(c, c->stream);
            if (rc != GS_OK) return rc;
            ids = c->kn.nearest;
        }
        const void* nrm;
        std::vector<float> staged; // (alive until the stream has been waited for below)
        if (normal) { // a host array: into the surface plane's 16-byte records, then to the context's scratch -- one device layout
            staged.resize((size_t)c->n * 4);
            for (size_t i = 0; i < (size_t)c->n; ++i) {
                staged[4 * i] = normal[3 * i]; staged[4 * i + 1] = normal[3 * i + 1]; staged[4 * i + 2] = normal[3 * i + 2]; staged[4 * i + 3] = 0.0f;
            }
            rc = c->pp.normal.reserve((uint64_t)c->n * 4u);
            if (rc != GS_OK) return rc;
            HIP_TRY(hipMemcpyAsync(c->pp.normal, staged.data(), (size_t)c->n * 16, hipMemcpyHostToDevice, c->stream));
            nrm = c->pp.normal;
        } else { // the context's own surface plane, in place: NaN everywhere when it was never estimated or has been dropped
            rc = surface_planes(c, c->stream);
            if (rc != GS_OK) return rc;
            nrm = c->sf.nrm;
        }
        if (!c->pp.slots) HIP_TRY(hipMalloc(c->pp.slots.out(), kWords * 8));
        HIP_TRY(hipMemsetAsync(c->pp.slots, 0, kWords * 8, c->stream));
        gs_launch_plane_pairs(state, c->scene.px, c->scene.py, c->scene.pz, ids, nrm, c->n, mask, value, pivot[0], pivot[1], pivot[2], max_dist2, c->pp.slots,
                              c->opt.grid_persist, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h.data(), c->pp.slots, kWords * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    // the copies add up in wrapping unsigned arithmetic; the totals are within i64 (gs_exact_sum.h)
    constexpr uint32_t words = GS_PLANE_QUANTITIES * GS_EX_LIMBS + 2u;
    int64_t total[words] = {};
    for (uint32_t s = 0; s < GS_PLANE_PAIRS_SLOTS; ++s)
        for (uint32_t i = 0; i < words; ++i) total[i] = (int64_t)((uint64_t)total[i] + (uint64_t)h[(size_t)s * GS_PLANE_PAIRS_SLOT_WORDS + i]);
    plane_finish(total, (uint64_t)total[words - 2u], (uint64_t)total[words - 1u], out);
    return GS_OK;
}

GS_EXPORT int32_t gs_pair_plane_moments_host(const float* px, const float* py, const float* pz, uint64_t n, const uint32_t* partner, const float* normal,
                                             const uint8_t* state, uint32_t mask, uint32_t value, const float pivot[3], float max_dist2,
                                             struct gs_pair_plane_moments* out) {
    static const char* who = "gs_pair_plane_moments_host";
    if ((!px || !py || !pz) && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null position plane", who);
    if (!partner && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null partner", who);
    if (!normal && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null normal", who);
    if (mask > 0xFFu || value > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "%s: filter (0x%x, 0x%x) does not fit the state byte", who, mask, value);
    if ((mask | value) && !state && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null state with the filter (0x%x, 0x%x)", who, mask, value);
    const int32_t rc = plane_check(who, pivot, max_dist2, out);
    if (rc != GS_OK) return rc;
    if (n >= 0x80000000ull) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %llu splats, a limb holds fewer than 2^31 terms", who, (unsigned long long)n);
    PlaneSums s;
    plane_sums_clear(&s);
    for (uint64_t i = 0; i < n; ++i) plane_host_one(&s, px, py, pz, n, partner, normal, state, mask, value, pivot, max_dist2, i);
    plane_finish(s.t, s.matched, s.paired, out);
    return GS_OK;
}
