// gs_consensus.hip -- the consensus entry points: score up to GS_CONSENSUS_MAX plane or ball hypotheses against the resident splats in
// one pass (gs_attr_consensus), the same loop over host planes (gs_consensus_host), the values of given splats (gs_attr_gather) and the
// plane through three points (gs_planes_through).  Part of the C ABI (include/gsplat/gs_abi.h "consensus"); the kernel is in
// k_consensus.hip, the value, the host loop and the plane in gs_consensus_host.h; gs_attr_gather runs gs_attr_values_kernel (k_attr.hip).
//
// The reference has no counterpart: it is a viewer.  An editor on it would export the 320-byte records and run RANSAC in numpy; here a
// thousand candidate planes cost one streaming pass and 8 KB come back, and gsplat.consensus builds find_plane / select_plane /
// detect_planes / densest_ball on it.
//
// gs_attr_consensus and gs_attr_gather drain the context's ring first (gs_wait), run on the context's stream and return when done, as
// the splat attributes do.  Neither launches anything in a frame: a context that never calls them launches exactly what it did before.
#include <cmath>
#include <vector>

#include "gs_runtime.h"
#include "gs_consensus_host.h"

static constexpr size_t kCountWords = (size_t)GS_CONSENSUS_MAX;
static constexpr size_t kSlotWords = (size_t)GS_STATE_SLOTS * GS_STATE_SLOT_STRIDE;

// the refusals that host and device share; nothing is written before they have passed
static int32_t consensus_check(const char* who, uint32_t kind, const float* params, uint32_t h, float lo, float hi, const uint64_t* counts) {
    if (kind != GS_ATTR_PLANE && kind != GS_ATTR_DIST2)
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: kind %u is neither GS_ATTR_PLANE (%d) nor GS_ATTR_DIST2 (%d)", who, kind, (int)GS_ATTR_PLANE, (int)GS_ATTR_DIST2);
    if (h < 1u || h > GS_CONSENSUS_MAX) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %u hypotheses are not 1 .. %u", who, h, GS_CONSENSUS_MAX);
    if (std::isnan(lo) || std::isnan(hi)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: range [%g, %g] holds a NaN", who, (double)lo, (double)hi);
    if (!params) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null params", who);
    if (!counts) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null counts", who);
    return GS_OK;
}

GS_EXPORT int32_t gs_attr_consensus(gs_ctx* c, uint32_t kind, const float* params, uint32_t h, float lo, float hi, uint32_t mask, uint32_t value,
                                    uint64_t* counts, uint64_t* matched) {
    static const char* who = "gs_attr_consensus";
    int32_t rc = resident_check(c, who, Plane::filtered, mask, value);
    if (rc != GS_OK) return rc;
    rc = consensus_check(who, kind, params, h, lo, hi, counts);
    if (rc != GS_OK) return rc;
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    std::vector<unsigned long long> out(kCountWords + kSlotWords, 0ull);
    if (c->n) {
        const uint8_t* state = (mask | value) ? c->scene.state : nullptr;
        // the table, padded with NaNs to whole batches of the kernel's loop: a NaN parameter counts nothing
        const uint32_t hp = (h + GS_CONSENSUS_PAD - 1u) / GS_CONSENSUS_PAD * GS_CONSENSUS_PAD;
        std::vector<float> table((size_t)hp * 4u, std::nanf(""));
        memcpy(table.data(), params, (size_t)h * 4u * sizeof(float));
        if (!c->cs.counts) HIP_TRY(hipMalloc(c->cs.counts.out(), (kCountWords + kSlotWords) * sizeof(unsigned long long)));
        if (!c->cs.params) HIP_TRY(hipMalloc(c->cs.params.out(), kCountWords * 4u * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(c->cs.params, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(c->cs.counts, 0, (kCountWords + kSlotWords) * sizeof(unsigned long long), c->stream));
        gs_launch_consensus(kind, state, c->scene.px, c->scene.py, c->scene.pz, c->n, c->cs.params, hp, lo, hi, mask, value, c->cs.counts,
                            c->cs.counts.get() + kCountWords, c->opt.grid_persist, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out.data(), c->cs.counts, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream)); // (also: the table's host copy is done with)
    }
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64 counts");
    for (uint32_t j = 0; j < h; ++j) counts[j] = out[j];
    if (matched) {
        uint64_t total = 0;
        for (int k = 0; k < GS_STATE_SLOTS; ++k) total += out[kCountWords + (size_t)k * GS_STATE_SLOT_STRIDE];
        *matched = total;
    }
    return GS_OK;
}

GS_EXPORT int32_t gs_consensus_host(const float* px, const float* py, const float* pz, uint64_t n, const uint8_t* state, uint32_t mask, uint32_t value,
                                    uint32_t kind, const float* params, uint32_t h, float lo, float hi, uint64_t* counts, uint64_t* matched) {
    static const char* who = "gs_consensus_host";
    if ((!px || !py || !pz) && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null position plane", who);
    if (mask > 0xFFu || value > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "%s: filter (0x%x, 0x%x) does not fit the state byte", who, mask, value);
    if ((mask | value) && !state && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null state with the filter (0x%x, 0x%x)", who, mask, value);
    const int32_t rc = consensus_check(who, kind, params, h, lo, hi, counts);
    if (rc != GS_OK) return rc;
    uint64_t total = 0;
    for (uint32_t j = 0; j < h; ++j) counts[j] = 0;
    consensus_host_loop(kind, px, py, pz, n, state, mask, value, params, h, lo, hi, counts, &total);
    if (matched) *matched = total;
    return GS_OK;
}

// ids per trip through the scratch buffers (64 MB of ids, 64 MB of values)
static constexpr uint64_t kTripIds = 1ull << 24;

GS_EXPORT int32_t gs_attr_gather(gs_ctx* c, const gs_attr* a, const uint32_t* ids, uint64_t m, float* dst) {
    static const char* who = "gs_attr_gather";
    int32_t rc = resident_check(c, who, Plane::none);
    if (rc != GS_OK) return rc;
    GsAttrDev dev;
    rc = attr_check(who, a, &dev);
    if (rc != GS_OK) return rc;
    if (m && !ids) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null ids", who);
    if (m && !dst) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null dst", who);
    rc = resident_drain(c); // (c->n is the ring's to change until it has drained)
    if (rc != GS_OK) return rc;
    for (uint64_t g = 0; g < m; ++g)
        if (ids[g] >= c->n)
            return fail(GS_ERR_INVALID_ARGUMENT, "%s: ids[%llu] = %u is not below the %llu resident splats", who, (unsigned long long)g, ids[g], (unsigned long long)c->n);
    if (!m) return GS_OK;
    if (attr_needs_cover(a)) {
        rc = cover_planes(c, c->stream);
        if (rc != GS_OK) return rc;
    }
    const uint64_t trip = std::min(m, kTripIds);
    if ((rc = c->cs.ids.reserve(trip)) != GS_OK || (rc = c->at.vals.reserve(trip)) != GS_OK) return rc;
    for (uint64_t first = 0; first < m; first += kTripIds) {
        const uint64_t k = std::min(kTripIds, m - first);
        HIP_TRY(hipMemcpyAsync(c->cs.ids, ids + first, (size_t)k * 4, hipMemcpyHostToDevice, c->stream));
        gs_launch_attr_values(a->kind, c->scene, c->cov, c->n, dev, c->cs.ids, 0u, (uint32_t)k, c->at.vals, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(dst + first, c->at.vals, (size_t)k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream)); // before the next trip overwrites the scratch buffers
    }
    return GS_OK;
}

GS_EXPORT int32_t gs_planes_through(const float* points, uint32_t h, float* params) {
    static const char* who = "gs_planes_through";
    if (h && !points) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null points", who);
    if (h && !params) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null params", who);
    for (uint32_t j = 0; j < h; ++j) plane_through(points + (size_t)j * 9u, params + (size_t)j * 4u);
    return GS_OK;
}
