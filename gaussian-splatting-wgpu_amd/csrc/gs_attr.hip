// gs_attr.hip -- the splat attributes' read-only entry points: summarise, histogram and read resident splats by one f32 value per
// splat (the selection by value, gs_state_attr, is with the state calls in gs_state.hip).  Part of the C ABI
// (include/gsplat/gs_abi.h "splat attributes"); the kernels are in k_attr.hip.
//
// The reference has no counterpart: it is a viewer.  An editor on it would scan the 320-byte records its host kept
// (renderer.ts:130-137); here a question about one float per splat is one streaming pass over that float's plane or record, and
// what comes back is 24 bytes, bins + 3 counts or 4 bytes per match.
//
// Every call drains the context's ring first (gs_wait), runs on the context's stream and returns when done, as gs_state_* and the
// splat edits do.  None of them launches anything in a frame: a context that never calls them launches exactly what it did before.
#include <cmath>

#include "gs_runtime.h"

static_assert(sizeof(gs_attr) == 24 && sizeof(struct gs_attr_summary) == 24, "gs_attr / gs_attr_summary layout");
static_assert(sizeof(GsAttrSlot) <= GS_STATE_SLOT_STRIDE * sizeof(unsigned long long), "a summary record fits its slot");

int32_t attr_check(const char* who, const gs_attr* a, GsAttrDev* dev) {
    if (!a) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null attribute", who);
    if (a->struct_size != sizeof(gs_attr)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: struct_size %u != %zu", who, a->struct_size, sizeof(gs_attr));
    if (a->kind >= GS_ATTR_COUNT) return fail(GS_ERR_INVALID_ARGUMENT, "%s: unknown attribute kind %u (GS_ATTR_COUNT = %d)", who, a->kind, (int)GS_ATTR_COUNT);
    const int used = a->kind == GS_ATTR_DIST2 ? 3 : a->kind == GS_ATTR_PLANE ? 4 : 0;
    for (int k = 0; k < used; ++k)
        if (!std::isfinite(a->p[k])) return fail(GS_ERR_INVALID_ARGUMENT, "%s: p[%d] = %g of attribute kind %u is not finite", who, k, (double)a->p[k], a->kind);
    for (int k = 0; k < 4; ++k) dev->p[k] = k < used ? a->p[k] : 0.0f;
    return GS_OK;
}

// What the three calls do first: the refusals that cost nothing, the attribute's, the drain of the ring, the coverage planes where
// the kind reads them.  *state: the plane the kernels filter on, null for (0, 0) -- every splat passes and the plane is not read.
static int32_t attr_begin(gs_ctx* c, const char* who, const gs_attr* a, uint32_t mask, uint32_t value, const void* out, const char* out_name,
                          GsAttrDev* dev, const uint8_t** state) {
    int32_t rc = resident_check(c, who, Plane::filtered, mask, value);
    if (rc != GS_OK) return rc;
    rc = attr_check(who, a, dev);
    if (rc != GS_OK) return rc;
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null %s", who, out_name);
    *state = (mask | value) ? c->scene.state : nullptr;
    return GS_OK;
}
static int32_t attr_drain(gs_ctx* c, const gs_attr* a) {
    int32_t rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    return attr_needs_cover(a) ? cover_planes(c, c->stream) : GS_OK;
}

GS_EXPORT int32_t gs_attr_summary(gs_ctx* c, const gs_attr* a, uint32_t mask, uint32_t value, struct gs_attr_summary* out) {
    GsAttrDev dev;
    const uint8_t* state = nullptr;
    int32_t rc = attr_begin(c, "gs_attr_summary", a, mask, value, out, "summary", &dev, &state);
    if (rc != GS_OK) return rc;
    rc = attr_drain(c, a);
    if (rc != GS_OK) return rc;
    constexpr size_t kWords = (size_t)GS_STATE_SLOTS * GS_STATE_SLOT_STRIDE;
    if (!c->at.slots) HIP_TRY(hipMalloc(c->at.slots.out(), kWords * sizeof(unsigned long long)));
    unsigned long long h[kWords] = {};
    for (int k = 0; k < GS_STATE_SLOTS; ++k) {
        GsAttrSlot empty{0ull, 0ull, 0xFFFFFFFFu, 0u};
        memcpy(h + (size_t)k * GS_STATE_SLOT_STRIDE, &empty, sizeof(empty));
    }
    HIP_TRY(hipMemcpyAsync(c->at.slots, h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    gs_launch_attr_summary(a->kind, state, c->scene, c->cov, c->n, dev, mask, value, c->at.slots, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, c->at.slots, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    GsAttrSlot total{0ull, 0ull, 0xFFFFFFFFu, 0u};
    for (int k = 0; k < GS_STATE_SLOTS; ++k) {
        GsAttrSlot s;
        memcpy(&s, h + (size_t)k * GS_STATE_SLOT_STRIDE, sizeof(s));
        total.matched += s.matched;
        total.nan += s.nan;
        total.kmin = std::min(total.kmin, s.kmin);
        total.kmax = std::max(total.kmax, s.kmax);
    }
    auto value_of = [](uint32_t key) { // the inverse of the kernels' order-preserving map
        const uint32_t b = (key >> 31) ? key ^ 0x80000000u : ~key;
        float v;
        memcpy(&v, &b, 4);
        return v;
    };
    const bool any = total.kmin != 0xFFFFFFFFu; // (the identities are keys of NaNs)
    out->matched = total.matched;
    out->nan = total.nan;
    out->min = any ? value_of(total.kmin) : INFINITY;
    out->max = any ? value_of(total.kmax) : -INFINITY;
    return GS_OK;
}

GS_EXPORT int32_t gs_attr_histogram(gs_ctx* c, const gs_attr* a, uint32_t mask, uint32_t value, float lo, float hi, uint32_t bins, uint64_t* counts) {
    GsAttrDev dev;
    const uint8_t* state = nullptr;
    int32_t rc = attr_begin(c, "gs_attr_histogram", a, mask, value, counts, "counts", &dev, &state);
    if (rc != GS_OK) return rc;
    if (bins < 1u || bins > 1024u) return fail(GS_ERR_INVALID_ARGUMENT, "gs_attr_histogram: %u bins are not 1 .. 1024", bins);
    if (!std::isfinite(lo) || !std::isfinite(hi)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_attr_histogram: range [%g, %g) is not finite", (double)lo, (double)hi);
    if (!(lo < hi)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_attr_histogram: range [%g, %g) is empty", (double)lo, (double)hi);
    const float width = hi - lo;
    if (!std::isfinite(width)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_attr_histogram: the width of [%g, %g) is not finite in f32", (double)lo, (double)hi);
    const float scale = (float)bins / width; // once, in f32: the kernel and a restating host multiply by the same number
    rc = attr_drain(c, a);
    if (rc != GS_OK) return rc;
    const uint32_t words = bins + 3u;
    rc = c->at.hist.reserve(words);
    if (rc != GS_OK) return rc;
    HIP_TRY(hipMemsetAsync(c->at.hist, 0, (size_t)words * sizeof(unsigned long long), c->stream));
    gs_launch_attr_histogram(a->kind, state, c->scene, c->cov, c->n, dev, mask, value, lo, hi, scale, bins, c->at.hist, c->opt.grid_persist, c->stream);
    HIP_TRY(hipGetLastError());
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64 counts");
    HIP_TRY(hipMemcpyAsync(counts, c->at.hist, (size_t)words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

// values per trip through the scratch buffer (64 MB)
static constexpr uint64_t kTripValues = 1ull << 24;

GS_EXPORT int32_t gs_attr_read(gs_ctx* c, const gs_attr* a, uint32_t mask, uint32_t value, float* dst, uint64_t cap, uint64_t* n, uint32_t* ids) {
    GsAttrDev dev;
    const uint8_t* state = nullptr;
    int32_t rc = attr_begin(c, "gs_attr_read", a, mask, value, n, "n", &dev, &state);
    if (rc != GS_OK) return rc;
    rc = attr_drain(c, a);
    if (rc != GS_OK) return rc;
    const bool all = state == nullptr; // every splat, dense: no selection runs and value g is splat g's
    uint64_t total = c->n;
    if (!all) {
        rc = edit_select(c, mask, value, dst != nullptr, &total); // (the list is built in the context's scratch: a refusal writes nothing)
        if (rc != GS_OK) return rc;
    }
    *n = total;
    if (!dst) { HIP_TRY(hipStreamSynchronize(c->stream)); return GS_OK; }
    if (cap < total) return fail(GS_ERR_INVALID_ARGUMENT, "gs_attr_read: %llu values needed, the buffer holds %llu", (unsigned long long)total, (unsigned long long)cap);
    const uint32_t* sel = all ? nullptr : c->ex.ids.get();
    if (total) {
        rc = c->at.vals.reserve(std::min(total, kTripValues));
        if (rc != GS_OK) return rc;
    }
    for (uint64_t first = 0; first < total; first += kTripValues) {
        const uint64_t m = std::min(kTripValues, total - first);
        gs_launch_attr_values(a->kind, c->scene, c->cov, c->n, dev, sel, (uint32_t)first, (uint32_t)m, c->at.vals, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(dst + first, c->at.vals, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream)); // before the next trip overwrites the scratch buffer
    }
    if (ids) {
        if (all) for (uint64_t i = 0; i < total; ++i) ids[i] = (uint32_t)i;
        else if (total) HIP_TRY(hipMemcpyAsync(ids, c->ex.ids, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}
