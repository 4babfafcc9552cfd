// gs_moments.hip -- the moments' entry points: the exact sums and sums of products of up to three attributes over the resident splats
// that pass a state filter, and the same numbers from host planes.  Part of the C ABI (include/gsplat/gs_abi.h "moments"); the
// kernel is in k_moments.hip, the arithmetic -- the split that both run and the finish that only the host runs -- in gs_exact_sum.h.
//
// The reference has no counterpart: it is a viewer.  An editor on it would sum the 320-byte records its host kept
// (renderer.ts:130-137) in whatever order and precision its language offers; here the answer is 160 bytes that any host can restate
// bit for bit, after one streaming pass over 4 bytes per attribute and splat.
//
// gs_attr_moments drains the context's ring first (gs_wait), runs on the context's stream and returns when done, as the splat
// attributes do.  It launches nothing in a frame: a context that never calls it launches exactly what it did before.
#include <cmath>

#include "gs_runtime.h"
#include "gs_exact_sum.h"

static_assert(sizeof(gs_exact) == 16 && sizeof(struct gs_attr_moments) == 160, "gs_exact / gs_attr_moments layout");
static_assert(GS_MOMENTS_MAX_ATTRS == 3u, "the kernel is instantiated for 1 .. 3 planes");
static_assert(GS_MOMENTS_SLOT_WORDS >= 9u * GS_EX_LIMBS + 2u, "a slot holds nine limb tables and the two counts");

// The record from the limb tables of `k` planes in the kernel's order (the k sums, then the products j <= l); entries of an
// attribute that was not given stay {+0.0, +0.0}.
static void moments_finish(const int64_t* tables, uint32_t k, uint64_t matched, uint64_t counted, struct gs_attr_moments* out) {
    memset(out, 0, sizeof(*out));
    out->matched = matched;
    out->counted = counted;
    uint32_t t = 0;
    for (uint32_t j = 0; j < k; ++j, ++t) ex_finish(tables + (size_t)t * GS_EX_LIMBS, &out->sum[j].hi, &out->sum[j].lo);
    static const int kProd[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}}; // 00, 01, 02, 11, 12, 22
    for (uint32_t j = 0; j < k; ++j)
        for (uint32_t l = j; l < k; ++l, ++t) {
            gs_exact* e = &out->prod[kProd[j][l]];
            ex_finish(tables + (size_t)t * GS_EX_LIMBS, &e->hi, &e->lo);
        }
}

GS_EXPORT int32_t gs_attr_moments(gs_ctx* c, const gs_attr* attrs, uint32_t n_attrs, uint32_t mask, uint32_t value, struct gs_attr_moments* out) {
    static const char* who = "gs_attr_moments";
    int32_t rc = resident_check(c, who, Plane::filtered, mask, value);
    if (rc != GS_OK) return rc;
    if (n_attrs < 1u || n_attrs > GS_MOMENTS_MAX_ATTRS) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %u attributes are not 1 .. %u", who, n_attrs, GS_MOMENTS_MAX_ATTRS);
    if (!attrs) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null attributes", who);
    GsAttrDev dev[GS_MOMENTS_MAX_ATTRS];
    bool cover = false;
    for (uint32_t j = 0; j < n_attrs; ++j) {
        rc = attr_check(who, attrs + j, dev + j);
        if (rc != GS_OK) return rc;
        cover = cover || attr_needs_cover(attrs + j);
    }
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null moments", who);
    if (c->n >= 0x80000000u) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %llu splats, a limb holds fewer than 2^31 terms", who, (unsigned long long)c->n);
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    if (cover) {
        rc = cover_planes(c, c->stream);
        if (rc != GS_OK) return rc;
    }
    const uint8_t* state = (mask | value) ? c->scene.state : nullptr;
    constexpr size_t kWords = (size_t)GS_MOMENTS_SLOTS * GS_MOMENTS_SLOT_WORDS;
    unsigned long long h[kWords] = {};
    if (c->n) {
        // the planes: a position plane is read in place, any other kind (LOG_SCALE_MAX too: its plane has the NaN exception) is
        // written densely first -- 4 B out and 4 B in per splat, no trips
        const float* plane[GS_MOMENTS_MAX_ATTRS] = {nullptr, nullptr, nullptr};
        for (uint32_t j = 0; j < n_attrs; ++j) {
            const uint32_t kind = attrs[j].kind;
            if (kind == GS_ATTR_POS_X) plane[j] = c->scene.px;
            else if (kind == GS_ATTR_POS_Y) plane[j] = c->scene.py;
            else if (kind == GS_ATTR_POS_Z) plane[j] = c->scene.pz;
            else {
                rc = c->mo.vals[j].reserve(((uint64_t)c->n + 3u) & ~3ull);
                if (rc != GS_OK) return rc;
                gs_launch_attr_values(kind, c->scene, c->cov, c->n, dev[j], nullptr, 0u, c->n, c->mo.vals[j], c->stream);
                HIP_TRY(hipGetLastError());
                plane[j] = c->mo.vals[j];
            }
        }
        if (!c->mo.slots) HIP_TRY(hipMalloc(c->mo.slots.out(), sizeof(h)));
        HIP_TRY(hipMemsetAsync(c->mo.slots, 0, sizeof(h), c->stream));
        gs_launch_moments(n_attrs, state, plane[0], plane[1], plane[2], c->n, mask, value, c->mo.slots, c->opt.grid_persist, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, c->mo.slots, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    // the copies add up in wrapping unsigned arithmetic; the totals are within i64 (gs_exact_sum.h)
    const uint32_t q = n_attrs + n_attrs * (n_attrs + 1u) / 2u, words = q * GS_EX_LIMBS + 2u;
    int64_t total[GS_MOMENTS_SLOT_WORDS] = {};
    for (uint32_t s = 0; s < GS_MOMENTS_SLOTS; ++s)
        for (uint32_t i = 0; i < words; ++i) total[i] = (int64_t)((uint64_t)total[i] + (uint64_t)h[(size_t)s * GS_MOMENTS_SLOT_WORDS + i]);
    moments_finish(total, n_attrs, (uint64_t)total[words - 2u], (uint64_t)total[words - 1u], out);
    return GS_OK;
}

GS_EXPORT int32_t gs_moments_host(const float* const* planes, uint32_t n_planes, uint64_t n, const uint8_t* state, uint32_t mask, uint32_t value,
                                  struct gs_attr_moments* out) {
    static const char* who = "gs_moments_host";
    if (n_planes < 1u || n_planes > GS_MOMENTS_MAX_ATTRS) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %u planes are not 1 .. %u", who, n_planes, GS_MOMENTS_MAX_ATTRS);
    if (!planes) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null planes", who);
    for (uint32_t j = 0; j < n_planes; ++j)
        if (!planes[j] && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null plane %u", who, j);
    if (mask > 0xFFu || value > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "%s: filter (0x%x, 0x%x) does not fit the state byte", who, mask, value);
    if ((mask | value) && !state && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null state with the filter (0x%x, 0x%x)", who, mask, value);
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null moments", who);
    if (n >= 0x80000000ull) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %llu splats, a limb holds fewer than 2^31 terms", who, (unsigned long long)n);
    int64_t tables[9 * GS_EX_LIMBS] = {};
    uint64_t matched = 0, counted = 0;
    const bool filter = (mask | value) != 0u;
    for (uint64_t i = 0; i < n; ++i) {
        if (filter && (state[i] & mask) != value) continue;
        ++matched;
        bool fin = true;
        for (uint32_t j = 0; j < n_planes; ++j) fin = fin && ex_finite(ex_bits(planes[j][i]));
        if (!fin) continue;
        ++counted;
        uint32_t t = 0;
        for (uint32_t j = 0; j < n_planes; ++j, ++t) ex_add_value(tables + (size_t)t * GS_EX_LIMBS, planes[j][i]);
        for (uint32_t j = 0; j < n_planes; ++j)
            for (uint32_t l = j; l < n_planes; ++l, ++t) ex_add_product(tables + (size_t)t * GS_EX_LIMBS, planes[j][i], planes[l][i]);
    }
    moments_finish(tables, n_planes, matched, counted, out);
    return GS_OK;
}
