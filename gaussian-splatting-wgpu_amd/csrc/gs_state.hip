// gs_state.hip -- the state plane's entry points: region, id, coverage and attribute selections, counting, restore.  Part of the C ABI
// (include/gsplat/gs_abi.h "splat state"; gs_state_coverage under "coverage", gs_state_attr under "splat attributes", gs_state_neigh under "neighbourhoods", gs_state_knn under "nearest neighbours", gs_state_cluster and gs_state_cluster_linked under "clusters"); the kernels are in k_state.hip, the projection that
// honours the plane in k_preprocess.hip (STATE).  Also what every call on the resident splats does first (gs_runtime.h).
//
// The reference has no counterpart: it is a viewer.  An editor on it would edit its own 320-byte records and upload them again
// (renderer.ts:130-137); here a selection is one streaming pass over 13 bytes per splat.
//
// Every call drains the context's ring first (gs_wait), runs on the context's stream and returns when done: a frame never sees
// a half-applied call, and the host never has to order a state call against its own frames.  None of them is a frame: nothing
// of the frame state, the statistics or a captured graph is touched (the graph's projection reads the plane when it is replayed).
#include "gs_runtime.h"

int32_t resident_check(gs_ctx* c, const char* who, Plane need, uint32_t mask, uint32_t value) {
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null ctx", who);
    if (need == Plane::filtered && (mask > 0xFFu || value > 0xFFu))
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: filter (0x%x, 0x%x) does not fit the state byte", who, mask, value);
    if ((need == Plane::always || (need == Plane::filtered && (mask | value))) && !has_state(c)) // (0, 0): what is resident needs no plane
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: the context was created without GS_FLAG_SPLAT_STATE", who);
    if (!c->scene_mem || (need == Plane::always && !c->scene.state)) return fail(GS_ERR_NO_SCENE, "%s: no splats uploaded", who);
    return GS_OK;
}
static constexpr size_t kCounterBytes = (size_t)GS_STATE_SLOTS * GS_STATE_SLOT_STRIDE * sizeof(unsigned long long);
int32_t resident_drain(gs_ctx* c, bool counter) {
    const int32_t rc = gs_wait(c);
    if (rc != GS_OK) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (counter && !c->st.counter) HIP_TRY(hipMalloc(c->st.counter.out(), kCounterBytes));
    return GS_OK;
}
int32_t stage_mask(gs_ctx* root, const uint8_t* mask, hipStream_t st, const uint8_t** dev) {
    const uint64_t bytes = (uint64_t)root->frame.width * root->frame.height; // the CANVAS, also on a slab context
    const int32_t rc = root->st.mask.reserve(bytes);
    if (rc != GS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(root->st.mask, mask, (size_t)bytes, hipMemcpyHostToDevice, st));
    *dev = root->st.mask;
    return GS_OK;
}
// A launch that counts: launch(slots) enqueues a kernel that adds its `matched` into the GS_STATE_SLOTS partial sums (gs_kernels.h).
// They are zeroed before it and added up after it; returns when the stream is done.  matched may be null.
template <class Launch>
static int32_t state_counted(gs_ctx* c, Launch launch, uint64_t* matched) {
    HIP_TRY(hipMemsetAsync(c->st.counter, 0, kCounterBytes, c->stream));
    launch(c->st.counter.get());
    HIP_TRY(hipGetLastError());
    unsigned long long h[GS_STATE_SLOTS * GS_STATE_SLOT_STRIDE];
    HIP_TRY(hipMemcpyAsync(h, c->st.counter, kCounterBytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint64_t total = 0;
    for (int k = 0; k < GS_STATE_SLOTS; ++k) total += h[k * GS_STATE_SLOT_STRIDE];
    if (matched) *matched = total;
    return GS_OK;
}
static int32_t state_check_op(const char* who, uint32_t op, uint32_t bits) {
    if (op < GS_STATE_SET || op > GS_STATE_ASSIGN) return fail(GS_ERR_INVALID_ARGUMENT, "%s: unknown op %u (GS_STATE_SET .. GS_STATE_ASSIGN)", who, op);
    if (bits > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "%s: bits 0x%x do not fit the state byte", who, bits);
    return GS_OK;
}
static uint8_t* plane(gs_ctx* c) { return const_cast<uint8_t*>(c->scene.state); }

GS_EXPORT int32_t gs_state_region(gs_ctx* c, const gs_region* rg, uint32_t op, uint32_t bits, uint64_t* matched) {
    int32_t rc = resident_check(c, "gs_state_region", Plane::always);
    if (rc != GS_OK) return rc;
    if (!rg) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_region: null region");
    if (rg->struct_size != sizeof(gs_region)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_region: struct_size %u != %zu", rg->struct_size, sizeof(gs_region));
    if (rg->kind > GS_REGION_SCREEN_MASK) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_region: unknown region kind %u", rg->kind);
    rc = state_check_op("gs_state_region", op, bits);
    if (rc != GS_OK) return rc;
    if (rg->where_mask > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_region: where_mask 0x%x does not fit the state byte", rg->where_mask);
    const bool screen = rg->kind == GS_REGION_SCREEN_RECT || rg->kind == GS_REGION_SCREEN_MASK;
    if (screen && !rg->uniforms160) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_region: a screen region needs uniforms160 (the camera)");
    if (rg->kind == GS_REGION_SCREEN_MASK && !rg->mask) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_region: GS_REGION_SCREEN_MASK needs a mask");
    rc = resident_drain(c, true);
    if (rc != GS_OK) return rc;

    GsRegionDev r{};
    for (int k = 0; k < 3; ++k) { r.a[k] = rg->a[k]; r.b[k] = rg->b[k]; }
    r.x0 = (float)rg->x0; r.y0 = (float)rg->y0; r.x1 = (float)rg->x1; r.y1 = (float)rg->y1;
    r.wi = c->frame.width; r.hi = c->frame.height; // the CANVAS, also on a slab context
    r.W = (float)r.wi; r.H = (float)r.hi;
    if (screen) {
        GsUniforms u;
        memcpy(&u, rg->uniforms160, sizeof(u));
        memcpy(r.proj, u.proj, sizeof(r.proj));
        for (int k = 0; k < 4; ++k) r.viewz[k] = u.view[4 * k + 2];
    }
    if (rg->kind == GS_REGION_SCREEN_MASK) {
        rc = stage_mask(c, rg->mask, c->stream, &r.mask);
        if (rc != GS_OK) return rc;
    }
    return state_counted(c, [&](unsigned long long* slots) {
        gs_launch_state_region(rg->kind, plane(c), c->scene, c->n, r, op, bits, rg->where_mask, rg->where_value, slots, c->stream);
    }, matched);
}

GS_EXPORT int32_t gs_state_ids(gs_ctx* c, const uint32_t* ids, uint64_t n, uint32_t op, uint32_t bits) {
    int32_t rc = resident_check(c, "gs_state_ids", Plane::always);
    if (rc != GS_OK) return rc;
    if (!ids && n) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_ids: null ids");
    rc = state_check_op("gs_state_ids", op, bits);
    if (rc != GS_OK) return rc;
    for (uint64_t i = 0; i < n; ++i) // before anything is changed
        if (ids[i] >= c->n)
            return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_ids: ids[%llu] = %u is not a splat (N = %u)", (unsigned long long)i, ids[i], c->n);
    rc = resident_drain(c, true);
    if (rc != GS_OK) return rc;
    if (!n) return GS_OK;
    rc = c->st.ids.reserve(n);
    if (rc != GS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(c->st.ids, ids, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    gs_launch_state_ids(plane(c), c->st.ids, n, op, bits, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream)); // (also: the caller's ids have been copied)
    return GS_OK;
}

GS_EXPORT int32_t gs_state_count(gs_ctx* c, uint32_t mask, uint32_t value, uint64_t* count) {
    int32_t rc = resident_check(c, "gs_state_count", Plane::always);
    if (rc != GS_OK) return rc;
    if (!count) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_count: null count");
    rc = resident_drain(c, true);
    if (rc != GS_OK) return rc;
    return state_counted(c, [&](unsigned long long* slots) { gs_launch_state_count(c->scene.state, c->n, mask, value, slots, c->stream); }, count);
}

// Select by what is seen: the pass over the coverage planes (gs_coverage.hip), which the first call that needs them allocates.
GS_EXPORT int32_t gs_state_coverage(gs_ctx* c, uint32_t min_hits, float min_weight, uint32_t covered, uint32_t where_mask, uint32_t where_value,
                                    uint32_t op, uint32_t bits, uint64_t* matched) {
    int32_t rc = resident_check(c, "gs_state_coverage", Plane::always);
    if (rc != GS_OK) return rc;
    rc = state_check_op("gs_state_coverage", op, bits);
    if (rc != GS_OK) return rc;
    if (!(min_weight >= 0.0f)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_coverage: min_weight %g is negative or not a number", (double)min_weight);
    if (where_mask > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_coverage: where_mask 0x%x does not fit the state byte", where_mask);
    rc = resident_drain(c, true);
    if (rc != GS_OK) return rc;
    rc = cover_planes(c, c->stream);
    if (rc != GS_OK) return rc;
    return state_counted(c, [&](unsigned long long* slots) {
        gs_launch_state_coverage(plane(c), c->cov, c->n, min_hits, min_weight, covered, op, bits, where_mask, where_value, slots, c->stream);
    }, matched);
}

// Select by value: the pass around a splat attribute (gs_attr.hip, k_attr.hip).
GS_EXPORT int32_t gs_state_attr(gs_ctx* c, const gs_attr* a, float lo, float hi, uint32_t inside, uint32_t where_mask, uint32_t where_value, uint32_t op,
                                uint32_t bits, uint64_t* matched) {
    int32_t rc = resident_check(c, "gs_state_attr", Plane::always);
    if (rc != GS_OK) return rc;
    GsAttrDev dev;
    rc = attr_check("gs_state_attr", a, &dev);
    if (rc != GS_OK) return rc;
    rc = state_check_op("gs_state_attr", op, bits);
    if (rc != GS_OK) return rc;
    if (lo != lo || hi != hi) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_attr: range [%g, %g] has a bound that is not a number", (double)lo, (double)hi);
    if (where_mask > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_attr: where_mask 0x%x does not fit the state byte", where_mask);
    rc = resident_drain(c, true);
    if (rc != GS_OK) return rc;
    if (attr_needs_cover(a)) {
        rc = cover_planes(c, c->stream);
        if (rc != GS_OK) return rc;
    }
    return state_counted(c, [&](unsigned long long* slots) {
        gs_launch_attr_state(a->kind, plane(c), c->scene, c->cov, c->n, dev, lo, hi, inside, op, bits, where_mask, where_value, slots, c->stream);
    }, matched);
}

// The prologue of a selection by a resident plane (the five calls below), the refusals in their order: resident_check, before() --
// the call's own refusals that come ahead of the op's --, the op, after() -- those that follow it --, the where_mask; then the drain
// with the counter and planes(c, stream), which the first call that needs them allocates.
static int32_t no_refusal() { return GS_OK; }
static int32_t state_check_range(const char* who, float lo, float hi) {
    if (lo != lo || hi != hi) return fail(GS_ERR_INVALID_ARGUMENT, "%s: range [%g, %g] has a bound that is not a number", who, (double)lo, (double)hi);
    return GS_OK;
}
template <class Before = int32_t (*)(), class After = int32_t (*)()>
static int32_t plane_select_begin(gs_ctx* c, const char* who, uint32_t op, uint32_t bits, uint32_t where_mask, int32_t (*planes)(gs_ctx*, hipStream_t),
                                  Before before = no_refusal, After after = no_refusal) {
    int32_t rc;
    if ((rc = resident_check(c, who, Plane::always)) != GS_OK || (rc = before()) != GS_OK || (rc = state_check_op(who, op, bits)) != GS_OK ||
        (rc = after()) != GS_OK)
        return rc;
    if (where_mask > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "%s: where_mask 0x%x does not fit the state byte", who, where_mask);
    if ((rc = resident_drain(c, true)) != GS_OK) return rc;
    return planes(c, c->stream);
}

// Select by neighbour count: the pass over the count plane (gs_neigh.hip).
GS_EXPORT int32_t gs_state_neigh(gs_ctx* c, uint32_t min_count, uint32_t max_count, uint32_t inside, uint32_t where_mask, uint32_t where_value, uint32_t op,
                                 uint32_t bits, uint64_t* matched) {
    const int32_t rc = plane_select_begin(c, "gs_state_neigh", op, bits, where_mask, neigh_plane);
    if (rc != GS_OK) return rc;
    return state_counted(c, [&](unsigned long long* slots) {
        gs_launch_state_neigh(plane(c), c->ng.plane, c->n, min_count, max_count, inside, op, bits, where_mask, where_value, slots, c->stream);
    }, matched);
}

// Select by the k-th nearest distance: the pass over the dist2 plane (gs_knn.hip) read as words, with gs_state_attr's float range.
GS_EXPORT int32_t gs_state_knn(gs_ctx* c, float lo, float hi, uint32_t inside, uint32_t where_mask, uint32_t where_value, uint32_t op, uint32_t bits,
                               uint64_t* matched) {
    const int32_t rc = plane_select_begin(c, "gs_state_knn", op, bits, where_mask, knn_planes, no_refusal, [&] { return state_check_range("gs_state_knn", lo, hi); });
    if (rc != GS_OK) return rc;
    return state_counted(c, [&](unsigned long long* slots) {
        gs_launch_state_knn(plane(c), c->kn.dist2, c->n, lo, hi, inside, op, bits, where_mask, where_value, slots, c->stream);
    }, matched);
}

// Select by a surface feature: the pass over one of the two surface planes (gs_surface.hip) -- the eigenvalues for the four shape
// kinds, the normal and count for the others --, with gs_state_knn's float range on the feature (gs_surface_math.h: sf_feature).
GS_EXPORT int32_t gs_state_surface(gs_ctx* c, const gs_surface_range* r, uint32_t where_mask, uint32_t where_value, uint32_t op, uint32_t bits,
                                   uint64_t* matched) {
    const char* who = "gs_state_surface";
    const int32_t rc = plane_select_begin(
        c, who, op, bits, where_mask, surface_planes,
        [&]() -> int32_t {
            if (!r) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null range", who);
            if (r->struct_size != sizeof(gs_surface_range)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: struct_size %u != %zu", who, r->struct_size, sizeof(gs_surface_range));
            if (r->kind > GS_SURFACE_COUNT) return fail(GS_ERR_INVALID_ARGUMENT, "%s: unknown kind %u (0 .. %u)", who, r->kind, GS_SURFACE_COUNT);
            return GS_OK;
        },
        [&] { return state_check_range(who, r->lo, r->hi); });
    if (rc != GS_OK) return rc;
    const void* rec = r->kind < GS_SURFACE_FACING ? c->sf.eig.get() : c->sf.nrm.get();
    return state_counted(c, [&](unsigned long long* slots) {
        gs_launch_state_surface(plane(c), rec, c->n, r->kind, r->lo, r->hi, r->inside, r->axis, op, bits, where_mask, where_value, slots, c->stream);
    }, matched);
}

// Select by cluster size: gs_state_neigh's pass over the size plane (gs_cluster.hip).
GS_EXPORT int32_t gs_state_cluster(gs_ctx* c, uint32_t min_size, uint32_t max_size, uint32_t inside, uint32_t where_mask, uint32_t where_value, uint32_t op,
                                   uint32_t bits, uint64_t* matched) {
    const int32_t rc = plane_select_begin(c, "gs_state_cluster", op, bits, where_mask, cluster_planes);
    if (rc != GS_OK) return rc;
    return state_counted(c, [&](unsigned long long* slots) {
        gs_launch_state_neigh(plane(c), c->cl.size, c->n, min_size, max_size, inside, op, bits, where_mask, where_value, slots, c->stream);
    }, matched);
}

// Select by covers: gs_state_neigh's pass over the covers plane (gs_thin.hip).  Kept: [1, 2^32 - 1]; dropped: [0, 0] under the member filter.
GS_EXPORT int32_t gs_state_thin(gs_ctx* c, uint32_t min_covers, uint32_t max_covers, uint32_t inside, uint32_t where_mask, uint32_t where_value, uint32_t op,
                                uint32_t bits, uint64_t* matched) {
    const int32_t rc = plane_select_begin(c, "gs_state_thin", op, bits, where_mask, thin_planes);
    if (rc != GS_OK) return rc;
    return state_counted(c, [&](unsigned long long* slots) {
        gs_launch_state_neigh(plane(c), c->th.covers, c->n, min_covers, max_covers, inside, op, bits, where_mask, where_value, slots, c->stream);
    }, matched);
}

// Select the clusters that hold a seed: every seed sets the flag word of its label (n zeroed words of the neighbourhoods' scratch),
// then the state pass over the label plane reads the flag of every splat's label.
GS_EXPORT int32_t gs_state_cluster_linked(gs_ctx* c, uint32_t seed_mask, uint32_t seed_value, uint32_t where_mask, uint32_t where_value, uint32_t op,
                                          uint32_t bits, uint64_t* matched) {
    int32_t rc = plane_select_begin(c, "gs_state_cluster_linked", op, bits, where_mask, cluster_planes, no_refusal, [&]() -> int32_t {
        if (seed_mask > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_cluster_linked: seed_mask 0x%x does not fit the state byte", seed_mask);
        return GS_OK;
    });
    if (rc != GS_OK) return rc;
    if (!c->n) { if (matched) *matched = 0; return GS_OK; }
    rc = c->ng.keysA.reserve(c->n);
    if (rc != GS_OK) return rc;
    uint32_t* flag = c->ng.keysA;
    HIP_TRY(hipMemsetAsync(flag, 0, (size_t)c->n * 4, c->stream));
    gs_launch_cluster_seeds(c->scene.state, c->cl.label, c->n, seed_mask, seed_value, flag, c->stream);
    return state_counted(c, [&](unsigned long long* slots) {
        gs_launch_state_cluster_linked(plane(c), c->cl.label, c->n, flag, op, bits, where_mask, where_value, slots, c->stream);
    }, matched);
}

GS_EXPORT int32_t gs_state_write(gs_ctx* c, const uint8_t* src, uint64_t n) {
    int32_t rc = resident_check(c, "gs_state_write", Plane::always);
    if (rc != GS_OK) return rc;
    if (n != c->n) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_write: n = %llu, the plane holds %u splats (whole plane only)", (unsigned long long)n, c->n);
    if (!src && n) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_write: null source");
    rc = resident_drain(c, true);
    if (rc != GS_OK) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(plane(c), src, (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}
