// gs_coverage.hip -- the coverage planes' entry points: accumulate the last frame's per-splat contribution, reset, read, and select
// by what is seen.  Part of the C ABI (include/gsplat/gs_abi.h "coverage"); the kernels are in k_coverage.hip.
//
// The reference has no counterpart: it is a viewer.  A host that wanted to know which splats a view shows would re-implement the
// blend; here the lists and records of the last frame are still resident and one blend-shaped pass keeps a record per splat.
//
// gs_coverage_accumulate follows gs_pick: it describes the last frame enqueued, waits for it if it is pending, runs on its ring
// member's stream and returns when done.  The other three drain the ring (gs_wait) and run on the context's stream, as the state
// calls do.  None of them is a frame: nothing of the frame state, the statistics or a captured graph is touched.
#include "gs_runtime.h"
#include "gs_tight.h"

static_assert(sizeof(gs_coverage_rec) == 16 && offsetof(gs_coverage_rec, hits) == 8 && offsetof(gs_coverage_rec, max_weight) == 12, "gs_coverage_rec layout");

// The planes of the root context: allocated and zeroed (on `st`) by the first call that needs them.
static int32_t planes_ensure(gs_ctx* root, hipStream_t st) {
    if (root->cov) return GS_OK;
    const size_t bytes = std::max<size_t>((size_t)root->n * sizeof(gs_coverage_rec), 256);
    HIP_TRY(hipMalloc(root->cov.out(), bytes));
    HIP_TRY(hipMemsetAsync(root->cov, 0, bytes, st));
    return GS_OK;
}
// What reset, read and gs_state_coverage share: the checks, the drain of the ring and the planes.
static int32_t cover_begin(gs_ctx* c, const char* who) {
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null ctx", who);
    if (!c->scene_mem) return fail(GS_ERR_NO_SCENE, "%s: no splats uploaded", who);
    const int32_t rc = gs_wait(c);
    if (rc != GS_OK) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    return planes_ensure(c, c->stream);
}

GS_EXPORT int32_t gs_coverage_accumulate(gs_ctx* root, const gs_cover_region* rg, uint64_t* pixels) {
    if (!root) return fail(GS_ERR_INVALID_ARGUMENT, "gs_coverage_accumulate: null ctx");
    if (!root->scene_mem) return fail(GS_ERR_NO_SCENE, "gs_coverage_accumulate: no splats uploaded");
    const uint32_t W = root->frame.width, H = root->frame.height;
    GsCoverDev r{0u, 0u, W, H, nullptr};
    if (rg) {
        if (rg->struct_size != sizeof(gs_cover_region))
            return fail(GS_ERR_INVALID_ARGUMENT, "gs_coverage_accumulate: struct_size %u != %zu", rg->struct_size, sizeof(gs_cover_region));
        if (rg->x1 > W || rg->y1 > H)
            return fail(GS_ERR_INVALID_ARGUMENT, "gs_coverage_accumulate: rect [%u, %u) x [%u, %u) reaches outside the %u x %u canvas", rg->x0, rg->x1, rg->y0,
                        rg->y1, W, H);
        if (rg->x0 >= rg->x1 || rg->y0 >= rg->y1)
            return fail(GS_ERR_INVALID_ARGUMENT, "gs_coverage_accumulate: empty rect [%u, %u) x [%u, %u)", rg->x0, rg->x1, rg->y0, rg->y1);
        r.x0 = rg->x0; r.y0 = rg->y0; r.x1 = rg->x1; r.y1 = rg->y1;
    }
    gs_ctx* c = last_of(root);
    if (!c->have_frame) return fail(GS_ERR_NO_FRAME, "gs_coverage_accumulate: no frame rendered");
    if (c->pending) { int32_t rc = wait_one(c); if (rc != GS_OK) return rc; } // (an overflowed frame has been re-rendered from full lists)
    HIP_TRY(hipSetDevice(c->cfg.device));
    int32_t rc = planes_ensure(root, c->stream);
    if (rc != GS_OK) return rc;
    // P in this slab: the rect cut to the slab's pixel columns
    const uint32_t sx0 = c->frame.px0, sx1 = std::min(W, c->frame.px0 + c->frame.slab_w);
    const uint32_t x0 = std::max(r.x0, sx0), x1 = std::min(r.x1, sx1);
    uint64_t count = 0;
    if (x0 < x1) {
        if (rg && rg->mask) {
            for (uint32_t y = r.y0; y < r.y1; ++y) {
                const uint8_t* row = rg->mask + (uint64_t)y * W;
                for (uint32_t x = x0; x < x1; ++x) count += row[x] != 0;
            }
            const uint64_t mb = (uint64_t)W * H; // the state calls' SCREEN_MASK staging (gs_state.hip)
            if (mb > root->st.mask_cap) {
                root->st.mask_cap = 0;
                HIP_TRY(hipMalloc(root->st.mask.out(), (size_t)mb));
                root->st.mask_cap = mb;
            }
            HIP_TRY(hipMemcpyAsync(root->st.mask, rg->mask, (size_t)mb, hipMemcpyHostToDevice, c->stream));
            r.mask = root->st.mask;
        } else {
            count = (uint64_t)(x1 - x0) * (r.y1 - r.y0);
        }
    }
    if (count) { // the 8x8 blocks that hold a pixel of the cut rect
        const uint32_t bx0 = x0 / 8u, bx1 = (x1 + 7u) / 8u, by0 = r.y0 / 8u, by1 = (r.y1 + 7u) / 8u;
        gs_launch_coverage(c->gdata, c->notes.valsS, c->ranges, c->frame, c->notes.last_tight ? GS_ID_MASK : 0xFFFFFFFFu, bx0, by0, bx1 - bx0, by1 - by0, r,
                           root->cov, c->stream);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(c->stream)); // (also: the caller's mask has been copied, the planes' first zeroing is done)
    if (pixels) *pixels = count;
    return GS_OK;
}

GS_EXPORT int32_t gs_coverage_reset(gs_ctx* c) {
    int32_t rc = cover_begin(c, "gs_coverage_reset");
    if (rc != GS_OK) return rc;
    HIP_TRY(hipMemsetAsync(c->cov, 0, std::max<size_t>((size_t)c->n * sizeof(gs_coverage_rec), 256), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

GS_EXPORT int32_t gs_coverage_read(gs_ctx* c, gs_coverage_rec* dst, uint64_t cap, uint64_t* n) {
    int32_t rc = cover_begin(c, "gs_coverage_read");
    if (rc != GS_OK) return rc;
    if (!n) return fail(GS_ERR_INVALID_ARGUMENT, "gs_coverage_read: null n");
    *n = c->n;
    if (!dst) { HIP_TRY(hipStreamSynchronize(c->stream)); return GS_OK; }
    if (cap < c->n) return fail(GS_ERR_INVALID_ARGUMENT, "gs_coverage_read: %llu records needed, the buffer holds %llu", (unsigned long long)c->n, (unsigned long long)cap);
    if (c->n) HIP_TRY(hipMemcpyAsync(dst, c->cov, (size_t)c->n * sizeof(gs_coverage_rec), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

GS_EXPORT int32_t gs_state_coverage(gs_ctx* c, uint32_t min_hits, float min_weight, uint32_t covered, uint32_t where_mask, uint32_t where_value,
                                    uint32_t op, uint32_t bits, uint64_t* matched) {
    int32_t rc = state_begin(c, "gs_state_coverage");
    if (rc != GS_OK) return rc;
    rc = state_check_op("gs_state_coverage", op, bits);
    if (rc != GS_OK) return rc;
    if (!(min_weight >= 0.0f)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_coverage: min_weight %g is negative or not a number", (double)min_weight);
    if (where_mask > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_coverage: where_mask 0x%x does not fit the state byte", where_mask);
    rc = state_drain(c);
    if (rc != GS_OK) return rc;
    rc = planes_ensure(c, c->stream);
    if (rc != GS_OK) return rc;
    rc = state_counter_zero(c);
    if (rc != GS_OK) return rc;
    gs_launch_state_coverage(const_cast<uint8_t*>(c->scene.state), c->cov, c->n, min_hits, min_weight, covered, op, bits, where_mask, where_value,
                             c->st.counter, c->stream);
    HIP_TRY(hipGetLastError());
    unsigned long long m = 0;
    rc = state_counter_sum(c, &m);
    if (rc != GS_OK) return rc;
    if (matched) *matched = m;
    return GS_OK;
}
