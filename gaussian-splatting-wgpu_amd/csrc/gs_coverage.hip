// gs_coverage.hip -- the coverage planes' entry points: accumulate the last frame's per-splat contribution, reset and read (the
// selection by what is seen, gs_state_coverage, is with the state calls in gs_state.hip).  Part of the C ABI
// (include/gsplat/gs_abi.h "coverage"); the kernel is in k_coverage.hip.
//
// The reference has no counterpart: it is a viewer.  A host that wanted to know which splats a view shows would re-implement the
// blend; here the lists and records of the last frame are still resident and one blend-shaped pass keeps a record per splat.
//
// gs_coverage_accumulate follows gs_pick: it describes the last frame enqueued, waits for it if it is pending, runs on its ring
// member's stream and returns when done.  The other two drain the ring (gs_wait) and run on the context's stream, as the state
// calls do.  None of them is a frame: nothing of the frame state, the statistics or a captured graph is touched.
#include "gs_runtime.h"

static_assert(sizeof(gs_coverage_rec) == 16 && offsetof(gs_coverage_rec, hits) == 8 && offsetof(gs_coverage_rec, max_weight) == 12, "gs_coverage_rec layout");

int32_t cover_planes(gs_ctx* root, hipStream_t st) {
    if (root->cov) return GS_OK;
    const size_t bytes = std::max<size_t>((size_t)root->n * sizeof(gs_coverage_rec), 256);
    HIP_TRY(hipMalloc(root->cov.out(), bytes));
    HIP_TRY(hipMemsetAsync(root->cov, 0, bytes, st));
    return GS_OK;
}
// What reset and read share: the checks, the drain of the ring and the planes.
static int32_t cover_begin(gs_ctx* c, const char* who) {
    const int32_t rc = resident_begin(c, who, Plane::none);
    return rc != GS_OK ? rc : cover_planes(c, c->stream);
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
    gs_ctx* c = nullptr;
    int32_t rc = last_frame(root, "gs_coverage_accumulate", &c);
    if (rc != GS_OK) return rc;
    rc = cover_planes(root, c->stream);
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
            rc = stage_mask(root, rg->mask, c->stream, &r.mask);
            if (rc != GS_OK) return rc;
        } else {
            count = (uint64_t)(x1 - x0) * (r.y1 - r.y0);
        }
    }
    if (count) { // the 8x8 blocks that hold a pixel of the cut rect
        const uint32_t bx0 = x0 / 8u, bx1 = (x1 + 7u) / 8u, by0 = r.y0 / 8u, by1 = (r.y1 + 7u) / 8u;
        gs_launch_coverage(frame_lists(c), bx0, by0, bx1 - bx0, by1 - by0, r, root->cov, c->stream);
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
