// gs_xform.hip -- the splat transforms' entry points: gs_xform_compose and gs_transform_splats.  Part of the C ABI
// (include/gsplat/gs_abi.h "splat transforms"); the kernel is in k_xform.hip, the host mathematics in gs_xform_math.hip.
//
// The reference has no counterpart: it is a viewer.  An editor on it would fetch its 320-byte records, rotate positions,
// quaternions and SH coefficients on the CPU and upload them again (renderer.ts:130-137); here a transform is one streaming pass
// over the planes it names, in place.
//
// gs_transform_splats drains the context's ring first (gs_wait), runs on the context's stream and returns when done, as gs_state_*
// and the splat edits do.  It is not a frame and not an upload: nothing of the frame state, the shadows, the capacities, the
// statistics or a captured graph is touched (the graph's projection reads the planes when it is replayed).
#include <cmath>

#include "gs_runtime.h"
#include "gs_xform_math.h"

GS_EXPORT int32_t gs_xform_compose(const float rot_rxyz[4], const float translate[3], float scale, const float pivot[3], gs_xform* out) {
    char msg[256] = "";
    const int32_t rc = gs_xform_compose_host(rot_rxyz, translate, scale, pivot, out, msg, sizeof(msg));
    return rc == GS_OK ? GS_OK : fail(rc, "%s", msg);
}

static bool all_finite(const float* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) return false;
    return true;
}

GS_EXPORT int32_t gs_transform_splats(gs_ctx* c, uint32_t mask, uint32_t value, const gs_xform* x, uint64_t* matched) {
    const char* who = "gs_transform_splats";
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null ctx", who);
    if (!x) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null xform", who);
    if (x->struct_size != sizeof(gs_xform)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: struct_size %u != %zu", who, x->struct_size, sizeof(gs_xform));
    if (x->flags & ~(GS_XFORM_POSITION | GS_XFORM_ORIENT | GS_XFORM_SIZE)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", who, x->flags);
    if ((x->flags & GS_XFORM_POSITION) && !all_finite(x->m, 12)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: m has a non-finite entry", who);
    if ((x->flags & GS_XFORM_ORIENT) && !(all_finite(x->q, 4) && all_finite(x->sh1, 9) && all_finite(x->sh2, 25) && all_finite(x->sh3, 49)))
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: q or a band matrix has a non-finite entry", who);
    if ((x->flags & GS_XFORM_SIZE) && !std::isfinite(x->log_scale)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: log_scale is not finite", who);
    if (c->scene_mem && c->scene_mem != c->scene_own.get()) // (before the ring is drained: a refusal does nothing at all)
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: this context borrows its splats (gs_share_splats): transform the owner", who);
    int32_t rc = resident_begin(c, who, Plane::filtered, mask, value); // the splat edits' prologue (gs_export.hip)
    if (rc != GS_OK) return rc;
    const bool all = !(mask | value); // every splat: no selection runs, the kernel is dense over 0..N
    uint64_t total = c->n;
    if (!all) {
        rc = edit_select(c, mask, value, x->flags != 0u, &total);
        if (rc != GS_OK) return rc;
    }
    gs_launch_xform(c->scene, c->n, all ? nullptr : c->ex.ids.get(), (uint32_t)total, *x, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (matched) *matched = total;
    return GS_OK;
}
