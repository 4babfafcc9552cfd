// gs_grade.hip -- the colour grades' entry points: gs_grade_compose and gs_grade_splats.  Part of the C ABI
// (include/gsplat/gs_abi.h "colour grades"); the kernel is in k_grade.hip, the host mathematics in gs_grade_math.hip.
//
// The reference has no counterpart: it is a viewer.  An editor on it would fetch its 320-byte records, edit 48 SH floats per splat
// on the CPU and upload them again (renderer.ts:130-137); here a grade is one streaming pass over the SH records (and the opacity
// logit) of the splats it names, in place.
//
// gs_grade_splats follows gs_transform_splats (gs_xform.hip) rule for rule: it drains the context's ring first, runs on the
// context's stream and returns when done.  It is not a frame and not an upload: nothing of the frame state, the shadows, the
// capacities, the statistics, a captured graph or the coverage / neighbour / cluster planes is touched.  No resident plane is
// derived from the SH or the opacity at upload (gs_repack_kernel derives smax alone, from the log-scales), so nothing is recomputed.
#include "gs_grade_math.h"
#include "gs_runtime.h"

GS_EXPORT int32_t gs_grade_compose(const float gain[3], const float offset[3], float saturation, float black, float white, float opacity_gain,
                                   gs_grade* out) {
    char msg[256] = "";
    const int32_t rc = gs_grade_compose_host(gain, offset, saturation, black, white, opacity_gain, out, msg, sizeof(msg));
    return rc == GS_OK ? GS_OK : fail(rc, "%s", msg);
}

GS_EXPORT int32_t gs_grade_splats(gs_ctx* c, uint32_t mask, uint32_t value, const gs_grade* g, uint64_t* matched) {
    const char* who = "gs_grade_splats";
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null ctx", who);
    char msg[256] = ""; // (a null grade included)
    if (gs_grade_validate_host(g, msg, sizeof(msg)) != GS_OK) return fail(GS_ERR_INVALID_ARGUMENT, "%s", msg);
    if (c->scene_mem && c->scene_mem != c->scene_own.get()) // (before the ring is drained: a refusal does nothing at all)
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: this context borrows its splats (gs_share_splats): grade the owner", who);
    int32_t rc = resident_begin(c, who, Plane::filtered, mask, value); // the splat edits' prologue (gs_export.hip)
    if (rc != GS_OK) return rc;
    const bool all = !(mask | value); // every splat: no selection runs, the kernel is dense over 0..N
    uint64_t total = c->n;
    if (!all) {
        rc = edit_select(c, mask, value, g->flags != 0u, &total);
        if (rc != GS_OK) return rc;
    }
    gs_launch_grade(c->scene, c->n, all ? nullptr : c->ex.ids.get(), (uint32_t)total, *g, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (matched) *matched = total;
    return GS_OK;
}
