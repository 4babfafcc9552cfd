// gs_grade_math.hip -- gs_grade_compose's mathematics (gs_abi.h "colour grades"): the 3x3 colour matrix, the band-0 offset and the
// logit step of a grade, in double, every output rounded to f32 once.  Plain C++: no HIP call, no context.
//
// The reference has no counterpart (a viewer never edits its coefficients); what fixes the offset is its own compute_color_from_sh
// (process_gaussians.wgsl:221-280): C = SH_C0 sh_0 + sum_k b_k(d) sh_k + 0.5 before the clamp.  With sh_k' = A sh_k for every k the
// sum becomes A (C - h), h = (1/2, 1/2, 1/2); for C' = A C + o the constant (A h + o - h) is still missing, and band 0 is the one
// coefficient whose basis function is a constant: sh_0' = A sh_0 + (A h + o - h) / SH_C0.
// The expressions are written exactly as gs_abi.h states them: a test restates them in double and compares the roundings bit for bit.
#include "gs_grade_math.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

static const double kShC0 = 0.28209479177387814;
static const double kLuma[3] = {0.2126, 0.7152, 0.0722}; // Rec. 709

static int32_t refuse(char* err, size_t errlen, const char* fmt, ...) {
    if (err && errlen) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, errlen, fmt, ap);
        va_end(ap);
    }
    return GS_ERR_INVALID_ARGUMENT;
}

int32_t gs_grade_compose_host(const float* gain, const float* offset, float saturation, float black, float white, float opacity_gain,
                              gs_grade* out, char* err, size_t errlen) {
    if (!out) return refuse(err, errlen, "gs_grade_compose: null out");
    double g[3] = {1.0, 1.0, 1.0}, off[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < 3; ++c) {
        if (gain && !std::isfinite(gain[c])) return refuse(err, errlen, "gs_grade_compose: gain[%d] is not finite", c);
        if (offset && !std::isfinite(offset[c])) return refuse(err, errlen, "gs_grade_compose: offset[%d] is not finite", c);
        if (gain) g[c] = gain[c];
        if (offset) off[c] = offset[c];
    }
    if (!std::isfinite(saturation)) return refuse(err, errlen, "gs_grade_compose: saturation is not finite");
    if (!std::isfinite(black)) return refuse(err, errlen, "gs_grade_compose: black is not finite");
    if (!std::isfinite(white)) return refuse(err, errlen, "gs_grade_compose: white is not finite");
    if (white == black) return refuse(err, errlen, "gs_grade_compose: white == black (%g)", (double)white);
    if (!std::isfinite(opacity_gain) || !(opacity_gain > 0.0f))
        return refuse(err, errlen, "gs_grade_compose: opacity_gain %g is not a finite positive number", (double)opacity_gain);
    const double s = 1.0 / ((double)white - (double)black);
    if (!std::isfinite(s)) return refuse(err, errlen, "gs_grade_compose: 1 / (white - black) is not finite");
    const double sat = saturation, blk = black;
    gs_grade o{};
    o.struct_size = (uint32_t)sizeof(gs_grade);
    bool identity = true;
    for (int c = 0; c < 3; ++c) {
        double A[3];
        for (int j = 0; j < 3; ++j) {
            const double delta = c == j ? 1.0 : 0.0;
            A[j] = (g[c] * (sat * delta + (1.0 - sat) * kLuma[j])) * s;
            o.a[3 * c + j] = (float)A[j];
            if (!std::isfinite(o.a[3 * c + j])) return refuse(err, errlen, "gs_grade_compose: gain, saturation, black, white: a[%d] overflows f32", 3 * c + j);
            identity = identity && o.a[3 * c + j] == (c == j ? 1.0f : 0.0f);
        }
        const double oc = off[c] - (g[c] * blk) * s;
        o.dc[c] = (float)(((((A[0] + A[1]) + A[2]) * 0.5 + oc) - 0.5) / kShC0);
        if (!std::isfinite(o.dc[c])) return refuse(err, errlen, "gs_grade_compose: gain, offset, black, white: dc[%d] overflows f32", c);
    }
    o.opacity_logit = (float)std::log((double)opacity_gain);
    if (!std::isfinite(o.opacity_logit)) return refuse(err, errlen, "gs_grade_compose: opacity_gain: the logit step is not finite");
    if (!identity) o.flags |= GS_GRADE_MATRIX;
    if (o.dc[0] != 0.0f || o.dc[1] != 0.0f || o.dc[2] != 0.0f) o.flags |= GS_GRADE_OFFSET;
    if (opacity_gain != 1.0f) o.flags |= GS_GRADE_OPACITY;
    *out = o;
    return GS_OK;
}

static bool all_finite(const float* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) return false;
    return true;
}

int32_t gs_grade_validate_host(const gs_grade* g, char* err, size_t errlen) {
    const char* who = "gs_grade_splats";
    if (!g) return refuse(err, errlen, "%s: null grade", who);
    if (g->struct_size != sizeof(gs_grade)) return refuse(err, errlen, "%s: struct_size %u != %zu", who, g->struct_size, sizeof(gs_grade));
    if (g->flags & ~(GS_GRADE_MATRIX | GS_GRADE_OFFSET | GS_GRADE_OPACITY)) return refuse(err, errlen, "%s: unknown flag bits 0x%x", who, g->flags);
    if (!(g->reserved == 0.0f)) return refuse(err, errlen, "%s: reserved is not 0", who);
    if ((g->flags & GS_GRADE_MATRIX) && !all_finite(g->a, 9)) return refuse(err, errlen, "%s: a has a non-finite entry", who);
    if ((g->flags & GS_GRADE_OFFSET) && !all_finite(g->dc, 3)) return refuse(err, errlen, "%s: dc has a non-finite entry", who);
    if ((g->flags & GS_GRADE_OPACITY) && !std::isfinite(g->opacity_logit)) return refuse(err, errlen, "%s: opacity_logit is not finite", who);
    return GS_OK;
}
