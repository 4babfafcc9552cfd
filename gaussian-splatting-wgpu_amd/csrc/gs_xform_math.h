// gs_xform_math.h -- the host mathematics of gs_xform_compose (gs_xform_math.hip): no HIP, no context, no GPU.  The entry point
// of the C ABI (gs_xform.hip) forwards to it; tools/xform_check compiles the same translation unit alone, as plain C++.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/gsplat/gs_abi.h"

// Fills *out (gs_abi.h "splat transforms").  Returns GS_OK, or GS_ERR_INVALID_ARGUMENT with the reason in err (errlen bytes).
int32_t gs_xform_compose_host(const float* rot_rxyz, const float* translate, float scale, const float* pivot, gs_xform* out, char* err,
                              size_t errlen);
// compute_color_from_sh's band-l terms (process_gaussians.wgsl:240-280, constants and signs included) at the unit direction d, in
// double: out[0 .. 2l]
void gs_xform_sh_basis(int l, const double d[3], double* out);
