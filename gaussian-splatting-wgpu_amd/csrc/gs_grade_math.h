// gs_grade_math.h -- the host mathematics of gs_grade_compose (gs_grade_math.hip): no HIP, no context, no GPU.  The entry point
// of the C ABI (gs_grade.hip) forwards to it; tools/grade_check compiles the same translation unit alone, as plain C++.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/gsplat/gs_abi.h"

// Fills *out (gs_abi.h "colour grades").  gain, offset: three floats or null (1,1,1 / 0,0,0).  Returns GS_OK, or
// GS_ERR_INVALID_ARGUMENT with the reason in err (errlen bytes); a refusal writes nothing to *out.
int32_t gs_grade_compose_host(const float* gain, const float* offset, float saturation, float black, float white, float opacity_gain,
                              gs_grade* out, char* err, size_t errlen);
// gs_grade_splats' refusals of a gs_grade (null, struct_size, unknown flag bits, reserved, a non-finite member of a FLAGGED part; a
// member of a part that is not flagged is not looked at), in that call's name.
int32_t gs_grade_validate_host(const gs_grade* g, char* err, size_t errlen);
