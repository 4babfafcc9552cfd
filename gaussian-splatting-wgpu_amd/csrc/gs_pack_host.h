// gs_pack_host.h -- the host side of the packed scenes (gs_pack_host.hip): the codec over host arrays and the file's header, writer
// and loader.  No HIP, no context, no GPU: the entry points of the C ABI (gs_pack.hip) forward to it, and tools/pack_check compiles
// the same translation unit alone, as plain C++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/gsplat/gs_abi.h"

inline int gs_pack_rest(int sh_degree) { return (sh_degree + 1) * (sh_degree + 1) - 1; } // K: higher coefficients per channel
inline uint64_t gs_pack_chunks(uint64_t n) { return (n + 255u) / 256u; }

// The 256 logits of gs_pack_logit_table, built once (in double, rounded to f32 once each).
const float* gs_pack_logits();

// records: n x 80 floats.  chunks: ceil(n / 256) x 18 floats; vertices: n x 4 words; sh: n x 3 K bytes (not touched at degree 0);
// *bad (may be null): the carried floats that fin replaced plus the NaN logits.
void gs_pack_encode_host(const float* records, uint64_t n, int sh_degree, float* chunks, uint32_t* vertices, uint8_t* sh, uint64_t* bad);
// the inverse, to 320-byte records: padding floats and the coefficients above sh_degree are +0
void gs_pack_decode_host(const float* chunks, const uint32_t* vertices, const uint8_t* sh, uint64_t n, int sh_degree, const float* table, float* records);

// What the header of a packed file says, checked against the file's size.
struct GsPackLayout {
    uint64_t n = 0, chunks = 0;
    int degree = 0;
    uint64_t chunk_off = 0, vertex_off = 0, sh_off = 0, file_bytes = 0;
};
std::string gs_pack_header(uint64_t n, int sh_degree);
uint64_t gs_pack_file_bytes(uint64_t n, int sh_degree); // header included
// head: the first `len` bytes of the file; file_size: all of it.  Returns GS_OK, or GS_ERR_INVALID_ARGUMENT with the defect in err
// ("<who>: <path>: <defect>"); a refusal leaves *L as it was.
int32_t gs_pack_parse_header(const char* who, const char* path, const unsigned char* head, size_t len, uint64_t file_size, GsPackLayout* L, char* err,
                             size_t errlen);
int32_t gs_pack_save_host(const char* path, const void* records, uint64_t n, int32_t sh_degree, char* err, size_t errlen);
// *records: malloc'ed, n x 320 bytes (at least one byte); the outputs are written on success only
int32_t gs_pack_load_host(const char* path, void** records, uint64_t* n, int32_t* sh_degree, char* err, size_t errlen);
