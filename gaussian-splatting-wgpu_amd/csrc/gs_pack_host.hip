// gs_pack_host.hip -- the host side of the packed scenes (gs_abi.h "packed scenes"): the codec over host arrays (gs_pack_math.h, the
// one copy the kernels compile too), the file's header, its writer and its loader.  Plain C++: no HIP call, no context.
//
// The reference has no counterpart: its only container is the float .ply (ply.ts:49-228), 248 bytes per splat at degree 3.  The
// layout here is the chunked one that splat editors and web viewers exchange -- 16 bytes per splat against per-256-splat bounds, one
// byte per higher SH coefficient --, stated in gs_abi.h; the files carry a marker line and only files with it are read.
#include "gs_pack_host.h"

#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gs_pack_math.h"

static int32_t refuse(char* err, size_t errlen, int32_t code, const char* fmt, ...) {
    if (err && errlen) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, errlen, fmt, ap);
        va_end(ap);
    }
    return code;
}

const float* gs_pack_logits() {
    static const struct Table {
        float v[256];
        Table() {
            for (int a = 0; a < 256; ++a) {
                const double x = a == 0 ? 0.5 / 255.0 : a == 255 ? 254.5 / 255.0 : (double)a / 255.0;
                v[a] = (float)std::log(x / (1.0 - x));
            }
        }
    } t;
    return t.v;
}

// ---- the codec ----------------------------------------------------------------------------------------------------------------------
static PkEntry entry_of(const float* f) { return pk_entry(f[0], f[1], f[2], f[4], f[5], f[6], f[8], f[9], f[10], f[11], f[12], f[16], f[17], f[18]); }

void gs_pack_encode_host(const float* records, uint64_t n, int sh_degree, float* chunks, uint32_t* vertices, uint8_t* sh, uint64_t* bad_out) {
    const int K = gs_pack_rest(sh_degree);
    uint64_t bad = 0;
    PkEntry e[GS_PACK_CHUNK];
    for (uint64_t g0 = 0; g0 < n; g0 += GS_PACK_CHUNK) {
        const uint32_t m = (uint32_t)(n - g0 < GS_PACK_CHUNK ? n - g0 : GS_PACK_CHUNK);
        uint32_t lo[9], hi[9];
        for (int k = 0; k < 9; ++k) { lo[k] = 0xFFFFFFFFu; hi[k] = 0u; }
        for (uint32_t j = 0; j < m; ++j) {
            e[j] = entry_of(records + (g0 + j) * 80);
            bad += e[j].bad;
            const float v[9] = {e[j].px, e[j].py, e[j].pz, e[j].sx, e[j].sy, e[j].sz, e[j].cr, e[j].cg, e[j].cb};
            for (int k = 0; k < 9; ++k) {
                const uint32_t key = pk_okey(v[k]);
                if (key < lo[k]) lo[k] = key;
                if (key > hi[k]) hi[k] = key;
            }
        }
        float* b = chunks + (g0 / GS_PACK_CHUNK) * GS_PACK_CHUNK_FLOATS;
        for (int part = 0; part < 3; ++part)
            for (int k = 0; k < 3; ++k) {
                b[6 * part + k] = pk_okey_value(lo[3 * part + k]);
                b[6 * part + 3 + k] = pk_okey_value(hi[3 * part + k]);
            }
        for (uint32_t j = 0; j < m; ++j) pk_vertex(e[j], b, vertices + (g0 + j) * 4);
    }
    for (uint64_t g = 0; g < n && K; ++g) {
        const float* f = records + g * 80;
        uint8_t* out = sh + g * 3 * (uint64_t)K;
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < K; ++i) {
                const float v = f[16 + 4 * (i + 1) + c];
                bad += !pk_finite(v);
                out[c * K + i] = (uint8_t)pk_sh_byte(v);
            }
    }
    if (bad_out) *bad_out = bad;
}

void gs_pack_decode_host(const float* chunks, const uint32_t* vertices, const uint8_t* sh, uint64_t n, int sh_degree, const float* table,
                         float* records) {
    const int K = gs_pack_rest(sh_degree);
    for (uint64_t g = 0; g < n; ++g) {
        float* f = records + g * 80;
        memset(f, 0, 320);
        const PkDecoded d = pk_decode(vertices + g * 4, chunks + (g / GS_PACK_CHUNK) * GS_PACK_CHUNK_FLOATS, table);
        for (int k = 0; k < 3; ++k) { f[k] = d.pos[k]; f[4 + k] = d.lsc[k]; f[16 + k] = d.dc[k]; }
        for (int k = 0; k < 4; ++k) f[8 + k] = d.rot[k];
        f[12] = d.logit;
        const uint8_t* in = sh + g * 3 * (uint64_t)K;
        for (int c = 0; c < 3 && K; ++c)
            for (int i = 0; i < K; ++i) f[16 + 4 * (i + 1) + c] = pk_sh_value(in[c * K + i]);
    }
}

// ---- the file -----------------------------------------------------------------------------------------------------------------------
static const char* const kChunkProps[18] = {"min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_scale_x", "min_scale_y", "min_scale_z",
                                            "max_scale_x", "max_scale_y", "max_scale_z", "min_r", "min_g", "min_b", "max_r", "max_g", "max_b"};
static const char* const kVertexProps[4] = {"packed_position", "packed_rotation", "packed_scale", "packed_color"};
static const char kMarker[] = "comment gsplat-packed 1";

std::string gs_pack_header(uint64_t n, int sh_degree) {
    const int K = gs_pack_rest(sh_degree);
    std::string h = std::string("ply\nformat binary_little_endian 1.0\n") + kMarker + "\nelement chunk " + std::to_string(gs_pack_chunks(n)) + "\n";
    for (const char* p : kChunkProps) h += std::string("property float ") + p + "\n";
    h += "element vertex " + std::to_string(n) + "\n";
    for (const char* p : kVertexProps) h += std::string("property uint ") + p + "\n";
    if (K) {
        h += "element sh " + std::to_string(n) + "\n";
        for (int k = 0; k < 3 * K; ++k) h += "property uchar f_rest_" + std::to_string(k) + "\n";
    }
    return h + "end_header\n";
}
uint64_t gs_pack_file_bytes(uint64_t n, int sh_degree) {
    return gs_pack_header(n, sh_degree).size() + gs_pack_chunks(n) * 72u + n * 16u + n * 3u * (uint64_t)gs_pack_rest(sh_degree);
}

// A decimal count below 2^31 and nothing else (no sign, no blank, no leading zero but "0" itself).
static bool parse_count(const std::string& s, uint64_t* out) {
    if (s.empty() || s.size() > 10 || (s.size() > 1 && s[0] == '0')) return false;
    uint64_t v = 0;
    for (char ch : s) {
        if (ch < '0' || ch > '9') return false;
        v = v * 10 + (uint64_t)(ch - '0');
    }
    if (v >= (1ull << 31)) return false;
    *out = v;
    return true;
}

int32_t gs_pack_parse_header(const char* who, const char* path, const unsigned char* head, size_t len, uint64_t file_size, GsPackLayout* L, char* err,
                             size_t errlen) {
    size_t pos = 0;
    int line_no = 0;
    std::string line;
    auto next = [&]() { // the next line without its newline; false at the end of `head`
        size_t e = pos;
        while (e < len && head[e] != '\n') ++e;
        if (e >= len) return false;
        line.assign((const char*)head + pos, e - pos);
        pos = e + 1;
        ++line_no;
        return true;
    };
    auto bad = [&](const char* what) {
        return refuse(err, errlen, GS_ERR_INVALID_ARGUMENT, "%s: %s: %s (header line %d)", who, path, what, line_no);
    };
    auto expect = [&](const std::string& want) { return next() && line == want; };
    auto element = [&](const char* name, uint64_t* count) {
        const std::string pre = std::string("element ") + name + " ";
        return line.compare(0, pre.size(), pre) == 0 && parse_count(line.substr(pre.size()), count);
    };
    if (!expect("ply")) return bad("not a ply file");
    if (!expect("format binary_little_endian 1.0")) return bad("the format is not binary_little_endian 1.0");
    if (!expect(kMarker)) return bad("the marker line 'comment gsplat-packed 1' is missing");
    uint64_t C = 0, n = 0, nsh = 0;
    if (!next() || !element("chunk", &C)) return bad("'element chunk <count>' expected");
    for (const char* p : kChunkProps)
        if (!expect(std::string("property float ") + p)) return bad("a chunk property is missing, renamed or of another type");
    if (!next() || !element("vertex", &n)) return bad("'element vertex <count>' expected");
    for (const char* p : kVertexProps)
        if (!expect(std::string("property uint ") + p)) return bad("a vertex property is missing, renamed or of another type");
    if (C != gs_pack_chunks(n)) return bad("the chunk count is not ceil(vertices / 256)");
    if (!next()) return bad("the header ends early");
    int degree = 0;
    if (line != "end_header") {
        if (!element("sh", &nsh)) return bad("'element sh <count>' or end_header expected");
        if (nsh != n) return bad("the sh count differs from the vertex count");
        int props = 0;
        for (;;) {
            if (!next()) return bad("the header ends early");
            if (line == "end_header") break;
            if (props >= 45 || line != "property uchar f_rest_" + std::to_string(props)) return bad("an sh property is missing, renamed or of another type");
            ++props;
        }
        degree = props == 9 ? 1 : props == 24 ? 2 : props == 45 ? 3 : -1;
        if (degree < 0) return bad("the sh element does not hold 9, 24 or 45 properties (degree 1, 2 or 3)");
    }
    GsPackLayout o;
    o.n = n; o.chunks = C; o.degree = degree;
    o.chunk_off = pos;
    o.vertex_off = o.chunk_off + C * 72u;
    o.sh_off = o.vertex_off + n * 16u;
    o.file_bytes = o.sh_off + n * 3u * (uint64_t)gs_pack_rest(degree);
    if (file_size != o.file_bytes) {
        return refuse(err, errlen, GS_ERR_INVALID_ARGUMENT, "%s: %s: the file holds %llu bytes, its header implies %llu", who, path,
                      (unsigned long long)file_size, (unsigned long long)o.file_bytes);
    }
    *L = o;
    return GS_OK;
}

namespace {
struct Closer {
    FILE* fp;
    ~Closer() { if (fp) fclose(fp); }
};
}

int32_t gs_pack_save_host(const char* path, const void* records, uint64_t n, int32_t sh_degree, char* err, size_t errlen) {
    static const char who[] = "gs_pack_save";
    if (!path) return refuse(err, errlen, GS_ERR_INVALID_ARGUMENT, "%s: null path", who);
    if (!records && n) return refuse(err, errlen, GS_ERR_INVALID_ARGUMENT, "%s: null records (%s)", who, path);
    if (sh_degree < 0 || sh_degree > 3) return refuse(err, errlen, GS_ERR_INVALID_ARGUMENT, "%s: sh_degree %d is not 0..3 (%s)", who, sh_degree, path);
    if (n >= (1ull << 31)) return refuse(err, errlen, GS_ERR_INVALID_ARGUMENT, "%s: %llu records reach the limit of 2^31 (%s)", who, (unsigned long long)n, path);
    const uint64_t K = (uint64_t)gs_pack_rest(sh_degree), C = gs_pack_chunks(n);
    std::vector<float> chunks;
    std::vector<uint32_t> vertices;
    std::vector<uint8_t> sh;
    try {
        chunks.resize((size_t)(C * 18u));
        vertices.resize((size_t)(n * 4u));
        sh.resize((size_t)(n * 3u * K));
    } catch (const std::bad_alloc&) {
        return refuse(err, errlen, GS_ERR_OUT_OF_MEMORY, "%s: out of host memory (%s)", who, path);
    }
    gs_pack_encode_host((const float*)records, n, sh_degree, chunks.data(), vertices.data(), sh.data(), nullptr);
    const std::string h = gs_pack_header(n, sh_degree);
    FILE* fp = fopen(path, "wb");
    if (!fp) return refuse(err, errlen, GS_ERR_INVALID_ARGUMENT, "%s: cannot create %s: %s", who, path, strerror(errno));
    auto put = [&](const void* p, size_t bytes) { return !bytes || fwrite(p, 1, bytes, fp) == bytes; }; // (an empty vector's data() may be null)
    bool ok = put(h.data(), h.size());
    ok = ok && put(chunks.data(), chunks.size() * 4);
    ok = ok && put(vertices.data(), vertices.size() * 4);
    ok = ok && put(sh.data(), sh.size());
    ok = (fclose(fp) == 0) && ok; // (a full disk may only show when the buffered tail is flushed)
    if (!ok) {
        const int32_t rc = refuse(err, errlen, GS_ERR_INVALID_ARGUMENT, "%s: cannot write %s: %s", who, path, strerror(errno));
        remove(path);
        return rc;
    }
    return GS_OK;
}

int32_t gs_pack_load_host(const char* path, void** records, uint64_t* n_out, int32_t* sh_degree, char* err, size_t errlen) {
    static const char who[] = "gs_pack_load";
    if (!path || !records || !n_out) return refuse(err, errlen, GS_ERR_INVALID_ARGUMENT, "%s: null argument", who);
    Closer f{fopen(path, "rb")};
    if (!f.fp) return refuse(err, errlen, GS_ERR_INVALID_ARGUMENT, "%s: cannot open %s", who, path);
    unsigned char head[8192];
    const size_t got = fread(head, 1, sizeof(head), f.fp);
    if (fseek(f.fp, 0, SEEK_END) != 0) return refuse(err, errlen, GS_ERR_INVALID_ARGUMENT, "%s: cannot seek in %s", who, path);
    const long fsize = ftell(f.fp);
    GsPackLayout L;
    const int32_t rc = gs_pack_parse_header(who, path, head, got, (uint64_t)(fsize < 0 ? 0 : fsize), &L, err, errlen);
    if (rc != GS_OK) return rc;
    // the counts are now backed by the file's size: allocate
    const size_t data = (size_t)(L.file_bytes - L.chunk_off);
    unsigned char* raw = (unsigned char*)malloc(data ? data : 1);
    float* out = (float*)malloc(L.n ? (size_t)L.n * 320 : 1);
    struct Free { void* a; void* b; ~Free() { free(a); free(b); } } guard{raw, out};
    if (!raw || !out) return refuse(err, errlen, GS_ERR_OUT_OF_MEMORY, "%s: out of host memory (%s)", who, path);
    if (fseek(f.fp, (long)L.chunk_off, SEEK_SET) != 0 || fread(raw, 1, data, f.fp) != data)
        return refuse(err, errlen, GS_ERR_INVALID_ARGUMENT, "%s: %s: short read", who, path);
    // (chunk_off is a header length: not a multiple of 4; the sections are copied to aligned arrays one trip at a time)
    std::vector<float> chunks((size_t)(L.chunks * 18u));
    if (!chunks.empty()) memcpy(chunks.data(), raw, chunks.size() * 4);
    const unsigned char* vsec = raw + (L.vertex_off - L.chunk_off);
    const unsigned char* ssec = raw + (L.sh_off - L.chunk_off);
    const uint64_t K3 = 3u * (uint64_t)gs_pack_rest(L.degree);
    const uint64_t trip = 65536; // whole chunks
    std::vector<uint32_t> verts((size_t)(trip * 4u));
    for (uint64_t g0 = 0; g0 < L.n; g0 += trip) {
        const uint64_t m = L.n - g0 < trip ? L.n - g0 : trip;
        memcpy(verts.data(), vsec + g0 * 16u, (size_t)(m * 16u));
        gs_pack_decode_host(chunks.data() + (g0 / 256u) * 18u, verts.data(), ssec + g0 * K3, m, L.degree, gs_pack_logits(), out + g0 * 80u);
    }
    guard.b = nullptr;
    *records = out;
    *n_out = L.n;
    if (sh_degree) *sh_degree = L.degree;
    return GS_OK;
}
