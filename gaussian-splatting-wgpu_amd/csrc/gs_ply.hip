// gs_ply.hip -- the native PLY loader: header parser, gs_ply_load (to host records), gs_upload_ply (streamed
// to the resident scene arrays).  Part of the C ABI (include/gsplat/gs_abi.h).
//
// Restates PackedGaussians (reference src/ply.ts:49-228) in C++: header rules of decodeHeader (:49-102: `element
// vertex N`, properties in file order, data right after "end_header\n"), readRawVertex (:104-123: ONLY float and
// uchar properties consume bytes; uchar is value/255), the SH read order f_dc_{0..2} then f_rest_{rgb*K+i}
// (:179-187), degree from the f_rest count (:168-176), and the packed 320-byte record (:190-198).  Degrees < 3 are
// zero-padded to 16 coefficients (the shader hard-codes 16: process_gaussians.wgsl:6).  The reference spends
// "seconds to a couple of minutes" here in JS (index.html:16); this is a single pass over a read() of the file.
#include <cstdlib>
#include <string>
#include <thread>

#include "gs_runtime.h"

struct PlyProp { std::string name; int type; /* 0 other (0 bytes), 1 float, 2 uchar */ uint32_t offset; };

// (PlyLayout, what the header says about a vertex, is in gs_runtime.h: the splat insertion streams a file too.)

// header: the first bytes of the file (at least up to and including "end_header\n")
static int32_t ply_parse_header(const unsigned char* buf, size_t len, PlyLayout& L) {
    static const char kEnd[] = "end_header";
    size_t hdr_end = std::string::npos;
    for (size_t i = 0; i + sizeof(kEnd) - 1 <= len; ++i)
        if (memcmp(buf + i, kEnd, sizeof(kEnd) - 1) == 0) { hdr_end = i; break; }
    if (hdr_end == std::string::npos) return fail(GS_ERR_INVALID_ARGUMENT, "gs_ply_load: no end_header");
    const std::string header((const char*)buf, hdr_end + sizeof(kEnd) - 1);
    L.data_off = hdr_end + sizeof(kEnd) - 1 + 1; // the byte after "end_header" (the newline), ply.ts:94
    std::vector<PlyProp> props;
    size_t pos = 0;
    while (pos < header.size()) {
        size_t eol = header.find('\n', pos);
        if (eol == std::string::npos) eol = header.size();
        std::string line = header.substr(pos, eol - pos);
        pos = eol + 1;
        size_t a = line.find_first_not_of(" \t\r"), b = line.find_last_not_of(" \t\r");
        if (a == std::string::npos) continue;
        line = line.substr(a, b - a + 1);
        if (line.rfind("element vertex", 0) == 0) {
            size_t d = line.find_first_of("0123456789");
            if (d != std::string::npos) L.vertex_count = strtoull(line.c_str() + d, nullptr, 10);
        } else if (line.rfind("property", 0) == 0) {
            char w0[64], w1[64], w2[128];
            if (sscanf(line.c_str(), "%63s %63s %127s", w0, w1, w2) == 3) {
                int type = strcmp(w1, "float") == 0 ? 1 : strcmp(w1, "uchar") == 0 ? 2 : 0;
                bool dup = false;
                for (auto& p : props) if (p.name == w2) { p.type = type; dup = true; }
                if (!dup) props.push_back({w2, type, 0});
            }
        } else if (line == "end_header") {
            break;
        }
    }
    uint32_t stride = 0, n_rest = 0;
    for (auto& p : props) {
        p.offset = stride;
        stride += p.type == 1 ? 4u : p.type == 2 ? 1u : 0u;
        if (p.name.rfind("f_rest_", 0) == 0) ++n_rest;
    }
    L.stride = stride;
    const uint32_t per_color = n_rest / 3;
    int degree = -1;
    for (int d = 0; d <= 3; ++d) if ((uint32_t)((d + 1) * (d + 1) - 1) == per_color && n_rest % 3 == 0) degree = d;
    if (degree < 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_ply_load: Unsupported SH degree (%u f_rest properties)", n_rest); // ply.ts:136
    L.degree = degree;
    auto find = [&](const std::string& name) -> const PlyProp* {
        for (auto& p : props) if (p.name == name) return &p;
        return nullptr;
    };
    const char* base_names[11] = {"x", "y", "z", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3", "opacity"};
    const int base_slot[11] = {0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12};
    L.nsrc = 0;
    L.all_float = true;
    auto add = [&](const PlyProp* p, int sl) {
        L.soff[L.nsrc] = p->offset; L.stype[L.nsrc] = (uint32_t)p->type; L.slot[L.nsrc] = (uint32_t)sl; ++L.nsrc;
        L.all_float = L.all_float && p->type == 1;
    };
    for (int i = 0; i < 11; ++i) {
        const PlyProp* p = find(base_names[i]);
        if (!p) return fail(GS_ERR_INVALID_ARGUMENT, "gs_ply_load: missing property %s", base_names[i]);
        add(p, base_slot[i]);
    }
    const int nsh = (degree + 1) * (degree + 1);
    for (int k = 0; k < nsh; ++k)
        for (int c = 0; c < 3; ++c) {
            char nm[32];
            if (k == 0) snprintf(nm, sizeof(nm), "f_dc_%d", c);
            else snprintf(nm, sizeof(nm), "f_rest_%u", (unsigned)(c * per_color + (k - 1)));
            const PlyProp* p = find(nm);
            if (!p) return fail(GS_ERR_INVALID_ARGUMENT, "gs_ply_load: missing property %s", nm);
            add(p, 16 + 4 * k + c);
        }
    return GS_OK;
}

GS_EXPORT int32_t gs_ply_load(const char* path, void** records, uint64_t* n_out, int32_t* sh_degree) {
    if (!path || !records || !n_out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_ply_load: null argument");
    *records = nullptr;
    *n_out = 0;
    File fp(fopen(path, "rb"));
    if (!fp) return fail(GS_ERR_INVALID_ARGUMENT, "gs_ply_load: cannot open %s", path);
    fseek(fp, 0, SEEK_END);
    const long fsize = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    struct FileBuf { // uninitialised storage: a std::vector would spend a pass zero-filling it
        unsigned char* p = nullptr; size_t n = 0;
        ~FileBuf() { free(p); }
        unsigned char* data() const { return p; }
        size_t size() const { return n; }
    } buf;
    buf.n = (size_t)std::max<long>(fsize, 0);
    buf.p = (unsigned char*)malloc(std::max<size_t>(buf.n, 1));
    if (!buf.p) return fail(GS_ERR_OUT_OF_MEMORY, "gs_ply_load: out of host memory");
    if (fsize > 0 && fread(buf.p, 1, (size_t)fsize, fp) != (size_t)fsize) return fail(GS_ERR_INVALID_ARGUMENT, "gs_ply_load: short read");
    fp.reset();
    PlyLayout L;
    int32_t rc = ply_parse_header(buf.data(), buf.size(), L);
    if (rc != GS_OK) return rc;
    const uint64_t vertex_count = L.vertex_count;
    const uint32_t stride = L.stride;
    if (buf.size() < L.data_off + vertex_count * (uint64_t)stride) return fail(GS_ERR_INVALID_ARGUMENT, "gs_ply_load: vertex data truncated");
    float* out = (float*)calloc((size_t)std::max<uint64_t>(vertex_count, 1) * 80, sizeof(float));
    if (!out) return fail(GS_ERR_OUT_OF_MEMORY, "gs_ply_load: out of host memory");
    // vertices are independent, so the pass is split over threads
    const unsigned char* vbase = buf.data() + L.data_off;
    auto work = [&](uint64_t i0, uint64_t i1) {
        for (uint64_t i = i0; i < i1; ++i) {
            const unsigned char* v = vbase + i * stride;
            float* rec = out + i * 80;
            if (L.all_float) {
                for (int s2 = 0; s2 < L.nsrc; ++s2) memcpy(&rec[L.slot[s2]], v + L.soff[s2], 4);
            } else {
                for (int s2 = 0; s2 < L.nsrc; ++s2) {
                    float f = 0.0f; // a property of another type reads as `undefined` in the reference; 0 here
                    if (L.stype[s2] == 1) memcpy(&f, v + L.soff[s2], 4);
                    else if (L.stype[s2] == 2) f = (float)((double)v[L.soff[s2]] / 255.0);
                    rec[L.slot[s2]] = f;
                }
            }
        }
    };
    unsigned nthreads = std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (vertex_count < 65536) nthreads = 1;
    std::vector<std::thread> pool;
    for (unsigned th = 1; th < nthreads; ++th)
        pool.emplace_back(work, vertex_count * th / nthreads, vertex_count * (th + 1) / nthreads);
    work(0, vertex_count / nthreads);
    for (auto& th : pool) th.join();
    *records = out;
    *n_out = vertex_count;
    if (sh_degree) *sh_degree = L.degree;
    return GS_OK;
}

GS_EXPORT void gs_ply_free(void* records) { free(records); }

// Streams a .ply straight into the resident scene arrays: the file is read in trips of 64 Ki vertices into one of
// two pinned staging buffers, copied to the device and converted THERE into the final layout (position planes, geometry and SH
// records: gs_ply_chunk_kernel) while the next trip is being read (TripRing::feed, gs_runtime.h).  No N x 320-byte array exists on
// either side: peak host memory is the two staging buffers (2 x 64 Ki x vertex stride, ~32 MB), whatever the size of the scene.  The
// reference builds the whole packed buffer in JS first (ply.ts:204-228: "seconds to a couple of minutes", index.html:16).  The
// callers are upload_source (gs_runtime.h) and append_source (gs_insert.hip): into a new scene, or into the tail of a grown one.
int32_t PlySource::open(const char* who, const char* path) {
    fp = File(fopen(path, "rb"));
    if (!fp) return fail(GS_ERR_INVALID_ARGUMENT, "%s: cannot open %s", who, path);
    std::vector<unsigned char> head(1 << 16);
    const size_t got = fread(head.data(), 1, head.size(), fp);
    int32_t rc = ply_parse_header(head.data(), got, L);
    if (rc != GS_OK) return rc;
    fseek(fp, 0, SEEK_END);
    const uint64_t fsize = (uint64_t)ftell(fp);
    const uint64_t n = L.vertex_count;
    if (n >= (1ull << 31)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: too many gaussians", who);
    if (fsize < L.data_off + n * (uint64_t)L.stride) return fail(GS_ERR_INVALID_ARGUMENT, "%s: vertex data truncated", who);
    if (L.stride > 0xFFFFu) return fail(GS_ERR_INVALID_ARGUMENT, "%s: vertex stride %u too large", who, L.stride); // (GsPlyTable: u16 offsets)
    return GS_OK;
}

int32_t PlySource::stream(const char* who, gs_ctx* c, const GsScene& dst, uint64_t first) {
    const uint64_t n = L.vertex_count;
    if (L.degree < 3 && n) { // coefficients the file does not have stay 0 (the shader hard-codes 16: process_gaussians.wgsl:6)
        hipError_t e0 = hipMemsetAsync((char*)dst.sh + (size_t)first * 192, 0, (size_t)n * 192, c->stream);
        if (e0 != hipSuccess) return fail(GS_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e0));
    }
    TripRing ring;
    int32_t rc = ring.init(std::max<size_t>((size_t)kStreamTrip * L.stride, 256), true);
    if (rc != GS_OK) return rc;
    GsPlyTable tab;
    tab.stride = L.stride; tab.nsrc = (uint32_t)L.nsrc; tab.all_float = L.all_float ? 1u : 0u;
    for (int k = 0; k < L.nsrc; ++k) { tab.soff[k] = (uint16_t)L.soff[k]; tab.stype[k] = (uint8_t)L.stype[k]; tab.slot[k] = (uint8_t)L.slot[k]; }
    fseek(fp, (long)L.data_off, SEEK_SET);
    rc = ring.feed((n + kStreamTrip - 1) / kStreamTrip, c->stream, [&](uint64_t it, unsigned char* h, unsigned char* d) {
        const uint64_t v0 = it * kStreamTrip, m = std::min(kStreamTrip, n - v0);
        if (fread(h, 1, (size_t)(m * L.stride), fp) != (size_t)(m * L.stride)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: short read", who);
        HIP_TRY(hipMemcpyAsync(d, h, (size_t)(m * L.stride), hipMemcpyHostToDevice, c->stream));
        gs_launch_ply_chunk(d, (uint32_t)m, (uint32_t)(first + v0), tab, dst, c->stream);
        return (int32_t)GS_OK;
    });
    if (rc != GS_OK) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

GS_EXPORT int32_t gs_upload_ply(gs_ctx* c, const char* path, uint64_t* n_out) {
    return upload_source<PlySource>("gs_upload_ply", c, path, n_out);
}
