// gs_pack.hip -- the packed scenes' entry points: the host codec's forwards, the export of resident splats into the 16-byte chunked
// format, the upload of such a file and the two halves of its stream (gs_append_packed is with the other insertions in
// gs_insert.hip: it shares their refusals and their install).  Part of the C ABI (include/gsplat/gs_abi.h "packed scenes"); the
// kernels are in k_pack.hip, the codec in gs_pack_math.h, the file's header, writer and loader in gs_pack_host.hip.
//
// The reference has no counterpart: its only container is the float .ply (ply.ts:49-228), 248 bytes per splat at degree 3, and for a
// scene streamed in from a file that file is the only host copy there would ever be.  An export here encodes the whole selection on
// the device (at most 61 bytes per splat of scratch beside the scene) and streams the three sections to the file through two pinned
// buffers; an upload reads the file in trips of whole chunks through two pinned buffers and decodes on the device.  Neither holds
// the scene on the host.
//
// Every resident call drains the context's ring first (resident_begin), runs on the context's stream and returns when done.  None
// of them launches anything in a frame: a context that never calls them launches exactly what it did before.
#include <cerrno>
#include <string>

#include "gs_pack_math.h"
#include "gs_runtime.h"

static_assert(sizeof(gs_pack_info) == 32 && offsetof(gs_pack_info, nonfinite) == 24, "gs_pack_info layout");

// ---- the host codec: forwards to gs_pack_host.hip (the message goes through the library's error channel) ---------------------------
static int32_t degree_check(const char* who, int32_t sh_degree) {
    if (sh_degree < 0 || sh_degree > 3) return fail(GS_ERR_INVALID_ARGUMENT, "%s: sh_degree %d is not 0..3", who, sh_degree);
    return GS_OK;
}
GS_EXPORT int32_t gs_pack_encode(const void* aos320, uint64_t n, int32_t sh_degree, float* chunks, uint32_t* vertices, uint8_t* sh, uint64_t* nonfinite) {
    const int32_t rc = degree_check("gs_pack_encode", sh_degree);
    if (rc != GS_OK) return rc;
    if (n && (!aos320 || !chunks || !vertices || (sh_degree > 0 && !sh))) return fail(GS_ERR_INVALID_ARGUMENT, "gs_pack_encode: null argument");
    gs_pack_encode_host((const float*)aos320, n, sh_degree, chunks, vertices, sh, nonfinite);
    return GS_OK;
}
GS_EXPORT int32_t gs_pack_decode(const float* chunks, const uint32_t* vertices, const uint8_t* sh, uint64_t n, int32_t sh_degree, void* aos320) {
    const int32_t rc = degree_check("gs_pack_decode", sh_degree);
    if (rc != GS_OK) return rc;
    if (n && (!aos320 || !chunks || !vertices || (sh_degree > 0 && !sh))) return fail(GS_ERR_INVALID_ARGUMENT, "gs_pack_decode: null argument");
    gs_pack_decode_host(chunks, vertices, sh, n, sh_degree, gs_pack_logits(), (float*)aos320);
    return GS_OK;
}
GS_EXPORT int32_t gs_pack_logit_table(float out[256]) {
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_pack_logit_table: null argument");
    memcpy(out, gs_pack_logits(), 256 * sizeof(float));
    return GS_OK;
}
GS_EXPORT int32_t gs_pack_save(const char* path, const void* records, uint64_t n, int32_t sh_degree) {
    char err[480] = "";
    const int32_t rc = gs_pack_save_host(path, records, n, sh_degree, err, sizeof(err));
    return rc == GS_OK ? rc : fail(rc, "%s", err);
}
GS_EXPORT int32_t gs_pack_load(const char* path, void** records, uint64_t* n, int32_t* sh_degree) {
    char err[480] = "";
    const int32_t rc = gs_pack_load_host(path, records, n, sh_degree, err, sizeof(err));
    return rc == GS_OK ? rc : fail(rc, "%s", err);
}

// ---- export -------------------------------------------------------------------------------------------------------------------------
// The selection's ids (sel, ascending; null: every index) in Morton order: the bounds of its splats with three finite coordinates
// (the neighbourhoods' bounds kernel under the selection's filter), the keys, the frame path's pair sort behind a private control
// block, driven as gs_neigh.hip's sorted_records drives it (four 8-bit passes: the keys reach 1 << 30).  *out: the sorted values,
// in the neighbourhoods' scratch.
static int32_t morton_order(gs_ctx* c, const char* who, uint32_t mask, uint32_t value, const uint32_t* sel, uint32_t m, const uint32_t** out) {
    gs_ctx::Neigh& s = c->ng;
    if (m >= (1u << 30)) return fail(GS_ERR_CAPACITY, "%s: %u splats, the Morton sort takes fewer than 2^30", who, m);
    const uint32_t passes = 4;
    const size_t ctl_sz = (sizeof(GsControl) + 255) & ~(size_t)255;
    const size_t st_sz = (size_t)passes * gs_sort_tiles(m) * 256 * 4;
    int32_t rc;
    if ((rc = s.bounds.reserve(16)) != GS_OK || (rc = s.keysA.reserve(m)) != GS_OK || (rc = s.valsA.reserve(m)) != GS_OK ||
        (rc = s.keysB.reserve(m)) != GS_OK || (rc = s.valsB.reserve(m)) != GS_OK || (rc = s.ctl.reserve(ctl_sz + st_sz)) != GS_OK)
        return rc;
    uint32_t hb[16] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    HIP_TRY(hipMemcpyAsync(s.bounds, hb, sizeof(hb), hipMemcpyHostToDevice, c->stream));
    gs_launch_neigh_bounds((mask | value) ? c->scene.state : nullptr, c->scene, c->n, mask, value, mask, value, s.bounds, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hb, s.bounds, sizeof(hb), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    GsPackBox box{};
    if (hb[7]) // (no splat with finite coordinates: every key is GS_PACK_KEY_LAST, the box is not read)
        for (int k = 0; k < 3; ++k) { box.lo[k] = pk_okey_value(hb[k]); box.hi[k] = pk_okey_value(hb[3 + k]); }
    HIP_TRY(hipMemsetAsync(s.ctl, 0, ctl_sz + st_sz, c->stream));
    GsControl* ctl = (GsControl*)s.ctl.get(); // view; the sort's status words follow it
    s.n32 = m;
    HIP_TRY(hipMemcpyAsync(&ctl->num_intersections, &s.n32, 4, hipMemcpyHostToDevice, c->stream));
    gs_launch_pack_keys(c->scene, c->n, sel, m, box, s.keysA, s.valsA, c->stream);
    const GsSort plan{{s.keysA, s.valsA}, {s.keysB, s.valsB}, passes, 8, 0, false, false}; // 8-bit digits of the key itself, counted by the sort
    const GsSortPair sorted = gs_launch_sort(plan, ctl, (uint32_t*)(s.ctl.get() + ctl_sz), m, std::max(c->opt.grid_persist, 1u), c->stream);
    HIP_TRY(hipGetLastError());
    uint32_t fault = 0;
    HIP_TRY(hipMemcpyAsync(&fault, &ctl->fault, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (fault) return fail(GS_ERR_DEVICE_FAULT, "%s: look-back spin bound exceeded in the Morton sort", who);
    *out = sorted.vals;
    return GS_OK;
}

// The file being written: closed by the destructor and, unless finish() succeeded, removed.
namespace {
struct PackWriter {
    const char* who;
    std::string path;
    FILE* fp = nullptr;
    bool done = false;
    PackWriter(const char* w, const char* p) : who(w), path(p) {}
    ~PackWriter() {
        if (fp) fclose(fp);
        if (fp && !done) remove(path.c_str());
    }
    int32_t err(const char* what) const { return fail(GS_ERR_INVALID_ARGUMENT, "%s: cannot %s %s: %s", who, what, path.c_str(), strerror(errno)); }
    int32_t open(const std::string& header) {
        fp = fopen(path.c_str(), "wb");
        if (!fp) return err("create");
        return fwrite(header.data(), 1, header.size(), fp) == header.size() ? GS_OK : err("write");
    }
    int32_t write(const void* p, size_t bytes) { return fwrite(p, 1, bytes, fp) == bytes ? GS_OK : err("write"); }
    int32_t finish() { // (a full disk may only show when the buffered tail is flushed)
        FILE* f = fp;
        fp = nullptr;
        if (fclose(f) == 0) { done = true; return GS_OK; }
        const int32_t rc = err("write");
        remove(path.c_str());
        return rc;
    }
};
// The two pinned bounce buffers of an export: `bytes` of device memory go to the file, the host writing trip k - 1 while trip k is
// being copied (gs_export_ply's scheme).
struct Bounce {
    static constexpr size_t kTrip = (size_t)1 << 20; // 65 536 vertices
    PinnedBuf<unsigned char> h[2]; // (an early exit frees them under a copy still in flight: the free waits for the device)
    Event done[2];
    int32_t init(size_t largest) {
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(hipHostMalloc(h[k].out(), std::max<size_t>(std::min(largest, kTrip), 256), hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(done[k].out(), hipEventDisableTiming));
        }
        return GS_OK;
    }
    int32_t drain(const unsigned char* dev, size_t bytes, PackWriter& w, hipStream_t st) {
        const size_t trips = (bytes + kTrip - 1) / kTrip;
        for (size_t it = 0; it <= trips && trips; ++it) {
            if (it < trips) {
                const size_t at = it * kTrip, m = std::min(kTrip, bytes - at);
                HIP_TRY(hipMemcpyAsync(h[it & 1], dev + at, m, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipEventRecord(done[it & 1], st));
            }
            if (it >= 1) { // its pinned buffer is not written again before trip it + 1 is enqueued
                const size_t at = (it - 1) * kTrip, m = std::min(kTrip, bytes - at);
                HIP_TRY(hipEventSynchronize(done[(it - 1) & 1]));
                const int32_t rc = w.write(h[(it - 1) & 1], m);
                if (rc != GS_OK) return rc;
            }
        }
        return GS_OK;
    }
};
}

GS_EXPORT int32_t gs_export_packed(gs_ctx* c, const char* path, uint32_t mask, uint32_t value, int32_t sh_degree, int32_t order, gs_pack_info* info,
                                   uint32_t* ids_out) {
    static const char who[] = "gs_export_packed";
    int32_t rc = resident_begin(c, who, Plane::filtered, mask, value);
    if (rc != GS_OK) return rc;
    if (!path) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null path", who);
    if (sh_degree < 0 || sh_degree > 3) return fail(GS_ERR_INVALID_ARGUMENT, "%s: sh_degree %d is not 0..3 (%s)", who, sh_degree, path);
    if (order != GS_PACK_ORDER_INDEX && order != GS_PACK_ORDER_MORTON)
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: order %d is neither GS_PACK_ORDER_INDEX nor GS_PACK_ORDER_MORTON (%s)", who, order, path);
    const bool all = !(mask | value);
    uint64_t total = c->n;
    if (!all) {
        rc = edit_select(c, mask, value, true, &total);
        if (rc != GS_OK) return rc;
    }
    const uint32_t m = (uint32_t)total;
    const uint32_t* sel = all ? nullptr : c->ex.ids.get();
    if (order == GS_PACK_ORDER_MORTON && m) {
        rc = morton_order(c, who, mask, value, sel, m, &sel);
        if (rc != GS_OK) return rc;
    }
    // the three sections and the counts of replaced floats, in one allocation: vertices | chunk records | SH bytes (whole chunks) | counts
    const uint32_t K = (uint32_t)gs_pack_rest(sh_degree);
    const uint64_t C = gs_pack_chunks(m);
    const size_t vert_at = 0, chunk_at = (size_t)m * 16, sh_at = chunk_at + (size_t)C * 72, bad_at = sh_at + (size_t)C * 768 * K,
                 bytes = bad_at + (size_t)C * 5 * 4;
    DevBuf<unsigned char> enc;
    HIP_TRY(hipMalloc(enc.out(), std::max<size_t>(bytes, 256)));
    gs_launch_pack_encode(c->scene, c->n, sel, m, K, (float*)(enc.get() + chunk_at), enc.get() + vert_at, enc.get() + sh_at,
                          (uint32_t*)(enc.get() + bad_at), c->stream);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> bad((size_t)C * (K ? 5 : 1));
    if (!bad.empty()) HIP_TRY(hipMemcpyAsync(bad.data(), enc.get() + bad_at, bad.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    gs_pack_info out{};
    out.count = m;
    out.chunks = C;
    for (uint32_t b : bad) out.nonfinite += b;
    const std::string header = gs_pack_header(m, sh_degree);
    out.file_bytes = header.size() + C * 72 + (uint64_t)m * 16 + (uint64_t)m * 3 * K;
    PackWriter w(who, path);
    rc = w.open(header);
    if (rc != GS_OK) return rc;
    Bounce bounce;
    rc = bounce.init(std::max<size_t>({(size_t)C * 72, (size_t)m * 16, (size_t)m * 3 * K})); // the largest section (or one trip)
    if (rc != GS_OK) return rc;
    if ((rc = bounce.drain(enc.get() + chunk_at, (size_t)C * 72, w, c->stream)) != GS_OK) return rc;
    if ((rc = bounce.drain(enc.get() + vert_at, (size_t)m * 16, w, c->stream)) != GS_OK) return rc;
    if ((rc = bounce.drain(enc.get() + sh_at, (size_t)m * 3 * K, w, c->stream)) != GS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    rc = w.finish();
    if (rc != GS_OK) return rc;
    if (ids_out && m) {
        if (!sel) for (uint32_t i = 0; i < m; ++i) ids_out[i] = i;
        else HIP_TRY(hipMemcpy(ids_out, sel, (size_t)m * 4, hipMemcpyDeviceToHost));
    }
    if (info) *info = out;
    return GS_OK;
}

// ---- upload: the two halves (gs_runtime.h), shared with gs_append_packed ------------------------------------------------------------
int32_t pack_open(const char* who, const char* path, PackSource* src) {
    src->fp = File(fopen(path, "rb"));
    if (!src->fp) return fail(GS_ERR_INVALID_ARGUMENT, "%s: cannot open %s", who, path);
    unsigned char head[8192];
    const size_t got = fread(head, 1, sizeof(head), src->fp);
    if (fseek(src->fp, 0, SEEK_END) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "%s: cannot seek in %s", who, path);
    const long fsize = ftell(src->fp);
    char err[480] = "";
    const int32_t rc = gs_pack_parse_header(who, path, head, got, (uint64_t)(fsize < 0 ? 0 : fsize), &src->L, err, sizeof(err));
    return rc == GS_OK ? rc : fail(rc, "%s", err);
}

int32_t pack_stream(const char* who, gs_ctx* c, PackSource& src, const GsScene& dst, uint64_t first) {
    const GsPackLayout& L = src.L;
    FILE* const fp = src.fp;
    const uint64_t n = L.n, K = (uint64_t)gs_pack_rest(L.degree), K3 = 3 * K;
    const uint64_t CH = 65536; // vertices per trip: 256 whole chunks
    const size_t stage_bytes = (size_t)(std::min<uint64_t>(CH, std::max<uint64_t>(n, 1)) * (16 + K3) + 256 * 72);
    PinnedBuf<unsigned char> h_stage[2]; // (an early exit frees them under copies still in flight: both frees wait for the device)
    DevBuf<unsigned char> d_stage[2];
    DevBuf<float> d_table;
    Event done[2];
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(hipHostMalloc(h_stage[k].out(), stage_bytes, hipHostMallocDefault));
        HIP_TRY(hipMalloc(d_stage[k].out(), stage_bytes));
        HIP_TRY(hipEventCreateWithFlags(done[k].out(), hipEventDisableTiming));
    }
    HIP_TRY(hipMalloc(d_table.out(), 256 * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(d_table, gs_pack_logits(), 256 * sizeof(float), hipMemcpyHostToDevice, c->stream)); // the table as data
    auto section = [&](uint64_t at, void* to, size_t bytes) {
        return !bytes || (fseek(fp, (long)at, SEEK_SET) == 0 && fread(to, 1, bytes, fp) == bytes);
    };
    uint32_t it = 0;
    for (uint64_t v0 = 0; v0 < n; v0 += CH, ++it) {
        const int k = (int)(it & 1u);
        const uint64_t m = std::min<uint64_t>(CH, n - v0), cm = gs_pack_chunks(m);
        const size_t chunk_at = (size_t)m * 16, sh_at = chunk_at + (size_t)cm * 72, bytes = sh_at + (size_t)(m * K3);
        if (it >= 2) HIP_TRY(hipEventSynchronize(done[k])); // the copy out of this staging buffer two trips ago has finished
        unsigned char* h = h_stage[k];
        if (!section(L.vertex_off + v0 * 16, h, (size_t)m * 16) || !section(L.chunk_off + (v0 / 256) * 72, h + chunk_at, (size_t)cm * 72) ||
            !section(L.sh_off + v0 * K3, h + sh_at, (size_t)(m * K3)))
            return fail(GS_ERR_INVALID_ARGUMENT, "%s: short read", who);
        HIP_TRY(hipMemcpyAsync(d_stage[k], h, bytes, hipMemcpyHostToDevice, c->stream));
        const unsigned char* d = d_stage[k];
        const GsPackTrip trip{(const uint4*)d, (const float*)(d + chunk_at), K ? d + sh_at : nullptr, d_table, (uint32_t)m, (uint32_t)K};
        gs_launch_pack_decode(trip, (uint32_t)(first + v0), dst, c->stream);
        HIP_TRY(hipEventRecord(done[k], c->stream));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

GS_EXPORT int32_t gs_upload_packed(gs_ctx* c, const char* path, uint64_t* n_out) {
    if (!c || !path) return fail(GS_ERR_INVALID_ARGUMENT, "gs_upload_packed: null argument");
    PackSource src;
    int32_t rc = pack_open("gs_upload_packed", path, &src);
    if (rc != GS_OK) return rc;
    const uint64_t n = src.L.n;
    hipError_t he = hipSetDevice(c->cfg.device);
    if (he != hipSuccess) return fail(GS_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(he));
    drop_shadows(c);
    rc = scene_alloc(c, n);
    if (rc != GS_OK) return rc;
    rc = pack_stream("gs_upload_packed", c, src, c->scene, 0);
    if (rc != GS_OK) return rc;
    if (n_out) *n_out = n;
    return GS_OK;
}
