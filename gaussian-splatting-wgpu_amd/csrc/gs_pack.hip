// gs_pack.hip -- the packed scenes' entry points: the host codec's forwards, the export of resident splats into the 16-byte chunked
// format, the upload of such a file and the file as a source (PackSource; gs_append_packed is with the other insertions in
// gs_insert.hip: it shares their refusals and their install).  Part of the C ABI (include/gsplat/gs_abi.h "packed scenes"); the
// kernels are in k_pack.hip, the codec in gs_pack_math.h, the file's header, writer and loader in gs_pack_host.hip.
//
// The reference has no counterpart: its only container is the float .ply (ply.ts:49-228), 248 bytes per splat at degree 3, and for a
// scene streamed in from a file that file is the only host copy there would ever be.  An export here encodes the whole selection on
// the device (at most 61 bytes per splat of scratch beside the scene) and streams the three sections to the file; an upload reads the
// file in trips of whole chunks and decodes on the device.  Both go through the one trip ring (TripRing, gs_runtime.h): neither
// holds the scene on the host.
//
// Every resident call drains the context's ring first (resident_begin), runs on the context's stream and returns when done.  None
// of them launches anything in a frame: a context that never calls them launches exactly what it did before.
#include "gs_file_writer.h"
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
// (neigh_bounds under the selection's filter on both sides), the keys, the pair sort behind a private control block (private_sort,
// gs_runtime.h; four 8-bit passes: the keys reach 1 << 30).  *out: the sorted values, in the neighbourhoods' scratch.
static int32_t morton_order(gs_ctx* c, const char* who, uint32_t mask, uint32_t value, const uint32_t* sel, uint32_t m, const uint32_t** out) {
    gs_ctx::Neigh& s = c->ng;
    if (m >= (1u << 30)) return fail(GS_ERR_CAPACITY, "%s: %u splats, the Morton sort takes fewer than 2^30", who, m);
    uint32_t hb[16];
    int32_t rc = neigh_bounds(c, (mask | value) ? c->scene.state : nullptr, mask, value, mask, value, hb);
    if (rc != GS_OK) return rc;
    GsPackBox box{};
    if (hb[7]) // (no splat with finite coordinates: every key is GS_PACK_KEY_LAST, the box is not read)
        for (int k = 0; k < 3; ++k) { box.lo[k] = pk_okey_value(hb[k]); box.hi[k] = pk_okey_value(hb[3 + k]); }
    GsSortPair sorted;
    rc = private_sort(c, m, 4, [&] { gs_launch_pack_keys(c->scene, c->n, sel, m, box, s.keysA, s.valsA, c->stream); }, &sorted);
    if (rc != GS_OK) return rc;
    HIP_TRY(hipGetLastError());
    uint32_t fault = 0;
    rc = private_sort_fault(c, &fault);
    if (rc != GS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (fault) return fail(GS_ERR_DEVICE_FAULT, "%s: look-back spin bound exceeded in the Morton sort", who);
    *out = sorted.vals;
    return GS_OK;
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
    FileWriter w(who, path);
    rc = w.open(header);
    if (rc != GS_OK) return rc;
    // the three sections go to the file in trips of 1 MiB (65 536 vertices), the host writing one trip while the next is being copied
    constexpr size_t kTrip = (size_t)1 << 20;
    TripRing ring;
    rc = ring.init(std::max<size_t>(std::min(std::max<size_t>({(size_t)C * 72, (size_t)m * 16, (size_t)m * 3 * K}), kTrip), 256), false);
    if (rc != GS_OK) return rc;
    auto section = [&](size_t from, size_t bytes) {
        auto part = [&](uint64_t it) { return std::min(kTrip, bytes - (size_t)it * kTrip); };
        return ring.drain((bytes + kTrip - 1) / kTrip, c->stream,
                          [&](uint64_t it, unsigned char* h) {
                              HIP_TRY(hipMemcpyAsync(h, enc.get() + from + (size_t)it * kTrip, part(it), hipMemcpyDeviceToHost, c->stream));
                              return (int32_t)GS_OK;
                          },
                          [&](uint64_t it, unsigned char* h) { return w.write(h, part(it)); });
    };
    if ((rc = section(chunk_at, (size_t)C * 72)) != GS_OK || (rc = section(vert_at, (size_t)m * 16)) != GS_OK ||
        (rc = section(sh_at, (size_t)m * 3 * K)) != GS_OK)
        return rc;
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

// ---- upload: the packed file as a source (gs_runtime.h), shared with gs_append_packed ------------------------------------------------
int32_t PackSource::open(const char* who, const char* path) {
    fp = File(fopen(path, "rb"));
    if (!fp) return fail(GS_ERR_INVALID_ARGUMENT, "%s: cannot open %s", who, path);
    unsigned char head[8192];
    const size_t got = fread(head, 1, sizeof(head), fp);
    if (fseek(fp, 0, SEEK_END) != 0) return fail(GS_ERR_INVALID_ARGUMENT, "%s: cannot seek in %s", who, path);
    const long fsize = ftell(fp);
    char err[480] = "";
    const int32_t rc = gs_pack_parse_header(who, path, head, got, (uint64_t)(fsize < 0 ? 0 : fsize), &L, err, sizeof(err));
    return rc == GS_OK ? rc : fail(rc, "%s", err);
}

// A trip is its vertices, their whole chunks' records and their SH bytes, read from the file's three sections into one staging buffer.
int32_t PackSource::stream(const char* who, gs_ctx* c, const GsScene& dst, uint64_t first) {
    const uint64_t n = L.n, K = (uint64_t)gs_pack_rest(L.degree), K3 = 3 * K;
    TripRing ring;
    int32_t rc = ring.init((size_t)(std::min(kStreamTrip, std::max<uint64_t>(n, 1)) * (16 + K3) + 256 * 72), true);
    if (rc != GS_OK) return rc;
    DevBuf<float> d_table;
    HIP_TRY(hipMalloc(d_table.out(), 256 * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(d_table, gs_pack_logits(), 256 * sizeof(float), hipMemcpyHostToDevice, c->stream)); // the table as data
    auto section = [&](uint64_t at, void* to, size_t bytes) {
        return !bytes || (fseek(fp, (long)at, SEEK_SET) == 0 && fread(to, 1, bytes, fp) == bytes);
    };
    rc = ring.feed((n + kStreamTrip - 1) / kStreamTrip, c->stream, [&](uint64_t it, unsigned char* h, unsigned char* d) {
        const uint64_t v0 = it * kStreamTrip, m = std::min(kStreamTrip, n - v0), cm = gs_pack_chunks(m);
        const size_t chunk_at = (size_t)m * 16, sh_at = chunk_at + (size_t)cm * 72, bytes = sh_at + (size_t)(m * K3);
        if (!section(L.vertex_off + v0 * 16, h, (size_t)m * 16) || !section(L.chunk_off + (v0 / 256) * 72, h + chunk_at, (size_t)cm * 72) ||
            !section(L.sh_off + v0 * K3, h + sh_at, (size_t)(m * K3)))
            return fail(GS_ERR_INVALID_ARGUMENT, "%s: short read", who);
        HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
        const GsPackTrip trip{(const uint4*)d, (const float*)(d + chunk_at), K ? d + sh_at : nullptr, d_table, (uint32_t)m, (uint32_t)K};
        gs_launch_pack_decode(trip, (uint32_t)(first + v0), dst, c->stream);
        return (int32_t)GS_OK;
    });
    if (rc != GS_OK) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

GS_EXPORT int32_t gs_upload_packed(gs_ctx* c, const char* path, uint64_t* n_out) {
    return upload_source<PackSource>("gs_upload_packed", c, path, n_out);
}
