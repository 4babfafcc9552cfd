// gs_export.hip -- the splat edits' entry points: list, export, compact and save resident splats by state.  Part of the C ABI
// (include/gsplat/gs_abi.h "splat edits"); the kernels are in k_export.hip.
//
// The reference has no counterpart: its host keeps the PackedGaussians buffer it uploaded (renderer.ts:130-137) and would filter
// and upload that again.  Here the scene may have been streamed from a file (gs_upload_ply) without any host copy, so the records
// come back out of the device planes: a stable stream compaction over the state plane picks them, the inverse of the upload's
// repack rebuilds the 320-byte records, and a plane-to-plane gather makes a deletion permanent.
//
// Every call drains the context's ring first (gs_wait), runs on the context's stream and returns when done, as gs_state_* do.
// None of them launches anything in a frame: a context that never calls them launches exactly what it did before.
#include "gs_file_writer.h"
#include "gs_runtime.h"

// What every entry point does first (gs_runtime.h): the refusals, a filter that needs the plane among them, and the drain of the ring.
static int32_t edit_begin(gs_ctx* c, const char* who, uint32_t mask, uint32_t value) { return resident_begin(c, who, Plane::filtered, mask, value); }

// Counts the matching splats (count + scan launches, the total read back like the state calls' counter); with want_ids also
// writes their indices, ascending, to c->ex.ids.
int32_t edit_select(gs_ctx* c, uint32_t mask, uint32_t value, bool want_ids, uint64_t* total) {
    const uint32_t nb = gs_select_blocks(c->n);
    int32_t rc = c->ex.counts.reserve((uint64_t)nb + 1);
    if (rc != GS_OK) return rc;
    gs_launch_select_count(c->scene.state, c->n, mask, value, c->ex.counts, c->stream);
    HIP_TRY(hipGetLastError());
    uint32_t t = 0;
    HIP_TRY(hipMemcpyAsync(&t, c->ex.counts.get() + nb, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *total = t;
    if (!want_ids || !t) return GS_OK;
    rc = c->ex.ids.reserve(t);
    if (rc != GS_OK) return rc;
    gs_launch_select_scatter(c->scene.state, c->n, mask, value, c->ex.counts, c->ex.ids, t, c->stream);
    HIP_TRY(hipGetLastError());
    return GS_OK;
}

GS_EXPORT int32_t gs_state_list(gs_ctx* c, uint32_t mask, uint32_t value, uint32_t* ids, uint64_t cap, uint64_t* n) {
    int32_t rc = edit_begin(c, "gs_state_list", mask, value);
    if (rc != GS_OK) return rc;
    if (!n) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_list: null n");
    uint64_t total = 0;
    rc = edit_select(c, mask, value, ids != nullptr, &total); // (the list is built in the context's scratch: a refusal writes nothing to ids)
    if (rc != GS_OK) return rc;
    *n = total;
    if (!ids) return GS_OK;
    if (cap < total) return fail(GS_ERR_INVALID_ARGUMENT, "gs_state_list: %llu ids needed, the buffer holds %llu", (unsigned long long)total, (unsigned long long)cap);
    if (total) HIP_TRY(hipMemcpyAsync(ids, c->ex.ids, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

static int32_t export_common(gs_ctx* c, const char* who, uint32_t mask, uint32_t value, void* out, uint64_t cap, uint64_t* n, uint32_t* ids_out,
                             bool device) {
    int32_t rc = edit_begin(c, who, mask, value);
    if (rc != GS_OK) return rc;
    if (!n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null n", who);
    const bool all = !(mask | value); // every splat, in place: no selection runs and the unpack reads splat g for record g
    uint64_t total = c->n;
    if (!all) {
        rc = edit_select(c, mask, value, out != nullptr, &total);
        if (rc != GS_OK) return rc;
    }
    *n = total;
    if (!out) return GS_OK;
    if (cap < total) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %llu records needed, the buffer holds %llu", who, (unsigned long long)total, (unsigned long long)cap);
    const uint32_t* sel = all ? nullptr : c->ex.ids.get();
    if (device) {
        gs_launch_unpack(c->scene, c->n, sel, 0, (uint32_t)total, out, ids_out, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
        return GS_OK;
    }
    DevBuf<> bounce; // the records as the caller wants them, one trip at a time
    HIP_TRY(hipMalloc(bounce.out(), std::max<size_t>((size_t)std::min(total, kBounceRecords) * GS_SPLAT_RECORD_BYTES, 256)));
    for (uint64_t first = 0; first < total; first += kBounceRecords) {
        const uint64_t m = std::min(kBounceRecords, total - first);
        gs_launch_unpack(c->scene, c->n, sel, (uint32_t)first, (uint32_t)m, bounce, nullptr, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync((char*)out + first * GS_SPLAT_RECORD_BYTES, bounce, (size_t)m * GS_SPLAT_RECORD_BYTES, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream)); // before the next trip overwrites the bounce buffer
    }
    if (ids_out) {
        if (all) for (uint64_t i = 0; i < total; ++i) ids_out[i] = (uint32_t)i;
        else if (total) HIP_TRY(hipMemcpy(ids_out, c->ex.ids, (size_t)total * 4, hipMemcpyDeviceToHost));
    }
    return GS_OK;
}

GS_EXPORT int32_t gs_export_splats(gs_ctx* c, uint32_t mask, uint32_t value, void* aos320, uint64_t cap_records, uint64_t* n, uint32_t* ids) {
    return export_common(c, "gs_export_splats", mask, value, aos320, cap_records, n, ids, false);
}
GS_EXPORT int32_t gs_export_splats_device(gs_ctx* c, uint32_t mask, uint32_t value, void* d_aos320, uint64_t cap_records, uint64_t* n,
                                          uint32_t* d_ids) {
    return export_common(c, "gs_export_splats_device", mask, value, d_aos320, cap_records, n, d_ids, true);
}

GS_EXPORT int32_t gs_compact(gs_ctx* c, uint32_t mask, uint32_t value, uint64_t* kept, uint32_t* ids) {
    int32_t rc = edit_begin(c, "gs_compact", mask, value);
    if (rc != GS_OK) return rc;
    if (c->scene_mem != c->scene_own.get())
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_compact: this context borrows its splats (gs_share_splats): compact the owner");
    uint64_t total = 0;
    rc = edit_select(c, mask, value, true, &total); // (0, 0) and kept == N take this path too: no special case
    if (rc != GS_OK) return rc;
    if (ids && total) HIP_TRY(hipMemcpyAsync(ids, c->ex.ids, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // like an upload from here on: the shadows borrow the old planes and hold arrays sized for the old N
    drop_shadows(c);
    DevBuf<> old_mem = std::move(c->scene_own); // moved aside before scene_alloc resets the owner; freed after the gather
    const GsScene old = c->scene;
    const uint32_t n_old = c->n;
    rc = scene_alloc(c, total, c->capacity, c->row_cap);
    if (rc != GS_OK) { // (as after an upload that failed: the context holds no scene)
        c->scene_own.reset();
        c->scene_mem = nullptr;
        c->scene = GsScene{};
        c->n = c->frame.n = 0;
        return rc;
    }
    gs_launch_compact_planes(old, n_old, c->ex.ids, (uint32_t)total, c->scene, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (kept) *kept = total;
    return GS_OK;
}

// ---- the .ply writer: gs_ply_load's inverse ---------------------------------------------------------------------------------
// One vertex is 17 + 3K floats, K = (degree + 1)^2 - 1: x y z, three normals (+0), f_dc_0..2, f_rest_{cK+i} = record float
// 16 + 4 (i + 1) + c, opacity, scale_0..2, rot_0..3 -- what PackedGaussians reads back (ply.ts:166-198).  Words, not floats: a
// NaN's payload goes through untouched.
static void ply_rows(const uint32_t* rec, uint64_t m, int K, uint32_t* out) {
    for (uint64_t i = 0; i < m; ++i, rec += 80) {
        *out++ = rec[0]; *out++ = rec[1]; *out++ = rec[2];
        *out++ = 0u; *out++ = 0u; *out++ = 0u;
        *out++ = rec[16]; *out++ = rec[17]; *out++ = rec[18];
        for (int ch = 0; ch < 3; ++ch)
            for (int k = 0; k < K; ++k) *out++ = rec[16 + 4 * (k + 1) + ch];
        *out++ = rec[12];
        *out++ = rec[4]; *out++ = rec[5]; *out++ = rec[6];
        *out++ = rec[8]; *out++ = rec[9]; *out++ = rec[10]; *out++ = rec[11];
    }
}
static std::string ply_header(uint64_t n, int K) {
    std::string h = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(n) + "\n";
    auto prop = [&](const std::string& name) { h += "property float " + name + "\n"; };
    for (const char* nm : {"x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"}) prop(nm);
    for (int k = 0; k < 3 * K; ++k) prop("f_rest_" + std::to_string(k));
    for (const char* nm : {"opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"}) prop(nm);
    return h + "end_header\n";
}
static constexpr uint64_t kPlyChunk = kStreamTrip; // records per trip, as a streamed upload

GS_EXPORT int32_t gs_ply_save(const char* path, const void* records, uint64_t n, int32_t sh_degree) {
    if (!path) return fail(GS_ERR_INVALID_ARGUMENT, "gs_ply_save: null path");
    if (!records && n) return fail(GS_ERR_INVALID_ARGUMENT, "gs_ply_save: null records (%s)", path);
    if (sh_degree < 0 || sh_degree > 3) return fail(GS_ERR_INVALID_ARGUMENT, "gs_ply_save: sh_degree %d is not 0..3 (%s)", sh_degree, path);
    const int K = (sh_degree + 1) * (sh_degree + 1) - 1;
    const size_t row = 17 + 3 * (size_t)K;
    FileWriter w("gs_ply_save", path);
    int32_t rc = w.open(ply_header(n, K));
    if (rc != GS_OK) return rc;
    std::vector<uint32_t> rows((size_t)std::min<uint64_t>(std::max<uint64_t>(n, 1), kPlyChunk) * row);
    for (uint64_t first = 0; first < n; first += kPlyChunk) {
        const uint64_t m = std::min(kPlyChunk, n - first);
        ply_rows((const uint32_t*)records + first * 80, m, K, rows.data());
        rc = w.write(rows.data(), (size_t)m * row * 4);
        if (rc != GS_OK) return rc;
    }
    return w.finish();
}

// gs_upload_ply's mirror image: the unpack kernel fills a device staging buffer with at most 64 Ki records, the buffer is copied
// to one of the ring's two pinned host buffers, and the host turns the PREVIOUS chunk into vertices and writes it while that copy
// runs (TripRing::drain, gs_runtime.h).  Peak host memory is the two pinned buffers (2 x 20 MB) and one chunk of vertices, whatever
// the size of the scene.
GS_EXPORT int32_t gs_export_ply(gs_ctx* c, const char* path, uint32_t mask, uint32_t value, int32_t sh_degree, uint64_t* n_out) {
    int32_t rc = edit_begin(c, "gs_export_ply", mask, value);
    if (rc != GS_OK) return rc;
    if (!path) return fail(GS_ERR_INVALID_ARGUMENT, "gs_export_ply: null path");
    if (sh_degree < 0 || sh_degree > 3) return fail(GS_ERR_INVALID_ARGUMENT, "gs_export_ply: sh_degree %d is not 0..3 (%s)", sh_degree, path);
    const bool all = !(mask | value);
    uint64_t total = c->n;
    if (!all) {
        rc = edit_select(c, mask, value, true, &total);
        if (rc != GS_OK) return rc;
    }
    const uint32_t* sel = all ? nullptr : c->ex.ids.get();
    const int K = (sh_degree + 1) * (sh_degree + 1) - 1;
    const size_t row = 17 + 3 * (size_t)K;
    const size_t chunk_bytes = (size_t)kPlyChunk * GS_SPLAT_RECORD_BYTES;
    FileWriter w("gs_export_ply", path);
    rc = w.open(ply_header(total, K));
    if (rc != GS_OK) return rc;
    DevBuf<> d_stage; // one: the unpack of a chunk waits, in stream order, for the copy of the chunk before it out of this buffer
    TripRing ring;
    HIP_TRY(hipMalloc(d_stage.out(), chunk_bytes));
    rc = ring.init(chunk_bytes, false);
    if (rc != GS_OK) return rc;
    std::vector<uint32_t> rows((size_t)kPlyChunk * row);
    auto records = [&](uint64_t it) { return std::min(kPlyChunk, total - it * kPlyChunk); };
    rc = ring.drain((total + kPlyChunk - 1) / kPlyChunk, c->stream,
                    [&](uint64_t it, unsigned char* h) {
                        gs_launch_unpack(c->scene, c->n, sel, (uint32_t)(it * kPlyChunk), (uint32_t)records(it), d_stage, nullptr, c->stream);
                        HIP_TRY(hipGetLastError());
                        HIP_TRY(hipMemcpyAsync(h, d_stage, (size_t)records(it) * GS_SPLAT_RECORD_BYTES, hipMemcpyDeviceToHost, c->stream));
                        return (int32_t)GS_OK;
                    },
                    [&](uint64_t it, unsigned char* h) {
                        ply_rows((const uint32_t*)h, records(it), K, rows.data());
                        return w.write(rows.data(), (size_t)records(it) * row * 4);
                    });
    if (rc != GS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    rc = w.finish();
    if (rc != GS_OK) return rc;
    if (n_out) *n_out = total;
    return GS_OK;
}
