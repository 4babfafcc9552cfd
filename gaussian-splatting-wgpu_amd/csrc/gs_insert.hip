// gs_insert.hip -- the splat insertion's entry points: append records, a .ply or a copy of a selection to the resident splats.  Part
// of the C ABI (include/gsplat/gs_abi.h "splat insertion"); the grow pass is in k_insert.hip, the tails are the upload's kernels
// with a destination offset (k_preprocess.hip) and the compaction's gather (k_export.hip).
//
// The reference has no counterpart: its host keeps the PackedGaussians buffer it uploaded (renderer.ts:130-137) and would
// concatenate and upload that again.  Here the scene may have been streamed from a file (gs_upload_ply) without any host copy, so
// the only other way to a second capture in the same context is gs_export_splats of everything, a host concatenation and a new
// upload.  gs_compact's mirror image: a new scene of another N is built from the old one on the device.
//
// Every call drains the context's ring first (resident_begin), runs on the context's stream and returns when done, as the splat
// edits do.  Atomic: every refusal is decided before anything is allocated or freed; the new scene is then built BESIDE the old
// one (scene_layout: the one copy of the layout arithmetic) and installed only when its tail is complete, so a HIP error or a short
// read on the way leaves the context with the old scene exactly as it was.  None of them launches anything in a frame: a context
// that never calls them launches exactly what it did before.
#include "gs_runtime.h"

// What every entry point refuses before it drains the ring.  new_state_check comes first, before the call's own pointers and the
// context are looked at (it needs neither); insert_check: the resident calls' refusals (resident_check) with the duplicate's filter,
// a non-zero new_state without the plane, and a context that borrows its scene; insert_fits: N + m below 2^31.
static int32_t new_state_check(const char* who, uint32_t new_state) {
    if (new_state > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "%s: new_state 0x%x does not fit the state byte", who, new_state);
    return GS_OK;
}
static int32_t insert_check(gs_ctx* c, const char* who, uint32_t new_state, uint32_t mask = 0, uint32_t value = 0) {
    const int32_t rc = resident_check(c, who, Plane::filtered, mask, value);
    if (rc != GS_OK) return rc;
    if (new_state && !has_state(c)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: the context was created without GS_FLAG_SPLAT_STATE (new_state must be 0)", who);
    if (c->scene_mem != c->scene_own.get())
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: this context borrows its splats (gs_share_splats): insert into the owner", who);
    return GS_OK;
}
static int32_t insert_fits(const gs_ctx* c, const char* who, uint64_t m) {
    if (m >= (1ull << 31) || (uint64_t)c->n + m >= (1ull << 31))
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: %u resident + %llu new splats reach the limit of 2^31", who, c->n, (unsigned long long)m);
    return GS_OK;
}

// The common part, m > 0 and every refusal behind: allocates the scene of N + m splats beside the old one, runs the grow pass and
// fill(new scene), which enqueues (or runs) what writes splats N .. N + m of the geometry planes, and installs the result the way
// gs_compact does: shadows dropped, the captured graph invalidated, the per-gaussian work arrays re-sized, the (key,value) and row
// capacities kept.  An error before the install leaves the context untouched (the new allocation goes with `mem`).
template <class Fill>
static int32_t insert_grow(gs_ctx* c, uint64_t m, uint32_t new_state, Fill fill) {
    const uint32_t n_old = c->n;
    const uint64_t n_new = (uint64_t)n_old + m;
    const bool state = has_state(c);
    DevBuf<> mem;
    HIP_TRY(hipMalloc(mem.out(), std::max<size_t>(scene_layout(nullptr, n_new, state).bytes, 256)));
    const GsScene dst = scene_layout(mem.get(), n_new, state).scene;
    gs_launch_grow(c->scene, n_old, dst, (uint32_t)n_new, new_state, c->opt.grid_persist * 2u, c->stream);
    HIP_TRY(hipGetLastError());
    int32_t rc = fill(dst);
    if (rc != GS_OK) return rc; // (mem is freed under what may still run: the free waits for the device)
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    // like a compaction from here on: the shadows borrow the old planes and hold arrays sized for the old N
    drop_shadows(c);
    rc = scene_install(c, std::move(mem), n_new, c->capacity, c->row_cap);
    if (rc != GS_OK) return rc; // (the work arrays could not be re-sized: as after an upload that failed, the context holds no scene)
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

static int32_t append_common(gs_ctx* c, const char* who, const void* aos, uint64_t m, uint32_t new_state, uint64_t* first, bool device) {
    int32_t rc = new_state_check(who, new_state);
    if (rc != GS_OK) return rc;
    if (!aos && m) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null records", who);
    rc = insert_check(c, who, new_state);
    if (rc != GS_OK) return rc;
    rc = insert_fits(c, who, m);
    if (rc != GS_OK) return rc;
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    const uint32_t n_old = c->n;
    if (m) {
        DevBuf<> bounce; // host records: the tail as the caller holds it (320 B x m beside the two scenes)
        const void* d_aos = aos;
        if (!device) {
            HIP_TRY(hipMalloc(bounce.out(), (size_t)m * GS_SPLAT_RECORD_BYTES));
            hipError_t e = hipMemcpy(bounce, aos, (size_t)m * GS_SPLAT_RECORD_BYTES, hipMemcpyHostToDevice);
            if (e != hipSuccess) return fail(GS_ERR_HIP, "%s: memcpy: %s", who, hipGetErrorString(e));
            d_aos = bounce;
        }
        rc = insert_grow(c, m, new_state, [&](const GsScene& dst) {
            gs_launch_repack(d_aos, (uint32_t)m, n_old, dst, c->stream);
            return (int32_t)GS_OK;
        }); // (synchronises the stream before the bounce buffer goes)
        if (rc != GS_OK) return rc;
    }
    if (first) *first = n_old;
    return GS_OK;
}

GS_EXPORT int32_t gs_append_splats(gs_ctx* c, const void* aos320, uint64_t m, uint32_t new_state, uint64_t* first) {
    return append_common(c, "gs_append_splats", aos320, m, new_state, first, false);
}
GS_EXPORT int32_t gs_append_splats_device(gs_ctx* c, const void* d_aos320, uint64_t m, uint32_t new_state, uint64_t* first) {
    return append_common(c, "gs_append_splats_device", d_aos320, m, new_state, first, true);
}

// A file behind the resident splats, over either source (PlySource, PackSource: gs_runtime.h).  The refusals in this order: new_state,
// a null path, insert_check, what the source's open refuses, insert_fits; then the drain.
template <class Source>
static int32_t append_source(const char* who, gs_ctx* c, const char* path, uint32_t new_state, uint64_t* first, uint64_t* m_out) {
    int32_t rc = new_state_check(who, new_state);
    if (rc != GS_OK) return rc;
    if (!path) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null path", who);
    rc = insert_check(c, who, new_state);
    if (rc != GS_OK) return rc;
    Source src;
    rc = src.open(who, path);
    if (rc != GS_OK) return rc;
    const uint64_t m = src.count();
    rc = insert_fits(c, who, m);
    if (rc != GS_OK) return rc;
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    const uint32_t n_old = c->n;
    if (m) {
        rc = insert_grow(c, m, new_state, [&](const GsScene& dst) { return src.stream(who, c, dst, n_old); });
        if (rc != GS_OK) return rc;
    }
    if (first) *first = n_old;
    if (m_out) *m_out = m;
    return GS_OK;
}
GS_EXPORT int32_t gs_append_ply(gs_ctx* c, const char* path, uint32_t new_state, uint64_t* first, uint64_t* m_out) {
    return append_source<PlySource>("gs_append_ply", c, path, new_state, first, m_out);
}
GS_EXPORT int32_t gs_append_packed(gs_ctx* c, const char* path, uint32_t new_state, uint64_t* first, uint64_t* m_out) {
    return append_source<PackSource>("gs_append_packed", c, path, new_state, first, m_out);
}

GS_EXPORT int32_t gs_duplicate_splats(gs_ctx* c, uint32_t mask, uint32_t value, uint32_t new_state, uint64_t* first, uint64_t* m_out,
                                      uint32_t* ids) {
    static const char who[] = "gs_duplicate_splats";
    int32_t rc = new_state_check(who, new_state);
    if (rc != GS_OK) return rc;
    rc = insert_check(c, who, new_state, mask, value);
    if (rc != GS_OK) return rc;
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    const uint32_t n_old = c->n;
    uint64_t m = 0;
    rc = edit_select(c, mask, value, true, &m); // (0, 0) takes this path too: every index, ascending
    if (rc != GS_OK) return rc;
    rc = insert_fits(c, who, m);
    if (rc != GS_OK) return rc;
    if (m) {
        rc = insert_grow(c, m, new_state, [&](const GsScene& dst) {
            gs_launch_compact_planes(c->scene, n_old, c->ex.ids, (uint32_t)m, dst, c->stream, n_old, false);
            return (int32_t)GS_OK;
        });
        if (rc != GS_OK) return rc;
        if (ids) HIP_TRY(hipMemcpy(ids, c->ex.ids, (size_t)m * 4, hipMemcpyDeviceToHost)); // (the selection's scratch outlives the scene)
    }
    if (first) *first = n_old;
    if (m_out) *m_out = m;
    return GS_OK;
}
