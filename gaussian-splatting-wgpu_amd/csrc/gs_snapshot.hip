// gs_snapshot.hip -- the entry points of snapshots and write-back: records scattered into the resident planes by index, and
// device-resident copies of a selection's parts that restore or swap in place.  Part of the C ABI (include/gsplat/gs_abi.h
// "snapshots and write-back"); the kernels are in k_snapshot.hip.
//
// The reference has no counterpart: its host keeps the PackedGaussians buffer it uploaded (renderer.ts:130-137), edits that and
// uploads it again.  Here gs_export_splats brings records out of the device planes; these calls are its inverse, so that an edit of
// a handful of splats, or the undo of a transform or a grade, costs what it touches and not an upload of the scene, which also
// drops the last frame, the shadows, a captured graph and every per-splat plane.
//
// Every call on a context drains its ring first (resident_drain), runs on the context's stream and returns when done, as
// gs_transform_splats does.  None is a frame or an upload: nothing of the frame state, the shadows, the capacities, the statistics,
// a captured graph or the coverage, neighbour and cluster planes is touched.  Every refusal is decided before anything is written.
#include <memory>
#include <new>

#include "gs_runtime.h"

static constexpr uint32_t kAllParts = GS_PART_RECORD | GS_PART_STATE;

// What the five calls on a context refuse after their own arguments and before the ring is drained: a null context, a context that
// borrows its scene, the resident calls' refusals (resident_check with the filter, when there is one) and GS_PART_STATE without
// the plane.
static int32_t snap_check(gs_ctx* c, const char* who, const char* verb, uint32_t parts, bool filtered = false, uint32_t mask = 0, uint32_t value = 0) {
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null ctx", who);
    if (c->scene_mem && c->scene_mem != c->scene_own.get())
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: this context borrows its splats (gs_share_splats): %s the owner", who, verb);
    const int32_t rc = resident_check(c, who, filtered ? Plane::filtered : Plane::none, mask, value);
    if (rc != GS_OK) return rc;
    if ((parts & GS_PART_STATE) && !has_state(c))
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: the context was created without GS_FLAG_SPLAT_STATE (GS_PART_STATE needs the plane)", who);
    return GS_OK;
}
static int32_t parts_check(const char* who, uint32_t parts) {
    if (parts & ~kAllParts) return fail(GS_ERR_INVALID_ARGUMENT, "%s: unknown part bits 0x%x", who, parts & ~kAllParts);
    return GS_OK;
}

// ---- write-back ---------------------------------------------------------------------------------------------------------------
// ids[p] against its predecessor (p > 0) and N: the refusal's message, or GS_OK
static int32_t id_check(const char* who, uint64_t p, bool have_prev, uint32_t prev, uint32_t id, uint32_t n) {
    if (id >= n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: ids[%llu] = %u is not a splat (N = %u)", who, (unsigned long long)p, id, n);
    if (have_prev && prev >= id)
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: ids[%llu] = %u does not exceed ids[%llu] = %u: the ids must be strictly ascending", who,
                    (unsigned long long)p, id, (unsigned long long)(p - 1), prev);
    return GS_OK;
}
// The host's list, before anything is copied.
static int32_t ids_check_host(const char* who, const uint32_t* ids, uint64_t m, uint32_t n) {
    for (uint64_t p = 0; p < m; ++p) {
        const int32_t rc = id_check(who, p, p > 0, p > 0 ? ids[p - 1] : 0u, ids[p], n);
        if (rc != GS_OK) return rc;
    }
    return GS_OK;
}
// The device's list: one small kernel takes the atomicMin of the first offending position into the state calls' counter word,
// which is read back before the scatter is launched.
static int32_t ids_check_device(gs_ctx* c, const char* who, const uint32_t* d_ids, uint64_t m) {
    unsigned long long bad = ~0ull;
    HIP_TRY(hipMemsetAsync(c->st.counter, 0xFF, sizeof(bad), c->stream));
    gs_launch_ids_ascending(d_ids, m, c->n, c->st.counter, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, c->st.counter, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (bad == ~0ull) return GS_OK;
    uint32_t pair[2] = {0u, 0u}; // ids[bad - 1], ids[bad]
    const uint64_t from = bad ? bad - 1 : 0;
    HIP_TRY(hipMemcpy(pair + (bad ? 0 : 1), d_ids + from, bad ? 8 : 4, hipMemcpyDeviceToHost));
    const int32_t rc = id_check(who, bad, bad > 0, pair[0], pair[1], c->n);
    return rc != GS_OK ? rc : fail(GS_ERR_INVALID_ARGUMENT, "%s: ids[%llu] is out of order", who, bad); // (the list changed under the call)
}

static int32_t write_common(gs_ctx* c, const char* who, const uint32_t* ids, uint64_t m, const void* aos, const uint8_t* states, uint32_t parts,
                            uint64_t* written, bool device) {
    int32_t rc = parts_check(who, parts);
    if (rc != GS_OK) return rc;
    if ((parts & GS_PART_RECORD) && !aos && m) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null records", who);
    if ((parts & GS_PART_STATE) && !states && m) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null states (GS_PART_STATE reads one byte per record)", who);
    rc = snap_check(c, who, "write to", parts);
    if (rc != GS_OK) return rc;
    if (m > c->n)
        return fail(GS_ERR_INVALID_ARGUMENT, "%s: m = %llu records, the scene holds %u splats%s", who, (unsigned long long)m, c->n,
                    ids ? " (the ids must be strictly ascending)" : " (ids == NULL writes splats 0 .. m)");
    if (ids && !device) {
        rc = ids_check_host(who, ids, m, c->n);
        if (rc != GS_OK) return rc;
    }
    rc = resident_drain(c, device && ids != nullptr && m != 0);
    if (rc != GS_OK) return rc;
    if (written) *written = 0;
    if (!m || !parts) return GS_OK;
    const bool rec = (parts & GS_PART_RECORD) != 0, st = (parts & GS_PART_STATE) != 0;
    if (device) {
        if (ids) {
            rc = ids_check_device(c, who, ids, m);
            if (rc != GS_OK) return rc;
        }
        gs_launch_write(aos, states, (uint32_t)m, ids, c->scene, c->n, parts, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (written) *written = m;
        return GS_OK;
    }
    // host pointers: through a bounce buffer of one trip's records, ids and state bytes
    const uint64_t trip = std::min(m, kBounceRecords);
    const size_t rec_bytes = rec ? (size_t)trip * GS_SPLAT_RECORD_BYTES : 0, ids_bytes = ids ? (size_t)trip * 4 : 0;
    DevBuf<> bounce;
    HIP_TRY(hipMalloc(bounce.out(), std::max<size_t>(rec_bytes + ids_bytes + (st ? (size_t)trip : 0), 256)));
    char* const d_rec = (char*)bounce.get();
    uint32_t* const d_ids = (uint32_t*)(d_rec + rec_bytes);
    uint8_t* const d_st = (uint8_t*)(d_rec + rec_bytes + ids_bytes);
    for (uint64_t first = 0; first < m; first += kBounceRecords) {
        const uint64_t k = std::min(kBounceRecords, m - first);
        if (rec) HIP_TRY(hipMemcpyAsync(d_rec, (const char*)aos + first * GS_SPLAT_RECORD_BYTES, (size_t)k * GS_SPLAT_RECORD_BYTES, hipMemcpyHostToDevice, c->stream));
        if (ids) HIP_TRY(hipMemcpyAsync(d_ids, ids + first, (size_t)k * 4, hipMemcpyHostToDevice, c->stream));
        if (st) HIP_TRY(hipMemcpyAsync(d_st, states + first, (size_t)k, hipMemcpyHostToDevice, c->stream));
        // (ids == NULL: record first + g goes to splat first + g: the planes' views are moved instead of a list being made)
        GsScene s = c->scene;
        uint32_t n = c->n;
        if (!ids) {
            s.px += first; s.py += first; s.pz += first; s.smax += first; s.geo += 2 * first; s.sh += 12 * first;
            if (s.state) s.state += first; // (first is a multiple of 2^20: whole words)
            n -= (uint32_t)first;
        }
        gs_launch_write(d_rec, d_st, (uint32_t)k, ids ? d_ids : nullptr, s, n, parts, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream)); // before the next trip overwrites the bounce buffer
    }
    if (written) *written = m;
    return GS_OK;
}

GS_EXPORT int32_t gs_write_splats(gs_ctx* c, const uint32_t* ids, uint64_t m, const void* aos320, const uint8_t* states, uint32_t parts, uint64_t* written) {
    return write_common(c, "gs_write_splats", ids, m, aos320, states, parts, written, false);
}
GS_EXPORT int32_t gs_write_splats_device(gs_ctx* c, const uint32_t* d_ids, uint64_t m, const void* d_aos320, const uint8_t* d_states, uint32_t parts,
                                         uint64_t* written) {
    return write_common(c, "gs_write_splats_device", d_ids, m, d_aos320, d_states, parts, written, true);
}

// ---- snapshots ------------------------------------------------------------------------------------------------------------------
// One device allocation, compact SoA, every section a multiple of 16 bytes: the id list (absent when dense), 3 x f32[m4] positions,
// float4[m][2] geometry, float4[m][12] SH, u8[m4] state; m4 = m rounded up to 4.  Only the parts taken have a section.
struct gs_snapshot {
    int device = 0;
    uint64_t serial = 0; // the scene_serial of the context it was taken from
    uint64_t count = 0, n_at_take = 0;
    uint32_t parts = 0;
    bool dense = false;
    size_t bytes = 0;
    DevBuf<> mem;
    GsSnapshotDev dev{};
};
// the sections behind `base` (null: only the size means anything); returns the bytes of the whole
static size_t snapshot_layout(char* base, uint64_t m, uint32_t parts, bool dense, GsSnapshotDev* d) {
    const size_t m4 = ((size_t)m + 3) & ~(size_t)3;
    size_t off = 0;
    *d = GsSnapshotDev{};
    if (!dense) { d->ids = (const uint32_t*)(base + off); off += m4 * 4; }
    if (parts & GS_PART_POSITION) {
        d->x = (float*)(base + off); off += m4 * 4;
        d->y = (float*)(base + off); off += m4 * 4;
        d->z = (float*)(base + off); off += m4 * 4;
    }
    if (parts & GS_PART_GEOMETRY) { d->geo = (float4*)(base + off); off += (size_t)m * 32; }
    if (parts & GS_PART_SH) { d->sh = (float4*)(base + off); off += (size_t)m * 192; }
    if (parts & GS_PART_STATE) { d->state = (uint32_t*)(base + off); off += m4; }
    return off;
}

GS_EXPORT int32_t gs_snapshot_take(gs_ctx* c, uint32_t mask, uint32_t value, uint32_t parts, gs_snapshot** out) {
    static const char who[] = "gs_snapshot_take";
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null out", who);
    int32_t rc = parts_check(who, parts);
    if (rc != GS_OK) return rc;
    rc = snap_check(c, who, "snapshot", parts, true, mask, value);
    if (rc != GS_OK) return rc;
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    const bool all = !(mask | value); // every splat: no selection runs, the snapshot is dense and keeps no id list
    uint64_t total = c->n;
    if (!all) {
        rc = edit_select(c, mask, value, true, &total);
        if (rc != GS_OK) return rc;
    }
    std::unique_ptr<gs_snapshot> s(new (std::nothrow) gs_snapshot);
    if (!s) return fail(GS_ERR_OUT_OF_MEMORY, "%s: out of host memory", who);
    s->device = c->cfg.device;
    s->serial = c->scene_serial;
    s->count = total;
    s->n_at_take = c->n;
    s->parts = parts;
    s->dense = all;
    GsSnapshotDev d;
    s->bytes = total ? snapshot_layout(nullptr, total, parts, all, &d) : 0;
    if (s->bytes) {
        HIP_TRY(hipMalloc(s->mem.out(), s->bytes));
        snapshot_layout((char*)s->mem.get(), total, parts, all, &s->dev);
        if (!all) HIP_TRY(hipMemcpyAsync(const_cast<uint32_t*>(s->dev.ids), c->ex.ids, (size_t)total * 4, hipMemcpyDeviceToDevice, c->stream));
        gs_launch_snapshot(0u, c->scene, c->n, s->dev, (uint32_t)total, parts, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *out = s.release();
    return GS_OK;
}

static int32_t apply_common(gs_ctx* c, const gs_snapshot* s, uint32_t parts, uint64_t* moved, uint32_t mode, const char* who) {
    if (!s) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null snapshot", who);
    int32_t rc = parts_check(who, parts);
    if (rc != GS_OK) return rc;
    if (!parts) parts = s->parts; // all that were taken
    if (parts & ~s->parts) return fail(GS_ERR_INVALID_ARGUMENT, "%s: part bits 0x%x were not taken (the snapshot holds 0x%x)", who, parts & ~s->parts, s->parts);
    rc = snap_check(c, who, mode == 1u ? "restore" : "swap with", parts);
    if (rc != GS_OK) return rc;
    if (c->scene_serial != s->serial)
        return fail(GS_ERR_INVALID_ARGUMENT,
                    "%s: the snapshot was taken from scene serial %llu, the context holds serial %llu: the scene was replaced or renumbered "
                    "(another context, an upload or a compaction since)",
                    who, (unsigned long long)s->serial, (unsigned long long)c->scene_serial);
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    const bool work = s->count && parts;
    if (work) {
        gs_launch_snapshot(mode, c->scene, c->n, s->dev, (uint32_t)s->count, parts, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (moved) *moved = work ? s->count : 0;
    return GS_OK;
}
GS_EXPORT int32_t gs_snapshot_restore(gs_ctx* c, const gs_snapshot* s, uint32_t parts, uint64_t* restored) {
    return apply_common(c, s, parts, restored, 1u, "gs_snapshot_restore");
}
GS_EXPORT int32_t gs_snapshot_swap(gs_ctx* c, gs_snapshot* s, uint32_t parts, uint64_t* swapped) {
    return apply_common(c, s, parts, swapped, 2u, "gs_snapshot_swap");
}

GS_EXPORT int32_t gs_snapshot_get_info(const gs_snapshot* s, gs_snapshot_info* out) {
    if (!s) return fail(GS_ERR_INVALID_ARGUMENT, "gs_snapshot_get_info: null snapshot");
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_snapshot_get_info: null out");
    out->count = s->count;
    out->n_at_take = s->n_at_take;
    out->device_bytes = s->bytes;
    out->parts = s->parts;
    out->dense = s->dense ? 1u : 0u;
    return GS_OK;
}

GS_EXPORT int32_t gs_snapshot_free(gs_snapshot* s) {
    if (!s) return GS_OK;
    if (s->mem) (void)hipSetDevice(s->device); // (the memory is the snapshot's own: the context may be long gone)
    delete s;
    return GS_OK;
}
