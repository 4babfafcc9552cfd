// gs_readback.hip -- what the host reads of the last frame: buffer taps and read-backs, statistics, per-pixel queries, and
// the assembly of slabs into one image.  Part of the C ABI (include/gsplat/gs_abi.h).  Everything here refers to the ring
// member that rendered the LAST frame (last_of) and reads what that frame left in its FrameNotes.
#include <cstddef>

#include "gs_runtime.h"
#include "gs_tight.h"

// A tight frame's lists name record slots and its records lie in slot order (k_preprocess.hip).  The taps keep their documented
// contents -- gaussian ids in the values, records at 64 * gaussian index -- in buffers rebuilt from the frame once, on demand.
static int32_t tight_tap(gs_ctx* c, bool want_gdata) {
    if (want_gdata ? c->gdataG_valid : c->valsG_valid) return GS_OK;
    if (c->pending) { int32_t rc = wait_one(c); if (rc != GS_OK) return rc; }
    const uint64_t I = std::min<uint64_t>(c->h_rep->num_intersections, c->capacity); // (of the frame waited for)
    const GsLists L = frame_lists(c);
    const size_t gbytes = std::max<size_t>((size_t)c->n * 64, 256);
    if (want_gdata) {
        if (!c->gdataG) HIP_TRY(hipMalloc(c->gdataG.out(), gbytes));
        HIP_TRY(hipMemsetAsync(c->gdataG, 0, gbytes, c->stream)); // gaussians without a record: all-zero
    } else if (!c->valsG) HIP_TRY(hipMalloc(c->valsG.out(), (size_t)c->capacity * 4));
    gs_launch_rows_rebuild_taps(L.values, L.gdata, L.nrec, (uint32_t)I, c->n, want_gdata ? nullptr : c->valsG.get(),
                                want_gdata ? c->gdataG.get() : nullptr, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    (want_gdata ? c->gdataG_valid : c->valsG_valid) = true;
    return GS_OK;
}

static int32_t tap(gs_ctx* c, int32_t which, void** ptr, uint64_t* bytes) {
    const FrameNotes& nt = c->notes;
    const uint64_t I = std::min<uint64_t>(c->h_rep->num_intersections, c->capacity);
    const uint64_t px = (uint64_t)c->frame.slab_w * c->frame.height;
    switch (which) {
    // (device words of a tight frame: the count plane of the projection's entries, not indexed by the gaussian -- gs_read_buffer
    // derives that frame's tile counts from its lists)
    case GS_BUF_TILE_COUNTS: *ptr = c->counts; *bytes = (uint64_t)c->n * 4; return GS_OK;
    case GS_BUF_TILE_OFFSETS:
        if (!c->last_debug) return fail(GS_ERR_NO_FRAME, "the offsets tap needs gs_render_debug (index-order scan)");
        *ptr = c->offsets; *bytes = (uint64_t)c->n * 4; return GS_OK;
    case GS_BUF_GAUSSIAN_DATA:
        *bytes = (uint64_t)c->n * 64;
        if (!nt.last_tight) { *ptr = c->gdata; return GS_OK; } // (word 2 of a record holds the gaussian's id: gs_read_buffer clears it)
        if (const int32_t rc = tight_tap(c, true); rc != GS_OK) return rc;
        *ptr = c->gdataG;
        return GS_OK;
    case GS_BUF_KEYS_UNSORTED:
    case GS_BUF_VALUES_UNSORTED:
        if (!c->last_debug || !c->keysU) return fail(GS_ERR_NO_FRAME, "unsorted taps need gs_render_debug");
        *ptr = which == GS_BUF_KEYS_UNSORTED ? c->keysU.get() : c->valsU.get(); *bytes = I * 4; return GS_OK;
    case GS_BUF_KEYS:
        *bytes = I * 4;
        if (!nt.last_keys16 && !nt.last_tight) { *ptr = nt.keysS; return GS_OK; }
        if (!c->keysG_valid) { // the frame never held full keys (16-bit tile ids, or no keys at all on the tight row pipeline): rebuild tile*1000 + bucket once
            if (c->pending) { int32_t rc = wait_one(c); if (rc != GS_OK) return rc; }
            if (!c->keysG) HIP_TRY(hipMalloc(c->keysG.out(), (size_t)c->capacity * 4));
            if (nt.last_tight) gs_launch_rows_rebuild_keys(c->ranges, c->T, nt.valsS, c->gdata, c->n + GS_RECORD_SLACK, (uint32_t)I, c->n, c->keysG, c->stream);
            else gs_launch_rebuild_keys((const uint16_t*)nt.keysS, nt.valsS, c->counts, (uint32_t)I, c->n, c->keysG, c->stream);
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->keysG_valid = true;
        }
        *ptr = c->keysG;
        return GS_OK;
    case GS_BUF_VALUES:
    case GS_BUF_BLOCK_MASKS: // tight frames: id | mask << 28 (gs_read_buffer separates them), rebuilt from the frame's slot | mask << 28
        *bytes = I * 4;
        if (!nt.last_tight) { *ptr = nt.valsS; return GS_OK; }
        if (const int32_t rc = tight_tap(c, false); rc != GS_OK) return rc;
        *ptr = c->valsG;
        return GS_OK;
    case GS_BUF_RANGES: *ptr = c->ranges; *bytes = (uint64_t)c->T * 4; return GS_OK;
    case GS_BUF_RGBA8: *ptr = c->last_ext ? c->last_ext : (void*)c->rgba8.get(); *bytes = px * 4; return GS_OK;
    case 12: // TESTS ONLY: the resident scene arrays as one block (position planes, largest log-scale, geometry, SH records)
        *ptr = c->scene_mem; *bytes = c->scene_bytes; return GS_OK;
    case 11: // PROFILING ONLY: per-walker stamps of the blend (GS_OPT_BLEND_ABLATION bit 16)
        if (!c->blend_prof) return fail(GS_ERR_INVALID_ARGUMENT, "no blend profile (GS_OPT_BLEND_ABLATION bit 16)");
        *ptr = c->blend_prof; *bytes = (uint64_t)c->blend_prof_blocks * 16; return GS_OK;
    case GS_BUF_RGB_F32:
        if (!c->rgbf) return fail(GS_ERR_INVALID_ARGUMENT, "GS_BUF_RGB_F32 needs GS_FLAG_F32_TAP");
        *ptr = c->rgbf; *bytes = px * 12; return GS_OK;
    case GS_BUF_ALPHA_F32:
    case GS_BUF_DEPTH_F32:
        if (!c->alpha || !c->depth)
            return fail(GS_ERR_INVALID_ARGUMENT, "%s needs GS_FLAG_AUX_OUTPUTS", which == GS_BUF_ALPHA_F32 ? "GS_BUF_ALPHA_F32" : "GS_BUF_DEPTH_F32");
        *ptr = which == GS_BUF_ALPHA_F32 ? c->alpha.get() : c->depth.get(); *bytes = px * 4; return GS_OK;
    default: return fail(GS_ERR_INVALID_ARGUMENT, "unknown buffer id %d", which);
    }
}

// GS_BUF_SPLAT_STATE: the plane as it is now -- of the scene, not of a frame (every ring member views the same one).
static int32_t state_tap(gs_ctx* c, void** ptr, uint64_t* bytes) {
    if (!has_state(c)) return fail(GS_ERR_INVALID_ARGUMENT, "GS_BUF_SPLAT_STATE needs GS_FLAG_SPLAT_STATE");
    if (!c->scene_mem || !c->scene.state) return fail(GS_ERR_NO_SCENE, "GS_BUF_SPLAT_STATE: no splats uploaded");
    *ptr = const_cast<uint8_t*>(c->scene.state);
    *bytes = c->n;
    return GS_OK;
}

int32_t last_frame(gs_ctx* root, const char* who, gs_ctx** out) {
    gs_ctx* c = last_of(root);
    if (who && !c->have_frame) return fail(GS_ERR_NO_FRAME, "%s: no frame rendered", who);
    if (c->pending) { int32_t rc = wait_one(c); if (rc != GS_OK) return rc; } // (an overflowed frame has been re-rendered from full lists)
    HIP_TRY(hipSetDevice(c->cfg.device));
    *out = c;
    return GS_OK;
}

// The size protocol of a read, for both kinds of tap: report the size; copy (*copy) only into a destination that is given, and
// refuse one that is too small.
static int32_t size_protocol(uint64_t bytes, const void* dst, uint64_t size, uint64_t* written, bool* copy) {
    if (written) *written = bytes;
    *copy = dst != nullptr;
    if (dst && size < bytes) return fail(GS_ERR_INVALID_ARGUMENT, "gs_read_buffer: need %llu bytes, got %llu", (unsigned long long)bytes, (unsigned long long)size);
    return GS_OK;
}

GS_EXPORT int32_t gs_read_buffer(gs_ctx* c, int32_t which, void* dst, uint64_t size, uint64_t* written) {
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_read_buffer: null ctx");
    void* p = nullptr;
    uint64_t bytes = 0;
    bool copy = false;
    if (which == GS_BUF_SPLAT_STATE) { // (state calls return when done: the plane is at rest; frames in flight only read it)
        int32_t rc = state_tap(c, &p, &bytes);
        if (rc == GS_OK) rc = size_protocol(bytes, dst, size, written, &copy);
        if (rc != GS_OK || !copy) return rc;
        HIP_TRY(hipSetDevice(c->cfg.device));
        if (bytes) HIP_TRY(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
        return GS_OK;
    }
    { int32_t rc = last_frame(c, "gs_read_buffer", &c); if (rc != GS_OK) return rc; }
    const GsLists L = frame_lists(c);
    const bool tight = c->notes.last_tight;
    const uint64_t I = std::min<uint64_t>(c->h_rep->num_intersections, c->capacity);
    // two buffers are made on the host, not copied: the block masks of a frame with the reference's binning (the blend tests every
    // block of the tile itself), and the tile counts of a tight frame (its count words hold row-item slots, k_preprocess.hip:
    // the tile counts of the tap are those of its lists)
    const bool all_masks = which == GS_BUF_BLOCK_MASKS && !tight, list_counts = which == GS_BUF_TILE_COUNTS && tight;
    if (all_masks) bytes = I * 4;
    else if (list_counts) bytes = (uint64_t)c->n * 4;
    else { int32_t rc = tap(c, which, &p, &bytes); if (rc != GS_OK) return rc; }
    { int32_t rc = size_protocol(bytes, dst, size, written, &copy); if (rc != GS_OK || !copy) return rc; }
    uint32_t* w = (uint32_t*)dst;
    if (all_masks) {
        const uint32_t nb = (c->frame.tile_size / 8) * (c->frame.tile_size / 8);
        const uint32_t all = nb >= 32 ? 0xFFFFFFFFu : (1u << nb) - 1u;
        for (uint64_t i = 0; i < bytes / 4; ++i) w[i] = all;
        return GS_OK;
    }
    if (list_counts) {
        std::vector<uint32_t> v(I);
        uint64_t vbytes = 0;
        { int32_t rc = tap(c, GS_BUF_VALUES, &p, &vbytes); if (rc != GS_OK) return rc; } // (gaussian ids: the frame's own values name record slots)
        if (I) HIP_TRY(hipMemcpy(v.data(), p, I * 4, hipMemcpyDeviceToHost));
        memset(w, 0, bytes);
        for (uint64_t i = 0; i < I; ++i) { const uint32_t g = v[i] & L.id_mask; if (g < c->n) w[g]++; }
        return GS_OK;
    }
    if (bytes) HIP_TRY(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
    if (which == GS_BUF_TILE_COUNTS) // device words also carry the depth bucket in their high 10 bits
        for (uint64_t i = 0; i < bytes / 4; ++i) w[i] &= GS_COUNT_MASK;
    if (which == GS_BUF_GAUSSIAN_DATA && !tight) // the record's id word: padding in the reference's record (a tight frame's copy has it cleared)
        for (uint64_t i = 0; i < bytes / 64; ++i) w[i * 16 + 2] = 0u;
    if (which == GS_BUF_VALUES && L.id_mask != 0xFFFFFFFFu) // strip what rides above the id
        for (uint64_t i = 0; i < bytes / 4; ++i) w[i] &= L.id_mask;
    if (which == GS_BUF_BLOCK_MASKS) { // tight frame: the mask's sub-blocks (tile/2, or the whole 8-pixel tile) as 8x8-block bits
        const uint32_t ts = c->frame.tile_size;
        for (uint64_t i = 0; i < bytes / 4; ++i) {
            const uint32_t m = w[i] >> GS_ID_BITS;
            uint32_t out = m & (ts == 8 ? 1u : 0xFu);
            if (ts == 32) { // quadrant q = (by/2)*2 + bx/2 of block (bx, by), 4 blocks per row
                out = 0;
                for (uint32_t by = 0; by < 4; ++by)
                    for (uint32_t bx = 0; bx < 4; ++bx)
                        if ((m >> ((by / 2) * 2 + bx / 2)) & 1u) out |= 1u << (by * 4 + bx);
            }
            w[i] = out;
        }
    }
    return GS_OK;
}

GS_EXPORT int32_t gs_read_rgba8(gs_ctx* c, void* dst, uint64_t size) {
    if (!dst) return fail(GS_ERR_INVALID_ARGUMENT, "gs_read_rgba8: null destination");
    return gs_read_buffer(c, GS_BUF_RGBA8, dst, size, nullptr);
}

GS_EXPORT int32_t gs_device_ptr(gs_ctx* c, int32_t which, void** d_ptr) {
    if (!c || !d_ptr) return fail(GS_ERR_INVALID_ARGUMENT, "gs_device_ptr: null argument");
    uint64_t bytes = 0;
    if (which == GS_BUF_SPLAT_STATE) return state_tap(c, d_ptr, &bytes);
    c = last_of(c);
    if (which == GS_BUF_RGBA8) { *d_ptr = c->rgba8; return GS_OK; }
    if (!c->have_frame) return fail(GS_ERR_NO_FRAME, "gs_device_ptr: no frame rendered");
    return tap(c, which, d_ptr, &bytes);
}

// GS_FLAG_TIMING: the stages of the last frame and their means over the frames since GS_OPT_RESET_TIMING (at most the event
// ring's), from the member's per-frame event brackets.
static void stage_times(const gs_ctx* c, gs_stats* out) {
    if (!c->have_events || c->frames == 0) return;
    const uint64_t last = c->frames - 1;
    uint64_t first = c->timed_from;
    if (last + 1 > GS_EV_RING && first < last + 1 - GS_EV_RING) first = last + 1 - GS_EV_RING;
    if (first > last) first = last;
    double sum[GS_STAGE_COUNT + 1] = {0};
    uint32_t cnt = 0;
    for (uint64_t fr = first; fr <= last; ++fr) {
        const Event* e = c->ev[fr % GS_EV_RING];
        float ms = 0, tot = 0;
        bool ok = true;
        float st[GS_STAGE_COUNT];
        for (int i = 0; i < GS_STAGE_COUNT && ok; ++i) {
            ok = hipEventElapsedTime(&ms, e[i], e[i + 1]) == hipSuccess;
            st[i] = ms * 1000.0f;
        }
        ok = ok && hipEventElapsedTime(&tot, e[0], e[GS_STAGE_COUNT]) == hipSuccess;
        if (!ok) continue;
        for (int i = 0; i < GS_STAGE_COUNT; ++i) sum[i] += st[i];
        sum[GS_STAGE_COUNT] += tot * 1000.0f;
        ++cnt;
        if (fr == last) {
            for (int i = 0; i < GS_STAGE_COUNT; ++i) out->stage_us[i] = st[i];
            out->frame_us = tot * 1000.0f;
        }
    }
    out->frames_timed = cnt;
    if (cnt) {
        for (int i = 0; i < GS_STAGE_COUNT; ++i) out->stage_us_mean[i] = (float)(sum[i] / cnt);
        out->frame_us_mean = (float)(sum[GS_STAGE_COUNT] / cnt);
    }
}

GS_EXPORT int32_t gs_get_stats(gs_ctx* root, gs_stats* out) {
    if (!root || !out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_get_stats: null argument");
    gs_ctx* c = nullptr; // everything below describes the context that rendered the last frame ...
    { int32_t rc = last_frame(root, nullptr, &c); if (rc != GS_OK) return rc; }
    const FrameNotes& nt = c->notes;
    memset(out, 0, sizeof(*out));
    out->num_gaussians = c->n;
    out->num_tiles = c->T;
    out->sort_passes = nt.last_passes ? nt.last_passes : c->passes;
    out->frames = over_ring(root, [](const gs_ctx* m) { return m->frames; }); // ... except the counters that are sums over the ring
    out->depth_ordered = (c->have_frame && !nt.last_by_index) ? 1u : 0u;
    if (c->have_frame) {
        if (!c->h_ctl_valid) { // the blend's counters live in the control block: fetched when somebody asks
            HIP_TRY(hipMemcpy(c->h_ctl, c->ctl, offsetof(GsControl, hist), hipMemcpyDeviceToHost));
            c->h_ctl_valid = true;
        }
        out->num_visible = c->h_rep->num_visible;
        out->num_intersections = c->h_rep->num_intersections;
        out->capacity = c->capacity;
        out->max_intersections_seen = std::max<uint64_t>(over_ring(root, [](const gs_ctx* m) { return m->max_I_seen; }, true), c->h_rep->num_intersections);
        out->truncated_frames = over_ring(root, [](const gs_ctx* m) { return m->truncated_frames; });
        out->frames_in_flight = (uint32_t)root->shadows.size() + 1u;
        out->graph_frames = over_ring(root, [](const gs_ctx* m) { return m->gr.frames; });
        out->tight_binning = nt.last_tight ? 1u : 0u;
        out->row_capacity = c->row_cap;
        if (nt.last_tight) {
            out->num_row_items = c->h_rep->num_items;
            out->num_row_slots = c->h_rep->num_slots;
        }
        for (int k = 0; k < 64; ++k) out->num_processed += c->h_ctl->num_processed[k];
        if (nt.blend_walkers >= 4) { // 8x8-block walkers (4 per 16-tile, 16 per 32-tile): sum over tiles of the deepest walker
            std::vector<uint32_t> depth(c->T);
            if (hipMemcpy(depth.data(), c->tile_depth, (size_t)c->T * 4, hipMemcpyDeviceToHost) == hipSuccess)
                for (uint32_t v : depth) out->num_processed += v;
        }
        for (int k = 0; k < 64; ++k) out->num_evaluated += c->h_ctl->num_evaluated[k];
        stage_times(c, out);
    }
    return GS_OK;
}

// Per-pixel splat queries on the last frame (k_pick.hip).  Not a frame: nothing of the frame state, the statistics or a
// captured graph is touched; the kernel is one more launch on the stream of the ring member that rendered the last frame.
GS_EXPORT int32_t gs_pick(gs_ctx* root, const gs_pick_query* queries, uint32_t n, gs_pick_result* results, uint32_t max_contrib,
                          gs_pick_contrib* contrib) {
    static_assert(sizeof(gs_pick_query) == 8 && sizeof(gs_pick_result) == 48 && sizeof(gs_pick_contrib) == 8, "gs_pick record layouts");
    if (!root || !queries || !results) return fail(GS_ERR_INVALID_ARGUMENT, "gs_pick: null argument");
    if (n == 0 || n > GS_PICK_MAX_QUERIES) return fail(GS_ERR_INVALID_ARGUMENT, "gs_pick: n must be 1..%u (got %u)", GS_PICK_MAX_QUERIES, n);
    if (max_contrib > GS_PICK_MAX_CONTRIB) return fail(GS_ERR_INVALID_ARGUMENT, "gs_pick: max_contrib must be at most %u (got %u)", GS_PICK_MAX_CONTRIB, max_contrib);
    if ((contrib != nullptr) != (max_contrib != 0))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_pick: contrib and max_contrib must be given together (contrib %s, max_contrib %u)",
                    contrib ? "set" : "null", max_contrib);
    for (uint32_t i = 0; i < n; ++i)
        if (queries[i].x >= root->frame.width || queries[i].y >= root->frame.height)
            return fail(GS_ERR_INVALID_ARGUMENT, "gs_pick: query %u: pixel (%u, %u) is outside the %u x %u canvas", i, queries[i].x, queries[i].y,
                        root->frame.width, root->frame.height);
    gs_ctx* c = nullptr;
    int32_t rc = last_frame(root, "gs_pick", &c);
    if (rc != GS_OK) return rc;
    auto& pk = root->pick;
    if (!pk.q) HIP_TRY(hipMalloc(pk.q.out(), (size_t)GS_PICK_MAX_QUERIES * sizeof(gs_pick_query)));
    if (!pk.r) HIP_TRY(hipMalloc(pk.r.out(), (size_t)GS_PICK_MAX_QUERIES * sizeof(gs_pick_result)));
    const uint64_t cbytes = (uint64_t)n * max_contrib * sizeof(gs_pick_contrib);
    rc = pk.c.reserve(cbytes);
    if (rc != GS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(pk.q, queries, (size_t)n * sizeof(gs_pick_query), hipMemcpyHostToDevice, c->stream));
    gs_launch_pick(frame_lists(c), pk.q, n, pk.r, max_contrib, max_contrib ? pk.c.get() : nullptr, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(results, pk.r, (size_t)n * sizeof(gs_pick_result), hipMemcpyDeviceToHost, c->stream));
    if (max_contrib) HIP_TRY(hipMemcpyAsync(contrib, pk.c, (size_t)cbytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

GS_EXPORT int32_t gs_assemble_slabs(gs_ctx* c, const void* d_slabs, const uint32_t* col_bounds, uint32_t n_slabs,
                                    uint64_t slab_stride_bytes, void* d_image) {
    if (!c || !d_slabs || !col_bounds || !d_image || n_slabs == 0 || n_slabs > 64)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_assemble_slabs: bad argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    uint32_t pxb[65];
    for (uint32_t g = 0; g <= n_slabs; ++g) pxb[g] = std::min(c->frame.width, col_bounds[g] * c->frame.tile_size);
    if (pxb[0] != 0 || pxb[n_slabs] != c->frame.width) return fail(GS_ERR_INVALID_ARGUMENT, "gs_assemble_slabs: bounds must cover the canvas");
    if (c->pxb_n != n_slabs || memcmp(c->pxb_host, pxb, (n_slabs + 1) * 4) != 0) {
        // boundaries change rarely: upload them once (synchronously), not every frame
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(c->d_pxb, pxb, (n_slabs + 1) * 4, hipMemcpyHostToDevice));
        memcpy(c->pxb_host, pxb, (n_slabs + 1) * 4);
        c->pxb_n = n_slabs;
    }
    gs_launch_assemble(d_slabs, d_image, c->frame.width, c->frame.height, c->d_pxb, n_slabs, slab_stride_bytes / 4, c->stream);
    HIP_TRY(hipGetLastError());
    return GS_OK;
}
