// gs_frame.hip -- frame sequencing: the launches of one frame, the frame graph, waiting and regrowth, the ring of frames in
// flight, tickets.  Part of the C ABI (include/gsplat/gs_abi.h).
//
// Replaces the frame orchestration of Renderer (reference src/renderer.ts:349-593 animate) and the host halves of
// ExclusiveScanner (src/exclusive_scan.ts:208-325) and GPUSorter (src/radix_sort/sort.ts:249-350).  Where the reference blocks on
// the queue 8 times per frame and reads I back to the CPU, this runtime enqueues one frame as ~10 kernels + 1 small memset on
// one HIP stream with no host synchronisation: I stays in device memory and grids are persistent (ticket loops).
#include <dlfcn.h>

#include "gs_runtime.h"
#include "gs_tight.h"

// roctx ranges named after the reference's stages (renderer.ts:406,421,467,477,501,546), opened around the launches of each
// stage when GS_FLAG_TIMING is set, so a rocprofv3 --marker-trace lines up with the reference's own console.log timings.
// The library is looked up at run time: no link dependency, silently absent when the profiler SDK is not installed.
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        void* h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_LAZY | RTLD_LOCAL);
        if (!h) h = dlopen("libroctx64.so.4", RTLD_LAZY | RTLD_LOCAL);
        if (h) {
            push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
            pop = (int (*)())dlsym(h, "roctxRangePop");
            if (!push || !pop) push = nullptr, pop = nullptr;
        }
    }
};
Roctx& roctx() { static Roctx r; return r; }
const char* const kStageRange[] = {"gsplat:process_gaussians", "gsplat:exclusive_scan", "gsplat:write_tile_ids", "gsplat:radix_sort",
                                   "gsplat:compute_ranges", "gsplat:compute_tiles"};
}

static inline void mark(gs_ctx* c, int i) { // stage boundary i: closes stage i-1, opens stage i
    if (!c->have_events) return;
    hipEventRecord(c->ev[c->frames % GS_EV_RING][i], c->stream);
    Roctx& r = roctx();
    if (r.push) {
        if (i > 0) r.pop();
        if (i < GS_STAGE_COUNT) r.push(kStageRange[i]);
    }
}

static void mark_cb(void* p, int i) { mark((gs_ctx*)p, i); }

GsLists frame_lists(const gs_ctx* c) {
    // (records: a tight frame's slots reach into the slack behind the first n, and its n is below 2^28; any other frame's are its n)
    return GsLists{c->gdata, c->notes.valsS, c->ranges, c->frame, c->notes.last_tight ? GS_ID_MASK : 0xFFFFFFFFu,
                   c->notes.last_tight ? c->n + GS_RECORD_SLACK : c->n};
}

// The projection's launch for this frame, left in c->pre: record_frame launches it, a replay patches the captured node from it.
static void prepare_projection(gs_ctx* c, const GsUniforms& u, bool tight) {
    gs_preprocess_prepare(c->pre, c->scene, u, c->frame, c->gdata, c->counts, tight, c->arena, c->rowptr, c->unit_off, c->unit_n, c->ctl, c->opt.tight_nb,
                          has_state(c), tint_of(c->opt.select_tint));
}

// ---- binning: one function per pipeline, from the first launch after the projection (stage mark 1) to `ranges` (mark 5 follows).
// Each returns the frame's notes: where the sorted lists are and what made them. ------------------------------------------------

// The tight row pipeline (k_rows.hip).  Stage brackets: "scan" = the gaussian-level sort by depth bucket, "emit" = the row sort
// (the row items take write_tile_ids' place), "sort" = count + scan + expansion into the final lists, "ranges" = nothing (they
// fall out of the scan).
// A tight frame's `counts` and `rowptr` hold the projection's ENTRIES (the cull's survivors of every 1024-index unit, dense from
// the unit's start), not a word per gaussian index; a frame of the reference's binning rewrites counts[i] for every i.
static FrameNotes bin_tight(gs_ctx* c) {
    hipStream_t st = c->stream;
    gs_launch_gsort(c->counts, c->rowptr, c->unit_off, c->unit_n, c->n, c->gsort_scratch, c->grec, c->chunk_table,
                    (uint32_t)gs_emit_chunks(std::max(c->capacity, c->row_cap)), &c->ctl->num_visible, &c->ctl->num_slots, c->opt.grid_persist, st);
    mark(c, 2);
    gs_launch_rows(c->arena, c->grec, c->chunk_table, c->rows_sorted, c->ctl, c->rows_status, (uint32_t)c->row_cap, c->M3, c->tileoff, c->rowtot, c->frame,
                   c->valsA, c->ranges, c->opt.grid_persist / 4u, c->sticky, c->h_rep, st, mark_cb, c);
    mark(c, 4);
    return FrameNotes{nullptr, c->valsA, /*passes*/ 1u, /*walkers*/ 1u, /*by_index*/ false, /*keys16*/ false, /*tight*/ true};
}

// What the two reference pipelines share behind their emission into keysA / valsA: the instance sort by `plan`, the ranges.
static FrameNotes sort_to_ranges(gs_ctx* c, const GsSort& plan, bool by_index) {
    hipStream_t st = c->stream;
    mark(c, 3);
    const GsSortPair sorted = gs_launch_sort(plan, c->ctl, c->sort_status, (uint32_t)c->capacity, c->opt.grid_persist, st);
    mark(c, 4);
    const uint32_t grid = c->opt.grid_persist * 2; // streaming: 8 workgroups/CU
    if (plan.keys16) gs_launch_ranges16((const uint16_t*)sorted.keys, c->ctl, (uint32_t)c->capacity, c->T, c->ranges, grid, c->sticky, c->h_rep, st);
    else gs_launch_ranges(sorted.keys, c->ctl, (uint32_t)c->capacity, c->T, c->ranges, grid, c->sticky, c->h_rep, st);
    return FrameNotes{sorted.keys, sorted.vals, plan.passes, /*walkers*/ 1u, by_index, plan.keys16, /*tight*/ false};
}

// The reference's order: scan counts in gaussian order, emit in gaussian order, sort by the full key.  debug: the unsorted arrays
// are copied for their taps, between emission and sort.
static int32_t bin_by_index(gs_ctx* c, bool debug, FrameNotes& nt) {
    hipStream_t st = c->stream;
    gs_launch_scan(c->counts, c->n, c->offsets, c->scan_status, &c->ctl->scan_ticket[0], c->ctl, st);
    mark(c, 2);
    gs_launch_emit(c->gdata, c->counts, c->offsets, c->frame, c->keysA, c->valsA, c->ctl, st);
    if (debug) {
        const size_t kb = (size_t)c->capacity * 4;
        if (!c->keysU) {
            HIP_TRY(hipMalloc(c->keysU.out(), kb));
            HIP_TRY(hipMalloc(c->valsU.out(), kb));
        }
        HIP_TRY(hipMemcpyAsync(c->keysU, c->keysA, kb, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(c->valsU, c->valsA, kb, hipMemcpyDeviceToDevice, st));
    }
    nt = sort_to_ranges(c, c->sort_index, true);
    return GS_OK;
}

// Depth-ordered emission: the key is tile*1000 + bucket, and the required order inside a tile is (bucket, gaussian index).
// Sorting the N_vis visible GAUSSIANS by bucket first (stable, 10 bits, ~16x fewer elements than instances: k_gsort.hip) and
// emitting their instances in that order leaves only the tile id for the stable instance sort: 2 digits of key/1000 instead of
// 3 of the key.  The sorted (key,value) arrays are identical.
static FrameNotes bin_by_depth(gs_ctx* c) {
    gs_launch_gsort(c->counts, nullptr, nullptr, nullptr, c->n, c->gsort_scratch, c->grec, c->chunk_table, (uint32_t)gs_emit_chunks(std::max(c->capacity, c->row_cap)),
                    &c->ctl->num_visible, &c->ctl->num_intersections, c->opt.grid_persist, c->stream);
    mark(c, 2);
    gs_launch_emit_balanced(c->gdata, c->grec, c->chunk_table, c->frame, c->keysA, c->valsA, c->ctl, c->opt.grid_persist * 2, c->tile_bits, c->tile_passes,
                            c->tile16, c->stream);
    return sort_to_ranges(c, c->sort_tile, false);
}

// Every launch of one frame, in order, on the context's stream (directly, or into a stream capture): zero, projection, binning,
// blend.  index_order: what a frame of the reference's binning emits in (enqueue_frame decides; a debug frame always does).
static int32_t record_frame(gs_ctx* c, const GsUniforms& u, bool debug, void* ext_rgba8, bool tight, bool index_order) {
    hipStream_t st = c->stream;
    const GsOptions& o = c->opt;
    gs_launch_zero(c->ctl_mem, tight ? c->ctl_bytes_tight : c->ctl_bytes, st); // (every part is a multiple of 256 bytes)
    c->h_ctl_valid = false;
    if (debug) HIP_TRY(hipMemsetAsync(c->gdata, 0, std::max<size_t>((size_t)c->n * 64, 256), st));
    mark(c, 0);
    prepare_projection(c, u, tight);
    gs_launch_preprocess(c->pre, st);
    mark(c, 1);
    FrameNotes& nt = c->notes;
    if (tight) nt = bin_tight(c);
    else if (!debug && !index_order) nt = bin_by_depth(c);
    else if (const int32_t rc = bin_by_index(c, debug, nt); rc != GS_OK) return rc;
    mark(c, 5);
    uint32_t* target = ext_rgba8 ? (uint32_t*)ext_rgba8 : c->rgba8.get();
    const bool prof = (o.blend_ablation & 0x10000u) != 0;
    if (prof && !c->blend_prof) HIP_TRY(hipMalloc(c->blend_prof.out(), (size_t)(1u << 20) * 16));
    const bool aux = (c->cfg.flags & GS_FLAG_AUX_OUTPUTS) != 0; // the planes go to the context's own buffers, also under gs_render_to
    const int walkers = gs_launch_blend(frame_lists(c), target, c->rgbf, aux, c->alpha, c->depth, c->ctl, c->tile_depth, (c->cfg.flags & GS_FLAG_EXACT_BLEND) != 0,
                                        o.blend_ablation & 0xFFFFu, st, prof ? c->blend_prof.get() : nullptr, &c->blend_prof_blocks);
    if (walkers == -2) return fail(GS_ERR_INVALID_ARGUMENT, "blend: GS_FLAG_AUX_OUTPUTS without its alpha / depth planes");
    if (walkers < 0) return fail(GS_ERR_INVALID_ARGUMENT, "unsupported tile size %u", c->frame.tile_size);
    nt.blend_walkers = (uint32_t)walkers;
    mark(c, 6);
    if (o.debug_view) gs_launch_debug_view(c->ranges, c->frame, o.debug_view, target, st); // developer views, after the timed stages
    return GS_OK; // (no copy back: the frame's report is in host-mapped memory when the stream has drained, gs_device.h GsReport)
}

void drop_graph(gs_ctx* c) {
    if (c->gr.exec) hipGraphExecDestroy(c->gr.exec);
    if (c->gr.graph) hipGraphDestroy(c->gr.graph);
    c->gr.exec = nullptr; c->gr.graph = nullptr; c->gr.pre_node = nullptr;
    c->gr.valid = false;
}

static int32_t enqueue_frame(gs_ctx* c, const GsUniforms& u, bool debug, void* ext_rgba8) {
    hipStream_t st = c->stream;
    bool index_order = (c->opt.emit_order == 1); // the emission order of this frame, where it takes the reference's binning
    if (c->opt.emit_order == 2) {
        // auto: the depth-ordered pipeline saves (passes - tile_passes) full sweeps of the instance arrays and the histogram
        // pass, and costs the gaussian-level counting sort (three small kernels, k_gsort.hip).  Measured at config B: whole
        // canvas (18.5 M instances) 1.42 vs 1.50 ms, one of 8 slabs (1.9-2.6 M) 418-508 vs 455-566 us, one of 4 slabs 586-699 vs
        // 618-743 us per frame; below ~1 M instances both are launch-bound and the same.
        const uint64_t saved = c->passes > c->tile_passes ? c->passes - c->tile_passes : 0;
        index_order = !(c->have_frame && saved * (uint64_t)c->h_rep->num_intersections >= 1000000ull);
    }
    // tight (opacity-aware) binning: product frames only; the sub-block mask shares the value word with the record slot, and the
    // largest slot the projection can hand out is below n + GS_RECORD_SLACK
    const bool tight = !debug && c->opt.tile_cull && c->tight_ok && (uint64_t)c->n + GS_RECORD_SLACK <= (1ull << GS_ID_BITS);
    // GS_OPT_FRAME_GRAPH: replay the captured frame instead of issuing its ~16 commands one by one (frames without per-stage
    // events or profiler output only).  The capture holds every buffer address and launch geometry of the frame, so anything
    // that moves a buffer or changes an option drops it (gr.valid); the emission order and the output address are part
    // of its identity (GraphKey).
    const bool graphable = c->opt.frame_graph && !debug && !c->have_events && !(c->opt.blend_ablation & 0x10000u) && c->n;
    if (graphable) {
        const GraphKey key{index_order, tight, ext_rgba8, c->alpha, c->depth};
        if (!c->gr.exec || !c->gr.valid || !(c->gr.key == key)) {
            if (c->gr.exec) HIP_TRY(hipStreamSynchronize(st)); // a replay of the old capture may still be running: not destroyed under it
            drop_graph(c);
            HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
            const int32_t rc = record_frame(c, u, debug, ext_rgba8, tight, index_order);
            const hipError_t e = hipStreamEndCapture(st, &c->gr.graph); // (held by the context at once: drop_graph destroys it)
            if (rc != GS_OK) { drop_graph(c); return rc; }
            if (e != hipSuccess || !c->gr.graph) return fail(GS_ERR_HIP, "frame graph capture: %s", hipGetErrorString(e));
            hipGraph_t g = c->gr.graph;
            HIP_TRY(hipGraphInstantiate(&c->gr.exec, g, nullptr, nullptr, 0));
            size_t nn = 0;
            HIP_TRY(hipGraphGetNodes(g, nullptr, &nn));
            std::vector<hipGraphNode_t> nodes(nn);
            HIP_TRY(hipGraphGetNodes(g, nodes.data(), &nn));
            uint32_t found = 0;
            for (hipGraphNode_t nd : nodes) {
                hipGraphNodeType ty;
                if (hipGraphNodeGetType(nd, &ty) != hipSuccess || ty != hipGraphNodeTypeKernel) continue;
                hipKernelNodeParams kp;
                if (hipGraphKernelNodeGetParams(nd, &kp) == hipSuccess && kp.func == c->pre.func) { c->gr.pre_node = nd; ++found; }
            }
            if (found != 1) { // cannot address the projection's node: this frame still runs from the capture, this member's later ones
                c->opt.frame_graph = false; // directly (until the option is set again)
                c->gr.pre_node = nullptr;
            }
            c->gr.key = key;
            c->gr.notes = c->notes;
            c->gr.valid = true;
        } else {
            c->notes = c->gr.notes;
            // (the launch descriptor too: the frame in between prepared it for ITS projection -- other kernel, grid and outputs)
            prepare_projection(c, u, tight);
            hipKernelNodeParams kp{};
            kp.func = const_cast<void*>(c->pre.func);
            kp.gridDim = dim3(c->pre.blocks); kp.blockDim = dim3(256); kp.sharedMemBytes = 0;
            kp.kernelParams = c->pre.args; kp.extra = nullptr;
            HIP_TRY(hipGraphExecKernelNodeSetParams(c->gr.exec, c->gr.pre_node, &kp));
        }
        HIP_TRY(hipGraphLaunch(c->gr.exec, st));
        c->gr.frames++;
    } else {
        const int32_t rc = record_frame(c, u, debug, ext_rgba8, tight, index_order);
        if (rc != GS_OK) return rc;
    }
    c->keysG_valid = c->valsG_valid = c->gdataG_valid = false;
    c->h_ctl_valid = false; // (a replayed frame too: record_frame, which also clears it, only runs for the capture)
    HIP_TRY(hipGetLastError());
    c->pending = true;
    c->have_frame = true;
    c->last_debug = debug;
    c->last_ext = ext_rgba8;
    c->last_u = u;
    c->frames++;
    return GS_OK;
}

static int32_t render_common(gs_ctx* c, const void* uniforms, bool debug, void* ext) {
    if (!c || !uniforms) return fail(GS_ERR_INVALID_ARGUMENT, "gs_render: null argument");
    if (!c->scene_mem) return fail(GS_ERR_NO_SCENE, "gs_render: no splats uploaded");
    HIP_TRY(hipSetDevice(c->cfg.device));
    GsUniforms u;
    static_assert(sizeof(GsUniforms) == GS_UNIFORM_BYTES, "uniform block must be 160 bytes");
    memcpy(&u, uniforms, sizeof(u));
    return enqueue_frame(c, u, debug, ext);
}

int32_t wait_one(gs_ctx* c) {
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_wait: null ctx");
    HIP_TRY(hipSetDevice(c->cfg.device));
    uint32_t dropped = 0; // frames enqueued before the last one that overflowed: their output was truncated and is gone
    const bool fresh = c->pending; // a frame was enqueued since the last wait: what this one finds has not been reported yet
    for (int attempt = 0; attempt < 8; ++attempt) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->pending = false;
        if (!c->have_frame) return GS_OK;
        // the sticky words cover EVERY frame enqueued since the last gs_wait (the control block only the last one)
        const uint32_t over_frames = c->h_rep->sticky[0], fault_any = c->h_rep->sticky[1];
        const uint64_t max_I = c->h_rep->sticky[2], max_rows = c->h_rep->sticky[3];
        if (over_frames || fault_any || max_I || max_rows) HIP_TRY(hipMemset(c->sticky, 0, 4 * 4)); // stream is idle
        c->h_rep->sticky[0] = c->h_rep->sticky[1] = c->h_rep->sticky[2] = c->h_rep->sticky[3] = 0;
        if (max_I > c->max_I_seen) c->max_I_seen = max_I;
        if (fault_any || c->h_rep->fault) return fail(GS_ERR_DEVICE_FAULT, "a look-back spin exceeded its bound (fault word set)");
        const uint64_t I = c->h_rep->num_intersections;
        uint64_t rows_last = 0; // arena slots the last frame asked for: 16 shards as large as its fullest one
        if (c->notes.last_tight)
            for (int k = 0; k < 16; ++k) rows_last = std::max<uint64_t>(rows_last, (uint64_t)c->h_rep->row_cursor[k] * 16);
        const bool last_over = I > c->capacity || c->h_rep->overflow;
        if (attempt == 0 && over_frames > (last_over ? 1u : 0u)) dropped = over_frames - (last_over ? 1u : 0u);
        const uint64_t need = std::max<uint64_t>(I, max_I), need_rows = std::max<uint64_t>(rows_last, max_rows);
        if (!last_over && need <= c->capacity && need_rows <= c->row_cap) break;
        // a frame overflowed the (key,value) capacity or the row-item arena: grow geometrically; re-render the last frame if it was one of them
        // (a refused frame stays the member's last one -- its report still says I > capacity -- until the member renders again: the
        // refusal is reported by the wait that follows the frame, not by every later one)
        if (need >= (1ull << 30)) return fresh ? fail(GS_ERR_CAPACITY, "%llu intersections exceed the 2^30 limit", (unsigned long long)need) : GS_OK;
        uint64_t want = c->capacity, want_rows = c->row_cap;
        if (need > c->capacity) want = std::min<uint64_t>(std::max<uint64_t>(need + need / 4, c->capacity * 2), (1ull << 30) - 1);
        if (need_rows > c->row_cap) want_rows = std::max<uint64_t>(need_rows + need_rows / 4, c->row_cap * 2);
        if (want == c->capacity && want_rows == c->row_cap) { // flagged, yet nothing asks for more: the next attempt would be the same
            if (last_over) return fail(GS_ERR_CAPACITY, "the frame reports an overflow that growing cannot fix (capacity %llu, rows %llu)",
                                       (unsigned long long)c->capacity, (unsigned long long)c->row_cap);
            break;
        }
        int32_t rc = alloc_kv(c, want, want_rows);
        if (rc != GS_OK) return rc;
        if (!last_over) break;
        if (attempt == 7) return fail(GS_ERR_CAPACITY, "capacity did not converge");
        c->frames--; // the re-render reuses the frame's slot in the event ring
        rc = enqueue_frame(c, c->last_u, c->last_debug, c->last_ext);
        if (rc != GS_OK) return rc;
    }
    if (dropped) {
        c->truncated_frames += dropped;
        return fail(GS_ERR_TRUNCATED, "%u frame(s) enqueued before the last one overflowed the (key,value) capacity and were rendered from "
                    "truncated lists; the capacity has been grown to %llu -- wait after every frame, or pass gs_config.max_intersections",
                    dropped, (unsigned long long)c->capacity);
    }
    return GS_OK;
}

GS_EXPORT int32_t gs_wait(gs_ctx* c) {
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_wait: null ctx");
    int32_t first = wait_one(c);
    char msg[sizeof(g_err)];
    if (first != GS_OK) memcpy(msg, g_err, sizeof(msg));
    for (gs_ctx* s : c->shadows) {
        const int32_t rc = wait_one(s);
        if (rc != GS_OK && first == GS_OK) { first = rc; memcpy(msg, g_err, sizeof(msg)); }
    }
    c->cap_hint = std::max(c->cap_hint, over_ring(c, [](const gs_ctx* m) { return m->capacity; }, true));
    c->row_hint = std::max(c->row_hint, over_ring(c, [](const gs_ctx* m) { return m->row_cap; }, true));
    if (first != GS_OK) memcpy(g_err, msg, sizeof(msg));
    return first;
}

// One more member of the ring: a context with this one's configuration that borrows its splats.
static int32_t add_shadow(gs_ctx* c) {
    gs_config cfg = c->cfg;
    cfg.stream = nullptr;
    cfg.max_intersections = 0; // starts from the owner's capacity (gs_share_splats)
    gs_ctx* s = nullptr;
    int32_t rc = gs_create(&cfg, &s);
    if (rc != GS_OK) return rc;
    s->fif = 1;
    s->is_shadow = true;
    rc = gs_share_splats(s, c);
    if (rc != GS_OK) { gs_destroy(s); return rc; }
    s->opt = c->opt; // (everything else a member starts with is gs_create's: its own counters, timed_from 0)
    c->shadows.push_back(s);
    return GS_OK;
}

GS_EXPORT int32_t gs_render(gs_ctx* c, const void* uniforms) {
    if (!c || !uniforms) return fail(GS_ERR_INVALID_ARGUMENT, "gs_render: null argument");
    gs_ctx* t = c;
    if (c->fif > 1 && c->scene_mem) {
        // a second frame while the first is still in flight: open the next slot of the ring (once), then take turns
        if (c->pending && c->shadows.size() + 1 < c->fif) {
            int32_t rc = add_shadow(c);
            if (rc != GS_OK) return rc;
            c->rr = (uint32_t)c->shadows.size(); // the new slot takes this frame
        }
        if (!c->shadows.empty()) {
            const uint32_t slot = c->rr++ % (uint32_t)(c->shadows.size() + 1);
            t = slot ? c->shadows[slot - 1] : c;
        }
        if (t->capacity < c->cap_hint || t->row_cap < c->row_hint) { // another member has met a bigger frame: grow before, not after, truncating one
            HIP_TRY(hipSetDevice(t->cfg.device));
            if (t->pending) { int32_t rc = wait_one(t); if (rc != GS_OK && rc != GS_ERR_TRUNCATED) return rc; }
            int32_t rc = alloc_kv(t, std::max(t->capacity, c->cap_hint), std::max(t->row_cap, c->row_hint));
            if (rc != GS_OK) return rc;
            t->have_frame = false;
        }
    }
    const int32_t rc = render_common(t, uniforms, false, nullptr);
    if (rc == GS_OK) c->last = t;
    return rc;
}
GS_EXPORT int32_t gs_render_debug(gs_ctx* c, const void* uniforms) {
    const int32_t rc = render_common(c, uniforms, true, nullptr);
    if (rc == GS_OK && c) c->last = c;
    return rc;
}
GS_EXPORT int32_t gs_render_to(gs_ctx* c, const void* uniforms, void* d_rgba8) {
    if (!d_rgba8) return fail(GS_ERR_INVALID_ARGUMENT, "gs_render_to: null output");
    const int32_t rc = render_common(c, uniforms, false, d_rgba8);
    if (rc == GS_OK && c) c->last = c;
    return rc;
}

GS_EXPORT int32_t gs_render_host(gs_ctx* c, const void* uniforms, void* host_dst, uint64_t size, uint64_t* ticket) {
    if (!c || !uniforms || !host_dst || !ticket) return fail(GS_ERR_INVALID_ARGUMENT, "gs_render_host: null argument");
    const uint64_t bytes = (uint64_t)c->frame.slab_w * c->frame.height * 4;
    if (size < bytes) return fail(GS_ERR_INVALID_ARGUMENT, "gs_render_host: need %llu bytes, got %llu", (unsigned long long)bytes, (unsigned long long)size);
    int32_t rc = gs_render(c, uniforms);
    if (rc != GS_OK) return rc;
    gs_ctx* t = last_of(c);
    if (!t->ev_done) HIP_TRY(hipEventCreateWithFlags(t->ev_done.out(), hipEventDisableTiming));
    HIP_TRY(hipMemcpyAsync(host_dst, t->rgba8, bytes, hipMemcpyDeviceToHost, t->stream));
    std::lock_guard<std::mutex> lk(c->ticket_mu);
    HIP_TRY(hipEventRecord(t->ev_done, t->stream));
    const uint64_t k = c->next_ticket++;
    c->tickets[k & 63u].ticket = k;
    c->tickets[k & 63u].member = t;
    *ticket = k;
    return GS_OK;
}

GS_EXPORT int32_t gs_wait_ticket(gs_ctx* c, uint64_t ticket) {
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_wait_ticket: null ctx");
    gs_ctx* t = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->ticket_mu);
        if (ticket == 0 || ticket >= c->next_ticket) return fail(GS_ERR_INVALID_ARGUMENT, "gs_wait_ticket: unknown ticket %llu", (unsigned long long)ticket);
        if (c->next_ticket - ticket > 64 || c->tickets[ticket & 63u].ticket != ticket) return GS_OK; // retired long ago: its member has rendered later frames since
        t = c->tickets[ticket & 63u].member;
    }
    // the member's event is re-recorded by every later frame it renders: waiting on it is waiting for at least this ticket's frame
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipEventSynchronize(t->ev_done));
    return GS_OK;
}
