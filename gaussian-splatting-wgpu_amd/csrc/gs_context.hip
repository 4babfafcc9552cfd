// gs_context.hip -- the context and its device memory: create / destroy, the capacity-based arrays and their regrowth, scene
// upload and sharing, options.  Part of the C ABI (include/gsplat/gs_abi.h).
//
// Replaces the setup/teardown of Renderer (reference src/renderer.ts:96-347).  Where the reference allocates six sort buffers
// and clears three buffers per frame, every buffer here is allocated once (capacity-based) and grown geometrically only when a
// frame overflows (wait_one, gs_frame.hip).  Every allocation is held by an owner (gs_runtime.h): the context frees itself.
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <memory>
#include <new>

#include "gs_runtime.h"

thread_local char g_err[512] = "";
int32_t fail(int32_t code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static uint32_t tiles_f32(uint32_t extent, uint32_t ts) { // ceil(f32(extent)/f32(ts)), process_gaussians.wgsl:79
    return (uint32_t)std::ceil((float)extent / (float)ts);
}
static uint32_t bits_for(uint64_t v) {
    uint32_t b = 0;
    while (v) { ++b; v >>= 1; }
    return b ? b : 1;
}

GS_EXPORT const char* gs_last_error(void) { return g_err; }
GS_EXPORT int32_t gs_abi_version(void) { return GS_ABI_VERSION; }

// (key,value) arrays for `capacity` instances, row-item arrays for `row_cap` slots, and the control/status block sized for both.
// The old arrays go BEFORE the new ones are allocated: a regrow at 50 M splats must not hold both sets.
int32_t alloc_kv(gs_ctx* c, uint64_t capacity, uint64_t row_cap) {
    if (capacity >= (1ull << 30)) return fail(GS_ERR_CAPACITY, "capacity %llu exceeds 2^30 intersections", (unsigned long long)capacity);
    if (row_cap >= (1ull << 31)) return fail(GS_ERR_CAPACITY, "%llu row items exceed the 2^31 limit", (unsigned long long)row_cap);
    c->gr.valid = false; // (callers have drained the stream: no replay of the captured frame is in flight)
    c->keysA.reset(); c->valsA.reset(); c->keysB.reset(); c->valsB.reset(); c->keysU.reset(); c->valsU.reset();
    c->keysG.reset(); c->chunk_table.reset(); c->arena.reset(); c->rows_sorted.reset(); c->M3.reset(); c->ctl_mem.reset();
    c->valsG.reset();
    c->keysG_valid = c->valsG_valid = c->gdataG_valid = false;
    capacity = std::max<uint64_t>(capacity, 4096);
    row_cap = (std::max<uint64_t>(row_cap, 4096) + 15) & ~(uint64_t)15;
    const size_t kb = (size_t)capacity * 4;
    HIP_TRY(hipMalloc(c->keysA.out(), kb));
    HIP_TRY(hipMalloc(c->valsA.out(), kb));
    HIP_TRY(hipMalloc(c->keysB.out(), kb));
    HIP_TRY(hipMalloc(c->valsB.out(), kb));
    c->sort_index = GsSort{{c->keysA, c->valsA}, {c->keysB, c->valsB}, c->passes, 8, 0, false, false};
    // (by tile: the balanced emission has written u16 tile ids where they fit, key/1000 is taken by the sweep otherwise; it has
    // also accumulated the digit counts)
    c->sort_tile = GsSort{{c->keysA, c->valsA}, {c->keysB, c->valsB}, c->tile_passes, c->tile_bits, c->tile16 ? 0u : 1u, c->tile16, true};
    HIP_TRY(hipMalloc(c->chunk_table.out(), (size_t)gs_emit_chunks(std::max(capacity, row_cap)) * 4));
    if (c->tight_ok) {
        HIP_TRY(hipMalloc(c->arena.out(), (size_t)row_cap * 12));
        HIP_TRY(hipMalloc(c->rows_sorted.out(), gs_rows_sorted_bytes(row_cap)));
        HIP_TRY(hipMalloc(c->M3.out(), (size_t)gs_rows_chunks(row_cap) * 256 * 4)); // (rows of the widest canvas: a frame uses 64 * ceil(ntx / 64) columns)
    }
    const size_t ctl_sz = (sizeof(GsControl) + 255) & ~(size_t)255;
    const size_t scan_sz = (((size_t)gs_scan_blocks(c->n ? c->n : 1) + 1) * 8 + 255) & ~(size_t)255;
    const size_t sort_sz = (size_t)std::max(c->passes, c->tile_passes) * gs_sort_tiles(capacity) * 256 * 4;
    const size_t rows_sz = c->tight_ok ? (size_t)gs_rows_sort_tiles(row_cap) * 256 * 4 : 0;
    const size_t depth_sz = ((size_t)c->T * 4 + 255) & ~(size_t)255;
    // layout: control block | blend depth | row-sort status || scan status | instance-sort status: a tight frame zeroes the first
    // three only (the instance sort's status alone is 27 MB at config B, and a tight frame never touches it)
    c->ctl_bytes = ctl_sz + depth_sz + rows_sz + scan_sz + sort_sz;
    c->ctl_bytes_tight = ctl_sz + depth_sz + rows_sz;
    HIP_TRY(hipMalloc(c->ctl_mem.out(), c->ctl_bytes));
    char* const base = (char*)c->ctl_mem.get();
    c->ctl = (GsControl*)base;
    c->tile_depth = (uint32_t*)(base + ctl_sz);
    c->rows_status = (uint32_t*)(base + ctl_sz + depth_sz);
    c->scan_status = (unsigned long long*)(base + ctl_sz + depth_sz + rows_sz);
    c->sort_status = (uint32_t*)(base + ctl_sz + depth_sz + rows_sz + scan_sz);
    c->capacity = capacity;
    c->row_cap = row_cap;
    c->frame.capacity = (uint32_t)capacity;
    c->frame.row_cap = (uint32_t)row_cap;
    return GS_OK;
}

GS_EXPORT int32_t gs_create(const gs_config* cfg, gs_ctx** out) {
    if (!cfg || !out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_create: null argument");
    if (cfg->struct_size != sizeof(gs_config)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_create: struct_size %u != %zu", cfg->struct_size, sizeof(gs_config));
    if (cfg->width == 0 || cfg->height == 0) return fail(GS_ERR_INVALID_ARGUMENT, "gs_create: empty canvas");
    if (cfg->tile_size != 8 && cfg->tile_size != 16 && cfg->tile_size != 32)
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_create: tile_size must be 8, 16 or 32 (got %u)", cfg->tile_size);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(GS_ERR_NO_DEVICE, "gs_create: no HIP device");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(GS_ERR_INVALID_ARGUMENT, "gs_create: device %d of %d", cfg->device, ndev);
    HIP_TRY(hipSetDevice(cfg->device));

    std::unique_ptr<gs_ctx> c(new (std::nothrow) gs_ctx()); // every early exit below frees what has been built so far
    if (!c) return fail(GS_ERR_OUT_OF_MEMORY, "gs_create: host allocation failed");
    c->cfg = *cfg;
    GsFrame& f = c->frame;
    f.width = cfg->width; f.height = cfg->height; f.tile_size = cfg->tile_size;
    f.ntx = tiles_f32(cfg->width, cfg->tile_size);
    f.nty = tiles_f32(cfg->height, cfg->tile_size);
    if (f.ntx >= 32768 || f.nty >= 65536) return fail(GS_ERR_INVALID_ARGUMENT, "gs_create: canvas too large");
    f.col0 = cfg->col_begin;
    f.col1 = cfg->col_end;
    if (f.col0 == 0 && f.col1 == 0) f.col1 = f.ntx;
    if (f.col1 > f.ntx || f.col0 >= f.col1) return fail(GS_ERR_INVALID_ARGUMENT, "gs_create: bad tile-column slab [%u,%u) of %u", f.col0, f.col1, f.ntx);
    f.full = (f.col0 == 0 && f.col1 == f.ntx) ? 1u : 0u;
    f.px0 = f.col0 * f.tile_size;
    f.slab_w = std::min(f.width, f.col1 * f.tile_size) - f.px0;
    c->T = f.ntx * f.nty;
    // largest key a rect can produce: tile (nty*ntx + ntx) (rows/cols one past the grid), bucket 999
    const uint64_t max_key = ((uint64_t)f.nty * f.ntx + f.ntx) * 1000ull + 999ull;
    if (max_key > 0xFFFFFFFFull) return fail(GS_ERR_INVALID_ARGUMENT, "gs_create: tile ids overflow the 32-bit key (write_tile_ids.wgsl:29)");
    c->key_bits = bits_for(max_key);
    c->passes = (c->key_bits + 7) / 8;
    const uint32_t tbits = bits_for((uint64_t)f.nty * f.ntx + f.ntx);
    c->tile_passes = (tbits + 7) / 8;
    c->tile_bits = (tbits + c->tile_passes - 1) / c->tile_passes;
    c->tile16 = ((uint64_t)f.nty * f.ntx + f.ntx) < 0xFFFFull;
    if ((uint64_t)(f.ntx + 1) * (f.nty + 1) > GS_COUNT_MASK) return fail(GS_ERR_INVALID_ARGUMENT, "gs_create: canvas has too many tiles");
    c->tight_ok = f.ntx <= 255u && f.nty <= 255u; // the row pipeline's digits are a tile row / a tile column: 8 bits each (k_rows.hip)

    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    c->opt.grid_persist = (uint32_t)prop.multiProcessorCount * 4;
    if (cfg->stream) c->stream = (hipStream_t)cfg->stream;
    else { HIP_TRY(hipStreamCreateWithFlags(c->own_stream.out(), hipStreamNonBlocking)); c->stream = c->own_stream; }

    HIP_TRY(hipMalloc(c->ranges.out(), (size_t)c->T * 4));
    HIP_TRY(hipMemset(c->ranges, 0, (size_t)c->T * 4));
    const size_t px = (size_t)f.slab_w * f.height;
    HIP_TRY(hipMalloc(c->rgba8.out(), px * 4));
    HIP_TRY(hipMemset(c->rgba8, 0, px * 4));
    if (cfg->flags & GS_FLAG_F32_TAP) HIP_TRY(hipMalloc(c->rgbf.out(), px * 12));
    if (cfg->flags & GS_FLAG_AUX_OUTPUTS) { // eagerly, with the context: every blend of this context writes them
        HIP_TRY(hipMalloc(c->alpha.out(), px * 4));
        HIP_TRY(hipMalloc(c->depth.out(), px * 4));
        HIP_TRY(hipMemset(c->alpha, 0, px * 4));
        HIP_TRY(hipMemset(c->depth, 0, px * 4));
    }
    HIP_TRY(hipHostMalloc(c->h_ctl.out(), sizeof(GsControl), hipHostMallocDefault));
    memset(c->h_ctl, 0, sizeof(GsControl));
    HIP_TRY(hipMalloc(c->d_pxb.out(), 65 * 4));
    HIP_TRY(hipMalloc(c->tileoff.out(), 256 * 256 * 4));
    HIP_TRY(hipMalloc(c->rowtot.out(), 256 * 4));
    HIP_TRY(hipMalloc(c->sticky.out(), 4 * 4));
    HIP_TRY(hipMemset(c->sticky, 0, 4 * 4));
    HIP_TRY(hipHostMalloc(c->h_rep.out(), sizeof(GsReport), hipHostMallocDefault));
    memset(c->h_rep, 0, sizeof(GsReport));
    if (cfg->flags & GS_FLAG_TIMING) {
        for (auto& row : c->ev)
            for (auto& e : row) HIP_TRY(hipEventCreate(e.out()));
        c->have_events = true;
    }
    c->fif = (c->own_stream && f.full) ? 3u : 1u; // a caller-supplied stream or a slab orders its work with the caller's: one frame
                                                  // (3: config B 682 / 787 / 804 / 764 frames/s with 1 / 2 / 3 / 4 in flight)
    *out = c.release();
    return GS_OK;
}

// The graph and its exec go before the buffers they point into; the members then free themselves, the owned stream last.
gs_ctx::~gs_ctx() { drop_graph(this); }

GS_EXPORT int32_t gs_destroy(gs_ctx* c) {
    if (!c) return GS_OK;
    hipSetDevice(c->cfg.device);
    drop_shadows(c); // they borrow this context's scene
    if (c->stream) hipStreamSynchronize(c->stream); // before anything it may still use is freed
    delete c;
    return GS_OK;
}

// Drops the previous scene and per-gaussian work arrays, allocates the work arrays for n gaussians.
static int32_t alloc_per_gaussian(gs_ctx* c, uint64_t n, uint64_t min_capacity = 0, uint64_t min_rows = 0) {
    c->gr.valid = false;
    c->scene_own.reset();
    c->scene_mem = nullptr;
    c->n = (uint32_t)n;
    c->frame.n = (uint32_t)n;
    c->have_frame = false;
    c->cov.reset(); // the coverage planes describe the scene that goes: they read as zero afterwards
    c->ng = gs_ctx::Neigh{}; // ... and so does the neighbour count plane (its scratch is sized for that scene)
    c->cl = gs_ctx::Cluster{}; // ... and the cluster planes: they read "no label, size 0" again
    c->kn = gs_ctx::Knn{}; // ... and the nearest-neighbour planes: NaN / GS_KNN_NONE again, and no k to refine
    c->sf = gs_ctx::Surface{}; // ... and the surface planes and kept sums: NaN / count 0 again, no sums to read
    c->th = gs_ctx::Thin{}; // ... and the thinning planes: GS_THIN_NONE / 0 again
    c->counts.reset(); c->offsets.reset(); c->grec.reset(); c->rowptr.reset(); c->gsort_scratch.reset(); c->gdata.reset(); c->gdataG.reset();
    c->unit_off.reset(); c->unit_n.reset();
    const size_t np = ((size_t)n + 63) & ~(size_t)63;
    // the entry planes of a tight frame (counts, rowptr, unit_off: k_gsort.hip) hold whole chunks of the gaussian-level sort, and the
    // unit counts one pair per chunk and a pair more; the counts past the last unit are zeroed here and never written
    const size_t ne = (size_t)gs_gsort_tiles((uint32_t)(n ? n : 1)) * 2048, nu = ne / 1024 + 2;
    HIP_TRY(hipMalloc(c->counts.out(), ne * 4));
    HIP_TRY(hipMalloc(c->offsets.out(), std::max<size_t>(np * 4, 256)));
    HIP_TRY(hipMalloc(c->grec.out(), std::max<size_t>(np * 16, 256)));
    HIP_TRY(hipMalloc(c->rowptr.out(), ne * 4));
    HIP_TRY(hipMalloc(c->unit_off.out(), ne * 2));
    HIP_TRY(hipMalloc(c->unit_n.out(), nu * 4));
    HIP_TRY(hipMemsetAsync(c->unit_n, 0, nu * 4, c->stream));
    HIP_TRY(hipMalloc(c->gsort_scratch.out(), gs_gsort_scratch_bytes((uint32_t)n)));
    HIP_TRY(hipMalloc(c->gdata.out(), ((size_t)n + GS_RECORD_SLACK) * 64));
    HIP_TRY(hipMemsetAsync(c->gdata, 0, ((size_t)n + GS_RECORD_SLACK) * 64, c->stream));
    uint64_t cap = c->cfg.max_intersections ? c->cfg.max_intersections : std::max<uint64_t>(4 * n, 1u << 22);
    cap = std::max<uint64_t>(cap, min_capacity);
    cap = std::min<uint64_t>(cap, (1ull << 30) - 1);
    // row-item slots: a visible gaussian takes one per tile row of its ellipse (about three of them at 1080p, about 40 % of the
    // gaussians visible); grown like the (key,value) capacity when a frame needs more
    const uint64_t rows = std::max<uint64_t>(std::max<uint64_t>(2 * n, 1u << 20), min_rows);
    return alloc_kv(c, cap, rows);
}

// Where the planes of a scene of n gaussians lie behind `base` (gs_runtime.h): the one copy of this arithmetic.
GsSceneLayout scene_layout(void* base, uint64_t n, bool state) {
    GsSceneLayout L;
    const size_t np = ((size_t)n + 63) & ~(size_t)63; // plane stride keeps every plane and both record arrays 256-byte aligned
    // (GS_FLAG_SPLAT_STATE: the state plane follows the SH records, on the next 256-byte boundary; np bytes, so that whole words
    // and 16-byte groups of it are the context's own)
    const size_t sh_end = np * 4 * 4 + np * 32 + (size_t)n * 192, state_at = (sh_end + 255) & ~(size_t)255;
    L.np = np;
    L.state_at = state_at;
    L.bytes = state ? state_at + np : sh_end;
    char* p = (char*)base;
    GsScene& s = L.scene;
    s.px = (float*)p; p += np * 4; s.py = (float*)p; p += np * 4; s.pz = (float*)p; p += np * 4;
    s.smax = (float*)p; p += np * 4;
    s.geo = (float4*)p; p += np * 32;
    s.sh = (float4*)p;
    s.state = state ? (const uint8_t*)base + state_at : nullptr;
    return L;
}
// c->scene_own holds a scene of n gaussians: the views into it.
static void scene_views(gs_ctx* c, uint64_t n) {
    const GsSceneLayout L = scene_layout(c->scene_own.get(), n, has_state(c));
    c->scene_mem = c->scene_own;
    c->scene_bytes = L.bytes;
    c->scene = L.scene;
}

// Drops the previous scene, allocates the per-gaussian work arrays and the resident scene arrays for n gaussians.
uint64_t scene_new_serial() {
    static std::atomic<uint64_t> next{1};
    return next.fetch_add(1, std::memory_order_relaxed);
}
int32_t scene_alloc(gs_ctx* c, uint64_t n, uint64_t min_capacity, uint64_t min_rows) {
    c->scene_serial = scene_new_serial(); // an upload or a compaction: the splats are numbered anew (an insertion installs, and keeps it)
    int32_t rc = alloc_per_gaussian(c, n, min_capacity, min_rows);
    if (rc != GS_OK) return rc;
    const GsSceneLayout L = scene_layout(nullptr, n, has_state(c));
    HIP_TRY(hipMalloc(c->scene_own.out(), std::max<size_t>(L.bytes, 256)));
    scene_views(c, n);
    if (has_state(c)) // zeroed by every upload
        HIP_TRY(hipMemsetAsync((char*)c->scene_mem + L.state_at, 0, std::max<size_t>(L.np, 4), c->stream));
    return GS_OK;
}

// Drops the previous scene, allocates the per-gaussian work arrays for n gaussians and takes `mem`, a complete scene of n gaussians
// laid out by scene_layout, as the resident one (gs_insert.hip).  On an error the context holds no scene, as after an upload that failed.
int32_t scene_install(gs_ctx* c, DevBuf<>&& mem, uint64_t n, uint64_t min_capacity, uint64_t min_rows) {
    const int32_t rc = alloc_per_gaussian(c, n, min_capacity, min_rows);
    if (rc != GS_OK) {
        c->scene = GsScene{};
        c->n = c->frame.n = 0;
        return rc;
    }
    c->scene_own = std::move(mem);
    scene_views(c, n);
    return GS_OK;
}

static int32_t upload_common(gs_ctx* c, const void* d_aos, uint64_t n) {
    int32_t rc = scene_alloc(c, n);
    if (rc != GS_OK) return rc;
    if (n) gs_launch_repack(d_aos, (uint32_t)n, 0, c->scene, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

// a new scene: the shadows of the ring are dropped (they hold arrays sized for the old one and borrow its planes); the next
// frame that finds its predecessor in flight opens a new one
void drop_shadows(gs_ctx* c) {
    for (gs_ctx* s : c->shadows) gs_destroy(s);
    c->shadows.clear();
    c->last = c;
    c->rr = 0;
    c->cap_hint = 0;
    c->row_hint = 0;
}
GS_EXPORT int32_t gs_share_splats(gs_ctx* c, gs_ctx* owner) {
    if (!c || !owner || c == owner) return fail(GS_ERR_INVALID_ARGUMENT, "gs_share_splats: needs two distinct contexts");
    if (c->cfg.device != owner->cfg.device) return fail(GS_ERR_INVALID_ARGUMENT, "gs_share_splats: contexts are on different devices");
    if (!c->is_shadow) drop_shadows(c);
    if (!owner->scene_mem) return fail(GS_ERR_NO_SCENE, "gs_share_splats: the owner holds no splats");
    if (has_state(c) && !has_state(owner))
        return fail(GS_ERR_INVALID_ARGUMENT, "gs_share_splats: this context has GS_FLAG_SPLAT_STATE, the owner keeps no state plane");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (c->pending) { int32_t rc = wait_one(c); if (rc != GS_OK) return rc; }
    // start from the capacity the owner has already grown to: a borrower exists to keep several frames in flight, and a
    // frame that overflows while others are queued behind it cannot be re-rendered (GS_ERR_TRUNCATED)
    int32_t rc = alloc_per_gaussian(c, owner->n, c->cfg.max_intersections ? 0 : owner->capacity, owner->row_cap);
    if (rc != GS_OK) return rc;
    c->scene_mem = owner->scene_mem; // borrowed, read-only during a frame; the owner must outlive this context
    c->scene_bytes = owner->scene_bytes;
    c->scene = owner->scene;
    c->scene_serial = scene_new_serial(); // (a borrower takes no snapshots; what it held before is another scene in any case)
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GS_OK;
}

GS_EXPORT int32_t gs_upload_splats_device(gs_ctx* c, const void* d_aos, uint64_t n) {
    if (!c || (!d_aos && n)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_upload_splats_device: null argument");
    if (n >= (1ull << 31)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_upload_splats: too many gaussians");
    HIP_TRY(hipSetDevice(c->cfg.device));
    drop_shadows(c);
    return upload_common(c, d_aos, n);
}

GS_EXPORT int32_t gs_upload_splats(gs_ctx* c, const void* aos, uint64_t n) {
    if (!c || (!aos && n)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_upload_splats: null argument");
    if (n >= (1ull << 31)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_upload_splats: too many gaussians");
    HIP_TRY(hipSetDevice(c->cfg.device));
    drop_shadows(c);
    DevBuf<> d; // bounce buffer: the records as the caller holds them
    const size_t bytes = (size_t)n * GS_SPLAT_RECORD_BYTES;
    HIP_TRY(hipMalloc(d.out(), std::max<size_t>(bytes, 256)));
    if (bytes) {
        hipError_t e = hipMemcpy(d, aos, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(GS_ERR_HIP, "upload memcpy: %s", hipGetErrorString(e));
    }
    return upload_common(c, d, n); // (synchronises the stream before d goes)
}

GS_EXPORT int32_t gs_host_alloc(uint64_t bytes, void** out) {
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "gs_host_alloc: null argument");
    *out = nullptr;
    HIP_TRY(hipHostMalloc(out, std::max<size_t>((size_t)bytes, 256), hipHostMallocDefault));
    return GS_OK;
}
GS_EXPORT void gs_host_free(void* p) { if (p) hipHostFree(p); }

GS_EXPORT int32_t gs_slab_width(gs_ctx* c, uint32_t* px_begin, uint32_t* px_width) {
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_slab_width: null ctx");
    if (px_begin) *px_begin = c->frame.px0;
    if (px_width) *px_width = c->frame.slab_w;
    return GS_OK;
}

// One member of the ring: the options go into its record (GsOptions) and nowhere else; GS_OPT_RESET_TIMING is no option but a
// reset of the member's own counters.
static int32_t set_option_one(gs_ctx* c, int32_t key, int64_t value) {
    c->gr.valid = false; // a captured frame holds the options it was recorded with
    GsOptions& o = c->opt;
    switch (key) {
    case GS_OPT_FRAME_GRAPH: o.frame_graph = (value != 0); return GS_OK;
    case GS_OPT_BLEND_ABLATION: o.blend_ablation = (uint32_t)value & 0x3FFFFu; return GS_OK;
    case GS_OPT_PERSISTENT_GRID: if (value <= 0) break; o.grid_persist = (uint32_t)value; return GS_OK;
    case GS_OPT_RESET_TIMING: c->timed_from = c->frames; c->max_I_seen = 0; c->truncated_frames = 0; return GS_OK;
    case GS_OPT_EMIT_ORDER: if (value < 0 || value > 2) break; o.emit_order = (int)value; return GS_OK;
    case GS_OPT_UNFUSED: return GS_OK; // (removed in ABI 3: the fused projection+scan+emission launch measured slower; accepted, ignored)
    case GS_OPT_DEBUG_VIEW: if (value < 0 || value > 4) break; o.debug_view = (uint32_t)value; return GS_OK;
    case GS_OPT_TILE_CULL: o.tile_cull = (value != 0); return GS_OK;
    case GS_OPT_PROJ_CHUNKS: if (value != 0 && value != 2 && value != 4 && value != 8) break; o.tight_nb = (uint32_t)value; return GS_OK;
    case GS_OPT_SELECT_TINT: // (the captured frame is dropped above: its projection node holds the tint by value)
        if (!has_state(c)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_set_option: GS_OPT_SELECT_TINT needs GS_FLAG_SPLAT_STATE");
        if (value < 0 || value > 0xFFFFFFFFll) break;
        o.select_tint = (uint32_t)value;
        return GS_OK;
    default: break;
    }
    return fail(GS_ERR_INVALID_ARGUMENT, "gs_set_option: bad key/value %d/%lld", key, (long long)value);
}
GS_EXPORT int32_t gs_set_option(gs_ctx* c, int32_t key, int64_t value) {
    if (!c) return fail(GS_ERR_INVALID_ARGUMENT, "gs_set_option: null ctx");
    if (key == GS_OPT_FRAMES_IN_FLIGHT) {
        if (value < 1 || value > 4) return fail(GS_ERR_INVALID_ARGUMENT, "gs_set_option: frames in flight must be 1..4");
        if (!c->own_stream || !c->frame.full) value = 1; // a caller-supplied stream / a slab: see gs_create
        int32_t rc = gs_wait(c);
        if (rc != GS_OK && rc != GS_ERR_TRUNCATED) return rc;
        while (c->shadows.size() + 1 > (size_t)value) { // the last frame may live in a shadow that goes away: taps need a new frame
            if (c->last == c->shadows.back()) { c->last = c; }
            gs_destroy(c->shadows.back());
            c->shadows.pop_back();
        }
        c->fif = (uint32_t)value;
        c->rr = 0;
        return GS_OK;
    }
    int32_t rc = set_option_one(c, key, value);
    for (gs_ctx* s : c->shadows) if (rc == GS_OK) rc = set_option_one(s, key, value);
    return rc;
}
