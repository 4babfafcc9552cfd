/*
 * gs_abi.h -- C ABI of the MI355X-native forward Gaussian-splat rasterizer.
 *
 * This is the drop-in boundary for the hot path of ldyken53/gaussian-splatting-wgpu: everything
 * `Renderer` (src/renderer.ts:96-102,349-593) asks of WebGPU per scene and per frame goes through
 * the entry points below.  Plain C: opaque handle, plain pointers and sizes, int32 status codes,
 * no C++ types, no exceptions, no torch types.  The reference has no FFI of its own (it is a
 * browser app); the N-API binding a Node host uses is gaussian-splatting-wgpu_amd/csrc/napi and
 * the binding stubs for other hosts are in INTEGRATION.md.
 *
 * Threading: a gs_ctx is not re-entrant: its functions must not be called concurrently on the same ctx (the one exception is
 * gs_wait_ticket, which another thread may call while the owner enqueues); different ctxs may be used from different threads.
 * Frames in flight: a whole-canvas ctx on its own stream keeps up to GS_OPT_FRAMES_IN_FLIGHT (default 3) frames in flight -- a
 * frame enqueued while the previous one is still on the device is rendered by a SHADOW of the ctx (own stream and per-frame
 * arrays, the same resident splats), gs_render taking turns over that ring.  With K frames enqueued: gs_wait waits for ALL of
 * them (and reports a capacity overflow of an earlier one as GS_ERR_TRUNCATED: only the last frame can be re-rendered; a frame of
 * the batch over the 2^30 limit makes it GS_ERR_CAPACITY instead, see there);
 * gs_read_rgba8, gs_read_buffer, gs_device_ptr and gs_get_stats describe the LAST frame enqueued (its ring member);
 * gs_render_host / gs_wait_ticket address a frame of their own.  A host that calls gs_wait after every gs_render (as
 * Renderer.animate does) never has more than one frame in flight and sees none of this.  Device work of one ring member is
 * ordered on one HIP stream.
 * Ownership: the ctx owns every device allocation; host pointers passed in are copied before the
 * call returns; output host buffers are caller-allocated.
 */
#ifndef GSPLAT_GS_ABI_H
#define GSPLAT_GS_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 3

/* ---- status codes (every function returns one; message via gs_last_error) ------------------ */
#define GS_OK 0
#define GS_ERR_INVALID_ARGUMENT (-1) /* null pointer, bad size, unsupported tile size ...           */
#define GS_ERR_NO_DEVICE (-2)        /* no HIP device / HIP runtime failure at create             */
#define GS_ERR_HIP (-3)              /* a HIP call failed; gs_last_error has hipGetErrorString      */
#define GS_ERR_OUT_OF_MEMORY (-4)
#define GS_ERR_NO_SCENE (-5)         /* gs_render before gs_upload_splats                           */
#define GS_ERR_NO_FRAME (-6)         /* read-back before any gs_render                              */
#define GS_ERR_DEVICE_FAULT (-7)     /* an in-kernel bounded spin gave up (decoupled look-back)     */
#define GS_ERR_CAPACITY (-8)         /* intersections exceed the hard limit (2^30, radix_sort.wgsl:220-221).  gs_wait: a frame enqueued
                                        since the last gs_wait -- the last one or an earlier one, on any ring member -- has I >= 2^30.
                                        The device sums instance counts in saturating 32-bit arithmetic: such a frame reports
                                        min(I, 2^32 - 1), never a wrapped count.  It is not re-rendered and nothing is grown for it
                                        (a last frame that ALSO overflowed the row-item arena is first rendered again with the arena, and
                                        the lists for the instances that had fitted, grown: only then is its I known) and no frame of the
                                        batch is counted in truncated_frames; its lists and image are truncated at the capacity and not
                                        to be used.  After the refusal gs_get_stats reads, for a frame that was the last one enqueued,
                                        num_intersections = min(I, 2^32 - 1), and max_intersections_seen >= that wherever in the batch or
                                        the ring the frame was; capacity and row_capacity are what they were.  The refusal is reported
                                        ONCE, by the gs_wait that follows the frame: later frames render normally, and a gs_wait that
                                        finds no new over-limit frame returns GS_OK.  A batch that holds an over-limit frame returns
                                        GS_ERR_CAPACITY whichever frame it was, also where an earlier frame of the batch merely overflowed
                                        the capacity (GS_ERR_TRUNCATED is not reported then); the batch's last frame is complete unless
                                        it is the refused one                                                                    */
#define GS_ERR_TRUNCATED (-9)        /* gs_wait: a frame enqueued BEFORE the last one overflowed the (key,value) capacity; its
                                        output came from truncated lists and cannot be re-rendered (the last frame is complete and
                                        the capacity has been grown)                                                          */

/* ---- byte layouts fixed by the reference ------------------------------------------------------
 * splat record   320 B  ply.ts:190-198 / process_gaussians.wgsl:1-7
 *     pos f32x3 @0, log_scale f32x3 @16, rot f32x4 (r,x,y,z) @32, opacity_logit f32 @48,
 *     sh 16 x (f32x3, stride 16) @64
 * uniform block  160 B  renderer.ts:15-24,371-392 / process_gaussians.wgsl:16-25
 *     view mat4 col-major @0, proj(=P*V) @64, cam_pos f32x3 @128, tan_fovx @140, tan_fovy @144,
 *     focal_x @148, focal_y @152, scale_modifier @156
 * GaussianData    64 B  process_gaussians.wgsl:8-15
 *     uv f32x2 @0, conic f32x3 @16, depth @28, color f32x3 @32, opacity @44, rect u32x4 @48
 */
#define GS_SPLAT_RECORD_BYTES 320
#define GS_UNIFORM_BYTES 160
#define GS_GAUSSIAN_DATA_BYTES 64

/* ---- configuration: what `new Renderer(canvas, camera, device, gaussians, tileSize)` fixes ---- */
#define GS_FLAG_EXACT_BLEND 0x1u /* blend with the canonical (as-written, unfused) f32 arithmetic: bit-equal to
                                    the CPU oracle; default is fused f32 + hardware exp2 (<=1e-4 per channel)  */
#define GS_FLAG_F32_TAP 0x2u     /* also keep the un-quantised f32 RGB accumulators (GS_BUF_RGB_F32)            */
#define GS_FLAG_TIMING 0x4u      /* bracket every stage with hipEvents; gs_get_stats returns stage microseconds */
#define GS_FLAG_AUX_OUTPUTS 0x8u /* also keep the per-pixel alpha and accumulated-depth planes (GS_BUF_ALPHA_F32, GS_BUF_DEPTH_F32),
                                    computed from the colour's own entries and weights; the rgba8 image is unchanged (alpha byte 255) */
#define GS_FLAG_SPLAT_STATE 0x10u /* keep one state byte per resident splat (GS_BUF_SPLAT_STATE, gs_state_*): hidden splats are not
                                    rendered, selected ones are drawn tinted.  Without the flag no frame changes by a bit          */

typedef struct gs_config {
    uint32_t struct_size;       /* = sizeof(gs_config); lets the struct grow                                     */
    uint32_t width, height;     /* canvas.width / canvas.height (renderer.ts:157,199,366)                       */
    uint32_t tile_size;         /* 8, 16 or 32 (index.html:20-24, app.ts:29,45)                                 */
    int32_t device;             /* HIP device ordinal                                                           */
    uint32_t col_begin, col_end;/* tile-column slab owned by this ctx, [begin,end); 0,0 = whole screen.  A slab only
                                   filters: its frame is the whole screen's frame cut to its columns, bit for bit, for
                                   any finite view matrix in the uniform block (scaled, sheared, non-rigid included) */
    uint32_t flags;             /* GS_FLAG_*                                                                     */
    uint64_t max_intersections; /* capacity hint for the (key,value) arrays; 0 = derive from the scene         */
    void* stream;               /* hipStream_t to run on; NULL = the ctx creates its own (so the legacy default stream,
                                   whose handle is 0, cannot be passed: give the ctx a created stream when its work must be
                                   ordered with other work, e.g. a collective)                                      */
} gs_config;

/* ---- per-frame statistics (the reference only console.logs these: renderer.ts:406-590) ------- */
enum {
    GS_STAGE_PREPROCESS = 0, /* process_gaussians.wgsl::main                       */
    GS_STAGE_SCAN = 1,       /* ExclusiveScanner.scan (exclusive_scan.ts:208-325)  */
    GS_STAGE_EMIT = 2,       /* write_tile_ids.wgsl::main                          */
    GS_STAGE_SORT = 3,       /* GPUSorter.sort (sort.ts:341-350)                   */
    GS_STAGE_RANGES = 4,     /* compute_ranges.wgsl::main                          */
    GS_STAGE_BLEND = 5,      /* compute_tiles.wgsl::main (+ the render.wgsl blit, which is the identity) */
    GS_STAGE_COUNT = 6
};

typedef struct gs_stats {
    uint64_t num_gaussians;       /* N                                                        */
    uint64_t num_visible;         /* gaussians that passed the cull (tile count > 0)          */
    uint64_t num_intersections;   /* I: what ExclusiveScanner.scan returns (renderer.ts:419)  */
    uint64_t num_processed;       /* list entries the blend read before tile early-exit (per tile: the deepest of its walkers; the
                                     id words are read 192 entries ahead of the records, so this runs up to 191 ahead of the last
                                     entry whose record was fetched) */
    uint32_t num_tiles;           /* T over the whole canvas                                  */
    uint32_t sort_passes;         /* 8-bit radix passes executed                              */
    uint64_t frames;              /* frames rendered by this ctx                              */
    float stage_us[GS_STAGE_COUNT]; /* per-stage device time of the last frame (GS_FLAG_TIMING) */
    float frame_us;               /* first kernel start -> last kernel end (GS_FLAG_TIMING)    */
    float stage_us_mean[GS_STAGE_COUNT]; /* mean over the frames since GS_OPT_RESET_TIMING (at most the last 256) */
    float frame_us_mean;
    uint32_t frames_timed;        /* frames the means cover                                    */
    uint32_t depth_ordered;       /* 1 if the last frame used the depth-ordered pipeline (GS_OPT_EMIT_ORDER)   */
    uint64_t num_evaluated;       /* blend: (8x8 pixel block, entry) pairs evaluated after the block cull */
    uint64_t capacity;            /* entries the (key,value) arrays hold now                                  */
    uint64_t max_intersections_seen; /* largest I of any frame of any ring member since GS_OPT_RESET_TIMING (as of the last gs_wait);
                                        an I beyond 32 bits reads 2^32 - 1                                                  */
    uint64_t truncated_frames;    /* frames since GS_OPT_RESET_TIMING that overflowed the capacity and could not be re-rendered
                                     (only possible when several frames are enqueued per gs_wait); a gs_wait that returns
                                     GS_ERR_CAPACITY counts none                                                  */
    uint32_t tight_binning;       /* 1 if the last frame used the opacity-aware (tight) binning of the product path: its
                                     instance lists are then a subset of the reference's (GS_OPT_TILE_CULL)             */
    uint32_t frames_in_flight;    /* contexts of the ring gs_render alternates between now (GS_OPT_FRAMES_IN_FLIGHT)      */
    uint64_t graph_frames;        /* frames replayed from the captured frame graph (GS_OPT_FRAME_GRAPH), summed over the ring */
    uint64_t num_row_items;       /* tight frames (ABI 3): row items = (gaussian, tile row) runs of tiles the lists were expanded from */
    uint64_t num_row_slots;       /*   ... slots reserved for them (items + rows that turned out empty)                               */
    uint64_t row_capacity;        /* row-item slots the context holds now (grown like `capacity`)                                  */
} gs_stats;

/* ---- debug taps: the buffers the reference author inspected by hand (renderer.ts:423-438,504-519) */
enum {
    GS_BUF_TILE_COUNTS = 0,   /* u32[N]     tileCountBuffer                                   */
    GS_BUF_TILE_OFFSETS = 1,  /* u32[N]     tileOffsetBuffer after the scan (needs gs_render_debug)  */
    GS_BUF_GAUSSIAN_DATA = 2, /* 64 B x N   gaussianDataBuffer (culled records are all-zero)  */
    GS_BUF_KEYS_UNSORTED = 3, /* u32[I]     tile_ids as written by write_tile_ids (needs gs_render_debug) */
    GS_BUF_VALUES_UNSORTED = 4,
    GS_BUF_KEYS = 5,          /* u32[I]     sorted tileIDBuffer                                */
    GS_BUF_VALUES = 6,        /* u32[I]     sorted gaussianIDBuffer                            */
    GS_BUF_RANGES = 7,        /* u32[T]     rangesBuffer                                       */
    GS_BUF_RGBA8 = 8,         /* u8[H][Wslab][4] renderTarget (rgba8unorm), this ctx's slab    */
    GS_BUF_RGB_F32 = 9,       /* f32[H][Wslab][3] (GS_FLAG_F32_TAP)                            */
    GS_BUF_BLOCK_MASKS = 10,  /* u32[I]     per sorted instance: one bit per 8x8 pixel block of its tile (row-major, tile_size/8
                                 per row) the blend evaluates it for; all blocks when the frame did not use tight binning  */
    /* 11 and 12 are the library's profiling and test taps */
    GS_BUF_ALPHA_F32 = 13,    /* f32[H][Wslab] (GS_FLAG_AUX_OUTPUTS) accumulated opacity A = 1 - T_final; 0 where no entry reaches.
                                 The colour is premultiplied: over a background B, C + (1 - A) B                              */
    GS_BUF_DEPTH_F32 = 14,    /* f32[H][Wslab] (GS_FLAG_AUX_OUTPUTS) accumulated depth D = sum of z alpha T over the kept entries,
                                 z = GaussianData.depth, in list order with the colour's association; expected depth = D / A
                                 where A > 0 (the division is left to the host)                                                */
    GS_BUF_SPLAT_STATE = 15   /* u8[N] (GS_FLAG_SPLAT_STATE) the state plane as it is NOW (not of the last frame); readable as soon as
                                 splats are resident, before any frame                                                          */
};

typedef struct gs_ctx gs_ctx;

/* Thread-local message of the last failing call on this thread. */
const char* gs_last_error(void);
int32_t gs_abi_version(void);

/* Replaces `new Renderer(...)` buffer/pipeline setup (renderer.ts:96-324). */
int32_t gs_create(const gs_config* cfg, gs_ctx** out);
/* Replaces Renderer.destroy()/destroyImpl (renderer.ts:90-94,326-347).  Safe before the first frame. */
int32_t gs_destroy(gs_ctx* ctx);

/* Replaces the pointDataBuffer upload (renderer.ts:130-137): takes the exact bytes of
 * PackedGaussians.gaussiansBuffer (ply.ts:204-220), n records of 320 B, host memory.  The records
 * are re-laid-out on the device; the caller's buffer is not referenced after return. */
int32_t gs_upload_splats(gs_ctx* ctx, const void* aos320, uint64_t n);
/* Native PackedGaussians (ply.ts:162-228): parses a binary little-endian 3DGS .ply with the reference's header and
 * property rules and returns n packed 320-byte records (malloc'ed; release with gs_ply_free).  sh_degree may be NULL. */
int32_t gs_ply_load(const char* path, void** records, uint64_t* n, int32_t* sh_degree);
void gs_ply_free(void* records);
/* gs_ply_load + gs_upload_splats. */
int32_t gs_upload_ply(gs_ctx* ctx, const char* path, uint64_t* n);
/* Same, from a device pointer (no PCIe copy).  The records must be COMPLETE when the call is made: the repack runs on the
 * context's stream and is not ordered against whatever stream produced them (synchronise the producer first).  Returns
 * after the repack; the caller may free d_aos320 then. */
int32_t gs_upload_splats_device(gs_ctx* ctx, const void* d_aos320, uint64_t n);
/* `ctx` renders `owner`'s resident splats (same device; read-only during a frame) with its own stream and per-frame
 * buffers: several contexts rendered round-robin keep several frames in flight, so one frame's blend (instruction-issue
 * bound) overlaps the next frame's binning and sort (memory/latency bound).  The reference has one frame in flight
 * (Renderer.animate awaits every stage, renderer.ts:394-587).  `owner` must outlive `ctx` and must not re-upload
 * meanwhile; a gs_compact of the owner counts as a re-upload (share again afterwards). */
int32_t gs_share_splats(gs_ctx* ctx, gs_ctx* owner);

/* Replaces one Renderer.animate() frame (renderer.ts:349-593): enqueues the whole frame for the
 * 160-byte uniform block and returns without waiting for the device. */
int32_t gs_render(gs_ctx* ctx, const void* uniforms160);
/* As gs_render, additionally keeping the unsorted (key,value) arrays for GS_BUF_*_UNSORTED. */
int32_t gs_render_debug(gs_ctx* ctx, const void* uniforms160);
/* As gs_render, writing the rgba8 slab image straight into caller-owned DEVICE memory
 * (u8[height][slab_width][4]); used to render into a collective's send buffer. */
int32_t gs_render_to(gs_ctx* ctx, const void* uniforms160, void* d_rgba8);
/* Blocks until the frame is complete (the reference awaits onSubmittedWorkDone 8x per frame).
 * Reports device-side faults; grows the (key,value) capacity and re-renders if the frame overflowed.  When several
 * frames were enqueued since the last gs_wait and an EARLIER one overflowed, that frame cannot be re-rendered: the
 * capacity is grown for the following frames and GS_ERR_TRUNCATED is returned (the last frame is complete).  A frame with 2^30
 * or more intersections, wherever in the batch, is refused with GS_ERR_CAPACITY (see there for what the context holds afterwards);
 * that takes precedence over GS_ERR_TRUNCATED, and the next gs_wait is clean. */
int32_t gs_wait(gs_ctx* ctx);

/* Pipelined presentation (a host that does not await every frame, unlike renderer.ts:394-587): as gs_render, plus an asynchronous
 * copy of the finished rgba8 slab image (height * slab_width * 4 bytes, <= size) into `host_dst` on the frame's own stream, so
 * frame k+1 is enqueued -- and rendered by the next member of the ring -- while frame k is still being blended and copied.
 * `host_dst` should come from gs_host_alloc (page-locked: the copy then overlaps the rendering; pageable memory also works, slower)
 * and must stay untouched until gs_wait_ticket(*ticket) has returned.  Tickets count up from 1 per root ctx. */
int32_t gs_render_host(gs_ctx* ctx, const void* uniforms160, void* host_dst, uint64_t size, uint64_t* ticket);
/* Blocks until the frame of that ticket and its copy are complete.  May be called from another thread than the one that
 * enqueues (one waiter per ticket).  A frame that overflowed a capacity is NOT re-rendered here: size the capacities first (render
 * the scene's largest views once with gs_render + gs_wait, or pass gs_config.max_intersections); the next gs_wait reports it
 * (GS_ERR_TRUNCATED).  At most 64 tickets may be outstanding. */
int32_t gs_wait_ticket(gs_ctx* ctx, uint64_t ticket);
/* Page-locked host memory for frame sinks. */
int32_t gs_host_alloc(uint64_t bytes, void** out);
void gs_host_free(void* p);

/* Replaces the blit to the canvas (render.wgsl, renderer.ts:549-574): copies the finished rgba8
 * image of this ctx's slab to host memory; size must be height*slab_width*4. */
int32_t gs_read_rgba8(gs_ctx* ctx, void* dst, uint64_t size);
/* Copies one debug tap to host memory.  *written receives the byte count; dst may be NULL to query it. */
int32_t gs_read_buffer(gs_ctx* ctx, int32_t which, void* dst, uint64_t size, uint64_t* written);
/* Device address of a tap (valid until the next gs_render / gs_destroy), for zero-copy consumers. */
int32_t gs_device_ptr(gs_ctx* ctx, int32_t which, void** d_ptr);
int32_t gs_get_stats(gs_ctx* ctx, gs_stats* out);
/* ---- picking: which splat is under a pixel of the LAST frame ------------------------------------
 * The planes of GS_FLAG_AUX_OUTPUTS tell how opaque a pixel is and how far its colour lies on average; they cannot tell WHICH
 * splat the user clicked.  gs_pick answers that for up to 65536 pixels per call by walking, for each of them, its tile's list of
 * the last frame (GS_BUF_VALUES / GS_BUF_RANGES / GS_BUF_GAUSSIAN_DATA, still resident) with the blend's own arithmetic,
 * compute_tiles.wgsl:44-66 restated: per entry  d = uv * (W, H) - pixel,  power = -0.5 (cx dx dx + cz dy dy) - cy dx dy,
 * alpha = min(0.99, opacity exp(power)),  test = T (1 - alpha),  cond = power <= 0 && alpha >= 1/255 && test >= 1e-4
 * (:60-63),  T = cond test + (1 - cond) T (:65).  An entry with cond = 1 is ACCEPTED; its weight is w = alpha T with T taken
 * before the entry.  The reference has no early termination: an entry rejected by test < 1e-4 may be followed by an accepted one.
 * The results are DEFINED by the canonical (GS_FLAG_EXACT_BLEND) arithmetic -- one f32 rounding per written operation, the
 * oracle's exp -- whatever blend the frame itself used: on a default (fused) frame they are the canonical answer, which differs
 * from what the fused kernel accumulated by its documented <= 1e-4 envelope; on an EXACT frame `alpha` and `depth_acc` equal
 * GS_BUF_ALPHA_F32 / GS_BUF_DEPTH_F32 bit for bit.  Every field is the same for tight and reference binning (a tight list drops
 * only entries no pixel of the tile accepts), gs_render and gs_render_debug, and every GS_OPT_EMIT_ORDER -- except list_length,
 * which describes the lists actually rendered.  The reference has no picking (a viewer, not an editor). */
#define GS_PICK_OK 0u
#define GS_PICK_OUTSIDE_SLAB 1u
#define GS_PICK_NONE 0xFFFFFFFFu
#define GS_PICK_MAX_QUERIES 65536u
#define GS_PICK_MAX_CONTRIB 256u
typedef struct gs_pick_query { uint32_t x, y; } gs_pick_query; /* CANVAS pixel coordinates */
typedef struct gs_pick_result { /* 48 bytes */
    uint32_t status;       /* GS_PICK_OK; GS_PICK_OUTSIDE_SLAB: x is on the canvas but not in this ctx's slab (every other field
                              0 / GS_PICK_NONE), so a multi-GPU host can send one query list to every rank                   */
    uint32_t list_length;  /* entries of the pixel's tile list in the frame that was rendered                               */
    uint32_t hit_count;    /* entries the blend accepts at this pixel (cond = 1, compute_tiles.wgsl:60-63)                   */
    uint32_t first_id;     /* gaussian index of the first accepted entry; GS_PICK_NONE if hit_count = 0                      */
    float first_depth;     /* its GaussianData.depth; 0 if none                                                             */
    uint32_t max_id;       /* accepted entry with the largest weight w (one f32 product alpha * T); the EARLIEST on ties;
                              GS_PICK_NONE if none                                                                          */
    float max_weight;      /* that w; 0 if none                                                                             */
    uint32_t median_id;    /* first accepted entry after which T <= 0.5; GS_PICK_NONE if T never gets there.  Unlike the mean
                              depth_acc / alpha, the median always lies on a surface: the orbit pivot / "focus here" depth     */
    float median_depth;    /* its GaussianData.depth; 0 if none                                                             */
    float alpha;           /* 1 - T_final: what GS_BUF_ALPHA_F32 holds for an EXACT frame                                    */
    float depth_acc;       /* sum of cond z alpha T in list order: what GS_BUF_DEPTH_F32 holds for an EXACT frame            */
    uint32_t reserved;     /* 0                                                                                             */
} gs_pick_result;
typedef struct gs_pick_contrib { uint32_t id; float weight; } gs_pick_contrib;
/* Answers `n` (1..GS_PICK_MAX_QUERIES) queries about the LAST frame enqueued (its ring member, like gs_read_buffer), waiting for
 * it first if it is still pending.  HOST pointers in and out (there is no device-pointer variant yet); `results` has n records.
 * `contrib` may be NULL (then max_contrib must be 0); otherwise max_contrib is 1..GS_PICK_MAX_CONTRIB and `contrib` has
 * n * max_contrib records: for query q, at contrib[q * max_contrib], the first min(hit_count, max_contrib) accepted entries in
 * list order with their weights, the remaining slots {GS_PICK_NONE, 0}.  One wave per query on the frame's own stream; the call
 * returns with the results on the host.  It is not a frame: no statistic, tap or option changes and a captured frame graph
 * stays valid.  GS_ERR_INVALID_ARGUMENT (the message names the query) for a pixel outside the canvas, GS_ERR_NO_FRAME when no
 * frame has been rendered since gs_create / the last upload. */
int32_t gs_pick(gs_ctx* ctx, const gs_pick_query* queries, uint32_t n, gs_pick_result* results, uint32_t max_contrib,
                gs_pick_contrib* contrib);

/* ---- splat state: hide, select and tint resident splats without re-upload ------------------------
 * A ctx created with GS_FLAG_SPLAT_STATE keeps a u8[N] plane inside its scene allocation, one byte per resident splat, zeroed by
 * every gs_upload_*.  GS_SPLAT_HIDDEN: the projection treats the splat exactly like one that fails in_frustum
 * (process_gaussians.wgsl:108-125): tile count 0, no GaussianData record, no instance.  GS_SPLAT_SELECTED: the splat's colour,
 * after compute_color_from_sh (:240-280), becomes col + k (tint - col) per channel (GS_OPT_SELECT_TINT; one f32 rounding per
 * operation).  Hidden wins over selected.  Bits 2-7 belong to the host (lock flags, layers): carried and filtered on, never
 * interpreted.  gs_share_splats carries the plane to a borrower (a flagged ctx cannot borrow from an unflagged owner); the shadows
 * of the frames-in-flight ring inherit it.  The reference has no counterpart (a viewer, not an editor): this is what an editor
 * does with the answer of gs_pick -- select / delete / inspect -- where a host would otherwise edit its own 320-byte records and
 * upload them again.
 * Membership of a region is a test of the splat's CENTRE (x, y, z of its record), fixed to the operation so that a host can
 * restate it bit for bit (one f32 rounding per operation, no contraction):
 *     ph = proj * (x, y, z, 1), pv = view * (x, y, z, 1), each row ((m[r] x + m[4+r] y) + m[8+r] z) + m[12+r]
 *     pw = 1 / (ph.w + 1e-7);  px = ((ph.x pw) 0.5 + 0.5) W;  py = ((ph.y pw) 0.5 + 0.5) H      (W, H: the CANVAS, also on a slab ctx)
 *     SCREEN_RECT  !(pv.z <= 0.2) && px >= x0 && px < x1 && py >= y0 && py < y1                 (x0.. converted to f32)
 *     SCREEN_MASK  !(pv.z <= 0.2) && px >= 0 && px < W && py >= 0 && py < H && mask[(int)py][(int)px] != 0
 *     SPHERE       (dx dx + dy dy) + dz dz <= r r,  d = position - a, r = b[0]
 *     BOX          a <= position <= b on every axis, both ends inclusive
 *     ALL          every splat
 * A NaN fails every test.  These select THROUGH surfaces; surface-only selection is Renderer.pick_rect / gs_pick followed by
 * gs_state_ids.
 * Ordering: every gs_state_* call first completes all frames enqueued on the ctx's ring, as gs_wait does (an error of that wait is
 * returned and nothing is applied), then runs on the ctx's stream and returns when done.  A state call is not a frame: taps,
 * statistics and gs_pick still describe what was rendered, a captured frame graph stays valid (it reads the plane when it is
 * replayed), and the NEXT frame sees the new state.  Contexts that the host drives itself through gs_share_splats are the
 * host's to drain before a state call, as they are before an upload.  On a ctx without GS_FLAG_SPLAT_STATE every call below, the
 * tap and GS_OPT_SELECT_TINT return GS_ERR_INVALID_ARGUMENT.  Multi-GPU: every rank holds its own copy of the scene; the host
 * applies the same call on every rank (the result is deterministic). */
#define GS_SPLAT_HIDDEN 0x1u
#define GS_SPLAT_SELECTED 0x2u
#define GS_STATE_SET 1u      /* s |= bits */
#define GS_STATE_CLEAR 2u    /* s &= ~bits */
#define GS_STATE_TOGGLE 3u   /* s ^= bits */
#define GS_STATE_ASSIGN 4u   /* s = bits */
enum { GS_REGION_ALL = 0, GS_REGION_SPHERE = 1, GS_REGION_BOX = 2, GS_REGION_SCREEN_RECT = 3, GS_REGION_SCREEN_MASK = 4 };
typedef struct gs_region {
    uint32_t struct_size, kind; /* = sizeof(gs_region), GS_REGION_*                                                    */
    float a[3], b[3];          /* SPHERE: a centre, b[0] radius.  BOX: a min, b max, both inclusive                     */
    uint32_t x0, y0, x1, y1;   /* SCREEN_RECT: canvas pixels [x0,x1) x [y0,y1)                                          */
    const void* uniforms160;   /* SCREEN_*: the camera (host pointer, copied)                                           */
    const uint8_t* mask;       /* SCREEN_MASK: host u8[height][width] of the CANVAS, nonzero = inside (copied)          */
    uint32_t where_mask, where_value; /* only splats with (s & where_mask) == where_value are touched                  */
} gs_region;
/* Applies `op` with `bits` (<= 0xFF) to the state byte of every splat in the region that passes the `where` filter.  *matched
 * (may be NULL) receives their number, whether or not their byte changed.  One streaming pass: 13 bytes read per splat. */
int32_t gs_state_region(gs_ctx* ctx, const gs_region* region, uint32_t op, uint32_t bits, uint64_t* matched);
/* The same for n splat indices (HOST pointer).  An id >= N: GS_ERR_INVALID_ARGUMENT, the message names the index, nothing is
 * changed.  Duplicates behave as the sequential application would (TOGGLE twice is a no-op). */
int32_t gs_state_ids(gs_ctx* ctx, const uint32_t* ids, uint64_t n, uint32_t op, uint32_t bits);
/* Number of splats with (s & mask) == value. */
int32_t gs_state_count(gs_ctx* ctx, uint32_t mask, uint32_t value, uint64_t* count);
/* Replaces the whole plane (n must be N) from host memory: undo / restore of what GS_BUF_SPLAT_STATE returned. */
int32_t gs_state_write(gs_ctx* ctx, const uint8_t* src, uint64_t n);

/* ---- splat edits: list, export, compact and save resident splats by state ------------------------
 * The state calls above stop at the byte; these bring splats back OUT of the library and make an edit permanent.  The reference
 * has no counterpart: its host keeps the PackedGaussians buffer it uploaded (renderer.ts:130-137) and would filter and upload
 * that again; gs_upload_ply streams a file into the device planes precisely so that no such host copy exists.
 * Filter: every call takes (mask, value); a splat matches when (s & mask) == value, exactly gs_state_count's filter.  mask or
 * value above 0xFF: GS_ERR_INVALID_ARGUMENT.  (0, 0) matches every splat and is accepted on a ctx WITHOUT GS_FLAG_SPLAT_STATE
 * (export and save what is resident); any other filter on such a ctx is refused like the state calls.
 * Ordering: matching splats are always delivered in ASCENDING index order -- the reference's tie-break order inside a depth
 * bucket, so a compacted scene renders what the scene with the same splats hidden rendered.  Every call first completes all
 * frames enqueued on the ctx's ring, as gs_state_* do (an error of that wait is the call's error and nothing is done), then runs
 * on the ctx's stream and returns when done.  GS_ERR_NO_SCENE before any upload.
 * Ownership: output buffers are caller-allocated; the selection scratch (one count per 1024 splats, the id list) belongs to the
 * ctx, grows on demand and goes with it.  A record is the 320-byte layout gs_upload_splats takes; the device scene carries 59 of
 * its 80 floats, so the 21 padding floats (float 3, 7, 13, 14, 15 and 19 + 4k, k = 0..15) come back as +0.0f and every other
 * float as the uploaded bit pattern (NaN payloads, -0 and infinities included).
 * Multi-GPU: every rank holds its own copy of the scene; the host applies the same call on every rank (the result is
 * deterministic). */
/* Indices of the matching splats, ascending.  ids == NULL: only *n is written (query).  cap < *n: GS_ERR_INVALID_ARGUMENT, the
 * message names the count needed, nothing is written to ids. */
int32_t gs_state_list(gs_ctx* ctx, uint32_t mask, uint32_t value, uint32_t* ids, uint64_t cap, uint64_t* n);
/* The matching splats as 320-byte records in HOST memory.  ids (may be NULL, else cap_records entries): the old index of every
 * record.  aos320 == NULL: query (only *n).  cap_records too small: as above.  One pass: 244 B read, 320 B written per splat. */
int32_t gs_export_splats(gs_ctx* ctx, uint32_t mask, uint32_t value, void* aos320, uint64_t cap_records, uint64_t* n, uint32_t* ids);
/* Same, DEVICE pointers (d_aos320 and d_ids); written on the ctx stream, complete on return. */
int32_t gs_export_splats_device(gs_ctx* ctx, uint32_t mask, uint32_t value, void* d_aos320, uint64_t cap_records, uint64_t* n,
                                uint32_t* d_ids);
/* Keeps the matching splats, drops the rest, renumbers: the ctx then holds *kept splats and is in the state of a ctx that was
 * given gs_upload_splats(the kept records, in order) followed by gs_state_write(their state bytes) -- the bytes are carried
 * unchanged, so a selection survives a delete and host bits 2-7 survive.  ids (HOST, may be NULL, capacity = N before the call):
 * ids[new index] = old index, how a host renumbers its own per-splat metadata.  Like an upload: the frames-in-flight shadows are
 * dropped, a captured frame graph is invalidated, taps, gs_read_rgba8 and gs_pick return GS_ERR_NO_FRAME until the next frame;
 * statistics windows are untouched; the per-gaussian work arrays are re-sized for the new N while the (key,value) and row
 * capacities stay at least as large as they were.  kept == 0 leaves the ctx as gs_upload_splats(ctx, NULL, 0) leaves it; kept == N
 * takes the same path.  Old and new scene are both resident during the call: 245 B x (N + kept).  A ctx that borrows its scene
 * (gs_share_splats) is refused with GS_ERR_INVALID_ARGUMENT: compact the owner.  For the owner's borrowers a compaction counts as
 * a re-upload: the owner must not compact while they render, and they must gs_share_splats again afterwards. */
int32_t gs_compact(gs_ctx* ctx, uint32_t mask, uint32_t value, uint64_t* kept, uint32_t* ids);
/* Inverse of gs_ply_load: n packed records -> binary little-endian 3DGS .ply as ply.ts:162-228 reads it.  Header `ply`, `format
 * binary_little_endian 1.0`, `element vertex n`, then `property float` x y z nx ny nz f_dc_0..2 f_rest_0..3K-1 opacity
 * scale_0..2 rot_0..3 with K = (sh_degree + 1)^2 - 1, `end_header`.  Normals are +0.0f; f_dc_c is record float 16 + c,
 * f_rest_{cK+i} record float 16 + 4(i+1) + c (ply.ts:178-187 inverted); coefficients above the degree are not written.  No ctx,
 * no GPU.  sh_degree outside 0..3, a null path or records, a file that cannot be created or fully written:
 * GS_ERR_INVALID_ARGUMENT naming the path and the errno text; a partial file is removed. */
int32_t gs_ply_save(const char* path, const void* records, uint64_t n, int32_t sh_degree);
/* gs_export_splats + gs_ply_save without a whole-scene host buffer: chunks of at most 64 Ki records are unpacked into a device
 * staging buffer, copied to one of two pinned host buffers and written while the next chunk is on its way -- gs_upload_ply's
 * mirror image.  Host memory does not grow with N.  *n (may be NULL): records written. */
int32_t gs_export_ply(gs_ctx* ctx, const char* path, uint32_t mask, uint32_t value, int32_t sh_degree, uint64_t* n);

/* ---- splat insertion: append records, a .ply or a copy of a selection to the resident splats ---------
 * The edits above select, hide, delete, export and save; these ADD splats to a ctx that already holds some, where gs_upload_*
 * would replace the whole scene: a second capture merged into the first (then moved and graded to match it: splat transforms,
 * colour grades), or the editor's "duplicate the selection".  The reference has no counterpart: its host keeps the records it
 * uploaded (renderer.ts:130-137) and would concatenate and upload them again; a scene streamed in by gs_upload_ply has no such
 * host copy, and gs_export_splats of everything + a host concatenation + a new upload is what these calls replace.  gs_compact's
 * mirror image: a new scene of another N is built from the old one on the device.
 * Where the new splats go: before the call the ctx holds N splats, afterwards N + m.  Old splats keep their indices and every bit
 * of their records and state bytes.  The new splats take the indices *first = N .. N + m - 1 in the order given: record order for
 * an append, file order for a .ply, ASCENDING source index for a duplicate (the reference's tie-break order and the splat edits'
 * rule); ids[j] is the source index of new splat *first + j.
 * What the ctx equals afterwards: a fresh ctx that was given gs_upload_splats(old records ++ new records) followed by
 * gs_state_write(old bytes ++ m x new_state) -- every tap and the image, bit for bit.  For gs_append_ply the new records are what
 * gs_ply_load makes of the file: coefficients above the file's SH degree are +0.0f, a uchar property is value / 255 evaluated in
 * double, any property order is accepted (the kernel and the two-buffer stream of gs_upload_ply, with a destination offset).
 * new_state: ONE byte, given to every new splat (GS_SPLAT_SELECTED: the new capture is what the next transform or grade acts on).
 * Above 0xFF: GS_ERR_INVALID_ARGUMENT.  Non-zero on a ctx without GS_FLAG_SPLAT_STATE: refused as the state calls refuse such a
 * ctx.  (mask, value) of a duplicate follow the splat edits' filter rules: above 0xFF refused, (0, 0) duplicates every splat and
 * works without the flag, any other filter needs it.
 * Like gs_compact in everything else: the call first completes all frames enqueued on the ctx's ring (an error of that wait is
 * the call's error and nothing is done), runs on the ctx's stream and returns when done; the frames-in-flight shadows are
 * dropped, a captured frame graph is invalidated, taps, gs_read_rgba8 and gs_pick return GS_ERR_NO_FRAME until the next frame;
 * statistics windows are untouched; the per-gaussian work arrays are re-sized for N + m while the (key,value) and row capacities
 * stay at least as large as they were.  The coverage, neighbour-count and cluster planes are dropped and read as their initial
 * values (0, 0, GS_CLUSTER_NONE): carrying them across an insertion is out of scope, accumulate / count / label again.  A ctx that
 * borrows its scene (gs_share_splats) is refused with GS_ERR_INVALID_ARGUMENT: insert into the owner; for the owner's borrowers
 * an insertion counts as a re-upload: the owner must not insert while they render, and they must gs_share_splats again
 * afterwards.  GS_ERR_NO_SCENE before any upload; a ctx that holds an EMPTY scene (gs_upload_splats(ctx, NULL, 0)) accepts
 * insertions.  Multi-GPU: the same call on every rank (the result is deterministic).
 * m == 0 -- an empty append, a .ply of 0 vertices, a filter that matches nothing -- is a no-op: *first = N, *m = 0, GS_OK, nothing
 * is reallocated, the shadows, a captured graph and the last frame stay (taps and gs_pick keep answering).
 * Atomic: every refusal -- a null or bad argument, N + m >= 2^31, a file that cannot be opened, a bad header, a file smaller than
 * data_off + m x stride, a vertex stride above 0xFFFF -- is decided before anything is allocated or freed.  The new scene is
 * then built BESIDE the old one and installed only when its tail is complete: a HIP error or a short read on the way leaves the
 * ctx with the old scene, its last frame and its planes exactly as they were.  (Only the re-sizing of the work arrays comes after
 * the install; should that run out of memory the ctx holds no scene, as after an upload that failed.)  Peak device memory is
 * therefore 245 B x (2 N + m) for the two scenes, plus the 320 B x m bounce buffer of a host append or the two 64 Ki-vertex
 * staging buffers of a .ply.  Every call costs O(N): amortised over-allocation for many small appends is out of scope.
 * *first, *m and ids may be NULL. */
int32_t gs_append_splats(gs_ctx* ctx, const void* aos320, uint64_t m, uint32_t new_state, uint64_t* first);
/* Same, DEVICE pointer: no PCIe copy.  The records must be complete before the call (it reads them on the ctx's stream). */
int32_t gs_append_splats_device(gs_ctx* ctx, const void* d_aos320, uint64_t m, uint32_t new_state, uint64_t* first);
/* gs_ply_load + gs_append_splats without the host records: the file is streamed into the tail of the new scene. */
int32_t gs_append_ply(gs_ctx* ctx, const char* path, uint32_t new_state, uint64_t* first, uint64_t* m);
/* Appends a copy of every splat with (s & mask) == value, in ascending source order; the copies get new_state, not their source's
 * byte.  ids (HOST, may be NULL, capacity = N before the call): ids[j] = source index of new splat *first + j. */
int32_t gs_duplicate_splats(gs_ctx* ctx, uint32_t mask, uint32_t value, uint32_t new_state, uint64_t* first, uint64_t* m,
                            uint32_t* ids /* HOST, may be NULL, capacity N */);

/* ---- splat transforms: move, rotate and scale resident splats in place -----------------------------
 * The verb the edits above lack: a similarity p' = s R (p - pivot) + pivot + t, uniform s > 0, applied to the resident splats that
 * pass a state filter, in ONE streaming pass over the affected planes -- no export / edit / re-upload round trip, no reallocation,
 * no frame kernel touched.  The reference has no counterpart (a viewer); the conventions a transform must respect are its own:
 * compute_cov3d (process_gaussians.wgsl:127-163) normalises rot every frame and builds the covariance from exp(log-scale);
 * compute_color_from_sh (:221-280) fixes the SH basis order, constants and signs, evaluated at dir = normalize(position - camera).
 * A NON-UNIFORM scale or a shear does not keep a splat an axis-aligned-scales-plus-rotation gaussian: out of scope, there is no
 * field for it.
 * Two layers.  gs_transform_splats applies exactly the f32 numbers of a gs_xform, with arithmetic a host can restate bit for bit
 * (one f32 rounding per written operation, no contraction, left to right -- the rule of gs_state_region).  Everything that needs
 * trigonometry or the SH rotation lives in gs_xform_compose: plain host code, no ctx, no GPU, computed in double, every output
 * rounded once.  A host may also fill the struct itself.
 * Per matching splat; only the parts named in `flags` are read or written, the others keep their bit patterns (NaN payloads
 * included); opacity, SH band 0 and the state byte are never written:
 *   POSITION  p'_r = ((m[4r] x + m[4r+1] y) + m[4r+2] z) + m[4r+3],  r = 0, 1, 2
 *   ORIENT    rot' = q * rot (Hamilton product, both (r,x,y,z), a = q, b = rot):
 *               r' = ((a.r b.r - a.x b.x) - a.y b.y) - a.z b.z        x' = ((a.r b.x + a.x b.r) + a.y b.z) - a.z b.y
 *               y' = ((a.r b.y - a.x b.z) + a.y b.r) + a.z b.x        z' = ((a.r b.z + a.x b.y) - a.y b.x) + a.z b.r
 *             not renormalised (compute_cov3d normalises per frame: any non-zero rot stays correct); and for every channel c and
 *             band l = 1, 2, 3 (coefficients k0 .. k0 + 2l, k0 = 1, 4, 9, record float 16 + 4k + c):
 *               out_i = sum_j D_l[i][j] in_j  evaluated as  acc = D[i][0] in_0;  acc = acc + D[i][j] in_j  for j ascending,
 *             every output of a band from the OLD values of the band (D_1 = sh1, D_2 = sh2, D_3 = sh3, row-major)
 *   SIZE      log-scale_k' = log-scale_k + log_scale, k = 0, 1, 2; the derived largest log-scale the slab cull reads is recomputed
 *             as fmaxf(l0', fmaxf(l1', l2')), the upload's own expression: a transformed ctx and a freshly uploaded one agree
 * Traffic per matched splat: POSITION 12 B read, 12 B written; ORIENT 16 + 180 B each way; SIZE 12 B read, 16 B written; plus
 * 1 B of state per RESIDENT splat when a filter other than (0, 0) is given (the selection of the splat edits, which reads the
 * plane once to count and once more to scatter, and moves 4 B of index per match each way).
 * Filter, refusals and ordering are those of the splat edits: (mask, value) as gs_state_count, above 0xFF refused, (0, 0) matches
 * every splat and is accepted on a ctx without GS_FLAG_SPLAT_STATE, any other filter on such a ctx is refused.  The call first
 * completes all frames enqueued on the ctx's ring (an error of that wait is the call's error, nothing is applied), runs on the
 * ctx's stream and returns when done.  It is NOT a frame and NOT an upload: taps, statistics and gs_pick keep describing the frame
 * that was rendered, the frames-in-flight shadows, the capacities and a captured frame graph stay (the graph reads the planes when
 * it is replayed); the NEXT frame sees the moved splats.  A ctx that borrows its scene (gs_share_splats) is refused: transform the
 * owner -- its borrowers then render the new scene, and as for a state call the host drains them first.  GS_ERR_NO_SCENE before
 * any upload; N == 0: *matched = 0, GS_OK.  Multi-GPU: the same call on every rank (the result is deterministic).
 * The inverse transform is NOT a bit-exact undo (every step rounds): a host that wants one exports the selection first.
 * (Or takes a gs_snapshot of the parts the transform names, on the device: "snapshots and write-back" below.)
 * "Bit for bit" has one exception a restating host must know: a NaN that an operation above PRODUCES or propagates (a NaN or an
 * infinite input in a flagged part: inf * 0, inf - inf) is a NaN on every machine, but IEEE 754 leaves its sign and payload open
 * and the device's choice differs from that of other processors (x86 produces 0xFFC00000 for inf * 0): compare such floats as
 * "NaN on both sides".  Floats of parts that are not flagged, and of splats that do not match, are never computed: their NaN
 * payloads survive untouched. */
#define GS_XFORM_POSITION 0x1u  /* positions                                   */
#define GS_XFORM_ORIENT   0x2u  /* rot quaternion and SH bands 1..3            */
#define GS_XFORM_SIZE     0x4u  /* the three log-scales (and the derived smax) */
typedef struct gs_xform {
    uint32_t struct_size, flags; /* = sizeof(gs_xform), GS_XFORM_*                                                   */
    float m[12];      /* row-major 3x4: p'_r = ((m[4r] x + m[4r+1] y) + m[4r+2] z) + m[4r+3]                         */
    float q[4];       /* (r,x,y,z), composed on the LEFT of the splat's rot                                          */
    float log_scale;  /* added to each of the three log-scales                                                       */
    float sh1[9], sh2[25], sh3[49]; /* row-major band matrices D_l; band 0 is never touched                          */
} gs_xform;
/* Fills *out for p' = scale R (p - pivot) + pivot + translate, R the rotation of rot_rxyz (any non-zero length; pivot NULL = the
 * origin): q = rot_rxyz normalised; m = [sR | t + pivot - sR pivot]; log_scale = (float)log(scale); D_l such that, with B_l(d) the
 * vector of compute_color_from_sh's band-l terms (constants and signs included), B_l(R^T d) = D_l^T B_l(d) for every unit d -- the
 * rotated splat seen from d shows what the original showed from R^T d.  flags = POSITION, plus ORIENT unless the normalised q is
 * +-(1,0,0,0), plus SIZE unless scale == 1.  A null pointer other than pivot, a zero or non-finite quaternion, scale <= 0 or
 * non-finite, a non-finite translate or pivot: GS_ERR_INVALID_ARGUMENT and a message. */
int32_t gs_xform_compose(const float rot_rxyz[4], const float translate[3], float scale, const float pivot[3], gs_xform* out);
/* Applies *x to every resident splat with (s & mask) == value; *matched (may be NULL) receives their number.  A wrong struct_size,
 * unknown flag bits or a non-finite member of a flagged part: GS_ERR_INVALID_ARGUMENT, nothing is applied.  flags == 0 is a valid
 * no-op that still reports *matched. */
int32_t gs_transform_splats(gs_ctx* ctx, uint32_t mask, uint32_t value, const gs_xform* x, uint64_t* matched);

/* ---- colour grades: recolour and fade resident splats in place ------------------------------------
 * The transforms move splats; a grade changes what they look like: brighten, tint, desaturate, set black and white points, fade --
 * on the resident splats that pass a state filter, in ONE streaming pass over their SH records (and the opacity logit), instead of
 * gs_export_splats (320 B per splat), a host edit of 48 coefficients per splat and a re-upload that drops the frame, the shadows,
 * a captured graph and the coverage / neighbour / cluster planes.  The reference has no counterpart (a viewer); the convention is
 * its compute_color_from_sh (process_gaussians.wgsl:221-280): C = max(0, SH_C0 sh_0 + sum_k b_k(d) sh_k + 0.5) per channel.
 * An affine map of the displayed colour, C' = A C + o (A 3x3 over (r,g,b)), holds in EVERY view direction when it is applied to the
 * coefficients:  sh_k' = A sh_k for k >= 1,  sh_0' = A sh_0 + (A h + o - h) / SH_C0,  h = (1/2, 1/2, 1/2) -- exact in real
 * arithmetic wherever the final clamp is inactive before and after.  Non-affine grades (gamma, curves) are out of scope; so is a
 * multiplicative opacity (it needs a sigmoid and its inverse): the opacity term is ADDED to the logit, which multiplies the ODDS
 * op / (1 - op) -- about the opacity itself where it is small.
 * Two layers, as for the transforms.  gs_grade_splats applies exactly the f32 numbers of a gs_grade (one f32 rounding per written
 * operation, no contraction, left to right); gs_grade_compose is plain host code in double, no ctx, no GPU, no transcendental on
 * the device.  A host may also fill the struct itself.
 * Per matching splat; only the parts named in `flags` are read or written, the others keep their bit patterns (NaN payloads
 * included); positions, log-scales, rot and the state byte are never written:
 *   MATRIX   for k = 0 .. 15, (r, g, b) = record floats 16 + 4k + 0..2:  out_c = (a[3c] r + a[3c+1] g) + a[3c+2] b,  c = 0, 1, 2,
 *            every output from the OLD triple
 *   OFFSET   band 0, channel c: v_c + dc[c], v = MATRIX's output when that flag is set, the stored value otherwise
 *   OPACITY  logit' = logit + opacity_logit   (record float 12)
 * Traffic per matched splat: MATRIX 192 B read, 192 B written; OFFSET 12 B each way when MATRIX is not set (nothing more when it
 * is); OPACITY 4 B each way; plus the selection's cost when a filter other than (0, 0) is given, as stated for the transforms.
 * No resident plane is derived from the SH or the opacity at upload (the largest log-scale is the only derived plane): a graded
 * ctx and one freshly uploaded with the graded records agree in every plane.
 * Filter, refusals and ordering are those of gs_transform_splats: (mask, value) as gs_state_count, above 0xFF refused, (0, 0)
 * matches every splat and is accepted on a ctx without GS_FLAG_SPLAT_STATE, any other filter on such a ctx is refused.  The call
 * first completes all frames enqueued on the ctx's ring, runs on the ctx's stream and returns when done.  It is NOT a frame and
 * NOT an upload: taps, statistics, gs_pick, the shadows, the capacities, a captured frame graph and the coverage, neighbour and
 * cluster planes stay; the NEXT frame shows the grade.  A ctx that borrows its scene (gs_share_splats) is refused: grade the
 * owner.  GS_ERR_NO_SCENE before any upload; N == 0: *matched = 0, GS_OK.
 * The inverse grade is NOT a bit-exact undo.  (A gs_snapshot of GS_PART_SH, or of GS_PART_GEOMETRY for the opacity, is one:
 * "snapshots and write-back" below.)  The transforms' one exception to "bit for bit" holds here too: a NaN that an
 * operation above produces or propagates is compared as "NaN on both sides"; floats of parts not flagged and of splats that do not
 * match are never computed. */
#define GS_GRADE_MATRIX  0x1u   /* all 16 coefficient triples through a (192 B read, 192 B written per matched splat) */
#define GS_GRADE_OFFSET  0x2u   /* dc added to band 0 (12 B each way when MATRIX is not set) */
#define GS_GRADE_OPACITY 0x4u   /* opacity_logit added to the logit (4 B each way) */
typedef struct gs_grade {       /* 64 bytes */
    uint32_t struct_size, flags; /* = sizeof(gs_grade), GS_GRADE_* */
    float a[9];                 /* row-major 3x3 over (r,g,b) */
    float dc[3];                /* added to SH coefficient 0 */
    float opacity_logit;        /* added to the opacity logit */
    float reserved;             /* 0 */
} gs_grade;
/* Fills *out for C' = diag(gain) Sat(saturation) ((C - black) / (white - black)) + offset, Sat(t) = t I + (1 - t) 1 w^T with the
 * Rec. 709 luma weights w = (0.2126, 0.7152, 0.0722), and for the opacity's odds multiplied by opacity_gain.  gain NULL = (1,1,1),
 * offset NULL = (0,0,0).  In double, with s = 1 / ((double)white - (double)black) and SH_C0 = 0.28209479177387814, every output
 * rounded ONCE to f32:
 *   A[c][j] = (gain[c] * (saturation * delta_cj + (1 - saturation) * w[j])) * s          -> a[3c + j]
 *   o_c     = offset[c] - (gain[c] * black) * s
 *   dc[c]   = ((((A[c][0] + A[c][1]) + A[c][2]) * 0.5 + o_c) - 0.5) / SH_C0              (the double A)
 *   opacity_logit = (float)log((double)opacity_gain)
 * flags = MATRIX unless the rounded a is exactly the identity, OFFSET unless all three rounded dc are 0, OPACITY unless
 * opacity_gain == 1: the defaults (NULL, NULL, 1, 0, 1, 1) give flags == 0.  A null out, a non-finite input, white == black (or a
 * non-finite s), opacity_gain <= 0, an output that is not finite in f32: GS_ERR_INVALID_ARGUMENT and a message naming the
 * argument; nothing is written. */
int32_t gs_grade_compose(const float gain[3], const float offset[3], float saturation, float black, float white,
                         float opacity_gain, gs_grade* out);
/* Applies *g to every resident splat with (s & mask) == value; *matched (may be NULL) receives their number.  A wrong struct_size,
 * unknown flag bits, reserved != 0 or a non-finite member of a flagged part: GS_ERR_INVALID_ARGUMENT, nothing is applied.
 * flags == 0 is a valid no-op that still reports *matched. */
int32_t gs_grade_splats(gs_ctx* ctx, uint32_t mask, uint32_t value, const gs_grade* g, uint64_t* matched);

/* ---- snapshots and write-back: exact undo for resident splat edits, records scattered back by index ----
 * The edits above change resident splats in place and none of them can be taken back: the inverse of a transform or a grade rounds
 * again.  gs_export_splats brings the records of a selection out; these calls are its inverse.  The reference has no counterpart: its
 * host keeps the PackedGaussians buffer it uploaded (renderer.ts:130-137), edits that and uploads it again -- here an upload of
 * N x 320 B that a scene streamed in by gs_upload_ply has no host copy for, and that drops the last frame, the frames-in-flight
 * shadows, a captured frame graph and the coverage, neighbour and cluster planes.
 * Two layers.  gs_write_splats scatters records (and state bytes) a host holds -- what gs_export_splats returned, edited in the
 * host's own code -- into the resident planes by index.  A gs_snapshot is a device-resident copy of the named parts of a selection
 * that is restored, or swapped with the scene, in place: no PCIe traffic, no reallocation.  A swap leaves the edited values in the
 * snapshot, so a second swap redoes the edit: undo and redo from one object; a journal of many edits is a host's stack of them.
 * Parts: what a call reads or writes of a splat, by the floats of its 320-byte record (the 21 padding floats belong to no part and
 * are ignored, whatever they hold).  FLOATS ARE COPIED AS WORDS: nothing is computed but the derived largest log-scale, so every
 * bit pattern -- NaN payloads, -0, infinities -- arrives unchanged, and a host restates every result exactly.  Every float of a part
 * that is not named keeps its bit pattern, and so does every splat that is not named.  A ctx written with records R at ids I
 * equals, in every plane, a fresh ctx that was given gs_upload_splats(the record array with R at I) followed by gs_state_write.
 * Traffic per splat and direction: POSITION 12 B, GEOMETRY 32 B (+ 4 B of the derived plane written), SH 192 B, STATE 1 B (through
 * its word), + 4 B of index unless dense; a write-back reads the 16-byte columns of the named parts of each 320-byte record (16 / 48
 * / 256 B); a swap moves its parts both ways.  Bound: HBM; rates: profiles/snapshots.txt.
 * Everything else follows gs_transform_splats.  (mask, value) as gs_state_count: above 0xFF refused, (0, 0) matches every splat and
 * works on a ctx without GS_FLAG_SPLAT_STATE, any other filter -- and GS_PART_STATE -- on such a ctx is refused as the state calls
 * refuse it.  Unknown part bits: GS_ERR_INVALID_ARGUMENT.  A ctx that borrows its scene (gs_share_splats) is refused by all five ctx
 * calls, before the ring is drained: write to / snapshot the owner (its borrowers read the owner's planes and render the result).
 * Otherwise the call first completes all frames enqueued on the ctx's ring (an error of that wait is the call's error, nothing is
 * done), runs on the ctx's stream and returns when done.  It is NOT a frame and NOT an upload: taps, statistics, gs_pick, the
 * shadows, the capacities, a captured frame graph and the coverage, neighbour and cluster planes stay; the NEXT frame shows the
 * written splats.  GS_ERR_NO_SCENE before any upload.  Every refusal is decided before anything is written.  Multi-GPU: the same
 * call on every rank (a snapshot belongs to its rank's ctx). */
#define GS_PART_POSITION 0x1u /* record floats 0..2                                  12 B */
#define GS_PART_GEOMETRY 0x2u /* record floats 4..6, 8..11, 12: log-scales, rot, opacity logit 32 B;
                                 the derived largest log-scale is recomputed as fmaxf(l0, fmaxf(l1, l2)),
                                 the upload's own expression */
#define GS_PART_SH       0x4u /* the 48 SH coefficients (record floats 16+4k+c)       192 B */
#define GS_PART_STATE    0x8u /* the state byte (needs GS_FLAG_SPLAT_STATE)             1 B */
#define GS_PART_RECORD   0x7u
/* Write-back.  Record g of the m given 320-byte records goes to splat ids[g]; ids == NULL: to splat g, and m <= N is required.
 * Only the parts named are written, from the corresponding floats of the record.  states: one byte per given record, read only
 * with GS_PART_STATE (may be NULL otherwise, must not be with it), assigned through word atomics as gs_state_ids' ASSIGN does.
 * ids must be strictly ascending and < N -- the order gs_state_list, gs_export_splats and gs_compact deliver; it rules out
 * duplicates, so the result depends on no order.  The host variant checks the list on the host before anything is copied; the
 * device variant with one small kernel whose answer is read back before the scatter is launched.  Both refuse with
 * GS_ERR_INVALID_ARGUMENT and a message that names the position and the two ids (or the id that is no splat); nothing is written.
 * The host variant stages through a bounce buffer, at most 2^20 records (320 MB) per trip, as the export does.  parts == 0 or
 * m == 0 is a valid no-op.  *written (may be NULL): m, or 0 for a no-op. */
int32_t gs_write_splats(gs_ctx* ctx, const uint32_t* ids, uint64_t m, const void* aos320, const uint8_t* states, uint32_t parts,
                        uint64_t* written);                                                              /* HOST pointers   */
/* Same, DEVICE pointers (d_ids, d_aos320, d_states): no PCIe copy.  They must be complete before the call (it reads them on the
 * ctx's stream). */
int32_t gs_write_splats_device(gs_ctx* ctx, const uint32_t* d_ids, uint64_t m, const void* d_aos320, const uint8_t* d_states,
                               uint32_t parts, uint64_t* written);                                       /* DEVICE pointers */
/* Snapshots.  gs_snapshot_take runs the splat edits' selection ((0, 0): dense, no selection runs and no id list is kept) and
 * gathers the named parts of the matching splats into ONE device allocation of the snapshot's own, compact SoA: the id list, 3 x
 * f32[m] positions, 2 x float4[m] geometry, 12 x float4[m] SH, u8[m] state (sections rounded up to 16 bytes).  Memory follows the
 * parts: a POSITION snapshot of a translate costs 16 B per splat (12 + the index), not 320.  count == 0 is a valid object.
 * gs_snapshot_restore scatters parts back (parts == 0: all that were taken; a part that was not taken is refused) and leaves the
 * snapshot unchanged: it can be applied again.  gs_snapshot_swap exchanges scene and snapshot contents in one pass.  A restored or
 * swapped GS_PART_GEOMETRY also stores the derived largest log-scale, so the ctx equals one freshly uploaded with those records.
 * Validity: a snapshot names splats by index.  Every scene carries a 64-bit serial, drawn from one process-wide counter whenever a
 * scene is installed by gs_upload_*, gs_share_splats or gs_compact; the snapshot stores it, and restore / swap on a ctx whose serial
 * differs -- another ctx, or the same ctx after an upload or a compaction -- are refused with GS_ERR_INVALID_ARGUMENT: the scene
 * was replaced or renumbered.  An insertion KEEPS the serial (old splats keep their indices): a snapshot stays valid across
 * gs_append_* and gs_duplicate_splats and leaves the new splats alone.  Snapshots that survive a compaction are out of scope.
 * Ownership: the snapshot owns its memory and remembers its device; gs_snapshot_free works at any time, also after gs_destroy of
 * the ctx, and gs_destroy frees no snapshot.  gs_snapshot_get_info needs no ctx and makes no GPU call.  *restored / *swapped (may
 * be NULL): the snapshot's count, or 0 when nothing was to be moved. */
typedef struct gs_snapshot gs_snapshot;
typedef struct gs_snapshot_info { uint64_t count, n_at_take, device_bytes; uint32_t parts, dense; } gs_snapshot_info; /* 32 B */
int32_t gs_snapshot_take(gs_ctx* ctx, uint32_t mask, uint32_t value, uint32_t parts, gs_snapshot** out);
int32_t gs_snapshot_restore(gs_ctx* ctx, const gs_snapshot* snapshot, uint32_t parts, uint64_t* restored); /* snapshot -> scene  */
int32_t gs_snapshot_swap(gs_ctx* ctx, gs_snapshot* snapshot, uint32_t parts, uint64_t* swapped);           /* snapshot <-> scene */
int32_t gs_snapshot_get_info(const gs_snapshot* snapshot, gs_snapshot_info* out);
int32_t gs_snapshot_free(gs_snapshot* snapshot);                                                           /* NULL is GS_OK      */

/* ---- coverage: per-splat contribution of the LAST frame, select by what is seen ---------------------
 * gs_state_region selects THROUGH surfaces and gs_pick answers for one pixel at a time; neither can say which splats the user
 * actually SEES in a region, nor that a splat contributes to no pixel of any of a set of views (floaters, buried interior
 * splats, importance scores for decimation).  The coverage planes keep one 16-byte record per resident splat and
 * gs_coverage_accumulate ADDS to them what the last frame shows of a set P of canvas pixels: a rect, optionally AND a
 * u8[height][width] mask (nonzero = inside), intersected with the ctx's slab.  Many views, one accumulation.
 * Every (pixel p in P, entry e of p's tile list) that the blend ACCEPTS contributes to the record of e's gaussian.  Accepted
 * means cond = 1 exactly as gs_pick defines it above: compute_tiles.wgsl:44-66 in the canonical (GS_FLAG_EXACT_BLEND)
 * arithmetic -- one f32 rounding per written operation, the oracle's exp, wg_min -- whatever blend the frame itself used.  The
 * contribution is the entry's weight w = fl(alpha * T), T taken before the entry (0 < w <= 0.99):
 *     sum_q      += (uint32_t)(w * 4294967296.0f)     floor(w 2^32); the product is exact
 *     hits       += 1                                  per accepted (pixel, entry) PAIR, not per pixel: a gaussian can sit twice in
 *                                                      one tile's list (the alias column of write_tile_ids.wgsl:26-31)
 *     max_weight  = max(max_weight, w)
 * Integer adds and a maximum (taken on the bit pattern, w > 0): the planes do not depend on the order in which the device adds,
 * two runs agree bit for bit and a host can restate them exactly (no float sum is involved).  sum_q wraps modulo 2^64 and hits
 * modulo 2^32; neither can happen before 2^32 accepted pairs of ONE splat (sum_q grows by less than 2^32 per pair).
 * The mean weight is sum_q / 2^32 / hits; sum_q / 2^32 is the importance score sum of alpha T.
 * The result is the same for tight and reference binning (a tight list drops only entries no pixel accepts, and an entry whose
 * sub-block bit is clear reaches 1/255 on no pixel of that block), gs_render and gs_render_debug, every GS_OPT_EMIT_ORDER,
 * EXACT and fused frames, direct and graph-replayed frames.  Hidden splats are in no list and get nothing.
 * Ownership: the planes belong to the ctx the calls are made on (the root of a frames-in-flight ring; a borrower of
 * gs_share_splats keeps its own): N x 16 bytes, allocated and zeroed by the first of the four calls below.  They are DROPPED --
 * they read as zero again -- by every gs_upload_*, gs_share_splats and gs_compact (the records are not carried through a
 * compaction), and untouched by state calls and transforms: a host that moves splats resets.  Multi-GPU: every rank accumulates
 * its own slab's pixels; the host adds the planes (sum_q, hits) and takes the maximum (max_weight). */
typedef struct gs_coverage_rec { /* 16 bytes, one per resident splat */
    uint64_t sum_q;      /* sum of floor(w 2^32) over the accepted pairs */
    uint32_t hits;       /* accepted (pixel, entry) pairs */
    float max_weight;    /* largest w; 0 if none */
} gs_coverage_rec;
typedef struct gs_cover_region {
    uint32_t struct_size;    /* = sizeof(gs_cover_region) */
    uint32_t x0, y0, x1, y1; /* canvas pixels [x0, x1) x [y0, y1) */
    const uint8_t* mask;     /* NULL, or host u8[height][width] of the CANVAS, nonzero = inside (copied): P = rect AND mask */
} gs_cover_region;
/* Adds the contribution of the LAST frame enqueued (its ring member, like gs_pick), waiting for it first if it is pending; runs on
 * that member's stream and returns when done.  region NULL = the whole canvas.  *pixels (may be NULL) receives |P| in THIS ctx's
 * slab; a region that misses the slab entirely is GS_OK with *pixels = 0, so a multi-GPU host sends one region to every rank.
 * One wave per 8x8 pixel block that intersects P.  It is not a frame: no tap, statistic, option or captured graph changes.
 * GS_ERR_NO_SCENE before any upload, GS_ERR_NO_FRAME when no frame has been rendered since gs_create / the last upload or
 * compaction, GS_ERR_INVALID_ARGUMENT (the message names the numbers) for a wrong struct_size, x1 > width, y1 > height or an empty
 * rect. */
int32_t gs_coverage_accumulate(gs_ctx* ctx, const gs_cover_region* region, uint64_t* pixels);
/* Zeroes the planes.  Completes all frames enqueued on the ctx's ring first, as the state calls do. */
int32_t gs_coverage_reset(gs_ctx* ctx);
/* The planes in HOST memory, N records in splat order, with gs_state_list's conventions: dst == NULL: only *n (= N) is written
 * (query); cap < N: GS_ERR_INVALID_ARGUMENT, the message names the count needed, nothing is written to dst.  Works on any ctx. */
int32_t gs_coverage_read(gs_ctx* ctx, gs_coverage_rec* dst, uint64_t cap, uint64_t* n);
/* Applies `op` with `bits` exactly as gs_state_region does, to the splats that pass (s & where_mask) == where_value and for which
 *     (hits >= min_hits && max_weight >= min_weight) == (covered != 0)
 * so covered = 0 names everything NOT seen, splats that were never in a list included.  *matched (may be NULL): their number.
 * Needs GS_FLAG_SPLAT_STATE and is refused like the other state calls without it; a NaN or negative min_weight, bits or
 * where_mask above 0xFF or an unknown op: GS_ERR_INVALID_ARGUMENT.  Completes the ring's frames first; one streaming pass over
 * 17 bytes per splat. */
int32_t gs_state_coverage(gs_ctx* ctx, uint32_t min_hits, float min_weight, uint32_t covered, uint32_t where_mask, uint32_t where_value,
                          uint32_t op, uint32_t bits, uint64_t* matched);

/* ---- splat attributes: summarise, histogram, read and select resident splats by VALUE -------------------
 * gs_state_region selects by where a splat is, gs_pick and gs_state_coverage by what a frame shows of it; these select by what a
 * splat IS -- opacity, size, anisotropy, base colour, distance from a point or a plane, accumulated importance -- the histogram
 * with a range slider of every splat editor ("opacity below x", "the largest 1 %", "everything broken"), without the
 * gs_export_splats / host / gs_state_ids round trip (244 B read, 320 B written and a PCIe copy per splat for one float of it).
 * The reference has no counterpart (a viewer).
 * The value v of splat i is ONE f32, defined like the region tests: one rounding per written operation, no contraction, left to
 * right, so that a host can restate it bit for bit.  "Record float k" is float k of the 320-byte record as uploaded (after a
 * gs_transform_splats: as a gs_export_splats would return it):
 *     POS_X / Y / Z      record float 0 / 1 / 2
 *     OPACITY_LOGIT      record float 12, raw: monotonic in the opacity, so a host turns a threshold o into log(o / (1 - o));
 *                        no transcendental runs on the device
 *     LOG_SCALE_MAX      fmaxf(l0, fmaxf(l1, l2)), l = record floats 4, 5, 6 (the upload's own expression for the slab cull's plane)
 *     LOG_SCALE_MIN      fminf(l0, fminf(l1, l2))         fmaxf / fminf: a NaN operand, quiet or signalling, is missing data and the
 *                        result is a NaN only when both are (IEEE 754-2019 maximumNumber / minimumNumber, numpy's fmax / fmin)
 *     LOG_SCALE_SUM      (l0 + l1) + l2                                    the log of the volume
 *     ANISOTROPY         LOG_SCALE_MAX - LOG_SCALE_MIN                     the log of the axis ratio, >= 0
 *     DC_R / G / B       record float 16 / 17 / 18
 *     DIST2              d = position - p[0..2];  (dx dx + dy dy) + dz dz  the SPHERE region's expression
 *     PLANE              ((p[0] x + p[1] y) + p[2] z) + p[3]               p = row 2 of `view`: the projection's depth pv.z
 *     COVER_HITS         (float)hits of the ctx's coverage record
 *     COVER_MAX_WEIGHT   max_weight
 *     COVER_SUM          (float)(uint32_t)(sum_q >> 32) + (float)(uint32_t)sum_q * 0x1p-32f     the importance, sum of alpha T
 * p is ignored by the kinds that do not name it.  The COVER_* kinds read the planes of the ctx the call is made on, allocated and
 * zeroed on first need exactly as gs_state_coverage does.  "Bit for bit" has two exceptions a restating host must know: a NaN that
 * an expression produces or propagates is a NaN on every machine but its sign and payload are open (compare "NaN on both sides");
 * and the sign of a zero that fminf / fmaxf chose between -0 and +0 is unspecified (LOG_SCALE_MIN / MAX, ANISOTROPY).
 * Filter, refusals and ordering are those of the splat edits: (mask, value) as gs_state_count, above 0xFF refused, (0, 0) matches
 * every splat and is accepted on a ctx without GS_FLAG_SPLAT_STATE, any other filter on such a ctx is refused.  Every call first
 * completes all frames enqueued on the ctx's ring, runs on the ctx's stream and returns when done; none is a frame or an upload
 * (taps, statistics, gs_pick, the shadows and a captured graph stay).  GS_ERR_NO_SCENE before any upload; N == 0: zero results,
 * GS_OK.  The three read-only calls work on a borrower of gs_share_splats; gs_state_attr has gs_state_region's rules.  A wrong
 * struct_size, kind >= GS_ATTR_COUNT or a non-finite p of DIST2 / PLANE: GS_ERR_INVALID_ARGUMENT and a message.  Multi-GPU: every
 * rank holds the scene; the scene kinds answer the same on every rank, the COVER_* kinds for the rank's own planes. */
enum { GS_ATTR_POS_X = 0, GS_ATTR_POS_Y, GS_ATTR_POS_Z, GS_ATTR_OPACITY_LOGIT,
       GS_ATTR_LOG_SCALE_MIN, GS_ATTR_LOG_SCALE_MAX, GS_ATTR_LOG_SCALE_SUM, GS_ATTR_ANISOTROPY,
       GS_ATTR_DC_R, GS_ATTR_DC_G, GS_ATTR_DC_B, GS_ATTR_DIST2, GS_ATTR_PLANE,
       GS_ATTR_COVER_HITS, GS_ATTR_COVER_MAX_WEIGHT, GS_ATTR_COVER_SUM, GS_ATTR_COUNT };
typedef struct gs_attr { uint32_t struct_size, kind; float p[4]; } gs_attr;   /* 24 bytes; struct_size = sizeof(gs_attr) */
/* (The record shares its name with the call that fills it, so it is a struct TAG only, not a typedef: C keeps tags and functions
 * in separate name spaces, and C++ reaches the tag through `struct gs_attr_summary` as written below.) */
struct gs_attr_summary { uint64_t matched, nan; float min, max; };  /* 24 bytes */
/* matched: splats that pass the filter; nan: how many of them have a NaN v; min / max over the others, +-inf included, in the
 * total order of the order-preserving map of the bit pattern, k = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000) -- so -0 < +0 and the
 * result does not depend on the order in which the device reduces.  No non-NaN value: min = +inf, max = -inf.  There is no mean:
 * a float sum depends on the order of the adds, and a host can restate every number this layer returns; the pivot an editor
 * wants is the centre of the bounds.  (An EXACT mean, which does not depend on the order, is gs_attr_moments' below.) */
int32_t gs_attr_summary(gs_ctx* ctx, const gs_attr* attr, uint32_t mask, uint32_t value, struct gs_attr_summary* out);
/* counts: HOST u64[bins + 3]: [0, bins) the bins, [bins] below, [bins + 1] above, [bins + 2] NaN; they add up to matched.
 * scale = (float)bins / (hi - lo), once, in f32.  Per matching splat: a NaN v goes to the NaN slot, v < lo below, v >= hi above,
 * otherwise b = (uint32_t)((v - lo) * scale) truncated, then min(b, bins - 1).  (The conversion saturates, and a NaN product --
 * only an infinite scale over a denormal width makes one, for v == lo -- is 0.)  Integer adds only: two runs agree bit for bit.
 * bins outside 1..1024, a non-finite lo or hi, !(lo < hi) or hi - lo not finite in f32: GS_ERR_INVALID_ARGUMENT. */
int32_t gs_attr_histogram(gs_ctx* ctx, const gs_attr* attr, uint32_t mask, uint32_t value, float lo, float hi, uint32_t bins, uint64_t* counts);
/* The values of the matching splats in ascending index order, HOST pointers, gs_state_list's conventions: dst == NULL: only *n
 * (query); cap < *n: GS_ERR_INVALID_ARGUMENT, the message names the count needed, nothing is written.  ids (may be NULL, else cap
 * entries) receives the indices.  (0, 0): dense over 0 .. N, no selection runs.  4 B moved per match where an export moves 320. */
int32_t gs_attr_read(gs_ctx* ctx, const gs_attr* attr, uint32_t mask, uint32_t value, float* dst, uint64_t cap, uint64_t* n, uint32_t* ids);
/* Applies `op` with `bits` exactly as gs_state_region does, to the splats that pass (s & where_mask) == where_value and for which
 *     (v >= lo && v <= hi) == (inside != 0)
 * A NaN v is in no range: inside = 0 with lo = -inf, hi = +inf selects exactly the NaN splats.  A NaN lo or hi is refused,
 * infinite bounds are allowed, lo > hi is a valid empty range.  Needs GS_FLAG_SPLAT_STATE; *matched (may be NULL) as for
 * gs_state_region.  One streaming pass: the state byte and the kind's bytes per splat. */
int32_t gs_state_attr(gs_ctx* ctx, const gs_attr* attr, float lo, float hi, uint32_t inside, uint32_t where_mask, uint32_t where_value,
                      uint32_t op, uint32_t bits, uint64_t* matched);

/* ---- moments: the exact mean and covariance of resident splats by value ---------------------------------------
 * The selections above answer "which splats"; this answers "where is the selection and how does it lie": the centroid as a pivot,
 * the principal axes, an oriented box, the plane to level a capture by.  A float sum depends on the order of the adds and could
 * not be restated, so this is not a float sum: the device accumulates integers and the host rounds ONCE.  The result does not
 * depend on the order, the grid, slabs or borrowers, and a host restates it with rational arithmetic (tests/moments_restate.py).
 * The reference has no counterpart (a viewer).
 * attrs[0 .. n_attrs) are gs_attr values as every attribute call takes them, n_attrs in 1 .. GS_MOMENTS_MAX_ATTRS; the same kind
 * may appear twice.  v_j(i) is attribute j's f32 value of splat i, exactly as gs_attr_read returns it.
 *     matched   the splats that pass (s & mask) == value
 *     counted   the matched splats whose n_attrs values are ALL finite.  A splat with a NaN or an infinity in any of them is left
 *               out of every sum; matched - counted is the number left out
 *     sum[j]    S_j  = sum over the counted splats of v_j
 *     prod[]    P_jl = sum over the counted splats of v_j v_l for j <= l, in the order 00, 01, 02, 11, 12, 22
 * These are sums of REAL numbers: a product of two f32 is exact (at most 48 significant bits), nothing is rounded before the end.
 * A gs_exact holds one of them: hi is the double nearest to the sum, ties to even; lo is the double nearest to (sum - hi).  An
 * exact zero is {+0.0, +0.0}; an entry with j or l >= n_attrs is {+0.0, +0.0} as well.  Nothing overflows: |sum| < 2^31 2^256, and
 * every non-zero term is a multiple of 2^-298, so no subnormal double is involved.
 * How: a finite f32 is m 2^e with an integer |m| < 2^24, a product m 2^e with |m| < 2^48 and e >= -298.  A term is added, with its
 * sign, as three 32-bit chunks into signed 64-bit limbs at bit position e + 298 (twenty limbs per sum); the host propagates the
 * carries into one big integer and rounds that to hi, subtracts hi exactly and rounds the rest to lo -- integer code, no long
 * double, no float add (csrc/gs_exact_sum.h, compiled into the kernel and the host alike).  One streaming pass: 4 B per attribute
 * and splat, 1 B of state with a filter; POS_X / Y / Z are read in place, any other kind is first written densely (4 B more each
 * way).
 * Filter, refusals, drain and ordering are gs_attr_summary's: (0, 0) matches every splat and works on a ctx without
 * GS_FLAG_SPLAT_STATE; the COVER_* kinds read the ctx's own coverage planes; the call works on a borrower of gs_share_splats and is
 * neither a frame nor an upload.  GS_ERR_NO_SCENE before any upload; N == 0: all zeros, GS_OK.  n_attrs outside 1 .. 3, a null
 * pointer, a wrong struct_size, kind >= GS_ATTR_COUNT or a non-finite p of DIST2 / PLANE: GS_ERR_INVALID_ARGUMENT, a message that
 * names the call, and *out untouched.  N >= 2^31 is refused too (a limb could overflow there; no device holds that many splats).
 * gs_moments_host computes the same record from n values per HOST plane, planes[0 .. n_planes): no ctx, no GPU, the same code.
 * state: u8[n], may be NULL when the filter is (0, 0).  For hosts that hold records, and for checking the shared code anywhere. */
#define GS_MOMENTS_MAX_ATTRS 3u
typedef struct gs_exact { double hi, lo; } gs_exact;   /* 16 bytes */
/* (A struct tag only, like gs_attr_summary: the record shares its name with the call that fills it.) */
struct gs_attr_moments { uint64_t matched, counted; gs_exact sum[3]; gs_exact prod[6]; };   /* 160 bytes */
int32_t gs_attr_moments(gs_ctx* ctx, const gs_attr* attrs, uint32_t n_attrs, uint32_t mask, uint32_t value, struct gs_attr_moments* out);
int32_t gs_moments_host(const float* const* planes, uint32_t n_planes, uint64_t n, const uint8_t* state, uint32_t mask, uint32_t value,
                        struct gs_attr_moments* out);

/* ---- neighbourhoods: count the splats within a radius, select by that count ---------------------------------
 * Every selection above asks about one splat at a time; these ask about a splat in relation to the others, which is what a splat
 * editor builds "remove floaters" (fewer than k others within r), "grow / shrink the selection" and a local density on -- without
 * the gs_export_splats / host k-d tree / gs_state_ids round trip.  The reference has no counterpart (a viewer).
 * THE COUNT.  Sources are the splats j with (s_j & src_mask) == src_value, queries the splats i with (s_i & qry_mask) == qry_value.
 * For a query i
 *     c_i = min(limit, #{ j != i : j is a source and d2(i, j) <= r2 })
 *     d = p_j - p_i per component;  d2 = (dx dx + dy dy) + dz dz;  r2 = radius * radius
 * -- the SPHERE region's expression: one f32 rounding per written operation, no contraction, so a host can restate it bit for bit.
 * It is symmetric in i and j (the negation is exact).  The comparison <= is INCLUSIVE.  A splat that is not a query gets 0.  A NaN
 * or infinite coordinate makes every comparison false: such a splat has no neighbours and is nobody's neighbour.  radius = 0 (or
 * one whose square is 0) counts exact duplicates.  Self is excluded by index, not by distance.  The result is an integer and does
 * not depend on the order in which the device visits anything: two runs agree bit for bit; a slab ctx, a borrower and a fresh ctx
 * answer the same.  `limit` saturates the count and lets the device stop early (limit = 1: "has a neighbour").
 * THE PLANE is u32[N] and belongs to the ctx the call is made on (the root of a ring; a borrower of gs_share_splats keeps its own).
 * It is allocated and zeroed by the first of the three calls, overwritten as a whole by gs_neigh_count, and DROPPED -- it reads as
 * zero again -- by every gs_upload_*, gs_share_splats and gs_compact, like the coverage planes.  State calls and transforms leave
 * it untouched: it describes the positions and states at the time of the count, and a host that moves splats counts again.
 * WORK BUDGET.  A radius that puts the scene into one cell of the device's grid makes the candidates N^2.  Before the query pass
 * the call computes `candidates` exactly; above max_candidates (0: GS_NEIGH_DEFAULT_CANDIDATES) it returns GS_ERR_CAPACITY with
 * both numbers in the message and leaves the plane as it was.  The query pass is issued in slices of whole workgroups (256
 * queries) of at most GS_NEIGH_SLICE_CANDIDATES candidates each (one workgroup where a single one exceeds that), so that no launch
 * is long.  The two constants come from the measured candidate rate (profiles/neighbours.txt): what finishes in 1 s and in 50 ms.
 * Prologue, ordering and refusals are those of the splat attributes: each (mask, value) as gs_state_count, above 0xFF refused,
 * (0, 0) matches every splat and is accepted on a ctx without GS_FLAG_SPLAT_STATE, any other filter on such a ctx is refused.
 * Every call first completes all frames enqueued on the ctx's ring, runs on the ctx's stream and returns when done; none is a
 * frame or an upload (taps, statistics, gs_pick, the shadows and a captured graph stay).  GS_ERR_NO_SCENE before any upload;
 * N == 0: zero results, GS_OK.  gs_neigh_count and gs_neigh_read work on a borrower; gs_state_neigh has gs_state_region's rules.
 * A wrong struct_size, a radius that is negative or not finite, a radius * radius that is not finite in f32, limit == 0 or
 * reserved != 0: GS_ERR_INVALID_ARGUMENT and a message that names the number. */
#define GS_NEIGH_DEFAULT_CANDIDATES (1ull << 38) /* 0.93 s at the measured 2.95e11 candidates / s */
#define GS_NEIGH_SLICE_CANDIDATES (1ull << 33)   /* 29 ms */
typedef struct gs_neigh {          /* 40 bytes */
    uint32_t struct_size;          /* = sizeof(gs_neigh) */
    float    radius;               /* finite, >= 0; r2 = radius * radius, ONE f32 product, must be finite */
    uint32_t limit;                /* 1 .. 2^32-1: counts saturate here, the device may stop at it */
    uint32_t src_mask, src_value;  /* SOURCES: splats j with (s_j & src_mask) == src_value */
    uint32_t qry_mask, qry_value;  /* QUERIES: splats i with (s_i & qry_mask) == qry_value */
    uint32_t reserved;             /* 0 */
    uint64_t max_candidates;       /* work budget, 0 = GS_NEIGH_DEFAULT_CANDIDATES */
} gs_neigh;
typedef struct gs_neigh_info {     /* 40 bytes */
    uint64_t queried, sources;     /* splats that pass the two filters */
    uint64_t candidates;           /* sum over the queries of the sources in the 27 cells around them, self included */
    uint32_t cells[3]; float cell_edge; /* the grid that was used (diagnostic; no result depends on it) */
} gs_neigh_info;
/* Counts into the plane.  info (may be NULL) is written whenever the grid was built, also when the budget refuses the call. */
int32_t gs_neigh_count(gs_ctx* ctx, const gs_neigh* q, gs_neigh_info* info);
/* The plane in HOST memory, N counts in splat order, with gs_coverage_read's conventions: dst == NULL: only *n (= N) is written
 * (query); cap < N: GS_ERR_INVALID_ARGUMENT, the message names the count needed, nothing is written to dst. */
int32_t gs_neigh_read(gs_ctx* ctx, uint32_t* dst, uint64_t cap, uint64_t* n);
/* Applies `op` with `bits` exactly as gs_state_region does, to the splats that pass (s & where_mask) == where_value and for which
 *     (c >= min_count && c <= max_count) == (inside != 0)
 * min_count > max_count is a valid empty range.  Needs GS_FLAG_SPLAT_STATE; *matched (may be NULL) as for gs_state_region.  One
 * streaming pass over 5 bytes per splat. */
int32_t gs_state_neigh(gs_ctx* ctx, uint32_t min_count, uint32_t max_count, uint32_t inside, uint32_t where_mask, uint32_t where_value,
                       uint32_t op, uint32_t bits, uint64_t* matched);

/* ---- clusters: label the splats that are connected within a radius, select by cluster ------------------------
 * A neighbour count is a local answer.  "Select the whole object I clicked on", "delete every island smaller than 200 splats" and
 * "keep only the main body" are global ones: a detached blob of floaters is dense inside and survives every count.  These calls
 * label the connected components on the device, with the neighbourhoods' grid, distance expression, work budget and slices.
 * THE DEFINITION.  MEMBERS are the splats i with (s_i & mask) == value (gs_state_count's filter).  Two members i != j are LINKED when
 *     d2(i, j) <= r2;   d = p_j - p_i per component;  d2 = (dx dx + dy dy) + dz dz;  r2 = radius * radius
 * -- the neighbourhoods' expression with nothing changed: one f32 rounding per written operation, no contraction, r2 ONE f32
 * product, the comparison <= INCLUSIVE.  A member with a NaN or infinite coordinate is linked to nobody.  A CLUSTER is a connected
 * component of that graph.  For every resident splat i
 *     member:                                label[i] = the smallest splat index in i's cluster,  size[i] = its members (>= 1)
 *     member with a non-finite coordinate:   label[i] = i (a singleton),                          size[i] = 1
 *     non-member:                            label[i] = GS_CLUSTER_NONE,                          size[i] = 0
 * Both planes are integers and depend on nothing but the positions, the state bytes and the radius: two runs, a slab ctx, a
 * borrower of gs_share_splats, a fresh ctx and a brute-force host restatement agree bit for bit.  radius = 0 (or one whose square
 * is 0) clusters exact duplicates.
 * THE PLANES are u32[N] each and belong to the ctx the call is made on (the root of a ring; a borrower keeps its own), like the
 * count plane.  They are allocated by the first call that needs them and read label = GS_CLUSTER_NONE, size = 0 before the first
 * labelling; gs_cluster_label overwrites both as a whole; they are DROPPED -- they read as before the first labelling again -- by
 * every gs_upload_*, gs_share_splats and gs_compact.  State calls and transforms leave them untouched: they describe the
 * positions and states at the time of the labelling, and a host that moves or re-filters splats labels again.
 * WORK.  A labelling builds the neighbourhoods' grid over the members, then runs ROUNDS: an edge pass over the candidates (a
 * concurrent union-find: each linked pair hooks the larger of its two roots under the smaller) followed by a pass that flattens the
 * trees, until a whole edge pass hooked nothing; one round does the work, the next one proves it.  max_candidates (0:
 * GS_NEIGH_DEFAULT_CANDIDATES) is the budget of ONE round: above it the call returns GS_ERR_CAPACITY with both numbers in the
 * message.  Every edge pass is issued in slices of at most GS_NEIGH_SLICE_CANDIDATES, as a count's query pass.  More than
 * GS_CLUSTER_MAX_ROUNDS rounds: GS_ERR_DEVICE_FAULT with the count in the message (unreachable; the bound that keeps the call
 * from running away).  A call that fails for any reason -- budget, allocation, round cap -- leaves both planes as they were.
 * Prologue, ordering and refusals are the neighbourhoods': the filter as gs_state_count, above 0xFF refused, (0, 0) matches every
 * splat and is accepted on a ctx without GS_FLAG_SPLAT_STATE, any other filter on such a ctx is refused.  Every call first
 * completes all frames enqueued on the ctx's ring, runs on the ctx's stream and returns when done; none is a frame or an upload.
 * GS_ERR_NO_SCENE before any upload; N == 0: zero results, GS_OK.  gs_cluster_label and gs_cluster_read work on a borrower; the
 * two state calls need GS_FLAG_SPLAT_STATE and have gs_state_region's rules (bits / where_mask / seed_mask above 0xFF and an
 * unknown op are refused, nothing is applied).  A wrong struct_size, a radius that is negative or not finite, a radius * radius
 * that is not finite in f32 or reserved != 0: GS_ERR_INVALID_ARGUMENT and a message that names the number. */
#define GS_CLUSTER_NONE 0xFFFFFFFFu
#define GS_CLUSTER_MAX_ROUNDS 64u
typedef struct gs_cluster {        /* 32 bytes */
    uint32_t struct_size;          /* = sizeof(gs_cluster) */
    float    radius;               /* finite, >= 0; r2 = radius * radius must be finite in f32 */
    uint32_t mask, value;          /* MEMBERS: splats i with (s_i & mask) == value */
    uint32_t reserved[2];          /* 0 */
    uint64_t max_candidates;       /* work budget PER ROUND, 0 = GS_NEIGH_DEFAULT_CANDIDATES */
} gs_cluster;
typedef struct gs_cluster_info {   /* 56 bytes */
    uint64_t members;              /* splats that pass the filter */
    uint64_t clusters;             /* members whose label is their own index */
    uint64_t largest;              /* the maximum of size */
    uint64_t candidates;           /* distance tests of one round: the members in the 27 cells around every member, self included */
    uint32_t rounds;               /* edge passes that were run */
    uint32_t cells[3]; float cell_edge; /* the grid that was used (diagnostic; no result depends on it) */
    uint32_t reserved;
} gs_cluster_info;
/* Labels into the two planes.  info (may be NULL) is written whenever the grid was built, also when the budget refuses the call
 * (members, candidates and the grid; clusters, largest and rounds are those of a completed labelling). */
int32_t gs_cluster_label(gs_ctx* ctx, const gs_cluster* q, gs_cluster_info* info);
/* The planes in HOST memory, N words each in splat order, with gs_neigh_read's conventions: labels and sizes may each be NULL, both
 * NULL: only *n (= N) is written (query); cap < N: GS_ERR_INVALID_ARGUMENT, the message names the count needed, nothing is written. */
int32_t gs_cluster_read(gs_ctx* ctx, uint32_t* labels, uint32_t* sizes, uint64_t cap, uint64_t* n);
/* Applies `op` with `bits` exactly as gs_state_region does, to the splats that pass (s & where_mask) == where_value and for which
 *     (size >= min_size && size <= max_size) == (inside != 0)
 * -- the plain expression on the plane value, so a non-member's 0 takes part, as in gs_state_neigh (whose pass this is, over the
 * size plane).  min_size > max_size is a valid empty range.  *matched (may be NULL) as for gs_state_region. */
int32_t gs_state_cluster(gs_ctx* ctx, uint32_t min_size, uint32_t max_size, uint32_t inside, uint32_t where_mask, uint32_t where_value,
                         uint32_t op, uint32_t bits, uint64_t* matched);
/* Applies `op` with `bits` to the splats that pass `where`, have label != GS_CLUSTER_NONE and whose cluster holds at least one
 * splat that passes (s & seed_mask) == seed_value as the state plane is NOW; the labels are those of the last labelling.  Two
 * passes: every seed sets the flag word of its label, then the state pass reads the flag of every splat's label. */
int32_t gs_state_cluster_linked(gs_ctx* ctx, uint32_t seed_mask, uint32_t seed_value, uint32_t where_mask, uint32_t where_value,
                                uint32_t op, uint32_t bits, uint64_t* matched);

/* ---- nearest neighbours: the k-th nearest distance and the nearest id per splat ------------------------------
 * A count and a labelling make the caller know a radius first, and a radius is a property of one capture's scale and density.
 * Statistical outlier removal ("my k-th nearest neighbour is further away than most splats' k-th nearest neighbour"), the local
 * spacing an editor shows, the initial scale of inserted points and, with the nearest splat's id, de-duplication after a merge
 * need the DISTANCE instead -- without the gs_export_splats / host k-d tree / gs_state_ids round trip.  The reference has no
 * counterpart (a viewer).
 * THE DEFINITION.  Sources are the splats j with (s_j & src_mask) == src_value, queries the splats i with (s_i & qry_mask) ==
 * qry_value.  With the neighbourhoods' expression unchanged
 *     d = p_j - p_i per component;  d2 = (dx dx + dy dy) + dz dz;  r2 = radius * radius
 * -- one f32 rounding per written operation, no contraction, r2 ONE f32 product, the comparison <= INCLUSIVE -- let, for a query i,
 *     D_i = the multiset { d2(i, j) : j a source, j != i, d2(i, j) <= r2 }.
 * Self is excluded by index, not by distance.  A NaN or infinite coordinate fails every comparison: such a splat has no neighbours
 * and is nobody's.  Then
 *     dist2[i]   = the k-th smallest element of D_i, or +inf (0x7F800000) when D_i has fewer than k elements: UNRESOLVED;
 *     nearest[i] = the smallest index j among the sources that attain min D_i (the TIE RULE: d2 first, then the smaller id), or
 *                  GS_KNN_NONE (0xFFFFFFFF) when D_i is empty;
 *     a splat that is not a query reads dist2 = NaN with exactly the bits 0x7FC00000 and nearest = GS_KNN_NONE.
 * Both numbers are functions of a multiset and of a total order (d2, then id): nothing depends on the order in which the device
 * visits anything, and a square is never -0, so the planes compare by bit pattern: two runs, a slab ctx, a borrower of
 * gs_share_splats, a fresh ctx and a brute-force host restatement agree bit for bit.  Exact duplicates have dist2 = +0.0.
 * RADIUS-INDEPENDENCE, the property the design rests on: a RESOLVED dist2[i] (finite) and, for k = 1, its nearest[i] DO NOT DEPEND
 * ON THE RADIUS.  D_i holds every source within r and nothing beyond, so when it has k elements its k-th smallest is the k-th
 * smallest over ALL sources (any source outside r is further than all of them), and its minimum with the tie rule is the nearest
 * source among all.  Only WHETHER a query is resolved depends on the radius.  (For k > 1 the nearest of an unresolved query with a
 * non-empty D_i is already the true nearest source, for the same reason.)  This is also why one grid pass suffices: everything
 * within r is in the 27 cells around the query, and nothing beyond r is accepted.
 * REFINE.  With GS_KNN_REFINE the queries are further restricted to the splats whose dist2 reads +inf NOW, only their two entries
 * are written and every other entry keeps its value; queried and unresolved count this call's queries only.  A host that doubles
 * the radius while unresolved > 0 therefore ends with the planes of a single search at the last radius, for the price of the
 * sparse remainder.  Refused (GS_ERR_INVALID_ARGUMENT) when k differs from the k of the last search without the flag on this ctx,
 * or when there has been none since the planes were last dropped.
 * THE PLANES are f32[N] (dist2) and u32[N] (nearest) and belong to the ctx the call is made on (the root of a ring; a borrower
 * keeps its own), like the count plane.  They are allocated by the first call that needs them and read NaN / GS_KNN_NONE before
 * the first search; gs_knn_search without GS_KNN_REFINE overwrites both as a whole; they are DROPPED -- they read as before the
 * first search again -- by every gs_upload_*, gs_share_splats and gs_compact, whatever drops the count plane and nothing else.
 * State calls and transforms leave them untouched: they describe the positions and states at the time of the search, and a host
 * that moves or re-filters splats searches again.  A call that fails for any reason -- budget, allocation, a refused argument --
 * leaves both planes as they were.
 * WORK.  A search builds the neighbourhoods' grid over the sources at the radius given, computes `candidates` exactly and, above
 * max_candidates (0: GS_NEIGH_DEFAULT_CANDIDATES), returns GS_ERR_CAPACITY with both numbers in the message; the query pass is
 * issued in the count's slices (GS_NEIGH_SLICE_CANDIDATES).  Per query the device keeps the k smallest accepted d2 (k <=
 * GS_KNN_MAX_K) and the (d2, id) minimum.  Measured rates: profiles/nearest.txt.
 * Prologue, ordering and refusals are the neighbourhoods': each (mask, value) as gs_state_count, above 0xFF refused, (0, 0)
 * matches every splat and is accepted on a ctx without GS_FLAG_SPLAT_STATE, any other filter on such a ctx is refused.  Every call
 * first completes all frames enqueued on the ctx's ring, runs on the ctx's stream and returns when done; none is a frame or an
 * upload (taps, statistics, gs_pick, the shadows and a captured graph stay).  GS_ERR_NO_SCENE before any upload; N == 0: zero
 * results, GS_OK.  gs_knn_search and gs_knn_read work on a borrower; gs_state_knn has gs_state_region's rules.  A wrong
 * struct_size, a radius that is negative or not finite, a radius * radius that is not finite in f32, k outside 1 .. GS_KNN_MAX_K,
 * unknown flag bits or reserved != 0: GS_ERR_INVALID_ARGUMENT and a message that names the number. */
#define GS_KNN_MAX_K 32u
#define GS_KNN_NONE 0xFFFFFFFFu
#define GS_KNN_REFINE 0x1u         /* gs_knn.flags: only the splats whose dist2 reads +inf now are queried and written */
typedef struct gs_knn {            /* 48 bytes */
    uint32_t struct_size;          /* = sizeof(gs_knn) */
    float    radius;               /* finite, >= 0; r2 = radius * radius, ONE f32 product, must be finite */
    uint32_t k;                    /* 1 .. GS_KNN_MAX_K */
    uint32_t flags;                /* GS_KNN_REFINE or 0 */
    uint32_t src_mask, src_value;  /* SOURCES: splats j with (s_j & src_mask) == src_value */
    uint32_t qry_mask, qry_value;  /* QUERIES: splats i with (s_i & qry_mask) == qry_value */
    uint64_t max_candidates;       /* work budget, 0 = GS_NEIGH_DEFAULT_CANDIDATES */
    uint64_t reserved;             /* 0 */
} gs_knn;
typedef struct gs_knn_info {       /* 48 bytes */
    uint64_t queried, sources;     /* splats that pass the two filters (queried: and, refining, read +inf) */
    uint64_t candidates;           /* sum over the queries of the sources in the 27 cells around them, self included */
    uint64_t unresolved;           /* queries that end with dist2 = +inf, those with a non-finite coordinate included */
    uint32_t cells[3]; float cell_edge; /* the grid that was used (diagnostic; no result depends on it) */
} gs_knn_info;
/* Searches into the two planes.  info (may be NULL) is written whenever the grid was built, also when the budget refuses the call
 * (queried, sources, candidates and the grid; unresolved is that of a completed search). */
int32_t gs_knn_search(gs_ctx* ctx, const gs_knn* q, gs_knn_info* info);
/* The planes in HOST memory, N values each in splat order, with gs_cluster_read's conventions: dist2 and nearest may each be NULL,
 * both NULL: only *n (= N) is written (query); cap < N: GS_ERR_INVALID_ARGUMENT, the message names the count needed, nothing is
 * written. */
int32_t gs_knn_read(gs_ctx* ctx, float* dist2, uint32_t* nearest, uint64_t cap, uint64_t* n);
/* Applies `op` with `bits` exactly as gs_state_region does, to the splats that pass (s & where_mask) == where_value and for which
 *     (v >= lo && v <= hi) == (inside != 0),   v = dist2
 * -- gs_state_attr's rule.  A NaN is in no range, so a splat that was no query is never selected with inside = 1; hi = +inf
 * includes the unresolved.  A NaN lo or hi is refused, infinite bounds are allowed, lo > hi is a valid empty range.  Needs
 * GS_FLAG_SPLAT_STATE; *matched (may be NULL) as for gs_state_region.  One streaming pass over 5 bytes per splat. */
int32_t gs_state_knn(gs_ctx* ctx, float lo, float hi, uint32_t inside, uint32_t where_mask, uint32_t where_value, uint32_t op, uint32_t bits,
                     uint64_t* matched);

/* ---- registration: the exact sums over matched pairs that a rigid or similarity fit needs --------------------
 * A splat insertion puts a second capture behind the resident one; bringing it ONTO the first needs, per step of a point-to-point
 * ICP, sums over PAIRS (p_i, q_i = p_j), j the partner of i: the two centroids, the 3x3 cross-covariance and the two spreads.
 * gs_attr_moments cannot give them (it never gathers a second splat); this call does, with the moments' arithmetic: the device
 * adds integers, the host rounds ONCE, nothing depends on the grid, the order, slabs or borrowers, and a host restates every sum
 * with rational arithmetic (tests/pairs_restate.py).  The reference has no counterpart (a viewer).
 *     matched   the splats i that pass (s_i & mask) == value
 *     j         partner[i]; with partner == NULL, the ctx's own `nearest` plane as gs_knn_read would return it now (a plane that
 *               was never searched or has been dropped reads GS_KNN_NONE everywhere: all zeros, GS_OK)
 *     paired    the matched i for which ALL of these hold:
 *                 j < N (GS_KNN_NONE and any other id >= N count as unpaired: never read, never an error);
 *                 all six coordinates of p = p_i and q = p_j are finite;
 *                 d2 <= max_dist2 with the neighbourhoods' expression on the positions as they are NOW: d = q - p per component,
 *                 d2 = (dx dx + dy dy) + dz dz, one f32 rounding per operation, no contraction, the comparison INCLUSIVE.  A d2
 *                 that overflows to +inf passes only max_dist2 = +inf.
 *               j == i is allowed; the partner's state byte is not looked at.
 *     sum_p[a], sum_q[a]   the sums over the paired splats of p_a and of q_a
 *     pq[3 a + b]          ... of p_a q_b (row-major)
 *     pp[a], qq[a]         ... of p_a^2 and of q_a^2
 * Sums of REAL numbers, each finished once into a gs_exact exactly as in the moments section; an exact zero is {+0.0, +0.0}.
 * One streaming pass: 16 B per splat (12 of position, 4 of partner id), 1 B of state with a filter, and a gather of 12 scattered
 * bytes for every matched splat whose partner is below N.  A HOST partner array is first copied to the device (4 B per splat).
 * Filter, refusals, drain and ordering are gs_attr_moments': the filter as gs_state_count, (0, 0) works on a ctx without
 * GS_FLAG_SPLAT_STATE; the call completes the ring's frames first, runs on the ctx's stream and is neither a frame nor an upload;
 * it works on a borrower of gs_share_splats and then reads THAT ctx's nearest plane.  GS_ERR_NO_SCENE before any upload; N == 0:
 * all zeros, GS_OK.  N >= 2^31, a NaN or negative max_dist2 or a null out: GS_ERR_INVALID_ARGUMENT, a message that names the call,
 * and *out untouched.
 * gs_pair_moments_host runs the same loop (csrc/gs_pair_host.h) on n values per HOST plane: no ctx, no GPU, the same code.
 * partner: u32[n], required when n > 0; state: u8[n], may be NULL when the filter is (0, 0). */
/* (A struct tag only, like gs_attr_moments: the record shares its name with the call that fills it.) */
struct gs_pair_moments {            /* 352 bytes */
    uint64_t matched, paired;
    gs_exact sum_p[3], sum_q[3];    /* sum of p_a, of q_a */
    gs_exact pq[9];                 /* sum of p_a q_b, row-major (a, b) */
    gs_exact pp[3], qq[3];          /* sum of p_a^2, of q_a^2 */
};
int32_t gs_pair_moments(gs_ctx* ctx, uint32_t mask, uint32_t value, const uint32_t* partner /* HOST u32[N] or NULL */, float max_dist2,
                        struct gs_pair_moments* out);
int32_t gs_pair_moments_host(const float* px, const float* py, const float* pz, uint64_t n, const uint32_t* partner, const uint8_t* state,
                             uint32_t mask, uint32_t value, float max_dist2, struct gs_pair_moments* out);

/* Point-to-plane.  The point metric pulls every moving splat towards ONE fixed splat; on walls and floors sampled at different places
 * the tangential part of each pair is sampling noise.  The plane metric penalises only the distance of p to the tangent plane of its
 * partner, r = n . (q - p); its linearised normal equations over (omega, t) are sum g g^T x = sum g r with g = ((p - pivot) x n, n).
 * gs_pair_plane_moments gives those sums exactly, with the arithmetic above; gsplat.register.fit_plane solves them in rational
 * arithmetic.  n is the partner's normal: gs_surface_estimate over the FIXED splats, once -- they do not move during an alignment.
 * A matched splat i (filter as above) with p = p_i, j = partner[i], q = p_j, n = normal[j] forms in f32, one rounding per written
 * operation, no contraction:
 *     u_a = p_a - pivot_a                       a = x, y, z
 *     d_a = q_a - p_a,  d2 = (dx dx + dy dy) + dz dz          (gs_pair_moments' d and d2)
 *     r   = (nx dx + ny dy) + nz dz             the signed distance of p to q's tangent plane
 *     cx  = uy nz - uz ny;  cy = uz nx - ux nz;  cz = ux ny - uy nx
 *     g   = (cx, cy, cz, nx, ny, nz)
 * It is PAIRED when j < N, gs_pair_moments' acceptance holds (six finite coordinates, d2 <= max_dist2 inclusive, an overflowed d2
 * passing only +inf), nx, ny, nz are finite (an unresolved or never-estimated normal is NaN 0x7FC00000) and cx, cy, cz, r are
 * finite.  Only paired splats enter the 29 sums, each a gs_exact finished once:
 *     G[21]   the upper triangle of sum g g^T, row-major (00, 01, .., 05, 11, .., 55)
 *     h[6]    sum g_k r
 *     rr      sum r r
 *     d2      sum of the f32 value d2 (a d2 of +inf, possible only with max_dist2 = +inf, counts as what its bit pattern splits
 *             into, 2^128)
 * Every term but d2's is the exact product of two f32.  The 480 bytes do not depend on the grid, the order, slabs or borrowers; a
 * host restates them with rational arithmetic (tests/plane_pairs_restate.py).
 * partner: HOST u32[N], or NULL for the ctx's nearest plane.  normal: HOST f32[N][3], or NULL for the ctx's surface normal plane in
 * place (never estimated or dropped: it reads NaN, nothing pairs, GS_OK).  Host arrays are first copied to the device (4 and 16 B per
 * splat).  One streaming pass of 16 B per splat and a gather of 12 + 16 scattered bytes per matched splat with j < N.  Filter,
 * drain, stream and refusals are gs_pair_moments'; also refused: a null pivot, a pivot component that is not finite.  A failed call
 * leaves *out untouched.  gs_pair_plane_moments_host runs the same loop (csrc/gs_plane_pair_host.h) on host planes; partner and
 * normal are required when n > 0. */
struct gs_pair_plane_moments {      /* 480 bytes */
    uint64_t matched, paired;
    gs_exact G[21];                 /* upper triangle of sum g g^T, row-major */
    gs_exact h[6];                  /* sum g_k r */
    gs_exact rr, d2;                /* sum r^2, sum d2 */
};
int32_t gs_pair_plane_moments(gs_ctx* ctx, uint32_t mask, uint32_t value, const uint32_t* partner /* HOST u32[N] or NULL */,
                              const float* normal /* HOST f32[N][3] or NULL */, const float pivot[3], float max_dist2,
                              struct gs_pair_plane_moments* out);
int32_t gs_pair_plane_moments_host(const float* px, const float* py, const float* pz, uint64_t n, const uint32_t* partner,
                                   const float* normal /* f32[n][3] */, const uint8_t* state, uint32_t mask, uint32_t value,
                                   const float pivot[3], float max_dist2, struct gs_pair_plane_moments* out);

/* ---- consensus: score many plane or ball hypotheses in one pass; the plane through three points --------------
 * gsplat.moments fits the least-squares plane through a selection that exists; FINDING the floor, a wall or a table top in an
 * unselected, cluttered capture is a robust fit (RANSAC): many candidate planes, each scored by how many splats lie within a distance
 * of it, the best kept.  One gs_attr_histogram or gs_state_attr pass per candidate streams the scene once per candidate; this call
 * streams it ONCE for up to GS_CONSENSUS_MAX candidates.  With GS_ATTR_DIST2 the same call answers "where is the densest ball of
 * radius r?" (the main object; a coarse seed for the registration).  The reference has no counterpart (a viewer).
 *     counts[j]  the number of splats i with (s_i & mask) == value and lo <= v_j(i) && v_j(i) <= hi, both ends INCLUSIVE
 *     v_j(i)     the GS_ATTR_PLANE or GS_ATTR_DIST2 value of splat i (splat attributes, above) with p = params[4 j .. 4 j + 3]:
 *                PLANE ((p[0] x + p[1] y) + p[2] z) + p[3];  DIST2 d = position - p[0..2], (dx dx + dy dy) + dz dz, p[3] ignored --
 *                one f32 rounding per operation, no contraction, so a host restates every count (tests/consensus_restate.py)
 *     *matched   (may be NULL) the splats that pass the filter
 * The expression is the whole rule.  Unlike a gs_attr, the parameters need NOT be finite: a NaN parameter or coordinate makes v a NaN,
 * a NaN is in no range, the splat is not counted for that hypothesis.  lo > hi is a valid empty range (every count 0); infinite lo and
 * hi are allowed.  Counts are integers: they do not depend on the grid, the order, slabs or borrowers, and two runs agree bit for bit.
 * params, counts and matched are HOST pointers: f32[h][4], u64[h], u64.
 * Filter, drain, ordering, borrowers and slabs are gs_attr_summary's: (mask, value) as gs_state_count, above 0xFF refused, (0, 0)
 * matches every splat and works on a ctx without GS_FLAG_SPLAT_STATE; the call completes the ring's frames first, runs on the ctx's
 * stream, returns when done and is neither a frame nor an upload.  GS_ERR_NO_SCENE before any upload; N == 0: all zeros, GS_OK.  A NaN
 * lo or hi, h outside 1 .. GS_CONSENSUS_MAX, a kind other than GS_ATTR_PLANE / GS_ATTR_DIST2, null params or counts:
 * GS_ERR_INVALID_ARGUMENT, a message that names the call, nothing written.
 * gs_consensus_host runs the same loop (csrc/gs_consensus_host.h) over n values per HOST plane: no ctx, no GPU, the same code.  state:
 * u8[n], may be NULL when the filter is (0, 0).  Its refusals are the same; n == 0 gives zeros. */
#define GS_CONSENSUS_MAX 4096u
int32_t gs_attr_consensus(gs_ctx* ctx, uint32_t kind, const float* params, uint32_t h, float lo, float hi, uint32_t mask, uint32_t value,
                          uint64_t* counts, uint64_t* matched);
int32_t gs_consensus_host(const float* px, const float* py, const float* pz, uint64_t n, const uint8_t* state, uint32_t mask, uint32_t value,
                          uint32_t kind, const float* params, uint32_t h, float lo, float hi, uint64_t* counts, uint64_t* matched);
/* The values of m GIVEN splats, in any order, repeats allowed: dst[g] = the value of splat ids[g] exactly as gs_attr_read returns it
 * (every kind; the COVER_* kinds read the ctx's planes as the other attribute calls do).  ids and dst are HOST pointers.  The ids are
 * checked before anything is launched: an id >= N is GS_ERR_INVALID_ARGUMENT, the message names the index, nothing is written.  m == 0:
 * GS_OK.  4 B up and 4 B down per id, in trips through the ctx's scratch.  Drain and ordering as gs_attr_read. */
int32_t gs_attr_gather(gs_ctx* ctx, const gs_attr* attr, const uint32_t* ids, uint64_t m, float* dst);
/* Host only (no ctx, no GPU): the plane through each of h point triples, points f32[h][9] = (a, b, c) in the order given, as
 * GS_ATTR_PLANE parameters, params f32[h][4].  Everything in DOUBLE, one rounding per operation as written, no contraction:
 *     u = b - a,  w = c - a
 *     n = (u1 w2 - u2 w1,  u2 w0 - u0 w2,  u0 w1 - u1 w0)
 *     len = sqrt((n0 n0 + n1 n1) + n2 n2)
 *     m = n / len                                       (three divisions)
 *     d = -((m0 a0 + m1 a1) + m2 a2)
 * Sign: if the component of m with the largest magnitude -- the FIRST such component on a tie -- is negative, m and d are negated.
 * params = (m0, m1, m2, d), each rounded to f32.  If len is not finite or not greater than 0 (a repeated point, collinear points, a
 * non-finite coordinate) all four are NaN: such a hypothesis counts nothing in gs_attr_consensus, so a sampler needs no special case.
 * h == 0: GS_OK; null points or params with h > 0: GS_ERR_INVALID_ARGUMENT. */
int32_t gs_planes_through(const float* points, uint32_t h, float* params);

/* ---- cell merge: one moment-matched splat per grid cell ---------------------------------------------------------
 * Every edit above keeps or drops splats; this one makes FEWER of them without punching holes: the splats of one cell of a uniform
 * grid become one splat with their weighted mean, covariance and colour (decimation by merging; gsplat.simplify builds "simplify the
 * scene to a tenth" on it with gs_append_splats_device and gs_compact).  The reference has no counterpart (a viewer).
 * All f32 operations take one rounding per written operation, no contraction; all f64 operations are plain + - *, only the finishing
 * uses /, sqrt and log.  The whole definition is compiled from one header, csrc/gs_merge_math.h, by the kernels and the host twin.
 * PER SPLAT i (f32; record floats: position 0..2, log-scales 4..6, rot 8..11, opacity logit 12, SH 16..63):
 *     a_i      the projection's sigmoid of the logit (process_gaussians.wgsl:282-294, both branches, gs_exp)
 *     sigma_k  gs_exp(s_k)
 *     Sig_i    the six entries xx xy xz yy yz zz of the projection's 3D covariance with scale modifier 1 (:127-162: normalised
 *              quaternion, M = S R, transpose(M) M), the same expression tree
 *     A_i      max(sigma0 sigma1, max(sigma0 sigma2, sigma1 sigma2)), max(a, b) = a < b ? b : a: the cross-section of the two largest
 *              axes, so a flat surfel weighs by its area
 *     w_i      a_i * A_i
 * ELIGIBLE: (s_i & mask) == value, a finite position, w_i finite and > 0, six finite Sig_i entries.  Everything else is never grouped,
 * marked or changed.
 * GRID: the bounds are those of the splats that pass the filter with a finite position (the neighbourhoods' bounds pass); the cell
 * coordinate and key are the neighbourhoods' (clamp((int)floorf((x - lo) * inv_h), 0, g - 1), x lowest); the edge is `cell` itself,
 * raised to widest / 1024 * 1.000001 (double, rounded to f32) when an axis would hold more than 1024 cells; info.cell_edge reports it.
 * GROUPS: the eligible splats of one cell in ascending index.  A cell with at least min_members (>= 2) is MERGED; merged groups are
 * numbered 0 .. G-1 in ascending cell key.  If the fullest cell holds more than max_members (0: GS_MERGE_DEFAULT_MAX_MEMBERS) the call
 * returns GS_ERR_CAPACITY with the edge in the message before anything is written: the loop over a group's members is sequential.
 * SUMS: GS_MERGE_SUM_DOUBLES doubles per merged group, from 0.0 over the members in ascending index; c = the position of the member
 * with the smallest index, as double; d = (double)p - c; w as double:
 *     [0] W += w   [1..3] S_k += w * d_k   [4..9] M_kl: t = d_k * d_l; t = (double)Sig_kl + t; t = w * t; M_kl += t  (xx xy xz yy yz zz)
 *     [10..57] H_j += w * (double)sh_j, j = 3 * coefficient + channel (record float 16 + 4 * coefficient + channel)
 *     [58] members   [59] first index   [60..62] c   [63] 0
 * FINISHING (f64): mu = S / W; position = (float)(c + mu); C_kl = M_kl / W - mu_k * mu_l; eigenvalues l1 >= l2 >= l3 of C by a fixed
 * number of cyclic Jacobi sweeps, each floored to 1e-30; log-scales (float)(0.5 * ln l_k), largest first; the eigenvectors are the
 * columns of a rotation (the third flipped when the determinant is negative), the quaternion (r, x, y, z) has unit norm and r >= 0;
 * A' = sqrt(l1 * l2), alpha' = min(0.99, W / A'), logit = (float)ln(alpha' / (1 - alpha')): opacity x area is conserved, k coincident
 * copies of a splat merge into that splat with opacity min(0.99, k a); SH'_j = (float)(H_j / W) (world frame: no rotation); the
 * padding floats are 0.  The sums are pinned bit for bit; the records up to the last places of /, sqrt and log.
 * THE CALLS.  gs_cell_merge writes G records of GS_SPLAT_RECORD_BYTES in group order to HOST memory, gs_cell_merge_device to DEVICE
 * memory; sums (double[G][64]) and group_of (u32[N]: the group's number or GS_MERGE_NONE) are HOST pointers and may be NULL; info may
 * be NULL.  After the outputs are complete, op (0: none, else GS_STATE_*) with bits is applied to the members of merged groups.  A NULL
 * record pointer with cap_records 0 is the COUNT-ONLY mode: only info is filled, nothing is marked.  cap_records < G:
 * GS_ERR_INVALID_ARGUMENT, info filled, nothing written or marked.  With op == 0 the calls work on a borrower of gs_share_splats as
 * gs_neigh_count does; with an op they have gs_state_region's rules: the borrower carries the owner's plane, the members are marked in
 * THAT plane (owner and every borrower see it), and contexts the host drives itself are the host's to drain first.
 * Prologue, drain, ordering and slabs are gs_neigh_count's;
 * the calls use the neighbourhoods' scratch and leave every plane alone.  GS_ERR_NO_SCENE before any upload; N == 0: zeros, GS_OK.
 * Refused with GS_ERR_INVALID_ARGUMENT and a message that names the call: a wrong struct_size, a cell that is not finite or <= 0,
 * min_members < 2, an op above GS_STATE_ASSIGN, bits above 0xFF or without an op, a filter above 0xFF, and an op or a filter other
 * than (0, 0) on a ctx without GS_FLAG_SPLAT_STATE.
 * gs_cell_merge_host runs the same computation over n HOST records (80 floats each) without a ctx or a GPU; state (u8[n]) may be NULL
 * when the filter is (0, 0) and op is 0, and is marked in place otherwise. */
#define GS_MERGE_SUM_DOUBLES 64u
#define GS_MERGE_NONE 0xFFFFFFFFu
#define GS_MERGE_DEFAULT_MAX_MEMBERS 65536u
typedef struct gs_merge {          /* 32 bytes */
    uint32_t struct_size;          /* = sizeof(gs_merge) */
    uint32_t mask, value;          /* the filter: (s & mask) == value */
    float    cell;                 /* the requested cell edge: finite, > 0 */
    uint32_t min_members;          /* >= 2: cells with fewer eligible splats are left alone */
    uint32_t max_members;          /* 0 = GS_MERGE_DEFAULT_MAX_MEMBERS */
    uint32_t op, bits;             /* 0, or GS_STATE_* applied to the merged members */
} gs_merge;
typedef struct gs_merge_info {     /* 48 bytes */
    uint64_t eligible;             /* splats that take part in the grouping */
    uint64_t groups;               /* G: merged groups = records */
    uint64_t members;              /* splats in merged groups */
    uint64_t largest;              /* eligible splats of the fullest cell */
    uint32_t cells[3]; float cell_edge; /* the grid and the edge that were used */
} gs_merge_info;
int32_t gs_cell_merge(gs_ctx* ctx, const gs_merge* params, void* aos320, uint64_t cap_records, double* sums, uint32_t* group_of,
                      gs_merge_info* info);
int32_t gs_cell_merge_device(gs_ctx* ctx, const gs_merge* params, void* d_aos320, uint64_t cap_records, double* sums, uint32_t* group_of,
                             gs_merge_info* info);
int32_t gs_cell_merge_host(const void* records, uint8_t* state, uint64_t n, const gs_merge* params, void* aos320, uint64_t cap_records,
                           double* sums, uint32_t* group_of, gs_merge_info* info);

/* ---- surface: per-splat normals and shape from neighbourhood covariance --------------------------------------
 * A count, a label and a k-th distance are one scalar per splat; a plane fit and a consensus are one global answer.  "Select what
 * lies on a surface", "select the horizontal surfaces" (floor, table tops and steps at once), "find the floaters that are dense but
 * have no surface", oriented normals for export and the point-to-plane variant of a registration need the LOCAL geometry: the
 * covariance of every splat's neighbourhood, its three eigenvalues and the eigenvector of the smallest.  The reference has no
 * counterpart (a viewer).
 * THE DEFINITION.  Sources are the splats j with (s_j & src_mask) == src_value, queries the splats i with (s_i & qry_mask) ==
 * qry_value.  With the neighbourhoods' expression unchanged
 *     d = p_j - p_i per component;  d2 = (dx dx + dy dy) + dz dz;  r2 = radius * radius
 * -- one f32 rounding per written operation, no contraction, r2 ONE f32 product, the comparison <= INCLUSIVE -- let, for a query i,
 *     D_i = the set of sources j != i with d2(i, j) <= r2.
 * Self is excluded by index, not by distance.  A NaN or infinite coordinate fails every comparison: such a splat has no neighbours
 * and is nobody's.
 * THE SUMS ARE INTEGERS, so nothing depends on the order in which the device visits anything.  Let E be frexpf(radius)'s exponent,
 * 2^(E-1) <= radius < 2^E, and s = 2^(16 - E) as an f32.  For an accepted j
 *     q_a = (int32) rintf(d_a * s),   a = x, y, z
 * -- the product by a power of two is exact, rintf rounds half to even: this is the ONE quantisation, its step between 2^-16 and
 * 2^-15 of the radius.  Per query
 *     count = |D_i| (u32);   S_a = the sum of q_a (3 x i64);   M_ab = the sum of q_a q_b for xx xy xz yy yz zz (6 x i64).
 * THE BOUND: |d_a| <= radius (1 + 2^-22) <= 2^E, so |q_a| <= 2^16 + 1 and |q_a q_b| <= 2^32 + 2^18 + 1; with fewer than 2^30 sources
 * (the cell sort's limit) no sum reaches 2^63: there is no wrap and no saturation rule.
 * THE FINISHING is f64, one header (csrc/gs_surface_math.h) compiled by the device and the host, in the cell merge's order of
 * operations with n = count:
 *     mu_a = (double)S_a / n;   C_ab = (double)M_ab / n - mu_a * mu_b        (i64 -> double rounds to nearest even)
 * then the cell merge's fixed number of cyclic Jacobi sweeps (the same two functions, no second copy).  The eigenvalues are ordered
 * l0 >= l1 >= l2, each clamped with l >= 0 ? l : 0, scaled to world units by the exact power of two 2^(2 (E - 16)) and rounded ONCE
 * to f32.  The normal is the eigenvector column of l2, flipped in f64 so that its component of largest magnitude is positive (a tie:
 * the lowest axis), then each component rounded once to f32.  With GS_SURFACE_ORIENT, in f32 on the rounded normal,
 *     e = toward - p_i;   t = (nx ex + ny ey) + nz ez;   the normal is negated when t < 0 and kept when t is 0 or NaN.
 * WHAT THE PLANES READ.  A query with count < 3 reads NaN with exactly the bits 0x7FC00000 in all six floats and keeps its count:
 * UNRESOLVED.  A splat that is not a query, or a query with a non-finite coordinate, reads NaN and count 0.  Sums, count and info
 * compare bit for bit between two runs, a slab ctx, a borrower of gs_share_splats, gs_surface_host and a brute-force host
 * restatement (tests/surface_restate.py); normal and eig bit for bit between the device and gs_surface_host.
 * THE PLANES are normal f32[N][3], eig f32[N][3] and count u32[N] (held as two 16-byte records per splat) and belong to the ctx the
 * call is made on (the root of a ring; a borrower keeps its own), like the nearest-neighbour planes.  They are allocated by the first
 * call that needs them and read NaN / count 0 before the first estimate; gs_surface_estimate overwrites them as a whole; they are
 * DROPPED -- they read as before the first estimate again -- by every gs_upload_*, gs_share_splats and gs_compact, whatever drops the
 * count plane and nothing else.  State calls and transforms leave them untouched: they describe the positions and states at the time
 * of the estimate, and a host that moves or re-filters splats estimates again.  A call that fails for any reason -- budget,
 * allocation, a refused argument -- leaves the planes and the kept sums as they were.
 * WORK.  An estimate builds the neighbourhoods' grid over the sources at the radius given, computes `candidates` exactly and, above
 * max_candidates (0: GS_NEIGH_DEFAULT_CANDIDATES), returns GS_ERR_CAPACITY with both numbers in the message; the query pass is issued
 * in the count's slices (GS_NEIGH_SLICE_CANDIDATES), each followed by its finishing pass.  Measured rates: profiles/surface.txt.
 * Prologue, ordering and refusals are gs_knn_search's: each (mask, value) as gs_state_count, above 0xFF refused, (0, 0) matches every
 * splat and is accepted on a ctx without GS_FLAG_SPLAT_STATE, any other filter on such a ctx is refused.  Every call first completes
 * all frames enqueued on the ctx's ring, runs on the ctx's stream and returns when done; none is a frame or an upload.
 * GS_ERR_NO_SCENE before any upload; N == 0: zero results, GS_OK.  gs_surface_estimate and the two reads work on a borrower;
 * gs_state_surface has gs_state_region's rules.  GS_ERR_INVALID_ARGUMENT and a message that names the number: a wrong struct_size, a
 * radius that is not above 0, negative or not finite, a radius * radius that is not finite in f32, 16 - E > 127 (s must be a finite
 * normal f32), unknown flag bits, reserved != 0. */
#define GS_SURFACE_ORIENT 0x1u     /* gs_surface.flags: the normals point towards `toward` */
#define GS_SURFACE_KEEP_SUMS 0x2u  /* gs_surface.flags: keep the ten integers per splat for gs_surface_read_sums */
#define GS_SURFACE_SUM_WORDS 10u   /* count, S x y z, M xx xy xz yy yz zz */
typedef struct gs_surface {        /* 56 bytes */
    uint32_t struct_size;          /* = sizeof(gs_surface) */
    float    radius;               /* finite, > 0; r2 = radius * radius, ONE f32 product, must be finite */
    uint32_t flags;                /* GS_SURFACE_ORIENT | GS_SURFACE_KEEP_SUMS */
    uint32_t src_mask, src_value;  /* SOURCES: splats j with (s_j & src_mask) == src_value */
    uint32_t qry_mask, qry_value;  /* QUERIES: splats i with (s_i & qry_mask) == qry_value */
    float    toward[3];            /* GS_SURFACE_ORIENT: the point the normals face (a viewpoint); ignored otherwise */
    uint64_t max_candidates;       /* work budget, 0 = GS_NEIGH_DEFAULT_CANDIDATES */
    uint64_t reserved;             /* 0 */
} gs_surface;
typedef struct gs_surface_info {   /* 48 bytes */
    uint64_t queried, sources;     /* splats that pass the two filters */
    uint64_t candidates;           /* sum over the queries of the sources in the 27 cells around them, self included */
    uint64_t unresolved;           /* queries that end with count < 3, those with a non-finite coordinate included */
    uint32_t cells[3]; float cell_edge; /* the grid that was used (diagnostic; no result depends on it) */
} gs_surface_info;
/* Estimates into the planes.  info (may be NULL) is written whenever the grid was built, also when the budget refuses the call
 * (queried, sources, candidates and the grid; unresolved is that of a completed estimate). */
int32_t gs_surface_estimate(gs_ctx* ctx, const gs_surface* q, gs_surface_info* info);
/* The planes in HOST memory in splat order, with gs_knn_read's conventions: normal (3 N floats), eig (3 N floats) and count (N words)
 * may each be NULL, all NULL: only *n (= N) is written (query); cap < N: GS_ERR_INVALID_ARGUMENT, the message names the count needed,
 * nothing is written. */
int32_t gs_surface_read(gs_ctx* ctx, float* normal, float* eig, uint32_t* count, uint64_t cap, uint64_t* n);
/* GS_SURFACE_SUM_WORDS x i64 per splat in splat order: count, S[3], M[6]; zeros for a splat that was no query.  Valid only after an
 * estimate with GS_SURFACE_KEEP_SUMS: the sums are dropped with the planes and by the next estimate without the flag, and the call is
 * then refused (GS_ERR_INVALID_ARGUMENT).  sums NULL: only *n is written; cap < N (in splats): refused as above. */
int32_t gs_surface_read_sums(gs_ctx* ctx, int64_t* sums, uint64_t cap, uint64_t* n);
/* Applies `op` with `bits` exactly as gs_state_region does, to the splats that pass (s & where_mask) == where_value and for which
 *     (v >= lo && v <= hi) == (inside != 0)
 * -- gs_state_knn's rule --, v computed from the stored f32 planes with one rounding per written operation:
 *     GS_SURFACE_VARIATION      l2 / ((l0 + l1) + l2)         surface variation: 0 on a plane, 1/3 for an isotropic blob
 *     GS_SURFACE_PLANARITY      (l1 - l2) / l0
 *     GS_SURFACE_LINEARITY      (l0 - l1) / l0
 *     GS_SURFACE_SPHERICITY     l2 / l0
 *     GS_SURFACE_FACING         fabsf((nx ax + ny ay) + nz az), axis used as given (not normalised)
 *     GS_SURFACE_FACING_SIGNED  the same without the fabsf
 *     GS_SURFACE_COUNT          the count as f32
 * A NaN (also 0 / 0) is in no range.  A NaN lo or hi, an unknown kind and a wrong struct_size are refused; infinite bounds are
 * allowed, lo > hi is a valid empty range.  Needs GS_FLAG_SPLAT_STATE; *matched (may be NULL) as for gs_state_region.  One streaming
 * pass over 17 bytes per splat. */
#define GS_SURFACE_VARIATION 0u
#define GS_SURFACE_PLANARITY 1u
#define GS_SURFACE_LINEARITY 2u
#define GS_SURFACE_SPHERICITY 3u
#define GS_SURFACE_FACING 4u
#define GS_SURFACE_FACING_SIGNED 5u
#define GS_SURFACE_COUNT 6u
typedef struct gs_surface_range {  /* 32 bytes */
    uint32_t struct_size;          /* = sizeof(gs_surface_range) */
    uint32_t kind;                 /* GS_SURFACE_VARIATION .. GS_SURFACE_COUNT */
    float    lo, hi;               /* neither a NaN */
    uint32_t inside;               /* 0: select what is outside the range */
    float    axis[3];              /* the two FACING kinds; ignored otherwise */
} gs_surface_range;
int32_t gs_state_surface(gs_ctx* ctx, const gs_surface_range* r, uint32_t where_mask, uint32_t where_value, uint32_t op, uint32_t bits,
                         uint64_t* matched);
/* The same computation without a ctx or a GPU, compiled from the same header: pos f32[n][3] (x y z interleaved), state u8[n] (may be
 * NULL when both filters are (0, 0)), normal f32[n][3], eig f32[n][3], count u32[n], sums i64[n][10] (may be NULL; GS_SURFACE_KEEP_SUMS
 * is not needed), info (may be NULL).  It tests all pairs: info.candidates = finite queries x finite sources, cells = 1 1 1,
 * cell_edge = 0.  The refusals are gs_surface_estimate's, a filter above 0xFF and a null array with n > 0 included. */
int32_t gs_surface_host(const float* pos, const uint8_t* state, uint64_t n, const gs_surface* q, float* normal, float* eig, uint32_t* count,
                        int64_t* sums, gs_surface_info* info);

/* ---- thinning: a blue-noise subsample of resident splats by rank and radius ----------------------------------
 * A count, a labelling and a cell merge cannot say "keep a subset such that no two kept splats are within a radius of each other,
 * every dropped splat has a kept one within that radius, and where two compete the more important one survives": a Poisson-disk
 * sample, the maximal independent set of the "within r" graph visited in priority order.  It decimates with REAL splats (the cell
 * merge blurs), spaces query sets for a registration evenly, collapses near-duplicates with a rule about who survives, and hands
 * out a partition for free: every dropped splat names the kept one that stands for it.  On the device, with the neighbourhoods'
 * grid, distance expression, work budget and slices.
 * MEMBERS, LINKS AND RANK.  MEMBERS are the splats i with (s_i & mask) == value (gs_state_count's filter).  Two members i != j are
 * LINKED when
 *     d2(i, j) <= r2;   d = p_j - p_i per component;  d2 = (dx dx + dy dy) + dz dz;  r2 = radius * radius
 * -- the neighbourhoods' expression with nothing changed: one f32 rounding per written operation, no contraction, r2 ONE f32
 * product, the comparison <= INCLUSIVE.  A member with a NaN or infinite coordinate is linked to nobody.  RANK is a 64-bit integer
 *     R_i = (P_i << 32) | H_i;   member j OUTRANKS member i when R_j > R_i, or when R_j == R_i and j < i.
 * P_i is 0 without a priority attribute.  With one -- a gs_attr evaluated exactly as gs_attr_read would -- P_i is the splat
 * attributes' order-preserving key of the value's bit pattern b, k = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000); with GS_THIN_ASCENDING
 * P_i = ~k instead, so smaller values win.  A NaN value has P_i = 0 in both directions: missing data never wins.  H_i by default is
 * this hash of the index, all arithmetic mod 2^32:
 *     h = i + seed * 0x9E3779B9;  h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;  h *= 0x846CA68B;  h ^= h >> 16;  H_i = h
 * -- every step invertible, so a bijection of i for a fixed seed, and R a total order by itself.  With GS_THIN_ORDER_INDEX
 * H_i = ~i: the lower index wins among equal priorities.
 * KEPT, KEEPER AND COVERS.  KEPT is the unique set obtained by visiting the members from the highest rank down: a member is kept
 * iff no member kept before it is linked to it (the lexicographically first maximal independent set).  Equivalently the unique
 * fixpoint of: a member is kept iff every linked member that outranks it is dropped; a member is dropped iff some linked member
 * that outranks it is kept.  For every resident splat i, two u32 planes:
 *     kept member:                          keeper[i] = i,   covers[i] = the members m with keeper[m] == i, itself included (>= 1)
 *     dropped member:                       keeper[i] = of the kept members linked to it the one that outranks all the others
 *                                           (there is one, by maximality),   covers[i] = 0
 *     member with a non-finite coordinate:  keeper[i] = i (linked to nobody, hence kept),   covers[i] = 1
 *     non-member:                           keeper[i] = GS_THIN_NONE,   covers[i] = 0
 * The sum of covers is the number of members.  Both planes are integers and functions of the positions, the state bytes, the
 * radius, the priority values, the flags and the seed only: two runs, a slab ctx, a borrower of gs_share_splats, a fresh ctx, the
 * host twin and a brute-force restatement agree bit for bit.  radius = 0 (or one whose square is 0) collapses exact duplicates.
 * THE PLANES belong to the ctx the call is made on, are allocated by the first call that needs them, read GS_THIN_NONE / 0 before
 * the first sample and are DROPPED -- they read so again -- by exactly what drops the count plane: every gs_upload_*,
 * gs_share_splats and gs_compact.  Nothing else drops them: they describe the positions, states and priorities at the time of the
 * sample.  A call that fails for any reason -- budget, allocation, the round cap, a refused argument -- leaves both as they were.
 * WORK.  A sample builds the neighbourhoods' grid over the members, writes R once, then runs ROUNDS of one query pass over the
 * candidates: an undecided member that finds a linked, outranking member KEPT in an earlier round becomes DROPPED; one that finds no
 * linked, outranking member still undecided becomes KEPT; the others wait.  Every round decides at least the highest-ranked
 * undecided member, so the rounds end; `rounds` is a function of the inputs too (a round reads the decisions of earlier rounds only).
 * One more query pass over the dropped members names their keepers and counts the covers.  max_candidates (0:
 * GS_NEIGH_DEFAULT_CANDIDATES) is the budget of ONE round, as for clusters; every pass is issued in the count's slices.  THE ROUND
 * CAP: more rounds than max_rounds (0: GS_THIN_DEFAULT_ROUNDS) is GS_ERR_CAPACITY with the rounds run and the members still
 * undecided in the message.  It can be hit by legitimate input: the rounds needed are the longest chain of linked members in
 * descending rank.  With the hash order that is O(log N) with high probability (15 rounds at 6.1 M splats and about 10 links per
 * splat); with GS_THIN_ORDER_INDEX, or a priority that is constant along a spatially sorted index order, it is as long as the
 * geometry makes it (a line of 2000 points in index order: 2000 rounds).  The default is what the hash order was seen to need at
 * 6.1 M splats times a margin (profiles/thin.txt); the cap keeps a chain-like input from costing thousands of passes unasked, and a
 * caller who wants such an order raises it.
 * Prologue, ordering, borrowers, slabs, N == 0 and refusals are the clusters': the filter as gs_state_count, above 0xFF refused,
 * (0, 0) accepted on a ctx without GS_FLAG_SPLAT_STATE, any other filter on such a ctx refused; every call first completes all
 * frames enqueued on the ctx's ring, runs on the ctx's stream and returns when done; none is a frame or an upload.
 * GS_ERR_NO_SCENE before any upload; N == 0: zero results, GS_OK.  gs_thin_sample and gs_thin_read work on a borrower; gs_state_thin needs
 * GS_FLAG_SPLAT_STATE and has gs_state_region's rules.  GS_ERR_INVALID_ARGUMENT and a message that names the number: a wrong
 * struct_size, a radius that is negative or not finite or whose square is not finite in f32, unknown flag bits, GS_THIN_ASCENDING
 * without a priority, a priority that gs_attr_read would refuse, a reserved word that is not 0. */
#define GS_THIN_NONE 0xFFFFFFFFu
#define GS_THIN_NO_PRIORITY 0xFFFFFFFFu /* gs_thin.priority.kind: no priority attribute, P_i = 0 */
#define GS_THIN_ORDER_INDEX 0x1u        /* gs_thin.flags: H_i = ~i */
#define GS_THIN_ASCENDING 0x2u          /* gs_thin.flags: P_i = ~k, smaller priority values win; needs a priority */
#define GS_THIN_DEFAULT_ROUNDS 64u      /* the hash order at 6.1 M splats, 15 rounds, times 4 (profiles/thin.txt) */
typedef struct gs_thin {           /* 72 bytes */
    uint32_t struct_size;          /* = sizeof(gs_thin) */
    float    radius;               /* finite, >= 0; r2 = radius * radius must be finite in f32 */
    uint32_t mask, value;          /* MEMBERS: splats i with (s_i & mask) == value */
    uint32_t flags;                /* GS_THIN_ORDER_INDEX | GS_THIN_ASCENDING */
    uint32_t seed;                 /* of the hash order */
    uint32_t max_rounds;           /* 0 = GS_THIN_DEFAULT_ROUNDS */
    uint32_t reserved0;            /* 0 */
    uint64_t max_candidates;       /* work budget PER ROUND, 0 = GS_NEIGH_DEFAULT_CANDIDATES */
    gs_attr  priority;             /* kind == GS_THIN_NO_PRIORITY: none (the rest of it is not read) */
    uint32_t reserved[2];          /* 0 */
} gs_thin;
typedef struct gs_thin_info {      /* 64 bytes */
    uint64_t members;              /* splats that pass the filter */
    uint64_t kept;                 /* members with keeper[i] == i */
    uint64_t dropped;              /* members - kept */
    uint64_t largest;              /* the maximum of covers */
    uint64_t candidates;           /* distance tests of a whole pass: the members in the 27 cells around every member, self included */
    uint32_t rounds;               /* round passes that were run */
    uint32_t cells[3]; float cell_edge; /* the grid that was used (diagnostic; no result depends on it) */
    uint32_t reserved;
} gs_thin_info;
/* Samples into the two planes.  info (may be NULL) is written whenever the grid was built, also when the budget refuses the call
 * (members, candidates and the grid; kept, dropped, largest and rounds are those of a completed sample). */
int32_t gs_thin_sample(gs_ctx* ctx, const gs_thin* q, gs_thin_info* info);
/* The planes in HOST memory, N words each in splat order, with gs_cluster_read's conventions: keeper and covers may each be NULL,
 * both NULL: only *n (= N) is written (query); cap < N: GS_ERR_INVALID_ARGUMENT, the message names the count needed, nothing is
 * written. */
int32_t gs_thin_read(gs_ctx* ctx, uint32_t* keeper, uint32_t* covers, uint64_t cap, uint64_t* n);
/* Applies `op` with `bits` exactly as gs_state_region does, to the splats that pass (s & where_mask) == where_value and for which
 *     (covers >= min_covers && covers <= max_covers) == (inside != 0)
 * -- the plain expression on the plane value: gs_state_cluster's pass over the covers plane.  "Kept" is [1, 2^32 - 1]; "dropped" is
 * [0, 0] under where = the member filter (a non-member reads 0 too).  *matched (may be NULL) as for gs_state_region. */
int32_t gs_state_thin(gs_ctx* ctx, uint32_t min_covers, uint32_t max_covers, uint32_t inside, uint32_t where_mask, uint32_t where_value,
                      uint32_t op, uint32_t bits, uint64_t* matched);
/* The same sample without a ctx or a GPU, by another algorithm (the members sorted by rank, a sequential greedy over a hashed grid
 * of the kept ones -- not the rounds): px, py, pz f32[n], state u8[n] (NULL: every state byte is 0), priority f32[n] the priority
 * VALUES (NULL: none; q->priority is not read), keeper and covers u32[n], info (may be NULL; rounds = 0, candidates = the distance
 * tests made, cells = 1 1 1, cell_edge = 0).  The refusals are gs_thin_sample's, with GS_THIN_ASCENDING refused when priority is NULL, a
 * filter above 0xFF and a null array with n > 0 included; n >= 2^32 is refused. */
int32_t gs_thin_host(const float* px, const float* py, const float* pz, uint64_t n, const uint8_t* state, const float* priority,
                     const gs_thin* q, uint32_t* keeper, uint32_t* covers, gs_thin_info* info);

/* Tuning / profiling knobs. */
#define GS_OPT_BLEND_ABLATION 1  /* bit 3 (8): the workgroup-per-tile blend kernel at tiles 16 and 32 (identical results; default = one
                                    wave per 8x8 pixel block); bit 2 (4): every blend kernel without its two parking culls (live box,
                                    transmittance bound: identical results, slower -- the test that they change no bit); bits 8-15: tile-column strip width of the default kernel's XCD mapping
                                    (0 = automatic).  The remaining bits act only in the PROFILING build (csrc/build.py --profiling,
                                    libgsplat_hip_prof.so; the product library ignores them): bits 0/1 break the image (1 skip the
                                    pixel loop, 2 gather from a cache-resident window), bit 5 counts the evaluations' footprint
                                    (tools/blend_footprint.py), bits 6/7 cap the kernel at 2 / 4 waves per SIMD, bit 16 records a
                                    start / end stamp per walker (GS_BUF 11, tools/blend_profile.py)                              */
#define GS_OPT_PERSISTENT_GRID 2 /* workgroups of the ticket-loop kernels (default 4 per CU)                          */
#define GS_OPT_RESET_TIMING 3    /* start a new averaging window for gs_stats.stage_us_mean                           */
#define GS_OPT_EMIT_ORDER 4      /* 1: the reference's gaussian-index emission order + sort by the full key (3-4 radix digits);
                                    0: depth-ordered pipeline: sort the visible GAUSSIANS by depth bucket, emit their instances
                                    in that order (work-balanced), sort the instances by tile only (2 digits);
                                    2 (default): choose per frame from the previous frame's instance count ((radix sweeps saved)
                                    x instances >= 1 M -> 0, else 1).  Sorted keys/values, ranges and image are identical in
                                    every mode.                                                                           */
#define GS_OPT_DEBUG_VIEW 6      /* the developer views commented out in compute_tiles.wgsl:35-38,67-70, drawn over the frame: 0 off,
                                    1 tile borders (last row/column of every tile red), 2 list length/1000 as grey, 3 pixel
                                    position gradient, 4 list length/100 in red+green                                    */
#define GS_OPT_UNFUSED 5         /* 1 (default): projection, scan and emission are three launches; 0: experimental single fused launch
                                    (identical results; measured slower in round 1)                                              */
#define GS_OPT_TILE_CULL 7       /* 1 (default): gs_render / gs_render_to bin TIGHTLY: an instance (gaussian, tile) is emitted only if
                                    some pixel of the tile can reach alpha >= 1/255 (conservative test, so no output bit changes:
                                    compute_tiles.wgsl:60-63 skips such an entry on every pixel), and carries a mask of the 8x8 pixel
                                    blocks it can touch.  GS_BUF_KEYS / VALUES / RANGES / TILE_COUNTS of such a frame describe that
                                    subset.  0: the reference's binning (every tile of the 3-sigma rect, process_gaussians.wgsl:74-86)
                                    as gs_render_debug always uses.                                                              */
#define GS_OPT_FRAMES_IN_FLIGHT 8 /* 1..4, default 3 for a whole-canvas ctx on its own stream (1 for slabs and caller-supplied streams).
                                    Renderer.animate awaits every frame (renderer.ts:404-587), so it never has two in flight; a host
                                    that enqueues frame k+1 before waiting for frame k gets it rendered by a shadow of the ctx (own
                                    stream and per-frame arrays, the same resident splats; created on first need), gs_render
                                    taking turns between them: frame k's blend overlaps frame k+1's binning.  Every frame's result
                                    is what a single context renders; gs_wait waits for all; read-backs, taps and statistics refer
                                    to the LAST frame.  1 = strictly one frame after the other.                                  */
#define GS_OPT_FRAME_GRAPH 9      /* 1: the frame's commands (1 memset, 12-14 kernels, 2 copies) are captured into a hipGraph the first time
                                    and replayed with one hipGraphLaunch afterwards; only the projection's uniforms change between
                                    frames (a kernel-node parameter update).  For hosts bound by launch cost: small scenes (config A:
                                    a frame is ~70 us of launches) and the narrow slabs of an 8-GPU run.  Frames with per-stage
                                    events (GS_FLAG_TIMING), gs_render_debug and the profiler taps are issued directly as before;
                                    the capture is redone when a buffer moves (capacity growth), an option or the emission order
                                    changes.  Renderer.animate re-encodes every pass every frame (renderer.ts:394-587).  Default 0. */
#define GS_OPT_PROJ_CHUNKS 10     /* tuning: 512-gaussian cull chunks per workgroup of the tight projection (2, 4 or 8; 0 = automatic)  */
#define GS_OPT_SELECT_TINT 11      /* (GS_FLAG_SPLAT_STATE) a<<24 | r<<16 | g<<8 | b: colour GS_SPLAT_SELECTED splats are drawn towards and how
                                    far (k = a / 255, tint = channel / 255); default 0x80FFFF00; a = 0: selection not drawn (the
                                    colour is left untouched, not multiplied by 0)                                              */
int32_t gs_set_option(gs_ctx* ctx, int32_t key, int64_t value);
/* Width in pixels of this ctx's slab (= width when the ctx owns the whole screen). */
int32_t gs_slab_width(gs_ctx* ctx, uint32_t* px_begin, uint32_t* px_width);

/* Multi-GPU presentation: scatter `n_slabs` gathered slab images (slab g = u8[height][w_g][4]) into one
 * row-major u8[height][width][4] DEVICE image.  col_bounds (host) has n_slabs+1 tile-column boundaries.
 * slab_stride_bytes = distance between consecutive slabs in d_slabs (what an all-gather of equally
 * sized, padded send buffers produces); 0 = slabs tightly packed in rank order.  Runs on the ctx stream. */
int32_t gs_assemble_slabs(gs_ctx* ctx, const void* d_slabs, const uint32_t* col_bounds, uint32_t n_slabs,
                          uint64_t slab_stride_bytes, void* d_image);

/* ---- packed scenes: save, load and append the 16-byte chunked splat format ---------------------------------
 * The float .ply is 248 bytes per splat at SH degree 3.  The packed file keeps position, rotation, log-scale and colour in four
 * 32-bit words per splat, quantised against the bounds of its chunk of 256 splats, plus one byte per higher SH coefficient: 16 bytes
 * per splat at degree 0, 61 at degree 3, and 72 bytes per chunk.  The reference has no counterpart (ply.ts:49-228 reads the float
 * .ply only).  No interoperability with third-party files is claimed: the files carry the line `comment gsplat-packed 1` and only
 * files with it are read.  THE DEFINITION (csrc/gs_pack_math.h is its one copy in code; all arithmetic f32, one IEEE rounding per
 * written operation; record floats f[] numbered as in a 320-byte record: 0..2 position, 4..6 log-scales, 8..11 rotation r x y z,
 * 12 opacity logit, 16 + 4 k + c SH coefficient k channel c; min / max as wg_min / wg_max below):
 *   fin(v) = v when finite, else +0.   unorm(v, b) = f2u_sat(min(T, max(0, v T + 0.5))), T = 2^b - 1 (a NaN gives 0).
 *   norm(v, lo, hi) = hi > lo ? (v - lo) / (hi - lo) : 0.   lerp(lo, hi, t) = lo (1 - t) + hi t.   dn(code, b) = (float)code / T.
 *   Entry g of the output belongs to chunk g / 256; the last chunk may be partial and its bounds come from its real entries only.
 *   Per entry: p_k = fin(f[k]); s_k = max(-20, min(20, fin(f[4 + k]))); c_k = fin(f[16 + k]) * 0.28209479177387814f + 0.5f;
 *   alpha a from o = f[12]: NaN -> 0; o >= 0 -> 1 / (1 + exp(-o)); else ez / (1 + ez), ez = exp(o) (exp: the canonical one);
 *   rotation from q = fin(f[8..11]): len = sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3); not (len > 0) or len not finite -> q = (1,0,0,0),
 *   else q_k / len; L = the lowest index with the largest |q_k|; q_L < 0 negates all four; t0 t1 t2 = the other three, ascending.
 *   Chunk record, 18 floats: min xyz, max xyz of p; the same of s; min rgb, max rgb of c -- exact minima and maxima in the total
 *   order of the bit patterns (-0 below +0; all values are finite), so that every reduction order gives the same bits.
 *   Vertex, four u32: packed_position = unorm(nx,11)<<21 | unorm(ny,10)<<11 | unorm(nz,11), n* = norm(p, lo, hi);
 *   packed_rotation = L<<30 | unorm(t0 h + 0.5, 10)<<20 | unorm(t1 h + 0.5, 10)<<10 | unorm(t2 h + 0.5, 10), h = 0.70710678118654752f;
 *   packed_scale like packed_position over s; packed_color = unorm(nr,8)<<24 | unorm(ng,8)<<16 | unorm(nb,8)<<8 | unorm(a,8).
 *   SH rest, degree d >= 1, K = (d+1)^2 - 1, 3K bytes per splat: byte c K + i = f2u_sat(min(255, max(0, (fin(f[16 + 4 (i+1) + c]) / 8
 *   + 0.5) * 256))).
 *   Decode: position and log-scale lerp(lo, hi, dn); f[16 + k] = (lerp(lo, hi, dn) - 0.5f) / 0.28209479177387814f;
 *   t_i = (dn(code_i, 10) - 0.5f) * 1.41421356237309505f, m = sqrt(max(0, 1 - ((t0 t0 + t1 t1) + t2 t2))) at index L, the t's at the
 *   others (not renormalised: the projection normalises); logit = table[a8], the 256 floats of gs_pack_logit_table:
 *   (float)log(x / (1 - x)) in double, x = a8 / 255, but 0.5 / 255 for code 0 and 254.5 / 255 for code 255 (every logit finite);
 *   SH rest (((float)byte + 0.5f) / 256 - 0.5f) * 8; coefficients above the file's degree and the 21 padding floats are +0.
 *   Morton order: lo_k, hi_k = the bounds of the selection's splats whose three coordinates are finite; per axis
 *   q_k = min(1023, f2i_sat(norm(p_k, lo_k, hi_k) * 1024)); bit b of x, y, z goes to key bit 3b, 3b+1, 3b+2; a splat with a non-finite
 *   coordinate gets the key 1<<30; the order is the stable ascending sort of the selection's ascending ids by key.
 * THE FILE: a little-endian binary .ply with exactly this header, then C = ceil(n / 256) chunk records, n vertices and, at degree
 * >= 1 only, n SH records:
 *     ply / format binary_little_endian 1.0 / comment gsplat-packed 1 / element chunk C / property float min_x min_y min_z max_x max_y
 *     max_z min_scale_x min_scale_y min_scale_z max_scale_x max_scale_y max_scale_z min_r min_g min_b max_r max_g max_b (one line
 *     each) / element vertex n / property uint packed_position packed_rotation packed_scale packed_color / [element sh n /
 *     property uchar f_rest_0 .. f_rest_{3K-1}] / end_header
 * A loader requires the marker, these names and types in this order, C consistent with n, n below 2^31 and a file of exactly the
 * implied size; anything else is GS_ERR_INVALID_ARGUMENT with a message naming the path and the defect, and nothing is allocated
 * from a count before the size check.  A refused file leaves every output as it was.
 * Host codec (no GPU, no context).  chunks: C x 18 floats; vertices: n x 4 words; sh: n x 3K bytes (may be NULL at degree 0);
 * nonfinite (may be NULL): the carried floats that fin replaced plus the NaN logits.  gs_pack_load's records are n x 320 bytes,
 * released with gs_ply_free. */
#define GS_PACK_ORDER_INDEX 0   /* ascending splat index */
#define GS_PACK_ORDER_MORTON 1  /* along a Morton curve through the selection's bounds: a chunk's splats are neighbours, its bounds tight */
int32_t gs_pack_encode(const void* aos320, uint64_t n, int32_t sh_degree, float* chunks, uint32_t* vertices, uint8_t* sh, uint64_t* nonfinite);
int32_t gs_pack_decode(const float* chunks, const uint32_t* vertices, const uint8_t* sh, uint64_t n, int32_t sh_degree, void* aos320);
int32_t gs_pack_save(const char* path, const void* records, uint64_t n, int32_t sh_degree);
int32_t gs_pack_load(const char* path, void** records, uint64_t* n, int32_t* sh_degree);
int32_t gs_pack_logit_table(float out[256]);
/* Resident scenes.  Each call drains the ring first, runs on the context's stream, returns when done and launches nothing in a
 * frame.  gs_export_packed writes the splats with (s & mask) == value ((0, 0): all, also without GS_FLAG_SPLAT_STATE) in `order`:
 * the whole selection is encoded on the device (at most 61 bytes per splat of device scratch) and streamed to the file through two
 * pinned buffers; the host never holds the scene.  ids (may be NULL; room for every resident splat): record g of the file is splat
 * ids[g].  info (may be NULL) is written on success.  A file that could not be completed is removed.  The scene is not changed.
 * gs_upload_packed replaces the scene like gs_upload_ply, gs_append_packed appends like gs_append_ply (same refusals, installed
 * only when complete, the old scene untouched by a failure); both read the file in trips of whole chunks and decode on the device.
 * The decoded records are exactly gs_pack_decode's, the derived planes what gs_upload_splats of those records derives. */
typedef struct gs_pack_info { /* 32 bytes */
    uint64_t count;      /* splats written                                          */
    uint64_t chunks;     /* ceil(count / 256)                                       */
    uint64_t file_bytes; /* the whole file, header included                         */
    uint64_t nonfinite;  /* carried floats that fin replaced, plus the NaN logits   */
} gs_pack_info;
int32_t gs_export_packed(gs_ctx* ctx, const char* path, uint32_t mask, uint32_t value, int32_t sh_degree, int32_t order, gs_pack_info* info,
                         uint32_t* ids);
int32_t gs_upload_packed(gs_ctx* ctx, const char* path, uint64_t* n);
int32_t gs_append_packed(gs_ctx* ctx, const char* path, uint32_t new_state, uint64_t* first, uint64_t* m);

/* ---- stand-alone stages, mirroring the reference's reusable classes ---------------------------- */
/* GPUSorter.sort (radix_sort/sort.ts:341-350): stable ascending sort of n u32 keys with u32 payloads,
 * host buffers, in place.  values may be NULL (keys only, as testSort does: radix_sort/utils.ts:55-81). */
int32_t gs_sort_pairs_u32(int32_t device, uint32_t* keys, uint32_t* values, uint64_t n, uint32_t key_bits);
/* ExclusiveScanner.scan (exclusive_scan.ts:208-325): in-place exclusive scan of n u32 (each < 2^22), returns the
 * total.  Sums saturate instead of wrapping: every offset is min(true prefix, 2^32 - 1), and so is the total. */
int32_t gs_exclusive_scan_u32(int32_t device, uint32_t* data, uint64_t n, uint64_t* total);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_GS_ABI_H */
