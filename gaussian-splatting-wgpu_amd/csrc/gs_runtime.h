// gs_runtime.h -- private to the runtime sources (gs_context / gs_frame / gs_readback / gs_state / gs_export / gs_insert / gs_snapshot / gs_xform / gs_coverage / gs_attr / gs_neigh / gs_cluster / gs_knn / gs_pack / gs_ply / gs_stages .hip):
//   the error channel (fail, HIP_TRY);
//   the owners of HIP resources (Owned: DevBuf, PinnedBuf, Event, Stream, File) and Scratch, a device buffer that grows on demand;
//   the context (gs_ctx, GsOptions, FrameNotes, GraphKey), the lists of its last frame (frame_lists) and sums over its ring (over_ring);
//   what the calls on the resident splats share: the prologue of a call that drains the ring (Plane, resident_check,
//   resident_drain, resident_begin), the last frame waited for (last_frame), the staging of a canvas mask (stage_mask), the
//   coverage planes (cover_planes), the neighbour count plane (neigh_plane), the cluster planes (cluster_planes), the splat edits'
//   selection (edit_select), the bounds kernel's round trip (neigh_bounds; what else the calls over the cell grid share is in
//   gs_neigh_host.h), the pair sort behind a private control block (private_sort and its helpers), the
//   check of a gs_attr (attr_check), the layout of a scene allocation (scene_layout, scene_install), the serial that tells one
//   numbering of the resident splats from the next (gs_ctx::scene_serial, scene_new_serial: what a gs_snapshot is valid for), a file
//   being streamed into the scene (PlySource, PackSource) and the two-buffer trip ring of every streamed call (TripRing).
//   (The file an export writes, FileWriter, is in gs_file_writer.h: it needs no HIP.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/gsplat/gs_abi.h"
#include "gs_kernels.h"
#include "gs_pack_host.h"

#define GS_EXPORT extern "C" __attribute__((visibility("default")))

// ---- errors: one message per thread (gs_last_error), one macro ---------------------------------------------
extern thread_local char g_err[512];
int32_t fail(int32_t code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return fail(e_ == hipErrorOutOfMemory ? GS_ERR_OUT_OF_MEMORY : GS_ERR_HIP, "%s: %s", #expr,      \
                        hipGetErrorString(e_));                                                             \
    } while (0)

// ---- owners: move-only, released by the destructor and by reset(), read like the raw pointer they hold -------
template <class P, auto Destroy>
struct Owned {
    P p = nullptr;
    Owned() = default;
    explicit Owned(P q) : p(q) {}
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : p(o.p) { o.p = nullptr; }
    Owned& operator=(Owned&& o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    ~Owned() { reset(); }
    void reset() { if (p) { (void)Destroy(p); p = nullptr; } }
    P* out() { reset(); return &p; } // for the creating call's out-parameter: whatever was held goes first
    P get() const { return p; }
    operator P() const { return p; }
    P operator->() const { return p; }
};
template <class T = void> using DevBuf = Owned<T*, hipFree>;        // hipMalloc
template <class T = void> using PinnedBuf = Owned<T*, hipHostFree>; // hipHostMalloc
// A device scratch buffer of `cap` elements that only grows: reserve(count) leaves room for at least count of them.  What it held
// is not kept, and is freed BEFORE the larger allocation is made (the smaller one goes first; every earlier call that used it has
// synchronised).  cap is 0 across the allocation, so a failed hipMalloc leaves an empty buffer and not a stale capacity.
template <class T>
struct Scratch : DevBuf<T> {
    uint64_t cap = 0;
    int32_t reserve(uint64_t count) {
        if (count <= cap) return GS_OK;
        cap = 0;
        HIP_TRY(hipMalloc(this->out(), (size_t)count * sizeof(T)));
        cap = count;
        return GS_OK;
    }
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using File = Owned<FILE*, fclose>;

// What record_frame notes about the frame it records (where the sorted result lives, which pipeline ran).  A REPLAY of the
// captured frame restores the capture's notes -- a frame recorded in between (gs_render_debug) would otherwise leave its own.
struct FrameNotes {
    uint32_t *keysS = nullptr, *valsS = nullptr; // views: the sorted result is in keysA/valsA or keysB/valsB (tight frames: no keys)
    uint32_t last_passes = 0;
    uint32_t blend_walkers = 1; // workgroups that walk each tile's list independently in the blend
    bool last_by_index = true;
    bool last_keys16 = false;   // the sorted keys are u16 tile ids (GS_BUF_KEYS is rebuilt on demand into keysG)
    bool last_tight = false;    // the frame used the tight (opacity-aware) binning
};

// What a captured frame depends on beside the buffers: the emission order, the binning, and the addresses it writes.
struct GraphKey {
    bool index = false, tight = false;
    void* ext = nullptr;
    float *alpha = nullptr, *depth = nullptr; // the aux planes (they never move: recorded so that a change cannot go unnoticed)
    bool operator==(const GraphKey& o) const { return index == o.index && tight == o.tight && ext == o.ext && alpha == o.alpha && depth == o.depth; }
};

// What gs_set_option sets and every member of the ring must share: set_option_one writes nowhere else, and a new member takes
// the record whole (add_shadow) -- an option cannot reach the one and miss the other.
struct GsOptions {
    int emit_order = 2;                 // GS_OPT_EMIT_ORDER: 0 depth-bucket order, 1 gaussian-index order (reference), 2 auto
    uint32_t debug_view = 0;            // GS_OPT_DEBUG_VIEW
    bool tile_cull = true;              // GS_OPT_TILE_CULL: tight (opacity-aware) binning in gs_render / gs_render_to
    uint32_t tight_nb = 0;              // GS_OPT_PROJ_CHUNKS: cull chunks per workgroup of the tight projection (0 = automatic)
    uint32_t blend_ablation = 0;        // profiling only (GS_OPT_BLEND_ABLATION)
    uint32_t select_tint = 0x80FFFF00u; // GS_OPT_SELECT_TINT (GS_FLAG_SPLAT_STATE): a<<24 | r<<16 | g<<8 | b
    uint32_t grid_persist = 0;          // GS_OPT_PERSISTENT_GRID: workgroups of the persistent (ticket-loop) kernels; gs_create: 4 per CU
    bool frame_graph = false;           // GS_OPT_FRAME_GRAPH: replay the captured frame
};

#define GS_EV_RING 256
struct gs_ctx {
    ~gs_ctx();
    gs_config cfg{};
    Stream own_stream;            // declared before every buffer: destroyed after them
    hipStream_t stream = nullptr; // view: own_stream, or the caller's cfg.stream
    GsFrame frame{};
    uint32_t T = 0, passes = 0, key_bits = 0; // passes: 8-bit digits of the full key (reference-order pipeline)
    uint32_t tile_passes = 0, tile_bits = 0;  // digits of key/1000 (depth-ordered pipeline)
    bool tile16 = false;                      // every tile id fits 16 bits: the depth-ordered instance sort moves u16 sort words
    bool tight_ok = false;                    // the canvas has at most 255 tile rows and columns (8-bit digits of the row pipeline)
    GsOptions opt;
    DevBuf<uint32_t> blend_prof;              // profiling only (ablation bit 16): 4 words per blend walker
    uint32_t blend_prof_blocks = 0;
    // Frames in flight (GS_OPT_FRAMES_IN_FLIGHT): when gs_render is called while this context's previous frame is still on the
    // device, the frame goes to a SHADOW context (own stream and per-frame arrays, this context's resident splats), created on
    // first need; gs_render then alternates between them, so one frame's blend (instruction-issue bound) overlaps the next
    // frame's projection / binning / sort (memory and latency bound).  gs_wait waits for all of them; read-backs, taps and
    // statistics refer to the context that rendered the LAST frame.
    uint32_t fif = 1;                         // allowed frames in flight (1 = none of the above)
    std::vector<gs_ctx*> shadows;             // owned: gs_destroy'ed before this context's scene goes
    bool is_shadow = false;
    gs_ctx* last = nullptr;                   // who rendered the last frame (this or a shadow); nullptr = this
    uint32_t rr = 0;                          // next slot of the ring {this, shadows...}
    uint64_t cap_hint = 0, row_hint = 0;      // largest capacities any member of the ring has grown to
    // gs_render_host / gs_wait_ticket (root ctx): the event of the last frame + copy of every ring member, who rendered which ticket
    Event ev_done;
    uint64_t next_ticket = 1;
    struct { uint64_t ticket; gs_ctx* member; } tickets[64] = {};
    std::mutex ticket_mu;
    // scene planes
    DevBuf<> scene_own;         // the resident scene, when this context uploaded it
    void* scene_mem = nullptr;  // view: scene_own, or after gs_share_splats the owner's scene_own (the owner must outlive this context)
    size_t scene_bytes = 0;
    GsScene scene{};            // views into scene_mem
    uint32_t n = 0;
    // Which numbering of splats the scene is: drawn from one process-wide counter (scene_new_serial) whenever a scene is installed
    // by gs_upload_*, gs_share_splats or gs_compact; an insertion KEEPS it (old splats keep their indices).  A gs_snapshot names
    // splats by index and stores the serial it was taken under: gs_snapshot_restore / _swap refuse any other (gs_snapshot.hip).
    uint64_t scene_serial = 0;  // 0: no scene yet
    // per-gaussian frame buffers (alloc_per_gaussian)
    DevBuf<uint32_t> counts, offsets, rowptr; // (counts / rowptr hold whole 2048-index chunks: a tight frame keeps its entries there)
    DevBuf<unsigned short> unit_off;          // tight frames: the entries' third plane, the gaussian's index inside its 1024-index unit
    DevBuf<uint32_t> unit_n;                  // ... and the survivors of every unit (2 per chunk + 2; zero past the last unit)
    DevBuf<> gdata;             // n + GS_RECORD_SLACK records (the tight projection's record slots, gs_device.h)
    DevBuf<> grec;              // visible gaussians in (depth bucket, index) order: {id, count word, prefix, arena address} (k_gsort.hip)
    DevBuf<> gsort_scratch;     // (bucket, run) table of the gaussian-level counting sort
    // (key,value) arrays and what grows with them (alloc_kv)
    uint64_t capacity = 0;
    DevBuf<uint32_t> keysA, valsA, keysB, valsB;
    GsSort sort_index{}, sort_tile{}; // the instance sort of the two reference pipelines over these arrays: full key / tile id only
    DevBuf<uint32_t> keysU, valsU;  // debug copies of the unsorted arrays, allocated by the first gs_render_debug
    DevBuf<uint32_t> keysG;         // full keys rebuilt on demand from a frame that holds u16 tile ids or none (GS_BUF_KEYS)
    bool keysG_valid = false;
    // a tight frame's lists name record slots and its records lie in slot order (k_preprocess.hip): the taps that document gaussian
    // ids / index order are rebuilt on demand, once per frame, like keysG (gs_readback.hip)
    DevBuf<uint32_t> valsG;         // GS_BUF_VALUES / GS_BUF_BLOCK_MASKS: gaussian id | sub-block mask << 28
    DevBuf<> gdataG;                // GS_BUF_GAUSSIAN_DATA: N x 64 B in index order, id word cleared, all-zero where the frame left no record
    bool valsG_valid = false, gdataG_valid = false;
    DevBuf<uint32_t> chunk_table;   // balanced emission: first gaussian of every EMIT_CHUNK output slots
    // tight row pipeline (k_rows.hip): row items in projection order / sorted by tile row, slot addresses in depth order
    uint64_t row_cap = 0;
    DevBuf<uint32_t> arena, rows_sorted, M3;
    DevBuf<uint32_t> tileoff, rowtot; // (fixed size: gs_create)
    // control block + look-back status words (one allocation, one memset per frame)
    DevBuf<> ctl_mem;
    size_t ctl_bytes = 0;
    size_t ctl_bytes_tight = 0;               // the part of the control block a tight frame polls: what its memset has to zero
    GsControl* ctl = nullptr;                 // views into ctl_mem, in its order:
    uint32_t* tile_depth = nullptr;           //   blend statistic: deepest staged entry per tile (quadrant kernel)
    uint32_t* rows_status = nullptr;          //   row sort (tight row pipeline)
    unsigned long long* scan_status = nullptr; //  [2][scan blocks]
    uint32_t* sort_status = nullptr;          //   instance sort (reference binning)
    // reports
    PinnedBuf<GsControl> h_ctl; // pinned copy of the control block's counters, fetched on demand (gs_get_stats)
    bool h_ctl_valid = false;
    PinnedBuf<GsReport> h_rep;  // host-mapped: the frame's last binning kernel writes its report here (gs_device.h); no per-frame copy
    DevBuf<uint32_t> sticky;    // device: [0] frames that overflowed, [1] fault, [2] largest I, [3] largest arena demand -- NOT in the
                                // per-frame memset (gs_frame_report)
    uint64_t max_I_seen = 0;       // largest instance count since GS_OPT_RESET_TIMING
    uint64_t truncated_frames = 0; // frames that overflowed the capacity and were NOT the frame gs_wait could re-render
    // outputs
    DevBuf<uint32_t> ranges, rgba8;
    DevBuf<float> rgbf;
    DevBuf<float> alpha, depth; // GS_FLAG_AUX_OUTPUTS: f32[H][slab_w] alpha and accumulated-depth planes, allocated in gs_create (a shadow
                                // inherits the flag and owns its own), never moved afterwards
    DevBuf<uint32_t> d_pxb;     // assemble: pixel boundaries (device copy of pxb_host)
    uint32_t pxb_host[65] = {};
    uint32_t pxb_n = 0;
    // gs_pick (root ctx): device copies of the queries, the results and the contributor records; allocated on first use
    struct { DevBuf<> q, r; Scratch<uint8_t> c; } pick;
    // gs_state_* (gs_state.hip): the matched / count word, device copies of an id list and of a canvas mask (stage_mask); grown on demand
    struct { DevBuf<unsigned long long> counter; Scratch<uint32_t> ids; Scratch<uint8_t> mask; } st;
    // splat edits (gs_export.hip): the selection's per-workgroup counts and its id list; grown on demand
    struct { Scratch<uint32_t> counts, ids; } ex;
    // splat attributes (gs_attr.hip): the summary's slot records, the histogram's bins + 3 words, one trip of values; grown on demand
    struct { DevBuf<unsigned long long> slots; Scratch<unsigned long long> hist; Scratch<float> vals; } at;
    // consensus (gs_consensus.hip): GS_CONSENSUS_MAX count words and the matched slots behind them, the device copy of the hypothesis
    // table (both of fixed size, allocated on first use), and the device copy of one trip of a gather's ids; grown on demand
    struct { DevBuf<unsigned long long> counts; DevBuf<float> params; Scratch<uint32_t> ids; } cs;
    // moments (gs_moments.hip): the slot copies of the limb tables, and one dense plane of N values per attribute that is not a
    // position plane; grown on demand
    struct { DevBuf<unsigned long long> slots; Scratch<float> vals[3]; } mo;
    // pair moments (gs_pairs.hip): the slot copies of the 21 limb tables, and the device copy of a host partner array; grown on demand
    struct { DevBuf<unsigned long long> slots; Scratch<uint32_t> partner; } pr;
    // plane pair moments (gs_plane_pairs.hip): the slot copies of the 29 limb tables, and the device copy of a host normal array as
    // 16-byte records {nx, ny, nz, 0} (the surface plane's layout); grown on demand.  A host partner array goes to pr.partner.
    struct { DevBuf<unsigned long long> slots; Scratch<float> normal; } pp;
    // gs_coverage_* (gs_coverage.hip; root ctx): N x 16 B gs_coverage_rec, allocated and zeroed on first use, dropped with the scene
    DevBuf<> cov;
    // neighbourhoods (gs_neigh.hip): the count plane u32[N], allocated and zeroed on first use, dropped with the scene like cov; the
    // scratch of a count -- the sort's two pairs and private control block, the sorted source / query records, the cell table, the
    // candidates per workgroup, the bounds words -- grown on demand, dropped with the scene too
    struct Neigh {
        DevBuf<uint32_t> plane;
        Scratch<uint32_t> keysA, valsA, keysB, valsB, skeys, bounds;
        Scratch<uint8_t> ctl, src, qry, table;
        Scratch<unsigned long long> sums;
        uint32_t n32 = 0; // the sort's count, copied from here into the private control block
    } ng;
    // clusters (gs_cluster.hip): the label and size planes u32[N], allocated (label = GS_CLUSTER_NONE, size = 0) on first use and
    // dropped with the scene like the count plane; a labelling works in ng's scratch and commits into them at its end
    struct Cluster { DevBuf<uint32_t> label, size; } cl;
    // nearest neighbours (gs_knn.hip): the k-th nearest squared distance f32[N] (held as words) and the nearest source's id u32[N],
    // allocated (NaN 0x7FC00000 / GS_KNN_NONE) on first use and dropped with the scene like the count plane; k: that of the last
    // search without GS_KNN_REFINE (0: none yet), which a refinement must repeat.  A search works in ng's scratch.
    struct Knn { DevBuf<uint32_t> dist2, nearest; uint32_t k = 0; } kn;
    // thinning (gs_thin.hip): the keeper and covers planes u32[N], allocated (keeper = GS_THIN_NONE, covers = 0) on first use and
    // dropped with the scene like the count plane; rank: the u64 per sorted member of a sample, grown on demand and dropped with them.
    // A sample works in ng's scratch beside it and commits into the planes at its end.
    struct Thin { DevBuf<uint32_t> keeper, covers; Scratch<unsigned long long> rank; } th;
    // surface (gs_surface.hip): two 16-byte records per splat, {nx, ny, nz, count} and {l0, l1, l2, 0}, allocated (NaN 0x7FC00000 /
    // count 0) on first use and dropped with the scene like the nearest-neighbour planes; sums: the ten i64 per splat of the last
    // estimate with GS_SURFACE_KEEP_SUMS (have_sums: they are that estimate's), dropped with the planes; the slice's sums of an
    // estimate without the flag and the staging of a read, grown on demand.  An estimate works in ng's scratch.
    struct Surface {
        DevBuf<> nrm, eig;
        DevBuf<int64_t> sums;
        bool have_sums = false;
        Scratch<int64_t> slice;
        Scratch<uint32_t> out;
    } sf;
    // cell merge (gs_merge.hip): the byte planes of the run heads, the merged runs and the members; the compaction's counts; the run
    // begins, the merged runs, the members' ids, the group numbers and the statistics words; one trip of sums and of records.  Grown
    // on demand; the sort works in ng's scratch.
    struct { Scratch<uint8_t> flags, member, rec; Scratch<uint32_t> counts, heads, mruns, ids, group_of, stats; Scratch<double> sums; } mg;
    Event ev[GS_EV_RING][GS_STAGE_COUNT + 1]; // ring of per-frame stage brackets (GS_FLAG_TIMING)
    bool have_events = false;
    uint64_t timed_from = 0; // first frame index included in the stage means
    // frame graph (GS_OPT_FRAME_GRAPH): the frame's launches captured once, replayed with hipGraphLaunch; only the projection's
    // uniforms change from frame to frame (kernel-node parameter update)
    struct {
        bool valid = false;
        hipGraph_t graph = nullptr; // destroyed by drop_graph, before the buffers the capture points into
        hipGraphExec_t exec = nullptr;
        hipGraphNode_t pre_node = nullptr;
        GraphKey key;
        FrameNotes notes; // of the captured frame
        uint64_t frames = 0;
    } gr;
    GsPreprocessLaunch pre{};
    // frame state
    FrameNotes notes; // of the last frame enqueued
    bool have_frame = false, pending = false, last_debug = false;
    void* last_ext = nullptr;
    GsUniforms last_u{};
    uint64_t frames = 0;
};

// gs_context.hip
int32_t alloc_kv(gs_ctx* c, uint64_t capacity, uint64_t row_cap); // the caller has drained the stream
int32_t scene_alloc(gs_ctx* c, uint64_t n, uint64_t min_capacity = 0, uint64_t min_rows = 0); // min_*: capacities a compaction keeps
// The layout of a scene allocation as a function of (n, state plane or not): the views of a scene of n gaussians that starts at
// `base` (null: only np, state_at and bytes mean anything), the plane stride in gaussians, the offset of the state plane and the
// bytes of the whole.  scene_alloc and the splat insertion (which builds the new scene beside the old one) share this one copy.
struct GsSceneLayout {
    GsScene scene{};
    size_t np = 0, state_at = 0, bytes = 0;
};
GsSceneLayout scene_layout(void* base, uint64_t n, bool state);
// scene_alloc with the scene given: drops the previous scene and the per-gaussian work arrays, allocates those for n gaussians
// and takes `mem` (complete, laid out by scene_layout) as the resident scene
int32_t scene_install(gs_ctx* c, DevBuf<>&& mem, uint64_t n, uint64_t min_capacity, uint64_t min_rows);
// the next value of the process-wide scene counter (never 0): scene_alloc and gs_share_splats give it to c->scene_serial,
// scene_install does not
uint64_t scene_new_serial();
void drop_shadows(gs_ctx* c);
// gs_frame.hip
void drop_graph(gs_ctx* c);
int32_t wait_one(gs_ctx* c);
// The lists of the last frame `c` enqueued, as the blend of that frame and the queries on it read them.  The one place that
// knows that a tight frame's values carry the sub-block mask above the record slot.
GsLists frame_lists(const gs_ctx* c);
// The sum -- or the maximum -- of get(member) over the ring {root, its shadows}.
template <class Get>
uint64_t over_ring(const gs_ctx* root, Get get, bool maximum = false) {
    uint64_t v = get(root);
    for (const gs_ctx* s : root->shadows) v = maximum ? std::max<uint64_t>(v, get(s)) : v + get(s);
    return v;
}
// gs_state.hip: the prologue of a call on the resident splats that drains the ring.  resident_check holds the refusals that cost
// nothing, in this order: null context, a filter that does not fit the state byte (Plane::filtered), a context without
// GS_FLAG_SPLAT_STATE where the call needs the plane, no scene.  resident_drain is gs_wait (an error of the wait is the call's
// error: nothing is applied), hipSetDevice and, with `counter`, the allocation of st.counter.  resident_begin is one after the
// other, for the calls that check their own arguments after the drain.
enum class Plane {
    none,     // the call reads no state plane
    filtered, // ... reads it for a filter other than (0, 0), which matches every splat
    always    // ... is refused without it
};
int32_t resident_check(gs_ctx* c, const char* who, Plane need, uint32_t mask = 0, uint32_t value = 0);
int32_t resident_drain(gs_ctx* c, bool counter = false);
inline int32_t resident_begin(gs_ctx* c, const char* who, Plane need, uint32_t mask = 0, uint32_t value = 0) {
    const int32_t rc = resident_check(c, who, need, mask, value);
    return rc != GS_OK ? rc : resident_drain(c);
}
// a canvas mask (u8[height][width] of the root's canvas) copied to root->st.mask on `st`; *dev: the device copy
int32_t stage_mask(gs_ctx* root, const uint8_t* mask, hipStream_t st, const uint8_t** dev);
// gs_readback.hip: the ring member that rendered the last frame, waited for if it is pending, its device current.  who: refuses
// with GS_ERR_NO_FRAME when no frame was rendered (null: the caller copes with that)
int32_t last_frame(gs_ctx* root, const char* who, gs_ctx** c);
// gs_coverage.hip: the coverage planes of the root context, allocated and zeroed (on `st`) by the first call that needs them
int32_t cover_planes(gs_ctx* root, hipStream_t st);
// gs_neigh.hip: the neighbour count plane of `c`, allocated and zeroed (on `st`) by the first call that needs it
int32_t neigh_plane(gs_ctx* c, hipStream_t st);
size_t plane_bytes(const gs_ctx* c); // of a u32[N] plane: whole 16-byte groups (the state pass reads a uint4 per thread)
// gs_neigh.hip: the bounds kernel under a source and a query filter (state: the plane, or null when both are (0, 0)): seeds the 16
// words, launches, reads them back into hb and synchronises.  hb[0..2] / [3..5]: pk_okey of the finite sources' lowest / highest
// coordinates; hb[6..9]: sources, finite sources, queried, finite queried.
int32_t neigh_bounds(gs_ctx* c, const uint8_t* state, uint32_t smask, uint32_t svalue, uint32_t qmask, uint32_t qvalue, uint32_t hb[16],
                     const uint32_t* gate = nullptr);
// The pair sort behind a private control block -- the frame path's instance sort outside a frame: 8-bit digits of the key itself,
// counted by the sort.  private_sort_bytes: the control block and the status words of `passes` passes over n pairs that follow it.
// private_sort_plan: the plan over four arrays.  gs_sort_pairs_u32 has no context and drives these two itself; a call on a context
// uses private_sort, which on c->stream reserves c->ng's four arrays and ctl for n pairs (private_sort_reserve: a caller that must
// not fail later reserves for its largest `passes` up front), zeroes the block, sets the count, calls keys() -- it enqueues what
// writes ng.keysA / valsA -- and launches the sort; *sorted: the pair that holds the result.  private_sort_fault enqueues the read of
// the block's fault word (set when a look-back exceeded its spin bound); it must be waited for before the next private_sort.
static constexpr size_t kCtlBytes = (sizeof(GsControl) + 255) & ~(size_t)255;
inline size_t private_sort_bytes(uint64_t n, uint32_t passes) { return kCtlBytes + (size_t)passes * gs_sort_tiles(n) * 256 * 4; }
inline GsSort private_sort_plan(uint32_t* keysA, uint32_t* valsA, uint32_t* keysB, uint32_t* valsB, uint32_t passes) {
    return GsSort{{keysA, valsA}, {keysB, valsB}, passes, 8, 0, false, false};
}
inline int32_t private_sort_reserve(gs_ctx* c, uint32_t n, uint32_t passes) {
    gs_ctx::Neigh& s = c->ng;
    int32_t rc;
    if ((rc = s.keysA.reserve(n)) != GS_OK || (rc = s.valsA.reserve(n)) != GS_OK || (rc = s.keysB.reserve(n)) != GS_OK ||
        (rc = s.valsB.reserve(n)) != GS_OK)
        return rc;
    return s.ctl.reserve(private_sort_bytes(n, passes));
}
template <class Keys>
int32_t private_sort(gs_ctx* c, uint32_t n, uint32_t passes, Keys keys, GsSortPair* sorted) {
    gs_ctx::Neigh& s = c->ng;
    const int32_t rc = private_sort_reserve(c, n, passes);
    if (rc != GS_OK) return rc;
    HIP_TRY(hipMemsetAsync(s.ctl, 0, private_sort_bytes(n, passes), c->stream));
    GsControl* ctl = (GsControl*)s.ctl.get(); // view; the sort's status words follow it
    s.n32 = n;
    HIP_TRY(hipMemcpyAsync(&ctl->num_intersections, &s.n32, 4, hipMemcpyHostToDevice, c->stream));
    keys();
    *sorted = gs_launch_sort(private_sort_plan(s.keysA, s.valsA, s.keysB, s.valsB, passes), ctl, (uint32_t*)(s.ctl.get() + kCtlBytes), n,
                             std::max(c->opt.grid_persist, 1u), c->stream);
    return GS_OK;
}
inline int32_t private_sort_fault(gs_ctx* c, uint32_t* fault) {
    HIP_TRY(hipMemcpyAsync(fault, &((const GsControl*)c->ng.ctl.get())->fault, 4, hipMemcpyDeviceToHost, c->stream));
    return GS_OK;
}
// gs_cluster.hip: the label and size planes of `c`, allocated and set to their initial reading (on `st`) by the first call that needs them
int32_t cluster_planes(gs_ctx* c, hipStream_t st);
// gs_knn.hip: the nearest-neighbour planes of `c`, allocated and set to their initial reading (on `st`) by the first call that needs them
int32_t knn_planes(gs_ctx* c, hipStream_t st);
// gs_thin.hip: the keeper and covers planes of `c`, allocated and set to their initial reading (on `st`) by the first call that needs them
int32_t thin_planes(gs_ctx* c, hipStream_t st);
// gs_surface.hip: the surface planes of `c`, allocated and set to their initial reading (on `st`) by the first call that needs them
int32_t surface_planes(gs_ctx* c, hipStream_t st);
// gs_export.hip: the splat edits' selection: counts the splats with (s & mask) == value and, with want_ids, leaves their indices,
// ascending, in c->ex.ids
int32_t edit_select(gs_ctx* c, uint32_t mask, uint32_t value, bool want_ids, uint64_t* total);
// records per trip through the bounce buffer of the host export and of the host write-back (320 MB)
static constexpr uint64_t kBounceRecords = 1ull << 20;
// gs_ply.hip: what decodeHeader (ply.ts:49-102) and PackedGaussians' constructor (:162-228) derive from the header: where the vertex
// data starts, the vertex count and stride, and for each of the 11 + 3 (degree + 1)^2 values of a packed record its byte offset and
// type in a vertex and its float slot in the 320-byte record (ply.ts:190-198).
struct PlyLayout {
    uint64_t data_off = 0, vertex_count = 0;
    uint32_t stride = 0;
    int degree = 0, nsrc = 0;
    uint32_t soff[11 + 48], stype[11 + 48], slot[11 + 48];
    bool all_float = true;
};
// A file being streamed into the scene, in two forms with the same three members (upload_source below and append_source, gs_insert.hip,
// are written once over them).  open: opens the file, reads its header and refuses what cannot be streamed; allocates nothing on the
// device.  count: its vertices.  stream: vertex v becomes splat first + v of `dst` (a scene that has room for them) in trips of
// kStreamTrip vertices through a TripRing with device staging, converted on the device while the next trip is being read; returns
// when the stream is done.  `who` names the caller in the messages.
static constexpr uint64_t kStreamTrip = 65536; // vertices per trip: 256 whole chunks of a packed file
// gs_ply.hip: a .ply.  Refused: 2^31 vertices or more, a vertex stride above 0xFFFF, a file shorter than data_off + count * stride.
// stream zeroes the SH of the new splats first when the file's degree is below 3.
struct PlySource {
    File fp;
    PlyLayout L;
    int32_t open(const char* who, const char* path);
    uint64_t count() const { return L.vertex_count; }
    int32_t stream(const char* who, gs_ctx* c, const GsScene& dst, uint64_t first);
};
// gs_pack.hip: a packed file.  Refused: a header that is not exactly the format's, a size other than the header implies (gs_pack_host.h).
struct PackSource {
    File fp;
    GsPackLayout L;
    int32_t open(const char* who, const char* path);
    uint64_t count() const { return L.n; }
    int32_t stream(const char* who, gs_ctx* c, const GsScene& dst, uint64_t first);
};
// gs_upload_ply / gs_upload_packed: the file becomes the scene (the file is opened before anything of the context is dropped)
template <class Source>
int32_t upload_source(const char* who, gs_ctx* c, const char* path, uint64_t* n_out) {
    if (!c || !path) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null argument", who);
    Source src;
    int32_t rc = src.open(who, path);
    if (rc != GS_OK) return rc;
    hipError_t he = hipSetDevice(c->cfg.device);
    if (he != hipSuccess) return fail(GS_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(he));
    drop_shadows(c);
    rc = scene_alloc(c, src.count());
    if (rc != GS_OK) return rc;
    rc = src.stream(who, c, c->scene, 0);
    if (rc != GS_OK) return rc;
    if (n_out) *n_out = src.count();
    return GS_OK;
}
// The two-buffer trip ring of every streamed call: two pinned host buffers and two events (with `device`, two device staging buffers
// beside them), so that the host works on one trip while the device copies the other.  Peak host memory is the two buffers, whatever
// the size of the scene.  An early exit of a caller frees the pinned buffers under a copy still in flight: the free waits for the device.
struct TripRing {
    PinnedBuf<unsigned char> h[2];
    DevBuf<unsigned char> d[2];
    Event done[2];
    int32_t init(size_t bytes, bool device) {
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(hipHostMalloc(h[k].out(), bytes, hipHostMallocDefault));
            if (device) HIP_TRY(hipMalloc(d[k].out(), bytes));
            HIP_TRY(hipEventCreateWithFlags(done[k].out(), hipEventDisableTiming));
        }
        return GS_OK;
    }
    // file -> device: trip(it, pinned, staging) fills the pinned buffer from the file and enqueues the copy and the kernel on `st`
    template <class Trip>
    int32_t feed(uint64_t trips, hipStream_t st, Trip trip) {
        for (uint64_t it = 0; it < trips; ++it) {
            const int k = (int)(it & 1u);
            if (it >= 2) HIP_TRY(hipEventSynchronize(done[k])); // the copy out of this pinned buffer two trips ago has finished
            const int32_t rc = trip(it, h[k].get(), d[k].get());
            if (rc != GS_OK) return rc;
            HIP_TRY(hipEventRecord(done[k], st));
        }
        return GS_OK;
    }
    // device -> file: enqueue(it, pinned) enqueues the kernel and the copy into the pinned buffer on `st`; consume(it, pinned) writes
    // trip it - 1 while that copy runs (its pinned buffer is not written again before trip it + 1 is enqueued).  The last trip is
    // consumed before the call returns.
    template <class Enqueue, class Consume>
    int32_t drain(uint64_t trips, hipStream_t st, Enqueue enqueue, Consume consume) {
        for (uint64_t it = 0; it <= trips && trips; ++it) {
            int32_t rc;
            if (it < trips) {
                if ((rc = enqueue(it, h[it & 1u].get())) != GS_OK) return rc;
                HIP_TRY(hipEventRecord(done[it & 1u], st));
            }
            if (it >= 1) {
                HIP_TRY(hipEventSynchronize(done[(it - 1) & 1u]));
                if ((rc = consume(it - 1, h[(it - 1) & 1u].get())) != GS_OK) return rc;
            }
        }
        return GS_OK;
    }
};
// gs_attr.hip: the refusals of a gs_attr (null, struct_size, kind, a non-finite p of the kinds that read it) in `who`'s name; *dev:
// its parameters as the kernels take them.  attr_needs_cover: the kind reads the coverage planes (cover_planes first)
int32_t attr_check(const char* who, const gs_attr* a, GsAttrDev* dev);
inline bool attr_needs_cover(const gs_attr* a) { return a->kind >= GS_ATTR_COVER_HITS; }
inline gs_ctx* last_of(gs_ctx* c) { return (c && c->last) ? c->last : c; }
inline bool has_state(const gs_ctx* c) { return (c->cfg.flags & GS_FLAG_SPLAT_STATE) != 0; }
inline GsTint tint_of(uint32_t argb) { // a<<24 | r<<16 | g<<8 | b -> what the projection applies (each quotient one f32 division)
    return GsTint{{(float)((argb >> 16) & 255u) / 255.0f, (float)((argb >> 8) & 255u) / 255.0f, (float)(argb & 255u) / 255.0f},
                  (float)(argb >> 24) / 255.0f};
}
