// gs_kernels.h -- host-side launchers of the gfx950 kernels (definitions next to each kernel).
#pragma once
#include "gs_device.h"
#include "gs_consensus_host.h" // GsAttrDev
#include "gs_grid_math.h"      // GsNeighGrid

void gs_launch_repack(const void* d_aos, uint32_t n, uint32_t first, const GsScene& s, hipStream_t st); // record r -> splat first + r
void gs_launch_ply_chunk(const void* d_raw, uint32_t m, uint32_t first, const GsPlyTable& t, const GsScene& s, hipStream_t st);
struct GsPreprocessLaunch { // the projection's launch as data (its uniforms, and w2 derived from them, are the only kernel arguments that change per frame)
    const void* func;
    uint32_t blocks;
    GsScene s; GsUniforms u; GsFrame f;
    void* gdata; uint32_t* counts; GsTightOut to; GsTint tint;
    float w2; // slab reach cull: >= the squared spectral norm of u.view's 3x3 (gs_view_norm2)
    void* args[8];
};
float gs_view_norm2(const GsUniforms& u);
// state: the STATE instantiation (honours s.state and the tint); false launches exactly the kernels a context without the plane has
void gs_preprocess_prepare(GsPreprocessLaunch& L, const GsScene& s, const GsUniforms& u, const GsFrame& f, void* gdata, uint32_t* counts,
                           bool tight, uint32_t* arena, uint32_t* rowptr, unsigned short* unit_off, uint32_t* unit_n, GsControl* ctl,
                           uint32_t tight_nb = 0, bool state = false, GsTint tint = GsTint{});
void gs_launch_preprocess(GsPreprocessLaunch& L, hipStream_t st);
void gs_launch_zero(void* p, uint64_t bytes, hipStream_t st); // bytes: a multiple of 16
uint32_t gs_scan_blocks(uint32_t n);
void gs_launch_scan(const uint32_t* counts, uint32_t n, uint32_t* offsets, unsigned long long* status, uint32_t* ticket, GsControl* ctl,
                    hipStream_t st);
uint64_t gs_emit_chunks(uint64_t capacity);
// grec: the gaussian-level sort's records {id, count word, first output slot, -} in (bucket, index) order
void gs_launch_emit_balanced(const void* gdata, const void* grec, const uint32_t* chunk_table, const GsFrame& f, uint32_t* keys, uint32_t* values,
                             GsControl* ctl, uint32_t grid, uint32_t hist_bits, uint32_t hist_passes, bool keys16, hipStream_t st);
void gs_launch_emit(const void* gdata, const uint32_t* counts, const uint32_t* offsets, const GsFrame& f, uint32_t* keys, uint32_t* values,
                    GsControl* ctl, hipStream_t st);
void gs_launch_ranges16(const uint16_t* tiles, const GsControl* ctl, uint32_t capacity, uint32_t T, uint32_t* ranges, uint32_t grid,
                        uint32_t* sticky, GsReport* rep, hipStream_t st);
void gs_launch_rebuild_keys(const uint16_t* tiles, const uint32_t* vals, const uint32_t* counts, uint32_t count, uint32_t n, uint32_t* keys,
                            hipStream_t st);
void gs_launch_ranges(const uint32_t* keys, const GsControl* ctl, uint32_t capacity, uint32_t T, uint32_t* ranges, uint32_t grid,
                      uint32_t* sticky, GsReport* rep, hipStream_t st);
uint32_t gs_sort_tiles(uint64_t capacity);
// One instance sort: the pair of arrays that holds the input, the pair the sweeps alternate with, and the digit plan -- `passes`
// digits of `bits` bits of the sort word (the key, or key/1000 when by_tile).  keys16: the key arrays hold uint16_t sort words
// (by_tile must be 0 and have_hist true).  have_hist: the digit counts are already in ctl->hist (the balanced emission leaves them).
struct GsSortPair { uint32_t *keys, *vals; };
struct GsSort {
    GsSortPair in, alt;
    uint32_t passes, bits, by_tile;
    bool keys16, have_hist;
};
GsSortPair gs_launch_sort(const GsSort& s, GsControl* ctl, uint32_t* status, uint32_t capacity, uint32_t grid, hipStream_t st); // the pair that holds the result
// The lists of one frame as their readers take them (blend, pick, coverage): the projection's records, the values in list order, the
// per-tile ranges, the frame geometry, and the mask that leaves a value's record slot (GS_ID_MASK where the sub-block mask of the
// tight binning rides above it, all ones otherwise).  A value names the record at gdata + 64 * slot; the gaussian's id is word 2
// of that record (slot = id on a frame of the reference's binning).  nrec: records the array holds.
struct GsLists {
    const void* gdata;
    const uint32_t* values;
    const uint32_t* ranges;
    GsFrame f;
    uint32_t id_mask;
    uint32_t nrec;
};
int gs_launch_blend(const GsLists& L, uint32_t* rgba8, float* rgbf, bool aux, float* alpha, float* depth, GsControl* ctl, uint32_t* tile_depth,
                    bool exact, uint32_t ablation, hipStream_t st, uint32_t* prof = nullptr, uint32_t* prof_blocks = nullptr);
void gs_launch_debug_view(const uint32_t* ranges, const GsFrame& f, uint32_t view, uint32_t* rgba8, hipStream_t st);
void gs_launch_assemble(const void* slabs, void* image, uint32_t width, uint32_t height, const uint32_t* d_px_bounds, uint32_t n_slabs,
                        uint64_t slab_stride_px, hipStream_t st);
// k_gsort.hip: the visible gaussians sorted by depth bucket (stable) with their quantity (tile count / row-item slots) scanned in that order
uint32_t gs_gsort_tiles(uint32_t n);
uint64_t gs_gsort_scratch_bytes(uint32_t n);
// Two input forms.  unit_n == nullptr: words (and aux_in, optional) hold one word per gaussian INDEX.  Otherwise the tight projection's
// entries: per 1024-index unit u, unit_n[u] survivors in index order at u * 1024 + e of words / aux_in / unit_off (the index inside the
// unit); the planes hold gs_gsort_tiles(n) * 2048 entries, unit_n 2 * gs_gsort_tiles(n) + 2 words (zero past the last unit).
void gs_launch_gsort(const uint32_t* words, const uint32_t* aux_in, const unsigned short* unit_off, const uint32_t* unit_n, uint32_t n, void* scratch,
                     void* grec, uint32_t* chunk_table, uint32_t chunk_cap, uint32_t* tot_visible, uint32_t* tot_quantity, uint32_t grid, hipStream_t st);
// k_rows.hip: the tight row pipeline (row sort, per-chunk counts, scan, expansion into the final per-tile lists + ranges)
uint32_t gs_rows_sort_tiles(uint64_t row_cap);
uint32_t gs_rows_chunks(uint64_t row_cap);
size_t gs_rows_sorted_bytes(uint64_t row_cap); // rows_sorted: an 8-byte payload plane and a 2-byte span plane for row_cap items (k_rows.hip)
void gs_launch_rows(const uint32_t* arena, const void* grec, const uint32_t* chunk_table, uint32_t* rows_sorted, GsControl* ctl, uint32_t* sort_status, uint32_t row_cap,
                    uint32_t* M3, uint32_t* tileoff, uint32_t* rowtot, const GsFrame& f, uint32_t* values, uint32_t* ranges, uint32_t cus,
                    uint32_t* sticky, GsReport* rep, hipStream_t st, void (*mark)(void*, int), void* mark_arg);
// the taps of a tight frame, whose lists name record slots (gdata: its records, nrec of them): the keys; the values with the
// gaussian's id in the slot's place (ids_out, may be null); the records in index order, id word cleared (gdata_out, zeroed by the
// caller, may be null)
void gs_launch_rows_rebuild_keys(const uint32_t* ranges, uint32_t T, const uint32_t* vals, const void* gdata, uint32_t nrec, uint32_t count, uint32_t n,
                                 uint32_t* keys, hipStream_t st);
void gs_launch_rows_rebuild_taps(const uint32_t* vals, const void* gdata, uint32_t nrec, uint32_t count, uint32_t n, uint32_t* ids_out, void* gdata_out,
                                 hipStream_t st);
// k_state.hip: the state plane's streaming kernels (gs_state.hip).  The plane is 256-byte aligned with np >= n bytes behind it.
struct GsRegionDev { // a gs_region as the kernel reads it
    float a[3], b[3];       // SPHERE: centre, radius in b[0].  BOX: min, max
    float x0, y0, x1, y1;   // SCREEN_RECT bounds as f32
    float W, H;             // canvas size as f32
    uint32_t wi, hi;        // ... and as integers (mask stride and bound)
    float proj[16];         // the camera's proj (= P * V), column-major
    float viewz[4];         // row 2 of its view matrix: m[2], m[6], m[10], m[14]
    const uint8_t* mask;    // SCREEN_MASK: device u8[hi][wi]
};
// `matched` / `count` are GS_STATE_SLOTS partial sums, GS_STATE_SLOT_STRIDE words (256 bytes) apart, zeroed by the caller and added up
// on the host: a workgroup adds to slot (workgroup % GS_STATE_SLOTS).  One word would take every workgroup's atomic in turn: 5 958
// of them at 6.1 M splats were 76 us of a kernel that moves its 79 MB in 20 (profiles/state_ops.txt).
#define GS_STATE_SLOTS 32
#define GS_STATE_SLOT_STRIDE 32
void gs_launch_state_region(uint32_t kind, uint8_t* state, const GsScene& s, uint32_t n, const GsRegionDev& r, uint32_t op, uint32_t bits,
                            uint32_t where_mask, uint32_t where_value, unsigned long long* matched, hipStream_t st);
void gs_launch_state_ids(uint8_t* state, const uint32_t* ids, uint64_t n, uint32_t op, uint32_t bits, hipStream_t st);
void gs_launch_state_count(const uint8_t* state, uint32_t n, uint32_t mask, uint32_t value, unsigned long long* count, hipStream_t st);
// gs_state_coverage: the region pass with a membership read from the coverage planes (16 bytes per splat: gs_coverage_rec)
void gs_launch_state_coverage(uint8_t* state, const void* planes, uint32_t n, uint32_t min_hits, float min_weight, uint32_t covered, uint32_t op,
                              uint32_t bits, uint32_t where_mask, uint32_t where_value, unsigned long long* matched, hipStream_t st);
// k_attr.hip: the splat attributes (gs_attr.hip; gs_state_attr in gs_state.hip).  kind: GS_ATTR_* (checked by the caller); cov: the
// coverage planes, read by the COVER_* kinds only; state: null = every splat passes (the (0, 0) filter: the plane is not read).
// (GsAttrDev, a gs_attr's parameters as the kernels read them, is gs_consensus_host.h's: the host loop of the consensus calls reads it too)
// the state pass of gs_launch_state_region around (v >= lo && v <= hi) == inside
void gs_launch_attr_state(uint32_t kind, uint8_t* state, const GsScene& s, const void* cov, uint32_t n, const GsAttrDev& a, float lo, float hi,
                          uint32_t inside, uint32_t op, uint32_t bits, uint32_t where_mask, uint32_t where_value, unsigned long long* matched,
                          hipStream_t st);
// slots: GS_STATE_SLOTS records GS_STATE_SLOT_STRIDE words apart, a workgroup folds into record (workgroup % GS_STATE_SLOTS); the
// caller initialises them (matched = nan = 0, kmin = 0xFFFFFFFF, kmax = 0) and folds them.  Keys: the order-preserving map of gs_abi.h.
struct GsAttrSlot { unsigned long long matched, nan; uint32_t kmin, kmax; };
void gs_launch_attr_summary(uint32_t kind, const uint8_t* state, const GsScene& s, const void* cov, uint32_t n, const GsAttrDev& a, uint32_t mask,
                            uint32_t value, unsigned long long* slots, hipStream_t st);
// counts: bins + 3 words, zeroed by the caller (bins, below, above, NaN); grid: workgroups of the grid-stride loop (clamped to the work)
void gs_launch_attr_histogram(uint32_t kind, const uint8_t* state, const GsScene& s, const void* cov, uint32_t n, const GsAttrDev& a, uint32_t mask,
                              uint32_t value, float lo, float hi, float scale, uint32_t bins, unsigned long long* counts, uint32_t grid, hipStream_t st);
// out[g] = v of splat ids[first + g], or of splat first + g when ids is null, g = 0 .. m
void gs_launch_attr_values(uint32_t kind, const GsScene& s, const void* cov, uint32_t n, const GsAttrDev& a, const uint32_t* ids, uint32_t first,
                           uint32_t m, float* out, hipStream_t st);
// k_consensus.hip: consensus (gs_consensus.hip).  kind: GS_ATTR_DIST2 or GS_ATTR_PLANE (checked by the caller).  params: f32[hp][4] on the
// device, hp = h rounded up to GS_CONSENSUS_PAD hypotheses, the padding filled with NaNs (a NaN parameter counts nothing).  counts: hp
// u64 words, zeroed by the caller: counts[j] += splats that pass the filter with lo <= v_j <= hi.  slots: the GS_STATE_SLOTS partial
// sums of `matched`, zeroed by the caller, who also adds them.  grid: workgroups of the grid-stride loop (clamped to the work).
#define GS_CONSENSUS_PAD 8u
void gs_launch_consensus(uint32_t kind, const uint8_t* state, const float* px, const float* py, const float* pz, uint32_t n, const float* params,
                         uint32_t hp, float lo, float hi, uint32_t mask, uint32_t value, unsigned long long* counts, unsigned long long* slots,
                         uint32_t grid, hipStream_t st);
// k_moments.hip: moments (gs_moments.hip).  Exact sums and sums of products (j <= l, gs_abi.h's order) of `planes` f32 planes, 1 .. 3 (the
// same plane may be given twice), over the splats that pass the filter and whose values are all finite.  slots: GS_MOMENTS_SLOTS copies
// GS_MOMENTS_SLOT_WORDS words apart, zeroed by the caller; a workgroup adds to copy (workgroup % GS_MOMENTS_SLOTS).  A copy is
// Q = planes + planes (planes + 1) / 2 tables of GS_EX_LIMBS signed 64-bit limbs (gs_exact_sum.h), the sums first, then matched,
// counted.  The caller adds the copies.  grid: workgroups of the grid-stride loop (clamped to the work).
#define GS_MOMENTS_SLOTS 8
#define GS_MOMENTS_SLOT_WORDS 192 // >= 9 * 20 + 2, a multiple of 32 words
void gs_launch_moments(uint32_t planes, const uint8_t* state, const float* p0, const float* p1, const float* p2, uint32_t n, uint32_t mask,
                       uint32_t value, unsigned long long* slots, uint32_t grid, hipStream_t st);
// k_pairs.hip: pair moments (gs_pairs.hip).  The exact sums over the pairs (p_i, p_partner[i]) of the splats that pass the filter: 21
// tables of GS_EX_LIMBS limbs in gs_pair_host.h's order, then matched, paired.  partner: u32[n] on the device, read as a uint4 per
// whole quad; an id >= n is never an index.  slots: GS_PAIRS_SLOTS copies GS_PAIRS_SLOT_WORDS words apart, zeroed by the caller, who
// also adds them; a workgroup adds to copy (workgroup % GS_PAIRS_SLOTS).  grid: workgroups of the grid-stride loop (clamped to the work).
#define GS_PAIRS_SLOTS 8
#define GS_PAIRS_SLOT_WORDS 448 // >= 21 * 20 + 2, a multiple of 32 words
void gs_launch_pairs(const uint8_t* state, const float* px, const float* py, const float* pz, const uint32_t* partner, uint32_t n, uint32_t mask,
                     uint32_t value, float max_d2, unsigned long long* slots, uint32_t grid, hipStream_t st);
// k_plane_pairs.hip: plane pair moments (gs_plane_pairs.hip).  The exact sums of the point-to-plane normal equations over the pairs
// (p_i, p_partner[i], normal[partner[i]]) of the splats that pass the filter: 29 tables of GS_EX_LIMBS limbs in gs_plane_pair_host.h's
// order, then matched, paired.  partner as for gs_launch_pairs; normal: n 16-byte records {nx, ny, nz, any} on the device (the surface
// plane, or a staged host array), gathered by partner id only.  pivot: three floats by value.  slots: GS_PLANE_PAIRS_SLOTS copies
// GS_PLANE_PAIRS_SLOT_WORDS words apart, zeroed by the caller, who also adds them.  grid as for gs_launch_pairs.
#define GS_PLANE_PAIRS_SLOTS 8
#define GS_PLANE_PAIRS_SLOT_WORDS 608 // >= 29 * 20 + 2, a multiple of 32 words
void gs_launch_plane_pairs(const uint8_t* state, const float* px, const float* py, const float* pz, const uint32_t* partner, const void* normal,
                           uint32_t n, uint32_t mask, uint32_t value, float pvx, float pvy, float pvz, float max_d2, unsigned long long* slots,
                           uint32_t grid, hipStream_t st);
// k_neigh.hip: neighbourhoods (gs_neigh.hip) over the cell grid of the finite sources (GsNeighGrid, gs_grid_math.h).
// out: 16 words the caller initialises ([0..2] all ones, the rest 0): min / max order-preserving keys of x, y, z over the finite
// sources, then sources, finite sources, queries, finite queries.  state null: every splat passes both filters.  gate (u32[n], or
// null: no gate): a splat is a query -- in keys: a member -- only if its word there is +inf's (a refining gs_knn_search; null for
// every other caller).
void gs_launch_neigh_bounds(const uint8_t* state, const GsScene& s, uint32_t n, uint32_t smask, uint32_t svalue, uint32_t qmask, uint32_t qvalue,
                            const uint32_t* gate, uint32_t* out, hipStream_t st);
void gs_launch_neigh_keys(const uint8_t* state, const GsScene& s, uint32_t n, uint32_t mask, uint32_t value, const uint32_t* gate, const GsNeighGrid& g,
                          uint32_t* keys, uint32_t* vals, hipStream_t st);
// the sorted pairs -> {x, y, z, id} records (16 B, n of them allocated) and, with `table` (blocks x {start, end}, zeroed), the
// members' keys in sorted order (skeys, n allocated) and each block's run
void gs_launch_neigh_records(const uint32_t* keys, const uint32_t* vals, uint32_t n, const GsNeighGrid& g, const GsScene& s, void* rec, uint32_t* skeys,
                             void* table, hipStream_t st);
// What the candidates kernel, the query passes and the clusters' edge pass read of the sources: the records and their keys in cell
// order, the {start, end} table.  nrec bounds what a table entry may name (it never names more: gs_neigh_records_kernel).
struct NeighSources {
    const float4* __restrict__ rec;
    const uint32_t* __restrict__ keys;
    const uint2* __restrict__ table;
    uint32_t nrec;
};
// The built grid as a launch takes it (neigh_build fills it: NeighBuilt, gs_neigh_host.h): the sources, the nqry query records in
// cell order (the sources' own when both filters are the same) and the grid.
struct NeighView { NeighSources src{}; const float4* qrec = nullptr; uint32_t nqry = 0; GsNeighGrid g{}; };
// sums[b]: candidates of sorted queries 256 b .. 256 b + 255
void gs_launch_neigh_cands(const NeighView& v, unsigned long long* sums, hipStream_t st);
// the query pass over workgroups [first_block, first_block + blocks) of 256 sorted queries: plane[id] = min(limit, count)
void gs_launch_neigh_query(const NeighView& v, uint32_t first_block, uint32_t blocks, float r2, uint32_t limit, uint32_t n, uint32_t* plane, hipStream_t st);
// gs_state_neigh: the state pass with a membership read from the count plane (u32[n], 16-byte aligned)
void gs_launch_state_neigh(uint8_t* state, const uint32_t* plane, uint32_t n, uint32_t min_count, uint32_t max_count, uint32_t inside, uint32_t op,
                           uint32_t bits, uint32_t where_mask, uint32_t where_value, unsigned long long* matched, hipStream_t st);
// k_cluster.hip: clusters (gs_cluster.hip): a union-find over parent[n] (indexed by splat: a member starts as its own root, a
// non-member holds GS_CLUSTER_NONE) fed by the neighbourhoods' candidate walk over the members' sorted records.
// parent / count of every splat: count = 1 for a member with a non-finite coordinate (it has no record), else 0
void gs_launch_cluster_init(const uint8_t* state, const GsScene& s, uint32_t n, uint32_t mask, uint32_t value, uint32_t* parent, uint32_t* count,
                            hipStream_t st);
// the edge pass over workgroups [first_block, first_block + blocks) of 256 sorted members (v.src's records are queries and sources
// alike: v.qrec is not read); *changed |= 1 when a root was hooked
void gs_launch_cluster_edges(const NeighView& v, uint32_t first_block, uint32_t blocks, float r2, uint32_t n, uint32_t* parent, uint32_t* changed,
                             hipStream_t st);
void gs_launch_cluster_flatten(const void* rec, uint32_t nrec, uint32_t n, uint32_t* parent, hipStream_t st); // parent[id] = its root
// count[root] += the records under it (flat trees); fold: one add per wave and distinct root
void gs_launch_cluster_sizes(const void* rec, uint32_t nrec, uint32_t n, const uint32_t* parent, uint32_t* count, bool fold, hipStream_t st);
// the two planes from parent / count; slots: the GS_STATE_SLOTS partial records (zeroed by the caller), word 0 += clusters, word 1 =
// max(word 1, largest size)
void gs_launch_cluster_commit(const uint32_t* parent, const uint32_t* count, uint32_t n, uint32_t* labels, uint32_t* sizes, unsigned long long* slots,
                              hipStream_t st);
// gs_state_cluster_linked: flag[label[i]] = 1 for every splat i with (s_i & mask) == value and a label (flag: n words, zeroed), then
// the state pass over the label plane with the membership flag[label] != 0
void gs_launch_cluster_seeds(const uint8_t* state, const uint32_t* labels, uint32_t n, uint32_t mask, uint32_t value, uint32_t* flag, hipStream_t st);
void gs_launch_state_cluster_linked(uint8_t* state, const uint32_t* labels, uint32_t n, const uint32_t* flag, uint32_t op, uint32_t bits, uint32_t where_mask,
                                    uint32_t where_value, unsigned long long* matched, hipStream_t st);
// k_thin.hip: thinning (gs_thin.hip) over the neighbourhoods' grid, records and slices.  rank (u64) and status (u32) are indexed by SORTED
// POSITION, beside the record; the work planes keeper / covers by splat index.
// keeper / covers of every splat: {i, 1} for a member with a non-finite coordinate (it has no record), else {GS_THIN_NONE, 0}
void gs_launch_thin_init(const uint8_t* state, const GsScene& s, uint32_t n, uint32_t mask, uint32_t value, uint32_t* keeper, uint32_t* covers,
                         hipStream_t st);
// rank[t] of the member at sorted position t (prio: the priority values f32[n] by splat index, or null), status[t] = 0 (undecided)
void gs_launch_thin_rank(const void* rec, uint32_t nrec, uint32_t n, const float* prio, uint32_t flags, uint32_t seed, unsigned long long* rank,
                         uint32_t* status, hipStream_t st);
// one round over workgroups [first_block, first_block + blocks) of 256 sorted members (v.src's records are queries and sources alike:
// v.qrec is not read); round: 1, 2, ... (the stamp of its decisions); *undecided += the members it leaves undecided
void gs_launch_thin_round(const NeighView& v, uint32_t first_block, uint32_t blocks, float r2, uint32_t round, const unsigned long long* rank, uint32_t* status,
                          uint32_t* undecided, hipStream_t st);
// after the last round: keeper[id] of every sorted member, covers[keeper] += 1
void gs_launch_thin_assign(const NeighView& v, uint32_t first_block, uint32_t blocks, float r2, uint32_t n, const unsigned long long* rank,
                           const uint32_t* status, uint32_t* keeper, uint32_t* covers, hipStream_t st);
// the two planes from the work planes; slots: the GS_STATE_SLOTS partial records (zeroed by the caller), word 0 += kept, word 1 =
// max(word 1, largest covers)
void gs_launch_thin_commit(const uint32_t* wkeeper, const uint32_t* wcovers, uint32_t n, uint32_t* keeper, uint32_t* covers, unsigned long long* slots,
                           hipStream_t st);
// k_knn.hip: nearest neighbours (gs_knn.hip) over the neighbourhoods' grid, records and slices.
// a whole search's start: dist2[i] = +inf for a splat that passes (mask, value) (state null: every splat), NaN 0x7FC00000 for the
// others; nearest[i] = GS_KNN_NONE
void gs_launch_knn_init(const uint8_t* state, uint32_t n, uint32_t mask, uint32_t value, uint32_t* dist2, uint32_t* nearest, hipStream_t st);
// the query pass over workgroups [first_block, first_block + blocks) of 256 sorted queries: dist2[id] = the k-th smallest accepted d2
// or +inf, nearest[id] = the smallest id at the smallest accepted d2 or GS_KNN_NONE; *unresolved += the queries that end +inf.
// k: 1 .. GS_KNN_MAX_K (k KB of dynamic LDS)
void gs_launch_knn_query(const NeighView& v, uint32_t first_block, uint32_t blocks, float r2, uint32_t k, uint32_t n, uint32_t* dist2, uint32_t* nearest,
                         uint32_t* unresolved, hipStream_t st);
// gs_state_knn: the state pass with the float-range membership (v >= lo && v <= hi) == inside over the dist2 plane read as words
void gs_launch_state_knn(uint8_t* state, const uint32_t* dist2, uint32_t n, float lo, float hi, uint32_t inside, uint32_t op, uint32_t bits,
                         uint32_t where_mask, uint32_t where_value, unsigned long long* matched, hipStream_t st);
// k_surface.hip: surface (gs_surface.hip) over the neighbourhoods' grid, records and slices.  The two planes are 16-byte records per
// splat: nrm = {nx, ny, nz, count as a word}, eig = {l0, l1, l2, 0}.
// a whole estimate's start: NaN 0x7FC00000 in the six floats, count 0
void gs_launch_surface_init(uint32_t n, void* nrm, void* eig, hipStream_t st);
// the query pass over workgroups [first_block, first_block + blocks) of 256 sorted queries: the ten words count, S[3], M[6] of sorted
// query t, word k at out[id * 10 + k] (by_id: the kept plane) or at out[k * word_stride + t - 256 first_block] (the slice's scratch,
// word_stride >= 256 blocks); scale: 2^(16 - E); *unresolved += the queries that end with count < 3
void gs_launch_surface_query(const NeighView& v, uint32_t first_block, uint32_t blocks, float r2, float scale, uint32_t n, int64_t* out, bool by_id,
                             uint64_t word_stride, uint32_t* unresolved, hipStream_t st);
// sorted queries first .. first + count: their ten words, addressed as the query pass wrote them (first = 256 first_block), -> the
// two records of their splats; unscale: 2^(2 (E - 16)); orient: towards toward[3]
void gs_launch_surface_finish(const void* qrec, uint32_t first, uint32_t count, uint32_t n, const int64_t* in, bool by_id, uint64_t word_stride,
                              double unscale, bool orient, const float toward[3], void* nrm, void* eig, hipStream_t st);
// xyz[3 i ..] = the first three floats of record i, w[i] = its fourth word (each may be null)
void gs_launch_surface_unpack(const void* rec, uint32_t n, float* xyz, uint32_t* w, hipStream_t st);
// gs_state_surface: the state pass with the float-range membership over a feature of ONE plane's record (the eig plane for kinds below
// GS_SURFACE_FACING, the nrm plane for the others)
void gs_launch_state_surface(uint8_t* state, const void* plane, uint32_t n, uint32_t kind, float lo, float hi, uint32_t inside, const float axis[3], uint32_t op,
                             uint32_t bits, uint32_t where_mask, uint32_t where_value, unsigned long long* matched, hipStream_t st);
// k_export.hip: the splat edits (gs_export.hip).  Selection = splats with (s & mask) == value in ascending order: `counts` holds
// gs_select_blocks(n) + 1 words (one per 1024 splats; after the launch their exclusive prefix, the total last), `ids` the total.
uint32_t gs_select_blocks(uint32_t n);
void gs_launch_select_count(const uint8_t* state, uint32_t n, uint32_t mask, uint32_t value, uint32_t* counts, hipStream_t st); // count + scan
void gs_launch_select_scatter(const uint8_t* state, uint32_t n, uint32_t mask, uint32_t value, const uint32_t* offsets, uint32_t* ids, uint32_t cap,
                              hipStream_t st);
// records [first, first + m) of the selection (ids null: of the scene) as 320-byte records; out_ids (may be null): their indices
void gs_launch_unpack(const GsScene& s, uint32_t n, const uint32_t* ids, uint32_t first, uint32_t m, void* d_aos, uint32_t* out_ids, hipStream_t st);
// new splat first + g of `d` = splat ids[g] of `o` (every plane; with_state, which needs first == 0: the state byte too when both keep one)
void gs_launch_compact_planes(const GsScene& o, uint32_t n_old, const uint32_t* ids, uint32_t m, const GsScene& d, hipStream_t st, uint32_t first = 0,
                              bool with_state = true);
// k_insert.hip: the splat insertion's grow pass (gs_insert.hip): splats 0 .. n_old of `o` to the same indices of `d`, a scene laid
// out for n_new >= n_old splats (every plane moves: the plane stride depends on N), and the WHOLE state plane of `d`, when it keeps
// one: the old bytes, then new_state for splats n_old .. n_new, then 0 up to the plane stride
void gs_launch_grow(const GsScene& o, uint32_t n_old, const GsScene& d, uint32_t n_new, uint32_t new_state, uint32_t grid, hipStream_t st);
// k_snapshot.hip: snapshots and write-back (gs_snapshot.hip).  A snapshot's device memory as the kernels take it: entry g (0 .. m) is
// splat ids[g], or splat g when ids is null (a dense snapshot); x, y, z: f32[m] each; geo: float4[m][2]; sh: float4[m][12]; state:
// u8[m] in whole words.  A part that was not taken has null pointers and is never asked for.
struct GsSnapshotDev {
    const uint32_t* ids;
    float *x, *y, *z;
    float4 *geo, *sh;
    uint32_t* state;
};
// mode 0: take (scene -> snapshot), 1: restore (snapshot -> scene), 2: swap; parts: GS_PART_*, only their columns are launched
void gs_launch_snapshot(uint32_t mode, const GsScene& sc, uint32_t n, const GsSnapshotDev& s, uint32_t m, uint32_t parts, hipStream_t st);
// record g (0 .. m) of d_aos -> the parts named of splat ids[g], or of splat g when ids is null; d_states: one byte per record, read
// with GS_PART_STATE only.  The caller has checked the ids (gs_launch_ids_ascending, or on the host).
void gs_launch_write(const void* d_aos, const uint8_t* d_states, uint32_t m, const uint32_t* ids, const GsScene& s, uint32_t n, uint32_t parts,
                     hipStream_t st);
// *first_bad (set to all ones by the caller) = the first position g with ids[g] >= n or ids[g] <= ids[g - 1], if there is one
void gs_launch_ids_ascending(const uint32_t* ids, uint64_t m, uint32_t n, unsigned long long* first_bad, hipStream_t st);
// k_xform.hip: gs_transform_splats.  Entry g (0 .. m) is splat ids[g], or splat g when ids is null (then m = n); the parts named in
// x.flags are transformed in place.
struct gs_xform;
void gs_launch_xform(const GsScene& s, uint32_t n, const uint32_t* ids, uint32_t m, const gs_xform& x, hipStream_t st);
// k_grade.hip: gs_grade_splats.  Entries as for gs_launch_xform; the parts named in x.flags (SH coefficients, band 0, the opacity
// logit) are graded in place.
struct gs_grade;
void gs_launch_grade(const GsScene& s, uint32_t n, const uint32_t* ids, uint32_t m, const gs_grade& x, hipStream_t st);
// k_pack.hip: the packed scenes (gs_pack.hip).  Entry g (0 .. m) is splat ids[g], or splat g when ids is null.
struct GsPackBox { float lo[3], hi[3]; }; // the bounds of the selection's splats with three finite coordinates
// keys[g] = the Morton key of entry g under `box` (GS_PACK_KEY_LAST with a non-finite coordinate), vals[g] = its splat
void gs_launch_pack_keys(const GsScene& s, uint32_t n, const uint32_t* ids, uint32_t m, const GsPackBox& box, uint32_t* keys, uint32_t* vals,
                         hipStream_t st);
// The three sections of the m entries: C = ceil(m / 256) chunk records (18 floats), m vertices (16 B), and with K > 0 the SH bytes,
// 256 x 3K per chunk (the buffer holds whole chunks; the bytes behind entry m are 0 or untouched).  bad: 5 C words, the replaced
// floats per chunk (C words of the vertices, then 4 C of the SH bytes): the caller adds them up.
void gs_launch_pack_encode(const GsScene& s, uint32_t n, const uint32_t* ids, uint32_t m, uint32_t K, float* chunks, void* vertices, void* sh_bytes,
                           uint32_t* bad, hipStream_t st);
// One trip of a packed file on the device: m vertices that start at a chunk boundary (16-byte aligned), their chunk records, their
// 3K SH bytes each (null with K = 0) and the 256 logits.  Vertex v becomes splat first + v of `dst`.
struct GsPackTrip {
    const uint4* vertices;
    const float* chunks;
    const uint8_t* sh;
    const float* table;
    uint32_t m, K;
};
void gs_launch_pack_decode(const GsPackTrip& t, uint32_t first, const GsScene& dst, hipStream_t st);
// k_pick.hip: gs_pick, one wave per query over the last frame's lists (queries: {x, y} pairs; results: 12 words per query;
// contrib: max_contrib {id, weight} pairs per query, or null)
void gs_launch_pick(const GsLists& L, const void* d_queries, uint32_t n, void* d_results, uint32_t max_contrib, void* d_contrib, hipStream_t st);
// k_coverage.hip: gs_coverage_accumulate, one wave per 8x8 pixel block [bx0, bx0 + nbx) x [by0, by0 + nby) (in blocks) over the last
// frame's lists, adding into `planes` (16 bytes per splat: gs_coverage_rec)
struct GsCoverDev { // a gs_cover_region as the kernel reads it
    uint32_t x0, y0, x1, y1; // canvas pixels [x0, x1) x [y0, y1)
    const uint8_t* mask;     // device u8[height][width] of the canvas, or null
};
void gs_launch_coverage(const GsLists& L, uint32_t bx0, uint32_t by0, uint32_t nbx, uint32_t nby, const GsCoverDev& r, void* planes, hipStream_t st);
// k_merge.hip: the cell merge (gs_merge.hip; every expression is gs_merge_math.h's).  keys: (cell key, id) per splat, `none` for a splat
// that is not eligible.  heads: flag[t] = 1 where a run of equal sorted keys begins (a byte plane for gs_launch_select_*).  runs: run r
// spans heads[r] .. heads[r + 1] (n behind the last); flag[r] = 1 when it is merged (key < none, at least min_members long); stats
// (three words, zeroed by the caller): eligible, largest run, members of merged runs.  sums: groups first .. first + count, group g =
// merged run mruns[g], one wave each, into sums[(g - first) * 64]; group_of (u32[n]) and member (u8[n]) may be null.  finish: count
// groups' sums -> 320-byte records.
void gs_launch_merge_keys(const uint8_t* state, const GsScene& s, uint32_t n, uint32_t mask, uint32_t value, const GsNeighGrid& g, uint32_t* keys,
                          uint32_t* vals, hipStream_t st);
void gs_launch_merge_heads(const uint32_t* keys, uint32_t n, uint8_t* flag, hipStream_t st);
void gs_launch_merge_runs(const uint32_t* keys, const uint32_t* heads, uint32_t runs, uint32_t n, uint32_t none, uint32_t min_members, uint8_t* flag,
                          uint32_t* stats, hipStream_t st);
void gs_launch_merge_sums(const uint32_t* vals, const uint32_t* heads, uint32_t runs, const uint32_t* mruns, uint32_t first, uint32_t count,
                          uint32_t nsorted, const GsScene& s, uint32_t n, double* sums, uint32_t* group_of, uint8_t* member, hipStream_t st);
void gs_launch_merge_finish(const double* sums, uint32_t count, void* d_aos, hipStream_t st);
