// k_snapshot.hip -- the kernels behind snapshots and write-back (gs_snapshot.hip, gs_abi.h "snapshots and write-back"): the inverse
// of the export.  The reference has no counterpart: its host keeps the 320-byte records it uploaded (renderer.ts:130-137) and would
// edit and upload those again.
//
// Nothing is computed but the derived largest log-scale: every float is moved as a word, so a NaN's payload goes through untouched.
//   snapshot : ONE kernel family over (entry, 16-byte column) in gs_compact_planes_kernel's indexing -- column 0 the three
//              position floats, 1-2 the geometry float4s, 3-14 the SH float4s, 15 the state byte -- with a mode: take (scene ->
//              snapshot), restore (snapshot -> scene) or swap (both ways in one pass).  Only the columns of the parts asked for are
//              launched (parts -> a dense local column index), so threads and bytes are proportional to the parts, not to 16
//              columns.  Entry g is splat ids[g], or splat g when the snapshot is dense.  The snapshot side is compact SoA and
//              fully coalesced (consecutive threads, consecutive float4s); the scene side is a gather / scatter of whole 16-byte
//              units (12 bytes of three 4-byte planes for the positions).  Traffic per entry and direction, take or restore:
//              POSITION 12 B read + 12 B written, GEOMETRY 32 + 32 (+ 4 B of smax written by a restore), SH 192 + 192, STATE 1 + 1,
//              plus 4 B of id per launched column when not dense (served by the cache: the threads of an entry are neighbours).
//              A swap reads and writes both sides: twice that.  Bound: HBM.
//              The state byte: the column-15 thread of every FOURTH entry owns one whole word of the snapshot's u8[m] (its own
//              byte and its three neighbours', 0 past m: gs_compact_planes_kernel's rule), and reaches the scene's bytes through
//              the word atomics of gs_state_ids_kernel's ASSIGN (an AND that clears, then an OR that sets).  The ids of one
//              snapshot are distinct, so no two entries touch one byte; a swap reads its bytes before it assigns them, and nobody
//              else writes them.
//   write    : gs_repack_kernel with a destination list: one thread per (given record, 16-byte source column), 20 columns; record
//              g goes to splat ids[g], or g.  Columns of parts not named return before they load: POSITION column 0, GEOMETRY
//              columns 1-3 (3: the opacity logit; 1 also stores smax), SH columns 4-19.  320 B of record read (less for fewer
//              parts: 16 / 48 / 256 B), 244 B scattered per record.  Bound: HBM.  The state bytes take a pass of their own, one
//              thread per entry, the same two word atomics.
//   ascending: one thread per id; an id that is no splat or does not exceed its predecessor takes an atomicMin of its position into
//              one 64-bit word.  4 B read per id (the predecessor's from the cache).
// Every index formed from an id is guarded by id < n.  No MFMA anywhere (no contraction).  Every float4 is a plain vector load or store.
#include "gs_device.h"
#include "gs_kernels.h"

// local column j of the launch -> column 0..15 of gs_compact_planes_kernel's indexing, given the parts that are launched
__device__ __forceinline__ uint32_t snap_column(uint32_t j, uint32_t parts) {
    uint32_t c = j;
    if (!(parts & 0x1u)) c += 1u;
    if (!(parts & 0x2u) && c >= 1u) c += 2u;
    if (!(parts & 0x4u) && c >= 3u) c += 12u;
    return c;
}
static uint32_t snap_columns(uint32_t parts) { return (parts & 0x1u ? 1u : 0u) + (parts & 0x2u ? 2u : 0u) + (parts & 0x4u ? 12u : 0u) + (parts & 0x8u ? 1u : 0u); }

// the byte of splat id := b, through the word that holds it (gs_state_ids_kernel's ASSIGN)
__device__ __forceinline__ void state_assign(uint32_t* words, uint32_t id, uint32_t b) {
    const uint32_t sh = (id & 3u) * 8u;
    uint32_t* w = words + (id >> 2);
    atomicAnd(w, ~((0xFFu & ~b) << sh));
    atomicOr(w, b << sh);
}

// MODE 0: take, 1: restore, 2: swap
template <int MODE>
__global__ __launch_bounds__(256) void gs_snapshot_kernel(float* px, float* py, float* pz, float* smax, float4* geo, float4* sh, uint8_t* state, uint32_t n,
                                                           GsSnapshotDev s, uint32_t m, uint32_t parts, uint32_t ncols) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)m * ncols) return;
    const uint32_t g = (uint32_t)(t / ncols), c = snap_column((uint32_t)(t % ncols), parts);
    if (c == 15u) {
        if (g & 3u) return;
        uint32_t* words = reinterpret_cast<uint32_t*>(state);
        uint32_t from_scene = 0u;
        const uint32_t from_snap = MODE != 0 ? s.state[g >> 2] : 0u;
        for (uint32_t k = 0; k < 4u && g + k < m; ++k) {
            const uint32_t id = s.ids ? s.ids[g + k] : g + k;
            if (id >= n) continue; // (never: the ids come from the selection over this scene, which has not shrunk since)
            if (MODE != 1) from_scene |= (uint32_t)state[id] << (8u * k);
            if (MODE != 0) state_assign(words, id, (from_snap >> (8u * k)) & 0xFFu);
        }
        if (MODE != 1) s.state[g >> 2] = from_scene;
        return;
    }
    const uint32_t id = s.ids ? s.ids[g] : g;
    if (id >= n) return; // (never, as above)
    if (c == 0u) {
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (MODE != 1) { x = px[id]; y = py[id]; z = pz[id]; }
        if (MODE != 0) { const float a = s.x[g], b = s.y[g], d = s.z[g]; px[id] = a; py[id] = b; pz[id] = d; }
        if (MODE != 1) { s.x[g] = x; s.y[g] = y; s.z[g] = z; }
        return;
    }
    float4* scene_at = c < 3u ? geo + ((uint64_t)id * 2 + (c - 1u)) : sh + ((uint64_t)id * 12 + (c - 3u));
    float4* snap_at = c < 3u ? s.geo + ((uint64_t)g * 2 + (c - 1u)) : s.sh + ((uint64_t)g * 12 + (c - 3u));
    if (MODE == 0) { *snap_at = *scene_at; return; }
    const float4 v = *snap_at;
    if (MODE == 2) *snap_at = *scene_at;
    *scene_at = v;
    if (c == 1u) smax[id] = __builtin_fmaxf(v.x, __builtin_fmaxf(v.y, v.z));
}

void gs_launch_snapshot(uint32_t mode, const GsScene& sc, uint32_t n, const GsSnapshotDev& s, uint32_t m, uint32_t parts, hipStream_t st) {
    const uint32_t ncols = snap_columns(parts);
    const uint64_t total = (uint64_t)m * ncols;
    if (!total) return;
    const dim3 grid((uint32_t)((total + 255) / 256));
#define GS_SNAPSHOT_LAUNCH(M)                                                                                                              \
    hipLaunchKernelGGL(gs_snapshot_kernel<M>, grid, dim3(256), 0, st, (float*)sc.px, (float*)sc.py, (float*)sc.pz, (float*)sc.smax, (float4*)sc.geo, \
                       (float4*)sc.sh, const_cast<uint8_t*>(sc.state), n, s, m, parts, ncols)
    if (mode == 0u) GS_SNAPSHOT_LAUNCH(0);
    else if (mode == 1u) GS_SNAPSHOT_LAUNCH(1);
    else GS_SNAPSHOT_LAUNCH(2);
#undef GS_SNAPSHOT_LAUNCH
}

// ---- 320-byte AoS -> the planes of the splats named: gs_repack_kernel (k_preprocess.hip) with a destination list ----------------
__global__ __launch_bounds__(256) void gs_write_records_kernel(const float4* __restrict__ aos, uint32_t m, const uint32_t* __restrict__ ids, uint32_t n,
                                                                uint32_t parts, float* px, float* py, float* pz, float* smax, float* geo, float* sh) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)m * 20) return; // 20 float4 per source record
    const uint32_t g = (uint32_t)(t / 20), c = (uint32_t)(t % 20);
    const uint32_t part = c == 0u ? 0x1u : c < 4u ? 0x2u : 0x4u;
    if (!(parts & part)) return;
    const uint32_t d = ids ? ids[g] : g;
    if (d >= n) return; // (never: the caller has checked the ids)
    const float4 v = aos[t];
    float* r = geo + (uint64_t)d * 8;
    if (c == 0) { px[d] = v.x; py[d] = v.y; pz[d] = v.z; }
    else if (c == 1) { r[0] = v.x; r[1] = v.y; r[2] = v.z; smax[d] = __builtin_fmaxf(v.x, __builtin_fmaxf(v.y, v.z)); }
    else if (c == 2) { r[4] = v.x; r[5] = v.y; r[6] = v.z; r[7] = v.w; }
    else if (c == 3) { r[3] = v.x; }
    else {
        float* q = sh + (uint64_t)d * 48 + 3 * (c - 4);
        q[0] = v.x;
        q[1] = v.y;
        q[2] = v.z;
    }
}
__global__ __launch_bounds__(256) void gs_write_states_kernel(const uint8_t* __restrict__ bytes, uint32_t m, const uint32_t* __restrict__ ids, uint32_t n,
                                                               uint32_t* words) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= m) return;
    const uint32_t d = ids ? ids[g] : g;
    if (d < n) state_assign(words, d, bytes[g]);
}
void gs_launch_write(const void* d_aos, const uint8_t* d_states, uint32_t m, const uint32_t* ids, const GsScene& s, uint32_t n, uint32_t parts,
                     hipStream_t st) {
    if (!m) return;
    const uint64_t total = (uint64_t)m * 20;
    if (parts & 0x7u)
        hipLaunchKernelGGL(gs_write_records_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, (const float4*)d_aos, m, ids, n, parts,
                           (float*)s.px, (float*)s.py, (float*)s.pz, (float*)s.smax, (float*)s.geo, (float*)s.sh);
    if ((parts & 0x8u) && s.state)
        hipLaunchKernelGGL(gs_write_states_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, d_states, m, ids, n,
                           reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(s.state)));
}

// ---- ids strictly ascending and below n: *first_bad = min(*first_bad, the first position that is not) -----------------------------
__global__ __launch_bounds__(256) void gs_ids_ascending_kernel(const uint32_t* __restrict__ ids, uint64_t m, uint32_t n, unsigned long long* first_bad) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= m) return;
    const uint32_t id = ids[g];
    if (id >= n || (g > 0 && ids[g - 1] >= id)) atomicMin(first_bad, (unsigned long long)g);
}
void gs_launch_ids_ascending(const uint32_t* ids, uint64_t m, uint32_t n, unsigned long long* first_bad, hipStream_t st) {
    if (!m) return;
    hipLaunchKernelGGL(gs_ids_ascending_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, ids, m, n, first_bad);
}
