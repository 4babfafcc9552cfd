// k_gsort.hip -- the gaussian-level stage of the depth-ordered pipeline: the frame's visible gaussians, sorted by the depth
// bucket of their sort key, with a per-gaussian quantity (tile count, or row-item slots) scanned in that order.
//
// The reference sorts every (tile, gaussian) INSTANCE by tile*1000 + bucket (write_tile_ids.wgsl:31, radix_sort.wgsl).  The
// order it needs inside a tile is (bucket, gaussian index); sorting the N_vis visible GAUSSIANS by bucket first (stable, so
// index order survives inside a bucket: 7-16x fewer elements than instances) and binning their instances in that order
// leaves only the tile id for the stable instance binning.
//
// Round 2 fed this stage from a chained look-back scan that compacted the visible gaussians (31 us for 24 MB, bound by the
// chain) and counted buckets over tiles of the COMPACTED list (4 launches, 85 us).  Here the unit of work is a chunk of 2048
// consecutive gaussian INDICES, so nothing has to be compacted or scanned beforehand and no workgroup waits for another.  The
// NT chunks are cut into G contiguous RUNS of ceil(NT / G) chunks (G = the context's persistent grid, about one workgroup
// per residency slot of the scatter); one workgroup owns a run in hist and in scatter, and the (bucket, run) table M has one
// column per RUN: a (chunk, bucket) cell holds 0.8 gaussians on average at 6.1 M, so a per-chunk table was bigger than the
// data it indexed.  When NT <= G a run is one chunk.
//   hist     every run counts the buckets of its visible gaussians, chunk after chunk into ONE LDS histogram
//                                                                          -> M[bucket][run] = (gaussians, quantity)
//   rowscan  every bucket's row of M is scanned over the runs (exclusive)  -> row totals
//   scatter  every run builds its bucket bases once (scan of the row totals + its column of M), then walks its chunks in
//            ascending order: rank the chunk's visible gaussians by bucket where they are (wave ballots; a wave's items are
//            in index order, so the rank is stable), reorder them through LDS, scan their quantity in that order and write
//            one record {id, word, prefix, aux} per gaussian at  base[bucket] + rank;  then base[bucket] advances by the
//            chunk's own (count, quantity) of the bucket.  Plus the chunk table (first gaussian of every 1024 units of the quantity) that the reference-binning
//            emission and the row sort of the tight pipeline (k_rows.hip) start from.
// Position in (bucket, index) order = bucket base + gaussians of the bucket in earlier runs (the table) + gaussians of the
// bucket in earlier chunks of this run (carried in the base) + stable rank inside the chunk: runs and chunks are ascending
// index ranges, so the order inside a bucket is the gaussian index order, which is what write_tile_ids.wgsl:31 plus a stable
// sort gives.  The table is written by one kernel and read by the next: launch boundaries are the only ordering needed.
//
// Two input forms (template parameter DENSE of hist and scatter).  The reference's binning hands over one count word per gaussian
// INDEX.  The tight projection hands over ENTRIES: per unit of 1024 indices the cull's survivors in index order, dense from the
// unit's start, and their number (see gs_gsort_hist_kernel) -- at 40 % visible the N-indexed form read 12 N bytes to sort 0.4 N
// records and spent three fifths of its ranking lanes on zero words.
//
// Saturation.  Quantities are summed in 64 bits and stored as sat32(sum).  For non-negative terms
// sat32(sat32(a) + b) == sat32(a + b), so the carried base stays 32 bits wide in LDS (a 64-bit base would cost 4 KB and the
// fourth workgroup of a CU) and still equals sat32(true 64-bit base) at every chunk: `off`, the chunk table and the totals
// saturate exactly where a per-chunk table made them saturate.  The one step that needs care is the chunk's own quantity of a
// bucket, read from the saturated in-chunk prefix P: if P at the bucket's END is saturated the new base is saturated as well,
// because the base of a bucket already counts every earlier bucket of this chunk (base >= P at the bucket's START), so
// base + (end - start) >= P(end) >= 2^32 - 1; otherwise both P values are exact.
#include "gs_binning.h"

#define GC_ITEMS 8
#define GC_THREADS 256
#define GC (GC_THREADS * GC_ITEMS) // gaussian indices per chunk
#define GBINS 1024                 // bucket = u32(min(50 depth, 999)) < 1000 (write_tile_ids.wgsl:31)
#ifndef GS_GSORT_RUNS_Q
#define GS_GSORT_RUNS_Q 4          // runs = persistent grid * Q / 4 (swept 2 / 3 / 4 / 8: profiles/README.md)
#endif
// The (bucket, run) table is stored [bucket / 8][run][bucket % 8]: the 1024 entries a run's workgroup writes (hist) or
// reads (scatter) are 128 whole 64-byte sectors instead of 1024 partial ones, and a bucket's row is still a strided stream.
__device__ __forceinline__ uint64_t m_index(uint32_t b, uint32_t col, uint32_t ncol) { return ((uint64_t)(b >> 3) * ncol + col) * 8u + (b & 7u); }

// One workgroup per run: chunks [run * cpr, min((run + 1) * cpr, NT)); the loads of chunk k + 1 are issued before the LDS
// atomics of chunk k.
//
// DENSE (the tight pipeline): `words` is not indexed by the gaussian.  The projection compacts the cull's survivors of every
// UNIT of GU = 1024 consecutive indices in index order (k_preprocess.hip): unit_n[u] of them, survivor e of unit u at entry
// u * GU + e of three planes -- the count word (0: ends without a tile), the aux word, and the gaussian's offset inside the
// unit (u16).  A chunk is two units, T = n0 + n1 entries; position p < T of the chunk is entry p of unit 2c when p < n0, else
// entry p - n0 of unit 2c + 1: positions ascend with the gaussian index.  The sort neither loads nor ranks the culled 60 %.
// unit_n holds 2 NT + 2 words, those past the last unit zero: a chunk's pair is one aligned 8-byte load.
#define GU (GC / 2)
// (clamped: the planes hold whole chunks, so no value of a count can take a load out of them)
__device__ __forceinline__ uint2 unit_pair(const uint2* __restrict__ unit_n, uint32_t c) {
    const uint2 v = unit_n[c];
    return make_uint2(v.x < GU ? v.x : GU, v.y < GU ? v.y : GU);
}
template <bool DENSE>
__global__ __launch_bounds__(GC_THREADS) void gs_gsort_hist_kernel(const uint32_t* __restrict__ words, const uint2* __restrict__ unit_n, uint32_t n,
                                                                   uint2* __restrict__ M, uint32_t ncol, uint32_t cpr, uint32_t NT) {
    __shared__ uint32_t s_cnt[GBINS];
    __shared__ unsigned long long s_sum[GBINS]; // a run's quantity can exceed 32 bits (2048 x 2^22 tiles a chunk): saturated on store
    const uint32_t run = blockIdx.x, tid = threadIdx.x;
    const uint32_t c0 = run * cpr, c1 = c0 + cpr < NT ? c0 + cpr : NT;
    for (uint32_t b = tid; b < GBINS; b += GC_THREADS) { s_cnt[b] = 0u; s_sum[b] = 0ull; }
    uint32_t wv[GC_ITEMS];
    // DENSE: item j of thread t is entry (j % 4) * 256 + t of unit 2c + j / 4 (the order inside a chunk is free here)
    uint2 un = make_uint2(0u, 0u); // the units' survivors of the chunk being loaded
    auto load = [&](uint32_t c, uint32_t (&o)[GC_ITEMS]) {
#pragma unroll
        for (int j = 0; j < GC_ITEMS; ++j) {
            if (DENSE) {
                const uint32_t e = (uint32_t)(j & 3) * GC_THREADS + tid;
                o[j] = (e < (j < 4 ? un.x : un.y)) ? words[c * GC + (uint32_t)(j >> 2) * GU + e] : 0u;
            } else {
                const uint32_t k = c * GC + j * GC_THREADS + tid;
                o[j] = (k < n) ? words[k] : 0u;
            }
        }
    };
    if (DENSE) un = unit_pair(unit_n, c0);
    load(c0, wv);
    if (DENSE) un = c0 + 1u < c1 ? unit_pair(unit_n, c0 + 1u) : make_uint2(0u, 0u);
    __syncthreads();
    for (uint32_t c = c0; c < c1; ++c) {
        uint32_t nx[GC_ITEMS];
        if (c + 1u < c1) load(c + 1u, nx); // (uniform)
        else {
#pragma unroll
            for (int j = 0; j < GC_ITEMS; ++j) nx[j] = 0u;
        }
        if (DENSE) un = c + 2u < c1 ? unit_pair(unit_n, c + 2u) : make_uint2(0u, 0u); // (consumed by the next trip's loads)
#pragma unroll
        for (int j = 0; j < GC_ITEMS; ++j) {
            const uint32_t w = wv[j];
            if (w & GS_COUNT_MASK) {
                const uint32_t b = w >> GS_COUNT_BITS;
                atomicAdd(&s_cnt[b], 1u);
                atomicAdd(&s_sum[b], (unsigned long long)(w & GS_COUNT_MASK));
            }
        }
#pragma unroll
        for (int j = 0; j < GC_ITEMS; ++j) wv[j] = nx[j];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t i = 0; i < GBINS / GC_THREADS; ++i) { // thread t: buckets 4t .. 4t+3 (32 contiguous bytes)
        const uint32_t b = tid * (GBINS / GC_THREADS) + i;
        M[m_index(b, run, ncol)] = make_uint2(s_cnt[b], sat32(s_sum[b]));
    }
}

// One workgroup of 1024 threads per 8 buckets (one 64-byte sector per run): thread (cl = t / 8, sub = t % 8) owns the runs
// [cl * per, (cl + 1) * per) of bucket 8 * blockIdx + sub -- eight at 1024 runs, one batch of independent loads; the
// 128 partial sums of a bucket are scanned by lane shifts of 8 inside a wave and through LDS across the 16 waves.
#define GR_THREADS 1024
__device__ __forceinline__ void scan_stride8(uint32_t& x, unsigned long long& y, uint32_t lane) { // inclusive over lanes l, l-8, l-16, ...
#pragma unroll
    for (int d = 8; d < 64; d <<= 1) {
        const uint32_t ox = __shfl_up(x, d, 64), lo = __shfl_up((uint32_t)y, d, 64), hi = __shfl_up((uint32_t)(y >> 32), d, 64);
        if ((int)lane >= d) { x += ox; y += ((unsigned long long)hi << 32) | lo; }
    }
}
__global__ __launch_bounds__(GR_THREADS) void gs_gsort_rowscan_kernel(uint2* __restrict__ M, uint32_t ncol, uint2* __restrict__ rowtot) {
    __shared__ uint32_t s_x[GR_THREADS / 64][8];
    __shared__ unsigned long long s_y[GR_THREADS / 64][8];
    const uint32_t nt = ncol, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, cl = tid >> 3, sub = tid & 7u;
    const uint32_t per = (nt + GR_THREADS / 8 - 1u) / (GR_THREADS / 8);
    const uint32_t c0 = cl * per < nt ? cl * per : nt, c1 = (cl + 1u) * per < nt ? (cl + 1u) * per : nt;
    uint2* row = M + (uint64_t)blockIdx.x * ncol * 8u + sub;
    uint32_t ax = 0;
    unsigned long long ay = 0;
    for (uint32_t c = c0; c < c1; c += 8u) {
        uint2 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (c + k < c1) ? row[(uint64_t)(c + k) * 8u] : make_uint2(0u, 0u);
#pragma unroll
        for (int k = 0; k < 8; ++k) { ax += v[k].x; ay += v[k].y; }
    }
    uint32_t ix = ax;
    unsigned long long iy = ay;
    scan_stride8(ix, iy, lane);
    if (lane >= 56u) { s_x[w][sub] = ix; s_y[w][sub] = iy; } // the wave's total of each of its 8 sub-buckets
    __syncthreads();
    uint32_t rx = ix - ax, tx = 0;
    unsigned long long ry = iy - ay, ty = 0;
#pragma unroll
    for (uint32_t k = 0; k < GR_THREADS / 64; ++k) {
        const uint32_t vx = s_x[k][sub];
        const unsigned long long vy = s_y[k][sub];
        if (k < w) { rx += vx; ry += vy; }
        tx += vx; ty += vy;
    }
    for (uint32_t c = c0; c < c1; c += 8u) {
        uint2 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (c + k < c1) ? row[(uint64_t)(c + k) * 8u] : make_uint2(0u, 0u);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (c + k < c1) row[(uint64_t)(c + k) * 8u] = make_uint2(rx, sat32(ry));
            rx += v[k].x; ry += v[k].y;
        }
    }
    if (tid < 8u) rowtot[blockIdx.x * 8u + sub] = make_uint2(tx, sat32(ty));
}

struct alignas(16) GsortShared {
    uint2 base[GBINS];                 // next sorted position / next quantity offset (saturated) of the bucket in this run
    unsigned short binstart[GBINS];    // first slot of the bucket in the chunk's sorted order
    union {
        unsigned short whist[GC_THREADS / 64][GBINS]; // per-wave running counts while ranking ([wave][bucket]) ...
        uint32_t P[GC];                               // ... then the prefix of the sorted quantities
        uint4 zero[GC / 4];                           // (the counters again, for clearing them 16 bytes at a time)
    } u;
    unsigned short id[GC];             // index inside the chunk
    uint32_t word[GC], aux[GC];
    GsPair w2[GC_THREADS / 64];
    uint32_t w1[GC_THREADS / 64];
    uint32_t ptot;                     // P one past the last slot: the chunk's whole quantity (saturated)
};
static_assert(sizeof(unsigned short) * (GC_THREADS / 64) * GBINS == sizeof(uint32_t) * GC, "the ranking counters and the prefix share their storage");
static_assert(sizeof(GsortShared) <= 40 * 1024, "four workgroups per CU");

// Output: ONE 16-byte record per visible gaussian in (bucket, index) order -- {gaussian id, count word, exclusive prefix of the
// quantity, aux} -- because a (chunk, bucket) run is about two gaussians long: four separate arrays were four scattered 4-byte
// stores each (round 2), a record is one 16-byte store.  aux_in (optional, tight row pipeline): a second per-gaussian word
// (the arena address of its row-item slots).  chunk_table[c] = the gaussian whose quantity interval holds c * 1024 (the
// reference-binning emission and the row sort start there).  tot_*: visible gaussians, total quantity (saturated).
// One workgroup per run, 38 KB of LDS: four workgroups per CU.  The row totals, the run's table column and the first chunk
// are loaded before the first barrier; inside the loop the next chunk's words (+ aux) are loaded into registers before the
// current one is ranked, so only the first chunk's load latency is exposed.  Every barrier of a trip is reached by all 256
// threads: the trip count and `nc` are uniform over the workgroup.
// DENSE: wave w owns positions [w L, (w + 1) L) of the chunk's T entries, L = 64 ceil(T / 256): item j of lane l is position
// w L + 64 j + l, so (item, lane) is still the index order and waves still own ascending ranges; the rounds past T hold
// nothing and the uniform `if (vis)` skips them.  The index inside the chunk comes from the entry's offset plane.
template <bool DENSE>
__global__ __launch_bounds__(GC_THREADS) void gs_gsort_scatter_kernel(const uint32_t* __restrict__ words, const uint32_t* __restrict__ aux_in,
                                                                      const unsigned short* __restrict__ unit_off, const uint2* __restrict__ unit_n, uint32_t n,
                                                                      const uint2* __restrict__ M, uint32_t ncol, uint32_t cpr, uint32_t NT,
                                                                      const uint2* __restrict__ rowtot, uint4* __restrict__ grec,
                                                                      uint32_t* __restrict__ chunk_table, uint32_t chunk_cap,
                                                                      uint32_t* __restrict__ tot_visible, uint32_t* __restrict__ tot_quantity) {
    __shared__ GsortShared S;
    const uint32_t run_id = blockIdx.x;
    const uint32_t chunk0 = run_id * cpr, chunk1 = chunk0 + cpr < NT ? chunk0 + cpr : NT;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    constexpr uint32_t BPT = GBINS / GC_THREADS; // buckets per thread (4 consecutive)

    // ---- every global load of the prologue up front: the first chunk's count words (+ aux), the row totals, the run's column ----
    uint32_t nwv[GC_ITEMS], nav[GC_ITEMS]; // the NEXT trip's words: wave w reads indices w * 512 + j * 64 + lane of its chunk
    uint32_t nid[GC_ITEMS];                // DENSE: ... and their indices inside the chunk
    uint2 un = make_uint2(0u, 0u);         // DENSE: the units' survivors of the chunk that load_chunk loads next ...
    uint2 unx = make_uint2(0u, 0u);        // ... and of the chunk whose entries nwv / nav / nid hold
#pragma unroll
    for (int j = 0; j < GC_ITEMS; ++j) nwv[j] = nav[j] = nid[j] = 0u;
    const uint32_t whole = n / GC;         // chunks below this one need no bounds checks
    auto load_chunk = [&](uint32_t c) {
        if (DENSE) {
            // Round j < R (uniform) loads its three values WHATEVER the lane holds -- a position past T reads entry 0 of the chunk
            // -- and nothing here depends on a loaded value: the validity test, the unit's half and the id wait for the trip that
            // consumes them (a load under a lane's condition, or arithmetic on its result, is waited for right behind its issue,
            // eight load latencies a trip instead of one).  Rounds past R keep what an earlier trip left: masked as well.
            const uint32_t T = un.x + un.y;
            const uint32_t R = (T + 255u) >> 8; // rounds that hold an entry: a wave's range is 64 R positions
            const uint32_t p0 = w * (R << 6) + lane;
#pragma unroll
            for (int j = 0; j < GC_ITEMS; ++j) {
                if ((uint32_t)j < R) {
                    const uint32_t p = p0 + j * 64 < T ? p0 + j * 64 : 0u;
                    const uint32_t e = c * GC + (p >= un.x ? GU + (p - un.x) : p);
                    nwv[j] = words[e];
                    nav[j] = aux_in[e];
                    nid[j] = (uint32_t)unit_off[e];
                }
            }
            unx = un;
            return;
        }
        const uint32_t k0 = c * GC + w * (64 * GC_ITEMS) + lane;
        if (c < whole) { // (uniform)
#pragma unroll
            for (int j = 0; j < GC_ITEMS; ++j) nwv[j] = words[k0 + j * 64];
#pragma unroll
            for (int j = 0; j < GC_ITEMS; ++j) nav[j] = aux_in ? aux_in[k0 + j * 64] : 0u;
        } else {
#pragma unroll
            for (int j = 0; j < GC_ITEMS; ++j) {
                const uint32_t k = k0 + j * 64;
                nwv[j] = (k < n) ? words[k] : 0u;
                nav[j] = (aux_in && k < n) ? aux_in[k] : 0u;
            }
        }
    };
    if (DENSE) un = unit_pair(unit_n, chunk0);
    load_chunk(chunk0);
    if (DENSE) un = chunk0 + 1u < chunk1 ? unit_pair(unit_n, chunk0 + 1u) : make_uint2(0u, 0u);
    {
        uint2 t[BPT], mm[BPT];
#pragma unroll
        for (uint32_t i = 0; i < BPT; ++i) { t[i] = rowtot[tid * BPT + i]; mm[i] = M[m_index(tid * BPT + i, run_id, ncol)]; }

        // ---- bucket bases: exclusive scan of the row totals, plus this run's entry of the scanned table ----
        GsPair acc; acc.x = 0u; acc.y = 0ull;
#pragma unroll
        for (uint32_t i = 0; i < BPT; ++i) { acc.x += t[i].x; acc.y += t[i].y; }
        GsPair total;
        GsPair run = block_excl2<GC_THREADS / 64>(acc, tid, S.w2, total);
#pragma unroll
        for (uint32_t i = 0; i < BPT; ++i) {
            S.base[tid * BPT + i] = make_uint2(run.x + mm[i].x, sat32(run.y + mm[i].y));
            run.x += t[i].x; run.y += t[i].y;
        }
        if (run_id == 0 && tid == 0) { *tot_visible = total.x; *tot_quantity = sat32(total.y); }
    }

    for (uint32_t chunk = chunk0; chunk < chunk1; ++chunk) {
        // (the barrier that ends a trip, or block_excl2's above, separates the last reads of P / word / id / aux from here)
        uint32_t wv[GC_ITEMS], av[GC_ITEMS];
#pragma unroll
        for (int j = 0; j < GC_ITEMS; ++j) { wv[j] = nwv[j]; av[j] = nav[j]; }
        uint32_t idv[GC_ITEMS];
#pragma unroll
        for (int j = 0; j < GC_ITEMS; ++j) idv[j] = 0u;
        if (DENSE) { // what load_chunk left undecided: which positions hold an entry, and the index inside the chunk
            const uint32_t T = unx.x + unx.y, R = (T + 255u) >> 8, p0 = w * (R << 6) + lane;
#pragma unroll
            for (int j = 0; j < GC_ITEMS; ++j) {
                const uint32_t p = p0 + j * 64;
                if (!((uint32_t)j < R && p < T)) wv[j] = 0u; // (j >= R: the position is the next wave's)
                idv[j] = (p >= unx.x ? GU : 0u) + nid[j];
            }
        }
        if (chunk + 1u < chunk1) load_chunk(chunk + 1u); // (uniform) prefetch: consumed at the top of the next trip
        if (DENSE) un = chunk + 2u < chunk1 ? unit_pair(unit_n, chunk + 2u) : make_uint2(0u, 0u); // (the pair of the chunk after that)
        {   // zero this wave's ranking counters (2 KB: 32 bytes a lane)
            S.u.zero[w * (GBINS / 8) + lane] = make_uint4(0u, 0u, 0u, 0u);
            S.u.zero[w * (GBINS / 8) + 64 + lane] = make_uint4(0u, 0u, 0u, 0u);
        }
        // ---- rank the visible gaussians by bucket where they are: (item, lane) of wave w IS the index order ----
        // peers = visible lanes holding the same bucket (10 ballots)
        uint32_t rank2[GC_ITEMS / 2];
#pragma unroll
        for (int j = 0; j < GC_ITEMS; ++j) {
            if (!(wv[j] & GS_COUNT_MASK)) wv[j] = 0u;
            const unsigned long long vis = __ballot(wv[j] != 0u);
            uint32_t r = 0;
            if (vis) { // (uniform over the wave)
                const uint32_t d = wv[j] >> GS_COUNT_BITS;
                uint32_t plo = (uint32_t)vis, phi = (uint32_t)(vis >> 32); // (the ballots of wave_rank in place: 128 instructions more as a call)
#pragma unroll
                for (int b = 0; b < 10; ++b) {
                    const uint32_t bit = (d >> b) & 1u;
                    const unsigned long long bal = __ballot(bit != 0u);
                    const uint32_t inv = bit - 1u;
                    plo &= (uint32_t)bal ^ inv;
                    phi &= (uint32_t)(bal >> 32) ^ inv;
                }
                r = wave_rank_peers(S.u.whist[w], d, plo, phi, wv[j] != 0u, lt_mask); // < 2048
            }
            rank2_put(rank2, j, r);
        }
        __syncthreads();
        // ---- per-wave counts -> exclusive across waves; bucket starts inside the chunk; the chunk's visible gaussians ----
        uint32_t nc;
        {
            uint32_t tot[BPT], acc = 0;
#pragma unroll
            for (uint32_t i = 0; i < BPT; ++i) {
                const uint32_t b = tid * BPT + i;
                uint32_t run = 0;
#pragma unroll
                for (int k = 0; k < GC_THREADS / 64; ++k) { const uint32_t c = S.u.whist[k][b]; S.u.whist[k][b] = (unsigned short)run; run += c; }
                tot[i] = run;
                acc += run;
            }
            uint32_t run = block_excl_u32<GC_THREADS / 64, uint32_t>(acc, tid, S.w1, nc);
#pragma unroll
            for (uint32_t i = 0; i < BPT; ++i) { S.binstart[tid * BPT + i] = (unsigned short)run; run += tot[i]; }
        }
        // (uniform) nothing visible: the bases do not move.  Every read of the ranking counters lies before block_excl_u32's
        // barriers and nothing written since is read again, so the next trip may start at once.
        if (nc == 0) continue;
        __syncthreads();
        // ---- reorder through LDS: the sorted arrays were last read before the barrier that ended the previous trip ----
#pragma unroll
        for (int j = 0; j < GC_ITEMS; ++j) {
            if (wv[j]) {
                const uint32_t d = wv[j] >> GS_COUNT_BITS;
                const uint32_t r = rank2_get(rank2, j);
                const uint32_t pos = (uint32_t)S.binstart[d] + (uint32_t)S.u.whist[w][d] + r;
                S.id[pos] = (unsigned short)(DENSE ? idv[j] : w * (64 * GC_ITEMS) + j * 64 + lane);
                S.word[pos] = wv[j];
                S.aux[pos] = av[j];
            }
        }
        __syncthreads(); // (every wave has read the ranking counters as well: the prefix below overwrites them)
        // ---- exclusive scan of the quantities in sorted order (thread t: slots 8t .. 8t+7) ----
        {
            uint32_t c[GC_ITEMS], acc = 0; // (8 x 2^22 at most)
#pragma unroll
            for (int j = 0; j < GC_ITEMS; ++j) {
                const uint32_t p = tid * GC_ITEMS + j;
                c[j] = (p < nc) ? (S.word[p] & GS_COUNT_MASK) : 0u;
                acc += c[j];
            }
            unsigned long long total;
            unsigned long long run = block_excl_u32<GC_THREADS / 64, unsigned long long>(acc, tid, S.w1, total);
#pragma unroll
            for (int j = 0; j < GC_ITEMS; ++j) { S.u.P[tid * GC_ITEMS + j] = sat32(run); run += c[j]; }
            if (tid == 0) S.ptot = sat32(total);
        }
        __syncthreads();
        // ---- store: coalesced over the sorted slots ----
#pragma unroll
        for (int j = 0; j < GC_ITEMS; ++j) {
            const uint32_t pos = j * GC_THREADS + tid;
            if (pos >= nc) continue;
            const uint32_t x = S.word[pos];
            const uint32_t b = x >> GS_COUNT_BITS, first = S.binstart[b];
            const uint2 base = S.base[b];
            const uint32_t g = base.x + (pos - first);
            const unsigned long long off64 = (unsigned long long)base.y + (S.u.P[pos] - S.u.P[first]);
            const uint32_t off = sat32(off64);
            grec[g] = make_uint4(chunk * GC + (uint32_t)S.id[pos], x, off, S.aux[pos]);
            const uint32_t cnt = x & GS_COUNT_MASK; // > 0: only visible gaussians are here
            if (off != 0xFFFFFFFFu) {
                const unsigned long long lastq = (off64 + cnt - 1ull) >> GS_EMIT_CHUNK_SHIFT;
                const uint32_t last = lastq > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)lastq;
                for (uint32_t c = (uint32_t)((off64 + (1u << GS_EMIT_CHUNK_SHIFT) - 1ull) >> GS_EMIT_CHUNK_SHIFT); c <= last && c < chunk_cap; ++c) chunk_table[c] = g;
            }
        }
        // ---- the bases advance by the chunk's own (count, quantity) of every bucket (see "Saturation" in the header) ----
        if (chunk + 1u < chunk1) { // (uniform)
            uint32_t dx[BPT], py[BPT + 1];
            uint32_t s = S.binstart[tid * BPT];
            py[0] = s < GC ? S.u.P[s] : S.ptot;
#pragma unroll
            for (uint32_t i = 0; i < BPT; ++i) {
                const uint32_t b = tid * BPT + i;
                const uint32_t e = (b + 1u < GBINS) ? (uint32_t)S.binstart[b + 1u] : nc;
                dx[i] = e - s;
                py[i + 1] = e < GC ? S.u.P[e] : S.ptot;
                s = e;
            }
            __syncthreads(); // every thread has read the bases, P and the bucket starts of this trip
#pragma unroll
            for (uint32_t i = 0; i < BPT; ++i) {
                uint2 v = S.base[tid * BPT + i];
                v.x += dx[i];
                v.y = py[i + 1] == 0xFFFFFFFFu ? 0xFFFFFFFFu : sat32((unsigned long long)v.y + (py[i + 1] - py[i]));
                S.base[tid * BPT + i] = v;
            }
        }
    }
}

// ---- host launchers --------------------------------------------------------------------------------
uint32_t gs_gsort_tiles(uint32_t n) { return (n + GC - 1) / GC; }
// An upper bound for every n and every number of runs: the table has min(NT, runs) <= NT columns.
uint64_t gs_gsort_scratch_bytes(uint32_t n) { return ((uint64_t)GBINS * gs_gsort_tiles(n ? n : 1) + GBINS) * sizeof(uint2); }
// words: one word per gaussian INDEX (quantity in the low 22 bits, depth bucket in the high 10; 0 = not visible); scratch:
// gs_gsort_scratch_bytes(n) bytes; grid: the context's persistent grid, from which the number of runs follows.  Output
// records in (bucket, index) order; tot_visible / tot_quantity: device words.
// unit_n != nullptr: the DENSE input form -- words, aux_in and unit_off are the entry planes (whole chunks: gs_gsort_tiles(n) * 2048
// entries each), unit_n the 2 * gs_gsort_tiles(n) + 2 unit counts.
void gs_launch_gsort(const uint32_t* words, const uint32_t* aux_in, const unsigned short* unit_off, const uint32_t* unit_n, uint32_t n, void* scratch,
                     void* grec, uint32_t* chunk_table, uint32_t chunk_cap, uint32_t* tot_visible, uint32_t* tot_quantity, uint32_t grid, hipStream_t st) {
    if (!n) return;
    const uint32_t NT = gs_gsort_tiles(n);
    uint64_t want = (uint64_t)grid * GS_GSORT_RUNS_Q / 4u;
    if (!want) want = 1;
    const uint32_t cpr = (uint32_t)((NT + want - 1) / want); // chunks per run
    const uint32_t G = (NT + cpr - 1) / cpr;                 // runs that hold a chunk: min(NT, want) at most
    uint2* M = (uint2*)scratch;
    uint2* rowtot = M + (uint64_t)GBINS * G;
    const uint2* un = (const uint2*)unit_n;
    if (un) hipLaunchKernelGGL(gs_gsort_hist_kernel<true>, dim3(G), dim3(GC_THREADS), 0, st, words, un, n, M, G, cpr, NT);
    else hipLaunchKernelGGL(gs_gsort_hist_kernel<false>, dim3(G), dim3(GC_THREADS), 0, st, words, un, n, M, G, cpr, NT);
    hipLaunchKernelGGL(gs_gsort_rowscan_kernel, dim3(GBINS / 8), dim3(GR_THREADS), 0, st, M, G, rowtot);
    if (un) hipLaunchKernelGGL(gs_gsort_scatter_kernel<true>, dim3(G), dim3(GC_THREADS), 0, st, words, aux_in, unit_off, un, n, (const uint2*)M, G, cpr, NT,
                               (const uint2*)rowtot, (uint4*)grec, chunk_table, chunk_cap, tot_visible, tot_quantity);
    else hipLaunchKernelGGL(gs_gsort_scatter_kernel<false>, dim3(G), dim3(GC_THREADS), 0, st, words, aux_in, unit_off, un, n, (const uint2*)M, G, cpr, NT,
                            (const uint2*)rowtot, (uint4*)grec, chunk_table, chunk_cap, tot_visible, tot_quantity);
}
