// k_pack.hip -- the kernels behind the packed scenes (gs_pack.hip, gs_abi.h "packed scenes"): Morton keys of a selection, the
// encoder of the 16-byte chunked layout, the SH bytes, and the decoder into the device planes.  The reference has no counterpart:
// its only container is the float .ply (ply.ts:49-228).  The arithmetic is gs_pack_math.h, the one copy the host codec compiles too.
//
// Entry g (0 .. m) is splat ids[g], or splat g when ids is null (index order without a filter: the gathers are dense reads).
//   keys   : one thread per entry: 12 B gathered, 8 B written (Morton key, id) for the pair sort (k_sort.hip).
//   encode : ONE WAVE PER CHUNK of 256 entries, four entries per lane (entry 64 j + lane: every store of a j is one contiguous KiB).
//            Per entry 4 B of id, 12 B of position, 32 B of geometry and the 12 B of SH band 0 are gathered; everything that does not
//            depend on the bounds (the rotation word, the alpha code) is finished at once, so 9 floats and 2 words per entry stay in
//            registers.  The 18 bounds are reduced over the wave as order keys (integer min / max: any order gives the same bits)
//            with six xor-shuffle steps; no LDS, no atomics.  Lanes 0 .. 17 write the 72-byte chunk record, every lane its four
//            vertices as one 16-byte store each, lane 0 the chunk's count of replaced floats.  60 B read, 16.3 B written per entry.
//            Bound: HBM (the gather's sectors: 32 of every 192 SH bytes are used).
//   sh     : one workgroup per chunk, one thread per output WORD of the chunk's contiguous 256 x 3K bytes (word-aligned for every
//            K: 768 K bytes); a byte is one SH float of one splat, so a word gathers four floats 12 bytes apart (or across a channel /
//            splat boundary) and the store is a whole coalesced word -- byte stores would cost a quarter of the bandwidth.  3K x 4 B
//            read, 3K B written per entry.  Bound: HBM / L2 (a splat's 180 bytes are read by ~45 neighbouring threads).
//   decode : one thread per (vertex, part), 16 parts: part 0 decodes the four words against the chunk record and writes the
//            position planes, smax, the 32-byte geometry record and SH band 0; part k writes coefficient k (its three bytes, or +0
//            above the file's degree).  Written at a destination offset `first`, as gs_ply_chunk_kernel does: upload and append share
//            it.  The logit table comes in as data (1 KiB, built on the host in double).  61 B read, 244 B written per splat.  Bound: HBM.
// No MFMA anywhere (no contraction).  No kernel uses scratch memory (profiles/packed.txt).  Every store is a plain vector store.
#include "gs_device.h"
#include "gs_kernels.h"
#include "gs_pack_math.h"

__global__ __launch_bounds__(256) void gs_pack_keys_kernel(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                            uint32_t n, const uint32_t* __restrict__ ids, uint32_t m, GsPackBox box,
                                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= m) return;
    const uint32_t id = ids ? ids[g] : g;
    uint32_t key = GS_PACK_KEY_LAST;
    if (id < n) key = pk_morton_key(px[id], py[id], pz[id], box.lo, box.hi); // (always: ids come from the selection over this scene)
    keys[g] = key;
    vals[g] = id;
}
void gs_launch_pack_keys(const GsScene& s, uint32_t n, const uint32_t* ids, uint32_t m, const GsPackBox& box, uint32_t* keys, uint32_t* vals,
                         hipStream_t st) {
    if (!m) return;
    hipLaunchKernelGGL(gs_pack_keys_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, s.px, s.py, s.pz, n, ids, m, box, keys, vals);
}

__global__ __launch_bounds__(256) void gs_pack_encode_kernel(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                              const float4* __restrict__ geo, const float* __restrict__ sh, uint32_t n,
                                                              const uint32_t* __restrict__ ids, uint32_t m, float* __restrict__ chunks,
                                                              uint4* __restrict__ vertices, uint32_t* __restrict__ bad) {
    const uint32_t chunk = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if ((uint64_t)chunk * GS_PACK_CHUNK >= m) return; // (the whole wave: no lane of a live wave leaves before the shuffles)
    PkEntry e[4];
    uint32_t lo[9], hi[9], nbad = 0u;
#pragma unroll
    for (int k = 0; k < 9; ++k) { lo[k] = 0xFFFFFFFFu; hi[k] = 0u; }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t g = chunk * GS_PACK_CHUNK + 64u * (uint32_t)j + lane;
        float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0;
        float x = 0.0f, y = 0.0f, z = 0.0f, d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
        const bool live = g < m;
        if (live) {
            const uint32_t id = ids ? ids[g] : g;
            if (id < n) { // (always: ids come from the selection over this scene)
                x = px[id]; y = py[id]; z = pz[id];
                g0 = geo[(uint64_t)id * 2]; g1 = geo[(uint64_t)id * 2 + 1];
                const float* q = sh + (uint64_t)id * 48;
                d0 = q[0]; d1 = q[1]; d2 = q[2];
            }
        }
        e[j] = pk_entry(x, y, z, g0.x, g0.y, g0.z, g1.x, g1.y, g1.z, g1.w, g0.w, d0, d1, d2);
        if (live) {
            nbad += e[j].bad;
            const float v[9] = {e[j].px, e[j].py, e[j].pz, e[j].sx, e[j].sy, e[j].sz, e[j].cr, e[j].cg, e[j].cb};
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const uint32_t key = pk_okey(v[k]);
                lo[k] = key < lo[k] ? key : lo[k];
                hi[k] = key > hi[k] ? key : hi[k];
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const uint32_t a = (uint32_t)__shfl_xor((int)lo[k], d, 64), b = (uint32_t)__shfl_xor((int)hi[k], d, 64);
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
    }
    const uint32_t total_bad = wave_sum(nbad);
    float b[18]; // the chunk record, on every lane
#pragma unroll
    for (int part = 0; part < 3; ++part)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            b[6 * part + k] = pk_okey_value(lo[3 * part + k]);
            b[6 * part + 3 + k] = pk_okey_value(hi[3 * part + k]);
        }
    float mine = b[0];
#pragma unroll
    for (int k = 1; k < 18; ++k) mine = lane == (uint32_t)k ? b[k] : mine;
    if (lane < GS_PACK_CHUNK_FLOATS) chunks[(uint64_t)chunk * GS_PACK_CHUNK_FLOATS + lane] = mine;
    if (lane == 0u) bad[chunk] = total_bad;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t g = chunk * GS_PACK_CHUNK + 64u * (uint32_t)j + lane;
        uint32_t w[4];
        pk_vertex(e[j], b, w);
        if (g < m) vertices[g] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__global__ __launch_bounds__(256) void gs_pack_sh_kernel(const float* __restrict__ sh, uint32_t n, const uint32_t* __restrict__ ids, uint32_t m, uint32_t K,
                                                          uint32_t* __restrict__ out, uint32_t* __restrict__ bad) {
    const uint32_t chunk = blockIdx.x, first = chunk * GS_PACK_CHUNK; // (the grid is ceil(m / 256): first < m)
    const uint32_t cnt = m - first < GS_PACK_CHUNK ? m - first : GS_PACK_CHUNK;
    const uint32_t K3 = 3u * K, bytes = cnt * K3, words = (bytes + 3u) / 4u;
    uint32_t* const dst = out + (uint64_t)chunk * (64u * K3); // 256 x 3K bytes per chunk
    uint32_t nbad = 0u;
    for (uint32_t w = threadIdx.x; w < words; w += 256u) {
        uint32_t word = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t at = 4u * w + k;
            if (at < bytes) {
                const uint32_t j = at / K3, r = at - j * K3, c = r / K, i = r - c * K;
                const uint32_t id = ids ? ids[first + j] : first + j;
                const float v = id < n ? sh[(uint64_t)id * 48 + 3u * (i + 1u) + c] : 0.0f; // (always id < n)
                nbad += pk_finite(v) ? 0u : 1u;
                word |= pk_sh_byte(v) << (8u * k);
            }
        }
        dst[w] = word;
    }
    const uint32_t total_bad = wave_sum(nbad);
    if ((threadIdx.x & 63u) == 0u) bad[(uint64_t)chunk * 4u + (threadIdx.x >> 6)] = total_bad;
}

void gs_launch_pack_encode(const GsScene& s, uint32_t n, const uint32_t* ids, uint32_t m, uint32_t K, float* chunks, void* vertices, void* sh_bytes,
                           uint32_t* bad, hipStream_t st) {
    if (!m) return;
    const uint32_t C = (uint32_t)(((uint64_t)m + GS_PACK_CHUNK - 1u) / GS_PACK_CHUNK);
    hipLaunchKernelGGL(gs_pack_encode_kernel, dim3((C + 3u) / 4u), dim3(256), 0, st, s.px, s.py, s.pz, s.geo, (const float*)s.sh, n, ids, m, chunks,
                       (uint4*)vertices, bad);
    if (K) hipLaunchKernelGGL(gs_pack_sh_kernel, dim3(C), dim3(256), 0, st, (const float*)s.sh, n, ids, m, K, (uint32_t*)sh_bytes, bad + C);
}

__global__ __launch_bounds__(256) void gs_pack_decode_kernel(GsPackTrip t, uint32_t first, float* px, float* py, float* pz, float* smax, float* geo,
                                                              float* sh) {
    const uint64_t id = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (uint64_t)t.m * 16) return;
    const uint32_t v = (uint32_t)(id >> 4), part = (uint32_t)(id & 15u);
    const uint64_t g = (uint64_t)first + v;
    if (part == 0u) {
        const uint4 q = t.vertices[v];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        const PkDecoded d = pk_decode(w, t.chunks + (uint64_t)(v >> 8) * GS_PACK_CHUNK_FLOATS, t.table);
        px[g] = d.pos[0]; py[g] = d.pos[1]; pz[g] = d.pos[2];
        smax[g] = __builtin_fmaxf(d.lsc[0], __builtin_fmaxf(d.lsc[1], d.lsc[2])); // as gs_repack_kernel derives it
        float4* r = reinterpret_cast<float4*>(geo) + g * 2;
        r[0] = make_float4(d.lsc[0], d.lsc[1], d.lsc[2], d.logit);
        r[1] = make_float4(d.rot[0], d.rot[1], d.rot[2], d.rot[3]);
        float* c0 = sh + g * 48;
        c0[0] = d.dc[0]; c0[1] = d.dc[1]; c0[2] = d.dc[2];
    } else {
        float a = 0.0f, b = 0.0f, c = 0.0f; // coefficient `part`: zero above the file's degree
        if (part <= t.K) {
            const uint8_t* in = t.sh + (uint64_t)v * (3u * t.K) + (part - 1u);
            a = pk_sh_value(in[0]); b = pk_sh_value(in[t.K]); c = pk_sh_value(in[2u * t.K]);
        }
        float* q = sh + g * 48 + 3u * part;
        q[0] = a; q[1] = b; q[2] = c;
    }
}
void gs_launch_pack_decode(const GsPackTrip& t, uint32_t first, const GsScene& dst, hipStream_t st) {
    const uint64_t total = (uint64_t)t.m * 16;
    if (!total) return;
    hipLaunchKernelGGL(gs_pack_decode_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, t, first, (float*)dst.px, (float*)dst.py,
                       (float*)dst.pz, (float*)dst.smax, (float*)dst.geo, (float*)dst.sh);
}
