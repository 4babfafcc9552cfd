// gs_grid_math.h -- the uniform cell grid of the neighbourhoods (gs_neigh.hip, k_neigh.hip, k_cluster.hip, k_knn.hip) and of the cell
// merge (gs_merge.hip, k_merge.hip, gs_merge_math.h), written once for host and device: the grid record, the finite test, the cell
// coordinate, the key packing and the choice of the grid on the host.  Plain C++ when the compiler is not hipcc (tools/merge_check
// builds it with a host compiler and sanitizers).  Why the cell expression is safe for a 27-cell search is argued in k_neigh.hip.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_GRID __host__ __device__ __forceinline__
#else
#define GS_GRID inline
#endif

// The grid over the finite members: cell coordinate of x on axis k = clamp((int)floorf((x - lo[k]) * inv_h), 0, g[k] - 1), key =
// cz << bxy | cy << bx | cx (bx, bxy - bx: the bits of g[0] - 1, g[1] - 1).  `none` = g[2] << bxy is above every key and marks a splat
// that is no member: it sorts last.  The neighbourhoods' {start, end} table has `blocks` = none >> shift entries, one per 2^shift
// consecutive keys (shift 0: one per cell); the cell merge reads neither.
struct GsNeighGrid { float lo[3]; float inv_h; uint32_t g[3]; uint32_t bx, bxy, shift, blocks, none; };

GS_GRID bool neigh_finite(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; // (a NaN fails)
}
GS_GRID int neigh_cell(float x, float lo, float inv_h, uint32_t g) {
    return (int)fminf(fmaxf(floorf((x - lo) * inv_h), 0.0f), (float)(g - 1u)); // (fmaxf: a NaN product -- 0 * inf -- is cell 0)
}
GS_GRID uint32_t neigh_key(const GsNeighGrid& g, float x, float y, float z) {
    const uint32_t cx = (uint32_t)neigh_cell(x, g.lo[0], g.inv_h, g.g[0]), cy = (uint32_t)neigh_cell(y, g.lo[1], g.inv_h, g.g[1]),
                   cz = (uint32_t)neigh_cell(z, g.lo[2], g.inv_h, g.g[2]);
    return (cz << g.bxy) | (cy << g.bx) | cx;
}

// ---- host only ------------------------------------------------------------------------------------------------------------------------
inline uint32_t neigh_bits_of(uint32_t v) { uint32_t b = 0; while (b < 32 && (v >> b)) ++b; return b; }
// The grid for members with the finite bounds lo .. hi and a wanted cell edge (the neighbourhoods ask for 1.0011 radius: the margin
// the cell expression's rounding needs for the 27-cell search, k_neigh.hip; the cell merge for the requested edge itself): the
// smallest edge h >= wanted that leaves at most 1024 cells per axis; the key layout and the table's blocks.  *edge: h.
inline void neigh_choose_grid(const float lo[3], const float hi[3], float wanted, GsNeighGrid* g, float* edge) {
    double ext[3], widest = 0.0;
    for (int k = 0; k < 3; ++k) { ext[k] = (double)hi[k] - (double)lo[k]; widest = ext[k] > widest ? ext[k] : widest; }
    float h = wanted;
    const float hmin = (float)(widest / 1024.0 * 1.000001);
    h = h < hmin ? hmin : h; // (std::max(h, hmin))
    if (!(h >= 1e-30f)) h = widest > 0.0 ? 1e-30f : 1.0f; // (all members in one point and no edge wanted: any edge does)
    if (!(fabsf(h) < INFINITY)) h = 3.0e38f;
    for (int k = 0; k < 3; ++k) {
        const double cells = floor(ext[k] / (double)h) + 1.0;
        g->g[k] = (uint32_t)(cells < 1024.0 ? cells : 1024.0);
        g->lo[k] = lo[k];
    }
    g->inv_h = 1.0f / h;
    g->bx = neigh_bits_of(g->g[0] - 1u);
    g->bxy = g->bx + neigh_bits_of(g->g[1] - 1u);
    g->none = g->g[2] << g->bxy; // <= 2^30
    const uint32_t kb = neigh_bits_of(g->none - 1u);
    g->shift = kb > 24u ? kb - 24u : 0u; // < bxy, so `none` is a multiple of 2^shift
    g->blocks = g->none >> g->shift;     // <= 2^24
    *edge = h;
}
