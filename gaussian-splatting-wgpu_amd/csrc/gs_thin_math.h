// gs_thin_math.h -- thinning (gs_abi.h "thinning"): what the kernels (k_thin.hip), the entry points and the host twin (gs_thin.hip,
// gs_thin_host) share, written once -- the hash of the index, the priority key, the rank, the refusals of a gs_thin that need no
// context -- and the host twin itself.  Plain C++ when the compiler is not hipcc (tools/thin_check builds it with a host compiler and
// sanitizers).
//
//   the rank      thin_hash, thin_pkey, thin_rank: R = (P << 32) | H.  thin_outranks: R_j > R_i, or equal and j < i.
//   the refusals  thin_check: struct_size, radius, flags, ascending without a priority, reserved words; r2 = radius * radius, ONE
//                 f32 product (every translation unit that includes this is compiled without contraction).
//   host only     thin_host: ANOTHER algorithm than the device's rounds -- the members sorted by rank, visited from the highest down;
//                 a member is dropped when a kept member is linked to it, and the kept ones go into a hashed grid of cells one
//                 radius wide, so a visit looks at the kept members of 27 cells.  The distance expression is the header's.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/gsplat/gs_abi.h"
#include "gs_grid_math.h" // neigh_finite

#include <algorithm>
#include <unordered_map>
#include <vector>

// ---- the rank -------------------------------------------------------------------------------------------------------------------------
GS_GRID uint32_t thin_hash(uint32_t i, uint32_t seed) { // a bijection of i for a fixed seed: every step is invertible mod 2^32
    uint32_t h = i + seed * 0x9E3779B9u;
    h ^= h >> 16; h *= 0x7FEB352Du;
    h ^= h >> 15; h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}
// P of a priority value given as its bit pattern: the splat attributes' order-preserving key, complemented when ascending; a NaN
// (either sign, quiet or signalling) is 0 in both directions.
GS_GRID uint32_t thin_pkey(uint32_t b, bool ascending) {
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0u;
    const uint32_t k = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return ascending ? ~k : k;
}
// have: there is a priority, whose value's bits are b
GS_GRID uint64_t thin_rank(uint32_t i, bool have, uint32_t b, uint32_t flags, uint32_t seed) {
    const uint32_t p = have ? thin_pkey(b, (flags & GS_THIN_ASCENDING) != 0u) : 0u;
    const uint32_t h = (flags & GS_THIN_ORDER_INDEX) ? ~i : thin_hash(i, seed);
    return ((uint64_t)p << 32) | h;
}
GS_GRID bool thin_outranks(uint64_t rj, uint32_t j, uint64_t ri, uint32_t i) { return rj > ri || (rj == ri && j < i); }

// ---- the refusals ---------------------------------------------------------------------------------------------------------------------
// Those of a gs_thin that need no context, in the header's order (the radius's own come from the caller: the device path has
// neigh_check_radius); have_priority: the call has priority values.  msg: the message's tail, it names the number.
inline bool thin_check(const gs_thin* q, bool have_priority, char* msg, size_t cap) {
    const uint32_t known = GS_THIN_ORDER_INDEX | GS_THIN_ASCENDING;
    if (q->flags & ~known) { snprintf(msg, cap, "unknown flags 0x%x", q->flags & ~known); return false; }
    if ((q->flags & GS_THIN_ASCENDING) && !have_priority) { snprintf(msg, cap, "flags 0x%x: GS_THIN_ASCENDING without a priority", q->flags); return false; }
    if (q->reserved0 != 0u) { snprintf(msg, cap, "reserved0 = %u is not 0", q->reserved0); return false; }
    for (int k = 0; k < 2; ++k)
        if (q->reserved[k] != 0u) { snprintf(msg, cap, "reserved[%d] = %u is not 0", k, q->reserved[k]); return false; }
    return true;
}

// ---- host only ------------------------------------------------------------------------------------------------------------------------
struct ThinCell {
    int64_t x, y, z;
    bool operator==(const ThinCell& o) const { return x == o.x && y == o.y && z == o.z; }
};
struct ThinCellHash {
    size_t operator()(const ThinCell& c) const {
        uint64_t h = (uint64_t)c.x * 0x9E3779B97F4A7C15ull;
        h = (h ^ (h >> 29)) + (uint64_t)c.y * 0xBF58476D1CE4E5B9ull;
        h = (h ^ (h >> 31)) + (uint64_t)c.z * 0x94D049BB133111EBull;
        return (size_t)(h ^ (h >> 32));
    }
};
// The whole call over host arrays.  0: done; 1: refused, msg says why.  The arguments are checked by the caller's rules (the header).
inline int thin_host(const float* px, const float* py, const float* pz, uint64_t n, const uint8_t* state, const float* priority, const gs_thin* q,
                     uint32_t* keeper, uint32_t* covers, gs_thin_info* info, char* msg, size_t cap) {
    if (!q) { snprintf(msg, cap, "null query"); return 1; }
    if (q->struct_size != sizeof(gs_thin)) { snprintf(msg, cap, "struct_size %u != %zu", q->struct_size, sizeof(gs_thin)); return 1; }
    if (q->mask > 0xFFu || q->value > 0xFFu) { snprintf(msg, cap, "filter (0x%x, 0x%x) does not fit the state byte", q->mask, q->value); return 1; }
    const float radius = q->radius;
    if (!(fabsf(radius) < INFINITY) || radius < 0.0f) { snprintf(msg, cap, "radius %g is negative or not finite", (double)radius); return 1; }
    const float r2 = radius * radius; // once, in f32
    if (!(fabsf(r2) < INFINITY)) { snprintf(msg, cap, "radius %g squared is not finite in f32", (double)radius); return 1; }
    if (!thin_check(q, priority != nullptr, msg, cap)) return 1;
    if (n >= (1ull << 32)) { snprintf(msg, cap, "%llu splats, an index takes 32 bits", (unsigned long long)n); return 1; }
    if (n && (!px || !py || !pz || !keeper || !covers)) { snprintf(msg, cap, "null array with n = %llu", (unsigned long long)n); return 1; }
    gs_thin_info out;
    memset(&out, 0, sizeof(out));
    out.cells[0] = out.cells[1] = out.cells[2] = 1u;

    // the members: rank, and the finite ones in descending rank
    struct Item { uint64_t r; uint32_t i; };
    std::vector<Item> order;
    std::vector<uint64_t> rank(n, 0);
    double maxabs = 0.0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t sv = state ? state[i] : 0u;
        keeper[i] = GS_THIN_NONE;
        covers[i] = 0u;
        if ((sv & q->mask) != q->value) continue;
        ++out.members;
        if (!neigh_finite(px[i], py[i], pz[i])) { keeper[i] = (uint32_t)i; covers[i] = 1u; ++out.kept; continue; } // linked to nobody
        uint32_t b = 0u;
        if (priority) memcpy(&b, priority + i, 4);
        rank[i] = thin_rank((uint32_t)i, priority != nullptr, b, q->flags, q->seed);
        order.push_back(Item{rank[i], (uint32_t)i});
        maxabs = std::max(maxabs, std::max((double)fabsf(px[i]), std::max((double)fabsf(py[i]), (double)fabsf(pz[i]))));
    }
    std::sort(order.begin(), order.end(), [](const Item& a, const Item& b) { return a.r != b.r ? a.r > b.r : a.i < b.i; });

    // Cells of edge h: a linked pair has |d| <= radius + 2^-74 per component (the products and r2 itself may underflow: each is off
    // by at most 2^-150), so with h above that the two cells differ by at most one per axis; h is also kept above maxabs 2^-50, which
    // bounds a cell coordinate by 2^50 (a larger h only puts more members into a cell).
    double h = ((double)radius + ldexp(1.0, -73)) * 1.001;
    h = std::max(h, maxabs * ldexp(1.0, -50));
    const auto cell_of = [&](uint32_t i) { return ThinCell{(int64_t)floor((double)px[i] / h), (int64_t)floor((double)py[i] / h), (int64_t)floor((double)pz[i] / h)}; };
    std::unordered_map<ThinCell, std::vector<uint32_t>, ThinCellHash> kept;
    for (const Item& it : order) {
        const uint32_t i = it.i;
        const ThinCell c = cell_of(i);
        bool found = false;
        uint32_t best = 0u;
        for (int64_t dz = -1; dz <= 1; ++dz)
            for (int64_t dy = -1; dy <= 1; ++dy)
                for (int64_t dx = -1; dx <= 1; ++dx) {
                    const auto at = kept.find(ThinCell{c.x + dx, c.y + dy, c.z + dz});
                    if (at == kept.end()) continue;
                    for (const uint32_t j : at->second) { // every kept member outranks i: it was visited before
                        ++out.candidates;
                        const float ex = px[j] - px[i], ey = py[j] - py[i], ez = pz[j] - pz[i];
                        if (!((ex * ex + ey * ey) + ez * ez <= r2)) continue;
                        if (!found || thin_outranks(rank[j], j, rank[best], best)) best = j;
                        found = true;
                    }
                }
        if (found) {
            keeper[i] = best;
            covers[best] += 1u;
        } else {
            keeper[i] = i;
            covers[i] = 1u;
            ++out.kept;
            kept[c].push_back(i);
        }
    }
    out.dropped = out.members - out.kept;
    for (uint64_t i = 0; i < n; ++i) out.largest = std::max<uint64_t>(out.largest, covers[i]);
    if (info) *info = out;
    return 0;
}
