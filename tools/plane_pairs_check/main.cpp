// tools/plane_pairs_check -- gs_plane_pair_host.h (on gs_pair_host.h and gs_exact_sum.h) on its own, for a host compiler with
// sanitizers (tests/test_register_plane.py builds it with -fsanitize=address,undefined and runs it as its own process).
//
//   plane_pairs_check [FILE]   FILE: "N", "pvx pvy pvz" and then N lines "px py pz partner nx ny nz" -- f32 bit patterns and a u32 id
//                              in hex.  Prints the plane pair moments of the scene with the filter (0, 0) and max_dist2 = +inf as
//                              gs_pair_plane_moments_host orders them: "matched M paired P", then one line "hi lo" (the doubles' bit
//                              patterns in hex) per quantity, 29 in all.
// Before that it runs the host pairing loop on a scene of its own -- NaN, infinities, the largest and the smallest finite values among
// ordinary ones, in arrays of exactly N elements (3 N for the normals) so that a read at or past N is the sanitizer's to catch -- with
// the partner planes all NONE, ids >= N, every id equal and j == i, the normal planes unit, NaN for a third and huge, with and without
// a filter, at three bounds, summing once in index order and once from both ends inwards: the limbs and both counts must be equal.
// Then it prints "plane_pairs_check ok".
#include <cfloat>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "gs_plane_pair_host.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static float f32_of(uint32_t b) { float v; memcpy(&v, &b, 4); return v; }
static uint64_t bits_of(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

struct Scene {
    std::vector<float> x, y, z;
    std::vector<uint8_t> state;
};

static Scene own_scene(uint32_t n) {
    Scene s;
    uint32_t w = 12345u;
    for (uint32_t i = 0; i < n; ++i) {
        float v[3];
        for (int a = 0; a < 3; ++a) {
            w = w * 1664525u + 1013904223u;
            v[a] = (float)((int32_t)(w >> 8) % 20001 - 10000) * 1.0e-3f;
        }
        if (i % 37u == 5u) v[i % 3u] = std::numeric_limits<float>::quiet_NaN();
        if (i % 41u == 7u) v[(i + 1u) % 3u] = (i & 1u) ? INFINITY : -INFINITY;
        if (i % 43u == 9u) v[i % 3u] = (i & 1u) ? FLT_MAX : -FLT_MAX; // d2 overflows to +inf
        if (i % 47u == 11u) v[(i + 2u) % 3u] = f32_of(1u);            // 2^-149
        if (i % 10u == 5u) { v[0] = s.x[i - 1u]; v[1] = s.y[i - 1u]; v[2] = s.z[i - 1u]; } // an exact duplicate of its predecessor
        s.x.push_back(v[0]); s.y.push_back(v[1]); s.z.push_back(v[2]);
        s.state.push_back((uint8_t)((i * 7u) & 0x73u) | (i % 3u == 0u ? 0x04u : 0u));
    }
    return s;
}

// kind 0: unit-length axes in turn; 1: those with NaN 0x7FC00000 for every third splat; 2: huge, so that c or r overflows
static std::vector<float> own_normals(uint32_t n, int kind) {
    std::vector<float> out;
    for (uint32_t i = 0; i < n; ++i) {
        float v[3] = {0.6f, 0.0f, 0.8f};
        if (i % 3u == 1u) { v[0] = 0.0f; v[1] = 1.0f; v[2] = 0.0f; }
        if (i % 3u == 2u) { v[0] = -0.8f; v[1] = 0.6f; v[2] = 0.0f; }
        if (kind == 1 && i % 3u == 1u) v[0] = v[1] = v[2] = f32_of(0x7FC00000u);
        if (kind == 2) { v[0] *= 1.0e38f; v[1] *= 3.0e37f; v[2] *= (i & 1u) ? 1.0e-30f : 2.0e38f; }
        out.push_back(v[0]); out.push_back(v[1]); out.push_back(v[2]);
    }
    return out;
}

static PlaneSums run(const Scene& s, const std::vector<uint32_t>& partner, const std::vector<float>& normal, uint32_t mask, uint32_t value,
                     const float pivot[3], float max_d2, bool inwards) {
    PlaneSums sums;
    plane_sums_clear(&sums);
    const uint64_t n = s.x.size();
    const uint8_t* st = (mask | value) ? s.state.data() : nullptr;
    const auto one = [&](uint64_t i) { plane_host_one(&sums, s.x.data(), s.y.data(), s.z.data(), n, partner.data(), normal.data(), st, mask, value, pivot, max_d2, i); };
    if (!inwards) {
        for (uint64_t i = 0; i < n; ++i) one(i);
    } else {
        for (uint64_t lo = 0, hi = n; lo < hi;) {
            one(--hi);
            if (lo < hi) one(lo++);
        }
    }
    return sums;
}

static bool table_zero(const PlaneSums& a, uint32_t t) {
    for (uint32_t k = 0; k < GS_EX_LIMBS; ++k)
        if (a.t[(size_t)t * GS_EX_LIMBS + k] != 0) return false;
    return true;
}

static void self_check() {
    // the factor table: the upper triangle row-major, then (k, r), then (r, r)
    uint32_t t = 0;
    for (uint32_t a = 0; a < 6u; ++a)
        for (uint32_t b = a; b < 6u; ++b, ++t) CHECK(plane_fa(t) == a && plane_fb(t) == b);
    for (uint32_t k = 0; k < 6u; ++k, ++t) CHECK(plane_fa(t) == k && plane_fb(t) == 6u);
    CHECK(t == GS_PLANE_RR && plane_fa(t) == 6u && plane_fb(t) == 6u);

    const uint32_t n = 1043u; // 3 mod 4
    const Scene s = own_scene(n);
    std::vector<uint32_t> none(n, 0xFFFFFFFFu), beyond(n), one(n, n / 2u), self(n);
    const uint32_t past[5] = {n, n + 1u, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (uint32_t i = 0; i < n; ++i) {
        self[i] = i;
        beyond[i] = (i % 3u == 0u) ? past[(i / 3u) % 5u] : (i * 577u + 13u) % n;
    }
    const std::vector<uint32_t>* planes[4] = {&none, &beyond, &one, &self};
    const std::vector<float> normals[3] = {own_normals(n, 0), own_normals(n, 1), own_normals(n, 2)};
    const float bounds[3] = {0.0f, 4.0f, INFINITY};
    const float pivots[2][3] = {{0.0f, 0.0f, 0.0f}, {1.0e4f, -3.0e3f, 77.5f}};
    for (int p = 0; p < 4; ++p)
        for (int nk = 0; nk < 3; ++nk)
            for (int f = 0; f < 2; ++f)
                for (int b = 0; b < 3; ++b)
                    for (int pv = 0; pv < 2; ++pv) {
                        const uint32_t mask = f ? 0x04u : 0u, value = mask;
                        const PlaneSums a = run(s, *planes[p], normals[nk], mask, value, pivots[pv], bounds[b], false);
                        const PlaneSums c = run(s, *planes[p], normals[nk], mask, value, pivots[pv], bounds[b], true);
                        CHECK(a.matched == c.matched && a.paired == c.paired);
                        CHECK(memcmp(a.t, c.t, sizeof(a.t)) == 0);
                        CHECK(a.matched == (f ? (n + 2u) / 3u : n) && a.paired <= a.matched);
                        if (p == 0) {
                            CHECK(a.paired == 0u);
                            for (uint32_t q = 0; q < GS_PLANE_QUANTITIES; ++q) CHECK(table_zero(a, q));
                            double hi, lo;
                            ex_finish(a.t, &hi, &lo);
                            CHECK(bits_of(hi) == 0u && bits_of(lo) == 0u); // an exact zero is {+0.0, +0.0}
                        }
                        if (p == 3) { // j == i: d = 0, so r = 0 and d2 = 0 whatever the bound: h, rr and d2 are exact zeros
                            if (nk == 0) CHECK(a.paired > 0u);
                            for (uint32_t q = GS_PLANE_H; q < GS_PLANE_QUANTITIES; ++q) CHECK(table_zero(a, q));
                            const PlaneSums z = run(s, self, normals[nk], mask, value, pivots[pv], 0.0f, false);
                            CHECK(a.paired == z.paired && memcmp(a.t, z.t, sizeof(a.t)) == 0);
                        }
                    }
    // the bound is inclusive, an overflowed d2 passes +inf only, a NaN normal is matched but not paired
    {
        Scene t2;
        t2.x = {0.0f, 3.0f, 2.0e19f, -2.0e19f}; t2.y = {0.0f, 4.0f, 0.0f, 0.0f}; t2.z = {0.0f, 0.0f, 0.0f, 0.0f};
        const std::vector<uint32_t> part = {1u, 0u, 3u, 2u};
        std::vector<float> nz(12, 0.0f);
        for (int i = 0; i < 4; ++i) nz[3 * i + 2] = 1.0f;
        const float zero[3] = {0.0f, 0.0f, 0.0f};
        CHECK(run(t2, part, nz, 0u, 0u, zero, 25.0f, false).paired == 2u);
        CHECK(run(t2, part, nz, 0u, 0u, zero, std::nextafterf(25.0f, 0.0f), false).paired == 0u);
        CHECK(run(t2, part, nz, 0u, 0u, zero, FLT_MAX, false).paired == 2u);
        CHECK(run(t2, part, nz, 0u, 0u, zero, INFINITY, false).paired == 4u);
        nz[3] = nz[4] = nz[5] = f32_of(0x7FC00000u); // splat 1's normal: splat 0, whose partner it is, is no longer paired
        const PlaneSums a = run(t2, part, nz, 0u, 0u, zero, 25.0f, false);
        CHECK(a.matched == 4u && a.paired == 1u);
    }
}

int main(int argc, char** argv) {
    self_check();
    if (failures) return 1;
    printf("plane_pairs_check ok\n");
    if (argc < 2) return 0;
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    unsigned long long n = 0;
    unsigned pb[3] = {0, 0, 0};
    if (fscanf(f, "%llu", &n) != 1 || fscanf(f, "%x %x %x", &pb[0], &pb[1], &pb[2]) != 3) { fclose(f); printf("bad header\n"); return 2; }
    const float pivot[3] = {f32_of(pb[0]), f32_of(pb[1]), f32_of(pb[2])};
    Scene s;
    std::vector<uint32_t> partner;
    std::vector<float> normal;
    for (unsigned long long i = 0; i < n; ++i) {
        unsigned b[7] = {0, 0, 0, 0, 0, 0, 0};
        if (fscanf(f, "%x %x %x %x %x %x %x", &b[0], &b[1], &b[2], &b[3], &b[4], &b[5], &b[6]) != 7) { fclose(f); printf("bad row %llu\n", i); return 2; }
        s.x.push_back(f32_of(b[0])); s.y.push_back(f32_of(b[1])); s.z.push_back(f32_of(b[2]));
        partner.push_back(b[3]);
        normal.push_back(f32_of(b[4])); normal.push_back(f32_of(b[5])); normal.push_back(f32_of(b[6]));
    }
    fclose(f);
    const PlaneSums a = run(s, partner, normal, 0u, 0u, pivot, INFINITY, false), c = run(s, partner, normal, 0u, 0u, pivot, INFINITY, true);
    if (a.matched != c.matched || a.paired != c.paired || memcmp(a.t, c.t, sizeof(a.t)) != 0) { printf("the two orders differ\n"); return 1; }
    printf("matched %" PRIu64 " paired %" PRIu64 "\n", a.matched, a.paired);
    for (unsigned t = 0; t < GS_PLANE_QUANTITIES; ++t) {
        double hi, lo;
        ex_finish(a.t + (size_t)t * GS_EX_LIMBS, &hi, &lo);
        printf("%016" PRIx64 " %016" PRIx64 "\n", bits_of(hi), bits_of(lo));
    }
    return 0;
}
