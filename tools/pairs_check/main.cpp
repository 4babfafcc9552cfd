// tools/pairs_check -- gs_pair_host.h (on gs_exact_sum.h) on its own, for a host compiler with sanitizers (tests/test_register.py
// builds it with -fsanitize=address,undefined and runs it as its own process).
//
//   pairs_check [FILE]     FILE: "N" and then N lines "px py pz partner" -- three f32 bit patterns and a u32 id in hex.  Prints the pair
//                          moments of the scene with the filter (0, 0) and max_dist2 = +inf as gs_pair_moments_host orders them:
//                          "matched M paired P", then one line "hi lo" (the doubles' bit patterns in hex) per quantity.
// Before that it runs the host pairing loop on a scene of its own -- NaN, infinities, the largest and the smallest finite values among
// ordinary ones, in arrays of exactly N elements so that a read at or past N is the sanitizer's to catch -- with the partner planes
// all NONE, ids >= N, every id equal and j == i, with and without a filter, at three bounds, summing once in index order and once
// from both ends inwards: the limbs and both counts must be equal.  Then it prints "pairs_check ok".
#include <cfloat>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "gs_pair_host.h"

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

static PairSums run(const Scene& s, const std::vector<uint32_t>& partner, uint32_t mask, uint32_t value, float max_d2, bool inwards) {
    PairSums sums;
    pair_sums_clear(&sums);
    const uint64_t n = s.x.size();
    const uint8_t* st = (mask | value) ? s.state.data() : nullptr;
    if (!inwards) {
        for (uint64_t i = 0; i < n; ++i) pair_host_one(&sums, s.x.data(), s.y.data(), s.z.data(), n, partner.data(), st, mask, value, max_d2, i);
    } else {
        for (uint64_t lo = 0, hi = n; lo < hi;) {
            pair_host_one(&sums, s.x.data(), s.y.data(), s.z.data(), n, partner.data(), st, mask, value, max_d2, --hi);
            if (lo < hi) pair_host_one(&sums, s.x.data(), s.y.data(), s.z.data(), n, partner.data(), st, mask, value, max_d2, lo++);
        }
    }
    return sums;
}

static void self_check() {
    const uint32_t n = 1043u; // 3 mod 4
    const Scene s = own_scene(n);
    std::vector<uint32_t> none(n, 0xFFFFFFFFu), beyond(n), one(n, n / 2u), self(n);
    const uint32_t past[5] = {n, n + 1u, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (uint32_t i = 0; i < n; ++i) {
        self[i] = i;
        beyond[i] = (i % 3u == 0u) ? past[(i / 3u) % 5u] : (i * 577u + 13u) % n;
    }
    const std::vector<uint32_t>* planes[4] = {&none, &beyond, &one, &self};
    const float bounds[3] = {0.0f, 4.0f, INFINITY};
    for (int p = 0; p < 4; ++p)
        for (int f = 0; f < 2; ++f)
            for (int b = 0; b < 3; ++b) {
                const uint32_t mask = f ? 0x04u : 0u, value = mask;
                const PairSums a = run(s, *planes[p], mask, value, bounds[b], false), c = run(s, *planes[p], mask, value, bounds[b], true);
                CHECK(a.matched == c.matched && a.paired == c.paired);
                CHECK(memcmp(a.t, c.t, sizeof(a.t)) == 0);
                CHECK(a.matched == (f ? (n + 2u) / 3u : n) && a.paired <= a.matched);
                if (p == 0) {
                    CHECK(a.paired == 0u);
                    for (uint32_t k = 0; k < GS_PAIR_QUANTITIES * GS_EX_LIMBS; ++k) CHECK(a.t[k] == 0);
                    double hi, lo;
                    ex_finish(a.t, &hi, &lo);
                    CHECK(bits_of(hi) == 0u && bits_of(lo) == 0u); // an exact zero is {+0.0, +0.0}
                }
                if (p == 3) { // j == i: every finite splat pairs with itself at d2 = 0, so the bound does not matter and p = q
                    const PairSums z = run(s, self, mask, value, 0.0f, false);
                    CHECK(a.paired == z.paired && a.paired > 0u && memcmp(a.t, z.t, sizeof(a.t)) == 0);
                    for (uint32_t k = 0; k < 3u * GS_EX_LIMBS; ++k) CHECK(a.t[(size_t)GS_PAIR_SUM_P * GS_EX_LIMBS + k] == a.t[(size_t)GS_PAIR_SUM_Q * GS_EX_LIMBS + k]);
                    for (uint32_t k = 0; k < 3u * GS_EX_LIMBS; ++k) CHECK(a.t[(size_t)GS_PAIR_PP * GS_EX_LIMBS + k] == a.t[(size_t)GS_PAIR_QQ * GS_EX_LIMBS + k]);
                    for (uint32_t d = 0; d < 3u; ++d)
                        for (uint32_t k = 0; k < GS_EX_LIMBS; ++k) CHECK(a.t[(size_t)(GS_PAIR_PQ + 4u * d) * GS_EX_LIMBS + k] == a.t[(size_t)(GS_PAIR_PP + d) * GS_EX_LIMBS + k]);
                }
                if (p == 2 && b == 2 && !f) CHECK(a.paired > n / 2u); // everyone's partner is one finite splat
            }
    // the bound is inclusive, and an overflowed d2 passes +inf only
    {
        Scene t;
        t.x = {0.0f, 3.0f, FLT_MAX, -FLT_MAX}; t.y = {0.0f, 4.0f, 0.0f, 0.0f}; t.z = {0.0f, 0.0f, 0.0f, 0.0f};
        const std::vector<uint32_t> part = {1u, 0u, 3u, 2u};
        CHECK(run(t, part, 0u, 0u, 25.0f, false).paired == 2u);
        CHECK(run(t, part, 0u, 0u, std::nextafterf(25.0f, 0.0f), false).paired == 0u);
        CHECK(run(t, part, 0u, 0u, FLT_MAX, false).paired == 2u);
        CHECK(run(t, part, 0u, 0u, INFINITY, false).paired == 4u);
    }
}

int main(int argc, char** argv) {
    self_check();
    if (failures) return 1;
    printf("pairs_check ok\n");
    if (argc < 2) return 0;
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    unsigned long long n = 0;
    if (fscanf(f, "%llu", &n) != 1) { fclose(f); printf("bad header\n"); return 2; }
    Scene s;
    std::vector<uint32_t> partner;
    for (unsigned long long i = 0; i < n; ++i) {
        unsigned b[4] = {0, 0, 0, 0};
        if (fscanf(f, "%x %x %x %x", &b[0], &b[1], &b[2], &b[3]) != 4) { fclose(f); printf("bad row %llu\n", i); return 2; }
        s.x.push_back(f32_of(b[0])); s.y.push_back(f32_of(b[1])); s.z.push_back(f32_of(b[2]));
        partner.push_back(b[3]);
    }
    fclose(f);
    const PairSums a = run(s, partner, 0u, 0u, INFINITY, false), c = run(s, partner, 0u, 0u, INFINITY, true);
    if (a.matched != c.matched || a.paired != c.paired || memcmp(a.t, c.t, sizeof(a.t)) != 0) { printf("the two orders differ\n"); return 1; }
    printf("matched %" PRIu64 " paired %" PRIu64 "\n", a.matched, a.paired);
    for (unsigned t = 0; t < GS_PAIR_QUANTITIES; ++t) {
        double hi, lo;
        ex_finish(a.t + (size_t)t * GS_EX_LIMBS, &hi, &lo);
        printf("%016" PRIx64 " %016" PRIx64 "\n", bits_of(hi), bits_of(lo));
    }
    return 0;
}
