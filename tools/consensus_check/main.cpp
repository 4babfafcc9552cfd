// tools/consensus_check -- gs_consensus_host.h on its own, for a host compiler with sanitizers (tests/test_consensus.py builds it with
// -fsanitize=address,undefined and runs it as its own process).
//
//   consensus_check [FILE]   FILE: "N H KIND LO HI" (KIND 11 = DIST2, 12 = PLANE; LO, HI f32 bit patterns in hex), then N lines
//                            "px py pz" and H lines "p0 p1 p2 p3", all f32 bit patterns in hex.  Prints "matched M" and then one
//                            count per line, with the filter (0, 0), as gs_consensus_host returns them.
// Without FILE it runs the host loop on a scene of its own -- NaN, infinities, denormals, the largest finite values and exact duplicates
// among ordinary ones, in arrays of exactly n elements so that a read at or past n is the sanitizer's to catch -- at the lengths
// 0, 1, 3, 4, 5, 1023, 1024, 1025 and 4099, with 1, 2, 63, 64, 65 and 4096 hypotheses (tables of exactly 4 h floats, NaN and infinite
// parameters among them), both kinds, with and without a filter, over ranges that are empty (lo > hi), infinite, a single value that
// occurs and its f32 neighbours; once in index order and once from both ends inwards: the counts must be equal, and equal to a
// count written out here.  Then gs_planes_through's plane_through on axis-aligned, repeated, collinear, non-finite and sign-tie
// triples.  Then it prints "consensus_check ok".
#include <cfloat>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "gs_consensus_host.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static float f32_of(uint32_t b) { float v; memcpy(&v, &b, 4); return v; }
static uint32_t bits_of(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }

struct Scene {
    std::vector<float> x, y, z;
    std::vector<uint8_t> state;
};

static Scene own_scene(uint32_t n) {
    Scene s;
    uint32_t w = 2463534242u;
    for (uint32_t i = 0; i < n; ++i) {
        float v[3];
        for (int a = 0; a < 3; ++a) {
            w = w * 1664525u + 1013904223u;
            v[a] = (float)((int32_t)(w >> 8) % 20001 - 10000) * 1.0e-3f;
        }
        if (i % 37u == 5u) v[i % 3u] = std::numeric_limits<float>::quiet_NaN();
        if (i % 41u == 7u) v[(i + 1u) % 3u] = (i & 1u) ? INFINITY : -INFINITY;
        if (i % 43u == 9u) v[i % 3u] = (i & 1u) ? FLT_MAX : -FLT_MAX;
        if (i % 47u == 11u) v[(i + 2u) % 3u] = f32_of(1u); // 2^-149
        if (i % 10u == 5u) { v[0] = s.x[i - 1u]; v[1] = s.y[i - 1u]; v[2] = s.z[i - 1u]; } // an exact duplicate of its predecessor
        s.x.push_back(v[0]); s.y.push_back(v[1]); s.z.push_back(v[2]);
        s.state.push_back((uint8_t)((i * 7u) & 0x73u) | (i % 3u == 0u ? 0x04u : 0u));
    }
    return s;
}

static std::vector<float> own_table(uint32_t kind, uint32_t h) {
    std::vector<float> p;
    uint32_t w = 88172645u;
    for (uint32_t j = 0; j < h; ++j) {
        float v[4];
        for (int a = 0; a < 4; ++a) {
            w = w * 1664525u + 1013904223u;
            v[a] = (float)((int32_t)(w >> 8) % 2001 - 1000) * (kind == GS_ATTR_PLANE && a < 3 ? 1.0e-3f : 1.0e-2f);
        }
        if (j % 29u == 1u) v[j % 4u] = std::numeric_limits<float>::quiet_NaN();
        if (j % 31u == 2u) v[j % 3u] = (j & 1u) ? INFINITY : -INFINITY;
        if (j % 33u == 4u) v[0] = v[1] = v[2] = v[3] = 0.0f;
        for (int a = 0; a < 4; ++a) p.push_back(v[a]);
    }
    return p;
}

struct Counts {
    std::vector<uint64_t> c;
    uint64_t matched = 0;
};

static Counts run(const Scene& s, uint32_t kind, const std::vector<float>& p, uint32_t mask, uint32_t value, float lo, float hi, bool inwards) {
    Counts out;
    const uint32_t h = (uint32_t)(p.size() / 4u);
    out.c.assign(h, 0u);
    const uint64_t n = s.x.size();
    const uint8_t* st = (mask | value) ? s.state.data() : nullptr;
    if (!inwards) {
        consensus_host_loop(kind, s.x.data(), s.y.data(), s.z.data(), n, st, mask, value, p.data(), h, lo, hi, out.c.data(), &out.matched);
        return out;
    }
    auto one = [&](uint64_t i) {
        if (kind == GS_ATTR_DIST2) consensus_host_one<GS_ATTR_DIST2>(s.x.data(), s.y.data(), s.z.data(), st, mask, value, p.data(), h, lo, hi, out.c.data(), &out.matched, i);
        else consensus_host_one<GS_ATTR_PLANE>(s.x.data(), s.y.data(), s.z.data(), st, mask, value, p.data(), h, lo, hi, out.c.data(), &out.matched, i);
    };
    for (uint64_t a = 0, b = n; a < b;) {
        one(--b);
        if (a < b) one(a++);
    }
    return out;
}

// the count of one hypothesis written out: volatile keeps every operation a rounding of its own whatever the flags
static uint64_t count_one(const Scene& s, uint32_t kind, const float* p, uint32_t mask, uint32_t value, float lo, float hi) {
    uint64_t c = 0;
    for (size_t i = 0; i < s.x.size(); ++i) {
        if ((mask | value) && (s.state[i] & mask) != value) continue;
        volatile float v;
        if (kind == GS_ATTR_DIST2) {
            volatile float dx = s.x[i] - p[0], dy = s.y[i] - p[1], dz = s.z[i] - p[2];
            volatile float xx = dx * dx, yy = dy * dy, zz = dz * dz, t = xx + yy;
            v = t + zz;
        } else {
            volatile float a = p[0] * s.x[i], b = p[1] * s.y[i], cc = p[2] * s.z[i], t = a + b, u = t + cc;
            v = u + p[3];
        }
        const float r = v;
        if (r >= lo && r <= hi) ++c;
    }
    return c;
}

static void self_check() {
    const uint32_t lengths[9] = {0u, 1u, 3u, 4u, 5u, 1023u, 1024u, 1025u, 4099u};
    const uint32_t tables[6] = {1u, 2u, 63u, 64u, 65u, 4096u};
    const uint32_t kinds[2] = {GS_ATTR_PLANE, GS_ATTR_DIST2};
    for (uint32_t n : lengths) {
        const Scene s = own_scene(n);
        for (uint32_t h : tables)
            for (uint32_t kind : kinds) {
                if ((uint64_t)n * h > 2000000u && n != 4099u) continue; // (the largest table against a long scene: once per kind, at the longest)
                const std::vector<float> p = own_table(kind, h);
                // a value that occurs: hypothesis 0 against the middle splat (if it is a number)
                float v0 = 1.0f;
                if (n) {
                    const GsAttrDev a = {{p[0], p[1], p[2], p[3]}};
                    const float v = kind == GS_ATTR_DIST2 ? attr_of_pos<GS_ATTR_DIST2>(a, s.x[n / 2u], s.y[n / 2u], s.z[n / 2u])
                                                          : attr_of_pos<GS_ATTR_PLANE>(a, s.x[n / 2u], s.y[n / 2u], s.z[n / 2u]);
                    if (v == v && std::isfinite(v)) v0 = v;
                }
                const float up = std::nextafterf(v0, INFINITY), down = std::nextafterf(v0, -INFINITY);
                const float ranges[7][2] = {{-INFINITY, INFINITY}, {v0, v0}, {v0, INFINITY}, {up, INFINITY}, {-INFINITY, down}, {1.0f, -1.0f}, {-1.5f, 1.5f}};
                const int nr = (uint64_t)n * h > 2000000u ? 2 : 7;
                for (int f = 0; f < 2; ++f)
                    for (int r = 0; r < nr; ++r) {
                        const uint32_t mask = f ? 0x04u : 0u, value = mask;
                        const float lo = ranges[r][0], hi = ranges[r][1];
                        const Counts a = run(s, kind, p, mask, value, lo, hi, false), b = run(s, kind, p, mask, value, lo, hi, true);
                        CHECK(a.matched == b.matched && a.c == b.c);
                        CHECK(a.matched == (f ? (n + 2u) / 3u : n));
                        const uint32_t probe[4] = {0u, h / 2u, h - 1u, h > 4u ? 4u : 0u};
                        for (uint32_t j : probe) CHECK(a.c[j] == count_one(s, kind, p.data() + 4u * j, mask, value, lo, hi));
                        for (uint32_t j = 0; j < h; ++j) CHECK(a.c[j] <= a.matched);
                        if (r == 5)
                            for (uint32_t j = 0; j < h; ++j) CHECK(a.c[j] == 0u); // lo > hi: the empty range
                        if (r == 1 && n && !f && v0 != 1.0f) CHECK(a.c[0] >= 1u); // inclusive at both ends
                        if (h > 1u) CHECK(a.c[1] == 0u);                          // a NaN parameter (p[1] of hypothesis 1): in no range
                    }
            }
    }
}

static void planes_check() {
    auto plane = [](std::vector<float> t) {
        std::vector<float> out(4);
        CHECK(t.size() == 9u);
        plane_through(t.data(), out.data());
        return out;
    };
    auto is = [](const std::vector<float>& p, float a, float b, float c, float d) {
        return bits_of(p[0]) == bits_of(a) && bits_of(p[1]) == bits_of(b) && bits_of(p[2]) == bits_of(c) && bits_of(p[3]) == bits_of(d);
    };
    auto all_nan = [](const std::vector<float>& p) { return p[0] != p[0] && p[1] != p[1] && p[2] != p[2] && p[3] != p[3]; };
    CHECK(is(plane({0, 0, 1, 1, 0, 1, 0, 1, 1}), 0.0f, 0.0f, 1.0f, -1.0f));      // z = 1
    CHECK(is(plane({0, 0, 1, 0, 1, 1, 1, 0, 1}), -0.0f, -0.0f, 1.0f, -1.0f));    // the other orientation: negated to +z
    CHECK(is(plane({2, 0, 0, 2, 1, 0, 2, 0, 1}), 1.0f, 0.0f, 0.0f, -2.0f));      // x = 2
    CHECK(all_nan(plane({1, 2, 3, 1, 2, 3, 4, 5, 6})));                           // a repeated point
    CHECK(all_nan(plane({0, 0, 0, 1, 1, 1, 2, 2, 2})));                           // collinear
    CHECK(all_nan(plane({0, 0, 0, 1, 0, 0, NAN, 1, 0})));                         // a NaN coordinate
    CHECK(all_nan(plane({0, 0, 0, 1, 0, 0, 0, INFINITY, 0})));                    // an infinite one
    CHECK(is(plane({0, 0, 0, FLT_MAX, 0, 0, 0, FLT_MAX, 0}), 0.0f, 0.0f, 1.0f, -0.0f)); // no finite f32 input overflows the doubles
    // a sign tie: n = (1, -1, 0) / sqrt 2 up to orientation; the FIRST of the two largest components decides, and is made positive
    const std::vector<float> t = plane({0, 0, 0, 1, 1, 0, 0, 0, 1}), u = plane({0, 0, 0, 0, 0, 1, 1, 1, 0});
    CHECK(t[0] > 0.0f && t[1] == -t[0] && t[2] == 0.0f && u[0] == t[0] && u[1] == t[1]);
    // every finite result is a unit normal to f32 precision and passes through a
    const std::vector<float> g = plane({0.5f, -1.25f, 2.0f, 1.5f, 0.75f, -0.5f, -2.0f, 0.25f, 1.0f});
    const double len = std::sqrt((double)g[0] * g[0] + (double)g[1] * g[1] + (double)g[2] * g[2]);
    CHECK(std::fabs(len - 1.0) < 1e-6 && std::fabs(g[0] * 0.5 + g[1] * -1.25 + g[2] * 2.0 + g[3]) < 1e-6);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        self_check();
        planes_check();
        if (failures) return 1;
        printf("consensus_check ok\n");
        return 0;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    unsigned long long n = 0;
    unsigned h = 0, kind = 0, lob = 0, hib = 0;
    if (fscanf(f, "%llu %u %u %x %x", &n, &h, &kind, &lob, &hib) != 5) { fclose(f); printf("bad header\n"); return 2; }
    Scene s;
    for (unsigned long long i = 0; i < n; ++i) {
        unsigned b[3] = {0, 0, 0};
        if (fscanf(f, "%x %x %x", &b[0], &b[1], &b[2]) != 3) { fclose(f); printf("bad row %llu\n", i); return 2; }
        s.x.push_back(f32_of(b[0])); s.y.push_back(f32_of(b[1])); s.z.push_back(f32_of(b[2]));
    }
    std::vector<float> p;
    for (unsigned j = 0; j < h; ++j) {
        unsigned b[4] = {0, 0, 0, 0};
        if (fscanf(f, "%x %x %x %x", &b[0], &b[1], &b[2], &b[3]) != 4) { fclose(f); printf("bad hypothesis %u\n", j); return 2; }
        for (int a = 0; a < 4; ++a) p.push_back(f32_of(b[a]));
    }
    fclose(f);
    const Counts a = run(s, kind, p, 0u, 0u, f32_of(lob), f32_of(hib), false), c = run(s, kind, p, 0u, 0u, f32_of(lob), f32_of(hib), true);
    if (a.matched != c.matched || a.c != c.c) { printf("the two orders differ\n"); return 1; }
    printf("matched %" PRIu64 "\n", a.matched);
    for (unsigned j = 0; j < h; ++j) printf("%" PRIu64 "\n", a.c[j]);
    return 0;
}
