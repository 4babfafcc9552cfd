// tools/surface_check -- gs_surface_math.h on its own, for a host compiler with sanitizers (tests/test_surface.py builds it with
// -fsanitize=address,undefined and runs it as its own process).
//
//   surface_check [FILE RADIUS]   FILE: n raw positions (x y z f32 each); prints one line of ten decimal i64 per position: its sums as
//                                 surface_host returns them, every splat a source and a query.
// Without arguments it runs sf_check and surface_host on scenes of its own -- NaN, infinities, denormals and -0.0 among the
// coordinates, exact duplicates, neighbours exactly on the radius, points on a plane and on a line -- in arrays of exactly n
// positions, states, normals, eigenvalues, counts and sums, so that a read or a write at or past the end is the sanitizer's to catch,
// at the lengths 0, 1, 2, 3, 4, 5, 63, 64, 65 and 300, at radii on both sides of a change of the exponent, with and without filters,
// with and without the orientation.  It checks what does not need a second implementation: every |q| is within the header's bound
// (through M_aa <= count (2^16 + 1)^2), the sums of a query equal a second pass in another order, counts are symmetric when every
// splat is a source and a query, count < 3 and non-queries read the NaN bits, eigenvalues are finite, ordered and not negative,
// normals have unit length and their largest component positive, an oriented normal differs from the plain one by its sign only and
// faces the point, the features are in their ranges, and every refusal names its number.  Then it prints "surface_check ok".
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "gs_surface_math.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static uint32_t bits_of(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }

static gs_surface query(float radius, uint32_t flags = 0, uint32_t sm = 0, uint32_t sv = 0, uint32_t qm = 0, uint32_t qv = 0) {
    gs_surface q{};
    q.struct_size = sizeof(gs_surface);
    q.radius = radius; q.flags = flags;
    q.src_mask = sm; q.src_value = sv; q.qry_mask = qm; q.qry_value = qv;
    q.toward[0] = 0.5f; q.toward[1] = -2.0f; q.toward[2] = 7.0f;
    return q;
}

struct Scene {
    std::vector<float> pos;
    std::vector<uint8_t> state;
};
static Scene own_scene(uint32_t n, int shape) { // shape 0: a cloud, 1: a plane with noise, 2: a line
    Scene s;
    s.pos.assign((size_t)n * 3, 0.0f);
    s.state.assign(n, 0);
    uint32_t w = 2463534242u;
    auto rnd = [&](float lo, float hi) { w = w * 1664525u + 1013904223u; return lo + (hi - lo) * (float)(w >> 8) / 16777216.0f; };
    for (uint32_t i = 0; i < n; ++i) {
        float* p = &s.pos[(size_t)i * 3];
        const float a = rnd(0.0f, 1.0f), b = rnd(0.0f, 1.0f), c = rnd(0.0f, 1.0f);
        if (shape == 0) { p[0] = a; p[1] = b; p[2] = c; }
        else if (shape == 1) { p[0] = a; p[1] = b; p[2] = 0.5f * a - 0.25f * b + 0.001f * c; }
        else { p[0] = a; p[1] = 2.0f * a; p[2] = -a; }
        s.state[i] = (uint8_t)(i % 3u);
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    if (n > 40) {
        s.pos[3 * 5] = nan; s.pos[3 * 7 + 1] = inf; s.pos[3 * 9 + 2] = -inf; s.pos[3 * 11] = -0.0f; s.pos[3 * 13 + 1] = 1e-45f;
        for (int k = 0; k < 3; ++k) s.pos[3 * 21 + k] = s.pos[3 * 20 + k]; // duplicates
        for (int k = 0; k < 3; ++k) s.pos[3 * 31 + k] = s.pos[3 * 30 + k] + (k == 0 ? 0.25f : 0.0f); // exactly on the radius 0.25 (a + 0.25 may round: then just near it)
    }
    return s;
}

static void run(const Scene& s, uint32_t n, float radius, uint32_t flags, bool filtered) {
    gs_surface q = filtered ? query(radius, flags, 3, 1, 3, 2) : query(radius, flags);
    SfScale sc;
    char why[160];
    CHECK(sf_check(&q, &sc, why, sizeof why));
    std::vector<float> nrm((size_t)n * 3), eig((size_t)n * 3), nrm0((size_t)n * 3), eig0((size_t)n * 3);
    std::vector<uint32_t> count(n), count0(n);
    std::vector<int64_t> sums((size_t)n * SF_SUM_WORDS);
    gs_surface_info info, info0;
    surface_host(s.pos.data(), s.state.data(), n, &q, sc, nrm.data(), eig.data(), count.data(), sums.data(), &info);
    gs_surface plain = q;
    plain.flags = 0;
    surface_host(s.pos.data(), s.state.data(), n, &plain, sc, nrm0.data(), eig0.data(), count0.data(), nullptr, &info0); // (sums may be null)
    CHECK(info.queried == info0.queried && info.sources == info0.sources && info.unresolved == info0.unresolved && info.candidates == info0.candidates);
    const int64_t qmax = (1 << 16) + 1;
    uint64_t unresolved = 0, queried = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const int64_t* w = &sums[(size_t)i * SF_SUM_WORDS];
        const bool is_q = !filtered || (s.state[i] & 3u) == 2u;
        queried += is_q ? 1u : 0u;
        CHECK(w[0] == (int64_t)count[i] && count[i] == count0[i]);
        if (!is_q) {
            for (uint32_t k = 0; k < SF_SUM_WORDS; ++k) CHECK(w[k] == 0);
        }
        CHECK(w[4] >= 0 && w[7] >= 0 && w[9] >= 0);
        CHECK(w[4] <= w[0] * qmax * qmax && w[7] <= w[0] * qmax * qmax && w[9] <= w[0] * qmax * qmax);
        for (int a = 0; a < 3; ++a) CHECK(w[1 + a] <= w[0] * qmax && w[1 + a] >= -w[0] * qmax);
        // a second pass in descending order: the same integers
        if (is_q && neigh_finite(s.pos[3 * i], s.pos[3 * i + 1], s.pos[3 * i + 2])) {
            SfSums a{};
            for (uint32_t j = n; j-- > 0;) {
                if (j == i || (filtered && (s.state[j] & 3u) != 1u)) continue;
                const float dx = s.pos[3 * j] - s.pos[3 * i], dy = s.pos[3 * j + 1] - s.pos[3 * i + 1], dz = s.pos[3 * j + 2] - s.pos[3 * i + 2];
                if (!((dx * dx + dy * dy) + dz * dz <= sc.r2)) continue;
                const int32_t qx = sf_quant(dx, sc.s), qy = sf_quant(dy, sc.s), qz = sf_quant(dz, sc.s);
                CHECK(std::llabs((long long)qx) <= qmax && std::llabs((long long)qy) <= qmax && std::llabs((long long)qz) <= qmax);
                sf_add(a, 1u, qx, qy, qz);
            }
            CHECK((int64_t)a.n == w[0] && a.S[0] == w[1] && a.S[1] == w[2] && a.S[2] == w[3]);
            for (int k = 0; k < 6; ++k) CHECK(a.M[k] == w[4 + k]);
        }
        const float* nv = &nrm[(size_t)i * 3];
        const float* ev = &eig[(size_t)i * 3];
        if (!is_q || count[i] < 3u) {
            for (int k = 0; k < 3; ++k) CHECK(bits_of(nv[k]) == SF_NAN_BITS && bits_of(ev[k]) == SF_NAN_BITS);
            unresolved += is_q ? 1u : 0u;
            continue;
        }
        CHECK(std::isfinite(ev[0]) && ev[0] >= ev[1] && ev[1] >= ev[2] && ev[2] >= 0.0f);
        const double len = std::sqrt((double)nv[0] * nv[0] + (double)nv[1] * nv[1] + (double)nv[2] * nv[2]);
        CHECK(std::fabs(len - 1.0) < 1e-6);
        const float* n0 = &nrm0[(size_t)i * 3];
        int big = 0;
        if (std::fabs(n0[1]) > std::fabs(n0[big])) big = 1;
        if (std::fabs(n0[2]) > std::fabs(n0[big])) big = 2;
        CHECK(n0[big] > 0.0f);
        for (int k = 0; k < 3; ++k) CHECK(bits_of(ev[k]) == bits_of(eig0[(size_t)i * 3 + k]));
        if (flags & GS_SURFACE_ORIENT) {
            const bool same = nv[0] == n0[0] && nv[1] == n0[1] && nv[2] == n0[2], neg = nv[0] == -n0[0] && nv[1] == -n0[1] && nv[2] == -n0[2];
            CHECK(same || neg);
            const float ex = q.toward[0] - s.pos[3 * i], ey = q.toward[1] - s.pos[3 * i + 1], ez = q.toward[2] - s.pos[3 * i + 2];
            CHECK(!((nv[0] * ex + nv[1] * ey) + nv[2] * ez < 0.0f));
        } else {
            for (int k = 0; k < 3; ++k) CHECK(bits_of(nv[k]) == bits_of(n0[k]));
        }
        const float axis[3] = {0.0f, 0.6f, -0.8f};
        const float var = sf_feature(GS_SURFACE_VARIATION, nv, ev, count[i], axis), pla = sf_feature(GS_SURFACE_PLANARITY, nv, ev, count[i], axis),
                    lin = sf_feature(GS_SURFACE_LINEARITY, nv, ev, count[i], axis), sph = sf_feature(GS_SURFACE_SPHERICITY, nv, ev, count[i], axis),
                    fac = sf_feature(GS_SURFACE_FACING, nv, ev, count[i], axis), sig = sf_feature(GS_SURFACE_FACING_SIGNED, nv, ev, count[i], axis);
        if (ev[0] > 0.0f) {
            CHECK(var >= 0.0f && var <= 0.3334f && pla >= 0.0f && pla <= 1.0f && lin >= 0.0f && lin <= 1.0f && sph >= 0.0f && sph <= 1.0f);
        } else {
            CHECK(var != var && pla != pla); // 0 / 0: in no range
            CHECK(!sf_member(var, -INFINITY, INFINITY, true) && sf_member(var, -INFINITY, INFINITY, false));
        }
        CHECK(fac >= 0.0f && fac <= 1.000001f && std::fabs(sig) == fac);
        CHECK(sf_feature(GS_SURFACE_COUNT, nv, ev, count[i], axis) == (float)count[i]);
    }
    CHECK(unresolved == info.unresolved && queried == info.queried);
    if (!filtered) { // every splat a source and a query: acceptance is symmetric, so the counts add up to an even number
        uint64_t total = 0;
        for (uint32_t i = 0; i < n; ++i) total += count[i];
        CHECK(total % 2u == 0u);
    }
}

static void refusals() {
    SfScale sc;
    char why[160];
    auto refused = [&](gs_surface q, const char* fragment) {
        why[0] = 0;
        CHECK(!sf_check(&q, &sc, why, sizeof why));
        CHECK(strstr(why, fragment) != nullptr);
    };
    CHECK(!sf_check(nullptr, &sc, why, sizeof why) && strstr(why, "null query"));
    gs_surface q = query(0.5f);
    q.struct_size = 48;
    refused(q, "struct_size 48");
    refused(query(std::numeric_limits<float>::quiet_NaN()), "radius nan");
    refused(query(std::numeric_limits<float>::infinity()), "radius inf");
    refused(query(-0.5f), "radius -0.5");
    refused(query(0.0f), "not above 0");
    refused(query(2e19f), "squared");
    refused(query(1e-36f), "2^135");
    refused(query(1e-45f), "2^");
    refused(query(0.5f, 4u), "flags 0x4");
    q = query(0.5f);
    q.reserved = 5;
    refused(q, "reserved 5");
    // the scale on both sides of a change of the exponent
    const float below = std::nextafterf(0.25f, 0.0f), above = std::nextafterf(1.0f, 2.0f);
    q = query(0.25f); CHECK(sf_check(&q, &sc, why, sizeof why) && sc.e == -1 && sc.s == 131072.0f && sc.r2 == 0.0625f);
    q = query(below); CHECK(sf_check(&q, &sc, why, sizeof why) && sc.e == -2 && sc.s == 262144.0f);
    q = query(1.0f); CHECK(sf_check(&q, &sc, why, sizeof why) && sc.e == 1 && sc.s == 32768.0f && sc.unscale == std::ldexp(1.0, -30));
    q = query(above); CHECK(sf_check(&q, &sc, why, sizeof why) && sc.e == 1 && sc.s == 32768.0f);
    q = query(std::ldexp(1.0f, -112)); CHECK(sf_check(&q, &sc, why, sizeof why) && sc.e == -111 && sc.s == std::ldexp(1.0f, 127)); // the smallest radius taken
    CHECK(sf_quant(0.25f, 131072.0f) == 32768 && sf_quant(below, 262144.0f) == 65536 && sf_quant(-2.5f, 1.0f) == -2 && sf_quant(3.5f, 1.0f) == 4); // half to even
}

int main(int argc, char** argv) {
    if (argc == 3) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
        std::vector<float> pos;
        float buf[3];
        while (fread(buf, 4, 3, f) == 3) pos.insert(pos.end(), buf, buf + 3);
        fclose(f);
        const uint64_t n = pos.size() / 3;
        gs_surface q = query((float)atof(argv[2]));
        SfScale sc;
        char why[160];
        if (!sf_check(&q, &sc, why, sizeof why)) { printf("%s\n", why); return 2; }
        std::vector<float> nrm(n * 3), eig(n * 3);
        std::vector<uint32_t> count(n);
        std::vector<int64_t> sums(n * SF_SUM_WORDS);
        gs_surface_info info;
        surface_host(pos.data(), nullptr, n, &q, sc, nrm.data(), eig.data(), count.data(), sums.data(), &info);
        for (uint64_t i = 0; i < n; ++i) {
            for (uint32_t k = 0; k < SF_SUM_WORDS; ++k) printf("%" PRId64 "%c", sums[i * SF_SUM_WORDS + k], k + 1 == SF_SUM_WORDS ? '\n' : ' ');
        }
        return 0;
    }
    refusals();
    const uint32_t lengths[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 300};
    const float radii[] = {0.25f, std::nextafterf(0.25f, 0.0f), 1.0f, std::nextafterf(1.0f, 2.0f), 0.05f, 1e-30f, 1e3f};
    for (uint32_t n : lengths)
        for (int shape = 0; shape < 3; ++shape) {
            const Scene s = own_scene(n, shape);
            for (float radius : radii)
                for (uint32_t flags : {0u, (uint32_t)GS_SURFACE_ORIENT, (uint32_t)(GS_SURFACE_ORIENT | GS_SURFACE_KEEP_SUMS)})
                    for (bool filtered : {false, true}) run(s, n, radius, flags, filtered);
        }
    if (failures) { printf("surface_check: %d checks failed\n", failures); return 1; }
    printf("surface_check ok\n");
    return 0;
}
