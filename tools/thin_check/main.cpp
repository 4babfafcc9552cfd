// tools/thin_check -- gs_thin_math.h on its own, for a host compiler with sanitizers (tests/test_thin.py builds it with
// -fsanitize=address,undefined and runs it as its own process).
//
//   thin_check [FILE RADIUS FLAGS SEED]   FILE: n raw positions (x y z f32 each); prints one line "keeper covers" per position, the
//                                         planes thin_host returns with every splat a member and no priority.
// Without arguments it runs thin_host on scenes of its own -- NaN, infinities, denormals and -0.0 among the coordinates, exact
// duplicates, neighbours exactly on the radius -- in arrays of exactly n positions, states, priorities, keepers and covers, so that a
// read or a write at or past the end is the sanitizer's to catch, at the lengths 0, 1, 2, 3, 4, 5, 63, 64, 65 and 300, at the radii 0,
// 1e-30, 0.05, 0.25 and 100, in the hash and the index order, with and without a priority (ties and NaNs in it), ascending, with and
// without a filter.  It checks what does not need a second implementation: the kept members are independent (no two linked), the set
// is maximal (every dropped member's keeper is kept and linked to it), no linked kept member outranks a dropped member's keeper,
// every kept member that is linked to a dropped one ranks below its keeper or is it, non-members read NONE / 0, non-finite members
// are their own keepers with covers 1, covers counts the keepers and sums to the members, the info numbers are the planes', the hash
// is a bijection on 2^20 indices, and every refusal names its number.  Then it prints "thin_check ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "gs_thin_math.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static gs_thin query(float radius, uint32_t flags = 0, uint32_t seed = 0, uint32_t mask = 0, uint32_t value = 0) {
    gs_thin q;
    memset(&q, 0, sizeof(q));
    q.struct_size = sizeof(gs_thin);
    q.radius = radius; q.flags = flags; q.seed = seed; q.mask = mask; q.value = value;
    q.priority.struct_size = sizeof(gs_attr);
    q.priority.kind = GS_THIN_NO_PRIORITY;
    return q;
}

struct Scene {
    std::vector<float> x, y, z, prio;
    std::vector<uint8_t> state;
};
static Scene own_scene(uint32_t n) {
    Scene s;
    s.x.assign(n, 0.0f); s.y.assign(n, 0.0f); s.z.assign(n, 0.0f); s.prio.assign(n, 0.0f);
    s.state.assign(n, 0);
    uint32_t w = 2463534242u;
    auto rnd = [&]() { w = w * 1664525u + 1013904223u; return (float)(w >> 8) / 16777216.0f; };
    for (uint32_t i = 0; i < n; ++i) {
        s.x[i] = rnd(); s.y[i] = rnd(); s.z[i] = 0.25f * rnd();
        s.prio[i] = (float)(i % 7u) - 3.0f; // ties
        s.state[i] = (uint8_t)(i % 3u);
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    if (n > 40) {
        s.x[5] = nan; s.y[7] = inf; s.z[9] = -inf; s.x[11] = -0.0f; s.y[13] = 1e-45f;
        s.x[21] = s.x[20]; s.y[21] = s.y[20]; s.z[21] = s.z[20];                     // duplicates
        s.x[22] = s.x[20]; s.y[22] = s.y[20]; s.z[22] = s.z[20];
        s.x[30] = 0.5f; s.y[30] = 0.5f; s.z[30] = 0.125f;
        s.x[31] = 0.75f; s.y[31] = 0.5f; s.z[31] = 0.125f;                           // exactly on the radius 0.25
        s.prio[3] = nan; s.prio[4] = -nan; s.prio[6] = inf; s.prio[8] = -inf; s.prio[12] = -0.0f; s.prio[14] = 0.0f;
    }
    return s;
}

static bool linked(const Scene& s, uint32_t i, uint32_t j, float r2) {
    if (i == j || !neigh_finite(s.x[i], s.y[i], s.z[i]) || !neigh_finite(s.x[j], s.y[j], s.z[j])) return false;
    const float dx = s.x[j] - s.x[i], dy = s.y[j] - s.y[i], dz = s.z[j] - s.z[i];
    return (dx * dx + dy * dy) + dz * dz <= r2;
}

static void run(const Scene& s, uint32_t n, float radius, uint32_t flags, uint32_t seed, bool with_prio, bool filtered) {
    const gs_thin q = query(radius, flags, seed, filtered ? 3u : 0u, filtered ? 1u : 0u);
    // arrays of exactly n elements (data() of an empty vector may be null: n == 0 passes null arrays)
    std::vector<float> x(s.x.begin(), s.x.begin() + n), y(s.y.begin(), s.y.begin() + n), z(s.z.begin(), s.z.begin() + n), pr(s.prio.begin(), s.prio.begin() + n);
    std::vector<uint8_t> st(s.state.begin(), s.state.begin() + n);
    std::vector<uint32_t> keeper(n, 7u), covers(n, 7u);
    gs_thin_info info;
    char msg[160] = "";
    const float* prio = with_prio ? pr.data() : nullptr;
    static float none_f; static uint32_t none_u; // (n == 0 with a priority: a non-null pointer that is never read)
    const int rc = thin_host(x.data(), y.data(), z.data(), n, filtered ? st.data() : nullptr, with_prio && !n ? &none_f : prio, &q,
                             n ? keeper.data() : &none_u, n ? covers.data() : &none_u, &info, msg, sizeof(msg));
    CHECK(rc == 0);
    if (rc != 0) { printf("refused: %s\n", msg); return; }
    const float r2 = radius * radius;
    Scene v; v.x = x; v.y = y; v.z = z;
    std::vector<uint64_t> R(n);
    std::vector<uint32_t> count(n, 0u);
    uint64_t members = 0, kept = 0, largest = 0, sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t b = 0; if (with_prio) memcpy(&b, &pr[i], 4);
        R[i] = thin_rank(i, with_prio, b, flags, seed);
    }
    for (uint32_t i = 0; i < n; ++i) {
        const bool mem = !filtered || (st[i] & 3u) == 1u;
        if (!mem) { CHECK(keeper[i] == GS_THIN_NONE && covers[i] == 0u); continue; }
        ++members;
        CHECK(keeper[i] < n);
        if (keeper[i] >= n) continue;
        ++count[keeper[i]];
        if (!neigh_finite(x[i], y[i], z[i])) { CHECK(keeper[i] == i && covers[i] == 1u); }
        if (keeper[i] == i) { ++kept; CHECK(covers[i] >= 1u); }
        else {
            const uint32_t k = keeper[i];
            CHECK(covers[i] == 0u && keeper[k] == k && linked(v, i, k, r2) && thin_outranks(R[k], k, R[i], i));
        }
    }
    for (uint32_t i = 0; i < n; ++i) {
        const bool mem = !filtered || (st[i] & 3u) == 1u;
        if (!mem) continue;
        CHECK(covers[i] == (keeper[i] == i ? count[i] : 0u));
        sum += covers[i];
        largest = covers[i] > largest ? covers[i] : largest;
        for (uint32_t j = 0; j < n; ++j) {
            const bool memj = !filtered || (st[j] & 3u) == 1u;
            if (!memj || keeper[j] != j || !linked(v, i, j, r2)) continue;
            CHECK(keeper[i] != i);                                                        // independent
            if (keeper[i] != i && keeper[i] < n && j != keeper[i]) CHECK(thin_outranks(R[keeper[i]], keeper[i], R[j], j)); // the best of them
        }
    }
    CHECK(sum == members && info.members == members && info.kept == kept && info.dropped == members - kept && info.largest == largest);
    CHECK(info.rounds == 0u && info.cells[0] == 1u && info.cell_edge == 0.0f);
}

static void refusals() {
    float x[2] = {0, 1}, pr[2] = {0, 1};
    uint32_t k[2], c[2];
    char msg[160];
    auto refused = [&](gs_thin q, const float* prio, const char* what) {
        msg[0] = 0;
        k[0] = k[1] = c[0] = c[1] = 9u;
        const int rc = thin_host(x, x, x, 2, nullptr, prio, &q, k, c, nullptr, msg, sizeof(msg));
        CHECK(rc == 1 && strstr(msg, what) != nullptr && k[0] == 9u && c[1] == 9u);
        if (rc != 1 || !strstr(msg, what)) printf("  message: %s (wanted %s)\n", msg, what);
    };
    gs_thin q = query(0.5f);
    q.struct_size = 40; refused(q, nullptr, "struct_size 40");
    q = query(NAN); refused(q, nullptr, "radius nan");
    q = query(-0.5f); refused(q, nullptr, "radius -0.5");
    q = query(INFINITY); refused(q, nullptr, "radius inf");
    q = query(2e19f); refused(q, nullptr, "squared");
    q = query(0.5f, 4u); refused(q, nullptr, "unknown flags 0x4");
    q = query(0.5f, GS_THIN_ASCENDING); refused(q, nullptr, "GS_THIN_ASCENDING without a priority");
    q = query(0.5f); q.reserved0 = 5; refused(q, nullptr, "reserved0 = 5");
    q = query(0.5f); q.reserved[1] = 6; refused(q, pr, "reserved[1] = 6");
    q = query(0.5f, 0, 0, 0x100, 0); refused(q, nullptr, "0x100");
    q = query(0.5f, 0, 0, 0, 0x1FF); refused(q, nullptr, "0x1ff");
    msg[0] = 0;
    CHECK(thin_host(x, x, x, 2, nullptr, nullptr, nullptr, k, c, nullptr, msg, sizeof(msg)) == 1 && strstr(msg, "null query"));
    q = query(0.5f);
    CHECK(thin_host(nullptr, x, x, 2, nullptr, nullptr, &q, k, c, nullptr, msg, sizeof(msg)) == 1 && strstr(msg, "null array"));
    q = query(0.5f, GS_THIN_ASCENDING);
    CHECK(thin_host(x, x, x, 2, nullptr, pr, &q, k, c, nullptr, msg, sizeof(msg)) == 0 && k[0] == 0u && k[1] == 1u); // sqrt(3) apart: both kept
}

int main(int argc, char** argv) {
    if (argc == 5) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { printf("cannot open %s\n", argv[1]); return 1; }
        std::vector<float> raw;
        float buf[3];
        while (fread(buf, 4, 3, f) == 3) raw.insert(raw.end(), buf, buf + 3);
        fclose(f);
        const uint32_t n = (uint32_t)(raw.size() / 3);
        std::vector<float> x(n), y(n), z(n);
        for (uint32_t i = 0; i < n; ++i) { x[i] = raw[3 * i]; y[i] = raw[3 * i + 1]; z[i] = raw[3 * i + 2]; }
        std::vector<uint32_t> keeper(n), covers(n);
        const gs_thin q = query((float)atof(argv[2]), (uint32_t)strtoul(argv[3], nullptr, 0), (uint32_t)strtoul(argv[4], nullptr, 0));
        char msg[160];
        static uint32_t none_u;
        if (thin_host(x.data(), y.data(), z.data(), n, nullptr, nullptr, &q, n ? keeper.data() : &none_u, n ? covers.data() : &none_u, nullptr, msg,
                      sizeof(msg)) != 0) { printf("refused: %s\n", msg); return 1; }
        for (uint32_t i = 0; i < n; ++i) printf("%u %u\n", keeper[i], covers[i]);
        return 0;
    }
    const uint32_t lengths[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 300};
    const float radii[] = {0.0f, 1e-30f, 0.05f, 0.25f, 100.0f};
    const Scene s = own_scene(300);
    for (uint32_t n : lengths)
        for (float radius : radii)
            for (uint32_t order = 0; order < 3; ++order)
                for (int p = 0; p < 3; ++p)
                    for (int filtered = 0; filtered < 2; ++filtered)
                        run(s, n, radius, (order == 2 ? GS_THIN_ORDER_INDEX : 0u) | (p == 2 ? GS_THIN_ASCENDING : 0u), order == 1 ? 12345u : 0u, p != 0, filtered != 0);
    for (uint32_t seed : {0u, 12345u}) { // a bijection of 32-bit words: no two of 2^20 indices collide
        std::vector<uint32_t> h(1u << 20);
        for (uint32_t i = 0; i < (1u << 20); ++i) h[i] = thin_hash(i, seed);
        std::sort(h.begin(), h.end());
        CHECK(std::adjacent_find(h.begin(), h.end()) == h.end());
    }
    CHECK(thin_pkey(0x7FC00000u, false) == 0u && thin_pkey(0x7FC00000u, true) == 0u && thin_pkey(0xFFC00000u, true) == 0u && thin_pkey(0x7F800001u, false) == 0u);
    CHECK(thin_pkey(0x80000000u, false) < thin_pkey(0u, false) && thin_pkey(0x80000000u, true) > thin_pkey(0u, true)); // -0 < +0
    CHECK(thin_pkey(0xFF800000u, false) > 0u && thin_pkey(0x7F800000u, true) > 0u);                                    // an infinity still beats a NaN
    refusals();
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("thin_check ok\n");
    return 0;
}
