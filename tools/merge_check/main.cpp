// tools/merge_check -- gs_merge_math.h on its own, for a host compiler with sanitizers (tests/test_simplify.py builds it with
// -fsanitize=address,undefined and runs it as its own process).
//
//   merge_check [FILE CELL]   FILE: n raw 320-byte records; CELL: the edge.  Prints "eligible E groups G members M largest L cells X Y Z"
//                             and then one line of 64 hexadecimal u64 words per merged group: its sums as merge_host returns them, with
//                             the filter (0, 0) and min_members 2.
// Without arguments it runs merge_host on scenes of its own -- NaN, infinities, denormals and -0.0 among the coordinates, zero
// quaternions, infinite and NaN scales and logits, exact duplicates, members on cell faces, in arrays of exactly n records, n sums and n
// group numbers so that a read or a write at or past the end is the sanitizer's to catch -- at the lengths 0, 1, 2, 3, 5, 63, 64, 65,
// 257, 1023 and 1025, with edges that give one cell, many cells and the 1024-cell clamp, with and without a filter and an op, in the
// count-only mode, with a capacity one short and with max_members at and below the fullest cell.  It checks what does not need a second
// implementation: the counts add up, group numbers are dense and ascending in first member, the members of a group are the splats that
// name it, every sum's bookkeeping slots hold the group's length, first member and its position, marked splats are exactly the members,
// the records are finite with zero padding, sorted scales, a unit quaternion with r >= 0 and an opacity of at most 0.99, and k copies
// of a splat come back as that splat.  Then it prints "merge_check ok".
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "gs_merge_math.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static float f32_of(uint32_t b) { float v; memcpy(&v, &b, 4); return v; }

static gs_merge params(float cell, uint32_t mask, uint32_t value, uint32_t op, uint32_t bits, uint32_t max_members = 0) {
    gs_merge p{};
    p.struct_size = sizeof(gs_merge);
    p.mask = mask; p.value = value; p.cell = cell; p.min_members = 2; p.max_members = max_members; p.op = op; p.bits = bits;
    return p;
}

struct Scene {
    std::vector<float> rec;
    std::vector<uint8_t> state;
};
static Scene own_scene(uint32_t n) {
    Scene s;
    s.rec.assign((size_t)n * 80, 0.0f);
    uint32_t w = 2463534242u;
    auto rnd = [&](float lo, float hi) { w = w * 1664525u + 1013904223u; return lo + (hi - lo) * (float)(w >> 8) / 16777216.0f; };
    for (uint32_t i = 0; i < n; ++i) {
        float* r = s.rec.data() + (size_t)i * 80;
        for (int a = 0; a < 3; ++a) r[a] = rnd(0.0f, 8.0f);
        for (int a = 0; a < 3; ++a) r[4 + a] = rnd(-5.0f, -1.0f);
        for (int a = 0; a < 4; ++a) r[8 + a] = rnd(-1.0f, 1.0f);
        r[12] = rnd(-4.0f, 4.0f);
        for (int k = 0; k < 16; ++k)
            for (int ch = 0; ch < 3; ++ch) r[16 + 4 * k + ch] = rnd(-1.0f, 1.0f);
        r[3] = r[7] = r[13] = 123.0f; // padding junk that must not come back
        if (i % 37u == 5u) r[i % 3u] = std::numeric_limits<float>::quiet_NaN();
        if (i % 41u == 7u) r[(i + 1u) % 3u] = (i & 1u) ? INFINITY : -INFINITY;
        if (i % 43u == 9u) r[i % 3u] = (i & 1u) ? -0.0f : f32_of(1u);
        if (i % 47u == 11u) r[8] = r[9] = r[10] = r[11] = 0.0f;
        if (i % 53u == 13u) r[4 + i % 3u] = (i & 1u) ? INFINITY : std::numeric_limits<float>::quiet_NaN();
        if (i % 59u == 17u) r[12] = (i & 1u) ? -200.0f : std::numeric_limits<float>::quiet_NaN();
        if (i % 10u == 5u) memcpy(r, r - 80, 320);                    // an exact duplicate of its predecessor
        if (i % 16u == 3u) r[0] = 2.0f;                               // on a face of the edge-0.5 grid (when the bounds start at 0)
        s.state.push_back((uint8_t)((i * 7u) & 0x73u) | (i % 3u == 0u ? 0x04u : 0u));
    }
    return s;
}

static void check_merge(const Scene& s, uint32_t n, float cell, uint32_t mask, uint32_t value, uint32_t op) {
    const gs_merge p = params(cell, mask, value, op, op ? 0x80u : 0u);
    std::vector<uint8_t> st = s.state;
    gs_merge_info count{};
    CHECK(merge_host(s.rec.data(), st.data(), n, &p, nullptr, 0, nullptr, nullptr, &count) == 0);
    CHECK(st == s.state);
    const size_t G = (size_t)count.groups;
    CHECK(count.members >= 2 * count.groups && count.members <= count.eligible && count.eligible <= n && count.largest <= count.eligible);
    if (G > 0) { // one short: nothing written
        std::vector<float> few((G - 1) * 80 + 1, -7.0f);
        gs_merge_info i2{};
        CHECK(merge_host(s.rec.data(), st.data(), n, &p, few.data(), G - 1, nullptr, nullptr, &i2) == 2);
        CHECK(st == s.state && few[0] == -7.0f && i2.groups == count.groups);
    }
    std::vector<float> out(G * 80);
    std::vector<double> sums(G * 64);
    std::vector<uint32_t> gof(n);
    gs_merge_info info{};
    float dummy = 0.0f;
    CHECK(merge_host(s.rec.data(), st.data(), n, &p, G ? out.data() : &dummy, G, sums.data(), gof.data(), &info) == 0);
    CHECK(info.groups == count.groups && info.members == count.members && info.eligible == count.eligible && info.largest == count.largest);
    std::vector<uint32_t> len(G, 0), first(G, 0xFFFFFFFFu);
    uint64_t members = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const bool in = gof[i] != GS_MERGE_NONE;
        CHECK(!in || gof[i] < G);
        if (in && gof[i] < G) { ++len[gof[i]]; ++members; if (first[gof[i]] == 0xFFFFFFFFu) first[gof[i]] = i; }
        const uint8_t want = (uint8_t)(in && op ? (s.state[i] | 0x80u) : s.state[i]);
        CHECK(st[i] == want);
        if (in) CHECK((mask | value) == 0u || (s.state[i] & mask) == value);
    }
    CHECK(members == info.members);
    uint32_t largest = 0;
    for (size_t g = 0; g < G; ++g) {
        const double* a = sums.data() + g * 64;
        const float* r = out.data() + g * 80;
        CHECK(len[g] >= 2u && a[58] == (double)len[g] && a[59] == (double)first[g] && a[63] == 0.0 && a[0] > 0.0);
        for (int k = 0; k < 3; ++k) CHECK(a[60 + k] == (double)s.rec[(size_t)first[g] * 80 + k]);
        largest = len[g] > largest ? len[g] : largest;
        for (int k = 0; k < 80; ++k) CHECK(std::isfinite(r[k]));
        CHECK(r[3] == 0.0f && r[7] == 0.0f && r[13] == 0.0f && r[14] == 0.0f && r[15] == 0.0f && r[19] == 0.0f && r[79] == 0.0f);
        CHECK(r[4] >= r[5] && r[5] >= r[6] && r[8] >= 0.0f);
        const double qn = std::sqrt((double)r[8] * r[8] + (double)r[9] * r[9] + (double)r[10] * r[10] + (double)r[11] * r[11]);
        CHECK(std::fabs(qn - 1.0) < 1e-6);
        CHECK(1.0 / (1.0 + std::exp(-(double)r[12])) <= 0.99 + 1e-6);
    }
    CHECK(largest <= info.largest);
    if (info.largest >= 3) { // max_members at the fullest cell is accepted, one below is refused before anything is written
        gs_merge q = params(cell, mask, value, op, op ? 0x80u : 0u, (uint32_t)info.largest);
        std::vector<uint8_t> st2 = s.state;
        gs_merge_info i3{};
        CHECK(merge_host(s.rec.data(), st2.data(), n, &q, G ? out.data() : &dummy, G, nullptr, nullptr, &i3) == 0);
        q.max_members = (uint32_t)info.largest - 1u;
        st2 = s.state;
        std::vector<uint32_t> gof2(n, 5u);
        CHECK(merge_host(s.rec.data(), st2.data(), n, &q, G ? out.data() : &dummy, G, nullptr, gof2.data(), &i3) == 1);
        CHECK(st2 == s.state && i3.largest == info.largest);
        for (uint32_t i = 0; i < n; ++i) CHECK(gof2[i] == 5u);
    }
}

static void copies_check() {
    const Scene s = own_scene(4);
    for (uint32_t k : {2u, 3u, 200u}) {
        std::vector<float> rec((size_t)k * 80);
        for (uint32_t i = 0; i < k; ++i) memcpy(rec.data() + (size_t)i * 80, s.rec.data(), 320);
        rec.shrink_to_fit();
        const gs_merge p = params(0.5f, 0, 0, 0, 0);
        gs_merge_info info{};
        float out[80];
        double sums[64];
        std::vector<uint32_t> gof(k);
        CHECK(merge_host(rec.data(), nullptr, k, &p, out, 1, sums, gof.data(), &info) == 0);
        CHECK(info.groups == 1 && info.members == k && info.largest == k);
        for (int a = 0; a < 3; ++a) CHECK(out[a] == rec[a]);
        const double a1 = 1.0 / (1.0 + std::exp(-(double)rec[12])), want = std::fmin(0.99, k * a1), got = 1.0 / (1.0 + std::exp(-(double)out[12]));
        CHECK(std::fabs(got - want) <= 1e-5 * want);
        for (int j = 0; j < 48; ++j) CHECK(std::fabs(out[16 + 4 * (j / 3) + j % 3] - rec[16 + 4 * (j / 3) + j % 3]) <= 1e-6f);
    }
}

int main(int argc, char** argv) {
    if (argc < 3) {
        const uint32_t lengths[11] = {0u, 1u, 2u, 3u, 5u, 63u, 64u, 65u, 257u, 1023u, 1025u};
        const float cells[3] = {1.0e4f, 0.5f, 1.0e-6f};
        for (uint32_t n : lengths) {
            const Scene s = own_scene(n);
            for (float cell : cells)
                for (int f = 0; f < 2; ++f)
                    for (uint32_t op : {0u, 1u}) check_merge(s, n, cell, f ? 0x04u : 0u, f ? 0x04u : 0u, op);
        }
        copies_check();
        if (failures) return 1;
        printf("merge_check ok\n");
        return 0;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<float> rec;
    float buf[80];
    while (fread(buf, 320, 1, f) == 1) rec.insert(rec.end(), buf, buf + 80);
    fclose(f);
    rec.shrink_to_fit();
    const uint64_t n = rec.size() / 80;
    const gs_merge p = params(strtof(argv[2], nullptr), 0, 0, 0, 0);
    gs_merge_info info{};
    if (merge_host(rec.data(), nullptr, n, &p, nullptr, 0, nullptr, nullptr, &info) != 0) { printf("refused\n"); return 1; }
    std::vector<float> out((size_t)info.groups * 80 + 1);
    std::vector<double> sums((size_t)info.groups * 64 + 1);
    if (merge_host(rec.data(), nullptr, n, &p, out.data(), info.groups, sums.data(), nullptr, &info) != 0) { printf("refused\n"); return 1; }
    printf("eligible %" PRIu64 " groups %" PRIu64 " members %" PRIu64 " largest %" PRIu64 " cells %u %u %u\n", info.eligible, info.groups, info.members,
           info.largest, info.cells[0], info.cells[1], info.cells[2]);
    for (uint64_t g = 0; g < info.groups; ++g) {
        for (int k = 0; k < 64; ++k) {
            uint64_t b;
            memcpy(&b, &sums[(size_t)g * 64 + k], 8);
            printf("%" PRIx64 "%c", b, k == 63 ? '\n' : ' ');
        }
    }
    return 0;
}
