// grade_check -- gs_grade_compose's host mathematics and gs_grade_splats' refusals (csrc/gs_grade_math.hip) as a stand-alone program,
// meant to be built with -fsanitize=address,undefined (tests/test_colours.py does):
//   g++ -std=c++17 -fsanitize=address,undefined -I gaussian-splatting-wgpu_amd/csrc tools/grade_check/main.cpp \
//       -x c++ gaussian-splatting-wgpu_amd/csrc/gs_grade_math.hip -o grade_check && ./grade_check
// Over a few hundred seeded parameter sets it checks what a grade must do to a displayed colour -- a grey (v, v, v) goes to
// gain_c ((v - black) / (white - black)) + offset_c whatever the saturation, the luma of Sat(t) C is the luma of C, the band-0
// offset is (A h + o - h) / SH_C0 --, the flag rules, and that the refusals of both calls refuse without writing.  Exit status 0
// and "grade_check ok" when everything holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "gs_grade_math.h"

static int g_bad = 0;
#define EXPECT(cond, ...)                  \
    do {                                   \
        if (!(cond)) {                     \
            if (++g_bad <= 20) {           \
                printf("FAIL %s: ", #cond); \
                printf(__VA_ARGS__);       \
                printf("\n");              \
            }                              \
        }                                  \
    } while (0)

static const double kShC0 = 0.28209479177387814;
static const double kLuma[3] = {0.2126, 0.7152, 0.0722};

static void check_one(const float* gain, const float* offset, float sat, float black, float white, float og) {
    gs_grade x;
    char err[256] = "";
    const int32_t rc = gs_grade_compose_host(gain, offset, sat, black, white, og, &x, err, sizeof(err));
    EXPECT(rc == GS_OK, "rc %d (%s)", rc, err);
    if (rc != GS_OK) return;
    EXPECT(x.struct_size == sizeof(gs_grade) && sizeof(gs_grade) == 64, "struct_size %u", x.struct_size);
    EXPECT(x.reserved == 0.0f, "reserved %g", (double)x.reserved);
    const double s = 1.0 / ((double)white - (double)black);
    double scale = 1.0; // the magnitude the tolerances are relative to
    for (int k = 0; k < 9; ++k) scale = std::fmax(scale, std::fabs((double)x.a[k]));
    for (int c = 0; c < 3; ++c) {
        const double g = gain ? gain[c] : 1.0, off = offset ? offset[c] : 0.0;
        scale = std::fmax(scale, std::fabs(off) + std::fabs(g * black * s));
        // a grey v: A (v, v, v) + o = g (v - black) s + off, for v = 1/2 read off dc
        const double row = (double)x.a[3 * c] + x.a[3 * c + 1] + x.a[3 * c + 2];
        EXPECT(std::fabs(row - g * s) <= 1e-6 * scale, "row %d sums to %.9g, gain / (white - black) = %.9g", c, row, g * s);
        const double want = (g * (0.5 - black) * s + off - 0.5) / kShC0;
        EXPECT(std::fabs((double)x.dc[c] - want) <= 1e-6 * scale / kShC0, "dc[%d] %.9g vs %.9g", c, (double)x.dc[c], want);
    }
    // luma is kept by the saturation: w^T (diag(1/g) A) = s w^T  (where no gain is 0)
    bool gains = true;
    for (int c = 0; c < 3; ++c) gains = gains && (!gain || std::fabs(gain[c]) > 0.05f);
    if (gains)
        for (int j = 0; j < 3; ++j) {
            double v = 0.0;
            for (int c = 0; c < 3; ++c) v += kLuma[c] * (double)x.a[3 * c + j] / (gain ? gain[c] : 1.0);
            EXPECT(std::fabs(v - s * kLuma[j]) <= 2e-5 * scale, "luma column %d: %.9g vs %.9g", j, v, s * kLuma[j]);
        }
    EXPECT(std::fabs((double)x.opacity_logit - std::log((double)og)) <= 1e-6 * (1.0 + std::fabs(std::log((double)og))), "logit %.9g", (double)x.opacity_logit);
    bool identity = true, zero = true;
    for (int k = 0; k < 9; ++k) identity = identity && x.a[k] == (k % 4 == 0 ? 1.0f : 0.0f);
    for (int c = 0; c < 3; ++c) zero = zero && x.dc[c] == 0.0f;
    const uint32_t want = (identity ? 0u : GS_GRADE_MATRIX) | (zero ? 0u : GS_GRADE_OFFSET) | (og == 1.0f ? 0u : GS_GRADE_OPACITY);
    EXPECT(x.flags == want, "flags %u, want %u", x.flags, want);
    EXPECT(gs_grade_validate_host(&x, err, sizeof(err)) == GS_OK, "a composed grade is refused: %s", err);
}

int main() {
    std::mt19937 rng(20241019u);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    int cases = 0;
    for (int k = 0; k < 400; ++k) {
        float gain[3], off[3];
        for (float& v : gain) v = (k % 7 == 0 ? -1.0f : 0.1f) + 2.0f * uni(rng);
        for (float& v : off) v = 0.4f * uni(rng) - 0.2f;
        const float sat = k % 5 == 0 ? 1.0f : 2.0f * uni(rng);
        const float black = k % 3 == 0 ? 0.0f : 0.3f * uni(rng) - 0.1f;
        const float white = k % 4 == 0 ? 1.0f : 0.5f + uni(rng);
        const float og = k % 6 == 0 ? 1.0f : std::exp(6.0f * uni(rng) - 3.0f);
        check_one((k & 1) ? gain : nullptr, (k & 2) ? off : nullptr, sat, black, white, og);
        ++cases;
    }
    check_one(nullptr, nullptr, 1.0f, 0.0f, 1.0f, 1.0f);
    ++cases;
    gs_grade x;
    char err[128] = "";
    EXPECT(gs_grade_compose_host(nullptr, nullptr, 1.0f, 0.0f, 1.0f, 1.0f, &x, err, sizeof(err)) == GS_OK && x.flags == 0u, "the defaults: flags %u", x.flags);
    // refusals of the compose: nothing is written
    memset(&x, 0x5A, sizeof(x));
    const gs_grade before = x;
    const float one[3] = {1, 1, 1}, ng[3] = {1, NAN, 1}, io[3] = {0, 0, INFINITY}, big[3] = {3e38f, 1, 1};
    EXPECT(gs_grade_compose_host(one, nullptr, 1.0f, 0.0f, 1.0f, 1.0f, nullptr, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "null out");
    EXPECT(gs_grade_compose_host(ng, nullptr, 1.0f, 0.0f, 1.0f, 1.0f, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "nan gain");
    EXPECT(gs_grade_compose_host(one, io, 1.0f, 0.0f, 1.0f, 1.0f, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "inf offset");
    EXPECT(gs_grade_compose_host(one, nullptr, NAN, 0.0f, 1.0f, 1.0f, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "nan saturation");
    EXPECT(gs_grade_compose_host(one, nullptr, 1.0f, -INFINITY, 1.0f, 1.0f, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "inf black");
    EXPECT(gs_grade_compose_host(one, nullptr, 1.0f, 0.0f, NAN, 1.0f, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "nan white");
    EXPECT(gs_grade_compose_host(one, nullptr, 1.0f, 0.25f, 0.25f, 1.0f, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "white == black");
    EXPECT(gs_grade_compose_host(one, nullptr, 1.0f, 0.0f, 1.0f, 0.0f, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "opacity_gain 0");
    EXPECT(gs_grade_compose_host(one, nullptr, 1.0f, 0.0f, 1.0f, -2.0f, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "opacity_gain < 0");
    EXPECT(gs_grade_compose_host(one, nullptr, 1.0f, 0.0f, 1.0f, INFINITY, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "opacity_gain inf");
    EXPECT(gs_grade_compose_host(big, nullptr, 1.0f, 0.0f, 0.5f, 1.0f, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "a overflows f32");
    EXPECT(gs_grade_compose_host(one, nullptr, 1.0f, 0.0f, 1.0f, NAN, &x, nullptr, 0) == GS_ERR_INVALID_ARGUMENT, "opacity_gain nan, no message buffer");
    EXPECT(memcmp(&x, &before, sizeof(x)) == 0, "a refusal wrote to *out");
    EXPECT(strstr(err, "gs_grade_compose") != nullptr, "message: %s", err);
    // refusals of gs_grade_splats' check; a member of a part that is not flagged is not looked at
    gs_grade g;
    const float tintv[3] = {1.1f, 0.9f, 1.0f}, offv[3] = {0.05f, 0.05f, 0.05f};
    EXPECT(gs_grade_compose_host(tintv, offv, 0.5f, 0.02f, 0.9f, 0.5f, &g, err, sizeof(err)) == GS_OK && g.flags == 7u, "flags %u", g.flags);
    EXPECT(gs_grade_validate_host(nullptr, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "null grade");
    gs_grade y = g;
    y.struct_size = 60;
    EXPECT(gs_grade_validate_host(&y, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "struct_size");
    y = g; y.flags = 0xF;
    EXPECT(gs_grade_validate_host(&y, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "unknown flag");
    y = g; y.reserved = 1.0f;
    EXPECT(gs_grade_validate_host(&y, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "reserved");
    y = g; y.a[5] = NAN;
    EXPECT(gs_grade_validate_host(&y, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "nan in a");
    y.flags = GS_GRADE_OFFSET | GS_GRADE_OPACITY;
    EXPECT(gs_grade_validate_host(&y, err, sizeof(err)) == GS_OK, "a is not flagged: %s", err);
    y = g; y.dc[2] = INFINITY;
    EXPECT(gs_grade_validate_host(&y, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "inf in dc");
    y.flags = GS_GRADE_MATRIX;
    EXPECT(gs_grade_validate_host(&y, err, sizeof(err)) == GS_OK, "dc is not flagged: %s", err);
    y = g; y.opacity_logit = NAN;
    EXPECT(gs_grade_validate_host(&y, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "nan logit");
    EXPECT(strstr(err, "gs_grade_splats") != nullptr, "message: %s", err);
    y.flags = 0u;
    EXPECT(gs_grade_validate_host(&y, nullptr, 0) == GS_OK, "flags 0 looks at no member");
    if (g_bad) {
        printf("grade_check: %d checks failed\n", g_bad);
        return 1;
    }
    printf("grade_check ok: %d grades\n", cases);
    return 0;
}
