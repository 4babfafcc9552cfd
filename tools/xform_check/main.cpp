// xform_check -- gs_xform_compose's host mathematics (csrc/gs_xform_math.hip) as a stand-alone program, meant to be built with
// -fsanitize=address,undefined (tests/test_transform.py does):
//   g++ -std=c++17 -fsanitize=address,undefined -I gaussian-splatting-wgpu_amd/csrc tools/xform_check/main.cpp \
//       -x c++ gaussian-splatting-wgpu_amd/csrc/gs_xform_math.hip -o xform_check && ./xform_check
// Over a few hundred seeded rotations (and the quarter turns) it checks that every D_l is orthogonal, that D_l^T B_l(d) = B_l(R^T d)
// on directions the solve never saw, that q is normalised and m = [sR | t + pivot - sR pivot], and that the refusals refuse without
// writing.  Exit status 0 and "xform_check ok" when everything holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "gs_xform_math.h"

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

static void check_one(const float q[4], const float t[3], float s, const float* pivot, std::mt19937& rng) {
    gs_xform x;
    char err[256] = "";
    const int32_t rc = gs_xform_compose_host(q, t, s, pivot, &x, err, sizeof(err));
    EXPECT(rc == GS_OK, "rc %d (%s)", rc, err);
    if (rc != GS_OK) return;
    EXPECT(x.struct_size == sizeof(gs_xform), "struct_size %u", x.struct_size);
    double len = 0.0;
    for (int k = 0; k < 4; ++k) len += (double)x.q[k] * x.q[k];
    EXPECT(std::fabs(len - 1.0) < 1e-6, "|q|^2 = %.9g", len);
    // the rotation part of m is s times an orthogonal matrix
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double dot = 0.0;
            for (int c = 0; c < 3; ++c) dot += (double)x.m[4 * a + c] * x.m[4 * b + c];
            EXPECT(std::fabs(dot - (a == b ? (double)s * s : 0.0)) < 1e-5 * (double)s * s, "m rows %d.%d = %.9g", a, b, dot);
        }
    // the pivot stays where it is, moved by t
    const float zero[3] = {0, 0, 0};
    const float* p = pivot ? pivot : zero;
    for (int r = 0; r < 3; ++r) {
        const double v = (double)x.m[4 * r] * p[0] + (double)x.m[4 * r + 1] * p[1] + (double)x.m[4 * r + 2] * p[2] + x.m[4 * r + 3];
        EXPECT(std::fabs(v - ((double)p[r] + t[r])) < 1e-4 * (1.0 + std::fabs(v)), "pivot row %d: %.9g", r, v);
    }
    EXPECT(std::fabs((double)x.log_scale - std::log((double)s)) < 1e-6, "log_scale %.9g", (double)x.log_scale);
    const float* D[3] = {x.sh1, x.sh2, x.sh3};
    std::uniform_real_distribution<double> uni(-1.0, 1.0);
    for (int l = 1; l <= 3; ++l) {
        const int n = 2 * l + 1;
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < n; ++b) {
                double dot = 0.0;
                for (int c = 0; c < n; ++c) dot += (double)D[l - 1][a * n + c] * D[l - 1][b * n + c];
                EXPECT(std::fabs(dot - (a == b ? 1.0 : 0.0)) < 2e-6, "band %d rows %d.%d = %.9g", l, a, b, dot);
            }
        for (int trial = 0; trial < 4; ++trial) { // D^T B(d) = B(R^T d), R = the rotation part of m / s
            double d[3], e[3], n2 = 0.0;
            do {
                n2 = 0.0;
                for (int c = 0; c < 3; ++c) { d[c] = uni(rng); n2 += d[c] * d[c]; }
            } while (n2 < 0.01 || n2 > 1.0);
            for (int c = 0; c < 3; ++c) d[c] /= std::sqrt(n2);
            for (int c = 0; c < 3; ++c) e[c] = ((double)x.m[c] * d[0] + (double)x.m[4 + c] * d[1] + (double)x.m[8 + c] * d[2]) / s;
            double y[7], yr[7];
            gs_xform_sh_basis(l, d, y);
            gs_xform_sh_basis(l, e, yr);
            for (int j = 0; j < n; ++j) {
                double v = 0.0;
                for (int i = 0; i < n; ++i) v += (double)D[l - 1][i * n + j] * y[i];
                EXPECT(std::fabs(v - yr[j]) < 5e-6, "band %d term %d: %.9g vs %.9g", l, j, v, yr[j]);
            }
        }
    }
}

int main() {
    std::mt19937 rng(20240611u);
    std::normal_distribution<float> nrm(0.0f, 1.0f);
    int cases = 0;
    for (int k = 0; k < 300; ++k) {
        float q[4], t[3], pv[3];
        for (float& v : q) v = nrm(rng) * (k % 5 == 0 ? 7.0f : 1.0f);
        for (float& v : t) v = nrm(rng);
        for (float& v : pv) v = 2.0f * nrm(rng);
        const float s = (k % 3 == 0) ? 1.0f : (k % 3 == 1 ? 0.5f : 3.0f);
        check_one(q, t, s, (k & 1) ? pv : nullptr, rng);
        ++cases;
    }
    const float h = 0.70710678f;
    const float quarter[][4] = {{1, 0, 0, 0}, {h, h, 0, 0}, {h, -h, 0, 0}, {0, 1, 0, 0}, {h, 0, h, 0}, {h, 0, -h, 0}, {0, 0, 1, 0},
                                {h, 0, 0, h}, {h, 0, 0, -h}, {0, 0, 0, 1}, {-3, 0, 0, 0}};
    const float t0[3] = {0.25f, -1.5f, 0.625f};
    for (const auto& q : quarter) {
        check_one(q, t0, 1.0f, nullptr, rng);
        ++cases;
    }
    // refusals: nothing is written
    gs_xform x;
    memset(&x, 0x5A, sizeof(x));
    gs_xform before = x;
    char err[64];
    const float one[4] = {1, 0, 0, 0}, zq[4] = {0, 0, 0, 0}, nq[4] = {1, NAN, 0, 0}, it[3] = {INFINITY, 0, 0};
    EXPECT(gs_xform_compose_host(nullptr, t0, 1.0f, nullptr, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "null rot");
    EXPECT(gs_xform_compose_host(one, nullptr, 1.0f, nullptr, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "null translate");
    EXPECT(gs_xform_compose_host(one, t0, 1.0f, nullptr, nullptr, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "null out");
    EXPECT(gs_xform_compose_host(zq, t0, 1.0f, nullptr, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "zero quaternion");
    EXPECT(gs_xform_compose_host(nq, t0, 1.0f, nullptr, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "nan quaternion");
    EXPECT(gs_xform_compose_host(one, it, 1.0f, nullptr, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "inf translate");
    EXPECT(gs_xform_compose_host(one, t0, 1.0f, it, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "inf pivot");
    EXPECT(gs_xform_compose_host(one, t0, 0.0f, nullptr, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "scale 0");
    EXPECT(gs_xform_compose_host(one, t0, -1.0f, nullptr, &x, err, sizeof(err)) == GS_ERR_INVALID_ARGUMENT, "scale < 0");
    EXPECT(gs_xform_compose_host(one, t0, NAN, nullptr, &x, nullptr, 0) == GS_ERR_INVALID_ARGUMENT, "scale nan, no message buffer");
    EXPECT(memcmp(&x, &before, sizeof(x)) == 0, "a refusal wrote to *out");
    EXPECT(strstr(err, "gs_xform_compose") != nullptr, "message: %s", err);
    if (g_bad) {
        printf("xform_check: %d checks failed\n", g_bad);
        return 1;
    }
    printf("xform_check ok: %d transforms\n", cases);
    return 0;
}
