// tools/moments_check -- gs_exact_sum.h on its own, for a host compiler with sanitizers (tests/test_moments.py builds it with
// -fsanitize=address,undefined and runs it as its own process).
//
//   moments_check FILE     FILE: "K N" and then N lines of K f32 bit patterns in hex.  Prints the exact sums and sums of products of
//                          the rows whose K values are all finite, as gs_moments_host orders them: "counted C", then one line
//                          "hi lo" (the doubles' bit patterns in hex) per quantity -- the K sums, then the products j <= l.
// Before that it checks the limb bounds at the extreme exponents and prints "moments_check ok".
#include <cfloat>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gs_exact_sum.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static float f32_of(uint32_t b) { float v; memcpy(&v, &b, 4); return v; }
static uint64_t bits_of(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

static void self_check() {
    // the largest term: FLT_MAX^2 = (2^24 - 1)^2 2^208 sits at bit 506, limb 15, and ends in limb 17 of 20
    {
        const uint32_t b = 0x7F7FFFFFu;
        uint32_t c[3];
        const uint32_t p = ex_pos2(b, b), L = ex_chunks((uint64_t)ex_mant(b) * ex_mant(b), p, c);
        CHECK(p == 506u && L == 15u && L + 2u < GS_EX_LIMBS && c[2] != 0u && c[2] < (1u << 16));
        int64_t t[GS_EX_LIMBS] = {};
        ex_add_product(t, f32_of(b), f32_of(b));
        double hi, lo;
        ex_finish(t, &hi, &lo);
        const double m = (double)FLT_MAX; // FLT_MAX^2 in double is exact: 48 significant bits, exponent 255
        CHECK(hi == m * m && lo == 0.0 && !std::signbit(lo));
    }
    // the smallest: (2^-149)^2 = 2^-298 is bit 0 of limb 0
    {
        uint32_t c[3];
        const uint32_t p = ex_pos2(1u, 1u), L = ex_chunks((uint64_t)ex_mant(1u) * ex_mant(1u), p, c);
        CHECK(p == 0u && L == 0u && c[0] == 1u && c[1] == 0u && c[2] == 0u);
        int64_t t[GS_EX_LIMBS] = {};
        ex_add_product(t, f32_of(1u), f32_of(0x80000001u));
        double hi, lo;
        ex_finish(t, &hi, &lo);
        CHECK(hi == -std::ldexp(1.0, -298) && lo == 0.0 && !std::signbit(lo));
    }
    // single values: 2^-149 at bit 149, FLT_MAX at bit 402
    CHECK(ex_pos1(1u) == 149u && ex_pos1(0x7F7FFFFFu) == 402u);
    // 2^31 - 1 copies of the largest chunk in one limb, of either sign, stay within i64; the finish takes such a limb
    for (int sign = 1; sign >= -1; sign -= 2) {
        int64_t limb = 0;
        CHECK(!__builtin_mul_overflow((int64_t)0xFFFFFFFFll, (int64_t)0x7FFFFFFFll, &limb));
        limb *= sign;
        int64_t t[GS_EX_LIMBS] = {};
        t[10] = limb; // limb 10's unit is 2^(320 - 298) = 2^22, limb 9's 2^-10
        t[9] = sign * (int64_t)0x7FFFFFFFll * 3; // and something below it
        double hi, lo;
        ex_finish(t, &hi, &lo);
        // the value is (limb 2^32 + t[9]) 2^-10 exactly; limb 2^32 alone needs 95 bits, so compare through long integers
        const __int128 v = (__int128)limb * ((__int128)1 << 32) + t[9];
        const __int128 h = (__int128)std::ldexp(hi, 10), l = (__int128)std::ldexp(lo, 10);
        CHECK(std::ldexp(hi, 10) == (double)h && std::ldexp(lo, 10) == (double)l); // both are integers there
        CHECK(h + l == v);                                                         // hi + lo holds all 95 bits
        CHECK((double)v == std::ldexp(hi, 10));                                    // the compiler's own i128 -> double rounds to nearest
    }
    // ties to even, and the rest
    {
        int64_t t[GS_EX_LIMBS] = {};
        ex_add_value(t, 0x1p53f);
        ex_add_value(t, 1.0f);
        double hi, lo;
        ex_finish(t, &hi, &lo);
        CHECK(hi == 0x1p53 && lo == 1.0);
        ex_add_value(t, 2.0f);
        ex_finish(t, &hi, &lo);
        CHECK(hi == 0x1p53 + 4.0 && lo == -1.0);
        ex_add_value(t, -0x1p53f);
        ex_add_value(t, -3.0f);
        ex_finish(t, &hi, &lo);
        CHECK(hi == 0.0 && lo == 0.0 && !std::signbit(hi) && !std::signbit(lo));
    }
}

int main(int argc, char** argv) {
    self_check();
    if (failures) return 1;
    printf("moments_check ok\n");
    if (argc < 2) return 0;
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    unsigned k = 0;
    unsigned long long n = 0;
    if (fscanf(f, "%u %llu", &k, &n) != 2 || k < 1u || k > 3u) { fclose(f); printf("bad header\n"); return 2; }
    const unsigned q = k + k * (k + 1u) / 2u;
    std::vector<int64_t> tables((size_t)q * GS_EX_LIMBS, 0);
    unsigned long long counted = 0;
    for (unsigned long long i = 0; i < n; ++i) {
        float v[3] = {0, 0, 0};
        bool fin = true;
        for (unsigned j = 0; j < k; ++j) {
            unsigned b = 0;
            if (fscanf(f, "%x", &b) != 1) { fclose(f); printf("bad row %llu\n", i); return 2; }
            v[j] = f32_of(b);
            fin = fin && ex_finite(b);
        }
        if (!fin) continue;
        ++counted;
        unsigned t = 0;
        for (unsigned j = 0; j < k; ++j, ++t) ex_add_value(&tables[(size_t)t * GS_EX_LIMBS], v[j]);
        for (unsigned j = 0; j < k; ++j)
            for (unsigned l = j; l < k; ++l, ++t) ex_add_product(&tables[(size_t)t * GS_EX_LIMBS], v[j], v[l]);
    }
    fclose(f);
    printf("counted %llu\n", counted);
    for (unsigned t = 0; t < q; ++t) {
        double hi, lo;
        ex_finish(&tables[(size_t)t * GS_EX_LIMBS], &hi, &lo);
        printf("%016" PRIx64 " %016" PRIx64 "\n", bits_of(hi), bits_of(lo));
    }
    return 0;
}
