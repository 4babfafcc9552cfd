// pack_check -- the host side of the packed scenes (csrc/gs_pack_host.hip and gs_pack_math.h) as a stand-alone program, meant to
// be built with -fsanitize=address,undefined (tests/test_packed.py does):
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I gaussian-splatting-wgpu_amd/csrc tools/pack_check/main.cpp \
//       -x c++ gaussian-splatting-wgpu_amd/csrc/gs_pack_host.hip -o pack_check && ./pack_check <scratch directory>
// It runs the codec over every chunk margin (n = 0, 1, 255, 256, 257, 513, 3001) at degrees 0..3 on records with NaN, infinities,
// denormals, zero quaternions and logits beyond +-89, in arrays sized exactly (a write past an end is the sanitizer's to find);
// round-trips files through the writer and the loader; and feeds the header parser every prefix of a valid header, headers with one
// byte changed and the refusals of the format.  Exit status 0 and "pack_check ok" when everything holds.
//   ./pack_check --exp <hex word> ...   prints the bit pattern of pk_exp of every argument (the test holds it to the oracle's expf).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "gs_pack_host.h"
#include "gs_pack_math.h"

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

static std::vector<float> records(uint64_t n, uint32_t seed) {
    std::mt19937 rng(seed);
    std::normal_distribution<float> nrm(0.0f, 1.0f);
    std::vector<float> r(n * 80);
    for (float& v : r) v = nrm(rng);
    const float special[] = {NAN, INFINITY, -INFINITY, 1e-45f, -0.0f, 3.0e38f, -3.0e38f, 100.0f, -100.0f, 0.0f};
    for (uint64_t g = 0; g < n; g += 3) r[g * 80 + (g * 7) % 80] = special[(g / 3) % 10];
    for (uint64_t g = 1; g < n; g += 5) r[g * 80 + 12] = special[(g / 5) % 10];
    for (uint64_t g = 2; g < n; g += 11)
        for (int k = 8; k < 12; ++k) r[g * 80 + k] = (g % 2) ? 0.0f : 1e-45f;
    return r;
}

static void codec(uint64_t n, int degree) {
    const std::vector<float> rec = records(n, 1000u + (uint32_t)n + (uint32_t)degree);
    const uint64_t C = gs_pack_chunks(n), K3 = 3u * (uint64_t)gs_pack_rest(degree);
    std::vector<float> chunks(C * 18);
    std::vector<uint32_t> verts(n * 4);
    std::vector<uint8_t> sh(n * K3);
    uint64_t bad = 0;
    gs_pack_encode_host(rec.data(), n, degree, chunks.data(), verts.data(), sh.data(), &bad);
    uint64_t want_bad = 0;
    for (uint64_t g = 0; g < n; ++g) {
        const float* f = &rec[g * 80];
        const int carried[] = {0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 16, 17, 18};
        for (int k : carried) want_bad += !std::isfinite(f[k]);
        want_bad += std::isnan(f[12]);
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < gs_pack_rest(degree); ++i) want_bad += !std::isfinite(f[16 + 4 * (i + 1) + c]);
    }
    EXPECT(bad == want_bad, "n %llu degree %d: nonfinite %llu, counted %llu", (unsigned long long)n, degree, (unsigned long long)bad, (unsigned long long)want_bad);
    for (float v : chunks) EXPECT(std::isfinite(v), "a chunk bound is not finite");
    std::vector<float> back(n * 80);
    gs_pack_decode_host(chunks.data(), verts.data(), sh.data(), n, degree, gs_pack_logits(), back.data());
    for (uint64_t g = 0; g < n; ++g) {
        const float *f = &rec[g * 80], *d = &back[g * 80];
        const float* b = &chunks[(g / 256) * 18];
        for (int k = 0; k < 80; ++k) EXPECT(std::isfinite(d[k]), "decoded float %d of record %llu is not finite", k, (unsigned long long)g);
        for (int k = 0; k < 3; ++k) {
            const float p = pk_fin(f[k]);
            if (!std::isfinite(b[3 + k] - b[k])) continue; // (a chunk that spans more than f32 holds: norm is 0 or NaN there)
            const double step = ((double)b[3 + k] - (double)b[k]) / (k == 1 ? 1023.0 : 2047.0);
            EXPECT(std::fabs((double)d[k] - (double)p) <= 0.505 * step + 1e-30, "position %d of record %llu: %g vs %g", k, (unsigned long long)g, d[k], p);
        }
    }
}

static std::string slurp(const std::string& path) {
    std::string s;
    if (FILE* fp = fopen(path.c_str(), "rb")) {
        char buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), fp)) > 0) s.append(buf, got);
        fclose(fp);
    }
    return s;
}
static void spill(const std::string& path, const std::string& bytes) {
    FILE* fp = fopen(path.c_str(), "wb");
    if (!fp) { EXPECT(false, "cannot create %s", path.c_str()); return; }
    fwrite(bytes.data(), 1, bytes.size(), fp);
    fclose(fp);
}
// the loader refuses and leaves its outputs as they were
static void refused(const std::string& path, const char* what) {
    void* rec = (void*)0x5A5A;
    uint64_t n = 77;
    int32_t deg = 78;
    char err[256] = "";
    const int32_t rc = gs_pack_load_host(path.c_str(), &rec, &n, &deg, err, sizeof(err));
    EXPECT(rc == GS_ERR_INVALID_ARGUMENT, "%s: rc %d", what, rc);
    EXPECT(rec == (void*)0x5A5A && n == 77 && deg == 78, "%s: a refusal wrote an output", what);
    EXPECT(strstr(err, path.c_str()) != nullptr, "%s: the message does not name the path: %s", what, err);
    if (rc == GS_OK) free(rec);
}

static void files(const std::string& dir) {
    const std::string path = dir + "/pack_check.ply";
    char err[256] = "";
    for (uint64_t n : {0u, 1u, 256u, 257u, 3001u})
        for (int degree = 0; degree <= 3; ++degree) {
            const std::vector<float> rec = records(n, 7u + (uint32_t)n);
            EXPECT(gs_pack_save_host(path.c_str(), rec.data(), n, degree, err, sizeof(err)) == GS_OK, "save: %s", err);
            const std::string raw = slurp(path);
            EXPECT(raw.size() == gs_pack_file_bytes(n, degree), "file of %zu bytes, %llu implied", raw.size(), (unsigned long long)gs_pack_file_bytes(n, degree));
            void* out = nullptr;
            uint64_t m = 0;
            int32_t deg = -1;
            EXPECT(gs_pack_load_host(path.c_str(), &out, &m, &deg, err, sizeof(err)) == GS_OK, "load: %s", err);
            EXPECT(m == n && deg == degree, "loaded %llu records of degree %d", (unsigned long long)m, deg);
            if (out && n) {
                std::vector<float> chunks(gs_pack_chunks(n) * 18), back(n * 80);
                std::vector<uint32_t> verts(n * 4);
                std::vector<uint8_t> sh(n * 3 * (uint64_t)gs_pack_rest(degree));
                gs_pack_encode_host(rec.data(), n, degree, chunks.data(), verts.data(), sh.data(), nullptr);
                gs_pack_decode_host(chunks.data(), verts.data(), sh.data(), n, degree, gs_pack_logits(), back.data());
                EXPECT(memcmp(out, back.data(), n * 320) == 0, "the loaded records differ from the decoded ones (n %llu degree %d)", (unsigned long long)n, degree);
            }
            free(out);
        }
    // every prefix of a valid file's header, and the header with one byte changed, through the parser and the loader
    const std::vector<float> rec = records(300, 5u);
    EXPECT(gs_pack_save_host(path.c_str(), rec.data(), 300, 2, err, sizeof(err)) == GS_OK, "save: %s", err);
    const std::string good = slurp(path);
    const size_t hdr = gs_pack_header(300, 2).size();
    const std::string bad_path = dir + "/pack_check_bad.ply";
    for (size_t cut = 0; cut < hdr; cut += (cut < 64 ? 1 : 7)) {
        GsPackLayout L;
        L.n = 4242;
        const int32_t rc = gs_pack_parse_header("pack_check", "prefix", (const unsigned char*)good.data(), cut, good.size(), &L, err, sizeof(err));
        EXPECT(rc == GS_ERR_INVALID_ARGUMENT && L.n == 4242, "a header cut at %zu was accepted", cut);
    }
    std::mt19937 rng(99u);
    for (int trial = 0; trial < 400; ++trial) {
        std::string g = good.substr(0, hdr + 64);
        const size_t at = rng() % hdr;
        const char ch = (char)(rng() & 0xFF);
        if (g[at] == ch) continue;
        g[at] = ch;
        GsPackLayout L;
        const int32_t rc = gs_pack_parse_header("pack_check", "garbled", (const unsigned char*)g.data(), g.size(), good.size(), &L, err, sizeof(err));
        EXPECT(rc == GS_ERR_INVALID_ARGUMENT, "a header with byte %zu changed to 0x%02x was accepted", at, (unsigned)(unsigned char)ch);
    }
    auto replaced = [&](const std::string& from, const std::string& to) {
        std::string g = good;
        const size_t at = g.find(from);
        EXPECT(at != std::string::npos, "%s not in the header", from.c_str());
        if (at != std::string::npos) g.replace(at, from.size(), to);
        return g;
    };
    spill(bad_path, replaced("comment gsplat-packed 1\n", ""));
    refused(bad_path, "missing marker");
    spill(bad_path, replaced("property uint packed_scale", "property uint packed_size"));
    refused(bad_path, "renamed property");
    spill(bad_path, replaced("property float min_r", "property double min_r"));
    refused(bad_path, "retyped property");
    spill(bad_path, replaced("element chunk 2", "element chunk 3"));
    refused(bad_path, "chunk count");
    spill(bad_path, replaced("element vertex 300", "element vertex 4000000000"));
    refused(bad_path, "vertex count");
    spill(bad_path, replaced("element vertex 300", "element vertex 2147483647"));
    refused(bad_path, "a count the file does not back");
    spill(bad_path, good.substr(0, good.size() - 1));
    refused(bad_path, "one byte short");
    spill(bad_path, good + "x");
    refused(bad_path, "one byte long");
    spill(bad_path, gs_pack_header(0, 0).substr(0, gs_pack_header(0, 0).size() - 11) + "element sh 0\nend_header\n");
    refused(bad_path, "an sh element at degree 0");
    spill(bad_path, "");
    refused(bad_path, "an empty file");
    refused(dir + "/pack_check_missing.ply", "a file that does not exist");
    remove(path.c_str());
    remove(bad_path.c_str());
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "--exp") == 0) {
        for (int k = 2; k < argc; ++k) printf("%08x\n", pk_bits(pk_exp(pk_float((uint32_t)strtoul(argv[k], nullptr, 16)))));
        return 0;
    }
    if (argc < 2) {
        printf("usage: pack_check <scratch directory> | --exp <hex word> ...\n");
        return 2;
    }
    for (uint64_t n : {0u, 1u, 255u, 256u, 257u, 513u, 3001u})
        for (int degree = 0; degree <= 3; ++degree) codec(n, degree);
    files(argv[1]);
    float table[256];
    memcpy(table, gs_pack_logits(), sizeof(table));
    for (int a = 0; a < 256; ++a) EXPECT(std::isfinite(table[a]) && (a == 0 || table[a] > table[a - 1]), "logit %d", a);
    if (g_bad) {
        printf("pack_check: %d checks failed\n", g_bad);
        return 1;
    }
    printf("pack_check ok\n");
    return 0;
}
