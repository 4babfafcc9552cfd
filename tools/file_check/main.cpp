// file_check -- the file an export writes (csrc/gs_file_writer.h) as a stand-alone program, meant to be built with
// -fsanitize=address,undefined (tests/test_export.py does):
//   g++ -std=c++17 -fsanitize=address,undefined -I gaussian-splatting-wgpu_amd/csrc tools/file_check/main.cpp -o file_check \
//       && ./file_check <scratch directory>
// It defines the library's `fail` itself (the header needs nothing else) and holds the writer to what its callers rely on: a
// finished file is the header and the bytes written, nothing more; a writer that goes away without finish() leaves no file; a path
// that cannot be created is refused with the caller's name and "cannot create" and leaves nothing; a second writer on a path
// replaces the first file.  It writes ordinary files under the directory it is given and nowhere else.  Exit status 0 and
// "file_check ok" when everything holds.
#include <cstdarg>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "gs_file_writer.h"

static char g_err[512];
int32_t fail(int32_t code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static int g_bad = 0;
#define EXPECT(cond)                                             \
    do {                                                         \
        if (!(cond)) {                                           \
            ++g_bad;                                             \
            printf("FAIL line %d: %s (%s)\n", __LINE__, #cond, g_err); \
        }                                                        \
    } while (0)

static bool exists(const std::string& p) {
    struct stat st;
    return stat(p.c_str(), &st) == 0;
}
static bool holds(const std::string& p, const std::string& want) {
    FILE* f = fopen(p.c_str(), "rb");
    if (!f) return false;
    std::string got(want.size() + 16, '\0');
    got.resize(fread(&got[0], 1, got.size(), f));
    fclose(f);
    return got == want;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: file_check <scratch directory>\n");
        return 2;
    }
    const std::string dir = argv[1], path = dir + "/out.bin";
    const std::string header = "ply\nformat binary_little_endian 1.0\nend_header\n";
    std::vector<unsigned char> big(3 * 65536 + 7); // more than the C library buffers: written through before finish()
    for (size_t i = 0; i < big.size(); ++i) big[i] = (unsigned char)(i * 131u + 17u);
    const std::string body((const char*)big.data(), big.size());

    { // finished: exactly the header and the bytes written, in order, in pieces of any size (an empty one among them)
        FileWriter w("check_a", path.c_str());
        EXPECT(w.open(header) == GS_OK);
        EXPECT(w.write(big.data(), 1) == GS_OK);
        EXPECT(w.write(big.data() + 1, 0) == GS_OK);
        EXPECT(w.write(big.data() + 1, big.size() - 1) == GS_OK);
        EXPECT(w.finish() == GS_OK);
        EXPECT(w.done && !w.fp);
    }
    EXPECT(holds(path, header + body));
    { // a header alone
        FileWriter w("check_b", path.c_str());
        EXPECT(w.open(header) == GS_OK && w.finish() == GS_OK);
    }
    EXPECT(holds(path, header)); // ... which replaced the longer file
    { // destroyed without finish(): no file, whether or not anything was written; the file it replaced is gone too
        FileWriter w("check_c", path.c_str());
        EXPECT(w.open(header) == GS_OK);
        EXPECT(w.write(big.data(), big.size()) == GS_OK);
        EXPECT(exists(path));
    }
    EXPECT(!exists(path));
    { // never opened: the destructor touches nothing
        FileWriter w("check_d", path.c_str());
    }
    EXPECT(!exists(path));
    { // a directory that does not exist
        const std::string missing = dir + "/no_such_dir/out.bin";
        FileWriter w("check_e", missing.c_str());
        g_err[0] = 0;
        EXPECT(w.open(header) == GS_ERR_INVALID_ARGUMENT);
        const std::string msg = g_err;
        EXPECT(msg.find("check_e: cannot create " + missing + ": ") == 0);
        EXPECT(msg.find(strerror(ENOENT)) != std::string::npos);
        EXPECT(!w.fp && !exists(missing) && !exists(dir + "/no_such_dir"));
    }
    { // a second writer on the same path replaces the first file
        FileWriter first("check_f", path.c_str());
        EXPECT(first.open(header) == GS_OK && first.write(big.data(), big.size()) == GS_OK && first.finish() == GS_OK);
        EXPECT(holds(path, header + body));
        FileWriter second("check_g", path.c_str());
        EXPECT(second.open("second\n") == GS_OK && second.write("xyz", 3) == GS_OK && second.finish() == GS_OK);
        EXPECT(holds(path, "second\nxyz"));
    }
    EXPECT(holds(path, "second\nxyz")); // finished writers leave their file when they go
    remove(path.c_str());
    if (g_bad) {
        printf("file_check: %d failed\n", g_bad);
        return 1;
    }
    printf("file_check ok\n");
    return 0;
}
