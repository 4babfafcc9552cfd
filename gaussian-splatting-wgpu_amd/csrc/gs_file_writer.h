// gs_file_writer.h -- the file an export writes (gs_ply_save, gs_export_ply, gs_export_packed): closed by the destructor and, unless
// finish() succeeded, removed.  Needs the C library, the error codes and a declaration of fail (the library's is in gs_context.hip;
// tools/file_check defines its own and builds this header with a host compiler and sanitizers, without HIP).
#pragma once
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/gsplat/gs_abi.h"

int32_t fail(int32_t code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

struct FileWriter {
    const char* who; // the caller, named in the messages
    std::string path;
    FILE* fp = nullptr;
    bool done = false;
    FileWriter(const char* w, const char* p) : who(w), path(p) {}
    FileWriter(const FileWriter&) = delete;
    FileWriter& operator=(const FileWriter&) = delete;
    ~FileWriter() {
        if (fp) fclose(fp);
        if (fp && !done) remove(path.c_str());
    }
    int32_t err(const char* what) const { return fail(GS_ERR_INVALID_ARGUMENT, "%s: cannot %s %s: %s", who, what, path.c_str(), strerror(errno)); }
    int32_t open(const std::string& header) {
        fp = fopen(path.c_str(), "wb");
        if (!fp) return err("create");
        return write(header.data(), header.size());
    }
    int32_t write(const void* p, size_t bytes) { return fwrite(p, 1, bytes, fp) == bytes ? GS_OK : err("write"); }
    int32_t finish() { // (a full disk may only show when the buffered tail is flushed)
        FILE* f = fp;
        fp = nullptr;
        if (fclose(f) == 0) { done = true; return GS_OK; }
        const int32_t rc = err("write");
        remove(path.c_str());
        return rc;
    }
};
