// shard_files.cpp — see shard_files.hpp.
#include "shard_files.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstring>

namespace mxec {

std::string hex(const uint8_t* d, size_t n) {
    static const char* k = "0123456789abcdef";
    std::string s(2 * n, '0');
    for (size_t i = 0; i < n; ++i) {
        s[2 * i] = k[d[i] >> 4];
        s[2 * i + 1] = k[d[i] & 15];
    }
    return s;
}

bool unhex32(const std::string& s, uint8_t* out) {
    if (s.size() != 64) return false;
    auto v = [](char c) -> int {
        if (c >= '0' && c <= '9') return c - '0';
        if (c >= 'a' && c <= 'f') return c - 'a' + 10;
        if (c >= 'A' && c <= 'F') return c - 'A' + 10;
        return -1;
    };
    for (int i = 0; i < 32; ++i) {
        int hi = v(s[size_t(2 * i)]), lo = v(s[size_t(2 * i + 1)]);
        if (hi < 0 || lo < 0) return false;
        out[i] = uint8_t(hi << 4 | lo);
    }
    return true;
}

bool manifest_digest32(const std::string& s, uint8_t* out) { return unhex32(s, out) && hex(out, 32) == s; }

std::string chunk_name(uint32_t index) {
    char b[32];
    std::snprintf(b, sizeof b, "%06u", index);
    return b;
}

// Exactly n bytes from / to fd (EINTR retried); false when it ends early.
static bool read_all(int fd, uint8_t* dst, size_t n) {
    size_t got = 0;
    while (got < n) {
        const ssize_t r = ::read(fd, dst + got, n - got);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) break;
        got += size_t(r);
    }
    return got == n;
}

static bool write_all(int fd, const uint8_t* src, size_t n) {
    size_t put = 0;
    while (put < n) {
        const ssize_t w = ::write(fd, src + put, n - put);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) break;
        put += size_t(w);
    }
    return put == n;
}

// `p` open for reading and its size; -1 with the thread's error set.
static int open_sized(const fs::path& p, uint64_t* size) {
    const int fd = ::open(p.c_str(), O_RDONLY | O_CLOEXEC);
    struct stat st;
    if (fd >= 0 && ::fstat(fd, &st) == 0) {
        *size = uint64_t(st.st_size);
        return fd;
    }
    const int e = errno;
    if (fd >= 0) ::close(fd);
    set_error(MXEC_E_IO, "IO error: " + p.string() + ": " + std::strerror(e));
    return -1;
}

int read_file(const fs::path& p, Bytes& out) {
    uint64_t size = 0;
    const int fd = open_sized(p, &size);
    if (fd < 0) return MXEC_E_IO;
    out.resize(size_t(size));
    const bool ok = read_all(fd, out.data(), out.size());
    ::close(fd);
    if (!ok) return set_error(MXEC_E_IO, "IO error: read failed for " + p.string());
    return MXEC_OK;
}

int read_file_to(const fs::path& p, uint8_t* dst, uint64_t want, uint64_t* size) {
    const int fd = open_sized(p, size);
    if (fd < 0) return MXEC_E_IO;
    const bool ok = *size != want || read_all(fd, dst, size_t(want));
    ::close(fd);
    if (!ok) return set_error(MXEC_E_IO, "IO error: read failed for " + p.string());
    return MXEC_OK;
}

int write_file(const fs::path& p, const uint8_t* data, size_t len) {
    const int fd = ::open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd < 0) return set_error(MXEC_E_IO, "IO error: cannot create " + p.string() + ": " + std::strerror(errno));
    const bool ok = write_all(fd, data, len);
    if (::close(fd) != 0 || !ok) return set_error(MXEC_E_IO, "IO error: write failed for " + p.string());
    return MXEC_OK;
}

int replace_file(const fs::path& dir, const std::string& name, const uint8_t* data, size_t len) {
    static std::atomic<uint64_t> seq{0};
    const fs::path tmp = dir / ("." + name + ".heal." + std::to_string(::getpid()) + "." + std::to_string(seq++));
    const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0644);
    if (fd < 0) return set_error(MXEC_E_IO, "IO error: cannot create " + tmp.string() + ": " + std::strerror(errno));
    bool ok = write_all(fd, data, len) && ::fsync(fd) == 0;
    ok = (::close(fd) == 0) && ok;
    if (ok && ::rename(tmp.c_str(), (dir / name).c_str()) != 0) ok = false;
    if (!ok) {
        const std::string why = std::strerror(errno);
        ::unlink(tmp.c_str());
        return set_error(MXEC_E_IO, "IO error: heal write failed for " + (dir / name).string() + ": " + why);
    }
    const int dfd = ::open(dir.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
    if (dfd >= 0) {
        (void)::fsync(dfd);
        ::close(dfd);
    }
    return MXEC_OK;
}

int read_manifest(const fs::path& ec_dir, Manifest& m) {
    Bytes raw;
    MXEC_TRY(read_file(ec_dir / "manifest.json", raw));
    // fs::read_to_string fails with an I/O error (InvalidData) on bytes that
    // are not UTF-8; then serde_json::from_str (filesystem.rs:3164-3171).
    if (!utf8_valid(raw.data(), raw.size()))
        return set_error(MXEC_E_IO, "IO error: stream did not contain valid UTF-8");
    std::string s(raw.begin(), raw.end());
    std::string why;
    if (!parse_manifest(s, m, &why)) return set_error(MXEC_E_JSON, "JSON error: " + why);
    if (m.chunks.size() < m.chunk_count) return set_error(MXEC_E_JSON, "JSON error: manifest lists fewer chunks than chunk_count");
    return MXEC_OK;
}

}  // namespace mxec
