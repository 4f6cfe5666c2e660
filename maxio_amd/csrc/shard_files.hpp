// shard_files.hpp — everything the storage entry points do to the file
// system: chunk files `{key}.ec/{index:06}` and manifest.json (mod.rs:145-189)
// read and written whole, a rebuilt shard replaced atomically, hex digests,
// and the pooled byte buffers the chunks are read into.
//
// Host-only (no HIP): built into libmaxio_ec.so and, on its own with
// -fsanitize=address,undefined, into the CPU test harness
// tests/c_manifest/shard_files_check.cpp.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <filesystem>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "error.hpp"
#include "manifest.hpp"

namespace mxec {

namespace fs = std::filesystem;

std::string hex(const uint8_t* d, size_t n);       // lower case, 2n characters
bool unhex32(const std::string& s, uint8_t* out);  // 64 hex digits of either case
// A manifest's recorded digest as the bytes a computed one is compared with.
// The reference compares strings, hex::encode(hash) != chunk_info.sha256
// (chunk_reader.rs:108-109, :184-185), so only the 64 lower-case digits hex()
// produces can ever match: anything else (upper case included) is false, and
// the caller treats the shard as one whose digest never matches.
bool manifest_digest32(const std::string& s, uint8_t* out);
std::string chunk_name(uint32_t index);            // "{index:06}"

// Byte buffers whose resize() leaves new bytes uninitialised: a chunk about
// to be overwritten by read(2) or a decode need not be zero-filled first.
//
// Large buffers come from a process-wide free list by power-of-two class: a
// GET allocates a chunk-sized buffer per shard, and fresh mmap'd memory costs
// a page fault per 4 KiB on first touch and a TLB shoot-down across every
// request thread on munmap -- with 64 request threads that took more host
// CPU than the data copies.  Pages past the requested size are never
// touched, so the rounding costs address space, not memory.
class BigPool {
public:
    static constexpr size_t kMin = size_t(256) << 10;
    static BigPool& get() {
        static BigPool* p = new BigPool;  // never destroyed: used from static destructors
        return *p;
    }
    static size_t cls(size_t n) {
        size_t c = kMin;
        while (c < n) c <<= 1;
        return c;
    }
    void* take(size_t c) {
        {
            std::lock_guard<std::mutex> g(mu_);
            auto it = free_.find(c);
            if (it != free_.end() && !it->second.empty()) {
                void* p = it->second.back();
                it->second.pop_back();
                cached_ -= c;
                return p;
            }
        }
        void* p = std::malloc(c);
        if (!p) throw std::bad_alloc();
        return p;
    }
    void give(void* p, size_t c) {
        {
            std::lock_guard<std::mutex> g(mu_);
            if (cached_ + c <= kCap) {
                free_[c].push_back(p);
                cached_ += c;
                return;
            }
        }
        std::free(p);
    }

private:
    static constexpr size_t kCap = size_t(2) << 30;  // bytes kept for reuse
    std::mutex mu_;
    std::map<size_t, std::vector<void*>> free_;
    size_t cached_ = 0;
};

template <class T>
struct NoInitAlloc : std::allocator<T> {
    using value_type = T;
    template <class U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    NoInitAlloc() = default;
    template <class U>
    NoInitAlloc(const NoInitAlloc<U>&) {}
    T* allocate(size_t n) {
        const size_t b = n * sizeof(T);
        if (b < BigPool::kMin) return std::allocator<T>::allocate(n);
        return static_cast<T*>(BigPool::get().take(BigPool::cls(b)));
    }
    void deallocate(T* p, size_t n) {
        const size_t b = n * sizeof(T);
        if (b < BigPool::kMin) return std::allocator<T>::deallocate(p, n);
        BigPool::get().give(p, BigPool::cls(b));
    }
    template <class U, class... A>
    void construct(U* p, A&&... a) {
        if constexpr (sizeof...(A) == 0) ::new (static_cast<void*>(p)) U;
        else ::new (static_cast<void*>(p)) U(std::forward<A>(a)...);
    }
};
using Bytes = std::vector<uint8_t, NoInitAlloc<uint8_t>>;

// std::fs::read: whole file or an io::Error.
int read_file(const fs::path& p, Bytes& out);
// read_file into a caller buffer of exactly `want` bytes; *size gets the
// file's size (when it differs, nothing is read and MXEC_OK is returned so
// the caller can report the mismatch like read_file + size check would).
int read_file_to(const fs::path& p, uint8_t* dst, uint64_t want, uint64_t* size);
int write_file(const fs::path& p, const uint8_t* data, size_t len);
// A rebuilt shard under its final name, all of it or not at all: written to
// a temporary name in the same directory, fsynced, renamed over the final
// name, and the directory entry fsynced.
int replace_file(const fs::path& dir, const std::string& name, const uint8_t* data, size_t len);

// manifest.json of `ec_dir` as fs::read_to_string + serde_json::from_str read
// it (filesystem.rs:3164-3171), with chunks.size() >= chunk_count.
int read_manifest(const fs::path& ec_dir, Manifest& m);

}  // namespace mxec
