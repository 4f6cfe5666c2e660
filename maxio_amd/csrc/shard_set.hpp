// shard_set.hpp — one object's k+m shards in host memory, ready for a decode:
// what try_reconstruct_data_chunk (chunk_reader.rs:157-226) builds before it
// calls ReedSolomon::reconstruct.  The heal of a scrub, the locate pass and a
// GET with a bad chunk all build it the same way.
#pragma once

#include <algorithm>

#include "shard_files.hpp"

namespace mxec {

struct ShardSet {
    const Manifest* man = nullptr;
    int k = 0, m = 0, total = 0;
    uint64_t shard = 0;
    std::vector<Bytes> bufs;       // the shards this set read or is to rebuild
    std::vector<uint8_t*> ptrs;    // every shard, in `bufs` or adopted; never null
    std::vector<size_t> lens;      // want(i)
    std::vector<uint8_t> present;  // 0: an erasure, rebuilt by decode

    // Whether open() checks (k, m) as ReedSolomon::new would: never (a GET
    // decodes only what the PUT wrote), only with parity, or always.
    enum RsCheck { kNoCheck, kCheckParity, kCheckAlways };

    // The geometry of `manifest`, which must outlive the set.
    int open(const Manifest& manifest, RsCheck check) {
        man = &manifest;
        k = int(manifest.chunk_count);
        m = manifest.has_parity ? int(manifest.parity_shards) : 0;
        shard = manifest.has_shard ? manifest.shard_size : manifest.chunk_size;
        if (check == kCheckAlways || (check == kCheckParity && m > 0)) {
            const int rc = mxec_rs_check(k, m);
            if (rc) return set_error(rc, std::string("RS init error: ") + mxec_strerror(rc));
        }
        total = k + m;
        if (int(manifest.chunks.size()) < total) return set_error(MXEC_E_JSON, "JSON error: manifest lists fewer shards than k+m");
        bufs.assign(size_t(total), Bytes());
        ptrs.assign(size_t(total), nullptr);
        present.assign(size_t(total), 0);
        lens.resize(size_t(total));
        for (int i = 0; i < total; ++i) lens[size_t(i)] = want(i);
        return MXEC_OK;
    }

    // The length the digest of shard i covers (:184): a data chunk's real
    // bytes, a parity shard whole.  The kernels read bytes past it as zero,
    // which is Vec::resize(shard_size).
    size_t want(int i) const { return size_t(i < k ? std::min<uint64_t>(man->chunks[size_t(i)].size, shard) : shard); }

    // Shard i lives in someone else's memory, want(i) bytes of it.
    void adopt(int i, uint8_t* p) {
        static uint8_t none;  // a zero-length shard still needs a pointer for the C API
        ptrs[size_t(i)] = p ? p : &none;
        present[size_t(i)] = 1;
    }
    void adopt(int i, Bytes& b) { adopt(i, b.data()); }

    // Shard i from its file; whether it was there at want(i) bytes.  A file
    // of another size cannot match its digest: it is an erasure up front.
    // *there: the file could be read at all.
    bool read(const fs::path& dir, int i, bool* there = nullptr) {
        Bytes& b = bufs[size_t(i)];
        const bool got = read_file(dir / chunk_name(uint32_t(i)), b) == MXEC_OK;
        if (there) *there = got;
        const bool ok = got && b.size() == want(i);
        adopt(i, b);
        present[size_t(i)] = ok;
        return ok;
    }

    // Shard i is an erasure with a buffer of its own for the decode to fill.
    void blank(int i, bool zero) {
        Bytes& b = bufs[size_t(i)];
        if (zero) b.assign(want(i), 0);
        else b.resize(want(i));
        adopt(i, b);
        present[size_t(i)] = 0;
    }

    // ReedSolomon::reconstruct over the set: every erasure (flags 0) or every
    // erased data shard (MXEC_F_DATA_ONLY) rebuilt in place.  With `expected`
    // (total x 32 bytes) present shards are hashed first and one that differs
    // becomes an erasure.
    int decode(mxec_ctx* ctx, const uint8_t* expected, uint32_t flags, int* n_present) {
        return mxec_reconstruct(ctx, k, m, shard, ptrs.data(), lens.data(),
                                reinterpret_cast<const uint8_t(*)[32]>(expected), present.data(), flags, n_present);
    }
};

}  // namespace mxec
