// chunk_reader.hpp — what the two pull-stream readers share: the handle
// behind mxec_reader_* (storage_get.cpp), the host path that loads, verifies
// and repairs a range of chunks (load_chunks, storage_get.cpp), and the
// encrypted reader's state behind the same handle (storage_reader_enc.cpp).
#pragma once

#include <string>
#include <vector>

#include "runtime.hpp"
#include "shard_files.hpp"

namespace mxec {

struct LoadedChunk {
    Bytes data;
    // When set, the chunk's bytes go straight to this caller buffer of
    // exactly the manifest's size instead of `data` (one-shot GET: the chunk
    // lands where it is served, no intermediate copy).
    uint8_t* dst = nullptr;
    uint64_t dst_size = 0;  // the file's size as read into dst
    int err = MXEC_OK;  // non-zero: this chunk fails the read that reaches it
    std::string msg;
    const uint8_t* ptr() const { return dst ? dst : data.data(); }
    uint64_t size() const { return dst ? dst_size : data.size(); }
    void fail(int code, const std::string& why) {
        err = code;
        msg = why;
    }
};

// Chunks [first, last] of the object into `out`, verified against the
// manifest, the bad ones rebuilt in one decode when it has parity; `dsts`
// (optional, one per chunk, nullptr = none) places chunks in caller memory
// (LoadedChunk::dst).
int load_chunks(mxec_ctx* ctx, const fs::path& dir, const Manifest& man, uint32_t first, uint32_t last,
                std::vector<LoadedChunk>& out, uint8_t* const* dsts = nullptr);

// The encrypted reader (mxec_reader_open_encrypted): its read and its end.
struct EncReader;
int64_t enc_reader_read(EncReader& e, uint8_t* buf, uint64_t cap);
void enc_reader_free(EncReader* e);

}  // namespace mxec

struct mxec_reader {
    mxec_ctx* ctx = nullptr;
    mxec::fs::path dir;
    mxec::Manifest man;
    uint32_t next = 0, end = 0;  // next chunk to load, last chunk of the range
    uint64_t skip = 0, remaining = 0, batch_bytes = 0;
    std::vector<mxec::LoadedChunk> batch;
    size_t bi = 0;
    uint64_t pos = 0;
    mxec::EncReader* enc = nullptr;  // set: an encrypted reader, which uses ctx, dir and man only
    ~mxec_reader() { mxec::enc_reader_free(enc); }
};
