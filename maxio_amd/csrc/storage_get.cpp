// storage_get.cpp — the read side at the file level: MaxIO's
// VerifiedChunkReader (chunk_reader.rs:12-276, ranges :52-82) as a streaming
// reader and as a one-shot GET into the caller's buffer, plain and
// encrypt-then-EC.  A GET verifies every chunk of a range in one batch where
// the reference hashes chunk by chunk.
#include <algorithm>
#include <cstring>
#include <memory>

#include "chunk_reader.hpp"
#include "ops.hpp"
#include "shard_set.hpp"

using namespace mxec;

namespace {

// load_chunk_sync (:87-152) for chunks [first, last]: read, size check, one
// batched digest pass; with parity every bad chunk is rebuilt in one decode
// (:130-150), without parity a bad chunk carries its original error.
//
// The reference rebuilds a bad chunk with try_reconstruct_data_chunk, which
// re-reads and re-hashes every shard (:157-226), once per bad chunk.  Here:
// when a chunk of the range is already known bad before hashing (its file is
// missing or has the wrong size), every other shard is read up front and
// hashed in the SAME pass as the range; a chunk that only fails its digest
// costs one more pass over the shards not yet hashed.  Either way each shard
// is hashed once and every bad chunk of the range comes out of one decode.
struct RangeLoad {
    mxec_ctx* ctx;
    const fs::path& dir;
    const Manifest& man;
    const uint32_t first, last;
    std::vector<LoadedChunk>& out;  // one per chunk of the range; dst set by the caller
    ShardSet set;                   // holds the shards outside the range
    // Shards outside the range: read at the length the digest covers (:184)
    // and not failed since / digest matched.
    std::vector<uint8_t> loaded, verified;
    bool extra_read = false;

    bool in_range(size_t i) const { return i >= first && i <= last; }

    // The range's chunks from their files; whether one is bad already.
    bool read_range() {
        bool known_bad = false;
        for (uint32_t idx = first; idx <= last; ++idx) {
            LoadedChunk& lc = out[idx - first];
            const uint64_t size = man.chunks[idx].size;
            const int rc = lc.dst ? read_file_to(dir / chunk_name(idx), lc.dst, size, &lc.dst_size)
                                  : read_file(dir / chunk_name(idx), lc.data);
            if (rc != MXEC_OK)
                lc.fail(MXEC_E_IO, "failed to read chunk " + std::to_string(idx) + ": " + last_error());
            else if (lc.size() != size)
                lc.fail(MXEC_E_INTEGRITY, "chunk " + std::to_string(idx) + " size mismatch: expected " +
                                              std::to_string(size) + ", got " + std::to_string(lc.size()));
            known_bad = known_bad || lc.err;
        }
        return known_bad;
    }

    void read_extra() {
        extra_read = true;
        for (int i = 0; i < set.total; ++i)
            if (!in_range(size_t(i))) loaded[size_t(i)] = set.read(dir, i);
    }

    // One digest pass over everything loaded and not yet hashed: the good
    // chunks of the range (range = true) and the shards outside it.
    int hash_pass(bool range) {
        std::vector<const uint8_t*> hp;
        std::vector<size_t> hl, who;
        for (uint32_t idx = first; range && idx <= last; ++idx)
            if (const LoadedChunk& lc = out[idx - first]; !lc.err) {
                hp.push_back(lc.ptr());
                hl.push_back(lc.size());
                who.push_back(idx);
            }
        for (size_t i = 0; i < loaded.size(); ++i)
            if (loaded[i] && !verified[i]) {
                hp.push_back(set.ptrs[i]);
                hl.push_back(set.lens[i]);
                who.push_back(i);
            }
        if (hp.empty()) return MXEC_OK;
        std::vector<uint8_t> dig(hp.size() * 32);
        MXEC_TRY(mxec_sha256_batch(ctx, hp.data(), hl.data(), hp.size(), reinterpret_cast<uint8_t(*)[32]>(dig.data())));
        for (size_t t = 0; t < who.size(); ++t) {
            const size_t i = who[t];
            const std::string got = hex(&dig[t * 32], 32);
            const bool ok = got == man.chunks[i].sha256;
            if (!in_range(i))
                loaded[i] = verified[i] = ok;  // a failed shard is an erasure, not hashed again
            else if (!ok)
                out[i - first].fail(MXEC_E_INTEGRITY, "checksum mismatch on chunk " + std::to_string(i) +
                                                          ": expected " + man.chunks[i].sha256 + ", got " + got);
        }
        return MXEC_OK;
    }

    // try_reconstruct_data_chunk (:157-226) over every shard at once.
    // Present shards are passed in place (the decode only reads them);
    // missing ones get uninitialised buffers the decode overwrites whole, a
    // chunk bound for the caller's buffer is rebuilt there.  verify = true:
    // the shards are not hashed yet, so mxec_reconstruct hashes every present
    // one against the manifest in the same upload (a mismatch is one more
    // erasure) -- one upload, one hash launch, one decode for a range with a
    // known-bad chunk.  Returns MXEC_OK with every range chunk good or
    // carrying its error; with verify, 1 when too few shards verified (the
    // caller then finds out chunk by chunk).
    int decode(bool verify) {
        std::vector<uint8_t> expected(verify ? size_t(set.total) * 32 : 0);
        for (int i = 0; i < set.total; ++i) {
            bool have = false;
            if (in_range(size_t(i))) {
                LoadedChunk& lc = out[size_t(i) - first];
                have = !lc.err;
                if (lc.dst) set.adopt(i, lc.dst);  // exactly chunks[i].size == want(i) bytes
                else if (have) set.adopt(i, lc.data);
                else set.blank(i, false);
            } else {
                have = loaded[size_t(i)];  // then where read_extra put it
                if (!have) set.blank(i, false);
            }
            // As hash_pass compares, and chunk_reader.rs:108-109, :184-185: the
            // lower-case hex string.  Any other digest never matches.
            if (have && verify && !manifest_digest32(man.chunks[size_t(i)].sha256, &expected[size_t(i) * 32]))
                have = false;
            set.present[size_t(i)] = have;
        }
        int np = 0;
        const int rc = set.decode(ctx, verify ? expected.data() : nullptr, MXEC_F_DATA_ONLY, &np);
        if (verify && rc == MXEC_E_TOO_FEW_SHARDS_PRESENT) return 1;
        const std::string msg = rc ? std::string(last_error()) : std::string();
        for (uint32_t idx = first; idx <= last; ++idx) {
            LoadedChunk& lc = out[idx - first];
            if (!lc.err) continue;  // good, or (verify) rebuilt in place after a mismatch
            if (rc) {
                lc.fail(rc, msg);
                continue;
            }
            if (lc.dst) lc.dst_size = set.want(int(idx));
            else lc.data.swap(set.bufs[idx]);  // want(idx) bytes, rebuilt
            lc.err = MXEC_OK;
            lc.msg.clear();
        }
        return MXEC_OK;
    }

    int run() {
        MXEC_TRY(set.open(man, ShardSet::kNoCheck));
        loaded.assign(size_t(set.total), 0);
        verified.assign(size_t(set.total), 0);
        const bool parity = set.m > 0;
        if (read_range() && parity) {
            read_extra();
            const int rc = decode(true);
            if (rc <= 0) return rc;
            // Too few shards verified: hash shard by shard to give each range
            // chunk its own error (or rebuild from what did verify).
        }
        MXEC_TRY(hash_pass(true));
        const bool bad = std::any_of(out.begin(), out.end(), [](const LoadedChunk& lc) { return lc.err != 0; });
        if (!parity || !bad) return MXEC_OK;
        if (!extra_read) {
            read_extra();
            MXEC_TRY(hash_pass(false));
        }
        return decode(false);
    }
};

// Bytes served from a chunk of `size` bytes from offset `from` on, `left` still wanted.
uint64_t served(uint64_t size, uint64_t from, uint64_t left) { return std::min(size > from ? size - from : 0, left); }

}  // namespace

// chunk_reader.hpp declares it: the encrypted reader's degraded path is this one.
int mxec::load_chunks(mxec_ctx* ctx, const fs::path& dir, const Manifest& man, uint32_t first, uint32_t last,
                      std::vector<LoadedChunk>& out, uint8_t* const* dsts) {
    out.assign(last - first + 1, LoadedChunk{});
    for (size_t c = 0; dsts && c < out.size(); ++c) out[c].dst = dsts[c];
    return RangeLoad{ctx, dir, man, first, last, out, {}, {}, {}, false}.run();
}

extern "C" {

int mxec_reader_open(mxec_ctx* ctx, const char* ec_dir, uint64_t offset, uint64_t length, uint64_t batch_bytes,
                     mxec_reader** out) {
    return guarded([&]() -> int {
        if (!ec_dir || !out) return set_error(MXEC_E_INVALID_ARG, "null argument");
        *out = nullptr;
        auto r = std::make_unique<mxec_reader>();
        MXEC_TRY(read_manifest(ec_dir, r->man));
        r->ctx = ctx;
        r->dir = ec_dir;
        r->batch_bytes = batch_bytes ? batch_bytes : (uint64_t(64) << 20);
        const Manifest& man = r->man;
        if (length == UINT64_MAX) length = offset < man.total_size ? man.total_size - offset : 0;
        if (offset + length > man.total_size) length = man.total_size > offset ? man.total_size - offset : 0;
        if (length > 0 && man.total_size > 0) {  // else Done at once (:40, :53-65)
            if (man.chunk_size == 0) return set_error(MXEC_E_JSON, "JSON error: chunk_size is 0");
            r->next = uint32_t(offset / man.chunk_size);
            r->end = uint32_t((offset + length - 1) / man.chunk_size);
            r->skip = offset % man.chunk_size;
            if (r->end >= man.chunk_count || r->end >= man.chunks.size())
                return set_error(MXEC_E_JSON, "JSON error: range past chunk_count");
            r->remaining = length;
        }
        *out = r.release();
        return MXEC_OK;
    });
}

int64_t mxec_reader_read(mxec_reader* r, uint8_t* buf, uint64_t cap) {
    return guarded([&]() -> int64_t {
        if (!r || (cap && !buf)) return set_error(MXEC_E_INVALID_ARG, "null argument");
        if (r->enc) return enc_reader_read(*r->enc, buf, cap);
        uint64_t copied = 0;
        while (copied < cap && r->remaining > 0) {
            if (r->bi >= r->batch.size()) {
                // NeedLoad: the next chunks up to batch_bytes (at least one)
                uint32_t last = r->next;
                uint64_t bytes = r->man.chunks[r->next].size;
                while (last < r->end && bytes + r->man.chunks[last + 1].size <= r->batch_bytes)
                    bytes += r->man.chunks[++last].size;
                const int rc = load_chunks(r->ctx, r->dir, r->man, r->next, last, r->batch);
                if (rc) return copied ? int64_t(copied) : int64_t(rc);
                r->next = last + 1;
                r->bi = 0;
                r->pos = r->skip;  // skip applies to the first chunk of the range only
                r->skip = 0;
            }
            LoadedChunk& c = r->batch[r->bi];
            if (c.err) {  // serve everything before it first, as the reference streams
                if (copied) return int64_t(copied);
                return set_error(c.err, c.msg);
            }
            const uint64_t take = served(c.data.size(), r->pos, std::min(cap - copied, r->remaining));
            if (take) std::memcpy(buf + copied, c.data.data() + r->pos, take);
            copied += take;
            r->pos += take;
            r->remaining -= take;
            if (r->pos >= c.data.size()) {
                c.data = Bytes();
                ++r->bi;
                r->pos = 0;
            }
        }
        return int64_t(copied);
    });
}

void mxec_reader_close(mxec_reader* r) { delete r; }

int mxec_get_object_chunked(mxec_ctx* ctx, const char* ec_dir, uint64_t offset, uint64_t length, uint8_t* out,
                            uint64_t out_cap, uint64_t* out_len) {
    return guarded([&]() -> int {
        if (!ec_dir || !out_len) return set_error(MXEC_E_INVALID_ARG, "null argument");
        *out_len = 0;
        // The reader's semantics (mxec_reader_open / _read over the whole range
        // in one batch), with every chunk the range covers whole read straight
        // into its place in `out`: no intermediate chunk buffer, no copy out.
        mxec_reader* r = nullptr;
        MXEC_TRY(mxec_reader_open(ctx, ec_dir, offset, length, uint64_t(1) << 40, &r));
        std::unique_ptr<mxec_reader, void (*)(mxec_reader*)> guard(r, mxec_reader_close);
        if (r->remaining > out_cap || (r->remaining && !out))
            return set_error(MXEC_E_INVALID_ARG, "output buffer too small");
        if (r->remaining == 0) return MXEC_OK;
        const Manifest& man = r->man;
        const uint32_t first = r->next, last = r->end;
        // Where each chunk's bytes are served: the first from `skip`, the rest
        // whole, in order, until `remaining` runs out (mxec_reader_read).
        auto from = [&](uint32_t c) { return c == first ? r->skip : uint64_t(0); };
        std::vector<uint8_t*> dsts(last - first + 1, nullptr);
        uint64_t pos = 0, left = r->remaining;
        for (uint32_t c = first; c <= last && left; ++c) {
            const uint64_t sz = man.chunks[c].size;
            const uint64_t take = served(sz, from(c), left);
            if (take == sz && sz > 0) dsts[c - first] = out + pos;
            pos += take;
            left -= take;
        }
        // Windows of at most kGetWindow bytes of chunks (at least one chunk): one
        // hash round trip per window, and a slot's device staging stays bounded
        // however large the object.
        // MXEC_GET_WINDOW (bytes, read at mxec_open) overrides the window (tests).
        const uint64_t kGetWindow = ctx->c.knobs.get_window;
        std::vector<LoadedChunk> batch;
        uint64_t& done = *out_len;  // the bytes served, also before an error
        left = r->remaining;
        for (uint32_t w0 = first; w0 <= last && left;) {
            uint32_t w1 = w0;
            uint64_t bytes = man.chunks[w0].size;
            while (w1 < last && bytes + man.chunks[w1 + 1].size <= kGetWindow) bytes += man.chunks[++w1].size;
            MXEC_TRY(load_chunks(ctx, r->dir, man, w0, w1, batch, &dsts[w0 - first]));
            for (uint32_t c = w0; c <= w1 && left; ++c) {
                const LoadedChunk& lc = batch[c - w0];
                if (lc.err) return set_error(lc.err, lc.msg);  // after the bytes before it (reader semantics)
                const uint64_t take = served(lc.size(), from(c), left);
                if (!lc.dst && take) std::memcpy(out + done, lc.data.data() + from(c), take);
                done += take;
                left -= take;
            }
            w0 = w1 + 1;
        }
        return MXEC_OK;
    });
}

int mxec_get_object_chunked_encrypted(mxec_ctx* ctx, const char* ec_dir, const uint8_t key[32],
                                      const uint8_t* aad_prefix, uint32_t aad_prefix_len, uint32_t frame_size,
                                      uint64_t plaintext_size, uint64_t offset, uint64_t length, uint8_t* out,
                                      uint64_t out_cap, uint64_t* out_len) {
    return guarded([&]() -> int {
        if (!ec_dir || !key || !out_len || (aad_prefix_len && !aad_prefix))
            return set_error(MXEC_E_INVALID_ARG, "null argument");
        if (frame_size == 0 || frame_size % 16) return set_error(MXEC_E_INVALID_ARG, "frame_size must be a positive multiple of 16");
        *out_len = 0;
        Manifest man;
        MXEC_TRY(read_manifest(ec_dir, man));
        if (plaintext_size == UINT64_MAX) {
            if (!man.has_plain) return set_error(MXEC_E_JSON, "JSON error: manifest has no plaintext_size");
            plaintext_size = man.plaintext_size;
        }
        if (offset >= plaintext_size || length == 0) return MXEC_OK;
        const uint64_t end = length == UINT64_MAX || length > plaintext_size - offset ? plaintext_size : offset + length;
        // FrameDecryptor::ciphertext_offset / for_range: the frames that cover
        // [offset, end), read through the verified chunk reader (with_range).
        const uint64_t fl = uint64_t(frame_size) + MXEC_FRAME_OVERHEAD;
        const uint64_t f0 = offset / frame_size, f1 = (end - 1) / frame_size;
        const uint64_t ct_off = f0 * fl;
        const uint64_t ct_len = std::min<uint64_t>(man.total_size - std::min(man.total_size, ct_off), (f1 - f0 + 1) * fl);
        if (end - offset > out_cap || !out) return set_error(MXEC_E_INVALID_ARG, "output buffer too small");
        Bytes ct(size_t(ct_len) + 1);  // every byte written by the GET below
        uint64_t got = 0;
        MXEC_TRY(mxec_get_object_chunked(ctx, ec_dir, ct_off, ct_len, ct.data(), ct_len, &got));
        const uint64_t nf = f1 - f0 + 1;
        const uint64_t pt_lo = f0 * frame_size, pt_hi = std::min<uint64_t>(plaintext_size, (f1 + 1) * uint64_t(frame_size));
        std::vector<uint8_t> aads(size_t(nf) * 32);
        MXEC_TRY(mxec_frame_aads(ctx, aad_prefix, aad_prefix_len, f0, nf, reinterpret_cast<uint8_t(*)[32]>(aads.data())));
        uint64_t n = 0;
        if (offset == pt_lo && end == pt_hi) {
            // The range is whole frames (a full GET): decrypt straight into out.
            MXEC_TRY(mxec_frames_decrypt(ctx, key, f0, aads.data(), 32, frame_size, ct.data(), got, pt_hi - pt_lo,
                                         out, out_cap, &n));
        } else {
            Bytes pt(size_t(pt_hi - pt_lo) + 1);
            MXEC_TRY(mxec_frames_decrypt(ctx, key, f0, aads.data(), 32, frame_size, ct.data(), got, pt_hi - pt_lo,
                                         pt.data(), pt.size(), &n));
            std::memcpy(out, pt.data() + (offset - pt_lo), size_t(end - offset));
        }
        *out_len = end - offset;
        return MXEC_OK;
    });
}

}  // extern "C"
