// storage_multipart.cpp — CompleteMultipartUpload as a stream
// (complete_multipart_chunked filesystem.rs:1147-1310 and
// complete_multipart_chunked_encrypted :1315-1560, which hold one I/O buffer,
// one frame and one chunk): mxec_complete_multipart_streamed and
// mxec_complete_multipart_streamed_encrypted of include/maxio_ec.h.  The parts
// go through a chunk writer (storage_writer.cpp) in order and nothing is
// buffered: a plain part in pieces of at most 1 MiB through the writer's host
// path, an encrypted part's frames through the writer's device-side feed,
// which decrypts them in HBM straight into the plaintext ring its encrypt
// launches read.  part_plan.hpp has the arithmetic; the buffered drivers of
// storage_put.cpp are the yardstick for every byte and every error.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstring>

#include "ops.hpp"
#include "part_plan.hpp"
#include "shard_files.hpp"

using namespace mxec;

// The multipart ETag (:1240-1244): MD5 over the parts' raw MD5s, "-N".
int mxec::multipart_etag(mxec_ctx* ctx, const mxec_multipart_part* parts, uint32_t n_parts, char* etag_out) {
    std::vector<uint8_t> md5s(size_t(n_parts) * 16 + 1);
    for (uint32_t p = 0; p < n_parts; ++p) std::memcpy(&md5s[size_t(p) * 16], parts[p].md5, 16);
    mxec_body_sums sums;
    const uint8_t* b = md5s.data();
    const uint64_t l = uint64_t(n_parts) * 16;
    MXEC_TRY(mxec_body_sums_batch(ctx, &b, &l, 1, MXEC_SUM_MD5, &sums));
    std::snprintf(etag_out, 48, "%s-%u", hex(sums.md5, 16).c_str(), n_parts);
    return MXEC_OK;
}

namespace {

int open_error(const char* path) {  // read_file's text
    return set_error(MXEC_E_IO, std::string("IO error: ") + path + ": " + std::strerror(errno));
}

// The part files the feed is reading: opened when a step first needs them and
// closed once the feed has moved past them, so an upload of 10 000 parts holds
// no more descriptors than one launch draws from.
struct PartFiles {
    const mxec_multipart_part* parts = nullptr;
    std::vector<int> fds;
    size_t low = 0;  // every part below is closed for good
    ~PartFiles() { done_below(fds.size()); }
    int get(uint32_t p, int* fd) {
        if (fds[p] < 0) {
            fds[p] = ::open(parts[p].path, O_RDONLY | O_CLOEXEC);
            if (fds[p] < 0) return open_error(parts[p].path);
        }
        *fd = fds[p];
        return MXEC_OK;
    }
    void done_below(size_t p) {
        for (; low < p && low < fds.size(); ++low)
            if (fds[low] >= 0) {
                ::close(fds[low]);
                fds[low] = -1;
            }
    }
};

// Every part file opened and sized, the lengths decided and the checks that
// need no writer made: nothing has been created when this fails.
int open_parts(const mxec_multipart_part* parts, uint32_t n_parts, bool have_key, PartFiles& files,
               std::vector<PartSpec>& specs) {
    files.parts = parts;
    files.fds.assign(n_parts, -1);
    for (uint32_t p = 0; p < n_parts; ++p) {
        const mxec_multipart_part& part = parts[p];
        if (!part.path) return set_error(MXEC_E_INVALID_ARG, "null part path");
        int fd = -1;
        MXEC_TRY(files.get(p, &fd));
        struct stat sb;
        if (::fstat(fd, &sb) != 0) return open_error(part.path);
        ::close(fd);  // the feed opens it again
        files.fds[p] = -1;
        if (!part.encrypted) {
            specs.push_back({uint64_t(sb.st_size), false});
            continue;
        }
        if (!have_key) return set_error(MXEC_E_INVALID_ARG, "encrypted part without upload key");
        uint64_t need = 0;
        if (!frame_stream_len(part.size, &need))
            return set_error(MXEC_E_INVALID_ARG, "part size: the frame stream does not fit in 64 bits");
        if (uint64_t(sb.st_size) < need) return set_error(MXEC_E_INTEGRITY, "truncated encrypted frame");
        specs.push_back({part.size, true});
    }
    return MXEC_OK;
}

// A writer that is closed on every path.
struct WriterHandle {
    void* w = nullptr;
    ~WriterHandle() {
        if (w) mxec_writer_close(w);
    }
};

// Plain bytes [off, off + len) of a part file, len <= kFeedPiece, to the writer.
int push_plain(void* w, int fd, const char* path, uint64_t off, uint64_t len, std::vector<uint8_t>& buf) {
    buf.resize(size_t(kFeedPiece));
    uint64_t got = 0;
    while (got < len) {
        const ssize_t n = ::pread(fd, buf.data() + got, size_t(len - got), off_t(off + got));
        if (n < 0 && errno == EINTR) continue;
        // fewer bytes than the file's size said
        if (n <= 0) return set_error(MXEC_E_IO, std::string("IO error: read failed for ") + path);
        got += uint64_t(n);
    }
    return mxec_writer_write(w, buf.data(), len);
}

}  // namespace

extern "C" {

int mxec_complete_multipart_streamed(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size, uint32_t parity_shards,
                                     const mxec_multipart_part* parts, uint32_t n_parts, uint64_t window_bytes,
                                     char etag_out[48]) {
    return guarded([&]() -> int {
        if ((n_parts && !parts) || !etag_out || !ec_dir) return set_error(MXEC_E_INVALID_ARG, "null argument");
        for (uint32_t p = 0; p < n_parts; ++p)
            if (parts[p].encrypted) return set_error(MXEC_E_INVALID_ARG, "encrypted part: use the _encrypted driver");
        PartFiles files;
        std::vector<PartSpec> specs;
        MXEC_TRY(open_parts(parts, n_parts, false, files, specs));
        const PartPlan plan = part_plan(specs.data(), specs.size(), 1);  // no ring: the lengths only
        if (plan.parts.size() != specs.size()) return set_error(MXEC_E_INVALID_ARG, "the parts' sizes do not fit in 64 bits");
        WriterHandle h;
        MXEC_TRY(mxec_writer_open(ctx, ec_dir, chunk_size, parity_shards, plan.body_len, UINT64_MAX, window_bytes, &h.w));
        std::vector<uint8_t> buf;
        for (uint32_t p = 0; p < n_parts; ++p) {
            for (uint64_t off = 0; off < specs[p].size; off += kFeedPiece) {
                int fd = -1;
                MXEC_TRY(files.get(p, &fd));
                MXEC_TRY(push_plain(h.w, fd, parts[p].path, off, std::min(kFeedPiece, specs[p].size - off), buf));
            }
            files.done_below(size_t(p) + 1);
        }
        MXEC_TRY(mxec_writer_finish(h.w));
        return multipart_etag(ctx, parts, n_parts, etag_out);
    });
}

int mxec_complete_multipart_streamed_encrypted(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size,
                                               uint32_t parity_shards, const mxec_multipart_part* parts,
                                               uint32_t n_parts, const uint8_t upload_key[32], const char* upload_id,
                                               const uint8_t key[32], const uint8_t nonce_prefix[4],
                                               const uint8_t* aad_prefix, uint32_t aad_prefix_len,
                                               uint64_t window_bytes, char etag_out[48]) {
    return guarded([&]() -> int {
        if ((n_parts && !parts) || !etag_out || !ec_dir || !key || !nonce_prefix || (aad_prefix_len && !aad_prefix))
            return set_error(MXEC_E_INVALID_ARG, "null argument");
        PartFiles files;
        std::vector<PartSpec> specs;
        MXEC_TRY(open_parts(parts, n_parts, upload_key && upload_id, files, specs));
        uint64_t body = 0;
        for (const PartSpec& s : specs) {
            if (s.size > UINT64_MAX - body) return set_error(MXEC_E_INVALID_ARG, "the parts' sizes do not fit in 64 bits");
            body += s.size;
        }
        const PartPlan plan = part_plan(specs.data(), specs.size(), writer_ring_bytes(body));
        if (!plan.ok) return set_error(MXEC_E_INVALID_ARG, "the parts' sizes do not fit in 64 bits");
        WriterHandle h;
        MXEC_TRY(mxec_writer_open_encrypted(ctx, ec_dir, chunk_size, parity_shards, plan.body_len, key, nonce_prefix,
                                            aad_prefix, aad_prefix_len, window_bytes, 0, &h.w));
        bool any_enc = false;
        for (const PartSpec& s : specs) any_enc = any_enc || (s.encrypted && s.size);
        if (any_enc) MXEC_TRY(writer_feed_key(h.w, upload_key, upload_id));
        std::vector<uint8_t> buf;
        MXEC_TRY(part_feed(plan, [&](const FeedStep& s) -> int {
            int fd = -1;
            if (!s.launch) {
                files.done_below(s.part);
                MXEC_TRY(files.get(s.part, &fd));
                return push_plain(h.w, fd, parts[s.part].path, s.part_off, s.len, buf);
            }
            files.done_below(s.jobs[0].part);
            WriterFeedSrc src[kFeedFrames];
            for (uint32_t j = 0; j < s.n_jobs; ++j) {
                const uint32_t p = s.jobs[j].part;
                MXEC_TRY(files.get(p, &fd));
                src[j] = WriterFeedSrc{fd, parts[p].path, parts[p].part_number};
            }
            return writer_feed_frames(h.w, s, src);
        }));
        MXEC_TRY(mxec_writer_finish(h.w));
        return multipart_etag(ctx, parts, n_parts, etag_out);
    });
}

}  // extern "C"
