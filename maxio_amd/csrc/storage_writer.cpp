// storage_writer.cpp — put_object_chunked (filesystem.rs:686-773) as a push
// stream: mxec_writer_open / _write / _finish / _close of include/maxio_ec.h.
// The body arrives in pieces of any size; each byte goes to its chunk's file
// and to the chunk's slot of a bounded HBM window, a completed chunk is hashed
// there and folded into the running parity (mxec_encode_update_strided_device,
// count = 1, ping-ponging between two sets of m rows), and finish() writes
// the parity files and manifest.json.  The arithmetic is writer_plan.hpp's.
//
// Streams: uploads and parity passes run in order on the writer's own stream,
// created at the highest priority so that this short work does not queue
// behind a hash chain on a shared hardware queue; a chunk's SHA-256 runs on
// its window slot's stream behind the chunk's last upload, so the ~55 MB/s
// hash chains of consecutive chunks overlap each other and the uploads.  The
// last chunk's chain and the m parity rows' share one launch (behind the last
// fold): side by side they take one chain's time, not two.  A slot is reused
// once its chunk's hash and parity pass have finished -- the only device wait
// inside write().
//
// Body digests (mxec_writer_open_sums): the Md5 and ChecksumHasher of the
// reference's loop (filesystem.rs:700-725) advance on one more stream, in
// runs of at most 1 MiB over bytes already in the window, each queued behind
// its last byte's upload (run_body_sums' update form; the chains' state stays
// in HBM between runs, so nothing waits between them).  A slot's reuse then
// also waits for its chunk's last run.
//
// The encrypted writer (mxec_writer_open_encrypted; put_object_chunked_encrypted
// filesystem.rs:835-1060, frames of crypto.rs:94-117): the caller writes
// plaintext, which goes up into a ring of kRingRuns stretches of 1 MiB, not
// into the window.  With a stretch's last byte (or the body's) one launch of
// the GCM kernel's window form encrypts its 16 frames straight into the chunk
// slots (frame_plan.hpp has the arithmetic), on the main stream behind the
// upload, under key tables prepared once at open; its AADs are hashed on the
// host and go up in front of it.  The ciphertext comes down on a stream of its
// own through two more staging pieces and goes to the chunk files one or two
// pieces later; a chunk the launch completes takes complete() as ever.  The
// body digests run over the plaintext ring, one run per stretch.  A stretch is
// reused once its launch and its digest run have finished, a slot once its
// chunk's hash, fold and download have.
//
// The device-side feed (writer_feed_key / writer_feed_frames, ops.hpp; the
// streaming CompleteMultipartUpload of storage_multipart.cpp): the frames of
// encrypted multipart parts, 16 at a time (part_plan.hpp's launches), are read
// from the part files into one of two page-locked pieces, go up into one of
// two stretches of a ciphertext bounce, and one launch of the GCM kernel's
// ring form on the main stream decrypts them under the upload key straight
// into the plaintext ring at the body offset; `written` advances and the
// encrypt launches that are then due follow in stream order, exactly as after
// an upload.  A stretch of the ring is waited for as enc_write waits for it.
// The frame statuses come down behind each launch and are checked no later
// than the next reuse of their bounce stretch, all of them in finish() before
// a parity file or the manifest is written.
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <cstring>

#include "frame_plan.hpp"
#include "kernels.hpp"
#include "part_plan.hpp"
#include "ops.hpp"
#include "sha256_host.hpp"
#include "shard_files.hpp"
#include "writer_plan.hpp"

using namespace mxec;

namespace {

constexpr uint64_t kPiece = uint64_t(1) << 20;  // bytes per staging piece (at most)
constexpr int kPieces = 2;                      // page-locked staging pieces per writer

struct WindowSlot {
    hipStream_t hash = nullptr;     // the chunk's SHA-256 and its digest's way down
    hipEvent_t hashed = nullptr;    // ... finished
    hipEvent_t folded = nullptr;    // the chunk's parity pass on the main stream finished
    uint64_t chunk = UINT64_MAX;    // the chunk whose digest has not been collected yet
    uint64_t dig_at = 0;            // ... and its entry in the digest landing zone
    // With body digests: the chunk's last run on the digest stream finished,
    // and the launch tables of its runs (free again once it has).
    hipEvent_t summed = nullptr;
    DescArena sum_tables;
};

// Table bytes one digest run takes (pointers, CRC tile map and scratch of at
// most kSumRun bytes; the arena chains a block should one take more).
constexpr size_t kSumRunTables = 512;

constexpr int kRingRuns = 4;    // plaintext stretches (kEncRun each) resident in HBM
constexpr int kDownPieces = 2;  // page-locked pieces for ciphertext on its way down

struct RingRun {
    hipEvent_t encrypted = nullptr;  // the stretch's encrypt launch finished
    hipEvent_t summed = nullptr;     // ... and its digest run (with body digests)
    bool busy = false, sum_busy = false;
    DescArena sum_tables, enc_tables;  // the launches' tables: free again with the events above
};
// A stretch of the frame stream, at most kPiece, between its slots and the chunk files.
struct DownPiece {
    PinnedBuf buf;
    hipEvent_t landed = nullptr;
    uint64_t off = 0, len = 0;
};
// The plaintext ring's bytes for a body: the whole of a body within one
// stretch, else one stretch per MiB up to kRingRuns.
uint64_t ring_bytes_for(uint64_t plain_len) {
    const uint64_t runs = std::min<uint64_t>(kRingRuns, enc_run_count(plain_len));
    return runs <= 1 ? std::max<uint64_t>(plain_len, 256) : runs * kEncRun;
}

// One launch of the device-side feed in flight: its part frames on the host,
// its statuses, and what a failed frame's message needs.
constexpr int kFeedBounces = 2;
struct FeedBounce {
    PinnedBuf ct, st;           // the frames, job after job | their statuses, landed
    hipEvent_t done = nullptr;  // ... behind the launch on the main stream
    bool busy = false;
    DescArena tables;
    uint32_t frames = 0;
    uint64_t expect[kFeedFrames];  // each frame's index in its part
    uint64_t hdr_at[kFeedFrames];  // ... and where its stored nonce lies in ct
};
struct FeedState {
    uint8_t key[32];
    GcmKey tables;  // the host copy of what key_dev holds
    DevBuf key_dev;
    std::string aad_prefix;         // "PART" 0 upload_id 0 (part_aad_builder, filesystem.rs:147-163)
    uint64_t ring_bytes = 0;
    DevBuf ct_dev, aad_dev, st_dev;  // kFeedBounces * (kEncRunStream | kFeedFrames * 32 | kFeedFrames * 4)
    PinnedBuf aad_host;
    FeedBounce b[kFeedBounces];
    uint64_t next = 0;
    ~FeedState() {  // the upload key does not outlive the writer on the host
        explicit_bzero(key, sizeof key);
        explicit_bzero(&tables, sizeof tables);
    }
};

struct EncState {
    uint64_t plain_len = 0;
    WriterPlan pplan;  // the plaintext as one body: the over-run and short-finish texts are in its bytes
    uint8_t key[32];
    uint8_t prefix[4];
    GcmKey tables;     // the host copy of what key_dev holds
    DevBuf key_dev;
    std::vector<uint8_t> aad_msg;  // aad_prefix, then room for the index
    DevBuf ring, aad_dev;          // kRingRuns * kEncRun | kRingRuns * kEncFrames * 32
    PinnedBuf aad_host;
    RingRun runs[kRingRuns];
    hipStream_t down_s = nullptr;
    DownPiece down[kDownPieces];
    uint64_t down_head = 0, down_next = 0;  // pieces gone to their files | queued
    uint64_t filed = 0;                     // stream bytes in the chunk files
    std::unique_ptr<FeedState> feed;        // writer_feed_key; null otherwise

    uint8_t* ring_ptr(uint64_t run) const { return static_cast<uint8_t*>(ring.p) + (run % kRingRuns) * kEncRun; }
    size_t aad_at(uint64_t run) const { return size_t(run % kRingRuns) * kEncFrames * 32; }
    ~EncState() {  // neither key outlives the writer on the host
        explicit_bzero(key, sizeof key);
        explicit_bzero(&tables, sizeof tables);
    }
};

}  // namespace

struct mxec_writer {
    mxec_ctx* ctx = nullptr;
    Device* dev = nullptr;
    int dev_index = 0;
    fs::path dir;
    WriterPlan plan;
    uint32_t m = 0;  // parity rows (0: none, version 1)
    bool has_plain = false;
    uint64_t plaintext_size = 0;
    uint64_t written = 0;
    uint64_t sa = 0;  // bytes between slots and between parity rows on the device
    bool finished = false;
    int err = 0;  // poisoned: every later call returns this
    std::string err_msg;

    hipStream_t s = nullptr;
    hipEvent_t uploaded = nullptr;  // a chunk's last upload: its hash stream waits for it
    DevBuf window, parity, dig;     // slots * sa | 2 * m * sa | (slots + 1 + m) * 32: a digest per slot,
                                    //   then the last chunk's and the m parity rows' (one launch)
    int cur = -1;                   // which parity set holds the running parity (-1: none yet)
    PinnedBuf stage[kPieces], hdig;  // hdig: dig's landing zone
    hipEvent_t staged[kPieces] = {nullptr, nullptr};
    bool stage_busy[kPieces] = {false, false};
    int next_stage = 0;
    std::vector<WindowSlot> slots;
    std::vector<std::string> sha;  // the manifest's entries: k data digests, then m parity
    int fd = -1;                   // the open chunk file

    // Body digests (mxec_writer_open_sums; which == 0: none of this exists).
    uint32_t which = 0;
    hipStream_t sum_s = nullptr;    // the digest runs, in body order
    hipEvent_t sums_done = nullptr;  // the last run and the record's way down
    DevBuf sum_state;               // the body's state record, then its mxec_body_sums
    PinnedBuf hsums;                // ... landed
    mxec_body_sums sums{};          // after finish()
    uint8_t* sums_out_dev() const { return static_cast<uint8_t*>(sum_state.p) + MXEC_SUMS_STATE_BYTES; }

    std::unique_ptr<EncState> enc;  // mxec_writer_open_encrypted; null otherwise

    uint8_t* slot_ptr(uint64_t slot) const { return static_cast<uint8_t*>(window.p) + slot * sa; }
    uint8_t* parity_set(int which) const { return static_cast<uint8_t*>(parity.p) + uint64_t(which) * m * sa; }

    ~mxec_writer() {
        if (fd >= 0) ::close(fd);
        if (!dev) return;
        (void)hipSetDevice(dev->id);
        // Nothing of ours may still run when the buffers go.
        if (s) (void)hipStreamSynchronize(s);
        if (sum_s) (void)hipStreamSynchronize(sum_s);
        if (enc && enc->down_s) (void)hipStreamSynchronize(enc->down_s);
        for (WindowSlot& w : slots)
            if (w.hash) (void)hipStreamSynchronize(w.hash);
        // The parity passes and chunk hashes took their tables from the slots'
        // rings, fenced by events on the streams destroyed below.
        slots_settle(*dev);
        if (sum_s) {
            (void)hipStreamSynchronize(sum_s);
            affinity_untag(sum_s);
            (void)hipStreamDestroy(sum_s);
        }
        if (sums_done) (void)hipEventDestroy(sums_done);
        if (enc) {
            if (enc->down_s) {
                (void)hipStreamSynchronize(enc->down_s);
                affinity_untag(enc->down_s);
                (void)hipStreamDestroy(enc->down_s);
            }
            for (RingRun& r : enc->runs) {
                if (r.encrypted) (void)hipEventDestroy(r.encrypted);
                if (r.summed) (void)hipEventDestroy(r.summed);
            }
            for (DownPiece& p : enc->down)
                if (p.landed) (void)hipEventDestroy(p.landed);
            if (enc->key_dev.p) (void)hipMemset(enc->key_dev.p, 0, sizeof(GcmKey));
            if (enc->feed) {
                for (FeedBounce& fb : enc->feed->b)
                    if (fb.done) (void)hipEventDestroy(fb.done);
                if (enc->feed->key_dev.p) (void)hipMemset(enc->feed->key_dev.p, 0, sizeof(GcmKey));
            }
        }
        for (WindowSlot& w : slots) {
            if (w.summed) (void)hipEventDestroy(w.summed);
            if (w.hash) {
                (void)hipStreamSynchronize(w.hash);
                affinity_untag(w.hash);
                (void)hipStreamDestroy(w.hash);
            }
            if (w.hashed) (void)hipEventDestroy(w.hashed);
            if (w.folded) (void)hipEventDestroy(w.folded);
        }
        for (hipEvent_t e : staged)
            if (e) (void)hipEventDestroy(e);
        if (uploaded) (void)hipEventDestroy(uploaded);
        if (s) {
            affinity_untag(s);
            (void)hipStreamDestroy(s);
        }
    }
};

namespace {

int new_stream(mxec_writer& w, hipStream_t* s, bool urgent = false) {
    int least = 0, greatest = 0;
    if (urgent) MXEC_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    if (urgent) MXEC_HIP(hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest));
    else MXEC_HIP(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    affinity_tag(*s, w.dev);
    return MXEC_OK;
}
int new_event(hipEvent_t* e) {
    MXEC_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming | hipEventBlockingSync));
    return MXEC_OK;
}

int poison(mxec_writer& w, int rc) {
    if (rc && !w.err) {
        w.err = rc;
        w.err_msg = last_error();
    }
    return rc;
}

// The slot's chunk has been hashed and folded: its digest to the manifest.
int collect(mxec_writer& w, uint64_t slot) {
    WindowSlot& ws = w.slots[slot];
    if (ws.chunk == UINT64_MAX) return MXEC_OK;
    MXEC_HIP(hipEventSynchronize(ws.hashed));
    if (w.m) MXEC_HIP(hipEventSynchronize(ws.folded));
    if (w.which && !w.enc) MXEC_HIP(hipEventSynchronize(ws.summed));  // queued before the chunk completed
    w.sha[ws.chunk] = hex(static_cast<const uint8_t*>(w.hdig.p) + ws.dig_at * 32, 32);
    ws.chunk = UINT64_MAX;
    return MXEC_OK;
}

// len bytes to dst on the device through the staging pieces; returns once src is reusable.
int upload(mxec_writer& w, uint8_t* dst, const uint8_t* src, uint64_t len) {
    for (uint64_t off = 0; off < len; off += kPiece) {
        const uint64_t n = std::min(kPiece, len - off);
        const int i = w.next_stage;
        w.next_stage = (i + 1) % kPieces;
        if (w.stage_busy[i]) MXEC_HIP(hipEventSynchronize(w.staged[i]));
        std::memcpy(w.stage[i].p, src + off, size_t(n));
        MXEC_HIP(hipMemcpyAsync(dst + off, w.stage[i].p, size_t(n), hipMemcpyHostToDevice, w.s));
        MXEC_HIP(hipEventRecord(w.staged[i], w.s));
        w.stage_busy[i] = true;
    }
    return MXEC_OK;
}

// Chunk j is whole in its slot (its uploads queued on w.s): fold and hash.
int complete(mxec_writer& w, uint64_t j) {
    const uint64_t slot = w.plan.slot_of(j), len = w.plan.chunk_len(j);
    WindowSlot& ws = w.slots[slot];
    const uint8_t* p = w.slot_ptr(slot);
    if (w.m) {
        // The short last chunk is never padded: it goes in as data_len.
        const int to = w.cur == 0 ? 1 : 0;
        MXEC_TRY(mxec_encode_update_strided_device(w.ctx, w.dev_index, w.s, int(w.plan.k), int(w.m), w.plan.chunk_size,
                                                   1, int(j), 1, p, 0, w.sa, &len,
                                                   w.cur < 0 ? nullptr : w.parity_set(w.cur), 0, w.sa,
                                                   w.parity_set(to), 0, w.sa));
        w.cur = to;
        MXEC_HIP(hipEventRecord(ws.folded, w.s));
    }
    // write_chunk's digest (filesystem.rs:1070) over the resident bytes; with
    // the last chunk, compute_and_write_parity's (:1131) over the rows its
    // fold has just finished, in the same launch.
    const bool last = w.m && j + 1 == w.plan.k;
    std::vector<const uint8_t*> msg{p};
    std::vector<uint64_t> lens{len};
    for (uint32_t i = 0; i < w.m && last; ++i) {
        msg.push_back(w.parity_set(w.cur) + uint64_t(i) * w.sa);
        lens.push_back(w.plan.chunk_size);
    }
    ws.dig_at = last ? w.slots.size() : slot;
    uint8_t* dd = static_cast<uint8_t*>(w.dig.p) + ws.dig_at * 32;
    MXEC_HIP(hipEventRecord(w.uploaded, w.s));
    MXEC_HIP(hipStreamWaitEvent(ws.hash, w.uploaded, 0));
    MXEC_TRY(mxec_sha256_batch_device(w.ctx, w.dev_index, ws.hash, msg.data(), lens.data(), msg.size(), dd));
    MXEC_HIP(hipMemcpyAsync(static_cast<uint8_t*>(w.hdig.p) + ws.dig_at * 32, dd, msg.size() * 32,
                            hipMemcpyDeviceToHost, ws.hash));
    MXEC_HIP(hipEventRecord(ws.hashed, ws.hash));
    ws.chunk = j;
    return MXEC_OK;
}

int open_chunk_file(mxec_writer& w, uint64_t j) {
    const fs::path p = w.dir / chunk_name(uint32_t(j));
    w.fd = ::open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (w.fd < 0) return set_error(MXEC_E_IO, "IO error: cannot create " + p.string() + ": " + std::strerror(errno));
    return MXEC_OK;
}
int write_chunk_bytes(mxec_writer& w, uint64_t j, const uint8_t* p, uint64_t len) {
    while (len) {
        const ssize_t n = ::write(w.fd, p, size_t(len));
        if (n < 0 && errno == EINTR) continue;
        if (n <= 0) return set_error(MXEC_E_IO, "IO error: write failed for " + (w.dir / chunk_name(uint32_t(j))).string());
        p += n;
        len -= uint64_t(n);
    }
    return MXEC_OK;
}
int close_chunk_file(mxec_writer& w, uint64_t j) {
    const int rc = ::close(w.fd);
    w.fd = -1;
    if (rc != 0) return set_error(MXEC_E_IO, "IO error: write failed for " + (w.dir / chunk_name(uint32_t(j))).string());
    return MXEC_OK;
}

// One run of the body digests over bytes whose uploads are queued on w.s:
// the next piece of the body's chains, on the digest stream behind them.
int queue_sum_run(mxec_writer& w, const SumRun& r) {
    const uint64_t slot = w.plan.slot_of(r.chunk);
    WindowSlot& ws = w.slots[slot];
    if (r.at == 0) MXEC_TRY(ws.sum_tables.reserve(size_t(writer_sum_runs_of(w.plan, r.chunk)) * kSumRunTables));
    MXEC_HIP(hipEventRecord(w.uploaded, w.s));
    MXEC_HIP(hipStreamWaitEvent(w.sum_s, w.uploaded, 0));
    {
        DevScope ds;
        MXEC_TRY(ds.open(w.ctx, w.dev_index));
        const SumsUpdate upd{static_cast<uint8_t*>(w.sum_state.p),
                             (r.first ? MXEC_SUMS_F_FIRST : 0u) | (r.last ? MXEC_SUMS_F_FINAL : 0u)};
        MXEC_TRY(run_body_sums(*ds.d, *ds.slot, w.sum_s, {w.slot_ptr(slot) + r.at}, {r.len}, w.which, w.sums_out_dev(),
                               sizeof(mxec_body_sums), &upd, &ws.sum_tables));
    }
    if (r.closes) MXEC_HIP(hipEventRecord(ws.summed, w.sum_s));
    if (!r.last) return MXEC_OK;
    MXEC_HIP(hipMemcpyAsync(w.hsums.p, w.sums_out_dev(), sizeof(mxec_body_sums), hipMemcpyDeviceToHost, w.sum_s));
    MXEC_HIP(hipEventRecord(w.sums_done, w.sum_s));
    return MXEC_OK;
}

int take_run(mxec_writer& w, const WriterRun& r, const uint8_t* buf) {
    const uint64_t slot = w.plan.slot_of(r.chunk);
    if (r.opens) {
        MXEC_TRY(collect(w, slot));  // back-pressure: the slot's last chunk must be done with
        MXEC_TRY(open_chunk_file(w, r.chunk));
    }
    MXEC_TRY(write_chunk_bytes(w, r.chunk, buf + r.src, r.len));
    MXEC_TRY(upload(w, w.slot_ptr(slot) + r.at, buf + r.src, r.len));
    if (w.which)
        MXEC_TRY(writer_sum_due(w.plan, r.chunk, r.at, r.at + r.len, [&](const SumRun& q) { return queue_sum_run(w, q); }));
    if (!r.completes) return MXEC_OK;
    MXEC_TRY(close_chunk_file(w, r.chunk));
    return complete(w, r.chunk);
}

// Parity row i of the running parity to its file, through the staging pieces.
int write_parity_file(mxec_writer& w, uint32_t i) {
    const uint64_t j = w.plan.k + i, size = w.plan.chunk_size;
    const uint8_t* row = w.parity_set(w.cur) + uint64_t(i) * w.sa;
    MXEC_TRY(open_chunk_file(w, j));
    // Piece n + 1 comes down while piece n goes to the file.
    const uint64_t n_pieces = (size + kPiece - 1) / kPiece;
    auto fetch = [&](uint64_t n) -> int {
        const uint64_t off = n * kPiece;
        const int b = int(n % kPieces);
        MXEC_HIP(hipMemcpyAsync(w.stage[b].p, row + off, size_t(std::min(kPiece, size - off)), hipMemcpyDeviceToHost, w.s));
        MXEC_HIP(hipEventRecord(w.staged[b], w.s));
        return MXEC_OK;
    };
    MXEC_TRY(fetch(0));
    for (uint64_t n = 0; n < n_pieces; ++n) {
        if (n + 1 < n_pieces) MXEC_TRY(fetch(n + 1));
        const int b = int(n % kPieces);
        MXEC_HIP(hipEventSynchronize(w.staged[b]));
        MXEC_TRY(write_chunk_bytes(w, j, static_cast<const uint8_t*>(w.stage[b].p), std::min(kPiece, size - n * kPiece)));
    }
    return close_chunk_file(w, j);
}

// ---- the encrypted writer ---------------------------------------------------------------------------

// The oldest piece on its way down, to its chunks' files.
int file_piece(mxec_writer& w) {
    EncState& e = *w.enc;
    DownPiece& p = e.down[e.down_head % kDownPieces];
    MXEC_HIP(hipEventSynchronize(p.landed));
    const uint8_t* bytes = static_cast<const uint8_t*>(p.buf.p);
    MXEC_TRY(writer_cut(w.plan, p.off, p.len, [&](const WriterRun& c) -> int {
        if (c.opens) MXEC_TRY(open_chunk_file(w, c.chunk));
        MXEC_TRY(write_chunk_bytes(w, c.chunk, bytes + c.src, c.len));
        return c.completes ? close_chunk_file(w, c.chunk) : MXEC_OK;
    }));
    e.filed = p.off + p.len;
    ++e.down_head;
    return MXEC_OK;
}
// Every queued piece that holds stream bytes below `upto`, to the files.
int file_until(mxec_writer& w, uint64_t upto) {
    while (w.enc->filed < upto && w.enc->down_head < w.enc->down_next) MXEC_TRY(file_piece(w));
    return MXEC_OK;
}

// Stream bytes [off, off + len), len <= kPiece, from their slots to a staging
// piece, behind whatever the download stream already waits for.
int fetch_piece(mxec_writer& w, uint64_t off, uint64_t len) {
    EncState& e = *w.enc;
    if (e.down_next - e.down_head == kDownPieces) MXEC_TRY(file_piece(w));
    DownPiece& p = e.down[e.down_next % kDownPieces];
    uint8_t* dst = static_cast<uint8_t*>(p.buf.p);
    MXEC_TRY(ring_segments(w.plan.chunk_size, w.plan.slots, off, len, [&](uint64_t slot, uint64_t at, uint64_t src, uint64_t n) -> int {
        MXEC_HIP(hipMemcpyAsync(dst + src, w.slot_ptr(slot) + at, size_t(n), hipMemcpyDeviceToHost, e.down_s));
        return MXEC_OK;
    }));
    MXEC_HIP(hipEventRecord(p.landed, e.down_s));
    p.off = off;
    p.len = len;
    ++e.down_next;
    return MXEC_OK;
}

// The stretch's digest run over the plaintext ring, behind its upload on w.s.
int queue_plain_sums(mxec_writer& w, const EncRun& q) {
    EncState& e = *w.enc;
    RingRun& rr = e.runs[q.index % kRingRuns];
    MXEC_TRY(rr.sum_tables.reserve(std::max<size_t>(4096, kSumRunTables)));
    MXEC_HIP(hipEventRecord(w.uploaded, w.s));
    MXEC_HIP(hipStreamWaitEvent(w.sum_s, w.uploaded, 0));
    {
        DevScope ds;
        MXEC_TRY(ds.open(w.ctx, w.dev_index));
        const SumsUpdate upd{static_cast<uint8_t*>(w.sum_state.p),
                             (q.index == 0 ? MXEC_SUMS_F_FIRST : 0u) | (q.last ? MXEC_SUMS_F_FINAL : 0u)};
        MXEC_TRY(run_body_sums(*ds.d, *ds.slot, w.sum_s, {e.ring_ptr(q.index)}, {q.plain_len}, w.which, w.sums_out_dev(),
                               sizeof(mxec_body_sums), &upd, &rr.sum_tables));
    }
    MXEC_HIP(hipEventRecord(rr.summed, w.sum_s));
    rr.sum_busy = true;
    if (!q.last) return MXEC_OK;
    MXEC_HIP(hipMemcpyAsync(w.hsums.p, w.sums_out_dev(), sizeof(mxec_body_sums), hipMemcpyDeviceToHost, w.sum_s));
    MXEC_HIP(hipEventRecord(w.sums_done, w.sum_s));
    return MXEC_OK;
}

// The stretch's plaintext is whole in the ring (its uploads queued on w.s):
// its frames into the window, its ciphertext on its way down, its chunks
// completed.
int queue_enc_run(mxec_writer& w, const EncRun& q) {
    EncState& e = *w.enc;
    RingRun& rr = e.runs[q.index % kRingRuns];
    const WriterPlan& p = w.plan;
    // Back-pressure: a slot the launch opens must be done with its last chunk
    // (hash and fold: collect; download: in its file).  The launch touches at
    // most p.slots chunks, so that chunk was completed by an earlier launch.
    MXEC_TRY(writer_cut(p, q.stream_off, q.stream_len, [&](const WriterRun& c) -> int {
        if (!c.opens || !p.reuses(c.chunk)) return MXEC_OK;
        MXEC_TRY(file_until(w, (p.evicts(c.chunk) + 1) * p.chunk_size));
        return collect(w, p.slot_of(c.chunk));
    }));
    if (w.which) MXEC_TRY(queue_plain_sums(w, q));
    // Frame i's AAD = SHA-256(aad_prefix || i as u64 LE) (build_frame_aad, filesystem.rs:118-128).
    uint8_t* ah = static_cast<uint8_t*>(e.aad_host.p) + e.aad_at(q.index);
    uint8_t* ad = static_cast<uint8_t*>(e.aad_dev.p) + e.aad_at(q.index);
    const size_t pl = e.aad_msg.size() - 8;
    for (uint64_t f = 0; f < q.frames; ++f) {
        for (int b = 0; b < 8; ++b) e.aad_msg[pl + size_t(b)] = uint8_t((q.first_frame + f) >> (8 * b));
        sha256_host(e.aad_msg.data(), e.aad_msg.size(), ah + f * 32);
    }
    MXEC_HIP(hipMemcpyAsync(ad, ah, size_t(q.frames) * 32, hipMemcpyHostToDevice, w.s));
    mxec_frames_job job{};
    std::memcpy(job.nonce_prefix, e.prefix, 4);
    job.frame_size = uint32_t(kFramePlain);
    job.first_index = q.first_frame;
    job.aad_dev = ad;
    job.aad_len = 32;
    job.in_dev = e.ring_ptr(q.index);
    job.len = q.plain_len;
    const mxec_frames_window win{static_cast<uint8_t*>(w.window.p), p.chunk_size, w.sa, p.slots};
    {
        DevScope ds;
        MXEC_TRY(ds.open(w.ctx, w.dev_index));
        MXEC_TRY(gcm_window_check(job, win, false));
        MXEC_TRY(rr.enc_tables.reserve(4096));
        MXEC_TRY(gcm_encrypt_window(*ds.d, *ds.slot, w.s, static_cast<const GcmKey*>(e.key_dev.p), job, q.stream_off, win,
                                    &rr.enc_tables));
    }
    MXEC_HIP(hipEventRecord(rr.encrypted, w.s));
    rr.busy = true;
    MXEC_HIP(hipStreamWaitEvent(e.down_s, rr.encrypted, 0));
    for (uint64_t off = 0; off < q.stream_len; off += kPiece)
        MXEC_TRY(fetch_piece(w, q.stream_off + off, std::min(kPiece, q.stream_len - off)));
    return writer_cut(p, q.stream_off, q.stream_len,
                      [&](const WriterRun& c) -> int { return c.completes ? complete(w, c.chunk) : MXEC_OK; });
}

// `len` plaintext bytes (no over-run) into the ring, stretch by stretch.
int enc_write(mxec_writer& w, const uint8_t* buf, uint64_t len) {
    EncState& e = *w.enc;
    for (uint64_t src = 0; src < len;) {
        const uint64_t run = w.written / kEncRun, at = w.written - run * kEncRun;
        const uint64_t n = std::min(len - src, kEncRun - at);
        RingRun& rr = e.runs[run % kRingRuns];
        if (at == 0) {  // the stretch's last tenant: the only wait for the ring
            if (rr.busy) MXEC_HIP(hipEventSynchronize(rr.encrypted));
            if (rr.sum_busy) MXEC_HIP(hipEventSynchronize(rr.summed));
            rr.busy = rr.sum_busy = false;
        }
        MXEC_TRY(upload(w, e.ring_ptr(run) + at, buf + src, n));
        const uint64_t from = w.written;
        w.written += n;
        src += n;
        MXEC_TRY(enc_runs_due(e.plain_len, from, w.written, [&](const EncRun& q) { return queue_enc_run(w, q); }));
    }
    return MXEC_OK;
}

// ---- the device-side feed ---------------------------------------------------------------------------

// The bounce stretch's launch has finished: its frames' statuses, the first
// bad one as mxec_frames_decrypt words it.
int feed_settle(FeedBounce& fb) {
    if (!fb.busy) return MXEC_OK;
    MXEC_HIP(hipEventSynchronize(fb.done));
    fb.busy = false;
    const int32_t* st = static_cast<const int32_t*>(fb.st.p);
    for (uint32_t f = 0; f < fb.frames; ++f) {
        if (st[f] == 0) continue;
        uint64_t got = 0;  // the stored index: nonce bytes 4..11, LE
        const uint8_t* h = static_cast<const uint8_t*>(fb.ct.p) + fb.hdr_at[f] + 4;
        for (int j = 7; j >= 0; --j) got = (got << 8) | h[j];
        return gcm_frame_fail(st[f], fb.expect[f], got);
    }
    return MXEC_OK;
}

int read_at(int fd, uint8_t* dst, uint64_t len, uint64_t off, const char* path) {
    while (len) {
        const ssize_t n = ::pread(fd, dst, size_t(len), off_t(off));
        if (n < 0 && errno == EINTR) continue;
        if (n <= 0) return set_error(MXEC_E_IO, std::string("IO error: read failed for ") + (path ? path : "part file"));
        dst += n;
        off += uint64_t(n);
        len -= uint64_t(n);
    }
    return MXEC_OK;
}

// One launch of part_plan.hpp: its frames from the part files into the ring
// at the body offset, then whatever encrypt launches are due.
int feed_launch(mxec_writer& w, const FeedStep& L, const WriterFeedSrc* src) {
    EncState& e = *w.enc;
    FeedState& fs = *e.feed;
    if (!L.launch || L.n_jobs == 0 || L.n_jobs > kFeedFrames || L.frames == 0 || L.frames > kFeedFrames ||
        L.body_off != w.written || L.body_end < L.body_off || L.body_end > e.plain_len)
        return set_error(MXEC_E_INVALID_ARG, "feed step out of order at plaintext byte " + std::to_string(w.written));
    const uint64_t bi = fs.next % kFeedBounces;
    FeedBounce& fb = fs.b[bi];
    MXEC_TRY(feed_settle(fb));  // the stretch's last launch: its statuses before its frames go
    uint8_t* ct = static_cast<uint8_t*>(fb.ct.p);
    uint8_t* ct_dev = static_cast<uint8_t*>(fs.ct_dev.p) + bi * kEncRunStream;
    uint8_t* ah = static_cast<uint8_t*>(fs.aad_host.p) + bi * kFeedFrames * 32;
    uint8_t* ad = static_cast<uint8_t*>(fs.aad_dev.p) + bi * kFeedFrames * 32;
    int32_t* st_dev = static_cast<int32_t*>(fs.st_dev.p) + bi * kFeedFrames;
    mxec_frames_job jobs[kFeedFrames];
    uint64_t ring_off[kFeedFrames];
    uint64_t at = 0, body = L.body_off;
    uint32_t nf = 0;
    std::vector<uint8_t> msg;
    for (uint32_t j = 0; j < L.n_jobs; ++j) {
        const FeedJob& q = L.jobs[j];
        if (q.frames == 0 || nf + q.frames > L.frames || q.plain_bytes == 0 || q.plain_bytes > q.frames * kFramePlain ||
            q.stream_bytes != q.plain_bytes + kFrameExtra * q.frames || q.ring_off != body % fs.ring_bytes ||
            q.plain_bytes > L.body_end - body)
            return set_error(MXEC_E_INVALID_ARG, "feed step does not match the writer's ring");
        MXEC_TRY(read_at(src[j].fd, ct + at, q.stream_bytes, q.file_off, src[j].path));
        // Frame i's AAD = SHA-256("PART" 0 upload_id 0 part_number_le4 0 || i as u64 LE) (:147-163).
        msg.assign(fs.aad_prefix.begin(), fs.aad_prefix.end());
        for (int b = 0; b < 4; ++b) msg.push_back(uint8_t(src[j].part_number >> (8 * b)));
        msg.push_back(0);
        const size_t pl = msg.size();
        msg.resize(pl + 8);
        mxec_frames_job& jb = jobs[j];
        jb = mxec_frames_job{};
        jb.frame_size = uint32_t(kFramePlain);
        jb.first_index = q.first_frame;
        jb.aad_dev = ad + size_t(nf) * 32;
        jb.aad_len = 32;
        jb.in_dev = ct_dev + at;
        jb.len = q.plain_bytes;
        ring_off[j] = q.ring_off;
        for (uint64_t f = 0; f < q.frames; ++f, ++nf) {
            for (int b = 0; b < 8; ++b) msg[pl + size_t(b)] = uint8_t((q.first_frame + f) >> (8 * b));
            sha256_host(msg.data(), msg.size(), ah + size_t(nf) * 32);
            fb.expect[nf] = q.first_frame + f;
            fb.hdr_at[nf] = at + f * kFrameBytes;
        }
        at += q.stream_bytes;
        body += q.plain_bytes;
    }
    if (nf != L.frames || body != L.body_end) return set_error(MXEC_E_INVALID_ARG, "feed step does not match the writer's ring");
    // Back-pressure: a stretch the launch opens must be done with its last
    // tenant (its encrypt launch, its digest run), as in enc_write.
    for (uint64_t r = L.open_first; r < L.open_first + L.open_count; ++r) {
        RingRun& rr = e.runs[r % kRingRuns];
        if (rr.busy) MXEC_HIP(hipEventSynchronize(rr.encrypted));
        if (rr.sum_busy) MXEC_HIP(hipEventSynchronize(rr.summed));
        rr.busy = rr.sum_busy = false;
    }
    MXEC_HIP(hipMemcpyAsync(ct_dev, ct, size_t(at), hipMemcpyHostToDevice, w.s));
    MXEC_HIP(hipMemcpyAsync(ad, ah, size_t(nf) * 32, hipMemcpyHostToDevice, w.s));
    const mxec_frames_ring ring{static_cast<uint8_t*>(e.ring.p), fs.ring_bytes};
    {
        DevScope ds;
        MXEC_TRY(ds.open(w.ctx, w.dev_index));
        MXEC_TRY(gcm_ring_check(jobs, L.n_jobs, ring_off, &ring, st_dev, false));
        MXEC_TRY(fb.tables.reserve(4096));
        MXEC_TRY(gcm_decrypt_ring(*ds.d, *ds.slot, w.s, static_cast<const GcmKey*>(fs.key_dev.p), jobs, L.n_jobs, ring_off,
                                  ring, st_dev, &fb.tables));
    }
    MXEC_HIP(hipMemcpyAsync(fb.st.p, st_dev, size_t(nf) * sizeof(int32_t), hipMemcpyDeviceToHost, w.s));
    MXEC_HIP(hipEventRecord(fb.done, w.s));
    fb.busy = true;
    fb.frames = nf;
    ++fs.next;
    const uint64_t from = w.written;
    w.written = L.body_end;
    return enc_runs_due(e.plain_len, from, w.written, [&](const EncRun& q) { return queue_enc_run(w, q); });
}

int finish(mxec_writer& w) {
    if (w.enc && w.enc->feed)  // no parity file and no manifest over a part frame that failed
        for (FeedBounce& fb : w.enc->feed->b) MXEC_TRY(feed_settle(fb));
    if (w.enc) {
        if (w.written != w.enc->plain_len)
            return set_error(MXEC_E_INVALID_ARG, writer_short_msg(w.enc->pplan, w.written));
        MXEC_TRY(file_until(w, w.plan.total_len));  // the last launch went with the last byte
    } else if (w.written != w.plan.total_len) {
        return set_error(MXEC_E_INVALID_ARG, writer_short_msg(w.plan, w.written));
    }
    if (w.plan.total_len == 0) {  // one empty chunk (:740-743), no parity (:748)
        MXEC_TRY(open_chunk_file(w, 0));
        MXEC_TRY(close_chunk_file(w, 0));
        if (w.which && w.enc) {  // one empty run, first and last
            EncRun q{};
            q.last = true;
            MXEC_TRY(queue_plain_sums(w, q));
        } else if (w.which) {
            MXEC_TRY(writer_sum_due(w.plan, 0, 0, 0, [&](const SumRun& q) { return queue_sum_run(w, q); }));
        }
        MXEC_TRY(complete(w, 0));
    }
    const uint64_t k = w.plan.k;
    // The rows come down on w.s beside the last chunks' hash chains.
    for (uint32_t i = 0; i < w.m; ++i) MXEC_TRY(write_parity_file(w, i));
    for (uint64_t slot = 0; slot < w.slots.size(); ++slot) MXEC_TRY(collect(w, slot));
    const uint8_t* hd = static_cast<const uint8_t*>(w.hdig.p) + (w.slots.size() + 1) * 32;  // landed with the last chunk's
    for (uint32_t i = 0; i < w.m; ++i) w.sha[k + i] = hex(hd + size_t(i) * 32, 32);
    if (w.which) {  // queued with the body's last byte
        MXEC_HIP(hipEventSynchronize(w.sums_done));
        std::memcpy(&w.sums, w.hsums.p, sizeof w.sums);
    }
    Manifest man;
    man.version = w.m ? 2 : 1;
    man.total_size = w.plan.total_len;
    man.chunk_size = w.plan.chunk_size;
    man.chunk_count = uint32_t(k);
    for (uint64_t j = 0; j < k + w.m; ++j)
        man.chunks.push_back({uint32_t(j), j < k ? w.plan.chunk_len(j) : w.plan.chunk_size, w.sha[j],
                              uint8_t(j < k ? 0 : 1)});
    man.has_parity = man.has_shard = w.m > 0;
    man.parity_shards = w.m;
    man.shard_size = w.plan.chunk_size;
    man.has_plain = w.has_plain;
    man.plaintext_size = w.plaintext_size;
    const std::string js = manifest_json(man);
    return write_file(w.dir / "manifest.json", reinterpret_cast<const uint8_t*>(js.data()), js.size());
}

// What mxec_writer_open_encrypted adds to an open.
struct EncOpen {
    uint64_t plain_len;
    const uint8_t* key;
    const uint8_t* prefix;
    const uint8_t* aad_prefix;
    uint32_t aad_prefix_len;
};

// The encrypted writer's own buffers, streams and key tables.
int open_enc(mxec_writer& w, const EncOpen& eo) {
    w.enc = std::make_unique<EncState>();
    EncState& e = *w.enc;
    e.plain_len = eo.plain_len;
    e.pplan = WriterPlan::make(kEncRun, eo.plain_len, 0);
    std::memcpy(e.key, eo.key, 32);
    std::memcpy(e.prefix, eo.prefix, 4);
    e.aad_msg.assign(size_t(eo.aad_prefix_len) + 8, 0);
    if (eo.aad_prefix_len) std::memcpy(e.aad_msg.data(), eo.aad_prefix, eo.aad_prefix_len);
    // The key schedule, H^1..H^256 and the position table, once for every launch.
    gcm_prepare_key(e.key, e.tables);
    MXEC_TRY(e.key_dev.ensure(sizeof(GcmKey)));
    MXEC_HIP(hipMemcpy(e.key_dev.p, &e.tables, sizeof(GcmKey), hipMemcpyHostToDevice));
    MXEC_TRY(e.ring.ensure(size_t(ring_bytes_for(eo.plain_len))));
    MXEC_TRY(e.aad_dev.ensure(size_t(kRingRuns * kEncFrames * 32)));
    MXEC_TRY(e.aad_host.ensure(size_t(kRingRuns * kEncFrames * 32)));
    for (RingRun& r : e.runs) {
        MXEC_TRY(new_event(&r.encrypted));
        if (w.which) MXEC_TRY(new_event(&r.summed));
        r.sum_tables.owner = r.enc_tables.owner = w.dev;
    }
    MXEC_TRY(new_stream(w, &e.down_s));
    for (DownPiece& p : e.down) {
        MXEC_TRY(p.buf.ensure(size_t(std::min(kPiece, std::max<uint64_t>(w.plan.total_len, 4096)))));
        MXEC_TRY(new_event(&p.landed));
    }
    return MXEC_OK;
}

int open_writer(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size, uint32_t parity_shards, uint64_t total_len,
                uint64_t plaintext_size, uint64_t window_bytes, uint32_t which, void** out,
                const EncOpen* eo = nullptr) {
    return guarded([&]() -> int {
        if (!ctx || !ec_dir || !out) return set_error(MXEC_E_INVALID_ARG, "null argument");
        *out = nullptr;
        if (eo && (!eo->key || !eo->prefix || (eo->aad_prefix_len && !eo->aad_prefix)))
            return set_error(MXEC_E_INVALID_ARG, "null argument");
        if (chunk_size == 0) return set_error(MXEC_E_INVALID_ARG, "chunk_size must be > 0");
        if (which & ~uint32_t(0x1F)) return set_error(MXEC_E_INVALID_ARG, "unknown digest flag");
        if (eo) {
            // k, the chunk lengths and the guards below come from the frame stream's length.
            if (!frame_stream_len(eo->plain_len, &total_len))
                return set_error(MXEC_E_INVALID_ARG, "plaintext_len: the frame stream does not fit in 64 bits");
            plaintext_size = eo->plain_len;
            // One launch writes up to kEncRunStream bytes, which touch
            // ceil(kEncRunStream / chunk_size) + 1 chunks at the most: the
            // window holds at least those (two, for chunks of 1 MiB and more).
            if (chunk_size < kEncRunStream) {
                const uint64_t need = ((kEncRunStream - 1) / chunk_size + 2) * chunk_size;
                const uint64_t asked = window_bytes ? window_bytes : WriterPlan::kDefaultSlots * chunk_size;
                window_bytes = std::max(asked, need);
            }
        }
        auto w = std::make_unique<mxec_writer>();
        w->plan = WriterPlan::make(chunk_size, total_len, window_bytes);
        w->m = parity_shards > 0 && total_len > 0 ? parity_shards : 0;  // :748
        // The reference writes the data chunks, then hits this guard inside
        // compute_and_write_parity; k is known here, so nothing is created.
        if (w->m && (w->plan.k > 255 || w->plan.k + w->m > 255)) return too_many_shards(w->plan.k, w->m);
        if (w->plan.k > UINT32_MAX)
            return set_error(MXEC_E_INVALID_ARG, "more than 2^32 - 1 chunks: increase chunk_size");
        if (w->m) MXEC_TRY(check_km(int(w->plan.k), int(w->m)));
        w->ctx = ctx;
        w->dir = ec_dir;
        w->has_plain = plaintext_size != UINT64_MAX;
        w->plaintext_size = plaintext_size;
        Device* d = pick_device(&ctx->c, -1);  // round robin, kept for the writer's life
        if (!d) return set_error(MXEC_E_INVALID_ARG, "no device in context");
        for (size_t i = 0; i < ctx->c.devs.size(); ++i)
            if (ctx->c.devs[i].get() == d) w->dev_index = int(i);
        MXEC_HIP(hipSetDevice(d->id));
        w->dev = d;
        w->sa = round_up(chunk_size, kSlotAlign);
        const uint64_t n_slots = w->plan.slots;
        MXEC_TRY(w->window.ensure(size_t(n_slots * w->sa)));
        if (w->m) MXEC_TRY(w->parity.ensure(size_t(2 * uint64_t(w->m) * w->sa)));
        MXEC_TRY(w->dig.ensure(size_t((n_slots + 1 + w->m) * 32)));
        MXEC_TRY(w->hdig.ensure(size_t((n_slots + 1 + w->m) * 32)));
        for (int b = 0; b < kPieces; ++b) {
            // A plain writer's uploads end with their chunk, an encrypted one's with their MiB of plaintext.
            const uint64_t longest = eo ? std::max<uint64_t>(chunk_size, eo->plain_len) : chunk_size;
            MXEC_TRY(w->stage[b].ensure(size_t(std::min(kPiece, std::max<uint64_t>(longest, 4096)))));
            MXEC_TRY(new_event(&w->staged[b]));
        }
        MXEC_TRY(new_stream(*w, &w->s, true));
        MXEC_TRY(new_event(&w->uploaded));
        w->slots.resize(size_t(n_slots));
        for (WindowSlot& ws : w->slots) {
            MXEC_TRY(new_stream(*w, &ws.hash));
            MXEC_TRY(new_event(&ws.hashed));
            MXEC_TRY(new_event(&ws.folded));
        }
        w->which = which;
        if (which) {
            MXEC_TRY(w->sum_state.ensure(MXEC_SUMS_STATE_BYTES + sizeof(mxec_body_sums)));
            MXEC_TRY(w->hsums.ensure(sizeof(mxec_body_sums)));
            MXEC_TRY(new_stream(*w, &w->sum_s));
            MXEC_TRY(new_event(&w->sums_done));
            for (WindowSlot& ws : w->slots) {
                if (eo) continue;  // an encrypted writer's runs are over the plaintext ring (open_enc)
                MXEC_TRY(new_event(&ws.summed));
                ws.sum_tables.owner = d;
                MXEC_TRY(ws.sum_tables.reserve(std::max<size_t>(4096, size_t(writer_sum_runs_of(w->plan, 0)) * kSumRunTables)));
            }
        }
        w->sha.resize(size_t(w->plan.k + w->m));
        if (eo) MXEC_TRY(open_enc(*w, *eo));
        std::error_code ec;
        fs::create_directories(w->dir, ec);
        if (ec) return set_error(MXEC_E_IO, "IO error: " + ec.message());
        *out = w.release();
        return MXEC_OK;
    });
}

}  // namespace

// The plaintext ring an encrypted writer of plain_len bytes has (part_plan.hpp's ring_bytes).
uint64_t mxec::writer_ring_bytes(uint64_t plain_len) { return ring_bytes_for(plain_len); }

int mxec::writer_feed_key(void* wp, const uint8_t* upload_key, const char* upload_id) {
    return guarded([&]() -> int {
        auto* w = static_cast<mxec_writer*>(wp);
        if (!w || !w->enc || !upload_key || !upload_id) return set_error(MXEC_E_INVALID_ARG, "null argument");
        if (w->err) return set_error(w->err, w->err_msg);
        if (w->enc->feed) return set_error(MXEC_E_INVALID_ARG, "the feed's key is already set");
        MXEC_HIP(hipSetDevice(w->dev->id));
        w->enc->feed = std::make_unique<FeedState>();  // the writer's close takes it from here on
        FeedState& fs = *w->enc->feed;
        std::memcpy(fs.key, upload_key, 32);
        fs.aad_prefix = std::string("PART") + '\0' + upload_id + '\0';
        fs.ring_bytes = ring_bytes_for(w->enc->plain_len);
        gcm_prepare_key(fs.key, fs.tables);
        MXEC_TRY(fs.key_dev.ensure(sizeof(GcmKey)));
        MXEC_HIP(hipMemcpy(fs.key_dev.p, &fs.tables, sizeof(GcmKey), hipMemcpyHostToDevice));
        MXEC_TRY(fs.ct_dev.ensure(size_t(kFeedBounces * kEncRunStream)));
        MXEC_TRY(fs.aad_dev.ensure(size_t(kFeedBounces * kFeedFrames * 32)));
        MXEC_TRY(fs.aad_host.ensure(size_t(kFeedBounces * kFeedFrames * 32)));
        MXEC_TRY(fs.st_dev.ensure(size_t(kFeedBounces * kFeedFrames * sizeof(int32_t))));
        for (FeedBounce& fb : fs.b) {
            MXEC_TRY(fb.ct.ensure(size_t(kEncRunStream)));
            MXEC_TRY(fb.st.ensure(size_t(kFeedFrames * sizeof(int32_t))));
            MXEC_TRY(new_event(&fb.done));
            fb.tables.owner = w->dev;
        }
        return MXEC_OK;
    });
}

int mxec::writer_feed_frames(void* wp, const FeedStep& step, const WriterFeedSrc* src) {
    return guarded([&]() -> int {
        auto* w = static_cast<mxec_writer*>(wp);
        if (!w || !w->enc || !w->enc->feed || !src) return set_error(MXEC_E_INVALID_ARG, "null argument");
        if (w->err) return set_error(w->err, w->err_msg);
        if (w->finished) return set_error(MXEC_E_INVALID_ARG, "write after finish");
        MXEC_HIP(hipSetDevice(w->dev->id));
        return poison(*w, feed_launch(*w, step, src));
    });
}

extern "C" {

int mxec_writer_open(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size, uint32_t parity_shards,
                     uint64_t total_len, uint64_t plaintext_size, uint64_t window_bytes, void** out) {
    return open_writer(ctx, ec_dir, chunk_size, parity_shards, total_len, plaintext_size, window_bytes, 0, out);
}

int mxec_writer_open_sums(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size, uint32_t parity_shards,
                          uint64_t total_len, uint64_t plaintext_size, uint64_t window_bytes, uint32_t which,
                          void** out) {
    return open_writer(ctx, ec_dir, chunk_size, parity_shards, total_len, plaintext_size, window_bytes, which, out);
}

int mxec_writer_open_encrypted(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size, uint32_t parity_shards,
                               uint64_t plaintext_len, const uint8_t key[32], const uint8_t nonce_prefix[4],
                               const uint8_t* aad_prefix, uint32_t aad_prefix_len, uint64_t window_bytes,
                               uint32_t which, void** out) {
    const EncOpen eo{plaintext_len, key, nonce_prefix, aad_prefix, aad_prefix_len};
    return open_writer(ctx, ec_dir, chunk_size, parity_shards, 0, 0, window_bytes, which, out, &eo);
}

int mxec_writer_write(void* wp, const uint8_t* buf, uint64_t len) {
    return guarded([&]() -> int {
        auto* w = static_cast<mxec_writer*>(wp);
        if (!w || (len && !buf)) return set_error(MXEC_E_INVALID_ARG, "null argument");
        if (w->err) return set_error(w->err, w->err_msg);
        if (w->finished) return set_error(MXEC_E_INVALID_ARG, "write after finish");
        const WriterPlan& body = w->enc ? w->enc->pplan : w->plan;  // the bytes the caller counts in
        if (writer_overruns(body, w->written, len))
            return poison(*w, set_error(MXEC_E_INVALID_ARG, writer_overrun_msg(body, w->written, len)));
        MXEC_HIP(hipSetDevice(w->dev->id));
        if (w->enc) return poison(*w, enc_write(*w, buf, len));
        const int rc = writer_cut(w->plan, w->written, len, [&](const WriterRun& r) {
            const int e = take_run(*w, r, buf);
            if (!e) w->written += r.len;
            return e;
        });
        return poison(*w, rc);
    });
}

int mxec_writer_finish(void* wp) {
    return guarded([&]() -> int {
        auto* w = static_cast<mxec_writer*>(wp);
        if (!w) return set_error(MXEC_E_INVALID_ARG, "null argument");
        if (w->err) return set_error(w->err, w->err_msg);
        if (w->finished) return MXEC_OK;
        MXEC_HIP(hipSetDevice(w->dev->id));
        const int rc = poison(*w, finish(*w));
        w->finished = rc == MXEC_OK;
        return rc;
    });
}

int mxec_writer_sums(void* wp, mxec_body_sums* out) {
    return guarded([&]() -> int {
        auto* w = static_cast<mxec_writer*>(wp);
        if (!w) return set_error(MXEC_E_INVALID_ARG, "null argument");
        if (w->err) return set_error(w->err, w->err_msg);
        if (w->which == 0) return MXEC_OK;
        if (!out) return set_error(MXEC_E_INVALID_ARG, "null argument");
        if (!w->finished) return set_error(MXEC_E_INVALID_ARG, "sums before finish");
        const mxec_body_sums& h = w->sums;
        if (w->which & MXEC_SUM_MD5) std::memcpy(out->md5, h.md5, 16);
        if (w->which & MXEC_SUM_CRC32) out->crc32 = h.crc32;
        if (w->which & MXEC_SUM_CRC32C) out->crc32c = h.crc32c;
        if (w->which & MXEC_SUM_SHA1) std::memcpy(out->sha1, h.sha1, 20);
        if (w->which & MXEC_SUM_SHA256) std::memcpy(out->sha256, h.sha256, 32);
        return MXEC_OK;
    });
}

void mxec_writer_close(void* wp) { delete static_cast<mxec_writer*>(wp); }

}  // extern "C"
