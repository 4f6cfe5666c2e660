// storage_reader_enc.cpp — GET of an encrypt-then-EC object as a pull stream:
// FrameDecryptor::for_range over VerifiedChunkReader (crypto.rs:186-420,
// filesystem.rs:1618-1630, :1700-1725) behind mxec_reader_open_encrypted and
// the plain reader's mxec_reader_read / _close.  The arithmetic is
// read_plan.hpp's.
//
// A round takes the next chunks of the range's frame stream, up to
// batch_bytes: each goes from its file through two page-locked pieces into its
// slot of a ring in HBM (chunk j in slot j % slots), is hashed where it lies
// and compared with the manifest.  One launch of the GCM kernel's decrypt
// window form then takes every frame that is now whole in verified chunks out
// of the ring, under key tables prepared once at open; its AADs are hashed on
// the host and go up in front of it.  The statuses come down first; plaintext
// comes down only for frames in front of the first one that failed, only the
// bytes the range wants, a piece at a time as read() asks for it.  A frame cut
// by the round's end keeps its chunks' slots until a later round completes it.
// Rounds run one after the other on the reader's own stream.
//
// A chunk that is missing, short or fails its digest sends the round's chunks
// through the plain reader's host path (load_chunks: the same errors, the same
// repair from parity), and what it rebuilt goes up into its slot: the rare
// path, which need not stay in HBM.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstring>
#include <memory>

#include "chunk_reader.hpp"
#include "frame_plan.hpp"
#include "kernels.hpp"
#include "ops.hpp"
#include "read_plan.hpp"
#include "sha256_host.hpp"

using namespace mxec;

namespace {

constexpr uint64_t kPiece = uint64_t(1) << 20;         // bytes per page-locked piece (at most)
constexpr int kPieces = 2;                             // pieces for chunk bytes on their way up
constexpr uint64_t kDefaultBatch = uint64_t(64) << 20;  // the plain reader's

}  // namespace

struct mxec::EncReader {
    mxec_ctx* ctx = nullptr;
    Device* dev = nullptr;
    int dev_index = 0;
    const fs::path* dir = nullptr;  // the handle's
    const Manifest* man = nullptr;
    ReadPlan plan;
    uint64_t sa = 0;          // bytes between slots
    uint64_t max_frames = 0;  // of one launch

    uint8_t key[32];
    GcmKey tables;  // the host copy of what key_dev holds
    DevBuf key_dev;
    std::vector<uint8_t> aad_msg;  // aad_prefix, then room for the index

    hipStream_t s = nullptr;
    hipEvent_t done = nullptr;  // what read() waits for
    PinnedBuf stage[kPieces];
    hipEvent_t staged[kPieces] = {nullptr, nullptr};
    bool stage_busy[kPieces] = {false, false};
    int next_stage = 0;
    DevBuf window, plain, aad_dev, status_dev, dig_dev;  // slots * sa | a launch's plaintext | ...
    PinnedBuf aad_host, status_host, dig_host, out_piece;
    DescArena launch_tables;

    uint64_t loaded = 0;      // chunks below it are in the ring or done with
    uint64_t next_frame = 0;  // frames below it are decrypted
    // Plaintext the range wants that is still in HBM, and the piece of it on the host.
    uint64_t pend_off = 0, pend_len = 0;
    uint64_t piece_pos = 0, piece_len = 0;
    // The error that ends the stream, returned once every byte in front of it has been.
    int err = 0;
    std::string err_msg;

    uint8_t* slot_ptr(uint64_t chunk) const { return static_cast<uint8_t*>(window.p) + (chunk % plan.slots) * sa; }
    bool finished() const { return plan.empty() || next_frame >= plan.f_end; }

    ~EncReader() {
        // Neither key outlives the reader, on the host or in HBM.
        explicit_bzero(key, sizeof key);
        explicit_bzero(&tables, sizeof tables);
        if (!dev) return;
        (void)hipSetDevice(dev->id);
        if (s) (void)hipStreamSynchronize(s);
        // The chunk hashes took their tables from the slots' rings, fenced by
        // events on the stream destroyed below (as the writer's, storage_writer.cpp).
        if (s) slots_settle(*dev);
        if (key_dev.p) (void)hipMemset(key_dev.p, 0, sizeof(GcmKey));
        for (hipEvent_t e : staged)
            if (e) (void)hipEventDestroy(e);
        if (done) (void)hipEventDestroy(done);
        if (s) {
            affinity_untag(s);
            (void)hipStreamDestroy(s);
        }
    }
};

namespace {

int fail(EncReader& e, int code, const std::string& msg) {
    e.err = code;
    e.err_msg = msg;
    return MXEC_OK;  // it is returned by the read that reaches it
}

int wait(EncReader& e) {
    MXEC_HIP(hipEventRecord(e.done, e.s));
    MXEC_HIP(hipEventSynchronize(e.done));
    return MXEC_OK;
}

// The next staging piece, free to be filled.
int take_piece(EncReader& e, int* which) {
    const int i = e.next_stage;
    e.next_stage = (i + 1) % kPieces;
    if (e.stage_busy[i]) MXEC_HIP(hipEventSynchronize(e.staged[i]));
    e.stage_busy[i] = false;
    *which = i;
    return MXEC_OK;
}
int send_piece(EncReader& e, int i, uint8_t* dst, uint64_t n) {
    MXEC_HIP(hipMemcpyAsync(dst, e.stage[i].p, size_t(n), hipMemcpyHostToDevice, e.s));
    MXEC_HIP(hipEventRecord(e.staged[i], e.s));
    e.stage_busy[i] = true;
    return MXEC_OK;
}

// Chunk j from its file into its slot, piece by piece.  *ok = false when the
// file cannot be read or has another size than the manifest says: the host
// path then finds the words for it.
int read_chunk(EncReader& e, uint64_t j, bool* ok) {
    *ok = false;
    const uint64_t size = e.plan.chunk_len(j);
    const fs::path p = *e.dir / chunk_name(uint32_t(j));
    const int fd = ::open(p.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd < 0) return MXEC_OK;
    struct stat st;
    bool good = ::fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && uint64_t(st.st_size) == size;
    int rc = MXEC_OK;
    for (uint64_t off = 0; good && off < size;) {
        const uint64_t n = std::min(kPiece, size - off);
        int i = 0;
        if ((rc = take_piece(e, &i)) != MXEC_OK) break;
        auto* dst = static_cast<uint8_t*>(e.stage[i].p);
        for (uint64_t got = 0; got < n;) {
            const ssize_t r = ::read(fd, dst + got, size_t(n - got));
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) {
                good = false;
                break;
            }
            got += uint64_t(r);
        }
        if (!good) break;
        if ((rc = send_piece(e, i, e.slot_ptr(j) + off, n)) != MXEC_OK) break;
        off += n;
    }
    ::close(fd);
    *ok = good && rc == MXEC_OK;
    return rc;
}

// Host bytes (a rebuilt chunk) into chunk j's slot.
int upload_chunk(EncReader& e, uint64_t j, const uint8_t* src, uint64_t len) {
    for (uint64_t off = 0; off < len; off += kPiece) {
        const uint64_t n = std::min(kPiece, len - off);
        int i = 0;
        MXEC_TRY(take_piece(e, &i));
        std::memcpy(e.stage[i].p, src + off, size_t(n));
        MXEC_TRY(send_piece(e, i, e.slot_ptr(j) + off, n));
    }
    return MXEC_OK;
}

// Chunks [first, first + count) into their slots, verified; *good_upto = the
// first chunk that could be neither verified nor rebuilt (its error latched),
// or first + count.
int load_round(EncReader& e, uint64_t first, uint64_t count, uint64_t* good_upto) {
    const Manifest& man = *e.man;
    std::vector<uint8_t> sound(size_t(count), 0);
    std::vector<const uint8_t*> msgs;
    std::vector<uint64_t> lens, who;
    for (uint64_t c = 0; c < count; ++c) {
        bool ok = false;
        MXEC_TRY(read_chunk(e, first + c, &ok));
        if (!ok) continue;
        msgs.push_back(e.slot_ptr(first + c));
        lens.push_back(e.plan.chunk_len(first + c));
        who.push_back(c);
    }
    if (!msgs.empty()) {  // hashed where they lie, behind their uploads
        auto* dd = static_cast<uint8_t*>(e.dig_dev.p);
        MXEC_TRY(mxec_sha256_batch_device(e.ctx, e.dev_index, e.s, msgs.data(), lens.data(), msgs.size(), dd));
        MXEC_HIP(hipMemcpyAsync(e.dig_host.p, dd, msgs.size() * 32, hipMemcpyDeviceToHost, e.s));
        MXEC_TRY(wait(e));
        for (size_t t = 0; t < who.size(); ++t)
            sound[size_t(who[t])] =
                hex(static_cast<const uint8_t*>(e.dig_host.p) + t * 32, 32) == man.chunks[size_t(first + who[t])].sha256;
    }
    *good_upto = first + count;
    if (msgs.size() == count && std::find(sound.begin(), sound.end(), 0) == sound.end()) return MXEC_OK;
    // The degraded path: the plain reader's, over the round's chunks.
    std::vector<LoadedChunk> batch;
    MXEC_TRY(load_chunks(e.ctx, *e.dir, man, uint32_t(first), uint32_t(first + count - 1), batch));
    MXEC_HIP(hipSetDevice(e.dev->id));
    for (uint64_t c = 0; c < count; ++c) {
        const LoadedChunk& lc = batch[size_t(c)];
        if (lc.err) {
            *good_upto = first + c;
            return fail(e, lc.err, lc.msg);
        }
        if (!sound[size_t(c)]) MXEC_TRY(upload_chunk(e, first + c, lc.data.data(), lc.data.size()));
    }
    return MXEC_OK;
}

// The stored index of frame f (nonce bytes 4..11, LE), from where it lies in the ring.
int stored_index(EncReader& e, uint64_t f, uint64_t* got) {
    uint8_t b[8];
    MXEC_TRY(ring_segments(e.plan.cs, e.plan.slots, e.plan.frame_off(f) + 4, 8,
                           [&](uint64_t slot, uint64_t at, uint64_t src, uint64_t n) -> int {
                               MXEC_HIP(hipMemcpyAsync(b + src, static_cast<uint8_t*>(e.window.p) + slot * e.sa + at,
                                                       size_t(n), hipMemcpyDeviceToHost, e.s));
                               return MXEC_OK;
                           }));
    MXEC_HIP(hipStreamSynchronize(e.s));
    *got = 0;
    for (int j = 7; j >= 0; --j) *got = (*got << 8) | b[j];
    return MXEC_OK;
}

// Frames [next_frame, g) are whole in verified chunks: decrypt them, and note
// what of their plaintext the range wants.  A frame that fails ends the stream
// there.
int decrypt_frames(EncReader& e, uint64_t g) {
    const ReadPlan& p = e.plan;
    const uint64_t a = e.next_frame, n = g - a;
    // Frame i's AAD = SHA-256(aad_prefix || i as u64 LE) (build_frame_aad, filesystem.rs:118-128).
    auto* ah = static_cast<uint8_t*>(e.aad_host.p);
    const size_t pl = e.aad_msg.size() - 8;
    for (uint64_t f = 0; f < n; ++f) {
        for (int b = 0; b < 8; ++b) e.aad_msg[pl + size_t(b)] = uint8_t((a + f) >> (8 * b));
        sha256_host(e.aad_msg.data(), e.aad_msg.size(), ah + f * 32);
    }
    MXEC_HIP(hipMemcpyAsync(e.aad_dev.p, ah, size_t(n) * 32, hipMemcpyHostToDevice, e.s));
    mxec_frames_job job{};
    job.frame_size = uint32_t(p.fs);
    job.first_index = a;
    job.aad_dev = static_cast<const uint8_t*>(e.aad_dev.p);
    job.aad_len = 32;
    job.len = (g - 1) * p.fs + p.frame_plain(g - 1) - a * p.fs;
    job.out_dev = static_cast<uint8_t*>(e.plain.p);
    const mxec_frames_window win{static_cast<uint8_t*>(e.window.p), p.cs, e.sa, p.slots};
    auto* st_dev = static_cast<int32_t*>(e.status_dev.p);
    {
        DevScope ds;
        MXEC_TRY(ds.open(e.ctx, e.dev_index));
        MXEC_TRY(gcm_window_check(job, win, false, true));
        MXEC_TRY(e.launch_tables.reserve(size_t(n) * sizeof(GcmFrame) + 4096));  // the last launch has finished
        MXEC_TRY(gcm_decrypt_window(*ds.d, *ds.slot, e.s, static_cast<const GcmKey*>(e.key_dev.p), job, p.frame_off(a),
                                    win, st_dev, &e.launch_tables));
    }
    MXEC_HIP(hipMemcpyAsync(e.status_host.p, st_dev, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost, e.s));
    MXEC_TRY(wait(e));
    const auto* st = static_cast<const int32_t*>(e.status_host.p);
    uint64_t good = 0;
    while (good < n && st[good] == 0) ++good;
    const ReadSpan w = p.want(a, a + good);
    e.pend_off = w.dev_off;
    e.pend_len = w.len;
    e.next_frame = a + good;
    if (good == n) return MXEC_OK;
    uint64_t got = 0;
    if (st[good] == 2) MXEC_TRY(stored_index(e, a + good, &got));
    (void)gcm_frame_fail(st[good], a + good, got);
    return fail(e, MXEC_E_INTEGRITY, last_error());
}

// One round: the next chunks, then every frame they complete.
int next_round(EncReader& e) {
    const ReadPlan& p = e.plan;
    if (e.loaded >= p.c_end)  // every chunk of the range is in, and a frame is still not whole
        return fail(e, MXEC_E_INTEGRITY, "truncated encrypted frame");
    const ReadChunks r = p.round(e.loaded, e.next_frame);
    uint64_t upto = 0;
    MXEC_TRY(load_round(e, r.first, r.count, &upto));
    e.loaded = upto;
    const uint64_t g = p.frames_whole(e.next_frame, p.resident_end(upto));
    if (g > e.next_frame && !e.err) return decrypt_frames(e, g);
    if (g > e.next_frame) {  // in front of an unrecoverable chunk: its error waits behind theirs, if any
        const int chunk_err = e.err;
        const std::string chunk_msg = e.err_msg;
        e.err = 0;
        MXEC_TRY(decrypt_frames(e, g));
        if (!e.err) fail(e, chunk_err, chunk_msg);
    }
    return MXEC_OK;
}

// The next piece of the pending plaintext, down into out_piece.
int fetch_plain(EncReader& e) {
    const uint64_t n = std::min(kPiece, e.pend_len);
    MXEC_HIP(hipMemcpyAsync(e.out_piece.p, static_cast<const uint8_t*>(e.plain.p) + e.pend_off, size_t(n),
                            hipMemcpyDeviceToHost, e.s));
    MXEC_TRY(wait(e));
    e.pend_off += n;
    e.pend_len -= n;
    e.piece_pos = 0;
    e.piece_len = n;
    return MXEC_OK;
}

int new_event(hipEvent_t* ev) {
    MXEC_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming | hipEventBlockingSync));
    return MXEC_OK;
}

// The reader's device, buffers, stream and key tables.
int open_enc(EncReader& e, mxec_ctx* ctx, const uint8_t* key, const uint8_t* aad_prefix, uint32_t aad_prefix_len) {
    const ReadPlan& p = e.plan;
    e.ctx = ctx;
    std::memcpy(e.key, key, 32);
    e.aad_msg.assign(size_t(aad_prefix_len) + 8, 0);
    if (aad_prefix_len) std::memcpy(e.aad_msg.data(), aad_prefix, aad_prefix_len);
    if (p.empty() || p.c0 == p.c_end) return MXEC_OK;  // nothing is read: no device is needed
    Device* d = pick_device(&ctx->c, -1);  // round robin, kept for the reader's life
    if (!d) return set_error(MXEC_E_INVALID_ARG, "no device in context");
    for (size_t i = 0; i < ctx->c.devs.size(); ++i)
        if (ctx->c.devs[i].get() == d) e.dev_index = int(i);
    MXEC_HIP(hipSetDevice(d->id));
    e.dev = d;
    // The key schedule, H^1..H^256 and the position table, once for every launch.
    gcm_prepare_key(e.key, e.tables);
    MXEC_TRY(e.key_dev.ensure(sizeof(GcmKey)));
    MXEC_HIP(hipMemcpy(e.key_dev.p, &e.tables, sizeof(GcmKey), hipMemcpyHostToDevice));
    // A launch's frames lie in at most slots * chunk_size stream bytes, and all but the object's last are fl long.
    e.max_frames = std::min(p.f_end - p.f0, p.slots * p.cs / p.fl + 2);
    MXEC_TRY(e.window.ensure(size_t(p.slots * e.sa)));
    MXEC_TRY(e.plain.ensure(size_t(e.max_frames * p.fs)));
    MXEC_TRY(e.aad_dev.ensure(size_t(e.max_frames * 32)));
    MXEC_TRY(e.aad_host.ensure(size_t(e.max_frames * 32)));
    MXEC_TRY(e.status_dev.ensure(size_t(e.max_frames * sizeof(int32_t))));
    MXEC_TRY(e.status_host.ensure(size_t(e.max_frames * sizeof(int32_t))));
    MXEC_TRY(e.dig_dev.ensure(size_t(p.slots * 32)));
    MXEC_TRY(e.dig_host.ensure(size_t(p.slots * 32)));
    const uint64_t piece = std::min(kPiece, std::max<uint64_t>(p.cs, 4096));
    for (int b = 0; b < kPieces; ++b) {
        MXEC_TRY(e.stage[b].ensure(size_t(piece)));
        MXEC_TRY(new_event(&e.staged[b]));
    }
    MXEC_TRY(e.out_piece.ensure(size_t(std::min(kPiece, std::max<uint64_t>(p.end - p.off, 4096)))));
    MXEC_HIP(hipStreamCreateWithFlags(&e.s, hipStreamNonBlocking));
    affinity_tag(e.s, d);
    MXEC_TRY(new_event(&e.done));
    e.launch_tables.owner = d;
    return MXEC_OK;
}

}  // namespace

int64_t mxec::enc_reader_read(EncReader& e, uint8_t* buf, uint64_t cap) {
    if (e.dev) MXEC_HIP(hipSetDevice(e.dev->id));
    uint64_t copied = 0;
    while (copied < cap) {
        if (e.piece_pos < e.piece_len) {
            const uint64_t n = std::min(cap - copied, e.piece_len - e.piece_pos);
            std::memcpy(buf + copied, static_cast<const uint8_t*>(e.out_piece.p) + e.piece_pos, size_t(n));
            copied += n;
            e.piece_pos += n;
            continue;
        }
        int rc = MXEC_OK;
        if (e.pend_len) {
            rc = fetch_plain(e);
        } else if (e.err) {  // every byte in front of it has been served
            if (copied) return int64_t(copied);
            return set_error(e.err, e.err_msg);
        } else if (e.finished()) {
            break;
        } else {
            rc = next_round(e);
        }
        if (rc) {  // the device or the file system: it ends the stream like any other error
            e.pend_len = 0;
            fail(e, rc, last_error());
        }
    }
    return int64_t(copied);
}

void mxec::enc_reader_free(EncReader* e) { delete e; }

extern "C" {

int mxec_reader_open_encrypted(mxec_ctx* ctx, const char* ec_dir, const uint8_t key[32], const uint8_t* aad_prefix,
                               uint32_t aad_prefix_len, uint32_t frame_size, uint64_t plaintext_size, uint64_t offset,
                               uint64_t length, uint64_t batch_bytes, mxec_reader** out) {
    return guarded([&]() -> int {
        if (!ctx || !ec_dir || !key || !out || (aad_prefix_len && !aad_prefix))
            return set_error(MXEC_E_INVALID_ARG, "null argument");
        *out = nullptr;
        if (frame_size == 0 || frame_size % 16)
            return set_error(MXEC_E_INVALID_ARG, "frame_size must be a positive multiple of 16");
        if (frame_size > 0x7FFFFF00u) return set_error(MXEC_E_INVALID_ARG, "frame_size must be below 2^31 for a window");
        auto r = std::make_unique<mxec_reader>();
        MXEC_TRY(read_manifest(ec_dir, r->man));
        r->ctx = ctx;
        r->dir = ec_dir;
        const Manifest& man = r->man;
        if (plaintext_size == UINT64_MAX) {
            if (!man.has_plain) return set_error(MXEC_E_JSON, "JSON error: manifest has no plaintext_size");
            plaintext_size = man.plaintext_size;
        }
        r->enc = new EncReader();
        EncReader& e = *r->enc;
        e.dir = &r->dir;
        e.man = &r->man;
        const bool reads = offset < plaintext_size && length && man.total_size > 0;
        if (reads && man.chunk_size == 0) return set_error(MXEC_E_JSON, "JSON error: chunk_size is 0");
        e.sa = round_up(std::max<uint64_t>(man.chunk_size, 1), kSlotAlign);
        e.plan = ReadPlan::make(frame_size, plaintext_size, man.total_size, std::max<uint64_t>(man.chunk_size, 1), offset,
                                length, batch_bytes ? batch_bytes : kDefaultBatch);
        const ReadPlan& p = e.plan;
        if (p.c_end > man.chunk_count || p.c_end > man.chunks.size())
            return set_error(MXEC_E_JSON, "JSON error: range past chunk_count");
        for (uint64_t j = p.c0; j < p.c_end; ++j)
            if (man.chunks[size_t(j)].size != p.chunk_len(j))
                return set_error(MXEC_E_JSON, "JSON error: chunk " + std::to_string(j) + " is not its share of total_size");
        e.loaded = p.c0;
        e.next_frame = p.f0;
        MXEC_TRY(open_enc(e, ctx, key, aad_prefix, aad_prefix_len));
        *out = r.release();
        return MXEC_OK;
    });
}

}  // extern "C"
