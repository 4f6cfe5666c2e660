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
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <cstring>

#include "ops.hpp"
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

    uint8_t* slot_ptr(uint64_t slot) const { return static_cast<uint8_t*>(window.p) + slot * sa; }
    uint8_t* parity_set(int which) const { return static_cast<uint8_t*>(parity.p) + uint64_t(which) * m * sa; }

    ~mxec_writer() {
        if (fd >= 0) ::close(fd);
        if (!dev) return;
        (void)hipSetDevice(dev->id);
        // Nothing of ours may still run when the buffers go.
        if (s) (void)hipStreamSynchronize(s);
        if (sum_s) {
            (void)hipStreamSynchronize(sum_s);
            affinity_untag(sum_s);
            (void)hipStreamDestroy(sum_s);
        }
        if (sums_done) (void)hipEventDestroy(sums_done);
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
    if (w.which) MXEC_HIP(hipEventSynchronize(ws.summed));  // queued before the chunk completed
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

int finish(mxec_writer& w) {
    if (w.written != w.plan.total_len) return set_error(MXEC_E_INVALID_ARG, writer_short_msg(w.plan, w.written));
    if (w.plan.total_len == 0) {  // one empty chunk (:740-743), no parity (:748)
        MXEC_TRY(open_chunk_file(w, 0));
        MXEC_TRY(close_chunk_file(w, 0));
        if (w.which)  // one empty run, first and last
            MXEC_TRY(writer_sum_due(w.plan, 0, 0, 0, [&](const SumRun& q) { return queue_sum_run(w, q); }));
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

int open_writer(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size, uint32_t parity_shards, uint64_t total_len,
                uint64_t plaintext_size, uint64_t window_bytes, uint32_t which, void** out) {
    return guarded([&]() -> int {
        if (!ctx || !ec_dir || !out) return set_error(MXEC_E_INVALID_ARG, "null argument");
        *out = nullptr;
        if (chunk_size == 0) return set_error(MXEC_E_INVALID_ARG, "chunk_size must be > 0");
        if (which & ~uint32_t(0x1F)) return set_error(MXEC_E_INVALID_ARG, "unknown digest flag");
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
            MXEC_TRY(w->stage[b].ensure(size_t(std::min(kPiece, std::max<uint64_t>(chunk_size, 4096)))));
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
                MXEC_TRY(new_event(&ws.summed));
                ws.sum_tables.owner = d;
                MXEC_TRY(ws.sum_tables.reserve(std::max<size_t>(4096, size_t(writer_sum_runs_of(w->plan, 0)) * kSumRunTables)));
            }
        }
        w->sha.resize(size_t(w->plan.k + w->m));
        std::error_code ec;
        fs::create_directories(w->dir, ec);
        if (ec) return set_error(MXEC_E_IO, "IO error: " + ec.message());
        *out = w.release();
        return MXEC_OK;
    });
}

}  // namespace

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

int mxec_writer_write(void* wp, const uint8_t* buf, uint64_t len) {
    return guarded([&]() -> int {
        auto* w = static_cast<mxec_writer*>(wp);
        if (!w || (len && !buf)) return set_error(MXEC_E_INVALID_ARG, "null argument");
        if (w->err) return set_error(w->err, w->err_msg);
        if (w->finished) return set_error(MXEC_E_INVALID_ARG, "write after finish");
        if (writer_overruns(w->plan, w->written, len))
            return poison(*w, set_error(MXEC_E_INVALID_ARG, writer_overrun_msg(w->plan, w->written, len)));
        MXEC_HIP(hipSetDevice(w->dev->id));
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
