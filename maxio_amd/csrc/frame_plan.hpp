// frame_plan.hpp — the arithmetic of the streaming encrypted PUT
// (storage_writer.cpp, put_object_chunked_encrypted filesystem.rs:835-1060 as a
// push stream; frames of crypto.rs:94-117): how a plaintext length becomes a
// frame stream, which frames are whole once so much plaintext has arrived and
// which encrypt launches are then due, where frame f lies in the stream, which
// stretches of a ring of chunk slots a range of the stream occupies, and which
// chunks a range completes.  Only integers; nothing is read or written.
//
// Host-only (no HIP, no I/O): storage_writer.cpp calls it, and
// tests/c_manifest/frame_plan_check.cpp runs it on its own under
// -fsanitize=address,undefined.
#pragma once

#include <cstdint>

namespace mxec {

constexpr uint64_t kFramePlain = 65536;                      // FRAME_CHUNK_SIZE (crypto.rs)
constexpr uint64_t kFrameExtra = 28;                         // nonce(12) + tag(16)
constexpr uint64_t kFrameBytes = kFramePlain + kFrameExtra;  // a whole frame in the stream

// Frames of a plaintext: ceil(plain / 64 KiB), none for an empty one.
inline uint64_t frame_count(uint64_t plain) { return plain == 0 ? 0 : (plain - 1) / kFramePlain + 1; }

// The frame stream's length; false when it does not fit in 64 bits (a
// plaintext within 2^64 / 2341 of 2^64).
inline bool frame_stream_len(uint64_t plain, uint64_t* out) {
    const uint64_t extra = kFrameExtra * frame_count(plain);  // < 2^54
    if (plain > UINT64_MAX - extra) return false;
    *out = plain + extra;
    return true;
}

// Frame f (< frame_count): its plaintext bytes, and its place in the stream.
inline uint64_t frame_plain_len(uint64_t plain, uint64_t f) {
    const uint64_t left = plain - f * kFramePlain;
    return left < kFramePlain ? left : kFramePlain;
}
inline uint64_t frame_stream_off(uint64_t f) { return f * kFrameBytes; }
inline uint64_t frame_stream_len_of(uint64_t plain, uint64_t f) { return frame_plain_len(plain, f) + kFrameExtra; }

// Frames that are whole once `at` (<= plain) plaintext bytes have arrived: a
// frame is whole with its last byte, the body's short last frame with the
// body's.
inline uint64_t frames_whole(uint64_t plain, uint64_t at) { return at == plain ? frame_count(plain) : at / kFramePlain; }

// The frames that become due when the plaintext grows from `from` to `to`
// (from <= to <= plain): [first, first + count).
struct FrameSpan {
    uint64_t first, count;
};
inline FrameSpan frames_due(uint64_t plain, uint64_t from, uint64_t to) {
    const uint64_t a = frames_whole(plain, from);
    return {a, frames_whole(plain, to) - a};
}

// One encrypt launch: the whole frames of one kEncRun-aligned stretch of the
// plaintext.  However small the writes are, a launch is due only with its
// stretch's last byte (or the body's), so there is one launch per MiB, never
// one per frame or per write.
constexpr uint64_t kEncFrames = 16;
constexpr uint64_t kEncRun = kEncFrames * kFramePlain;        // 1 MiB of plaintext
constexpr uint64_t kEncRunStream = kEncFrames * kFrameBytes;  // ... is at most this much of the stream
struct EncRun {
    uint64_t index;        // plaintext [index * kEncRun, + plain_len)
    uint64_t plain_len;    // <= kEncRun; > 0
    uint64_t first_frame;  // = index * kEncFrames
    uint64_t frames;       // <= kEncFrames
    uint64_t stream_off;   // of its first frame
    uint64_t stream_len;
    bool last;             // of the body
};
inline uint64_t enc_run_count(uint64_t plain) { return plain == 0 ? 0 : (plain - 1) / kEncRun + 1; }
inline EncRun enc_run(uint64_t plain, uint64_t r) {
    EncRun e;
    e.index = r;
    const uint64_t left = plain - r * kEncRun;
    e.plain_len = left < kEncRun ? left : kEncRun;
    e.first_frame = r * kEncFrames;
    e.frames = (e.plain_len - 1) / kFramePlain + 1;
    e.stream_off = frame_stream_off(e.first_frame);
    e.stream_len = e.plain_len + kFrameExtra * e.frames;
    e.last = left <= kEncRun;
    return e;
}
// The launches that become due when the plaintext grows from `from` to `to`
// (from < to <= plain): those whose last byte lies in [from, to).  In order, to
// f(run) -> status; stops at the first non-zero status and returns it.
template <class F>
int enc_runs_due(uint64_t plain, uint64_t from, uint64_t to, F&& f) {
    for (uint64_t r = from / kEncRun; r < enc_run_count(plain); ++r) {
        const EncRun e = enc_run(plain, r);
        // The run's last byte is at r * kEncRun + plain_len - 1 (no carry: it is below plain).
        if (r * kEncRun + (e.plain_len - 1) >= to) return 0;
        if (const int rc = f(e)) return rc;
    }
    return 0;
}

// A ring of chunk slots: stream byte x lives in slot (x / chunk_size) % slots
// at x % chunk_size (mxec_frames_window).  The stretches of the ring that the
// stream range [off, off + len) occupies, in stream order, to
// f(slot, at, src, len) -> status (src: offset within the range); stops at the
// first non-zero status and returns it.  A range that ends exactly on a chunk
// boundary has no empty stretch after it.
template <class F>
int ring_segments(uint64_t chunk_size, uint64_t slots, uint64_t off, uint64_t len, F&& f) {
    uint64_t src = 0;
    while (src < len) {
        const uint64_t chunk = off / chunk_size, at = off - chunk * chunk_size;
        const uint64_t room = chunk_size - at, n = len - src < room ? len - src : room;
        if (const int rc = f(chunk % slots, at, src, n)) return rc;
        src += n;
        off += n;  // may wrap to 0 with the range's last byte at 2^64 - 1; the loop has then ended
    }
    return 0;
}

// The chunks that the stream range [off, off + len) completes, of a stream of
// `total` bytes in chunks of chunk_size: [first, first + count).  A chunk is
// complete with its last byte, the short last chunk with the stream's.
inline uint64_t chunks_whole(uint64_t chunk_size, uint64_t total, uint64_t at) {
    if (total == 0) return 0;  // the empty body's one empty chunk is finish()'s
    return at == total ? (total - 1) / chunk_size + 1 : at / chunk_size;
}
inline FrameSpan chunks_completed(uint64_t chunk_size, uint64_t total, uint64_t off, uint64_t len) {
    const uint64_t a = chunks_whole(chunk_size, total, off);
    return {a, chunks_whole(chunk_size, total, off + len) - a};
}

}  // namespace mxec
