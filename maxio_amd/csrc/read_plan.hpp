// read_plan.hpp — the arithmetic of the streaming encrypted GET
// (storage_reader_enc.cpp: FrameDecryptor::for_range over VerifiedChunkReader,
// crypto.rs:186-420, filesystem.rs:1618-1630, :1700-1725, as a pull stream):
// which frames a plaintext range needs and which stream bytes and chunks hold
// them, how many chunks a round takes and how many slots the ring of chunk
// slots needs, which frames are whole once so many chunks are resident, which
// chunks a decrypted frame releases, and what the first and the last frame of
// a range skip.  Only integers; nothing is read or written.
//
// Host-only (no HIP, no I/O): storage_reader_enc.cpp calls it, and
// tests/c_manifest/read_plan_check.cpp runs it on its own under
// -fsanitize=address,undefined.
#pragma once

#include <cstdint>

namespace mxec {

constexpr uint64_t kReadFrameExtra = 28;  // nonce(12) + tag(16)

// Products and sums that stop at 2^64 - 1: a stream position up there lies
// beyond every stream, which is all that is asked of it.
inline uint64_t read_mul_sat(uint64_t a, uint64_t b) { return b && a > UINT64_MAX / b ? UINT64_MAX : a * b; }
inline uint64_t read_add_sat(uint64_t a, uint64_t b) { return a > UINT64_MAX - b ? UINT64_MAX : a + b; }

struct ReadChunks {
    uint64_t first, count;
};
struct ReadSpan {
    uint64_t dev_off, len;  // of a launch's contiguous plaintext: what the range wants of it
};

struct ReadPlan {
    uint64_t fs = 0, fl = 0;          // a frame's plaintext bytes and its bytes in the stream
    uint64_t plain = 0;               // the object's plaintext bytes
    uint64_t total = 0;               // the frame stream as stored (manifest total_size)
    uint64_t cs = 0;                  // chunk_size
    uint64_t off = 0, end = 0;        // the plaintext range [off, end), clamped; off == end: nothing to serve
    uint64_t f0 = 0, f_end = 0;       // frames [f0, f_end) cover it
    uint64_t ct_off = 0, ct_end = 0;  // the stream bytes read: those frames, as far as the stream goes
    uint64_t c0 = 0, c_end = 0;       // chunks [c0, c_end) hold them
    uint64_t batch = 0;               // a round's chunk bytes (at least one chunk)
    uint64_t round_max = 0;           // ... and its chunks at the most
    uint64_t slots = 0;               // the ring: chunk j lives in slot j % slots

    // fs: a positive multiple of 16; cs > 0; length == UINT64_MAX: to the end.
    static ReadPlan make(uint64_t fs, uint64_t plain, uint64_t total, uint64_t cs, uint64_t offset, uint64_t length,
                         uint64_t batch_bytes) {
        ReadPlan p;
        p.fs = fs;
        p.fl = fs + kReadFrameExtra;
        p.plain = plain;
        p.total = total;
        p.cs = cs;
        p.batch = batch_bytes;
        if (offset >= plain || length == 0) return p;  // FrameDecryptor::for_range of nothing
        p.off = offset;
        p.end = length > plain - offset ? plain : offset + length;
        p.f0 = p.off / fs;
        p.f_end = (p.end - 1) / fs + 1;
        p.ct_off = read_mul_sat(p.f0, p.fl);
        p.ct_end = p.frame_end(p.f_end - 1);  // the plaintext's last frame may be short
        if (p.ct_end > total) p.ct_end = total;
        if (p.ct_off >= p.ct_end) {  // the stream ends before the first frame: no chunk is read
            p.ct_off = p.ct_end = 0;
            return p;
        }
        p.c0 = p.ct_off / cs;
        p.c_end = (p.ct_end - 1) / cs + 1;
        const uint64_t nc = p.c_end - p.c0;
        p.round_max = batch_bytes / cs + 1;  // the short last chunk may come on top of batch_bytes / cs whole ones
        // One frame touches at most `touch` chunks; while it waits for its last
        // byte, fewer than that are held, and a round's come on top.  Never
        // fewer slots than one frame can touch plus one, never more than the
        // range has chunks.
        const uint64_t touch = (p.fl - 1) / cs + 2;
        uint64_t want = read_add_sat(p.round_max, touch - 1);
        if (want < touch + 1) want = touch + 1;
        p.slots = want < nc ? want : nc;
        if (p.round_max > p.slots) p.round_max = p.slots;
        return p;
    }

    bool empty() const { return off == end; }
    uint64_t chunk_len(uint64_t j) const {
        const uint64_t at = j * cs;  // below total
        return total - at < cs ? total - at : cs;
    }
    uint64_t frame_plain(uint64_t f) const {
        const uint64_t left = plain - f * fs;
        return left < fs ? left : fs;
    }
    uint64_t frame_off(uint64_t f) const { return read_mul_sat(f, fl); }
    uint64_t frame_end(uint64_t f) const { return read_add_sat(frame_off(f), frame_plain(f) + kReadFrameExtra); }

    // The stream bytes resident once chunks [c0, upto) are: [ct_off, this).
    uint64_t resident_end(uint64_t upto) const {
        const uint64_t e = read_mul_sat(upto, cs);
        return e < total ? e : total;
    }

    // Frames [next, result) are whole in stream bytes below `resident`
    // (next <= result <= f_end).  Every frame but the plaintext's last is fl
    // bytes long.
    uint64_t frames_whole(uint64_t next, uint64_t resident) const {
        if (next >= f_end) return f_end;
        const uint64_t last = (plain - 1) / fs;  // plain > 0: the range is not empty
        uint64_t g = resident / fl;              // frames of fl bytes that end at or below `resident`
        if (g >= last) g = frame_end(last) <= resident ? last + 1 : last;
        if (g > f_end) g = f_end;
        return g < next ? next : g;
    }

    // The first chunk still wanted once frames below `next` are decrypted:
    // chunks below it may be overwritten.
    uint64_t held_from(uint64_t next) const {
        if (next >= f_end) return c_end;
        const uint64_t c = frame_off(next) / cs;
        return c < c0 ? c0 : c > c_end ? c_end : c;
    }
    ReadChunks releases(uint64_t next_before, uint64_t next_after) const {
        const uint64_t a = held_from(next_before);
        return {a, held_from(next_after) - a};
    }

    // The next round: chunks from `loaded` (all below it are resident or
    // released) while they fit in `batch` bytes, at least one, no more than
    // the ring has room for beside the chunks frame `next` still holds.
    ReadChunks round(uint64_t loaded, uint64_t next) const {
        if (loaded >= c_end) return {loaded, 0};
        const uint64_t held = loaded - held_from(next);
        uint64_t room = slots - held;  // >= 1: read_plan_check.cpp
        if (room > round_max) room = round_max;
        if (room > c_end - loaded) room = c_end - loaded;
        uint64_t n = 1, bytes = chunk_len(loaded);
        while (n < room && bytes + chunk_len(loaded + n) <= batch) bytes += chunk_len(loaded + n++);
        return {loaded, n};
    }

    // Frames [a, g) decrypted into one contiguous run from a's first byte on:
    // what of it the range wants.  The first frame of a range skips its head,
    // the last its tail.
    ReadSpan want(uint64_t a, uint64_t g) const {
        if (a >= g) return {0, 0};
        const uint64_t base = a * fs;
        const uint64_t lo = off > base ? off : base;
        uint64_t hi = g - 1 == (plain - 1) / fs ? plain : g * fs;
        if (hi > end) hi = end;
        return {lo - base, hi > lo ? hi - lo : 0};
    }
};

}  // namespace mxec
