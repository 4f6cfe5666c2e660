// writer_plan.hpp — the arithmetic of the streaming PUT (storage_writer.cpp,
// put_object_chunked filesystem.rs:686-773 as a push stream): how a declared
// length becomes chunks, how one write() is cut into per-chunk runs, which
// window slot a chunk takes and whose work it must wait for, and the over-run
// and short-finish errors, and which runs of the body digests are due as a
// chunk's bytes arrive.  Only integers; nothing is read or written.
//
// Host-only (no HIP, no I/O): storage_writer.cpp calls it, and
// tests/c_manifest/writer_plan_check.cpp and writer_sums_check.cpp run it on
// their own under -fsanitize=address,undefined.
#pragma once

#include <cstdint>
#include <string>

namespace mxec {

struct WriterPlan {
    uint64_t chunk_size = 0, total_len = 0;
    uint64_t k = 1;      // data chunks: ceil(total_len / chunk_size), 1 for an empty body (:740-743)
    uint64_t slots = 2;  // chunks resident in the window at once

    // chunk_size > 0.  window_bytes: 0 = kDefaultSlots chunks; at least two
    // chunks are used, never more than k.
    static constexpr uint64_t kDefaultSlots = 4;
    static WriterPlan make(uint64_t chunk_size, uint64_t total_len, uint64_t window_bytes) {
        WriterPlan p;
        p.chunk_size = chunk_size;
        p.total_len = total_len;
        // (total_len - 1) / chunk_size + 1: no carry past 2^64 as total_len + chunk_size - 1 has.
        p.k = total_len == 0 ? 1 : (total_len - 1) / chunk_size + 1;
        uint64_t s = window_bytes == 0 ? kDefaultSlots : window_bytes / chunk_size;
        if (s < 2) s = 2;
        p.slots = s < p.k ? s : p.k;
        return p;
    }
    // Chunk j's length: chunk_size but for the last, which is never padded.
    uint64_t chunk_len(uint64_t j) const { return j + 1 < k ? chunk_size : total_len - (k - 1) * chunk_size; }
    // The window slot chunk j lives in, and the chunk whose hash and parity
    // pass must have finished before j's first byte goes there (j >= slots).
    uint64_t slot_of(uint64_t j) const { return j % slots; }
    bool reuses(uint64_t j) const { return j >= slots; }
    uint64_t evicts(uint64_t j) const { return j - slots; }
};

// One stretch of a write() that lies in one chunk.
struct WriterRun {
    uint64_t chunk;      // its chunk
    uint64_t at;         // offset within the chunk
    uint64_t src;        // offset within the write()'s buffer
    uint64_t len;        // > 0
    bool opens;          // the chunk's first byte
    bool completes;      // the chunk's last byte
};

// Writing past the declared length: refused whole, before any byte is taken.
inline bool writer_overruns(const WriterPlan& p, uint64_t written, uint64_t len) {
    return len > p.total_len - written;
}
inline std::string writer_overrun_msg(const WriterPlan& p, uint64_t written, uint64_t len) {
    return "write of " + std::to_string(len) + " bytes at " + std::to_string(written) + " runs past the " +
           std::to_string(p.total_len) + " declared bytes";
}
inline std::string writer_short_msg(const WriterPlan& p, uint64_t written) {
    return "body ended at " + std::to_string(written) + " of " + std::to_string(p.total_len) + " declared bytes";
}

// The runs of a write of `len` bytes with `written` bytes before it (no
// over-run: writer_overruns first), in order, to f(run) -> status; stops at
// the first non-zero status and returns it.  A zero-length write has no run.
// An empty body's one empty chunk never sees a run: finish() completes it.
template <class F>
int writer_cut(const WriterPlan& p, uint64_t written, uint64_t len, F&& f) {
    uint64_t src = 0;
    while (src < len) {
        WriterRun r;
        r.chunk = written / p.chunk_size;
        r.at = written - r.chunk * p.chunk_size;
        const uint64_t room = p.chunk_len(r.chunk) - r.at;
        r.len = len - src < room ? len - src : room;
        r.src = src;
        r.opens = r.at == 0;
        r.completes = r.len == room;
        if (const int rc = f(r)) return rc;
        src += r.len;
        written += r.len;
    }
    return 0;
}

// The body digests of a writer opened with them advance in runs over bytes
// already in the window: a run ends at its chunk's end or at each whole
// kSumRun of the chunk, whichever comes first, so every chunk is tiled exactly
// once and a run never crosses a slot.  The body's first run starts its
// chains, its last one ends them.  An empty body's one empty chunk is one
// empty run, first and last.
constexpr uint64_t kSumRun = uint64_t(1) << 20;
struct SumRun {
    uint64_t chunk;
    uint64_t at;   // offset within the chunk, a multiple of kSumRun
    uint64_t len;  // <= kSumRun; 0 only for the empty body
    bool first;    // of the body
    bool last;     // of the body
    bool closes;   // the chunk's last run: its slot may be reused once this has run
};

// How many runs a chunk has.
inline uint64_t writer_sum_runs_of(const WriterPlan& p, uint64_t chunk) {
    const uint64_t len = p.chunk_len(chunk);
    return len == 0 ? 1 : (len - 1) / kSumRun + 1;
}

// The runs of `chunk` that become due when its uploaded bytes grow from
// `from` to `to` (from < to <= the chunk's length, or 0 and 0 for the empty
// body's chunk): those whose last byte lies in [from, to).  In order, to
// f(run) -> status; stops at the first non-zero status and returns it.
template <class F>
int writer_sum_due(const WriterPlan& p, uint64_t chunk, uint64_t from, uint64_t to, F&& f) {
    const uint64_t len = p.chunk_len(chunk);
    uint64_t at = from / kSumRun * kSumRun;  // the run that byte `from` lies in
    for (;;) {
        // at + kSumRun may pass 2^64 in a chunk that ends near it; len - at does not.
        const uint64_t end = len - at <= kSumRun ? len : at + kSumRun;
        if (end > to) return 0;
        SumRun r;
        r.chunk = chunk;
        r.at = at;
        r.len = end - at;
        r.first = chunk == 0 && at == 0;
        r.closes = end == len;
        r.last = r.closes && chunk + 1 == p.k;
        if (const int rc = f(r)) return rc;
        if (r.closes) return 0;
        at = end;
    }
}

}  // namespace mxec
