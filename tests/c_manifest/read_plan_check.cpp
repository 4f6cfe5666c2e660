// read_plan_check.cpp — maxio_amd/csrc/read_plan.hpp on its own, built with
// -fsanitize=address,undefined by tests/test_reader_encrypted_abi.py: the
// streaming encrypted GET's rounds are played over a model of the ring of
// chunk slots, for many geometries and ranges, and every step is checked:
//   * every frame the range needs is decrypted exactly once, in order;
//   * no frame is decrypted before its last byte is resident (every chunk it
//     touches is in its slot);
//   * no slot is overwritten while a pending frame touches its chunk;
//   * a round has room for at least one chunk, never holds more chunks than
//     the ring has slots, and a launch's frames span at most slots * chunk_size;
//   * the plaintext bytes served add up to the range.
// Prints "ok <cases> <rounds>"; a failed check prints the case and exits 1.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../../maxio_amd/csrc/read_plan.hpp"

using namespace mxec;

namespace {

uint64_t g_cases = 0, g_rounds = 0;

struct Case {
    uint64_t fs, plain, total, cs, off, len, batch;
};

[[noreturn]] void fail(const Case& c, const char* what, uint64_t a = 0, uint64_t b = 0) {
    std::printf("FAILED %s (%" PRIu64 ", %" PRIu64 "): fs %" PRIu64 " plain %" PRIu64 " total %" PRIu64 " cs %" PRIu64
                " off %" PRIu64 " len %" PRIu64 " batch %" PRIu64 "\n",
                what, a, b, c.fs, c.plain, c.total, c.cs, c.off, c.len, c.batch);
    std::exit(1);
}

uint64_t stream_len(uint64_t plain, uint64_t fs) { return plain + 28 * (plain ? (plain - 1) / fs + 1 : 0); }

// Plays the reader's loop (storage_reader_enc.cpp next_round) over the plan.
void play(const Case& c) {
    ++g_cases;
    const ReadPlan p = ReadPlan::make(c.fs, c.plain, c.total, c.cs, c.off, c.len, c.batch);
    // What the buffered call serves (mxec_get_object_chunked_encrypted).
    uint64_t want_bytes = 0;
    if (c.off < c.plain && c.len) want_bytes = c.len > c.plain - c.off ? c.plain - c.off : c.len;
    if (p.end - p.off != want_bytes) fail(c, "range", p.end - p.off, want_bytes);
    if (p.empty()) return;
    if (p.f0 != c.off / c.fs || p.f_end != (c.off + want_bytes - 1) / c.fs + 1) fail(c, "frames", p.f0, p.f_end);
    const bool truncated = p.frame_end(p.f_end - 1) > c.total;
    if (p.c0 == p.c_end) {
        if (!truncated || p.frame_off(p.f0) < c.total) fail(c, "no chunk read of a stream that holds a frame");
        return;
    }
    if (p.slots == 0 || p.slots > p.c_end - p.c0) fail(c, "slots", p.slots, p.c_end - p.c0);
    const uint64_t touch_most = (p.fl + c.cs - 2) / c.cs + 1;  // chunks a frame can touch, at the worst phase
    if (p.slots < p.c_end - p.c0 && p.slots < touch_most + 1) fail(c, "fewer slots than a frame touches plus one", p.slots);
    std::vector<uint64_t> slot(p.slots, UINT64_MAX);  // the chunk in each slot
    std::map<uint64_t, int> done;
    uint64_t loaded = p.c0, next = p.f0, served = 0;
    while (loaded < p.c_end) {
        ++g_rounds;
        const ReadChunks r = p.round(loaded, next);
        if (r.first != loaded || r.count == 0 || loaded + r.count > p.c_end) fail(c, "round", r.first, r.count);
        const uint64_t held = p.held_from(next);
        if (loaded - held + r.count > p.slots) fail(c, "more chunks than slots", loaded - held, r.count);
        uint64_t bytes = 0;
        for (uint64_t j = loaded; j < loaded + r.count; ++j) {
            bytes += p.chunk_len(j);
            uint64_t& s = slot[j % p.slots];
            if (s != UINT64_MAX && s >= held) fail(c, "overwrites a chunk a pending frame touches", j, s);
            s = j;
        }
        if (r.count > 1 && bytes > c.batch) fail(c, "round above batch_bytes", bytes);
        loaded += r.count;
        const uint64_t resident = p.resident_end(loaded);
        const uint64_t g = p.frames_whole(next, resident);
        if (g < next || g > p.f_end) fail(c, "frames_whole", next, g);
        for (uint64_t f = next; f < g; ++f) {
            const uint64_t a = p.frame_off(f), e = p.frame_end(f);
            if (e > resident || e > c.total) fail(c, "decrypted before its last byte is resident", f, e);
            for (uint64_t j = a / c.cs; j <= (e - 1) / c.cs; ++j)
                if (slot[j % p.slots] != j) fail(c, "a chunk of the frame is not in its slot", f, j);
            if (++done[f] != 1) fail(c, "decrypted twice", f);
        }
        if (g < p.f_end && p.frame_end(g) <= resident) fail(c, "a whole frame left waiting", g);
        if (g > next && p.frame_end(g - 1) - p.frame_off(next) > p.slots * c.cs)
            fail(c, "a launch wider than the window", next, g);
        const ReadSpan w = p.want(next, g);
        if (g > next) {
            const uint64_t lo = next * c.fs + w.dev_off;
            if (lo != c.off + served) fail(c, "span does not continue the range", lo, served);
            if (w.dev_off >= c.fs && w.len) fail(c, "skip beyond the first frame", w.dev_off);
        }
        served += w.len;
        const ReadChunks rel = p.releases(next, g);
        if (rel.first != held || rel.first + rel.count != p.held_from(g)) fail(c, "releases", rel.first, rel.count);
        next = g;
    }
    if (!truncated) {
        if (next != p.f_end) fail(c, "frames left", next, p.f_end);
        if (served != want_bytes) fail(c, "bytes served", served, want_bytes);
    } else if (next == p.f_end) {
        fail(c, "a truncated frame was decrypted");
    }
    for (uint64_t f = p.f0; f < next; ++f)
        if (done[f] != 1) fail(c, "needed frame not decrypted", f);
}

void ranges(uint64_t fs, uint64_t plain, uint64_t total, uint64_t cs, const std::vector<uint64_t>& batches) {
    std::vector<uint64_t> offs, lens = {UINT64_MAX, UINT64_MAX - 1, 0, 1, fs - 1, fs, fs + 1, 3 * fs, plain};
    if (total / cs > 5000) lens = {UINT64_MAX, 1, fs + 1};  // thousands of rounds a range: fewer of them
    const uint64_t nf = plain ? (plain - 1) / fs + 1 : 0;
    for (uint64_t f : {uint64_t(0), uint64_t(1), nf / 2, nf ? nf - 1 : 0})
        for (int d = -1; d <= 1; ++d) offs.push_back(f * fs + uint64_t(d));  // every frame edge; -1 of 0 wraps to 2^64 - 1
    offs.push_back(plain);
    offs.push_back(plain + 5);
    for (uint64_t b : batches)
        for (uint64_t o : offs)
            for (uint64_t l : lens) play({fs, plain, total, cs, o, l, b});
}

}  // namespace

int main() {
    const uint64_t kChunks[] = {1, 7, 91, 92, 93, 101, uint64_t(1) << 20};
    const uint64_t kFrames[] = {16, 64, 65536};
    for (uint64_t fs : kFrames)
        for (uint64_t cs : kChunks) {
            // a handful of frames, the last one short, whole, or one byte long
            const uint64_t frames = cs == 1 && fs == 65536 ? 2 : 5;
            for (uint64_t plain : {frames * fs + 13, frames * fs, frames * fs + 1, uint64_t(1), uint64_t(0)}) {
                const uint64_t total = stream_len(plain, fs);
                // one chunk per round, a few, the default
                ranges(fs, plain, total, cs, {1, cs, 250, 3 * cs + 1, uint64_t(64) << 20});
                // a stream cut short, and one with bytes left over
                if (total > 5) ranges(fs, plain, total - 5, cs, {1, uint64_t(64) << 20});
                ranges(fs, plain, total + 40, cs, {1, uint64_t(64) << 20});
            }
        }
    // 101 frames of 92 bytes against chunks of 101: a boundary at every frame offset
    ranges(64, 101 * 64, stream_len(101 * 64, 64), 101, {1, 250, uint64_t(64) << 20});
    // lengths near 2^64: ranges high up in objects whose streams just fit
    for (uint64_t fs : kFrames)
        for (uint64_t cs : {uint64_t(1) << 20, uint64_t(1) << 40}) {
            const uint64_t plain = (UINT64_MAX / (fs + 28)) * fs - fs + 3;  // its stream ends below 2^64
            const uint64_t total = stream_len(plain, fs);
            const uint64_t nf = (plain - 1) / fs + 1;
            for (uint64_t o : {plain - 1, plain - 3, plain - 4, (nf - 3) * fs - 1, (nf - 3) * fs, (nf - 3) * fs + 1, plain, UINT64_MAX})
                for (uint64_t l : {UINT64_MAX, UINT64_MAX - o, uint64_t(1), 2 * fs + 7})
                    for (uint64_t b : {uint64_t(1), uint64_t(64) << 20}) play({fs, plain, total, cs, o, l, b});
        }
    std::printf("ok %" PRIu64 " %" PRIu64 "\n", g_cases, g_rounds);
    return 0;
}
