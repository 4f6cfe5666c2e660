// part_plan_check.cpp — maxio_amd/csrc/part_plan.hpp against a byte-by-byte
// model, on its own under -fsanitize=address,undefined
// (tests/test_multipart_streamed_abi.py builds and runs it).
//
// For every part list and ring size: the parts lie end to end in the body; an
// encrypted part's file length is size + 28 per 64 KiB frame; the feed steps
// produce every plaintext byte exactly once, in body order, a launch's bytes
// at (body offset) % ring; no launch carries more than 16 frames or more
// plaintext than the ring; a job's file range is its frames'; the stretches a
// launch opens are those whose first byte it writes; and there are no more
// launches than ceil(frames / 16) + plain<->encrypted transitions + 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../maxio_amd/csrc/part_plan.hpp"

using namespace mxec;

namespace {

int g_case = 0;

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) {                                                                     \
            std::fprintf(stderr, "case %d line %d: %s\n", g_case, __LINE__, #c);       \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

constexpr uint64_t FS = 65536, MIB = uint64_t(1) << 20;

void run(const std::vector<PartSpec>& parts, uint64_t ring) {
    ++g_case;
    const PartPlan p = part_plan(parts.data(), parts.size(), ring);
    CHECK(p.ok);
    CHECK(p.parts.size() == parts.size());
    uint64_t body = 0, frames = 0, transitions = 0;
    for (size_t i = 0; i < parts.size(); ++i) {
        const PartInfo& pi = p.parts[i];
        CHECK(pi.body_off == body && pi.size == parts[i].size && pi.encrypted == parts[i].encrypted);
        if (pi.encrypted) {
            const uint64_t nf = (pi.size + FS - 1) / FS;
            CHECK(pi.frames == nf && pi.file_len == pi.size + 28 * nf);
            frames += nf;
        }
        if (i && parts[i].encrypted != parts[i - 1].encrypted) ++transitions;
        body += pi.size;
    }
    CHECK(p.body_len == body);
    // The model: who produced each body byte, and where the ring says it went.
    std::vector<uint8_t> made(size_t(body), 0);
    uint64_t at = 0, launches = 0, opened = 0;
    const int rc = part_feed(p, [&](const FeedStep& s) -> int {
        CHECK(s.body_off == at && s.body_end > s.body_off && s.body_end <= body);
        if (!s.launch) {
            const PartInfo& pi = p.parts[s.part];
            CHECK(!pi.encrypted && s.len > 0 && s.len <= kFeedPiece && s.part_off + s.len <= pi.size);
            CHECK(pi.body_off + s.part_off == s.body_off && s.body_end == s.body_off + s.len);
            for (uint64_t b = 0; b < s.len; ++b) CHECK(made[size_t(s.body_off + b)]++ == 0);
            at = s.body_end;
            return 0;
        }
        ++launches;
        CHECK(s.n_jobs >= 1 && s.n_jobs <= kFeedFrames && s.frames >= 1 && s.frames <= 16);
        CHECK(s.body_end - s.body_off <= ring);
        uint64_t nf = 0, x = s.body_off;
        for (uint32_t j = 0; j < s.n_jobs; ++j) {
            const FeedJob& q = s.jobs[j];
            const PartInfo& pi = p.parts[q.part];
            CHECK(pi.encrypted && q.frames >= 1 && q.first_frame + q.frames <= pi.frames);
            CHECK(j == 0 || s.jobs[j - 1].part < q.part);  // one job per part it draws from
            CHECK(q.file_off == q.first_frame * (FS + 28));
            CHECK(q.stream_bytes == q.plain_bytes + 28 * q.frames && q.file_off + q.stream_bytes <= pi.file_len);
            const uint64_t start = q.first_frame * FS;
            CHECK(q.plain_bytes > 0 && start + q.plain_bytes <= pi.size);
            // whole frames, but for the part's last
            CHECK(q.plain_bytes == q.frames * FS || (q.first_frame + q.frames == pi.frames && start + q.plain_bytes == pi.size));
            CHECK((q.plain_bytes + FS - 1) / FS == q.frames);
            CHECK(pi.body_off + start == x);  // jobs lie end to end
            CHECK(q.ring_off < ring);
            for (uint64_t o = 0; o < q.plain_bytes; ++o) {
                CHECK((q.ring_off + o) % ring == (x + o) % ring);
                CHECK(made[size_t(x + o)]++ == 0);
            }
            x += q.plain_bytes;
            nf += q.frames;
        }
        CHECK(nf == s.frames && x == s.body_end);
        // the stretches whose first byte lies in [body_off, body_end)
        uint64_t first = 0, count = 0;
        for (uint64_t r = s.body_off / MIB; r * MIB < s.body_end; ++r)
            if (r * MIB >= s.body_off) {
                if (!count) first = r;
                ++count;
            }
        CHECK(s.open_count == count && (count == 0 || s.open_first == first));
        opened += count;
        at = s.body_end;
        return 0;
    });
    CHECK(rc == 0 && at == body);
    for (uint64_t b = 0; b < body; ++b) CHECK(made[size_t(b)] == 1);
    CHECK(launches <= (frames + 15) / 16 + transitions + 1);
    if (frames == 0) CHECK(launches == 0);
    (void)opened;
    // a callback's status stops the feed and comes back
    if (body) CHECK(part_feed(p, [](const FeedStep&) { return 7; }) == 7);
}

std::vector<PartSpec> all(std::initializer_list<uint64_t> sizes, bool enc) {
    std::vector<PartSpec> v;
    for (uint64_t s : sizes) v.push_back({s, enc});
    return v;
}

}  // namespace

int main() {
    const uint64_t ring4 = 4 * MIB;
    for (bool enc : {true, false}) {
        run({}, ring4);
        run(all({0}, enc), 256);
        run(all({1}, enc), 256);
        run(all({0, 1, 0}, enc), 256);
        run(all({65535}, enc), ring4);
        run(all({65536}, enc), ring4);
        run(all({65537}, enc), ring4);
        run(all({65535, 65536, 65537}, enc), ring4);
        run(all({3 * FS, 16 * FS, 17 * FS}, enc), ring4);         // multiples of 64 KiB
        run(all({3 * FS + 1000, 40000, 16 * FS + 1}, enc), ring4);  // and sizes that are not
        run(std::vector<PartSpec>(40, PartSpec{1, enc}), 256);
        run(all({FS + 5, 1, 2 * FS, 0, FS - 1}, enc), ring4);
        // a body that wraps the ring several times, the wrap inside a part frame
        run(all({4 * MIB - 100, FS + 300}, enc), ring4);
        run(all({5 * MIB + 3, 8 * MIB, 777, 3 * MIB - 1}, enc), ring4);
        run(all({MIB + 77, 2 * MIB + 1, MIB - 5, 3 * MIB}, enc), MIB);
        run(all({MIB + 77, 2 * MIB + 1, MIB - 5, 3 * MIB}, enc), MIB + 12345);
    }
    // plain and encrypted alternating
    run({{100000, false}, {100000, true}, {100000, false}}, ring4);
    run({{100000, true}, {100000, false}, {100000, true}, {0, false}, {1, true}}, ring4);
    run({{3 * FS + 1000, true}, {40000, false}}, ring4);
    {
        std::vector<PartSpec> v;
        for (int i = 0; i < 12; ++i) v.push_back({uint64_t(i % 3 == 0 ? MIB + 5 : 70000 + 4096 * i), i % 2 == 0});
        run(v, ring4);
        run(v, MIB);
    }
    // lengths that do not fit, and a ring too small for a launch, are refused
    {
        const PartSpec big[2] = {{UINT64_MAX - 5, false}, {10, false}};
        if (part_plan(big, 2, ring4).ok) return 1;
        const PartSpec enc_big[1] = {{UINT64_MAX - 5, true}};
        if (part_plan(enc_big, 1, ring4).ok) return 1;
        const PartSpec two[1] = {{2 * MIB, true}};
        if (part_plan(two, 1, MIB - 1).ok || part_plan(two, 1, 0).ok) return 1;
        if (!part_plan(two, 1, 2 * MIB).ok || !part_plan(two, 1, MIB).ok) return 1;
    }
    std::printf("part_plan ok: %d cases\n", g_case);
    return 0;
}
