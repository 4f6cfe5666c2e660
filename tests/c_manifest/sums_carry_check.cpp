// Stand-alone harness for maxio_amd/csrc/sums_carry.hpp (the carry arithmetic
// of the resumable body digests), built with -fsanitize=address,undefined by
// tests/test_sums_update_abi.py.  No input.  It checks, and prints one line
// per check ("<name> ok <cases>"); the first failure prints the case to stderr
// and exits 2:
//   identity  every pending 0..63 x len 0..200: head + 64 * blocks + rest ==
//             pending + len, the new tail < 64, and the fields' meaning
//   pad       the padding block count (1 up to 55 pending bytes, 2 from 56)
//   replay    a 700-byte message cut in two and in three at every pair of
//             lengths from a set: the blocks a chain would compress, put
//             together as the kernel does, are the message's, in order
//   wide      lengths up to 2^64 - 1 do not wrap
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../maxio_amd/csrc/sums_carry.hpp"

using namespace mxec;

static void fail(const char* what, uint64_t a, uint64_t b) {
    std::fprintf(stderr, "%s: pending/at %" PRIu64 " len %" PRIu64 "\n", what, a, b);
    std::exit(2);
}

// The kernel's steps over bytes instead of compressions: `blocks` receives
// every full block in order, `tail` / `bytes` are the record.
struct Chain {
    std::vector<uint8_t> blocks;
    uint8_t tail[64];
    uint64_t bytes = 0;
    void update(const uint8_t* p, uint64_t len) {
        const uint32_t pending = uint32_t(bytes) & 63u;
        const SumsCarry k = sums_carry(pending, len);
        for (uint32_t t = 0; t < k.take; ++t) tail[k.head - k.take + t] = p[t];
        if (k.head == 64) blocks.insert(blocks.end(), tail, tail + 64);
        const uint8_t* q = p + k.take;
        blocks.insert(blocks.end(), q, q + 64 * k.blocks);
        q += 64 * k.blocks;
        for (uint32_t t = 0; t < k.rest; ++t) tail[t] = q[t];
        bytes += len;
        if (k.tail != (bytes & 63u)) fail("tail is not the byte count's", pending, len);
    }
};

int main() {
    uint64_t n = 0;
    for (uint32_t pending = 0; pending < 64; ++pending)
        for (uint64_t len = 0; len <= 200; ++len, ++n) {
            const SumsCarry k = sums_carry(pending, len);
            if (k.head + 64 * k.blocks + k.rest != pending + len) fail("identity", pending, len);
            if (k.tail >= 64) fail("tail", pending, len);
            if (k.tail != (pending + len) % 64) fail("tail value", pending, len);
            if (k.take + 64 * k.blocks + k.rest != len) fail("piece bytes", pending, len);
            if (pending == 0 && (k.take || k.head)) fail("nothing pends", pending, len);
            if (pending && k.head != (pending + len < 64 ? pending + len : 64)) fail("head", pending, len);
            if (k.head != 0 && k.head != 64 && (k.blocks || k.rest)) fail("open block", pending, len);
            if ((k.head == 64) + k.blocks != (pending + len) / 64) fail("block count", pending, len);
        }
    std::printf("identity ok %" PRIu64 "\n", n);

    if (sums_pad_blocks(0) != 1 || sums_pad_blocks(55) != 1 || sums_pad_blocks(56) != 2 || sums_pad_blocks(63) != 2)
        fail("pad", 0, 0);
    for (uint32_t t = 0; t < 64; ++t)
        if (sums_pad_blocks(t) != (t <= 55 ? 1 : 2)) fail("pad", t, 0);
    std::printf("pad ok 64\n");

    std::vector<uint8_t> msg(700);
    for (size_t i = 0; i < msg.size(); ++i) msg[i] = uint8_t(i * 7 + 3);
    const uint64_t cuts[] = {0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 129, 200};
    n = 0;
    for (uint64_t a : cuts)
        for (uint64_t b : cuts)
            for (uint64_t c : cuts) {
                // heap copies of exactly the piece's size: a read past a piece is an error here
                std::vector<uint8_t> p0(msg.begin(), msg.begin() + a), p1(msg.begin() + a, msg.begin() + a + b),
                    p2(msg.begin() + a + b, msg.begin() + a + b + c);
                Chain ch;
                ch.update(p0.data(), a);
                ch.update(p1.data(), b);
                ch.update(p2.data(), c);
                const uint64_t total = a + b + c;
                if (ch.blocks.size() != total / 64 * 64) fail("replay block count", a, b);
                for (size_t i = 0; i < ch.blocks.size(); ++i)
                    if (ch.blocks[i] != msg[i]) fail("replay block bytes", a, b);
                for (uint64_t i = 0; i < total % 64; ++i)
                    if (ch.tail[i] != msg[total / 64 * 64 + i]) fail("replay tail bytes", a, b);
                ++n;
            }
    std::printf("replay ok %" PRIu64 "\n", n);

    n = 0;
    for (uint32_t pending : {0u, 1u, 63u})
        for (uint64_t len : {UINT64_MAX, UINT64_MAX - 1, UINT64_MAX - 63, uint64_t(1) << 63, (uint64_t(1) << 32) + 5}) {
            const SumsCarry k = sums_carry(pending, len);
            if (k.take + 64 * k.blocks + k.rest != len || k.tail >= 64) fail("wide", pending, len);
            if (k.blocks > len / 64) fail("wide blocks", pending, len);
            ++n;
        }
    std::printf("wide ok %" PRIu64 "\n", n);
    return 0;
}
