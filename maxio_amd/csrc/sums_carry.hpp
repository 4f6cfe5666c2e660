// sums_carry.hpp — the carry arithmetic of the resumable body digests
// (digest_kernel.hip body_hash_update_kernel): how a piece of any length joins
// a Merkle–Damgård chain that holds up to 63 pending bytes of an unfinished
// 64-byte block, and how many blocks the padding takes at the end.  Only
// integers; nothing is read or written.
//
// Free of HIP: constexpr functions, which the kernel may call as they are, and
// tests/c_manifest/sums_carry_check.cpp runs the same lines on its own under
// -fsanitize=address,undefined.
#pragma once

#include <cstdint>

namespace mxec {

struct SumsCarry {
    uint32_t take;    // bytes from the head of the piece that go behind the pending ones (0 when none pend)
    uint32_t head;    // bytes in the pending block once they have: 64 = it is complete and compressed
    uint64_t blocks;  // full 64-byte blocks that follow, straight from the piece at piece + take
    uint32_t rest;    // bytes of the piece after those blocks, kept at the front of the tail
    uint32_t tail;    // pending bytes afterwards, < 64
};

// pending < 64.  head + 64 * blocks + rest == pending + len.
constexpr SumsCarry sums_carry(uint32_t pending, uint64_t len) {
    SumsCarry c{};
    const uint32_t room = 64 - pending;
    c.take = pending == 0 ? 0 : (len < room ? uint32_t(len) : room);
    c.head = pending == 0 ? 0 : pending + c.take;
    const uint64_t left = len - c.take;  // 0 unless head is 0 or 64
    c.blocks = left / 64;
    c.rest = uint32_t(left % 64);
    c.tail = (c.head == 64 ? 0 : c.head) + c.rest;
    return c;
}

// Blocks of the final padding behind `tail` pending bytes: 0x80, zeros and the
// 64-bit length need 9 bytes more.
constexpr int sums_pad_blocks(uint32_t tail) { return tail + 9 <= 64 ? 1 : 2; }

}  // namespace mxec
