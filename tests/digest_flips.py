"""The flip plan: batches of k = 2, m = 1 objects whose EXPECTED SHA-256
digests are wrong by single bits, shared by tests/test_digest_flip_plan.py
(CPU) and tests/test_digest_compare_gpu.py.

The bitrot guard of a verified GET is "SHA-256 of the shard as read equals
the digest the manifest recorded" (chunk_reader.rs:176-196: a mismatch is an
erasure; :199-208: fewer than k shards left is an error).  With three shards,
an object whose expected digests are wrong in m + 1 = 2 of them must fail; a
compare that overlooks either flipped bit leaves k verified shards and serves
the object.  Plain Python and numpy: parity from the oracle, digests from
hashlib, every expectation stated by the class rules below and re-derived
from hashlib alone by test_digest_flip_plan.py.

Bit b (0..255) of a digest is bit b % 8 (LSB = 0) of byte b // 8.

Classes (shuffled with a fixed seed so failing objects are not adjacent):

FAIL     all present; bit b flipped in shard b % 3's digest and its partner
         bit in shard (b + 1) % 3's: status -10, mask only shard (b + 2) % 3.
         Bit set ALL: one object per bit b, partner 255 - b (every bit is
         flipped in two objects, and but for b = 2 mod 3 in two shard
         positions).  Bit set BYTES: 32
         flips, byte j at bit j % 8, two to an object (bytes j and 31 - j).
MISSING  shard s0 absent (buffer 0xEE, expected entry 0xFF bytes: never to be
         consulted); one bit flipped in one of the two present shards: -10,
         mask only the other present shard.  3 x 2 x 4 bit positions (one per
         quarter of the digest); per s0 a twin without a flip: status 0,
         s0 rebuilt.
SWAP     all present, the correct digests of two shards exchanged: -10, mask
         only the third shard.
ONE      all present, a single flipped bit: status 0 (the threshold is m + 1
         mismatches, not fewer), the shard is rebuilt to the same bytes.
CLEAN    nothing flipped: status 0.
EMPTY    (on request) the last data chunk has length 0, digest of b""; one
         bit flipped there and one in the parity's digest: -10.
"""
from __future__ import annotations

import hashlib
import random
from dataclasses import dataclass

import numpy as np

K, M, TOTAL = 2, 1, 3
OK, TOO_FEW = 0, -10  # include/maxio_ec.h MXEC_E_TOO_FEW_SHARDS_PRESENT
ALL = tuple(range(256))
BYTES = tuple(8 * j + j % 8 for j in range(32))
MISSING_FILL, PAD_FILL = 0xEE, 0xA5
SHUFFLE_SEED = 0xD16E57


@dataclass(frozen=True)
class Obj:
    cls: str
    present: tuple        # input mask, one flag per shard
    lens: tuple           # byte length of every shard
    flips: tuple = ()     # (shard, bit) flips in the expected digests
    swap: tuple = ()      # two shards whose correct digests are exchanged
    status: int = OK      # expected status
    mask: tuple = (1, 1, 1)  # expected mask on return (device calls)


def _only(*keep):
    return tuple(1 if i in keep else 0 for i in range(TOTAL))


def layout(bits, S, last, empty=False, controls=16):
    """The objects of one batch (no data yet).  bits: ALL or BYTES."""
    full, lens = (1, 1, 1), (S, last, S)
    objs = []
    if bits is ALL:
        pairs = [(b, 255 - b) for b in ALL]
    else:
        assert bits is BYTES
        pairs = [(BYTES[j], BYTES[31 - j]) for j in range(16)]
    for n, (b0, b1) in enumerate(pairs):
        objs.append(Obj("FAIL", full, lens, ((n % 3, b0), ((n + 1) % 3, b1)), (), TOO_FEW, _only((n + 2) % 3)))
    c = 0
    for s0 in range(TOTAL):
        there = [i for i in range(TOTAL) if i != s0]
        pres = _only(*there)
        for f in there:
            other = [i for i in there if i != f][0]
            for q in range(4):
                bit = 64 * q + (13 * c + 7 * q) % 64
                objs.append(Obj("MISSING", pres, lens, ((f, bit),), (), TOO_FEW, _only(other)))
            c += 1
        objs.append(Obj("MISSING", pres, lens))  # the twin: s0 rebuilt
    for a, b in [(0, 1), (0, 2), (1, 2)] * 2:
        objs.append(Obj("SWAP", full, lens, (), (a, b), TOO_FEW, _only(3 - a - b)))
    for n in range(controls):
        objs.append(Obj("ONE", full, lens, ((n % 3, (16 * n + 5 * n % 16) % 256),)))
    for _ in range(controls):
        objs.append(Obj("CLEAN", full, lens))
    if empty:
        for b1, b2 in ((3, 250), (200, 40)):
            objs.append(Obj("EMPTY", full, (S, 0, S), ((1, b1), (2, b2)), (), TOO_FEW, _only(0)))
    random.Random(SHUFFLE_SEED).shuffle(objs)
    return objs


def flip(digest: bytes, bit: int) -> bytes:
    d = bytearray(digest)
    d[bit // 8] ^= 1 << (bit % 8)
    return bytes(d)


class Plan:
    """A batch with its data.  Arrays, n objects:
    orig      (n, 3, stride) the healthy shards; past a shard's length PAD_FILL
    given     (n, 3, stride) what a call receives: orig, absent shards MISSING_FILL
    digests   (n, 3, 32) hashlib over each shard's own length
    expected  (n, 3, 32) what the call is told: digests with the flips / swaps,
              absent shards' entries 0xFF
    present   (n, 3) input mask; status (n,); mask (n, 3) expected on return
    lens      (n, 3)"""

    def __init__(self, bits, S, last, stride, empty=False, controls=16, seed=1, given_out=None):
        import oracle

        assert stride >= S >= last
        self.objs = layout(bits, S, last, empty, controls)
        self.S, self.stride = S, stride
        n = self.n = len(self.objs)
        rng = np.random.default_rng(seed)
        self.lens = np.array([o.lens for o in self.objs], np.uint64)
        self.present = np.array([o.present for o in self.objs], np.uint8)
        self.status = np.array([o.status for o in self.objs], np.int32)
        self.mask = np.array([o.mask for o in self.objs], np.uint8)
        self.orig = np.full((n, TOTAL, stride), PAD_FILL, np.uint8)
        self.digests = np.zeros((n, TOTAL, 32), np.uint8)
        self.expected = np.zeros((n, TOTAL, 32), np.uint8)
        for o, ob in enumerate(self.objs):
            for j in range(K):
                self.orig[o, j, :ob.lens[j]] = np.frombuffer(rng.bytes(ob.lens[j]), np.uint8)
            data = [self.orig[o, j, :ob.lens[j]] for j in range(K)]
            self.orig[o, K, :S] = oracle.encode(data, M, S)[0]
            dig = [hashlib.sha256(self.orig[o, i, :ob.lens[i]].tobytes()).digest() for i in range(TOTAL)]
            exp = list(dig)
            for shard, bit in ob.flips:
                exp[shard] = flip(exp[shard], bit)
            if ob.swap:
                a, b = ob.swap
                exp[a], exp[b] = dig[b], dig[a]
            for i in range(TOTAL):
                if not ob.present[i]:
                    exp[i] = b"\xff" * 32
                self.digests[o, i] = np.frombuffer(dig[i], np.uint8)
                self.expected[o, i] = np.frombuffer(exp[i], np.uint8)
        self.given = given_out if given_out is not None else np.empty_like(self.orig)
        assert self.given.shape == self.orig.shape
        self.fill_given(self.given)

    def fill_given(self, out):
        out[...] = self.orig
        out[self.present == 0] = MISSING_FILL

    def failing(self):
        return np.flatnonzero(self.status != OK)
