"""The frame jobs that pin AES-256-GCM at the edges gcm_kernel.hip has, shared
by the oracle's CPU pin (test_oracle_gcm.py) and the GPU sweep
(test_gcm_edges_gpu.py) so that both see the same frames.  Host only: seeded
numpy data, nothing from the library under test.

The kernel's lane l folds blocks l, l + 256, ... of a frame's GHASH sequence
of m = na + nb + 1 blocks (na AAD blocks, nb payload blocks, the length
block), two payload blocks per step while a whole pair is left.  lane_cases()
puts m on both sides of every multiple of 256 up to 769 for every na that
moves the AAD / payload boundary inside or across a lane pass, with a whole
and a partial last block, under frame indices whose high word is not zero."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

LANE_FRAME_SIZE = 16384
AAD_LENS = (0, 1, 15, 16, 17, 32, 33, 4080, 4096, 4101)  # na = 0 1 1 1 2 2 3 255 256 257
SEQ_LENS = (255, 256, 257, 258, 511, 512, 513, 514, 769)  # m
LAST_BLOCK = (16, 1, 15)
SMALL_LENS = (1, 15, 16, 17)
INDICES = (0, 2**32 - 1, 2**32, 2**40 + 3, 0x0102030405060708, 2**64 - 1)
COUNTER_EDGE_BLOCKS = 65534  # the longest frame whose counters 2 + j stay below 2^16
LONG_COUNTER_BLOCKS = 65535  # the shortest frame with a counter of 2^16: the long-counter AES path


class Job(NamedTuple):
    key: bytes
    prefix: bytes
    frame_size: int
    first_index: int
    aad_len: int
    aads: tuple      # one AAD of aad_len bytes per frame; () when aad_len == 0
    pt: bytes

    @property
    def n_frames(self) -> int:
        return (len(self.pt) + self.frame_size - 1) // self.frame_size

    @property
    def frames_len(self) -> int:
        return len(self.pt) + 28 * self.n_frames

    @property
    def label(self) -> tuple:
        return self.aad_len, len(self.pt), self.first_index

    def oracle_args(self) -> dict:
        return {"aads": list(self.aads) or None, "first_index": self.first_index, "frame_size": self.frame_size}


def _bytes(rng, n: int) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _keys(rng, n: int, twin: tuple | None = None) -> list:
    keys = [_bytes(rng, 32) for _ in range(n)]
    if twin:  # byte-equal, yet another buffer
        keys[twin[1]] = bytes(bytearray(keys[twin[0]]))
        assert keys[twin[1]] == keys[twin[0]] and keys[twin[1]] is not keys[twin[0]]
    return keys


def _prefix(rng, i: int) -> bytes:
    p = bytearray(_bytes(rng, 4))
    p[i % 4] |= 0x80
    return bytes(p)


def _job(rng, key, i, frame_size, first_index, aad_len, n) -> Job:
    nf = (n + frame_size - 1) // frame_size
    aads = tuple(_bytes(rng, aad_len) for _ in range(nf)) if aad_len else ()
    return Job(key, _prefix(rng, i), frame_size, first_index, aad_len, aads, _bytes(rng, n))


@functools.lru_cache(maxsize=None)
def lane_cases() -> tuple:
    rng = np.random.default_rng(0x6C616E65)
    keys = _keys(rng, 8, twin=(2, 5))
    lens = []
    for aad_len in AAD_LENS:
        na = (aad_len + 15) // 16
        for m in SEQ_LENS:
            nb = m - na - 1
            if nb >= 1:
                lens += [(aad_len, 16 * (nb - 1) + t) for t in LAST_BLOCK]
        lens += [(aad_len, n) for n in SMALL_LENS]
    assert all(n <= LANE_FRAME_SIZE for _, n in lens)
    return tuple(_job(rng, keys[i % 8], i, LANE_FRAME_SIZE, INDICES[i % len(INDICES)], aad_len, n)
                 for i, (aad_len, n) in enumerate(lens))


@functools.lru_cache(maxsize=None)
def stream_cases() -> tuple:
    rng = np.random.default_rng(0x7374726D)
    keys = _keys(rng, 3)
    return (
        # the index carries into its high word between frames 1 and 2
        _job(rng, keys[0], 0, 4096, 2**32 - 2, 32, 2 * 4096 + 55),
        _job(rng, keys[1], 1, 1024, 7, 17, 10 * 1024 + 77),
        # more frames of one key than a full chip's first pass takes (4 frames
        # per workgroup): a workgroup meets this key again and keeps its table
        _job(rng, keys[2], 2, 16, 2**32 - 1200, 1, 16 * 2299 + 3),
    )


@functools.lru_cache(maxsize=None)
def tiny_cases(n: int) -> tuple:
    rng = np.random.default_rng(0x74696E79)
    keys = _keys(rng, 23)
    out, k, left = [], 0, 0
    for i in range(n):
        if left == 0:
            k, left = (k + 1) % 23, int(rng.integers(1, 6))
        left -= 1
        ln = int(rng.integers(1, 601))
        aad_len = (0, 1, 17, 32)[int(rng.integers(0, 4))]
        first = int(rng.integers(0, 2**64, dtype=np.uint64))
        out.append(_job(rng, keys[k], i, 608, first, aad_len, ln))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def counter_edge_case() -> Job:
    """A first frame of exactly 65534 blocks (counters 2 .. 0xFFFF: every
    value of counter bytes 0 and 1) and a short second one, the index
    carrying into its high word between them."""
    rng = np.random.default_rng(0x63747265)
    fs = COUNTER_EDGE_BLOCKS * 16
    return _job(rng, _bytes(rng, 32), 3, fs, 2**32 - 1, 17, fs + 16 * 300 + 5)


@functools.lru_cache(maxsize=None)
def long_counter_case() -> Job:
    """A first frame of exactly 65535 blocks, the first whose last counter
    (0x10000) leaves the two low counter bytes, and a short second one; a
    17-byte AAD, the index carrying into its high word between them."""
    rng = np.random.default_rng(0x6C6F6E67)
    fs = LONG_COUNTER_BLOCKS * 16
    return _job(rng, _bytes(rng, 32), 1, fs, 2**32 - 1, 17, fs + 16 * 41 + 9)


def key_pass_cases(cus: int) -> tuple:
    """tiny_cases(2 * 4 * cus + 37) with eight long frames at the start of each
    of the three grid-stride passes of a full chip (jobs 0 .. 7, 4 cus .. 4 cus
    + 7, 8 cus .. 8 cus + 7: workgroups 0 and 1, four frames each), so that a
    frame group meets a long frame under another key in every pass.  A frame
    of m <= 256 GHASH blocks never multiplies by H^256 (each lane folds one
    block into a zero accumulator), so the tiny frames alone cannot tell a
    stale H^256 table from a fresh one; these have m >= 258."""
    lane = lane_cases()
    long_ones = [j for j in lane if (j.aad_len + 15) // 16 + (len(j.pt) + 15) // 16 + 1 >= 258]
    jobs = list(tiny_cases(2 * 4 * cus + 37))
    for p in range(3):
        for t in range(8):
            k = 37 * p + 5 * t
            while p and long_ones[k % len(long_ones)].key == jobs[4 * cus * (p - 1) + t].key:
                k += 1
            jobs[4 * cus * p + t] = long_ones[k % len(long_ones)]
    return tuple(jobs)


def flips(job: Job) -> list:
    """(what, byte offset in the frame or the AAD, bit) of a single frame job:
    the tamper positions of test_gcm_edges_gpu.py and test_gcm_form_edges_gpu.py."""
    ln = len(job.pt)
    at = [("prefix", 0), ("prefix", 3)] + [("index", b) for b in range(4, 12)]
    at += [("ciphertext", 12), ("ciphertext", 12 + ln - 1), ("tag", 12 + ln), ("tag", 12 + ln + 15)]
    at += [("aad", 0), ("aad", job.aad_len - 1)]
    return [(what, off, 1 << (k % 8)) for k, (what, off) in enumerate(at)]


def tamper_picks() -> list:
    """The lane cases that get tampered with: AADs of 1, 2 and 257 blocks, a
    partial last block, an index with a non-zero high word."""
    lane = lane_cases()
    return [next(i for i, j in enumerate(lane) if j.aad_len == aad_len and len(j.pt) > 16
                 and len(j.pt) % 16 and j.first_index >= 2**32) for aad_len in (1, 17, 4101)]


def frame_slices(job: Job):
    """(frame offset in the stream, payload offset, payload bytes, index) per frame."""
    fl = job.frame_size + 28
    for f in range(job.n_frames):
        off = f * job.frame_size
        yield f * fl, off, min(job.frame_size, len(job.pt) - off), (job.first_index + f) % 2**64
