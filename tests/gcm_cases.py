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


def frame_slices(job: Job):
    """(frame offset in the stream, payload offset, payload bytes, index) per frame."""
    fl = job.frame_size + 28
    for f in range(job.n_frames):
        off = f * job.frame_size
        yield f * fl, off, min(job.frame_size, len(job.pt) - off), (job.first_index + f) % 2**64
