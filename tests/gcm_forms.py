"""The window and ring forms of the GCM frame kernel as a host-only model, and
the plan that sends the frames of gcm_cases.py through them.  Numpy only,
nothing from the library under test.

The model.  gcm_kernel.hip compiles three forms beside the contiguous ones:

  * window (encrypt and decrypt): byte x of a job's frame stream lies at
        base + ((x // chunk_size) % slots) * slot_stride + x % chunk_size;
  * ring (decrypt): plaintext byte o of a job lies at
        base + (ring_off + o) % ring_bytes.

window_positions() and ring_positions() are those two lines.  An Image is the
expected content of one buffer: GUARD bytes of 0xA5, a pre-filled body, GUARD
bytes again, with the bytes of one or more jobs placed into the body by a
mapping.  check() compares a buffer read back from the device with an Image
and names the first differing byte: a guard, a body byte outside every job,
or byte o of frame f of a job and the field (nonce, ciphertext, tag or
plaintext) it belongs to.

The plan.  lane_plan() gives every single-frame job of gcm_cases.lane_cases()
two window geometries and two ring geometries:

  * window: one single boundary of a named class (WINDOW_CLASSES; `none` is
    the uncut frame) and one `many`, a chunk size near 1000 that is no
    multiple of 16, so that about one block in sixty is cut and the frame
    wraps from the last slot to slot 0 somewhere;
  * ring: `none` (the ring cannot be cut more than once, so the uncut store
    path takes the place of `many`) and one wrap of a named class
    (RING_CLASSES).

The classes name where the kernel's lanes change what they do.  Lane l of a
frame's 256 folds blocks l, l + 256, ... of the GHASH sequence of na AAD
blocks, nb payload blocks and the length block; after a leading AAD block it
takes two whole payload blocks per step while `i + 256 < full_end`
(full_end = na + len // 16) and leaves the rest to a one-block tail loop.
lane_blocks() replays that loop structure.  `second-pass` cuts payload block
256 - na (sequence block 256, the first one lane 0 takes in its second pass),
`pair-to-tail` the lowest payload block that the tail loop takes.

Which class a case gets is chosen so that every class meets every AAD length
and every GHASH length m of the case table for which it exists;
tests/test_gcm_forms_plan.py asserts that, and that slot_stride - chunk_size
(0, 256, an odd value) and the whole periods in stream_off (0, 1, 2^33 + 5)
each meet every class."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import gcm_cases

GUARD = 64
GUARD_BYTE = 0xA5
OVERHEAD = 28  # nonce 12 + tag 16

PADS = (0, 256, 37)              # slot_stride - chunk_size
PERIODS = (0, 1, 2**33 + 5)      # whole periods of slots * chunk_size in stream_off
WINDOW_CLASSES = ("none", "nonce", "header-end", "second-pass", "pair-to-tail", "last-block", "tag", "slot-wrap")
RING_CLASSES = ("second-pass", "pair-to-tail", "last-block", "block-boundary", "end")


# ---- the two mappings ----

def window_positions(n: int, stream_off: int, chunk: int, stride: int, slots: int) -> np.ndarray:
    """Where stream bytes stream_off .. stream_off + n - 1 lie in a window."""
    x = np.uint64(stream_off) + np.arange(n, dtype=np.uint64)
    at = ((x // np.uint64(chunk)) % np.uint64(slots)) * np.uint64(stride) + x % np.uint64(chunk)
    return at.astype(np.int64)


def ring_positions(n: int, ring_off: int, ring_bytes: int) -> np.ndarray:
    """Where plaintext bytes 0 .. n - 1 of a job lie in a ring."""
    return (np.int64(ring_off) + np.arange(n, dtype=np.int64)) % np.int64(ring_bytes)


# ---- expected images ----

class Image:
    """GUARD | body | GUARD.  `initial` is what goes up to the device, `want`
    what must be there afterwards."""

    def __init__(self, body: np.ndarray, kind: str):
        assert kind in ("window", "ring", "plaintext") and body.dtype == np.uint8
        g = np.full(GUARD, GUARD_BYTE, np.uint8)
        self.kind = kind
        self.n = body.size
        self.initial = np.concatenate([g, body, g])
        self.want = self.initial.copy()
        self._part = np.full(self.n, -1, np.int64)
        self._byte = np.zeros(self.n, np.int64)
        self._parts = []

    @property
    def size(self) -> int:
        return self.n + 2 * GUARD

    def place(self, data: bytes, pos: np.ndarray, frame_size: int, plain_len: int, what, resident: bool = False):
        """data[k] is expected at body byte pos[k].  data is a frame stream
        (kind window) or a plaintext of plain_len bytes in frames of
        frame_size.  resident: the bytes are there before the launch (a
        decrypt's input) instead of written by it."""
        d = np.frombuffer(data, np.uint8)
        assert d.size == pos.size and (pos >= 0).all() and (pos < self.n).all(), "a mapped byte lies outside the body"
        assert (self._part[pos] == -1).all(), "two mapped bytes collide"
        self._part[pos] = len(self._parts)
        self._byte[pos] = np.arange(d.size)
        assert (self._byte[pos] == np.arange(d.size)).all(), "two mapped bytes collide"  # a later one overwrote it
        self._parts.append((what, frame_size, plain_len))
        self.want[GUARD + pos] = d
        if resident:
            self.initial[GUARD + pos] = d

    def where(self, i: int) -> str:
        """What byte i of the buffer (guards included) is."""
        if i < GUARD or i >= GUARD + self.n:
            return f"guard byte {i if i < GUARD else i - self.n - GUARD} {'before' if i < GUARD else 'after'} the {self.kind}"
        p = int(self._part[i - GUARD])
        if p < 0:
            return f"{self.kind} byte {i - GUARD} outside the job"
        what, fs, plain = self._parts[p]
        k = int(self._byte[i - GUARD])
        if self.kind != "window":
            return f"{what}: plaintext byte {k % fs} (block {k % fs // 16}) of frame {k // fs}"
        f, o = divmod(k, fs + OVERHEAD)
        ln = min(fs, plain - f * fs)
        field = "nonce" if o < 12 else "ciphertext" if o < 12 + ln else "tag"
        return f"{what}: {field}, byte {o} of frame {f}" + (f" (payload block {(o - 12) // 16})" if field == "ciphertext" else "")


def check(got: np.ndarray, image: Image, what="") -> None:
    """got: the buffer read back, guards included.  Raises AssertionError
    naming the first byte that differs from image.want."""
    assert got.shape == image.want.shape, (what, got.shape, image.want.shape)
    bad = np.flatnonzero(got != image.want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} bytes differ, the first at {i}: {image.where(i)}: "
                             f"got {got[i]:#04x}, want {image.want[i]:#04x}")


def _fill(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def window_image(stream: bytes, w: "Win", frame_size: int, plain_len: int, what, seed: int = 1,
                 resident: bool = False) -> Image:
    """A window of w.slots slots pre-filled from the RNG, the stream in it."""
    img = Image(_fill(w.slots * w.stride, seed), "window")
    img.place(stream, window_positions(len(stream), w.stream_off, w.chunk, w.stride, w.slots), frame_size, plain_len,
              what, resident)
    return img


def ring_image(jobs, r_bytes: int, seed: int = 1) -> Image:
    """jobs: (plaintext, ring_off, frame_size, what) each; a ring pre-filled from the RNG."""
    img = Image(_fill(r_bytes, seed), "ring")
    for pt, off, fs, what in jobs:
        img.place(pt, ring_positions(len(pt), off, r_bytes), fs, len(pt), what)
    return img


def plaintext_image(pt: bytes, frame_size: int, what) -> Image:
    """A contiguous plaintext buffer, 0x5A before the launch."""
    img = Image(np.full(len(pt), 0x5A, np.uint8), "plaintext")
    img.place(pt, np.arange(len(pt), dtype=np.int64), frame_size, len(pt), what)
    return img


# ---- geometries ----

class Win(NamedTuple):
    cls: str
    chunk: int
    stride: int
    slots: int
    stream_off: int
    cut: int  # frame offset of the class's boundary: bytes cut - 1 and cut lie in different chunks (0: none / many)

    @property
    def pad(self) -> int:
        return self.stride - self.chunk

    @property
    def periods(self) -> int:
        return self.stream_off // (self.slots * self.chunk)

    def args(self) -> tuple:
        return self.chunk, self.stride, self.slots


class Ring(NamedTuple):
    cls: str
    ring_bytes: int
    ring_off: int
    cut: int  # plaintext bytes in front of the wrap (0: none)


def window_valid(w: Win, plain_len: int, frame_size: int) -> bool:
    """gcm_window_check's conditions on a geometry."""
    span = plain_len + OVERHEAD * ((plain_len + frame_size - 1) // frame_size)
    return (w.chunk > 0 and w.stride >= w.chunk and w.slots >= 1 and w.slots <= 2**62 // w.chunk
            and span <= w.slots * w.chunk and w.stream_off + span < 2**64)


def ring_valid(r: Ring, plain_lens) -> bool:
    """gcm_ring_check's conditions (one offset given: the jobs lie end to end)."""
    return r.ring_bytes > 0 and r.ring_off < r.ring_bytes and sum(plain_lens) <= r.ring_bytes


def boundaries(w: Win, span: int) -> list:
    """The stream offsets b in 1 .. span - 1 whose bytes b - 1 and b lie in different chunks."""
    first = w.chunk - w.stream_off % w.chunk
    return list(range(first, span, w.chunk))


@functools.lru_cache(maxsize=None)
def lane_blocks(na: int, n: int) -> tuple:
    """The kernel's lane loops over a frame of n payload bytes behind na AAD
    blocks: (payload blocks taken first in a pair step, second in a pair
    step, by the tail loop), each sorted."""
    nb, full_end = (n + 15) // 16, na + n // 16
    m = na + nb + 1
    first, second, tail = [], [], []
    for lane in range(256):
        i = lane
        if i < na:
            i += 256
        while i + 256 < full_end and i >= na:
            first.append(i - na)
            second.append(i + 256 - na)
            i += 512
        while i < m:
            if na <= i < na + nb:
                tail.append(i - na)
            i += 256
    assert sorted(first + second + tail) == list(range(nb))
    return tuple(sorted(first)), tuple(sorted(second)), tuple(sorted(tail))


def inside_block(block: int, n: int, k: int):
    """An offset strictly inside payload block `block` of n payload bytes, or None (a one-byte block)."""
    t = min(16, n - 16 * block)
    return 16 * block + 1 + k % (t - 1) if t >= 2 else None


def payload_cuts(na: int, n: int, k: int) -> dict:
    """Payload offsets (bytes in front of the boundary) of the payload classes that exist for this frame."""
    nb = (n + 15) // 16
    out = {}
    if 0 <= 256 - na < nb and inside_block(256 - na, n, k) is not None:
        out["second-pass"] = inside_block(256 - na, n, k)
    tail = lane_blocks(na, n)[2]
    if tail and inside_block(tail[0], n, k) is not None:
        out["pair-to-tail"] = inside_block(tail[0], n, k)
    last = inside_block(nb - 1, n, k) if n % 16 else None  # inside a partial last block, else on the block's start
    out["last-block"] = last if last is not None else 16 * (nb - 1)
    return out


def window_cuts(na: int, n: int, k: int) -> dict:
    """Frame offsets of the window's single-boundary classes that exist for this frame."""
    out = {"nonce": 1 + k % 11, "header-end": 12, "tag": 12 + n + 1 + k % 15, "slot-wrap": 1 + (7919 * k + 13) % (n + 27)}
    out.update({c: 12 + o for c, o in payload_cuts(na, n, k).items()})
    return out


def ring_cuts(na: int, n: int, k: int) -> dict:
    """Plaintext offsets of the ring's wrap classes that exist for this frame (a wrap needs 1 <= cut <= n)."""
    nb = (n + 15) // 16
    out = {c: o for c, o in payload_cuts(na, n, k).items() if o >= 1}
    if nb >= 2:
        out["block-boundary"] = 16 * (1 + (7919 * k) % (nb - 1))
    out["end"] = n  # the job's last byte is the ring's last: room == len, no wrap
    return out


def one_boundary(cls: str, span: int, cut: int, k: int, i: int) -> Win:
    """A window with exactly one boundary inside a stream of span bytes, at
    offset cut; k counts the class's uses and rotates pad, periods and slots."""
    pad, periods = PADS[k % 3], PERIODS[k // 3 % 3]
    if cls == "none":
        chunk = span + 5 + i % 9
        slots = 1 + k % 2
        start = (slots - 1) * chunk + (chunk - span if k % 4 == 0 else i % 5)  # k % 4 == 0: the frame ends its chunk
        cut = 0
    else:
        chunk = max(cut, span - cut) + 3 + i % 5
        slots = 2 if cls == "slot-wrap" else 2 + k % 2
        first = slots - 1 if cls == "slot-wrap" else (k // 2) % (slots - 1)
        start = first * chunk + chunk - cut
    return Win(cls, chunk, chunk + pad, slots, periods * slots * chunk + start, cut)


def many(frame_len: int, k: int, i: int) -> Win:
    chunk = 1001 + 2 * (i % 8)  # odd: no multiple of 16
    slots = (frame_len + chunk - 1) // chunk + 1
    first = slots - 1 - k % min(slots, 3)  # the frame wraps to slot 0 when it is longer than what is left
    start = first * chunk + chunk - (1 + (31 * i) % min(frame_len - 1, chunk - 1))  # a boundary even in a tiny frame
    return Win("many", chunk, chunk + PADS[k % 3], slots, PERIODS[k // 3 % 3] * slots * chunk + start, 0)


def one_wrap(cls: str, n: int, cut: int, i: int, total: int = 0) -> Ring:
    """A ring in which a job's plaintext wraps after cut bytes (cut == 0:
    class none, it does not); total: the bytes of all jobs laid end to end."""
    r_bytes = max(n, total) + 1 + (7 * i) % 97
    if cls == "none":
        return Ring(cls, r_bytes, (13 * i) % (r_bytes - max(n, total) + 1), 0)
    return Ring(cls, r_bytes, r_bytes - cut, cut)


class Planned(NamedTuple):
    i: int        # index into gcm_cases.lane_cases()
    job: gcm_cases.Job
    na: int
    m: int
    windows: tuple  # (single boundary, many or None when thinned out)
    rings: tuple    # (single wrap, none)


def _pick(classes, seen: dict, aad_len: int, m: int) -> str:
    """The class least met so far by this AAD length and this m."""
    return min(classes, key=lambda c: (seen.get((c, "aad", aad_len), 0) + seen.get((c, "m", m), 0),
                                       seen.get((c, "all"), 0)))


@functools.lru_cache(maxsize=None)
def lane_plan(many_every: int = 1) -> tuple:
    """many_every = k: only every k-th case gets its `many` window."""
    out, seen_w, seen_r = [], {}, {}
    for i, job in enumerate(gcm_cases.lane_cases()):
        n, na = len(job.pt), (job.aad_len + 15) // 16
        m = na + (n + 15) // 16 + 1

        def use(cls, seen):  # -> how often the class was used before
            for key in ((cls, "aad", job.aad_len), (cls, "m", m), (cls, "all")):
                seen[key] = seen.get(key, 0) + 1
            return seen[(cls, "all")] - 1

        cuts = window_cuts(na, n, i)
        cls = _pick(["none"] + sorted(cuts), seen_w, job.aad_len, m)
        w1 = one_boundary(cls, n + OVERHEAD, cuts.get(cls, 0), use(cls, seen_w), i)
        w2 = many(n + OVERHEAD, use("many", seen_w), i) if i % many_every == 0 else None
        cuts = ring_cuts(na, n, i)
        cls = _pick(sorted(cuts), seen_r, job.aad_len, m)
        use(cls, seen_r)
        out.append(Planned(i, job, na, m, (w1, w2), (one_wrap(cls, n, cuts[cls], i), one_wrap("none", n, 0, i))))
    return tuple(out)


def second_of_a_pair(na: int, n: int, below: int) -> int:
    """The highest payload block under `below` that a lane takes second in a pair step."""
    return max(j for j in lane_blocks(na, n)[1] if j < below)


# ---- multi-frame jobs ----

def late_window(job, i: int) -> Win:
    """A window barely larger than a multi-frame job's stream, the stream
    starting half a frame before a period's end, 2^33 + 5 periods in: every
    frame but the first has its rebased pos in the second period."""
    chunk = 1001 + 2 * (i % 8)
    slots = (job.frames_len + chunk - 1) // chunk
    start = slots * chunk - (job.frame_size + OVERHEAD) // 2
    return Win("late", chunk, chunk + PADS[(i + 2) % 3], slots, PERIODS[2] * slots * chunk + start, 0)


def second_period_frames(w: Win, job) -> int:
    """How many frames of job have pos >= slots * chunk_size once the launch is
    rebased into the first period (pos = stream_off mod period + f * frame length)."""
    period = w.slots * w.chunk
    return sum(w.stream_off % period + f * (job.frame_size + OVERHEAD) >= period for f in range(job.n_frames))


def middle_wrap(job, i: int) -> Ring:
    """The ring's wrap inside a middle frame of a multi-frame job, off any block boundary."""
    cut = job.frame_size * (job.n_frames // 2) + min(job.frame_size, 16) // 2 + 3
    assert 0 < cut < len(job.pt)
    return one_wrap("middle-frame", len(job.pt), cut, i)


def counter_cut_block(job) -> int:
    """A payload block deep in the first (large) frame of a counter edge job
    that a lane takes second in a pair step."""
    na = (job.aad_len + 15) // 16
    return second_of_a_pair(na, job.frame_size, 40000)


def counter_window(job, uncut: bool = False) -> Win:
    """One boundary inside counter_cut_block(job), an odd stride pad, 2^33 + 5
    periods; uncut: one chunk holds both frames."""
    if uncut:
        return one_boundary("none", job.frames_len, 0, 1, 3)
    return one_boundary("pair-second", job.frames_len, 12 + 16 * counter_cut_block(job) + 5, 8, 3)


def counter_ring(job) -> Ring:
    return one_wrap("pair-second", len(job.pt), 16 * counter_cut_block(job) + 5, 3)
