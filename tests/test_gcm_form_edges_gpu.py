"""GPU: the window and ring forms of the GCM frame kernel (gcm_kernel.hip
gcm_frames_kernel<false, true>, <true, true> and <true, false, true>) at the
lane, counter, AAD and index edges of tests/gcm_cases.py, which
test_gcm_edges_gpu.py sends through the contiguous forms only.

Every expected byte is oracle.frames_encrypt's (pinned to OpenSSL on these
very frames by tests/test_oracle_gcm.py) or the job's own plaintext, laid out
by the numpy model of tests/gcm_forms.py; where each frame is cut comes from
that module's plan, whose promises tests/test_gcm_forms_plan.py asserts on the
CPU.  Nothing is compared with another GPU form.

  * encrypt window: the whole window image, every byte outside the mapped
    range and between slots included, inside guards;
  * decrypt window: the oracle's stream scattered by numpy; the plaintext
    inside guards, a status per frame inside sentinels, the window unchanged;
  * ring: the oracle's contiguous stream; the whole ring image inside guards,
    the statuses inside sentinels.

All buffers of a test lie in one device allocation with GUARD bytes of 0xA5
around each, so a stray access lands in memory the test owns; every geometry
passes the library's own argument checks."""
from __future__ import annotations

import collections
import functools
import json
from typing import NamedTuple

import numpy as np
import pytest

import gcm_cases
import gcm_forms as F
import oracle

pytestmark = pytest.mark.gpu

FORMS = ("encrypt-window", "decrypt-window", "ring")
MANY_EVERY = 1  # every k-th lane case gets its `many` window (gcm_forms.lane_plan)
SENTINEL = -7
LAUNCHES = collections.Counter()  # (form, class) -> launches


@pytest.fixture(scope="module", autouse=True)
def launch_counts():
    yield
    by_form = {f: {c: n for (g, c), n in sorted(LAUNCHES.items()) if g == f} for f in FORMS}
    print("\nlaunches per form and class: " + json.dumps(by_form))


@functools.lru_cache(maxsize=None)
def _stream(job) -> bytes:
    return oracle.frames_encrypt(job.key, job.prefix, job.pt, **job.oracle_args())


def _up(n: int) -> int:
    return (n + 15) // 16 * 16


class Pool:
    """The plaintexts, AADs and frame streams of jobs, uploaded once: three
    device tensors, job i's three pieces at the residues skew(i) of 16."""

    def __init__(self, jobs, streams=None, skew=lambda i: (i % 16, (5 * i + 1) % 16, (3 * i + 2) % 16)):
        import torch

        self.jobs = jobs
        self.streams = streams or [_stream(j) for j in jobs]
        parts = ([j.pt for j in jobs], self.streams, [b"".join(j.aads) for j in jobs])
        self.offs, self.dev = [], []
        for which, datas in enumerate(parts):
            offs, n = [], F.GUARD
            for i, d in enumerate(datas):
                offs.append(_up(n) + skew(i)[which])
                n = offs[-1] + len(d) + F.GUARD
            host = np.full(n, F.GUARD_BYTE, np.uint8)
            for o, d in zip(offs, datas):
                host[o:o + len(d)] = np.frombuffer(d, np.uint8)
            self.offs.append(offs)
            self.dev.append(torch.from_numpy(host).cuda())
            assert self.dev[-1].data_ptr() % 16 == 0

    def ptr(self, which: int, i: int) -> int:
        return self.dev[which].data_ptr() + self.offs[which][i]

    def job(self, i: int, **side) -> dict:
        """The native job of jobs[i]; side: in_dev / out_dev."""
        j = self.jobs[i]
        return dict({"key": j.key, "nonce_prefix": j.prefix, "frame_size": j.frame_size, "first_index": j.first_index,
                     "aad_dev": self.ptr(2, i) if j.aad_len else 0, "aad_len": j.aad_len, "len": len(j.pt)}, **side)


class Arena:
    """Images one after another in one device buffer: one upload, the
    launches, one download."""

    def __init__(self):
        self.images, self.offs, self.whats, self.n = [], [], [], 0

    def add(self, img: F.Image, what, residue=None) -> int:
        """-> the image's number; residue: of its body's address modulo 16."""
        off = self.n if residue is None else _up(self.n + F.GUARD) + residue - F.GUARD
        self.images.append(img)
        self.offs.append(off)
        self.whats.append(what)
        self.n = off + img.size
        return len(self.images) - 1

    def upload(self):
        import torch

        self.initial = np.full(self.n, F.GUARD_BYTE, np.uint8)
        for o, img in zip(self.offs, self.images):
            self.initial[o:o + img.size] = img.initial
        self.dev = torch.from_numpy(self.initial).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def reset(self):
        import torch

        self.dev.copy_(torch.from_numpy(self.initial))

    def ptr(self, k: int) -> int:
        return self.dev.data_ptr() + self.offs[k] + F.GUARD

    def check(self):
        import torch

        torch.cuda.synchronize()
        got = self.dev.cpu().numpy()
        between = np.ones(self.n, bool)
        for o, img, what in zip(self.offs, self.images, self.whats):
            F.check(got[o:o + img.size], img, what)
            between[o:o + img.size] = False
        assert (got[between] == F.GUARD_BYTE).all(), "a byte between two buffers was written"


class Statuses:
    """One int32 per frame of every launch, a sentinel in front of each launch's and one behind the last."""

    def __init__(self, counts):
        import torch

        self.at = np.cumsum([1] + [n + 1 for n in counts])[:-1]
        self.counts = counts
        self.dev = torch.full((int(sum(counts)) + len(counts) + 1,), SENTINEL, dtype=torch.int32, device="cuda")

    def ptr(self, k: int) -> int:
        return self.dev.data_ptr() + 4 * int(self.at[k])

    def check(self, wants, whats):
        got = self.dev.cpu().numpy()
        want = np.full(got.size, SENTINEL, np.int32)
        for a, w in zip(self.at, wants):
            want[a:a + len(w)] = w
        for a, n, w, what in zip(self.at, self.counts, wants, whats):
            bad = np.flatnonzero(got[a:a + n] != np.asarray(w, np.int32))
            assert bad.size == 0, (what, f"{bad.size} frame statuses differ, the first of frame {bad[0]}: "
                                         f"got {got[a + bad[0]]}, want {w[bad[0]]}")
        assert (got == want).all(), "a status outside the launches' frames was written"


class Run(NamedTuple):
    """One launch: pool jobs `i` (one; the ring form takes several, laid end
    to end from the geometry's ring_off on) under geometry g.  pts / statuses:
    what a decrypt gives when not the jobs' plaintexts and zeros."""
    i: tuple
    g: tuple
    pts: tuple = None
    statuses: tuple = None
    residue: int = None      # of the window's or ring's base modulo 16
    residue_out: int = None  # of a decrypt window's plaintext buffer


def launch_all(ctx, form: str, pool: Pool, runs, times: int = 1):
    """Builds every run's expected images, uploads them in one buffer,
    launches, downloads once and compares."""
    arena = Arena()
    win, out, whats, wants, native = [], [], [], [], []
    for r in runs:
        jobs = [pool.jobs[i] for i in r.i]
        what = (form, r.g, [j.label for j in jobs][:3])
        pts = r.pts or [j.pt for j in jobs]
        whats.append(what)
        wants.append(r.statuses or [0] * sum(j.n_frames for j in jobs))
        LAUNCHES[form, r.g.cls] += times
        if form == "ring":
            assert F.ring_valid(r.g, [len(p) for p in pts]), what
            starts = np.cumsum([0] + [len(p) for p in pts[:-1]])
            offs = [int((r.g.ring_off + a) % r.g.ring_bytes) for a in starts]
            img = F.ring_image([(p, o, j.frame_size, j.label) for p, o, j in zip(pts, offs, jobs)], r.g.ring_bytes,
                               seed=r.i[0])
            win.append(arena.add(img, what, r.residue))
            native.append(([pool.job(i, in_dev=pool.ptr(1, i)) for i in r.i], offs))
            continue
        (i,), (job,) = r.i, jobs
        assert F.window_valid(r.g, len(job.pt), job.frame_size), what
        img = F.window_image(pool.streams[i], r.g, job.frame_size, len(job.pt), what, seed=i,
                             resident=form == "decrypt-window")
        win.append(arena.add(img, what, r.residue))
        if form == "decrypt-window":
            out.append(arena.add(F.plaintext_image(pts[0], job.frame_size, what), what, r.residue_out))
    arena.upload()
    st = Statuses([len(w) for w in wants]) if form != "encrypt-window" else None
    for t in range(times):
        for k, r in enumerate(runs):
            if form == "ring":
                jobs, offs = native[k]
                ctx.frames_decrypt_ring_device(jobs, offs, arena.ptr(win[k]), r.g.ring_bytes, st.ptr(k))
            elif form == "encrypt-window":
                ctx.frames_encrypt_window_device(pool.job(r.i[0], in_dev=pool.ptr(0, r.i[0])), r.g.stream_off,
                                                 arena.ptr(win[k]), *r.g.args())
            else:
                ctx.frames_decrypt_window_device(pool.job(r.i[0], out_dev=arena.ptr(out[k])), r.g.stream_off,
                                                 arena.ptr(win[k]), *r.g.args(), st.ptr(k))
        arena.check()
        if st:
            st.check(wants, whats)
        if t + 1 < times:
            arena.reset()
            st.dev.fill_(SENTINEL)
    return arena


@pytest.fixture(scope="module")
def lane_pool():
    return Pool(gcm_cases.lane_cases())


@pytest.fixture(scope="module")
def stream_pool():
    return Pool(gcm_cases.stream_cases())


@pytest.fixture(scope="module")
def counter_pool():
    return Pool((gcm_cases.counter_edge_case(), gcm_cases.long_counter_case()))


@pytest.mark.parametrize("aad_len", gcm_cases.AAD_LENS)
@pytest.mark.parametrize("form", FORMS)
def test_lane_sweep(ctx, lane_pool, form, aad_len):
    """Every lane case of this AAD length at its two planned geometries: a
    single boundary of a named class and `many` (window), a single wrap of a
    named class and none (ring)."""
    plan = [p for p in F.lane_plan(MANY_EVERY) if p.job.aad_len == aad_len]
    assert len(plan) >= 4
    runs = [Run((p.i,), g) for p in plan for g in (p.rings if form == "ring" else p.windows) if g is not None]
    launch_all(ctx, form, lane_pool, runs)


@pytest.mark.parametrize("form", FORMS)
def test_stream_cases(ctx, stream_pool, form):
    """Several frames, the index carry between frames, 2300 frames of 16
    bytes.  Window: barely larger than the stream, 2^33 + 5 periods into it,
    every frame but the first in the second period of the rebased launch.
    Ring: the wrap inside a middle frame."""
    jobs = gcm_cases.stream_cases()
    runs = [Run((i,), F.middle_wrap(j, i) if form == "ring" else F.late_window(j, i)) for i, j in enumerate(jobs)]
    if form != "ring":
        assert all(F.second_period_frames(r.g, j) == j.n_frames - 1 for r, j in zip(runs, jobs))
    launch_all(ctx, form, stream_pool, runs)


TINY_BAD = 97  # one tiny job in 97 has a flipped tag bit


@pytest.fixture(scope="module")
def tiny_pool():
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    jobs = gcm_cases.tiny_cases(2 * 4 * cus + 37)
    streams = []
    for i, j in enumerate(jobs):
        s = bytearray(_stream(j))
        if i % TINY_BAD == 5:
            s[12 + len(j.pt) + i % 16] ^= 1 << (i % 8)
        streams.append(bytes(s))
    return Pool(jobs, streams)


def _end_to_end(jobs, cls: str) -> F.Ring:
    """One ring for all jobs end to end, the wrap inside a job in the middle."""
    total = sum(len(j.pt) for j in jobs)
    q = next(i for i in range(len(jobs) // 2, len(jobs)) if len(jobs[i].pt) >= 2)
    cut = sum(len(j.pt) for j in jobs[:q]) + len(jobs[q].pt) // 2
    return F.Ring(cls, total + 53, total + 53 - cut, cut)


def test_tiny_frames_through_the_ring_form(ctx, tiny_pool):
    """At least two grid-stride passes of every workgroup and a ragged last
    one in ONE ring launch: 2 * 4 * CUs + 37 jobs of 1 .. 600 bytes, each
    under its own key (23 keys that change every few jobs), end to end in one
    ring, the wrap inside a job in the middle.  A job in 97 has a flipped tag
    bit, so the statuses show their order; its plaintext is still the job's.
    Twice: the second launch starts with warm tables."""
    jobs = tiny_pool.jobs
    statuses = tuple(int(i % TINY_BAD == 5) for i in range(len(jobs)))
    assert 1 in statuses[-TINY_BAD:] and len({j.key for j in jobs}) == 23
    launch_all(ctx, "ring", tiny_pool, [Run(tuple(range(len(jobs))), _end_to_end(jobs, "many-jobs"), statuses=statuses)],
               times=2)


@pytest.fixture(scope="module")
def key_pass_pool():
    import torch

    return Pool(gcm_cases.key_pass_cases(torch.cuda.get_device_properties(0).multi_processor_count))


def _packed(datas, jobs, kind: str):
    """One image of all jobs' streams or plaintexts, 0x5A around and between them; -> (image, offsets in its body)."""
    offs, n = [], 32
    for i, d in enumerate(datas):
        offs.append(_up(n) + (7 * i + 3) % 16)
        n = offs[-1] + len(d) + 32
    img = F.Image(np.full(n, 0x5A, np.uint8), kind)
    for o, d, j in zip(offs, datas, jobs):
        img.place(d, o + np.arange(len(d), dtype=np.int64), j.frame_size, len(j.pt), j.label)
    return img, offs


@pytest.mark.parametrize("form", ("ring", "contiguous"))
def test_long_frames_meet_another_key_in_every_pass(ctx, key_pass_pool, form):
    """The tiny frames again, with long frames (m >= 258) under another key at
    the head of each of the three grid-stride passes: a frame of up to 256
    GHASH blocks never multiplies by the key's H^256 table, so only these
    notice a table that was not reloaded for the new key.  The ring form in
    one launch, twice; the contiguous forms beside it, which had the same gap."""
    pool = key_pass_pool
    jobs, every = pool.jobs, range(len(pool.jobs))
    if form == "ring":
        launch_all(ctx, "ring", pool, [Run(tuple(every), _end_to_end(jobs, "key-passes"))], times=2)
        return
    arena = Arena()
    frames, o_fr = _packed(pool.streams, jobs, "window")
    plain, o_pt = _packed([j.pt for j in jobs], jobs, "plaintext")
    arena.add(frames, "contiguous encrypt")
    arena.add(plain, "contiguous decrypt")
    arena.upload()
    ctx.frames_device([pool.job(i, in_dev=pool.ptr(0, i), out_dev=arena.ptr(0) + o_fr[i]) for i in every])
    st = ctx.frames_device([pool.job(i, in_dev=pool.ptr(1, i), out_dev=arena.ptr(1) + o_pt[i]) for i in every],
                           decrypt=True)
    arena.check()
    assert st == [0] * len(jobs), [(i, s) for i, s in enumerate(st) if s][:8]


@pytest.mark.parametrize("which", (0, 1), ids=("65534-blocks", "65535-blocks"))
@pytest.mark.parametrize("form", FORMS)
def test_counter_edges(ctx, counter_pool, form, which):
    """The last frame of the short-counter AES path and the first of the long
    one, one boundary inside the large frame, in a block that a lane takes
    second in a pair step; encrypt also with both frames uncut."""
    job = counter_pool.jobs[which]
    runs = [Run((which,), F.counter_ring(job) if form == "ring" else F.counter_window(job))]
    if form == "encrypt-window":
        runs.append(Run((which,), F.counter_window(job, uncut=True)))
    launch_all(ctx, form, counter_pool, runs)


def _tamper_cut(job, what: str, off: int, k: int, ring: bool) -> int:
    """A boundary inside the 16-byte block or field that holds the flipped
    byte: a frame offset (window) or a plaintext offset (ring; the first
    block for the nonce and the AAD, the last for the tag)."""
    n = len(job.pt)
    last = (n - 1) // 16
    block = (off - 12) // 16 if what == "ciphertext" else last if what == "tag" else 0
    inside = F.inside_block(block, n, k)
    if inside is None:  # a last block of one byte: on its start
        inside = 16 * block
    if ring or what == "ciphertext":
        return inside if ring else 12 + inside
    if what == "tag":
        return min(max(off, 12 + n + 1), 12 + n + 15)
    return 12 if what == "aad" else min(off + 1, 11)


@pytest.mark.parametrize("form", FORMS[1:])
def test_tamper_positions(ctx, form):
    """One flipped bit anywhere in a frame or its AAD, the frame cut where the
    bit is: status 2 for the stored index, 1 for anything else, and a clean
    copy of the job beside it (ring: in the same launch) or right after it
    (window) gives 0 and the exact plaintext.  What a failed frame leaves as
    plaintext is the oracle's CTR keystream under the stored nonce."""
    lane = gcm_cases.lane_cases()
    jobs, streams, runs = [], [], []
    for i in gcm_cases.tamper_picks():
        j = lane[i]
        n = len(j.pt)
        for k, (what, off, bit) in enumerate(gcm_cases.flips(j)):
            s, a = bytearray(_stream(j)), bytearray(j.aads[0])
            (a if what == "aad" else s)[off] ^= bit
            left = oracle.gcm_encrypt(j.key, bytes(s[:12]), bytes(s[12:12 + n]), bytes(a))[0]
            assert (left == j.pt) == (what in ("tag", "aad"))
            rc, _ = oracle.frames_decrypt(j.key, bytes(s), n, **dict(j.oracle_args(), aads=[bytes(a)]))
            assert rc == (-44 if what == "index" else -41)
            status = 2 if what == "index" else 1
            jobs += [j._replace(aads=(bytes(a),)), j]
            streams += [bytes(s), _stream(j)]
            bad, good = len(jobs) - 2, len(jobs) - 1
            cut = _tamper_cut(j, what, off, k, form == "ring")
            if form == "ring":
                g = F.one_wrap("tamper-" + what, n, cut, k, total=2 * n)
                runs.append(Run((bad, good), g, pts=(left, j.pt), statuses=(status, 0)))
            else:
                g = F.one_boundary("tamper-" + what, n + 28, cut, k, i)
                assert F.boundaries(g, n + 28) == [cut]
                runs += [Run((bad,), g, pts=(left,), statuses=(status,)), Run((good,), g)]
    launch_all(ctx, form, Pool(jobs, streams), runs)


@pytest.mark.parametrize("form", FORMS)
def test_every_pointer_alignment(ctx, form):
    """include/maxio_ec.h asks no alignment of any pointer: the three-frame
    job with the window's or ring's base, the contiguous side (in_dev of
    encrypt and ring, out_dev of decrypt), aad_dev and ring_off at all 16
    residues of each, the pairings mixed."""
    job = gcm_cases.stream_cases()[0]
    n = len(job.pt)
    side = lambda i: (5 * i + 1) % 16  # noqa: E731
    pool = Pool((job,) * 16, skew=lambda i: (side(i), side(i), (3 * i + 2) % 16))
    runs = []
    for i in range(16):
        if form == "ring":
            r_bytes = n + 100 + i
            cut = 4096 + 1500 + i
            cut += (r_bytes - cut - (7 * i + 3)) % 16  # ring_off = r_bytes - cut at residue 7 i + 3
            runs.append(Run((i,), F.Ring("alignment", r_bytes, r_bytes - cut, cut), residue=i))
            assert runs[-1].g.ring_off % 16 == (7 * i + 3) % 16
        else:
            w = F.late_window(job, i)
            runs.append(Run((i,), w._replace(cls="alignment"), residue=i, residue_out=side(i)))
    arena = launch_all(ctx, form, pool, runs)
    every = set(range(16))
    assert {pool.ptr(2, i) % 16 for i in range(16)} == every
    assert {pool.ptr(0 if form == "encrypt-window" else 1, i) % 16 for i in range(16)} == every
    assert {arena.ptr(k) % 16 for k in range(0, len(arena.images), 2 if form == "decrypt-window" else 1)} == every
    if form == "decrypt-window":
        assert {arena.ptr(k) % 16 for k in range(1, len(arena.images), 2)} == every
    if form == "ring":
        assert {r.g.ring_off % 16 for r in runs} == every
