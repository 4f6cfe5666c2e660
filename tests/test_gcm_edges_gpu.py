"""GPU: the AES-256-GCM frame kernel (gcm_kernel.hip) at the edges it has,
every frame against the oracle (oracle/gcm_oracle.c, pinned to OpenSSL on
these very frames by tests/test_oracle_gcm.py):

  * frame indices whose high word is not zero, on both sides;
  * AADs with a partial last block, of 1, 2, 3 and 255 .. 257 blocks;
  * GHASH sequences on both sides of every multiple of the 256 lanes, with a
    whole and a partial last payload block;
  * the last frame of the short-counter AES path (65534 blocks);
  * several grid-stride passes of tiny frames, a ragged last pass;
  * which byte of a frame was tampered with, and which frame's error wins;
  * job pointers at every byte alignment (include/maxio_ec.h asks for none)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import gcm_cases
import maxio_amd
import oracle

pytestmark = pytest.mark.gpu

E_INTEGRITY, ORC_AUTH, ORC_INDEX = -41, -41, -44
AUTH_MSG = "AES-GCM decryption failed: authentication error"


@functools.lru_cache(maxsize=None)
def _want(job) -> bytes:
    return oracle.frames_encrypt(job.key, job.prefix, job.pt, **job.oracle_args())


def _up(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


class Packed:
    """jobs laid out in four device tensors: plaintexts and frame streams at
    16-byte steps plus the given byte skew, AADs packed byte to byte, and a
    buffer for the way back.  GUARD bytes of 0xA5 lie between neighbours."""

    GUARD = 32

    def __init__(self, jobs, skew=lambda i: (0, 0, 0)):
        import torch

        self.jobs = jobs
        self.o_pt, self.o_fr, self.o_aad, self.o_back = [], [], [], []
        n_pt = n_fr = n_aad = n_back = self.GUARD
        for i, j in enumerate(jobs):
            s_pt, s_fr, s_back = skew(i)
            self.o_pt.append(_up(n_pt) + s_pt)
            self.o_fr.append(_up(n_fr) + s_fr)
            self.o_back.append(_up(n_back) + s_back)
            self.o_aad.append(n_aad)
            n_pt = self.o_pt[-1] + len(j.pt) + self.GUARD
            n_fr = self.o_fr[-1] + j.frames_len + self.GUARD
            n_back = self.o_back[-1] + len(j.pt) + self.GUARD
            n_aad += j.aad_len * j.n_frames
        pt = np.full(n_pt, 0xA5, np.uint8)
        aad = np.full(n_aad + self.GUARD, 0xA5, np.uint8)
        for i, j in enumerate(jobs):
            pt[self.o_pt[i]:self.o_pt[i] + len(j.pt)] = np.frombuffer(j.pt, np.uint8)
            if j.aad_len:
                a = b"".join(j.aads)
                aad[self.o_aad[i]:self.o_aad[i] + len(a)] = np.frombuffer(a, np.uint8)
        self.pt = torch.from_numpy(pt).cuda()
        self.aad = torch.from_numpy(aad).cuda()
        self.fr = torch.full((n_fr,), 0xA5, dtype=torch.uint8, device="cuda")
        self.back = torch.full((n_back,), 0xA5, dtype=torch.uint8, device="cuda")

    def _job(self, i, in_dev, out_dev):
        j = self.jobs[i]
        return {"key": j.key, "nonce_prefix": j.prefix, "frame_size": j.frame_size, "first_index": j.first_index,
                "aad_dev": self.aad.data_ptr() + self.o_aad[i] if j.aad_len else 0, "aad_len": j.aad_len,
                "in_dev": in_dev, "len": len(j.pt), "out_dev": out_dev}

    def encrypt_jobs(self):
        return [self._job(i, self.pt.data_ptr() + self.o_pt[i], self.fr.data_ptr() + self.o_fr[i])
                for i in range(len(self.jobs))]

    def decrypt_jobs(self):
        return [self._job(i, self.fr.data_ptr() + self.o_fr[i], self.back.data_ptr() + self.o_back[i])
                for i in range(len(self.jobs))]

    @staticmethod
    def _check_layout(host, offs, lens, what):
        """Every job's bytes and the untouched 0xA5 between neighbours."""
        mask = np.ones(host.size, bool)
        for o, n in zip(offs, lens):
            mask[o:o + n] = False
        assert (host[mask] == 0xA5).all(), f"{what}: bytes outside every job's range were written"

    def check_frames(self):
        """The frame streams on the device against the oracle, job by job."""
        import torch

        torch.cuda.synchronize()
        host = self.fr.cpu().numpy()
        for i, j in enumerate(self.jobs):
            got = host[self.o_fr[i]:self.o_fr[i] + j.frames_len].tobytes()
            if got != _want(j):
                pytest.fail(f"job {i} (aad_len, len, first_index) = {j.label}: " + _first_difference(j, got, _want(j)))
        self._check_layout(host, self.o_fr, [j.frames_len for j in self.jobs], "frames")
        return host

    def check_plaintexts(self, status):
        import torch

        torch.cuda.synchronize()
        bad = [(i, s, self.jobs[i].label) for i, s in enumerate(status) if s != 0]
        assert not bad, f"decrypt statuses (job, status, (aad_len, len, first_index)): {bad[:5]}"
        host = self.back.cpu().numpy()
        for i, j in enumerate(self.jobs):
            got = host[self.o_back[i]:self.o_back[i] + len(j.pt)].tobytes()
            assert got == j.pt, f"job {i} (aad_len, len, first_index) = {j.label}: plaintext differs"
        self._check_layout(host, self.o_back, [len(j.pt) for j in self.jobs], "plaintexts")


def _first_difference(job, got: bytes, want: bytes) -> str:
    for f, (fo, _, ln, index) in enumerate(gcm_cases.frame_slices(job)):
        for name, a, b in (("header", fo, fo + 12), ("ciphertext", fo + 12, fo + 12 + ln),
                           ("tag", fo + 12 + ln, fo + 28 + ln)):
            if got[a:b] != want[a:b]:
                at = next(k for k in range(b - a) if got[a + k] != want[a + k])
                return (f"frame {f} (index {index}): {name} differs from byte {at} of {b - a}: "
                        f"got {got[a + at:a + at + 16].hex()}, want {want[a + at:a + at + 16].hex()}")
    return "length differs"


@pytest.fixture(scope="module")
def sweep(ctx):
    """lane_cases() + stream_cases() encrypted by one launch, left on the device."""
    p = Packed(gcm_cases.lane_cases() + gcm_cases.stream_cases())
    ctx.frames_device(p.encrypt_jobs())
    return p


def test_lane_sweep_encrypt_then_decrypt(ctx, sweep):
    sweep.check_frames()
    sweep.check_plaintexts(ctx.frames_device(sweep.decrypt_jobs(), decrypt=True))


def test_many_small_frames_several_passes(ctx):
    """At least two passes of every workgroup (four frames each) and a ragged
    last one, over frames of 1 .. 600 bytes under 23 keys that change every
    few jobs."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = Packed(gcm_cases.tiny_cases(2 * 4 * cus + 37))
    for _ in range(2):  # twice: the second run starts with warm tables and clocks
        p.fr.fill_(0xA5)
        p.back.fill_(0xA5)
        ctx.frames_device(p.encrypt_jobs())
        p.check_frames()
        p.check_plaintexts(ctx.frames_device(p.decrypt_jobs(), decrypt=True))


def test_counter_boundary_frame(ctx):
    """Host forms over a frame of exactly 65534 blocks: counters 2 .. 0xFFFF,
    every value of the two counter bytes that the short path looks up."""
    job = gcm_cases.counter_edge_case()
    got = ctx.frames_encrypt(job.key, job.prefix, job.pt, **job.oracle_args())
    if got != _want(job):
        pytest.fail(f"(aad_len, len, first_index) = {job.label}: " + _first_difference(job, got, _want(job)))
    assert ctx.frames_decrypt(job.key, got, len(job.pt), **job.oracle_args()) == job.pt


_flips = gcm_cases.flips  # shared with test_gcm_form_edges_gpu.py


def test_tamper_positions(ctx, sweep):
    """One flipped bit anywhere in a frame or its AAD fails that job and no
    other; the host form names both indices of an index mismatch in full."""
    import torch

    lane = gcm_cases.lane_cases()
    picks = gcm_cases.tamper_picks()
    frames_host = sweep.check_frames()
    # jobs: clean, flipped, clean, flipped, ..., clean; each on its own copy
    entries = [(i, flip) for i in picks for flip in _flips(lane[i])]
    jobs, streams, aads = [], [], []
    for i, flip in entries:
        for fl in (None, flip):
            j = lane[i]
            s = bytearray(frames_host[sweep.o_fr[i]:sweep.o_fr[i] + j.frames_len].tobytes())
            a = bytearray(j.aads[0])
            if fl:
                what, off, bit = fl
                (a if what == "aad" else s)[off] ^= bit
            jobs.append(j)
            streams.append(bytes(s))
            aads.append(bytes(a))
    jobs.append(lane[picks[0]])
    streams.append(_want(lane[picks[0]]))
    aads.append(lane[picks[0]].aads[0])
    p = Packed([j._replace(aads=(a,)) for j, a in zip(jobs, aads)])
    fr = np.full(p.fr.numel(), 0xA5, np.uint8)
    for o, s in zip(p.o_fr, streams):
        fr[o:o + len(s)] = np.frombuffer(s, np.uint8)
    p.fr = torch.from_numpy(fr).cuda()
    status = ctx.frames_device(p.decrypt_jobs(), decrypt=True)
    torch.cuda.synchronize()
    back = p.back.cpu().numpy()
    for n, (i, flip) in enumerate(entries):
        j, (what, off, bit) = lane[i], flip
        where = (j.label, what, off, bit)
        assert status[2 * n] == 0, ("clean neighbour", where)
        assert back[p.o_back[2 * n]:p.o_back[2 * n] + len(j.pt)].tobytes() == j.pt, ("clean neighbour", where)
        assert status[2 * n + 1] == E_INTEGRITY, where
        args = dict(j.oracle_args(), aads=[aads[2 * n + 1]])
        rc, _ = oracle.frames_decrypt(j.key, streams[2 * n + 1], len(j.pt), **args)
        assert rc == (ORC_INDEX if what == "index" else ORC_AUTH), where
        if what == "index":
            stored = int.from_bytes(streams[2 * n + 1][4:12], "little")
            assert stored == j.first_index ^ (bit << (8 * (off - 4)))
            with pytest.raises(maxio_amd.RSError) as e:
                ctx.frames_decrypt(j.key, streams[2 * n + 1], len(j.pt), **args)
            assert e.value.code == E_INTEGRITY, where
            assert f"frame index mismatch: expected {j.first_index}, got {stored}" in str(e.value), where
    assert status[-1] == 0


def test_first_failing_frame_wins(ctx):
    """Two frames of one stream fail differently: the first failing frame's
    error is the one reported, as the reference's sequential decryptor does."""
    rng = np.random.default_rng(0x66697273)
    key, prefix = rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), bytes([0x80, 1, 2, 3])
    fs, first = 1008, 2**32 - 1
    pt = rng.integers(0, 256, 4 * fs, dtype=np.uint8).tobytes()
    good = ctx.frames_encrypt(key, prefix, pt, first_index=first, frame_size=fs)
    assert good == oracle.frames_encrypt(key, prefix, pt, first_index=first, frame_size=fs)
    fl = fs + 28
    tag_of, index_of = (lambda f: f * fl + 12 + fs + 3), (lambda f: f * fl + 4 + 5)

    def outcome(flips):
        bad = bytearray(good)
        for at in flips:
            bad[at] ^= 0x20
        rc, _ = oracle.frames_decrypt(key, bytes(bad), len(pt), first_index=first, frame_size=fs)
        with pytest.raises(maxio_amd.RSError) as e:
            ctx.frames_decrypt(key, bytes(bad), len(pt), first_index=first, frame_size=fs)
        assert e.value.code == E_INTEGRITY
        return rc, str(e.value)

    rc, msg = outcome([tag_of(1), index_of(2)])
    assert rc == ORC_AUTH and AUTH_MSG in msg and "index mismatch" not in msg
    rc, msg = outcome([index_of(1), tag_of(2)])
    assert rc == ORC_INDEX
    assert f"frame index mismatch: expected {2**32}, got {2**32 ^ (0x20 << 40)}" in msg


def test_every_pointer_alignment(ctx):
    """include/maxio_ec.h asks no alignment of in_dev, out_dev and aad_dev:
    a three-frame job at all 16 residues of each, the pairings mixed."""
    job = gcm_cases.stream_cases()[0]
    p = Packed((job,) * 16, skew=lambda i: (i, (5 * i + 1) % 16, (3 * i + 2) % 16))
    assert {o % 16 for o in p.o_pt} == {o % 16 for o in p.o_fr} == {o % 16 for o in p.o_back} == set(range(16))
    ctx.frames_device(p.encrypt_jobs())
    p.check_frames()
    p.check_plaintexts(ctx.frames_device(p.decrypt_jobs(), decrypt=True))


def test_device_forms_reject_before_launch(ctx):
    """Bad jobs are turned away before anything is enqueued, the good jobs
    next to them included: the pointers here are ones no kernel could read.
    A decrypt that checked nothing raises; it does not report statuses."""
    good = {"key": bytes(32), "in_dev": 4096, "out_dev": 8192, "len": 100, "frame_size": 1024}
    for bad, text in ((dict(good, frame_size=1000), "frame_size must be a positive multiple of 16"),
                      (dict(good, frame_size=0), "frame_size must be a positive multiple of 16"),
                      (dict(good, in_dev=0), "null argument"),
                      (dict(good, out_dev=0), "null argument"),
                      (dict(good, aad_len=17), "null argument")):
        for decrypt in (False, True):
            with pytest.raises(maxio_amd.RSError) as e:
                ctx.frames_device([good, bad], decrypt=decrypt)
            assert e.value.code == -21 and text in str(e.value), (bad, decrypt)
