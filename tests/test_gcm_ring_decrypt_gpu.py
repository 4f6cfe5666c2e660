"""GPU: the GCM frame kernel's ring form alone (mxec_frames_decrypt_ring_device,
gcm_kernel.hip gcm_frames_kernel<true, false, true>): contiguous frame streams
of any number of jobs decrypted into a byte ring,

    plaintext byte o of job j -> base + (ring_off[j] + o) % bytes.

The streams are oracle.frames_encrypt's.  The ring is pre-filled from the RNG
and has 64 guard bytes of 0xAA on each side; the status array has a sentinel on
each side.  After every case the guards are intact, the ring's bytes outside
the jobs' ranges are unchanged and the sentinels are intact.

Replaces: FrameDecryptor (crypto.rs:186-420) over the frames of multipart
parts (filesystem.rs:1375-1387), whose plaintext never reaches the host."""
from __future__ import annotations

import numpy as np
import pytest

import maxio_amd
import oracle

pytestmark = pytest.mark.gpu

E_ARG = -21
GUARD = 64
RNG = np.random.default_rng(0x72696E67)
KEY = RNG.integers(0, 256, 32, dtype=np.uint8).tobytes()
PREFIX = bytes([0x81, 2, 3, 4])


def _bytes(n):
    return RNG.integers(0, 256, n, dtype=np.uint8).tobytes()


def ring_decrypt(ctx, jobs, ring_bytes, shift=0):
    """jobs: dicts of stream (bytes), n, ring_off and optionally frame_size,
    first_index, aads, key.  The ring starts `shift` bytes into its
    allocation.  Returns (per job: the plaintext read back from its range
    modulo the ring, statuses) after checking guards, the rest of the ring and
    the sentinels."""
    import torch

    fill = RNG.integers(0, 256, ring_bytes, dtype=np.uint8)
    host = np.full(shift + GUARD + ring_bytes + GUARD, 0xAA, np.uint8)
    host[shift + GUARD:shift + GUARD + ring_bytes] = fill
    d_ring = torch.from_numpy(host.copy()).cuda()
    keep, native, offs, nfs = [], [], [], []
    for j in jobs:
        fsz = j.get("frame_size", 64)
        nfs.append((j["n"] + fsz - 1) // fsz)
        d_in = torch.from_numpy(np.frombuffer(j["stream"] or b"\0", np.uint8).copy()).cuda()
        aads = j.get("aads")
        d_aad = torch.from_numpy(np.frombuffer(b"".join(aads) if aads else b"\0", np.uint8).copy()).cuda()
        keep += [d_in, d_aad]
        native.append({"key": j.get("key", KEY), "frame_size": fsz, "first_index": j.get("first_index", 0),
                       "aad_dev": d_aad.data_ptr() if aads else 0, "aad_len": len(aads[0]) if aads else 0,
                       "in_dev": d_in.data_ptr(), "len": j["n"]})
        offs.append(j["ring_off"])
    total = sum(nfs)
    d_st = torch.full((total + 2,), -7, dtype=torch.int32, device="cuda")
    ctx.frames_decrypt_ring_device(native, offs, d_ring.data_ptr() + shift + GUARD, ring_bytes, d_st.data_ptr() + 4)
    torch.cuda.synchronize()
    got, st = d_ring.cpu().numpy(), d_st.cpu().numpy()
    assert (got[:shift + GUARD] == 0xAA).all() and (got[shift + GUARD + ring_bytes:] == 0xAA).all(), \
        "a guard byte of the ring was written"
    assert st[0] == -7 and st[-1] == -7, "a status outside the jobs' frames was written"
    ring = got[shift + GUARD:shift + GUARD + ring_bytes]
    mine = np.zeros(ring_bytes, bool)
    out, at = [], 1
    for j, nf in zip(jobs, nfs):
        pos = (j["ring_off"] + np.arange(j["n"], dtype=np.int64)) % ring_bytes
        assert not mine[pos].any(), "the test's own ranges overlap"
        mine[pos] = True
        out.append((ring[pos].tobytes(), [int(v) for v in st[at:at + nf]]))
        at += nf
    assert (ring[~mine] == fill[~mine]).all(), "a ring byte outside the jobs' ranges was written"
    return out


def one(ctx, pt, ring_bytes, ring_off, frame_size=64, aad_len=0, first_index=0, shift=0, damage=None):
    nf = (len(pt) + frame_size - 1) // frame_size
    aads = [_bytes(aad_len) for _ in range(nf)] if aad_len else None
    stream = bytearray(oracle.frames_encrypt(KEY, PREFIX, pt, aads=aads, first_index=first_index, frame_size=frame_size))
    if damage:
        damage(stream, aads)
    job = {"stream": bytes(stream), "n": len(pt), "ring_off": ring_off, "frame_size": frame_size,
           "first_index": first_index, "aads": aads}
    return ring_decrypt(ctx, [job], ring_bytes, shift)[0]


def check(got, pt, what):
    out, st = got
    assert st == [0] * len(st), (what, st)
    a, b = np.frombuffer(out, np.uint8), np.frombuffer(pt, np.uint8)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, f"{what}: {bad.size} plaintext bytes differ, the first at {bad[0]}"


CUTS = (0, 1, 15, 16, 17, 63, 64, 65, 100, 144, 167, 168)


@pytest.mark.parametrize("cut", CUTS)
def test_cut_positions(ctx, cut):
    """The wrap after `cut` plaintext bytes of two 64-byte frames and one of 40:
    none (0 and 168), inside a block, on a block boundary, on a frame boundary,
    inside the second frame, inside the partial last block, on the job's end."""
    pt = _bytes(2 * 64 + 40)
    check(one(ctx, pt, 200, (200 - cut) % 200, aad_len=32), pt, cut)


@pytest.mark.parametrize("ring_bytes,shift", ((199, 0), (200, 1), (200, 7), (199, 7)))
@pytest.mark.parametrize("cut", CUTS)
def test_cut_positions_unaligned(ctx, cut, ring_bytes, shift):
    pt = _bytes(2 * 64 + 40)
    check(one(ctx, pt, ring_bytes, (ring_bytes - cut) % ring_bytes, aad_len=32, shift=shift), pt,
          (cut, ring_bytes, shift))


@pytest.mark.parametrize("aad_len", (0, 32))
@pytest.mark.parametrize("n", (16384, 16383))
def test_pair_step_frames(ctx, n, aad_len):
    """frame_size 16 384: 1 024 blocks, two per lane step.  The wrap in the
    first block of a lane's pair (block 3), in the second (block 259), on a
    block boundary (block 300) and, for 16 383, inside the partial last block,
    which the tail loop takes."""
    pt = _bytes(n)
    cuts = [16 * 3 + 5, 16 * 259 + 5, 16 * 300]
    if n == 16383:
        cuts.append(16 * 1023 + 7)
    for cut in cuts:
        ring = n + 500
        check(one(ctx, pt, ring, ring - cut, frame_size=16384, aad_len=aad_len, first_index=2 ** 40 + 3), pt,
              (n, aad_len, cut))


@pytest.mark.parametrize("slack", (1000, 0))
def test_the_reference_frame(ctx, slack):
    """65 536-byte frames, three and a short one, the wrap at offset 12 345 of
    frame 1; with no slack the job fills the ring."""
    n = 3 * 65536 + 777
    pt = _bytes(n)
    ring = n + slack
    cut = 65536 + 12345
    check(one(ctx, pt, ring, ring - cut, frame_size=65536, aad_len=32), pt, slack)


def test_several_jobs_in_one_launch(ctx):
    """Three jobs under different keys, 32-byte AADs, first indices 0, 5 and
    2^32 + 1, lengths 65, 1 and 192 end to end in a ring of 300, the wrap inside
    the third; statuses in job order."""
    lens, firsts = (65, 1, 192), (0, 5, 2 ** 32 + 1)
    start = 300 - 65 - 1 - 100  # the third job wraps after 100 bytes
    jobs, pts, at = [], [], start
    for n, first in zip(lens, firsts):
        key, pt = _bytes(32), _bytes(n)
        nf = (n + 63) // 64
        aads = [_bytes(32) for _ in range(nf)]
        jobs.append({"stream": oracle.frames_encrypt(key, PREFIX, pt, aads=aads, first_index=first, frame_size=64),
                     "n": n, "ring_off": at % 300, "first_index": first, "aads": aads, "key": key})
        pts.append(pt)
        at += n
    got = ring_decrypt(ctx, jobs, 300)
    assert [st for _, st in got] == [[0, 0], [0], [0, 0, 0]]
    assert b"".join(out for out, _ in got) == b"".join(pts)
    # a job under another job's key fails every frame, the others do not
    jobs[1]["key"] = jobs[0]["key"]
    got = ring_decrypt(ctx, jobs, 300)
    assert [st for _, st in got] == [[0, 0], [1], [0, 0, 0]]


def _flip(stream, at, bit=1):
    stream[at] ^= bit


def _swap(stream, f, g):
    a, b = bytes(stream[92 * f:92 * (f + 1)]), bytes(stream[92 * g:92 * (g + 1)])
    stream[92 * f:92 * (f + 1)], stream[92 * g:92 * (g + 1)] = b, a


DAMAGE = {
    "ciphertext bit of frame 1": (lambda s, a: _flip(s, 92 + 12 + 30, 0x20), [0, 1, 0]),
    "aad byte of frame 2": (lambda s, a: a.__setitem__(2, bytes([a[2][0] ^ 1]) + a[2][1:]), [0, 0, 1]),
    "frames 0 and 1 swapped": (lambda s, a: _swap(s, 0, 1), [2, 2, 0]),
    "index and tag of frame 1": (lambda s, a: (_flip(s, 92 + 4), _flip(s, 92 + 76 + 15, 0x80)), [0, 2, 0]),
}


@pytest.mark.parametrize("what", sorted(DAMAGE))
def test_statuses_name_the_frame_at_fault(ctx, what):
    """Three 64-byte frames, the wrap inside frame 1: only the damaged frames
    report, an index mismatch before a tag mismatch, and the good frames'
    plaintext is still right."""
    damage, want = DAMAGE[what]
    pt = _bytes(3 * 64)
    out, st = one(ctx, pt, 250, 250 - 90, aad_len=32, damage=damage)
    assert st == want, (what, st)
    for f in range(3):
        if want[f] == 0:
            assert out[64 * f:64 * (f + 1)] == pt[64 * f:64 * (f + 1)], (what, f)


@pytest.mark.parametrize("broken", (False, True))
def test_no_wrap_equals_the_contiguous_form(ctx, broken):
    import torch

    n, fsz = 3 * 4096 + 55, 4096
    pt = _bytes(n)
    stream = bytearray(oracle.frames_encrypt(KEY, PREFIX, pt, first_index=9, frame_size=fsz))
    if broken:
        stream[(4096 + 28) + 12 + 100] ^= 2  # frame 1's ciphertext
    job = {"stream": bytes(stream), "n": n, "ring_off": 0, "frame_size": fsz, "first_index": 9}
    out, st = ring_decrypt(ctx, [job], n + 4096)[0]
    d_in = torch.from_numpy(np.frombuffer(bytes(stream), np.uint8).copy()).cuda()
    d_out = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
    jst = ctx.frames_device([{"key": KEY, "frame_size": fsz, "first_index": 9, "in_dev": d_in.data_ptr(), "len": n,
                              "out_dev": d_out.data_ptr()}], decrypt=True)
    torch.cuda.synchronize()
    assert st == ([0, 1, 0, 0] if broken else [0] * 4)
    assert (jst[0] != 0) == broken
    assert d_out.cpu().numpy().tobytes() == out  # the same bytes, the failed frame's included
    if not broken:
        assert out == pt


def test_argument_errors_leave_everything_untouched(ctx):
    import ctypes

    import torch

    from maxio_amd import _native as N

    ring_bytes = 300
    host = np.full(GUARD + ring_bytes + GUARD, 0xAA, np.uint8)
    host[GUARD:GUARD + ring_bytes] = RNG.integers(0, 256, ring_bytes, dtype=np.uint8)
    d_ring = torch.from_numpy(host.copy()).cuda()
    d_in = torch.from_numpy(RNG.integers(0, 256, 4096, dtype=np.uint8)).cuda()
    d_st = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    base, st = d_ring.data_ptr() + GUARD, d_st.data_ptr()
    job = {"key": KEY, "frame_size": 64, "len": 128, "in_dev": d_in.data_ptr()}
    two = [dict(job, len=200), dict(job, len=101)]  # 301 plaintext bytes against 300
    cases = [([job], [0], base, ring_bytes, 0, "null argument"),
             ([job], [0], 0, ring_bytes, st, "null argument"),
             ([dict(job, key=None)], [0], base, ring_bytes, st, "null argument"),
             ([dict(job, in_dev=0)], [0], base, ring_bytes, st, "null argument"),
             ([dict(job, aad_len=17)], [0], base, ring_bytes, st, "null argument"),
             ([job], [0], base, 0, st, "ring bytes"),
             ([job], [ring_bytes], base, ring_bytes, st, "ring_off"),
             ([job, job], [0, 2 ** 40], base, ring_bytes, st, "ring_off"),
             ([dict(job, frame_size=0)], [0], base, ring_bytes, st, "frame_size"),
             ([dict(job, frame_size=24)], [0], base, ring_bytes, st, "frame_size"),
             ([dict(job, frame_size=2 ** 31)], [0], base, ring_bytes, st, "frame_size"),
             (two, [0, 200], base, ring_bytes, st, "overwrite itself")]
    for jobs, offs, b, nbytes, s, text in cases:
        with pytest.raises(maxio_amd.RSError) as e:
            ctx.frames_decrypt_ring_device(jobs, offs, b, nbytes, s)
        assert e.value.code == E_ARG and text in str(e.value), (jobs, offs, str(e.value))
    lib = maxio_amd.lib()
    ring = N.FramesRing(base, ring_bytes)
    arr = (N.FramesJob * 1)()
    offs = (ctypes.c_uint64 * 1)(0)
    assert lib.mxec_frames_decrypt_ring_device(ctx.handle, 0, None, None, 1, offs, ctypes.byref(ring), st) == E_ARG
    assert lib.mxec_frames_decrypt_ring_device(ctx.handle, 0, None, arr, 1, offs, None, st) == E_ARG
    assert lib.mxec_frames_decrypt_ring_device(ctx.handle, 0, None, arr, 1, None, ctypes.byref(ring), st) == E_ARG
    # nothing to do: MXEC_OK
    assert lib.mxec_frames_decrypt_ring_device(ctx.handle, 0, None, None, 0, None, None, None) == 0
    ctx.frames_decrypt_ring_device([dict(job, len=0, in_dev=0), dict(job, len=0)], [5, 299], base, ring_bytes, 0)
    torch.cuda.synchronize()
    assert (d_ring.cpu().numpy() == host).all() and (d_st.cpu().numpy() == -7).all()
    # what fits runs: a stream of noise has neither frame's index and touches no more than its plaintext
    ctx.frames_decrypt_ring_device([job], [250], base, ring_bytes, st)
    torch.cuda.synchronize()
    assert d_st.cpu().numpy().tolist() == [2, 2] + [-7] * 14
    got = d_ring.cpu().numpy()
    assert (got[:GUARD] == 0xAA).all() and (got[GUARD + ring_bytes:] == 0xAA).all()
    assert (got[GUARD + 78:GUARD + 250] == host[GUARD + 78:GUARD + 250]).all()
