"""GPU: the GCM frame kernel's decrypt window form alone
(mxec_frames_decrypt_window_device, gcm_kernel.hip gcm_frames_kernel<true, true>):
a job's frame stream read out of a ring of chunk slots,

    byte x <- base + ((x / chunk_size) % slots) * slot_stride + x % chunk_size.

The stream is oracle.frames_encrypt's, scattered by that mapping in numpy into
a window whose other bytes come from the RNG, so a read outside the mapped
range changes a tag.  The plaintext buffer is pre-filled with 0xAA with 64
guard bytes on each side, which must still be 0xAA afterwards; expected are
the plaintext and a status 0 per frame.

Replaces: FrameDecryptor (crypto.rs:186-420) over chunks resident in HBM."""
from __future__ import annotations

import numpy as np
import pytest

import maxio_amd
import oracle

pytestmark = pytest.mark.gpu

E_ARG = -21
GUARD = 64
RNG = np.random.default_rng(0x64656372)
KEY = RNG.integers(0, 256, 32, dtype=np.uint8).tobytes()
PREFIX = bytes([0x81, 2, 3, 4])


def _bytes(n):
    return RNG.integers(0, 256, n, dtype=np.uint8).tobytes()


def positions(n: int, off: int, c: int, stride: int, slots: int) -> np.ndarray:
    x = off + np.arange(n, dtype=np.uint64)
    at = ((x // np.uint64(c)) % np.uint64(slots)) * np.uint64(stride) + x % np.uint64(c)
    assert len(np.unique(at)) == n
    return at.astype(np.int64)


def scatter(stream: bytes, off: int, c: int, stride: int, slots: int) -> np.ndarray:
    win = RNG.integers(0, 256, slots * stride, dtype=np.uint8)
    win[positions(len(stream), off, c, stride, slots)] = np.frombuffer(stream, np.uint8)
    return win


def decrypt(ctx, win, n, frame_size, c, stride, slots, off, aads, first_index=0, key=KEY):
    """Decrypts n plaintext bytes out of the window (numpy or a device tensor);
    returns (plaintext with its guards, statuses)."""
    import torch

    nf = (n + frame_size - 1) // frame_size
    d_win = win if isinstance(win, torch.Tensor) else torch.from_numpy(win).cuda()
    d_aad = torch.from_numpy(np.frombuffer(b"".join(aads) if aads else b"\0", np.uint8).copy()).cuda()
    d_out = torch.full((n + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    d_st = torch.full((nf + 2,), -7, dtype=torch.int32, device="cuda")
    job = {"key": key, "frame_size": frame_size, "first_index": first_index, "aad_dev": d_aad.data_ptr() if aads else 0,
           "aad_len": len(aads[0]) if aads else 0, "len": n, "out_dev": d_out.data_ptr() + GUARD}
    ctx.frames_decrypt_window_device(job, off, d_win.data_ptr(), c, stride, slots, d_st.data_ptr() + 4)
    torch.cuda.synchronize()
    out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
    assert (out[:GUARD] == 0xAA).all() and (out[GUARD + n:] == 0xAA).all(), "a guard byte of the plaintext was written"
    assert st[0] == -7 and st[-1] == -7, "a status outside the job's frames was written"
    return out[GUARD:GUARD + n].tobytes(), [int(v) for v in st[1:-1]]


def run(ctx, pt, frame_size, c, stride, slots, off, aad_len=0, first_index=0, damage=None):
    """Encrypts with the oracle, scatters, decrypts on the device.  damage(stream, aads): what to break first."""
    nf = (len(pt) + frame_size - 1) // frame_size
    aads = [_bytes(aad_len) for _ in range(nf)] if aad_len else None
    stream = bytearray(oracle.frames_encrypt(KEY, PREFIX, pt, aads=aads, first_index=first_index, frame_size=frame_size))
    if damage:
        damage(stream, aads)
    win = scatter(bytes(stream), off, c, stride, slots)
    return decrypt(ctx, win, len(pt), frame_size, c, stride, slots, off, aads, first_index)


def check(got, pt, what):
    out, st = got
    assert st == [0] * len(st), (what, st)
    a, b = np.frombuffer(out, np.uint8), np.frombuffer(pt, np.uint8)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, f"{what}: {bad.size} plaintext bytes differ, the first at {bad[0]}"


@pytest.mark.parametrize("pad", (0, 256))
@pytest.mark.parametrize("cut", (1, 11, 12, 13, 27, 28, 75, 76, 77, 91, 92))
def test_cut_positions(ctx, cut, pad):
    """A chunk boundary at frame offset `cut` of the first 92-byte frame: inside
    the stored nonce, on its end, in a block, on a block boundary, in the tag,
    on the frame's end; the later frames are cut elsewhere."""
    c = 200
    pt = _bytes(2 * 64 + 40)
    check(run(ctx, pt, 64, c, c + pad, 3, c - cut, aad_len=32), pt, (cut, pad))


@pytest.mark.parametrize("c,frame_size,n,off", ((7, 64, 5 * 64 + 13, 3), (16, 64, 5 * 64 + 13, 5),
                                                (20000, 65536, 3 * 65536 + 777, 12345)))
def test_several_cuts_per_frame(ctx, c, frame_size, n, off):
    span = n + 28 * ((n + frame_size - 1) // frame_size)
    slots = (span + c - 1) // c  # the ring wraps inside the job
    pt = _bytes(n)
    check(run(ctx, pt, frame_size, c, c + 256, slots, off, aad_len=32), pt, (c, frame_size))


@pytest.mark.parametrize("aad_len", (0, 32))
@pytest.mark.parametrize("n", (16384, 16383))
def test_pair_step_frames_and_a_cut_partial_block(ctx, n, aad_len):
    """frame_size 16 384: 1 024 blocks, two per lane step.  With 16 383 bytes
    the partial last block (frame bytes 16 380 .. 16 394) is cut at 16 385 and
    reads 15 bytes, never 16; the index's high word is not zero."""
    pt = _bytes(n)
    check(run(ctx, pt, 16384, 16385, 16385 + 256, 2, 0, aad_len=aad_len, first_index=2 ** 40 + 3), pt, (n, aad_len))
    check(run(ctx, pt, 16384, 5000, 5000, 5, 4999, aad_len=aad_len, first_index=2 ** 64 - 1), pt,
          (n, aad_len, "small chunks"))


def test_more_frames_of_one_key_than_a_first_pass_takes(ctx):
    """2 300 frames of 16 bytes: every workgroup (four frames) comes round
    again under the same key and keeps its table."""
    n = 16 * 2299 + 3
    span = n + 28 * 2300
    pt = _bytes(n)
    check(run(ctx, pt, 16, 1000, 1000 + 256, span // 1000 + 2, 999, aad_len=1, first_index=2 ** 32 - 1200), pt,
          "grid stride")


def _flip(stream, at, bit=1):
    stream[at] ^= bit


def _first_ct_byte_after_a_boundary(frame, c, off):
    """The first ciphertext byte of `frame` (92-byte frames) that starts a chunk."""
    for x in range(92 * frame + 12, 92 * frame + 76):
        if (off + x) % c == 0:
            return x
    raise AssertionError("no boundary in the frame's ciphertext")


STATUS_CASES = {
    "tag bit of frame 2": (lambda s, a: _flip(s, 92 * 2 + 76 + 5, 0x10), 2, 1),
    "ciphertext byte after a boundary": (lambda s, a: _flip(s, _first_ct_byte_after_a_boundary(1, 7, 3)), 1, 1),
    "stored index of frame 3": (lambda s, a: _flip(s, 92 * 3 + 4 + 2, 0x04), 3, 2),
    "aad byte": (lambda s, a: a.__setitem__(4, bytes([a[4][0] ^ 1]) + a[4][1:]), 4, 1),
    "index and tag of one frame": (lambda s, a: (_flip(s, 92 * 1 + 4), _flip(s, 92 * 1 + 76 + 15, 0x80)), 1, 2),
}


@pytest.mark.parametrize("what", sorted(STATUS_CASES))
def test_statuses_name_the_frame_at_fault(ctx, what):
    """5 frames of 64 bytes and a short one, chunks of 7: only the named frame
    reports its fault, an index mismatch before a tag mismatch; the others
    report 0 and decrypt."""
    damage, frame, status = STATUS_CASES[what]
    c, fsz, n, off = 7, 64, 5 * 64 + 13, 3
    span = n + 28 * 6
    pt = _bytes(n)
    out, st = run(ctx, pt, fsz, c, c + 256, (span + c - 1) // c, off, aad_len=32, damage=damage)
    want = [0] * 6
    want[frame] = status
    assert st == want, (what, st)
    for f in range(6):
        if f != frame:
            assert out[64 * f:64 * (f + 1)] == pt[64 * f:64 * (f + 1)], (what, f)


def test_round_trip_through_the_encrypt_window_form(ctx):
    import torch

    c, stride, slots, off, n = 5000, 5000 + 256, 9, 4321, 2 * 16384 + 99
    pt = _bytes(n)
    aads = [_bytes(32) for _ in range(3)]
    d_pt = torch.from_numpy(np.frombuffer(pt, np.uint8).copy()).cuda()
    d_aad = torch.from_numpy(np.frombuffer(b"".join(aads), np.uint8).copy()).cuda()
    d_win = torch.from_numpy(RNG.integers(0, 256, slots * stride, dtype=np.uint8)).cuda()
    job = {"key": KEY, "nonce_prefix": PREFIX, "frame_size": 16384, "first_index": 7, "aad_dev": d_aad.data_ptr(),
           "aad_len": 32, "in_dev": d_pt.data_ptr(), "len": n}
    ctx.frames_encrypt_window_device(job, off, d_win.data_ptr(), c, stride, slots)
    torch.cuda.synchronize()
    check(decrypt(ctx, d_win, n, 16384, c, stride, slots, off, aads, first_index=7), pt, "round trip")


@pytest.mark.parametrize("broken", (False, True))
def test_no_boundary_touched_equals_the_contiguous_form(ctx, broken):
    import torch

    n, fsz, off = 3 * 4096 + 55, 4096, 17
    pt = _bytes(n)
    stream = bytearray(oracle.frames_encrypt(KEY, PREFIX, pt, first_index=9, frame_size=fsz))
    if broken:
        stream[(4096 + 28) + 12 + 100] ^= 2  # frame 1's ciphertext
    win = scatter(bytes(stream), off, 100000, 100000, 1)
    out, st = decrypt(ctx, win, n, fsz, 100000, 100000, 1, off, None, first_index=9)
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
    import torch

    c, slots = 106, 2
    d_win = torch.from_numpy(RNG.integers(0, 256, slots * c, dtype=np.uint8)).cuda()
    d_out = torch.full((4096,), 0xAA, dtype=torch.uint8, device="cuda")
    d_st = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    job = {"key": KEY, "frame_size": 64, "len": 2 * 64 + 1, "out_dev": d_out.data_ptr()}  # 213 stream bytes against 212
    win = dict(base_dev=d_win.data_ptr(), chunk_size=c, slot_stride=c, slots=slots, status_dev=d_st.data_ptr())
    cases = [(job, win, "exceed the window"),
             (dict(job, len=128, out_dev=0), win, "null argument"),
             (dict(job, len=128), dict(win, status_dev=0), "null argument"),
             (dict(job, len=128, key=None), win, "null argument"),
             (dict(job, len=128, aad_len=17), win, "null argument"),
             (dict(job, len=128), dict(win, base_dev=0), "null argument"),
             (dict(job, len=128, frame_size=0), win, "frame_size"),
             (dict(job, len=128, frame_size=24), win, "frame_size"),
             (dict(job, len=128, frame_size=2 ** 31), win, "frame_size"),
             (dict(job, len=128), dict(win, chunk_size=0), "chunk_size"),
             (dict(job, len=128), dict(win, slot_stride=c - 1), "slot_stride"),
             (dict(job, len=128), dict(win, slots=0), "slots")]
    for j, w, text in cases:
        with pytest.raises(maxio_amd.RSError) as e:
            ctx.frames_decrypt_window_device(j, 0, **w)
        assert e.value.code == E_ARG and text in str(e.value), (j, w, str(e.value))
    lib = maxio_amd.lib()
    assert lib.mxec_frames_decrypt_window_device(ctx.handle, 0, None, None, 0, None, None) == E_ARG
    ctx.frames_decrypt_window_device(dict(job, len=0, out_dev=0), 7, **dict(win, status_dev=0))  # nothing to do: MXEC_OK
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xAA).all() and (d_st.cpu().numpy() == -7).all()
    # one byte less fits; a stream of noise has neither frame's index (which comes before its tag) and
    # touches no more than its plaintext
    ctx.frames_decrypt_window_device(dict(job, len=128), 0, **win)
    torch.cuda.synchronize()
    assert d_st.cpu().numpy().tolist() == [2, 2] + [-7] * 14
    assert (d_out.cpu().numpy()[128:] == 0xAA).all()
