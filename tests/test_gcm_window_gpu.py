"""GPU: the GCM frame kernel's window form alone
(mxec_frames_encrypt_window_device, gcm_kernel.hip gcm_frames_kernel<false, true>):
a job's frame stream stored into a ring of chunk slots,

    byte x -> base + ((x / chunk_size) % slots) * slot_stride + x % chunk_size.

Expected bytes are oracle.frames_encrypt's, scattered by that mapping in numpy
into a window pre-filled with 0xAA; every byte outside the mapped range must
still be 0xAA afterwards."""
from __future__ import annotations

import numpy as np
import pytest

import maxio_amd
import oracle

pytestmark = pytest.mark.gpu

E_ARG = -21
RNG = np.random.default_rng(0x77696E64)
KEY = RNG.integers(0, 256, 32, dtype=np.uint8).tobytes()
PREFIX = bytes([0x81, 2, 3, 4])


def _bytes(n):
    return RNG.integers(0, 256, n, dtype=np.uint8).tobytes()


def scatter(stream: bytes, off: int, c: int, stride: int, slots: int) -> np.ndarray:
    win = np.full(slots * stride, 0xAA, np.uint8)
    x = off + np.arange(len(stream), dtype=np.uint64)
    at = ((x // np.uint64(c)) % np.uint64(slots)) * np.uint64(stride) + x % np.uint64(c)
    assert len(np.unique(at)) == len(stream)
    win[at.astype(np.int64)] = np.frombuffer(stream, np.uint8)
    return win


def run(ctx, pt, frame_size, c, stride, slots, off, aad_len=0, first_index=0, key=KEY):
    """Encrypts pt into a window on the device; returns (window bytes, expected window bytes)."""
    import torch

    nf = (len(pt) + frame_size - 1) // frame_size
    aads = [_bytes(aad_len) for _ in range(nf)] if aad_len else None
    stream = oracle.frames_encrypt(key, PREFIX, pt, aads=aads, first_index=first_index, frame_size=frame_size)
    want = scatter(stream, off, c, stride, slots)
    d_pt = torch.from_numpy(np.frombuffer(pt, np.uint8).copy()).cuda()
    d_aad = torch.from_numpy(np.frombuffer(b"".join(aads) if aads else b"\0", np.uint8).copy()).cuda()
    d_win = torch.full((slots * stride,), 0xAA, dtype=torch.uint8, device="cuda")
    job = {"key": key, "nonce_prefix": PREFIX, "frame_size": frame_size, "first_index": first_index,
           "aad_dev": d_aad.data_ptr() if aads else 0, "aad_len": aad_len, "in_dev": d_pt.data_ptr(), "len": len(pt)}
    ctx.frames_encrypt_window_device(job, off, d_win.data_ptr(), c, stride, slots)
    torch.cuda.synchronize()
    return d_win.cpu().numpy(), want


def check(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} window bytes differ, the first at {bad[0]}: " \
                          f"got {got[bad[0]]:#x}, want {want[bad[0]]:#x}"


@pytest.mark.parametrize("pad", (0, 256))
@pytest.mark.parametrize("cut", (1, 11, 12, 13, 27, 28, 75, 76, 77, 91, 92))
def test_cut_positions(ctx, cut, pad):
    """A chunk boundary at frame offset `cut` of the first 92-byte frame: inside
    the nonce, on its end, in a block, on a block boundary, in the tag, on
    the frame's end; the later frames are cut elsewhere."""
    c = 200
    got, want = run(ctx, _bytes(2 * 64 + 40), 64, c, c + pad, 3, c - cut, aad_len=32)
    check(got, want, (cut, pad))


@pytest.mark.parametrize("c,frame_size,n,off", ((7, 64, 5 * 64 + 13, 3), (16, 64, 5 * 64 + 13, 5),
                                                (20000, 65536, 3 * 65536 + 777, 12345)))
def test_several_cuts_per_frame(ctx, c, frame_size, n, off):
    span = n + 28 * ((n + frame_size - 1) // frame_size)
    slots = (span + c - 1) // c  # the ring wraps inside the job
    got, want = run(ctx, _bytes(n), frame_size, c, c + 256, slots, off, aad_len=32)
    check(got, want, (c, frame_size))


def test_wrap_a_job_of_exactly_two_chunks(ctx):
    got, want = run(ctx, _bytes(2 * 64), 64, 92, 92 + 256, 2, 50)  # 184 stream bytes over three chunk pieces
    check(got, want, "wrap")
    got, want = run(ctx, _bytes(2 * 64), 64, 92, 92, 2, 5 * 92)
    check(got, want, "aligned")


def test_one_byte_more_than_the_window_is_refused_untouched(ctx):
    import torch

    pt = _bytes(2 * 64 + 1)  # 213 stream bytes against 2 * 106
    d_pt = torch.from_numpy(np.frombuffer(pt, np.uint8).copy()).cuda()
    d_win = torch.full((2 * 106,), 0xAA, dtype=torch.uint8, device="cuda")
    job = {"key": KEY, "nonce_prefix": PREFIX, "frame_size": 64, "in_dev": d_pt.data_ptr(), "len": len(pt)}
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.frames_encrypt_window_device(job, 0, d_win.data_ptr(), 106, 106, 2)
    assert e.value.code == E_ARG and "overwrite itself" in str(e.value)
    torch.cuda.synchronize()
    assert (d_win.cpu().numpy() == 0xAA).all()
    ctx.frames_encrypt_window_device(dict(job, len=2 * 64), 0, d_win.data_ptr(), 106, 106, 2)  # one byte less fits


def test_no_boundary_touched_equals_the_contiguous_form(ctx):
    import torch

    pt = _bytes(3 * 4096 + 55)
    got, want = run(ctx, pt, 4096, 100000, 100000, 1, 17, aad_len=0, first_index=9)
    check(got, want, "one chunk")
    d_pt = torch.from_numpy(np.frombuffer(pt, np.uint8).copy()).cuda()
    d_out = torch.full((100000,), 0xAA, dtype=torch.uint8, device="cuda")
    ctx.frames_device([{"key": KEY, "nonce_prefix": PREFIX, "frame_size": 4096, "first_index": 9,
                        "in_dev": d_pt.data_ptr(), "len": len(pt), "out_dev": d_out.data_ptr() + 17}])
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == got).all()


@pytest.mark.parametrize("aad_len", (0, 32))
@pytest.mark.parametrize("n", (16384, 16383))
def test_pair_step_frames_and_a_cut_partial_block(ctx, n, aad_len):
    """frame_size 16 384: 1 024 blocks, two per lane step.  With 16 383 bytes
    the partial last block (frame bytes 16 380 .. 16 394) is cut at 16 385;
    the index's high word is not zero."""
    got, want = run(ctx, _bytes(n), 16384, 16385, 16385 + 256, 2, 0, aad_len=aad_len, first_index=2 ** 40 + 3)
    check(got, want, (n, aad_len))
    got, want = run(ctx, _bytes(n), 16384, 5000, 5000, 5, 4999, aad_len=aad_len, first_index=2 ** 64 - 1)
    check(got, want, (n, aad_len, "small chunks"))


def test_more_frames_of_one_key_than_a_first_pass_takes(ctx):
    """2 300 frames of 16 bytes: every workgroup (four frames) comes round
    again under the same key and keeps its table."""
    n = 16 * 2299 + 3
    span = n + 28 * 2300
    got, want = run(ctx, _bytes(n), 16, 1000, 1000 + 256, span // 1000 + 2, 999, aad_len=1, first_index=2 ** 32 - 1200)
    check(got, want, "grid stride")


def test_argument_errors_and_an_empty_job(ctx):
    import torch

    d = torch.full((4096,), 0xAA, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    good = {"key": KEY, "frame_size": 64, "in_dev": p, "len": 100}
    win = dict(base_dev=p + 1024, chunk_size=200, slot_stride=200, slots=4)
    cases = [(dict(good, key=None), win, "null argument"),
             (dict(good, in_dev=0), win, "null argument"),
             (dict(good, aad_len=17), win, "null argument"),
             (good, dict(win, base_dev=0), "null argument"),
             (dict(good, frame_size=0), win, "frame_size"),
             (dict(good, frame_size=72), win, "frame_size"),
             (good, dict(win, chunk_size=0), "chunk_size"),
             (good, dict(win, slot_stride=199), "slot_stride"),
             (good, dict(win, slots=0), "slots"),
             (good, dict(win, slots=2 ** 63), "2^62")]
    for job, w, text in cases:
        with pytest.raises(maxio_amd.RSError) as e:
            ctx.frames_encrypt_window_device(job, 7, **w)
        assert e.value.code == E_ARG and text in str(e.value), (job, w, str(e.value))
    lib = maxio_amd.lib()
    assert lib.mxec_frames_encrypt_window_device(ctx.handle, 0, None, None, 0, None) == E_ARG
    ctx.frames_encrypt_window_device(dict(good, len=0, in_dev=0), 7, **win)  # nothing to do: MXEC_OK
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 0xAA).all()
