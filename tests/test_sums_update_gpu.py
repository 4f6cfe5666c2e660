"""GPU: body digests that resume (mxec_body_sums_update_device; digest_kernel.hip
body_hash_update_kernel, crc_finish_update_kernel) against hashlib, zlib and
the oracle's CRC32C -- bit-exact, as tests/test_digest_gpu.py checks the
one-shot call.  A body arrives in pieces, its state stays in a 512-byte record
in HBM between calls; the pieces here are cut at every boundary the carry has:
a pending block that fills exactly, overflows, or never fills; padding of one
and of two blocks; CRC units, rows and tiles; every pointer misalignment.

Replaces: Md5::update / ChecksumHasher::update per stream piece
(filesystem.rs:722-725)."""
from __future__ import annotations

import ctypes
import functools
import hashlib
import itertools
import zlib

import numpy as np
import pytest

import maxio_amd
import oracle
from maxio_amd import _native as N

pytestmark = pytest.mark.gpu

ALL = 0x1F
TILE = 128 << 10
STATE, REC = maxio_amd.SUMS_STATE_BYTES, 76
FIRST, FINAL = maxio_amd.SUMS_F_FIRST, maxio_amd.SUMS_F_FINAL
E_ARG = -21
# tests/test_digest_gpu.py's LENGTHS up to TILE + 1
LENGTHS = [0, 1, 15, 16, 17, 55, 56, 63, 64, 65, 119, 120, 128, 4095, 4096, 4097, TILE - 1, TILE, TILE + 1]


def _bytes(n: int, seed: int = 0) -> bytes:
    return np.random.default_rng(7000 + seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def _want(body: bytes) -> bytes:
    """The 76-byte mxec_body_sums record of a body."""
    return (hashlib.md5(body).digest() + zlib.crc32(body).to_bytes(4, "little") +
            oracle.crc32c(body).to_bytes(4, "little") + hashlib.sha1(body).digest() + hashlib.sha256(body).digest())


def _dev(data: bytes, pad: int = 0):
    import torch

    return torch.frombuffer(bytearray(data + bytes(max(pad, 1))), dtype=torch.uint8).cuda()


def _fill(n: int, value: int):
    import torch

    return torch.full((max(n, 1),), value, dtype=torch.uint8, device="cuda")


def _host(t) -> np.ndarray:
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _run(ctx, base: int, bodies, which=ALL, state_fill=0x5C, out_fill=0):
    """bodies: one list of (offset, length) pieces per body, all of the same
    count; call j takes piece j of every body (FIRST with the first, FINAL
    with the last).  Returns the n records."""
    n, calls = len(bodies), len(bodies[0])
    assert all(len(b) == calls for b in bodies)
    state, out = _fill(n * STATE, state_fill), _fill(n * REC, out_fill)
    for j in range(calls):
        flags = (FIRST if j == 0 else 0) | (FINAL if j == calls - 1 else 0)
        ctx.body_sums_update_device([base + b[j][0] for b in bodies], [b[j][1] for b in bodies], state.data_ptr(),
                                    out.data_ptr(), which, flags)
    return _host(out).reshape(n, REC)


def _pieces(off: int, lens):
    out = []
    for n in lens:
        out.append((off, n))
        off += n
    return out


def test_every_cut_of_a_200_byte_body(ctx):
    body = _bytes(200, 1)
    src = _dev(body)
    rec = _run(ctx, src.data_ptr(), [_pieces(0, (c, 200 - c)) for c in range(201)])
    for c in range(201):
        assert rec[c].tobytes() == _want(body), c


def test_every_triple_of_block_edge_lengths(ctx):
    """1000 bodies, three calls: tails that fill exactly (56 + 8 is not in the
    set, 63 + 1 and 64 + 0 are), overflow into a second block (63 + 65),
    never complete one (1 + 1 + 1, 0 + 55 + 0), and totals whose padding
    takes one block (55, 119) or two (56, 63, 120)."""
    lens = (0, 1, 55, 56, 63, 64, 65, 119, 120, 128)
    src_bytes = _bytes(3 * 128, 2)
    src = _dev(src_bytes)
    triples = list(itertools.product(lens, repeat=3))
    assert len(triples) == 1000
    rec = _run(ctx, src.data_ptr(), [_pieces(0, t) for t in triples])
    for t, r in zip(triples, rec):
        assert r.tobytes() == _want(src_bytes[:sum(t)]), t


@pytest.mark.parametrize("lens", [(TILE - 1, 1, TILE + 17), (4095, 4097, 15, 16, 17)])
def test_crc_boundaries_at_every_pointer_offset(ctx, lens):
    total = sum(lens)
    src_bytes = _bytes(total + 16, 3)
    src = _dev(src_bytes)
    assert src.data_ptr() % 16 == 0
    rec = _run(ctx, src.data_ptr(), [_pieces(off, lens) for off in range(16)])
    for off in range(16):
        assert rec[off].tobytes() == _want(src_bytes[off:off + total]), off


def test_long_carry(ctx):
    """64 pieces of 4099 bytes: the pending tail walks through every residue
    3 * j mod 64."""
    body = _bytes(64 * 4099, 4)
    src = _dev(body)
    rec = _run(ctx, src.data_ptr(), [_pieces(0, [4099] * 64)])
    assert rec[0].tobytes() == _want(body)


def test_first_final_in_one_call_is_the_one_shot_call(ctx):
    src_bytes = _bytes(max(LENGTHS), 5)
    src = _dev(src_bytes)
    base = src.data_ptr()
    n = len(LENGTHS)
    rec = _run(ctx, base, [[(0, ln)] for ln in LENGTHS], out_fill=0x11)
    shot = _fill(n * REC, 0x11)
    ctx.body_sums_device([base] * n, LENGTHS, shot.data_ptr(), ALL)
    shot = _host(shot).reshape(n, REC)
    for i, ln in enumerate(LENGTHS):
        assert rec[i].tobytes() == shot[i].tobytes(), ln
        assert rec[i].tobytes() == _want(src_bytes[:ln]), ln


def test_null_pieces_of_length_zero(ctx):
    body = _bytes(100, 6)
    src = _dev(body)
    state, out = _fill(2 * STATE, 0), _fill(2 * REC, 0)
    base = src.data_ptr()
    ctx.body_sums_update_device([None, base], [0, 60], state.data_ptr(), None, ALL, FIRST)
    ctx.body_sums_update_device([base, None], [100, 0], state.data_ptr(), None, ALL, 0)
    ctx.body_sums_update_device([None, base + 60], [0, 40], state.data_ptr(), out.data_ptr(), ALL, FINAL)
    rec = _host(out).reshape(2, REC)
    assert rec[0].tobytes() == rec[1].tobytes() == _want(body)
    ctx.body_sums_update_device([None], [0], state.data_ptr(), out.data_ptr(), ALL, FIRST | FINAL)
    assert _host(out)[:REC].tobytes() == _want(b"")


def test_garbage_in_the_record_is_ignored_at_first(ctx):
    body = _bytes(300, 7)
    src = _dev(body)
    pieces = [_pieces(0, (77, 223))]
    a = _run(ctx, src.data_ptr(), pieces, state_fill=0xFF)
    b = _run(ctx, src.data_ptr(), pieces, state_fill=0x00)
    assert a[0].tobytes() == b[0].tobytes() == _want(body)


@pytest.mark.parametrize("which", [maxio_amd.SUM_MD5, maxio_amd.SUM_CRC32 | maxio_amd.SUM_SHA1])
def test_subsets_leave_the_other_fields_untouched(ctx, which):
    body = _bytes(3000, 8)
    src = _dev(body)
    rec = _run(ctx, src.data_ptr(), [_pieces(0, (1001, 1999))], which=which, out_fill=0xAA)[0].tobytes()
    want = _want(body)
    fields = [(maxio_amd.SUM_MD5, 0, 16), (maxio_amd.SUM_CRC32, 16, 20), (maxio_amd.SUM_CRC32C, 20, 24),
              (maxio_amd.SUM_SHA1, 24, 44), (maxio_amd.SUM_SHA256, 44, 76)]
    for flag, lo, hi in fields:
        assert rec[lo:hi] == (want[lo:hi] if which & flag else b"\xAA" * (hi - lo)), flag


def test_two_records_advanced_in_alternating_calls(ctx):
    a, b = _bytes(5000, 9), _bytes(7001, 10)
    sa, sb = _dev(a), _dev(b)
    state, out = _fill(2 * STATE, 0x33), _fill(2 * REC, 0)
    st, o = state.data_ptr(), out.data_ptr()
    cuts_a, cuts_b = _pieces(0, (13, 2000, 2987)), _pieces(0, (4096, 1, 2904))
    for j in range(3):
        flags = (FIRST if j == 0 else 0) | (FINAL if j == 2 else 0)
        ctx.body_sums_update_device([sa.data_ptr() + cuts_a[j][0]], [cuts_a[j][1]], st, o, ALL, flags)
        ctx.body_sums_update_device([sb.data_ptr() + cuts_b[j][0]], [cuts_b[j][1]], st + STATE, o + REC, ALL, flags)
    rec = _host(out).reshape(2, REC)
    assert rec[0].tobytes() == _want(a) and rec[1].tobytes() == _want(b)


def test_argument_errors_enqueue_nothing(ctx):
    lib = N.lib()
    src = _dev(_bytes(64, 11))
    state, out = _fill(STATE, 0xC3), _fill(REC, 0x3C)
    p, st, o = src.data_ptr(), state.data_ptr(), out.data_ptr()

    def call(ptrs, lens, which, flags, st_, o_):
        arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
        ln = (ctypes.c_uint64 * len(lens))(*lens)
        return lib.mxec_body_sums_update_device(ctx.handle, 0, None, arr, ln, len(ptrs), which, flags, st_, o_)

    assert call([p], [64], 0x20, FIRST | FINAL, st, o) == E_ARG          # unknown `which` bit
    assert call([p], [64], ALL | 0x100, FIRST | FINAL, st, o) == E_ARG
    assert call([p], [64], ALL, 4, st, o) == E_ARG                       # unknown `flags` bit
    assert call([p], [64], ALL, FIRST | FINAL | 0x80, st, o) == E_ARG
    assert call([p], [64], ALL, FIRST, None, o) == E_ARG                 # null state_dev
    assert call([p], [64], ALL, FINAL, st, None) == E_ARG                # null out_dev with FINAL
    assert call([p], [64], ALL, FIRST | FINAL, st, None) == E_ARG
    assert call([None], [64], ALL, FIRST, st, o) == E_ARG                # a null piece of non-zero length
    assert call([p, None], [64, 1], ALL, FIRST, st, o) == E_ARG
    assert b"null piece pointer 1" in lib.mxec_last_error()
    # nothing to do is not an error
    assert call([p], [64], 0, FIRST | FINAL, st, o) == 0
    assert lib.mxec_body_sums_update_device(ctx.handle, 0, None, None, None, 0, ALL, FIRST, st, o) == 0
    assert _host(state).tobytes() == b"\xC3" * STATE
    assert _host(out).tobytes() == b"\x3C" * REC
