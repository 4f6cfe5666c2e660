"""GPU: the streaming encrypted GET (mxec_reader_open_encrypted): a pull
stream whose reads, concatenated, are what mxec_get_object_chunked_encrypted
returns for the same arguments -- every range, read size and batch size --
and whose failures stream: a bad frame or an unrecoverable chunk fails the
read that reaches it, after the plaintext of every frame in front of it.

Small objects are built from oracle.frames_encrypt with 64-byte frames (92
bytes in the stream) and stored with put_object_chunked in chunks of 101:
coprime to 92, so over 101 frames a chunk boundary falls at every frame offset.

Replaces: FrameDecryptor::for_range over VerifiedChunkReader (crypto.rs:186-420,
filesystem.rs:1618-1630, :1700-1725)."""
from __future__ import annotations

import os
import shutil
import threading

import numpy as np
import pytest

import maxio_amd
import oracle

pytestmark = pytest.mark.gpu

E_INTEGRITY = -41
RNG = np.random.default_rng(0x72656164)
KEY = RNG.integers(0, 256, 32, dtype=np.uint8).tobytes()
NONCE = bytes([9, 8, 7, 6])
AAD = oracle.object_aad_prefix("bkt", "obj/key", "v3")
FS, FL = 64, 92
LENGTHS = (None, 0, 1, 64, 65, 1000)
READS = (1, 7, 4096, None)
BATCHES = (1, 250, 0)


def _bytes(n):
    return RNG.integers(0, 256, n, dtype=np.uint8).tobytes()


def offsets(n):
    return (0, 1, 63, 64, 65, 640, n - 1, n, n + 5)


def stream_of(pt, frame_size=FS, key=KEY):
    nf = (len(pt) + frame_size - 1) // frame_size
    return oracle.frames_encrypt(key, NONCE, pt, aads=[oracle.frame_aad(AAD, i) for i in range(nf)],
                                 frame_size=frame_size)


def drain(reader, read_size):
    """Everything the reader gives, and the error that ended it (or None)."""
    out = []
    try:
        while True:
            b = reader.read((1 << 24) if read_size is None else read_size)  # None: more than any object here
            if not b:
                return b"".join(out), None
            out.append(b)
    except maxio_amd.RSError as e:
        return b"".join(out), e


def stream_read(ctx, d, off=0, ln=None, read_size=None, batch=0, n=None, frame_size=FS, key=KEY):
    with ctx.open_reader_encrypted(d, key, AAD, off, ln, plaintext_size=n, frame_size=frame_size,
                                   batch_bytes=batch) as r:
        got, err = drain(r, read_size)
        if err is not None:  # after an error, every later read returns it again
            for _ in range(2):
                with pytest.raises(maxio_amd.RSError) as again:
                    r.read(10)
                assert (again.value.code, str(again.value)) == (err.code, str(err))
        return got, err


def buffered(ctx, d, off=0, ln=None, n=None, frame_size=FS, key=KEY):
    try:
        return ctx.get_object_chunked_encrypted(d, key, AAD, off, ln, plaintext_size=n, frame_size=frame_size), None
    except maxio_amd.RSError as e:
        return b"", e


@pytest.fixture(scope="module")
def small(ctx, tmp_path_factory):
    """101 frames of 64 bytes in 92 chunks of 101, m = 2; (dir, plaintext, every range's buffered answer)."""
    d = str(tmp_path_factory.mktemp("small") / "o.ec")
    pt = _bytes(101 * FS)
    ctx.put_object_chunked(d, 101, 2, stream_of(pt))
    assert len(os.listdir(d)) == 92 + 2 + 1
    want = {(o, l): ctx.get_object_chunked_encrypted(d, KEY, AAD, o, l, plaintext_size=len(pt), frame_size=FS)
            for o in offsets(len(pt)) for l in LENGTHS}
    assert want[(0, None)] == pt and want[(65, 1000)] == pt[65:1065]
    return d, pt, want


@pytest.fixture(scope="module")
def big(ctx, tmp_path_factory):
    """Three 64 KiB frames and a short one, chunks of 20 000, m = 2, written by the library; no plaintext_size passed."""
    d = str(tmp_path_factory.mktemp("big") / "o.ec")
    pt = _bytes(3 * 65536 + 777)
    ctx.put_object_chunked_encrypted(d, 20000, 2, KEY, NONCE, AAD, pt)
    want = {(o, l): ctx.get_object_chunked_encrypted(d, KEY, AAD, o, l) for o in offsets(len(pt)) for l in LENGTHS}
    assert want[(0, None)] == pt
    return d, pt, want


@pytest.mark.parametrize("batch", BATCHES)
def test_small_object_equals_the_buffered_get(ctx, small, batch):
    d, pt, want = small
    for (o, l), w in want.items():
        for rs in READS:
            got, err = stream_read(ctx, d, o, l, rs, batch, n=len(pt))
            assert err is None and got == w, (o, l, rs, batch, err, len(got), len(w))


@pytest.mark.parametrize("batch", BATCHES)
def test_64k_frames_equal_the_buffered_get(ctx, big, batch):
    d, pt, want = big
    for (o, l), w in want.items():
        for rs in READS:
            if rs == 1 and len(w) > 5000:
                rs = 4097  # 200 000 one-byte reads tell nothing the small object's have not
            got, err = stream_read(ctx, d, o, l, rs, batch, frame_size=65536)
            assert err is None and got == w, (o, l, rs, batch, err, len(got), len(w))


def test_chunk_smaller_than_a_frame(ctx, tmp_path):
    """Chunks of 7: a 92-byte frame lies in 14 or 15 of them, one chunk a round."""
    d = str(tmp_path / "o.ec")
    pt = _bytes(5 * FS)
    ctx.put_object_chunked(d, 7, 2, stream_of(pt))
    assert len(os.listdir(d)) == 66 + 2 + 1
    for o, l in ((0, None), (1, 64), (63, 2), (64, 65), (100, 1000), (319, None), (320, None)):
        for rs in (1, 7, None):
            got, err = stream_read(ctx, d, o, l, rs, 1, n=len(pt))
            assert err is None and got == pt[o:][:l], (o, l, rs)


def _flip(path, at):
    with open(path, "r+b") as f:
        f.seek(at)
        b = f.read(1)
        f.seek(at)
        f.write(bytes([b[0] ^ 0x40]))


def _chunk(d, i):
    return os.path.join(d, "%06d" % i)


DAMAGE = {
    "a data chunk deleted": lambda d: os.remove(_chunk(d, 3)),
    "one byte flipped": lambda d: _flip(_chunk(d, 4), 50),
    "a chunk truncated": lambda d: os.truncate(_chunk(d, 5), 60),
    "two chunks bad in one round": lambda d: (_flip(_chunk(d, 6), 0), os.remove(_chunk(d, 7))),
}


@pytest.mark.parametrize("what", sorted(DAMAGE))
def test_degraded_with_parity_reads_the_same(ctx, small, tmp_path, what):
    src, pt, want = small
    d = str(tmp_path / "o.ec")
    shutil.copytree(src, d)
    DAMAGE[what](d)
    for batch in (0, 1):  # all the chunks in one round; one a round
        got, err = stream_read(ctx, d, 0, None, 4096, batch, n=len(pt))
        assert err is None and got == pt, (what, batch, err)
    got, err = stream_read(ctx, d, 300, 500, 7, 250, n=len(pt))
    assert err is None and got == pt[300:800], (what, err)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("bad", (0, 5, 91))
def test_unrecoverable_chunk_fails_after_the_frames_before_it(ctx, tmp_path, batch, bad):
    d = str(tmp_path / "o.ec")
    pt = _bytes(101 * FS)
    ctx.put_object_chunked(d, 101, 0, stream_of(pt))
    _flip(_chunk(d, bad), 17)
    whole = (bad * 101) // FL  # frames that end before chunk `bad`
    for rs in (1, 4096, None):
        got, err = stream_read(ctx, d, 0, None, rs, batch, n=len(pt))
        assert got == pt[:whole * FS], (bad, rs, len(got))
        assert err is not None and err.code == E_INTEGRITY and "checksum mismatch on chunk %d" % bad in str(err)
    _, berr = buffered(ctx, d, n=len(pt))
    assert (berr.code, str(berr)) == (err.code, str(err))
    got, err = stream_read(ctx, d, 70, 20, 3, batch, n=len(pt))  # a range the bad chunk is no part of
    if bad != 0 and bad != 1:
        assert err is None and got == pt[70:90]


def _frame_cases(pt):
    s = bytearray(stream_of(pt))
    j = 37
    tag = bytearray(s)
    tag[FL * j + 12 + FS + 3] ^= 0x08
    swap = bytearray(s)
    swap[FL * j:FL * (j + 1)], swap[FL * (j + 1):FL * (j + 2)] = s[FL * (j + 1):FL * (j + 2)], s[FL * j:FL * (j + 1)]
    return {
        "tag": (bytes(tag), KEY, j, "AES-GCM decryption failed: authentication error"),
        "swap": (bytes(swap), KEY, j, "frame index mismatch: expected %d, got %d" % (j, j + 1)),
        "short": (bytes(s[:-5]), KEY, 100, "truncated encrypted frame"),
        "key": (bytes(s), bytes(32), 0, "AES-GCM decryption failed: authentication error"),
    }


@pytest.mark.parametrize("what", ("tag", "swap", "short", "key"))
def test_bad_frames_inside_good_chunks(ctx, tmp_path, what):
    """The damaged stream is stored as it is, so every chunk matches its digest:
    the plaintext of the frames before the bad one, then crypto.rs's error --
    the code and text of the buffered call for the same object."""
    pt = _bytes(101 * FS)
    stream, key, first_bad, text = _frame_cases(pt)[what]
    d = str(tmp_path / "o.ec")
    ctx.put_object_chunked(d, 101, 2, stream)
    _, berr = buffered(ctx, d, n=len(pt), key=key)
    assert berr is not None and berr.code == E_INTEGRITY and text in str(berr)
    for batch in BATCHES:
        for rs in (1, 4096, None):
            got, err = stream_read(ctx, d, 0, None, rs, batch, n=len(pt), key=key)
            assert got == pt[:first_bad * FS], (what, batch, rs, len(got))
            assert err is not None and (err.code, str(err)) == (berr.code, str(berr)), (what, str(err))
    # a range in front of the bad frame is served whole; one that starts in it gives nothing
    if first_bad:
        got, err = stream_read(ctx, d, 5, first_bad * FS - 5, 7, 1, n=len(pt), key=key)
        assert err is None and got == pt[5:first_bad * FS]
    got, err = stream_read(ctx, d, first_bad * FS + 3, 10, 7, 1, n=len(pt), key=key)
    assert got == b"" and err is not None and text in str(err)


def test_empty_object_and_ranges_past_the_end(ctx, small, tmp_path):
    d = str(tmp_path / "e.ec")
    ctx.put_object_chunked_encrypted(d, 101, 2, KEY, NONCE, AAD, b"")
    for n in (None, 0):
        assert stream_read(ctx, d, 0, None, 10, 0, n=n) == (b"", None)
    src, pt, _ = small
    for o in (len(pt), len(pt) + 5, 2 ** 64 - 2):
        assert stream_read(ctx, src, o, None, 10, 1, n=len(pt)) == (b"", None)
    assert stream_read(ctx, src, 2 ** 63, 2 ** 64 - 2, 10, 1, n=len(pt)) == (b"", None)


def test_open_errors_are_the_buffered_calls(ctx, small, tmp_path):
    src, pt, _ = small
    for kw in (dict(frame_size=0), dict(frame_size=24), dict(plaintext_size=None)):  # the manifest has no plaintext_size
        args = dict(plaintext_size=len(pt), frame_size=FS)
        args.update(kw)
        with pytest.raises(maxio_amd.RSError) as b:
            ctx.get_object_chunked_encrypted(src, KEY, AAD, 0, None, **args)
        with pytest.raises(maxio_amd.RSError) as s:
            ctx.open_reader_encrypted(src, KEY, AAD, 0, None, **args)
        assert (s.value.code, str(s.value)) == (b.value.code, str(b.value)), kw
    with pytest.raises(maxio_amd.RSError) as s:
        ctx.open_reader_encrypted(str(tmp_path / "none.ec"), KEY, AAD, plaintext_size=5)
    with pytest.raises(maxio_amd.RSError) as b:
        ctx.get_object_chunked_encrypted(str(tmp_path / "none.ec"), KEY, AAD, plaintext_size=5)
    assert s.value.code == b.value.code


def test_two_readers_from_two_threads(ctx, small):
    d, pt, _ = small
    got = {}

    def work(name, off, batch):
        got[name] = [stream_read(ctx, d, off, None, 97, batch, n=len(pt)) for _ in range(3)]

    ts = [threading.Thread(target=work, args=("a", 0, 1)), threading.Thread(target=work, args=("b", 33, 250))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got["a"] == [(pt, None)] * 3 and got["b"] == [(pt[33:], None)] * 3


def test_closed_mid_stream_and_as_a_context_manager(ctx, small):
    d, pt, _ = small
    r = ctx.open_reader_encrypted(d, KEY, AAD, plaintext_size=len(pt), frame_size=FS, batch_bytes=1)
    assert r.read(100) == pt[:100]
    r.close()  # frames pending, chunks resident: nothing left running
    r.close()
    with ctx.open_reader_encrypted(d, KEY, AAD, 10, 30, plaintext_size=len(pt), frame_size=FS) as r:
        assert r.read(1000) == pt[10:40]
        assert r.read(1000) == b""
    assert stream_read(ctx, d, 0, None, None, 0, n=len(pt)) == (pt, None)
