"""GPU: the streaming encrypted PUT, mxec_writer_open_encrypted
(maxio_amd/csrc/storage_writer.cpp) through Context.open_writer_encrypted.

The caller writes plaintext; after finish() the directory holds exactly the
files and the manifest.json text put_object_chunked_encrypted
(filesystem.rs:835-1060) writes for the concatenated body, however it was
split.  The expected directory is helpers.expected_ec_object over the oracle's
frame stream (oracle.frames_encrypt, AADs from hashlib)."""
from __future__ import annotations

import functools
import hashlib
import os
import threading
import zlib

import numpy as np
import pytest

import maxio_amd
import oracle
from helpers import expected_ec_object
from test_writer_gpu import body_of, read_dir, schedule, stream_in

pytestmark = pytest.mark.gpu

E_255, E_ARG = -20, -21
FP = 65536
KEY = bytes(range(7, 39))
PREFIX = bytes([0x90, 1, 2, 3])
AAD = b"bucket\0some/key\0v1\0"
N4 = 3 * FP + 777


def aads_of(n, aad=AAD):
    return [hashlib.sha256(aad + i.to_bytes(8, "little")).digest() for i in range((n + FP - 1) // FP)] or None


@functools.lru_cache(maxsize=None)
def stream_of(n, seed=0, key=KEY, prefix=PREFIX, aad=AAD):
    return oracle.frames_encrypt(key, prefix, body_of(n, seed), aads=aads_of(n, aad)) if n else b""


@functools.lru_cache(maxsize=None)
def expected(n, c, m, seed=0, key=KEY, prefix=PREFIX, aad=AAD):
    return expected_ec_object(stream_of(n, seed, key, prefix, aad), c, m, plaintext_size=n)


def assert_dir(d, n, c, m, **kw):
    files, manifest = expected(n, c, m, **kw)
    got = read_dir(d)
    assert sorted(got) == sorted(list(files) + ["manifest.json"])
    for name, want in files.items():
        assert got[name] == want, name
    assert got["manifest.json"].decode() == manifest


def put(ctx, d, c, m, n, kind="one", seed=0, **kw):
    with ctx.open_writer_encrypted(d, c, m, n, KEY, PREFIX, AAD, **kw) as w:
        stream_in(w, body_of(n, seed), schedule(kind, n, c))
        return w


@pytest.mark.parametrize("kind", ("one", "4099", "random"))
@pytest.mark.parametrize("m", (0, 2))
@pytest.mark.parametrize("c", (20000, 65563, 65564, 65565, 100000))
def test_write_schedules_give_the_same_directory(ctx, tmp_path, c, m, kind):
    for n in (0, 1, FP - 1, FP, FP + 1, N4):
        d = str(tmp_path / ("o%d.ec" % n))
        put(ctx, d, c, m, n, kind)
        assert_dir(d, n, c, m)


def test_same_files_as_the_buffered_call(ctx, tmp_path):
    c, m, n = 65565, 2, N4
    a, b = str(tmp_path / "stream.ec"), str(tmp_path / "buffered.ec")
    put(ctx, a, c, m, n, "random")
    ctx.put_object_chunked_encrypted(b, c, m, KEY, PREFIX, AAD, body_of(n))
    assert read_dir(a) == read_dir(b)


def test_plaintext_digests(ctx, tmp_path):
    n, body = N4, body_of(N4)
    with ctx.open_writer_encrypted(str(tmp_path / "a.ec"), 100000, 2, n, KEY, PREFIX, AAD, which=0x1F) as w:
        stream_in(w, body, schedule("4099", n, 100000))
        w.finish()
        s = w.sums()
    assert s["md5"] == hashlib.md5(body).digest() and s["sha1"] == hashlib.sha1(body).digest()
    assert s["sha256"] == hashlib.sha256(body).digest()
    assert s["crc32"] == zlib.crc32(body) and s["crc32c"] == oracle.crc32c(body)
    # a subset leaves the other fields of the caller's record untouched
    from maxio_amd import _native as N
    import ctypes

    with ctx.open_writer_encrypted(str(tmp_path / "b.ec"), 100000, 0, n, KEY, PREFIX, AAD, which=0x05) as w:
        w.write(body)
        w.finish()
        r = N.BodySums()
        ctypes.memset(ctypes.byref(r), 0xEE, ctypes.sizeof(r))
        assert maxio_amd.lib().mxec_writer_sums(w._w, ctypes.byref(r)) == 0
    assert bytes(r.md5) == hashlib.md5(body).digest() and r.crc32c == oracle.crc32c(body)
    assert r.crc32 == 0xEEEEEEEE and bytes(r.sha1) == b"\xEE" * 20 and bytes(r.sha256) == b"\xEE" * 32
    # an empty body has digests too
    with ctx.open_writer_encrypted(str(tmp_path / "c.ec"), 100000, 2, 0, KEY, PREFIX, AAD, which=0x1F) as w:
        w.finish()
        assert w.sums()["md5"] == hashlib.md5(b"").digest()


@pytest.mark.parametrize("c,n", ((20000, N4), ((1 << 20) + 20, (2 << 20) + 5)))
def test_window_of_two_chunks_with_reuse(ctx, tmp_path, c, n):
    """Small chunks: the window grows to what one launch touches and is still
    reused.  Chunks of 1 MiB + 20: two slots, a 16-frame launch, ciphertext
    pieces cut at 1 MiB and file writes a piece behind."""
    d = str(tmp_path / "o.ec")
    put(ctx, d, c, 2, n, "random", window_bytes=2 * c)
    assert_dir(d, n, c, 2)


def test_round_trip_and_recovery(ctx, tmp_path):
    c, m, n = 65565, 2, N4
    d = str(tmp_path / "o.ec")
    put(ctx, d, c, m, n, "4099")
    assert ctx.get_object_chunked_encrypted(d, KEY, AAD, plaintext_size=n) == body_of(n)
    os.remove(os.path.join(d, "000001"))
    assert ctx.get_object_chunked_encrypted(d, KEY, AAD, plaintext_size=n) == body_of(n)


def test_two_writers_at_once(ctx, tmp_path):
    c, m, ns = 20000, 2, (N4, 2 * FP + 1)
    keys = (KEY, bytes(range(100, 132)))
    prefixes = (PREFIX, bytes([0xA0, 9, 8, 7]))
    barrier, errors = threading.Barrier(2), []

    def run(i):
        try:
            n, body = ns[i], body_of(ns[i], seed=i)
            w = ctx.open_writer_encrypted(str(tmp_path / ("t%d.ec" % i)), c, m, n, keys[i], prefixes[i], AAD)
            step = (n + 7) // 8
            for r in range(8):
                barrier.wait(timeout=60)
                w.write(body[r * step:(r + 1) * step])
            w.finish()
            w.close()
        except Exception as e:  # noqa: BLE001
            errors.append((i, repr(e)))
            barrier.abort()

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(2):
        assert_dir(str(tmp_path / ("t%d.ec" % i)), ns[i], c, m, seed=i, key=keys[i], prefix=prefixes[i])


# ---- errors ---------------------------------------------------------------------------------------

def test_overrun_short_finish_and_poison(ctx, tmp_path):
    c, n = 20000, FP + 5
    d = str(tmp_path / "o.ec")
    w = ctx.open_writer_encrypted(d, c, 2, n, KEY, PREFIX, AAD, which=0x01)
    w.write(body_of(n)[:n - 3])
    with pytest.raises(maxio_amd.RSError) as e0:
        w.sums()
    assert e0.value.code == E_ARG and "sums before finish" in str(e0.value)
    with pytest.raises(maxio_amd.RSError) as e1:
        w.write(b"\0" * 4)  # one byte too many, counted in plaintext bytes
    assert e1.value.code == E_ARG
    assert "write of 4 bytes at %d runs past the %d declared bytes" % (n - 3, n) in str(e1.value)
    with pytest.raises(maxio_amd.RSError) as e2:  # poisoned: a write that would fit repeats the error
        w.write(b"\0" * 3)
    with pytest.raises(maxio_amd.RSError) as e3:
        w.finish()
    assert str(e2.value) == str(e1.value) == str(e3.value)
    w.close()
    assert not os.path.exists(os.path.join(d, "manifest.json"))
    d2 = str(tmp_path / "short.ec")
    w = ctx.open_writer_encrypted(d2, c, 2, n, KEY, PREFIX, AAD)
    w.write(body_of(n)[:n - 1])
    with pytest.raises(maxio_amd.RSError) as e:
        w.finish()
    assert e.value.code == E_ARG and "body ended at %d of %d declared bytes" % (n - 1, n) in str(e.value)
    w.close()
    assert not os.path.exists(os.path.join(d2, "manifest.json"))


def test_close_without_finish_leaves_no_manifest(ctx, tmp_path):
    d = str(tmp_path / "o.ec")
    w = ctx.open_writer_encrypted(d, 20000, 2, N4, KEY, PREFIX, AAD)
    w.write(body_of(N4))
    w.close()
    assert "manifest.json" not in os.listdir(d)


def test_open_errors_create_nothing(ctx, tmp_path):
    d = str(tmp_path / "o.ec")
    with pytest.raises(maxio_amd.RSError) as e:  # 256 chunks of the frame stream
        ctx.open_writer_encrypted(d, 16, 2, 256 * 16 - 28, KEY, PREFIX, AAD)
    assert e.value.code == E_255 and not os.path.exists(d)
    for key, prefix in ((None, PREFIX), (KEY, None)):
        with pytest.raises(maxio_amd.RSError) as e:
            ctx.open_writer_encrypted(d, 20000, 2, 100, key, prefix, AAD)
        assert e.value.code == E_ARG and not os.path.exists(d)
    import ctypes

    h = ctypes.c_void_p()
    k = (ctypes.c_uint8 * 32)()
    assert maxio_amd.lib().mxec_writer_open_encrypted(ctx.handle, d.encode(), 20000, 2, 100, k, k, None, 5, 0, 0,
                                                      ctypes.byref(h)) == E_ARG  # aad_prefix_len without aad_prefix
    assert not h.value and not os.path.exists(d)
