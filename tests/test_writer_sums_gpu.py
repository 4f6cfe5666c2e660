"""GPU: the streaming PUT's own body digests, mxec_writer_open_sums /
mxec_writer_sums (maxio_amd/csrc/storage_writer.cpp) through
Context.open_writer(which=...) and ChunkWriter.sums().

The directory is what tests/test_writer_gpu.py expects of a writer without
digests (helpers.expected_ec_object); sums() is hashlib's MD5 / SHA-1 /
SHA-256, zlib's CRC32 and the oracle's CRC32C of the concatenated body,
however it was split across write() calls and digest runs.

Replaces: the Md5 / ChecksumHasher of put_object_chunked's loop
(filesystem.rs:700-725) and PutResult.etag / checksum_value (:775-777)."""
from __future__ import annotations

import hashlib
import os
import threading
import zlib

import pytest

import maxio_amd
import oracle
from test_writer_gpu import assert_dir, body_of, schedule, stream_in

pytestmark = pytest.mark.gpu

ALL = 0x1F
E_ARG = -21
MIB = 1 << 20


def want(body: bytes, which: int = ALL) -> dict:
    d = {}
    if which & maxio_amd.SUM_MD5:
        d["md5"] = hashlib.md5(body).digest()
    if which & maxio_amd.SUM_CRC32:
        d["crc32"] = zlib.crc32(body)
    if which & maxio_amd.SUM_CRC32C:
        d["crc32c"] = oracle.crc32c(body)
    if which & maxio_amd.SUM_SHA1:
        d["sha1"] = hashlib.sha1(body).digest()
    if which & maxio_amd.SUM_SHA256:
        d["sha256"] = hashlib.sha256(body).digest()
    return d


@pytest.mark.parametrize("kind", ("one", "4099", "random"))
@pytest.mark.parametrize("m", (0, 2))
@pytest.mark.parametrize("c", (20000, 65536))
def test_schedules_give_the_directory_and_the_bodys_sums(ctx, tmp_path, c, m, kind):
    for n in (0, 1, c - 1, c, c + 1, 3 * c + 777):
        d = str(tmp_path / ("o%d.ec" % n))
        with ctx.open_writer(d, c, m, n, which=ALL) as w:
            stream_in(w, body_of(n), schedule(kind, n, c))
            w.finish()
            got = w.sums()
        assert_dir(d, n, c, m)
        assert got == want(body_of(n)), n


def test_a_chunk_that_crosses_the_run_cut(ctx, tmp_path):
    """Chunks of 2 MiB + 20: three digest runs each, the last of 20 bytes,
    through a window of two chunks (the third chunk reuses the first's slot)."""
    c, m = 2 * MIB + 20, 2
    n = 2 * c + 777
    d = str(tmp_path / "o.ec")
    with ctx.open_writer(d, c, m, n, window_bytes=2 * c, which=ALL) as w:
        stream_in(w, body_of(n), schedule("random", n, c))
        w.finish()
        got = w.sums()
    assert_dir(d, n, c, m)
    assert got == want(body_of(n))


@pytest.mark.parametrize("which", [maxio_amd.SUM_MD5, maxio_amd.SUM_CRC32C, maxio_amd.SUM_CRC32 | maxio_amd.SUM_SHA1,
                                   maxio_amd.SUM_MD5 | maxio_amd.SUM_SHA256])
def test_which_subsets(ctx, tmp_path, which):
    import ctypes

    from maxio_amd import _native as N

    c, n = 20000, 3 * 20000 + 777
    d = str(tmp_path / "o.ec")
    with ctx.open_writer(d, c, 2, n, which=which) as w:
        stream_in(w, body_of(n), schedule("4099", n, c))
        w.finish()
        assert w.sums() == want(body_of(n), which)
        # the fields not asked for are left as they were
        r = N.BodySums()
        ctypes.memset(ctypes.byref(r), 0xAA, ctypes.sizeof(r))
        assert N.lib().mxec_writer_sums(w._w, ctypes.byref(r)) == 0
        raw = bytes(r)
        for flag, lo, hi in [(1, 0, 16), (2, 16, 20), (4, 20, 24), (8, 24, 44), (16, 44, 76)]:
            if not which & flag:
                assert raw[lo:hi] == b"\xAA" * (hi - lo), flag
    assert_dir(d, n, c, 2)


def test_which_zero_is_the_plain_writer(ctx, tmp_path):
    import ctypes

    from maxio_amd import _native as N

    c, n = 20000, 2 * 20000 + 5
    d = str(tmp_path / "o.ec")
    with ctx.open_writer(d, c, 2, n, which=0) as w:
        assert w.sums() == {}  # even before finish: nothing was asked for
        w.write(body_of(n))
        w.finish()
        assert w.sums() == {}
        r = N.BodySums()
        ctypes.memset(ctypes.byref(r), 0xAA, ctypes.sizeof(r))
        assert N.lib().mxec_writer_sums(w._w, ctypes.byref(r)) == 0
        assert bytes(r) == b"\xAA" * 76
    assert_dir(d, n, c, 2)
    h = ctypes.c_void_p()
    assert N.lib().mxec_writer_open_sums(ctx.handle, d.encode(), c, 2, n, (1 << 64) - 1, 0, 0x20, ctypes.byref(h)) == E_ARG
    assert not h.value
    assert N.lib().mxec_writer_sums(None, None) == E_ARG


def test_sums_before_finish(ctx, tmp_path):
    c, n = 20000, 2 * 20000 + 5
    w = ctx.open_writer(str(tmp_path / "o.ec"), c, 2, n, which=ALL)
    with pytest.raises(maxio_amd.RSError) as e:
        w.sums()
    assert e.value.code == E_ARG and "sums before finish" in str(e.value)
    w.write(body_of(n))
    with pytest.raises(maxio_amd.RSError) as e:  # every byte written is still not a finish
        w.sums()
    assert "sums before finish" in str(e.value)
    w.finish()
    assert w.sums() == want(body_of(n))
    assert w.sums() == want(body_of(n))  # and again
    w.close()


def test_sums_after_a_short_finish_is_the_poisoning_error(ctx, tmp_path):
    c, n = 20000, 2 * 20000 + 5
    d = str(tmp_path / "o.ec")
    w = ctx.open_writer(d, c, 2, n, which=ALL)
    w.write(body_of(n)[:n - 1])
    with pytest.raises(maxio_amd.RSError) as e:
        w.finish()
    assert "body ended at %d of %d declared bytes" % (n - 1, n) in str(e.value)
    with pytest.raises(maxio_amd.RSError) as e2:
        w.sums()
    assert e2.value.code == e.value.code == E_ARG and str(e2.value) == str(e.value)
    w.close()
    assert not os.path.exists(os.path.join(d, "manifest.json"))


def test_frame_stream_digests_are_of_the_bytes_written(ctx, tmp_path):
    c, n = 20000, 3 * 20000 + 777
    d = str(tmp_path / "o.ec")
    with ctx.open_writer(d, c, 2, n, plaintext_size=n - 56, which=maxio_amd.SUM_MD5) as w:
        w.write(body_of(n))
        w.finish()
        assert w.sums() == want(body_of(n), maxio_amd.SUM_MD5)
    assert_dir(d, n, c, 2, plaintext_size=n - 56)


def test_two_writers_on_two_threads_keep_their_own_sums(ctx, tmp_path):
    c, m = 20000, 2
    ns = [3 * c + 777, 5 * c + 1]
    rounds = 8
    barrier = threading.Barrier(len(ns))
    errors, got = [], {}

    def run(i):
        try:
            n, body = ns[i], body_of(ns[i], seed=i + 1)
            step = (n + rounds - 1) // rounds
            w = ctx.open_writer(str(tmp_path / ("t%d.ec" % i)), c, m, n, window_bytes=2 * c, which=ALL)
            for r in range(rounds):
                barrier.wait(timeout=60)
                w.write(body[r * step:(r + 1) * step])
            w.finish()
            got[i] = w.sums()
            w.close()
        except Exception as e:  # noqa: BLE001
            errors.append((i, repr(e)))
            barrier.abort()

    ts = [threading.Thread(target=run, args=(i,)) for i in range(len(ns))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i, n in enumerate(ns):
        assert_dir(str(tmp_path / ("t%d.ec" % i)), n, c, m, seed=i + 1)
        assert got[i] == want(body_of(n, seed=i + 1)), i
    assert got[0] != got[1]
