"""GPU: the streaming PUT, mxec_writer_open / _write / _finish / _close
(maxio_amd/csrc/storage_writer.cpp) through Context.open_writer.

After finish() the directory holds exactly the files and the manifest.json
text put_object_chunked (filesystem.rs:686-773) writes for the concatenated
body, however the body was split across write() calls.  The expected
directory is helpers.expected_ec_object: oracle parity, hashlib digests, the
serde_json::to_string_pretty layout."""
from __future__ import annotations

import functools
import os
import threading

import numpy as np
import pytest

import maxio_amd
from helpers import expected_ec_object
from maxio_amd import _native as N

pytestmark = pytest.mark.gpu

CHUNKS = (20000, 65536)  # 20 000 is not a multiple of 64
MS = (0, 2, 3)
E_255, E_ARG = -20, -21


def lengths(c):
    return (0, 1, c - 1, c, c + 1, 3 * c, 3 * c + 777)


@functools.lru_cache(maxsize=None)
def body_of(n, seed=0):
    return np.random.default_rng(4100 + seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def expected(n, c, m, plaintext_size=None, seed=0):
    return expected_ec_object(body_of(n, seed), c, m, plaintext_size)


def read_dir(d):
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


def assert_dir(d, n, c, m, plaintext_size=None, seed=0):
    files, manifest = expected(n, c, m, plaintext_size, seed)
    got = read_dir(d)
    assert sorted(got) == sorted(list(files) + ["manifest.json"])
    for name, want in files.items():
        assert got[name] == want, name
    assert got["manifest.json"].decode() == manifest


def schedule(kind, n, c):
    """The sizes of the write() calls of one body."""
    if kind == "one":
        return [n]
    if kind == "4099":
        return [min(4099, n - o) for o in range(0, n, 4099)]
    rng = np.random.default_rng(n * 31 + c)
    out, left = [], n
    while left:
        out.append(min(left, int(rng.integers(1, int(2.5 * c) + 1))))
        left -= out[-1]
    return out


def stream_in(w, body, sizes):
    at = 0
    for s in sizes:
        w.write(body[at:at + s])
        at += s
    assert at == len(body)


@pytest.mark.parametrize("kind", ("one", "4099", "random"))
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("c", CHUNKS)
def test_write_schedules_give_the_same_directory(ctx, tmp_path, c, m, kind):
    for n in lengths(c):
        d = str(tmp_path / ("o%d.ec" % n))
        with ctx.open_writer(d, c, m, n) as w:
            stream_in(w, body_of(n), schedule(kind, n, c))
        assert_dir(d, n, c, m)


def test_zero_length_writes_change_nothing(ctx, tmp_path):
    c, n, m = 20000, 3 * 20000 + 777, 2
    d = str(tmp_path / "o.ec")
    w = ctx.open_writer(d, c, m, n)
    body = body_of(n)
    w.write(b"")
    w.write(body[:c])
    w.write(b"")
    w.write(body[c:])
    w.write(b"")
    w.finish()
    w.finish()  # a second finish is a no-op
    w.close()
    assert_dir(d, n, c, m)


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("c", CHUNKS)
def test_window_reuse(ctx, tmp_path, c, m):
    """12 chunks (the last one short) through a window of two."""
    n = 11 * c + 5
    d = str(tmp_path / "o.ec")
    with ctx.open_writer(d, c, m, n, window_bytes=2 * c) as w:
        stream_in(w, body_of(n), schedule("random", n, c))
    assert_dir(d, n, c, m)


@pytest.mark.parametrize("m", (0, 2))
def test_plaintext_size_recorded(ctx, tmp_path, m):
    c, n = 20000, 3 * 20000 + 777
    d = str(tmp_path / "o.ec")
    with ctx.open_writer(d, c, m, n, plaintext_size=n - 28 * 2) as w:
        w.write(body_of(n))
    assert_dir(d, n, c, m, plaintext_size=n - 28 * 2)
    assert '"plaintext_size": %d' % (n - 56) in open(os.path.join(d, "manifest.json")).read()


@pytest.mark.parametrize("m", MS)
def test_round_trip(ctx, tmp_path, m):
    c, n = 65536, 3 * 65536 + 777
    d = str(tmp_path / "o.ec")
    with ctx.open_writer(d, c, m, n) as w:
        stream_in(w, body_of(n), schedule("4099", n, c))
    assert ctx.get_object_chunked(d) == body_of(n)


def _concurrent(c_, tmp_path):
    """Four writers on four threads, their writes interleaved by a barrier per round."""
    c, m = 20000, 2
    ns = [3 * c + 777, 5 * c, 2 * c + 1, 4 * c - 1]
    rounds = 8
    barrier = threading.Barrier(len(ns))
    errors = []

    def run(i):
        try:
            n, body = ns[i], body_of(ns[i], seed=i)
            step = (n + rounds - 1) // rounds
            w = c_.open_writer(str(tmp_path / ("t%d.ec" % i)), c, m, n, window_bytes=2 * c)
            for r in range(rounds):
                barrier.wait(timeout=60)
                w.write(body[r * step:(r + 1) * step])
            w.finish()
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
        assert_dir(str(tmp_path / ("t%d.ec" % i)), n, c, m, seed=i)


def test_concurrent_writers(ctx, tmp_path):
    _concurrent(ctx, tmp_path)


def test_concurrent_writers_on_two_logical_devices(ctx_with, tmp_path):
    _concurrent(ctx_with(MXEC_TEST_LOGICAL_DEVICES=2), tmp_path)


# ---- errors ---------------------------------------------------------------------------------------

def test_overrun_poisons_the_writer(ctx, tmp_path):
    c, n = 20000, 2 * 20000 + 5
    d = str(tmp_path / "o.ec")
    w = ctx.open_writer(d, c, 2, n)
    w.write(body_of(n)[:n - 3])
    with pytest.raises(maxio_amd.RSError) as e1:
        w.write(b"\0" * 4)  # one byte too many: refused whole
    assert e1.value.code == E_ARG
    with pytest.raises(maxio_amd.RSError) as e2:  # the writer repeats its error, even for a write that would fit
        w.write(b"\0" * 3)
    with pytest.raises(maxio_amd.RSError) as e3:
        w.finish()
    assert str(e2.value) == str(e1.value) == str(e3.value)
    w.close()
    assert not os.path.exists(os.path.join(d, "manifest.json"))


def test_short_finish_writes_no_manifest(ctx, tmp_path):
    c, n = 20000, 2 * 20000 + 5
    d = str(tmp_path / "o.ec")
    w = ctx.open_writer(d, c, 2, n)
    w.write(body_of(n)[:n - 1])
    with pytest.raises(maxio_amd.RSError) as e:
        w.finish()
    assert e.value.code == E_ARG
    assert "body ended at %d of %d declared bytes" % (n - 1, n) in str(e.value)
    with pytest.raises(maxio_amd.RSError) as e2:  # poisoned: the missing byte no longer helps
        w.write(body_of(n)[n - 1:])
    assert str(e2.value) == str(e.value)
    w.close()
    assert not os.path.exists(os.path.join(d, "manifest.json"))


def test_too_many_shards_fails_at_open_with_the_buffered_calls_text(ctx, tmp_path):
    c, n, m = 16, 256 * 16, 2  # 256 declared chunks
    d = str(tmp_path / "stream.ec")
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.open_writer(d, c, m, n)
    assert e.value.code == E_255
    assert not os.path.exists(d), "the directory must not be created"
    with pytest.raises(maxio_amd.RSError) as b:
        ctx.put_object_chunked(str(tmp_path / "buffered.ec"), c, m, bytes(n))
    assert str(b.value) == str(e.value)
    # 256 chunks without parity are fine (version 1)
    with ctx.open_writer(d, c, 0, n) as w:
        w.write(body_of(n))
    assert_dir(d, n, c, 0)


def test_argument_errors(ctx, tmp_path):
    import ctypes

    lib, d = N.lib(), str(tmp_path / "o.ec").encode()
    h = ctypes.c_void_p()
    none = (1 << 64) - 1
    assert lib.mxec_writer_open(ctx.handle, d, 0, 2, 100, none, 0, ctypes.byref(h)) == E_ARG  # chunk_size = 0
    assert not os.path.exists(d) and not h.value
    assert lib.mxec_writer_open(None, d, 16, 2, 100, none, 0, ctypes.byref(h)) == E_ARG
    assert lib.mxec_writer_open(ctx.handle, None, 16, 2, 100, none, 0, ctypes.byref(h)) == E_ARG
    assert lib.mxec_writer_open(ctx.handle, d, 16, 2, 100, none, 0, None) == E_ARG
    assert not os.path.exists(d)
    assert lib.mxec_writer_write(None, b"x", 1) == E_ARG
    assert lib.mxec_writer_finish(None) == E_ARG
    lib.mxec_writer_close(None)
    assert lib.mxec_writer_open(ctx.handle, d, 16, 2, 100, none, 0, ctypes.byref(h)) == 0
    assert lib.mxec_writer_write(h, None, 1) == E_ARG  # a null buffer is the call's error, not the writer's
    assert lib.mxec_writer_write(h, None, 0) == 0
    lib.mxec_writer_close(h)


def test_close_without_finish_leaves_no_manifest(ctx, tmp_path):
    c, n = 20000, 3 * 20000
    d = str(tmp_path / "o.ec")
    w = ctx.open_writer(d, c, 2, n)
    w.write(body_of(n))
    w.close()
    assert "manifest.json" not in os.listdir(d)
    with pytest.raises(RuntimeError):  # the context manager closes without finishing on an exception
        with ctx.open_writer(d, c, 2, n) as w2:
            w2.write(body_of(n))
            raise RuntimeError("handler failed")
    assert "manifest.json" not in os.listdir(d)
