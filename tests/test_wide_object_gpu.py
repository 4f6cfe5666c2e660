"""GPU: the file layer at k = 251 -- PUT, the streaming writer, GET, the
streaming reader, scrub, locate and the encrypted stream over one object of
251 data chunks and 4 parity shards, k + m = 255, the widest the reference
stores (filesystem.rs:1095).

Shape: chunk_size 4 099 (odd, no multiple of anything), a body of 250 * 4 099
+ 17 bytes, so the last data chunk is 17 bytes.  The expected directory is
helpers.expected_ec_object (oracle parity, hashlib digests, the
serde_json::to_string_pretty manifest); every body read back is compared with
the bytes that went in.  The device-resident passes at this width are
tests/test_wide_stripes_gpu.py's."""
from __future__ import annotations

import functools
import hashlib
import os
import shutil

import numpy as np
import pytest

import maxio_amd
import oracle
from helpers import expected_ec_object
from test_writer_gpu import read_dir, schedule, stream_in

pytestmark = pytest.mark.gpu

C, M, K = 4099, 4, 251
N = 250 * C + 17
WINDOW = 7 * C
KEY = bytes(range(11, 43))
PREFIX = bytes([0x77, 1, 2, 3])
AAD = oracle.object_aad_prefix("bkt", "wide/key", "v1")
FP = 65536
N_PT = N - 28 * 16  # 16 frames: the frame stream is N bytes, 251 chunks again
ONE, HEALED = 1, 2
WHICH = maxio_amd.SUM_MD5 | maxio_amd.SUM_SHA256


@functools.lru_cache(maxsize=None)
def body_of(n):
    return np.random.default_rng(251000 + n).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def expected(n=N):
    return expected_ec_object(body_of(n), C, M)


def assert_dir(d, want=None):
    files, manifest = want or expected()
    got = read_dir(d)
    assert sorted(got) == sorted(list(files) + ["manifest.json"])
    for name, b in files.items():
        assert got[name] == b, name
    assert got["manifest.json"].decode() == manifest


@pytest.fixture(scope="module")
def pristine(ctx, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("wide") / "o.ec")
    ctx.put_object_chunked(d, C, M, body_of(N))
    return d


@pytest.fixture()
def ec(pristine, tmp_path):
    d = str(tmp_path / "o.ec")
    shutil.copytree(pristine, d)
    return d


def name(i):
    return "%06d" % i


def flip(d, shard, at, bits=0x10):
    p = os.path.join(d, name(shard))
    b = bytearray(open(p, "rb").read())
    b[at] ^= bits
    open(p, "wb").write(bytes(b))


def drain(r, n=1 << 16):
    out = []
    while True:
        b = r.read(n)
        if not b:
            return b"".join(out)
        out.append(b)


# ---- the directory ----------------------------------------------------------------------------

def test_buffered_put_writes_the_expected_directory(pristine):
    files, _ = expected()
    assert len(files) == K + M and len(files[name(K - 1)]) == 17
    assert_dir(pristine)


@pytest.mark.parametrize("kind", ("4099", "random"))
def test_writer_through_a_window_of_seven_chunks(ctx, tmp_path, kind):
    """The seeded parity pass slides its window of 7 across all 251 columns;
    the digests are the buffered call's."""
    d = str(tmp_path / "o.ec")
    with ctx.open_writer(d, C, M, N, window_bytes=WINDOW, which=WHICH) as w:
        stream_in(w, body_of(N), schedule(kind, N, C))
        w.finish()
        sums = w.sums()
    assert_dir(d)
    assert sums == {"md5": hashlib.md5(body_of(N)).digest(), "sha256": hashlib.sha256(body_of(N)).digest()}
    buffered = ctx.put_object_chunked_sums(str(tmp_path / "b.ec"), C, M, body_of(N), "SHA256")
    assert maxio_amd.ec.put_result(sums, "SHA256") == buffered
    assert_dir(str(tmp_path / "b.ec"))


# ---- reads ------------------------------------------------------------------------------------

ACROSS_128 = (128 * C - 100, 300)  # the last 100 bytes of chunk 127, the first 200 of chunk 128


def read_every_way(ctx, d):
    body = body_of(N)
    assert ctx.get_object_chunked(d) == body
    off, ln = ACROSS_128
    assert ctx.get_object_chunked(d, off, ln) == body[off:off + ln]
    for batch in (0, 1):
        with ctx.open_reader(d, batch_bytes=batch) as r:
            assert drain(r) == body, batch
        with ctx.open_reader(d, off, ln, batch_bytes=batch) as r:
            assert drain(r, 77) == body[off:off + ln], batch


def test_reads_of_the_healthy_object(ctx, pristine):
    read_every_way(ctx, pristine)


# Four losses each, as many as m = 4 carries: the first chunk, both sides of
# 128 between them, the 17-byte chunk, a parity file; deleted, or corrupt in place.
DAMAGE = {"four-deleted": ((0, 128, K - 1, K + 1), ()),
          "three-deleted-one-corrupt": ((0, K - 1, K + M - 1), ((127, C - 1),))}


def damage(d, which):
    gone, bad = DAMAGE[which]
    for i in gone:
        os.remove(os.path.join(d, name(i)))
    for i, at in bad:
        flip(d, i, at)


@pytest.mark.parametrize("which", list(DAMAGE))
def test_reads_with_four_shards_lost(ctx, ec, which):
    damage(ec, which)
    read_every_way(ctx, ec)


@pytest.mark.parametrize("which", list(DAMAGE))
def test_a_fifth_loss_fails(ctx, ec, which):
    """test_storage_gpu.py test_too_many_failures, at 250 of 251."""
    damage(ec, which)
    flip(ec, 200, 5)
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.get_object_chunked(ec)
    assert e.value.name == "TooFewShardsPresent"
    assert "only 250 of 251 required shards available" in str(e.value)
    with ctx.open_reader(ec) as r:
        with pytest.raises(maxio_amd.RSError) as e:
            drain(r)
    assert e.value.name == "TooFewShardsPresent"


def test_try_reconstruct_data_chunk(ctx, ec):
    damage(ec, "four-deleted")
    files, _ = expected()
    for target in (0, 128, K - 1):
        assert ctx.try_reconstruct_data_chunk(ec, target) == files[name(target)], target


# ---- scrub and locate -------------------------------------------------------------------------

def test_scrub_heals_chunk_200(ctx, ec):
    flip(ec, 200, C - 1)
    r = ctx.scrub_object(ec, parity=True)
    assert r["parity_consistent"] == 0 and r["parity_first_bad"] == C - 1 and (r["k"], r["m"]) == (K, M)
    r = ctx.scrub_object(ec, heal=True)
    assert r["verdict"] == HEALED and r["n_damaged"] == 1 and r["n_healed"] == 1
    assert [i for i, s in enumerate(r["shard_state"]) if s] == [200]
    assert_dir(ec)


@pytest.mark.parametrize("shard", (200, K - 1, K + M - 1))
def test_locate_names_and_heals_the_shard(ctx, ec, shard):
    at = {200: 2049, K - 1: 16, K + M - 1: 0}[shard]
    flip(ec, shard, at)
    r = ctx.locate_object(ec, heal=True)
    assert r == {"k": K, "m": M, "outcome": ONE, "shard": shard, "first_bad": at, "n_bad": 1, "healed": 1}
    assert_dir(ec)


# ---- the encrypted stream ---------------------------------------------------------------------

def test_encrypted_round_trip(ctx, tmp_path):
    """16 frames of 64 KiB + 28 cut across 251 chunks by the writer, put back
    together by the reader, with and without a chunk to rebuild."""
    pt = body_of(N_PT)
    aads = [oracle.frame_aad(AAD, i) for i in range((N_PT + FP - 1) // FP)]
    stream = oracle.frames_encrypt(KEY, PREFIX, pt, aads=aads)
    assert len(stream) == N
    d = str(tmp_path / "e.ec")
    with ctx.open_writer_encrypted(d, C, M, N_PT, KEY, PREFIX, AAD, window_bytes=WINDOW) as w:
        stream_in(w, pt, schedule("random", N_PT, C))
    assert_dir(d, expected_ec_object(stream, C, M, plaintext_size=N_PT))
    for lost in ((), (128, K - 1)):
        for i in lost:
            os.remove(os.path.join(d, name(i)))
        for batch in (0, 1):
            with ctx.open_reader_encrypted(d, KEY, AAD, batch_bytes=batch) as r:
                assert drain(r) == pt, (lost, batch)
        off = 7 * FP - 5  # across a frame edge and chunks 111 / 112
        with ctx.open_reader_encrypted(d, KEY, AAD, off, 4200) as r:
            assert drain(r, 1000) == pt[off:off + 4200]


# ---- the 255 boundary -------------------------------------------------------------------------

def test_one_more_chunk_is_refused(ctx, tmp_path):
    """k + m = 255 is accepted by every PUT form above; 252 + 4 by none, with
    the reference's text.  The writers know at open and create nothing.  The
    buffered call writes the data chunks first and meets the guard at the
    parity, as the reference does (filesystem.rs:1095 inside
    compute_and_write_parity): no manifest and no parity file, so no object."""
    n = N + C
    body = body_of(n)
    assert (n + C - 1) // C == 252
    errors = []
    for form in ("writer", "writer-encrypted", "buffered", "buffered-sums"):
        d = str(tmp_path / (form + ".ec"))
        with pytest.raises(maxio_amd.RSError) as e:
            if form == "writer":
                ctx.open_writer(d, C, M, n, window_bytes=WINDOW)
            elif form == "writer-encrypted":
                ctx.open_writer_encrypted(d, C, M, N_PT + C, KEY, PREFIX, AAD)
            elif form == "buffered":
                ctx.put_object_chunked(d, C, M, body)
            else:
                ctx.put_object_chunked_sums(d, C, M, body, "SHA256")
        assert e.value.name == "TooManyShards255", form
        assert "252 data + 4 parity = 256 > 255" in str(e.value) and "Increase --chunk-size" in str(e.value)
        errors.append(str(e.value))
        if form.startswith("writer"):
            assert not os.path.exists(d), form
        else:
            assert sorted(os.listdir(d)) == [name(j) for j in range(252)], form
    assert len(set(errors)) == 1
