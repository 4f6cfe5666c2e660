"""GPU: CompleteMultipartUpload as a stream -- mxec_complete_multipart_streamed
and mxec_complete_multipart_streamed_encrypted -- through the C ABI, checked
file by file and byte for byte against the layout the reference writes
(oracle frames / parity, hashlib digests, to_string_pretty manifest) and
against the buffered drivers' directories for the same arguments; the ETags;
a streaming GET, degraded too; and the buffered drivers' errors.

Replaces: complete_multipart_chunked (filesystem.rs:1147-1310) and
complete_multipart_chunked_encrypted (:1315-1560), which stream."""
from __future__ import annotations

import hashlib
import os
import threading

import numpy as np
import pytest

import maxio_amd
import oracle
from helpers import expected_ec_object

pytestmark = pytest.mark.gpu

FS = oracle.FRAME_CHUNK_SIZE
FL = FS + 28
MIB = 1 << 20
UPLOAD_ID = "upl-7f3a"
IDP = oracle.object_aad_prefix("b", "k", None)


def _rand(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


UPLOAD_KEY, KEY, PREFIX = _rand(32, 1), _rand(32, 2), b"NPFX"


def _check_dir(ec: str, files: dict, manifest: str):
    assert sorted(os.listdir(ec)) == sorted(list(files) + ["manifest.json"])
    assert open(os.path.join(ec, "manifest.json")).read() == manifest
    for name, want in files.items():
        assert open(os.path.join(ec, name), "rb").read() == want, name


def _same_dirs(a: str, b: str):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for name in os.listdir(a):
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name


def _aads(prefix: bytes, n: int):
    return [oracle.frame_aad(prefix, i) for i in range(n)]


def _part_frames(body: bytes, part_number: int, upload_key=UPLOAD_KEY, upload_id=UPLOAD_ID) -> bytes:
    """The part as upload_part stored it under SSE: frames under the upload key, part AADs (:147-163)."""
    prefix = b"PART\0" + upload_id.encode() + b"\0" + part_number.to_bytes(4, "little") + b"\0"
    n = (len(body) + FS - 1) // FS
    return oracle.frames_encrypt(upload_key, b"UPLD", body, _aads(prefix, n) or None) if n else b""


def _write_parts(tmp_path, spec, seed, upload_key=UPLOAD_KEY, tag=""):
    """spec: (size, encrypted) per part.  Returns (parts, bodies)."""
    parts, bodies = [], []
    for i, (sz, enc) in enumerate(spec):
        b = _rand(sz, seed + i)
        p = tmp_path / f"part{tag}{i + 1}"
        p.write_bytes(_part_frames(b, i + 1, upload_key) if enc else b)
        parts.append({"path": str(p), "size": sz, "etag": hashlib.md5(b).hexdigest(), "part_number": i + 1,
                      "encrypted": bool(enc)})
        bodies.append(b)
    return parts, bodies


def _etag(parts):
    return '"' + hashlib.md5(b"".join(bytes.fromhex(p["etag"]) for p in parts)).hexdigest() + "-%d" % len(parts) + '"'


# ---- the plain driver -------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes,chunk,m,window", [([70000, 1], 65536, 4, 0), ([0], 4096, 2, 0), ([300, 200], 1000, 0, 0),
                                                  ([MIB + 3, 2 * MIB, 5], MIB, 2, 2 * MIB), ([], 4096, 2, 0)])
def test_streamed_plain_layout_and_etag(ctx, tmp_path, sizes, chunk, m, window):
    parts, bodies = _write_parts(tmp_path, [(s, False) for s in sizes], 50)
    ec = str(tmp_path / "mp.ec")
    etag = ctx.complete_multipart_streamed(ec, chunk, m, parts, window_bytes=window)
    whole = b"".join(bodies)
    files, man = expected_ec_object(whole, chunk, m)
    _check_dir(ec, files, man)
    assert etag == _etag(parts)
    assert ctx.get_object_chunked(ec, capacity=max(1, len(whole))) == whole
    ref = str(tmp_path / "buffered.ec")
    assert ctx.complete_multipart_chunked(ref, chunk, m, parts) == etag
    _same_dirs(ec, ref)


def test_plain_part_size_is_the_files(ctx, tmp_path):
    """part.size is ignored for a plain part, as in the reference and the buffered driver."""
    parts, bodies = _write_parts(tmp_path, [(5000, False), (70, False)], 60)
    parts[0]["size"] = 17
    ec = str(tmp_path / "mp.ec")
    ctx.complete_multipart_streamed(ec, 4096, 2, parts)
    files, man = expected_ec_object(b"".join(bodies), 4096, 2)
    _check_dir(ec, files, man)


# ---- the encrypted driver ---------------------------------------------------------------------------

def _read_back(ctx, ec, plain, m):
    def read_all():
        got = []
        with ctx.open_reader_encrypted(ec, KEY, IDP) as r:
            while True:
                b = r.read(MIB)
                if not b:
                    return b"".join(got)
                got.append(b)

    assert read_all() == plain
    if m and plain:
        os.unlink(os.path.join(ec, "000000"))
        assert read_all() == plain


ENC_CASES = {
    "the buffered test's shape": ([(3 * FS + 1000, True), (40000, False)], MIB, 2),
    "frames misaligned to parts": ([(FS + 5, True), (1, True), (2 * FS, True), (0, True), (FS - 1, True)], 65565, 2),
    "plain, encrypted, plain": ([(100000, False), (100000, True), (100000, False)], 65536, 2),
    "encrypted, plain, encrypted": ([(100000, True), (100000, False), (100000, True)], 100000, 3),
    "the ring's wrap inside a part frame": ([(4 * MIB - 100, True), (FS + 300, True)], MIB + 20, 2),
    "all parts plain": ([(70000, False), (1, False), (FS, False)], 65536, 2),
    "120 tiny parts, 16 to a launch": ([(1 + i % 3, i % 4 != 3) for i in range(120)], 4096, 2),
    "an empty upload": ([], 4096, 2),
    "one empty encrypted part": ([(0, True)], 4096, 2),
}


@pytest.mark.parametrize("what", sorted(ENC_CASES))
def test_streamed_encrypted_layout_and_round_trip(ctx, tmp_path, what):
    spec, chunk, m = ENC_CASES[what]
    parts, bodies = _write_parts(tmp_path, spec, 70)
    ec = str(tmp_path / "mpe.ec")
    etag = ctx.complete_multipart_streamed_encrypted(ec, chunk, m, parts, UPLOAD_KEY, UPLOAD_ID, KEY, PREFIX, IDP)
    plain = b"".join(bodies)
    nfr = (len(plain) + FS - 1) // FS
    ct = oracle.frames_encrypt(KEY, PREFIX, plain, _aads(IDP, nfr) or None) if nfr else b""
    files, man = expected_ec_object(ct, chunk, m, plaintext_size=len(plain))
    _check_dir(ec, files, man)
    assert etag == _etag(parts)
    if not plain:
        assert sorted(os.listdir(ec)) == ["000000", "manifest.json"] and '"plaintext_size": 0' in man
    ref = str(tmp_path / "buffered.ec")
    assert ctx.complete_multipart_chunked_encrypted(ref, chunk, m, parts, UPLOAD_KEY, UPLOAD_ID, KEY, PREFIX, IDP) == etag
    _same_dirs(ec, ref)
    _read_back(ctx, ec, plain, m)


def test_trailing_bytes_of_an_encrypted_part_are_ignored(ctx, tmp_path):
    parts, bodies = _write_parts(tmp_path, [(FS + 77, True), (30, False)], 80)
    with open(parts[0]["path"], "ab") as f:
        f.write(b"trailing")
    ec = str(tmp_path / "mpe.ec")
    ctx.complete_multipart_streamed_encrypted(ec, 50000, 2, parts, UPLOAD_KEY, UPLOAD_ID, KEY, PREFIX, IDP)
    plain = b"".join(bodies)
    ct = oracle.frames_encrypt(KEY, PREFIX, plain, _aads(IDP, 2))
    _check_dir(ec, *expected_ec_object(ct, 50000, 2, plaintext_size=len(plain)))


# ---- failures: the buffered driver's code and text -----------------------------------------------------

def _both_fail(ctx, tmp_path, parts, upload_key=UPLOAD_KEY, upload_id=UPLOAD_ID, chunk=65536):
    """The streamed and the buffered call over the same arguments; returns the two errors."""
    errs = []
    for name, call in (("s", ctx.complete_multipart_streamed_encrypted), ("b", ctx.complete_multipart_chunked_encrypted)):
        with pytest.raises(maxio_amd.RSError) as e:
            call(str(tmp_path / f"fail_{name}.ec"), chunk, 2, parts, upload_key, upload_id, KEY, PREFIX, IDP)
        errs.append(e.value)
    assert errs[0].code == errs[1].code and str(errs[0]) == str(errs[1]), (str(errs[0]), str(errs[1]))
    return errs[0]


def test_a_flipped_bit_in_a_part_frame(ctx, tmp_path):
    """The second frame of the second encrypted part: an authentication error, and no manifest."""
    parts, _ = _write_parts(tmp_path, [(2 * FS, True), (2 * FS + 9, True)], 90)
    raw = bytearray(open(parts[1]["path"], "rb").read())
    raw[FL + 12 + 1000] ^= 4
    open(parts[1]["path"], "wb").write(bytes(raw))
    e = _both_fail(ctx, tmp_path, parts)
    assert e.code == -41 and "authentication" in str(e)
    assert not os.path.exists(tmp_path / "fail_s.ec" / "manifest.json")


def test_two_stored_frames_swapped(ctx, tmp_path):
    parts, _ = _write_parts(tmp_path, [(5000, False), (3 * FS, True)], 91)
    raw = open(parts[1]["path"], "rb").read()
    open(parts[1]["path"], "wb").write(raw[FL:2 * FL] + raw[:FL] + raw[2 * FL:])
    e = _both_fail(ctx, tmp_path, parts)
    assert e.code == -41 and "frame index mismatch: expected 0, got 1" in str(e)
    assert not os.path.exists(tmp_path / "fail_s.ec" / "manifest.json")


def test_a_part_under_another_part_number(ctx, tmp_path):
    parts, _ = _write_parts(tmp_path, [(FS + 1, True), (1000, True)], 92)
    parts[1]["part_number"] = 7
    e = _both_fail(ctx, tmp_path, parts)
    assert e.code == -41 and "authentication" in str(e)


def test_a_truncated_encrypted_part(ctx, tmp_path):
    parts, _ = _write_parts(tmp_path, [(1000, False), (FS + 5, True)], 93)
    raw = open(parts[1]["path"], "rb").read()
    open(parts[1]["path"], "wb").write(raw[:-1])
    e = _both_fail(ctx, tmp_path, parts)
    assert e.code == -41 and "truncated encrypted frame" in str(e)
    assert not os.path.exists(tmp_path / "fail_s.ec")


def test_a_missing_part_file(ctx, tmp_path):
    parts, _ = _write_parts(tmp_path, [(1000, False), (2000, True)], 94)
    parts.append({"path": str(tmp_path / "nope"), "size": 5, "etag": "00" * 16, "part_number": 3})
    e = _both_fail(ctx, tmp_path, parts)
    assert e.code == -40 and e.name == "Io"
    assert not os.path.exists(tmp_path / "fail_s.ec")
    plain = [dict(p, encrypted=False) for p in parts]
    with pytest.raises(maxio_amd.RSError) as s:
        ctx.complete_multipart_streamed(str(tmp_path / "a.ec"), 4096, 2, plain)
    with pytest.raises(maxio_amd.RSError) as b:
        ctx.complete_multipart_chunked(str(tmp_path / "b.ec"), 4096, 2, plain)
    assert s.value.code == -40 and str(s.value) == str(b.value)
    assert not os.path.exists(tmp_path / "a.ec")


def test_an_encrypted_part_without_the_upload_key(ctx, tmp_path):
    parts, _ = _write_parts(tmp_path, [(1000, True)], 95)
    with pytest.raises(maxio_amd.RSError) as s:
        ctx.complete_multipart_streamed_encrypted(str(tmp_path / "a.ec"), 4096, 2, parts, None, None, KEY, PREFIX, IDP)
    assert s.value.code == -21 and "encrypted part without upload key" in str(s.value)
    lib = maxio_amd.lib()
    import ctypes

    etag = ctypes.create_string_buffer(48)
    k = np.frombuffer(KEY, np.uint8)
    pre = np.frombuffer(PREFIX, np.uint8)
    rc = lib.mxec_complete_multipart_chunked_encrypted(ctx.handle, str(tmp_path / "b.ec").encode(), 4096, 2,
                                                       ctx._parts(parts), 1, None, None, k.ctypes.data, pre.ctypes.data,
                                                       None, 0, etag)
    assert rc == -21 and lib.mxec_last_error().decode() in str(s.value)
    assert not os.path.exists(tmp_path / "a.ec")


def test_an_encrypted_part_given_to_the_plain_driver(ctx, tmp_path):
    parts, _ = _write_parts(tmp_path, [(1000, False), (1000, True)], 96)
    with pytest.raises(maxio_amd.RSError) as s:
        ctx.complete_multipart_streamed(str(tmp_path / "a.ec"), 4096, 2, parts)
    with pytest.raises(maxio_amd.RSError) as b:
        ctx.complete_multipart_chunked(str(tmp_path / "b.ec"), 4096, 2, parts)
    assert s.value.code == -21 and str(s.value) == str(b.value)
    assert not os.path.exists(tmp_path / "a.ec")


def test_the_writers_open_errors_apply(ctx, tmp_path):
    parts, _ = _write_parts(tmp_path, [(3000, False)], 97)
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.complete_multipart_streamed(str(tmp_path / "a.ec"), 0, 2, parts)
    assert e.value.code == -21 and "chunk_size" in str(e.value)
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.complete_multipart_streamed_encrypted(str(tmp_path / "b.ec"), 10, 2, parts, UPLOAD_KEY, UPLOAD_ID, KEY, PREFIX,
                                                  IDP)
    assert e.value.code == -20  # 303 chunks and 2: k + m > 255
    assert not os.path.exists(tmp_path / "a.ec") and not os.path.exists(tmp_path / "b.ec")


# ---- two completions at once --------------------------------------------------------------------------

def test_two_completions_at_once(ctx, tmp_path):
    """Two threads on one context, different upload and object keys."""
    jobs = []
    for t in range(2):
        uk, key = _rand(32, 200 + t), _rand(32, 300 + t)
        parts, bodies = _write_parts(tmp_path, [(2 * FS + 11 + t, True), (50000, False), (17 * FS, True)], 400 + 10 * t,
                                     upload_key=uk, tag=f"t{t}_")
        jobs.append({"uk": uk, "key": key, "parts": parts, "plain": b"".join(bodies), "ec": str(tmp_path / f"t{t}.ec"),
                     "err": None})

    def work(j):
        try:
            j["etag"] = ctx.complete_multipart_streamed_encrypted(j["ec"], MIB // 2 + 7, 2, j["parts"], j["uk"], UPLOAD_ID,
                                                                  j["key"], PREFIX, IDP)
        except Exception as e:  # noqa: BLE001 -- reported below, on the main thread
            j["err"] = e

    threads = [threading.Thread(target=work, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for j in jobs:
        assert j["err"] is None, j["err"]
        plain = j["plain"]
        ct = oracle.frames_encrypt(j["key"], PREFIX, plain, _aads(IDP, (len(plain) + FS - 1) // FS))
        _check_dir(j["ec"], *expected_ec_object(ct, MIB // 2 + 7, 2, plaintext_size=len(plain)))
        assert j["etag"] == _etag(j["parts"])
