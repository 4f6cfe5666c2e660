"""CPU: pin the encrypt-then-EC frame oracle (oracle/gcm_oracle.c) — AES-256
(FIPS-197), GCM (SP 800-38D) and the crypto.rs frame layout — against the
published vectors and against OpenSSL's EVP_aes_256_gcm (an independent
implementation, loaded from the system libcrypto).  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import gcm_cases
import openssl_gcm
import oracle

needs_openssl = pytest.mark.skipif(openssl_gcm.lib() is None, reason="libcrypto not loadable")


def _rand(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def test_fips197_aes256_vector():
    # FIPS-197 Appendix C.3
    key = bytes(range(32))
    assert oracle.aes256_block(key, bytes.fromhex("00112233445566778899aabbccddeeff")).hex() == \
        "8ea2b7ca516745bfeafc49904b496089"


def test_gcm_published_cases():
    # McGrew & Viega GCM spec, test cases 13 and 14 (AES-256, zero key and IV).
    key, iv = bytes(32), bytes(12)
    ct, tag = oracle.gcm_encrypt(key, iv, b"")
    assert ct == b"" and tag.hex() == "530f8afbc74536b9a963b4f1c4cb738b"
    ct, tag = oracle.gcm_encrypt(key, iv, bytes(16))
    assert ct.hex() == "cea7403d4d606b6e074ec5d3baf39d18"
    assert tag.hex() == "d0d1c8a799996bf0265b98b5d48ab919"


@needs_openssl
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 100, 4096, 65536, 65537])
@pytest.mark.parametrize("aad_len", [0, 20, 32])
def test_gcm_matches_openssl(n, aad_len):
    key, iv = _rand(32, 1 + n), _rand(12, 2 + n)
    pt, aad = _rand(n, 3 + n), _rand(aad_len, 4 + n)
    ct, tag = oracle.gcm_encrypt(key, iv, pt, aad)
    assert (ct, tag) == openssl_gcm.encrypt(key, iv, pt, aad)
    assert oracle.gcm_decrypt(key, iv, ct, tag, aad) == pt
    bad = bytes([tag[0] ^ 1]) + tag[1:]
    assert oracle.gcm_decrypt(key, iv, ct, bad, aad) is None
    assert openssl_gcm.decrypt(key, iv, ct, bad, aad) is None


def test_gf128_mul_is_commutative_and_distributive():
    a, b, c = _rand(16, 5), _rand(16, 6), _rand(16, 7)
    assert oracle.gf128_mul(a, b) == oracle.gf128_mul(b, a)
    bc = bytes(x ^ y for x, y in zip(b, c))
    lhs = oracle.gf128_mul(a, bc)
    rhs = bytes(x ^ y for x, y in zip(oracle.gf128_mul(a, b), oracle.gf128_mul(a, c)))
    assert lhs == rhs


@needs_openssl
@pytest.mark.parametrize("n", [0, 23, 65536, 2 * 65536 + 1000])
def test_frames_layout_and_round_trip(n):
    """crypto.rs tests round_trip_small/empty/multi_frame: frame = nonce(prefix
    || index LE) || ciphertext || tag; len = n + 28 per frame; each frame is
    an independent AES-256-GCM message (checked with OpenSSL)."""
    key, prefix = bytes([0x42]) * 32, bytes([1, 2, 3, 4])
    pt = bytes(i % 256 for i in range(n))
    fs = oracle.FRAME_CHUNK_SIZE
    nfr = (n + fs - 1) // fs
    aads = [oracle.frame_aad(oracle.object_aad_prefix("bkt", "obj/key", None), i) for i in range(nfr)]
    out = oracle.frames_encrypt(key, prefix, pt, aads)
    assert len(out) == n + 28 * nfr
    for i in range(nfr):
        fr = out[i * (fs + 28):(i + 1) * (fs + 28)]
        ln = min(fs, n - i * fs)
        assert fr[:12] == prefix + i.to_bytes(8, "little")
        ct, tag = openssl_gcm.encrypt(key, fr[:12], pt[i * fs:i * fs + ln], aads[i])
        assert fr[12:12 + ln] == ct and fr[12 + ln:12 + ln + 16] == tag
    rc, back = oracle.frames_decrypt(key, out, n, aads)
    assert rc == 0 and back == pt


def _check_job_against_openssl(job):
    """Every frame of job: the header, the ciphertext and tag as OpenSSL
    gives them for that nonce, and the way back."""
    out = oracle.frames_encrypt(job.key, job.prefix, job.pt, **job.oracle_args())
    assert len(out) == job.frames_len, job.label
    for f, (fo, po, ln, index) in enumerate(gcm_cases.frame_slices(job)):
        fr = out[fo:fo + 12 + ln + 16]
        assert fr[:12] == job.prefix + index.to_bytes(8, "little"), (job.label, f)
        ct, tag = openssl_gcm.encrypt(job.key, fr[:12], job.pt[po:po + ln], job.aads[f] if job.aads else b"")
        assert fr[12:12 + ln] == ct, (job.label, f, "ciphertext")
        assert fr[12 + ln:] == tag, (job.label, f, "tag")
    rc, back = oracle.frames_decrypt(job.key, out, len(job.pt), **job.oracle_args())
    assert rc == 0 and back == job.pt, job.label


@needs_openssl
def test_lane_and_stream_cases_match_openssl():
    """The GPU sweep's own frames (gcm_cases.py): indices up to 2^64 - 1, AADs
    of 0 .. 4101 bytes with partial last blocks, block counts on both sides
    of every multiple of 256 up to 769."""
    jobs = gcm_cases.lane_cases() + gcm_cases.stream_cases()
    assert {j.aad_len for j in jobs} >= set(gcm_cases.AAD_LENS)
    assert {j.first_index for j in jobs} >= set(gcm_cases.INDICES)
    for job in jobs:
        _check_job_against_openssl(job)


@needs_openssl
def test_tiny_cases_match_openssl():
    for job in gcm_cases.tiny_cases(300):
        _check_job_against_openssl(job)


@needs_openssl
def test_counter_boundary_frame_matches_openssl():
    """One frame of 65534 blocks: the last counter is 0xFFFF."""
    job = gcm_cases.counter_edge_case()
    assert job.n_frames == 2 and job.frame_size == 65534 * 16
    _check_job_against_openssl(job)


@needs_openssl
def test_long_counter_frame_matches_openssl():
    """One frame of 65535 blocks: the last counter is 0x10000, the first that
    the kernel's short-counter path cannot make."""
    job = gcm_cases.long_counter_case()
    assert job.n_frames == 2 and job.frame_size == 65535 * 16 and job.aad_len == 17
    assert job.first_index < 2**32 <= job.first_index + 1
    _check_job_against_openssl(job)


def test_case_table_shape():
    """The table holds what the sweep relies on: every (na, m, last block)
    combination, single frames, and the byte-equal keys in two buffers."""
    lane = gcm_cases.lane_cases()
    assert all(j.n_frames == 1 and j.frame_size == 16384 for j in lane)
    seen = {((j.aad_len + 15) // 16, (j.aad_len + 15) // 16 + (len(j.pt) + 15) // 16 + 1, len(j.pt) % 16 or 16)
            for j in lane}
    for na in (0, 1, 2, 3, 255, 256, 257):
        for m in gcm_cases.SEQ_LENS:
            if m - na - 1 >= 1:
                assert {(na, m, t) for t in (16, 1, 15)} <= seen, (na, m)
    keys = {id(j.key): j.key for j in lane}
    assert len(keys) == 8 and len(set(keys.values())) == 7
    assert all(any(b & 0x80 for b in j.prefix) for j in lane)
    tiny = gcm_cases.tiny_cases(300)
    assert len({j.key for j in tiny}) == 23 and all(1 <= len(j.pt) <= 600 and j.n_frames == 1 for j in tiny)
    assert [j.n_frames for j in gcm_cases.stream_cases()] == [3, 11, 2300]


def test_frames_errors():
    key, prefix = bytes([7]) * 32, b"abcd"
    pt = _rand(3 * 1000, 9)
    out = bytearray(oracle.frames_encrypt(key, prefix, pt, frame_size=1000))
    # frame swap -> index mismatch (crypto.rs:330-340)
    f0, f1 = bytes(out[:1028]), bytes(out[1028:2056])
    swapped = f1 + f0 + bytes(out[2056:])
    assert oracle.frames_decrypt(key, swapped, 3000, frame_size=1000)[0] == -44
    # flipped ciphertext bit -> authentication error (:355-360)
    out[1028 + 12 + 5] ^= 0x10
    assert oracle.frames_decrypt(key, bytes(out), 3000, frame_size=1000)[0] == -41
    # wrong AAD (cross-object swap) -> authentication error
    good = oracle.frames_encrypt(key, prefix, pt[:500], [b"A" * 32], frame_size=1000)
    assert oracle.frames_decrypt(key, good, 500, [b"B" * 32], frame_size=1000)[0] == -41
