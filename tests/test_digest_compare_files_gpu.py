"""GPU: the digest compare at the file layer, handed a manifest whose recorded
SHA-256 strings are wrong by one hex digit, or upper case.

The GET's healthy path compares the lower-case hex string, as the reference
does (chunk_reader.rs:108-109 and :184-185, hex::encode(..) !=
chunk_info.sha256); the verifying decode taken when a chunk file is missing
(storage_get.cpp decode(true)) and the scrubber (storage_scrub.cpp) compare
the parsed 32 bytes.  Both must agree with the reference: one changed digit is
a mismatch at exactly that shard whichever digit it is, and a digest that is
not the 64 lower-case digits never matches on either path.

The object: 434 bytes in 100-byte chunks with m = 2 (k = 5, the last chunk 34
bytes), laid down as filesystem.rs writes it (tests/helpers.py
expected_ec_object: parity from the oracle, digests from hashlib), so nothing
expected here comes from the library.
"""
from __future__ import annotations

import json
import os
import shutil

import numpy as np
import pytest

import maxio_amd
from helpers import expected_ec_object

pytestmark = pytest.mark.gpu

CHUNK, SIZE, K, M = 100, 434, 5, 2
TOTAL = K + M
S_OK, S_MISSING, S_BAD = maxio_amd.SHARD_OK, maxio_amd.SHARD_MISSING, maxio_amd.SHARD_BAD_DIGEST
UNRECOVERABLE_GET = ("Integrity", "TooFewShardsPresent")  # as tests/test_storage_gpu.py, test_storage_paths_gpu.py
BODY = np.random.default_rng(434).integers(0, 256, SIZE, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def pristine(tmp_path_factory):
    ec = tmp_path_factory.mktemp("digest_files") / "pristine.ec"
    os.makedirs(ec)
    files, manifest = expected_ec_object(BODY, CHUNK, M)
    assert sorted(files) == ["%06d" % i for i in range(TOTAL)]
    for name, data in files.items():
        (ec / name).write_bytes(data)
    (ec / "manifest.json").write_text(manifest)
    return str(ec)


def _copy(pristine, tmp_path, name):
    ec = str(tmp_path / name)
    shutil.copytree(pristine, ec)
    return ec


def _snapshot(ec):
    return {n: open(os.path.join(ec, n), "rb").read() for n in sorted(os.listdir(ec))}


def _edit(ec, fn):
    """fn(chunks) rewrites the manifest's chunk entries in place."""
    mp = os.path.join(ec, "manifest.json")
    man = json.load(open(mp))
    fn(man["chunks"])
    open(mp, "w").write(json.dumps(man, indent=2))


def _change_digit(chunks, shard, pos):
    """Digit `pos` of the shard's sha256 replaced by the one differing in its lowest bit."""
    h = chunks[shard]["sha256"]
    assert len(h) == 64 and h == h.lower()
    chunks[shard]["sha256"] = h[:pos] + "%x" % (int(h[pos], 16) ^ 1) + h[pos + 1:]


def test_pristine_object_reads_and_scrubs_clean(ctx, pristine):
    assert ctx.get_object_chunked(pristine) == BODY
    r = ctx.scrub_object(pristine, parity=True, digests=True)
    assert r["verdict"] == maxio_amd.SCRUB_CLEAN and r["shard_state"] == [S_OK] * TOTAL and (r["k"], r["m"]) == (K, M)


def test_one_changed_digit_is_a_mismatch_at_that_shard(ctx, pristine, tmp_path):
    """Every hex position 0..63, over every shard: the scrub names exactly that
    shard, the GET (which rebuilds a data chunk whose digest does not match)
    still returns the body."""
    for pos in range(64):
        shard = pos % TOTAL
        ec = _copy(pristine, tmp_path, "p%02d.ec" % pos)
        _edit(ec, lambda chunks: _change_digit(chunks, shard, pos))
        before = _snapshot(ec)
        r = ctx.scrub_object(ec, parity=False, digests=True)
        want = [S_BAD if i == shard else S_OK for i in range(TOTAL)]
        assert r["shard_state"] == want and r["n_damaged"] == 1, (pos, shard, r)
        assert r["verdict"] == maxio_amd.SCRUB_DAMAGED, (pos, r)
        assert ctx.get_object_chunked(ec) == BODY, (pos, shard)
        assert _snapshot(ec) == before


@pytest.mark.parametrize("missing", [None, 3], ids=["all-files", "chunk3-missing"])
def test_three_changed_digits_is_unrecoverable(ctx, pristine, tmp_path, missing):
    """Three shards (a data chunk and both parity shards) with one wrong digit
    each, two of them in the digest's last word: more than m.  With every file
    there the GET finds out by the string compare; with chunk 3's file gone it
    takes the verifying decode (mxec_reconstruct's compare) first."""
    ec = _copy(pristine, tmp_path, "three.ec")
    changed = [(1, 60), (5, 7), (6, 63)]
    _edit(ec, lambda chunks: [_change_digit(chunks, s, p) for s, p in changed])
    if missing is not None:
        os.remove(os.path.join(ec, "%06d" % missing))
    before = _snapshot(ec)
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.get_object_chunked(ec)
    assert e.value.name in UNRECOVERABLE_GET, str(e.value)
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.try_reconstruct_data_chunk(ec, 0)
    assert e.value.name == "TooFewShardsPresent", str(e.value)
    r = ctx.scrub_object(ec, heal=True)
    assert r["verdict"] == maxio_amd.SCRUB_UNRECOVERABLE and r["n_healed"] == 0, r
    want = [S_BAD if i in (1, 5, 6) else S_MISSING if i == missing else S_OK for i in range(TOTAL)]
    assert r["shard_state"] == want and r["n_damaged"] == (3 if missing is None else 4), r
    assert _snapshot(ec) == before


def test_two_changed_digits_are_two_erasures(ctx, pristine, tmp_path):
    """m = 2 wrong digests (last word, first word) with a third chunk's file
    missing is one erasure too many; without the missing file the GET serves
    the body."""
    ec = _copy(pristine, tmp_path, "two.ec")
    _edit(ec, lambda chunks: [_change_digit(chunks, 0, 62), _change_digit(chunks, 6, 1)])
    assert ctx.get_object_chunked(ec) == BODY
    for t in range(K):
        assert ctx.try_reconstruct_data_chunk(ec, t) == BODY[t * CHUNK:(t + 1) * CHUNK]
    os.remove(os.path.join(ec, "000002"))
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.get_object_chunked(ec)
    assert e.value.name in UNRECOVERABLE_GET, str(e.value)


def test_upper_case_digests_never_match(ctx, pristine, tmp_path):
    """The reference compares strings (chunk_reader.rs:108-109, :184-185), so
    an upper-case manifest verifies no shard: on the healthy path, on the path
    a missing chunk file takes, in try_reconstruct and in the scrubber alike."""
    ec = _copy(pristine, tmp_path, "upper.ec")

    def upper(chunks):
        for c in chunks:
            assert c["sha256"] != c["sha256"].upper()  # 64 digits with a letter among them
            c["sha256"] = c["sha256"].upper()

    _edit(ec, upper)
    before = _snapshot(ec)
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.get_object_chunked(ec)
    whole = e.value.name
    assert whole in UNRECOVERABLE_GET, str(e.value)
    r = ctx.scrub_object(ec, parity=False, digests=True)
    assert r["shard_state"] == [S_BAD] * TOTAL and r["n_damaged"] == TOTAL, r
    r = ctx.scrub_object(ec, heal=True)
    assert r["verdict"] == maxio_amd.SCRUB_UNRECOVERABLE and r["n_healed"] == 0, r
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.try_reconstruct_data_chunk(ec, 0)
    assert e.value.name == "TooFewShardsPresent", str(e.value)
    assert _snapshot(ec) == before
    os.remove(os.path.join(ec, "000001"))
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.get_object_chunked(ec)
    assert e.value.name == whole, str(e.value)  # the same way as with every file there
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.get_object_chunked(ec, offset=250, length=100)  # a range that does not hold the missing chunk
    assert e.value.name in UNRECOVERABLE_GET, str(e.value)


def test_one_upper_case_digest_is_one_erasure_and_is_not_healed_against(ctx, pristine, tmp_path):
    """A single upper-case entry is that shard's mismatch and nothing more; a
    heal cannot vouch for a rebuilt shard against it, the scrub's or the
    locate's (storage_scrub.cpp rebuild_and_replace)."""
    ec = _copy(pristine, tmp_path, "one_upper.ec")

    def upper2(chunks):
        assert chunks[2]["sha256"] != chunks[2]["sha256"].upper()
        chunks[2]["sha256"] = chunks[2]["sha256"].upper()

    _edit(ec, upper2)
    r = ctx.scrub_object(ec, parity=False, digests=True)
    assert r["shard_state"] == [S_BAD if i == 2 else S_OK for i in range(TOTAL)], r
    assert ctx.get_object_chunked(ec) == BODY
    os.remove(os.path.join(ec, "000004"))
    assert ctx.get_object_chunked(ec) == BODY  # two erasures, m = 2
    shutil.copy(os.path.join(pristine, "000004"), os.path.join(ec, "000004"))
    # damage shard 2 itself: the parity pass locates it, but there is no digest to check a rebuild against
    raw = bytearray(open(os.path.join(ec, "000002"), "rb").read())
    raw[5] ^= 0x10
    open(os.path.join(ec, "000002"), "wb").write(bytes(raw))
    before = _snapshot(ec)
    r = ctx.locate_object(ec, heal=True)
    assert (r["outcome"], r["shard"], r["healed"]) == (maxio_amd.LOCATE_ONE, 2, 0), r
    r = ctx.scrub_object(ec, heal=True)
    assert r["n_healed"] == 0 and r["verdict"] == maxio_amd.SCRUB_UNRECOVERABLE, r
    assert _snapshot(ec) == before
    assert ctx.get_object_chunked(ec) == BODY
