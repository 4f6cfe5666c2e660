"""GPU: two file-level behaviours of the storage host code that no other
test pins -- mxec_try_reconstruct_data_chunk over a `{key}.ec` directory
(storage_scrub.cpp) and how many messages a GET hashes (storage_get.cpp).
Every expected value was recorded from the library before the storage code
was split, so the split cannot move them unnoticed.

Reference: try_reconstruct_data_chunk, chunk_reader.rs:157-226; the message
counts have none (the reference hashes chunk by chunk)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import maxio_amd

pytestmark = pytest.mark.gpu


# ---- mxec_try_reconstruct_data_chunk ------------------------------------------

CHUNK, SIZE, K, M = 100, 350, 4, 2  # the reference scenarios' shape: last chunk 50 bytes


def _put350(ctx, tmp_path, parity=M):
    body = np.random.default_rng(350).integers(0, 256, SIZE, dtype=np.uint8).tobytes()
    ec = tmp_path / "t.ec"
    ctx.put_object_chunked(str(ec), CHUNK, parity, body)
    return body, ec


def _chunk(body, t):
    return body[t * CHUNK:(t + 1) * CHUNK]


def test_try_reconstruct_healthy_targets(ctx, tmp_path):
    """Every healthy target is its own bytes; the short last chunk is 50."""
    body, ec = _put350(ctx, tmp_path)
    for t in range(K):
        assert ctx.try_reconstruct_data_chunk(str(ec), t) == _chunk(body, t)
    assert len(ctx.try_reconstruct_data_chunk(str(ec), K - 1)) == 50


def test_try_reconstruct_target_past_data(ctx, tmp_path):
    _, ec = _put350(ctx, tmp_path)
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.try_reconstruct_data_chunk(str(ec), K)
    assert e.value.name == "InvalidIndex"


def test_try_reconstruct_without_parity_fails(ctx, tmp_path):
    """ReedSolomon::new(k, 0) fails before any shard is read: this path runs
    the geometry check even when m = 0 (scrub and locate do not)."""
    _, ec = _put350(ctx, tmp_path, parity=0)
    assert "parity_shards" not in json.loads((ec / "manifest.json").read_text())
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.try_reconstruct_data_chunk(str(ec), 0)
    assert e.value.name == "TooFewParityShards"
    assert str(e.value).startswith("TooFewParityShards (-5): RS init error: ")


def test_try_reconstruct_too_few_shards(ctx, tmp_path):
    _, ec = _put350(ctx, tmp_path)
    for i in (0, 2, 5):
        os.remove(ec / f"{i:06}")
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.try_reconstruct_data_chunk(str(ec), 0)
    assert e.value.name == "TooFewShardsPresent"
    assert "only 3 of 4 required shards available" in str(e.value)


def test_try_reconstruct_unparsable_digest_is_an_erasure(ctx, tmp_path):
    """A missing file plus a manifest digest of 63 hex digits: two erasures,
    m = 2, every data chunk still comes back."""
    body, ec = _put350(ctx, tmp_path)
    os.remove(ec / "000001")
    man = json.loads((ec / "manifest.json").read_text())
    man["chunks"][3]["sha256"] = man["chunks"][3]["sha256"][:63]
    (ec / "manifest.json").write_text(json.dumps(man))
    for t in range(K):
        assert ctx.try_reconstruct_data_chunk(str(ec), t) == _chunk(body, t)
    os.remove(ec / "000004")  # a third erasure is one too many
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.try_reconstruct_data_chunk(str(ec), 1)
    assert e.value.name == "TooFewShardsPresent"


def test_try_reconstruct_overlong_file_is_an_erasure(ctx, tmp_path):
    body, ec = _put350(ctx, tmp_path)
    for t in (2, 3):
        with open(ec / f"{t:06}", "ab") as f:
            f.write(b"\x00")
        assert ctx.try_reconstruct_data_chunk(str(ec), t) == _chunk(body, t)
    assert ctx.try_reconstruct_data_chunk(str(ec), 0) == _chunk(body, 0)


def test_try_reconstruct_small_output_buffer(ctx, tmp_path):
    _, ec = _put350(ctx, tmp_path)
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.try_reconstruct_data_chunk(str(ec), 0, CHUNK - 1)
    assert e.value.name == "InvalidArgument" and "output buffer too small" in str(e.value)
    assert len(ctx.try_reconstruct_data_chunk(str(ec), 0, CHUNK)) == CHUNK


# ---- what a GET hashes ---------------------------------------------------------

# damage -> ((messages, batches) of a whole-object GET, of the range (200, 700)),
# summed over the context's SHA-256 combiners.
HASHED = {
    "none": ((8, 1), (7, 1)),
    "missing": ((10, 1), (10, 1)),
    "corrupt": ((11, 2), (11, 2)),
    "short": ((10, 1), (10, 1)),
    "missing+corrupt": ((10, 1), (10, 1)),
    "missing+parity": ((9, 1), (7, 1)),
}


def _hashed(ctx):
    n = maxio_amd.lib().mxec_ctx_device_count(ctx.handle)
    st = [ctx.combiner_stats(d) for d in range(n)]
    return sum(s["messages"] for s in st), sum(s["batches"] for s in st)


@pytest.mark.parametrize("damage", list(HASHED))
def test_get_hashes_each_shard_once(ctx_with, tmp_path, damage):
    """1 000 bytes in 128-byte chunks, m = 3: shards 0-7 data, 8-10 parity.
    The whole object is chunks 0-7, the range (200, 700) chunks 1-7.

    none             the range's chunks, one pass: 8 and 7.
    missing (2)      known bad before hashing: every present shard goes
                     through mxec_reconstruct's verify in the same call --
                     7 of the range + 3 parity = 10; for the range 6 + shard
                     0 + 3 parity = 10.
    corrupt (4)      only a digest failure: the range's chunks (8 / 7), then
                     one more pass over the shards outside it (3 / 4) and a
                     plain decode: 11 in two batches.
    short (1)        as missing: 10.
    missing+corrupt  (2 missing, 6 corrupt) one verifying decode over the 10
                     present shards; shard 6 fails there and is not hashed again.
    missing+parity   (0 and 10 missing, 9 corrupt) whole: 7 + shards 8, 9 = 9
                     in the one verifying decode.  The range does not hold
                     chunk 0 and its 7 chunks are good: one pass, no decode."""
    ctx = ctx_with(MXEC_GET_WINDOW=None)
    body = np.random.default_rng(9).integers(0, 256, 1000, dtype=np.uint8).tobytes()
    ec = tmp_path / "o.ec"
    ctx.put_object_chunked(str(ec), 128, 3, body)  # k = 8

    def corrupt(i):
        raw = bytearray((ec / f"{i:06}").read_bytes())
        raw[5] ^= 0x40
        (ec / f"{i:06}").write_bytes(raw)

    if damage in ("missing", "missing+corrupt"):
        os.remove(ec / "000002")
    if damage == "corrupt":
        corrupt(4)
    elif damage == "short":
        (ec / "000001").write_bytes(bytes(7))
    elif damage == "missing+corrupt":
        corrupt(6)
    elif damage == "missing+parity":
        os.remove(ec / "000000")
        corrupt(9)
        os.remove(ec / "000010")

    got = []
    for off, ln in ((0, None), (200, 700)):
        m0, b0 = _hashed(ctx)
        out = ctx.get_object_chunked(str(ec), off, ln, capacity=1000)
        m1, b1 = _hashed(ctx)
        assert out == (body[off:] if ln is None else body[off:off + ln])
        got.append((m1 - m0, b1 - b0))
    print("HASHED", damage, tuple(got))
    assert tuple(got) == HASHED[damage]
