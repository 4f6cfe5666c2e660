"""GPU: mxec_scrub_object -- the scrub / heal call over one `{key}.ec`
directory (storage_scrub.cpp), which the reference does not have (SURVEY.md §3.2,
§5: no scrubber, no heal-on-read, no background repair).

Objects are written with put_object_chunked: five data chunks with a short
last one, two parity shards, chunk sizes 20 000 and 65 536.  Expectations:
the parity check's offset is the flipped byte's (the oracle's parity equals
the stored one, so the first difference is the flip), the digest pass names
the damaged file, and a heal leaves every file byte-equal to the original
and touches nothing when it cannot.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

OK = (1 << 64) - 1
CLEAN, DAMAGED, HEALED, UNRECOVERABLE = 0, 1, 2, 3
S_OK, S_MISSING, S_BAD_SIZE, S_BAD_DIGEST, S_HEALED = 0, 1, 2, 3, 0x80
K, M = 5, 2


def _put(ctx, tmp_path, chunk_size, parity=M, seed=7):
    body = np.random.default_rng(seed + chunk_size).integers(0, 256, 4 * chunk_size + chunk_size // 3 + 1,
                                                            dtype=np.uint8).tobytes()
    ec = str(tmp_path / "obj.ec")
    os.makedirs(ec)
    ctx.put_object_chunked(ec, chunk_size, parity, body)
    return ec, body


def _snapshot(ec):
    return {n: open(os.path.join(ec, n), "rb").read() for n in sorted(os.listdir(ec))}


def _flip(ec, name, at):
    p = os.path.join(ec, name)
    b = bytearray(open(p, "rb").read())
    b[at] ^= 0x10
    open(p, "wb").write(bytes(b))


SIZES = [20000, 65536]


@pytest.mark.parametrize("chunk_size", SIZES)
def test_untouched_object_is_clean_in_every_mode(ctx, tmp_path, chunk_size):
    ec, _ = _put(ctx, tmp_path, chunk_size)
    before = _snapshot(ec)
    assert sorted(before) == ["%06d" % i for i in range(K + M)] + ["manifest.json"]
    # the stored parity is the oracle's
    want = oracle.encode([before["%06d" % j] for j in range(K)], M, chunk_size)
    assert [before["%06d" % (K + i)] for i in range(M)] == [w.tobytes() for w in want]
    for mode in (dict(parity=True), dict(parity=False, digests=True), dict(parity=True, digests=True),
                 dict(parity=True, heal=True)):
        r = ctx.scrub_object(ec, **mode)
        assert r["verdict"] == CLEAN and r["n_damaged"] == 0 and r["n_healed"] == 0, mode
        assert (r["k"], r["m"]) == (K, M) and r["shard_state"] == [S_OK] * (K + M)
        if mode.get("parity"):
            assert r["parity_consistent"] == 1 and r["parity_first_bad"] == OK
        else:
            assert r["parity_consistent"] == -1
    assert _snapshot(ec) == before


@pytest.mark.parametrize("chunk_size", SIZES)
def test_flipped_parity_byte(ctx, tmp_path, chunk_size):
    ec, body = _put(ctx, tmp_path, chunk_size)
    at = chunk_size - 3
    _flip(ec, "%06d" % (K + 1), at)
    r = ctx.scrub_object(ec, parity=True)
    assert r["verdict"] == DAMAGED and r["parity_consistent"] == 0 and r["parity_first_bad"] == at
    assert r["shard_state"] == [S_OK] * (K + M)  # this mode cannot say which shard
    r = ctx.scrub_object(ec, parity=False, digests=True)
    assert r["verdict"] == DAMAGED and r["n_damaged"] == 1 and r["parity_consistent"] == -1
    assert r["shard_state"] == [S_OK] * (K + 1) + [S_BAD_DIGEST]
    # a flipped data byte shows at its offset too (every parity row changes there)
    _flip(ec, "%06d" % (K + 1), at)
    _flip(ec, "000002", 1234)
    r = ctx.scrub_object(ec, parity=True, digests=True)
    assert r["verdict"] == DAMAGED and r["parity_first_bad"] == 1234
    assert r["shard_state"] == [S_OK, S_OK, S_BAD_DIGEST] + [S_OK] * (K + M - 3)


@pytest.mark.parametrize("chunk_size", SIZES)
def test_heal_rewrites_a_deleted_data_file_and_a_truncated_parity_file(ctx, tmp_path, chunk_size):
    ec, body = _put(ctx, tmp_path, chunk_size)
    before = _snapshot(ec)
    os.remove(os.path.join(ec, "000004"))  # the short last chunk
    with open(os.path.join(ec, "%06d" % K), "r+b") as f:
        f.truncate(chunk_size - 1)
    r = ctx.scrub_object(ec, parity=True)  # a missing file: damaged, the kernel is not run
    assert r["verdict"] == DAMAGED and r["parity_consistent"] == -1 and r["n_damaged"] == 2
    assert r["shard_state"] == [S_OK] * 4 + [S_MISSING, S_BAD_SIZE, S_OK]
    r = ctx.scrub_object(ec, parity=True, heal=True)
    assert r["verdict"] == HEALED and r["n_healed"] == 2 and r["n_damaged"] == 2
    assert r["shard_state"] == [S_OK] * 4 + [S_MISSING | S_HEALED, S_BAD_SIZE | S_HEALED, S_OK]
    assert _snapshot(ec) == before  # every chunk file, manifest.json, and no other name
    r = ctx.scrub_object(ec, parity=True, digests=True)
    assert r["verdict"] == CLEAN and r["parity_consistent"] == 1 and r["shard_state"] == [S_OK] * (K + M)
    assert ctx.get_object_chunked(ec) == body


def test_three_damaged_shards_with_m_2_is_unrecoverable_and_touches_nothing(ctx, tmp_path):
    ec, _ = _put(ctx, tmp_path, 20000)
    os.remove(os.path.join(ec, "000001"))
    _flip(ec, "000003", 19999)
    with open(os.path.join(ec, "%06d" % (K + 1)), "ab") as f:
        f.write(b"x")
    before = _snapshot(ec)
    r = ctx.scrub_object(ec, parity=True, heal=True)
    assert r["verdict"] == UNRECOVERABLE and r["n_damaged"] == 3 and r["n_healed"] == 0
    assert r["shard_state"] == [S_OK, S_MISSING, S_OK, S_BAD_DIGEST, S_OK, S_OK, S_BAD_SIZE]
    assert _snapshot(ec) == before


def test_rebuilt_shard_that_disagrees_with_the_manifest_is_not_written(ctx, tmp_path):
    ec, _ = _put(ctx, tmp_path, 20000)
    mp = os.path.join(ec, "manifest.json")
    man = json.load(open(mp))
    d = man["chunks"][2]["sha256"]
    text = open(mp).read().replace(d, ("0" if d[0] != "0" else "1") + d[1:])
    open(mp, "w").write(text)
    os.remove(os.path.join(ec, "000002"))
    before = _snapshot(ec)
    r = ctx.scrub_object(ec, heal=True)
    assert r["verdict"] == UNRECOVERABLE and r["n_damaged"] == 1 and r["n_healed"] == 0
    assert r["shard_state"][2] == S_MISSING
    assert _snapshot(ec) == before


def test_object_without_parity(ctx, tmp_path):
    ec, _ = _put(ctx, tmp_path, 20000, parity=0)
    before = _snapshot(ec)
    assert sorted(before) == ["%06d" % i for i in range(K)] + ["manifest.json"]
    r = ctx.scrub_object(ec, parity=True, digests=True)
    assert (r["k"], r["m"]) == (K, 0) and r["verdict"] == CLEAN and r["parity_consistent"] == -1
    _flip(ec, "000000", 0)
    r = ctx.scrub_object(ec, parity=True, digests=True)
    assert r["verdict"] == DAMAGED and r["shard_state"] == [S_BAD_DIGEST] + [S_OK] * (K - 1)
    before = _snapshot(ec)
    r = ctx.scrub_object(ec, heal=True)
    assert r["verdict"] == UNRECOVERABLE and r["parity_consistent"] == -1 and r["n_healed"] == 0
    assert _snapshot(ec) == before


def test_scrub_errors_come_back_as_from_the_get_path(ctx, tmp_path):
    import maxio_amd

    with pytest.raises(maxio_amd.RSError) as e:
        ctx.scrub_object(str(tmp_path / "nothing.ec"))
    assert e.value.name == "Io"
    ec, _ = _put(ctx, tmp_path, 20000)
    open(os.path.join(ec, "manifest.json"), "w").write("{")
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.scrub_object(ec)
    assert e.value.name == "Json"
