"""GPU: mxec_locate_object -- the scrub's cheap pass, naming the damaged shard
of one `{key}.ec` directory and healing it by hashing the one rebuilt shard
(storage_scrub.cpp), beside mxec_scrub_object.

Objects are written with put_object_chunked at the reference's own test
shape (350 B in 100-byte chunks: 4 + 2) and at 20 000-byte chunks (five data
chunks with a short last one, three parity shards).  Expectations: the shard
is the one the test damaged, first_bad / n_bad are the bytes it changed, a
heal leaves the directory byte-equal to the pristine copy, and nothing is
touched when the heal cannot be vouched for.

Reference: none -- MaxIO has no scrubber."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import maxio_amd

pytestmark = pytest.mark.gpu

OK = (1 << 64) - 1
CLEAN, ONE, MANY, SKIPPED = 0, 1, 2, 3
SCRUB_HEALED = 2
# (chunk size, body bytes, k, m)
SHAPES = [(100, 350, 4, 2), (20000, 4 * 20000 + 6667, 5, 3)]


@pytest.fixture(params=SHAPES, ids=lambda s: "chunk%d" % s[0])
def shape(request):
    return request.param


def _put(ctx, tmp_path, shape, parity=None, seed=11):
    chunk, n, _, m = shape
    body = np.random.default_rng(seed + chunk).integers(0, 256, n, dtype=np.uint8).tobytes()
    ec = str(tmp_path / "obj.ec")
    os.makedirs(ec)
    ctx.put_object_chunked(ec, chunk, m if parity is None else parity, body)
    return ec, body


def _snapshot(ec):
    return {n: open(os.path.join(ec, n), "rb").read() for n in sorted(os.listdir(ec))}


def _flip(ec, shard, at, bits=0x10):
    p = os.path.join(ec, "%06d" % shard)
    b = bytearray(open(p, "rb").read())
    b[at] ^= bits
    open(p, "wb").write(bytes(b))


def _zero(ec, shard):
    p = os.path.join(ec, "%06d" % shard)
    n = os.path.getsize(p)
    open(p, "wb").write(bytes(n))
    return n


def _hashed(ctx):
    """Messages the SHA-256 combiners of the context's devices have hashed."""
    n = maxio_amd.lib().mxec_ctx_device_count(ctx.handle)
    return sum(ctx.combiner_stats(d)["messages"] for d in range(n))


def test_untouched_object_is_clean(ctx, tmp_path, shape):
    ec, _ = _put(ctx, tmp_path, shape)
    before = _snapshot(ec)
    _, _, k, m = shape
    assert sorted(before) == ["%06d" % i for i in range(k + m)] + ["manifest.json"]
    for heal in (False, True):
        r = ctx.locate_object(ec, heal=heal)
        assert r == {"k": k, "m": m, "outcome": CLEAN, "shard": None, "first_bad": OK, "n_bad": 0, "healed": 0}
    assert _snapshot(ec) == before


@pytest.mark.parametrize("which", ["data0", "short", "parity0", "parity_last"])
def test_one_flipped_byte_is_located_and_healed(ctx, tmp_path, shape, which):
    ec, body = _put(ctx, tmp_path, shape)
    before = _snapshot(ec)
    chunk, _, k, m = shape
    shard = {"data0": 0, "short": k - 1, "parity0": k, "parity_last": k + m - 1}[which]
    at = len(before["%06d" % shard]) - 1 if which != "data0" else 0
    _flip(ec, shard, at)
    damaged = _snapshot(ec)
    r = ctx.locate_object(ec)
    assert r == {"k": k, "m": m, "outcome": ONE, "shard": shard, "first_bad": at, "n_bad": 1, "healed": 0}
    assert _snapshot(ec) == damaged  # without HEAL nothing is written
    r = ctx.locate_object(ec, heal=True)
    assert r == {"k": k, "m": m, "outcome": ONE, "shard": shard, "first_bad": at, "n_bad": 1, "healed": 1}
    assert _snapshot(ec) == before  # every chunk file, manifest.json untouched, no temporary name left
    assert ctx.locate_object(ec)["outcome"] == CLEAN
    assert ctx.get_object_chunked(ec) == body


@pytest.mark.parametrize("which", ["data", "parity"])
def test_a_zeroed_shard_file_is_located_and_healed(ctx, tmp_path, shape, which):
    ec, body = _put(ctx, tmp_path, shape)
    before = _snapshot(ec)
    _, _, k, m = shape
    shard = 1 if which == "data" else k + 1
    _zero(ec, shard)
    was = np.frombuffer(before["%06d" % shard], np.uint8)
    r = ctx.locate_object(ec)
    assert (r["outcome"], r["shard"], r["healed"]) == (ONE, shard, 0)
    assert r["n_bad"] == int(np.count_nonzero(was)) and r["first_bad"] == int(np.flatnonzero(was)[0])
    r = ctx.locate_object(ec, heal=True)
    assert (r["outcome"], r["shard"], r["healed"]) == (ONE, shard, 1)
    assert _snapshot(ec) == before
    assert ctx.get_object_chunked(ec) == body


def test_two_damaged_shards_is_many_and_nothing_is_written(ctx, tmp_path, shape):
    ec, _ = _put(ctx, tmp_path, shape)
    _, _, k, m = shape
    _flip(ec, 0, 3)
    _flip(ec, k, 41)
    damaged = _snapshot(ec)
    for heal in (False, True):
        r = ctx.locate_object(ec, heal=heal)
        assert (r["outcome"], r["shard"], r["healed"], r["first_bad"], r["n_bad"]) == (MANY, None, 0, 3, 2)
        assert _snapshot(ec) == damaged


def test_missing_or_wrong_sized_file_is_skipped(ctx, tmp_path, shape):
    ec, _ = _put(ctx, tmp_path, shape)
    _, _, k, m = shape
    with open(os.path.join(ec, "%06d" % k), "ab") as f:
        f.write(b"x")
    state = _snapshot(ec)
    r = ctx.locate_object(ec, heal=True)
    assert r == {"k": k, "m": m, "outcome": SKIPPED, "shard": None, "first_bad": OK, "n_bad": 0, "healed": 0}
    assert _snapshot(ec) == state
    os.remove(os.path.join(ec, "%06d" % k))
    os.remove(os.path.join(ec, "000001"))
    state = _snapshot(ec)
    assert ctx.locate_object(ec, heal=True)["outcome"] == SKIPPED
    assert _snapshot(ec) == state


def test_one_parity_shard_is_skipped(ctx, tmp_path, shape):
    ec, _ = _put(ctx, tmp_path, shape, parity=1)
    _, _, k, _ = shape
    _flip(ec, 0, 0)
    state = _snapshot(ec)
    r = ctx.locate_object(ec, heal=True)
    assert (r["k"], r["m"], r["outcome"], r["healed"]) == (k, 1, SKIPPED, 0)
    assert _snapshot(ec) == state


@pytest.mark.parametrize("digest", ["wrong", "unparsable"])
def test_wrong_manifest_digest_for_the_located_shard_is_not_healed(ctx, tmp_path, shape, digest):
    ec, _ = _put(ctx, tmp_path, shape)
    mp = os.path.join(ec, "manifest.json")
    d = json.load(open(mp))["chunks"][2]["sha256"]
    bad = (("0" if d[0] != "0" else "1") + d[1:]) if digest == "wrong" else "zz" + d[2:]
    text = open(mp).read().replace(d, bad)
    open(mp, "w").write(text)
    _flip(ec, 2, 5)
    state = _snapshot(ec)
    r = ctx.locate_object(ec, heal=True)
    assert (r["outcome"], r["shard"], r["healed"], r["first_bad"]) == (ONE, 2, 0, 5)
    assert _snapshot(ec) == state  # nothing created, changed or removed


def test_heal_hashes_one_message_where_the_scrub_hashes_k_m_1(ctx, tmp_path, shape):
    """The digest pass is spared: locate's heal hashes the rebuilt shard
    alone; the scrub's heal hashes every present shard, then the rebuilt one."""
    _, _, k, m = shape
    os.makedirs(tmp_path / "a")
    os.makedirs(tmp_path / "b")
    ec_a, _ = _put(ctx, tmp_path / "a", shape)
    ec_b, _ = _put(ctx, tmp_path / "b", shape)
    before = _snapshot(ec_a)
    _flip(ec_a, 1, 7)
    _flip(ec_b, 1, 7)
    n0 = _hashed(ctx)
    assert ctx.locate_object(ec_a)["outcome"] == ONE
    n1 = _hashed(ctx)
    assert ctx.locate_object(ec_a, heal=True)["healed"] == 1
    n2 = _hashed(ctx)
    r = ctx.scrub_object(ec_b, parity=True, heal=True)
    n3 = _hashed(ctx)
    assert r["verdict"] == SCRUB_HEALED
    assert (n1 - n0, n2 - n1, n3 - n2) == (0, 1, k + m + 1)
    assert _snapshot(ec_a) == before == _snapshot(ec_b)


def test_errors_come_back_as_from_the_scrub(ctx, tmp_path, shape):
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.locate_object(str(tmp_path / "nothing.ec"))
    assert e.value.name == "Io"
    ec, _ = _put(ctx, tmp_path, shape)
    r = maxio_amd._native.LocateReport()
    import ctypes

    rc = maxio_amd.lib().mxec_locate_object(ctx.handle, ec.encode(), 2, ctypes.byref(r))
    assert rc == -21  # unknown flag
    open(os.path.join(ec, "manifest.json"), "w").write("{")
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.locate_object(ec)
    assert e.value.name == "Json"
