"""GPU: the digest compare of every verified reconstruct, handed WRONG
expected digests -- wrong by single bits, exchanged, or at the wrong index
(tests/digest_flips.py; tests/test_digest_flip_plan.py shows on the CPU that
every expectation follows from hashlib alone).

The rest of the suite corrupts shard bytes (about half of the 256 digest bits
change) or passes correct digests, so a compare that skips a word, a byte or
an index passes it.  Here an object of k = 2, m = 1 whose expected digests are
wrong in m + 1 shards by one bit each must fail with
MXEC_E_TOO_FEW_SHARDS_PRESENT (chunk_reader.rs:176-208: a mismatch is an
erasure, fewer than k left is an error); overlooking either bit leaves k
verified shards and status 0.  Everything is bit-exact; every test asserts the
whole status vector (and on the device calls the whole returned mask) against
the plan, no object skipped.

The compare sites and the cases that reach them:

  sha256_kernel.hip, the tail of each form (compare on the device, exp_idx)
      one-wave   batch_device[one-*]
      split      batch_device[split-*]
      lag pair   batch_device[lagpair-*, auto-*], strided[own-launch-*], batch_host[whole-A];
                 its piece mode batch_host[pieces-A] (one piece) and [pieces-C] (resumed chain)
      stream     batch_device[stream-*] (16-byte aligned shards asserted)
  reconstruct.cpp verify_digests_device (ok flags)       batch_device, strided[own-launch-*]
  reconstruct.cpp verify_combined_speculating (memcmp)   strided[combiner-*]
  reconstruct.cpp mxec_reconstruct (memcmp)              test_reconstruct_one_object
  pipeline_get.cpp verify_collect (ok[slot])             batch_host[pieces-*]
  pipeline_get.cpp upload_and_verify (ok flags)          batch_host[whole-A]

Shapes (shard 0 and the parity S bytes, the last data chunk 55):
  A  S = 120 (one and two padding blocks), stride 128, bit set ALL: 323
     objects, ~950 messages -- every lane of a wave, several workgroups, both
     lanes of a lag-pair message hold a verdict.
  B  S = 32 KiB + 64 + 17: two stream-form segments, a multi-block chain in
     every form, an odd tail; bit set BYTES, 83 objects.
  C  S = 1 MiB + 64 + 17 (host batch only): with 1 MiB pieces the chain is
     carried across two pieces in the device state slots and compared in the
     last; bit set BYTES, 83 objects.

The EMPTY class (a zero-length last data chunk) runs on the calls whose
lengths are per shard: the device batch (clamp_lens and the decode tables take
a zero length, the SHA-256 forms hash empty messages) and the host batch; the
strided call's lengths are one table for every object, so it has none.

mxec_reconstruct_batch_host: include/maxio_ec.h promises a failing object's
status and that its present shards' buffers are not written; it says nothing
about that object's mask on return (nor about its missing shards' buffers),
so neither is asserted there.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import digest_flips as df
import maxio_amd

pytestmark = pytest.mark.gpu

K, M, TOTAL = df.K, df.M, df.TOTAL
SHAPES = {  # bits, S, last, stride (a multiple of 16: the stream form's alignment)
    "A": (df.ALL, 120, 55, 128),
    "B": (df.BYTES, 32 * 1024 + 64 + 17, 55, 33024),
    "C": (df.BYTES, (1 << 20) + 64 + 17, 55, (1 << 20) + 256),
}


@functools.lru_cache(maxsize=None)
def _plan(shape, empty):
    """Built once per shape and shared; tests copy `given`, never write it."""
    bits, S, last, stride = SHAPES[shape]
    p = df.Plan(bits, S, last, stride, empty=empty)
    for a in (p.orig, p.given, p.expected, p.digests):
        a.setflags(write=False)
    return p


def _suspect(p):
    """(n, 3) flags: shards whose expected digest is wrong (flipped or swapped)."""
    s = np.zeros((p.n, TOTAL), bool)
    for o, ob in enumerate(p.objs):
        for shard, _ in ob.flips:
            s[o, shard] = True
        for shard in ob.swap:
            s[o, shard] = True
    return s


def _check(p, given, out, rc, msg, status, mask=None, speculative=False, present_only=False):
    """given: what the call received, out: the buffers after it.
    speculative: a failing object's shards that were missing on input may
    have been written, and only when its input mask had k shards
    (tests/test_contract_gpu.py).  present_only: of a failing object only the
    present shards' buffers are promised (the host batch)."""
    assert rc == df.TOO_FEW, rc
    first = p.objs[int(p.failing()[0])]  # the call's own error is the first failing object's
    assert f"too many missing/corrupt shards: only {sum(first.mask)} of {K} required" in msg, msg
    assert status.shape == p.status.shape
    wrong = np.flatnonzero(status != p.status)  # the whole vector; the message names the first few
    assert wrong.size == 0, (wrong.size, [(int(o), int(status[o]), p.objs[o]) for o in wrong[:5]])
    if mask is not None:
        bad = np.flatnonzero((mask != p.mask).any(axis=1))
        assert bad.size == 0, [(int(o), p.objs[o], mask[o]) for o in bad[:5]]
    suspect = _suspect(p)
    S = p.S
    for o, ob in enumerate(p.objs):
        for i in range(TOTAL):
            L = ob.lens[i]
            if ob.status != df.OK:
                if not ob.present[i] and (present_only or (speculative and sum(ob.present) >= K)):
                    continue
                assert np.array_equal(out[o, i], given[o, i]), ("failing object written", o, i, ob)
                continue
            # served: every shard back bit-exact (rebuilt where it was missing
            # or did not verify); a verified shard is never written at all
            assert np.array_equal(out[o, i, :L], p.orig[o, i, :L]), (o, i, ob)
            assert np.array_equal(out[o, i, S:], given[o, i, S:]), ("written past the shard", o, i, ob)
            if ob.present[i] and not suspect[o, i]:
                assert np.array_equal(out[o, i], given[o, i]), ("verified shard written", o, i, ob)


# ---- mxec_reconstruct_batch_device: always compares on the device -----------------

@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("form", ["auto", "lagpair", "split", "one", "stream"])
def test_batch_device(ctx_with, form, shape):
    """exp_idx = the present shards' global indices, so the MISSING class makes
    exp_idx[i] != i.  The call verifies before it rebuilds: a failing object is
    untouched entirely."""
    import torch

    ctx = ctx_with(MXEC_SHA_FORM=form)
    p = _plan(shape, True)
    dev = torch.from_numpy(p.given.copy()).cuda()
    exp = torch.from_numpy(p.expected.copy()).cuda()
    base = dev.data_ptr()
    ptrs = [base + (o * TOTAL + i) * p.stride for o in range(p.n) for i in range(TOTAL)]
    # the stream form's precondition (run_sha takes another form, silently, for an unaligned message)
    assert p.stride % 16 == 0 and all(q % 16 == 0 for q in ptrs)
    pres = p.present.reshape(-1).copy()
    torch.cuda.synchronize()
    rc, status = ctx.reconstruct_batch_device([(K, M, p.S)] * p.n, ptrs, pres,
                                              shard_len=[int(x) for x in p.lens.reshape(-1)],
                                              expected_ptr=exp.data_ptr())
    msg = maxio_amd.lib().mxec_last_error().decode()
    torch.cuda.synchronize()
    _check(p, p.given, dev.cpu().numpy(), rc, msg, status, pres.reshape(p.n, TOTAL))


# ---- mxec_reconstruct_strided_device: the combiner + host memcmp, or its own launch --

@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("how", ["combiner", "own-launch"])
def test_strided_device(ctx, ctx_with, how, shape):
    """combiner: the default context hashes through the combiner and compares
    on the host (the digests have to find their way back to this caller);
    own-launch: MXEC_COMBINE_BELOW=1 takes the call's own launch and the
    compare on the device."""
    import torch

    c = ctx if how == "combiner" else ctx_with(MXEC_COMBINE_BELOW=1)
    p = _plan(shape, False)
    assert (p.lens == p.lens[0]).all()
    dev = torch.from_numpy(p.given.copy()).cuda()
    exp = torch.from_numpy(p.expected.copy()).cuda()
    assert dev.data_ptr() % 16 == 0
    pres = p.present.reshape(-1).copy()
    torch.cuda.synchronize()
    m0 = c.combiner_stats()["messages"]
    rc, status = c.reconstruct_strided_device(K, M, p.S, p.n, dev.data_ptr(), TOTAL * p.stride, p.stride, pres,
                                              shard_len=[int(x) for x in p.lens[0]], expected_ptr=exp.data_ptr())
    msg = maxio_amd.lib().mxec_last_error().decode()
    torch.cuda.synchronize()
    hashed = c.combiner_stats()["messages"] - m0
    assert hashed == (int(p.present.sum()) if how == "combiner" else 0), hashed  # the path the case names
    _check(p, p.given, dev.cpu().numpy(), rc, msg, status, pres.reshape(p.n, TOTAL), speculative=True)


# ---- mxec_reconstruct_batch_host: piece-major (verdict ok[slot]) or one launch ------

@pytest.mark.parametrize("piece_mb,shape", [(1, "A"), (1, "C"), (0, "A")], ids=["pieces-A", "pieces-C", "whole-A"])
def test_batch_host(ctx_with, piece_mb, shape):
    """pieces-A: every message is one piece, first and final at once.
    pieces-C: the chain is resumed from the state slots, the verdict is
    ok[slot] with slot = the message's index in the wave.  whole-A:
    MXEC_PIPE_PIECE_MB=0, one run_sha with exp_idx after the whole upload."""
    ctx = ctx_with(device_mask=1, MXEC_PIPE_PIECE_MB=piece_mb)
    bits, S, last, stride = SHAPES[shape]
    if shape == "C":
        n = len(df.layout(bits, S, last, empty=True))
        buf = ctx.host_array(n * TOTAL * stride).reshape(n, TOTAL, stride)
        p = df.Plan(bits, S, last, stride, empty=True, given_out=buf)  # used once: not kept
    else:
        p = _plan(shape, True)
        buf = ctx.host_array(p.n * TOTAL * stride).reshape(p.n, TOTAL, stride)
        buf[...] = p.given
    given = p.orig.copy()
    p.fill_given(given)
    pres = p.present.reshape(-1).copy()
    w0 = ctx.pipe_stats()["verify_waves"]
    rc, status = ctx.reconstruct_batch_host([(K, M, S)] * p.n,
                                            [buf[o, i].ctypes.data for o in range(p.n) for i in range(TOTAL)], pres,
                                            shard_len=[int(x) for x in p.lens.reshape(-1)],
                                            expected=np.ascontiguousarray(p.expected).reshape(-1))
    msg = maxio_amd.lib().mxec_last_error().decode()
    waves = ctx.pipe_stats()["verify_waves"] - w0
    assert (waves > 0) == (piece_mb > 0), waves  # piece-major waves, or none
    mask = pres.reshape(p.n, TOTAL)
    assert mask[p.status == df.OK].all()
    _check(p, given, buf, rc, msg, status, present_only=True)
    ctx.host_free(buf)


# ---- mxec_reconstruct: one object from host shards, compared on the host ------------

def test_reconstruct_one_object(ctx):
    p = _plan("A", True)
    for o, ob in enumerate(p.objs):
        shards = [p.given[o, i, :ob.lens[i]] if ob.present[i] else None for i in range(TOTAL)]
        expected = [p.expected[o, i].tobytes() for i in range(TOTAL)]
        if ob.status != df.OK:
            with pytest.raises(maxio_amd.RSError) as e:
                ctx.reconstruct(shards, K, M, p.S, shard_len=list(ob.lens), expected=expected)
            assert e.value.name == "TooFewShardsPresent", (o, ob)
            assert f"only {sum(ob.mask)} of {K} required shards available" in str(e.value), (o, ob, str(e.value))
            continue
        out, present = ctx.reconstruct(shards, K, M, p.S, shard_len=list(ob.lens), expected=expected)
        assert present.all(), (o, ob)
        for i in range(TOTAL):
            assert np.array_equal(out[i], p.orig[o, i, :ob.lens[i]]), (o, i, ob)
