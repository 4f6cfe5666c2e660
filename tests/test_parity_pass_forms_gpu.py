"""GPU: the three forms of each parity pass (host pointers, strided device
batch, mixed device batch; maxio_amd/csrc/parity_pass.cpp) agree with each
other and with the oracle.

Per shape and form: the encode is oracle.encode; the verify reports
MXEC_VERIFY_OK in every row and the locate a clean record; after one flipped
byte in data shard 0 the verify's first_bad is that byte's offset in every row
(no parity coefficient of an MDS code is zero) and the locate's record is
(offset, 1, 0, 0), outcome ONE, shard 0.

Shapes, each where a kernel can still go wrong: 1+2 at S = 1; 3+2 at S = 100
(byte-exact edge path); 4+2 at S = 4112 with a 17-byte last chunk (tile edge
plus zero padding); 10+4 at S = 65536 (fast path).  The strided batches hold
three objects with the flip in the middle one, so every object's result
entries are addressed; the mixed batch holds all four shapes in one call."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle
from locate_ref import CLEAN_RECORD

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 1, 1), (3, 2, 100, 100), (4, 2, 4112, 17), (10, 4, 65536, 65536)]  # k, m, S, last chunk's length
IDS = ["%d+%d_S%d" % s[:3] for s in SHAPES]
VERIFY_OK = (1 << 64) - 1
ONE = 1
REC = np.dtype([("first_bad", "<u8"), ("n_bad", "<u8"), ("shard_min", "<u4"), ("shard_max", "<u4")])
N_STRIDED = 3


def _round(x, a=256):
    return (x + a - 1) // a * a


@functools.lru_cache(maxsize=None)
def reference(i: int, obj: int = 0):
    """Shape i's object `obj`: (data chunks, the oracle's parity, the flip's
    offset in data shard 0).  Computed once; callers copy before they write."""
    k, m, S, last = SHAPES[i]
    rng = np.random.default_rng(7100 + 10 * i + obj)
    data = [rng.integers(0, 256, S if j < k - 1 else last, dtype=np.uint8) for j in range(k)]
    par = oracle.encode(data, m, S)
    for a in data + par:
        a.setflags(write=False)
    return data, par, int(rng.integers(0, data[0].size))


def _lens(i):
    k, _, S, last = SHAPES[i]
    return [S] * (k - 1) + [last]


def _records(t):
    return [tuple(int(v) for v in r) for r in np.frombuffer(t.cpu().numpy().tobytes(), REC)]


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_host_form(ctx, i):
    k, m, S, _ = SHAPES[i]
    data, par, x = reference(i)
    got, _ = ctx.encode(data, m, S, digests=False)
    assert all(np.array_equal(g, p) for g, p in zip(got, par))
    assert ctx.verify(data, par, S) == (True, [VERIFY_OK] * m)
    r = ctx.locate(data, par, S)
    assert (r["first_bad"], r["n_bad"], r["shard_min"], r["shard_max"]) == CLEAN_RECORD and r["outcome"] == 0
    bad = [d.copy() for d in data]
    bad[0][x] ^= 0x5A
    assert ctx.verify(bad, par, S) == (False, [x] * m)
    r = ctx.locate(bad, par, S)
    assert (r["first_bad"], r["n_bad"], r["outcome"], r["shard"]) == (x, 1, ONE, 0)
    assert (r["shard_min"], r["shard_max"]) == (0, 0)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_strided_form(ctx, i):
    import torch

    import maxio_amd

    k, m, S, _ = SHAPES[i]
    Sp, n = _round(S), N_STRIDED
    refs = [reference(i, o) for o in range(n)]
    h = np.full((n, k + m, Sp), 0xA5, np.uint8)  # parity slots and the bytes past every length: garbage
    for o, (data, _, _) in enumerate(refs):
        for j, d in enumerate(data):
            h[o, j, :d.size] = d
    t = torch.from_numpy(h).cuda()
    fb = torch.zeros(n * m, dtype=torch.int64, device="cuda")
    out = torch.zeros(n * REC.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    layout = (t.data_ptr(), (k + m) * Sp, Sp, t.data_ptr() + k * Sp, (k + m) * Sp, Sp)

    def verify_and_locate():
        ctx.verify_strided_device(k, m, S, n, *layout, fb.data_ptr(), data_len=_lens(i))
        ctx.locate_strided_device(k, m, S, n, *layout, out.data_ptr(), data_len=_lens(i))
        torch.cuda.synchronize()
        return [int(v) & VERIFY_OK for v in fb.cpu().tolist()], _records(out)

    ctx.encode_strided_device(k, m, S, n, *layout, data_len=_lens(i))
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    for o, (_, par, _) in enumerate(refs):
        assert all(np.array_equal(got[o, k + r, :S], par[r]) for r in range(m)), o
    assert verify_and_locate() == ([VERIFY_OK] * (n * m), [CLEAN_RECORD] * n)
    x = refs[1][2]
    t[1, 0, x] ^= 0x5A
    want_fb = [VERIFY_OK] * m + [x] * m + [VERIFY_OK] * m
    assert verify_and_locate() == (want_fb, [CLEAN_RECORD, (x, 1, 0, 0), CLEAN_RECORD])
    assert maxio_amd.locate_outcome(x, 1, 0, 0) == (ONE, 0)


def test_mixed_form(ctx):
    """All four shapes in one call of each mixed entry point."""
    import torch

    import maxio_amd

    shapes = [(k, m, S) for (k, m, S, _) in SHAPES]
    refs = [reference(i) for i in range(len(SHAPES))]
    ts, dptr, pptr, dlen = [], [], [], []
    for i, ((k, m, S, _), (data, _, _)) in enumerate(zip(SHAPES, refs)):
        h = np.full((k + m, _round(S)), 0xA5, np.uint8)
        for j, d in enumerate(data):
            h[j, :d.size] = d
        t = torch.from_numpy(h).cuda()
        ts.append(t)
        dptr += [t[j].data_ptr() for j in range(k)]
        pptr += [t[k + r].data_ptr() for r in range(m)]
        dlen += _lens(i)
    rows = sum(m for (_, m, _) in shapes)
    fb = torch.zeros(rows, dtype=torch.int64, device="cuda")
    out = torch.zeros(len(shapes) * REC.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def verify_and_locate():
        ctx.verify_batch_device(shapes, dptr, pptr, fb.data_ptr(), data_len=dlen)
        ctx.locate_batch_device(shapes, dptr, pptr, out.data_ptr(), data_len=dlen)
        torch.cuda.synchronize()
        return [int(v) & VERIFY_OK for v in fb.cpu().tolist()], _records(out)

    ctx.encode_batch_device(shapes, dptr, pptr, data_len=dlen)
    torch.cuda.synchronize()
    for (k, m, S), t, (_, par, _) in zip(shapes, ts, refs):
        got = t.cpu().numpy()
        assert all(np.array_equal(got[k + r, :S], par[r]) for r in range(m)), (k, m, S)
    assert verify_and_locate() == ([VERIFY_OK] * rows, [CLEAN_RECORD] * len(shapes))
    want_fb, want_rec = [], []
    for (k, m, S), t, (_, _, x) in zip(shapes, ts, refs):
        t[0, x] ^= 0x5A
        want_fb += [x] * m
        want_rec.append((x, 1, 0, 0))
    got_fb, got_rec = verify_and_locate()
    assert (got_fb, got_rec) == (want_fb, want_rec)
    assert [maxio_amd.locate_outcome(*r) for r in got_rec] == [(ONE, 0)] * len(shapes)
