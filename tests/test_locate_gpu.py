"""GPU: mxec_locate -- which shard is damaged, from the parity alone
(mxec_locate, mxec_locate_strided_device, mxec_locate_batch_device;
rs_kernel.hip rs_locate_fast / rs_locate_edge).

The kernel walks the stripe as the verify does, forms every row's syndrome
and, where one is non-zero, classifies each bad byte column; an object's
record is (first_bad, n_bad, shard_min, shard_max).  Every expectation here
is tests/locate_ref.py -- numpy over the oracle's matrix, field arithmetic
and encode -- applied to the bytes as they stand on the device.

Shapes are test_verify_gpu.py's: S = 5 * 16384 + 4096 + 48, 6 objects, shard
pitch rounded to 256, a short last data chunk, contexts capped at 7 and 61
workgroups; m in {2, 3, 4, 8} with that file's k per m, and k = 1, m = 2
(parity is a byte copy of the data).

Reference: none -- the crate has no locator and MaxIO no scrubber (SURVEY.md
§3.2, §5)."""
from __future__ import annotations

import numpy as np
import pytest

import locate_ref
import oracle
from locate_ref import CLEAN_RECORD, NO_SHARD
from test_verify_gpu import GRIDS, K_OF, N, OFFSETS, S, SHORT

pytestmark = pytest.mark.gpu

SHAPES = [(K_OF[m], m) for m in (2, 3, 4, 8)] + [(1, 2)]
REC = np.dtype([("first_bad", "<u8"), ("n_bad", "<u8"), ("shard_min", "<u4"), ("shard_max", "<u4")])
CLEAN, ONE, MANY = 0, 1, 2


def _torch():
    import torch

    return torch


def _round(x, a=256):
    return (x + a - 1) // a * a


def _records(t) -> list[tuple]:
    return [tuple(int(v) for v in r) for r in np.frombuffer(t.cpu().numpy().tobytes(), REC)]


@pytest.fixture(params=GRIDS, ids=lambda g: f"grid{g}")
def gctx(request, ctx_with):
    return ctx_with(MXEC_TEST_RS_GRID=request.param)


@pytest.fixture(params=SHAPES, ids=lambda s: "k%dm%d" % s)
def km(request):
    return request.param


class Uniform:
    """N objects of (k, m, S) in one tensor, encoded by the library."""

    def __init__(self, ctx, k, m, seed):
        torch = _torch()
        self.ctx, self.k, self.m = ctx, k, m
        self.Sp = _round(S)
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.t = torch.randint(0, 256, (N, k + m, self.Sp), dtype=torch.uint8, device="cuda", generator=g)
        self.dl = [S] * (k - 1) + [SHORT]
        self.out = torch.zeros(N * REC.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        Sp, t = self.Sp, self.t
        ctx.encode_strided_device(k, m, S, N, t.data_ptr(), (k + m) * Sp, Sp, t.data_ptr() + k * Sp,
                                  (k + m) * Sp, Sp, data_len=self.dl)
        torch.cuda.synchronize()

    def length(self, shard):
        return self.dl[shard] if shard < self.k else S

    def locate(self):
        torch = _torch()
        k, m, Sp, t = self.k, self.m, self.Sp, self.t
        self.out.fill_(0x55)  # the call initialises the records itself
        torch.cuda.synchronize()
        self.ctx.locate_strided_device(k, m, S, N, t.data_ptr(), (k + m) * Sp, Sp, t.data_ptr() + k * Sp,
                                       (k + m) * Sp, Sp, self.out.data_ptr(), data_len=self.dl)
        torch.cuda.synchronize()
        return _records(self.out)

    def expected(self):
        h = self.t.cpu().numpy()
        return [locate_ref.locate(h[o], self.k, self.m, S, self.dl) for o in range(N)]


def test_clean_batch_and_garbage_past_the_lengths(gctx, km):
    b = Uniform(gctx, *km, 2000 + km[1])
    assert b.expected() == [CLEAN_RECORD] * N  # the encode is the oracle's
    assert b.locate() == [CLEAN_RECORD] * N    # ... over records pre-filled with 0x55
    b.t[:, b.k - 1, SHORT:] = 0xC3
    b.t[:, :, S:] = 0x3C
    assert b.locate() == [CLEAN_RECORD] * N


def _at(x, length):
    """OFFSETS entry x within a shard of `length` bytes: the same distance from its end."""
    return x if x < length else length - 1 - (S - 1 - x)


def test_one_flipped_byte_every_shard_in_turn(gctx, km):
    b = Uniform(gctx, *km, 2100 + km[1])
    for c in range(b.k + b.m):
        for g in range(0, len(OFFSETS), N):
            want = [CLEAN_RECORD] * N
            for o, x in enumerate(OFFSETS[g:g + N]):
                x = _at(x, b.length(c))
                b.t[o, c, x] ^= 0x40
                want[o] = (x, 1, c, c)
            assert b.expected() == want, (c, g)
            got = b.locate()
            assert got == want, (c, g)
            assert all(locate_ref.outcome(r) == ((ONE, c) if r[1] else (CLEAN, None)) for r in got)
            for o, x in enumerate(OFFSETS[g:g + N]):
                b.t[o, c, _at(x, b.length(c))] ^= 0x40
    assert b.expected() == [CLEAN_RECORD] * N  # every flip undone


def test_several_corruptions_at_once(gctx, km):
    """Different objects, different shards, one launch; the others stay clean."""
    b = Uniform(gctx, *km, 2200 + km[1])
    k, m = km
    for x in (3, 4096 + 7, 3 * 16384 + 1, 16):
        b.t[0, 0, x] ^= 0x81            # data shard 0, several tiles
    b.t[2, k + m - 1, S - 1] ^= 0x01    # the last parity shard's last byte
    b.t[2, k + m - 1, 8192] ^= 0xFF
    b.t[4, k - 1, SHORT - 1] ^= 0x10    # the short chunk's last byte
    want = b.expected()
    assert [locate_ref.outcome(r) for r in want] == [(ONE, 0), (CLEAN, None), (ONE, k + m - 1), (CLEAN, None),
                                                     (ONE, k - 1), (CLEAN, None)]
    assert want[0][:2] == (3, 4) and want[2][:2] == (8192, 2) and want[4][:2] == (SHORT - 1, 1)
    assert b.locate() == want


def test_one_shard_overwritten_whole(gctx, km):
    """The slow path's worst case: every column of one shard is bad.  n_bad
    is the number of bytes that actually changed."""
    torch = _torch()
    b = Uniform(gctx, *km, 2300 + km[1])
    k, m = km
    g = torch.Generator(device="cuda").manual_seed(99)
    changed = {}
    for o, c in ((1, k // 2), (3, k + m - 1), (5, k - 1)):
        n = b.length(c)
        new = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        changed[o] = int((new != b.t[o, c, :n]).sum().item())
        b.t[o, c, :n] = new
    want = b.expected()
    for o, c in ((1, k // 2), (3, k + m - 1), (5, k - 1)):
        assert locate_ref.outcome(want[o]) == (ONE, c)
        assert want[o][1] == changed[o] and changed[o] > b.length(c) * 0.99
    assert [want[o] for o in (0, 2, 4)] == [CLEAN_RECORD] * 3
    assert b.locate() == want


def test_two_shards_at_different_offsets_is_many(gctx, km):
    b = Uniform(gctx, *km, 2400 + km[1])
    k, m = km
    b.t[1, 0, 100] ^= 0x02
    b.t[1, k + 1, 4 * 16384 + 5] ^= 0x02    # a data and a parity shard
    b.t[3, k, 17] ^= 0x04
    b.t[3, k + m - 1, 16384] ^= 0x04        # two parity shards
    if k >= 2:
        b.t[5, 0, S - 1] ^= 0x08
        b.t[5, 1, 0] ^= 0x08                # two data shards
    want = b.expected()
    assert want[1] == (100, 2, 0, k + 1) and want[3] == (17, 2, k, k + m - 1)
    assert want[5] == ((0, 2, 0, 1) if k >= 2 else CLEAN_RECORD)
    assert [locate_ref.outcome(r)[0] for r in want] == [CLEAN, MANY, CLEAN, MANY, CLEAN, MANY if k >= 2 else CLEAN]
    assert b.locate() == want


def test_two_shards_at_the_same_offset(gctx, km):
    """One column damaged in two shards.  With m >= 3 the syndrome fits no
    single shard: NO_SHARD.  With m = 2 any non-zero syndrome pair is some
    column's multiple or not; the restatement says which."""
    b = Uniform(gctx, *km, 2500 + km[1])
    k, m = km
    pairs = [(0, 0, k, 5), (1, k - 1, k + m - 1, SHORT - 1), (2, k, k + 1, 4096), (4, 0, k + 1, S - 1)]
    if k >= 2:
        pairs.append((5, 0, 1, 16383))
    for o, c0, c1, x in pairs:
        b.t[o, c0, x] ^= 0x21
        b.t[o, c1, x] ^= 0x5A
    want = b.expected()
    for o, c0, c1, x in pairs:
        assert want[o][:2] == (x, 1)
        if m >= 3:
            assert want[o][2:] == (NO_SHARD, NO_SHARD), (o, want[o])
            assert locate_ref.outcome(want[o]) == (MANY, None)
    assert want[3] == CLEAN_RECORD
    assert b.locate() == want


def test_padding_of_the_short_chunk_cannot_be_named(gctx, km):
    """A parity corruption whose syndrome is proportional to the short
    chunk's column: past that chunk's length it is NO_SHARD (zero padding is
    not stored, so it cannot be corrupt); below it, it is indistinguishable
    from a corruption of the chunk and names it."""
    b = Uniform(gctx, *km, 2600 + km[1])
    k, m = km
    M = oracle.matrix(k, m)[k:]
    j = k - 1
    for o, x, e in ((0, SHORT, 0x37), (2, S - 1, 0x01), (3, SHORT + 4096, 0xFF), (4, SHORT - 1, 0x37)):
        for i in range(m):
            b.t[o, k + i, x] ^= oracle.gf_mul(int(M[i, j]), e)
    want = b.expected()
    assert want[0] == (SHORT, 1, NO_SHARD, NO_SHARD) and want[2] == (S - 1, 1, NO_SHARD, NO_SHARD)
    assert want[3] == (SHORT + 4096, 1, NO_SHARD, NO_SHARD)
    assert want[4] == (SHORT - 1, 1, j, j)
    assert want[1] == CLEAN_RECORD and want[5] == CLEAN_RECORD
    assert b.locate() == want


# ---- grouped and unaligned forms -----------------------------------------------------

class Mixed:
    """One device buffer per object of (k, m, size, dl), shard slots `off`
    bytes into 256-byte aligned rows (off != 0: the byte-exact edge kernel),
    encoded by the library."""

    def __init__(self, ctx, objs, seed, off=0):
        torch = _torch()
        self.ctx, self.objs, self.off = ctx, objs, off
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.t, self.dptr, self.pptr, self.dlen = [], [], [], []
        for (k, m, size, dl) in objs:
            t = torch.randint(0, 256, (k + m, _round(size + 16)), dtype=torch.uint8, device="cuda", generator=g)
            self.t.append(t)
            self.dptr += [t[j].data_ptr() + off for j in range(k)]
            self.pptr += [t[k + i].data_ptr() + off for i in range(m)]
            self.dlen += dl
        self.shapes = [(k, m, size) for (k, m, size, _) in objs]
        self.out = torch.zeros(len(objs) * REC.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.encode_batch_device(self.shapes, self.dptr, self.pptr, data_len=self.dlen)
        torch.cuda.synchronize()

    def locate(self):
        torch = _torch()
        self.out.fill_(0x55)
        torch.cuda.synchronize()
        self.ctx.locate_batch_device(self.shapes, self.dptr, self.pptr, self.out.data_ptr(), data_len=self.dlen)
        torch.cuda.synchronize()
        return _records(self.out)

    def expected(self):
        out = []
        for (k, m, size, dl), t in zip(self.objs, self.t):
            h = t.cpu().numpy()[:, self.off:self.off + size]
            out.append(locate_ref.locate(h, k, m, size, dl))
        return out


def _mixed_objects():
    """(k, m, S) that share m and that do not, two k per m (two tables in
    one launch), sizes that are no tile multiple, short last chunks."""
    return [(4, 2, 3 * 16384 + 999, [3 * 16384 + 999] * 3 + [40000]),
            (10, 4, 16384 + 17, [16384 + 17] * 9 + [1]),
            (7, 2, 5 * 4096 + 1, [5 * 4096 + 1] * 6 + [5 * 4096]),
            (4, 2, 70001, [70001] * 4),
            (6, 8, 2 * 8192 + 4095, [2 * 8192 + 4095] * 5 + [8192]),
            (3, 4, 12345, [12345] * 2 + [12000]),
            (1, 2, 9000, [8000]),
            (5, 3, 4096, [4096] * 5)]


def _damage(b):
    """One finding per object kind: data shard, parity shard, two shards, padding, clean."""
    objs = b.objs
    o = b.off
    assert [s[:2] for s in objs] == [(4, 2), (10, 4), (7, 2), (4, 2), (6, 8), (3, 4), (1, 2), (5, 3)]
    b.t[0][2, o + 40000] ^= 0x01                                             # data shard 2
    b.t[1][10 + 3, o + 16384 + 16] ^= 0x80                                  # last parity shard, last byte
    b.t[2][6, o + 5 * 4096 - 1] ^= 0x7F                                      # the short chunk's last byte
    b.t[4][0, o + 8191] ^= 0x10
    b.t[4][6 + 7, o + 8192] ^= 0x10                                          # two shards: MANY
    b.t[5][1, o + 12344] ^= 0xFF                                             # data shard 1, last byte
    b.t[6][0, o + 7999] ^= 0x02                                              # k = 1
    for i in range(3):                                                       # shaped like shard 4, all columns: still shard 4
        b.t[7][5 + i, o + 77] ^= oracle.gf_mul(int(oracle.matrix(5, 3)[5 + i, 4]), 0x99)


def test_batch_device_mixed_shapes(gctx):
    b = Mixed(gctx, _mixed_objects(), 2700)
    clean = [CLEAN_RECORD] * len(b.objs)
    assert b.expected() == clean and b.locate() == clean
    _damage(b)
    want = b.expected()
    assert [locate_ref.outcome(r) for r in want] == [(ONE, 2), (ONE, 13), (ONE, 6), (CLEAN, None), (MANY, None),
                                                     (ONE, 1), (ONE, 0), (ONE, 4)]
    assert b.locate() == want


@pytest.mark.parametrize("off", [1])
def test_unaligned_pointers_take_the_edge_kernel(gctx, off):
    b = Mixed(gctx, _mixed_objects(), 2800, off=off)
    clean = [CLEAN_RECORD] * len(b.objs)
    assert b.expected() == clean and b.locate() == clean
    # Garbage around every slot and past the short chunks' lengths: not read.
    for (k, m, size, dl), t in zip(b.objs, b.t):
        t[:, :off] = 0xEE
        t[:, off + size:] = 0xEE
        t[k - 1, off + dl[-1]:] = 0xEE
    assert b.locate() == clean
    _damage(b)
    want = b.expected()
    assert [locate_ref.outcome(r)[0] for r in want] == [ONE, ONE, ONE, CLEAN, MANY, ONE, ONE, ONE]
    assert b.locate() == want


def test_unaligned_whole_shard_and_padding(gctx):
    """The edge kernel's slow path over a whole shard, and its length rule."""
    torch = _torch()
    k, m, size = 4, 3, 2 * 16384 + 4096 + 7
    short = size - 3000
    b = Mixed(gctx, [(k, m, size, [size] * 3 + [short])] * 3, 2900, off=1)
    g = torch.Generator(device="cuda").manual_seed(5)
    b.t[0][1, 1:1 + size] = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda", generator=g)
    M = oracle.matrix(k, m)[k:]
    for i in range(m):
        b.t[2][k + i, 1 + short] ^= oracle.gf_mul(int(M[i, k - 1]), 0x42)
    want = b.expected()
    assert locate_ref.outcome(want[0]) == (ONE, 1) and want[0][1] > size * 0.99
    assert want[1] == CLEAN_RECORD and want[2] == (short, 1, NO_SHARD, NO_SHARD)
    assert b.locate() == want


# ---- host form -----------------------------------------------------------------------

def _host_object(seed, k=4, m=2, size=100, last=50):
    rng = np.random.default_rng(seed)
    data = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(k - 1)] + [rng.integers(0, 256, last, dtype=np.uint8)]
    return data, oracle.encode(data, m, size)


def _host_rows(data, par, size):
    rows = np.zeros((len(data) + len(par), size), np.uint8)
    for j, d in enumerate(data):
        rows[j, :d.size] = d
    for i, p in enumerate(par):
        rows[len(data) + i] = p
    return rows


def test_host_locate_4_2_100(ctx):
    """The reference's own test shape: 350 B -> 4 + 2 chunks of 100."""
    data, par = _host_object(3000)
    dl = [d.size for d in data]

    def both():
        r = ctx.locate(data, par, 100)
        rec = (r["first_bad"], r["n_bad"], r["shard_min"], r["shard_max"])
        assert rec == locate_ref.locate(_host_rows(data, par, 100), 4, 2, 100, dl)
        assert (r["outcome"], r["shard"]) == locate_ref.outcome(rec)
        return r

    assert both()["outcome"] == CLEAN
    for c, x in ((0, 0), (3, 49), (4, 99), (5, 16), (1, 63)):
        buf = data[c] if c < 4 else par[c - 4]
        buf[x] ^= 0x11
        r = both()
        assert (r["outcome"], r["shard"], r["first_bad"], r["n_bad"]) == (ONE, c, x, 1)
        buf[x] ^= 0x11
    data[0][7] ^= 1
    par[1][70] ^= 1
    assert both()["outcome"] == MANY


def test_reed_solomon_locate(ctx):
    import maxio_amd

    rng = np.random.default_rng(3001)
    rs = maxio_amd.ReedSolomon(4, 2, ctx)
    shards = [bytearray(rng.integers(0, 256, 20000, dtype=np.uint8).tobytes()) for _ in range(4)]
    shards += [bytearray(20000), bytearray(20000)]
    rs.encode(shards)
    assert rs.locate(shards)["outcome"] == CLEAN
    shards[2][19999] ^= 0x80
    r = rs.locate(shards)
    assert (r["outcome"], r["shard"], r["first_bad"], r["n_bad"]) == (ONE, 2, 19999, 1)


def test_error_codes(ctx):
    """m = 0 is the crate's error; one parity row cannot locate and more than
    eight do not fit one row block.  Decided before anything is enqueued: the
    device forms are given pointers no kernel could read."""
    import maxio_amd

    d = np.zeros(100, np.uint8)
    for m, name in ((0, "TooFewParityShards"), (1, None), (9, None)):
        with pytest.raises(maxio_amd.RSError) as e:
            ctx.locate([d, d], [d] * m, 100)
        assert (e.value.name == name) if name else (e.value.code == -21), (m, e.value)
        with pytest.raises(maxio_amd.RSError) as e:
            ctx.locate_strided_device(2, m, 100, 1, 16, 4096, 256, 16, 4096, 256, 16)
        assert (e.value.name == name) if name else (e.value.code == -21), (m, e.value)
        with pytest.raises(maxio_amd.RSError) as e:
            ctx.locate_batch_device([(2, 2, 100), (2, m, 100)], [16] * 4, [16] * (2 + m), 16)
        assert (e.value.name == name) if name else (e.value.code == -21), (m, e.value)
