"""GPU: ReedSolomon::verify on the device (mxec_verify, mxec_verify_strided_device,
mxec_verify_batch_device; rs_kernel.hip rs_verify_fast / rs_verify_edge).

The kernel recomputes the parity like the encode does and compares it with
the stored parity instead of storing it; a row's result is the lowest byte
offset at which the two differ, or VERIFY_OK.  Every expectation here comes
from the oracle and a numpy compare of the bytes as they stand on the device:

    want = oracle.encode(data, m, S)
    first_bad = np.flatnonzero(want[i] != stored[i])[0]   (VERIFY_OK if none)

Shapes are test_grid_stride_gpu.py's: S = 5 * 16384 + 4096 + 48 (6 tiles at
V = 4, 11 at V = 2, the last one cut), 6 objects, shard pitch rounded to 256,
a short last data chunk, and contexts capped at 7 and 61 workgroups so that
each workgroup walks many tiles across object boundaries.

Reference: the crate's ReedSolomon::verify (reed-solomon-erasure 6.0.0),
which MaxIO never calls -- it has no scrubber.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

GRIDS = [7, 61]
OK = (1 << 64) - 1
K_OF = {1: 3, 2: 4, 3: 5, 4: 8, 5: 4, 6: 10, 7: 2, 8: 6, 12: 9}  # test_grid_stride_gpu.py's k per m
S = 5 * 16384 + 4096 + 48
N = 6
SHORT = S - 5000


def _torch():
    import torch

    return torch


def _round(x, a=256):
    return (x + a - 1) // a * a


@pytest.fixture(params=GRIDS, ids=lambda g: f"grid{g}")
def gctx(request, ctx_with):
    return ctx_with(MXEC_TEST_RS_GRID=request.param)


def _expected(h, k, m, size, dl):
    """first_bad of one object from its host copy h[k + m][>= size]."""
    want = oracle.encode([h[j, :dl[j]] for j in range(k)], m, size)
    out = []
    for i in range(m):
        d = np.flatnonzero(want[i] != h[k + i, :size])
        out.append(int(d[0]) if d.size else OK)
    return out


class Uniform:
    """N objects of (k, m, S) in one tensor, encoded by the library."""

    def __init__(self, ctx, m, seed):
        torch = _torch()
        self.ctx, self.m, self.k = ctx, m, K_OF[m]
        self.Sp = _round(S)
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.t = torch.randint(0, 256, (N, self.k + m, self.Sp), dtype=torch.uint8, device="cuda", generator=g)
        self.dl = [S] * (self.k - 1) + [SHORT]
        self.fb = torch.zeros(N * m, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        k, Sp, t = self.k, self.Sp, self.t
        ctx.encode_strided_device(k, m, S, N, t.data_ptr(), (k + m) * Sp, Sp, t.data_ptr() + k * Sp,
                                  (k + m) * Sp, Sp, data_len=self.dl)
        torch.cuda.synchronize()

    def verify(self):
        torch = _torch()
        k, m, Sp, t = self.k, self.m, self.Sp, self.t
        self.fb.fill_(0x55)  # the call fills the entries itself
        torch.cuda.synchronize()
        self.ctx.verify_strided_device(k, m, S, N, t.data_ptr(), (k + m) * Sp, Sp, t.data_ptr() + k * Sp,
                                       (k + m) * Sp, Sp, self.fb.data_ptr(), data_len=self.dl)
        torch.cuda.synchronize()
        return self.fb.cpu().numpy().view(np.uint64).reshape(N, m).tolist()

    def expected(self):
        h = self.t.cpu().numpy()
        return [_expected(h[o], self.k, self.m, S, self.dl) for o in range(N)]


MS = [1, 2, 3, 4, 5, 6, 7, 8, 12]


@pytest.mark.parametrize("m", MS)
def test_clean_batch_and_garbage_past_the_lengths(gctx, m):
    b = Uniform(gctx, m, 1000 + m)
    assert b.expected() == [[OK] * m] * N  # the encode is the oracle's
    assert b.verify() == [[OK] * m] * N
    # Nothing past a length is read: the short chunk's tail and the pitch
    # padding of every shard, parity included, hold garbage.
    b.t[:, b.k - 1, SHORT:] = 0xC3
    b.t[:, :, S:] = 0x3C
    assert b.verify() == [[OK] * m] * N


# Vector edge, lane block, tile edges at V = 2 and V = 4, inside the cut last
# tile, the last byte.
OFFSETS = [0, 15, 16, 4095, 4096, 8191, 8192, 16383, 16384, 5 * 16384 + 4096 + 17, S - 1]


@pytest.mark.parametrize("m", MS)
def test_one_flipped_parity_byte(gctx, m):
    b = Uniform(gctx, m, 1100 + m)
    for n, x in enumerate(OFFSETS):
        o, i = (n * 5 + 1) % N, (n * 3 + m - 1) % m
        b.t[o, b.k + i, x] ^= 0x40
        want = [[OK] * m for _ in range(N)]
        want[o][i] = x
        assert b.verify() == want, (m, o, i, x)
        b.t[o, b.k + i, x] ^= 0x40
    assert b.expected() == [[OK] * m] * N  # every flip undone


@pytest.mark.parametrize("m", MS)
def test_flipped_data_byte_shows_in_every_row(gctx, m):
    """Every coefficient of the parity matrix is non-zero, so a data byte at
    x changes byte x of every parity row."""
    b = Uniform(gctx, m, 1200 + m)
    for o, j, x in [(1, 0, 4097), (4, b.k - 1, SHORT - 1), (5, b.k // 2, S - 1 if b.k > 2 else 0)]:
        b.t[o, j, x] ^= 0x01
    want = b.expected()
    assert want[1] == [4097] * m and want[4] == [SHORT - 1] * m and want[0] == [OK] * m
    assert b.verify() == want


@pytest.mark.parametrize("m", MS)
def test_two_flips_in_one_row_report_the_lower(gctx, m):
    """The reduction is a min across workgroups: the flip in the later tile
    is made first, and both are in place when the kernel runs."""
    b = Uniform(gctx, m, 1300 + m)
    o, i = 3, m - 1
    b.t[o, b.k + i, 4 * 16384 + 100] ^= 0x80
    b.t[o, b.k + i, 16384 + 5] ^= 0x80
    b.t[2, b.k, S - 1] ^= 0x02
    b.t[2, b.k, 8192 + 4096 + 33] ^= 0x02
    want = b.expected()
    assert want[o][i] == 16384 + 5 and want[2][0] == 8192 + 4096 + 33
    assert b.verify() == want


# ---- grouped form ---------------------------------------------------------------

def _mixed_objects(rng, ms, n_per=3):
    """test_grid_stride_gpu.py's shapes: (k, m, S, dl) per object."""
    objs = []
    for m in ms:
        for _ in range(n_per):
            k = int(rng.integers(1, 11))
            size = int(rng.integers(3, 40)) * 4096 + int(rng.integers(0, 4096))
            last = int(rng.integers(1, size + 1))
            objs.append((k, m, size, [size] * (k - 1) + [last]))
    return objs


class Mixed:
    """One device buffer per object, shard slots `off` bytes into 256-byte
    aligned rows (off = 0: aligned; data_off / parity_off != 0: the byte-exact
    edge kernel), encoded by the library."""

    def __init__(self, ctx, objs, seed, data_off=0, parity_off=0):
        torch = _torch()
        self.ctx, self.objs, self.doff, self.poff = ctx, objs, data_off, parity_off
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.t, self.dptr, self.pptr, self.dlen = [], [], [], []
        for (k, m, size, dl) in objs:
            t = torch.randint(0, 256, (k + m, _round(size + 16)), dtype=torch.uint8, device="cuda", generator=g)
            self.t.append(t)
            self.dptr += [t[j].data_ptr() + data_off for j in range(k)]
            self.pptr += [t[k + i].data_ptr() + parity_off for i in range(m)]
            self.dlen += dl
        self.shapes = [(k, m, size) for (k, m, size, _) in objs]
        self.fb = torch.zeros(sum(m for (_, m, _, _) in objs), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.encode_batch_device(self.shapes, self.dptr, self.pptr, data_len=self.dlen)
        torch.cuda.synchronize()

    def verify(self):
        torch = _torch()
        self.fb.fill_(0x55)
        torch.cuda.synchronize()
        self.ctx.verify_batch_device(self.shapes, self.dptr, self.pptr, self.fb.data_ptr(), data_len=self.dlen)
        torch.cuda.synchronize()
        flat = self.fb.cpu().numpy().view(np.uint64).tolist()
        out, at = [], 0
        for (_, m, _, _) in self.objs:
            out.append(flat[at:at + m])
            at += m
        return out

    def expected(self):
        out = []
        for (k, m, size, dl), t in zip(self.objs, self.t):
            h = t.cpu().numpy()
            rows = np.stack([h[j, self.doff:self.doff + size] for j in range(k)] +
                            [h[k + i, self.poff:self.poff + size] for i in range(m)])
            out.append(_expected(rows, k, m, size, dl))
        return out


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6, 7, 8])
def test_grouped_one_corrupt_object_among_clean_neighbours(gctx, m):
    b = Mixed(gctx, _mixed_objects(np.random.default_rng(1400 + m), [m], n_per=5), 1500 + m)
    clean = [[OK] * m] * len(b.objs)
    assert b.expected() == clean and b.verify() == clean
    k, _, size, dl = b.objs[2]
    x = size - 1 - (m * 977) % min(size, 9000)
    b.t[2][k + m - 1, x] ^= 0x10
    want = [[OK] * m for _ in b.objs]
    want[2][m - 1] = x
    assert b.expected() == want and b.verify() == want
    b.t[2][k + m - 1, x] ^= 0x10
    y = dl[-1] - 1  # the last byte of the short chunk: all rows
    b.t[2][k - 1, y] ^= 0x01
    want[2] = [y] * m
    assert b.expected() == want and b.verify() == want


def test_mixed_m_in_one_call(gctx):
    """Several m in one call: one launch per m, results object-major."""
    rng = np.random.default_rng(1600)
    objs = _mixed_objects(rng, [1, 2, 3, 4, 6], n_per=2)
    b = Mixed(gctx, [objs[i] for i in rng.permutation(len(objs))], 1601)
    for o in (0, 3, 7):
        k, m, size, _ = b.objs[o]
        b.t[o][k + (o % m), (o * 4099) % size] ^= 0x04
    want = b.expected()
    assert sum(v != OK for row in want for v in row) == 3
    assert b.verify() == want


# ---- unaligned form ---------------------------------------------------------------

@pytest.mark.parametrize("which", ["data", "parity", "both"])
@pytest.mark.parametrize("off", [1, 7])
def test_unaligned_pointers_take_the_byte_exact_kernel(gctx, off, which):
    size = 3 * 16384 + 999
    objs = [(k, m, size, [size] * (k - 1) + [size - 123]) for (k, m) in [(4, 2), (10, 4), (3, 12)] for _ in range(3)]
    b = Mixed(gctx, objs, 1700 + off, data_off=off if which != "parity" else 0,
              parity_off=off if which != "data" else 0)
    clean = [[OK] * m for (_, m, _, _) in objs]
    assert b.expected() == clean and b.verify() == clean
    # Garbage around every slot and past the short chunk's length: not read.
    for (k, m, _, dl), t in zip(objs, b.t):
        t[:k, :b.doff] = 0xEE
        t[:k, b.doff + size:] = 0xEE
        t[k - 1, b.doff + dl[-1]:] = 0xEE
        t[k:, :b.poff] = 0xEE
        t[k:, b.poff + size:] = 0xEE
    assert b.expected() == clean and b.verify() == clean
    want = [list(r) for r in clean]
    for (o, i, x) in [(0, 0, 0), (1, 1, 17), (4, 3, size - 1), (5, 0, 4096 * 5 + 15), (7, 11, 16384)]:
        b.t[o][objs[o][0] + i, b.poff + x] ^= 0x20
        want[o][i] = x
    assert b.expected() == want and b.verify() == want
    o, j, x = 8, 2, size - 123 - 1  # the short chunk's last byte: every row of that object
    b.t[o][j, b.doff + x] ^= 0x01
    want[o] = [x] * 12
    assert b.expected() == want and b.verify() == want


# ---- host form ----------------------------------------------------------------------

def test_host_verify_k1_parity_rows_are_copies(ctx):
    rng = np.random.default_rng(1800)
    d = rng.integers(0, 256, 70001, dtype=np.uint8)
    par = oracle.encode([d], 2, d.size)
    assert np.array_equal(par[0], d) and np.array_equal(par[1], d)
    assert ctx.verify([d], par, d.size) == (True, [OK, OK])
    par[1][12345] ^= 1
    assert ctx.verify([d], par, d.size) == (False, [OK, 12345])


def test_host_verify_4_2_short_last_chunk(ctx):
    rng = np.random.default_rng(1801)
    size = 20000
    data = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(3)] + [rng.integers(0, 256, 777, dtype=np.uint8)]
    par = oracle.encode(data, 2, size)
    assert ctx.verify(data, par, size) == (True, [OK, OK])
    par[0][size - 1] ^= 0x80
    par[1][16] ^= 0x80
    par[1][19999] ^= 0x80
    assert ctx.verify(data, par, size) == (False, [size - 1, 16])
    par = oracle.encode(data, 2, size)
    data[3][776] ^= 1
    assert ctx.verify(data, par, size) == (False, [776, 776])


def test_host_verify_m0_is_the_crates_error(ctx):
    import maxio_amd

    d = np.zeros(100, np.uint8)
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.verify([d, d], [], 100)
    assert e.value.name == "TooFewParityShards"


def test_reed_solomon_verify_true_and_false(ctx):
    import maxio_amd

    rng = np.random.default_rng(1802)
    rs = maxio_amd.ReedSolomon(4, 2, ctx)
    shards = [bytearray(rng.integers(0, 256, 20000, dtype=np.uint8).tobytes()) for _ in range(4)]
    shards += [bytearray(20000), bytearray(20000)]
    rs.encode(shards)
    assert [bytes(s) for s in shards[4:]] == [p.tobytes() for p in oracle.encode(shards[:4], 2, 20000)]
    assert rs.verify(shards) is True
    shards[5][0] ^= 1
    assert rs.verify(shards) is False
    shards[5][0] ^= 1
    shards[1][19999] ^= 1
    assert rs.verify(shards) is False


# ---- enqueue-only, on the caller's stream -----------------------------------------------

def test_device_forms_enqueue_on_the_callers_stream(ctx):
    """The verify is queued behind work already on the caller's stream and
    the call returns while that work still runs: a flip made by a kernel
    queued on the stream just before the call is seen, and only by the
    stream's verify."""
    torch = _torch()
    b = Uniform(ctx, 2, 1900)
    k, m, Sp, t = b.k, b.m, b.Sp, b.t
    st = torch.cuda.Stream()
    busy = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
    x = 3 * 16384 + 9
    fb2 = torch.zeros(sum([m] * N), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for _ in range(200):  # ~0.5 GB of traffic each: the stream stays busy for tens of ms
            busy.add_(1.0)
        t[4, k + 1, x] ^= 0x08
    ctx.verify_strided_device(k, m, S, N, t.data_ptr(), (k + m) * Sp, Sp, t.data_ptr() + k * Sp,
                              (k + m) * Sp, Sp, b.fb.data_ptr(), data_len=b.dl, stream=st.cuda_stream)
    ctx.verify_batch_device([(k, m, S)] * N, [t[o, j].data_ptr() for o in range(N) for j in range(k)],
                            [t[o, k + i].data_ptr() for o in range(N) for i in range(m)], fb2.data_ptr(),
                            data_len=b.dl * N, stream=st.cuda_stream)
    returned_early = not st.query()
    torch.cuda.synchronize()
    want = [[OK] * m for _ in range(N)]
    want[4][1] = x
    assert b.fb.cpu().numpy().view(np.uint64).reshape(N, m).tolist() == want
    assert fb2.cpu().numpy().view(np.uint64).reshape(N, m).tolist() == want
    assert returned_early, "the calls waited for the stream"
