"""GPU: mxec_encode_update_strided_device, the seeded parity pass
(rs_kernel.hip kSeed, rs_update_fast / rs_update_edge): parity_out =
parity_in ^ M(k, m)[:, first .. first + count) * data window.

Oracle: oracle.encode (the crate's algorithm on the CPU), bit-exact.  The
parity of the data with the not-yet-folded shards zeroed is, by linearity,
the XOR of oracle.encode over each folded shard alone; those per-shard
parities are computed once per shape and shared.

The running parity a streaming PUT keeps (filesystem.rs:1121-1124 computes it
only once every chunk is on disk; this call replaces nothing in the crate)."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import oracle
from maxio_amd import _native as N

pytestmark = pytest.mark.gpu

N_OBJ, K = 3, 10
# One m per row-count template the uniform encode instantiates (R = 1..8, V by
# r_total), and m = 10: two row blocks (8 + 2) at the two-vector geometry.
MS = (1, 2, 3, 4, 5, 6, 7, 8, 10)
# 36 917: two whole 16 KiB tiles, a cut tile and an odd tail; 16 384: exactly
# one tile, nothing cut; 8 192 + 16; 1.
SIZES = (36917, 16384, 8192 + 16, 1)
PARTS = {
    "whole": [(0, 10)],
    "1-4-5": [(0, 1), (1, 4), (5, 5)],
    "singles": [(j, 1) for j in range(10)],
    "3-7-last-first": [(3, 7), (0, 3)],
}
FILL = 0xEE
OK, E_FEW_DATA, E_FEW_PARITY, E_EMPTY, E_255, E_ARG = 0, -3, -5, -11, -20, -21


def pitch_of(S):
    return (S + 255) // 256 * 256 + 256


@functools.lru_cache(maxsize=None)
def shape(m, S, last=None):
    """Data of N_OBJ objects and, per object and data shard, the parity of
    that shard alone ([o][j] -> (m, S) uint8).  last: the last shard's length."""
    rng = np.random.default_rng(9000 + 131 * m + S + 7 * (last or 0))
    data = rng.integers(0, 256, (N_OBJ, K, S), dtype=np.uint8)
    zero = np.zeros(S, np.uint8)

    def shard(o, j):  # the device keeps random bytes past `last`: they must not be read
        return data[o, j, :last] if last is not None and j == K - 1 else data[o, j]

    alone = [[np.stack(oracle.encode([shard(o, j) if i == j else zero for i in range(K)], m, S)) for j in range(K)]
             for o in range(N_OBJ)]
    full = [np.stack(oracle.encode([shard(o, j) for j in range(K)], m, S)) for o in range(N_OBJ)]
    for o in range(N_OBJ):  # the linearity this file leans on, against the oracle itself
        acc = np.zeros((m, S), np.uint8)
        for j in range(K):
            acc ^= alone[o][j]
        assert np.array_equal(acc, full[o])
    data.setflags(write=False)
    return data, alone, full


class Mem:
    """Device rows: data [N_OBJ][K][pitch], two parity sets [N_OBJ][m][pitch], each
    `off` bytes into its allocation, everything past a row's S bytes FILL."""

    def __init__(self, data, m, S, off=0):
        import torch

        self.torch, self.m, self.S, self.off, self.pitch = torch, m, S, off, pitch_of(S)
        host = np.full((N_OBJ, K, self.pitch), FILL, np.uint8)
        host[:, :, :S] = data
        self.d = self._up(host)
        self.par = [self._up(np.full((N_OBJ, m, self.pitch), FILL, np.uint8)) for _ in range(2)]

    def _up(self, a):
        t = self.torch.full((a.size + 16,), FILL, dtype=self.torch.uint8, device="cuda")
        t[self.off:self.off + a.size] = self.torch.from_numpy(a.reshape(-1)).cuda()
        self.torch.cuda.synchronize()
        return t

    def data_ptr(self, first):
        return self.d.data_ptr() + self.off + first * self.pitch

    def par_ptr(self, which):
        return self.par[which].data_ptr() + self.off

    def rows(self, which):
        self.torch.cuda.synchronize()
        n = N_OBJ * self.m * self.pitch
        return self.par[which][self.off:self.off + n].cpu().numpy().reshape(N_OBJ, self.m, self.pitch)

    def update(self, ctx, first, count, src, dst, data_len=None):
        """src: a parity set index, or None for parity_in = NULL."""
        ctx.encode_update_strided_device(
            K, self.m, self.S, N_OBJ, first, count, self.data_ptr(first), K * self.pitch, self.pitch,
            None if src is None else self.par_ptr(src), self.m * self.pitch, self.pitch,
            self.par_ptr(dst), self.m * self.pitch, self.pitch, data_len=data_len)


def want_after(alone, m, S, folded):
    out = np.zeros((N_OBJ, m, S), np.uint8)
    for o in range(N_OBJ):
        for j in folded:
            out[o] ^= alone[o][j]
    return out


def run_partition(ctx, m, S, parts, off=0, last=None):
    """Folds the windows in order, ping-ponging; after every step the rows
    equal the oracle's parity of the shards folded so far, and the bytes past
    S in every row are untouched."""
    data, alone, full = shape(m, S, last)
    mem = Mem(data, m, S, off)
    folded, src = [], None
    for first, count in parts:
        dst = 0 if src != 0 else 1
        dl = None
        if last is not None:
            dl = [last if first + i == K - 1 else S for i in range(count)]
        mem.update(ctx, first, count, src, dst, data_len=dl)
        folded += list(range(first, first + count))
        got = mem.rows(dst)
        assert np.array_equal(got[:, :, :S], want_after(alone, m, S, folded)), (first, count)
        assert (got[:, :, S:] == FILL).all(), "wrote past the shard size"
        src = dst
    assert sorted(folded) == list(range(K))
    assert np.array_equal(mem.rows(src)[:, :, :S], np.stack(full))


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("m", MS)
def test_window_partitions(ctx, m, S):
    for name, parts in PARTS.items():
        run_partition(ctx, m, S, parts)


# data_len ending inside a tile, exactly on a tile boundary (16 KiB and 8 KiB
# tiles both), and at 1; the short shard's window is folded on its own.
@pytest.mark.parametrize("last", (20000, 16384, 1))
@pytest.mark.parametrize("m", (2, 4, 6, 10))
def test_short_last_shard(ctx, m, last):
    run_partition(ctx, m, 36917, [(0, 9), (9, 1)], last=last)
    run_partition(ctx, m, 36917, [(9, 1), (0, 9)], last=last)


@pytest.mark.parametrize("m", MS)
def test_unaligned_pointers_take_the_edge_kernel(ctx, m):
    for name, parts in PARTS.items():
        run_partition(ctx, m, 36917, parts, off=1)
    run_partition(ctx, m, 36917, [(0, 9), (9, 1)], off=1, last=20000)


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("m", (2, 4, 8, 10))
def test_grid_cap_walks_many_tiles_per_workgroup(ctx_with, m, off):
    c = ctx_with(MXEC_TEST_RS_GRID=2)
    run_partition(c, m, 36917, PARTS["1-4-5"], off=off)
    run_partition(c, m, 36917, [(0, 9), (9, 1)], off=off, last=20000)


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("m", (3, 10))
def test_idempotent_and_parity_in_untouched(ctx, m, off):
    S = 36917
    data, alone, full = shape(m, S)
    mem = Mem(data, m, S, off)
    mem.update(ctx, 0, 4, None, 0)
    seed = mem.rows(0).copy()
    mem.update(ctx, 4, 6, 0, 1)
    once = mem.rows(1).copy()
    mem.update(ctx, 4, 6, 0, 1)
    assert np.array_equal(mem.rows(1), once)
    assert np.array_equal(mem.rows(0), seed)
    assert np.array_equal(once[:, :, :S], np.stack(full))


@pytest.mark.parametrize("m", (2, 5, 10))
@pytest.mark.parametrize("S", (36917, 1))
def test_null_parity_in_is_a_zero_seed(ctx, m, S):
    import torch

    data, alone, full = shape(m, S)
    mem = Mem(data, m, S)
    mem.update(ctx, 2, 5, None, 1)
    from_null = mem.rows(1).copy()
    mem.par[0].zero_()
    mem.par[1].fill_(FILL)
    torch.cuda.synchronize()
    mem.update(ctx, 2, 5, 0, 1)
    assert np.array_equal(mem.rows(1), from_null)
    assert np.array_equal(from_null[:, :, :S], want_after(alone, m, S, range(2, 7)))


# ---- errors: all decided before anything is enqueued ------------------------------------------

def _call(ctx, mem, **over):
    a = dict(k=K, m=mem.m, S=mem.S, n_obj=N_OBJ, first=2, count=3, data=mem.data_ptr(2),
             pin=mem.par_ptr(0), pout=mem.par_ptr(1), dev=0)
    a.update(over)
    P = mem.pitch
    return N.lib().mxec_encode_update_strided_device(
        ctx.handle, a["dev"], None, a["k"], a["m"], a["S"], a["n_obj"], a["first"], a["count"], a["data"], K * P, P,
        None, a["pin"], a["m"] * P, P, a["pout"], a["m"] * P, P)


ERRORS = [
    ("k=0", dict(k=0, first=0, count=0), E_FEW_DATA),
    ("m=0", dict(m=0), E_FEW_PARITY),
    ("k+m=256", dict(k=250, m=6), E_255),
    ("shard_size=0", dict(S=0), E_EMPTY),
    ("first<0", dict(first=-1), E_ARG),
    ("count=0", dict(count=0), E_ARG),
    ("count<0", dict(count=-1), E_ARG),
    ("first+count>k", dict(first=8, count=3), E_ARG),
    ("first=k", dict(first=K, count=1), E_ARG),
    ("null-data", dict(data=None), E_ARG),
    ("null-parity_out", dict(pout=None), E_ARG),
    ("in==out", dict(pin="out"), E_ARG),
    ("in-overlaps-out-by-one-byte", dict(pin="out+S-1"), E_ARG),
    ("out-row-inside-in-extent", dict(pin="out-pitch+1"), E_ARG),
    ("dev=count", dict(dev=-1), E_ARG),
]


@pytest.mark.parametrize("name,over,code", ERRORS, ids=[e[0] for e in ERRORS])
def test_error_table(ctx, name, over, code):
    import torch

    m, S = 3, 8192 + 16
    data, _, _ = shape(m, S)
    mem = Mem(data, m, S)
    over = dict(over)
    if isinstance(over.get("pin"), str):
        over["pin"] = mem.par_ptr(1) + {"out": 0, "out+S-1": S - 1, "out-pitch+1": 1 - mem.pitch}[over["pin"]]
    if over.get("dev") == -1:
        over["dev"] = len(ctx.device_ids())
    before = mem.rows(1).copy()
    assert _call(ctx, mem, **over) == code, N.lib().mxec_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(mem.rows(1), before), "an error enqueued work"


def test_adjacent_rows_do_not_count_as_overlap(ctx):
    """in and out interleaved row by row, S bytes each, touching but sharing no byte."""
    import torch

    m, S = 2, 4096
    data, alone, full = shape(m, S)
    mem = Mem(data, m, S)
    buf = torch.zeros(N_OBJ * m * 2 * S + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    base, P = buf.data_ptr(), mem.pitch
    rc = N.lib().mxec_encode_update_strided_device(
        ctx.handle, 0, None, K, m, S, N_OBJ, 0, K, mem.data_ptr(0), K * P, P, None,
        base, m * 2 * S, 2 * S, base + S, m * 2 * S, 2 * S)
    assert rc == OK, N.lib().mxec_last_error()
    torch.cuda.synchronize()
    got = buf[:N_OBJ * m * 2 * S].cpu().numpy().reshape(N_OBJ, m, 2, S)
    assert np.array_equal(got[:, :, 1], np.stack(full)) and not got[:, :, 0].any()
