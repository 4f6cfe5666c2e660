"""GPU: wide stripes (k > 64) through every device-resident RS pass.

k = ceil(body / chunk_size) grows with the object, and the reference only
stops at k + m > 255 (filesystem.rs:1095), so a stripe of two hundred shards
is the ordinary big object.  Everything indexed by k runs here with more than
six bits of it, and above 127 with its top bit set: the tile body's 4-wide k
loop and its tail (rs_kernel.hip rs_tile, tab + j * stride * 8), the seeded
pass's table offset by the window's `first`, the locate's ratio -> j byte
table (locate_plan.hpp, 0xFF = none) and il[j], the decode keys and the
k x k host inversion, descriptor tables of hundreds of entries and decode
tables of tens of KiB in the coefficient arena.

Oracle: oracle.compute_parity / encode / reconstruct / matrix (the crate's
algorithm on the CPU) and tests/locate_ref.py, bit-exact; the original bytes
where a pass rebuilds them.  The host algebra alone is pinned on the CPU by
tests/c_manifest/gf256_check.cpp, so a failure here that passes there is the
kernel's.

Geometry (test_encode_update_gpu.py's): S = 36 917 -- two whole tiles, a cut
tile and an odd tail at 16 KiB and at 8 KiB tiles -- 3 objects per shape in
one buffer [3][k + m][pitch], pitch = S rounded up to 256 plus 256, the last
data shard 5 000 bytes short, every byte past a row's length FILL.  A pass
is checked by comparing the whole buffer with its expected image, so what it
must not touch (present shards, the fill, the bytes past a short shard's
length) is checked with what it must write.  (243, 12) is 28.6 MB.

The 256-shard reconstruct contract (include/maxio_ec.h mxec_reconstruct) is
pinned at the end of the file."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import locate_ref
import oracle
from locate_ref import CLEAN_RECORD

pytestmark = pytest.mark.gpu

# Every k mod 4 (the loop tail), both sides of 128, k + m = 255, row templates
# R = 1, 2, 3, 4, 5 and 8, both vector geometries (16 KiB tiles for r <= 4,
# 8 KiB beyond), two row blocks (12 = 8 + 4).
WIDE = [(127, 2), (129, 3), (130, 4), (250, 5), (200, 8), (247, 8), (251, 4), (254, 1), (243, 12)]
IDS = ["k%dm%d" % s for s in WIDE]
N_OBJ, S = 3, 36917
SHORT = S - 5000
PITCH = (S + 255) // 256 * 256 + 256
FILL = 0xEE
SCRIBBLE = 0x11  # what a lost shard holds before it is rebuilt
OK = (1 << 64) - 1
REC = np.dtype([("first_bad", "<u8"), ("n_bad", "<u8"), ("shard_min", "<u4"), ("shard_max", "<u4")])

# The narrow shapes of the suite reach a few dozen coefficients; between them
# these reach every one, so the v_perm tables run with all 255 here first.
_seen = set()
for _k, _m in WIDE:
    _seen |= set(oracle.matrix(_k, _m)[_k:].reshape(-1).tolist())
assert _seen == set(range(1, 256)), "WIDE no longer reaches every non-zero coefficient: %d of 255" % len(_seen - {0})
assert {k % 4 for k, _ in WIDE} == {0, 1, 2, 3} and any(k + m == 255 for k, m in WIDE)
assert max(N_OBJ * (k + m) * PITCH for k, m in WIDE) < 30e6


def _torch():
    import torch

    return torch


def lens_of(k, m, size=S, short=SHORT):
    return [size] * (k - 1) + [short] + [size] * m


def _image(k, m, size, short, pitch, n_obj, seed):
    """Host image [n_obj][k + m][pitch] of encoded objects (parity and digests
    by oracle.compute_parity), FILL past every row's length; the k + m digests
    per object as reconstruct's expected_sha256 wants them."""
    rng = np.random.default_rng(seed)
    dl = lens_of(k, m, size, short)
    img = np.full((n_obj, k + m, pitch), FILL, np.uint8)
    digests = []
    for o in range(n_obj):
        for j in range(k):
            img[o, j, :dl[j]] = rng.integers(0, 256, dl[j], dtype=np.uint8)
        par, dig, rc = oracle.compute_parity([img[o, j, :dl[j]] for j in range(k)], m, size)
        assert rc == 0
        for i in range(m):
            img[o, k + i, :size] = par[i]
        digests.append(np.frombuffer(b"".join(dig), np.uint8).reshape(k + m, 32))
    img.setflags(write=False)
    return img, np.stack(digests)


@functools.lru_cache(maxsize=None)
def shape(k, m):
    return _image(k, m, S, SHORT, PITCH, N_OBJ, 77000 + 257 * k + m)


def same(got, want, what=""):
    """Whole-buffer equality that says where it first breaks."""
    if np.array_equal(got, want):
        return
    at = np.argwhere(got != want)
    raise AssertionError("%s: %d bytes differ, first at %s: got %#x want %#x" % (
        what, len(at), tuple(at[0]), got[tuple(at[0])], want[tuple(at[0])]))


class Rows:
    """A host array on the device, `off` bytes into an allocation that is FILL
    around it (off = 1: every pointer unaligned, the rs_*_edge kernels)."""

    def __init__(self, host, off=0):
        torch = _torch()
        self.off, self.shape_ = off, host.shape
        self.flat = torch.full((host.size + 16,), FILL, dtype=torch.uint8, device="cuda")
        self.t = self.flat[off:off + host.size].view(*host.shape)
        self.put(host)

    def put(self, host):
        self.t.copy_(_torch().from_numpy(host if host.flags.writeable else host.copy()))
        _torch().cuda.synchronize()

    def get(self):
        _torch().cuda.synchronize()
        edge = self.flat.cpu().numpy()
        assert (edge[:self.off] == FILL).all() and (edge[self.off + self.t.numel():] == FILL).all(), "wrote outside"
        return edge[self.off:self.off + self.t.numel()].reshape(self.shape_)

    @property
    def ptr(self):
        return self.t.data_ptr()


class Stripe:
    """N_OBJ objects of one wide shape on the device, as the oracle encoded
    them (parity=False: the parity rows still FILL)."""

    def __init__(self, k, m, off=0, parity=True):
        self.k, self.m, self.total = k, m, k + m
        self.host, self.digests = shape(k, m)
        self.lens = lens_of(k, m)
        self.dl = self.lens[:k]
        start = self.host
        if not parity:
            start = self.host.copy()
            start[:, k:] = FILL
        self.rows = Rows(start, off)
        self.t = self.rows.t
        self.ostride = self.total * PITCH

    def args(self):
        """k, m, S, n_obj, data, strides, parity, strides: what the strided passes share."""
        return (self.k, self.m, S, N_OBJ, self.rows.ptr, self.ostride, PITCH, self.rows.ptr + self.k * PITCH,
                self.ostride, PITCH)

    def verify(self, ctx):
        torch = _torch()
        fb = torch.full((N_OBJ * self.m,), 0x55, dtype=torch.int64, device="cuda")  # the call fills the entries itself
        torch.cuda.synchronize()
        ctx.verify_strided_device(*self.args(), fb.data_ptr(), data_len=self.dl)
        torch.cuda.synchronize()
        return fb.cpu().numpy().view(np.uint64).reshape(N_OBJ, self.m).tolist()

    def locate(self, ctx):
        torch = _torch()
        out = torch.full((N_OBJ * REC.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.locate_strided_device(*self.args(), out.data_ptr(), data_len=self.dl)
        torch.cuda.synchronize()
        return [tuple(int(v) for v in r) for r in np.frombuffer(out.cpu().numpy().tobytes(), REC)]


# ---- encode -----------------------------------------------------------------------------------

def check_encode(ctx, k, m, off=0):
    s = Stripe(k, m, off, parity=False)
    ctx.encode_strided_device(*s.args(), data_len=s.dl)
    same(s.rows.get(), s.host, "encode (%d, %d)" % (k, m))


@pytest.mark.parametrize("k,m", WIDE, ids=IDS)
def test_encode(ctx, k, m):
    check_encode(ctx, k, m)


# ---- verify -----------------------------------------------------------------------------------

def check_verify(ctx, k, m, off=0):
    """test_verify_gpu.py's conventions: a row's entry is the lowest differing
    offset; a data flip at x shows at x in every row, because no coefficient
    of the parity rows is zero; a parity flip shows in its own row."""
    s = Stripe(k, m, off)
    clean = [[OK] * m for _ in range(N_OBJ)]
    assert s.verify(ctx) == clean
    flips = {0: 4097, k - 1: SHORT - 1, k: 8191, k + m - 1: S - 1}
    flips.update({j: 16384 + j for j in (127, 128) if j < k - 1})  # either side of index 128
    for n, (c, x) in enumerate(sorted(flips.items())):
        o = n % N_OBJ
        s.t[o, c, x] ^= 0x40
        want = [list(r) for r in clean]
        if c < k:
            want[o] = [x] * m
        else:
            want[o][c - k] = x
        assert s.verify(ctx) == want, (k, m, o, c, x)
        s.t[o, c, x] ^= 0x40
    assert s.verify(ctx) == clean
    same(s.rows.get(), s.host, "verify wrote")


@pytest.mark.parametrize("k,m", WIDE, ids=IDS)
def test_verify(ctx, k, m):
    check_verify(ctx, k, m)


# ---- locate -----------------------------------------------------------------------------------

LOCATABLE = [(k, m) for k, m in WIDE if 2 <= m <= 8]


def check_locate(ctx, k, m, off=0):
    """One flipped byte per object per launch names every shard 0 .. k + m - 1
    in turn: the record is (x, 1, c, c) by construction; the first and the
    last launch are also put to locate_ref over the bytes as they stand."""
    s = Stripe(k, m, off)
    clean = [CLEAN_RECORD] * N_OBJ
    assert s.locate(ctx) == clean
    starts = list(range(0, s.total, N_OBJ))
    named = set()
    for c0 in starts:
        want, flips = list(clean), []
        for o, c in enumerate(range(c0, min(c0 + N_OBJ, s.total))):
            x, e = (c * 977 + 13) % s.lens[c], c * 37 % 255 + 1
            s.t[o, c, x] ^= e
            flips.append((o, c, x, e))
            want[o] = (x, 1, c, c)
            named.add(c)
        if c0 in (starts[0], starts[-1]):
            h = s.rows.get()
            assert [locate_ref.locate(h[o], k, m, S, s.dl) for o in range(N_OBJ)] == want
        assert s.locate(ctx) == want, (k, m, c0)
        for o, c, x, e in flips:
            s.t[o, c, x] ^= e
    assert named == set(range(s.total))
    assert s.locate(ctx) == clean
    same(s.rows.get(), s.host, "locate wrote")


@pytest.mark.parametrize("k,m", LOCATABLE, ids=["k%dm%d" % s for s in LOCATABLE])
def test_locate(ctx, k, m):
    assert locate_ref.ratio_table(k, m).count(0xFF) == 256 - k
    check_locate(ctx, k, m)


# ---- the seeded parity pass -------------------------------------------------------------------

def parts_of(k):
    """Windows of 7 in order (the streaming writer's); the last three first;
    one shard, then 128 that end at index 128, then the rest."""
    third = [(0, 1), (1, min(128, k - 1))] + ([(129, k - 129)] if k > 129 else [])
    return {"sevens": [(f, min(7, k - f)) for f in range(0, k, 7)],
            "last3-first": [(k - 3, 3), (0, k - 3)],
            "1-128-rest": third}


PARTS = ("sevens", "last3-first", "1-128-rest")


@functools.lru_cache(maxsize=None)
def parity_after(k, m, name, step):
    """oracle.encode of every object's data with the shards not yet folded
    after `step` zeroed: [N_OBJ][m][S]."""
    host, _ = shape(k, m)
    parts = parts_of(k)[name]
    if step == len(parts) - 1:
        return host[:, k:, :S]
    folded = {j for f, c in parts[:step + 1] for j in range(f, f + c)}
    dl, zero = lens_of(k, m), np.zeros(S, np.uint8)
    return np.stack([np.stack(oracle.encode([host[o, j, :dl[j]] if j in folded else zero for j in range(k)], m, S))
                     for o in range(N_OBJ)])


def check_seeded(ctx, k, m, off=0, name="sevens"):
    """run_partition of test_encode_update_gpu.py: the windows folded in
    order, ping-ponging between two parity sets; the rows after the first, a
    middle and the last step equal the oracle's, and the last the full parity."""
    s = Stripe(k, m, off)
    par = [Rows(np.full((N_OBJ, m, PITCH), FILL, np.uint8), off) for _ in range(2)]
    parts = parts_of(k)[name]
    assert sorted(j for f, c in parts for j in range(f, f + c)) == list(range(k))
    src = None
    for step, (first, count) in enumerate(parts):
        dst = 0 if src != 0 else 1
        ctx.encode_update_strided_device(
            k, m, S, N_OBJ, first, count, s.rows.ptr + first * PITCH, s.ostride, PITCH,
            None if src is None else par[src].ptr, m * PITCH, PITCH, par[dst].ptr, m * PITCH, PITCH,
            data_len=s.dl[first:first + count])
        if step in (0, len(parts) // 2, len(parts) - 1):
            got = par[dst].get()
            same(got[:, :, :S], parity_after(k, m, name, step), "%s step %d (%d, %d)" % (name, step, first, count))
            assert (got[:, :, S:] == FILL).all(), "wrote past the shard size"
        src = dst
    same(par[src].get()[:, :, :S], s.host[:, k:, :S], "the final rows")
    same(s.rows.get(), s.host, "the seeded pass wrote its data")


@pytest.mark.parametrize("name", PARTS)
@pytest.mark.parametrize("k,m", WIDE, ids=IDS)
def test_seeded_pass(ctx, k, m, name):
    check_seeded(ctx, k, m, name=name)


# ---- reconstruct ------------------------------------------------------------------------------

def rs_of(m):
    """Shards lost per object of one launch: all m, about half (9 of 12: two
    row blocks in the decode, as 12 is), one."""
    return [m, 9 if m == 12 else max(1, (m + 1) // 2), 1]


def mixed_lost(k, r):
    """r lost shards, data and parity: the short shard first among the data."""
    nd = (r + 1) // 2
    data = list(dict.fromkeys(j % k for j in (k - 1, 0, 128, k // 2, k // 3, 127, 5, 1, 2)))[:nd]
    assert len(data) == nd
    return sorted(data + list(range(k, k + r - nd)))


def patterns(k, m):
    """name -> the lost shard indices of each object."""
    def straddle(r):
        a = 128 - (r + 1) // 2
        return list(range(a, min(a + r, k + m)))

    rs = rs_of(m)
    return {"lowest": [list(range(r)) for r in rs],
            "highest": [list(range(k - r, k)) for r in rs],  # the short shard among them
            "straddle128": [straddle(r) for r in rs],
            "parity": [list(range(k + m - r, k + m)) for r in rs],
            "mixed": [mixed_lost(k, r) for r in rs]}


def rebuild(ctx, s, lost, data_only=False, corrupt=(), digests=False, want_oracle=False):
    """One in-place reconstruct_strided_device over the stripe with object o's
    `lost[o]` shards scribbled over and flagged missing, `corrupt` (o, shard,
    x) bytes flipped in shards flagged present.  The whole buffer afterwards
    equals the original image (data_only: lost parity still scribbled), which
    holds a rebuilt short shard to its length: the bytes past it are FILL."""
    torch = _torch()
    k, m = s.k, s.m
    present = np.ones((N_OBJ, s.total), np.uint8)
    want, want_present = s.host.copy(), np.ones((N_OBJ, s.total), np.uint8)
    for o in range(N_OBJ):
        for i in lost[o]:
            present[o, i] = 0
            s.t[o, i, :s.lens[i]] = SCRIBBLE
            if data_only and i >= k:
                want[o, i, :S] = SCRIBBLE
                want_present[o, i] = 0
    for o, c, x in corrupt:
        assert present[o, c] and digests
        s.t[o, c, x] ^= 0x80
    dig = torch.from_numpy(s.digests).cuda() if digests else None
    given = s.rows.get() if want_oracle else None
    flags = present.reshape(-1).copy()
    rc, status = ctx.reconstruct_strided_device(k, m, S, N_OBJ, s.rows.ptr, s.ostride, PITCH, flags, shard_len=s.lens,
                                                expected_ptr=dig.data_ptr() if digests else None, data_only=data_only)
    assert rc == 0 and not status.any(), (rc, status, ctx._lib.mxec_last_error())
    got = s.rows.get()
    same(got, want, "reconstruct (%d, %d) lost %s" % (k, m, lost))
    assert np.array_equal(flags.reshape(N_OBJ, s.total), want_present)
    if want_oracle:
        for o in range(N_OBJ):
            bufs, _, orc = oracle.reconstruct([given[o, i, :s.lens[i]] if present[o, i] else None for i in range(s.total)],
                                              k, m, S, data_only=data_only)
            assert orc == 0
            for i in lost[o]:
                if i < k or not data_only:
                    assert np.array_equal(got[o, i, :s.lens[i]], bufs[i][:s.lens[i]]), (o, i)
    if data_only:
        s.rows.put(s.host)


def check_reconstruct(ctx, k, m, off=0):
    s = Stripe(k, m, off)
    pats = patterns(k, m)
    for name, lost in pats.items():
        assert all(1 <= len(p) <= m and len(set(p)) == len(p) for p in lost), (name, lost)
        rebuild(ctx, s, lost, want_oracle=name == "mixed")
    rebuild(ctx, s, pats["mixed"], data_only=True)
    # A silently corrupt present shard beside r - 1 lost ones: the digests
    # turn it into an erasure and it is rebuilt with them.
    lost = [list(range(1, r)) for r in rs_of(m)]
    rebuild(ctx, s, lost, digests=True,
            corrupt=[(0, k - 1, SHORT - 1), (1, k + m - 1, 8192), (2, 128 % k, s.lens[128 % k] - 1)])


@pytest.mark.parametrize("k,m", WIDE, ids=IDS)
def test_reconstruct(ctx, k, m):
    check_reconstruct(ctx, k, m)


# ---- once, not per shape ----------------------------------------------------------------------

CHECKS = {"encode": check_encode, "verify": check_verify, "locate": check_locate, "reconstruct": check_reconstruct}
for _name in PARTS:
    CHECKS["seeded-" + _name] = functools.partial(check_seeded, name=_name)


@pytest.mark.parametrize("what", list(CHECKS))
@pytest.mark.parametrize("k,m", [(251, 4), (200, 8)], ids=["k251m4", "k200m8"])
def test_capped_grid(ctx_with, k, m, what):
    """Seven workgroups: each strides over many tiles and across objects."""
    CHECKS[what](ctx_with(MXEC_TEST_RS_GRID=7), k, m)


@pytest.mark.parametrize("what", list(CHECKS))
@pytest.mark.parametrize("k,m", [(251, 4), (250, 5)], ids=["k251m4", "k250m5"])
def test_unaligned_pointers_take_the_edge_kernels(ctx, k, m, what):
    """Every pointer 1 byte into its allocation (the pitch is a multiple of 256)."""
    CHECKS[what](ctx, k, m, off=1)


BATCH = [(251, 4), (4, 2), (129, 3), (10, 4), (254, 1), (200, 8)]
BATCH_SIZES = (S, 8192 + 16)


@functools.lru_cache(maxsize=None)
def batch_object(k, m, size):
    pitch = (size + 255) // 256 * 256 + 256
    img, dig = _image(k, m, size, size - 777, pitch, 1, 88000 + 257 * k + m + size)
    return img[0], dig[0]


@pytest.mark.parametrize("multi", ["1", "0"])
def test_wide_beside_narrow_in_one_batch(ctx_with, multi):
    """Stripes of 255 and of 6 shards in the same mixed call, each at two
    shard sizes, under both launch forms test_mixed_batch_gpu.py selects with
    MXEC_RS_MULTI: encode, verify, locate and reconstruct, one call each."""
    torch = _torch()
    ctx = ctx_with(MXEC_RS_MULTI=multi)  # read at mxec_open
    objs = [(k, m, size) for (k, m) in BATCH for size in BATCH_SIZES]
    host = [batch_object(*ob)[0] for ob in objs]
    rows = []
    for (k, m, size), h in zip(objs, host):
        blank = h.copy()
        blank[k:] = FILL
        rows.append(Rows(blank))
    pitch = [h.shape[1] for h in host]
    lens = [lens_of(k, m, size, size - 777) for (k, m, size) in objs]

    def tables(which):
        """data pointers, parity pointers and data lengths of objects `which`."""
        return ([rows[n].ptr + j * pitch[n] for n in which for j in range(objs[n][0])],
                [rows[n].ptr + (objs[n][0] + i) * pitch[n] for n in which for i in range(objs[n][1])],
                [v for n in which for v in lens[n][:objs[n][0]]])

    dptr, pptr, dlen = tables(range(len(objs)))

    def all_same(what):
        for ob, r, h in zip(objs, rows, host):
            same(r.get(), h, "%s %s" % (what, ob))

    ctx.encode_batch_device(objs, dptr, pptr, data_len=dlen)
    all_same("encode")

    # verify: clean, then one flip per object -- the last data shard's last
    # byte in even objects, the last parity shard in odd ones.
    fb = torch.full((sum(m for _, m, _ in objs),), 0x55, dtype=torch.int64, device="cuda")

    def verify():
        torch.cuda.synchronize()
        ctx.verify_batch_device(objs, dptr, pptr, fb.data_ptr(), data_len=dlen)
        torch.cuda.synchronize()
        flat, out, at = fb.cpu().numpy().view(np.uint64).tolist(), [], 0
        for _, m, _ in objs:
            out.append(flat[at:at + m])
            at += m
        return out

    clean = [[OK] * m for _, m, _ in objs]
    assert verify() == clean
    flips, want = [], [list(r) for r in clean]
    for n, ((k, m, size), r) in enumerate(zip(objs, rows)):
        c, x = (k - 1, size - 778) if n % 2 == 0 else (k + m - 1, size - 1)
        r.t[c, x] ^= 0x08
        flips.append((r, c, x))
        want[n] = [x] * m if c < k else [OK] * (m - 1) + [x]
    assert verify() == want

    # locate takes 2 <= m <= 8: the same flips, without the (254, 1) objects.
    sub = [n for n, (_, m, _) in enumerate(objs) if m >= 2]
    out = torch.full((len(sub) * REC.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sd, sp, sl = tables(sub)
    ctx.locate_batch_device([objs[n] for n in sub], sd, sp, out.data_ptr(), data_len=sl)
    torch.cuda.synchronize()
    got = [tuple(int(v) for v in r) for r in np.frombuffer(out.cpu().numpy().tobytes(), REC)]
    assert got == [(flips[n][2], 1, flips[n][1], flips[n][1]) for n in sub]
    for r, c, x in flips:
        r.t[c, x] ^= 0x08
    assert verify() == clean

    # reconstruct: all m lost per object -- the highest data shards in even
    # objects, data and parity mixed in odd ones.
    present, slen, sptr = [], [], []
    for n, ((k, m, size), r, p) in enumerate(zip(objs, rows, pitch)):
        lost = list(range(k - m, k)) if n % 2 == 0 else mixed_lost(k, m)
        flags = np.ones(k + m, np.uint8)
        for i in lost:
            flags[i] = 0
            r.t[i, :lens[n][i]] = SCRIBBLE
        present.append(flags)
        slen += lens[n]
        sptr += [r.ptr + i * p for i in range(k + m)]
    flags = np.concatenate(present)
    torch.cuda.synchronize()
    rc, status = ctx.reconstruct_batch_device(objs, sptr, flags, shard_len=slen)
    assert rc == 0 and not status.any() and flags.all(), (rc, status)
    all_same("reconstruct")


def test_small_coefficient_arena_recycles_under_wide_tables(ctx_with):
    """A (251, 4) decode table of four rows is 4 * 251 * 32 B = 31.4 KiB: in
    48 KiB halves a second one never fits beside the first, so every batch
    with two distinct four-shard patterns closes a generation, and the next
    batch waits out the fences of the half it takes over
    (test_coef_arena_gpu.py has the narrow form of this)."""
    k, m = 251, 4
    ctx = ctx_with(MXEC_TEST_COEF_ARENA_KB=48)
    s = Stripe(k, m)
    before = ctx.coef_stats()["recycles"]
    rng = np.random.default_rng(4848)
    for rnd in range(5):
        lost = [sorted(rng.choice(k + m, r, replace=False).tolist()) for r in (4, 4, 1)]
        rebuild(ctx, s, lost, want_oracle=rnd == 0)
    assert ctx.coef_stats()["recycles"] - before >= 5


# ---- k + m = 256: the reconstructs take what the crate takes ----------------------------------

@functools.lru_cache(maxsize=None)
def shards_256(k, m, size):
    rng = np.random.default_rng(256000 + k)
    data = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(k)]
    return data + oracle.encode(data, m, size)


@pytest.mark.parametrize("lost", ["255-lost", "255-present"])
@pytest.mark.parametrize("k,m", [(252, 4), (255, 1)], ids=["k252m4", "k255m1"])
def test_reconstruct_takes_256_shards(ctx, k, m, lost):
    """ReedSolomon::new accepts 256 total shards and the reconstructs check
    only that (reconstruct_shape -> rs_check), while every encode refuses more
    than 255 as the reference does: a 256-shard stripe made elsewhere can be
    rebuilt here, shard index 255 among the lost or among the inputs."""
    torch = _torch()
    size = 8192 + 16
    shards = shards_256(k, m, size)
    gone = ([255] + [0, 128, k - 1][:m - 1]) if lost == "255-lost" else [0, 127, 128, k - 1][:m]
    assert len(set(gone)) == len(gone) <= m
    given = [None if i in gone else shards[i] for i in range(256)]
    bufs, _, orc = oracle.reconstruct(given, k, m, size)
    assert orc == 0 and all(np.array_equal(bufs[i], shards[i]) for i in range(256))

    out, present = ctx.reconstruct(given, k, m, size)
    assert present.all()
    for i in range(256):
        assert np.array_equal(out[i], bufs[i]), i

    host = np.stack(shards)
    dev = host.copy()
    dev[gone] = SCRIBBLE
    t = torch.from_numpy(dev).cuda()
    flags = np.ones(256, np.uint8)
    flags[gone] = 0
    torch.cuda.synchronize()
    rc, status = ctx.reconstruct_strided_device(k, m, size, 1, t.data_ptr(), 256 * size, size, flags)
    torch.cuda.synchronize()
    assert rc == 0 and not status.any() and flags.all(), (rc, ctx._lib.mxec_last_error())
    same(t.cpu().numpy(), host, "256 shards, lost %s" % gone)


def test_every_encode_refuses_256_shards(ctx):
    """The other half of the contract: 256 shards never come from here, and
    257 are the crate's TooManyShards to the reconstructs.  All decided
    before anything is enqueued: the device forms are given pointers no
    kernel could read."""
    import maxio_amd

    rc, _ = ctx.reconstruct_strided_device(253, 4, 64, 1, 16, 257 * 256, 256, np.ones(257, np.uint8))
    assert rc == -2

    d = np.zeros(64, np.uint8)
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.encode([d] * 252, 4, 64)
    assert e.value.name == "TooManyShards255"
    with pytest.raises(maxio_amd.RSError) as e:
        ctx.encode_strided_device(255, 1, 64, 1, 16, 256 * 256, 256, 16, 256 * 256, 256)
    assert e.value.name == "TooManyShards255"
