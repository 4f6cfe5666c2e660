"""GPU: the shape of the host pipeline's enqueue, pinned by its counters.

Each host-batch call -- a PUT with digests, a PUT without, an RS-only GET
with two shards missing, a verified GET with one shard missing and one
silently corrupt -- issues a fixed set of copies, wave-copy blocks,
verification groups and speculative pieces once the copy engine, the piece
size and speculation are fixed by knobs (nothing is left to the SDMA watch
or to timing).  The deltas of mxec_ctx_pipe_stats around each call, taken
alone, are compared with the values the library produced before the host
pipeline was split into pipe_hub / copy_watch / host_copy / pipeline_put /
pipeline_get: a refactor of that code must queue the same work.  Outputs are
bit-exact against the oracle.

Left out on purpose (they depend on timing): sdma_checks, sdma_slow,
sdma_down_checks, sdma_down_slow, the *_last_mbps rates, pace_waits."""
from __future__ import annotations

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

K, M, N = 4, 2, 6
S = (5 << 19) + 17            # 2.5 MiB + 17: a tail piece, an unaligned length, more than one 1 MiB piece
LAST = S - 3333               # short last data chunk
SLOT = (S + 255) // 256 * 256
COUNTERS = ("copies_1d", "copies_2d", "rows_2d", "wave_blocks", "verify_waves", "verify_groups", "calls",
            "calls_shared", "spec_pieces", "spec_redos")
CALLS = ("put_digests", "put_plain", "get_rs_only", "get_verified")

# Deltas of COUNTERS per call of CALLS, by (MXEC_PIPE_COPY, MXEC_PIPE_PIECE_MB,
# MXEC_GET_SPECULATE, memory).  Produced by commit 57b5466 ("Add
# ReedSolomon::verify on the GPU and mxec_scrub_object"), the last one with
# the pipeline in one file; two fresh processes there gave identical values
# for all 16 configurations.
_PLAIN = (36, 0, 0, 0, 0, 0, 1, 0, 0, 0)       # group form, one DMA per shard (no digests: never in pieces)
_WPLAIN = (0, 0, 0, 390, 0, 0, 1, 0, 0, 0)     # the same by wave copies
_WPUT = (1, 0, 0, 390, 0, 0, 1, 0, 0, 0)       # + the digests' download (pageable destination)


def _sdma(put, get):
    return (put + (0, 0, 1, 0, 0, 0), _PLAIN, _PLAIN, get)


EXPECTED = {
    ("sdma", "1", "1", "host_alloc"): _sdma((109, 0, 0, 0), (121, 0, 0, 0, 1, 1, 1, 0, 3, 6)),
    ("sdma", "1", "1", "pageable"): _sdma((109, 0, 0, 0), (121, 0, 0, 0, 1, 1, 1, 0, 3, 6)),
    ("sdma", "1", "0", "host_alloc"): _sdma((109, 0, 0, 0), (103, 0, 0, 0, 1, 1, 1, 0, 0, 0)),
    ("sdma", "1", "0", "pageable"): _sdma((109, 0, 0, 0), (103, 0, 0, 0, 1, 1, 1, 0, 0, 0)),
    ("sdma", "4", "1", "host_alloc"): _sdma((7, 12, 30, 0), (21, 9, 28, 0, 1, 1, 1, 0, 1, 6)),
    ("sdma", "4", "1", "pageable"): _sdma((37, 0, 0, 0), (49, 0, 0, 0, 1, 1, 1, 0, 1, 6)),
    ("sdma", "4", "0", "host_alloc"): _sdma((7, 12, 30, 0), (19, 7, 24, 0, 1, 1, 1, 0, 0, 0)),
    ("sdma", "4", "0", "pageable"): _sdma((37, 0, 0, 0), (43, 0, 0, 0, 1, 1, 1, 0, 0, 0)),
    ("waves", "1", "1", "host_alloc"): (_WPUT, _WPLAIN, _WPLAIN, (1, 0, 0, 520, 1, 1, 1, 0, 3, 6)),
    ("waves", "1", "1", "pageable"): _sdma((109, 0, 0, 0), (121, 0, 0, 0, 1, 1, 1, 0, 3, 6)),
    ("waves", "1", "0", "host_alloc"): (_WPUT, _WPLAIN, _WPLAIN, (1, 0, 0, 455, 1, 1, 1, 0, 0, 0)),
    ("waves", "1", "0", "pageable"): _sdma((109, 0, 0, 0), (103, 0, 0, 0, 1, 1, 1, 0, 0, 0)),
    ("waves", "4", "1", "host_alloc"): (_WPUT, _WPLAIN, _WPLAIN, (1, 0, 0, 520, 1, 1, 1, 0, 1, 6)),
    ("waves", "4", "1", "pageable"): _sdma((37, 0, 0, 0), (49, 0, 0, 0, 1, 1, 1, 0, 1, 6)),
    ("waves", "4", "0", "host_alloc"): (_WPUT, _WPLAIN, _WPLAIN, (1, 0, 0, 455, 1, 1, 1, 0, 0, 0)),
    ("waves", "4", "0", "pageable"): _sdma((37, 0, 0, 0), (43, 0, 0, 0, 1, 1, 1, 0, 0, 0)),
}

_reference = {}


def _batch():
    """The seeded batch, computed once: data chunks, oracle parity and digests."""
    if not _reference:
        rng = np.random.default_rng(0x5EED)
        objs = []
        for _ in range(N):
            chunks = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(K)]
            chunks[-1] = chunks[-1][:LAST].copy()
            par, dig, rc = oracle.compute_parity(chunks, M, S)
            assert rc == 0
            objs.append((chunks + [np.asarray(p, np.uint8) for p in par], dig))
        _reference["objs"] = objs
    return _reference["objs"]


def _buffers(ctx, mem):
    """N x (K + M) shard buffers of SLOT bytes: one mxec_host_alloc block
    (shards at a 256-byte pitch, so wave copies apply) or pageable arrays."""
    if mem == "host_alloc":
        block = ctx.host_array(N * (K + M) * SLOT)
        return block, [[block[(o * (K + M) + i) * SLOT:][:SLOT] for i in range(K + M)] for o in range(N)]
    return None, [[np.empty(SLOT, np.uint8) for _ in range(K + M)] for _ in range(N)]


def _delta(ctx, call):
    s0 = ctx.pipe_stats()
    call()
    s1 = ctx.pipe_stats()
    return tuple(int(s1[c] - s0[c]) for c in COUNTERS)


def measure(ctx, mem):
    """Runs the four calls on ctx from `mem` buffers, checks every output
    against the oracle and returns {call: deltas of COUNTERS}."""
    ref = _batch()
    lens = [S] * (K - 1) + [LAST] + [S] * M
    block, buf = _buffers(ctx, mem)
    objs = [(K, M, S)] * N
    dptr = [buf[o][j].ctypes.data for o in range(N) for j in range(K)]
    pptr = [buf[o][K + i].ctypes.data for o in range(N) for i in range(M)]
    sptr = [buf[o][i].ctypes.data for o in range(N) for i in range(K + M)]
    want_dig = np.frombuffer(b"".join(d for _, ds in ref for d in ds), np.uint8)

    def fill():
        for o in range(N):
            for j in range(K):
                buf[o][j][:lens[j]] = ref[o][0][j]
            for i in range(M):
                buf[o][K + i][:] = 0xEE

    def check():
        for o in range(N):
            for i in range(K + M):
                assert np.array_equal(buf[o][i][:lens[i]], ref[o][0][i]), (o, i)

    out = {}
    try:
        fill()
        dig = np.zeros(N * (K + M) * 32, np.uint8)
        st = []
        out["put_digests"] = _delta(ctx, lambda: st.append(
            ctx.encode_batch_host(objs, dptr, pptr, data_len=lens[:K] * N, digests=dig)))
        assert (st[0] == 0).all() and np.array_equal(dig, want_dig)
        check()

        fill()
        out["put_plain"] = _delta(ctx, lambda: st.append(
            ctx.encode_batch_host(objs, dptr, pptr, data_len=lens[:K] * N)))
        assert (st[1] == 0).all()
        check()

        present = np.ones((N, K + M), np.uint8)
        for o in range(N):
            for i in (o % (K + M), (o + 3) % (K + M)):
                present[o, i] = 0
                buf[o][i][:] = 0x5A
        pr = present.reshape(-1).copy()
        res = []
        out["get_rs_only"] = _delta(ctx, lambda: res.append(
            ctx.reconstruct_batch_host(objs, sptr, pr, shard_len=lens * N)))
        assert res[0][0] == 0 and not res[0][1].any() and pr.all()
        check()

        present = np.ones((N, K + M), np.uint8)
        for o in range(N):
            lost, bad = (o + 1) % (K + M), (o + 4) % (K + M)
            present[o, lost] = 0
            buf[o][lost][:] = 0x5A
            buf[o][bad][lens[bad] // 2] ^= 0x40  # silent corruption: caught by its digest, rebuilt
        pr = present.reshape(-1).copy()
        out["get_verified"] = _delta(ctx, lambda: res.append(
            ctx.reconstruct_batch_host(objs, sptr, pr, shard_len=lens * N, expected=want_dig.copy())))
        assert res[1][0] == 0 and not res[1][1].any() and pr.all()
        check()
    finally:
        if block is not None:
            ctx.host_free(block)
    return out


CONFIGS = [(copy, piece, spec) for copy in ("sdma", "waves") for piece in ("1", "4") for spec in ("1", "0")]


def config_ctx(ctx_with, copy, piece, spec):
    return ctx_with(device_mask=1, MXEC_PIPE_COPY=copy, MXEC_PIPE_PIECE_MB=piece, MXEC_GET_SPECULATE=spec)


@pytest.mark.parametrize("mem", ["host_alloc", "pageable"])
@pytest.mark.parametrize("copy,piece,spec", CONFIGS)
def test_pipeline_counters(ctx_with, copy, piece, spec, mem):
    got = measure(config_ctx(ctx_with, copy, piece, spec), mem)
    want = EXPECTED[(copy, piece, spec, mem)]
    for call, w in zip(CALLS, want):
        print(copy, piece, spec, mem, call, dict(zip(COUNTERS, got[call])))
    for call, w in zip(CALLS, want):
        assert got[call] == w, (call, dict(zip(COUNTERS, got[call])), dict(zip(COUNTERS, w)))
