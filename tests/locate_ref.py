"""Restatement of mxec_locate's algebra for the tests: numpy over the
oracle's matrix, field arithmetic and encode.  Nothing here comes from the
library under test.

For every byte column b of one object the syndrome is
s_i = stored_parity_i[b] ^ recomputed_parity_i[b].  A column whose s is not
all zero is bad and names a candidate:

  * exactly one s_i non-zero            -> parity shard k + i;
  * all m non-zero and s = M[:, j] * e  -> data shard j (e = s_0 / M[0][j]),
    if b lies below shard j's length;
  * anything else                       -> NO_SHARD.

The object's record is (lowest bad column or OK, number of bad columns,
min candidate, max candidate); clean: (OK, 0, 0xFFFFFFFF, 0)."""
from __future__ import annotations

import functools

import numpy as np

import oracle

OK = (1 << 64) - 1
NO_SHARD = 0xFFFFFFFE
CLEAN_RECORD = (OK, 0, 0xFFFFFFFF, 0)
CLEAN, ONE, MANY = 0, 1, 2


@functools.lru_cache(maxsize=None)
def _mul_table() -> np.ndarray:
    t = np.zeros((256, 256), np.uint8)
    for a in range(1, 256):
        for b in range(a, 256):
            t[a, b] = t[b, a] = oracle.gf_mul(a, b)
    return t


@functools.lru_cache(maxsize=None)
def parity_rows(k: int, m: int) -> np.ndarray:
    return oracle.matrix(k, m)[k:].copy()


def ratio_table(k: int, m: int) -> list[int]:
    """ratio -> j with ratio = M[1][j] / M[0][j]; 0xFF where no column has
    it.  Asserts what MDS promises: no zero entry, no two equal ratios."""
    M = parity_rows(k, m)
    tab = [0xFF] * 256
    for j in range(k):
        assert all(int(M[i, j]) != 0 for i in range(m)), (k, m, j)
        r = oracle.gf_div(int(M[1, j]), int(M[0, j]))
        assert tab[r] == 0xFF, f"columns {tab[r]} and {j} of ({k}, {m}) are proportional"
        tab[r] = j
    return tab


def locate(rows: np.ndarray, k: int, m: int, size: int, dl) -> tuple[int, int, int, int]:
    """rows[k + m][>= size]: the object's shards as they stand; dl: the k
    data lengths (bytes past them count as zero and are not looked at)."""
    want = oracle.encode([rows[j, :dl[j]] for j in range(k)], m, size)
    syn = np.stack([np.asarray(want[i], np.uint8)[:size] ^ rows[k + i, :size] for i in range(m)])
    cols = np.flatnonzero(syn.any(axis=0))
    if cols.size == 0:
        return CLEAN_RECORD
    s = syn[:, cols]                      # m x n_bad
    nz = (s != 0).sum(axis=0)
    cand = np.full(cols.size, NO_SHARD, np.int64)
    one = nz == 1
    cand[one] = k + (s[:, one] != 0).argmax(axis=0)
    full = nz == m
    if full.any():
        MUL, M = _mul_table(), parity_rows(k, m)
        sf, cf = s[:, full], cols[full]
        got = np.full(cf.size, NO_SHARD, np.int64)
        for j in range(k):
            # e = s_0 / M[0][j]: the one e with M[0][j] * e == s_0
            inv = int(np.flatnonzero(MUL[int(M[0, j])] == 1)[0])
            e = MUL[inv][sf[0]]
            fits = cf < dl[j]
            for i in range(m):
                fits &= MUL[int(M[i, j])][e] == sf[i]
            assert not (fits & (got != NO_SHARD)).any(), "two data shards fit one column"
            got[fits] = j
        cand[full] = got
    return int(cols[0]), int(cols.size), int(cand.min()), int(cand.max())


def outcome(rec) -> tuple[int, int | None]:
    _, n_bad, lo, hi = rec
    if n_bad == 0:
        return CLEAN, None
    if lo == hi and lo < 256:
        return ONE, lo
    return MANY, None
